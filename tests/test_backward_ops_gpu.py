"""Op-level adjoint tests of the training path's backward kernels (csrc/backward_ops.hip, csrc/dcn_backward.hip).

Every test builds the forward operation in float64 torch on the CPU from the same fp16-rounded operands the kernels see,
takes the true adjoint with torch.autograd.grad and compares the HIP result element by element.  Accumulating entry points
start from a non-zero buffer and are checked against base + gradient.

Bounds are derived from the arithmetic, not fitted:
  * an fp16 store rounds to nearest: |fp16(v) - v| <= EPS16 |v| (EPS16 = 2^-11, half an ulp), plus 2^-25 below the normal range;
  * an fp32 sum of n terms errs by at most ~n EPS32 sum|t| (EPS32 = 2^-24); where n is small the bound below is that, written
    as a multiple of sum|t| computed in float64.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers_dcn import far_stats as _far_stats, offsets as _offsets
from util import assert_close, fm_to_cpu, randn, rnd16, to_fm

pytestmark = pytest.mark.gpu

EPS16 = 2.0 ** -11
EPS32 = 2.0 ** -24
TINY16 = 2.0 ** -24           # fp16 subnormal spacing: the absolute floor of any fp16 store
R16 = EPS16 + 8 * EPS32       # one fp16 store of a value computed in fp32 (a few fp32 roundings before it)


def _ops():
    from tdvc_amd import ops
    return ops


def _grad(out_dot, leaves):
    return torch.autograd.grad(out_dot, leaves, allow_unused=False)


def _leaf(t):
    return t.double().clone().requires_grad_()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------------------ SE
# (C, N, H, W): fewer than 256 pixels (one block), a count that is not a multiple of 256, and >= 65 536 pixels where
# gate_backward's partial sums clamp at 256 blocks (tdvc_gate_backward) and se_gate's channel sum runs 257+ blocks
SE_CASES = [(64, 2, 9, 13), (128, 2, 9, 13), (64, 2, 37, 29), (128, 2, 37, 29), (64, 1, 257, 259), (128, 1, 256, 257)]


@pytest.mark.parametrize("C,N,H,W", SE_CASES, ids=[f"C{c}_{n}x{h}x{w}" for c, n, h, w in SE_CASES])
def test_se_backward(C, N, H, W, report):
    """y = x * gate(x) (scale_act_res(gate=...)); gate = sigmoid(W2 relu(W1 mean(x) + b1) + b2) (oracle SELayer):
    gate_backward -> se_gate_backward -> bcast_channel_add against float64 autograd"""
    ops = _ops()
    from tdvc_amd import _lib as L
    Cmid = C // 16
    npix = H * W
    x = rnd16(randn(N, C, H, W, seed=1) + 0.6 * randn(1, C, 1, 1, seed=2))        # per-channel means of O(1): the gate is live
    w1, b1 = randn(Cmid, C, seed=3) * C ** -0.5 * 2.0, randn(Cmid, seed=4) * 0.3
    w2, b2 = randn(C, Cmid, seed=5) * Cmid ** -0.5, randn(C, seed=6) * 0.3
    g = rnd16(randn(N, C, H, W, seed=7))
    dgate0 = randn(N, C, seed=8) * 0.5            # gradient already on the gate (the tape's mirror is accumulated into)
    base = rnd16(randn(N, C, H, W, seed=9) * 0.25)
    pbase = [randn(*s, seed=10 + i) * 0.1 for i, s in enumerate([(Cmid, C), (Cmid,), (C, Cmid), (C,)])]
    scale = 1.0 / 128

    # device forward state: the channel sums se_gate keeps, the gate, y
    xf = to_fm(x, ops)
    p = ops.SEParams(w1.cuda().contiguous(), b1.cuda(), w2.cuda().contiguous(), b2.cuda(), C, Cmid)
    nblocks = max(1, min(1024, npix // 256))
    partial = torch.empty((N, nblocks, C), dtype=torch.float32, device="cuda")
    L.check(L.lib().tdvc_channel_sum(ops.C.byref(xf.desc()), partial.data_ptr(), nblocks, ops._stream()), "channel_sum")
    gate = ops.se_gate(xf, p, partial=(partial, nblocks))
    y = ops.scale_act_res(xf, ops.FM.empty(N, H, W, C), gate=gate)

    # float64 reference
    xr, W1, B1, W2, B2 = (_leaf(t) for t in (x, w1, b1, w2, b2))
    gr = torch.sigmoid(torch.relu(xr.mean((2, 3)) @ W1.t() + B1) @ W2.t() + B2)
    yr = xr * gr[:, :, None, None]
    loss = (yr * g.double()).sum() + (gr * dgate0.double()).sum()
    dx_r, dw1_r, db1_r, dw2_r, db2_r = _grad(loss, (xr, W1, B1, W2, B2))
    assert_close(gate.cpu(), gr.detach(), 1e-5, 1e-6, f"SE gate C{C}", report)
    assert_close(fm_to_cpu(y), yr.detach(), EPS16, TINY16 + 1e-6, f"SE y C{C}", report)

    # device backward
    gf = to_fm(g, ops)
    dx = to_fm(base, ops)
    dgate = dgate0.cuda().clone()
    ops.gate_backward(gf, xf, gate, dx, dgate)
    # dgate = dgate0 + sum_pix g * x: an fp32 sum of npix products in blocks; 16 EPS32 sum|g x| is ~sqrt(depth) EPS32 with margin
    gx = (g.double() * x.double())
    dgate_ref = dgate0.double() + gx.sum((2, 3))
    assert_close(dgate.cpu(), dgate_ref, 0, 16 * EPS32 * gx.abs().sum((2, 3)) + EPS32 * dgate_ref.abs(), f"gate_backward dgate C{C} {H}x{W}", report)
    grads = [t.cuda().clone() for t in pbase]
    dmean = ops.se_gate_backward(p, partial, nblocks, npix, gate, dgate, scale, grads)
    ops.bcast_channel_add(dx, dmean, 1.0 / npix)
    # parameter gradients: fp32 chains of <= C-term dot products behind dgate (relative error <= 1e-6 of its terms): 1e-5 of the
    # tensor's largest value covers them
    # (and one fp32 rounding of base + scale * gradient)
    for name, got, b0, ref in zip(("dW1", "db1", "dW2", "db2"), grads, pbase, (dw1_r, db1_r, dw2_r, db2_r)):
        want = b0.double() + scale * ref
        assert_close(got.cpu(), want, 2 * EPS32, 1e-5 * scale * float(ref.abs().max()) + 1e-12, f"se_gate_backward {name} C{C} {H}x{W}", report)
    # dx: two fp16 stores (base + g * gate, then + dmean / npix): two half-ulps of the larger of the two values
    dx_ref = base.double() + dx_r
    mid = (base.double() + g.double() * gr.detach()[:, :, None, None]).abs()
    assert_close(fm_to_cpu(dx), dx_ref, EPS16, EPS16 * mid + 1e-6 * float(dx_ref.abs().max()) + TINY16, f"SE dx C{C} {H}x{W}", report)


# ------------------------------------------------------------------------------------------------------------------ GDN
@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
def test_gdn_backward(inverse, report):
    """y = x (beta + gamma . x^2)^(-+1/2): gdn_backward -> conv_dgrad -> mul2_accumulate, conv_wgrad(square_x=True, db=...)"""
    ops = _ops()
    N, C, H, W = 2, 128, 13, 21
    x = rnd16(randn(N, C, H, W, seed=21) * 0.8)
    g_ = torch.Generator().manual_seed(22)
    gamma = (0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g_)).contiguous()       # effective (non-negative) gamma
    beta = 0.5 + torch.rand(C, generator=g_)
    g = rnd16(randn(N, C, H, W, seed=23))
    base = rnd16(randn(N, C, H, W, seed=24) * 0.25)
    scale = 1.0 / 128

    pc = ops.pack_conv(gamma.reshape(C, C, 1, 1).cuda(), beta.cuda(), stride=1, pad=0)
    xf = to_fm(x, ops)
    y = ops.conv(xf, pc, square=True, gdn=ops.GDN_INV if inverse else ops.GDN_FWD, aux=xf)

    xr, G, B = _leaf(x), gamma.double().requires_grad_(), beta.double().requires_grad_()
    nr = F.conv2d(xr * xr, G.reshape(C, C, 1, 1), B)
    yr = xr * (nr.sqrt() if inverse else nr.rsqrt())
    dx_r, dg_r, db_r = _grad((yr * g.double()).sum(), (xr, G, B))
    assert_close(fm_to_cpu(y), yr.detach(), 2 * EPS16, 1e-4, f"{'I' if inverse else ''}GDN forward", report)

    # the sweep of autograd.record_gdn
    n32 = ops.conv(xf, pc, square=True, out_dtype=torch.float32)
    dx = to_fm(base, ops)
    dn = ops.gdn_backward(to_fm(g, ops), xf, n32, inverse, dx)
    t = ops.conv_dgrad(pc, dn, ops.FM.empty(N, H, W, C), accumulate=False)
    ops.mul2_accumulate(dx, xf, t)
    dgamma = torch.full((C * C,), 0.25, device="cuda")
    dbeta = torch.full((C,), -0.5, device="cuda")
    ops.conv_wgrad(pc, dn, xf, dgamma, scale=scale, square_x=True, db=dbeta)

    # The kernels see gamma and x^2 in fp16 (the packed weights, the squared input): n (fp32) is off by <= 2 EPS16 relative (all
    # terms are positive), r = n^(-+1/2) by EPS16, dn = dL/dn (stored in fp16) by 3 + 1 EPS16, t = gamma^T dn by 4 + 1 + 1 EPS16 of
    # sum gamma |dn|.  Float64 dn and the magnitudes those relative errors apply to:
    with torch.no_grad():
        n64 = nr.detach()
        dn_r = (0.5 * g.double() * x.double() / n64.sqrt()) if inverse else (-0.5 * g.double() * x.double() * n64.rsqrt() / n64)
        t_abs = F.conv2d(dn_r.abs(), G.detach().t().reshape(C, C, 1, 1))          # sum_o gamma[o][c] |dn[o]|  >= |t|
        x2 = x.double() ** 2
        # dgamma[o][c] = sum_pix dn[o] x[c]^2: dn is stored in fp16 (EPS16 relative per term), the sum is fp32
        dg_abs = torch.einsum("nohw,nchw->oc", dn_r.abs(), x2)
        db_abs = dn_r.abs().sum((0, 2, 3))
    # dgamma = sum dn x^2 (4 + 1 EPS16 per term), dbeta = sum dn (4 EPS16 per term), fp32 sums
    assert_close(dgamma.cpu().view(C, C) - 0.25, scale * dg_r, 0, scale * (6 * EPS16 * dg_abs) + 1e-7, "GDN dgamma", report)
    assert_close(dbeta.cpu() + 0.5, scale * db_r, 0, scale * (5 * EPS16 * db_abs) + 1e-7, "GDN dbeta", report)
    # dx = fp16(fp16(base + g r) + 2 x t): a half-ulp per store, r's error through |g|, t's through 2|x|
    with torch.no_grad():
        r = n64.sqrt() if inverse else n64.rsqrt()
        first = (base.double() + g.double() * r).abs()
        bound = EPS16 * first + EPS16 * g.double().abs() * r + 2 * x.double().abs() * 6 * EPS16 * t_abs
    dx_ref = base.double() + dx_r
    assert_close(fm_to_cpu(dx), dx_ref, R16, bound + TINY16, f"{'I' if inverse else ''}GDN dx", report)


# ------------------------------------------------------------------------------------------------------------------ resampling, broadcasts
UPS_CASES = [(2, 16, 7, 9), (1, 8, 1, 6), (2, 8, 5, 1), (1, 64, 17, 30)]


@pytest.mark.parametrize("N,C,H,W", UPS_CASES, ids=[f"{n}x{c}x{h}x{w}" for n, c, h, w in UPS_CASES])
def test_upsample2x_backward(N, C, H, W, report):
    """dx += U^T dy, U = F.interpolate(scale_factor=2, bilinear, align_corners=False); odd and 1-pixel-wide maps"""
    ops = _ops()
    dy = rnd16(randn(N, C, 2 * H, 2 * W, seed=31))
    base = rnd16(randn(N, C, H, W, seed=32) * 0.5)
    xr = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    (ref,) = _grad((up * dy.double()).sum(), (xr,))
    (ref_abs,) = _grad((up * dy.double().abs()).sum(), (xr,))        # bilinear weights are >= 0: the sum of |terms|
    dx = to_fm(base, ops)
    ops.upsample2x_backward(to_fm(dy, ops), dx)
    # <= 16 fp32 products summed (32 EPS32 sum|t|), one fp16 store
    assert_close(fm_to_cpu(dx), base.double() + ref, EPS16, 32 * EPS32 * ref_abs + TINY16, f"upsample2x_backward {N}x{C}x{H}x{W}", report)


@pytest.mark.parametrize("C", [144, 16])
def test_add_flow_backward(C, report):
    """off[c] += flow[c & 1] (ops.add_flow: DCN offsets + flow): dflow += sums over the even / odd offset channels"""
    ops = _ops()
    N, H, W = 2, 11, 19
    off = rnd16(randn(N, C, H, W, seed=41))
    flow = randn(N, 2, H, W, seed=42) * 3
    offf, flowf = to_fm(off, ops), to_fm(flow, ops, Cpad=2, dtype=torch.float32)
    ops.add_flow(offf, flowf)
    fr = _leaf(flow)
    yr = off.double() + fr.repeat(1, C // 2, 1, 1)
    assert_close(fm_to_cpu(offf), yr.detach(), EPS16, TINY16, f"add_flow C{C}", report)
    doff = rnd16(randn(N, C, H, W, seed=43))
    (ref,) = _grad((yr * doff.double()).sum(), (fr,))
    ref_abs = doff.double().abs().view(N, C // 2, 2, H, W).sum(1)
    fbase = randn(N, 2, H, W, seed=44)
    dflow = to_fm(fbase, ops, Cpad=2, dtype=torch.float32)
    ops.add_flow_backward(to_fm(doff, ops), dflow)
    # fp32 sums of C/2 fp16 values into an fp32 accumulator
    assert_close(fm_to_cpu(dflow), fbase.double() + ref, EPS32, (C // 2 + 1) * EPS32 * ref_abs + 1e-30, f"add_flow_backward C{C}", report)


def test_bcast_add_act_backward(report):
    """x = lrelu(x + b[c % 64], 0.1) over T = 4 slices of 64 channels, in place: dx <- dx lrelu'(z), db (a per-pixel map) += sum over slices"""
    ops = _ops()
    N, T, Cb, H, W, slope = 2, 4, 64, 13, 11, 0.1
    xpre = rnd16(randn(N, T * Cb, H, W, seed=51))
    b = rnd16(randn(N, Cb, H, W, seed=52))
    xf, bf = to_fm(xpre, ops), to_fm(b, ops)
    ops.bcast_add_act(xf, bf, T, slope)
    xr, br = _leaf(xpre), _leaf(b)
    z = xr + br.repeat(1, T, 1, 1)
    yr = F.leaky_relu(z, slope)
    assert_close(fm_to_cpu(xf), yr.detach(), EPS16, TINY16, "bcast_add_act", report)
    g = rnd16(randn(N, T * Cb, H, W, seed=53))
    dx_r, db_r = _grad((yr * g.double()).sum(), (xr, br))
    dbase = rnd16(randn(N, Cb, H, W, seed=54) * 0.5)
    gf, db = to_fm(g, ops), to_fm(dbase, ops)
    ops.bcast_add_act_backward(gf, xf, db, slope)
    assert_close(fm_to_cpu(gf), dx_r, R16, TINY16, "bcast_add_act_backward dx", report)
    # db: base + 4 fp32 terms (each g or fp32 g * slope), one fp16 store
    db_abs = dbase.double().abs() + dx_r.abs().view(N, T, Cb, H, W).sum(1)
    assert_close(fm_to_cpu(db), dbase.double() + db_r, EPS16, 8 * EPS32 * db_abs + TINY16, "bcast_add_act_backward db", report)


def test_clamp01_backward(report):
    """g * [0 < y < 1] against autograd of clamp(z, 0, 1), with z exactly 0 and 1 included.  torch passes the gradient on the closed
    interval; the kernel sees y only, and at y in {0, 1} it cannot tell z = 0 from z < 0: the only elements allowed to differ are
    those with z exactly on a bound"""
    ops = _ops()
    N, C, H, W = 2, 8, 9, 14
    z = rnd16(randn(N, C, H, W, seed=61) * 0.8 + 0.5)
    flat = z.view(-1)
    gen = torch.Generator().manual_seed(62)
    pick = torch.randperm(flat.numel(), generator=gen)
    flat[pick[:40]] = 0.0
    flat[pick[40:80]] = 1.0
    flat[pick[80:100]] = 1.0 - 2.0 ** -11          # largest fp16 below 1
    flat[pick[100:120]] = 2.0 ** -24               # smallest positive fp16
    zr = _leaf(z)
    yr = zr.clamp(0.0, 1.0)
    g = rnd16(randn(N, C, H, W, seed=63))
    (ref,) = _grad((yr * g.double()).sum(), (zr,))
    gf = to_fm(g, ops)
    ops.clamp01_backward(gf, to_fm(yr.detach().float(), ops))
    got = fm_to_cpu(gf).double()
    differ = got != ref
    on_bound = (z == 0.0) | (z == 1.0)
    report(f"clamp01_backward: {int(differ.sum())} elements differ from torch's closed-interval rule, all at z in {{0, 1}} ({int(on_bound.sum())} such)")
    assert not (differ & ~on_bound).any(), "clamp01_backward differs from the true derivative away from the bounds"
    assert torch.equal(got[on_bound], torch.zeros_like(got[on_bound])), "at y in {0, 1} the gradient must be blocked"


def test_act_backward_true_derivative(report):
    """LeakyReLU + residual: the kernel recovers the sign of z from y - res, with y = fp16(lrelu(z) + res).  Where |lrelu(z)| is below
    half the fp16 spacing at res the sum rounds back onto res (or past it) and the sign is lost; those elements, and only those, may
    take the other branch"""
    ops = _ops()
    N, C, H, W, slope = 2, 64, 9, 13, 0.1
    gen = torch.Generator().manual_seed(71)
    z = randn(N, C, H, W, seed=72) * torch.pow(2.0, -14.0 * torch.rand(N, C, H, W, generator=gen))      # magnitudes 2^-14 .. 1
    res = rnd16(randn(N, C, H, W, seed=73))
    lz = F.leaky_relu(z.double(), slope)
    y = (lz + res.double()).half().float()
    g = rnd16(randn(N, C, H, W, seed=74))
    out = ops.act_backward(to_fm(g, ops), to_fm(y, ops), ops.ACT_LRELU, slope, res=to_fm(res, ops), out=ops.FM.empty(N, H, W, C))
    got = fm_to_cpu(out)
    # the existing rule (the kernel's own reconstruction) holds exactly
    assert_close(got, torch.where(y - res > 0, g, rnd16(g * slope)), 0, 0, "act_backward lrelu + residual (stored-sign rule)", report)
    true = torch.where(z > 0, g, rnd16(g * slope))
    differ = got != true
    # fp16 spacing at |res|: 2^(floor(log2|res|) - 10), at least the subnormal spacing
    e = torch.floor(torch.log2(res.double().abs().clamp_min(2.0 ** -14)))
    spacing = torch.pow(2.0, e - 10)
    lost = lz.abs() <= spacing / 2
    report(f"act_backward: {int(differ.sum())} of {differ.numel()} elements take the other branch than the true derivative; "
           f"{int(lost.sum())} elements have |lrelu(z)| <= half the fp16 spacing at res")
    assert not (differ & ~lost).any(), "act_backward differs from the true derivative outside the fp16-resolution set"
    assert differ.any(), "the test data must reach the resolution limit"


# ------------------------------------------------------------------------------------------------------------------ FeatureFix gather
def _gather_blocks(fref, ind, scale, H, W):
    """the oracle's block gather (oracle/tdvc_ref/blocks.py FeatureFix.match) for a given patch index"""
    N, C = fref.shape[:2]
    ks = 3 * scale
    ru = F.unfold(fref, ks, padding=ks, stride=ks).transpose(2, 1).reshape(N, -1, C * ks * ks)
    idx = ind.view(N, 1, -1).expand(-1, C * ks * ks, -1).permute(0, 2, 1)
    g = torch.gather(ru, 1, idx).view(N, -1, C, ks, ks).permute(0, 2, 3, 4, 1).reshape(N, C * ks * ks, -1)
    return F.fold(g, (H, W), ks, padding=ks, stride=ks)


MATCH_CASES = [(40, 56, 4), (48, 72, 8), (56, 80, 8)]        # 40 x 56 and 56 x 80 are not multiples of 3 * scale


@pytest.mark.parametrize("H,W,scale", MATCH_CASES, ids=[f"{h}x{w}_s{s}" for h, w, s in MATCH_CASES])
def test_match_gather_backward(H, W, scale, report):
    """cat = [fin, out] * cos(fin, out), out = fref blocks gathered by idx: many output blocks share a reference block (their
    gradients must sum), and some point at border blocks that lie (partly) outside the map (out = 0 there: the dead branch)"""
    ops = _ops()
    N, C = 2, 64
    ks = 3 * scale
    nbh, nbw = (H + ks) // ks + 1, (W + ks) // ks + 1
    fin, fref = rnd16(randn(N, C, H, W, seed=81)), rnd16(randn(N, C, H, W, seed=82))
    gen = torch.Generator().manual_seed(83)
    hot = [nbw + 1, 2 * nbw + 2, 0, nbh * nbw - 1, nbw - 1]          # interior blocks, the outside corner, overhanging last block
    ind = torch.tensor(hot, dtype=torch.long)[torch.randint(0, len(hot), (N, nbh * nbw), generator=gen)]
    ind[:, ::3] = torch.randint(0, nbh * nbw, (N, (nbh * nbw + 2) // 3), generator=gen)
    fr_, rr_ = _leaf(fin), _leaf(fref)
    out = _gather_blocks(rr_, ind, scale, H, W)
    cor = F.cosine_similarity(fr_, out).unsqueeze(1)                  # test_feature_matching's cosine (eps 1e-8)
    cat = torch.cat([fr_, out], 1) * cor
    dcat = rnd16(randn(N, 2 * C, H, W, seed=84))
    dfin_r, dfref_r = _grad((cat * dcat.double()).sum(), (fr_, rr_))
    dead = int((out.detach().abs().sum(1) == 0).sum())
    report(f"match_gather_backward {H}x{W} s{scale}: {dead} output pixels read outside the map; reference blocks used "
           f"{int(torch.unique(ind).numel())} of {nbh * nbw}")
    assert dead > 0

    f_in, f_ref = to_fm(fin, ops), to_fm(fref, ops)
    idx = ind.to(torch.int32).cuda()
    catf = ops.FM.empty(N, H, W, 2 * C)
    ops.match_gather(f_in, f_ref, idx, scale, catf)
    assert_close(fm_to_cpu(catf), cat.detach(), 2 * EPS16, 1e-4, f"match_gather forward {H}x{W} s{scale}", report)
    b_in, b_ref = rnd16(randn(N, C, H, W, seed=85) * 0.5), rnd16(randn(N, C, H, W, seed=86) * 0.5)
    dfin, dfref = to_fm(b_in, ops), to_fm(b_ref, ops)
    ops.match_gather_backward(f_in, f_ref, idx, scale, to_fm(dcat, ops), dfin, dfref)
    # fp32 64-channel dot products per pixel (~64 EPS32 of the largest term), summed over the blocks that share a reference
    # block, then one fp16 store: 2e-5 of the tensor's largest gradient on top of the half-ulp
    ref_in, ref_ref = b_in.double() + dfin_r, b_ref.double() + dfref_r
    assert_close(fm_to_cpu(dfin), ref_in, EPS16, 2e-5 * float(dfin_r.abs().max()) + TINY16, f"match_gather_backward dfin {H}x{W} s{scale}", report)
    assert_close(fm_to_cpu(dfref), ref_ref, EPS16, 2e-5 * float(dfref_r.abs().max()) + TINY16, f"match_gather_backward dfref {H}x{W} s{scale}", report)


# ------------------------------------------------------------------------------------------------------------------ DCN backward
G_DCN, C_DCN = 8, 64
_ONEHOT = None


def _onehot():
    """(576, 64, 3, 3): output channel c * 9 + t of the reference DCN is the sampled column (c, t)"""
    global _ONEHOT
    if _ONEHOT is None:
        w = torch.zeros(C_DCN * 9, C_DCN, 3, 3, dtype=torch.float64)
        for c in range(C_DCN):
            for t in range(9):
                w[c * 9 + t, c, t // 3, t % 3] = 1.0
        _ONEHOT = w
    return _ONEHOT


def _ref_columns(x, off, mraw):
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    return dcn_v2_forward_ref(x, _onehot(), torch.zeros(C_DCN * 9, dtype=torch.float64), off, torch.sigmoid(mraw), 3, 3, 1, 1, 1, 1, 1, 1, G_DCN)


# kernel column channel k = g * 72 + t * 8 + j  <->  reference channel (g * 8 + j) * 9 + t
_KPERM = torch.tensor([(g * 8 + j) * 9 + t for g in range(G_DCN) for t in range(9) for j in range(8)])


def _dcn_inputs(regime, N, H, W, seed, band=None):
    x = rnd16(randn(N, C_DCN, H, W, seed=seed))
    off = _offsets(regime, N, H, W, seed + 1, band)
    mraw = rnd16(randn(N, H, W, 9 * G_DCN, seed=seed + 2) * 1.5)
    om = torch.cat([off, mraw], -1)                                       # NHWC [offsets 144 | mask logits 72]
    return x, om


def _ref_col2im(x, om, dcol):
    """float64: columns(x, off, sigmoid(mraw)) and the adjoint of <columns, dcol> in x, offsets and raw mask (NHWC for om)"""
    N, _, H, W = x.shape
    xr = _leaf(x)
    offr = _leaf(_nchw(om[..., :144]))
    mr = _leaf(_nchw(om[..., 144:]))
    cols = _ref_columns(xr, offr, mr)
    dcol_ref = _nchw(dcol)[:, torch.argsort(_KPERM)]                     # kernel order -> reference order
    dx, doff, dm = _grad((cols * dcol_ref.double()).sum(), (xr, offr, mr))
    with torch.enable_grad():
        xa = x.double().clone().requires_grad_()
        cols_abs = _ref_columns(xa, offr.detach(), mr.detach())
        (dx_abs,) = _grad((cols_abs * dcol_ref.double().abs()).sum(), (xa,))     # mask * bilinear weights >= 0: sum of |terms|
    return cols.detach(), dx, _nhwc(torch.cat([doff, dm], 1)), dx_abs


DCN_REGIMES = ["subpixel", "coherent", "wild", "border", "integer"]


def test_dcn_columns(report):
    """dcn_columns (the sampled columns for dW) vs the reference's columns, on a ragged N = 2 map with every offset regime mixed by rows"""
    ops = _ops()
    N, H, W = 2, 19, 27
    x = rnd16(randn(N, C_DCN, H, W, seed=91))
    offs = [_offsets(r, N, H, W, 92 + i) for i, r in enumerate(DCN_REGIMES)]
    rowsel = torch.arange(H) % len(DCN_REGIMES)
    off = torch.stack(offs)[rowsel, :, torch.arange(H)].permute(1, 0, 2, 3)
    mraw = rnd16(randn(N, H, W, 9 * G_DCN, seed=99) * 1.5)
    om = torch.cat([off, mraw], -1)
    col = ops.dcn_columns(to_fm(x, ops), ops.FM(om.half().cuda()), G_DCN)
    got = fm_to_cpu(col)
    ref = _ref_columns(x.double(), _nchw(om[..., :144]).double(), _nchw(om[..., 144:]).double())[:, _KPERM]
    # fp32 bilinear weights on fp16 values (4 products), __expf sigmoid (~1e-6 relative), one fp16 store of a value <= max|x|
    assert_close(got, ref, EPS16, 1e-5 * float(x.abs().max()) + TINY16, "dcn_columns", report)


def _run_col2im(ops, x, om, dcol, dom0):
    xf, omf = to_fm(x, ops), ops.FM(om.half().cuda())
    dom = ops.FM(dom0.half().cuda())
    dx32 = ops.dcn_col2im(xf, omf, ops.FM(dcol.half().cuda()), G_DCN, dom)
    torch.cuda.synchronize()
    return fm_to_cpu(dx32).double(), dom.t.float().cpu().double()


def _check_col2im(tag, got_dx, got_dom, ref, dom0, report):
    _, dx_r, dom_r, dx_abs = ref
    # dx: fp32 sums of dcol * mask * w (mask from __expf, weights fp32: ~1e-6 relative per term), window + far adds
    assert_close(got_dx, dx_r, 0, 1e-5 * dx_abs + 1e-30, f"{tag} dx", report)
    # d offset / d raw mask: per sample, fp32 8-channel dot products over 4 corners, then one fp16 store onto the prefilled dom
    want = dom0.double() + dom_r
    for name, sl in (("doffset", slice(0, 144)), ("dmask", slice(144, 216))):
        r = want[..., sl]
        assert_close(got_dom[..., sl], r, EPS16, 1e-4 * float(dom_r[..., sl].abs().max()) + TINY16, f"{tag} {name}", report)


@pytest.mark.parametrize("regime", DCN_REGIMES)
def test_dcn_col2im(regime, report):
    """dx, d offset and d raw mask of <columns(x, off, sigmoid(m)), dcol>, default and deterministic modes.  Map A (2 x 29 x 37:
    tiles overhang both edges) runs the regime everywhere in default mode; map B (the same map with the regime confined to rows
    14-15, the bottom rows of a tile) keeps the far records under the deterministic capacity and runs both modes"""
    ops = _ops()
    N, H, W = 2, 29, 37
    dcol = rnd16(randn(N, H, W, 72 * G_DCN, seed=101) * 0.5)
    dom0 = rnd16(randn(N, H, W, 27 * G_DCN, seed=102) * 0.1)
    prev = ops.DETERMINISTIC
    try:
        ops.DETERMINISTIC = False
        x, om = _dcn_inputs(regime, N, H, W, 110)
        active, far, h, w = _far_stats(om, H, W)
        report(f"dcn_col2im {regime} (full map): {far} of {active} active corners outside their tile's 24x24 window")
        if regime in ("coherent", "wild"):
            assert far > (active // 3 if regime == "coherent" else active // 5), "the regime must reach the far path"
        if regime == "border":
            for lo, hi, what in ((-1, 0, "h in (-1, 0)"), (H - 1, H, "h in (H-1, H)")):
                assert ((h > lo) & (h < hi)).any(), what
            assert ((w > -1) & (w < 0)).any() and ((w > W - 1) & (w < W)).any() and (h <= -1).any() and (w >= W).any()
        ref = _ref_col2im(x, om, dcol)
        got_dx, got_dom = _run_col2im(ops, x, om, dcol, dom0)
        _check_col2im(f"dcn_col2im {regime} default", got_dx, got_dom, ref, dom0, report)

        xb, omb = _dcn_inputs(regime, N, H, W, 120, band=(14, 16))
        active, far, _, _ = _far_stats(omb, H, W)
        cap = max(1 << 16, N * H * W * G_DCN * 36 // 8)
        report(f"dcn_col2im {regime} (band): {far} of {active} active corners far; deterministic record capacity {cap}")
        assert far <= cap
        refb = _ref_col2im(xb, omb, dcol)
        d_dx, d_dom = _run_col2im(ops, xb, omb, dcol, dom0)
        ops.DETERMINISTIC = True
        a_dx, a_dom = _run_col2im(ops, xb, omb, dcol, dom0)
        b_dx, b_dom = _run_col2im(ops, xb, omb, dcol, dom0)
    finally:
        ops.DETERMINISTIC = prev
    _check_col2im(f"dcn_col2im {regime} band default", d_dx, d_dom, refb, dom0, report)
    _check_col2im(f"dcn_col2im {regime} band deterministic", a_dx, a_dom, refb, dom0, report)
    assert torch.equal(a_dx, b_dx) and torch.equal(a_dom, b_dom), "deterministic mode: two runs differ"
    # the modes differ only in the order the far samples are added: fp32 summation order, bounded by the sum of |terms|
    assert_close(a_dx, d_dx, 0, 1e-5 * refb[3] + 1e-30, f"dcn_col2im {regime} default vs deterministic", report)
    assert torch.equal(a_dom, d_dom), "the offset / mask gradients do not depend on the mode"


def test_dcn_col2im_deterministic_capacity(report):
    """coherent motion above 8 px over a whole 2 x 29 x 37 map: nearly every sample is far, more than the record buffer holds
    (max(65 536, N H W G 36 / 8)); the deterministic mode must refuse instead of returning a partial dx"""
    ops = _ops()
    from tdvc_amd import _lib as L
    N, H, W = 2, 29, 37
    x, om = _dcn_inputs("coherent", N, H, W, 130)
    _, far, _, _ = _far_stats(om, H, W)
    cap = max(1 << 16, N * H * W * G_DCN * 36 // 8)
    report(f"dcn_col2im capacity: {far} far corners for a capacity of {cap}")
    assert far > cap
    dcol = rnd16(randn(N, H, W, 72 * G_DCN, seed=131) * 0.5)
    prev = ops.DETERMINISTIC
    ops.DETERMINISTIC = True
    try:
        with pytest.raises(L.TdvcHipError, match="exceed the record capacity"):
            ops.dcn_col2im(to_fm(x, ops), ops.FM(om.half().cuda()), ops.FM(dcol.half().cuda()), G_DCN, ops.FM.zeros(N, H, W, 216))
    finally:
        ops.DETERMINISTIC = prev


def test_dcn_fused_record_backward(report):
    """the tape's DCN backward (autograd.record_dcn_fused: columns -> conv_wgrad -> conv_dgrad -> col2im) on a ragged N = 2 map
    against autograd of dcn_v2_forward_ref: dW, db, dx, d offset, d raw mask"""
    ops = _ops()
    from tdvc_amd import autograd
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    N, H, W = 2, 13, 19
    x, om = _dcn_inputs("wild", N, H, W, 140)
    om[..., :144] = rnd16(om[..., :144] * (2.0 / 9.0))                  # sigma 2 px: window and far samples both
    w = rnd16(randn(C_DCN, C_DCN, 3, 3, seed=141) * (1.0 / 24))
    b = randn(C_DCN, seed=142) * 0.1
    g = rnd16(randn(N, C_DCN, H, W, seed=143) * 0.5)
    wp, bp = torch.nn.Parameter(w.cuda()), torch.nn.Parameter(b.cuda())
    pc = ops.pack_conv(wp, bp, stride=1, pad=1, ck=8 * G_DCN)
    xf, omf = to_fm(x, ops), ops.FM(om.half().cuda())
    out = ops.FM.empty(N, H, W, C_DCN)
    with autograd.record() as tape:
        ops.dcn_fused(xf, omf, pc, out, groups=G_DCN)
        tape.grad(out).t.copy_(_nhwc(g).half().cuda())
        tape.backward()
        dx = fm_to_cpu(tape.grad(xf)).double()
        dom = tape.grad(omf).t.float().cpu().double()
    xr, wr, br = _leaf(x), _leaf(w), _leaf(b)
    offr, mr = _leaf(_nchw(om[..., :144])), _leaf(_nchw(om[..., 144:]))
    y = dcn_v2_forward_ref(xr, wr, br, offr, torch.sigmoid(mr), 3, 3, 1, 1, 1, 1, 1, 1, G_DCN)
    dx_r, dw_r, db_r, doff_r, dm_r = _grad((y * g.double()).sum(), (xr, wr, br, offr, mr))
    # dW = sum_pix g col with the columns stored in fp16 (dcn_columns' bound per column: EPS16 relative + 1e-5 max|x|)
    with torch.no_grad():
        cols = _ref_columns(x.double(), offr.detach(), mr.detach())                    # (N, 576, H, W), channel c * 9 + t
        dw_abs = torch.einsum("nohw,nkhw->ok", g.double().abs(), cols.abs()).view(C_DCN, C_DCN, 3, 3)
        gsum = g.double().abs().sum((0, 2, 3)).view(C_DCN, 1, 1, 1)
        dcol_abs = torch.einsum("oct,nohw->ncthw", w.double().reshape(C_DCN, C_DCN, 9), g.double()).abs().reshape(N, 9 * C_DCN, H, W)
    assert_close(wp.grad.cpu(), dw_r, 0, 2 * EPS16 * dw_abs + 1e-5 * float(x.abs().max()) * gsum + 1e-6, "record_dcn_fused dW", report)
    # db = sum g: an fp32 sum of fp16 values
    assert_close(bp.grad.cpu(), db_r, 0, 64 * EPS32 * gsum.view(-1) + 1e-7, "record_dcn_fused db", report)
    # dx: dcol = fp16(W^T g) errs by EPS16 |dcol| per element, carried by the (non-negative) scatter weights: EPS16 times the
    # adjoint of |dcol|; then fp32 scatter sums (1e-5 of the same) and the fp16 mirror store
    xa = x.double().clone().requires_grad_()
    (dx_abs,) = _grad((_ref_columns(xa, offr.detach(), mr.detach()) * dcol_abs).sum(), (xa,))
    assert_close(dx, dx_r, R16, (EPS16 + 1e-5) * dx_abs + TINY16, "record_dcn_fused dx", report)
    # dom: 8-channel x 4-corner dot products per sample of the same fp16 dcol, stored in fp16: a few EPS16 of the tensor's scale
    dom_r = _nhwc(torch.cat([doff_r, dm_r], 1))
    assert_close(dom[..., :144], dom_r[..., :144], 2 * EPS16, 4 * EPS16 * float(dom_r[..., :144].abs().max()), "record_dcn_fused doffset", report)
    assert_close(dom[..., 144:], dom_r[..., 144:], 2 * EPS16, 4 * EPS16 * float(dom_r[..., 144:].abs().max()), "record_dcn_fused dmask", report)


# geometry classes (kh, kw, stride, cin, cout, shuffle, square_x, masked) of the conv weight gradients the tests in this file run
# at op level: the GDN / IGDN 1x1 over x^2, the DCN weight as a 1x1 conv over 576 sampled columns.  Read by the coverage guard
# in test_conv_backward_gpu.py.
WGRAD_CLASSES = {(1, 1, 1, 128, 128, False, True, False), (1, 1, 1, 9 * C_DCN, C_DCN, False, False, False)}


# ------------------------------------------------------------------------------------------------------------------ bias gradient
# C = 264: a last 256-channel block (blockIdx.z = 1) of 8 channels; 5 x 7: one pixel range, 40 x 52: two ranges of 1040 pixels
# (tdvc_bias_grad cuts npix / 1024 ranges), which a 256 / (C / 8)-lane walk does not divide evenly
BIAS_GRAD_CASES = [(C, H, W, dt) for C in (8, 216, 264) for (H, W) in ((5, 7), (40, 52)) for dt in (torch.float16, torch.float32)]


@pytest.mark.parametrize("C,H,W,dt", BIAS_GRAD_CASES, ids=[f"C{c}_{h}x{w}_{'f16' if dt == torch.float16 else 'f32'}" for c, h, w, dt in BIAS_GRAD_CASES])
def test_bias_grad_exact(C, H, W, dt):
    """db[dst[c] or c] += scale * sum over batch and pixels of g[..., c], c < nvalid (channel_sum_wide_kernel + reduce_rows_kernel).
    Inputs are small integers: every partial sum is an integer far below 2^24, so fp32 holds it exactly in any order and the result
    is compared bit for bit with a float64 sum.  With and without a dst_index (a permutation with -1 entries, nvalid < C)."""
    ops = _ops()
    from tdvc_amd import _lib as L
    N = 2
    gen = torch.Generator().manual_seed(C * 1000 + H)
    g = torch.randint(-4, 5, (N, H, W, C), generator=gen).to(dt).cuda()
    gf = ops.FM(g)
    s = g.cpu().double().sum((0, 1, 2))
    nwork = L.lib().tdvc_bias_grad_work_floats(N, C)
    for nvalid, indexed in ((C, False), (C - 3, True)):
        base = torch.randint(-8, 9, (C,), generator=gen).float() * 0.25
        dst = torch.randperm(C, generator=gen).to(torch.int32)
        dst[torch.randperm(C, generator=gen)[:3]] = -1
        want = base.double().clone()
        for c in range(nvalid):
            d = int(dst[c]) if indexed else c
            if d >= 0:
                want[d] += 0.5 * s[c]
        db = base.cuda()
        work = torch.full((nwork,), float("nan"), device="cuda")
        idx = dst.cuda() if indexed else None
        L.check(L.lib().tdvc_bias_grad(ops.C.byref(gf.desc()), nvalid, idx.data_ptr() if indexed else None, 0.5, db.data_ptr(), work.data_ptr(), nwork,
                                       ops._stream()), "bias_grad")
        assert torch.equal(db.cpu().double(), want), f"bias_grad C{C} {H}x{W} nvalid {nvalid} indexed {indexed}: {int((db.cpu().double() != want).sum())} of {C} differ"
