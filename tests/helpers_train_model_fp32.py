"""Case tables, data, float64 restatements and counted bounds of the fp32 adjoint forms the whole-model fp32 training mode adds
(tests/test_train_model_fp32_ops_gpu.py runs them on the GPU, tests/test_train_model_fp32_cases_cpu.py checks the restatements against
torch.autograd and the sensitivity of every bound without one).  Nothing here touches the compiled library.

Data is made on the CPU as NHWC tensors with full fp32 mantissas (the point of the mode: an fp16 rounding anywhere must show), except
where a row says otherwise.  EPS32 = 2^-24 is half an fp32 ulp, relative; the library builds with -ffp-contract=off and without
fast-math, so every fp32 operation is rounded once.  A bound is EPS32 x (the number of roundings a term passes on its way into the
result) x (the sum of the absolute terms, in float64), whatever the order of the additions.  The counts:

  add_flow_backward    a term doff[c] is added inside its chunk of 8 channels (3 additions: ((v0 + v2) + v4) + v6), the chunk sums are
                       added serially (C / 8), the total is added to dflow (1): C / 8 + 4.  dflow's old value is one of the terms.
  bcast_add_act_backward   dx = g or g * slope: one rounding, 1 x |dx|.  db = ((db0 + dx_0) + dx_1) + ...: a term passes its product and
                       at most T additions: T + 1.
  upsample2x_backward  weights wy * wx are exact (multiples of 1 / 16).  A term passes its product (1) and at most 16 + 1 serial
                       additions onto dx's old value (at most 4 x 4 output pixels see an input pixel with a non-zero weight): 18.
  match_gather_backward    da = ga cor + dc (b / D - ka a), cor = a.b / D, D = |a| |b|, ka = cor / |a|^2, dc = sum ga a + gb b
                       (csrc/backward_ops.hip::match_pair_grad; db by symmetry).  A term of a 64-channel sum passes its product, 7
                       additions in its lane and 3 shuffle additions: 11 (dc: one more, 12).  As in tests/helpers_fp32_ops.py the dot
                       errs by 11 EPS32 D, a squared norm by 11 EPS32 relative, its root by 6.5, D by 14, so |d cor| <= 26 EPS32
                       (|cor| <= 1).  ka = cor / w1: (26 + 11 + 1) EPS32 / w1.  ga cor: 27 EPS32 |ga|.  u = b / D - ka a:
                       EPS32 (16 |b| / D + 40 |a| / w1).  dc u with |dc| <= A = sum |ga a| + |gb b| and |u| <= |b| / D + |a| / w1:
                       EPS32 A (29 |b| / D + 53 |a| / w1).  The last addition and the accumulation into the mirror: 2 EPS32 |result| each
                       (|base| included), and dfref adds one such term per output block matched to the pixel's block.  Dead pairs
                       (D <= 1e-8: the source block lies outside the map, b = 0) give exactly 0 on both sides.
  spynet_level_input_backward   no count: the kernel is the fp16 form's and reads dcat8 through the generic 8-channel reader; the fp32
                       dcat8 is held to bit-identity with the fp16-dcat8 call on fp16-exact values and to an exact pass-through
                       (dflow_up = fp32(base + dcat8[6:8]) over a constant image) on full fp32 mantissas.
  dcn_columns          col = mask * sum_corners wt * v.  A term passes its product (1), at most 4 additions, the weight's own roundings
                       (1 - lh, 1 - lw, their product: 3), the product with the mask (1) and the mask's (expf to 1 ulp = 2 EPS32, the
                       addition, the division: 4): 13.
  dcn_col2im dx        a term dcol * mask * wt passes two products, the weight's 3 and the mask's 4 roundings: 9; n terms land on the
                       element (counted per element from the offsets) and are added in some order -- by the owner's plain LDS add, an
                       LDS atomic, a global atomic or the far path's sorted sum -- then the (up to) 9 windows and dx32's old value: n + 10
                       additions.  (n + 19) EPS32 sum|terms|: order-independent, so atomics are covered.
  dcn_col2im dom       d offset = mask * sum_corners wth * (sum_8 dcol_c x_c): product (1), 8 additions, wth's rounding (1), the
                       product with it (1), 4 additions, the mask (1 + 4), the addition onto dom (1): 21 over the 8 channels x 4
                       corners; d mask logit = dval * mask * (1 - mask): 3 + 1 roundings more for wt and the extra product: 25, and the
                       factor (1 - mask) is a difference of the ROUNDED mask: its absolute error is the mask's, 4 EPS32 mask, that is
                       4 mask / (1 - mask) EPS32 relative -- counted per element (a logit of 5 makes it 600).
                       Plus EPS32 |result| for the stored sum.
                       Offsets are the regimes of tests/helpers_dcn.py rounded to multiples of 2^-10: below 64 pixels integer + offset
                       is then exact in fp32 (17 bits) and so are lh, 1 - lh and the corner weights (20 fraction bits), so the kernel and
                       the float64 restatement sample the same positions with the same weights; the roundings the counts grant the
                       weights stay in the bounds.  x, dcol and the mask logits carry full fp32 mantissas.

Conv data / weight gradients use tests/test_conv_wgrad_f32_gpu.py's bounds unchanged; this file holds only their case rows.
"""
import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
ULP16 = 2.0 ** -11            # one fp16 ulp, relative: the perturbation every bound must notice
G_DCN, C_DCN = 8, 64


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))))


def draw(g, shape, scale=1.0):
    """normal values with full fp32 mantissas"""
    return torch.randn(shape, generator=g) * scale


def ratio(got, ref, bound):
    """max(|d| / bound) with 0 / 0 = 0 (an exact element under a zero bound)"""
    d = (got.double() - ref.double()).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(r.max())


def perturb(t, *key):
    """every element moved by one fp16 ulp, relative, up or down"""
    s = torch.randint(0, 2, t.shape, generator=gen("perturb", *key)).double() * 2 - 1
    return t.double() * (1.0 + s * ULP16)


# ------------------------------------------------------------------------------------------------- add_flow_backward
# (name, N, H, W, C of doff, doff buffer channels, dflow buffer channels)
AFB_CASES = [("view_c64_f8", 2, 5, 7, 64, 128, 8), ("dense_c144_f2", 1, 3, 9, 144, 144, 2), ("dense_c8_f8", 2, 1, 3, 8, 8, 8)]


def afb_data(row):
    name, N, H, W, C_, Cb, Cf = row
    g = gen("afb", name)
    return draw(g, (N, H, W, Cb)), draw(g, (N, H, W, Cf), 2.0)


def afb_ref(row, doffbuf, dflow):
    """-> (dflow after the call, float64; bound).  Channels 2.. of dflow are not touched."""
    C_, Cb = row[4], row[5]
    d = doffbuf.double()[..., Cb - C_:]
    want = dflow.double().clone()
    want[..., 0] += d[..., 0::2].sum(-1)
    want[..., 1] += d[..., 1::2].sum(-1)
    absr = dflow.double().abs().clone()
    absr[..., 0] += d[..., 0::2].abs().sum(-1)
    absr[..., 1] += d[..., 1::2].abs().sum(-1)
    bound = EPS32 * (C_ // 8 + 4) * absr
    bound[..., 2:] = 0.0
    return want, bound


# ------------------------------------------------------------------------------------------------- bcast_add_act_backward
# (name, N, H, W, Cb, T, leading buffer channels of x / dx: a cat-style view when non-zero)
BCB_CASES = [("view_c64_t4", 2, 5, 7, 64, 4, 64), ("dense_c64_t4", 1, 3, 3, 64, 4, 0), ("dense_c8_t3", 2, 1, 5, 8, 3, 0)]
BCB_SLOPE = 0.1


def bcb_data(row):
    """-> (x = the forward's stored OUTPUT lrelu(z), dx, db), buffers; x and dx share their view geometry"""
    name, N, H, W, Cb, T, lead = row
    g = gen("bcb", name)
    z = draw(g, (N, H, W, lead + T * Cb))
    x = torch.where(z > 0, z, z * torch.tensor(BCB_SLOPE))
    return x, draw(g, (N, H, W, lead + T * Cb)), draw(g, (N, H, W, Cb), 0.5)


def bcb_ref(row, xbuf, dxbuf, db):
    """-> (dx view after, db after, bound dx, bound db) in float64"""
    name, N, H, W, Cb, T, lead = row
    x, g = xbuf.double()[..., lead:], dxbuf.double()[..., lead:]
    dx = torch.where(x > 0, g, g * float(torch.tensor(BCB_SLOPE, dtype=torch.float32)))
    s = dx.reshape(N, H, W, T, Cb)
    want_db = db.double() + s.sum(3)
    return dx, want_db, EPS32 * dx.abs(), EPS32 * (T + 1) * (db.double().abs() + s.abs().sum(3))


# ------------------------------------------------------------------------------------------------- upsample2x_backward
# (name, N, h, w, C, dy buffer channels, dx buffer channels)
UPB_CASES = [("view_c64", 2, 5, 7, 64, 128, 128), ("dense_c8_1xw", 1, 1, 3, 8, 8, 8), ("dense_c16_hx1", 2, 4, 1, 16, 16, 16)]


def _up_matrix(n):
    """(2n, n) float64: row o of nn.Upsample(scale_factor=2, bilinear, align_corners=False) along one axis (csrc/pointwise.hip)"""
    U = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        s = max((o + 0.5) * 0.5 - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        U[o, i0] += 1.0 - (s - i0)
        U[o, i1] += s - i0
    return U


def upb_data(row):
    name, N, h, w, C_, Cy, Cx = row
    g = gen("upb", name)
    return draw(g, (N, 2 * h, 2 * w, Cy)), draw(g, (N, h, w, Cx), 0.5)


def upb_adjoint(dy, h, w):
    """U^T dy for NHWC float64 dy of size (N, 2h, 2w, C)"""
    return torch.einsum("oy,px,nopc->nyxc", _up_matrix(h), _up_matrix(w), dy)


def upb_ref(row, dybuf, dxbuf):
    name, N, h, w, C_, Cy, Cx = row
    dy, dx0 = dybuf.double()[..., Cy - C_:], dxbuf.double()[..., Cx - C_:]
    return dx0 + upb_adjoint(dy, h, w), EPS32 * 18 * (dx0.abs() + upb_adjoint(dy.abs(), h, w))


# ------------------------------------------------------------------------------------------------- match_gather_backward
# (name, N, H, W, scale, cat-style views): scale 8 is the training scale; 8 x 8 is the smallest map the launcher's fold-grid rule takes
# at scale 8 (one pooled cell, a 2 x 2 fold grid); 40 x 56 is no multiple of 3 * scale = 24: a ragged fold grid
MGB_CASES = [("8x8_s8", 2, 8, 8, 8, False), ("40x56_s8_ragged_view", 2, 40, 56, 8, True)]
MGB_C = 64


def mgb_grid(H, W, scale):
    ks = 3 * scale
    return ks, (H + ks) // ks + 1, (W + ks) // ks + 1


def mgb_data(row):
    """-> fin, fref, dcat (128 channels), dfin0, dfref0 as NHWC fp32 and idx (N, nbh * nbw) int64: a few hot reference blocks shared by
    many output blocks, the outside corner block and the overhanging last block among them"""
    name, N, H, W, scale, view = row
    ks, nbh, nbw = mgb_grid(H, W, scale)
    g = gen("mgb", name)
    hot = torch.tensor([nbw + 1, 0, nbh * nbw - 1, nbw - 1, min(2 * nbw + 1, nbh * nbw - 1)])
    idx = hot[torch.randint(0, len(hot), (N, nbh * nbw), generator=g)]
    idx[:, ::3] = torch.randint(0, nbh * nbw, (N, (nbh * nbw + 2) // 3), generator=g)
    idx[0, nbw + 1], idx[1, nbw + 1] = nbw + 1, 0         # the first block: itself in image 0 (live), the outside corner in image 1 (dead)
    sh = (N, H, W, MGB_C)
    return draw(g, sh), draw(g, sh), draw(g, (N, H, W, 2 * MGB_C)), draw(g, sh, 0.5), draw(g, sh, 0.5), idx


def mgb_source(idx, H, W, scale):
    """per output pixel: (flat source pixel in fref, clamped; valid) by the fold-grid rule of match_gather_kernel"""
    ks, nbh, nbw = mgb_grid(H, W, scale)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = idx[:, ((yy // ks + 1) * nbw + (xx // ks + 1)).reshape(-1)].view(-1, H, W)
    sy, sx = (m // nbw - 1) * ks + yy % ks, (m % nbw - 1) * ks + xx % ks
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return (sy.clamp(0, H - 1) * W + sx.clamp(0, W - 1)), ok


def mgb_forward(fin, fref, idx, scale):
    """cat = [a cor | b cor] (differentiable float64 restatement of match_gather; NHWC)"""
    N, H, W, C_ = fin.shape
    src, ok = mgb_source(idx, H, W, scale)
    b = torch.gather(fref.reshape(N, H * W, C_), 1, src.view(N, H * W, 1).expand(-1, -1, C_)).view(N, H, W, C_) * ok.unsqueeze(-1)
    cor = F.cosine_similarity(fin, b, dim=-1, eps=1e-8).unsqueeze(-1)        # a dead pair (b = 0) has cor = 0 and a zero gradient
    return torch.cat([fin * cor, b * cor], -1)


def mgb_ref(row, fin, fref, dcat, dfin0, dfref0, idx):
    """float64 restatement of match_pair_grad and its two gathers -> (dfin, dfref, bound dfin, bound dfref)"""
    name, N, H, W, scale, view = row
    a, ga, gb = fin.double(), dcat.double()[..., :MGB_C], dcat.double()[..., MGB_C:]
    src, ok = mgb_source(idx, H, W, scale)
    gidx = src.view(N, H * W, 1).expand(-1, -1, MGB_C)
    b = torch.gather(fref.double().reshape(N, H * W, MGB_C), 1, gidx).view(N, H, W, MGB_C) * ok.unsqueeze(-1)
    w12, w1, w2 = (a * b).sum(-1, keepdim=True), (a * a).sum(-1, keepdim=True), (b * b).sum(-1, keepdim=True)
    dc = (ga * a + gb * b).sum(-1, keepdim=True)
    A = (ga * a).abs().sum(-1, keepdim=True) + (gb * b).abs().sum(-1, keepdim=True)
    den = w1.sqrt() * w2.sqrt()
    live = den > 1e-8
    D = torch.where(live, den, torch.full_like(den, 1e-8))
    cor = w12 / D
    ka, kb = torch.where(live, cor / w1, torch.zeros_like(cor)), torch.where(live, cor / w2.clamp_min(1e-300), torch.zeros_like(cor))
    da = ga * cor + dc * (b / D - ka * a)
    db = gb * cor + dc * (a / D - kb * b)
    zero = torch.zeros_like(da)
    ea = torch.where(live, 27 * ga.abs() + A * (29 * b.abs() / D + 53 * a.abs() / w1), zero)
    eb = torch.where(live, 27 * gb.abs() + A * (29 * a.abs() / D + 53 * b.abs() / w2.clamp_min(1e-300)), zero)
    dfin = dfin0.double() + da
    bfin = EPS32 * (ea + 2 * da.abs() + 2 * dfin0.double().abs() + 2 * dfin.abs())
    # dfref[q] += sum of db over the output pixels whose source is q
    flat = lambda t: (t * ok.unsqueeze(-1)).reshape(N, H * W, MGB_C)
    sc = lambda t: torch.zeros(N, H * W, MGB_C, dtype=torch.float64).scatter_add_(1, gidx, flat(t)).view(N, H, W, MGB_C)
    cnt = sc(torch.ones_like(db))
    dfref = dfref0.double() + sc(db)
    bref = EPS32 * (sc(eb) + (cnt + 3) * (sc(db.abs()) + dfref0.double().abs()))
    return dfin, dfref, bfin, bref


# ------------------------------------------------------------------------------------------------- DCN backward on fp32 maps
# maps: one smaller than a col2im tile, one spanning three tiles in each direction with ragged edges (tile side 8: read from the
# library by the GPU test, asserted here against DCN_TILE)
DCN_TILE = 8
DCN_MAPS = {"sub_tile": (2, 5, 7), "tiles_3x3_ragged": (2, 19, 21)}
DCN_BAND = (8, 10)            # deterministic runs on the large map: the regime on these rows only (the far records fit their buffer)


def dcn_data(regime, mapname, band=None):
    """x (N, H, W, 64), om (N, H, W, 216) = [offsets 144 | mask logits 72], dcol (N, H, W, 576), dom0 (N, H, W, 216): fp32 NHWC"""
    from helpers_dcn import offsets
    N, H, W = DCN_MAPS[mapname]
    g = gen("dcn", regime, mapname, band)
    seed = int(torch.randint(0, 1 << 30, (1,), generator=g))
    off = torch.round(offsets(regime, N, H, W, seed, band) * 1024.0) / 1024.0        # multiples of 2^-10: exact positions in fp32
    x = draw(g, (N, H, W, C_DCN))
    om = torch.cat([off, draw(g, (N, H, W, 9 * G_DCN), 1.5)], -1)
    return x, om, draw(g, (N, H, W, 72 * G_DCN), 0.5), draw(g, (N, H, W, 27 * G_DCN), 0.1)


def dcn_bw_ref(x, om, dcol=None):
    """float64 restatement of dcn_columns_kernel / dcn_col2im_kernel (NHWC; column channel k = g * 72 + t * 8 + j).
    -> dict(col, col_abs) and, with dcol: dx, dx_abs, count (terms landing per element), dom, dom_abs"""
    x, om = x.double(), om.double()
    N, H, W, _ = x.shape
    G = G_DCN
    off = om[..., :18 * G].reshape(N, H, W, G, 9, 2)
    m = torch.sigmoid(om[..., 18 * G:]).reshape(N, H, W, G, 9)
    t = torch.arange(9)
    yy = torch.arange(H).view(1, H, 1, 1, 1).double() - 1 + (t // 3).view(1, 1, 1, 1, 9)
    xx = torch.arange(W).view(1, 1, W, 1, 1).double() - 1 + (t % 3).view(1, 1, 1, 1, 9)
    h, w = yy + off[..., 0], xx + off[..., 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    xg = x.reshape(N, H * W, G, 8)
    ni = torch.arange(N).view(N, 1, 1, 1, 1).expand(N, H, W, G, 9)
    gi = torch.arange(G).view(1, 1, 1, G, 1).expand(N, H, W, G, 9)
    corners = ((0, 0, (1 - lh) * (1 - lw), -(1 - lw), -(1 - lh)), (0, 1, (1 - lh) * lw, -lw, (1 - lh)),
               (1, 0, lh * (1 - lw), (1 - lw), -lh), (1, 1, lh * lw, lw, lh))
    col = torch.zeros(N, H, W, G, 9, 8, dtype=torch.float64)
    col_abs = torch.zeros_like(col)
    out = {}
    if dcol is not None:
        dc = dcol.double().reshape(N, H, W, G, 9, 8)
        dx, dxa = torch.zeros(N, H * W, G, 8, dtype=torch.float64), torch.zeros(N, H * W, G, 8, dtype=torch.float64)
        cnt = torch.zeros(N, H * W, G, dtype=torch.float64)
        dval, dh, dw = (torch.zeros(N, H, W, G, 9, dtype=torch.float64) for _ in range(3))
        dvala, dha, dwa = (torch.zeros(N, H, W, G, 9, dtype=torch.float64) for _ in range(3))
    for cy, cx, wt, wth, wtw in corners:
        yc, xc = hl + cy, wl + cx
        act = (inside & (yc >= 0) & (yc <= H - 1) & (xc >= 0) & (xc <= W - 1)).double()
        pi = (yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long()
        v = xg[ni, pi, gi]                                        # (N, H, W, G, 9, 8)
        wa = (act * wt).unsqueeze(-1)
        col += wa * v
        col_abs += wa * v.abs()
        if dcol is not None:
            sx, sxa = (dc * v).sum(-1), (dc.abs() * v.abs()).sum(-1)
            dval += act * wt * sx
            dh += act * wth * sx
            dw += act * wtw * sx
            dvala += act * wt * sxa
            dha += act * wth.abs() * sxa
            dwa += act * wtw.abs() * sxa
            contrib = (act * m * wt).unsqueeze(-1) * dc
            dx.index_put_((ni, pi, gi), contrib, accumulate=True)
            dxa.index_put_((ni, pi, gi), contrib.abs(), accumulate=True)
            cnt.index_put_((ni, pi, gi), act, accumulate=True)
    mm = m.unsqueeze(-1)
    out["col"], out["col_abs"] = (col * mm).reshape(N, H, W, 72 * G), (col_abs * mm).reshape(N, H, W, 72 * G)
    out["mask"] = m.reshape(N, H, W, 9 * G)
    if dcol is not None:
        out["dx"], out["dx_abs"] = dx.view(N, H, W, 8 * G), dxa.view(N, H, W, 8 * G)
        out["count"] = cnt.view(N, H, W, G, 1).expand(N, H, W, G, 8).reshape(N, H, W, 8 * G)
        doff = torch.stack([dh * m, dw * m], -1).reshape(N, H, W, 18 * G)
        doffa = torch.stack([dha * m, dwa * m], -1).reshape(N, H, W, 18 * G)
        dm, dma = (dval * m * (1 - m)).reshape(N, H, W, 9 * G), (dvala * m * (1 - m)).reshape(N, H, W, 9 * G)
        out["dom"], out["dom_abs"] = torch.cat([doff, dm], -1), torch.cat([doffa, dma], -1)
    return out


def dcn_col_bound(ref):
    return EPS32 * 13 * ref["col_abs"]


def dcn_dx_bound(ref, dx0=None):
    base = 0.0 if dx0 is None else dx0.double().abs()
    return EPS32 * (ref["count"] + 19) * (ref["dx_abs"] + base)


def dcn_dom_bound(ref, dom0):
    G = G_DCN
    m = ref["mask"]
    k = torch.cat([torch.full_like(ref["dom"][..., :18 * G], 21.0), 25.0 + 4.0 * m / (1.0 - m)], -1)
    want = dom0.double() + ref["dom"]
    return want, EPS32 * (k * (ref["dom_abs"] + dom0.double().abs()) + want.abs())


def dcn_forward_oracle(x, om, onehot_cols):
    """columns by the oracle's deformable conv (autograd-capable float64): NHWC in, NHWC out in the kernel's channel order"""
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    c = dcn_v2_forward_ref(nchw(x), onehot_cols, torch.zeros(C_DCN * 9, dtype=torch.float64), nchw(om[..., :144]),
                           torch.sigmoid(nchw(om[..., 144:])), 3, 3, 1, 1, 1, 1, 1, 1, G_DCN)
    kperm = torch.tensor([(g * 8 + j) * 9 + t for g in range(G_DCN) for t in range(9) for j in range(8)])
    return c[:, kperm].permute(0, 2, 3, 1)


def onehot_columns():
    w = torch.zeros(C_DCN * 9, C_DCN, 3, 3, dtype=torch.float64)
    for c in range(C_DCN):
        for t in range(9):
            w[c * 9 + t, c, t // 3, t % 3] = 1.0
    return w


# ------------------------------------------------------------------------------------------------- conv geometries new to fp32 backward
# rows in the format of tests/test_conv_wgrad_f32_gpu.py::CASES (name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked): one
# per geometry class of a whole-model fp32 step outside the coders, at the smallest map with borders and a ragged pixel block
CONV_CASES = [
    ("7x7_8_32", 2, 8, 32, 7, 1, 3, 9, 11, False, False, False),                 # SPyNet
    ("7x7_32_64", 1, 32, 64, 7, 1, 3, 9, 11, False, False, False),
    ("7x7_64_32", 1, 64, 32, 7, 1, 3, 9, 11, False, False, False),
    ("7x7_32_16", 1, 32, 16, 7, 1, 3, 9, 11, False, False, False),
    ("7x7_16_2", 2, 16, 2, 7, 1, 3, 9, 11, False, False, False),
    ("3x3_3_64", 2, 3, 64, 3, 1, 1, 9, 11, False, False, False),                  # the Cin = 8 (3 real channels) first layers
    ("3x3_64_64", 2, 64, 64, 3, 1, 1, 9, 11, False, False, False),
    ("3x3_128_64", 2, 128, 64, 3, 1, 1, 9, 11, False, False, False),
    ("3x3_64_216", 2, 64, 216, 3, 1, 1, 9, 11, False, False, False),              # the DCN's offset / mask conv
    ("3x3_s2_64_64", 2, 64, 64, 3, 2, 1, 12, 18, False, False, False),
    ("1x1_128_64", 2, 128, 64, 1, 1, 0, 9, 11, False, False, False),
    ("1x1_256_64", 2, 256, 64, 1, 1, 0, 9, 11, False, False, False),
    ("1x1_576_64", 2, 576, 64, 1, 1, 0, 9, 11, False, False, False),              # the DCN weight over its 576 sampled columns
    ("3x3_64_3", 2, 64, 3, 3, 1, 1, 9, 11, False, False, False),                  # the RGB head (planar fp32 output in the model)
]
# the (3, 1, 1) temporal conv is a 1x1 conv over 3 x 64 channels gathered from a 5-D parameter: its class, run by the GPU test on its own
TEMPORAL_CLASS = (1, 1, 1, 192, 64, False, False, False)


def conv_classes():
    return {(k, k, st, ci, co, sh, sq, mk) for (_, _, ci, co, k, st, _, _, _, sh, sq, mk) in CONV_CASES} | {TEMPORAL_CLASS}


def conv_ref(case):
    """float64 weight / data gradient of a case and the sums of absolute products its bounds use (the existing fp32 test's reference,
    restated here so that the CPU test can check the bounds' sensitivity without importing a GPU test module)"""
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    g = gen("conv", name)
    x, w = draw(g, (N, cin, H, W)), draw(g, (cout, cin, k, k), 1.0 / math.sqrt(cin * k * k))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = draw(g, (N, cout, Ho, Wo), 0.5)
    return x, w, gy, N * Ho * Wo, k * k * cout


def conv_grads64(x, w, gy, stride, pad):
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    gw, gx = torch.autograd.grad(F.conv2d(xr, wr, None, stride=stride, padding=pad), (wr, xr), gy.double())
    return gw, gx
