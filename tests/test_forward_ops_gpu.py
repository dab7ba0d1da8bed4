"""Op-level tests of the forward streaming kernels (csrc/pointwise.hip) against float64 references.

Every launcher here has a case table that reaches each of its dispatch forks and size-gated branches at the smallest size that takes
them (the fp32-map and mixed-dtype forms of add_flow, bcast_add_act, upsample2x and spynet_level_input's cat8, and every form of avgpool_k,
match_gather, channel_sum and cast_f32 / copy_cast live in tests/test_fp32_ops_gpu.py with tables in tests/helpers_fp32_ops.py; the call
classes below carry the dtypes, so the guard here and the fp32 guard there use one definition), plus the edge shapes (odd extents, 1-pixel rows and columns, N > 1) and feature-map views: channel slices (off != 0, pixel
stride > C), batch slices (FM.batch) and frame slices (FM.as_slices: images interleaved inside a pixel).  Output buffers are filled
with a NaN sentinel first; everything outside the view must come back byte-identical.  Inputs are exactly representable in the dtype the kernel reads.

Bounds come from the arithmetic, not from fitting:
  * kernels that are a fixed sequence of correctly rounded fp32 operations (no reduction, no transcendental) are compared bit for
    bit with the same sequence in torch fp32 on the CPU (the library builds with -ffp-contract=off): layouts, scale_act_res,
    add_flow, bcast_add_act, avgpool2, quantize, z_hat;
  * otherwise an fp16 store adds half an ulp (EPS16 |ref| + TINY16), and the fp32 expression adds a few EPS32 of the sum of its
    absolute terms, or of a Lipschitz constant times the fp32 error of a sampling coordinate;
  * the rate terms are checked per 256-element block (the kernel's partial sums), from a per-element bound on the logits / the
    normal CDF propagated through the likelihood and the log; the tensors are regime-homogeneous, so no error hides in a sum.
Where two kernels claim the same arithmetic (scale_act_res16 / scale_act_res, spynet_level_input<true> / <false>) they are compared
bit for bit at a production-size map, which is float64-checked in row bands that include every grid-stride boundary.

`test_production_streaming_classes_have_cases` runs one 1088x1920 inference frame and one 4x256x256 training forward and fails when
a call class (op, dtypes, options, size regime) that production reaches has no row in the tables below.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS16 = 2.0 ** -11
EPS32 = 2.0 ** -24
TINY16 = 2.0 ** -25
SENT16 = 0x7E5A                 # a quiet-NaN payload no kernel writes
SENT32 = 0x7FC0DEAD

# size thresholds of the dispatch (csrc/pointwise.hip)
SAR16_ONE_PASS = 4096 * 256 * 4     # tdvc_scale_act_res: scale_act_res16_kernel<U>'s grid is capped at 4096 blocks of 256 threads, U = 4 items each; beyond: grid-stride passes
FINAL_SUM_ONE = 256                 # final_sum_kernel loops when there are more than 256 partials (256 elements each: tdvc_eb_forward / tdvc_gc_forward)


def _ops():
    from tdvc_amd import ops
    return ops


def _lib():
    from tdvc_amd import _lib as L
    return L.lib()


def _chk(rc, what):
    from tdvc_amd import _lib as L
    L.check(rc, what)


def _ref(fm):
    return C.byref(fm.desc())


# ------------------------------------------------------------------------------------------------------------------ helpers
def buffer(shape, dtype, fill=None, gen=None):
    """a device buffer; fill=None: the sentinel; 'randn' / 'rand' draws (fp16-exact for fp16 buffers)"""
    if fill is None:
        t = torch.empty(shape, dtype=torch.int16 if dtype == torch.float16 else torch.int32, device="cuda")
        t.fill_(SENT16 if dtype == torch.float16 else SENT32)
        return t.view(dtype)
    t = (torch.randn if fill == "randn" else torch.rand)(shape, generator=gen, device="cuda")
    return t.to(dtype)


def view(fm):
    """the NHWC tensor a feature map describes (device, no copy)"""
    t = fm.t
    return torch.as_strided(t, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), t.storage_offset() + fm.off)


def outside_mask(fm):
    m = torch.ones(fm.t.shape, dtype=torch.bool, device=fm.t.device)
    view_of = torch.as_strided(m, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off)
    view_of.fill_(False)
    return m


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def assert_outside_unchanged(before, fm, what):
    m = outside_mask(fm)
    assert torch.equal(bits(before)[m], bits(fm.t)[m]), f"{what}: bytes outside the view changed"


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    eq = bits(got) == bits(want)
    assert bool(eq.all()), f"{what}: {int((~eq).sum())}/{eq.numel()} elements differ bit-wise, first at {tuple(int(i) for i in (~eq).nonzero()[0])}"


def assert_within(got, ref, bound, what, report=None):
    d = (got.double() - ref).abs()
    bad = ~(d <= bound)
    msg = f"{what}: max|d|={float(d.max()):.3e} max(|d|/bound)={float((d / bound).max()):.3f} nbad={int(bad.sum())}/{bad.numel()}"
    if report:
        report(msg)
    assert not bool(bad.any()), msg


def lrelu32(v, act, slope):
    """act_apply (csrc/common.h) in torch fp32"""
    if act == 1:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == 2:
        return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    return v


# ------------------------------------------------------------------------------------------------------------------ call classes
# One function per launcher maps its real arguments to the class the coverage guard compares; every test below asserts that its own
# arguments fall in the class its table row declares, so the tables cannot claim a class they do not run.
def _dt(fm):
    return "f32" if fm.f32 else "f16"


def cls_scale_act_res(a, out, gate=None, act=0, slope=0.0, res=None, res_sign=1.0, out2=None):
    fast = (not a.f32 and not out.f32 and (res is None or not res.f32) and (out2 is None or not out2.f32)
            and (gate is None or gate.data_ptr() % 16 == 0))          # :707-708
    total = a.N * a.H * a.W * ((a.C + 7) // 8)
    passes = ("multi" if total > SAR16_ONE_PASS else "one") if fast else "-"
    dts = (_dt(a), _dt(out), _dt(res) if res is not None else None, _dt(out2) if out2 is not None else None)
    return ("scale_act_res", "f16" if fast else "generic", dts, gate is not None, int(act), None if res is None else float(res_sign), passes)


def se_ways(C_):
    return 1 if 1024 // C_ < 1 else min(32, 1024 // C_)


def cls_se_gate(C_, nblocks):
    # :241 the four-loads loop runs (for the first of `ways` threads per channel) when nblocks > 3 * ways
    return ("se_gate", C_, "loop4" if nblocks > 3 * se_ways(C_) else "tail")


def cls_bcast(T, xdt="f16", bdt="f16"):
    return ("bcast_add_act", "t4" if T == 4 and xdt == bdt == "f16" else "generic", xdt, bdt)        # tdvc_bcast_add_act: fp32 maps take the generic kernel


def cls_eb(numel, noise, zhat_f32):
    return ("eb_forward", noise, "f32" if zhat_f32 else "f16", "multi" if (numel + 255) // 256 > FINAL_SUM_ONE else "single")


def cls_gc(numel, noise):
    return ("gc_forward", noise, "multi" if (numel + 255) // 256 > FINAL_SUM_ONE else "single")


def cls_quantize(y_f32, out_f32, noise):
    return ("quantize", "f32" if y_f32 else "f16", "f32" if out_f32 else "f16", noise)


def cls_spynet(ref, supp, flow_lo, flow_up):
    pix16 = lambda f: f.C >= 4 and f.sp % 4 == 0 and f.sn % 4 == 0 and f.desc().p % 16 == 0
    pix8 = lambda f: f.sp % 2 == 0 and f.sn % 2 == 0 and f.desc().p % 8 == 0
    vec = pix16(ref) and pix16(supp) and pix8(flow_up) and (flow_lo is None or pix8(flow_lo))      # :781-783
    return ("spynet_level_input", "vec" if vec else "scalar", flow_lo is not None)


def cls_resize(x, H, W, chscale):
    return ("resize_bilinear", "down" if H * W < x.H * x.W else "up", chscale is not None)


# ------------------------------------------------------------------------------------------------------------------ layouts
# (N, C, H, W, Cview, Cbuf, c0, dtype): nchw_to_fmap writes channels [c0, c0 + Cview) of a Cbuf-channel buffer (zeros beyond C)
LAYOUT_CASES = [(1, 3, 5, 7, 4, 4, 0, torch.float32), (2, 3, 5, 7, 8, 8, 0, torch.float16), (2, 3, 1, 9, 3, 12, 4, torch.float32),
                (3, 11, 6, 1, 16, 24, 8, torch.float16), (2, 64, 4, 6, 64, 128, 64, torch.float16), (1, 2, 7, 3, 2, 2, 0, torch.float32),
                (2, 3, 4, 5, 8, 16, 8, torch.float16), (1, 3, 5, 7, 8, 8, 0, torch.float32)]
LAYOUT_CLASSES = {("nchw_to_fmap", "f32" if dt == torch.float32 else "f16", C_, Cv) for (_, C_, _, _, Cv, _, _, dt) in LAYOUT_CASES} | \
                 {("fmap_to_nchw", "f32" if dt == torch.float32 else "f16") for (*_, dt) in LAYOUT_CASES}


def cls_from_nchw(Csrc, fm):
    return ("nchw_to_fmap", _dt(fm), Csrc, fm.C)


@pytest.mark.parametrize("N,C_,H,W,Cv,Cbuf,c0,dt", LAYOUT_CASES,
                         ids=[f"{n}x{c}x{h}x{w}_to{cv}_buf{cb}+{c0}_{str(d)[-7:]}" for n, c, h, w, cv, cb, c0, d in LAYOUT_CASES])
def test_layouts(N, C_, H, W, Cv, Cbuf, c0, dt):
    """nchw_to_fmap into a channel view (pad channels zero), fmap_to_nchw back out: bit-exact conversions"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(N, C_, H, W, generator=g, device="cuda")
    buf = buffer((N, H, W, Cbuf), dt)
    fm = ops.FM(buf, c0, N, Cv)
    before = buf.clone()
    assert cls_from_nchw(C_, fm) in LAYOUT_CLASSES
    ops.from_nchw(x, Cpad=Cv, dtype=dt, out=fm)
    torch.cuda.synchronize()
    want = torch.zeros(N, H, W, Cv, dtype=dt)
    want[..., :C_] = x.cpu().permute(0, 2, 3, 1).to(dt)
    assert_bits(view(fm), want, "nchw_to_fmap")
    assert_outside_unchanged(before, fm, "nchw_to_fmap")
    back = fm.to_nchw(C_)
    assert_bits(back, x.cpu().to(dt).float(), "fmap_to_nchw")


# ------------------------------------------------------------------------------------------------------------------ scale_act_res
# (name, N, H, W, C, dtypes, gate, act, res_sign (None: no residual), out2, views, gate_unaligned)
# dtypes: "a[>y[>out2]]", res in a's dtype, y and out2 default to a's ("f32>f32>f16": the analysis transform's last SE scaling, which
# stores the fp32 latent and its fp16 copy: coder.py run_g_a); views: the maps are channel slices of wider buffers (off != 0, sp > C)
SAR_CASES = [
    ("sub", 1, 8, 16, 64, "f16", False, 0, -1.0, False, False, False),         # f_cur - pred (pnet.py:115)
    ("gate", 2, 9, 13, 64, "f16", True, 0, None, False, False, False),          # SE scaling
    ("gate_lrelu", 2, 9, 13, 128, "f16", True, 2, None, False, False, False),
    ("gate_res", 2, 5, 7, 64, "f16", True, 0, 1.0, False, True, False),
    ("gate_lrelu_res", 1, 7, 9, 64, "f16", True, 2, 1.0, False, False, False),
    ("gate_lrelu_res_out2", 2, 3, 5, 64, "f16", True, 2, 1.0, True, True, False),
    ("gate_out2", 1, 4, 4, 64, "f16", True, 0, None, True, False, False),
    ("lrelu_res", 2, 5, 3, 64, "f16", False, 2, 1.0, False, True, False),
    ("relu", 1, 1, 11, 64, "f16", False, 1, None, False, False, False),
    ("res_plus", 1, 6, 1, 64, "f16", False, 0, 1.0, False, False, False),       # identity adds under the tape
    ("res_minus_out2", 1, 5, 5, 64, "f16", False, 0, -1.0, True, False, False),
    ("generic_unaligned_gate", 2, 9, 13, 64, "f16", True, 2, 1.0, True, True, True),
    ("generic_unaligned_gate_plain", 1, 7, 5, 64, "f16", True, 0, None, False, False, True),
    ("generic_f32", 2, 5, 7, 12, "f32", True, 2, -1.0, True, True, False),      # C not a multiple of 8: the masked tail chunk
    ("generic_f32_res", 1, 3, 9, 64, "f32", False, 0, 1.0, False, False, False),
    ("generic_f32_res_minus", 1, 3, 9, 64, "f32", False, 0, -1.0, False, False, False),
    ("generic_f32_gate", 1, 3, 9, 64, "f32", True, 0, None, False, False, False),
    ("generic_f32_gate_lrelu", 1, 3, 9, 64, "f32", True, 2, None, False, False, False),
    ("generic_f32_gate_res", 2, 3, 5, 64, "f32", True, 0, 1.0, False, True, False),     # the SE scaling plus identity of the fp32 mode's residual blocks
    ("generic_g_a_latent", 1, 5, 7, 128, "f32>f32>f16", True, 0, None, True, False, False),
    ("generic_g_a_latent_views", 2, 3, 4, 128, "f32>f32>f16", True, 0, None, True, True, False),
    ("generic_f16_in_f32_out", 2, 3, 4, 128, "f16>f32", True, 2, 1.0, True, True, False),
]
# at 1088 x 1920 x 64: 16.7 M 8-channel items, four grid-stride passes of the fp16 kernel (compared with the generic kernel)
SAR_BIG = [("big_sub", False, 0, -1.0, False), ("big_gate", True, 0, None, False), ("big_gate_lrelu_res", True, 2, 1.0, False),
           ("big_gate_lrelu", True, 2, None, False), ("big_gate_res_out2", True, 0, 1.0, True), ("big_gate_lrelu_res_out2", True, 2, 1.0, True),
           ("big_res_plus", False, 0, 1.0, False), ("big_gate_res", True, 0, 1.0, False)]
BIG_H, BIG_W = 1088, 1920


def _sar_dtypes(dt):
    """"a[>y[>out2]]" -> (a, y, out2); the residual comes in a's dtype"""
    p = dt.split(">")
    return p[0], p[1] if len(p) > 1 else p[0], p[2] if len(p) > 2 else p[0]


def _sar_row_class(N, H, W, C_, dt, gate, act, rs, out2, unaligned):
    adt, ydt, y2dt = _sar_dtypes(dt)
    fast = adt == ydt == y2dt == "f16" and not unaligned
    total = N * H * W * ((C_ + 7) // 8)
    dts = (adt, ydt, adt if rs is not None else None, y2dt if out2 else None)
    return ("scale_act_res", "f16" if fast else "generic", dts, gate, act, rs, ("multi" if total > SAR16_ONE_PASS else "one") if fast else "-")


SAR_CLASSES = {_sar_row_class(N, H, W, C_, dt, ga, act, rs, o2, un) for (_, N, H, W, C_, dt, ga, act, rs, o2, _, un) in SAR_CASES} | \
              {_sar_row_class(1, BIG_H, BIG_W, 64, "f16", ga, act, rs, o2, False) for (_, ga, act, rs, o2) in SAR_BIG}


def _sar_inputs(N, H, W, C_, dt, gate, rs, views, unaligned, seed):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(seed)
    tdt = torch.float16 if _sar_dtypes(dt)[0] == "f16" else torch.float32
    Cb = 2 * C_ + 8 if views else C_
    c0 = C_ + 8 if views else 0
    a = ops.FM(buffer((N, H, W, Cb), tdt, "randn", g), c0, N, C_)
    r = ops.FM(buffer((N, H, W, Cb), tdt, "randn", g), 0, N, C_) if rs is not None else None
    gt = None
    if gate:
        gbuf = torch.rand(N * C_ + 4, generator=g, device="cuda") * 1.5
        gt = gbuf[1:1 + N * C_].view(N, C_) if unaligned else gbuf[:N * C_].view(N, C_)
    return a, r, gt, Cb, c0


def _sar_want32(a, gate, act, slope, r, rs):
    """the kernel's sequence in torch fp32 on the CPU: ((a * gate) -> act) + rs * r"""
    v = view(a).cpu().float()
    if gate is not None:
        v = v * gate.cpu()[:, None, None, :]
    v = lrelu32(v, act, slope)
    if r is not None:
        v = v + torch.tensor(rs, dtype=torch.float32) * view(r).cpu().float()
    return v


def _sar_ref64(a, gate, act, slope, r, rs):
    v = view(a).cpu().double()
    if gate is not None:
        v = v * gate.cpu().double()[:, None, None, :]
    if act == 1:
        v = v.clamp_min(0)
    elif act == 2:
        v = torch.where(v > 0, v, v * float(torch.tensor(slope, dtype=torch.float32)))
    if r is not None:
        v = v + rs * view(r).cpu().double()
    return v


def _sar_bound(a, gate, r, ref64, f16):
    """three fp32 roundings (product, slope, sum) of at most |a g| + |r|, plus the store"""
    s = view(a).cpu().double().abs()
    if gate is not None:
        s = s * gate.cpu().double()[:, None, None, :]
    if r is not None:
        s = s + view(r).cpu().double().abs()
    return 3 * EPS32 * s + ((EPS16 * ref64.abs() + TINY16) if f16 else 0.0)


@pytest.mark.parametrize("row", SAR_CASES, ids=[r[0] for r in SAR_CASES])
def test_scale_act_res(row, report):
    ops = _ops()
    name, N, H, W, C_, dt, gate, act, rs, o2, views, unaligned = row
    a, r, gt, Cb, c0 = _sar_inputs(N, H, W, C_, dt, gate, rs, views, unaligned, seed=len(name))
    T = {"f16": torch.float16, "f32": torch.float32}
    _, ydt, y2dt = (T[d] for d in _sar_dtypes(dt))
    ybuf, y2buf = buffer((N, H, W, Cb), ydt), buffer((N, H, W, Cb), y2dt)
    y = ops.FM(ybuf, 0, N, C_)
    y2 = ops.FM(y2buf, c0, N, C_) if o2 else None
    yb, y2b = ybuf.clone(), y2buf.clone()
    slope = 0.1
    assert cls_scale_act_res(a, y, gt, act, slope, r, 1.0 if rs is None else rs, y2) == \
        _sar_row_class(N, H, W, C_, dt, gate, act, rs, o2, unaligned)
    ops.scale_act_res(a, y, gate=gt, act=act, slope=slope, res=r, res_sign=1.0 if rs is None else rs, out2=y2)
    torch.cuda.synchronize()
    want32 = _sar_want32(a, gt, act, slope, r, rs)
    assert_bits(view(y), want32.to(ydt), f"scale_act_res {name}")
    ref = _sar_ref64(a, gt, act, slope, r, rs)
    assert_within(view(y).cpu(), ref, _sar_bound(a, gt, r, ref, ydt == torch.float16), f"scale_act_res {name} vs float64", report)
    assert_outside_unchanged(yb, y, f"scale_act_res {name} y")
    if o2:
        assert_bits(view(y2), want32.to(y2dt), f"scale_act_res {name} out2")
        assert_outside_unchanged(y2b, y2, f"scale_act_res {name} out2")
    else:
        assert torch.equal(bits(y2buf), bits(y2b))


def _big_bands():
    """rows around every grid-stride boundary of the fp16 kernel (item u*T + pass*U*T, T = 4096*256 items of 8 channels), first and last rows"""
    T = 4096 * 256
    total = BIG_H * BIG_W * 8
    rows = {0, BIG_H - 1}
    for k in range(total // T + 1):
        p = (k * T) // 8
        r0 = p // BIG_W
        rows |= {max(0, r0 - 1), min(BIG_H - 1, r0), min(BIG_H - 1, r0 + 1)}
    return sorted(rows)


@pytest.mark.parametrize("row", SAR_BIG, ids=[r[0] for r in SAR_BIG])
def test_scale_act_res_production_size(row, report):
    """1 x 1088 x 1920 x 64: the fp16 grid-stride kernel (four passes) against the generic kernel (a gate view one float off 16-byte
    alignment; ones for the rows without a gate) bit for bit everywhere, and against float64 in row bands over every pass boundary"""
    ops = _ops()
    name, gate, act, rs, o2 = row
    N, H, W, C_ = 1, BIG_H, BIG_W, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    a = ops.FM(buffer((N, H, W, C_), torch.float16, "randn", g))
    r = ops.FM(buffer((N, H, W, C_), torch.float16, "randn", g)) if rs is not None else None
    g_al = (torch.rand(N, C_, generator=g, device="cuda") * 1.5) if gate else torch.ones(N, C_, device="cuda")
    gbuf = torch.zeros(N * C_ + 4, device="cuda")
    gbuf[1:1 + N * C_] = g_al.view(-1)
    g_un = gbuf[1:1 + N * C_].view(N, C_)                    # the same gate one float off 16-byte alignment
    y, yg = ops.FM(buffer((N, H, W, C_), torch.float16)), ops.FM(buffer((N, H, W, C_), torch.float16))
    y2 = ops.FM(buffer((N, H, W, C_), torch.float16)) if o2 else None
    y2g = ops.FM(buffer((N, H, W, C_), torch.float16)) if o2 else None
    rsv = 1.0 if rs is None else rs
    assert cls_scale_act_res(a, y, g_al if gate else None, act, 0.1, r, rsv, y2) == _sar_row_class(N, H, W, C_, "f16", gate, act, rs, o2, False)
    assert cls_scale_act_res(a, yg, g_un, act, 0.1, r, rsv, y2g)[1] == "generic"
    ops.scale_act_res(a, y, gate=g_al if gate else None, act=act, slope=0.1, res=r, res_sign=rsv, out2=y2)
    ops.scale_act_res(a, yg, gate=g_un, act=act, slope=0.1, res=r, res_sign=rsv, out2=y2g)
    torch.cuda.synchronize()
    diff = int((bits(y.t) != bits(yg.t)).sum())
    assert diff == 0, f"scale_act_res {name}: fp16 kernel and generic kernel differ in {diff} elements"
    if o2:
        assert torch.equal(bits(y2.t), bits(y.t)) and torch.equal(bits(y2g.t), bits(y.t))
    rows = torch.tensor(_big_bands())
    sub = lambda fm: ops.FM(fm.t[:, rows.cuda()].contiguous()) if fm is not None else None
    ab, rb = sub(a), sub(r)
    ref = _sar_ref64(ab, g_al if gate else None, act, 0.1, rb, rsv if rs is not None else None)
    got = y.t[:, rows.cuda()].cpu()
    assert_within(got, ref, _sar_bound(ab, g_al if gate else None, rb, ref, True), f"scale_act_res {name} bands ({len(rows)} rows) vs float64", report)


# ------------------------------------------------------------------------------------------------------------------ se_gate
# (C, nblocks): one partial, the serial tail only, the smallest count that enters the four-loads loop (3 ways + 1), a count with a
# ragged tail after the loop, production-like counts of the conv epilogue's channel sums
SE_CASES = [(64, 1), (64, 6), (64, 48), (64, 49), (64, 67), (64, 272), (128, 6), (128, 24), (128, 25), (128, 31), (128, 1020)]
SE_CLASSES = {cls_se_gate(c, nb) for c, nb in SE_CASES}


@pytest.mark.parametrize("C_,nblocks", SE_CASES, ids=[f"C{c}_nb{nb}" for c, nb in SE_CASES])
def test_se_gate(C_, nblocks, report):
    """gate = sigmoid(W2 relu(W1 mean + b1) + b2), mean = (sum of the partials) / npix: tdvc_se_gate on given partials"""
    N, Cmid, npix = 2, C_ // 16, 1000 * nblocks
    g = torch.Generator().manual_seed(C_ + nblocks)
    # per-block channel sums with a per-channel mean of O(1) per pixel; every partial matters (no cancellation to zero)
    partial = (torch.rand(N, nblocks, C_, generator=g) + 0.2) * 1000.0 * (torch.rand(1, 1, C_, generator=g) * 2 - 0.5)
    w1, b1 = torch.randn(Cmid, C_, generator=g) * C_ ** -0.5 * 2, torch.randn(Cmid, generator=g) * 0.3
    w2, b2 = torch.randn(C_, Cmid, generator=g) * Cmid ** -0.5, torch.randn(C_, generator=g) * 0.3
    d = [t.cuda().contiguous() for t in (partial, w1, b1, w2, b2)]
    gate = torch.empty(N, C_, device="cuda")
    inv = 1.0 / npix
    _chk(_lib().tdvc_se_gate(d[0].data_ptr(), nblocks, inv, N, C_, Cmid, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                             gate.data_ptr(), _ops()._stream()), "se_gate")
    P, W1, B1, W2, B2 = (t.double() for t in (partial, w1, b1, w2, b2))
    inv32 = float(torch.tensor(inv, dtype=torch.float32))
    mean = P.sum(1) * inv32
    pre = mean @ W1.t() + B1
    mid = pre.clamp_min(0)
    s = mid @ W2.t() + B2
    ref = torch.sigmoid(s)
    # fp32 error chain: the fixed-order sum of nblocks partials (<= nblocks + ways roundings), the scaling, two dot products
    e_mean = (nblocks + se_ways(C_) + 1) * EPS32 * P.abs().sum(1) * inv32
    e_mid = e_mean @ W1.abs().t() + (C_ + 1) * EPS32 * ((mean.abs() @ W1.abs().t()) + B1.abs())
    e_s = e_mid @ W2.abs().t() + (Cmid + 1) * EPS32 * ((mid @ W2.abs().t()) + B2.abs())
    bound = ref * (1 - ref) * e_s + 6 * EPS32 * ref
    assert_within(gate.cpu(), ref, bound, f"se_gate C{C_} nblocks {nblocks}", report)


# ------------------------------------------------------------------------------------------------------------------ bcast_add_act
# (N, H, W, Cb, T, wide): x has T slices of Cb channels; wide = x is a channel view (64 more channels in the buffer); batch and
# frame-slice views: test_batch_and_frame_views
BC_CASES = [(2, 8, 16, 64, 4, False), (1, 5, 7, 64, 4, True), (2, 3, 5, 64, 3, False), (1, 1, 9, 64, 2, True), (1, 4, 4, 8, 4, False)]
BC_CLASSES = {cls_bcast(T) for *_, T, _ in BC_CASES}            # fp16 maps; the fp32 and mixed rows: tests/helpers_fp32_ops.py


@pytest.mark.parametrize("N,H,W,Cb,T,wide", BC_CASES, ids=[f"{n}x{h}x{w}_T{t}x{c}{'_view' if v else ''}" for n, h, w, c, t, v in BC_CASES])
def test_bcast_add_act(N, H, W, Cb, T, wide):
    """x[..., t*Cb:(t+1)*Cb] = lrelu(x + b, 0.1) for every slice t; `wide`: x is a channel view of a buffer with 64 more channels"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(T * 10 + H)
    Cx = T * Cb
    xbuf = buffer((N, H, W, Cx + (64 if wide else 0)), torch.float16, "randn", g)
    x = ops.FM(xbuf, 64 if wide else 0, N, Cx)
    b = ops.FM(buffer((N, H, W, Cb), torch.float16, "randn", g))
    before = xbuf.clone()
    x0 = view(x).cpu().float()
    ops.bcast_add_act(x, b, T, 0.1)
    torch.cuda.synchronize()
    want = lrelu32(x0 + view(b).cpu().float().repeat(1, 1, 1, T), 2, 0.1).half()
    assert_bits(view(x), want, f"bcast_add_act T={T}")
    assert_outside_unchanged(before, x, "bcast_add_act")


# ------------------------------------------------------------------------------------------------------------------ upsample2x
# (N, h, w, C, in view, out view)
UP_CASES = [(2, 9, 15, 64, False, False), (1, 1, 7, 64, False, False), (1, 6, 1, 8, True, False), (3, 1, 1, 16, False, True),
            (2, 5, 4, 64, True, True)]
UP_CLASSES = {("upsample2x", "view" if (vin or vout) else "dense", "f16", "f16") for (*_, vin, vout) in UP_CASES}


def _dense(fm):
    return fm.off == 0 and fm.sp == fm.C and fm.sn == fm.H * fm.W * fm.C


def cls_upsample(x, out):
    return ("upsample2x", "dense" if _dense(x) and (out is None or _dense(out)) else "view", _dt(x), _dt(x if out is None else out))


@pytest.mark.parametrize("N,h,w,C_,vin,vout", UP_CASES, ids=[f"{n}x{h}x{w}x{c}{'_vin' if a else ''}{'_vout' if b else ''}" for n, h, w, c, a, b in UP_CASES])
def test_upsample2x(N, h, w, C_, vin, vout, report):
    """bilinear x2, align_corners=False (F.interpolate in float64); 1-pixel rows / columns reach the y1 / x1 clamps"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(h * 31 + w)
    x = ops.FM(buffer((N, h, w, C_ + (16 if vin else 0)), torch.float16, "randn", g), 16 if vin else 0, N, C_)
    ybuf = buffer((N, 2 * h, 2 * w, C_ + (8 if vout else 0)), torch.float16)
    y = ops.FM(ybuf, 8 if vout else 0, N, C_)
    before = ybuf.clone()
    assert cls_upsample(x, y) == ("upsample2x", "view" if (vin or vout) else "dense", "f16", "f16")
    ops.upsample2x(x, out=y)
    torch.cuda.synchronize()
    xc = view(x).cpu().double().permute(0, 3, 1, 2)
    ref = F.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    absr = F.interpolate(xc.abs(), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    # weights are exact (multiples of 1/4 and their complements); 6 roundings of products and sums of |terms| <= absr
    bound = 6 * EPS32 * absr + EPS16 * ref.abs() + TINY16
    assert_within(view(y).cpu(), ref, bound, f"upsample2x {N}x{h}x{w}x{C_}", report)
    assert_outside_unchanged(before, y, "upsample2x")


# ------------------------------------------------------------------------------------------------------------------ avgpool2
# (N, H, W, C of x, C of y, x buffer channels): odd extents (floor pooling), 2- and 3-pixel extents (one output row / column),
# y.C < x.C, a y view inside a wider buffer
AP_CASES = [(2, 32, 64, 3, 3, 4), (1, 7, 9, 3, 3, 4), (3, 2, 5, 4, 4, 4), (1, 3, 2, 4, 2, 4), (2, 11, 3, 2, 2, 6)]
# the class is that of the op-level entry ops.avgpool2 (y.C = x.C, fresh y): (x.C, x's pixel stride), for the rows that run it
AP_CLASSES = {("avgpool2", cx, cb) for (_, _, _, cx, cy, cb) in AP_CASES if cx == cy}


@pytest.mark.parametrize("N,H,W,Cx,Cy,Cb", AP_CASES, ids=[f"{n}x{h}x{w}_c{cx}to{cy}_buf{cb}" for n, h, w, cx, cy, cb in AP_CASES])
def test_avgpool2(N, H, W, Cx, Cy, Cb):
    """(a + b + c + d) * 0.25 in that order, fp32: bit-exact with torch fp32; y is a view of a wider sentinel buffer"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(H * W)
    x = ops.FM(buffer((N, H, W, Cb), torch.float32, "randn", g), 0, N, Cx)
    ybuf = buffer((N, H // 2, W // 2, Cy + 3), torch.float32)
    y = ops.FM(ybuf, 1, N, Cy)
    before = ybuf.clone()
    _chk(_lib().tdvc_avgpool2(_ref(x), _ref(y), ops._stream()), "avgpool2")
    torch.cuda.synchronize()
    xv = view(x).cpu()[:, :H // 2 * 2, :W // 2 * 2, :Cy]
    want = (((xv[:, 0::2, 0::2] + xv[:, 0::2, 1::2]) + xv[:, 1::2, 0::2]) + xv[:, 1::2, 1::2]) * 0.25
    assert_bits(view(y), want, f"avgpool2 {N}x{H}x{W}")
    ref = F.avg_pool2d(view(x).cpu().double().permute(0, 3, 1, 2)[:, :Cy], 2, 2).permute(0, 2, 3, 1)
    assert_within(view(y).cpu(), ref, 3 * EPS32 * F.avg_pool2d(view(x).cpu().double().abs().permute(0, 3, 1, 2)[:, :Cy], 2, 2).permute(0, 2, 3, 1),
                  "avgpool2 vs float64")
    assert_outside_unchanged(before, y, "avgpool2")
    if Cx == Cy:                           # the op-level entry (fresh output) as production calls it
        assert_bits(view(ops.avgpool2(x)), want, "ops.avgpool2")


# ------------------------------------------------------------------------------------------------------------------ resize_bilinear
# (N, h, w, H, W, C, Cbuf, chscale): down (the flow's way back), up (to the x32-padded size), 1-pixel source rows / columns, y.C < x.C
RS_CASES = [(1, 30, 50, 32, 64, 3, 4, False), (2, 64, 96, 57, 90, 2, 2, True), (1, 1, 7, 4, 9, 2, 2, True), (2, 5, 1, 3, 6, 3, 4, False),
            (1, 9, 11, 9, 11, 2, 4, False)]
RS_CLASSES = {("resize_bilinear", "down" if H * W < h * w else "up", cs) for (_, h, w, H, W, _, _, cs) in RS_CASES}


@pytest.mark.parametrize("N,h,w,H,W,C_,Cb,cs", RS_CASES, ids=[f"{n}x{h}x{w}to{H}x{W}_c{c}{'_sc' if s else ''}" for n, h, w, H, W, c, _, s in RS_CASES])
def test_resize_bilinear(N, h, w, H, W, C_, Cb, cs, report):
    """F.interpolate(size=, bilinear, align_corners=False) in float64, times the per-channel scale"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(h + 100 * W)
    x = ops.FM(buffer((N, h, w, Cb), torch.float32, "randn", g))
    sc = (torch.rand(Cb, generator=g, device="cuda") + 0.5) if cs else None
    assert cls_resize(x, H, W, sc) in RS_CLASSES
    ybuf = buffer((N, H, W, C_ + 2), torch.float32)
    y = ops.FM(ybuf, 2, N, C_)
    before = ybuf.clone()
    _chk(_lib().tdvc_resize_bilinear(_ref(x), _ref(y), sc.data_ptr() if cs else None, ops._stream()), "resize_bilinear")
    torch.cuda.synchronize()
    xc = view(x).cpu().double().permute(0, 3, 1, 2)[:, :C_]
    ref = F.interpolate(xc, size=(H, W), mode="bilinear", align_corners=False)
    absr = F.interpolate(xc.abs(), size=(H, W), mode="bilinear", align_corners=False)
    # the source coordinate in fp32 (ratio, +0.5, *, -0.5: 4 roundings of at most max(h, w)) moves the sample by L * dx, L the
    # largest difference between neighbours; 6 roundings of the weighted sum; the scale multiply
    L_ = max(float((xc[..., 1:, :] - xc[..., :-1, :]).abs().max()) if h > 1 else 0.0, float((xc[..., 1:] - xc[..., :-1]).abs().max()) if w > 1 else 0.0)
    bound = 4 * EPS32 * max(h, w) * L_ * 2 + 7 * EPS32 * absr
    if cs:
        s = sc[:C_].cpu().double().view(1, C_, 1, 1)
        ref, bound = ref * s, bound * s + EPS32 * (ref * s).abs()
    assert_within(view(y).cpu(), ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1), f"resize {h}x{w}->{H}x{W}", report)
    assert_outside_unchanged(before, y, "resize_bilinear")


# ------------------------------------------------------------------------------------------------------------------ add_flow
# (N, H, W, C of off, off buffer channels, flow buffer channels)
AF_CASES = [(1, 16, 24, 64, 64, 2), (2, 5, 7, 64, 128, 4), (1, 1, 9, 8, 16, 2)]
AF_CLASSES = {("add_flow", "dense" if Cb == C_ else "view", Cf, "f16") for (_, _, _, C_, Cb, Cf) in AF_CASES}


def cls_add_flow(off, flow):
    return ("add_flow", "dense" if _dense(off) else "view", flow.sp, _dt(off))


@pytest.mark.parametrize("N,H,W,C_,Cb,Cf", AF_CASES, ids=[f"{n}x{h}x{w}x{c}_buf{cb}_flow{cf}" for n, h, w, c, cb, cf in AF_CASES])
def test_add_flow(N, H, W, C_, Cb, Cf):
    """off[..., 2k] += flow_x, off[..., 2k+1] += flow_y (fp32 add, fp16 store): bit-exact"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(H + Cb)
    obuf = buffer((N, H, W, Cb), torch.float16, "randn", g)
    off = ops.FM(obuf, Cb - C_, N, C_)
    flow = ops.FM(buffer((N, H, W, Cf), torch.float32, "randn", g) * 4, 0, N, 2)
    before, o0 = obuf.clone(), view(off).cpu().float()
    assert cls_add_flow(off, flow) == ("add_flow", "dense" if Cb == C_ else "view", Cf, "f16")
    ops.add_flow(off, flow)
    torch.cuda.synchronize()
    want = (o0 + view(flow).cpu().repeat(1, 1, 1, C_ // 2)).half()
    assert_bits(view(off), want, "add_flow")
    assert_outside_unchanged(before, off, "add_flow")


# ------------------------------------------------------------------------------------------------------------------ spynet level input
def _level_ref64(ref, supp, flow_lo, H, W, rows=None):
    """float64: flow_up = 2 * interpolate(flow_lo, x2, align_corners=True); warped = grid_sample(supp, border, align_corners=True)
    -> (cat8 [N, h, W, 8], flow_up [N, h, W, 2]) for the given output rows (all when None)"""
    N = ref.shape[0]
    rows = torch.arange(H) if rows is None else rows
    if flow_lo is not None:
        up = F.interpolate(flow_lo.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1) * 2.0
        up = up[:, rows]
    else:
        up = torch.zeros(N, len(rows), W, 2, dtype=torch.float64)
    gx = torch.arange(W, dtype=torch.float64).view(1, 1, W) + up[..., 0]
    gy = rows.double().view(1, -1, 1) + up[..., 1]
    grid = torch.stack([2 * gx / max(W - 1, 1) - 1, 2 * gy / max(H - 1, 1) - 1], -1)
    warped = F.grid_sample(supp.double()[..., :3].permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="border",
                           align_corners=True).permute(0, 2, 3, 1)
    cat = torch.cat([ref.double()[:, rows, :, :3], warped, up], -1)
    return cat, up


def _level_bound(cat, up, supp, H, W, flow_lo):
    """fp16 store of cat8; flow_up: 4-term bilinear in fp32 (~5 EPS32 of max|flow_lo| * 2); the warp: the sampling coordinate
    through the normalise / unnormalise round trip (~8 EPS32 of max(W, |g|)) times the largest neighbour difference of supp,
    plus the fp32 four-term sum"""
    fl = float(flow_lo.abs().max()) if flow_lo is not None else 0.0
    # flow_up: the source coordinate ry * y (two roundings of at most max(h2, w2)) times the largest neighbour difference of
    # flow_lo, and 6 roundings of the four-term bilinear sum; all times 2
    Lf, n2 = 0.0, 1
    if flow_lo is not None:
        f_ = flow_lo.double()
        n2 = max(f_.shape[1], f_.shape[2])
        Lf = max(float((f_[:, 1:] - f_[:, :-1]).abs().max()) if f_.shape[1] > 1 else 0.0,
                 float((f_[:, :, 1:] - f_[:, :, :-1]).abs().max()) if f_.shape[2] > 1 else 0.0)
    e_up = 2 * (6 * EPS32 * fl + 2 * 2 * EPS32 * n2 * Lf)
    s3 = supp.double()[..., :3]
    Lx = float((s3[:, :, 1:] - s3[:, :, :-1]).abs().max()) if W > 1 else 0.0
    Ly = float((s3[:, 1:] - s3[:, :-1]).abs().max()) if H > 1 else 0.0
    gmax = max(W, H) + 2 * fl + 1
    e_warp = (10 * EPS32 * gmax + e_up) * (Lx + Ly) + 8 * EPS32 * float(s3.abs().max())
    b = torch.empty_like(cat)
    b[..., :3] = 0.0
    b[..., 3:6] = e_warp
    b[..., 6:] = e_up
    return b + EPS16 * cat.abs() + TINY16, e_up + EPS32 * up.abs()


# (N, H, W, with flow_lo, ref / supp channels): 4 -> the vector kernel, 3 -> the scalar one; H = 1 / W = 1 columns; an odd N
SP_CASES = [(2, 34, 60, True, 4), (2, 34, 60, True, 3), (2, 34, 60, False, 4), (1, 16, 24, False, 3), (3, 2, 8, True, 3),
            (1, 8, 2, True, 4), (1, 2, 2, True, 3)]
SP_CLASSES = {("spynet_level_input", "vec" if c == 4 else "scalar", fl) for (_, _, _, fl, c) in SP_CASES}


def _level_inputs(N, H, W, with_flow, Cs, g, scale=4.0):
    ops = _ops()
    ref = torch.rand(N, H, W, 4, generator=g, device="cuda")
    supp = torch.rand(N, H, W, 4, generator=g, device="cuda")
    flo = torch.randn(N, H // 2, W // 2, 2, generator=g, device="cuda") * scale if with_flow else None
    fm = lambda t: ops.FM(t[..., :Cs].contiguous()) if Cs < 4 else ops.FM(t)
    return ref, supp, flo, fm(ref), fm(supp), (ops.FM(flo) if with_flow else None)


@pytest.mark.parametrize("N,H,W,fl,Cs", SP_CASES, ids=[f"{n}x{h}x{w}{'_flow' if f else ''}_C{c}" for n, h, w, f, c in SP_CASES])
def test_spynet_level_input(N, H, W, fl, Cs, report):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(H * W + Cs)
    ref, supp, flo, rf, sf, ff = _level_inputs(N, H, W, fl, Cs, g)
    upbuf, catbuf = buffer((N, H, W, 4), torch.float32), buffer((N, H, W, 16), torch.float16)
    up, cat8 = ops.FM(upbuf, 2, N, 2), ops.FM(catbuf, 8, N, 8)
    ub, cb = upbuf.clone(), catbuf.clone()
    want_cls = ("spynet_level_input", "vec" if Cs == 4 else "scalar", fl)
    # the flow_up view is 8-byte aligned (off 2 floats): only the ref / supp pixels decide the kernel here
    assert cls_spynet(rf, sf, ff, up) == want_cls
    ops.spynet_level_input(rf, sf, ff, up, cat8)
    torch.cuda.synchronize()
    cat_r, up_r = _level_ref64(ref.cpu(), supp.cpu(), flo.cpu() if fl else None, H, W)
    bc, bu = _level_bound(cat_r, up_r, supp.cpu(), H, W, flo.cpu() if fl else None)
    assert_within(view(up).cpu(), up_r, bu, f"flow_up {N}x{H}x{W} C{Cs}", report)
    assert_within(view(cat8).cpu(), cat_r, bc, f"cat8 {N}x{H}x{W} C{Cs}", report)
    assert_outside_unchanged(ub, up, "flow_up")
    assert_outside_unchanged(cb, cat8, "cat8")


# the finest SPyNet level of a 1088 x 1920 frame, with and without flow
SP_BIG = [True, False]


@pytest.mark.parametrize("fl", SP_BIG, ids=["flow", "noflow"])
def test_spynet_level_input_production_size(fl, report):
    """<true> (4-float pixels) against <false> (3-float pixels) bit for bit at 1088 x 1920; float64 on row bands"""
    ops = _ops()
    N, H, W = 1, BIG_H, BIG_W
    g = torch.Generator(device="cuda").manual_seed(11)
    ref, supp, flo, rf4, sf4, ff = _level_inputs(N, H, W, fl, 4, g, scale=6.0)
    rf3, sf3 = ops.FM(ref[..., :3].contiguous()), ops.FM(supp[..., :3].contiguous())
    outs = []
    for rf, sf in ((rf4, sf4), (rf3, sf3)):
        up, cat8 = ops.FM(buffer((N, H, W, 2), torch.float32)), ops.FM(buffer((N, H, W, 8), torch.float16))
        outs.append((cls_spynet(rf, sf, ff, up)[1], up, cat8))
        ops.spynet_level_input(rf, sf, ff, up, cat8)
    torch.cuda.synchronize()
    assert [o[0] for o in outs] == ["vec", "scalar"]
    for k in (1, 2):
        nd = int((bits(outs[0][k].t) != bits(outs[1][k].t)).sum())
        assert nd == 0, f"spynet_level_input <true> / <false> differ in {nd} elements of {'flow_up' if k == 1 else 'cat8'}"
    rows = torch.tensor([0, 1, 2, H // 2 - 1, H // 2, H - 2, H - 1])
    cat_r, up_r = _level_ref64(ref.cpu(), supp.cpu(), flo.cpu() if fl else None, H, W, rows)
    bc, bu = _level_bound(cat_r, up_r, supp.cpu(), H, W, flo.cpu() if fl else None)
    assert_within(outs[0][1].t[:, rows.cuda()].cpu(), up_r, bu, "flow_up bands 1088x1920", report)
    assert_within(outs[0][2].t[:, rows.cuda()].cpu(), cat_r, bc, "cat8 bands 1088x1920", report)


# ------------------------------------------------------------------------------------------------------------------ quantize
# (N, H, W, C, y dtype, out dtype, noise, out buffer channels)
Q_CASES = [(2, 9, 15, 128, "f32", "f16", False, 128), (2, 9, 15, 128, "f32", "f32", False, 136), (1, 4, 5, 128, "f32", "f16", True, 128),
           (1, 4, 5, 128, "f32", "f32", True, 128), (1, 3, 7, 12, "f32", "f32", False, 16), (2, 1, 3, 16, "f16", "f16", True, 24),
           (1, 2, 2, 8, "f16", "f32", False, 8)]
Q_CLASSES = {cls_quantize(y == "f32", o == "f32", nz) for (_, _, _, _, y, o, nz, _) in Q_CASES}


@pytest.mark.parametrize("N,H,W,C_,ydt,odt,nz,Cb", Q_CASES, ids=[f"{n}x{h}x{w}x{c}_{y}to{o}{'_noise' if z else ''}" for n, h, w, c, y, o, z, _ in Q_CASES])
def test_quantize(N, H, W, C_, ydt, odt, nz, Cb):
    """rint (half to even, exact .5 ties included) or y + noise, in fp32; stored to fp16 / fp32 views: bit-exact"""
    ops = _ops()
    T = {"f16": torch.float16, "f32": torch.float32}
    g = torch.Generator(device="cuda").manual_seed(C_ + H)
    yv = torch.randn(N, H, W, C_, generator=g, device="cuda") * 6
    yv.view(-1)[::3] = torch.round(yv.view(-1)[::3]) + 0.5          # exact ties, both parities
    yv.view(-1)[1::7] = -torch.round(yv.view(-1)[1::7]) - 0.5
    y = ops.FM(yv.to(T[ydt]))
    noise = ops.FM(torch.rand(N, H, W, C_, generator=g, device="cuda").to(T[ydt]) - 0.5) if nz else None
    obuf = buffer((N, H, W, Cb), T[odt])
    out = ops.FM(obuf, Cb - C_, N, C_)
    before = obuf.clone()
    ops.quantize(y, out, noise=noise)
    torch.cuda.synchronize()
    y32 = view(y).cpu().float()
    want = (y32 + view(noise).cpu().float()) if nz else torch.round(y32)
    assert_bits(view(out), want.to(T[odt]), "quantize")
    assert_outside_unchanged(before, out, "quantize")


# ------------------------------------------------------------------------------------------------------------------ rate terms
def eb_params(C_, seed):
    """packed [C][59] table (tdvc_amd.model.coder.EntropyBottleneck._packed_tensor layout) with an overall slope of ~0.3 per unit:
    likelihoods from ~1 at the median to the floor within +-200"""
    g = torch.Generator().manual_seed(seed)
    m0 = F.softplus(torch.randn(C_, 3, generator=g) * 0.3) * 0.4
    mk = [F.softplus(torch.randn(C_, 9, generator=g) * 0.3) * 0.45 for _ in range(3)]
    m4 = F.softplus(torch.randn(C_, 3, generator=g) * 0.3) * 0.45
    b = torch.randn(C_, 13, generator=g) * 0.5
    f = torch.tanh(torch.randn(C_, 12, generator=g) * 0.5)
    med = torch.randn(C_, 1, generator=g) * 0.4
    return torch.cat([m0] + mk + [m4, b, f, med], 1).float().contiguous()


def _eb_logits64(P, v):
    """float64 restatement of eb_logits (csrc/pointwise_common.h) and the chain of absolute values that bounds its fp32 error"""
    m, b, f = P[:, :33], P[:, 33:46], P[:, 46:58]
    l = [m[:, i] * v + b[:, i] for i in range(3)]
    A = [(m[:, i] * v).abs() + b[:, i].abs() for i in range(3)]
    l = [l[i] + f[:, i] * torch.tanh(l[i]) for i in range(3)]
    A = [A[i] * (1 + f[:, i].abs()) + f[:, i].abs() for i in range(3)]
    for k in range(1, 4):
        mk = m[:, 3 + (k - 1) * 9: 3 + k * 9]
        t = [sum(mk[:, i * 3 + j] * l[j] for j in range(3)) + b[:, 3 * k + i] for i in range(3)]
        At = [sum(mk[:, i * 3 + j] * A[j] for j in range(3)) + b[:, 3 * k + i].abs() for i in range(3)]
        l = [t[i] + f[:, 3 * k + i] * torch.tanh(t[i]) for i in range(3)]
        A = [At[i] * (1 + f[:, 3 * k + i].abs()) + f[:, 3 * k + i].abs() for i in range(3)]
    out = sum(m[:, 30 + j] * l[j] for j in range(3)) + b[:, 12]
    Aout = sum(m[:, 30 + j] * A[j] for j in range(3)) + b[:, 12].abs()
    return out, Aout


def _bits_and_bound(su, sl, du, dl, fl=1e-9):
    """likelihood |su - sl| floored; its error from the two CDF errors du, dl and ~6 EPS32 of each CDF value (the floor is
    1-Lipschitz); -> (bits, bound, unfloored likelihood, relative likelihood error r).  The bound -log2(1 - r) is linear in r only
    while r is small: the tests assert max r < R_MAX on their tensors, so no element's slack can grow towards the ~20 bits of r -> 1"""
    lik = (su - sl).abs()
    likf = lik.clamp_min(fl)
    dlik = du + dl + 6 * EPS32 * (su + sl)
    r = dlik / likf
    b = -torch.log2(likf)
    return b, -torch.log2(1 - r.clamp(max=0.999999)) + 4 * EPS32 * b, lik, r


R_MAX = 1e-2          # largest relative likelihood error a rate-term bound may assume (a 0.0145-bit slack per element)


def eb_ref64(P, v):
    """v: (M, C) float64 (the kernel's own v) -> per-element (bits, bound, unfloored likelihood, r)"""
    P = P.double()
    u, Au = _eb_logits64(P, v + 0.5)
    lo, Al = _eb_logits64(P, v - 0.5)
    sign = -torch.sign(u + lo)
    su, sl = torch.sigmoid(sign * u), torch.sigmoid(sign * lo)
    # fp32 logits: each of the five layers adds <= 10 roundings (products, sums, tanhf within 2 ulp) of its absolute chain, which the
    # later layers amplify at most as they amplify the chain itself
    du, dl = su * (1 - su) * 50 * EPS32 * Au, sl * (1 - sl) * 50 * EPS32 * Al
    return _bits_and_bound(su, sl, du, dl)


def gc_ref64(v, scale):
    """v = |y (+ noise) - mean| float64 (with its fp32 error already folded into dv), scale after the 0.11 bound"""
    t_u, t_l = (0.5 - v) / scale, (-0.5 - v) / scale
    Phi = lambda t: 0.5 * torch.erfc(-t / math.sqrt(2.0))
    phi = lambda t: torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    up, lo = Phi(t_u), Phi(t_l)
    return up, lo, t_u, t_l, phi


def _block_check(partial, bits_ref, bound, nb, what, report):
    """per-block partial sums vs float64; the blocks' fp32 tree sums (depth 8) add 8 EPS32 of the block's bits"""
    pad = nb * 256 - bits_ref.numel()
    br = F.pad(bits_ref.reshape(-1), (0, pad)).view(nb, 256)
    bd = F.pad(bound.reshape(-1), (0, pad)).view(nb, 256)
    want = br.sum(1)
    bnd = bd.sum(1) + 8 * EPS32 * (want + bd.sum(1)) + 1e-30
    assert_within(partial[:nb].cpu(), want, bnd, what + " per-block partials", report)


# (regime, noise, z_hat dtype, N, H, W, C)
EB_CASES = [("center", False, "f16", 2, 5, 9, 128), ("center", True, "f32", 2, 5, 9, 128), ("floor", False, "f32", 1, 4, 4, 128),
            ("floor", True, "f16", 1, 4, 4, 128), ("tails", False, "f32", 2, 5, 9, 128), ("tails", True, "f32", 2, 5, 9, 128),
            ("v0", False, "f16", 1, 3, 5, 128), ("mixed", False, "f16", 2, 17, 17, 128), ("mixed", True, "f32", 2, 17, 17, 128),
            ("mixed", False, "f32", 2, 17, 17, 128), ("mixed", True, "f16", 2, 17, 17, 128), ("tails", False, "f16", 1, 3, 5, 128)]
EB_CLASSES = {cls_eb(N * H * W * C_, nz, zd == "f32") for (_, nz, zd, N, H, W, C_) in EB_CASES}


def _eb_pick(P, regime, n, noise, g):
    """v values (M, C) of one regime: integer offsets from the median (plus U(-1/2, 1/2) noise on the noise path) whose float64
    likelihood falls in the regime"""
    C_ = P.shape[0]
    med = P[:, 58].double()
    ks = torch.arange(-240, 241, dtype=torch.float64)
    cand = ks.view(-1, 1) + med.view(1, -1)                              # (K, C)
    if noise:
        cand = cand + (torch.rand(cand.shape, generator=g, dtype=torch.float64) - 0.5) * 0.9
    cand = cand.float().double()
    _, _, lik, _ = eb_ref64(P, cand)
    if regime == "center":
        ok = lik > 1e-2
    elif regime == "floor":
        ok = lik < 1e-11
    elif regime == "tails":
        ok = (lik > 1e-8) & (lik < 1e-3)
    else:
        ok = torch.ones_like(lik, dtype=torch.bool)
    out = torch.empty(n, C_, dtype=torch.float64)
    for c in range(C_):
        idx = ok[:, c].nonzero().view(-1)
        assert idx.numel() > 0, f"no candidate of regime {regime} in channel {c}"
        out[:, c] = cand[idx[torch.randint(idx.numel(), (n,), generator=g)], c]
    return out


@pytest.mark.parametrize("regime,nz,zd,N,H,W,C_", EB_CASES, ids=[f"{r}{'_noise' if z else ''}_{d}_{n}x{h}x{w}" for r, z, d, n, h, w, _ in EB_CASES])
def test_eb_forward(regime, nz, zd, N, H, W, C_, report):
    """factorised prior: z_hat bit-exact (rint(z - med) + med, or z + noise), per-block bits against float64 by regime, and the
    double-precision total against the kernel's own partials"""
    ops = _ops()
    g = torch.Generator().manual_seed(sum(map(ord, f"{regime}{nz}{zd}{H}")))
    P = eb_params(C_, seed=5)
    M = N * H * W
    if regime == "v0":
        v = P[:, 58].double().view(1, -1).expand(M, C_).clone()
    else:
        v = _eb_pick(P, regime, M, nz, g)
    if nz:
        n32 = ((torch.rand(M, C_, generator=g) - 0.5) * 0.25).float()
        z32 = (v.float() - n32)
    else:
        z32 = (v + (torch.rand(M, C_, generator=g, dtype=torch.float64) - 0.5) * 0.8).float()   # rounds back to v's integer offset
    z = ops.FM(z32.view(N, H, W, C_).cuda())
    noise = ops.FM(n32.view(N, H, W, C_).cuda()) if nz else None
    T = torch.float32 if zd == "f32" else torch.float16
    zbuf = buffer((N, H, W, C_ + 8), T)
    z_hat = ops.FM(zbuf, 8, N, C_)
    before = zbuf.clone()
    numel = M * C_
    nb = (numel + 255) // 256
    assert cls_eb(numel, nz, zd == "f32") in EB_CLASSES
    partial = torch.full((nb + 1,), 12345.0, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    Pd = P.cuda()
    _chk(_lib().tdvc_eb_forward(_ref(z), Pd.data_ptr(), _ref(noise) if nz else None, _ref(z_hat), out.data_ptr(), partial.data_ptr(), nb,
                                ops._stream()), "eb_forward")
    torch.cuda.synchronize()
    # the kernel's v, in torch fp32 on the CPU
    med32 = P[:, 58].view(1, C_)
    v32 = (z32 + n32) if nz else (torch.round(z32 - med32) + med32)
    assert_bits(view(z_hat), v32.view(N, H, W, C_).to(T), f"z_hat {regime}")
    assert_outside_unchanged(before, z_hat, "z_hat")
    assert float(partial[nb]) == 12345.0
    b_ref, b_bnd, lik, r = eb_ref64(P, v32.double())
    report(f"eb {regime}{' noise' if nz else ''}: max relative likelihood error of the bound {float(r.max()):.3e}")
    assert float(r.max()) < R_MAX, f"eb {regime}: the per-element bound reaches r = {float(r.max()):.3e} of the likelihood"
    if regime == "floor":
        assert bool((lik < 1e-10).all())
    elif regime == "tails":
        assert bool(((lik > 1e-9) & (lik < 1e-2)).all()), "tails regime left its range"
        hi = v32.double() > P[:, 58].double().view(1, C_)
        assert 0.2 < float(hi.double().mean()) < 0.8, "both tails"
    _block_check(partial, b_ref, b_bnd, nb, f"eb {regime}{' noise' if nz else ''}", report)
    tot = float(partial[:nb].double().sum())
    assert abs(float(out) - tot) <= 1e-12 * tot + 1e-9, f"eb final sum {float(out)} vs sum of partials {tot} ({nb} partials)"
    report(f"eb {regime}: {float(out):.6f} bits, float64 {float(b_ref.sum()):.6f}, {nb} partials")


# (regime, noise, N, H, W, C)
GC_CASES = [("center", False, 2, 9, 15, 128), ("center", True, 2, 9, 15, 128), ("below_bound", False, 1, 5, 7, 128),
            ("below_bound", True, 1, 5, 7, 128), ("v0", False, 1, 3, 5, 128), ("tails", False, 2, 5, 9, 128), ("tails", True, 2, 5, 9, 128),
            ("floor", False, 1, 4, 4, 128), ("floor", True, 1, 4, 4, 128), ("mixed", False, 2, 17, 17, 128), ("mixed", True, 2, 17, 17, 128)]
GC_CLASSES = {cls_gc(N * H * W * C_, nz) for (_, nz, N, H, W, C_) in GC_CASES}


@pytest.mark.parametrize("regime,nz,N,H,W,C_", GC_CASES, ids=[f"{r}{'_noise' if z else ''}_{n}x{h}x{w}" for r, z, n, h, w, _ in GC_CASES])
def test_gc_forward(regime, nz, N, H, W, C_, report):
    """Gaussian conditional: per-block bits against float64 (erfc), by regime, and the double-precision total"""
    ops = _ops()
    g = torch.Generator().manual_seed(sum(map(ord, f"gc{regime}{nz}{H}")))
    M = N * H * W
    mean = (torch.randn(M, C_, generator=g) * 3).float()
    if regime == "below_bound":
        sraw = torch.rand(M, C_, generator=g) * 0.6 - 0.5                   # [-0.5, 0.1): every scale is raised to 0.11
        k = torch.randint(0, 2, (M, C_), generator=g).double()
    else:
        # tails: scales of 2 and more keep the rounded offsets inside 1e-9 < likelihood < 1e-3
        sraw = torch.rand(M, C_, generator=g) * (0.7 if regime == "tails" else 2.5) + (2.0 if regime == "tails" else 0.2)
        zt = {"center": torch.rand(M, C_, generator=g) * 1.5, "tails": torch.rand(M, C_, generator=g) * 1.4 + 3.8,
              "floor": torch.rand(M, C_, generator=g) * 20 + 12, "v0": torch.zeros(M, C_),
              "mixed": torch.rand(M, C_, generator=g) * 9}[regime]
        k = torch.round(zt.double() * sraw.double() + (0.5 if regime in ("tails", "floor") else 0.0))
    sgn = torch.where(torch.rand(M, C_, generator=g) < 0.5, -1.0, 1.0).double()
    y = (mean.double() + sgn * k).float()
    n32 = ((torch.rand(M, C_, generator=g) - 0.5)).float() if nz else None
    s32 = sraw.float()
    gp = ops.FM(torch.cat([s32, mean], 1).view(N, H, W, 2 * C_).cuda())
    yf = ops.FM(torch.cat([y, torch.zeros(M, 8)], 1).view(N, H, W, C_ + 8).cuda(), 0, N, C_)
    noise = ops.FM(n32.view(N, H, W, C_).cuda()) if nz else None
    numel = M * C_
    nb = (numel + 255) // 256
    assert cls_gc(numel, nz) in GC_CLASSES
    partial = torch.full((nb + 1,), 12345.0, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    _chk(_lib().tdvc_gc_forward(_ref(yf), _ref(gp), _ref(noise) if nz else None, out.data_ptr(), partial.data_ptr(), nb, ops._stream()),
         "gc_forward")
    torch.cuda.synchronize()
    assert float(partial[nb]) == 12345.0
    # the kernel's v: |rint(y - mean)| in fp32 (a correctly rounded subtraction, then rint), or |(y + n) - mean| whose two fp32
    # roundings are carried as dv
    if nz:
        v = ((y.double() + n32.double()) - mean.double()).abs()
        dv = 2 * EPS32 * (y.double().abs() + n32.double().abs() + mean.double().abs())
    else:
        v = torch.round(y - mean).double().abs()
        dv = torch.zeros_like(v)
    scale = torch.maximum(s32, torch.tensor(0.11, dtype=torch.float32)).double()
    up, lo, t_u, t_l, phi = gc_ref64(v, scale)
    # CDF errors: the argument (subtract, divide, the product with k = fp32(1/sqrt 2): 4 EPS32 relative) plus dv / scale, times the
    # density; erfcf and the 0.5 scaling within 8 EPS32 of the value
    du = phi(t_u) * (4 * EPS32 * t_u.abs() + dv / scale) + 8 * EPS32 * up
    dl = phi(t_l) * (4 * EPS32 * t_l.abs() + dv / scale) + 8 * EPS32 * lo
    b_ref, b_bnd, lik, r = _bits_and_bound(up, lo, du, dl)
    report(f"gc {regime}{' noise' if nz else ''}: max relative likelihood error of the bound {float(r.max()):.3e}")
    assert float(r.max()) < R_MAX, f"gc {regime}: the per-element bound reaches r = {float(r.max()):.3e} of the likelihood"
    if regime == "floor":
        assert bool((lik < 1e-10).all())
    elif regime == "tails":
        assert bool(((lik > 1e-9) & (lik < 1e-3)).all()), "tails regime left its range"
    _block_check(partial, b_ref, b_bnd, nb, f"gc {regime}{' noise' if nz else ''}", report)
    tot = float(partial[:nb].double().sum())
    assert abs(float(out) - tot) <= 1e-12 * tot + 1e-9, f"gc final sum {float(out)} vs sum of partials {tot} ({nb} partials)"
    report(f"gc {regime}: {float(out):.6f} bits, float64 {float(b_ref.sum()):.6f}, {nb} partials")


# ------------------------------------------------------------------------------------------------------------------ batch / frame views
# FM.batch(n0, k): off = n0 * sn inside a buffer of more images; FM.as_slices(b, T, Cs): the T channel slices of image b as a batch of
# T images (sn = Cs < sp: the images interleave inside each pixel) -- the loop filter's 4-frame buffers (modules.py)
VIEW_CASES = [(op, kind) for op in ("scale_act_res", "bcast_add_act", "quantize", "upsample2x") for kind in ("batch", "slices")]


def _views(kind, dtype, H, W, C_, g=None, fill=None):
    """a view of `kind` over a fresh buffer (random when `fill`, sentinel otherwise): 2 images of C channels"""
    ops = _ops()
    if kind == "batch":
        return ops.FM(buffer((4, H, W, C_), dtype, fill, g)).batch(1, 2)
    return ops.FM(buffer((2, H, W, 2 * C_), dtype, fill, g)).as_slices(1, 2, C_)


@pytest.mark.parametrize("op,kind", VIEW_CASES, ids=[f"{o}_{k}" for o, k in VIEW_CASES])
def test_batch_and_frame_views(op, kind, report):
    """the storing and in-place kernels on batch and frame-slice views: values as on dense maps, every byte outside the view unchanged"""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(len(op) * 10 + len(kind))
    H, W = 6, 7
    if op == "scale_act_res":
        a, r = _views(kind, torch.float16, H, W, 64, g, "randn"), _views(kind, torch.float16, H, W, 64, g, "randn")
        y, y2 = _views(kind, torch.float16, H, W, 64), _views(kind, torch.float16, H, W, 64)
        gate = torch.rand(2, 64, generator=g, device="cuda")
        assert cls_scale_act_res(a, y, gate, 2, 0.1, r, 1.0, y2)[1] == "f16"
        before = [y.t.clone(), y2.t.clone()]
        ops.scale_act_res(a, y, gate=gate, act=2, slope=0.1, res=r, res_sign=1.0, out2=y2)
        torch.cuda.synchronize()
        want = _sar_want32(a, gate, 2, 0.1, r, 1.0).half()
        outs = [(y, want, before[0]), (y2, want, before[1])]
    elif op == "bcast_add_act":
        outs = []
        for T, Cb in ((4, 16), (2, 32)):                    # the T = 4 kernel and the generic one
            x = _views(kind, torch.float16, H, W, 64, g, "randn")
            b = _views(kind, torch.float16, H, W, Cb, g, "randn")
            before, x0 = x.t.clone(), view(x).cpu().float()
            ops.bcast_add_act(x, b, T, 0.1)
            torch.cuda.synchronize()
            outs.append((x, lrelu32(x0 + view(b).cpu().float().repeat(1, 1, 1, T), 2, 0.1).half(), before))
    elif op == "quantize":
        outs = []
        for nz in (False, True):
            y = _views(kind, torch.float32, H, W, 128, g, "randn")
            view(y).mul_(6.0)
            n = _views(kind, torch.float32, H, W, 128, g, "rand") if nz else None
            out = _views(kind, torch.float16, H, W, 128)
            before = out.t.clone()
            ops.quantize(y, out, noise=n)
            torch.cuda.synchronize()
            y32 = view(y).cpu()
            outs.append((out, ((y32 + view(n).cpu()) if nz else torch.round(y32)).half(), before))
    else:
        x = _views(kind, torch.float16, H, W, 64, g, "randn")
        y = _views(kind, torch.float16, 2 * H, 2 * W, 64)
        before = y.t.clone()
        ops.upsample2x(x, out=y)
        torch.cuda.synchronize()
        xc = view(x).cpu().double().permute(0, 3, 1, 2)
        ref = F.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        absr = F.interpolate(xc.abs(), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert_within(view(y).cpu(), ref, 6 * EPS32 * absr + EPS16 * ref.abs() + TINY16, f"upsample2x {kind} view", report)
        outs = [(y, None, before)]
    for fm, want, before in outs:
        assert fm.off > 0 and (fm.sn < fm.sp if kind == "slices" else fm.sn == fm.H * fm.W * fm.sp)
        if want is not None:
            assert_bits(view(fm), want, f"{op} {kind} view")
        assert_outside_unchanged(before, fm, f"{op} {kind} view")


# ------------------------------------------------------------------------------------------------------------------ coverage guard
def table_classes():
    return (LAYOUT_CLASSES | SAR_CLASSES | SE_CLASSES | BC_CLASSES | UP_CLASSES | AP_CLASSES | RS_CLASSES | AF_CLASSES | SP_CLASSES |
            Q_CLASSES | EB_CLASSES | GC_CLASSES)


def _recorder(monkeypatch, seen):
    """wrap the ops.* streaming entry points: every call adds its class to `seen` (the call itself runs unchanged)"""
    ops = _ops()

    def wrap(name, classify):
        fn = getattr(ops, name)

        def w(*a, **k):
            seen.add(classify(*a, **k))
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, w)

    def q_cls(y, out, noise=None):
        return cls_quantize(y.f32, out.f32, noise is not None)

    def se_cls(x, p, partial=None):
        nb = partial[1] if partial is not None else max(1, min(1024, x.H * x.W // 256))      # ops.se_gate
        return cls_se_gate(x.C, nb)

    def from_cls(x, Cpad=None, dtype=torch.float16, out=None):
        Cv = out.C if out is not None else (ops.pad8(x.shape[1]) if Cpad is None else Cpad)
        return ("nchw_to_fmap", "f32" if (out.f32 if out is not None else dtype == torch.float32) else "f16", x.shape[1], Cv)

    wrap("scale_act_res", cls_scale_act_res)
    wrap("se_gate", se_cls)
    wrap("bcast_add_act", lambda x, b, T, slope: cls_bcast(T, _dt(x), _dt(b)))
    wrap("add_flow", cls_add_flow)
    wrap("upsample2x", lambda x, out=None: cls_upsample(x, out))
    wrap("avgpool2", lambda x: ("avgpool2", x.C, x.sp))
    wrap("spynet_level_input", lambda r, s, fl, up, cat8: cls_spynet(r, s, fl, up))
    wrap("resize_bilinear", lambda x, H, W, chscale=None: cls_resize(x, H, W, chscale))
    wrap("eb_forward", lambda z, params, z_hat, bits_out, noise=None: cls_eb(z.N * z.H * z.W * z.C, noise is not None, z_hat.f32))
    wrap("gc_forward", lambda y, gp, bits_out, noise=None: cls_gc(y.N * y.H * y.W * y.C, noise is not None))
    wrap("quantize", q_cls)
    wrap("from_nchw", from_cls)
    to = ops.FM.to_nchw

    def to_nchw(self, C_=None):
        seen.add(("fmap_to_nchw", _dt(self)))
        return to(self, C_)
    monkeypatch.setattr(ops.FM, "to_nchw", to_nchw)


def test_production_streaming_classes_have_cases(monkeypatch, report):
    """one 1088 x 1920 inference frame and one 4 x 256 x 256 training-mode forward (under the tape, no backward): every class of
    streaming-kernel call they make must have a row in the case tables above"""
    from tdvc_amd import autograd, synth
    from tdvc_amd.model.pnet import VideoCompressor
    seen = set()
    _recorder(monkeypatch, seen)
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda().eval()
    g = synth.make_gop(1234, 2, BIG_H, BIG_W).float()
    refs = torch.stack([g[0], g[0], g[0], g[0]]).unsqueeze(0).cuda()
    with torch.no_grad():
        m(g[1:2].cuda(), refs, True)
    torch.cuda.synchronize()
    n_inf = len(seen)
    m.train()
    B, H, W = 4, 256, 256
    gop = synth.make_gop(99, 2, H, W).float()
    x = gop[1:2].expand(B, 3, H, W).contiguous().cuda()
    refs = gop[0].view(1, 1, 3, H, W).expand(B, 4, 3, H, W).contiguous().cuda()
    with autograd.record():
        m(x, refs, True)
    torch.cuda.synchronize()
    missing = sorted(seen - table_classes(), key=str)
    report(f"streaming-kernel call classes: {n_inf} in the 1088x1920 frame, {len(seen)} with the training forward; without a case: {missing}")
    report("classes seen: " + "; ".join(str(s) for s in sorted(seen, key=str)))
    assert len(seen) >= 10
    assert not missing, f"streaming-kernel call classes that production reaches without an op-level case: {missing}"
