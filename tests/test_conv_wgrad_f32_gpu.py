"""The fp32 conv backward of the fp32-coder training mode, op level, against float64 on the CPU.

Weight / bias gradient: conv_wgrad_f32_kernel (v_mfma_f32_32x32x2_f32) + the shared second stage; data gradient: conv_f32 on the
dgrad packing.  The reference is torch.nn.functional.conv2d in double with autograd.  The bounds are a priori: a sum of K products in
fp32, in ANY order, is within (K - 1 + 1) u of the exact sum of the absolute products (u = 2^-24: K - 1 additions, one rounding per
product); three more u cover the square of `square_x`, the multiplication by `scale` and the epilogue's additions, and u |result| the
final rounding of the accumulate into the non-zero destination:

    |dW - dW64| <= (K + 3) u (|g|^T |x|)64 |scale| + u |dW64|,    K = N Ho Wo,    dW64 = scale * gradient + base
    |db - db64| <= (K + 3) u sum|g| |scale| + u |db64|
    |dX - dX64| <= (K + 3) u (|g| * |w|)64 + u |dX64|,            K = live taps * Cout (12 taps for the masked conv)
"""
import pytest
import torch
import torch.nn.functional as F

from util import fm_to_cpu, randn, to_fm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON = 1.0e4           # padding channels of g and x are don't-care inputs: they must not reach any real output
F32 = torch.float32

CASES = [
    # name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked
    ("3x3_128_128", 2, 128, 128, 3, 1, 1, 11, 14, False, False, False),
    ("3x3_128_128_1x1map", 2, 128, 128, 3, 1, 1, 1, 1, False, False, False),          # the z grid of a 64 x 64 input
    ("3x3_s2_64_128", 2, 64, 128, 3, 2, 1, 12, 18, False, False, False),
    ("3x3_s2_128_128", 2, 128, 128, 3, 2, 1, 12, 18, False, False, False),
    ("3x3_s2_128_128_2x2map", 2, 128, 128, 3, 2, 1, 2, 2, False, False, False),
    ("1x1_s2_128_128", 2, 128, 128, 1, 2, 0, 12, 18, False, False, False),
    ("subpel_128_128", 1, 128, 512, 3, 1, 1, 6, 9, True, False, False),
    ("subpel_128_64", 1, 128, 256, 3, 1, 1, 6, 9, True, False, False),
    ("masked_5x5_128_256", 2, 128, 256, 5, 1, 2, 6, 7, False, False, True),           # all 25 wgrad_taps, plus bias
    ("1x1_512_426", 2, 512, 426, 1, 1, 0, 5, 7, False, False, False),
    ("1x1_426_341", 2, 426, 341, 1, 1, 0, 5, 7, False, False, False),
    ("1x1_341_256", 2, 341, 256, 1, 1, 0, 5, 7, False, False, False),
    ("gdn_1x1_128_128_sq", 2, 128, 128, 1, 1, 0, 9, 11, False, True, False),
    # the further classes of an fp32-coder step: the first analysis block's skip, h_s's 192-channel layers
    ("1x1_s2_64_128", 2, 64, 128, 1, 2, 0, 12, 18, False, False, False),
    ("3x3_128_192", 2, 128, 192, 3, 1, 1, 5, 7, False, False, False),
    ("subpel_192_192", 1, 192, 768, 3, 1, 1, 5, 7, True, False, False),
    ("3x3_192_256", 2, 192, 256, 3, 1, 1, 7, 9, False, False, False),
]
SCALE = 0.37             # not a power of two: the loss-scale multiplication rounds


def _ops():
    from tdvc_amd import ops
    return ops


def _case_data(case):
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    x = randn(N, cin, H, W, seed=401)
    w = randn(cout, cin, k, k, seed=402) * (1.0 / (cin * k * k) ** 0.5)
    b = randn(cout, seed=403) * 0.1
    live = [(dy, dx) for dy in range(k) for dx in range(k)]
    if masked:
        live = [(dy, dx) for dy in range(k) for dx in range(k) if dy < k // 2 or (dy == k // 2 and dx < k // 2)]
        mask = torch.zeros(k, k)
        for dy, dx in live:
            mask[dy, dx] = 1.0
        w = w * mask
    return x, w, b, live


def _fwd64(x, w, b, stride, pad, shuffle, square_x):
    y = F.conv2d(x * x if square_x else x, w, b, stride=stride, padding=pad)
    return F.pixel_shuffle(y, 2) if shuffle else y


def _reference(case, x, w, b):
    """float64: (gy, dW, db, dX of the plain conv, |g|^T|x|, sum|g|, |g| * |w|, K of the weight gradient)"""
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    y = _fwd64(xr, wr, br, stride, pad, shuffle, square_x)
    gy = randn(*y.shape, seed=404) * 0.5
    gw, gb = torch.autograd.grad(y, (wr, br), gy.double())
    # the sums of absolute products: the same bilinear maps on |g|, |x|, |w|
    xa, wa, ba = x.double().abs().requires_grad_(), w.double().abs().requires_grad_(), b.double().requires_grad_()
    aw, ab = torch.autograd.grad(_fwd64(xa, wa, ba, stride, pad, shuffle, square_x), (wa, ba), gy.double().abs())
    # data gradient of the conv itself (the GDN chain multiplies by 2x outside the conv): plain input
    xp, xpa = x.double().requires_grad_(), x.double().abs().requires_grad_()
    gx, = torch.autograd.grad(_fwd64(xp, w.double(), None, stride, pad, shuffle, False), xp, gy.double())
    ax, = torch.autograd.grad(_fwd64(xpa, w.double().abs(), None, stride, pad, shuffle, False), xpa, gy.double().abs())
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return gy, gw, gb, gx, aw, ab, ax, N * Ho * Wo


def _ratio(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    return float(r.max())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_backward_f32(case, report):
    ops = _ops()
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    x, w, b, live = _case_data(case)
    gy, gw, gb, gx, aw, ab, ax, K = _reference(case, x, w, b)

    wd, bd = w.cuda(), b.cuda()
    pc = ops.pack_conv(wd, bd, stride=stride, pad=pad, shuffle=shuffle, taps=live if masked else None)
    if masked:
        pc.orig["wgrad_taps"] = [(dy, dx) for dy in range(k) for dx in range(k)]        # as coder.ctx_conv builds it
    xf = to_fm(x, ops, dtype=F32)
    assert xf.f32 and xf.C == ops.pad8(cin)
    xf.t[..., cin:] = POISON
    g = to_fm(gy, ops, dtype=F32)
    if not shuffle:
        g.t[..., cout:] = POISON
    gq = ops.pixel_unshuffle(g) if shuffle else g
    assert gq.f32

    # ---- weight / bias gradient: accumulated onto non-zero buffers with a scale != 1
    base_w = (randn(w.numel(), seed=405) * 0.05).cuda()
    base_b = (randn(cout, seed=406) * 0.05).cuda()

    def run(defer=None):
        dw, db = base_w.clone(), base_b.clone()
        ops.conv_wgrad(pc, gq, xf, dw, scale=SCALE, square_x=square_x, db=db, defer=defer)
        if defer is not None:
            assert len(defer.items) == 1
            defer.flush()
        torch.cuda.synchronize()
        return dw, db

    dw, db = run()
    ref_w = SCALE * gw + base_w.cpu().double().view(gw.shape)
    ref_b = SCALE * gb + base_b.cpu().double()
    bound_w = (K + 3) * U * aw * SCALE + U * ref_w.abs()
    bound_b = (K + 3) * U * ab * SCALE + U * ref_b.abs()
    rw = _ratio(dw.cpu().view(gw.shape), ref_w, bound_w)
    rb = _ratio(db.cpu(), ref_b, bound_b)
    report(f"wgrad f32 {name}: K={K} max |dW - dW64| / bound = {rw:.4f}, max |db - db64| / bound = {rb:.4f}")
    assert float((dw - base_w).abs().max()) > 0
    if masked:
        assert float(gw[:, :, k - 1, k - 1].abs().max()) > 0            # the masked taps' gradient is filled too
    assert rw <= 1.0, f"wgrad f32 {name}: {rw} x the bound"
    assert rb <= 1.0, f"bgrad f32 {name}: {rb} x the bound"
    # bit-reproducible from launch to launch; the deferred second stage (WgradBatch) gives the same bits
    dw2, db2 = run()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{name}: two immediate launches differ"
    dw3, db3 = run(ops.WgradBatch())
    assert torch.equal(dw, dw3) and torch.equal(db, db3), f"{name}: the WgradBatch form differs from the immediate form"

    # ---- data gradient through ops.conv_dgrad on fp32 maps (conv_f32 on the dgrad packing), accumulated onto a non-zero map
    base_x = randn(N, cin, H, W, seed=407) * 0.1
    dx = to_fm(base_x, ops, dtype=F32)
    dx.t[..., cin:] = 3.0
    ops.PROFILE = []
    try:
        ops.conv_dgrad(pc, gq, dx, accumulate=True)
        torch.cuda.synchronize()
        kern = [e["kernel"] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert kern == ["conv_f32"], kern
    Kx = len(live) * cout
    ref_x = gx + base_x.double()
    rx = _ratio(fm_to_cpu(dx, cin), ref_x, (Kx + 3) * U * ax + U * ref_x.abs())
    report(f"dgrad f32 {name}: K={Kx} max |dX - dX64| / bound = {rx:.4f}")
    assert rx <= 1.0, f"dgrad f32 {name}: {rx} x the bound"
    assert torch.equal(dx.t[..., cin:], torch.full_like(dx.t[..., cin:], 3.0)), f"dgrad f32 {name}: padding channels of dX written"


def test_mixed_dtypes_are_refused(report):
    """fp16 dY with fp32 X (and the reverse): an error status with a message, nothing launched"""
    ops = _ops()
    from tdvc_amd import _lib as L
    w = randn(64, 64, 3, 3, seed=411) * 0.05
    pc = ops.pack_conv(w.cuda(), None, stride=1, pad=1)
    x, gy = randn(1, 64, 9, 11, seed=412), randn(1, 64, 9, 11, seed=413)
    for gd, xd in ((torch.float16, F32), (F32, torch.float16)):
        dw = torch.full((w.numel(),), 0.25, device="cuda")
        with pytest.raises(L.TdvcHipError, match="both fmaps must be fp16 or both fp32"):
            ops.conv_wgrad(pc, to_fm(gy, ops, dtype=gd), to_fm(x, ops, dtype=xd), dw)
        batch = ops.WgradBatch()
        with pytest.raises(L.TdvcHipError, match="both fmaps must be fp16 or both fp32"):
            ops.conv_wgrad(pc, to_fm(gy, ops, dtype=gd), to_fm(x, ops, dtype=xd), dw, defer=batch)
        torch.cuda.synchronize()
        assert not batch.items
        assert torch.equal(dw, torch.full_like(dw, 0.25)), "a refused call wrote dW"
    report("conv_wgrad: mixed fp16 / fp32 operands are refused before any launch")


# ------------------------------------------------------------------------------------------------------------------ coverage guard
def op_level_wgrad_f32_classes():
    """(kh, kw, stride, cin, cout, shuffle, square_x, masked) of every fp32 conv weight gradient that has a row in CASES"""
    return {(k, k, st, ci, co, sh, sq, mk) for (_, _, ci, co, k, st, _, _, _, sh, sq, mk) in CASES}


def test_fp32_training_wgrad_geometries_have_op_level_tests(report):
    """one coder_fp32 forward + backward of the whole model at 2 x 64 x 64: every fp32 conv weight-gradient geometry it runs
    (ops.PROFILE's `geo` of the conv_wgrad_f32 launches) must be a row of CASES"""
    from tdvc_amd import autograd, synth
    from tdvc_amd.model.pnet import VideoCompressor
    ops = _ops()
    B, H, W = 2, 64, 64
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda().train()
    m.train_coder_fp32 = True
    frames = synth.make_gop(1234, 7, H, W).float()
    x = frames[3:5].cuda()
    refs = torch.stack([torch.stack([frames[0], frames[0], frames[1], frames[2]]),
                        torch.stack([frames[0], frames[1], frames[2], frames[3]])]).cuda()
    ops.PROFILE = []
    try:
        with autograd.record() as tape:
            r, _, _, _, _ = m(x, refs, True)
            tape.grad_tensor(r).copy_((r - x) * (2.0 / r.numel()))
            tape.rate_grad = 1.0 / float(B * H * W)
            tape.backward()
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
    seen = {}
    for e in prof:
        if e["kernel"] == "conv_wgrad_f32":
            seen[e["geo"]] = seen.get(e["geo"], 0) + 1
    missing = sorted(set(seen) - op_level_wgrad_f32_classes())
    report(f"fp32 wgrad geometry classes of a coder_fp32 step: {len(seen)} ({sum(seen.values())} launches); without an op-level case: {missing}")
    assert len(seen) >= 10
    assert not missing, f"fp32 conv weight-gradient geometries without an op-level test: {missing}"
