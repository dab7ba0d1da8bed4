"""Deformable conv: fused fp16 kernel and the fp32 `_ext` operator vs the oracle; the
reference's own known-answer test `check_zero_offset` (main/utils/dcnv2/testcpu.py:34-69)."""
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, fm_to_cpu, randn, rnd16, to_fm

pytestmark = pytest.mark.gpu


def test_ext_zero_offset_kat(report):
    """zero offsets, mask = sigmoid(0) = 0.5, identity centre-tap weights => 2*output == input"""
    import _ext
    N, inC, inH, inW, outC, k = 2, 2, 4, 4, 2, 3
    w = torch.zeros(outC, inC, k, k)
    for c in range(inC):
        w[c, c, 1, 1] = 1.0
    x = randn(N, inC, inH, inW, seed=1)
    offset = torch.zeros(N, 2 * k * k, inH, inW)
    mask = torch.sigmoid(torch.zeros(N, k * k, inH, inW))
    out = _ext.dcn_v2_forward(x.cuda(), w.cuda(), torch.zeros(outC).cuda(), offset.cuda(), mask.cuda(),
                              k, k, 1, 1, 1, 1, 1, 1, 1)
    d = float((x - 2 * out.cpu()).abs().max())
    report(f"check_zero_offset: max|input - 2*output| = {d:.3e}")
    assert d < 1e-10


@pytest.mark.parametrize("cfg", [
    dict(B=2, C=2, Cout=2, H=4, W=4, k=3, s=1, p=1, d=1, G=1, osc=2.0),      # testcpu.py geometry
    dict(B=1, C=64, Cout=64, H=20, W=28, k=3, s=1, p=1, d=1, G=8, osc=3.0),  # hot-path geometry
    dict(B=2, C=16, Cout=24, H=11, W=13, k=3, s=2, p=1, d=1, G=4, osc=1.5),
    dict(B=1, C=8, Cout=8, H=9, W=9, k=3, s=1, p=2, d=2, G=2, osc=4.0),
])
def test_ext_forward_vs_oracle(cfg, report):
    import _ext
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    B, C, Cout, H, W, k, s, p, d, G = (cfg[x] for x in ("B", "C", "Cout", "H", "W", "k", "s", "p", "d", "G"))
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = randn(B, C, H, W, seed=2)
    w = randn(Cout, C, k, k, seed=3, scale=0.2)
    b = randn(Cout, seed=4)
    off = randn(B, 2 * G * k * k, Ho, Wo, seed=5, scale=cfg["osc"])
    m = torch.sigmoid(randn(B, G * k * k, Ho, Wo, seed=6))
    ref = dcn_v2_forward_ref(x, w, b, off, m, k, k, s, s, p, p, d, d, G)
    got = _ext.dcn_v2_forward(x.cuda(), w.cuda(), b.cuda(), off.cuda(), m.cuda(), k, k, s, s, p, p, d, d, G).cpu()
    assert_close(got, ref, 1e-5, 1e-5, f"_ext.dcn_v2_forward {cfg}", report)


def test_ext_errors():
    import _ext
    x = torch.zeros(1, 4, 8, 8).cuda()
    w = torch.zeros(4, 4, 3, 3).cuda()
    b = torch.zeros(4).cuda()
    off = torch.zeros(1, 18, 8, 8).cuda()
    m = torch.zeros(1, 9, 8, 8).cuda()
    with pytest.raises(RuntimeError):
        _ext.dcn_v2_forward(x, w, b, off, m, 5, 5, 1, 1, 1, 1, 1, 1, 1)          # kernel shape mismatch
    with pytest.raises(RuntimeError):
        _ext.dcn_v2_forward(x.cpu(), w, b, off, m, 3, 3, 1, 1, 1, 1, 1, 1, 1)    # CPU tensor
    with pytest.raises(RuntimeError):
        _ext.dcn_v2_forward(x, torch.zeros(4, 3, 3, 3).cuda(), b, off, m, 3, 3, 1, 1, 1, 1, 1, 1, 1)


def test_fused_dcn_rejects_batch_beyond_grid_limit():
    """the batch is the grid's y dimension (at most 65535): N = 65536 is an error on fp16 and on fp32 maps alike, raised before
    anything is launched -- y keeps every bit"""
    from tdvc_amd import _lib, ops
    N = 65536
    pc = ops.pack_conv(torch.zeros(64, 64, 3, 3), torch.zeros(64), stride=1, pad=1, ck=64)
    for dt in (torch.float16, torch.float32):
        x = ops.FM(torch.zeros(N, 1, 1, 64, dtype=dt, device="cuda"))
        om = ops.FM(torch.zeros(N, 1, 1, 216, dtype=dt, device="cuda"))
        sentinel = torch.full((N, 1, 1, 64), 0x5A5A, dtype=torch.int16, device="cuda")
        y = ops.FM(sentinel.clone().view(torch.float16))
        with pytest.raises(_lib.TdvcHipError):
            ops.dcn_fused(x, om, pc, y, groups=8, planar=False)
        torch.cuda.synchronize()
        assert torch.equal(y.t.view(torch.int16), sentinel)


@pytest.mark.parametrize("H,W", [(20, 28), (64, 96), (88, 104)])      # the last one is large enough for the LDS-window kernel
def test_fused_dcn_vs_oracle(H, W, report):
    """fp16 fused kernel (sampling + modulation + contraction + fp16 rounding + LeakyReLU) vs the
    oracle DCN module fed the same fp16-rounded operands"""
    from tdvc_amd import ops
    from oracle.tdvc_ref.blocks import DCN as RefDCN
    from tdvc_amd.model.modules import DCN
    from tdvc_amd.synth import fill_parameters
    ref = RefDCN(64, 64, 3, 1, 1, deformable_groups=8).eval()
    hold = torch.nn.Module(); hold.add_module("dconv", ref); fill_parameters(hold)
    with torch.no_grad():
        for p_ in ref.parameters():
            p_.copy_(rnd16(p_))
        ref.conv_offset_mask.weight.mul_(3.0)      # offsets of a few pixels
    m = DCN(64, 64, 3, 1, 1, deformable_groups=8)
    m.load_state_dict(ref.state_dict())
    m.cuda()
    x = rnd16(randn(2, 64, H, W, seed=7))
    y = rnd16(randn(2, 64, H, W, seed=8))
    with torch.no_grad():
        # the oracle's offsets come from an fp32 conv; round them like the fp16 path does
        offset, mask_ = ref.offsets_and_mask(y)
        om = ref.conv_offset_mask(y)
        om16 = rnd16(om)
        o1, o2, ml = torch.chunk(om16, 3, 1)
        from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
        out = dcn_v2_forward_ref(x, ref.weight, ref.bias, torch.cat((o1, o2), 1), torch.sigmoid(ml), 3, 3, 1, 1, 1, 1, 1, 1, 8)
        want = F.leaky_relu(out.half(), 0.1).float()
    dst = ops.FM.empty(2, H, W, 64)
    m.run(to_fm(x, ops), to_fm(y, ops), dst, act=ops.ACT_LRELU, slope=0.1)
    assert_close(fm_to_cpu(dst), want, 4e-3, 4e-3, f"fused DCN {H}x{W}", report)
    # the group-planar gather (default on large maps: one extra pass over x, corners of neighbouring pixels share lines)
    # samples the same values with the same arithmetic: bit-identical output
    om_fm = ops.conv(to_fm(y, ops), ops.pack_conv(m.conv_offset_mask.weight, m.conv_offset_mask.bias, stride=1, pad=1))
    pc = ops.pack_conv(m.weight, m.bias, stride=1, pad=1, ck=64)
    a, b = ops.FM.empty(2, H, W, 64), ops.FM.empty(2, H, W, 64)
    ops.dcn_fused(to_fm(x, ops), om_fm, pc, a, groups=8, act=ops.ACT_LRELU, slope=0.1, planar=False)
    ops.dcn_fused(to_fm(x, ops), om_fm, pc, b, groups=8, act=ops.ACT_LRELU, slope=0.1, planar=True)
    assert torch.equal(a.t, b.t) and torch.equal(a.t, dst.t), "group-planar gather differs from the NHWC gather"


def test_fractional_offsets_closed_form_on_affine_image(report):
    """the HIP operators against a closed form that needs no oracle (tests/test_oracle_dcn.py::affine_dcn_case: bilinear
    sampling is exact on an affine image): the fp32 `_ext` operator, and the fused fp16 kernels (gather and LDS-window) at the
    hot-path geometry with fp16-rounded operands"""
    import _ext
    from test_oracle_dcn import affine_dcn_case
    from tdvc_amd import ops
    x, w, b, off, m, want, ok = affine_dcn_case()
    got = _ext.dcn_v2_forward(x.cuda(), w.cuda(), b.cuda(), off.cuda(), m.cuda(), 3, 3, 1, 1, 1, 1, 1, 1, 2).cpu().double()
    sel = ok.unsqueeze(1).expand_as(want)
    e32 = float((got - want)[sel].abs().max())
    report(f"_ext.dcn_v2_forward vs the closed form on an affine image ({int(ok.sum())} interior pixels): max |d| {e32:.3e}")
    assert e32 < 2e-4 * max(1.0, float(want[sel].abs().max()))
    # fused fp16 kernels: 8 groups x 8 channels, 64 outputs; 96 x 128 pixels take the LDS-window kernel, 40 x 48 the gather kernel
    for H, W in ((96, 128), (40, 48)):
        x, w, b, off, m, _, ok = affine_dcn_case(N=1, G=8, cpg=8, Cout=64, H=H, W=W, seed=11, osc=1.4)
        x = (x * (4.0 / float(x.abs().max()))).half().float()               # fp16-exact operands, |x| <= 4
        w, off = w.half().float(), off.half().float()
        logit = torch.logit(m.clamp(1e-4, 1 - 1e-4)).half().float()            # the fused kernel takes mask LOGITS
        m = torch.sigmoid(logit)
        from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
        # closed form re-evaluated on the rounded operands: x is no longer exactly affine after fp16 rounding, so the reference
        # for the fp16 kernels is the restatement (itself pinned by the closed form above and in tests/test_oracle_dcn.py)
        want16 = dcn_v2_forward_ref(x, w, b, off, m, 3, 3, 1, 1, 1, 1, 1, 1, 8)
        om = torch.cat((off, logit), 1).permute(0, 2, 3, 1).contiguous()         # NHWC [offsets 144 | mask logits 72]
        pc = ops.pack_conv(w, b, stride=1, pad=1, ck=64)
        y = ops.FM.empty(1, H, W, 64)
        ops.dcn_fused(ops.FM(x.permute(0, 2, 3, 1).contiguous().half().cuda()), ops.FM(om.half().cuda()), pc, y, groups=8, round16=True, planar=False)
        gotf = y.t.float().cpu().permute(0, 3, 1, 2)
        sel = ok.unsqueeze(1).expand_as(gotf)
        d = (gotf - want16)[sel].abs()
        tol = 4e-3 * (1.0 + want16[sel].abs())
        report(f"fused DCN {H}x{W} on the (fp16-rounded) affine image, interior pixels: max |d| {float(d.max()):.3e} (|out| <= {float(want16[sel].abs().max()):.2f})")
        assert bool((d <= tol).all())


LDS_CASES = [
    # name, N, H, W, offset sigma (px), coherent shift (dy, dx), poison
    ("small_offsets", 1, 96, 128, 1.5, (0.0, 0.0), False),
    ("ragged_tile_edges", 2, 91, 117, 1.5, (0.0, 0.0), False),         # H % 8, W % 16 != 0: overhanging tiles
    ("coherent_motion", 1, 96, 128, 1.0, (11.3, -7.6), False),         # the window follows the tile's mean displacement
    ("wild_offsets", 1, 96, 128, 9.0, (0.0, 0.0), False),              # most samples leave the window: fallback gather
    ("nan_inf_offsets", 1, 96, 128, 1.5, (0.0, 0.0), True),
]


@pytest.mark.parametrize("case", LDS_CASES, ids=[c[0] for c in LDS_CASES])
def test_dcn_lds_window_kernel_equals_gather_kernel(case, report):
    """tdvc_dcn_fused takes the LDS-window kernel on maps of >= 8192 pixels; it must reproduce the L1-gather kernel bit for
    bit whatever the offsets do (same arithmetic, same accumulation order; only the source of the corner vectors differs)"""
    import ctypes

    from tdvc_amd import _lib, ops
    name, N, H, W, sigma, shift, poison = case
    fn = _lib.lib().tdvc_debug_enable_dcn_lds
    fn.argtypes = [ctypes.c_int]
    fn.restype = None
    g = torch.Generator().manual_seed(91)
    x = torch.randn(N, H, W, 64, generator=g)
    om = torch.randn(N, H, W, 216, generator=g)
    om[..., :144] *= sigma
    om[..., 0:144:2] += shift[0]
    om[..., 1:144:2] += shift[1]
    if poison:
        flat = om.view(-1)
        idx = torch.randint(0, flat.numel(), (400,), generator=g)
        flat[idx[:100]] = float("nan")
        flat[idx[100:200]] = float("inf")
        flat[idx[200:300]] = -float("inf")
        flat[idx[300:]] = 60000.0
    xf, omf = ops.FM(x.half().cuda()), ops.FM(om.half().cuda())
    pc = ops.pack_conv(torch.randn(64, 64, 3, 3, generator=g) * 0.05, torch.randn(64, generator=g) * 0.1, stride=1, pad=1, ck=64)
    outs = []
    try:
        for on in (1, 0):
            fn(on)
            y = ops.FM.empty(N, H, W, 64)
            ops.dcn_fused(xf, omf, pc, y, groups=8, act=ops.ACT_LRELU, slope=0.1, planar=False)
            outs.append(y.t.clone())
    finally:
        fn(1)
    a, b = outs
    if poison:
        # a NaN/Inf mask poisons its pixel in both kernels alike; compare bit patterns
        same = torch.equal(a.view(torch.int16), b.view(torch.int16))
    else:
        same = torch.equal(a, b)
        assert bool(torch.isfinite(a).all())
    nbad = int((a.view(torch.int16) != b.view(torch.int16)).sum())
    report(f"dcn_lds {name}: {a.numel()} outputs, {nbad} differ from the gather kernel")
    assert same, f"{nbad} outputs differ"


@pytest.mark.parametrize("cfg", [
    dict(B=2, C=2, Cout=2, H=4, W=4, k=3, s=1, p=1, d=1, G=1, osc=2.0),       # testcpu.py gradcheck geometry
    dict(B=2, C=64, Cout=64, H=12, W=20, k=3, s=1, p=1, d=1, G=8, osc=2.5),   # hot-path geometry
    dict(B=1, C=16, Cout=24, H=11, W=13, k=3, s=2, p=1, d=1, G=4, osc=1.5),
    dict(B=1, C=8, Cout=8, H=9, W=9, k=3, s=1, p=2, d=2, G=2, osc=4.0),
])
def test_ext_backward_vs_oracle(cfg, report):
    """`_ext.dcn_v2_backward` vs the C restatement of the reference's CPU backward kernels"""
    import _ext
    from oracle import dcn_c
    B, C, Cout, H, W, k, s, p, d, G = (cfg[x] for x in ("B", "C", "Cout", "H", "W", "k", "s", "p", "d", "G"))
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = randn(B, C, H, W, seed=12)
    w = randn(Cout, C, k, k, seed=13, scale=0.2)
    b = randn(Cout, seed=14)
    off = randn(B, 2 * G * k * k, Ho, Wo, seed=15, scale=cfg["osc"])
    m = torch.sigmoid(randn(B, G * k * k, Ho, Wo, seed=16))
    gy = randn(B, Cout, Ho, Wo, seed=17)
    want = dcn_c.backward(x, w, b, off, m, gy, k, k, s, s, p, p, d, d, G)
    got = _ext.dcn_v2_backward(x.cuda(), w.cuda(), b.cuda(), off.cuda(), m.cuda(), gy.cuda(), k, k, s, s, p, p, d, d, G)
    assert len(got) == 5
    for name, a, r in zip(("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias"), got, want):
        scale = float(r.abs().max()) + 1e-6
        assert_close(a.cpu(), r, 1e-4, 2e-5 * scale + 1e-6, f"_ext.dcn_v2_backward {name} C={C} {H}x{W}", report)


def test_ext_autograd_function(report):
    """the product-side autograd wrapper (twin of `_DCNv2`, dcn_v2_amp.py:23-119) backpropagates"""
    from tdvc_amd.dcn_ext import dcn_v2_conv
    from oracle import dcn_c
    x = randn(1, 8, 9, 9, seed=18).cuda().requires_grad_()
    w = randn(8, 8, 3, 3, seed=19, scale=0.2).cuda().requires_grad_()
    b = randn(8, seed=20).cuda().requires_grad_()
    off = randn(1, 2 * 2 * 9, 9, 9, seed=21, scale=1.5).cuda().requires_grad_()
    m = torch.sigmoid(randn(1, 2 * 9, 9, 9, seed=22)).cuda().requires_grad_()
    y = dcn_v2_conv(x, off, m, w, b, 1, 1, 1, 2, use_amp=False)
    gy = randn(*y.shape, seed=23).cuda()
    y.backward(gy)
    want = dcn_c.backward(x.detach().cpu(), w.detach().cpu(), b.detach().cpu(), off.detach().cpu(), m.detach().cpu(), gy.cpu(),
                          3, 3, 1, 1, 1, 1, 1, 1, 2)
    for t, r in zip((x, off, m, w, b), want):
        assert_close(t.grad.cpu(), r, 1e-4, 1e-4, "autograd grad", report)
