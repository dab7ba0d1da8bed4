"""Conv backward (data / weight / bias gradients) vs torch autograd in fp32 on the same fp16-rounded operands."""
import pytest
import torch
import torch.nn.functional as F

from util import assert_close, fm_to_cpu, randn, rnd16, to_fm

pytestmark = pytest.mark.gpu


def _ops():
    from tdvc_amd import ops
    return ops


CASES = [
    # name, N, cin, cout, k, stride, pad, H, W, shuffle
    ("3x3_64_64", 2, 64, 64, 3, 1, 1, 40, 72, False),
    ("3x3_64_64_large", 1, 64, 64, 3, 1, 1, 96, 128, False),       # dgrad on the LDS-DMA kernel
    ("3x3_3_64", 2, 3, 64, 3, 1, 1, 33, 47, False),
    ("3x3_128_192", 1, 128, 192, 3, 1, 1, 17, 30, False),
    ("1x1_128_64", 2, 128, 64, 1, 1, 0, 20, 36, False),
    ("7x7_8_32", 1, 8, 32, 7, 1, 3, 34, 60, False),
    ("7x7_32_16", 1, 32, 16, 7, 1, 3, 19, 25, False),
    ("3x3_s2_64_128", 2, 64, 128, 3, 2, 1, 32, 48, False),         # space-to-depth forward, sub-pixel dgrad
    ("1x1_s2_64_128", 1, 64, 128, 1, 2, 0, 32, 64, False),
    ("subpel_128_64", 1, 128, 256, 3, 1, 1, 12, 20, True),          # conv + PixelShuffle(2)
    # training-step geometries: the entropy-parameter 1x1 chain (channel counts not multiples of 8: padded g / x channels),
    # conv_offset_mask, the 64->3 heads, the coder's 128-channel layers, the 256->64 fusion
    ("1x1_512_426", 2, 512, 426, 1, 1, 0, 5, 7, False),
    ("1x1_426_341", 2, 426, 341, 1, 1, 0, 5, 7, False),
    ("1x1_341_256", 2, 341, 256, 1, 1, 0, 5, 7, False),
    ("3x3_64_216", 2, 64, 216, 3, 1, 1, 13, 19, False),
    ("3x3_64_3", 2, 64, 3, 3, 1, 1, 15, 21, False),
    ("3x3_128_128", 2, 128, 128, 3, 1, 1, 11, 14, False),
    ("3x3_s2_128_128", 2, 128, 128, 3, 2, 1, 12, 18, False),
    ("1x1_256_64", 2, 256, 64, 1, 1, 0, 9, 11, False),
    ("3x3_128_64", 2, 128, 64, 3, 1, 1, 11, 14, False),
    ("3x3_192_256", 2, 192, 256, 3, 1, 1, 7, 9, False),
    ("3x3_s2_64_64", 2, 64, 64, 3, 2, 1, 14, 18, False),
    ("1x1_s2_128_128", 2, 128, 128, 1, 2, 0, 12, 18, False),
    ("subpel_128_128", 1, 128, 512, 3, 1, 1, 6, 9, True),
    ("subpel_192_192", 1, 192, 768, 3, 1, 1, 5, 7, True),
    # SPyNet's 7x7 stack
    ("7x7_32_64", 1, 32, 64, 7, 1, 3, 15, 19, False),
    ("7x7_64_32", 1, 64, 32, 7, 1, 3, 15, 19, False),
    ("7x7_16_2", 2, 16, 2, 7, 1, 3, 13, 17, False),
]

POISON = 1.0e4           # padding channels of g and x are don't-care inputs: large finite values must not reach any real output


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_backward(case, report):
    ops = _ops()
    name, N, cin, cout, k, stride, pad, H, W, shuffle = case
    x = rnd16(randn(N, cin, H, W, seed=101))
    w = rnd16(randn(cout, cin, k, k, seed=102) * (1.0 / (cin * k * k) ** 0.5))
    b = randn(cout, seed=103) * 0.1
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(xr, wr, br, stride=stride, padding=pad)
    if shuffle:
        y = F.pixel_shuffle(y, 2)
    gy = rnd16(randn(*y.shape, seed=104) * 0.5)
    gx, gw, gb = torch.autograd.grad(y, (xr, wr, br), gy)

    wd, bd = w.cuda(), b.cuda()
    pc = ops.pack_conv(wd, bd, stride=stride, pad=pad, shuffle=shuffle)
    xf = to_fm(x, ops)
    # channel padding contract (convpack row / channel masks): the packed weights of padding channels are zero, so the padding
    # channels of x (forward, weight gradient) and of g (data and weight gradient) are read but never contribute
    xf.t[..., cin:] = POISON
    yf = ops.conv(xf, pc)
    assert_close(fm_to_cpu(yf, y.shape[1]), y.detach(), 2e-3, 2e-3, f"fwd {name}", report)
    g = to_fm(gy, ops)
    if not shuffle:
        g.t[..., cout:] = POISON
    gq = ops.pixel_unshuffle(g) if shuffle else g
    # data gradient, accumulated onto a non-zero buffer
    base = rnd16(randn(N, cin, H, W, seed=105) * 0.1)
    dx = to_fm(base, ops)
    dx.t[..., cin:] = 3.0
    ops.conv_dgrad(pc, gq, dx, accumulate=True)
    scale = float(gx.abs().max())
    assert_close(fm_to_cpu(dx, cin), gx + base, 3e-3, 3e-3 * max(1.0, scale), f"dgrad {name}", report)
    # the padding channels of dX are the dgrad conv's zero rows: an accumulating call leaves them as they were
    assert torch.equal(dx.t[..., cin:], torch.full_like(dx.t[..., cin:], 3.0)), f"dgrad {name}: padding channels of dX written"
    # weight / bias gradients accumulate into fp32 buffers
    dw = torch.full_like(wd, 0.25)
    db = torch.full_like(bd, -0.5)
    ops.conv_wgrad(pc, gq, xf, dw)
    ops.conv_bgrad(pc, gq, db)
    tol_w = 2e-3 * float(gw.abs().max()) + 1e-3
    assert_close(dw.cpu() - 0.25, gw, 2e-3, tol_w, f"wgrad {name}", report)
    assert_close(db.cpu() + 0.5, gb, 2e-3, 2e-3 * float(gb.abs().max()) + 1e-3, f"bgrad {name}", report)
    # bitwise reproducible; the fused form (bias gradient from the same launch) gives the same dW and a matching db
    dw2 = torch.full_like(wd, 0.25)
    db2 = torch.full_like(bd, -0.5)
    ops.conv_wgrad(pc, gq, xf, dw2, db=db2)
    assert torch.equal(dw, dw2)
    assert_close(db2.cpu() + 0.5, gb, 2e-3, 2e-3 * float(gb.abs().max()) + 1e-3, f"fused bgrad {name}", report)
    db3 = torch.full_like(bd, -0.5)
    ops.conv_wgrad(pc, gq, xf, torch.zeros_like(wd), db=db3)
    assert torch.equal(db2, db3)


def test_repack_follows_parameter_updates(report):
    """PackedConv references the device parameter: an in-place update + repack() changes forward and dgrad"""
    ops = _ops()
    w = torch.nn.Parameter(rnd16(randn(64, 64, 3, 3, seed=111) * 0.05).cuda())
    b = torch.nn.Parameter((randn(64, seed=112) * 0.1).cuda())
    pc = ops.pack_conv(w, b, stride=1, pad=1)
    x = rnd16(randn(1, 64, 24, 40, seed=113))
    xf = to_fm(x, ops)
    y0 = fm_to_cpu(ops.conv(xf, pc))
    g = to_fm(rnd16(randn(1, 64, 24, 40, seed=114)), ops)
    dx0 = fm_to_cpu(ops.conv_dgrad(pc, g, ops.FM.zeros(1, 24, 40, 64), accumulate=False))
    with torch.no_grad():
        w.mul_(0.5)
        b.add_(1.0)
    pc.repack()
    y1 = fm_to_cpu(ops.conv(xf, pc))
    dx1 = fm_to_cpu(ops.conv_dgrad(pc, g, ops.FM.zeros(1, 24, 40, 64), accumulate=False))
    ref = F.conv2d(x, w.detach().cpu(), b.detach().cpu(), padding=1)
    assert_close(y1, ref, 2e-3, 2e-3, "forward after repack", report)
    assert_close(dx1, 0.5 * dx0, 2e-3, 2e-3, "dgrad after repack", report)
    assert not torch.allclose(y0, y1)


def test_pack_batch_equals_per_layer_repack(report):
    """the one-launch re-pack of many layers (forward + dgrad forms, biases incl. the sub-pixel row order) writes
    exactly the bytes the per-layer repack() writes"""
    ops = _ops()
    geo = [(64, 64, 3, 1, 1, False), (128, 64, 3, 2, 1, False), (64, 128, 1, 1, 0, False), (256, 64, 3, 1, 1, True),
           (32, 64, 7, 1, 3, False), (64, 8, 3, 1, 1, False)]
    layers = []
    for i, (co, ci, k, s_, pd, shuf) in enumerate(geo):
        w = torch.nn.Parameter((randn(co, ci, k, k, seed=300 + i) * 0.05).cuda())
        b = torch.nn.Parameter((randn(co, seed=320 + i) * 0.1).cuda())
        pc = ops.pack_conv(w, b, stride=s_, pad=pd, shuffle=shuf)
        g = to_fm(rnd16(randn(1, co, 32 // s_, 64 // s_, seed=340 + i)), ops)
        layers.append((w, b, pc))
        ops.conv_dgrad(pc, g, ops.FM.zeros(1, 32, 64, max(ci, 8)), accumulate=False)      # builds the dgrad form
    batch = ops.PackBatch([pc for _, _, pc in layers])
    assert len(batch.pcs) >= len(layers)
    with torch.no_grad():
        for w, b, _ in layers:
            w.mul_(0.7).add_(0.01)
            b.sub_(0.3)
    for _, _, pc in layers:
        pc.repack()
    want = [(pc.w.clone(), None if pc.bias is None else pc.bias.clone()) for pc in batch.pcs]
    for pc in batch.pcs:
        pc.w.zero_()
        if pc.bsrc is not None:
            pc.bias.zero_()
    batch.run()
    torch.cuda.synchronize()
    for pc, (w0, b0) in zip(batch.pcs, want):
        assert torch.equal(pc.w, w0)
        if pc.bsrc is not None:
            assert torch.equal(pc.bias, b0)
    report(f"pack batch: {len(batch.pcs)} packed forms in {batch.total_blocks} blocks, bytes identical to repack()")


def test_act_backward_and_unshuffle(report):
    ops = _ops()
    y = rnd16(randn(2, 64, 9, 13, seed=121))
    r = rnd16(randn(2, 64, 9, 13, seed=122))
    g = rnd16(randn(2, 64, 9, 13, seed=123))
    out = ops.act_backward(to_fm(g, ops), to_fm(y, ops), ops.ACT_LRELU, 0.1, res=to_fm(r, ops), out=ops.FM.empty(2, 9, 13, 64))
    ref = torch.where(y - r > 0, g, rnd16(g * 0.1))
    assert_close(fm_to_cpu(out), ref, 1e-3, 1e-3, "act_backward lrelu + residual", report)
    out = ops.act_backward(to_fm(g, ops), to_fm(y, ops), ops.ACT_RELU)
    assert_close(fm_to_cpu(out), torch.where(y > 0, g, torch.zeros_like(g)), 0, 0, "act_backward relu", report)
    z = rnd16(randn(1, 16, 8, 10, seed=124))
    u = fm_to_cpu(ops.pixel_unshuffle(to_fm(z, ops)))
    assert torch.equal(u, z.view(1, 16, 4, 2, 5, 2).permute(0, 3, 5, 1, 2, 4).reshape(1, 64, 4, 5))


def _wgrad_tol(gw):
    return 2e-3 * float(gw.abs().max()) + 1e-3


def test_masked_5x5_context_conv_backward(report):
    """the masked (type A) 5x5 128->256 context conv: dX is the adjoint of the conv with the masked weight, dW covers all 25 taps
    (compressai multiplies the weight by the mask in the forward; autograd of F.conv2d(x, w_masked) still fills the masked taps)"""
    ops = _ops()
    N, H, W = 2, 11, 13
    x = rnd16(randn(N, 128, H, W, seed=131))
    w = rnd16(randn(256, 128, 5, 5, seed=132) * (1.0 / (128 * 12) ** 0.5))
    b = randn(256, seed=133) * 0.1
    live = [(dy, dx) for dy in range(5) for dx in range(5) if dy < 2 or (dy == 2 and dx < 2)]
    mask = torch.zeros(5, 5)
    for dy, dx in live:
        mask[dy, dx] = 1.0
    xr, wm, br = x.clone().requires_grad_(), (w * mask).requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(xr, wm, br, padding=2)
    gy = rnd16(randn(*y.shape, seed=134) * 0.5)
    gx, gw, gb = torch.autograd.grad(y, (xr, wm, br), gy)
    assert float(gw[:, :, 4, 4].abs().max()) > 0
    pc = ops.pack_conv((w * mask).cuda(), b.cuda(), stride=1, pad=2, taps=live)
    pc.orig["wgrad_taps"] = [(dy, dx) for dy in range(5) for dx in range(5)]        # as coder.ctx_conv builds it
    xf, g = to_fm(x, ops), to_fm(gy, ops)
    assert_close(fm_to_cpu(ops.conv(xf, pc), 256), y.detach(), 2e-3, 2e-3, "fwd masked 5x5", report)
    base = rnd16(randn(N, 128, H, W, seed=135) * 0.1)
    dx = to_fm(base, ops)
    ops.conv_dgrad(pc, g, dx, accumulate=True)
    assert_close(fm_to_cpu(dx, 128), gx + base, 3e-3, 3e-3 * max(1.0, float(gx.abs().max())), "dgrad masked 5x5", report)
    dw = torch.full((256 * 128 * 25,), 0.25, device="cuda")
    db = torch.full((256,), -0.5, device="cuda")
    ops.conv_wgrad(pc, g, xf, dw, db=db)
    assert_close(dw.cpu().view(256, 128, 5, 5) - 0.25, gw, 2e-3, _wgrad_tol(gw), "wgrad masked 5x5 (all 25 taps)", report)
    assert_close(db.cpu() + 0.5, gb, 2e-3, _wgrad_tol(gb), "bgrad masked 5x5", report)


def test_temporal_conv3d_backward(report):
    """Conv3d (3,1,1) stride 3, 64 -> 64, as it runs: a 1x1 192 -> 64 conv over three frame slices (WeightLayout.conv3d_temporal)
    whose input is the first 192 channels of a 256-channel buffer; dX lands in the same slice of a 256-channel gradient buffer"""
    ops = _ops()
    from tdvc_amd import convpack
    N, H, W = 2, 9, 14
    x256 = rnd16(randn(N, 256, H, W, seed=141))
    w = rnd16(randn(64, 64, 3, 1, 1, seed=142) * (1.0 / 192 ** 0.5))
    b = randn(64, seed=143) * 0.1
    xr, wr, br = x256[:, :192].clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = F.conv2d(xr, wr.permute(0, 2, 1, 3, 4).reshape(64, 192, 1, 1), br)          # input channel t * 64 + c <-> w[:, c, t]
    gy = rnd16(randn(*y.shape, seed=144) * 0.5)
    gx, gw, gb = torch.autograd.grad(y, (xr, wr, br), gy)
    pc = ops.pack_conv(w.cuda(), b.cuda(), stride=1, pad=0, layout=convpack.WeightLayout.conv3d_temporal(64, 64, 3))
    xbuf = to_fm(x256, ops)
    xf = xbuf.ch(0, 192)
    assert xf.sp > xf.C
    assert_close(fm_to_cpu(ops.conv(xf, pc), 64), y.detach(), 2e-3, 2e-3, "fwd temporal conv3d", report)
    g = to_fm(gy, ops)
    base = rnd16(randn(N, 256, H, W, seed=145) * 0.1)
    dbuf = to_fm(base, ops)
    ops.conv_dgrad(pc, g, dbuf.ch(0, 192), accumulate=True)
    got = fm_to_cpu(dbuf)
    assert_close(got[:, :192], gx + base[:, :192], 3e-3, 3e-3 * max(1.0, float(gx.abs().max())), "dgrad temporal conv3d", report)
    assert torch.equal(got[:, 192:], base[:, 192:]), "dgrad wrote outside its channel slice"
    dw = torch.full((64 * 64 * 3,), 0.25, device="cuda")
    db = torch.full((64,), -0.5, device="cuda")
    ops.conv_wgrad(pc, g, xf, dw, db=db)
    assert_close(dw.cpu().view(64, 64, 3, 1, 1) - 0.25, gw, 2e-3, _wgrad_tol(gw), "wgrad temporal conv3d", report)
    assert_close(db.cpu() + 0.5, gb, 2e-3, _wgrad_tol(gb), "bgrad temporal conv3d", report)


def _layer(ops, cout, cin, k, pad, seed):
    w = rnd16(randn(cout, cin, k, k, seed=seed) * (1.0 / (cin * k * k) ** 0.5))
    b = randn(cout, seed=seed + 1) * 0.1
    return w, b, ops.pack_conv(w.cuda(), b.cuda(), stride=1, pad=pad)


def test_wgrad_loss_scale(report):
    """conv_wgrad(scale=s) with s = 1/128 (Tape.inv_scale): dW += s * G and db += s * Gb, bit for bit (s is a power of two)"""
    ops = _ops()
    N, H, W = 2, 13, 22
    w, b, pc = _layer(ops, 64, 64, 3, 1, 151)
    x, g = to_fm(rnd16(randn(N, 64, H, W, seed=153)), ops), to_fm(rnd16(randn(N, 64, H, W, seed=154)), ops)
    dw1, db1 = torch.zeros(w.numel(), device="cuda"), torch.zeros(64, device="cuda")
    ops.conv_wgrad(pc, g, x, dw1, db=db1)
    s = 1.0 / 128
    bw, bb = (randn(w.numel(), seed=155) * 0.01).cuda(), (randn(64, seed=156) * 0.01).cuda()
    dws, dbs = bw.clone(), bb.clone()
    ops.conv_wgrad(pc, g, x, dws, scale=s, db=dbs)
    assert torch.equal(dws, bw + s * dw1) and torch.equal(dbs, bb + s * db1)
    assert float((dws - bw).abs().max()) > 0
    report("conv_wgrad scale 1/128: bit-identical to 1/128 x the unscaled gradient")


def test_wgrad_batch_equals_immediate(report):
    """WgradBatch (conv_wgrad(defer=...) + flush): five jobs over three layers, two jobs on each of two dW tensors, one job with db;
    torch.equal with the immediate per-layer launches in the same order, and against the float64 reference"""
    ops = _ops()
    N, H, W = 2, 11, 17
    layers = [_layer(ops, 64, 64, 3, 1, 161), _layer(ops, 64, 128, 1, 0, 163), _layer(ops, 32, 8, 7, 3, 165)]
    pads = [1, 0, 3]
    order = [(0, 0, False), (1, 1, True), (0, 2, False), (2, 3, False), (1, 4, False)]        # (layer, job seed, with db)
    data = []
    for li, js, _ in order:
        w, _, _ = layers[li]
        x = rnd16(randn(N, w.shape[1], H, W, seed=170 + js))
        gy = rnd16(randn(N, w.shape[0], H, W, seed=180 + js) * 0.5)
        data.append((x, gy, to_fm(x, ops), to_fm(gy, ops)))
    bases = [(randn(w.numel(), seed=190 + i) * 0.01).cuda() for i, (w, _, _) in enumerate(layers)]
    dbase = (randn(64, seed=195) * 0.01).cuda()

    def run(defer):
        dws = [t.clone() for t in bases]
        db = dbase.clone()
        for (li, _, with_db), (_, _, xf, gf) in zip(order, data):
            ops.conv_wgrad(layers[li][2], gf, xf, dws[li], db=db if with_db else None, defer=defer)
        if defer is not None:
            assert len(defer.items) == len(order)
            defer.flush()
        torch.cuda.synchronize()
        return dws, db

    dws_b, db_b = run(ops.WgradBatch())
    dws_i, db_i = run(None)
    for li in range(3):
        assert torch.equal(dws_b[li], dws_i[li]), f"batched dW of layer {li} differs from the immediate form"
    assert torch.equal(db_b, db_i)
    refs = [torch.zeros_like(w, dtype=torch.float64) for w, _, _ in layers]
    dbr = torch.zeros(64, dtype=torch.float64)
    for (li, _, with_db), (x, gy, _, _) in zip(order, data):
        w, b, _ = layers[li]
        wr, br = w.double().requires_grad_(), b.double().requires_grad_()
        gw, gb = torch.autograd.grad(F.conv2d(x.double(), wr, br, padding=pads[li]), (wr, br), gy.double())
        refs[li] += gw
        if with_db:
            dbr += gb
    for li, (w, _, _) in enumerate(layers):
        assert_close(dws_b[li].cpu().view(w.shape) - bases[li].cpu().view(w.shape), refs[li], 2e-3, _wgrad_tol(refs[li]), f"WgradBatch layer {li}", report)
    assert_close(db_b.cpu() - dbase.cpu(), dbr, 2e-3, _wgrad_tol(dbr), "WgradBatch db", report)


# ------------------------------------------------------------------------------------------------------------------ coverage guard
MASKED_CLASS = (5, 5, 1, 128, 256, False, False, True)       # test_masked_5x5_context_conv_backward
TEMPORAL_CLASS = (1, 1, 1, 192, 64, False, False, False)     # test_temporal_conv3d_backward


def op_level_wgrad_classes():
    """(kh, kw, stride, cin, cout, shuffle, square_x, masked) of every conv weight gradient that has an op-level test"""
    from test_backward_ops_gpu import WGRAD_CLASSES
    s = {(k, k, st, ci, co, sh, False, False) for (_, _, ci, co, k, st, _, _, _, sh) in CASES}
    return s | {MASKED_CLASS, TEMPORAL_CLASS} | WGRAD_CLASSES


def test_training_wgrad_geometries_have_op_level_tests(report):
    """one taped forward + backward of the whole model at 1 x 64 x 64: every conv weight-gradient geometry it runs
    (ops.PROFILE's `geo`) must be a row of the op-level case tables, so a new layer shape cannot reach training untested"""
    from tdvc_amd import autograd, synth
    from tdvc_amd.model.pnet import VideoCompressor
    ops = _ops()
    B, H, W = 1, 64, 64
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda().train()
    frames = synth.make_gop(1234, 7, H, W).float()
    x = frames[3:4].cuda()
    refs = torch.stack([frames[0], frames[0], frames[1], frames[2]]).unsqueeze(0).cuda()
    gen = torch.Generator().manual_seed(71)
    u = lambda *s: torch.rand(*s, generator=gen) - 0.5
    mk = lambda: {"z": u(B, 128, H // 64, W // 64), "y": u(B, 128, H // 16, W // 16), "y_lik": u(B, 128, H // 16, W // 16)}
    noise = {k: {kk: to_fm(v, ops, Cpad=128, dtype=torch.float32) for kk, v in mk().items()} for k in ("mv", "res")}
    ops.PROFILE = []
    try:
        with autograd.record() as tape:
            r, _, _, _, _ = m(x, refs, True, noise=noise)
            tape.grad_tensor(r).copy_((r - x) * (2.0 / r.numel()))
            tape.rate_grad = 1.0 / float(B * H * W)
            tape.backward()
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
    seen = {}
    for e in prof:
        if e["kernel"] == "conv_wgrad":
            seen[e["geo"]] = seen.get(e["geo"], 0) + 1
    tables = op_level_wgrad_classes()
    missing = sorted(set(seen) - tables)
    report(f"wgrad geometry classes of a training step: {len(seen)} ({sum(seen.values())} launches); without an op-level case: {missing}")
    assert len(seen) >= 10
    assert not missing, f"conv weight-gradient geometries without an op-level backward test: {missing}"
