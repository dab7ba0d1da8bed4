"""conv_wgrad_split_kernel and the training switch ops.f32_split_train, op level, against float64 on the CPU.

Every row of tests/test_conv_wgrad_f32_gpu.py::CASES and tests/helpers_train_model_fp32.py::CONV_CASES, with that test's data, poisoned
padding channels, non-zero destinations and SCALE, under `ops.f32_split_train(True)`:
  (a) the profiled kernel is conv_wgrad_split;
  (b) rms error of dW against float64 <= RATIO x conv_wgrad_f32's on the same inputs (RATIO = tests/test_conv_split_gpu.py's 4: sqrt(6) for
      six times the roundings, the rest for the MFMA's internal summation); the yardstick is the existing kernel;
  (c) db: the same rule, and -- a plain fp32 sum of dY -- the a-priori bound of tests/test_conv_wgrad_f32_gpu.py;
  (d) on the discriminator cases (tests/test_wgrad_split_cases_cpu.py) 3 x the rms error <= the best five-term sum's: a lost product fails;
  (e) two immediate launches and the WgradBatch form are bit-identical;
  (f) the masked 5x5 case fills the masked taps; square_x is the row gdn_1x1_128_128_sq;
  (g) dX through ops.conv_dgrad under the switch: conv_split, rms error <= RATIO x the conv_f32 dgrad's, padding channels untouched;
  (h) fp16 maps, or a mix, are refused by the split entry points before a launch; so is a window without an LDS plan."""
import pytest
import torch

import test_conv_split_gpu as CS
import test_conv_wgrad_f32_gpu as WG
from tests import helpers_conv_split as S
from tests import helpers_train_model_fp32 as H
from tests import helpers_wgrad_split as HW
from util import fm_to_cpu, randn, to_fm

pytestmark = pytest.mark.gpu

RATIO = CS.RATIO
ALL_CASES = list(WG.CASES) + list(H.CONV_CASES)
F32, U, SCALE, POISON = WG.F32, WG.U, WG.SCALE, WG.POISON


def _ops():
    from tdvc_amd import ops
    return ops


def _profiled(ops, fn):
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return [e["kernel"] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_conv_backward_split(case, report):
    ops = _ops()
    name, N, cin, cout, k, stride, pad, Hh, W, shuffle, square_x, masked = case
    x, w, b, live = WG._case_data(case)
    gy, gw, gb, gx, aw, ab, ax, K = WG._reference(case, x, w, b)

    pc = ops.pack_conv(w.cuda(), b.cuda(), stride=stride, pad=pad, shuffle=shuffle, taps=live if masked else None)
    if masked:
        pc.orig["wgrad_taps"] = [(dy, dx) for dy in range(k) for dx in range(k)]
    xf = to_fm(x, ops, dtype=F32)
    xf.t[..., cin:] = POISON
    g = to_fm(gy, ops, dtype=F32)
    if not shuffle:
        g.t[..., cout:] = POISON
    gq = ops.pixel_unshuffle(g) if shuffle else g
    base_w = (randn(w.numel(), seed=405) * 0.05).cuda()
    base_b = (randn(cout, seed=406) * 0.05).cuda()

    def run(split, defer=None):
        dw, db = base_w.clone(), base_b.clone()
        with ops.f32_split_train(split):
            ops.conv_wgrad(pc, gq, xf, dw, scale=SCALE, square_x=square_x, db=db, defer=defer)
            if defer is not None:
                assert len(defer.items) == 1
                defer.flush()
        torch.cuda.synchronize()
        return dw, db

    # (a) the kernel's name, and the existing kernel's without the switch
    assert _profiled(ops, lambda: run(True)) == ["conv_wgrad_split"]
    assert _profiled(ops, lambda: run(False)) == ["conv_wgrad_f32"]
    assert not ops.F32_SPLIT_TRAIN

    dws, dbs = run(True)
    dwf, dbf = run(False)
    ref_w = SCALE * gw + base_w.cpu().double().view(gw.shape)
    ref_b = SCALE * gb + base_b.cpu().double()
    # (b) dW
    es, ef = S.rms(dws.cpu().view(gw.shape).double() - ref_w), S.rms(dwf.cpu().view(gw.shape).double() - ref_w)
    report(f"wgrad split {name}: K={K} dW rms error vs float64 {es:.3e}, conv_wgrad_f32 {ef:.3e}, ratio {es / ef:.2f}")
    assert float((dws - base_w).abs().max()) > 0
    assert es <= RATIO * ef, f"wgrad split {name}: dW rms error {es:.3e} is {es / ef:.2f} x conv_wgrad_f32's {ef:.3e} (gate {RATIO})"
    # (c) db
    bs_, bf_ = S.rms(dbs.cpu().double() - ref_b), S.rms(dbf.cpu().double() - ref_b)
    rb = WG._ratio(dbs.cpu(), ref_b, (K + 3) * U * ab * SCALE + U * ref_b.abs())
    report(f"wgrad split {name}: db rms error {bs_:.3e}, conv_wgrad_f32 {bf_:.3e}, ratio {bs_ / max(bf_, 1e-300):.2f}; max |db - db64| / bound = {rb:.4f}")
    assert bs_ <= RATIO * bf_, f"wgrad split {name}: db rms error {bs_:.3e} is {bs_ / max(bf_, 1e-300):.2f} x conv_wgrad_f32's {bf_:.3e}"
    assert rb <= 1.0, f"bgrad split {name}: {rb} x the a-priori bound"
    # (d) a lost second-order product
    if name in HW.DISCRIMINATORS:
        exact = HW.wgrad_exact(case, x, gy, tuple(w.shape))
        assert torch.equal(exact, gw)
        five = min(S.rms(SCALE * (HW.wgrad_terms(case, x, gy, t, tuple(w.shape)) - exact)) for t in S.five_term_sets())
        report(f"wgrad split {name}: best five-term sum's rms error {five:.3e} = {five / es:.1f} x the kernel's")
        assert 3 * es <= five, f"wgrad split {name}: rms error {es:.3e} is within 3 x of a five-term sum's ({five:.3e})"
    # (e) reproducible, and the deferred second stage gives the same bits
    dw2, db2 = run(True)
    assert torch.equal(dws, dw2) and torch.equal(dbs, db2), f"{name}: two immediate launches differ"
    dw3, db3 = run(True, ops.WgradBatch())
    assert torch.equal(dws, dw3) and torch.equal(dbs, db3), f"{name}: the WgradBatch form differs from the immediate form"
    # (f) the masked taps carry a gradient
    if masked:
        got = (dws - base_w).cpu().view(gw.shape)[:, :, k - 1, k - 1]
        assert float(gw[:, :, k - 1, k - 1].abs().max()) > 0 and float(got.abs().max()) > 0
        assert S.rms(got.double() - SCALE * gw[:, :, k - 1, k - 1]) <= 1e-4 * S.rms(SCALE * gw[:, :, k - 1, k - 1])

    # (g) the data gradient: conv_split on the dgrad packing, onto a non-zero map
    base_x = randn(N, cin, Hh, W, seed=407) * 0.1
    ref_x = gx + base_x.double()

    def dgrad(split):
        dx = to_fm(base_x, ops, dtype=F32)
        dx.t[..., cin:] = 3.0
        with ops.f32_split_train(split):
            kern = _profiled(ops, lambda: ops.conv_dgrad(pc, gq, dx, accumulate=True))
        assert torch.equal(dx.t[..., cin:], torch.full_like(dx.t[..., cin:], 3.0)), f"dgrad {name}: padding channels of dX written"
        return kern, S.rms(fm_to_cpu(dx, cin).double() - ref_x)

    ks_, xs_ = dgrad(True)
    kf_, xf_ = dgrad(False)
    assert ks_ == ["conv_split"] and kf_ == ["conv_f32"], (ks_, kf_)
    report(f"dgrad split {name}: dX rms error vs float64 {xs_:.3e}, conv_f32 {xf_:.3e}, ratio {xs_ / xf_:.2f}")
    assert xs_ <= RATIO * xf_, f"dgrad split {name}: rms error {xs_:.3e} is {xs_ / xf_:.2f} x conv_f32's {xf_:.3e} (gate {RATIO})"


def test_inf_behind_the_border_and_in_padding_channels():
    """tests/test_conv_split_gpu.py's construction: a stride-2 3x3 layer with the single tap (0, 0) reads only odd rows and columns, and row 0 /
    column 0 are what the CLAMPED addresses of its out-of-image pixels point at.  Inf there, and Inf in the padding channels of both maps
    (20 of 24 ci, 36 of 40 co), must contribute exact zeros: mask and select come before the split"""
    ops = _ops()
    cin, cout = 20, 36
    x, gy = randn(1, cin, 9, 9, seed=431), randn(1, cout, 5, 5, seed=432) * 0.5
    w = randn(cout, cin, 3, 3, seed=433) * 0.1
    pc = ops.pack_conv(w.cuda(), None, stride=2, pad=1, taps=[(0, 0)])
    xi = x.clone()
    xi[:, :, 0, :] = float("inf")
    xi[:, :, :, 0] = float("-inf")
    outs = []
    for xs, poison in ((x, 0.0), (xi, float("inf"))):
        xf, g = to_fm(xs, ops, dtype=F32), to_fm(gy, ops, dtype=F32)
        assert xf.C == 24 and g.C == 40
        xf.t[..., cin:] = poison
        g.t[..., cout:] = poison
        dw, db = torch.zeros(w.numel(), device="cuda"), torch.zeros(cout, device="cuda")
        with ops.f32_split_train(True):
            ops.conv_wgrad(pc, g, xf, dw, db=db)
        torch.cuda.synchronize()
        outs.append((dw, db))
    (dw0, db0), (dw1, db1) = outs
    assert float(dw0.abs().max()) > 0 and bool(torch.isfinite(dw1).all()) and bool(torch.isfinite(db1).all())
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    ref = torch.einsum("noyx,ncyx->oc", gy.double(), torch.nn.functional.pad(x.double(), (1, 0, 1, 0))[:, :, 0:9:2, 0:9:2])
    got = dw0.cpu().view(cout, cin, 3, 3)
    assert S.rms(got[:, :, 0, 0].double() - ref) <= 1e-5 * S.rms(ref) and float(got[:, :, 1:, :].abs().max()) == 0.0


def test_split_entry_points_refuse_fp16_maps(report):
    """fp16 maps, or a mix, at tdvc_conv_wgrad_bias_split / tdvc_conv_wgrad_partials_split: an error status with a message, nothing launched"""
    ops = _ops()
    from tdvc_amd import _lib as L
    w = randn(64, 64, 3, 3, seed=411) * 0.05
    pc = ops.pack_conv(w.cuda(), None, stride=1, pad=1)
    x, gy = randn(1, 64, 9, 11, seed=412), randn(1, 64, 9, 11, seed=413)
    o = pc.orig
    for gd, xd in ((torch.float16, F32), (F32, torch.float16), (torch.float16, torch.float16)):
        g, xf = to_fm(gy, ops, dtype=gd), to_fm(x, ops, dtype=xd)
        dw = torch.full((w.numel(),), 0.25, device="cuda")
        tb, static, nwork = ops._wgrad_static(pc, xf.C, xf.N, g.H, g.W, o["taps"])
        work = torch.empty((nwork,), dtype=torch.float32, device="cuda")
        args = (g, xf, *static, 0, 1.0, dw, None, None, work, nwork)
        with pytest.raises(L.TdvcHipError, match="both fmaps must be fp32"):
            ops.launch("tdvc_conv_wgrad_bias_split", *args)
        with pytest.raises(L.TdvcHipError, match="both fmaps must be fp32"):
            ops.launch("tdvc_conv_wgrad_partials_split", *args, L.WgradReduceJob())
        torch.cuda.synchronize()
        assert torch.equal(dw, torch.full_like(dw, 0.25)), "a refused call wrote dW"
    # through the operator under the switch: an fp32 X with an fp16 dY reaches the split entry point and is refused; fp16 maps are not affected
    dw = torch.full((w.numel(),), 0.25, device="cuda")
    with ops.f32_split_train(True):
        batch = ops.WgradBatch()
        with pytest.raises(L.TdvcHipError, match="both fmaps must be fp32"):
            ops.conv_wgrad(pc, to_fm(gy, ops, dtype=torch.float16), to_fm(x, ops, dtype=F32), dw, defer=batch)
        assert not batch.items
        kern = _profiled(ops, lambda: ops.conv_wgrad(pc, to_fm(gy, ops), to_fm(x, ops), dw.clone()))
    assert kern == ["conv_wgrad"], kern
    assert torch.equal(dw, torch.full_like(dw, 0.25))
    report("conv_wgrad split entry points: fp16 and mixed operands refused before any launch; fp16 maps stay on conv_wgrad under the switch")


def test_window_without_an_lds_plan_is_refused():
    """7x7 stride 2 is in no case table: three planes of its X tile need more pieces per thread than the kernel holds; no silent fall-back"""
    ops = _ops()
    from tdvc_amd import _lib as L
    w = randn(64, 32, 7, 7, seed=421) * 0.02
    pc = ops.pack_conv(w.cuda(), None, stride=2, pad=3)
    x, gy = randn(1, 32, 12, 14, seed=422), randn(1, 64, 6, 7, seed=423)
    dw = torch.full((w.numel(),), 0.25, device="cuda")
    with ops.f32_split_train(True):
        with pytest.raises(L.TdvcHipError, match="no LDS plan"):
            ops.conv_wgrad(pc, to_fm(gy, ops, dtype=F32), to_fm(x, ops, dtype=F32), dw)
    torch.cuda.synchronize()
    assert torch.equal(dw, torch.full_like(dw, 0.25))
    ops.conv_wgrad(pc, to_fm(gy, ops, dtype=F32), to_fm(x, ops, dtype=F32), dw)          # the fp32 kernel takes it, as before
    torch.cuda.synchronize()
    assert not torch.equal(dw, torch.full_like(dw, 0.25))


def test_abi(report):
    from tdvc_amd import _lib as L
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 18
    assert hasattr(lib, "tdvc_conv_wgrad_bias_split") and hasattr(lib, "tdvc_conv_wgrad_partials_split")
    assert L.SIGNATURES["tdvc_conv_wgrad_bias_split"] == L.SIGNATURES["tdvc_conv_wgrad_bias"]
    assert L.SIGNATURES["tdvc_conv_wgrad_partials_split"] == L.SIGNATURES["tdvc_conv_wgrad_partials"]
