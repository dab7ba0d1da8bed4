"""CPU: the case tables, float64 restatements and counted bounds of tests/helpers_train_model_fp32.py, and the command line / constructor
of the whole-model fp32 training mode, without touching a device.

For every fp32 adjoint form: the restatement equals torch.autograd of the forward operation in float64, and the bound is sensitive --
moving one input by one fp16 ulp (2^-11 relative, every element, random sign) moves the result by more than the bound somewhere.  A bound
that fp16 arithmetic would pass proves nothing."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import helpers_train_model_fp32 as H


def _sensitive(what, ref, moved, bound):
    r = H.ratio(moved, ref, bound)
    assert r > 1.0, f"{what}: one fp16 ulp on an input moves the result by only {r:.3f} x the bound"


def _agree(what, a, b):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= 1e-12 * scale, f"{what}: the restatement differs from torch.autograd in float64"


# ------------------------------------------------------------------------------------------------------------------ point-wise forms
@pytest.mark.parametrize("row", H.AFB_CASES, ids=[r[0] for r in H.AFB_CASES])
def test_add_flow_backward_restatement_and_bound(row):
    name, N, Hh, W, C_, Cb, Cf = row
    doff, dflow = H.afb_data(row)
    want, bound = H.afb_ref(row, doff, dflow)
    fl = dflow.double()[..., :2].clone().requires_grad_()
    y = torch.zeros(N, Hh, W, C_, dtype=torch.float64) + fl.repeat(1, 1, 1, C_ // 2)          # add_flow: off[c] += flow[c & 1]
    (g,) = torch.autograd.grad((y * doff.double()[..., Cb - C_:]).sum(), fl)
    _agree("add_flow_backward", want[..., :2] - dflow.double()[..., :2], g)
    assert torch.equal(want[..., 2:], dflow.double()[..., 2:])
    moved, _ = H.afb_ref(row, H.perturb(doff, name), dflow)
    _sensitive(f"add_flow_backward {name}", want[..., :2], moved[..., :2], bound[..., :2])


@pytest.mark.parametrize("row", H.BCB_CASES, ids=[r[0] for r in H.BCB_CASES])
def test_bcast_add_act_backward_restatement_and_bound(row):
    name, N, Hh, W, Cb, T, lead = row
    x, dx, db = H.bcb_data(row)
    got_dx, got_db, b_dx, b_db = H.bcb_ref(row, x, dx, db)
    # forward: x = lrelu(x_pre + b repeated over the T slices); the stored output has the sign of its argument
    out = x.double()[..., lead:]
    pre = torch.where(out > 0, out, out / 0.1).clone().requires_grad_()
    b = torch.zeros(N, Hh, W, Cb, dtype=torch.float64, requires_grad=True)
    slope = float(torch.tensor(H.BCB_SLOPE, dtype=torch.float32))
    y = F.leaky_relu(pre + b.repeat(1, 1, 1, T), slope)
    g_pre, g_b = torch.autograd.grad((y * dx.double()[..., lead:]).sum(), (pre, b))
    _agree("bcast_add_act_backward dx", got_dx, g_pre)
    _agree("bcast_add_act_backward db", got_db - db.double(), g_b)
    m_dx, m_db, _, _ = H.bcb_ref(row, x, H.perturb(dx, name), db)
    _sensitive(f"bcast_add_act_backward dx {name}", got_dx, m_dx, b_dx)
    _sensitive(f"bcast_add_act_backward db {name}", got_db, m_db, b_db)


@pytest.mark.parametrize("row", H.UPB_CASES, ids=[r[0] for r in H.UPB_CASES])
def test_upsample2x_backward_restatement_and_bound(row):
    name, N, h, w, C_, Cy, Cx = row
    dy, dx0 = H.upb_data(row)
    want, bound = H.upb_ref(row, dy, dx0)
    xr = torch.zeros(N, C_, h, w, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    (g,) = torch.autograd.grad((up * dy.double()[..., Cy - C_:].permute(0, 3, 1, 2)).sum(), xr)
    _agree("upsample2x_backward", want - dx0.double()[..., Cx - C_:], g.permute(0, 2, 3, 1))
    moved, _ = H.upb_ref(row, H.perturb(dy, name), dx0)
    _sensitive(f"upsample2x_backward {name}", want, moved, bound)


@pytest.mark.parametrize("row", H.MGB_CASES, ids=[r[0] for r in H.MGB_CASES])
def test_match_gather_backward_restatement_and_bound(row):
    name, N, Hh, W, scale, view = row
    fin, fref, dcat, dfin0, dfref0, idx = H.mgb_data(row)
    assert scale == 8, "the training scale"
    dfin, dfref, bfin, bref = H.mgb_ref(row, fin, fref, dcat, dfin0, dfref0, idx)
    a, b = fin.double().clone().requires_grad_(), fref.double().clone().requires_grad_()
    ga, gb = torch.autograd.grad((H.mgb_forward(a, b, idx, scale) * dcat.double()).sum(), (a, b))
    _agree("match_gather_backward dfin", dfin - dfin0.double(), ga)
    _agree("match_gather_backward dfref", dfref - dfref0.double(), gb)
    _, ok = H.mgb_source(idx, Hh, W, scale)
    assert (~ok).any() and ok.any(), "the data must reach both the live and the dead (source outside the map) branch"
    for k, moved in enumerate((H.perturb(fin, name, 0), H.perturb(fref, name, 1))):
        args = [fin, fref]
        args[k] = moved.float().double()            # the kernel's input is an fp32 map: the moved values as fp32 numbers
        m_fin, m_ref, _, _ = H.mgb_ref(row, args[0], args[1], dcat, dfin0, dfref0, idx)
        _sensitive(f"match_gather_backward dfin {name} (input {k})", dfin, m_fin, bfin)
        _sensitive(f"match_gather_backward dfref {name} (input {k})", dfref, m_ref, bref)


# ------------------------------------------------------------------------------------------------------------------ DCN backward
def test_dcn_restatement_agrees_with_autograd_of_the_oracle():
    """columns, dx, d offset and d mask logit of <columns, dcol> on a small map with border-crossing offsets"""
    from helpers_dcn import offsets
    N, Hh, W = 1, 6, 7
    g = H.gen("dcn-cpu")
    off = offsets("border", N, Hh, W, 5)
    x = H.draw(g, (N, Hh, W, 64)).double()
    om = torch.cat([off, H.draw(g, (N, Hh, W, 72), 1.5)], -1).double()
    dcol = H.draw(g, (N, Hh, W, 576), 0.5).double()
    ref = H.dcn_bw_ref(x, om, dcol)
    xr, omr = x.clone().requires_grad_(), om.clone().requires_grad_()
    cols = H.dcn_forward_oracle(xr, omr, H.onehot_columns())
    _agree("dcn columns", ref["col"], cols.detach())
    dx, dom = torch.autograd.grad((cols * dcol).sum(), (xr, omr))
    _agree("dcn dx", ref["dx"], dx)
    _agree("dcn dom", ref["dom"], dom)
    assert float(ref["count"].max()) >= 8 and float(ref["count"].min()) >= 0
    assert (ref["dx_abs"] >= ref["dx"].abs() - 1e-12).all() and (ref["dom_abs"] >= ref["dom"].abs() - 1e-12).all()


@pytest.mark.parametrize("regime", ["subpixel", "border", "wild"])
def test_dcn_bounds_are_sensitive(regime):
    assert H.DCN_TILE == 8
    (n1, h1, w1), (n2, h2, w2) = H.DCN_MAPS["sub_tile"], H.DCN_MAPS["tiles_3x3_ragged"]
    assert n1 == n2 == 2 and h1 < H.DCN_TILE and w1 < H.DCN_TILE, "one map smaller than a col2im tile"
    assert h2 > 2 * H.DCN_TILE and w2 > 2 * H.DCN_TILE and h2 % H.DCN_TILE and w2 % H.DCN_TILE, "at least two tiles each way, ragged"
    x, om, dcol, dom0 = H.dcn_data(regime, "sub_tile")
    ref = H.dcn_bw_ref(x, om, dcol)
    want_dom, b_dom = H.dcn_dom_bound(ref, dom0)
    for k, name in enumerate(("x", "dcol", "mask")):
        xx, oo, dd = x.double(), om.double().clone(), dcol.double()
        if k == 0:
            xx = H.perturb(x, regime, k)
        elif k == 1:
            dd = H.perturb(dcol, regime, k)
        else:
            oo[..., 144:] = H.perturb(om[..., 144:], regime, k)
        moved = H.dcn_bw_ref(xx, oo, dd)
        m_dom, _ = H.dcn_dom_bound(moved, dom0)
        if k != 1:
            _sensitive(f"dcn_columns ({name})", ref["col"], moved["col"], H.dcn_col_bound(ref))
        if k != 0:
            _sensitive(f"dcn_col2im dx ({name})", ref["dx"], moved["dx"], H.dcn_dx_bound(ref))
        _sensitive(f"dcn_col2im dom ({name})", want_dom, m_dom, b_dom)


# ------------------------------------------------------------------------------------------------------------------ conv cases
def test_conv_case_table():
    import test_conv_wgrad_f32_gpu as WG
    names = [c[0] for c in H.CONV_CASES]
    assert len(set(names)) == len(names) and all(len(c) == len(WG.CASES[0]) for c in H.CONV_CASES)
    new = H.conv_classes() - WG.op_level_wgrad_f32_classes()
    assert len(new) == len(H.CONV_CASES) + 1, "every row (and the temporal conv) is a geometry class the existing fp32 test does not hold"
    for cls in ((7, 7, 1, 8, 32), (7, 7, 1, 32, 64), (7, 7, 1, 64, 32), (7, 7, 1, 32, 16), (7, 7, 1, 16, 2), (3, 3, 1, 3, 64), (3, 3, 1, 64, 64),
                (3, 3, 1, 128, 64), (3, 3, 1, 64, 216), (3, 3, 2, 64, 64), (1, 1, 1, 128, 64), (1, 1, 1, 256, 64), (1, 1, 1, 192, 64),
                (3, 3, 1, 64, 3)):
        assert cls + (False, False, False) in H.conv_classes(), cls


@pytest.mark.parametrize("case", [c for c in H.CONV_CASES if c[0] in ("7x7_8_32", "3x3_64_3", "3x3_s2_64_64", "1x1_576_64")], ids=lambda c: c[0])
def test_conv_bounds_are_sensitive(case):
    """the bounds of tests/test_conv_wgrad_f32_gpu.py on the new rows: (K + 3) u (|g|^T |x|) + u |dW|, (K + 3) u (|g| * |w|) + u |dX|"""
    name, N, cin, cout, k, stride, pad = case[:7]
    x, w, gy, Kw, Kx = H.conv_ref(case)
    gw, gx = H.conv_grads64(x, w, gy, stride, pad)
    aw, ax = H.conv_grads64(x.abs(), w.abs(), gy.abs(), stride, pad)
    mw, _ = H.conv_grads64(H.perturb(x, name, 0).float(), w, gy, stride, pad)
    _, mx = H.conv_grads64(x, H.perturb(w, name, 1).float(), gy, stride, pad)
    _sensitive(f"conv wgrad {name}", gw, mw, (Kw + 3) * H.EPS32 * aw + H.EPS32 * gw.abs())
    _sensitive(f"conv dgrad {name}", gx, mx, (Kx + 3) * H.EPS32 * ax + H.EPS32 * gx.abs())


# ------------------------------------------------------------------------------------------------------------------ CLI, constructor
def test_model_fp32_flag_parses_and_reaches_train_step():
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.tools.train import make_parser, step_kwargs
    from tdvc_amd.train import TrainStep
    ap = make_parser()
    assert ap.parse_args([]).model_fp32 is False
    assert step_kwargs(ap.parse_args([]))["model_fp32"] is False and step_kwargs(ap.parse_args([]))["loss_scale"] == 128.0
    text = " ".join(ap.format_help().split())
    assert "amp: False" in text and "--model-fp32" in text and "tools/train.py:152-159" in text
    for argv in (["--model-fp32"], ["--model-fp32", "--coder-fp32"]):
        kw = step_kwargs(ap.parse_args(argv + ["--iters", "3"]))
        assert kw["model_fp32"] is True and "loss_scale" not in kw
        m = VideoCompressor()
        step = TrainStep(m, **kw)
        assert m.train_model_fp32 is True and m.train_coder_fp32 is True and step.coder_fp32 is True
        assert step.loss_scale == 1.0 and step.dynamic_scale is False and step.clip == 2.0
    with pytest.raises(ValueError, match="loss_scale"):
        TrainStep(VideoCompressor(), **step_kwargs(ap.parse_args(["--model-fp32", "--loss-scale", "128"])))


def test_train_step_defaults_and_refusals():
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.train import TrainStep
    p = inspect.signature(TrainStep.__init__).parameters
    assert p["model_fp32"].default is False and p["coder_fp32"].default is False
    m = VideoCompressor()
    assert m.train_model_fp32 is False and m.model_fp32 is False
    step = TrainStep(m)
    assert m.train_model_fp32 is False and step.loss_scale == 1024.0 and step.dynamic_scale is True        # the default step is what it was
    for kw, what in ((dict(loss_scale=128.0), "loss_scale"), (dict(dynamic_scale=True), "dynamic_scale"), (dict(graph=True), "graph=True")):
        m = VideoCompressor()
        with pytest.raises(ValueError, match=what):
            TrainStep(m, model_fp32=True, **kw)
        assert m.train_model_fp32 is False, "a refused constructor must not switch the model"
    assert TrainStep(VideoCompressor(), model_fp32=True, loss_scale=1.0, dynamic_scale=False).loss_scale == 1.0


def test_model_fp32_alone_still_refuses_training():
    """no device needed: the refusal comes before the first launch"""
    from tdvc_amd.model.pnet import VideoCompressor
    m = VideoCompressor().train()
    m.model_fp32 = True
    with pytest.raises(ValueError, match="inference / coding mode"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 4, 3, 64, 64), True)
    m.train_model_fp32 = True
    with pytest.raises(RuntimeError, match="HIP device only"):            # the new flag lifts the refusal: the next check is the device's
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 4, 3, 64, 64), True)
