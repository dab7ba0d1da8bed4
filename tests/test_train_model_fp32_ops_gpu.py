"""The fp32 adjoint forms of the whole-model fp32 training mode (VideoCompressor.train_model_fp32), op level, against float64 on the CPU.
Case tables, restatements and counted bounds: tests/helpers_train_model_fp32.py (checked without a GPU by
tests/test_train_model_fp32_cases_cpu.py).  Every map is an fp32 map with full fp32 mantissas; accumulating entry points start from a
non-zero buffer; views are channel slices of wider buffers (the `cat` geometry), whose other channels must come back untouched."""
import pytest
import torch

import helpers_train_model_fp32 as H
import test_conv_wgrad_f32_gpu as WG
from helpers_dcn import DCN_REGIMES, far_stats

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENT = 7.25                 # what a byte the call must not write holds before and after


def _ops():
    from tdvc_amd import ops
    return ops


def _fm(t, ops, c0=0, C_=None):
    """NHWC cpu tensor -> an fp32 FM over a device copy (channels c0 .. c0 + C_ as a view)"""
    d = t.to(F32).cuda().contiguous()
    fm = ops.FM(d)
    return fm if (c0 == 0 and C_ is None) else fm.ch(c0, fm.C - c0 if C_ is None else C_)


def _check(what, got, want, bound, report):
    r = H.ratio(got, want, bound)
    report(f"{what}: max |got - float64| / bound = {r:.4f}")
    assert r <= 1.0, f"{what}: {r} x the bound"


# ------------------------------------------------------------------------------------------------------------------ point-wise forms
@pytest.mark.parametrize("row", H.AFB_CASES, ids=[r[0] for r in H.AFB_CASES])
def test_add_flow_backward_f32(row, report):
    ops = _ops()
    name, N, Hh, W, C_, Cb, Cf = row
    doff, dflow = H.afb_data(row)
    want, bound = H.afb_ref(row, doff, dflow)
    d, f = _fm(doff, ops, Cb - C_), _fm(dflow, ops)
    ops.add_flow_backward(d, f)
    torch.cuda.synchronize()
    _check(f"add_flow_backward f32 {name}", f.t.cpu(), want, bound, report)
    assert torch.equal(d.t.cpu(), doff), "add_flow_backward wrote its input"


@pytest.mark.parametrize("row", H.BCB_CASES, ids=[r[0] for r in H.BCB_CASES])
def test_bcast_add_act_backward_f32(row, report):
    ops = _ops()
    name, N, Hh, W, Cb, T, lead = row
    x, dx, db = H.bcb_data(row)
    w_dx, w_db, b_dx, b_db = H.bcb_ref(row, x, dx, db)
    xf, dxf, dbf = _fm(x, ops, lead), _fm(dx, ops, lead), _fm(db, ops)
    ops.bcast_add_act_backward(dxf, xf, dbf, H.BCB_SLOPE)
    torch.cuda.synchronize()
    _check(f"bcast_add_act_backward f32 dx {name}", dxf.t.cpu()[..., lead:], w_dx, b_dx, report)
    _check(f"bcast_add_act_backward f32 db {name}", dbf.t.cpu(), w_db, b_db, report)
    assert torch.equal(dxf.t.cpu()[..., :lead], dx[..., :lead]), "channels in front of the view were written"


@pytest.mark.parametrize("row", H.UPB_CASES, ids=[r[0] for r in H.UPB_CASES])
def test_upsample2x_backward_f32(row, report):
    ops = _ops()
    name, N, h, w, C_, Cy, Cx = row
    dy, dx0 = H.upb_data(row)
    want, bound = H.upb_ref(row, dy, dx0)
    dyf, dxf = _fm(dy, ops, Cy - C_), _fm(dx0, ops, Cx - C_)
    ops.upsample2x_backward(dyf, dxf)
    torch.cuda.synchronize()
    _check(f"upsample2x_backward f32 {name}", dxf.t.cpu()[..., Cx - C_:], want, bound, report)
    assert torch.equal(dxf.t.cpu()[..., :Cx - C_], dx0[..., :Cx - C_]), "channels in front of the view were written"


@pytest.mark.parametrize("row", H.MGB_CASES, ids=[r[0] for r in H.MGB_CASES])
def test_match_gather_backward_f32(row, report):
    """scale 8 (the training scale) on the smallest legal map and on a ragged fold grid; fin / fref / dcat / dfin / dfref all fp32"""
    ops = _ops()
    name, N, Hh, W, scale, view = row
    fin, fref, dcat, dfin0, dfref0, idx = H.mgb_data(row)
    w_fin, w_ref, b_fin, b_ref = H.mgb_ref(row, fin, fref, dcat, dfin0, dfref0, idx)
    if view:                                                # [fin | fref] and [dfin | dfref] as halves of 128-channel buffers
        both, dboth = _fm(torch.cat([fin, fref], -1), ops), _fm(torch.cat([dfin0, dfref0], -1), ops)
        f_in, f_ref, d_in, d_ref = both.ch(0, 64), both.ch(64, 64), dboth.ch(0, 64), dboth.ch(64, 64)
    else:
        f_in, f_ref, d_in, d_ref = _fm(fin, ops), _fm(fref, ops), _fm(dfin0, ops), _fm(dfref0, ops)
    ops.match_gather_backward(f_in, f_ref, idx.to(torch.int32).cuda(), scale, _fm(dcat, ops), d_in, d_ref)
    torch.cuda.synchronize()
    got_in = d_in.t.cpu()[..., :64]
    got_ref = d_ref.t.cpu()[..., 64:] if view else d_ref.t.cpu()
    _check(f"match_gather_backward f32 dfin {name}", got_in, w_fin, b_fin, report)
    _check(f"match_gather_backward f32 dfref {name}", got_ref, w_ref, b_ref, report)
    _, ok = H.mgb_source(idx, Hh, W, scale)
    dead = (~ok).unsqueeze(-1).expand_as(got_in)
    assert torch.equal(got_in[dead], dfin0[dead]), "a pair whose source lies outside the map must add exactly zero"


def test_spynet_level_input_backward_f32_dcat8(report):
    """The kernel is the fp16 form's; only dcat8's reader differs.  (a) fp16-exact gradient values in an fp32 dcat8 and in an fp16 dcat8:
    bit-identical dflow_up and dflow_lo.  (b) full fp32 mantissas in dcat8 over a constant image (every neighbour difference is exactly
    zero, so the warp term vanishes): dflow_up = fp32(base + dcat8[6:8]) bit for bit, which an fp16 read of dcat8 cannot give."""
    ops = _ops()
    N, Hh, W = 2, 6, 10
    g = H.gen("spynet-bw")
    supp = H.draw(g, (N, Hh, W, 4)).abs()
    flow_up = H.draw(g, (N, Hh, W, 2), 1.5)
    d16 = H.draw(g, (N, Hh, W, 8)).half().float()
    base_up, base_lo = H.draw(g, (N, Hh, W, 2)), H.draw(g, (N, Hh // 2, W // 2, 2))
    outs = []
    for dt in (torch.float16, F32):
        dup, dlo = _fm(base_up, ops), _fm(base_lo, ops)
        ops.spynet_level_input_backward(_fm(supp, ops), _fm(flow_up, ops), ops.FM(d16.to(dt).cuda()), dup, dlo)
        torch.cuda.synchronize()
        outs.append((dup.t.cpu(), dlo.t.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "fp32 dcat8 and fp16 dcat8 of equal values differ"
    assert not torch.equal(outs[1][0], base_up)
    d32 = H.draw(g, (N, Hh, W, 8))
    assert not torch.equal(d32, d32.half().float())
    dup = _fm(base_up, ops)
    ops.spynet_level_input_backward(_fm(torch.full((N, Hh, W, 4), 0.375), ops), _fm(flow_up, ops), _fm(d32, ops), dup, None)
    torch.cuda.synchronize()
    assert torch.equal(dup.t.cpu(), base_up + d32[..., 6:8]), "dflow_up != base + the fp32 flow-channel gradients, bit for bit"
    report("spynet_level_input_backward f32 dcat8: bit-identical to the fp16-dcat8 form on fp16-exact values; full-mantissa pass-through exact")


# ------------------------------------------------------------------------------------------------------------------ DCN backward
def _dcn_run(ops, x, om, dcol, dom0, dx_only=False):
    xf, omf, domf = _fm(x, ops), _fm(om, ops), _fm(dom0, ops)
    dx32 = ops.dcn_col2im(xf, omf, _fm(dcol, ops), H.G_DCN, domf)
    torch.cuda.synchronize()
    return dx32.t.cpu(), domf.t.cpu()


def _dcn_check(tag, dx, dom, ref, dom0, report):
    _check(f"{tag} dx", dx, ref["dx"], H.dcn_dx_bound(ref), report)
    want, bound = H.dcn_dom_bound(ref, dom0)
    _check(f"{tag} d offset", dom[..., :144], want[..., :144], bound[..., :144], report)
    _check(f"{tag} d mask", dom[..., 144:], want[..., 144:], bound[..., 144:], report)


def test_dcn_tile_is_the_table_s(report):
    assert _ops().dcn_col2im_tile() == H.DCN_TILE, "tests/helpers_train_model_fp32.py::DCN_MAPS was laid out for another tile size"


@pytest.mark.parametrize("regime", DCN_REGIMES)
def test_dcn_columns_f32(regime, report):
    ops = _ops()
    for mapname in H.DCN_MAPS:
        x, om, _, _ = H.dcn_data(regime, mapname)
        ref = H.dcn_bw_ref(x, om)
        col = ops.dcn_columns(_fm(x, ops), _fm(om, ops), H.G_DCN)
        torch.cuda.synchronize()
        assert col.f32
        _check(f"dcn_columns f32 {regime} {mapname}", col.t.cpu(), ref["col"], H.dcn_col_bound(ref), report)


@pytest.mark.parametrize("regime", DCN_REGIMES)
def test_dcn_col2im_f32(regime, report):
    """dx (window scatter, LDS and global atomics), d offset and d mask logit on fp32 maps, N = 2, G = 8: a map smaller than a tile (plain and
    deterministic), a 3 x 3-tile ragged map with the regime everywhere (plain), and the same map with the regime on two rows (plain and
    deterministic: the far records fit their buffer).  Two deterministic runs are bit-identical."""
    ops = _ops()
    prev = ops.DETERMINISTIC
    try:
        for mapname, band in (("sub_tile", None), ("tiles_3x3_ragged", None), ("tiles_3x3_ragged", H.DCN_BAND)):
            N, Hh, W = H.DCN_MAPS[mapname]
            x, om, dcol, dom0 = H.dcn_data(regime, mapname, band)
            active, far, _, _ = far_stats(om, Hh, W)
            ref = H.dcn_bw_ref(x, om, dcol)
            tag = f"dcn_col2im f32 {regime} {mapname}{' band' if band else ''}"
            report(f"{tag}: {far} of {active} active corners outside their tile's window; at most {int(ref['count'].max())} terms on an element")
            if mapname == "sub_tile":
                assert far == 0
            elif band is None and regime in ("coherent", "wild"):
                # (wild: sigma 9 px on a 19 x 21 map sends most far samples out of the MAP, where they are not active: an eighth stays)
                assert far > active // (5 if regime == "coherent" else 10), "the regime must reach the far path"
            ops.DETERMINISTIC = False
            dx, dom = _dcn_run(ops, x, om, dcol, dom0)
            _dcn_check(tag + " plain", dx, dom, ref, dom0, report)
            if mapname == "tiles_3x3_ragged" and band is None:
                continue
            assert far <= max(1 << 16, N * Hh * W * H.G_DCN * 36 // 8)
            ops.DETERMINISTIC = True
            a_dx, a_dom = _dcn_run(ops, x, om, dcol, dom0)
            b_dx, b_dom = _dcn_run(ops, x, om, dcol, dom0)
            _dcn_check(tag + " deterministic", a_dx, a_dom, ref, dom0, report)
            assert torch.equal(a_dx, b_dx) and torch.equal(a_dom, b_dom), f"{tag}: two deterministic runs differ"
            assert torch.equal(a_dom, dom), "the offset / mask gradients do not depend on the mode"
    finally:
        ops.DETERMINISTIC = prev


def test_dcn_backward_refuses_mixed_dtypes(report):
    """any fp16 map among fp32 ones (and the reverse): an error before any launch, the output buffers keep their sentinel"""
    ops = _ops()
    from tdvc_amd import _lib as L
    N, Hh, W = 1, 5, 7
    mk = lambda C_, dt: ops.FM(torch.full((N, Hh, W, C_), 0.5, dtype=dt, device="cuda"))
    for odd in range(4):
        for base in (F32, torch.float16):
            other = torch.float16 if base == F32 else F32
            dts = [other if i == odd else base for i in range(4)]
            x, om, dcol = mk(64, dts[0]), mk(216, dts[1]), mk(576, dts[2])
            dom = ops.FM(torch.full((N, Hh, W, 216), SENT, dtype=dts[3], device="cuda"))
            for det in (False, True):
                ops.DETERMINISTIC, prev = det, ops.DETERMINISTIC
                try:
                    with pytest.raises(L.TdvcHipError, match="all fmaps must be fp16 or all fp32"):
                        ops.dcn_col2im(x, om, dcol, H.G_DCN, dom)
                finally:
                    ops.DETERMINISTIC = prev
            torch.cuda.synchronize()
            assert torch.equal(dom.t, torch.full_like(dom.t, SENT)), "a refused dcn_col2im wrote dom"
            if odd < 2:
                with pytest.raises(L.TdvcHipError, match="all fmaps must be fp16 or all fp32"):
                    ops.dcn_columns(x, om, H.G_DCN)
    # a refused call leaves dx32 alone as well: through the raw entry point, with a caller-owned dx32
    import ctypes as C
    x, om, dcol, dom = mk(64, F32), mk(216, torch.float16), mk(576, F32), mk(216, F32)
    dx32 = torch.full((N, Hh, W, 64), SENT, device="cuda")
    nwork = L.lib().tdvc_dcn_col2im_work_floats(N, Hh, W, H.G_DCN)
    work = torch.full((nwork,), SENT, device="cuda")
    d = [f.desc() for f in (x, om, dcol, dom)]
    rc = L.lib().tdvc_dcn_col2im(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), H.G_DCN, dx32.data_ptr(), C.byref(d[3]), work.data_ptr(), nwork, ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and torch.equal(dx32, torch.full_like(dx32, SENT)) and torch.equal(work, torch.full_like(work, SENT))
    report("dcn_columns / dcn_col2im / dcn_col2im_det: mixed fp16 / fp32 maps are refused before any launch")


def test_dcn_fused_f32_under_a_tape_needs_the_mode(report):
    """ops.dcn_fused on fp32 maps keeps raising under a tape; inside the whole-model fp32 training mode it records, and its backward
    (fp16 output gradient -> fp32 columns, conv_wgrad_f32, conv_f32, fp32 col2im) agrees with float64 to fp16 rounding of that gradient"""
    ops = _ops()
    from tdvc_amd import _lib as L, autograd
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    N, Hh, W = H.DCN_MAPS["tiles_3x3_ragged"]
    x, om, _, _ = H.dcn_data("subpixel", "tiles_3x3_ragged")
    g = H.gen("dcn-fused")
    w, b = H.draw(g, (64, 64, 3, 3), 1.0 / 24), H.draw(g, (64,), 0.1)
    gy = H.draw(g, (N, Hh, W, 64), 0.5).half().float()                      # the output is fp16: so is its gradient
    wp, bp = torch.nn.Parameter(w.cuda()), torch.nn.Parameter(b.cuda())
    pc = ops.pack_conv(wp, bp, stride=1, pad=1, ck=64)
    xf, omf = _fm(x, ops), _fm(om, ops)
    with autograd.record():
        with pytest.raises(L.TdvcHipError, match="inference form"):
            ops.dcn_fused(xf, omf, pc, ops.FM.empty(N, Hh, W, 64), groups=8)
    ops.PROFILE = []
    try:
        with autograd.record() as tape, ops.train_model_fp32(True):
            out = ops.dcn_fused(xf, omf, pc, ops.FM.empty(N, Hh, W, 64), groups=8)
            tape.grad(out).t.copy_(gy.half().cuda())
            tape.backward()
            dx, dom = tape.grad(xf).t.cpu(), tape.grad(omf).t.cpu()
        torch.cuda.synchronize()
        kern = [e["kernel"] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert kern == ["dcn_columns_f32", "conv_wgrad_f32", "conv_f32", "dcn_col2im_f32"], kern
    assert dx.dtype == F32 and dom.dtype == F32
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().double()
    leaf = lambda t: t.double().clone().requires_grad_()
    xr, wr, br, offr, mr = leaf(nchw(x)), leaf(w), leaf(b), leaf(nchw(om[..., :144])), leaf(nchw(om[..., 144:]))
    y = dcn_v2_forward_ref(xr, wr, br, offr, torch.sigmoid(mr), 3, 3, 1, 1, 1, 1, 1, 1, 8)
    dx_r, dw_r, db_r, doff_r, dm_r = torch.autograd.grad((y * nchw(gy)).sum(), (xr, wr, br, offr, mr))
    rel = lambda a, r: float((a.double() - r).norm() / r.norm())
    errs = dict(dx=rel(dx.permute(0, 3, 1, 2), dx_r), dW=rel(wp.grad.cpu(), dw_r), db=rel(bp.grad.cpu(), db_r),
                doff=rel(dom[..., :144].permute(0, 3, 1, 2), doff_r), dmask=rel(dom[..., 144:].permute(0, 3, 1, 2), dm_r))
    report("record_dcn_fused on fp32 maps, relative L2 error against float64: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # every sum is fp32 over at most N H W = 798 (dW, db) or 64 x 36 terms: 1e-5 relative in L2 is orders above sqrt(n) EPS32 and orders
    # below one fp16 rounding (2^-11 = 4.9e-4 per operand)
    assert max(errs.values()) < 1e-5, errs


# ------------------------------------------------------------------------------------------------------------------ conv geometries
@pytest.mark.parametrize("case", H.CONV_CASES, ids=[c[0] for c in H.CONV_CASES])
def test_conv_backward_f32_new_geometries(case, report):
    """weight / bias / data gradient of the conv geometries a whole-model fp32 step adds to the coders', by the existing fp32 test's
    procedure and bounds (tests/test_conv_wgrad_f32_gpu.py::test_conv_backward_f32)"""
    WG.test_conv_backward_f32(case, report)


def test_temporal_conv_backward_f32(report):
    """the (3, 1, 1) stride-3 Conv3d of LoopFilter as a 1x1 conv over 3 x 64 channels gathered from the 5-D parameter: fp32 data gradient and
    weight gradient in the parameter's own layout, bounds as in tests/test_conv_wgrad_f32_gpu.py"""
    ops = _ops()
    import torch.nn.functional as Fn
    from tdvc_amd.model.modules import pk_conv
    N, Hh, W = 2, 9, 11
    g = H.gen("temporal")
    conv = torch.nn.Conv3d(64, 64, (3, 1, 1), stride=(3, 1, 1), bias=False).cuda()
    w5 = H.draw(g, (64, 64, 3, 1, 1), 1.0 / 14)
    with torch.no_grad():
        conv.weight.copy_(w5)

    class Holder(torch.nn.Module):
        _pk = lambda self, key, fn: fn()
    pc = pk_conv(Holder(), "bt", conv)
    x, gy = H.draw(g, (N, Hh, W, 192)), H.draw(g, (N, Hh, W, 64), 0.5)
    w2 = w5[:, :, :, 0, 0].permute(0, 2, 1).reshape(64, 192, 1, 1)                   # input channel t * 64 + c
    xr, wr = x.permute(0, 3, 1, 2).double().requires_grad_(), w2.double().requires_grad_()
    gw, gx = torch.autograd.grad(Fn.conv2d(xr, wr), (wr, xr), gy.permute(0, 3, 1, 2).double())
    aw, ax = H.conv_grads64(x.permute(0, 3, 1, 2).abs(), w2.abs(), gy.permute(0, 3, 1, 2).abs(), 1, 0)
    xf, gf = _fm(x, ops), _fm(gy, ops)
    dw = torch.zeros(w5.numel(), device="cuda")
    ops.PROFILE = []
    try:
        ops.conv_wgrad(pc, gf, xf, dw)
        dx = ops.conv_dgrad(pc, gf, ops.FM.zeros(N, Hh, W, 192, dtype=F32), accumulate=True)
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
    assert [e["kernel"] for e in prof] == ["conv_wgrad_f32", "conv_f32"] and prof[0]["geo"] == H.TEMPORAL_CLASS
    K = N * Hh * W
    got_w = dw.cpu().view(64, 64, 3).permute(0, 2, 1).reshape(64, 192, 1, 1)          # the parameter's (o, c, t) layout -> (o, t * 64 + c)
    _check("temporal conv wgrad f32", got_w, gw, (K + 3) * H.EPS32 * aw + H.EPS32 * gw.abs(), report)
    _check("temporal conv dgrad f32", dx.t.cpu().permute(0, 3, 1, 2), gx, (64 + 3) * H.EPS32 * ax + H.EPS32 * gx.abs(), report)


def test_planar_fp32_output_adjoint(report):
    """the RGB head in the fp32 mode: a 3x3 64 -> 3 conv on an fp32 map with a planar fp32 output and the [0, 1] clamp, recorded on a
    tape (autograd.record_conv's planar branch: the planar gradient becomes an fp32 map, clamp01_backward, conv_wgrad_f32, conv_f32
    dgrad) against float64 autograd.  Bounds as in tests/test_conv_wgrad_f32_gpu.py; pixels whose pre-clamp value lies within 1e-5 of a
    clamp bound are left out (the fp32 forward may put them on the other side)."""
    ops = _ops()
    import torch.nn.functional as Fn
    from tdvc_amd import autograd
    N, Hh, W = 2, 9, 11
    g = H.gen("planar")
    x, w, b = H.draw(g, (N, 64, Hh, W)), H.draw(g, (3, 64, 3, 3), 1.0 / 24), H.draw(g, (3,), 0.1) + 0.5
    gy = H.draw(g, (N, 3, Hh, W), 0.5)
    wp, bp = torch.nn.Parameter(w.cuda()), torch.nn.Parameter(b.cuda())
    pc = ops.pack_conv(wp, bp, stride=1, pad=1)
    xf = ops.from_nchw(x.cuda(), dtype=F32)
    rgb = torch.empty((N, 3, Hh, W), dtype=F32, device="cuda")
    ops.PROFILE = []
    try:
        with autograd.record() as tape:
            ops.conv(xf, pc, act=ops.ACT_CLAMP01, nchw_out=rgb)
            tape.grad_tensor(rgb).copy_(gy.cuda())
            tape.backward()
            dx = tape.grad(xf).to_nchw().cpu()
        torch.cuda.synchronize()
        kern = [(e["kernel"], e["shape"]) for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert [k for k, _ in kern] == ["conv_f32", "conv_wgrad_f32", "conv_f32"] and "nchw" in kern[0][1], kern
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    pre = Fn.conv2d(xr, wr, br, padding=1)
    near = ((pre.detach().abs() < 1e-5) | ((pre.detach() - 1).abs() < 1e-5))
    assert not near.any(), "a pre-clamp value sits on a clamp bound: choose another seed"
    live = ((pre.detach() > 0) & (pre.detach() < 1)).double()
    assert 0.2 < float(live.mean()) < 0.95, "the data must reach both sides of the clamp"
    gw, gb, gx = torch.autograd.grad(pre.clamp(0.0, 1.0), (wr, br, xr), gy.double())
    ge = gy.double() * live                                   # the gradient behind the clamp
    aw, ax = H.conv_grads64(x.abs(), w.abs(), ge.abs(), 1, 1)
    K, Kx = N * Hh * W, 9 * 3
    _check("planar fp32 output: dW", wp.grad.cpu(), gw, (K + 3) * H.EPS32 * aw + H.EPS32 * gw.abs(), report)
    _check("planar fp32 output: db", bp.grad.cpu(), gb, (K + 3) * H.EPS32 * ge.abs().sum((0, 2, 3)) + H.EPS32 * gb.abs(), report)
    _check("planar fp32 output: dX", dx, gx, (Kx + 3) * H.EPS32 * ax + H.EPS32 * gx.abs(), report)
    assert torch.equal(rgb.cpu(), rgb.cpu().clamp(0, 1)) and H.ratio(rgb.cpu(), pre.detach().clamp(0, 1), (64 * 9 + 3) * H.EPS32 * (Fn.conv2d(x.double().abs(), w.double().abs(), padding=1) + b.double().abs().view(1, 3, 1, 1))) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ coverage guard
def test_model_fp32_step_geometries_have_op_level_tests(report):
    """one train_model_fp32 forward + backward of the whole model at 1 x 64 x 64 under ops.PROFILE: every kernel of it is an fp32 kernel,
    and every fp32 weight-gradient geometry class is a row of this file's tables or of the existing fp32 test's"""
    import test_train_model_fp32_gpu as TM
    prof = TM.profiled_sweep()["prof"]
    seen = {}
    for e in prof:
        if e["kernel"] == "conv_wgrad_f32":
            seen[e["geo"]] = seen.get(e["geo"], 0) + 1
    tables = H.conv_classes() | WG.op_level_wgrad_f32_classes()
    missing = sorted(set(seen) - tables)
    report(f"fp32 wgrad geometry classes of a model_fp32 step: {len(seen)} ({sum(seen.values())} launches), {len(set(seen) - WG.op_level_wgrad_f32_classes())} "
           f"of them outside the coders; without an op-level case: {missing}")
    assert len(seen) >= 20
    assert not missing, f"fp32 conv weight-gradient geometries without an op-level test: {missing}"
    unused = sorted(H.conv_classes() - set(seen))
    assert not unused, f"case rows that no layer of the step runs: {unused}"
    # the DCN backward's shape class: G = 8 on a map of several col2im tiles (the op-level maps: below one tile, and 3 x 3 ragged tiles)
    dcn = [e["shape"] for e in prof if e["kernel"] in ("dcn_columns_f32", "dcn_col2im_f32")]
    assert dcn == ["G8 @1x64x64", "G8 @1x64x64"] and H.G_DCN == 8 and 64 > 2 * H.DCN_TILE, dcn
    # every recorded conv launches exactly one weight gradient, so the classes above are those of every conv_f32 forward and data
    # gradient of the step too (the case rows test the data gradient of their class next to its weight gradient)
    kernels = {e["kernel"] for e in prof}
    assert {"dcn_columns_f32", "dcn_col2im_f32"} <= kernels and not ({"dcn_columns", "dcn_col2im", "conv_wgrad"} & kernels), sorted(kernels)
