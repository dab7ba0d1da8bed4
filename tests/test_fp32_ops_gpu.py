"""The streaming launchers on fp32 maps (the whole-model fp32 mode, `VideoCompressor.model_fp32`), and avgpool_k, match_gather and
channel_sum in both dtypes, against CPU references: tables, float64 references and counted bounds in tests/helpers_fp32_ops.py.

Data and references are made on the CPU; outputs are views of NaN-sentinel buffers and every byte outside a view must come back unchanged;
each bounded test writes max(|d| / bound) through `report`.

`test_model_fp32_call_classes_have_cases` runs one 128x192 and one 1088x1920 frame in fp32 mode and fails when a streaming call class, or
the class of a conv on fp32 maps, that production reaches has no row -- in the tables here, in tests/test_forward_ops_gpu.py, in
tests/helpers_conv_exact.py or (coder layer shapes) in tests/test_conv_f32_gpu.py."""
import pytest
import torch

import test_conv_f32_gpu as CF
import test_forward_ops_gpu as FO
from test_forward_ops_gpu import assert_bits, assert_outside_unchanged, buffer, view
from tests import helpers_conv_exact as X
from tests import helpers_fp32_ops as H

pytestmark = pytest.mark.gpu

_ops, _lib, _chk, _ref = FO._ops, FO._lib, FO._chk, FO._ref


def window(data, c0, C_, N=None):
    """the CPU tensor `data` (N, H, W, Cbuf) on the device, and the FM of its channels [c0, c0 + C_)"""
    ops = _ops()
    t = data.cuda()
    return t, (ops.FM(t, c0, data.shape[0], C_) if (c0 or C_ != data.shape[3]) else ops.FM(t))


def sentinel_window(shape, dt, c0, C_):
    ops = _ops()
    t = buffer(shape, H.DT[dt])
    return t, (ops.FM(t, c0, shape[0], C_) if (c0 or C_ != shape[3]) else ops.FM(t))


def within(got, ref, bound, what, report):
    r = H.ratio(got, ref, bound)
    bad = ~((got.double() - ref).abs() <= bound)
    report(f"{what}: max(|d|/bound) = {r:.4f}, max |d| = {float((got.double() - ref).abs().max()):.3e}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound, max(|d|/bound) = {r:.3f}"


# ------------------------------------------------------------------------------------------------------------------ add_flow
@pytest.mark.parametrize("row", H.AF_CASES, ids=[r[0] for r in H.AF_CASES])
def test_add_flow_f32(row):
    """off[..., 2k] += flow_x, off[..., 2k+1] += flow_y on an fp32 offset map: one fp32 add, bit-exact"""
    ops = _ops()
    name, N, Hh, W, C_, Cb, Cf = row
    o_cpu, f_cpu = H.af_data(row)
    obuf, off = window(o_cpu, Cb - C_, C_)
    _, flow = window(f_cpu, 0, 2)
    before = obuf.clone()
    assert FO.cls_add_flow(off, flow) == H.af_class(row)
    ops.add_flow(off, flow)
    torch.cuda.synchronize()
    assert_bits(view(off), H.af_want(row, o_cpu, f_cpu), f"add_flow f32 {name}")
    assert_outside_unchanged(before, off, f"add_flow f32 {name}")


# ------------------------------------------------------------------------------------------------------------------ bcast_add_act
@pytest.mark.parametrize("row", H.BC_CASES, ids=[f"{r[0]}x{r[1]}x{r[2]}_T{r[4]}x{r[3]}_{r[5]}_{r[6]}{'_view' if r[7] else ''}" for r in H.BC_CASES])
def test_bcast_add_act_dtypes(row):
    """x[..., t Cb:(t+1) Cb] = lrelu(x + b, 0.1) in fp32, stored in x's dtype, for every (x, b) dtype pair: bit-exact.  Only fp16 x with fp16 b
    and T = 4 takes the T-slice kernel"""
    ops = _ops()
    N, Hh, W, Cb, T, xdt, bdt, wide = row
    x_cpu, b_cpu = H.bc_data(row)
    xbuf, x = window(x_cpu, 64 if wide else 0, T * Cb)
    _, b = window(b_cpu, 0, Cb)
    before = xbuf.clone()
    cls = FO.cls_bcast(T, FO._dt(x), FO._dt(b))
    assert cls in H.table_classes() | FO.BC_CLASSES and (cls[1] == "t4") == (T == 4 and xdt == "f16" and bdt == "f16")
    ops.bcast_add_act(x, b, T, 0.1)
    torch.cuda.synchronize()
    assert_bits(view(x), H.bc_want(row, x_cpu, b_cpu), f"bcast_add_act {xdt}/{bdt} T={T}")
    assert_outside_unchanged(before, x, "bcast_add_act")


# ------------------------------------------------------------------------------------------------------------------ upsample2x
@pytest.mark.parametrize("row", H.UP_CASES, ids=[f"{r[0]}x{r[1]}x{r[2]}x{r[3]}_{r[4]}to{r[5]}{'_vin' if r[6] else ''}{'_vout' if r[7] else ''}" for r in H.UP_CASES])
def test_upsample2x_dtypes(row, report):
    ops = _ops()
    N, h, w, C_, xdt, ydt, vin, vout = row
    x_cpu = H.up_data(row)
    _, x = window(x_cpu, 16 if vin else 0, C_)
    ybuf, y = sentinel_window((N, 2 * h, 2 * w, C_ + (8 if vout else 0)), ydt, 8 if vout else 0, C_)
    before = ybuf.clone()
    assert FO.cls_upsample(x, y) == ("upsample2x", "view" if (vin or vout) else "dense", xdt, ydt)
    ops.upsample2x(x, out=y)
    torch.cuda.synchronize()
    ref, bound = H.up_ref(row, x_cpu)
    within(view(y).cpu(), ref, bound, f"upsample2x {xdt}->{ydt} {N}x{h}x{w}x{C_}", report)
    assert_outside_unchanged(before, y, "upsample2x")
    if xdt == ydt == "f32" and not vout:              # the op-level entry allocates the output in x's dtype
        assert_bits(view(ops.upsample2x(x)), view(y), "ops.upsample2x")


# ------------------------------------------------------------------------------------------------------------------ spynet_level_input
@pytest.mark.parametrize("row", H.SP_CASES, ids=[f"{r[0]}x{r[1]}x{r[2]}{'_flow' if r[3] else ''}_C{r[4]}{'_win' if r[5] else ''}" for r in H.SP_CASES])
def test_spynet_level_input_f32_cat8(row, report):
    """an fp32 cat8: float64 with _level_bound's fp16 store term replaced by EPS32 |cat|; channels 0..2 are ref's bits; flow_up is the
    fp16-cat8 call's, bit for bit"""
    ops = _ops()
    N, Hh, W, fl, Cs, win = row
    ref, supp, flo = H.sp_data(row)
    fm = lambda t: ops.FM(t[..., :Cs].contiguous().cuda())
    rf, sf, ff = fm(ref), fm(supp), (ops.FM(flo.cuda()) if fl else None)
    upbuf, up = sentinel_window((N, Hh, W, 4), "f32", 2, 2)
    catbuf, cat8 = sentinel_window((N, Hh, W, 16 if win else 8), "f32", 8 if win else 0, 8)
    ub, cb = upbuf.clone(), catbuf.clone()
    assert H.cls_spynet32(FO.cls_spynet(rf, sf, ff, up), cat8) == ("spynet_level_input", "vec" if Cs == 4 else "scalar", fl, "f32")
    ops.spynet_level_input(rf, sf, ff, up, cat8)
    up16, cat16 = ops.FM(buffer((N, Hh, W, 2), torch.float32)), ops.FM(buffer((N, Hh, W, 8), torch.float16))
    ops.spynet_level_input(rf, sf, ff, up16, cat16)
    torch.cuda.synchronize()
    cat_r, up_r = FO._level_ref64(ref, supp, flo, Hh, W)
    bc, bu = FO._level_bound(cat_r, up_r, supp, Hh, W, flo)
    within(view(up).cpu(), up_r, bu, f"flow_up {N}x{Hh}x{W} C{Cs}", report)
    within(view(cat8).cpu(), cat_r, H.sp_bound32(bc, cat_r), f"fp32 cat8 {N}x{Hh}x{W} C{Cs}", report)
    assert_bits(view(cat8)[..., :3], ref[..., :3].contiguous(), "cat8 channels 0..2")
    assert_bits(view(up), view(up16), "flow_up, fp32 cat8 against fp16 cat8")
    assert_bits(view(cat8)[..., 6:], view(up), "cat8 channels 6..7 against flow_up")
    assert_outside_unchanged(ub, up, "flow_up")
    assert_outside_unchanged(cb, cat8, "cat8")


# ------------------------------------------------------------------------------------------------------------------ cast_f32 / copy_cast
@pytest.mark.parametrize("row", H.CC_CASES, ids=[r[0] for r in H.CC_CASES])
def test_cast_and_copy(row):
    ops = _ops()
    name, N, Hh, W, C_, sdt, ddt, vs, vd = row
    s_cpu = H.draw(H.gen("copy_cast", name), (N, Hh, W, C_ + (8 if vs else 0)), sdt)
    sbuf, src = window(s_cpu, 8 if vs else 0, C_)
    want = s_cpu[..., (8 if vs else 0):].to(H.DT[ddt])
    if name.startswith("cast_f32"):
        out = ops.cast_f32(src)
        torch.cuda.synchronize()
        assert out.f32 and FO._dense(out)
        assert_bits(view(out), want, name)
    else:
        dbuf, dst = sentinel_window((N, Hh, W, C_ + (16 if vd else 0)), ddt, 16 if vd else 0, C_)
        before = dbuf.clone()
        ops.copy_cast(src, dst)
        torch.cuda.synchronize()
        assert_bits(view(dst), want, name)
        assert_outside_unchanged(before, dst, name)
    assert torch.equal(FO.bits(sbuf.cpu()), FO.bits(s_cpu)), f"{name}: the source changed"


# ------------------------------------------------------------------------------------------------------------------ channel_sum
@pytest.mark.parametrize("row", H.CS_CASES, ids=[r[0] for r in H.CS_CASES])
def test_channel_sum(row, report):
    ops = _ops()
    name, dt, N, Hh, W, C_, nb, v = row
    x_cpu = H.cs_data(row)
    _, x = window(x_cpu, 8 if v else 0, C_)
    pbuf = buffer((N * nb * C_ + 64,), torch.float32)
    before = pbuf.clone()
    _chk(_lib().tdvc_channel_sum(_ref(x), pbuf.data_ptr(), nb, ops._stream()), "channel_sum")
    torch.cuda.synchronize()
    ref, bound = H.cs_ref(row, x_cpu)
    within(pbuf[:N * nb * C_].view(N, nb, C_).cpu(), ref, bound, f"channel_sum {name}", report)
    assert torch.equal(FO.bits(pbuf[N * nb * C_:]), FO.bits(before[N * nb * C_:])), f"channel_sum {name}: wrote past the partial sums"


# ------------------------------------------------------------------------------------------------------------------ avgpool_k
@pytest.mark.parametrize("row", H.AK_CASES, ids=[r[0] for r in H.AK_CASES])
def test_avgpool_k(row, report):
    ops = _ops()
    name, dt, N, Hh, W, C_, s, v = row
    x_cpu = H.ak_data(row)
    _, x = window(x_cpu, 16 if v else 0, C_)
    hp, wp = Hh // s, W // s
    lib = _lib()
    nwork = int(lib.tdvc_avgpool_k_work_floats(N, hp, wp, C_, s))
    assert nwork == N * hp * wp * -(-s // 8) * C_
    work, pooled = buffer((nwork + 64,), torch.float32), buffer((N * hp * wp * C_ + 64,), torch.float32)
    wb, pb = work.clone(), pooled.clone()
    _chk(lib.tdvc_avgpool_k(_ref(x), s, pooled.data_ptr(), hp, wp, work.data_ptr(), nwork, ops._stream()), "avgpool_k")
    torch.cuda.synchronize()
    ref, bound = H.ak_ref(row, x_cpu)
    n = N * hp * wp * C_
    within(pooled[:n].view(N, hp, wp, C_).cpu(), ref, bound, f"avgpool_k {name}", report)
    assert torch.equal(FO.bits(pooled[n:]), FO.bits(pb[n:])), f"avgpool_k {name}: wrote past the pooled map"
    assert torch.equal(FO.bits(work[nwork:]), FO.bits(wb[nwork:])), f"avgpool_k {name}: wrote past tdvc_avgpool_k_work_floats"
    assert_bits(ops.avgpool_k(x, s).view(-1), pooled[:n], f"ops.avgpool_k {name}")


# ------------------------------------------------------------------------------------------------------------------ match_gather
@pytest.mark.parametrize("row", H.MG_CASES, ids=[r[0] for r in H.MG_CASES])
def test_match_gather(row, report):
    ops = _ops()
    name, dts, N, Hh, W, scale, vr, vc = row
    fin_cpu, fref_cpu, idx = H.mg_data(row)
    ref, bound, clamped, outside = H.mg_ref(row, fin_cpu, fref_cpu, idx)
    assert clamped == outside and outside > 0, (clamped, outside)      # on the reference: the only pixels under the clamp are the zero sources
    _, fin = window(fin_cpu, 0, 64)
    _, fref = window(fref_cpu, 8 if vr else 0, 64)
    cbuf, cat = sentinel_window((N, Hh, W, 128 + (16 if vc else 0)), dts[2], 8 if vc else 0, 128)
    before = cbuf.clone()
    ops.match_gather(fin, fref, idx.cuda(), scale, cat)
    torch.cuda.synchronize()
    within(view(cat).cpu(), ref, bound, f"match_gather {name}", report)
    assert_outside_unchanged(before, cat, f"match_gather {name}")


# ------------------------------------------------------------------------------------------------------------------ the fp32 guard
def _record_fp32(monkeypatch, seen, convs):
    """tests/test_forward_ops_gpu.py's recorder plus the launchers it does not wrap, and the class of every ops.conv call on an fp32 map"""
    ops = _ops()
    from tdvc_amd import _lib as L
    FO._recorder(monkeypatch, seen)

    def wrap(name, classify):
        fn = getattr(ops, name)

        def w(*a, **k):
            seen.add(classify(*a, **k))
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, w)

    sp = ops.spynet_level_input                         # already wrapped: add the dtype of cat8 next to its class

    def spynet(r, s, fl, up, cat8):
        seen.add(H.cls_spynet32(FO.cls_spynet(r, s, fl, up), cat8))
        return sp(r, s, fl, up, cat8)
    monkeypatch.setattr(ops, "spynet_level_input", spynet)
    wrap("avgpool_k", lambda x, scale, out=None: H.cls_avgpool_k(FO._dt(x), x.C, scale, FO._dense(x)))
    wrap("match_gather", lambda fin, fref, idx, scale, cat: H.cls_match_gather((FO._dt(fin), FO._dt(fref), FO._dt(cat)), all(map(FO._dense, (fin, fref, cat)))))
    wrap("copy_cast", lambda s, d: H.cls_copy_cast(FO._dt(s), FO._dt(d), FO._dense(s) and FO._dense(d)))
    se = ops.se_gate                                    # channel_sum at the point ops calls it: se_gate without partial sums

    def se_gate(x, p, partial=None):
        if partial is None:
            seen.add(H.cls_channel_sum(FO._dt(x), x.C, x.H * x.W, max(1, min(1024, x.H * x.W // 256))))
        return se(x, p, partial)
    monkeypatch.setattr(ops, "se_gate", se_gate)
    conv = ops.conv

    def conv_rec(x, pc, *a, **k):
        if x.f32:
            kk = {n: v for n, v in k.items() if n not in ("chan_sum", "flow")}
            convs.add(X.conv_f32_class(L, ops.conv_desc(x, pc, *a, **kk)[0]))
        return conv(x, pc, *a, **k)
    monkeypatch.setattr(ops, "conv", conv_rec)


def _has_f32(cls):
    return any(e == "f32" or (isinstance(e, tuple) and "f32" in e) for e in cls)


def test_model_fp32_call_classes_have_cases(monkeypatch, report):
    from tdvc_amd import _lib as L, synth
    from tdvc_amd.model.pnet import VideoCompressor
    ops = _ops()
    seen, convs = set(), set()
    _record_fp32(monkeypatch, seen, convs)
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda().eval()
    m.model_fp32 = True
    for (Hh, W) in ((128, 192), (FO.BIG_H, FO.BIG_W)):
        g = synth.make_gop(1234, 2, Hh, W).float()
        refs = torch.stack([g[0], g[0], g[0], g[0]]).unsqueeze(0).cuda()
        with torch.no_grad():
            m(g[1:2].cuda(), refs, True)
        torch.cuda.synchronize()
    # streaming classes: every class with an fp32 map needs a row, here or in the tables of test_forward_ops_gpu
    tables = FO.table_classes() | H.table_classes()
    missing = sorted((c for c in seen if _has_f32(c) and c not in tables), key=str)
    report(f"fp32 mode, streaming call classes ({len(seen)}): " + "; ".join(str(s) for s in sorted(seen, key=str)))
    # conv classes: outside the coders the full class must be a row's; a coder layer's shape must be one tests/test_conv_f32_gpu.py runs
    rows = {X.conv_f32_class(L, X.guard_desc(L, ops._pick_ck, c)) for c in X.CASES if c.kernel == "conv_f32"}
    layers = {X.f32_layer(c) for c in convs}
    report(f"fp32 mode, conv_f32 call classes ({len(convs)}): " + "; ".join(str(s) for s in sorted(convs, key=str)))
    no_row = sorted((c for c in convs if X.f32_layer(c) not in X.F32_CODER_LAYERS and c not in rows), key=str)
    assert len(seen) >= 10 and len(convs) >= 40
    assert not missing, f"fp32-mode streaming call classes without an op-level case: {missing}"
    assert not no_row, f"conv_f32 call classes of the fp32 mode without a row in helpers_conv_exact.CASES: {no_row}"
    assert layers == X.F32_LAYERS | X.F32_CODER_LAYERS, (f"helpers_conv_exact's fp32 layer lists and production disagree: not listed "
                                                        f"{sorted(layers - X.F32_LAYERS - X.F32_CODER_LAYERS, key=str)}, listed but not run {sorted((X.F32_LAYERS | X.F32_CODER_LAYERS) - layers, key=str)}")
    assert X.F32_CODER_LAYERS <= CF.layers(), sorted(X.F32_CODER_LAYERS - CF.layers(), key=str)
    assert {c[4] for c in convs} == {(1, 1), (1, 2), (2, 1), (2, 2)}          # production takes all four instantiations (the CPU check: so do the rows)
