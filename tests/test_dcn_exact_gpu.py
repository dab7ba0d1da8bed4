"""The fused DCN forward kernels behind tdvc_dcn_fused, and the fp32 operator behind `_ext.dcn_v2_forward`, held to exact answers
(tests/helpers_dcn_exact.py: the case table, the three grades of data, the restated epilogue and the float64 bound).

  * every (case, path) is compared with the reference on its own, never with another path (the cross-check of the LDS-window
    kernel against the gather kernel stays in tests/test_dcn_gpu.py);
  * integer and dyadic grades: `torch.equal` against the reference; float64 grade: the bound of helpers_dcn_exact.f64_bound,
    element by element, the largest |err| / bound reported;
  * y is prefilled with a NaN sentinel, so a tile the remap never reaches shows as a non-finite output;
  * views: x and y are channel windows of one 192-channel buffer (as in MCNet.run), om the first 216 channels of a 232-channel
    buffer, in one case with spare images between the images; every element outside y's window keeps its sentinel bits, x its data.

Measured on an MI355X: see DESIGN.md, "Exact tests of the forward DCN"."""
import ctypes

import pytest
import torch

from tests import helpers_dcn_exact as X

pytestmark = pytest.mark.gpu

SENT = 0x7E5A                 # fp16 bit pattern of every element a launch must neither write nor use: a quiet NaN


def _ops():
    from tdvc_amd import ops
    return ops


def _lds_switch():
    from tdvc_amd import _lib
    fn = _lib.lib().tdvc_debug_enable_dcn_lds
    fn.argtypes, fn.restype = [ctypes.c_int], None
    return fn


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16).view(torch.float16)


class Buffers:
    """the three feature maps of a launch, dense or as production's views, with the expected bytes of everything but y"""

    def __init__(self, ops, case, d):
        N, H, W = case.N, case.H, case.W
        x = d.x.permute(0, 2, 3, 1).half()
        om = d.om.half()
        step = 2 if case.views == 2 else 1                               # spare images between the images: a batch stride of 2 H W C
        if case.views:
            xy = _sentinel(N * step, H, W, X.VIEW_BUF_C)
            xy[::step, ..., X.VIEW_X0:X.VIEW_X0 + X.CH] = x
            omb = _sentinel(N * step, H, W, X.VIEW_OM_C)
            omb[::step, ..., :27 * X.G] = om
        else:
            xy, omb = None, om
        self.case = case
        self.step = step
        self.om_start = omb
        self.om_buf = omb.cuda()
        om_fm = ops.FM(self.om_buf[::step])
        self.om = om_fm.ch(0, 27 * X.G) if case.views else om_fm
        if case.views:
            self.xy_start = xy
            self.xy_buf = xy.cuda()
            fm = ops.FM(self.xy_buf[::step])
            self.x, self.y = fm.ch(X.VIEW_X0, X.CH), fm.ch(X.VIEW_Y0, X.CH)
            assert self.x.sp == X.VIEW_BUF_C and self.y.sp == X.VIEW_BUF_C and self.om.sp == X.VIEW_OM_C
            assert case.views == 1 or (N > 1 and self.x.sn == 2 * H * W * X.VIEW_BUF_C and self.om.sn == 2 * H * W * X.VIEW_OM_C)
        else:
            self.x_start = x.contiguous()
            self.x_buf = self.x_start.cuda()
            self.y_buf = _sentinel(N, H, W, X.CH).cuda()
            self.x, self.y = ops.FM(self.x_buf), ops.FM(self.y_buf)

    def reset(self):
        if self.case.views:
            self.xy_buf.copy_(self.xy_start)
        else:
            self.y_buf.copy_(_sentinel(*self.y_buf.shape))

    def output(self):
        """(N, 64, H, W) fp32 on the CPU"""
        y = self.xy_buf[::self.step, ..., X.VIEW_Y0:X.VIEW_Y0 + X.CH] if self.case.views else self.y_buf
        return y.float().cpu().permute(0, 3, 1, 2).contiguous()

    def surroundings_intact(self):
        """every element outside y's window has the bits it started with: the sentinels, the spare images, x, om"""
        bits = lambda t: t.cpu().view(torch.int16)
        if not torch.equal(bits(self.om_buf), bits(self.om_start)):
            return False
        if not self.case.views:
            return torch.equal(bits(self.x_buf), bits(self.x_start))
        got, want = bits(self.xy_buf).clone(), bits(self.xy_start).clone()
        for t in (got, want):
            t[::self.step, ..., X.VIEW_Y0:X.VIEW_Y0 + X.CH] = 0
        return torch.equal(got, want)


def describe_mismatch(case, path, d, got, bad):
    """the first differing pixel with its tile, the sample classes of its 72 taps and the count of differing outputs"""
    idx = bad.nonzero()
    n, c, y, x = (int(v) for v in idx[0])
    th, tw = X.tile_shape(path)
    tiles_x = -(-case.W // tw)
    h, w = X.sample_positions(case, d)
    ch, cw = X.axis_class(h[n, y, x], case.H), X.axis_class(w[n, y, x], case.W)
    inside = int(((h[n, y, x] > -1) & (h[n, y, x] < case.H) & (w[n, y, x] > -1) & (w[n, y, x] < case.W)).sum())
    classes = ", ".join(f"{name}: {int((ch == i).sum())} h / {int((cw == i).sum())} w" for i, name in enumerate(X.AXIS_CLASSES))
    pixels = torch.unique(idx[:, [0, 2, 3]], dim=0)
    tiles = torch.unique(torch.stack([pixels[:, 0], (pixels[:, 1] // th) * tiles_x + pixels[:, 2] // tw], 1), dim=0)
    return (f"{int(bad.sum())} of {bad.numel()} outputs differ, in {len(pixels)} pixels of {len(tiles)} tiles; first at (n {n}, c {c}, y {y}, x {x}), "
            f"{th}x{tw} tile {(y // th) * tiles_x + x // tw} (ty {y // th}, tx {x // tw}; {X.tile_count(case, path)} tiles, {X.xcd_regime(X.tile_count(case, path), case.N)} remap): "
            f"got {float(got[n, c, y, x])!r}, want {float(d.ref[n, c, y, x])!r}; regime {case.regime}: {inside} of its 72 samples inside the map, per axis {classes}")


def check(case, path, d, got, report):
    assert bool(torch.isfinite(got).all()), f"{case.id} [{path}]: " + describe_mismatch(case, path, d, got, ~torch.isfinite(got))
    if case.grade == "f64":
        err = (got.double() - d.ref).abs()
        ratio = err / d.tol
        report(f"dcn exact {case.id} [{path}]: max |err| / bound = {float(ratio.max()):.3f}, max |err| = {float(err.max()):.3e}")
        assert bool((err <= d.tol).all()), f"{case.id} [{path}]: worst |err| / bound {float(ratio.max()):.3f}; " + describe_mismatch(case, path, d, got, err > d.tol)
        return
    bad = got != d.ref
    assert not bool(bad.any()), f"{case.id} [{path}] ({case.grade}): " + describe_mismatch(case, path, d, got, bad)
    assert torch.equal(got, d.ref)


@pytest.mark.parametrize("case,path", X.RUNS, ids=[f"{c.id}-{p}" for c, p in X.RUNS])
def test_dcn_fused_exact(case, path, report):
    ops = _ops()
    d = X.reference(case)
    lds = _lds_switch()
    big = case.H * case.W >= X.LDS_MIN_PIXELS
    assert path != "lds" or big, "the LDS-window kernel runs on maps of 8192 pixels or more"
    buf = Buffers(ops, case, d)
    pc = ops.pack_conv(d.w, d.b, stride=1, pad=1, ck=X.CH)
    try:
        lds(0 if path == "gather" else 1)                                # on large maps `gather` means the call with the LDS kernel switched off
        ops.dcn_fused(buf.x, buf.om, pc, buf.y, groups=X.G, act=case.act, slope=case.slope, round16=case.round16, planar=path == "planar")
        torch.cuda.synchronize()
    finally:
        lds(1)
    check(case, path, d, buf.output(), report)
    assert buf.surroundings_intact(), f"{case.id} [{path}]: an element outside the output window changed"


@pytest.mark.parametrize("case", X.EXT_CASES, ids=[c.id for c in X.EXT_CASES])
def test_ext_forward_exact(case, report):
    """dcn_f32_forward_kernel on data whose every intermediate is an exact fp32 value: the float64 reference, cast to fp32, bit for bit"""
    import _ext
    x, w, b, off, mask, want = X.ext_reference(case)
    got = _ext.dcn_v2_forward(x.cuda(), w.cuda(), b.cuda(), off.cuda(), mask.cuda(), *X.ext_args(case)).cpu()
    assert got.shape == want.shape
    bad = got != want
    if bool(bad.any()):
        n, c, y, xx = (int(v) for v in bad.nonzero()[0])
        pytest.fail(f"{case.id}: {int(bad.sum())} of {bad.numel()} outputs differ; first at (n {n}, c {c}, y {y}, x {xx}), pixel {y * want.shape[3] + xx}: "
                    f"got {float(got[n, c, y, xx])!r}, want {float(want[n, c, y, xx])!r}")
    assert torch.equal(got, want)
