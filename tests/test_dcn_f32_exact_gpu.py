"""tdvc_dcn_fused on fp32 maps (dcn_fused_kernel<float>, csrc/dcn_common.h) held to exact answers: the cases, data and references of
tests/helpers_dcn_exact.py on the small maps, once with an fp32 y and once with an fp16 y (tests/helpers_dcn_f32.py: the case
table, the epilogue rule of an fp32 output, the bound without its fp16 terms, and the genuinely-fp32 case).

  * integer and dyadic grades: `torch.equal` against the reference; float64 grade: helpers_dcn_f32.bound, element by element;
  * the fp32 case: x, w, offsets and logits that are no fp16 values, offsets hundreds of pixels long, three weights per output
    channel, held to helpers_dcn_f32.fp32_case_bound (24 EPS32 of the sum of magnitudes, counted rounding by rounding).  A kernel
    that rounds x, w or the logits to fp16 misses it by more than 100 x at its worst output, one that rounds the offsets by more
    than 1000 x, each in over 90 % of the outputs (tests/test_dcn_f32_cases_cpu.py asserts that on the CPU, one input at a time);
  * y is prefilled with a NaN sentinel, every element outside y's window keeps its bits (views: x and an fp32 y are channel windows
    of one 192-channel fp32 buffer, an fp16 y a window of an fp16 buffer of that shape; om 216 of 232 channels)."""
import pytest
import torch

from tests import helpers_dcn_exact as X
from tests import helpers_dcn_f32 as F

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x7E5A, 0x7FC5A5A5          # quiet NaNs: every element a launch must neither write nor use


def _sentinel(dtype, *shape):
    if dtype == torch.float32:
        return torch.full(shape, SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16).view(torch.float16)


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Buffers:
    """fp32 x and om, y in `ydt`; dense or as production's views"""

    def __init__(self, ops, case, d, ydt):
        N, H, W = case.N, case.H, case.W
        x = d.x.permute(0, 2, 3, 1).contiguous()
        step = 2 if case.views == 2 else 1
        self.case, self.step, self.ydt = case, step, ydt
        if case.views:
            xb = _sentinel(torch.float32, N * step, H, W, X.VIEW_BUF_C)
            xb[::step, ..., X.VIEW_X0:X.VIEW_X0 + X.CH] = x
            omb = _sentinel(torch.float32, N * step, H, W, X.VIEW_OM_C)
            omb[::step, ..., :27 * X.G] = d.om
            yb = xb if ydt == torch.float32 else _sentinel(ydt, N * step, H, W, X.VIEW_BUF_C)
        else:
            xb, omb, yb = x, d.om.contiguous(), _sentinel(ydt, N, H, W, X.CH)
        self.x_start, self.om_start, self.y_start = xb, omb, yb
        self.shared = case.views and ydt == torch.float32
        self.x_buf, self.om_buf = xb.cuda(), omb.cuda()
        self.y_buf = self.x_buf if self.shared else yb.cuda()
        fx, fo, fy = ops.FM(self.x_buf[::step]), ops.FM(self.om_buf[::step]), ops.FM(self.y_buf[::step])
        if case.views:
            self.x, self.om, self.y = fx.ch(X.VIEW_X0, X.CH), fo.ch(0, 27 * X.G), fy.ch(X.VIEW_Y0, X.CH)
            assert self.x.sp == X.VIEW_BUF_C and self.y.sp == X.VIEW_BUF_C and self.om.sp == X.VIEW_OM_C
            assert case.views == 1 or (N > 1 and self.x.sn == 2 * H * W * X.VIEW_BUF_C and self.om.sn == 2 * H * W * X.VIEW_OM_C)
        else:
            self.x, self.om, self.y = fx, fo, fy
        assert self.x.f32 and self.om.f32 and self.y.f32 == (ydt == torch.float32)

    def output(self):
        """(N, 64, H, W) fp32 on the CPU"""
        y = self.y_buf[::self.step, ..., X.VIEW_Y0:X.VIEW_Y0 + X.CH] if self.case.views else self.y_buf
        return y.float().cpu().permute(0, 3, 1, 2).contiguous()

    def surroundings_intact(self):
        """every element outside y's window has the bits it started with: the sentinels, the spare images, x, om"""
        if not torch.equal(_bits(self.om_buf), _bits(self.om_start)):
            return False
        if not self.shared and not torch.equal(_bits(self.x_buf), _bits(self.x_start)):
            return False
        if not self.case.views:
            return True
        got, want = _bits(self.y_buf).clone(), _bits(self.y_start).clone()
        for t in (got, want):
            t[::self.step, ..., X.VIEW_Y0:X.VIEW_Y0 + X.CH] = 0
        return torch.equal(got, want)


def _first(bad, got, ref):
    n, c, y, x = (int(v) for v in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} outputs; first at (n {n}, c {c}, y {y}, x {x}): got {float(got[n, c, y, x])!r}, want {float(ref[n, c, y, x])!r}"


def _run(case, d, y32):
    from tdvc_amd import ops
    buf = Buffers(ops, case, d, torch.float32 if y32 else torch.float16)
    pc = ops.pack_conv(d.w, d.b, stride=1, pad=1, ck=X.CH)
    ops.dcn_fused(buf.x, buf.om, pc, buf.y, groups=X.G, act=case.act, slope=case.slope, round16=case.round16)
    torch.cuda.synchronize()
    got = buf.output()
    tag = f"{case.id} [{'fp32' if y32 else 'fp16'} y]"
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite outputs: " + _first(~torch.isfinite(got), got, d.ref)
    assert buf.surroundings_intact(), f"{tag}: an element outside the output window changed"
    return got, tag


@pytest.mark.parametrize("case,y32", F.RUNS, ids=[f"{c.id}-{'y32' if y32 else 'y16'}" for c, y32 in F.RUNS])
def test_dcn_fused_f32_exact(case, y32, report):
    d = X.reference(case)
    got, tag = _run(case, d, y32)
    if case.grade == "f64":
        tol = F.bound(case, d, y32)
        err = (got.double() - d.ref).abs()
        report(f"dcn f32 exact {tag}: max |err| / bound = {float((err / tol).max()):.3f}, max |err| = {float(err.max()):.3e}")
        assert bool((err <= tol).all()), f"{tag}: worst |err| / bound {float((err / tol).max()):.3f}; " + _first(err > tol, got, d.ref)
        return
    want = F.expected_exact(case, d, y32)
    bad = got != want
    assert not bool(bad.any()), f"{tag} ({case.grade}): " + _first(bad, got, want)
    assert torch.equal(got, want)


def test_dcn_fused_f32_genuine_fp32_data(report):
    """no input is an fp16 value and the offsets are hundreds of pixels long: fp16 rounding of any one input misses the bound by more
    than two orders (tests/test_dcn_f32_cases_cpu.py)"""
    case, d = F.FP32_CASE, F.fp32_reference()
    got, tag = _run(case, d, True)
    tol = F.fp32_case_bound(d)
    err = (got.double() - d.ref).abs()
    report(f"dcn f32 exact {tag}: max |err| / bound = {float((err / tol).max()):.3f}, max |err| = {float(err.max()):.3e}")
    assert bool((err <= tol).all()), f"{tag}: worst |err| / bound {float((err / tol).max()):.3f}; " + _first(err > tol, got, d.ref)


def test_dcn_fused_f32_rejects_before_launch():
    """an fp16 om, or a planar scratch, with an fp32 x: an error, nothing launched"""
    from tdvc_amd import _lib, ops
    case = F.CASES[0]
    d = X.reference(case)
    pc = ops.pack_conv(d.w, d.b, stride=1, pad=1, ck=X.CH)
    x = ops.FM(d.x.permute(0, 2, 3, 1).contiguous().cuda())
    y = ops.FM(_sentinel(torch.float32, case.N, case.H, case.W, X.CH).cuda())
    with pytest.raises(_lib.TdvcHipError):
        ops.dcn_fused(x, ops.FM(d.om.half().cuda()), pc, y, groups=X.G)
    with pytest.raises(_lib.TdvcHipError):
        ops.dcn_fused(x, ops.FM(d.om.contiguous().cuda()), pc, y, groups=X.G, planar=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.t), _bits(_sentinel(torch.float32, case.N, case.H, case.W, X.CH)))
