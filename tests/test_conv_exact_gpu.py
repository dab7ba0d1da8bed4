"""Every forward conv kernel behind tdvc_conv2d / tdvc_conv_pair, held to exact answers (tests/helpers_conv_exact.py: the case
table, the three grades of data and the restated rounding sequences).

  * integer and dyadic grades: `torch.equal` against the reference -- padded output channels exactly zero, every byte outside the
    channel windows of x / y / res / res2 unchanged;
  * float64 grade (GDN, sigmoid): the bound derived in helpers_conv_exact.f64_reference, element by element;
  * the kernel that ran is the kernel the case names (tests/test_conv_exact_cases_cpu.py holds the same table to tdvc_conv_select
    without a GPU);
  * conv_f32 in the whole-model fp32 mode: all four instantiations, the LoopFilter's frame slices (SliceWindow), a residual narrower than
    the output, fp32 GDN; each row's call class is asserted to be the class its table entry declares (the fp32 guard of
    tests/test_fp32_ops_gpu.py compares those classes with production's);
  * kernels that walk their tiles in both directions run three times: twice under tdvc_debug_set_conv_walk(1) -- consecutive launches
    necessarily walk in opposite directions, whatever the parity was on entry -- and once under (0); all three must give the
    reference's bits.  The walk direction must never change a bit of the output."""
import ctypes
from contextlib import contextmanager

import pytest
import torch

from tests import helpers_conv_dispatch as HD
from tests import helpers_conv_exact as X

pytestmark = pytest.mark.gpu

SENT = 7.0                    # sentinel of every byte a launch must not touch (an exact fp16 / fp32 value no case computes everywhere)


def _ops():
    from tdvc_amd import ops
    return ops


def _call(name, value):
    from tdvc_amd import _lib
    fn = getattr(_lib.lib(), name)
    fn.argtypes, fn.restype = [ctypes.c_int], None
    fn(value)


@contextmanager
def switched(case):
    """the case's debug switches, restored whatever happens: a failing case must not leak a switched-off kernel"""
    try:
        for setter, off, _ in case.switches:
            _call(setter, off)
        yield
    finally:
        for setter, _, on in case.switches:
            _call(setter, on)
        _call("tdvc_debug_set_conv_walk", -1)          # re-reads the environment
        _call("tdvc_debug_set_pair_geometry", 0)


def last_kernel():
    from tdvc_amd import _lib
    return _lib.lib().tdvc_last_conv_kernel().decode()


class Window:
    """a channel window [off, off + C) of a wider, sentinel-filled NHWC buffer"""

    def __init__(self, ops, N, H, W, C, dtype=torch.float16, before=0, after=0, content=None):
        self.buf = torch.full((N, H, W, before + C + after), SENT, dtype=dtype, device="cuda")
        self.off, self.C = before, C
        self.fm = ops.FM(self.buf).ch(before, C) if before or after else ops.FM(self.buf)
        if content is not None:          # (N, c, H, W) fp32 on the CPU, c <= C: zero-padded to the window
            self.fill(content)
        self.start = self.buf.clone()

    def fill(self, content):
        nhwc = torch.zeros(self.buf.shape[:3] + (self.C,), dtype=self.buf.dtype)
        nhwc[..., :content.shape[1]] = content.permute(0, 2, 3, 1).to(self.buf.dtype)
        self.buf[..., self.off:self.off + self.C] = nhwc.cuda()

    def reset(self):
        self.buf.copy_(self.start)

    def inside(self):
        return self.buf[..., self.off:self.off + self.C].float().cpu().permute(0, 3, 1, 2).contiguous()

    def outside_intact(self):
        o = torch.cat([self.buf[..., :self.off], self.buf[..., self.off + self.C:]], -1)
        return bool((o == SENT).all())

    def unchanged(self):
        return torch.equal(self.buf, self.start)


class SliceWindow:
    """the LoopFilter's frame slices: FM.as_slices(1, 4, 64) of a sentinel-filled 2 x H x W x 256 buffer -- image n of the view is channels
    [64 n, 64 n + 64) of every pixel of image 1, image stride 64 < pixel stride 256 -- or `count` of the four from slice `first` on
    (.batch(first, count)).  Same interface as Window."""

    def __init__(self, ops, H, W, dtype, first=0, count=4, content=None):
        self.buf = torch.full((2, H, W, 256), SENT, dtype=dtype, device="cuda")
        self.lo, self.n = 64 * first, count
        self.fm = ops.FM(self.buf).as_slices(1, 4, 64)
        if (first, count) != (0, 4):
            self.fm = self.fm.batch(first, count)
        assert self.fm.sn == 64 and self.fm.sp == 256 and self.fm.N == count
        if content is not None:          # (count, c <= 64, H, W) fp32 on the CPU
            nhwc = torch.zeros(H, W, count, 64, dtype=dtype)
            nhwc[..., :content.shape[1]] = content.permute(2, 3, 0, 1).to(dtype)
            self.buf[1, :, :, self.lo:self.lo + 64 * count] = nhwc.reshape(H, W, 64 * count).cuda()
        self.start = self.buf.clone()

    def reset(self):
        self.buf.copy_(self.start)

    def inside(self):
        v = self.buf[1, :, :, self.lo:self.lo + 64 * self.n].float().cpu()
        return v.reshape(v.shape[0], v.shape[1], self.n, 64).permute(2, 3, 0, 1).contiguous()

    def outside_intact(self):
        o = self.buf.clone()
        o[1, :, :, self.lo:self.lo + 64 * self.n] = SENT
        return bool((o == SENT).all())

    def unchanged(self):
        return torch.equal(self.buf, self.start)


def first_mismatch(got, want):
    """where the kernel is wrong: the failing pixel, channel or tile index usually names the line"""
    bad = (got != want).nonzero()
    n, c, y, x = (int(v) for v in bad[0])
    rows, cols, chans = (torch.unique(bad[:, i]).tolist() for i in (2, 3, 1))
    return (f"{len(bad)} of {got.numel()} values differ; first at (n {n}, c {c}, y {y}, x {x}): got {float(got[n, c, y, x])!r}, want {float(want[n, c, y, x])!r}; "
            f"rows {rows[0]}..{rows[-1]} ({len(rows)}), columns {cols[0]}..{cols[-1]} ({len(cols)}), channels {chans[:8]} ({len(chans)})")


def check(case, d, got, tag, report):
    """got: (N, view channels, H, W) fp32 from the output window"""
    want = torch.zeros_like(got)
    if case.grade == "f64":
        want = want.double()
        want[:, :d.ref.shape[1]] = d.ref
        tol = torch.zeros_like(want)
        tol[:, :d.ref.shape[1]] = d.tol
        err = (got.double() - want).abs()
        worst = float((err / tol.clamp_min(X.TINY16)).max())
        report(f"conv exact {case.id} [{tag}]: max |d| / bound = {worst:.3f}, max |d| = {float(err.max()):.3e}")
        assert bool((err <= tol).all()), f"{case.id} [{tag}]: {int((err > tol).sum())} values outside the bound, worst ratio {worst:.3f}"
        return
    want[:, :d.ref.shape[1]] = d.ref
    assert torch.equal(got, want), f"{case.id} [{tag}] ({case.kernel}, {case.form}): " + first_mismatch(got, want)


def launches(case):
    """(walk mode, tag) per launch: both directions and the forced-forward walk for the kernels that have a reverse walk"""
    if case.kernel.split("(")[0] in X.REVERSE_WALKERS:
        return [(1, "alternating walk, first"), (1, "alternating walk, second"), (0, "forward walk")]
    return [(-1, "single launch")]


@pytest.mark.parametrize("case", X.CASES, ids=[c.id for c in X.CASES])
def test_conv_exact(case, report):
    ops = _ops()
    from tdvc_amd import _lib as L
    d = X.reference(case, X.make_data(case))
    kh, kw, stride, pad, taps = X.window(case)
    Ho, Wo = X.out_map(case)
    yH, yW = (2 * Ho, 2 * Wo) if case.out == "shuffle" else (Ho, Wo)
    yv, _ = X.y_channels(case)
    v = case.views
    f32 = torch.float32
    sl = (3, 1) if case.slices == "last1" else (0, 4)
    if case.slices:
        x = SliceWindow(ops, case.H, case.W, f32, *sl, content=d.x)
    else:
        x = Window(ops, case.N, case.H, case.W, X.x_channels(case), f32 if case.x_f32 else torch.float16, 8 * v, 8 * v, d.x)
    pc = ops.pack_conv(d.w, d.b, stride=stride, pad=pad, taps=taps, shuffle=case.out == "shuffle")
    res = {}
    for key, kind, r, (b, a) in (("res", case.res, d.r1, (0, 8)), ("res2", case.res2, d.r2, (16, 24))):
        if kind and case.slices:
            res[key] = SliceWindow(ops, yH, yW, f32 if kind == "f32" else torch.float16, *sl, content=r)
        elif kind:
            rc = case.res_c if key == "res" and case.res_c else yv          # res_c: a dense residual map narrower than y
            res[key] = Window(ops, case.N, yH, yW, rc, f32 if kind == "f32" else torch.float16, b * v, a * v, r[:, :rc])
    kwargs = dict(act=case.act, slope=case.slope, round16=case.round16, **{k: w.fm for k, w in res.items()})
    nchw = None
    if case.bcast:
        y = Window(ops, case.N, Ho, Wo, 256, before=8, after=16, content=d.slices if case.bcast == "inplace" else None)
        src = Window(ops, case.N, Ho, Wo, 256, before=16, after=8, content=d.slices) if case.bcast == "outofplace" else None
        kwargs.update(out=ops.FM(y.buf).ch(8, 64), bcast_T=4, bcast_slope=0.2)
        if src is not None:
            kwargs["res"] = ops.FM(src.buf).ch(16, 64)
            res["slice source"] = src
    elif case.out == "nchw":
        nchw = torch.full((case.N, case.cout, Ho, Wo), SENT, device="cuda")
        kwargs["nchw_out"] = nchw
    elif case.slices:
        y = SliceWindow(ops, yH, yW, f32 if case.out == "f32" else torch.float16, *sl)
        kwargs["out"] = y.fm
    else:
        y = Window(ops, case.N, yH, yW, yv, f32 if case.out == "f32" else torch.float16, 8 * v, case.narrow + 16 * v)
        kwargs["out"] = y.fm
    if case.gdn:
        kwargs.update(square=True, gdn=case.gdn, aux=x.fm)

    if case.x_f32 and case.bias:             # the row's call class (the fp32 guard compares these with production's) is that of this very launch
        real = X.conv_f32_class(L, ops.conv_desc(x.fm, pc, **kwargs)[0])
        assert real == X.conv_f32_class(L, X.guard_desc(L, ops._pick_ck, case)), (case.id, real)
        assert real[4] == X.f32_variant(case), (case.id, real[4])

    def launch():
        sums = [] if case.chan_sum else None
        if case.bias:
            ops.conv(x.fm, pc, chan_sum=sums, **kwargs)
        else:                            # ops.conv always passes a bias pointer: the bias-free descriptor goes to tdvc_conv2d directly
            desc = ops.conv_desc(x.fm, pc, **kwargs)[0]
            desc.bias = None
            L.check(L.lib().tdvc_conv2d(ctypes.byref(desc), ops._stream()), "conv2d")
        return sums

    with switched(case):
        for mode, tag in launches(case):
            if nchw is not None:
                nchw.fill_(SENT)
            else:
                y.reset()
            _call("tdvc_debug_set_conv_walk", mode)
            sums = launch()
            assert HD.outcome(last_kernel()) == case.kernel, f"{case.id}: ran on {last_kernel()}"
            torch.cuda.synchronize()
            if nchw is not None:
                check(case, d, nchw.cpu(), tag, report)
            else:
                check(case, d, y.inside(), tag, report)
                assert y.outside_intact(), f"{case.id} [{tag}]: wrote outside the output window"
            if case.chan_sum:            # fused channel sums: the sums of the stored values, exact on integer data
                assert sums, f"{case.id}: no fused channel sum offered"
                part = sums[0][0]
                assert torch.equal(part.sum(1).cpu(), d.ref.sum((2, 3))), f"{case.id} [{tag}]: channel sums"
        assert x.unchanged() and all(w.unchanged() for w in res.values()), f"{case.id}: an input buffer changed"


@pytest.mark.parametrize("case", X.PAIR_CASES, ids=[c.id for c in X.PAIR_CASES])
def test_conv_pair_exact(case, report):
    ops = _ops()
    d = X.reference(case, X.make_data(case))
    v = case.views
    x = Window(ops, case.N, case.H, case.W, 64, before=8 * v, after=8 * v, content=d.x)
    r2 = Window(ops, case.N, case.H, case.W, 64, before=16 * v, after=24 * v, content=d.r2) if case.res2 else None
    y = Window(ops, case.N, case.H, case.W, 64, before=8 * v, after=16 * v)
    pp = ops.pack_conv_pair(d.w.cuda(), d.b.cuda(), d.w2.cuda(), d.b2.cuda())
    assert ops.conv_pair_supported(x.fm, y.fm, r2.fm if r2 else None)
    with switched(case):
        for geo, tag in ((2, "30-column strips"), (4, "62-column strips")):
            y.reset()
            _call("tdvc_debug_set_pair_geometry", geo)
            ops.conv_pair(x.fm, pp, out=y.fm, act1=case.act, slope1=case.slope, act2=case.act2, slope2=case.slope2, add_input=case.add_input,
                          res2=r2.fm if r2 else None)
            torch.cuda.synchronize()
            check(case, d, y.inside(), tag, report)
            assert y.outside_intact(), f"{case.id} [{tag}]: wrote outside the output window"
        assert x.unchanged() and (r2 is None or r2.unchanged()), f"{case.id}: an input buffer changed"
