"""Cases, bound and the genuinely-fp32 data of the exact tests of tdvc_dcn_fused on fp32 maps (dcn_fused_kernel<float>, csrc/dcn_common.h):
tests/test_dcn_f32_exact_gpu.py launches them, tests/test_dcn_f32_cases_cpu.py holds the table and the fp32 case to what they claim.

Cases, data and references are those of tests/helpers_dcn_exact.py (`X`).  Restated here is only what an fp32 map changes:

  epilogue   acc + bias -> one rounding to fp16 if round16 -> the activation in fp32 -> stored as it is in an fp32 y, rounded once more in
             an fp16 y.
  bound      X.f64_bound without its EPS16 |col| term (no sample is stored in fp16); with an fp32 y and no round16 nothing is rounded
             to fp16 at all and 4 EPS32 |ref| stands where the R16 terms stood.
  fp32 case  that bound is wider than the cost of keeping x, w or the mask logits in fp16, so FP32_CASE has data and a bound of its own
             (fp32_case_bound): an fp32 kernel passes, the reference with any one input rounded to fp16 misses by over 100 x.
"""
import functools

import torch

from tests import helpers_dcn_exact as X

# the launcher makes no size-dependent choice (one kernel, 8x8 tiles): the small maps of X.CASES with partial tiles on both axes, two
# images, less than one tile, channel windows with spare images, and infinite / huge offsets on 65x131
_BIG = ("m65x131_int_huge", "m65x131_n2_int_views_strided", "m65x131_dy_views")
CASES = [c for c in X.CASES if c.H * c.W < X.LDS_MIN_PIXELS or c.id in _BIG]
RUNS = [(c, y32) for c in CASES for y32 in (True, False)]

# the case that tells an fp32 kernel from a widened fp16 one: no input is an fp16 value, and every sample is sent to a random position of
# a 36 x 375 map, so the offsets are tens to hundreds of pixels long (fp16 ulp 1/64 .. 1/4 px there).  It has a bound of its own, fp32_case_bound
FP32_CASE = X.Case("f32_36x375_anywhere", 1, 36, 375, "wild", "f64", round16=False)
FP32_NNZ = 3                               # non-zero weights per output channel of FP32_CASE
FP32_POS_STEP = 2.0 ** -12                 # its sampling positions are multiples of this


def expected_exact(case, d, y32):
    """int / dyadic grades: the stored bits"""
    v = d.pre.float()
    assert bool((v.double() == d.pre).all()), case.id
    if case.round16:
        v = X.h16(v)
    v = X._act(v, case.act, case.slope)
    return v if y32 else X.h16(v)


def bound(case, d, y32):
    """per output, the terms of X.f64_bound that remain (see the module docstring)"""
    sum_w = d.w.double().abs().sum((1, 2, 3)).view(1, X.CH, 1, 1)
    xmax = float(d.x.abs().max())
    absb = d.b.double().abs().view(1, X.CH, 1, 1)
    absx_ref = d.abs_sum - absb
    scale = max(1.0, case.slope) if case.act == X.ACT_LRELU else 1.0
    n_round = int(case.round16) + int(not y32)
    rounding = n_round * X.R16 if n_round else 4 * X.EPS32
    return sum_w * (1e-5 * xmax + X.TINY16) + 600 * X.EPS32 * (absx_ref + absb) + rounding * scale * d.ref.abs() + X.TINY16


def fp32_case_bound(d):
    """per output of FP32_CASE, an fp32 y and no round16.  The bound of `bound` is built for dense weights (600 EPS32 for 576 products in
    any order, 1e-5 max|x| per sample) and is wider than the error of fp16 rounding of x, w or the logits; this case is built so that an
    fp32 kernel's error has a much smaller bound, counted rounding by rounding (EPS32 is the unit roundoff 2^-24):

      position    base + offset and the fractions lh, lw, 1 - lh, 1 - lw are exact: every position is a multiple of 2^-12 below 2048, and
                  so is every offset (23 bits); hh * hw is exact too (at most 24 bits)
      mask        expf to 1 ulp (2 EPS32; 4 allowed), 1 + e (1), the division (1; 5 allowed): 10 EPS32 relative, its sensitivity to e < 1
      sample      corner weight * mask (1), hh * hw (1 allowed), four products and three sums as an fma chain of non-negative weights
                  (4 roundings, each relative to at most sum_i |w_i x_i|): 6 EPS32
      product     W * col: 1 EPS32 (0 if the matrix unit fuses it)
      sum         each output channel has FP32_NNZ non-zero weights; a product with a zero weight is an exact zero and adding it rounds
                  nothing, so FP32_NNZ + 1 additions (the bias included) round, each relative to at most abs_sum, in any order

    together (17 + FP32_NNZ + 1) EPS32 abs_sum, taken as 24 EPS32 abs_sum, plus the 4 EPS32 |ref| of `bound`.  Nothing in it is an
    fp16 quantity."""
    assert 17 + FP32_NNZ + 1 <= 24
    return 24 * X.EPS32 * d.abs_sum + 4 * X.EPS32 * d.ref.abs()


def _reference(case, x, w, b, om, abs_sum=True):
    d = X.Data(x, w, b, om)
    d.off_ref = X._nchw(om[..., :18 * X.G]).double()
    d.mask_ref = torch.sigmoid(X._nchw(om[..., 18 * X.G:]).double())
    xd, wd, bd = x.double(), w.double(), b.double()
    d.pre = X.dcn_ref(xd, wd, bd, d.off_ref, d.mask_ref)
    if abs_sum:
        d.abs_sum = X.dcn_ref(xd.abs(), wd.abs(), bd.abs(), d.off_ref, d.mask_ref)
    d.ref = X._act(d.pre, case.act, case.slope)
    return d


@functools.lru_cache(maxsize=None)
def fp32_reference():
    """data of FP32_CASE (fp32 values that are no fp16 values) with its float64 reference; shared, callers must not modify it"""
    c = FP32_CASE
    gen = torch.Generator().manual_seed(5150)
    x = torch.randn(c.N, X.CH, c.H, c.W, generator=gen)
    # FP32_NNZ weights per output channel, of magnitude 0.5 .. 1.5, at (cin, tap) = divmod(37 k mod 576, 9) for k = 3 cout + j: 192
    # different places, every input channel group and every tap among them
    w = torch.zeros(X.CH, X.CH * 9)
    k = torch.arange(X.CH * FP32_NNZ).view(X.CH, FP32_NNZ)
    val = (0.5 + torch.rand(X.CH, FP32_NNZ, generator=gen)) * (torch.randint(0, 2, (X.CH, FP32_NNZ), generator=gen) * 2 - 1)
    w.scatter_(1, (37 * k) % (X.CH * 9), val)
    w = w.view(X.CH, X.CH, 3, 3)
    b = torch.randn(X.CH, generator=gen) * 0.01
    yy, xx = X.base_positions(c.H, c.W)                                   # (H, 1, 1, 9), (1, W, 1, 9)
    ty = torch.round(torch.rand(c.N, c.H, c.W, X.G, 9, generator=gen) * (c.H - 1) / FP32_POS_STEP) * FP32_POS_STEP
    tx = torch.round(torch.rand(c.N, c.H, c.W, X.G, 9, generator=gen) * (c.W - 1) / FP32_POS_STEP) * FP32_POS_STEP
    off = torch.stack([ty - yy.unsqueeze(0), tx - xx.unsqueeze(0)], -1)   # exact: multiples of 2^-12 below 2048
    logit = (torch.randn(c.N, c.H, c.W, 9 * X.G, generator=gen) * 3).clamp(-8, 8)
    om = torch.cat([off.reshape(c.N, c.H, c.W, 18 * X.G), logit], -1)
    return _reference(c, x, w, b, om)


FP16_VARIANTS = ("x", "w", "logits", "offsets")


@functools.lru_cache(maxsize=None)
def fp32_reference_through_fp16(which):
    """what a kernel that rounds one of its inputs to fp16 and widens it again would compute at best: the same reference with that
    input rounded (`which` of FP16_VARIANTS)"""
    d = fp32_reference()
    x, w, om = d.x, d.w, d.om.clone()
    if which == "x":
        x = X.h16(x)
    elif which == "w":
        w = X.h16(w)
    elif which == "logits":
        om[..., 18 * X.G:] = X.h16(om[..., 18 * X.G:])
    else:
        assert which == "offsets"
        om[..., :18 * X.G] = X.h16(om[..., :18 * X.G])
    return _reference(FP32_CASE, x, w, d.b, om, abs_sum=False).ref
