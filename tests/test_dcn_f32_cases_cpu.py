"""Without a GPU: the case table of tests/test_dcn_f32_exact_gpu.py covers what it claims, and its fp32 case tells an fp32 kernel
from one that keeps x, w, the mask logits or the offsets in fp16."""
import pytest
import torch

from tests import helpers_dcn_exact as X
from tests import helpers_dcn_f32 as F


def test_case_table_covers_the_small_maps():
    shapes = {(c.N, c.H, c.W) for c in F.CASES}
    for s in ((1, 13, 21), (2, 20, 28), (1, 16, 32), (1, 3, 5), (1, 1, 9)):
        assert s in shapes, s
    assert {c.views for c in F.CASES} == {0, 1, 2}
    assert any(c.regime == "huge" and (c.H, c.W) == (65, 131) for c in F.CASES)
    assert {c.grade for c in F.CASES} == {"int", "dyadic", "f64"}
    assert {(c.round16, y32) for c, y32 in F.RUNS} == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(X.tile_count(c, "gather") > 1 for c in F.CASES if c.H * c.W > 64)            # more than one workgroup


def test_fp32_case_is_what_its_bound_assumes():
    c, d = F.FP32_CASE, F.fp32_reference()
    off_y, off_x = d.om[..., 0:18 * X.G:2], d.om[..., 1:18 * X.G:2]
    for t, share in ((d.x, 0.99), (d.w[d.w != 0], 0.99), (off_x, 0.95), (off_y, 0.9), (d.om[..., 18 * X.G:], 0.99)):
        # hardly a value is an fp16 value (the row offsets are the shorter ones, and below 1 most multiples of 2^-12 are fp16 values)
        assert float((X.h16(t) != t).float().mean()) > share
    h, w = X.sample_positions(c, d)
    inside = (h > -1) & (h < c.H) & (w > -1) & (w < c.W)
    assert float(inside.float().mean()) > 0.99                                              # every sample carries a weight
    # positions and offsets are multiples of 2^-12 below 2048: base + offset and the bilinear fractions are exact in fp32
    assert bool(((h.double() / F.FP32_POS_STEP) % 1 == 0).all()) and bool(((w.double() / F.FP32_POS_STEP) % 1 == 0).all())
    off = d.om[..., :18 * X.G].double()
    assert bool(((off / F.FP32_POS_STEP) % 1 == 0).all()) and float(off.abs().max()) < 2048
    # FP32_NNZ weights per output channel, every group of input channels and every tap among them
    nz = (d.w != 0).view(X.CH, X.G, 8, 9)
    assert bool((nz.sum((1, 2, 3)) == F.FP32_NNZ).all())
    assert bool(nz.any(0).any(1).all()), "a (group, tap) pair no output channel reads"
    assert float(d.om[..., 18 * X.G:].abs().max()) <= 8


def test_fp32_case_bound_holds_for_fp32_arithmetic():
    """the same operator in fp32 on the CPU (the oracle's code, not the kernel) stays inside the bound: it can be met"""
    d = F.fp32_reference()
    got = X.dcn_ref(d.x, d.w, d.b, d.off_ref.float(), torch.sigmoid(X._nchw(d.om[..., 18 * X.G:])))
    assert got.dtype == torch.float32
    assert bool(((got.double() - d.ref).abs() <= F.fp32_case_bound(d)).all())


# worst |err| / bound that rounding this one input to fp16 must reach at least, and the share of outputs it must push outside
FACTORS = {"x": 100, "w": 100, "logits": 100, "offsets": 1000}


@pytest.mark.parametrize("which", F.FP16_VARIANTS)
def test_fp32_case_discriminates(which):
    """one input rounded to fp16, everything else exact: the GPU test cannot pass on a kernel that keeps that input in fp16"""
    d = F.fp32_reference()
    tol = F.fp32_case_bound(d)
    err16 = (F.fp32_reference_through_fp16(which) - d.ref).abs()
    worst, outside = float((err16 / tol).max()), float((err16 > tol).float().mean())
    print(f"{which} rounded to fp16: max |err| / bound {worst:.0f}, outside the bound {outside:.3f} of the outputs")
    assert worst > FACTORS[which] and outside > 0.9, (which, worst, outside)
