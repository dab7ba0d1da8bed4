"""The gates of tests/test_conv_wgrad_split_gpu.py, checked without a GPU on the weight-gradient bilinear map in float64
(tests/helpers_wgrad_split.py over tests/helpers_conv_split.py's split3 / SIX / five_term_sets).

On the three discriminator cases the six-term sum, rounded to fp32 once, must be closer to the exact gradient than torch's fp32 chain, and
the best five-term sum at least 12 x further away than that chain.  Then a kernel held to <= 4 x the fp32 kernel's error (gate b) and to
3 x below the best five-term sum (gate d) can meet both, and one that loses a second-order product meets neither.  Measured with torch
fp32 autograd as the chain: five-term / chain 18.0 (1x1_s2_128_128, K = 108), 22.1 (1x1_512_426, K = 70), 70 (3x3_128_128_1x1map, K = 2);
six-term / chain 0.19, 0.23, 0.82.  At K = 308 (3x3_128_128) the five-term ratio is about 8: no discriminator."""
import pytest
import torch

import test_conv_wgrad_f32_gpu as WG
from tests import helpers_conv_split as S
from tests import helpers_wgrad_split as HW

BY_NAME = {c[0]: c for c in WG.CASES}


def _case(name):
    case = BY_NAME[name]
    x, w, b, live = WG._case_data(case)
    gy = WG._reference(case, x, w, b)[0]
    return case, x, gy, tuple(w.shape)


def test_the_six_products_are_conv_splits():
    assert len(S.SIX) == 6 and set(S.SIX) == {("h", "h"), ("h", "m"), ("m", "h"), ("m", "m"), ("h", "l"), ("l", "h")}
    assert all(len(t) == 5 for t in S.five_term_sets()) and len(S.five_term_sets()) == 3


def test_exact_gradient_is_the_references():
    """the bilinear restatement gives the float64 gradient tests/test_conv_wgrad_f32_gpu.py::_reference differentiates"""
    case, x, gy, wshape = _case("1x1_s2_128_128")
    w = torch.zeros(wshape)
    gw = WG._reference(case, x, w, torch.zeros(wshape[0]))[1]
    assert torch.equal(HW.wgrad_exact(case, x, gy, wshape), gw)


@pytest.mark.parametrize("name", HW.DISCRIMINATORS)
def test_gates_can_be_met_and_discriminate(name, report):
    case, x, gy, wshape = _case(name)
    exact = HW.wgrad_exact(case, x, gy, wshape)
    chain = S.rms(HW.wgrad_fp32_chain(case, x, gy, wshape).double() - exact)
    six = S.rms(HW.wgrad_terms(case, x, gy, S.SIX, wshape).float().double() - exact)          # rounded to fp32 once, as the kernel's store
    five = min(S.rms(HW.wgrad_terms(case, x, gy, t, wshape) - exact) for t in S.five_term_sets())
    report(f"wgrad split gates {name}: fp32 chain rms {chain:.3e}; six-term rounded once / chain = {six / chain:.2f}; "
           f"best five-term / chain = {five / chain:.1f}")
    assert chain > 0
    assert six < chain, f"{name}: the six-term sum ({six:.3e}) is not below the fp32 chain's error ({chain:.3e})"
    assert five >= 12 * chain, f"{name}: the best five-term sum is only {five / chain:.1f} x the fp32 chain's error"


def test_dropped_terms_bound():
    """the three products the kernel does not compute stay below (2 u^3 + u^4) |g| |x| per product"""
    case, x, gy, wshape = _case("1x1_512_426")
    g, xs = HW.operands(case, x, gy)
    gp, xp = S.split3(g), S.split3(xs)
    for parts, v in ((gp, g), (xp, xs)):
        assert torch.equal(parts["h"].double() + parts["m"].double() + parts["l"].double(), v.double())
    exact, six = HW.wgrad_exact(case, x, gy, wshape), HW.wgrad_terms(case, x, gy, S.SIX, wshape)
    absprod = HW._bilinear(case, g.double().abs(), xs.double().abs(), wshape)
    assert bool(((six - exact).abs() <= S.DROPPED * absprod * (1 + 1e-9)).all())
