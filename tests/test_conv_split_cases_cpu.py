"""CPU: the arithmetic conv_split is held to (tests/helpers_conv_split.py) is what its documentation says -- the bf16 triple is exact, the
six-term sum is within the stated bound of the full product, a five-term sum is not nearly as good -- and the two entry points are bound."""
import ctypes as C

import pytest
import torch

from tdvc_amd import _lib as L
from tests import helpers_conv_split as S
from util import randn

EPS32 = 2.0 ** -24


def _inputs():
    """normal draws, wide-range magnitudes, exact bf16 values, values with all 24 significand bits set, signed zeros"""
    wide = randn(4096, seed=41) * torch.exp2(torch.randint(-60, 60, (4096,), generator=torch.Generator().manual_seed(42)).float())
    full = torch.tensor([(2.0 ** 24 - 1) * 2.0 ** e for e in (-30, -24, 0, 10)] + [1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -8 + 2.0 ** -16), 3.0e38, (1.0 + 2.0 ** -23) * 2.0 ** -100])
    return torch.cat([randn(4096, seed=40), wide, randn(64, seed=43).to(torch.bfloat16).float(), full, torch.tensor([0.0, -0.0])])


def test_split3_is_exact():
    v = _inputs()
    p = S.split3(v)
    for k in "hml":                              # every part is a bf16 value
        assert torch.equal(p[k], p[k].to(torch.bfloat16).float())
    # h + m + l == v bit for bit: the partial sums h + m and (h + m) + l are exact in float64, compared as fp32
    back = (p["h"].double() + p["m"].double() + p["l"].double()).float()
    assert torch.equal(back.view(torch.int32)[v != 0], v.view(torch.int32)[v != 0]) and float(back[v == 0].abs().max()) == 0.0
    # the parts shrink by 2^-8 each (round to nearest: half an ulp of 8 bits)
    assert bool((p["m"].abs() <= S.U * p["h"].abs()).all()) and bool((p["l"].abs() <= S.U * S.U * p["h"].abs() * (1 + S.U)).all())


def test_split3_tiny_values_lose_only_the_l_part():
    """below about 2^-110 the l part (2^-16 of v) leaves bf16's normal range: the documented limit"""
    v = (1.0 + randn(512, seed=46).abs()) * 2.0 ** -114
    p = S.split3(v)
    err = (p["h"].double() + p["m"].double() + p["l"].double() - v.double()).abs()
    assert float(err.max()) <= 2.0 ** -134 and float(err.max()) > 0.0               # half an ulp of bf16's subnormals; h and m stay exact
    assert bool(((v - p["h"] - p["m"]).abs() <= S.U * S.U * v.abs()).all())


@pytest.mark.parametrize("K", [128, 1152])
def test_six_terms_within_the_dropped_bound_and_five_are_not(K):
    cin, k = (128, 1) if K == 128 else (128, 3)
    x = randn(1, cin, 12, 12, seed=44)
    w = randn(32, cin, k, k, seed=45) * K ** -0.5
    full = torch.nn.functional.conv2d(x.double(), w.double())
    mag = torch.nn.functional.conv2d(x.double().abs(), w.double().abs())
    six = S.conv_terms(x, w, S.SIX)
    assert bool(((six - full).abs() <= S.DROPPED * mag).all())
    # an fp32 fma chain over K terms: the yardstick of the issue's table (rms error about sqrt(K) EPS32 |acc| / 2)
    e6 = S.rms(six - full)
    e5 = min(S.rms(S.conv_terms(x, w, t) - full) for t in S.five_term_sets())
    assert e5 > 20 * e6                          # a lost second-order product costs 2^-16 per MAC, against the 2^-24 of the six-term sum


def test_new_symbols_are_bound():
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 17
    assert L.SIGNATURES["tdvc_conv2d_split"] == L.SIGNATURES["tdvc_conv2d_f32"]
    assert L.SIGNATURES["tdvc_pack_conv_weights_indexed_bf16x3"] == L.SIGNATURES["tdvc_pack_conv_weights_indexed_f32"]
    assert lib.tdvc_conv2d_split(None, None) != 0 and b"null descriptor" in lib.tdvc_last_error()      # rejected before any launch
    assert lib.tdvc_pack_conv_weights_indexed_bf16x3(*([None] * 7), 64, 64, 9, 32, None, None) != 0
    # an fp16 map is refused exactly as tdvc_conv2d_f32 refuses it, and the last kernel's name is not touched by a refusal
    d = L.ConvDesc()
    before = lib.tdvc_last_conv_kernel()
    assert lib.tdvc_conv2d_split(C.byref(d), None) == lib.tdvc_conv2d_f32(C.byref(d), None) != 0
    assert lib.tdvc_last_conv_kernel() == before
