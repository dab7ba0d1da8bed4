"""The RGB head (FeatureFix.featdown: 3x3, 64 -> 3, clamp to [0, 1], planar fp32) on conv_n16's streamed form, conv_head3_kernel: byte-equal
to conv_n16's own kernel, which `tdvc_debug_enable_conv_head3(0)` keeps reachable.  Maps: 96 x 96 (the smallest multiple-of-8 map above
the 8192-pixel floor of the streaming kernels), 72 x 136 (a last strip of 8 columns), 65 x 130 (a last tile row of one row, a last strip of
two columns) and 128 x 192 (three full strips).  One and two images, the input as a channel window of a wider buffer, bias on and off,
values that clamp at both ends; one exact-arithmetic case from tests/helpers_conv_exact.py."""
import ctypes as C

import pytest
import torch

from tests import helpers_conv_exact as X
from util import randn, rnd16

pytestmark = pytest.mark.gpu


def _ops():
    from tdvc_amd import ops
    return ops


def _head(ops, x, pc, act, N, H, W, cout, streamed):
    """-> (planar fp32 result as int32 words, kernel name, 1 when conv_head3_kernel ran)"""
    lib = ops.L.lib()
    out = torch.full((N, cout, H, W), float("nan"), dtype=torch.float32, device="cuda")
    with ops.rgb_head_kernel(streamed):
        ops.conv(x, pc, act=act, nchw_out=out)
    return out.view(torch.int32), lib.tdvc_last_conv_kernel().decode(), lib.tdvc_debug_conv_n16_last_form()


def _input(ops, N, H, W, window, seed):
    if window:                                           # channels 64 .. 127 of a 192-channel buffer: pixel stride 192
        return ops.FM(rnd16(randn(N, H, W, 192, seed=seed)).half().cuda()).ch(64, 64)
    return ops.FM(rnd16(randn(N, H, W, 64, seed=seed)).half().cuda())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("H,W", [(96, 96), (72, 136), (65, 130), (128, 192)])
def test_streamed_head_equals_conv_n16(H, W, N, window, bias):
    ops = _ops()
    x = _input(ops, N, H, W, window, seed=H + W + N)
    # 576 products of N(0, 1) x N(0, 0.03^2) around 0.5: a third of the outputs below 0, a quarter above 1
    pc = ops.pack_conv(rnd16(randn(3, 64, 3, 3, seed=41) * 0.03), torch.tensor([0.5, 0.4, 0.6]) if bias else None, stride=1, pad=1)
    old, name_old, form_old = _head(ops, x, pc, ops.ACT_CLAMP01, N, H, W, 3, False)
    new, name_new, form_new = _head(ops, x, pc, ops.ACT_CLAMP01, N, H, W, 3, True)
    assert (name_old, form_old) == ("conv_n16", 0) and (name_new, form_new) == ("conv_n16", 1)
    assert torch.equal(new, old)
    v = new.view(torch.float32)
    assert not bool(torch.isnan(v).any()), "every output pixel is written"
    lo, hi = float((v == 0).float().mean()), float((v == 1).float().mean())
    assert lo > 0.05 and hi > 0.05 and lo + hi < 0.95, (lo, hi)          # the clamp works at both ends, and not everywhere


@pytest.mark.parametrize("cout,act", [(1, 0), (2, 2), (4, 1)])
def test_other_widths_and_activations(cout, act):
    """every width the form takes (1 .. 4 planar channels) and the other activations of the shared epilogue"""
    ops = _ops()
    N, H, W = 2, 65, 130
    x = _input(ops, N, H, W, True, seed=9)
    pc = ops.pack_conv(rnd16(randn(cout, 64, 3, 3, seed=42) * 0.03), randn(cout, seed=43) * 0.2, stride=1, pad=1)
    kw = dict(slope=0.1) if act == 2 else {}
    lib = ops.L.lib()
    outs = []
    for streamed in (False, True):
        out = torch.full((N, cout, H, W), float("nan"), dtype=torch.float32, device="cuda")
        with ops.rgb_head_kernel(streamed):
            ops.conv(x, pc, act=act, nchw_out=out, **kw)
        assert lib.tdvc_last_conv_kernel().decode() == "conv_n16" and lib.tdvc_debug_conv_n16_last_form() == int(streamed)
        outs.append(out.view(torch.int32))
    assert torch.equal(outs[0], outs[1])


def test_exact_arithmetic_case():
    """dyadic data (tests/helpers_conv_exact.py): the accumulation is exact in any order and a good share of the outputs (about one in
    six with this seed) are fractions inside (0, 1), the rest clamped; the planar fp32 store must hold clamp(conv + bias) bit for bit"""
    ops = _ops()
    case = X.Case("head3_dy_nchw_clamp", "conv_n16", "e4", 64, 3, X.W3, 2, 65, 131, act=X.ACT_CLAMP01, out="nchw", grade="dyadic", ragged=True)
    d = X.reference(case, X.make_data(case))
    x = ops.from_nchw(d.x.cuda())
    pc = ops.pack_conv(d.w, d.b, stride=1, pad=1)
    got, name, form = _head(ops, x, pc, ops.ACT_CLAMP01, case.N, 65, 131, 3, True)
    assert (name, form) == ("conv_n16", 1)
    assert torch.equal(got.view(torch.float32).cpu(), d.ref)
    inside = (d.ref > 0) & (d.ref < 1)
    assert float(inside.float().mean()) > 0.1 and bool((d.ref == 0).any()) and bool((d.ref == 1).any())       # a property of the data, not of the kernel


def test_layers_outside_the_form_run_as_before():
    ops = _ops()
    lib = ops.L.lib()
    pc = ops.pack_conv(rnd16(randn(3, 64, 3, 3, seed=41) * 0.03), torch.tensor([0.5, 0.4, 0.6]), stride=1, pad=1)
    # a 64 x 64 map is below the floor of the streaming kernels: the kernel it had before, whatever the switch says
    x = _input(ops, 1, 64, 64, False, seed=3)
    d = ops.conv_desc(x, pc, None, act=ops.ACT_CLAMP01, nchw_out=torch.empty((1, 3, 64, 64), device="cuda"))[0]
    want = lib.tdvc_conv_select(C.byref(d)).decode()
    assert want != "conv_n16"
    a, name_a, _ = _head(ops, x, pc, ops.ACT_CLAMP01, 1, 64, 64, 3, True)
    b, name_b, _ = _head(ops, x, pc, ops.ACT_CLAMP01, 1, 64, 64, 3, False)
    assert name_a == name_b == want and torch.equal(a, b)
    # conv_n16's other layers keep its own kernel: an fmap output, and the 7x7 flow head (16 -> 2, fp32)
    xl = _input(ops, 1, 96, 96, False, seed=4)
    ops.conv(xl, pc, act=ops.ACT_CLAMP01, out_dtype=torch.float32)
    assert lib.tdvc_last_conv_kernel().decode() == "conv_n16" and lib.tdvc_debug_conv_n16_last_form() == 0
    x16 = ops.FM(rnd16(randn(1, 96, 96, 16, seed=5)).half().cuda())
    ops.conv(x16, ops.pack_conv(randn(2, 16, 7, 7, seed=6) * 0.05, randn(2, seed=7), stride=1, pad=3), out_dtype=torch.float32)
    assert lib.tdvc_last_conv_kernel().decode() == "conv_n16" and lib.tdvc_debug_conv_n16_last_form() == 0
