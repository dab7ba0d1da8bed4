"""conv_split (csrc/conv_split.hip, ops.f32_split): conv_f32's contract on the bf16 matrix pipe.  Every layer shape of tests/test_conv_f32_gpu.py
and the forms of its other tests, launched through ops.conv under the switch and held to: the kernel's name, conv_f32's own gate against
torch fp32 (RT = AT = 2e-5), exactly zero padded channels, and -- against float64 on the same inputs -- an rms error of at most 4 x
conv_f32's (sqrt(6) for six times the roundings, the rest for the MFMA's internal summation order).  On the two K <= 128 shapes the error
must also be 3 x below that of the best FIVE-term sum (tests/helpers_conv_split.py): a kernel that loses or doubles a product fails."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_f32_gpu as CF
from tests import helpers_conv_split as S
from util import assert_close, fm_to_cpu, randn, to_fm

pytestmark = pytest.mark.gpu

RT, AT = CF.RT, CF.AT
RATIO = 4.0
EXTRA = [
    # name, N, cin, cout, k, stride, pad, H, W
    ("3x3_8_64_halfstep", 1, 8, 64, 3, 1, 1, 9, 11),       # ck8 == 1: two taps per k-step, the padded half step
    ("7x7_64_32", 1, 64, 32, 7, 1, 3, 9, 11),
    ("7x7_16_2", 1, 16, 2, 7, 1, 3, 8, 8),                 # a single cout tile
]
CASES = list(CF.CASES) + EXTRA
FIVE_TERM_CASES = ("1x1_128_128", "1x1_s2_64_128")       # K <= 128


def _ops():
    from tdvc_amd import ops
    return ops


def _both(ops, x, pc, **kw):
    """(conv_f32's map, conv_split's map) of one call, the kernel names asserted"""
    lib = ops.L.lib()
    y32 = ops.conv(x, pc, **kw)
    assert lib.tdvc_last_conv_kernel() == b"conv_f32"
    with ops.f32_split(True):
        ys = ops.conv(x, pc, **kw)
    assert lib.tdvc_last_conv_kernel() == b"conv_split"
    assert not ops.F32_SPLIT
    return y32, ys


def _ratio(what, got_split, got_f32, ref64, report):
    es, ef = S.rms(got_split.double() - ref64), S.rms(got_f32.double() - ref64)
    report(f"conv_split {what}: rms error vs float64 {es:.3e}, conv_f32 {ef:.3e}, ratio {es / ef:.2f}")
    assert es <= RATIO * ef, f"conv_split {what}: rms error {es:.3e} is {es / ef:.2f} x conv_f32's {ef:.3e} (gate {RATIO})"
    return es


def _padded_zero(fm, cout):
    """gate (c): the channels a map carries beyond the layer's cout are exactly zero (they feed the next layer)"""
    if fm.C > cout:
        assert float(fm_to_cpu(fm)[:, cout:].abs().max()) == 0.0


def _lrelu64(v64):
    return torch.where(v64 > 0, v64, v64 * float(torch.tensor(0.01, dtype=torch.float32)))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_split_plain(case, report):
    ops = _ops()
    name, N, cin, cout, k, s, p, H, W = case
    x = randn(N, cin, H, W, seed=1)
    w = randn(cout, cin, k, k, seed=2) * (1.0 / (cin * k * k) ** 0.5)
    b = randn(cout, seed=3) * 0.1
    ref = F.leaky_relu(F.conv2d(x, w, b, stride=s, padding=p), 0.01)
    pc = ops.pack_conv(w, b, stride=s, pad=p)
    y32, ys = _both(ops, to_fm(x, ops, Cpad=ops.pad8(cin), dtype=torch.float32), pc, act=ops.ACT_LRELU, slope=0.01)
    assert ys.f32 and (ys.N, ys.H, ys.W, ys.C) == (y32.N, y32.H, y32.W, y32.C)
    got = fm_to_cpu(ys, cout)
    assert_close(got, ref, RT, AT, f"conv_split {name}", report)
    assert ys.C == ops.pad8(cout)
    _padded_zero(ys, cout)
    x64, w64, b64 = x.double(), w.double(), b.double()
    ref64 = _lrelu64(F.conv2d(x64, w64, b64, stride=s, padding=p))
    es = _ratio(name, got, fm_to_cpu(y32, cout), ref64, report)
    if name in FIVE_TERM_CASES:
        e5 = min(S.rms(_lrelu64(S.conv_terms(x, w, t, stride=s, padding=p) + b64.view(1, -1, 1, 1)) - ref64) for t in S.five_term_sets())
        report(f"conv_split {name}: best five-term sum's rms error {e5:.3e} = {e5 / es:.1f} x the kernel's")
        assert 3.0 * es <= e5, f"conv_split {name}: rms error {es:.3e} is not 3 x below a five-term sum's {e5:.3e}: a product is lost or doubled"


def test_conv_split_masked5x5(report):
    """the type-A masked 5x5 context conv 128 -> 256 (a tap list of 12)"""
    ops = _ops()
    from tdvc_amd.model.coder import MaskedConv2d
    M = 128
    cp = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
    with torch.no_grad():
        cp.weight.copy_(randn(2 * M, M, 5, 5, seed=4) * 0.02)
        cp.bias.copy_(randn(2 * M, seed=5) * 0.1)
    x = randn(1, M, 6, 9, seed=6) * 3.0
    wm, bb = (cp.weight.detach() * cp.mask), cp.bias.detach()
    pc = ops.pack_conv(cp.weight.detach(), bb, stride=1, pad=2, taps=cp.live_taps())
    y32, ys = _both(ops, to_fm(x, ops, dtype=torch.float32), pc)
    assert_close(fm_to_cpu(ys, 2 * M), F.conv2d(x, wm, bb, padding=2), RT, AT, "conv_split masked 5x5", report)
    _padded_zero(ys, 2 * M)
    _ratio("masked 5x5", fm_to_cpu(ys), fm_to_cpu(y32), F.conv2d(x.double(), wm.double(), bb.double(), padding=2), report)


def test_conv_split_gdn_shuffle_residual(report):
    """the forms of test_conv_f32_gdn_shuffle_residual: GDN / inverse GDN (the pool squares in fp32, then splits), PixelShuffle store, fp32
    and fp16 residuals, fp16 output"""
    ops = _ops()
    C, H, W = 128, 12, 20
    x = randn(1, C, H, W, seed=7)
    gamma = (randn(C, C, seed=8).abs() * 0.02 + 0.1 * torch.eye(C)).reshape(C, C, 1, 1)
    beta = randn(C, seed=9).abs() + 0.5
    r = randn(1, C, H, W, seed=10)
    pc = ops.pack_conv(gamma, beta, stride=1, pad=0)
    xf, rf = to_fm(x, ops, dtype=torch.float32), to_fm(r, ops, dtype=torch.float32)
    x64 = x.double()
    for inverse in (False, True):
        what = f"{'i' if inverse else ''}GDN + fp32 residual"
        norm = F.conv2d(x * x, gamma, beta)
        ref = x * (torch.sqrt(norm) if inverse else torch.rsqrt(norm)) + r
        y32, ys = _both(ops, xf, pc, square=True, gdn=ops.GDN_INV if inverse else ops.GDN_FWD, aux=xf, res=rf)
        assert_close(fm_to_cpu(ys, C), ref, RT, AT, f"conv_split {what}", report)
        _padded_zero(ys, C)
        # float64 of the kernel's function: the square is ONE fp32 rounding in both kernels (part of the input of the pool)
        n64 = F.conv2d((x * x).double(), gamma.double(), beta.double())
        _ratio(what, fm_to_cpu(ys), fm_to_cpu(y32), x64 * (n64.sqrt() if inverse else n64.rsqrt()) + r.double(), report)
    # sub-pixel conv: 128 -> 4 x 64, PixelShuffle(2), fp16 residual, fp16 output (the last layer of g_s + prediction)
    w = randn(256, C, 3, 3, seed=11) * 0.03
    b = randn(256, seed=12) * 0.1
    r16 = randn(1, 64, 2 * H, 2 * W, seed=13).half().float()
    pcs = ops.pack_conv(w, b, stride=1, pad=1, shuffle=True)
    y16, ys16 = _both(ops, xf, pcs, res=to_fm(r16, ops), out_dtype=torch.float16)
    assert not ys16.f32
    assert_close(fm_to_cpu(ys16, 64), F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2) + r16, 2e-3, 2e-3, "conv_split sub-pixel + fp16 residual -> fp16", report)
    _padded_zero(ys16, 64)
    # both kernels round the same fp32 sum to fp16: the ratio is about 1
    _ratio("sub-pixel + fp16 residual -> fp16", fm_to_cpu(ys16, 64), fm_to_cpu(y16, 64),
           F.pixel_shuffle(F.conv2d(x64, w.double(), b.double(), padding=1), 2) + r16.double(), report)
    y32, ys = _both(ops, xf, pcs)
    assert_close(fm_to_cpu(ys, 64), F.pixel_shuffle(F.conv2d(x, w, b, padding=1), 2), RT, AT, "conv_split sub-pixel fp32", report)
    _padded_zero(ys, 64)
    _ratio("sub-pixel fp32", fm_to_cpu(ys), fm_to_cpu(y32), F.pixel_shuffle(F.conv2d(x64, w.double(), b.double(), padding=1), 2), report)


def test_conv_split_inf_behind_the_border():
    """a stride-2 3x3 conv with the single tap (0, 0) reads only odd rows and columns; row 0 and column 0 are what the CLAMPED addresses of
    the out-of-image taps of the first output row / column point at.  Inf there must contribute exact zeros: the mask comes before the split"""
    ops = _ops()
    x = randn(1, 16, 9, 9, seed=14)
    w = randn(32, 16, 3, 3, seed=15) * 0.1
    b = randn(32, seed=16) * 0.1
    xi = x.clone()
    xi[:, :, 0, :] = float("inf")
    xi[:, :, :, 0] = float("-inf")
    pc = ops.pack_conv(w, b, stride=2, pad=1, taps=[(0, 0)])
    with ops.f32_split(True):
        clean = fm_to_cpu(ops.conv(to_fm(x, ops, dtype=torch.float32), pc))
        got = fm_to_cpu(ops.conv(to_fm(xi, ops, dtype=torch.float32), pc))
        assert ops.L.lib().tdvc_last_conv_kernel() == b"conv_split"
    wz = torch.zeros_like(w)
    wz[:, :, 0, 0] = w[:, :, 0, 0]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    assert_close(got, F.conv2d(x, wz, b, stride=2, padding=1), RT, AT, "conv_split single tap s2")


@pytest.mark.parametrize("cout,cin,k,ck", [(64, 64, 3, 32), (2, 16, 7, 16), (40, 8, 3, 8), (426, 512, 1, 64)])
def test_packed_split_layout(cout, cin, k, ck):
    """PackedConv.packed_split() against a python restatement of the layout: the fp32 fragment order, every value split, per k-step the
    h, m and l planes of 64 lanes x 8 bf16; built lazily and made stale by repack() as the fp32 twin is"""
    ops = _ops()
    w = randn(cout, cin, k, k, seed=17)
    pc = ops.pack_conv(w, None, stride=1, pad=k // 2, ck=ck)
    assert pc.wsplit is None
    got = pc.packed_split()
    assert got.dtype == torch.bfloat16 and pc.wsplit is got and pc.packed_split() is got
    taps = [(dy, dx) for dy in range(k) for dx in range(k)]
    want = S.ref_pack_split(S.ref_pack_f32(w.numpy(), cin, taps, ck))
    assert got.numel() == want.size
    assert np.array_equal(got.float().cpu().numpy().reshape(want.shape), want)
    pc.wsrc.mul_(2.0)
    pc.repack()
    assert pc.wsplit is None and pc.wsplit_buf is got                # stale: the buffer is kept for the next use
    again = pc.packed_split()
    assert again.data_ptr() == got.data_ptr() and np.array_equal(again.float().cpu().numpy().reshape(want.shape), 2.0 * want)
