"""`tdvc_conv_desc::flow`: OffsetGen's level-1 fusion conv (1x1, 128 -> 64, LeakyReLU, on conv_mfma_v5) with the flow added in its epilogue
is byte for byte the conv followed by `tdvc_add_flow`.  Maps of 96 x 96 (whole 16 x 32 workgroup tiles) and 72 x 136 (ragged last tile row
and column), one and two images, the output as a channel window; flow values that overflow fp16, zeros, and values that put the sum
exactly between two fp16 numbers.  On a 32 x 32 map the selected kernel does not add the flow: `ops.conv` falls back to the two launches."""
import ctypes as C

import pytest
import torch

from util import randn, rnd16

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B


def _ops():
    from tdvc_amd import ops
    return ops


def _bits(fm):
    base = fm.t.view(torch.int16).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


@pytest.fixture()
def add_flow_calls(monkeypatch):
    ops = _ops()
    calls = []
    real = ops.add_flow
    monkeypatch.setattr(ops, "add_flow", lambda off, flow: (calls.append(1), real(off, flow))[1])
    return calls


def _layer(ops):
    return ops.pack_conv(rnd16(randn(64, 128, 1, 1, seed=21) * 0.09), randn(64, seed=22) * 0.1, stride=1, pad=0)


def _half_ulp(v):
    """half the spacing of the fp16 numbers at |v| (fp32 tensor of fp16 values): v + it lies exactly between two of them"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 11.0)


def _flow_for(plain_nhwc):
    """an fp32 flow (N, H, W, 2) for a conv output (N, H, W, 64) given as float: random in general; rows 0-3 of every image carry the
    special values -- overflow to +-Inf, exact zeros, signed zero, and rounding ties against channel 0 (x) / channel 1 (y)"""
    N, H, W, _ = plain_nhwc.shape
    f = randn(N, H, W, 2, seed=31) * 4.0
    f[:, 0, :, 0], f[:, 0, :, 1] = 1.0e5, -1.0e5
    f[:, 1, :, :] = 0.0
    f[:, 1, ::2, 1] = -0.0
    f[:, 2, :, 0] = _half_ulp(plain_nhwc[:, 2, :, 0])
    f[:, 2, :, 1] = -_half_ulp(plain_nhwc[:, 2, :, 1])
    f[:, 3, :, 0] = 3.0 * _half_ulp(plain_nhwc[:, 3, :, 0])
    f[:, 3, :, 1] = 65504.0                                                # the largest fp16 number: overflows only where the conv value is large enough
    return f


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("H,W", [(96, 96), (72, 136)])
def test_flow_in_the_epilogue_equals_conv_then_add_flow(H, W, N, window, add_flow_calls):
    ops = _ops()
    lib = ops.L.lib()
    x = ops.FM(rnd16(randn(N, H, W, 128, seed=H + N)).half().cuda())
    pc = _layer(ops)
    lr = dict(act=ops.ACT_LRELU, slope=0.1)
    want = ops.conv(x, pc, **lr)
    assert lib.tdvc_last_conv_kernel().decode() == "conv_mfma_v5"
    plain = _bits(want).view(torch.float16).float().cpu()
    fbuf = torch.zeros(N, H, W, 4)
    fbuf[..., 1:3] = _flow_for(plain)
    fbuf[..., 0], fbuf[..., 3] = 123.0, -77.0                               # neighbours of the two flow channels: never added
    flow = ops.FM(fbuf.cuda()).ch(1, 2)
    ops.add_flow(want, flow)
    assert add_flow_calls == [1]
    want = _bits(want)

    if window:
        buf = ops.FM.empty(N, H, W, 192)
        buf.t.view(torch.int16).fill_(SENTINEL)
        out = buf.ch(64, 64)
    else:
        buf = out = ops.FM.empty(N, H, W, 64)
    got = ops.conv(x, pc, out=out, flow=flow, **lr)
    assert lib.tdvc_last_conv_kernel().decode() == "conv_mfma_v5"
    assert add_flow_calls == [1], "the flow must have been added by the conv itself"
    got = _bits(got)
    assert torch.equal(got, want)
    if window:
        w = buf.t.view(torch.int16)
        assert bool((w[..., :64] == SENTINEL).all()) and bool((w[..., 128:] == SENTINEL).all()), "channels outside the window were written"
    # the special rows did what they are there for
    v = got.view(torch.float16)
    assert bool(torch.isinf(v[:, 0]).all()) and bool((v[:, 0, :, 0] > 0).all()) and bool((v[:, 0, :, 1] < 0).all())
    assert torch.equal(v[:, 1].float().cpu(), plain[:, 1]), "a flow of zero leaves the conv's own values"
    tie = plain[:, 2, :, 0].cuda().double() + fbuf[:, 2, :, 1].cuda().double()
    assert bool((tie.half().double() != tie).any()), "no rounding tie in the test data"


def test_small_map_falls_back_to_two_launches(add_flow_calls):
    ops = _ops()
    lib = ops.L.lib()
    N, H, W = 2, 32, 32
    x = ops.FM(rnd16(randn(N, H, W, 128, seed=77)).half().cuda())
    pc = _layer(ops)
    lr = dict(act=ops.ACT_LRELU, slope=0.1)
    flow = ops.FM((randn(N, H, W, 2, seed=78) * 4.0).cuda())
    want = ops.conv(x, pc, **lr)
    assert lib.tdvc_last_conv_kernel().decode() == "conv_mfma_v9"
    ops.add_flow(want, flow)
    d = ops.conv_desc(x, pc, None, **lr)[0]
    assert lib.tdvc_conv_flow_supported(C.byref(d)) == 0
    got = ops.conv(x, pc, flow=flow, **lr)
    assert add_flow_calls == [1, 1], "the flow must have been added by add_flow behind the conv"
    assert torch.equal(_bits(got), _bits(want))


def test_flow_is_refused_where_it_cannot_be_meant():
    ops = _ops()
    x = ops.FM(rnd16(randn(1, 96, 96, 128, seed=5)).half().cuda())
    flow = ops.FM(torch.zeros(1, 96, 96, 2, device="cuda"))
    with pytest.raises(ops.L.TdvcHipError):
        ops.conv(x, _layer(ops), flow=flow, chan_sum=[])
    d = ops.conv_desc(x, _layer(ops), None, act=ops.ACT_LRELU, slope=0.1)[0]
    d.flow = ops.FM(torch.zeros(1, 96, 95, 2, device="cuda")).desc()       # another geometry: rejected before anything is launched
    assert ops.L.lib().tdvc_conv2d(C.byref(d), None) == -1 and b"flow" in ops.L.lib().tdvc_last_error()
