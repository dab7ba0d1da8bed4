"""`tdvc_scale_act_res3`: the scaling pass with a second result, y3 = b + sign * y from the rounded y, is byte for byte the two launches
it replaces (`scale_act_res` into y, then `scale_act_res(b, y3, res=y, res_sign=sign)`).  64 channels; totals that are no multiple of the
grid-stride unroll (256 threads x 4 items), strided residual and `b` views, gate on and off, both activations, NaN / Inf in `b`."""
import pytest
import torch

from util import randn

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B


def _ops():
    from tdvc_amd import ops
    return ops


def _bits(fm):
    base = fm.t.view(torch.int16).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


def _inputs(N, H, W, strided, seed):
    ops = _ops()
    mk = lambda s, Cb: (randn(N, H, W, Cb, seed=s) * 2.0).half().cuda()
    a = ops.FM(mk(seed, 64))
    if strided:                                        # 64-channel windows of wider buffers, as prediction1 sits in the 256-channel stack
        r = ops.FM(mk(seed + 1, 256)).ch(192, 64)
        b = ops.FM(mk(seed + 2, 192)).ch(64, 64)
    else:
        r, b = ops.FM(mk(seed + 1, 64)), ops.FM(mk(seed + 2, 64))
    gate = torch.sigmoid(randn(N, 64, seed=seed + 3)).cuda()
    return a, r, b, gate


def _two_launches(ops, a, r, b, gate, act, slope):
    y, y3 = ops.FM.empty(a.N, a.H, a.W, 64), ops.FM.empty(a.N, a.H, a.W, 64)
    ops.scale_act_res(a, y, gate=gate, act=act, slope=slope, res=r)
    ops.scale_act_res(b, y3, res=y, res_sign=-1.0)
    return _bits(y), _bits(y3)


def _fused(ops, a, r, b, gate, act, slope):
    y, y3 = ops.FM.empty(a.N, a.H, a.W, 64), ops.FM.empty(a.N, a.H, a.W, 64)
    y.t.view(torch.int16).fill_(SENTINEL)
    y3.t.view(torch.int16).fill_(SENTINEL)
    ops.scale_act_res3(a, y, b, y3, -1.0, gate=gate, act=act, slope=slope, res=r)
    return _bits(y), _bits(y3)


@pytest.mark.parametrize("act,slope", [(0, 0.0), (1, 0.0), (2, 0.1)])                  # none (the model's), ReLU, LeakyReLU
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("N,H,W", [(1, 40, 52), (2, 96, 96), (1, 33, 47)])        # 16.25, 144 and 12.1 rounds of 1024 items
def test_three_outputs_equal_two_launches(N, H, W, strided, gated, act, slope):
    ops = _ops()
    a, r, b, gate = _inputs(N, H, W, strided, seed=100 + H)
    g = gate if gated else None
    want_y, want_y3 = _two_launches(ops, a, r, b, g, act, slope)
    got_y, got_y3 = _fused(ops, a, r, b, g, act, slope)
    assert torch.equal(got_y, want_y)
    assert torch.equal(got_y3, want_y3)
    assert not bool((got_y3 == SENTINEL).all())


def test_map_larger_than_one_grid_sweep():
    """more items than 4096 workgroups x 256 threads x 4: the grid-stride loop goes round, with a ragged last round"""
    ops = _ops()
    N, H, W = 1, 728, 728                               # 728 * 728 * 8 = 4 239 872 items > 4 194 304
    assert H * W * 8 > 4096 * 1024 and (H * W * 8) % 1024 != 0
    a, r, b, gate = _inputs(N, H, W, False, seed=300)
    want_y, want_y3 = _two_launches(ops, a, r, b, gate, 0, 0.0)
    got_y, got_y3 = _fused(ops, a, r, b, gate, 0, 0.0)
    assert torch.equal(got_y, want_y) and torch.equal(got_y3, want_y3)


def test_nan_and_inf_in_b_propagate_as_in_the_separate_launch():
    ops = _ops()
    a, r, b, gate = _inputs(1, 40, 52, False, seed=400)
    words = b.t.view(torch.int16)
    words[0, 0, 0, 0] = 0x7C00                          # +Inf
    words[0, 0, 1, 1] = -1024                           # 0xFC00, -Inf
    words[0, 1, 0, 2] = 0x7E00                          # quiet NaN
    words[0, 1, 1, 3] = 0x7E01                          # NaN with a payload
    words[0, 2, 0, 4] = 0x7BFF                          # 65504: b - y overflows where y < -16
    a.t[0, 2, 0, 4] = -60000.0
    a.t[0, 3, 3, 5] = float("inf")                      # Inf in y itself: b - Inf
    want_y, want_y3 = _two_launches(ops, a, r, b, gate, 0, 0.0)
    got_y, got_y3 = _fused(ops, a, r, b, gate, 0, 0.0)
    assert torch.equal(got_y, want_y) and torch.equal(got_y3, want_y3)
    y3 = got_y3.view(torch.float16)
    assert torch.isinf(y3[0, 0, 0, 0]) and torch.isinf(y3[0, 0, 1, 1]) and torch.isnan(y3[0, 1, 0, 2]) and torch.isnan(y3[0, 1, 1, 3])


def test_other_dtypes_fall_back_to_two_launches():
    ops = _ops()
    a, r, b, gate = _inputs(1, 40, 52, False, seed=500)
    y32, y3 = ops.FM.empty(1, 40, 52, 64, dtype=torch.float32), ops.FM.empty(1, 40, 52, 64)
    ops.scale_act_res3(a, y32, b, y3, -1.0, gate=gate, res=r)                          # fp32 y: not the fused kernel's form
    want = ops.FM.empty(1, 40, 52, 64)
    ops.scale_act_res(b, want, res=y32, res_sign=-1.0)
    assert torch.equal(_bits(y3), _bits(want))
    import ctypes as C
    lib = ops.L.lib()
    da, d32, db, d3 = a.desc(), y32.desc(), b.desc(), y3.desc()
    assert lib.tdvc_scale_act_res3(C.byref(da), None, 0, 0.0, None, 1.0, C.byref(d32), C.byref(db), -1.0, C.byref(d3), None) == -1
    dy = want.desc()
    assert lib.tdvc_scale_act_res3(C.byref(da), None, 0, 0.0, None, 1.0, C.byref(dy), C.byref(db), -1.0, C.byref(dy), None) == -1      # y3 aliases y
