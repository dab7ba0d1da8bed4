"""`tdvc_avgpool2_pyramid`: both SPyNet image pyramids in one launch are, level by level and image by image, the bytes of five chained
`tdvc_avgpool2` calls per map.  Maps: one 32 x 32 block (a single workgroup per map), 64 x 96 and 96 x 160 (several blocks in both
directions, more columns than rows)."""
import pytest
import torch

from util import randn

pytestmark = pytest.mark.gpu


def _ops():
    from tdvc_amd import ops
    return ops


def _bits(fm):
    """the int32 words of an fp32 FM view, (N, H, W, C), as a copy"""
    base = fm.t.view(torch.int32).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


def _chain(ops, x):
    out = []
    for _ in range(5):
        x = ops.avgpool2(x)
        out.append(x)
    return out


def _maps(N, H, W, seed):
    """two fp32 maps of 4 channels with values whose sums round (random mantissas, mixed magnitudes and signs)"""
    a = randn(N, H, W, 4, seed=seed) * torch.exp(randn(N, H, W, 4, seed=seed + 1) * 3.0)
    b = randn(N, H, W, 4, seed=seed + 2)
    b[..., 3] = 0.0                                   # the model's maps: RGB padded to four channels
    return a.cuda(), b.cuda()


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("H,W", [(32, 32), (64, 96), (96, 160)])
def test_pyramid_equals_five_chained_calls(H, W, N):
    ops = _ops()
    ta, tb = _maps(N, H, W, seed=7 * H + W + N)
    a, b = ops.FM(ta), ops.FM(tb)
    assert ops.avgpool2_pyramid_supported(a, b)
    la, lb = ops.avgpool2_pyramid(a, b)
    for name, got, want in (("a", la, _chain(ops, a)), ("b", lb, _chain(ops, b))):
        assert len(got) == 5
        for k in range(5):
            assert (got[k].N, got[k].H, got[k].W, got[k].C) == (N, H >> (k + 1), W >> (k + 1), 4)
            g, w = _bits(got[k]), _bits(want[k])
            for n in range(N):
                assert torch.equal(g[n], w[n]), f"map {name}, level {k + 1}, image {n}"


def test_pyramid_scalar_path_on_channel_windows():
    """three-channel windows of wider buffers (pixels that are not aligned 4-float words): the kernel's scalar form"""
    ops = _ops()
    N, H, W = 2, 64, 96
    ta, tb = (randn(N, H, W, 5, seed=s).cuda() for s in (91, 92))
    a, b = ops.FM(ta).ch(1, 3), ops.FM(tb).ch(2, 3)
    assert ops.avgpool2_pyramid_supported(a, b)
    la, lb = ops.avgpool2_pyramid(a, b)
    for got, want in ((la, _chain(ops, a)), (lb, _chain(ops, b))):
        for k in range(5):
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"level {k + 1}"


def test_pyramid_rejects_what_it_cannot_take():
    import ctypes as C
    ops = _ops()
    L = ops.L
    a = ops.FM(torch.zeros(1, 48, 64, 4, device="cuda"))
    assert not ops.avgpool2_pyramid_supported(a, a)                       # 48 is no multiple of 32
    ok = ops.FM(torch.zeros(1, 64, 64, 4, device="cuda"))
    lv = [ops.FM(torch.zeros(1, 64 >> k, 64 >> k, 4, device="cuda")) for k in range(1, 6)]
    good = (L.FMapDesc * 5)(*[f.desc() for f in lv])
    bad = (L.FMapDesc * 5)(*[f.desc() for f in lv[:4]], lv[3].desc())    # the last level has the geometry of the fourth
    d = ok.desc()
    assert L.lib().tdvc_avgpool2_pyramid(C.byref(d), C.byref(d), good, bad, None) == -1
    assert b"level 5" in L.lib().tdvc_last_error()
    da = a.desc()
    assert L.lib().tdvc_avgpool2_pyramid(C.byref(da), C.byref(da), good, good, None) == -1
