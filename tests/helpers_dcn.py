"""Offset regimes of the DCN tests at the fused kernel's geometry (8 groups x 8 channels, 3x3, stride 1, pad 1), shared by the
backward tests (tests/test_backward_ops_gpu.py) and the exact forward tests (tests/helpers_dcn_exact.py).  Pure torch / numpy."""
import numpy as np
import torch

G_DCN, C_DCN = 8, 64
DCN_REGIMES = ["subpixel", "coherent", "wild", "border", "integer"]


def rnd16(t):
    return t.half().float()


def far_stats(om, H, W):
    """bilinear corners (inside the map) of every (n, pixel, group, tap) sample, and those of them that fall outside the 24 x 24
    scatter window of the sample's 8 x 8 tile (dcn_col2im_kernel: the far path)"""
    o = om[..., :18 * G_DCN].double().numpy().reshape(om.shape[0], H, W, G_DCN, 9, 2)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = np.arange(9)
    h = (yy[:, :, None, None] - 1 + t // 3)[None] + o[..., 0]
    w = (xx[:, :, None, None] - 1 + t % 3)[None] + o[..., 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = np.floor(h), np.floor(w)
    wy0 = (yy // 8 * 8 - 8)[None, :, :, None, None]
    wx0 = (xx // 8 * 8 - 8)[None, :, :, None, None]
    active = far = 0
    for cy, cx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cyy, cxx = hl + cy, wl + cx
        act = inside & (cyy >= 0) & (cyy <= H - 1) & (cxx >= 0) & (cxx <= W - 1)
        inwin = (cyy - wy0 >= 0) & (cyy - wy0 < 24) & (cxx - wx0 >= 0) & (cxx - wx0 < 24)
        active += int(act.sum())
        far += int((act & ~inwin).sum())
    return active, far, h, w


def offsets(regime, N, H, W, seed, band=None):
    """(N, H, W, 144) fp16-valued offsets [g*18 + 2t: dy, +1: dx]; `band` = (r0, r1): the regime only on those rows, sub-pixel elsewhere"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    shape = (N, H, W, G_DCN, 9, 2)
    if regime == "subpixel":
        o = rn(*shape) * 0.5
    elif regime == "coherent":
        o = rn(*shape) * 0.3
        o[..., 0] += 11.3
        o[..., 1] -= 7.6
    elif regime == "wild":
        o = rn(*shape) * 9.0
    elif regime == "border":
        # sample positions anywhere in [-2, H + 1] x [-2, W + 1]: every border, the open intervals (-1, 0) and (H-1, H) included
        yy = torch.arange(H).view(1, H, 1, 1, 1).float() - 1 + torch.arange(9).view(1, 1, 1, 1, 9).div(3, rounding_mode="floor")
        xx = torch.arange(W).view(1, 1, W, 1, 1).float() - 1 + torch.arange(9).view(1, 1, 1, 1, 9) % 3
        th = torch.rand(N, H, W, G_DCN, 9, generator=gen) * (H + 3) - 2
        tw = torch.rand(N, H, W, G_DCN, 9, generator=gen) * (W + 3) - 2
        o = torch.stack([th - yy, tw - xx], -1)
    elif regime == "integer":
        o = torch.randint(-12, 13, shape, generator=gen).float()
    else:
        raise ValueError(regime)
    if band is not None:
        calm = rn(*shape) * 0.3
        rows = torch.zeros(1, H, 1, 1, 1, 1, dtype=torch.bool)
        rows[:, band[0]:band[1]] = True
        o = torch.where(rows, o, calm)
    return rnd16(o.reshape(N, H, W, 18 * G_DCN))
