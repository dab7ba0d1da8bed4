"""PSNR and MS-SSIM of the evaluation loop (`tools/predict.py:87-100`), on the GPU.

`ms_ssim` / `ssim` keep the signatures of `main/model/ms_ssim_torch.py:87-191` (float32 NCHW inputs, `data_range`,
`size_average`, `weights`, optional 1-D `win`); every level is one HIP pass over X and Y (`csrc/metrics.hip`) instead of
ten depthwise convolutions over five full-size products.  No CPU / eager fallback: the HIP library must load.

Both are differentiable (MS-SSIM as a training distortion, the reference's commented `train_lambda * msssim + bpp`,
`tools/train.py:133,139`): an input that requires grad takes a `torch.autograd.Function` whose backward is one HIP launch
per level, coarse to fine (`tdvc_ssim_level_backward`); `ms_ssim_value_and_grad` is the same without an autograd graph.
With no input requiring grad nothing changes: same launches, same bits."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .ops import launch

_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss_1d(size: int = 11, sigma: float = 1.5) -> list[float]:
    """ms_ssim_torch.py:5-18 (float32 arithmetic: exp, normalise by the sum)"""
    c = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).tolist()


def _check(X, Y, win_size):
    if X.dim() != 4:
        raise ValueError("Input images must 4-d tensor.")
    if X.dtype != Y.dtype or X.device != Y.device:
        raise ValueError("Input images must have the same dtype.")
    if X.shape != Y.shape:
        raise ValueError("Input images must have the same dimensions.")
    if win_size % 2 != 1:
        raise ValueError("Window size must be odd.")
    if not X.is_cuda:
        raise RuntimeError("tdvc_amd.metrics runs on the GPU only (no CPU fallback)")


def _level(X, Y, taps, data_range):
    """-> (ssim, cs) per image, already through the reference's (v + 1) / 2 (ms_ssim_torch.py:79-81)"""
    N, Cc, H, W = X.shape
    n = L.lib().tdvc_ssim_level_work_floats(N, Cc, H, W, len(taps))
    if n <= 0:
        raise ValueError(f"ms_ssim: image {H}x{W} smaller than the {len(taps)}-tap window (or window > 15 taps)")
    work = torch.empty(n, dtype=torch.float32, device=X.device)
    out = torch.empty(2, N, dtype=torch.float32, device=X.device)
    win = (C.c_float * len(taps))(*taps)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    launch("tdvc_ssim_level", X, Y, N, Cc, H, W, win, len(taps), c1, c2, out[0], out[1], work, n)
    return (out[0] + 1) / 2, (out[1] + 1) / 2


def _pool(X):
    N, Cc, H, W = X.shape
    Ho, Wo = (H + 2 * (H % 2) - 2) // 2 + 1, (W + 2 * (W % 2) - 2) // 2 + 1
    out = torch.empty(N, Cc, Ho, Wo, dtype=torch.float32, device=X.device)
    launch("tdvc_avgpool2_pad_f32", X, N * Cc, H, W, out)
    return out


def _taps(win_size, win_sigma, win):
    return gauss_1d(win_size, win_sigma) if win is None else [float(v) for v in torch.as_tensor(win).reshape(-1, torch.as_tensor(win).shape[-1])[0]]


def _prep(X, Y, win_size, win_sigma, win):
    return X.float().contiguous(), Y.float().contiguous(), _taps(win_size, win_sigma, win)


def _pooled(n):
    return (n + 2 * (n % 2) - 2) // 2 + 1


def _check_pyramid(H, W, levels, ntaps):
    """the ValueError of `_level`, for every level and before anything is launched"""
    for _ in range(levels):
        if H < ntaps or W < ntaps or ntaps > 15:
            raise ValueError(f"ms_ssim: image {H}x{W} smaller than the {ntaps}-tap window (or window > 15 taps)")
        H, W = _pooled(H), _pooled(W)


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _level_backward(X, Y, taps, data_range, g_ssim, g_cs, g_pool=None, scale=1.0):
    """d(sum_n g_ssim[n] * S[n] + g_cs[n] * CS[n]) / dX of one level (S, CS: the raw means, before (v + 1) / 2) plus the
    un-pooled gradient `g_pool` of the next level; g_ssim / g_cs: device tensors of N floats"""
    N, Cc, H, W = X.shape
    dx = torch.empty_like(X)
    win = (C.c_float * len(taps))(*taps)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    launch("tdvc_ssim_level_backward", X, Y, N, Cc, H, W, win, len(taps), c1, c2, g_ssim, g_cs, float(scale), g_pool, dx)
    return dx


def _upstream(g, like):
    """an autograd upstream gradient as a contiguous fp32 device vector (None -> zeros)"""
    return torch.zeros_like(like) if g is None else g.to(torch.float32).contiguous()


class _SsimFn(torch.autograd.Function):
    """(ssim, cs) per image of one level, both through (v + 1) / 2"""

    @staticmethod
    def forward(ctx, X, Y, taps, data_range):
        ctx.save_for_backward(X, Y)
        ctx.taps, ctx.data_range = taps, data_range
        return _level(X, Y, taps, data_range)

    @staticmethod
    def backward(ctx, gs, gc):
        X, Y = ctx.saved_tensors
        gs, gc = 0.5 * _upstream(gs, X.new_empty(X.shape[0])), 0.5 * _upstream(gc, X.new_empty(X.shape[0]))      # (v + 1) / 2
        dX = _level_backward(X, Y, ctx.taps, ctx.data_range, gs, gc) if ctx.needs_input_grad[0] else None
        dY = _level_backward(Y, X, ctx.taps, ctx.data_range, gs, gc) if ctx.needs_input_grad[1] else None
        return dX, dY, None, None


def ssim(X, Y, win_size=11, win_sigma=1.5, win=None, data_range=255, size_average=True, full=False):
    _check(X, Y, win_size)
    if _needs_grad(X, Y):
        taps = _taps(win_size, win_sigma, win)
        _check_pyramid(X.shape[2], X.shape[3], 1, len(taps))
        s, cs = _SsimFn.apply(X.float().contiguous(), Y.float().contiguous(), taps, float(data_range))
        if size_average:
            s, cs = s.mean(), cs.mean()
        return (s, cs) if full else s
    X, Y, taps = _prep(X, Y, win_size, win_sigma, win)
    s, cs = _level(X, Y, taps, float(data_range))
    if size_average:
        s, cs = s.mean(), cs.mean()
    return (s, cs) if full else s


_W_CACHE: dict = {}


def _weights_on(weights, device):
    """the level weights as a device tensor, made once per (weights, device): no host-to-device copy in a later call, so the
    differentiable path can be captured into a HIP graph"""
    key = (weights, device)
    if key not in _W_CACHE:
        _W_CACHE[key] = torch.tensor(weights, dtype=torch.float32, device=device)
    return _W_CACHE[key]


def _combine(mcs, s, w):
    """ms_ssim_torch.py:183-188 on the stacked cs [L][N] and the last level's ssim [N]: the expression of `ms_ssim` below"""
    return torch.prod((mcs[:-1] ** w[:-1].unsqueeze(1)) * (s ** w[-1]), dim=0)


def _pyramid(X, Y, taps, data_range, levels):
    """forward levels, keeping the pooled pyramids -> (xs, ys, stacked cs [L][N], ssim of the last level [N])"""
    xs, ys, mcs = [X], [Y], []
    for lv in range(levels):
        s, cs = _level(xs[-1], ys[-1], taps, data_range)
        mcs.append(cs)
        if lv + 1 < levels:
            xs.append(_pool(xs[-1]))
            ys.append(_pool(ys[-1]))
    return xs, ys, torch.stack(mcs, dim=0), s


def _pyramid_backward(xs, ys, taps, data_range, mcs, s, weights, grad_out, wrt_x, wrt_y):
    """msssim_level_grads, then the level backward from the coarsest level to the finest: one launch per level and operand"""
    levels, N = mcs.shape
    out = torch.empty(2 * levels + 1, N, dtype=torch.float32, device=mcs.device)
    g_ssim, g_cs = out[:levels], out[levels:2 * levels]
    w = (C.c_float * levels)(*weights)
    launch("tdvc_msssim_level_grads", mcs, s, w, levels, N, grad_out, out[2 * levels], g_ssim, g_cs)
    dX = dY = None
    for lv in reversed(range(levels)):
        if wrt_x:
            dX = _level_backward(xs[lv], ys[lv], taps, data_range, g_ssim[lv], g_cs[lv], dX)
        if wrt_y:
            dY = _level_backward(ys[lv], xs[lv], taps, data_range, g_ssim[lv], g_cs[lv], dY)
    return dX, dY


def _weights(weights):
    w = _WEIGHTS if weights is None else tuple(float(v) for v in weights)
    if not 1 <= len(w) <= 8:
        raise ValueError("ms_ssim: 1 to 8 level weights")
    return w


def ms_ssim_value_and_grad(X, Y, data_range=255, weights=None, win_size=11, win_sigma=1.5, win=None, grad_out=None, wrt="x"):
    """-> (ms [N], gradient): the per-image MS-SSIM of `ms_ssim(size_average=False)` (bit for bit) and
    d(sum_n grad_out[n] * ms[n]) / dX (wrt="x"), / dY (wrt="y") or the pair of them (wrt="both"), fp32, without an autograd
    graph.  grad_out: device tensor of N floats, default ones.  Nothing here waits for the GPU or copies to it after the
    first call with a given `weights`, so it can be captured into a HIP graph."""
    if wrt not in ("x", "y", "both"):
        raise ValueError('wrt must be "x", "y" or "both"')
    _check(X, Y, win_size)
    X, Y, taps = _prep(X.detach(), Y.detach(), win_size, win_sigma, win)
    weights = _weights(weights)
    _check_pyramid(X.shape[2], X.shape[3], len(weights), len(taps))
    if grad_out is not None:
        grad_out = grad_out.detach().to(device=X.device, dtype=torch.float32).contiguous()
        if grad_out.numel() != X.shape[0]:
            raise ValueError("grad_out must hold one value per image")
    xs, ys, mcs, s = _pyramid(X, Y, taps, float(data_range), len(weights))
    val = _combine(mcs, s, _weights_on(weights, X.device))
    dX, dY = _pyramid_backward(xs, ys, taps, float(data_range), mcs, s, weights, grad_out, wrt != "y", wrt != "x")
    return val, ((dX, dY) if wrt == "both" else dX if wrt == "x" else dY)


class _MsSsimFn(torch.autograd.Function):
    """per-image MS-SSIM; the backward is `ms_ssim_value_and_grad`'s, on the pyramids kept by the forward"""

    @staticmethod
    def forward(ctx, X, Y, taps, data_range, weights):
        xs, ys, mcs, s = _pyramid(X, Y, taps, data_range, len(weights))
        ctx.kept = (xs, ys, mcs, s, taps, data_range, weights)
        return _combine(mcs, s, _weights_on(weights, X.device))

    @staticmethod
    def backward(ctx, g):
        xs, ys, mcs, s, taps, data_range, weights = ctx.kept
        dX, dY = _pyramid_backward(xs, ys, taps, data_range, mcs, s, weights, _upstream(g, s), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dX, dY, None, None, None


def ms_ssim(X, Y, win_size=11, win_sigma=1.5, win=None, data_range=255, size_average=True, full=False, weights=None):
    """ms_ssim_torch.py:132-191: cs of the first levels and ssim of the last, weighted product"""
    _check(X, Y, win_size)
    if _needs_grad(X, Y):
        taps, weights = _taps(win_size, win_sigma, win), _weights(weights)
        _check_pyramid(X.shape[2], X.shape[3], len(weights), len(taps))
        val = _MsSsimFn.apply(X.float().contiguous(), Y.float().contiguous(), taps, float(data_range), weights)
        return val.mean() if size_average else val
    X, Y, taps = _prep(X, Y, win_size, win_sigma, win)
    w = torch.tensor(_WEIGHTS if weights is None else [float(v) for v in weights], dtype=torch.float32, device=X.device)
    mcs = []
    for lv in range(w.numel()):
        s, cs = _level(X, Y, taps, float(data_range))
        mcs.append(cs)
        if lv + 1 < w.numel():
            X, Y = _pool(X), _pool(Y)
    mcs = torch.stack(mcs, dim=0)
    val = torch.prod((mcs[:-1] ** w[:-1].unsqueeze(1)) * (s ** w[-1]), dim=0)
    return val.mean() if size_average else val


def psnr(recon: torch.Tensor, target: torch.Tensor) -> float:
    """tools/predict.py:87-88: 10 log10(1 / MSE) on [0, 1] images"""
    mse = float(torch.mean((recon.float() - target.float()) ** 2))
    return 10.0 * math.log10(1.0 / mse) if mse > 0 else float("inf")
