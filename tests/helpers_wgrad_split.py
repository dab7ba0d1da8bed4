"""conv_wgrad_split's arithmetic (csrc/conv_backward.hip, conv_wgrad_split_kernel) restated on the CPU: the weight-gradient bilinear map
dW = sum over pixels of dY * X applied to the bf16 parts of tests/helpers_conv_split.split3, in float64 (every part is a bf16 value, every
product of two parts exact).  SIX names (dY part, X part) here: the products gh xh, gh xm, gm xh, gm xm, gh xl, gl xh."""
import torch
import torch.nn.functional as F

from tests import helpers_conv_split as S

# the cases of tests/test_conv_wgrad_f32_gpu.py::CASES on which a lost second-order product shows: K = N Ho Wo <= 108 roundings of the
# fp32 chain, so the 2^-16 relative size of a dropped product stands well above the chain's error (at K = 308 it is only 8 x above)
DISCRIMINATORS = ("1x1_s2_128_128", "1x1_512_426", "3x3_128_128_1x1map")


def _bilinear(case, g64, x64, wshape):
    """float64 dW of y = conv(x [squared], W) for the output gradient g64 (the conv's own, un-shuffled output): linear in g64 and in x64"""
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, w, None, stride=stride, padding=pad)
    gw, = torch.autograd.grad(y, w, g64)
    return gw


def operands(case, x, gy):
    """the fp32 operands the kernel contracts: dY as the conv's own output gradient (pixel_unshuffle of a sub-pixel layer's) and X, squared in
    fp32 with one rounding where the case says so"""
    shuffle, square_x = case[9], case[10]
    g = F.pixel_unshuffle(gy, 2) if shuffle else gy
    xs = (x * x) if square_x else x
    return g.float().contiguous(), xs.float().contiguous()


def wgrad_terms(case, x, gy, terms, wshape):
    """float64 weight gradient summed over the given (dY part, X part) products of the split operands"""
    g, xs = operands(case, x, gy)
    gp, xp = S.split3(g), S.split3(xs)
    out = None
    for a, b in terms:
        t = _bilinear(case, gp[a].double(), xp[b].double(), wshape)
        out = t if out is None else out + t
    return out


def wgrad_exact(case, x, gy, wshape):
    g, xs = operands(case, x, gy)
    return _bilinear(case, g.double(), xs.double(), wshape)


def wgrad_fp32_chain(case, x, gy, wshape):
    """the same gradient by torch's fp32 autograd: a chain of K fp32 multiply-adds per element"""
    name, N, cin, cout, k, stride, pad, H, W, shuffle, square_x, masked = case
    g, xs = operands(case, x, gy)
    w = torch.zeros(wshape, dtype=torch.float32, requires_grad=True)
    gw, = torch.autograd.grad(F.conv2d(xs, w, None, stride=stride, padding=pad), w, g)
    return gw
