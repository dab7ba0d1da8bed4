"""The case table, the data and the references of the exact forward-DCN tests (tests/test_dcn_exact_gpu.py launches the cases on
the GPU, tests/test_dcn_exact_cases_cpu.py holds, without a GPU, the table to what it claims).

tdvc_dcn_fused has three forward implementations behind one entry point (csrc/dcn.hip): `gather` (dcn_fused_kernel<half_t>,
csrc/dcn_common.h, 8x8 tiles, corners through L1), `planar` (the same kernel on the group-planar copy of x) and `lds` (dcn_lds_kernel,
8x16 tiles, maps of 8192 pixels or more).  All of them take the sampling rule from dcn_corners and store through dcn_store
(csrc/dcn_common.h).  Geometry is the fused kernel's own: 64 -> 64 channels, 8 groups, 3x3, stride 1, pad 1.

Three grades of data, all made here:

  int     x, w in {-2..2} (w thinned to `density`), integer bias and offsets, mask logits +-60000: 1 / (1 + exp(-m)) is exactly 1
          or 0 by IEEE arithmetic alone (exp underflows to 0 or overflows to inf).  Every modulated sample is an integer fp16
          value, every partial sum an exact fp32 integer in any order, every output an fp16 value: the stored bits are the
          reference's whatever the path, the tile walk or the window.
  dyadic  offsets in multiples of 0.5, logits in DYADIC_LOGITS, w in multiples of 2^-9, bias of 2^-3.  Bilinear weights are in
          {0, 1/4, 1/2, 1} times a mask in {0, 1/2, 1}: samples are multiples of 2^-3 of magnitude <= 2 (exact in fp16), the
          accumulation is exact (units of 2^-12), the outputs are no fp16 values -- the stored bits are decided by the epilogue's rounding
          sequence, restated in `epilogue()`.
  f64     fp16-rounded random x, w and logits (sigma 1.5) against dcn_v2_forward_ref in float64, with the bound of `f64_bound()`.

The preconditions of the exact grades are asserted on the REFERENCE (`check_exact`), never on the kernel's output."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from tests import helpers_dcn as HDCN

G, CH = HDCN.G_DCN, HDCN.C_DCN
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_CLAMP01 = 0, 1, 2, 3

EPS16 = 2.0 ** -11            # the constants of tests/test_backward_ops_gpu.py
EPS32 = 2.0 ** -24
TINY16 = 2.0 ** -24
R16 = EPS16 + 8 * EPS32

LDS_MIN_PIXELS = 8192         # tdvc_dcn_fused: the LDS-window kernel from this map size on
BIG = 60000.0                 # an fp16 value; as a logit it saturates the sigmoid, as an offset it lies outside every map
# Logit 0 rests on the hardware returning exactly 1.0 for exp2(-0) and exactly 0.5 for the reciprocal of 2.0 (DESIGN.md has what
# the suite measured)
DYADIC_LOGITS = (-BIG, 0.0, BIG)

# x / y channel windows of the 192-channel buffer MCNet.run hands the operator, and the width of the wider offset/mask buffer
VIEW_BUF_C, VIEW_X0, VIEW_Y0, VIEW_OM_C = 192, 64, 128, 232

OLD_REGIMES = tuple(HDCN.DCN_REGIMES)                    # random offsets: subpixel, coherent, wild, border, integer
NEW_REGIMES = ("edges", "coherent_int", "half", "huge")
PATHS = ("gather", "planar", "lds")
SMALL, ALL = ("gather", "planar"), ("gather", "planar", "lds")


@dataclass(frozen=True)
class Case:
    id: str
    N: int
    H: int
    W: int
    regime: str               # OLD_REGIMES | NEW_REGIMES
    grade: str                # "int" | "dyadic" | "f64"
    paths: tuple = SMALL
    shift: tuple = (0, 0)     # coherent_int / half: the integer displacement the offsets scatter around
    act: int = ACT_NONE
    slope: float = 0.0
    round16: bool = True
    views: int = 0            # 1: x, y channel windows of one sentinel-filled 192-channel buffer, om 216 of 232 channels;
                              # 2: the same, and the batch stride is twice H*W*C (every other image of the buffers is spare)
    density: float = 0.5
    seed: int = 0


C = Case
L01, L25 = dict(act=ACT_LRELU, slope=0.1), dict(act=ACT_LRELU, slope=0.25)
CASES = [
    # ---- gather and planar on small maps.  13x21: 2x3 tiles, N = 1: the remainder remap with q = 0; 20x28: 12 tiles, N = 2 the
    # identity regime, N = 1 the remainder remap with q = 1, r = 4 (below 8 tiles min(c, r) is c whatever r is); 16x32: 8 tiles,
    # the divisible-by-8 remap; 3x5 and 1x9: less than one tile, every sample near a border
    C("s13x21_int_edges", 1, 13, 21, "edges", "int"),
    C("s13x21_dy_edges_lrelu01_r16", 1, 13, 21, "edges", "dyadic", **L01),
    C("s13x21_f64_wild", 1, 13, 21, "wild", "f64", round16=False),
    C("s13x21_dy_views", 1, 13, 21, "half", "dyadic", act=ACT_RELU, views=1),
    C("s20x28_int_coherent", 1, 20, 28, "coherent_int", "int", shift=(3, -2), act=ACT_RELU),
    C("s20x28_n2_dy_half_relu", 2, 20, 28, "half", "dyadic", act=ACT_RELU, round16=False),
    C("s20x28_n2_f64_border_lrelu01_r16", 2, 20, 28, "border", "f64", **L01),
    C("s16x32_dy_edges_clamp_r16", 1, 16, 32, "edges", "dyadic", act=ACT_CLAMP01),
    C("s16x32_int_integer_lrelu25", 1, 16, 32, "integer", "int", round16=False, **L25),
    C("s3x5_dy_edges_none", 1, 3, 5, "edges", "dyadic", round16=False),
    C("s1x9_int_edges_relu_r16", 1, 1, 9, "edges", "int", act=ACT_RELU),
    C("s1x9_dy_edges_lrelu25_r16", 1, 1, 9, "edges", "dyadic", **L25),
    # ---- all three paths at or just above 8192 pixels.  65x131: 9x9 = 81 LDS tiles and 9x17 = 153 gather tiles, both 1 mod 8
    # (N = 1: the remainder remap, N = 2: identity); 64x128: 64 LDS tiles, the divisible remap, most tiles on the interior fast
    # path; 9x911: shorter than the 20-row window, no tile interior (114 LDS tiles: remainder 2); 600x14: narrower than a tile
    C("m65x131_int_integer", 1, 65, 131, "integer", "int", ALL),
    C("m65x131_n2_dy_half_lrelu01", 2, 65, 131, "half", "dyadic", ALL, round16=False, **L01),
    C("m65x131_n2_f64_subpixel", 2, 65, 131, "subpixel", "f64", ("lds",), act=ACT_RELU),
    C("m64x128_f64_subpixel_lrelu01_r16", 1, 64, 128, "subpixel", "f64", ALL, **L01),
    C("m64x128_dy_half_relu_r16", 1, 64, 128, "half", "dyadic", ALL, act=ACT_RELU),
    C("m9x911_dy_edges_clamp", 1, 9, 911, "edges", "dyadic", ALL, act=ACT_CLAMP01, round16=False),
    C("m9x911_int_coherent", 1, 9, 911, "coherent_int", "int", ALL, shift=(2, -9)),
    C("m600x14_dy_half_none_r16", 1, 600, 14, "half", "dyadic", ALL),
    C("m600x14_f64_border", 1, 600, 14, "border", "f64", ALL, round16=False, **L25),
    # ---- the regimes at 65x131 on the LDS path
    C("m65x131_dy_edges_lrelu25", 1, 65, 131, "edges", "dyadic", ALL, round16=False, **L25),
    C("m65x131_int_edges", 1, 65, 131, "edges", "int", ("gather", "lds"), act=ACT_RELU),
    C("m65x131_int_coherent", 1, 65, 131, "coherent_int", "int", ("gather", "lds"), shift=(11, -8)),      # the window leaves the map on one side
    C("m65x131_dy_coherent_half", 1, 65, 131, "half", "dyadic", ("lds",), shift=(11, -8), act=ACT_CLAMP01),
    C("m65x131_f64_wild", 1, 65, 131, "wild", "f64", ("gather", "lds")),                                    # a third of the samples take the fallback gather
    C("m65x131_int_huge", 1, 65, 131, "huge", "int", ALL, **L25),
    C("m65x131_f64_border", 1, 65, 131, "border", "f64", ("planar", "lds"), round16=False),
    C("m65x131_f64_coherent", 1, 65, 131, "coherent", "f64", ("lds",), act=ACT_CLAMP01),
    # ---- views: production's layout (MCNet.run: x = feats.ch(64, 64), y = feats.ch(128, 64) of one allocation)
    C("m65x131_n2_int_views_strided", 2, 65, 131, "integer", "int", ALL, views=2),
    C("m65x131_dy_views", 1, 65, 131, "half", "dyadic", ("gather", "lds"), views=1, **L01),
]
del C

RUNS = [(c, p) for c in CASES for p in c.paths]


# ------------------------------------------------------------------------------------------------- launcher arithmetic, restated
def tile_shape(path):
    return (8, 16) if path == "lds" else (8, 8)                         # DL_TY x DL_TX | DCN_TPY x DCN_TPX


def tile_count(case, path):
    th, tw = tile_shape(path)
    return -(-case.W // tw) * -(-case.H // th)


def xcd_regime(gx, N):
    """which branch of tdvc_xcd_tile (csrc/common.h) a grid of gx tiles x N images takes"""
    if gx % 8 == 0:
        return "divisible"
    return "remainder" if N == 1 else "identity"


def xcd_tile(b, gx, N):
    if gx % 8 != 0 and N != 1:
        return b
    q, r, c = gx >> 3, gx & 7, b & 7
    return c * q + min(c, r) + (b >> 3)


# ------------------------------------------------------------------------------------------------- data
def h16(t):
    return t.half().float()


def _ints(gen, shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=gen).float()


def base_positions(H, W):
    """un-displaced sample rows / columns of the 3x3, stride 1, pad 1 taps: (H, 1, 1, 9) and (1, W, 1, 9)"""
    t = torch.arange(9)
    yy = torch.arange(H).view(H, 1, 1, 1).float() - 1 + t.div(3, rounding_mode="floor").view(1, 1, 1, 9)
    xx = torch.arange(W).view(1, W, 1, 1).float() - 1 + (t % 3).view(1, 1, 1, 9)
    return yy, xx


def edge_targets(base, L, half, k):
    """sample positions along one axis of length L, chosen per sample by the index tensor k: the points where the open-interval
    test, the corner flags and the clamps decide the answer, and two interior points next to the tap's own position"""
    if half:
        fixed, rel = [-1.5, -1.0, -0.5, 0.0, L - 1.0, L - 0.5, float(L), L + 0.5], (0.5, -1.5)
    else:
        fixed, rel = [-2.0, -1.0, 0.0, L - 1.0, float(L), L + 1.0], (1.0, -2.0)
    cands = [torch.full_like(base, v) for v in fixed] + [(base + d).clamp(0, L - 1) for d in rel]
    return torch.gather(torch.stack(cands, -1), -1, (k % len(cands)).unsqueeze(-1)).squeeze(-1), len(cands)


def edge_offsets(base_h, base_w, H, W, half):
    """offsets that send every sample (any leading shape) to an edge position; all (row class, column class) pairs are reached"""
    shape = torch.broadcast_shapes(base_h.shape, base_w.shape)
    bh, bw = base_h.expand(shape).contiguous(), base_w.expand(shape).contiguous()
    k = torch.arange(bh.numel()).view(shape)
    th, nh = edge_targets(bh, H, half, k)
    tw, _ = edge_targets(bw, W, half, k // nh)
    return th - bh, tw - bw


def new_offsets(case, gen):
    """(N, H, W, 144) offsets of the regimes this file adds"""
    N, H, W = case.N, case.H, case.W
    shape = (N, H, W, G, 9, 2)
    half = case.grade == "dyadic"
    if case.regime == "edges":
        yy, xx = base_positions(H, W)
        oh, ow = edge_offsets(yy.view(1, H, 1, 1, 9).expand(N, H, W, G, 9), xx.view(1, 1, W, 1, 9).expand(N, H, W, G, 9), H, W, half)
        o = torch.stack([oh, ow], -1)
    elif case.regime in ("coherent_int", "half"):
        # -5..5 around the shift (integers, or multiples of 0.5): the LDS window moves as a whole and the samples straddle its margin
        o = torch.randint(-10, 11, shape, generator=gen).float() / 2 if case.regime == "half" else torch.randint(-5, 6, shape, generator=gen).float()
        o[..., 0] += case.shift[0]
        o[..., 1] += case.shift[1]
    elif case.regime == "huge":
        # integer offsets, a few hundred of them +-inf or +-60000: the kernel's rule is that such a sample lies outside and contributes zero
        o = torch.randint(-12, 13, shape, generator=gen).float()
        flat = o.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)[:400]
        for i, v in enumerate((float("inf"), -float("inf"), BIG, -BIG)):
            flat[idx[100 * i:100 * (i + 1)]] = v
    else:
        raise ValueError(case.regime)
    return o.reshape(N, H, W, 18 * G)


@dataclass
class Data:
    x: torch.Tensor                      # (N, 64, H, W) fp32 holding fp16 values
    w: torch.Tensor                      # (64, 64, 3, 3)
    b: torch.Tensor                      # (64,)
    om: torch.Tensor                     # (N, H, W, 216) NHWC [offsets 144 | mask logits 72], fp16 values (inf included)
    off_ref: torch.Tensor = None         # (N, 144, H, W) float64: the offsets the reference receives (inf -> a finite far-outside value)
    mask_ref: torch.Tensor = None        # (N, 72, H, W) float64: sigmoid of the logits
    pre: torch.Tensor = None             # (N, 64, H, W) float64: contraction + bias
    abs_sum: torch.Tensor = None         # sum |W| |col| (+ |bias|)
    ref: torch.Tensor = None             # expected output: exact grades fp32 holding the fp16 bits, f64 grade float64
    tol: torch.Tensor = None             # f64 grade: elementwise bound


def make_data(case):
    assert case.grade in ("int", "dyadic", "f64") and case.regime in OLD_REGIMES + NEW_REGIMES, case.id
    gen = torch.Generator().manual_seed(3000 + case.seed + sum(map(ord, case.id)))
    N, H, W = case.N, case.H, case.W
    if case.grade == "f64":              # the inputs of test_backward_ops_gpu._dcn_inputs, with a weight and a bias
        assert case.regime in OLD_REGIMES, case.id
        x = h16(torch.randn(N, CH, H, W, generator=gen))
        w = h16(torch.randn(CH, CH, 3, 3, generator=gen) / 24)
        b = torch.randn(CH, generator=gen) * 0.1
        off = HDCN.offsets(case.regime, N, H, W, int(torch.randint(0, 1 << 30, (1,), generator=gen)))
        logit = h16(torch.randn(N, H, W, 9 * G, generator=gen) * 1.5)
        return Data(x, w, b, torch.cat([off, logit], -1))
    x = _ints(gen, (N, CH, H, W), 2)
    keep = (torch.rand(CH, CH, 3, 3, generator=gen) < case.density).float()
    if case.grade == "int":
        assert case.regime in ("edges", "coherent_int", "huge", "integer"), case.id
        w = _ints(gen, (CH, CH, 3, 3), 2) * keep
        b = _ints(gen, (CH,), 8)
        levels = torch.tensor([-BIG, BIG])
    else:
        assert case.regime in ("edges", "half"), case.id
        w = _ints(gen, (CH, CH, 3, 3), 64) * keep / 512
        b = _ints(gen, (CH,), 16) / 8
        levels = torch.tensor(DYADIC_LOGITS)
    off = HDCN.offsets("integer", N, H, W, 7 + case.seed) if case.regime == "integer" else new_offsets(case, gen)
    logit = levels[torch.randint(0, len(levels), (N, H, W, 9 * G), generator=gen)]
    om = torch.cat([off, logit], -1)
    fin = torch.isfinite(om)
    assert bool((h16(om)[fin] == om[fin]).all()) and float(om[fin].abs().max()) <= BIG, (case.id, "the offsets must be fp16 values")
    step = 1.0 if case.grade == "int" else 2.0
    assert bool(((off[torch.isfinite(off)] * step) % 1 == 0).all()), case.id
    return Data(x, w, b, om)


# ------------------------------------------------------------------------------------------------- references
def _act(v, act, slope):
    """csrc/common.h act_apply in the dtype of v (fp32: the kernel's arithmetic, v * float32(slope))"""
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32).to(v.dtype))
    if act == ACT_CLAMP01:
        return v.clamp(0.0, 1.0)
    assert act == ACT_NONE
    return v


def epilogue(v, act, slope, round16):
    """the rounding sequence of both kernels' epilogues on the exact fp32 value v = acc + bias: one round-to-nearest-even to fp16
    if round_before_act, act_apply in fp32, round-to-nearest-even to fp16"""
    assert v.dtype == torch.float32
    if round16:
        v = h16(v)
    return h16(_act(v, act, slope))


def dcn_ref(x, w, b, off, mask):
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    return dcn_v2_forward_ref(x, w, b, off, mask, 3, 3, 1, 1, 1, 1, 1, 1, G)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def check_exact(case, d):
    """the preconditions of the exact grades, on the reference: every partial sum an exact fp32 value in any order (the sum of
    the magnitudes stays below 2^24 units of the products), the value that enters the epilogue an exact fp32 value, and for the
    integer grade every output below 2048 and an integer times the slope: an fp16 value at every stage"""
    unit = 1.0 if case.grade == "int" else 2.0 ** 12                    # samples in 2^-3, w in 2^-9
    assert float(d.abs_sum.max()) * unit < 2 ** 24, (case.id, float(d.abs_sum.max()))
    assert bool(((d.pre * unit) % 1 == 0).all()), case.id
    if case.grade == "int":
        assert float(d.pre.abs().max()) < 2048, (case.id, float(d.pre.abs().max()))
        assert case.act in (ACT_NONE, ACT_RELU) or (case.act == ACT_LRELU and np.log2(case.slope) % 1 == 0), case.id
        want = _act(d.pre, case.act, case.slope)
        assert bool((want.half().double() == want).all()) and bool((d.ref.double() == want).all()), case.id


def f64_bound(case, d, absx_ref):
    """per output, assembled from terms the project already uses (tests/test_backward_ops_gpu.py):
         sum_k |W_k| (EPS16 |col_k| + 1e-5 max|x| + TINY16)   each of the 576 modulated samples as the kernel holds it: fp32 bilinear
                                                               weights on fp16 values, the __expf sigmoid (~1e-6 relative), one fp16
                                                               store of a value <= max|x| (test_dcn_columns' bound per column)
       + 600 EPS32 (sum_k |W_k| |col_k| + |bias|)              the fp32 accumulation over 576 products plus the bias, any order
       + n_round R16 |ref| max(1, slope) + TINY16              the fp16 store, and the fp16 rounding before the activation if asked for
    sum_k |W_k| |col_k| is a second reference call on |W| and |x|: the mask and the bilinear weights are non-negative"""
    sum_w = d.w.double().abs().sum((1, 2, 3)).view(1, CH, 1, 1)
    xmax = float(d.x.abs().max())
    n_round = 2 if case.round16 else 1
    scale = max(1.0, case.slope) if case.act == ACT_LRELU else 1.0
    return (EPS16 * absx_ref + sum_w * (1e-5 * xmax + TINY16) + 600 * EPS32 * (absx_ref + d.b.double().abs().view(1, CH, 1, 1))
            + n_round * R16 * scale * d.ref.abs() + TINY16)


@functools.lru_cache(maxsize=None)
def reference(case):
    """the data of a case with its expected output; computed once and shared by the paths (callers must not modify it)"""
    d = make_data(case)
    off = _nchw(d.om[..., :18 * G]).double()
    # the oracle turns an infinite offset into NaN (inf - inf in its fractions); the kernels' rule is that such a sample lies
    # outside the map and contributes zero, which is what the oracle computes for a finite position far outside
    d.off_ref = torch.where(torch.isinf(off), torch.sign(off) * BIG, off)
    logit = _nchw(d.om[..., 18 * G:]).double()
    d.mask_ref = torch.sigmoid(logit)
    if case.grade != "f64":              # the sigmoid of the saturating logits, by IEEE arithmetic alone
        assert bool((d.mask_ref == torch.where(logit > 0, 1.0, torch.where(logit < 0, 0.0, 0.5))).all()), case.id
    x, w, b = d.x.double(), d.w.double(), d.b.double()
    d.pre = dcn_ref(x, w, b, d.off_ref, d.mask_ref)
    d.abs_sum = dcn_ref(x.abs(), w.abs(), b.abs(), d.off_ref, d.mask_ref)
    assert bool(torch.isfinite(d.pre).all()), case.id
    if case.grade == "f64":
        d.ref = _act(d.pre, case.act, case.slope)
        d.tol = f64_bound(case, d, d.abs_sum - b.abs().view(1, CH, 1, 1))
    else:
        d.ref = epilogue(d.pre.float(), case.act, case.slope, case.round16)
        check_exact(case, d)
    return d


# ------------------------------------------------------------------------------------------------- sample geometry (CPU guard, diagnostics)
def sample_positions(case, d):
    """h, w of every sample: float64 (N, H, W, G, 9), from the offsets the reference receives"""
    yy, xx = base_positions(case.H, case.W)
    o = d.off_ref.permute(0, 2, 3, 1).reshape(case.N, case.H, case.W, G, 9, 2)
    return yy.double().unsqueeze(0) + o[..., 0], xx.double().unsqueeze(0) + o[..., 1]


AXIS_CLASSES = ("== -1", "in (-1, 0)", "== L-1", "in (L-1, L)", "== L", "beyond")


def axis_class(p, L):
    """index into AXIS_CLASSES per sample, -1 for the plain interior [0, L-1)"""
    c = torch.full(p.shape, -1, dtype=torch.long)
    c[(p > L - 1) & (p < L)] = 3
    c[(p > -1) & (p < 0)] = 1
    c[p == -1] = 0
    c[p == L - 1] = 2
    c[p == L] = 4
    c[(p < -1) | (p > L)] = 5
    return c


def lds_window_stats(case, d):
    """dcn_lds_kernel's window rule, restated: the window of a tile is 20 x 28 pixels, 6 around the 8 x 16 tile, moved by the rintf of
    the tile's mean offset (each offset clamped to +-64; lanes of overhanging pixels read the clamped pixel's record).  A tile whose
    window lies inside the map takes the interior fast path; a sample whose (clamped) corners leave the window takes the per-lane
    fallback gather; only a fallback sample inside the map carries a weight, and so a value the gather could get wrong.
    -> (tiles, interior tiles, samples of valid pixels, fallback samples inside the map, those of them in interior tiles, all fallback samples)"""
    N, H, W = case.N, case.H, case.W
    th, tw = tile_shape("lds")
    ty, tx = -(-H // th), -(-W // tw)
    rows = torch.arange(ty * th).clamp(max=H - 1)
    cols = torch.arange(tx * tw).clamp(max=W - 1)
    o = d.om[..., :18 * G].double().reshape(N, H, W, G * 9, 2)[:, rows][:, :, cols]          # (N, ty*8, tx*16, 72, 2), inf kept
    o = o.clamp(-64, 64).reshape(N, ty, th, tx, tw, G * 9, 2)
    centre = torch.round(o.mean((2, 4, 5)))                                                  # (N, ty, tx, 2): rintf = ties to even
    wy0 = torch.arange(ty).view(1, ty, 1) * th - 6 + centre[..., 0]
    wx0 = torch.arange(tx).view(1, 1, tx) * tw - 6 + centre[..., 1]
    interior = (wy0 >= 0) & (wx0 >= 0) & (wy0 + 20 <= H) & (wx0 + 28 <= W)
    h, w = sample_positions(case, d)
    pix_y, pix_x = torch.arange(H) // th, torch.arange(W) // tw
    wy0p = wy0[:, pix_y][:, :, pix_x].view(N, H, W, 1, 1)
    wx0p = wx0[:, pix_y][:, :, pix_x].view(N, H, W, 1, 1)
    intp = interior[:, pix_y][:, :, pix_x].view(N, H, W, 1, 1)
    hl, wl = torch.floor(h.clamp(-2, H + 1)), torch.floor(w.clamp(-2, W + 1))
    y0, y1 = hl.clamp(0, H - 1), (hl + 1).clamp(0, H - 1)
    x0, x1 = wl.clamp(0, W - 1), (wl + 1).clamp(0, W - 1)
    inwin = (y0 - wy0p >= 0) & (y1 - wy0p < 20) & (x0 - wx0p >= 0) & (x1 - wx0p < 28)
    fall = ~inwin
    live = fall & (h > -1) & (w > -1) & (h < H) & (w < W)
    return int(interior.numel()), int(interior.sum()), int(fall.numel()), int(live.sum()), int((live & intp).sum()), int(fall.sum())


# ------------------------------------------------------------------------------------------------- _ext.dcn_v2_forward (fp32, NCHW)
@dataclass(frozen=True)
class ExtCase:
    id: str
    B: int
    C: int
    Cout: int
    H: int
    W: int
    G: int
    kernel: tuple
    stride: tuple
    pad: tuple
    dil: tuple
    grade: str                # "int" | "dyadic": there is no fp16 here, every value is exact in fp32


EXT_CASES = [
    ExtCase("ext_cout72_two_passes", 1, 16, 72, 7, 11, 4, (3, 3), (1, 1), (1, 1), (1, 1), "dyadic"),     # 77 pixels: two blocks, the second partial; cob = 0, 64 (8 channels)
    ExtCase("ext_7x7_49_taps", 2, 4, 8, 9, 10, 2, (7, 7), (1, 1), (3, 3), (1, 1), "int"),                # all 49 rows of the LDS array; 90 pixels
    ExtCase("ext_7x7_49_taps_dy", 1, 4, 8, 6, 7, 2, (7, 7), (1, 1), (3, 3), (1, 1), "dyadic"),           # 42 pixels: below one block
    ExtCase("ext_1x3_strides_2_1", 2, 8, 12, 9, 8, 2, (1, 3), (2, 1), (0, 2), (1, 2), "dyadic"),         # 5 x 8 = 40 output pixels
    ExtCase("ext_1x3_strides_2_1_int", 1, 8, 12, 19, 13, 4, (1, 3), (2, 1), (0, 2), (1, 2), "int"),      # 10 x 13 = 130 pixels: three blocks
]


def ext_out_map(c):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c.kernel, c.stride, c.pad, c.dil
    return (c.H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (c.W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def ext_args(c):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c.kernel, c.stride, c.pad, c.dil
    return (kh, kw, sh, sw, ph, pw, dh, dw, c.G)


@functools.lru_cache(maxsize=None)
def ext_reference(c):
    """-> (x, w, b, offset, mask, expected fp32 output): the `edges` regime at the case's geometry, integer or dyadic data"""
    from oracle.tdvc_ref.blocks import dcn_v2_forward_ref
    gen = torch.Generator().manual_seed(4000 + sum(map(ord, c.id)))
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c.kernel, c.stride, c.pad, c.dil
    K = kh * kw
    Ho, Wo = ext_out_map(c)
    half = c.grade == "dyadic"
    x = _ints(gen, (c.B, c.C, c.H, c.W), 2)
    w = _ints(gen, (c.Cout, c.C, kh, kw), 2) if not half else _ints(gen, (c.Cout, c.C, kh, kw), 8) / 64
    b = _ints(gen, (c.Cout,), 8) if not half else _ints(gen, (c.Cout,), 16) / 8
    t = torch.arange(K)
    bh = (torch.arange(Ho).view(Ho, 1, 1) * sh - ph + (t.div(kw, rounding_mode="floor") * dh).view(1, 1, K)).float()
    bw = (torch.arange(Wo).view(1, Wo, 1) * sw - pw + ((t % kw) * dw).view(1, 1, K)).float()
    oh, ow = edge_offsets(bh.view(1, 1, Ho, 1, K).expand(c.B, c.G, Ho, Wo, K), bw.view(1, 1, 1, Wo, K).expand(c.B, c.G, Ho, Wo, K), c.H, c.W, half)
    off = torch.stack([oh, ow], -1).permute(0, 1, 4, 5, 2, 3).reshape(c.B, c.G * 2 * K, Ho, Wo).contiguous()       # channel g*2K + 2t (+1)
    levels = torch.tensor([0.0, 0.5, 1.0] if half else [0.0, 1.0])
    mask = levels[torch.randint(0, len(levels), (c.B, c.G * K, Ho, Wo), generator=gen)]
    args = ext_args(c)
    ref = dcn_v2_forward_ref(x.double(), w.double(), b.double(), off.double(), mask.double(), *args)
    mag = dcn_v2_forward_ref(x.double().abs(), w.double().abs(), b.double().abs(), off.double(), mask.double(), *args)
    unit = 2.0 ** 9 if half else 1.0                                     # samples in 2^-3 (weights 2^-2, mask 2^-1), w in 2^-6
    assert float(mag.max()) * unit < 2 ** 24 and bool(((ref * unit) % 1 == 0).all()) and bool((ref.float().double() == ref).all()), c.id
    return x, w, b, off, mask, ref.float()
