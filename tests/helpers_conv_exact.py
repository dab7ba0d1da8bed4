"""The case table and the data of the exact forward-conv tests (tests/test_conv_exact_gpu.py launches the cases on the GPU,
tests/test_conv_exact_cases_cpu.py holds, without a GPU, every case to the kernel it is there for).

Three grades of data, all made here:

  int     x, w in {-2..2} (w thinned to `density`), integer bias and residuals, slopes 2^-k.  Every product and every partial
          sum is an exact fp32 integer in any order and any split, every stage is an exact fp16 value: the kernel's answer is
          the integer convolution bit for bit whatever its summation order, tile walk or epilogue form.
  dyadic  x in multiples of 2^-3, w of 2^-6, bias of 2^-9: the accumulation is still exact, the outputs are not fp16 values,
          so the stored bits are decided by the epilogue's rounding sequence, which `epilogue()` restates per form
          (csrc/conv_common.h: "e4" = epilogue4, "generic" = epilogue_pack + epilogue_store_row, "lean" =
          epilogue_lean_seq and the epilogues of their own in conv_mfma_v10, conv_mfma_v11, conv_row and conv_c8).
  f64     operations that are inexact by nature (GDN's root, the sigmoid) on dyadic data, against float64 with a bound
          derived in `f64_reference()`.

The preconditions of the exact grades are asserted on the REFERENCE (`check_exact`), never on the kernel's output."""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from tests import helpers_conv_dispatch as HD

W1, W3, W5, W7, WM, S1, S3 = range(7)            # indices into helpers_conv_dispatch.WINDOWS
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_CLAMP01, ACT_SIGMOID = 0, 1, 2, 3, 4
GDN_FWD, GDN_INV = 1, 2

EPS16 = 2.0 ** -11            # the constants of tests/test_backward_ops_gpu.py
EPS32 = 2.0 ** -24
TINY16 = 2.0 ** -24
R16 = EPS16 + 8 * EPS32

ROW_ALL, ROW_NO_C64 = 15, 15 & ~2       # tdvc_debug_enable_conv_row: one bit per geometry
REVERSE_WALKERS = ["direct", "conv_mfma_v2", "conv_mfma_v3", "conv_mfma_v5", "conv_mfma_v7", "conv_mfma_v10", "conv_mfma_v11", "conv_row"]


@dataclass(frozen=True)
class Case:
    id: str
    kernel: str               # what tdvc_conv_select / tdvc_last_conv_kernel must name ("direct": any conv_mfma<..>)
    form: str                 # "e4" | "generic" | "lean" | "gdn" (pool rounded to fp16 before the root) | "gdn32" (conv_f32: fp32 pool and multiplicand) | "pair"
    cin: int
    cout: int
    win: int
    N: int
    H: int                    # the INPUT map
    W: int
    act: int = ACT_NONE
    slope: float = 0.0
    res: str = None           # None | "f16" | "f32"
    res2: str = None
    out: str = "f16"          # "f16" | "f32" | "nchw" | "shuffle"
    narrow: int = 0
    round16: bool = False
    bias: bool = True
    s2d: bool = False
    gdn: int = 0
    bcast: str = None         # None | "inplace" | "outofplace"
    x_f32: bool = False
    chan_sum: bool = False
    views: bool = False       # x, y, res, res2 are channel windows of wider, sentinel-filled buffers
    res_c: int = 0            # res is a dense map of its own with only this many channels (fewer than y's): SPyNet's 2-channel flow
    slices: str = None        # None | "all" | "last1": x, y, res are FM.as_slices(1, 4, 64) of 2 x H x W x 256 buffers (image stride 64 <
                              # pixel stride 256, the LoopFilter's frame slices), N = 4; "last1": .batch(3, 1) of them, N = 1
    switches: tuple = ()      # ((setter, value while the case runs, value restored), ...)
    multi: bool = False       # more tiles (rows) than workgroups, with a remainder -- or, for the one-tile-per-workgroup kernels, many tiles
    ragged: bool = False      # the map is no multiple of the kernel's tile in either direction
    grade: str = "int"
    density: float = 1.0
    seed: int = 0
    # conv_pair only
    act2: int = ACT_NONE
    slope2: float = 0.0
    add_input: bool = False


def sw(name, off, on):
    return ("tdvc_debug_enable_" + name, off, on)


NO_V9, NO_GDN128, NO_ROW = sw("conv_v9", 0, 1), sw("gdn128", 0, 1), sw("conv_row", 0, ROW_ALL)

C = Case
CASES = [
    # ---- conv_mfma_v10: 16x32 tiles, 3x3 64 -> 64k, lean.  conv_row's 64-channel geometry takes the <= 1 residual forms first
    C("v10_ragged_2res", "conv_mfma_v10", "lean", 64, 64, W3, 1, 65, 131, act=ACT_RELU, res="f16", res2="f16", ragged=True),      # 8515 px: H % 16 = 1, W % 32 = 3
    C("v10_ragged_norow", "conv_mfma_v10", "lean", 64, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, switches=(sw("conv_row", ROW_NO_C64, ROW_ALL),), ragged=True),
    C("v10_multi", "conv_mfma_v10", "lean", 64, 128, W3, 4, 113, 161, act=ACT_LRELU, slope=0.125, res="f16", res2="f16", multi=True, ragged=True),   # 48 tiles on 32 workgroups
    C("v10_views_narrow", "conv_mfma_v10", "lean", 64, 128, W3, 2, 65, 131, res="f16", res2="f16", narrow=32, views=True, ragged=True),
    C("v10_dy_lrelu01", "conv_mfma_v10", "lean", 64, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    C("v10_dy_relu", "conv_mfma_v10", "lean", 64, 64, W3, 1, 65, 131, act=ACT_RELU, switches=(sw("conv_row", ROW_NO_C64, ROW_ALL),), grade="dyadic", ragged=True),
    C("v10_dy_none_1res", "conv_mfma_v10", "lean", 64, 64, W3, 1, 65, 131, res="f16", switches=(sw("conv_row", ROW_NO_C64, ROW_ALL),), grade="dyadic", ragged=True),
    # ---- conv_mfma_v7: 16x32 tiles, 3x3 32 / 64 -> 64k, always the generic transposed form (counted waits: one epilogue)
    C("v7_ragged_c32", "conv_mfma_v7", "generic", 32, 64, W3, 1, 65, 131, act=ACT_RELU, res="f16", ragged=True),
    C("v7_multi_c32", "conv_mfma_v7", "generic", 32, 128, W3, 4, 113, 161, act=ACT_LRELU, slope=0.5, res="f16", res2="f16", multi=True, ragged=True),
    C("v7_shuffle_c64", "conv_mfma_v7", "generic", 64, 256, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, out="shuffle", res="f16", ragged=True),     # sub-pixel store: not lean, so neither conv_row nor v10
    C("v7_views", "conv_mfma_v7", "generic", 32, 64, W3, 2, 65, 131, res="f16", views=True, ragged=True),
    C("v7_dy_lrelu01", "conv_mfma_v7", "generic", 32, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    C("v7_dy_none", "conv_mfma_v7", "generic", 32, 64, W3, 1, 65, 131, grade="dyadic", ragged=True),
    C("v7_dy_relu_1res", "conv_mfma_v7", "generic", 32, 64, W3, 1, 65, 131, act=ACT_RELU, res="f16", grade="dyadic", ragged=True),
    C("v7_dy_lrelu_dyadic", "conv_mfma_v7", "generic", 32, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, grade="dyadic", ragged=True),
    # ---- conv_mfma_v11: 16x32 tiles, 3x3 Cin >= 128, lean arithmetic also on the sub-pixel store
    C("v11_ragged_2res", "conv_mfma_v11", "lean", 128, 128, W3, 1, 65, 131, act=ACT_RELU, res="f16", res2="f16", ragged=True),    # two residuals: conv_row has no such form
    C("v11_multi", "conv_mfma_v11", "lean", 128, 128, W3, 4, 113, 161, act=ACT_LRELU, slope=0.25, res="f16", switches=(NO_ROW,), multi=True, ragged=True),
    C("v11_c192", "conv_mfma_v11", "lean", 192, 64, W3, 1, 65, 131, act=ACT_RELU, density=0.5, ragged=True),                      # Cin that conv_row does not take
    C("v11_shuffle", "conv_mfma_v11", "lean", 128, 256, W3, 1, 65, 131, act=ACT_LRELU, slope=0.5, out="shuffle", res="f16", switches=(NO_ROW,), ragged=True),
    C("v11_views", "conv_mfma_v11", "lean", 128, 64, W3, 2, 65, 131, res="f16", res2="f16", views=True, ragged=True),
    C("v11_dy_lrelu01", "conv_mfma_v11", "lean", 128, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    # ---- conv_row: runs of rows over 256 / ncb slots; strips of 32 (C128, s2d) or 64 (C64, C128W) columns; Ho >= 16
    C("row_c64_ragged", "conv_row", "lean", 64, 64, W3, 1, 65, 131, act=ACT_RELU, res="f16", ragged=True),                        # 3 strips (last 3 px) x 65 rows = 195 one-row runs on 256 slots
    C("row_c64_ho16", "conv_row", "lean", 64, 128, W3, 1, 16, 513, act=ACT_LRELU, slope=0.25, multi=True, ragged=True),           # the row floor Ho = 16; 9 strips, last 1 px
    C("row_c64_ho17_n3", "conv_row", "lean", 64, 64, W3, 3, 17, 483, res2="f16", multi=True, ragged=True),                        # 16 k + 1 rows; the lone residual arrives as res2
    C("row_c128_ragged", "conv_row", "lean", 128, 128, W3, 1, 65, 131, act=ACT_LRELU, slope=0.5, res="f16", multi=True, ragged=True),
    C("row_c128_shuffle", "conv_row", "lean", 128, 256, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, out="shuffle", res="f16", multi=True, ragged=True),
    C("row_c128w", "conv_row", "lean", 128, 64, W3, 2, 33, 257, act=ACT_RELU, res="f16", multi=True, ragged=True),                # 128 -> 64: the wide-strip geometry
    C("row_views", "conv_row", "lean", 64, 64, W3, 2, 65, 131, act=ACT_RELU, res="f16", views=True, multi=True, ragged=True),
    C("row_c64_long_runs", "conv_row", "lean", 64, 256, W3, 4, 65, 131, act=ACT_RELU, res="f16", multi=True, ragged=True),        # 780 rows on 256 / 4 = 64 slots: runs of 12 or 13 rows that cross strip and image ends
    C("row_dy_lrelu01", "conv_row", "lean", 64, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", grade="dyadic", ragged=True),
    C("row_dy_shuffle", "conv_row", "lean", 128, 256, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, out="shuffle", res="f16", grade="dyadic", multi=True, ragged=True),
    C("row_s2d", "conv_row(s2d)", "lean", 64, 128, S3, 1, 130, 262, act=ACT_RELU, s2d=True, res="f16", multi=True, ragged=True),  # 65 x 131 output
    C("row_s2d_dy", "conv_row(s2d)", "lean", 64, 128, S3, 1, 130, 262, act=ACT_LRELU, slope=0.1, s2d=True, grade="dyadic", multi=True, ragged=True),
    # the instantiations <geometry, activation, residual, shuffle> that a 1080p P-frame launches and no case above reaches: no activation
    # without a residual, the sub-pixel store without a residual (the 128 -> 512 layers), the 128 -> 64 geometry without a residual
    C("row_c128_plain", "conv_row", "lean", 128, 128, W3, 1, 65, 131, multi=True, ragged=True),
    C("row_c128_plain_shuffle", "conv_row", "lean", 128, 256, W3, 1, 65, 131, out="shuffle", multi=True, ragged=True),
    C("row_c128_none_res", "conv_row", "lean", 128, 128, W3, 1, 65, 131, res="f16", multi=True, ragged=True),
    C("row_c128_none_res_shuffle", "conv_row", "lean", 128, 256, W3, 1, 65, 131, out="shuffle", res="f16", multi=True, ragged=True),
    C("row_c128_relu", "conv_row", "lean", 128, 128, W3, 1, 65, 131, act=ACT_RELU, multi=True, ragged=True),
    C("row_c128_lrelu", "conv_row", "lean", 128, 128, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, multi=True, ragged=True),
    C("row_c128_lrelu_shuffle512", "conv_row", "lean", 128, 512, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, out="shuffle", multi=True, ragged=True),
    C("row_c64_plain", "conv_row", "lean", 64, 64, W3, 1, 65, 131, ragged=True),
    C("row_c64_relu", "conv_row", "lean", 64, 64, W3, 1, 65, 131, act=ACT_RELU, ragged=True),
    C("row_c128w_plain", "conv_row", "lean", 128, 64, W3, 1, 65, 131, ragged=True),
    C("row_c128w_relu", "conv_row", "lean", 128, 64, W3, 1, 65, 131, act=ACT_RELU, ragged=True),
    C("row_c128w_lrelu", "conv_row", "lean", 128, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.25, ragged=True),
    # ---- conv_mfma_v3: 8x32 tiles on 512 slots; every epilogue form
    C("v3_multi", "conv_mfma_v3", "lean", 128, 256, W3, 4, 75, 100, act=ACT_RELU, res="f16", multi=True, ragged=True),            # 40 tiles on 32 workgroups, H % 8 = 3, W % 32 = 4, below the streaming floor, above v9's
    C("v3_ragged", "conv_mfma_v3", "lean", 64, 64, W3, 2, 67, 69, act=ACT_LRELU, slope=0.25, res="f16", res2="f16", ragged=True), # 9246 px over the batch: H % 8 = 3, W % 32 = 5
    C("v3_e4_f32out", "conv_mfma_v3", "e4", 64, 64, W3, 2, 67, 69, act=ACT_LRELU, slope=0.25, out="f32", res="f32", ragged=True),
    C("v3_e4_round16_nobias", "conv_mfma_v3", "e4", 64, 64, W3, 2, 67, 69, act=ACT_RELU, round16=True, bias=False, ragged=True),
    C("v3_shuffle", "conv_mfma_v3", "generic", 64, 256, W3, 2, 67, 69, act=ACT_RELU, out="shuffle", res="f16", ragged=True),
    C("v3_s2d", "conv_mfma_v3(s2d)", "lean", 128, 128, S3, 2, 134, 138, act=ACT_RELU, s2d=True, res="f16", ragged=True),          # 2 x 67 x 69 output (ops.conv keeps the plain stride-2 form up to 8192 pixels); Cin 128: not conv_row's s2d geometry
    C("v3_s2d_multi", "conv_mfma_v3(s2d)", "e4", 64, 256, S3, 4, 150, 200, out="f32", s2d=True, multi=True, ragged=True),          # 75 x 100 output, 40 tiles on 32 workgroups
    C("v3_views_narrow", "conv_mfma_v3", "lean", 64, 128, W3, 2, 67, 69, res="f16", narrow=64, views=True, ragged=True),
    C("v3_dy_lean", "conv_mfma_v3", "lean", 64, 64, W3, 2, 67, 69, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    C("v3_dy_e4_round16", "conv_mfma_v3", "e4", 64, 64, W3, 2, 67, 69, act=ACT_LRELU, slope=0.1, round16=True, res="f16", grade="dyadic", ragged=True),
    C("v3_dy_generic", "conv_mfma_v3", "generic", 64, 256, W3, 2, 67, 69, act=ACT_LRELU, slope=0.1, out="shuffle", res="f16", grade="dyadic", ragged=True),
    C("v3_sigmoid", "conv_mfma_v3", "e4", 64, 64, W3, 2, 67, 69, act=ACT_SIGMOID, grade="f64", ragged=True),
    C("v3_dy_clamp01", "conv_mfma_v3", "e4", 64, 64, W3, 2, 67, 69, act=ACT_CLAMP01, grade="dyadic", ragged=True),
    # ---- conv_mfma_v5: the 1x1 kernel, 16x32 tiles on 256 slots
    C("v5_ragged", "conv_mfma_v5", "lean", 128, 64, W1, 1, 65, 131, act=ACT_RELU, res="f16", ragged=True),
    C("v5_multi_c512", "conv_mfma_v5", "lean", 512, 128, W1, 4, 113, 161, act=ACT_LRELU, slope=0.25, res="f16", res2="f16", multi=True, ragged=True),
    C("v5_chan_sum", "conv_mfma_v5", "lean", 64, 64, W1, 3, 65, 131, act=ACT_RELU, chan_sum=True, ragged=True),
    C("v5_stride2", "conv_mfma_v5", "lean", 64, 128, S1, 1, 37, 71, act=ACT_RELU, switches=(NO_V9,), ragged=True),                                    # the skip convs: any map size
    C("v5_e4_nchw", "conv_mfma_v5", "e4", 64, 64, W1, 1, 65, 131, act=ACT_RELU, out="nchw", ragged=True),                         # integer planar store: the indexing
    C("v5_dy_nchw_clamp", "conv_mfma_v5", "e4", 64, 64, W1, 1, 65, 131, act=ACT_CLAMP01, out="nchw", grade="dyadic", ragged=True),     # 40 % of the outputs are fractions in (0, 1), planar fp32
    C("v5_dy_nchw_lrelu", "conv_mfma_v5", "e4", 64, 64, W1, 2, 65, 131, act=ACT_LRELU, slope=0.1, out="nchw", grade="dyadic", ragged=True),   # v * 0.1f: planar fp32 values that are no fp16 values
    C("v5_sigmoid", "conv_mfma_v5", "e4", 64, 64, W1, 1, 65, 131, act=ACT_SIGMOID, grade="f64", ragged=True),
    C("v5_e4_f32res", "conv_mfma_v5", "e4", 64, 64, W1, 1, 65, 131, res="f32", res2="f16", bias=False, ragged=True),
    C("v5_views_narrow", "conv_mfma_v5", "lean", 64, 128, W1, 2, 65, 131, res="f16", narrow=32, views=True, ragged=True),
    C("v5_bcast_inplace", "conv_mfma_v5(bcast)", "lean", 64, 64, W1, 1, 65, 131, bcast="inplace", views=True, ragged=True),
    C("v5_bcast_outofplace", "conv_mfma_v5(bcast)", "lean", 128, 64, W1, 2, 65, 131, bcast="outofplace", views=True, ragged=True),
    C("v5_dy_lean", "conv_mfma_v5", "lean", 128, 64, W1, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    C("v5_dy_lrelu_dyadic", "conv_mfma_v5", "lean", 128, 64, W1, 1, 65, 131, act=ACT_LRELU, slope=0.25, res="f16", grade="dyadic", ragged=True),
    C("v5_dy_none", "conv_mfma_v5", "lean", 128, 64, W1, 1, 65, 131, grade="dyadic", ragged=True),
    C("v5_dy_e4", "conv_mfma_v5", "e4", 128, 64, W1, 1, 65, 131, act=ACT_LRELU, slope=0.1, out="f32", res="f16", grade="dyadic", ragged=True),
    C("v5_dy_bcast", "conv_mfma_v5(bcast)", "lean", 64, 64, W1, 1, 65, 131, bcast="inplace", views=True, grade="dyadic", ragged=True),
    # ---- conv_mfma_v2: 16x32 tiles, one per workgroup; windows v3 does not take (5x5, 7x7, masked)
    C("v2_5x5", "conv_mfma_v2", "lean", 128, 256, W5, 1, 49, 67, act=ACT_RELU, res="f16", density=0.5, switches=(NO_V9,), multi=True, ragged=True),
    C("v2_masked", "conv_mfma_v2", "lean", 128, 64, WM, 2, 49, 67, act=ACT_LRELU, slope=0.25, res="f16", res2="f16", switches=(NO_V9,), multi=True, ragged=True),
    C("v2_5x5_shuffle", "conv_mfma_v2", "generic", 64, 256, W5, 1, 49, 67, act=ACT_RELU, out="shuffle", res="f16", density=0.5, switches=(NO_V9,), multi=True, ragged=True),   # sub-pixel store: the generic transposed form
    C("v2_7x7_e4", "conv_mfma_v2", "e4", 64, 64, W7, 1, 49, 67, act=ACT_LRELU, slope=0.5, out="f32", density=0.5, switches=(NO_V9,), multi=True, ragged=True),
    C("v2_dy_lean", "conv_mfma_v2", "lean", 64, 64, W5, 1, 49, 67, act=ACT_LRELU, slope=0.1, res="f16", grade="dyadic", density=0.5, switches=(NO_V9,), multi=True, ragged=True),
    C("v2_dy_clamp01", "conv_mfma_v2", "e4", 64, 64, W5, 1, 49, 67, act=ACT_CLAMP01, switches=(NO_V9,), grade="dyadic", density=0.5, multi=True, ragged=True),
    C("v2_sigmoid", "conv_mfma_v2", "e4", 64, 64, W5, 1, 49, 67, act=ACT_SIGMOID, switches=(NO_V9,), grade="f64", density=0.5, multi=True, ragged=True),
    C("v2_views", "conv_mfma_v2", "lean", 128, 64, WM, 2, 49, 67, act=ACT_RELU, res="f16", res2="f16", views=True, switches=(NO_V9,), multi=True, ragged=True),
    # ---- the direct kernel conv_mfma<ck/8, cout tiles, stride>: 8x32 tiles, one per workgroup
    C("direct_s2_3x3", "direct", "lean", 64, 64, S3, 2, 37, 71, act=ACT_RELU, res="f16", switches=(NO_V9,), multi=True, ragged=True),          # 19 x 36 output
    C("direct_c16_7x7", "direct", "e4", 16, 32, W7, 1, 19, 37, act=ACT_LRELU, slope=0.25, switches=(NO_V9,), multi=True, ragged=True),
    C("direct_small_cout2_f32", "direct", "e4", 16, 2, W7, 1, 19, 37, out="f32", res="f32", switches=(NO_V9,), multi=True, ragged=True),
    C("direct_cout20", "direct", "e4", 8, 20, W3, 1, 19, 37, act=ACT_RELU, switches=(NO_V9,), multi=True, ragged=True),                        # pad8(20) = 24: four padded channels
    C("direct_c8_large", "direct", "lean", 8, 64, W3, 1, 65, 131, act=ACT_RELU, res="f16", multi=True, ragged=True),                           # a residual: not conv_c8's
    C("direct_shuffle_small", "direct", "generic", 32, 256, W3, 1, 9, 15, act=ACT_RELU, out="shuffle", res="f16", switches=(NO_V9,), multi=True, ragged=True),   # < 256 px: below v3's floor
    C("direct_dy_lean", "direct", "lean", 64, 64, S3, 2, 37, 71, act=ACT_LRELU, slope=0.1, res="f16", switches=(NO_V9,), grade="dyadic", multi=True, ragged=True),
    C("direct_dy_e4", "direct", "e4", 16, 32, W7, 1, 19, 37, act=ACT_LRELU, slope=0.1, res="f16", switches=(NO_V9,), grade="dyadic", multi=True, ragged=True),
    C("direct_sigmoid", "direct", "e4", 16, 32, W7, 1, 19, 37, act=ACT_SIGMOID, switches=(NO_V9,), grade="f64", multi=True, ragged=True),
    C("direct_dy_clamp01", "direct", "e4", 16, 32, W7, 1, 19, 37, act=ACT_CLAMP01, switches=(NO_V9,), grade="dyadic", multi=True, ragged=True),
    C("direct_views", "direct", "lean", 64, 64, S3, 2, 37, 71, act=ACT_RELU, res="f16", views=True, switches=(NO_V9,), multi=True, ragged=True),
    # ---- conv_mfma_v9: split-K for <= 8192 pixels over the batch; epilogue4
    C("v9_3x3", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, act=ACT_RELU, res="f16", ragged=True),
    C("v9_1x1_odd_cout", "conv_mfma_v9", "e4", 512, 426, W1, 1, 9, 13, act=ACT_LRELU, slope=0.5, density=0.5, ragged=True),                     # pad8(426) = 432
    C("v9_s2", "conv_mfma_v9", "e4", 64, 128, S3, 1, 33, 47, res="f16", res2="f16", ragged=True),
    C("v9_masked_f32", "conv_mfma_v9", "e4", 128, 256, WM, 1, 17, 30, out="f32", round16=True, act=ACT_LRELU, slope=0.25, ragged=True),
    C("v9_shuffle", "conv_mfma_v9", "e4", 128, 128, W3, 1, 9, 15, act=ACT_RELU, out="shuffle", res="f16", ragged=True),
    C("v9_views", "conv_mfma_v9", "e4", 64, 64, W3, 2, 17, 30, res="f16", narrow=32, views=True, ragged=True),
    C("v9_floor_8192", "conv_mfma_v9", "e4", 32, 16, W3, 1, 64, 128, act=ACT_RELU, ragged=False),                                               # exactly LARGE_MAP_PIXELS: still v9
    C("v9_dy_e4", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, act=ACT_LRELU, slope=0.1, res="f16", res2="f16", grade="dyadic", ragged=True),
    C("v9_dy_round16", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, act=ACT_LRELU, slope=0.1, round16=True, grade="dyadic", ragged=True),
    C("v9_dy_none_f32", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, out="f32", res="f32", grade="dyadic", ragged=True),
    C("v9_dy_relu_1res", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, act=ACT_RELU, res="f16", grade="dyadic", ragged=True),
    C("v9_dy_lrelu_dyadic", "conv_mfma_v9", "e4", 128, 128, W3, 2, 17, 30, act=ACT_LRELU, slope=0.25, grade="dyadic", ragged=True),
    C("v9_sigmoid", "conv_mfma_v9", "e4", 64, 16, W3, 1, 17, 30, act=ACT_SIGMOID, grade="f64", ragged=True),
    C("v9_dy_clamp01", "conv_mfma_v9", "e4", 64, 16, W3, 1, 17, 30, act=ACT_CLAMP01, out="f32", grade="dyadic", ragged=True),
    C("v9_gdn", "conv_mfma_v9", "e4", 128, 128, W1, 1, 17, 30, gdn=GDN_FWD, res="f16", grade="f64", ragged=True),                              # small map: the pool is NOT rounded before the root
    # ---- conv_c8: the first layer, 3x3 8 -> 64, row segments of 32 pixels, four per workgroup
    C("c8_ragged", "conv_c8", "lean", 8, 64, W3, 1, 65, 131, act=ACT_RELU, ragged=True),
    C("c8_multi_n3", "conv_c8", "lean", 8, 64, W3, 3, 91, 97, act=ACT_LRELU, slope=0.25, multi=True, ragged=True),                             # 3 x 91 x 4 = 1092 segments on 273 workgroups
    C("c8_views", "conv_c8", "lean", 8, 64, W3, 2, 65, 131, views=True, ragged=True),
    C("c8_dy", "conv_c8", "lean", 8, 64, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, grade="dyadic", ragged=True),
    # ---- conv_n16: cout <= 32 on large maps, 8x64 tiles, epilogue4
    C("n16_7x7_c8_2", "conv_n16", "e4", 8, 2, W7, 1, 65, 131, out="f32", res="f32", ragged=True),
    C("n16_7x7_c32_16", "conv_n16", "e4", 32, 16, W7, 1, 65, 131, act=ACT_RELU, density=0.5, ragged=True),
    C("n16_3x3_c64_3_nchw", "conv_n16", "e4", 64, 3, W3, 2, 65, 131, out="nchw", ragged=True),                                              # integer planar store: the indexing
    C("n16_dy_nchw_clamp", "conv_n16", "e4", 64, 3, W3, 2, 65, 131, act=ACT_CLAMP01, out="nchw", grade="dyadic", ragged=True),                 # the model's last layer: clamp into planar fp32
    C("n16_views", "conv_n16", "e4", 32, 16, W3, 2, 65, 131, act=ACT_RELU, res="f16", views=True, ragged=True),
    C("n16_c16_32_multi", "conv_n16", "e4", 16, 32, W3, 4, 209, 259, act=ACT_LRELU, slope=0.25, res="f16", multi=True, ragged=True),            # 4 x 27 x 5 = 540 tiles on at most 512 workgroups
    C("n16_dy", "conv_n16", "e4", 32, 16, W3, 1, 65, 131, act=ACT_LRELU, slope=0.1, res="f16", grade="dyadic", ragged=True),
    C("n16_sigmoid", "conv_n16", "e4", 16, 8, W3, 1, 65, 131, act=ACT_SIGMOID, grade="f64", ragged=True),
    # ---- gdn128 and the generic GDN path (conv_mfma_v5's generic transposed form on a 1x1 over x^2)
    C("gdn128_fwd", "gdn128", "gdn", 128, 128, W1, 1, 65, 131, gdn=GDN_FWD, grade="f64", ragged=True),
    C("gdn128_fwd_res_n2", "gdn128", "gdn", 128, 128, W1, 2, 65, 131, gdn=GDN_FWD, res="f16", grade="f64", ragged=True),
    C("gdn128_inv", "gdn128", "gdn", 128, 128, W1, 1, 65, 131, gdn=GDN_INV, grade="f64", ragged=True),
    C("gdn128_views", "gdn128", "gdn", 128, 128, W1, 2, 65, 131, gdn=GDN_FWD, res="f16", views=True, grade="f64", ragged=True),              # x (= aux), res and y as channel windows
    C("gdn_generic_fwd", "conv_mfma_v5", "gdn", 128, 128, W1, 1, 65, 131, gdn=GDN_FWD, switches=(NO_GDN128,), grade="f64", ragged=True),
    C("gdn_generic_inv_res_c64", "conv_mfma_v5", "gdn", 64, 64, W1, 1, 65, 131, gdn=GDN_INV, res="f16", grade="f64", ragged=True),
    # ---- conv_f32: the fp32 islands
    C("f32_3x3", "conv_f32", "e4", 64, 64, W3, 1, 33, 47, act=ACT_LRELU, slope=0.25, x_f32=True, out="f32", res="f32", ragged=True),
    C("f32_5x5_masked", "conv_f32", "e4", 128, 256, WM, 1, 17, 30, x_f32=True, out="f32", ragged=True),
    C("f32_large", "conv_f32", "e4", 8, 64, W3, 1, 65, 131, act=ACT_RELU, x_f32=True, out="f32", ragged=True),
    C("f32_dy_lrelu01", "conv_f32", "e4", 64, 64, W3, 1, 33, 47, act=ACT_LRELU, slope=0.1, x_f32=True, out="f32", res="f32", grade="dyadic", ragged=True),
    C("f32_dy_clamp01", "conv_f32", "e4", 64, 64, W3, 1, 33, 47, act=ACT_CLAMP01, x_f32=True, out="f32", grade="dyadic", ragged=True),
    C("f32_sigmoid", "conv_f32", "e4", 64, 64, W3, 1, 33, 47, act=ACT_SIGMOID, x_f32=True, out="f16", grade="f64", ragged=True),             # an fp16 store, as the bound assumes
    C("f32_views", "conv_f32", "e4", 64, 64, W3, 2, 33, 47, act=ACT_RELU, x_f32=True, out="f32", res="f32", views=True, ragged=True),
]


def _f32(id, cin, cout, win, N, H, W, form="e4", **kw):
    return Case(id, "conv_f32", form, cin, cout, win, N, H, W, x_f32=True, ragged=True, **{"out": "f32", **kw})


# ---- conv_f32, whole-model fp32 mode: every instantiation <MT, NT> (f32_variant) at the smallest maps that take it.  A workgroup is 2 pixel
# blocks of NT groups of 32 pixels, flattened over batch, rows and columns.  Output maps:
#   1 x 129 x 131 = 16899 = 132 * 128 + 3   NT 2: the last workgroup's first block has 3 pixels, its second group and second block none
#   2 x  91 x  93 = 16926 = 132 * 128 + 30  NT 2: image 0 ends at pixel 8463 = 264 * 32 + 15, inside a 32-pixel group
#   1 x  33 x  47 =  1551 =  24 *  64 + 15  NT 1: the same tail; 2 x 33 x 47 = 3102 = 48 * 64 + 30 with image 0 ending inside a group
#   1 x  19 x  37 =   703 =  10 *  64 + 63  NT 1: a full first block and a second block of 31 pixels
#   4 x  65 x  65 = 16900 = 132 * 128 + 4   NT 2 on the four frame slices of one image
_FIRST_NEW_F32 = len(CASES)
CASES += [
    # SPyNet's 7x7 layers (ck 8: 49 taps, the zero-weight padded half step); 16 -> 2 adds the 2-channel fp32 flow into an 8-channel map
    _f32("f32_7x7_8_32", 8, 32, W7, 1, 33, 47, act=ACT_RELU),
    _f32("f32_7x7_8_32_nt2", 8, 32, W7, 1, 129, 131, act=ACT_RELU, grade="dyadic"),
    _f32("f32_7x7_32_64", 32, 64, W7, 2, 33, 47, act=ACT_RELU),
    _f32("f32_7x7_32_64_nt2", 32, 64, W7, 2, 91, 93, act=ACT_RELU, density=0.5),
    _f32("f32_7x7_64_32", 64, 32, W7, 1, 19, 37, act=ACT_RELU, grade="dyadic"),
    _f32("f32_7x7_64_32_nt2", 64, 32, W7, 1, 129, 131, act=ACT_RELU, density=0.5),
    _f32("f32_7x7_32_16", 32, 16, W7, 2, 33, 47, act=ACT_RELU),
    _f32("f32_7x7_32_16_nt2", 32, 16, W7, 2, 91, 93, act=ACT_RELU, grade="dyadic"),
    _f32("f32_7x7_16_2", 16, 2, W7, 1, 33, 47, res="f32", res_c=2),
    _f32("f32_7x7_16_2_nt2", 16, 2, W7, 1, 129, 131, res="f32", res_c=2, grade="dyadic"),
    # 3x3 64 -> 64, <2, 2>: the feature extractor, the residual stacks (one and two fp32 residuals), MCNet / LoopFilter windows
    _f32("f32_c64_nt2_none", 64, 64, W3, 1, 129, 131),
    _f32("f32_c64_nt2_none_views", 64, 64, W3, 2, 91, 93, views=True),
    _f32("f32_c64_nt2_relu", 64, 64, W3, 1, 129, 131, act=ACT_RELU, grade="dyadic"),
    _f32("f32_c64_nt2_lrelu", 64, 64, W3, 2, 91, 93, act=ACT_LRELU, slope=0.25),
    _f32("f32_c64_nt2_lrelu_views", 64, 64, W3, 1, 129, 131, act=ACT_LRELU, slope=0.1, views=True, grade="dyadic"),
    _f32("f32_c64_nt2_res", 64, 64, W3, 1, 129, 131, res="f32", grade="dyadic"),
    _f32("f32_c64_nt2_res_views", 64, 64, W3, 2, 91, 93, res="f32", views=True),
    _f32("f32_c64_nt2_res12", 64, 64, W3, 1, 129, 131, res="f32", res2="f32"),                               # F32MAPS: an fp32 res2
    _f32("f32_c64_nt2_res12_views", 64, 64, W3, 2, 91, 93, res="f32", res2="f32", views=True, grade="dyadic"),
    _f32("f32_c64_nt2_f16res_f32res2", 64, 64, W3, 1, 129, 131, act=ACT_LRELU, slope=0.1, res="f16", res2="f32", grade="dyadic"),
    # the LoopFilter's frame slices: image stride 64 < pixel stride 256; with and without .batch(3, 1)
    _f32("f32_slices_none", 64, 64, W3, 4, 65, 65, slices="all"),
    _f32("f32_slices_res", 64, 64, W3, 4, 65, 65, res="f32", slices="all", grade="dyadic"),
    _f32("f32_slices_lrelu", 64, 64, W3, 4, 65, 65, act=ACT_LRELU, slope=0.25, slices="all"),
    _f32("f32_slices_last1_lrelu", 64, 64, W3, 1, 129, 131, act=ACT_LRELU, slope=0.1, slices="last1", grade="dyadic"),
    # 3x3 64 -> 64, <2, 1>
    _f32("f32_c64_none_views", 64, 64, W3, 2, 33, 47, views=True),
    _f32("f32_c64_lrelu", 64, 64, W3, 1, 19, 37, act=ACT_LRELU, slope=0.25),
    _f32("f32_c64_lrelu_views", 64, 64, W3, 2, 33, 47, act=ACT_LRELU, slope=0.1, views=True, grade="dyadic"),
    # the plain stride-2 form (fp32 maps never take the space-to-depth view) on odd input maps: 65 x 93 -> 33 x 47, 257 x 261 -> 129 x 131
    _f32("f32_s2_c64_views", 64, 64, S3, 1, 65, 93, act=ACT_LRELU, slope=0.25, views=True),
    _f32("f32_s2_c64_views_nt2", 64, 64, S3, 1, 257, 261, act=ACT_LRELU, slope=0.1, views=True, grade="dyadic"),
    _f32("f32_c8_64_nt2", 8, 64, W3, 1, 129, 131, act=ACT_LRELU, slope=0.25),
    # conv_offset_mask, cout 216: rows 216..255 of the last cout tiles store nothing
    _f32("f32_c64_216_nt2", 64, 216, W3, 1, 129, 131),
    _f32("f32_c64_216_views", 64, 216, W3, 2, 33, 47, views=True, grade="dyadic"),
    # the model's last layer: clamp into planar fp32
    _f32("f32_c64_3_nchw_nt2", 64, 3, W3, 1, 129, 131, act=ACT_CLAMP01, out="nchw", grade="dyadic"),
    # 3x3 128 -> 64 and the 1x1 layers (Cin 192 = 6 chunks of ck 32, 256 = 8)
    _f32("f32_c128_64_lrelu", 128, 64, W3, 1, 33, 47, act=ACT_LRELU, slope=0.25, density=0.5),
    _f32("f32_c128_64_nt2_none", 128, 64, W3, 1, 129, 131, density=0.5),
    _f32("f32_c128_64_nt2_lrelu", 128, 64, W3, 2, 91, 93, act=ACT_LRELU, slope=0.1, grade="dyadic", density=0.5),
    _f32("f32_c128_64_nt2_lrelu_views", 128, 64, W3, 1, 129, 131, act=ACT_LRELU, slope=0.25, views=True, density=0.5),
    _f32("f32_1x1_192_64_nt2_views", 192, 64, W1, 1, 129, 131, views=True),
    _f32("f32_1x1_128_64_lrelu", 128, 64, W1, 2, 33, 47, act=ACT_LRELU, slope=0.1, grade="dyadic"),
    _f32("f32_1x1_128_64_nt2_lrelu", 128, 64, W1, 1, 129, 131, act=ACT_LRELU, slope=0.25),
    _f32("f32_1x1_256_64_nt2_lrelu", 256, 64, W1, 2, 91, 93, act=ACT_LRELU, slope=0.1, grade="dyadic"),
    # fp32 GDN / inverse GDN: fp32 pool, fp32 multiplicand (conv_common.h:99-102), float64 grade
    _f32("f32_gdn_fwd_c128", 128, 128, W1, 1, 33, 47, form="gdn32", gdn=GDN_FWD, res="f32", grade="f64"),
    _f32("f32_gdn_inv_c128", 128, 128, W1, 1, 33, 47, form="gdn32", gdn=GDN_INV, res="f32", grade="f64"),
    _f32("f32_gdn_fwd_c64", 64, 64, W1, 1, 33, 47, form="gdn32", gdn=GDN_FWD, grade="f64"),
    _f32("f32_gdn_inv_c64", 64, 64, W1, 1, 33, 47, form="gdn32", gdn=GDN_INV, grade="f64"),
]
F32_MODE_CASES = CASES[_FIRST_NEW_F32:]         # tests/test_conv_exact_cases_cpu.py checks the exactness preconditions of these on the CPU

# (window (kh, kw, taps), stride, Cin, cout) of every conv that `VideoCompressor.model_fp32` runs on fp32 maps.  F32_LAYERS: everything
# outside the two coders -- each call class of these (conv_f32_class) has a row above; F32_CODER_LAYERS: the layers of MVCoder / ResCoder,
# whose shapes tests/test_conv_f32_gpu.py holds.  tests/test_fp32_ops_gpu.py::test_model_fp32_call_classes_have_cases holds the union to
# what production reaches, in both directions.
_K1, _K3, _K7, _KM = (1, 1, 1), (3, 3, 9), (7, 7, 49), (5, 5, 12)
F32_LAYERS = {(_K7, 1, 8, 32), (_K7, 1, 32, 64), (_K7, 1, 64, 32), (_K7, 1, 32, 16), (_K7, 1, 16, 2),
              (_K3, 1, 8, 64), (_K3, 1, 64, 64), (_K3, 2, 64, 64), (_K3, 1, 64, 216), (_K3, 1, 64, 3), (_K3, 1, 128, 64),
              (_K1, 1, 128, 64), (_K1, 1, 192, 64), (_K1, 1, 256, 64)}
F32_CODER_LAYERS = {(_K3, 2, 64, 128), (_K3, 2, 128, 128), (_K3, 1, 128, 128), (_K1, 2, 64, 128), (_K1, 2, 128, 128), (_K1, 1, 128, 128),
                    (_K3, 1, 128, 192), (_K3, 1, 192, 256), (_K3, 1, 128, 256), (_K3, 1, 128, 512), (_K3, 1, 192, 768), (_KM, 1, 128, 256),
                    (_K1, 1, 512, 426), (_K1, 1, 432, 341), (_K1, 1, 344, 256)}

# conv_pair: two 3x3 64 -> 64 convs in one launch; strips of 30 or 62 columns (both run for every case)
PAIR_CASES = [
    C("pair_w61", "conv_pair", "pair", 64, 64, W3, 1, 135, 61, act=ACT_RELU, add_input=True, ragged=True),                         # 62 k - 1
    C("pair_w62", "conv_pair", "pair", 64, 64, W3, 1, 133, 62, act=ACT_RELU, act2=ACT_LRELU, slope2=0.5, res2="f16", ragged=True),            # 62 k: full 62-column strips, ragged in the 30-column geometry (2 strips + 2 px) and in H; conv2 sums stay integers: a slope only after it
    C("pair_w63", "conv_pair", "pair", 64, 64, W3, 2, 131, 63, act=ACT_RELU, add_input=True, res2="f16", views=True, ragged=True),  # 62 k + 1: a last strip of one column
    C("pair_w125_n3", "conv_pair", "pair", 64, 64, W3, 3, 67, 125, act=ACT_NONE, act2=ACT_RELU, add_input=True, multi=True, ragged=True),
    C("pair_dy", "conv_pair", "pair", 64, 64, W3, 1, 133, 63, act=ACT_LRELU, slope=0.125, act2=ACT_LRELU, slope2=0.125, add_input=True, res2="f16", grade="dyadic", ragged=True),
]
del C


def window(case):
    return HD.WINDOWS[case.win]


def out_map(case):
    kh, kw, stride, pad, _ = window(case)
    return (case.H + 2 * pad - kh) // stride + 1, (case.W + 2 * pad - kw) // stride + 1


def f32_variant_of(cout, npix):
    """conv_f32's template instantiation <MT, NT> (csrc/conv_f32.hip:290-297): one 32-row cout tile up to cout 32, else two per wave;
    two 32-pixel groups per wave from N * Ho * Wo = 16384 output pixels on"""
    return (1 if cout <= 32 else 2, 2 if npix >= 16384 else 1)


def f32_variant(case):
    Ho, Wo = out_map(case)
    return f32_variant_of(case.cout, case.N * Ho * Wo)


def conv_f32_class(L, d):
    """the call class of a conv_f32 launch, from its descriptor (a case's guard_desc or a production call's ops.conv_desc):
    (window (kh, kw, taps), stride, Cin, cout, <MT, NT>, act, (dtype, C) of res and res2, (gdn, dtype of the multiplicand), output
    kind, output dtype, layout).  Layout: "slices" when a map's image stride is smaller than its pixel stride (FM.as_slices), else
    "window" when a map's pixel stride exceeds its channels, else "dense"."""
    Ho = (d.x.H + 2 * d.pad - d.kh) // d.stride + 1
    Wo = (d.x.W + 2 * d.pad - d.kw) // d.stride + 1
    dt = lambda m: "f32" if m.dtype == L.F32 else "f16"
    rs = lambda m: (dt(m), int(m.C)) if m.p else None
    kind = {L.OUT_NHWC: "nhwc", L.OUT_SHUFFLE2: "shuffle", L.OUT_NCHW_F32: "nchw"}[d.out_mode]
    maps = [d.x] + ([d.y] if kind != "nchw" else []) + [m for m in (d.res, d.res2, d.aux) if m.p]
    layout = "slices" if any(m.sn < m.sp for m in maps) else "window" if any(m.sp != m.C for m in maps) else "dense"
    return ((int(d.kh), int(d.kw), int(d.ntaps)), int(d.stride), int(d.x.C), int(d.cout), f32_variant_of(d.cout, d.x.N * Ho * Wo), int(d.act),
            rs(d.res), rs(d.res2), (int(d.gdn), dt(d.aux)) if d.gdn else None, kind, "f32" if kind == "nchw" else dt(d.y), layout)


def f32_layer(cls):
    """(window, stride, Cin, cout) of a conv_f32 class"""
    return cls[:4]


def x_channels(case):
    return HD.pad8(case.cin)


def y_channels(case):
    """(channels of the output view, channels the conv defines inside it)"""
    if case.out == "nchw" or (case.out == "f32" and not case.x_f32):
        return case.cout, case.cout
    c = case.cout // 4 if case.out == "shuffle" else case.cout
    return HD.pad8(c) - case.narrow, min(c, HD.pad8(c) - case.narrow)


# ------------------------------------------------------------------------------------------------- the CPU guard's descriptor
def guard_desc(L, pick_ck, case):
    """the descriptor ops.conv builds for the case, over dummy pointers (helpers_conv_dispatch)"""
    kw = dict(act=case.act, slope=case.slope, res=case.res, res2=case.res2, out=case.out, narrow=case.narrow)
    if case.form == "gdn32":                # the GDN call of ops.conv on fp32 maps: x, the multiplicand (aux == x), res and y all fp32
        d = HD.desc(L, lambda *a: 32, case.cin, case.cout, window(case), case.H, case.W, case.N, res=case.res, out="f32", x_f32=True)
        d.square_input, d.gdn = 1, case.gdn
        d.aux = HD.fmap(L, HD.PX, case.N, case.H, case.W, case.cin, dtype=L.F32)
    elif case.gdn:
        d = HD.gdn_desc(L, case.cin, case.H, case.W, case.N, case.gdn, res=case.res)
    elif case.bcast:
        d = HD.bcast_desc(L, case.cin, case.H, case.W, case.N)
        if case.bcast == "outofplace":
            d.res = HD.fmap(L, HD.PR1, case.N, case.H, case.W, 64, 256)
    elif case.s2d:
        # ops.conv_desc: up to ops.SMALL_MAP_PIXELS output pixels over the batch a stride-2 3x3 layer runs in its plain form
        assert case.N * (case.H // 2) * (case.W // 2) > 8192 and case.win == S3 and case.cin % 32 == 0 and case.cout >= 64, case.id
        d = HD.s2d_desc(L, case.cin, case.cout, case.H // 2, case.W // 2, case.N, **kw)
    else:
        assert not (case.win == S3 and case.cin % 32 == 0 and case.cout >= 64 and not case.x_f32) or case.N * out_map(case)[0] * out_map(case)[1] <= 8192, case.id
        d = HD.desc(L, pick_ck, x_channels(case), case.cout, window(case), case.H, case.W, case.N, bias=case.bias, round16=case.round16,
                    x_f32=case.x_f32, **kw)
        if case.out == "f32" and not case.x_f32 and case.cout % 8:      # ops.conv: an fp32 output of an fp16 conv is exactly cout wide
            for m in (d.y, d.res, d.res2):
                if m.p:
                    m.C = m.sp = case.cout
                    m.sn = m.H * m.W * m.sp
    if case.res_c:                                                       # a dense residual map of its own, narrower than y
        d.res.C = d.res.sp = case.res_c
        d.res.sn = d.res.H * d.res.W * case.res_c
    if case.slices:                                                      # FM.as_slices(b, 4, 64) [.batch(3, 1)]: images interleaved inside a pixel
        assert case.cin == case.cout == 64 and case.N == (4 if case.slices == "all" else 1) and not case.views and not case.res2, case.id
        for m in (d.x, d.y, d.res):
            if m.p:
                m.sn, m.sp = 64, 256
    if case.views and not case.bcast:                                    # wider buffers: only the strides change
        for m, extra in ((d.x, 16), (d.y, 24), (d.res, 8), (d.res2, 40)):
            if m.p:
                m.sp += extra
                m.sn = m.H * m.W * m.sp
        if case.gdn:
            d.aux.sp, d.aux.sn = d.x.sp, d.x.sn
    return d


# ------------------------------------------------------------------------------------------------- data
def _ints(gen, shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=gen).float()


def _thin(gen, w, density):
    return w if density >= 1.0 else w * (torch.rand(w.shape, generator=gen) < density).float()


@dataclass
class Data:
    x: torch.Tensor                      # (N, cin, H, W) fp32 holding the values the kernel sees
    w: torch.Tensor                      # (cout, cin, kh, kw), masked taps already zero
    b: torch.Tensor | None
    r1: torch.Tensor | None = None       # residuals at the output geometry, output-view channels
    r2: torch.Tensor | None = None
    taps: list | None = None
    w2: torch.Tensor | None = None       # conv_pair
    b2: torch.Tensor | None = None
    slices: torch.Tensor | None = None   # bcast: (N, 256, H, W), the four 64-channel slices
    ref: torch.Tensor | None = None      # (N, yc, Ho, Wo): expected values of the conv-defined channels, exactly
    tol: torch.Tensor | None = None      # f64 grade: elementwise bound


def make_data(case):
    g = torch.Generator().manual_seed(1000 + case.seed + sum(map(ord, case.id)))
    kh, kw, stride, pad, taps = window(case)
    Ho, Wo = out_map(case)
    yH, yW = (2 * Ho, 2 * Wo) if case.out == "shuffle" else (Ho, Wo)
    _, yc = y_channels(case)
    integer = case.grade == "int"
    if integer:
        x = _ints(g, (case.N, case.cin, case.H, case.W), 2)
        w = _thin(g, _ints(g, (case.cout, case.cin, kh, kw), 2), case.density)
        b = _ints(g, (case.cout,), 8)
        mk_res = lambda: _ints(g, (case.N, yc, yH, yW), 16)
    else:
        x = _ints(g, (case.N, case.cin, case.H, case.W), 16) / 8
        w = _thin(g, _ints(g, (case.cout, case.cin, kh, kw), 8), case.density) / 64
        b = _ints(g, (case.cout,), 256) / 512
        mk_res = lambda: _ints(g, (case.N, yc, yH, yW), 256) / 64
    if case.act == ACT_SIGMOID:          # keeps |conv| <= 8 (f64_reference)
        w = w / 8
    if taps is not None:
        m = torch.zeros(kh, kw)
        for dy, dx in taps:
            m[dy, dx] = 1
        w = w * m
    d = Data(x, w, b if case.bias else None, taps=taps)
    if case.gdn:                         # gamma >= 0, beta > 0: a positive pool
        d.w = w.abs() / 4 + (torch.eye(case.cout).view(case.cout, case.cin, 1, 1) / 8 if case.cin == case.cout else 0)
        d.b = (b.abs() + 1 / 8)
    if case.res:
        d.r1 = mk_res()
    if case.res2:
        d.r2 = mk_res()
    if case.bcast:
        d.slices = (_ints(g, (case.N, 256, Ho, Wo), 16) if integer else _ints(g, (case.N, 256, Ho, Wo), 256) / 64)
    if case.kernel == "conv_pair":       # integer grade: the ternary chain (w1 at density 0.5, w2 at 0.25)
        if integer:
            d.w, d.w2 = _thin(g, _ints(g, (64, 64, 3, 3), 1), 0.5), _thin(g, _ints(g, (64, 64, 3, 3), 1), 0.25)
            d.b2 = _ints(g, (64,), 8)
        else:
            d.w2, d.b2 = _ints(g, (64, 64, 3, 3), 4) / 64, _ints(g, (64,), 256) / 512
    return d


def h16(t):
    return t.half().float()


def check_exact(case, stages, abs_sum):
    """the preconditions of the exact grades, on the reference: sums below 2^24 in the accumulator's units, and (integer grade)
    every stored or fp16-rounded stage at most 2048 and an exact fp16 value (an integer, or an integer times the slope 2^-k)"""
    unit = 1.0 if case.grade == "int" else 2.0 ** 9
    assert float(abs_sum.max()) * unit < 2 ** 24, (case.id, float(abs_sum.max()))
    if case.grade == "int":
        for name, s in stages:
            assert float(s.abs().max()) <= 2048 and bool((h16(s) == s).all()), (case.id, name, float(s.abs().max()))


def _act32(v, act, slope):
    """csrc/common.h act_apply, in fp32"""
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))
    if act == ACT_CLAMP01:
        return v.clamp(0.0, 1.0)
    assert act == ACT_NONE
    return v


def _max_slope16(h, act, slope):
    """packed fp16 activation of the lean forms: max(h, h * fp16(slope)), the product rounded to fp16"""
    if act == ACT_RELU:
        return torch.maximum(h, torch.zeros_like(h))
    if act == ACT_LRELU:
        return torch.maximum(h, h16(h * h16(torch.tensor(slope))))
    return h


def epilogue(form, v, act, slope, round16, r1, r2, out_f32):
    """the rounding sequences of csrc/conv_common.h on the exact fp32 value v = conv + bias (output geometry)"""
    stages = [("conv + bias", v)]
    if form == "e4":                     # epilogue4: everything in fp32, one rounding at the store
        if round16:
            v = h16(v)
        v = _act32(v, act, slope)
        stages.append(("activation", v))
        for r in (r1, r2):
            if r is not None:
                v = v + r
                stages.append(("residual sum", v))
        return (v if out_f32 else h16(v)), stages
    assert not out_f32 and not round16
    if form == "generic":                # epilogue_pack: max(v, v * slope) in fp32, rounded; fp16 residual adds
        s = torch.tensor({ACT_NONE: 1.0, ACT_RELU: 0.0}.get(act, slope), dtype=torch.float32)
        h = h16(torch.maximum(v, v * s))
    else:                                # lean: rounded first, the activation in packed fp16
        assert form == "lean"
        h = _max_slope16(h16(v), act, slope)
    stages.append(("activation", h))
    for r in (r1, r2):
        if r is not None:
            h = h16(h + r)
            stages.append(("residual sum", h))
    return h, stages


def reference(case, d):
    """fills d.ref (and d.tol for the f64 grade); asserts the grade's preconditions"""
    _, _, stride, pad, _ = window(case)
    if case.kernel == "conv_pair":
        return _pair_reference(case, d)
    if case.grade == "f64":
        return f64_reference(case, d)
    v = F.conv2d(d.x, d.w, d.b, stride=stride, padding=pad)
    abs_sum = F.conv2d(d.x.abs(), d.w.abs(), None if d.b is None else d.b.abs(), stride=stride, padding=pad)
    if case.out == "shuffle":
        v = F.pixel_shuffle(v, 2)
    _, yc = y_channels(case)
    v = v[:, :yc]
    if case.bcast:                       # lean row (no activation), then bcast_add_act's arithmetic per slice
        h = h16(v)
        s = d.slices.view(case.N, 4, 64, *v.shape[2:]) + h[:, None]
        y = h16(torch.where(s > 0, s, s * torch.tensor(0.2, dtype=torch.float32)))
        check_exact(case, [("conv + bias", v), ("slice + conv", s)], abs_sum)      # 0.2 is no dyadic slope: the product s * 0.2f and the store round as restated
        d.ref = y.reshape(case.N, 256, *v.shape[2:])
        return d
    y, stages = epilogue(case.form, v, case.act, case.slope, case.round16, d.r1, d.r2, case.out in ("f32", "nchw"))
    check_exact(case, stages + [("output", y)], abs_sum)
    if case.chan_sum:                    # the fused channel sums are fp32 sums of the stored values in the kernel's order: exact below 2^24
        assert case.grade == "int" and float(y.abs().sum((2, 3)).max()) < 2 ** 24, case.id
    d.ref = y
    return d


def _pair_reference(case, d):
    """the sequence of tests/test_conv_pair_gpu.py::_ref: both conv results and both activations rounded to fp16, fp16 adds"""
    a1 = F.conv2d(d.x, d.w, d.b, padding=1)
    t = h16(_act32(h16(a1), case.act, case.slope))
    a2 = F.conv2d(t, d.w2, d.b2, padding=1)
    y = h16(_act32(h16(a2), case.act2, case.slope2))
    stages = [("conv1", a1), ("intermediate map", t), ("conv2", a2), ("activation 2", y)]
    if case.add_input:
        y = h16(y + d.x)
        stages.append(("+ x", y))
    if d.r2 is not None:
        y = h16(y + d.r2)
        stages.append(("+ res2", y))
    s1 = F.conv2d(d.x.abs(), d.w.abs(), d.b.abs(), padding=1)
    s2 = F.conv2d(t.abs(), d.w2.abs(), d.b2.abs(), padding=1)
    check_exact(case, stages, torch.maximum(s1.max(), s2.max()))
    if case.grade == "dyadic":           # t is a multiple of 2^-12 after the slope, w2 of 2^-6: conv2's unit is 2^-18
        assert float(s2.max()) * 2.0 ** 18 < 2 ** 24 and float(s1.max()) * 2.0 ** 9 < 2 ** 24, case.id
    d.ref = y
    return d


def f64_reference(case, d):
    """GDN / inverse GDN and the sigmoid on dyadic data.  The fp32 value that enters the inexact operation is exact (asserted), so
    the kernel's error is: the operation itself (v_rsq_f32 / v_sqrt_f32 / v_exp_f32 + v_rcp_f32, about one fp32 ulp each), one fp32
    product, one fp32 add per residual, one fp16 store:
        |d| <= EPS16 |ref| + 8 EPS32 (|x root| + |res|) + TINY16        (= R16 |ref| + TINY16 without a residual)
    Form "gdn" (gdn128, and the generic transposed epilogue): the pool is STORED AS fp16 before the root (conv_gdn128.hip, "norm +
    beta -> fp16"; epilogue_pack's PackedRow) -- the reference rounds it the same way, exactly, instead of widening the bound.
    Sigmoid, 1 / (1 + __expf(-v)) with __expf = v_exp_f32(v log2 e): the rounded product v log2 e errs by EPS32 |v| log2 e and the rounded
    constant log2 e by half as much again, i.e. 1.5 |v| EPS32 relative in e^-v; v_exp_f32 itself is good to one ulp (2 EPS32), the add and the
    division to EPS32 each.  |v| <= 8 here (asserted): 12 + 2 + 1 + 1 = 16 EPS32 next to the fp16 store,
        |d| <= (EPS16 + 16 EPS32) |ref| + TINY16"""
    _, _, stride, pad, _ = window(case)
    _, yc = y_channels(case)
    if case.gdn:
        x2 = d.x * d.x
        assert bool((h16(x2) == x2).all()), "x^2 must be an exact fp16 value (packed fp16 square in gdn128)"
        pool = F.conv2d(x2, d.w, d.b)
        assert float(F.conv2d(x2, d.w.abs(), d.b.abs()).max()) * 2.0 ** 14 < 2 ** 24       # unit: 2^-6 (x^2) * 2^-8 (gamma); beta in 2^-9
        assert float(pool.min()) > 0
        p = (h16(pool) if case.form == "gdn" else pool).double()
        term = d.x.double() * (p.rsqrt() if case.gdn == GDN_FWD else p.sqrt())
        ref, mag = term, term.abs()
        if d.r1 is not None:
            ref, mag = ref + d.r1.double(), mag + d.r1.double().abs()
        d.ref = ref
        if case.form == "gdn32":
            # conv_f32, fp32 multiplicand and fp32 store (conv_common.h:99-102): a (1.0f / sqrtf(pool)) forward, a sqrtf(pool) inverse.  The
            # library is built without fast-math and hipcc rounds fp32 sqrt and division correctly by default (no
            # -fno-hip-fp32-correctly-rounded-divide-sqrt, csrc/Makefile), so each operation errs by at most EPS32 relative.  The pool and
            # a are exact: forward = root, division, product (3), inverse = root, product (2) roundings of the term, one more of the sum
            # when a residual is added, none at the fp32 store.  1 + 2^-16 covers the second-order terms.
            assert case.out == "f32"
            k = 3 if case.gdn == GDN_FWD else 2
            d.tol = (k * term.abs() + (ref.abs() if d.r1 is not None else 0.0)) * EPS32 * (1 + 2.0 ** -16)
            return d
        d.tol = (R16 * ref.abs() if d.r1 is None else EPS16 * ref.abs() + 8 * EPS32 * mag) + TINY16
        return d
    assert case.act == ACT_SIGMOID
    v = F.conv2d(d.x, d.w, d.b, stride=stride, padding=pad)[:, :yc]
    assert float(F.conv2d(d.x.abs(), d.w.abs(), d.b.abs(), stride=stride, padding=pad).max()) * 2.0 ** 12 < 2 ** 24
    assert float(v.abs().max()) <= 8
    d.ref = torch.sigmoid(v.double())
    d.tol = (EPS16 + 16 * EPS32) * d.ref.abs() + TINY16
    return d
