"""Case tables, data, float64 references and counted bounds of the streaming launchers on fp32 maps (tests/test_fp32_ops_gpu.py runs them on
the GPU, tests/test_fp32_ops_cases_cpu.py checks the tables, and the sensitivity of every bound, without one).  Nothing here touches
the compiled library.

All data is made on the CPU, as NHWC tensors in the dtype the kernel reads (fp16 maps hold fp16-exact values).  The bounds, with their counts
(EPS32 = 2^-24 is half an fp32 ulp, relative; the library builds with -ffp-contract=off and without fast-math, so every fp32 operation,
division and square root included, is rounded correctly once):

  add_flow, bcast_add_act, cast_f32 / copy_cast   one fp32 add (and the slope product) per element, or none: compared bit for bit with
                  the same fp32 sequence in torch on the CPU, stored in the output's dtype.
  upsample2x      weights are exact multiples of 1/4; four products, three sums: 6 roundings of at most |w| * |x| each, so
                  6 EPS32 absr with absr the interpolation of |x|; an fp16 output adds its store, EPS16 |ref| + TINY16.
  spynet_level_input   tests/test_forward_ops_gpu.py::_level_bound (the flow's bilinear sum, the sampling coordinate's round trip times the
                  largest neighbour difference, the four-term warp sum) with the fp16 store of cat8, EPS16 |cat| + TINY16, replaced by
                  EPS32 |cat|: an fp32 cat8 stores the fp32 values the kernel computed.  Channels 0..2 are copies (bit-equal to ref),
                  flow_up does not depend on cat8's dtype (bit-equal to the fp16-cat8 call).
  channel_sum     per (image, block, channel): a lane adds ceil(per / lanes) values serially, then `lanes` lane sums are added serially:
                  (ceil(per / lanes) + lanes) EPS32 sum|x| over the block, whatever the order inside the four-load loop.
  avgpool_k       a strip of at most 8 rows: ceil(8 scale / lanes) serial adds per lane, `lanes` lane sums, nsplit strip sums, one division:
                  (ceil(8 scale / lanes) + lanes + nsplit + 1) EPS32 mean|x| of the cell.
  match_gather    cor = a.b / max(|a| |b|, 1e-8) over 64 channels.  A term of the dot or of a squared norm passes one product, 7 serial
                  additions in its lane and 3 shuffle additions: 11 roundings.  The dot errs by 11 EPS32 sum|a_i b_i| <= 11 EPS32 |a| |b|
                  (Cauchy-Schwarz): relative to the DENOMINATOR, so free of the dot's conditioning.  Each norm: 11 EPS32 relative in
                  the square, halved by the root, plus the root's own rounding: 6.5; the product of the two roots and the division: 2.
                  |d cor| <= (11 + 13 + 2) EPS32 = 26 EPS32, inside the 80 EPS32 the bound grants.  An element a cor (b cor) rounds once
                  more: 80 EPS32 |a| + EPS32 |ref|, plus EPS16 |ref| + TINY16 for an fp16 cat.  Pixels with |a| |b| < 1e-6 would take
                  the 1e-8 clamp, where the relative argument fails: the data has none but the zero sources (cor = 0 exactly), asserted
                  on the reference.
"""

import torch
import torch.nn.functional as F

EPS16 = 2.0 ** -11
EPS32 = 2.0 ** -24
TINY16 = 2.0 ** -25
DT = {"f16": torch.float16, "f32": torch.float32}


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(str(k) for k in key))))


def draw(g, shape, dt, scale=1.0, shift=0.0):
    """normal values in the dtype the kernel reads: fp16-exact for an fp16 map, full fp32 mantissas for an fp32 one"""
    return (torch.randn(shape, generator=g) * scale + shift).to(DT[dt])


def lrelu32(v, slope):
    return torch.where(v > 0, v, v * torch.tensor(slope, dtype=torch.float32))


def ratio(got, ref, bound):
    """max(|d| / bound) with 0 / 0 = 0 (an exact element under a zero bound)"""
    d = (got.double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------- call classes (shared with the guard)
def dt_of(fm):
    return "f32" if fm.f32 else "f16"


def is_dense(fm):
    return fm.off == 0 and fm.sp == fm.C and fm.sn == fm.H * fm.W * fm.C


def cls_spynet32(base, cat8):
    """tests/test_forward_ops_gpu.py::cls_spynet plus the dtype of cat8"""
    return base + (dt_of(cat8),)


def cs_lanes(C_):
    return 256 // (C_ // 8)


def cls_channel_sum(dt, C_, npix, nblocks):
    per = -(-npix // nblocks)
    return ("channel_sum", dt, C_, "loop4" if per > 3 * cs_lanes(C_) else "tail")         # channel_sum_block (pointwise_common.h): the four-loads loop


def cls_avgpool_k(dt, C_, scale, dense):
    return ("avgpool_k", dt, C_, "split" if scale > 8 else "one", "dense" if dense else "view")      # nsplit = ceil(scale / POOL_ROWS)


def cls_match_gather(dts, dense):
    return ("match_gather", tuple(dts), "dense" if dense else "view")


def cls_copy_cast(sdt, ddt, dense):
    return ("copy_cast", sdt, ddt, "dense" if dense else "view")


# ------------------------------------------------------------------------------------------------- add_flow
# (name, N, H, W, C of off, off buffer channels, flow buffer channels); off is fp32, the flow always is
AF_CASES = [("dense_c64_f2", 1, 16, 24, 64, 64, 2), ("view_c64_f4", 2, 5, 7, 64, 128, 4), ("view_c8_f8", 1, 1, 9, 8, 16, 8),
            ("dense_c8_f2", 3, 3, 1, 8, 8, 2), ("dense_c64_f8", 1, 4, 6, 64, 64, 8)]


def af_class(row):
    _, _, _, _, C_, Cb, Cf = row
    return ("add_flow", "dense" if Cb == C_ else "view", Cf, "f32")


def af_data(row):
    name, N, H, W, C_, Cb, Cf = row
    g = gen("add_flow", name)
    return draw(g, (N, H, W, Cb), "f32"), draw(g, (N, H, W, Cf), "f32", 4.0)


def af_want(row, off, flow):
    C_, Cb = row[4], row[5]
    return off[..., Cb - C_:] + flow[..., :2].repeat(1, 1, 1, C_ // 2)


# ------------------------------------------------------------------------------------------------- bcast_add_act
# (N, H, W, Cb, T, x dtype, b dtype, wide): every (x, b) dtype pair with every T the launcher forks on
BC_CASES = [(2, 8, 16, 64, 4, "f32", "f32", False), (1, 5, 7, 64, 4, "f32", "f16", True), (1, 3, 5, 8, 4, "f16", "f32", False),
            (1, 5, 7, 64, 4, "f16", "f16", True), (2, 3, 5, 64, 3, "f32", "f32", True), (1, 1, 9, 8, 3, "f32", "f16", False),
            (1, 4, 1, 64, 3, "f16", "f32", True), (1, 2, 3, 8, 3, "f16", "f16", False), (1, 1, 9, 64, 2, "f32", "f32", True),
            (3, 2, 2, 8, 2, "f32", "f16", False), (1, 3, 3, 64, 2, "f16", "f32", False), (1, 1, 1, 8, 2, "f16", "f16", True)]


def bc_data(row):
    N, H, W, Cb, T, xdt, bdt, wide = row
    g = gen("bcast", *row)
    return draw(g, (N, H, W, T * Cb + (64 if wide else 0)), xdt), draw(g, (N, H, W, Cb), bdt)


def bc_want(row, xbuf, b):
    N, H, W, Cb, T, xdt, bdt, wide = row
    x = xbuf[..., (64 if wide else 0):]
    return lrelu32(x.float() + b.float().repeat(1, 1, 1, T), 0.1).to(DT[xdt])


# ------------------------------------------------------------------------------------------------- upsample2x
# (N, h, w, C, x dtype, y dtype, x view, y view): the 1 x w, h x 1 and 1 x 1 clamps in every dtype pair that has an fp32 map
UP_CASES = [(2, 9, 15, 64, "f32", "f32", False, False), (1, 1, 7, 64, "f32", "f32", True, False), (1, 6, 1, 8, "f32", "f32", False, True),
            (3, 1, 1, 16, "f32", "f32", True, True), (2, 5, 4, 64, "f32", "f16", False, True), (1, 1, 5, 8, "f32", "f16", True, False),
            (1, 3, 1, 8, "f32", "f16", False, False), (2, 5, 4, 64, "f16", "f32", True, False), (1, 1, 1, 8, "f16", "f32", False, True),
            (1, 7, 1, 16, "f16", "f32", False, False), (1, 1, 6, 8, "f16", "f32", False, False)]


def up_data(row):
    N, h, w, C_, xdt, ydt, vin, vout = row
    return draw(gen("upsample", *row), (N, h, w, C_ + (16 if vin else 0)), xdt)


def up_ref(row, xbuf, x16=False):
    """-> (float64 reference, bound), NHWC.  x16: the reference of the same values rounded to fp16 (the sensitivity check)"""
    N, h, w, C_, xdt, ydt, vin, vout = row
    x = xbuf[..., (16 if vin else 0):]
    x = (x.half() if x16 else x).double().permute(0, 3, 1, 2)
    ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    absr = F.interpolate(x.abs(), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    return ref, 6 * EPS32 * absr + ((EPS16 * ref.abs() + TINY16) if ydt == "f16" else 0.0)


# ------------------------------------------------------------------------------------------------- spynet_level_input, fp32 cat8
# (N, H, W, with flow_lo, ref / supp channels (4: the vector kernel, 3: the scalar one), cat8 a window of a 16-channel buffer)
SP_CASES = [(2, 34, 60, True, 4, False), (2, 34, 60, True, 3, True), (1, 16, 24, False, 4, True), (1, 16, 24, False, 3, False),
            (1, 2, 2, True, 4, True), (3, 2, 8, True, 3, False), (1, 8, 2, True, 4, False), (1, 2, 2, False, 3, True)]


def sp_data(row):
    N, H, W, fl, Cs, win = row
    g = gen("spynet", *row)
    ref, supp = torch.rand(N, H, W, 4, generator=g), torch.rand(N, H, W, 4, generator=g)
    flo = torch.randn(N, H // 2, W // 2, 2, generator=g) * 4.0 if fl else None
    return ref, supp, flo


def sp_bound32(bc16, cat):
    """_level_bound's cat8 bound with the fp16 store term replaced: EPS16 |cat| + TINY16 -> EPS32 |cat|"""
    return bc16 - (EPS16 * cat.abs() + TINY16) + EPS32 * cat.abs()


# ------------------------------------------------------------------------------------------------- cast_f32 / copy_cast
# (name, N, H, W, C, src dtype, dst dtype, src view, dst view); "cast_f32" rows go through ops.cast_f32 (fresh dense output)
CC_CASES = [("cast_f32", 2, 5, 7, 64, "f16", "f32", False, False), ("cast_f32_view", 1, 3, 9, 64, "f16", "f32", True, False),
            ("copy_f16_f32_dst_view", 1, 6, 5, 64, "f16", "f32", False, True), ("copy_f32_f32_views", 2, 1, 7, 8, "f32", "f32", True, True)]


def cc_class(row):
    _, _, _, _, _, sdt, ddt, vs, vd = row
    return cls_copy_cast(sdt, ddt, not (vs or vd))


# ------------------------------------------------------------------------------------------------- channel_sum
# (name, dtype, N, H, W, C, nblocks, x view).  lanes = 256 / (C / 8) pixel lanes; a block of `per` = ceil(npix / nblocks) pixels runs the
# four-load loop when per > 3 lanes, otherwise only the tail loop
CS_CASES = [
    ("c8_loop", "f32", 1, 31, 33, 8, 1, False),              # lanes 256, per 1023: one pass of the loop for lanes 0..254, then the tail
    ("c64_loop", "f32", 2, 17, 23, 64, 3, True),             # lanes 32, per 131 > 96; 391 = 3 * 131 - 2: a shorter last block
    ("c128_loop", "f32", 1, 9, 11, 128, 2, False),           # lanes 16, per 50 > 48
    ("c256_loop", "f32", 1, 7, 9, 256, 2, True),             # lanes 8, per 32 > 24
    ("c64_tail", "f32", 2, 7, 11, 64, 3, False),             # per 26 <= 96: tail only; last block 25 pixels < 32 lanes
    ("c256_tail", "f32", 1, 5, 5, 256, 2, False),            # per 13 <= 24; last block 12
    ("c128_tail_empty", "f32", 1, 2, 5, 128, 6, True),       # per 2: blocks 0..4 hold two pixels, block 5 none
    ("c8_tail", "f32", 1, 1, 9, 8, 2, True),
    ("c64_loop_f16", "f16", 2, 17, 23, 64, 3, False),
    ("c128_tail_f16", "f16", 1, 3, 5, 128, 2, True),
    ("c8_loop_f16", "f16", 1, 31, 33, 8, 1, True),
    ("c256_loop_f16", "f16", 1, 7, 9, 256, 2, False),
]


def cs_class(row):
    _, dt, N, H, W, C_, nb, v = row
    return cls_channel_sum(dt, C_, H * W, nb)


def cs_data(row):
    name, dt, N, H, W, C_, nb, v = row
    return draw(gen("channel_sum", name), (N, H, W, C_ + (8 if v else 0)), dt, 1.0, 0.25)


def cs_ref(row, xbuf, x16=False):
    """-> (float64 sums [N][nblocks][C], bound)"""
    name, dt, N, H, W, C_, nb, v = row
    x = xbuf[..., (8 if v else 0):]
    x = (x.half() if x16 else x).double().reshape(N, H * W, C_)
    per = -(-(H * W) // nb)
    ref, mag = torch.zeros(N, nb, C_, dtype=torch.float64), torch.zeros(N, nb, C_, dtype=torch.float64)
    for b in range(nb):
        blk = x[:, b * per:min((b + 1) * per, H * W)]
        ref[:, b], mag[:, b] = blk.sum(1), blk.abs().sum(1)
    lanes = cs_lanes(C_)
    return ref, (-(-per // lanes) + lanes) * EPS32 * mag


# ------------------------------------------------------------------------------------------------- avgpool_k
# (name, dtype, N, H, W, C, scale, x view).  nsplit = ceil(scale / 8) strips per cell: 2 -> 1, 8 -> 1, 11 -> 2 (a last strip of 3 rows),
# 17 -> 3 (a last strip of 1 row); floor pooling: rows and columns beyond (H // scale) * scale are not read
AK_CASES = [
    ("s2_c64", "f32", 2, 7, 9, 64, 2, False),
    ("s8_c8", "f32", 1, 19, 27, 8, 8, True),
    ("s11_c64", "f32", 1, 25, 36, 64, 11, False),
    ("s11_c64_view", "f32", 2, 12, 23, 64, 11, True),
    ("s17_c256", "f32", 1, 36, 19, 256, 17, True),
    ("s17_c8", "f32", 1, 17, 35, 8, 17, False),
    ("s2_c256_f16", "f16", 1, 5, 4, 256, 2, True),
    ("s8_c64_f16", "f16", 2, 9, 17, 64, 8, False),
    ("s11_c8_f16", "f16", 1, 23, 12, 8, 11, False),
    ("s17_c64_f16", "f16", 1, 18, 35, 64, 17, True),
]


def ak_class(row):
    _, dt, N, H, W, C_, s, v = row
    return cls_avgpool_k(dt, C_, s, not v)


def ak_data(row):
    name, dt, N, H, W, C_, s, v = row
    return draw(gen("avgpool_k", name), (N, H, W, C_ + (16 if v else 0)), dt, 1.0, 0.25)


def ak_ref(row, xbuf, x16=False):
    name, dt, N, H, W, C_, s, v = row
    x = xbuf[..., (16 if v else 0):]
    x = (x.half() if x16 else x).double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(x, s, s).permute(0, 2, 3, 1)
    mag = F.avg_pool2d(x.abs(), s, s).permute(0, 2, 3, 1)
    lanes, nsplit = cs_lanes(C_), -(-s // 8)
    return ref, (-(-8 * s // lanes) + lanes + nsplit + 1) * EPS32 * mag


# ------------------------------------------------------------------------------------------------- match_gather
# (name, (fin, fref, cat) dtypes, N, H, W, scale, fref view, cat view).  Blocks are 3 scale x 3 scale pixels; the block grid is that of
# F.fold(kernel = stride = padding = 3 scale): (H + ks) // ks + 1 rows, row and column 0 and the last lie (partly) outside the map
MG_CASES = [
    ("s11_f32", ("f32", "f32", "f32"), 1, 88, 120, 11, True, False),          # 88 = 2 * 33 + 22, 120 = 3 * 33 + 21: blocks overhang the frame
    ("s12_f32_f16out", ("f32", "f32", "f16"), 1, 100, 150, 12, False, True),   # 100 = 2 * 36 + 28, 150 = 4 * 36 + 6
    ("s1_f32", ("f32", "f32", "f32"), 2, 8, 8, 1, False, True),
    ("s1_f16", ("f16", "f16", "f16"), 2, 8, 8, 1, True, False),
    ("s11_f16", ("f16", "f16", "f16"), 1, 88, 120, 11, False, False),
    ("s1_f16in_f32out", ("f16", "f32", "f32"), 1, 8, 8, 1, False, False),
    ("s1_f16_f16_f32", ("f16", "f16", "f32"), 1, 8, 8, 1, True, True),            # the remaining dtype triples the launcher accepts
    ("s1_f32_f16_f16", ("f32", "f16", "f16"), 1, 8, 8, 1, False, True),
    ("s1_f32_f16_f32", ("f32", "f16", "f32"), 2, 8, 8, 1, True, False),
    ("s1_f16_f32_f16", ("f16", "f32", "f16"), 1, 8, 8, 1, False, False),
]


def mg_class(row):
    _, dts, _, _, _, _, vr, vc = row
    return cls_match_gather(dts, not (vr or vc))


def mg_grid(H, W, scale):
    ks = 3 * scale
    return ks, (H + ks) // ks + 1, (W + ks) // ks + 1


def mg_data(row):
    """-> (fin [N,H,W,64], fref buffer, idx [N, nbh * nbw] int32).  idx is a test input: a fixed permutation of the block grid per image,
    then hand-set entries: the first interior block reads border block 0 (entirely outside: zeros), the second the last block of the grid,
    the third the last block of row 1 (overhangs the right edge), the fourth itself"""
    name, dts, N, H, W, scale, vr, vc = row
    g = gen("match_gather", name)
    fin = draw(g, (N, H, W, 64), dts[0], 1.0, 0.5)
    fref = draw(g, (N, H, W, 64 + (8 if vr else 0)), dts[1], 1.0, -0.5)
    ks, nbh, nbw = mg_grid(H, W, scale)
    idx = torch.stack([torch.randperm(nbh * nbw, generator=g) for _ in range(N)]).to(torch.int32)
    idx[:, 1 * nbw + 1] = 0
    idx[:, 1 * nbw + 2] = nbh * nbw - 1
    idx[:, 2 * nbw + 1] = 1 * nbw + nbw - 1
    idx[:, 2 * nbw + 2] = 2 * nbw + 2
    return fin, fref, idx


def mg_ref(row, fin, frefbuf, idx, x16=False):
    """plain indexing of the kernel's rule (pointwise.hip match_gather_kernel): pixel (y, x) lies in block (y // ks + 1, x // ks + 1); its
    match m = idx[block] names the block whose pixel at the same offset is the source, zeros when that lies outside the map;
    cor = a.b / max(|a| |b|, 1e-8); cat = [a cor | b cor]  -> (ref [N,H,W,128], bound, number of pixels under the 1e-6 clamp guard,
    number of pixels whose source lies outside)"""
    name, dts, N, H, W, scale, vr, vc = row
    ks, nbh, nbw = mg_grid(H, W, scale)
    fref = frefbuf[..., (8 if vr else 0):]
    a = (fin.half() if x16 else fin).double()
    fr = (fref.half() if x16 else fref).double()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blk = (yy // ks + 1) * nbw + (xx // ks + 1)
    m = idx.long()[:, blk.reshape(-1)].reshape(N, H, W)
    sy, sx = (m // nbw - 1) * ks + yy % ks, (m % nbw - 1) * ks + xx % ks
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    n_ix = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    b = fr[n_ix, sy.clamp(0, H - 1), sx.clamp(0, W - 1)] * inside.unsqueeze(-1)
    na, nb_ = a.norm(dim=-1), b.norm(dim=-1)
    cor = (a * b).sum(-1) / (na * nb_).clamp_min(1e-8)
    ref = torch.cat([a * cor.unsqueeze(-1), b * cor.unsqueeze(-1)], -1)
    mag = torch.cat([a.abs(), b.abs()], -1)
    bound = 80 * EPS32 * mag + EPS32 * ref.abs() + ((EPS16 * ref.abs() + TINY16) if dts[2] == "f16" else 0.0)
    return ref, bound, int(((na * nb_) < 1e-6).sum()), int((~inside).sum())


def table_classes():
    """the call classes the tables of this module hold (bcast_add_act, upsample2x and spynet_level_input classes are built by the GPU
    module from tests/test_forward_ops_gpu.py's class functions on the real arguments; here from the rows, in the same form)"""
    out = {af_class(r) for r in AF_CASES} | {cc_class(r) for r in CC_CASES} | {cs_class(r) for r in CS_CASES} | {ak_class(r) for r in AK_CASES}
    out |= {mg_class(r) for r in MG_CASES}
    out |= {("bcast_add_act", "t4" if (T == 4 and xdt == bdt == "f16") else "generic", xdt, bdt) for (_, _, _, _, T, xdt, bdt, _) in BC_CASES}
    out |= {("upsample2x", "view" if (vi or vo) else "dense", xdt, ydt) for (_, _, _, _, xdt, ydt, vi, vo) in UP_CASES}
    out |= {("spynet_level_input", "vec" if Cs == 4 else "scalar", fl, "f32") for (_, _, _, fl, Cs, _) in SP_CASES}
    return out
