// conv_split -- conv_f32's contract (fp32 activations, fp32 weights, fp32-grade results: the fp32 islands of pnet.py:33,57) on the bf16
// matrix pipe, which is 16x faster than v_mfma_f32_32x32x2_f32.  Strictly opt-in (ops.f32_split / tdvc_conv2d_split): tdvc_conv2d never
// comes here.
//
// Arithmetic.  Every fp32 operand v is split into three bf16 values, each conversion round-to-nearest-even:
//     h = bf16(v),  m = bf16(v - h),  l = bf16((v - h) - m)
// Both subtractions are exact in fp32 (the file is built with -ffp-contract=off), and h + m + l == v exactly for every normal fp32 value
// (8 + 8 + 8 significand bits) whose bf16 rounding is finite; only the l part of values below about 2^-110 underflows.  The upper limit: a
// finite |v| above bf16's largest value rounded up (from about 3.39e38 to FLT_MAX) gives h = Inf, and an in-image Inf gives v - h = NaN:
// such operands produce NaN outputs where conv_f32 would produce Inf or a finite sum.  Nothing is clamped.  A MAC x * w is the sum of SIX products, each
// exact in the MFMA's fp32 product:  xh wh  +  xh wm + xm wh  +  xm wm + xh wl + xl wh.  The three dropped terms (xm wl, xl wm, xl wl) are
// bounded per product by (2 u^3 + u^4) |x| |w|, u = 2^-8: about 2 EPS32 |x| |w|, with no factor K.
// The weights are split once, by the packer; the activations in registers, after the border mask (a clamped border address that holds Inf
// or NaN contributes exact zeros) and after the GDN pool's fp32 square (one rounding, as conv_f32).
//
// Two accumulators per tile (2 x 2 tiles: 128 of the 256 registers a wave has at two waves per SIMD, __launch_bounds__(256, 2)).  xh wh goes to `acc`, the five small products (<= 2^-8 of it) to `lo`, which is added once at the end: a
// small product added to the large running sum would be rounded at the sum's ulp -- six roundings per MAC instead of conv_f32's one --
// while in a sum of its own it is rounded at 2^-8 of that.  The main accumulator then sees exactly conv_f32's number of roundings or fewer
// (the bf16 MFMA adds 16 products per instruction, the fp32 one 2).
//
// Same implicit GEMM, fragment order and tap walk as conv_f32: lane (r, hh) holds 8 consecutive input channels of one tap, which IS the
// A / B operand lane map of v_mfma_f32_32x32x16_bf16 -- one k-step of the fp16 layout is one MFMA per product, six per k-step (192 matrix
// cycles) where conv_f32 issues eight fp32 MFMAs (512).  Packing (tdvc_pack_conv_weights_indexed_bf16x3): [cout tile 32][k-step][plane
// h, m, l][lane 64][8 bf16], so every fragment load of a wave is one coalesced 1 KB line.
#include "conv_common.h"

using convk::ConvParams;

int conv_f32_validate(const tdvc_conv_desc* d, int& Ho, int& Wo);                                                            // conv_f32.hip
void conv_f32_params(const tdvc_conv_desc* d, int Ho, int Wo, ConvParams& p, int& cout_tiles, int& total_px);
void tdvc_set_last_conv_kernel(const char* name);                                                                            // conv_dispatch.hip

namespace {

struct SplitExtra {
  const float* x;          // fp32 activations (ConvParams::x is typed half_t*)
  const __bf16* w;         // the three-plane bf16 packing
  int ck8;                 // channel chunk / 8 of the packing
  int cout_tiles;          // 32-row tiles of the padded cout
  int total_px;
};

// split3(): common.h

// MT cout tiles x NT pixel groups of 32 per wave, as conv_f32_kernel; per k-step MT * 3 weight fragments and NT activation fragments
// feed 6 * MT * NT MFMAs
template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void conv_split_kernel(const ConvParams p, const SplitExtra e) {
  __shared__ int tdy[TDVC_MAX_TAPS], tdx[TDVC_MAX_TAPS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, r = lane & 31;
  if (tid < p.ntaps) { tdy[tid] = p.tap_dy[tid]; tdx[tid] = p.tap_dx[tid]; }
  __syncthreads();
  // workgroup = 2 pixel blocks (NT * 32 pixels each) x 2 cout blocks (MT tiles each): waves 0,1 share the pixels, 0,2 the weights
  const int ct0 = (blockIdx.y * 2 + (wave & 1)) * MT;
  if (ct0 >= e.cout_tiles) return;                      // wave-uniform; no barrier follows
  const int pb = blockIdx.x * 2 + (wave >> 1);

  const int hw = p.Ho * p.Wo;
  bool pv[NT];
  int pn[NT], poy[NT], pox[NT], iy0[NT], ix0[NT];
  const float* xn[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int px = (pb * NT + nt) * 32 + r;
    pv[nt] = px < e.total_px;
    const int pxc = pv[nt] ? px : 0;
    pn[nt] = pxc / hw;
    const int rem = pxc - pn[nt] * hw;
    poy[nt] = rem / p.Wo;
    pox[nt] = rem - poy[nt] * p.Wo;
    iy0[nt] = poy[nt] * p.in_stride - p.pad;
    ix0[nt] = pox[nt] * p.in_stride - p.pad;
    xn[nt] = e.x + (long)pn[nt] * p.x_sn;
  }
  if (!__builtin_amdgcn_readfirstlane(__ballot(pv[0]) != 0ull)) return;      // a pixel block past the end (wave-uniform)

  const int T = p.nchunks * p.steps;
  const int ck8 = e.ck8, CK = ck8 * 8, H2 = ck8 >> 1;
  const __bf16* wp = e.w + ((long)ct0 * T) * 1536 + lane * 8;      // tile ct0 + mt: + mt * T * 1536; plane pl of step g: + (g * 3 + pl) * 512

  f32x16 acc[MT][NT], lo[MT][NT];
  convk::zero_acc(acc);
  convk::zero_acc(lo);

  // conv_f32's software pipeline: the fragments of step g + 1 are ISSUED before the MFMAs of step g and consumed behind them; fetch() only
  // issues loads and derives the border mask, every use of a loaded register (mask, square, split) sits in mfmas(), and sched_barrier(0)
  // pins the order load / matrix / load / matrix.
  bf16x8 a[2][MT][3];
  f32x4 b[2][NT][2];
  unsigned bm[2][NT];
  auto fetch = [&](int g, bf16x8 (&af)[MT][3], f32x4 (&bf)[NT][2], unsigned (&mk)[NT]) {
    const int gc = min(g, T - 1);
    const int ch = gc / p.steps, s = gc - ch * p.steps;
    int tap, cofs;
    if (ck8 == 1) {
      tap = min(2 * s + hh, p.ntaps - 1);               // the padded half step carries zero weights
      cofs = ch * 8;
    } else {
      tap = s / H2;
      cofs = ch * CK + (s - tap * H2) * 16 + hh * 8;
    }
    const int dy = tdy[tap], dx = tdx[tap];
    const int cc = min(cofs, p.Cin - 8);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const __bf16* ap = wp + ((long)mt * T + gc) * 1536;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) af[mt][pl] = *reinterpret_cast<const bf16x8*>(ap + pl * 512);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int iy = iy0[nt] + dy, ix = ix0[nt] + dx;
      const bool ok = (int)pv[nt] & (int)(g < T) & (int)(iy >= 0) & (int)(iy < p.H) & (int)(ix >= 0) & (int)(ix < p.W) & (int)(cofs < p.Cin);   // no short-circuit branches
      const int iyc = min(max(iy, 0), p.H - 1), ixc = min(max(ix, 0), p.W - 1);
      const float* bp = xn[nt] + ((long)iyc * p.W + ixc) * p.x_sp + cc;
      bf[nt][0] = *reinterpret_cast<const f32x4*>(bp);
      bf[nt][1] = *reinterpret_cast<const f32x4*>(bp + 4);
      // out-of-image taps are zeroed by an OPAQUE bit mask (conv_f32: a select sank the loads behind branches, a multiply turns Inf at
      // a clamped border address into NaN), BEFORE the split: exact zeros in all three parts for any bit pattern
      unsigned m = ok ? 0xFFFFFFFFu : 0u;
      asm volatile("" : "+v"(m));
      mk[nt] = m;
    }
  };
  auto mfmas = [&](bf16x8 (&af)[MT][3], f32x4 (&bf)[NT][2], unsigned (&mk)[NT]) {
    bf16x8 xh[NT], xm[NT], xl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = __uint_as_float(__float_as_uint(bf[nt][j >> 2][j & 3]) & mk[nt]);
        if (p.square) v *= v;
        __bf16 h, m, l;
        split3(v, h, m, l);
        xh[nt][j] = h; xm[nt][j] = m; xl[nt][j] = l;
      }
    // the five small products, smallest first, into `lo`; product by product over the MT * NT tiles, so that consecutive MFMAs never
    // wait for each other's accumulator
#define TDVC_SPLIT_PRODUCT(ACC, WPL, XPART)                                                                                            \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                                                  \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                                                \
        ACC[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt][WPL], XPART[nt], ACC[mt][nt], 0, 0, 0);
    TDVC_SPLIT_PRODUCT(lo, 1, xm)
    TDVC_SPLIT_PRODUCT(lo, 2, xh)
    TDVC_SPLIT_PRODUCT(lo, 0, xl)
    TDVC_SPLIT_PRODUCT(lo, 1, xh)
    TDVC_SPLIT_PRODUCT(lo, 0, xm)
    TDVC_SPLIT_PRODUCT(acc, 0, xh)
#undef TDVC_SPLIT_PRODUCT
  };
  fetch(0, a[0], b[0], bm[0]);
  for (int g = 0; g < T; g += 2) {
    fetch(g + 1, a[1], b[1], bm[1]);                    // g + 1 == T: a zeroed activation fragment (mask 0), harmless
    __builtin_amdgcn_sched_barrier(0);
    mfmas(a[0], b[0], bm[0]);
    __builtin_amdgcn_sched_barrier(0);
    fetch(g + 2, a[0], b[0], bm[0]);                    // unconditional (past the end: clamped addresses, mask 0): a load under a
    __builtin_amdgcn_sched_barrier(0);                  // branch makes hipcc drain vmcnt(0) at the join
    mfmas(a[1], b[1], bm[1]);                           // g + 1 == T (odd T): adds exact zeros
    __builtin_amdgcn_sched_barrier(0);
  }

#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (!pv[nt]) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][4 * g + i] + lo[mt][nt][4 * g + i];
        convk::epilogue4<true>(p, pn[nt], poy[nt], pox[nt], (ct0 + mt) * 32 + 8 * g + 4 * hh, v);
      }
  }
}

// one thread per item of tdvc_pack_conv_weights_indexed_f32 (8 values of one lane): gathered as there, split, written as three 16-byte
// fragments at [tile][k-step][plane][lane]
__global__ void pack_indexed_bf16x3_kernel(const float* __restrict__ w, const int* __restrict__ row_off, const int* __restrict__ chan_off,
                                           const int* __restrict__ tap_off, const unsigned char* __restrict__ row_mask,
                                           const unsigned char* __restrict__ chan_mask, const unsigned char* __restrict__ tap_mask,
                                           int cout, int cin, int ntaps, int ck, int nchunks, int steps, long total, __bf16* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63);
  long q = e >> 6;
  const int s = (int)(q % steps); q /= steps;
  const int ch = (int)(q % nchunks);
  const int t = (int)(q / nchunks);
  const int ck8 = ck >> 3;
  const int r = lane & 31, h = lane >> 5;
  const int co = t * 32 + r, kc = 2 * s + h;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (kc < ntaps * ck8 && co < cout) {
    const int tap = kc / ck8, c8 = kc - tap * ck8;
    const int ro = row_off[co], to = tap_off[tap];
    const unsigned tm = tap_mask[tap];
    if (ro >= 0 && (tm & row_mask[co]) == 0u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = ch * ck + c8 * 8 + j;
        if (ci < cin) {
          const int cof = chan_off[ci];
          if (cof >= 0 && (tm & chan_mask[ci]) == 0u) o[j] = w[(long)ro + cof + to];
        }
      }
    }
  }
  bf16x8 ph, pm, pl;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 hj, mj, lj;
    split3(o[j], hj, mj, lj);
    ph[j] = hj; pm[j] = mj; pl[j] = lj;
  }
  bf16x8* dst = reinterpret_cast<bf16x8*>(out) + (e >> 6) * 192 + lane;
  dst[0] = ph; dst[64] = pm; dst[128] = pl;
}

}  // namespace

extern "C" int tdvc_pack_conv_weights_indexed_bf16x3(const float* w, const int32_t* row_off, const int32_t* chan_off, const int32_t* tap_off,
                                                     const uint8_t* row_mask, const uint8_t* chan_mask, const uint8_t* tap_mask,
                                                     int cout, int cin, int ntaps, int ck, void* dst, void* stream) {
  TDVC_CHECK(w && row_off && chan_off && tap_off && row_mask && chan_mask && tap_mask && dst && aligned16(dst),
             "tdvc_pack_conv_weights_indexed_bf16x3: null / unaligned pointer");
  const int64_t bytes16 = tdvc_conv_packed_bytes(cout, cin, ntaps, ck);          // the fp16 blob: 16 bytes per item, here 3 x 16
  TDVC_CHECK(bytes16 > 0, "tdvc_pack_conv_weights_indexed_bf16x3: bad geometry");
  const int ck8 = ck / 8, nchunks = (cin + ck - 1) / ck, steps = (ntaps * ck8 + 1) / 2;
  const long total = bytes16 / 16;
  hipLaunchKernelGGL(pack_indexed_bf16x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     w, row_off, chan_off, tap_off, row_mask, chan_mask, tap_mask, cout, cin, ntaps, ck, nchunks, steps, total,
                     reinterpret_cast<__bf16*>(dst));
  return tdvc_launch_status("tdvc_pack_conv_weights_indexed_bf16x3");
}

// conv_f32's contract and validation (its messages name tdvc_conv2d_f32); `d->w` is the three-plane bf16 packing
extern "C" int tdvc_conv2d_split(const tdvc_conv_desc* d, void* stream) {
  int Ho, Wo;
  if (const int rc = conv_f32_validate(d, Ho, Wo)) return rc;
  TDVC_CHECK(!d->chan_sum && !d->flow.p, "tdvc_conv2d_split: chan_sum / flow are not available on the fp32 path");

  ConvParams p;
  SplitExtra e;
  conv_f32_params(d, Ho, Wo, p, e.cout_tiles, e.total_px);
  e.x = reinterpret_cast<const float*>(d->x.p);
  e.w = reinterpret_cast<const __bf16*>(d->w);
  e.ck8 = d->ck / 8;
  tdvc_set_last_conv_kernel("conv_split");
  // conv_f32's launch rule: workgroup = 2 x (NT * 32) pixels by 2 x MT cout tiles; small maps keep NT = 1 so that the few pixels still
  // spread over the CUs
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool big = e.total_px >= 16384;
  if (e.cout_tiles == 1) {
    if (big) hipLaunchKernelGGL((conv_split_kernel<1, 2>), dim3((unsigned)((e.total_px + 127) / 128), 1), dim3(256), 0, st, p, e);
    else hipLaunchKernelGGL((conv_split_kernel<1, 1>), dim3((unsigned)((e.total_px + 63) / 64), 1), dim3(256), 0, st, p, e);
  } else {
    const unsigned gy = (unsigned)((e.cout_tiles + 3) / 4);
    if (big) hipLaunchKernelGGL((conv_split_kernel<2, 2>), dim3((unsigned)((e.total_px + 127) / 128), gy), dim3(256), 0, st, p, e);
    else hipLaunchKernelGGL((conv_split_kernel<2, 1>), dim3((unsigned)((e.total_px + 63) / 64), gy), dim3(256), 0, st, p, e);
  }
  return tdvc_launch_status("tdvc_conv2d_split");
}
