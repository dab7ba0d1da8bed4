// conv_mfma_v5 — barrier-free, weight-stationary 1x1 conv (stride 1, Cin <= ~1000, Cout >= 64): the
// multi-frame fusion conv (256 -> 64), the GDN / inverse-GDN norm pools (128 -> 128 with the squared
// -input prologue), OffsetGen's 1x1 fusions.
//
// A 1x1 conv has no halo and no reuse between pixels: under the workgroup-tiled kernels a stage is one
// tap = 8 MFMAs per wave between two barriers, i.e. barrier-bound (the shared-tile weight-stationary kernel
// this replaced: 491 us for 256 -> 64 at 1080p = 2.7 TB/s algorithmic).  Here every wave owns a PRIVATE 2x32-pixel tile in LDS (5 KB) next to the
// resident weights, so after the one-time weight load there is NO barrier: waves drift apart and one
// wave's publish / epilogue / stores overlap its SIMD partner's MFMAs.  Measured 296 us = 4.5 TB/s
// algorithmic (0.57 of HBM peak) for the same layer.
// (The same scheme was tried for 3x3 windows — each wave loading its own 4-row halo — and measured 20 %
// SLOWER than a shared tile, so v5 only takes 1x1; 3x3 is conv_mfma_v7.)
// A 1x1 window makes the staging geometry a constant: the wave's tile is 2 x 32 pixels x 4 chunks of 16 bytes = 256 items,
// four per lane; item j * 64 + lane is chunk idx & 3 of pixel idx >> 2, and every tap reads the tile at offset 0 (a descriptor
// may still list (0, 0) more than once: one weight slice per listed tap).
#include <type_traits>

#include "conv_common.h"

using convk::ConvParams;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int WR = 2, TW5 = 32, CK5 = 32, PS5 = 80, NTHR5 = 512, NWAVE = 8;
constexpr int WSL5 = 4096;
constexpr int TL = WR * TW5 * 4 / 64;        // 16-byte loads per lane per stage
constexpr int WTILE5 = WR * TW5 * PS5;       // private LDS bytes per wave; also the epilogue's transpose scratch
static_assert(WTILE5 >= 32 * 144, "the wave's tile doubles as the 32 x 144 B transpose scratch");

// nbtiles: workgroup tiles (16 x 32 output pixels = 8 wave tiles)
template <int SIMPLE>      // 0: per-register epilogue4, 1: transposed generic, 2: transposed lean, 4: lean + broadcast add, 5: lean + flow add
__global__ __launch_bounds__(NTHR5, 1) void conv_mfma_v5_kernel(const ConvParams p, const int nbtiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* bias_s = reinterpret_cast<float*>(smem + 256);               // (the first 256 bytes held tap offsets: all zero for 1x1; the map stays)
  unsigned char* wlds = smem + 512;                                   // nchunks x ntaps x 4 KB, shared, read-only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned char* tbuf = wlds + p.nchunks * p.ntaps * WSL5 + wave * WTILE5;   // this wave's private tile

  const int hh = lane >> 5, r = lane & 31;
  const int cb = blockIdx.y, n = blockIdx.z;
  const int ntaps = p.ntaps, nchunks = p.nchunks;

  const int first = blockIdx.x, stride = gridDim.x;
  const int my_tiles = (nbtiles - first + stride - 1) / stride;
  const int nstages = my_tiles * nchunks;
  if (nstages <= 0) return;

  if (tid < 64) bias_s[tid] = p.bias ? p.bias[blockIdx.y * 64 + tid] : 0.f;
  {
    const int nslices = nchunks * ntaps;
    for (int i = tid; i < nslices * 256; i += NTHR5) {
      const int sl = i >> 8, u = i & 255;            // u = q*64 + lane, q = mt*2 + s2
      const int qq = u >> 6, ln = u & 63;
      const half_t* src = p.w + ((((long)(cb * 2 + (qq >> 1)) * nchunks * ntaps + sl) * 2 + (qq & 1)) * 64 + ln) * 8;
      *reinterpret_cast<half8*>(wlds + sl * WSL5 + u * 16) = *reinterpret_cast<const half8*>(src);
    }
  }
  __syncthreads();          // the only barrier: weights and bias are visible

  const int c8off = (lane & 3) * 8;            // item idx = j * 64 + lane: chunk idx & 3 (= lane & 3) of pixel idx >> 2 of the 2 x 32 tile
  const half_t* xn = p.x + (long)n * p.x_sn;

  u32x4 treg[2][TL];
  unsigned okmask[2] = {0u, 0u};
  auto issue = [&](auto setc, int S) {
    constexpr int SET = decltype(setc)::value;
    const int tile_i = S / nchunks, ch = S - tile_i * nchunks;
    const int tile = convk::walk_tile(p, nbtiles, first, stride, tile_i);
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int iy0 = ty * (WR * NWAVE) + wave * WR - p.pad, ix0 = tx * TW5 - p.pad;
    const int cg = ch * CK5 + c8off;
    const bool cok = cg < p.Cin;
    const int cgc = cok ? cg : 0;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < TL; ++j) {
      const int pix = (j * 64 + lane) >> 2;
      const int iy = (iy0 + pix / TW5) * p.in_stride, ix = (ix0 + pix % TW5) * p.in_stride;    // in_stride > 1 only with pad 0
      const bool ok = cok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const int iyc = min(max(iy, 0), p.H - 1), ixc = min(max(ix, 0), p.W - 1);
      const half_t* src = xn + ((long)iyc * p.W + ixc) * p.x_sp + cgc;
      treg[SET][j] = *reinterpret_cast<const u32x4*>(src);
      m |= (ok ? 1u : 0u) << j;
    }
    okmask[SET] = m;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  int base[WR];
#pragma unroll
  for (int nt = 0; nt < WR; ++nt) base[nt] = (nt * TW5 + r) * PS5 + hh * 16;

  f32x16 acc[2][WR];
  convk::zero_acc(acc);

  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // tdvc_conv_desc::chan_sum: this lane's channels 8 (lane & 7) .. + 8 over the pixels it stored
  issue(I0{}, 0);
  if (nstages > 1) issue(I1{}, 1);

  auto stage = [&](auto setc, int S) {
    constexpr int SET = decltype(setc)::value;
    const int tile_i = S / nchunks, ch = S - tile_i * nchunks;
    // publish: wave-private tile, in-order LDS within the wave -> no barrier
#pragma unroll
    for (int j = 0; j < TL; ++j) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      u32x4 val = ((okmask[SET] >> j) & 1u) ? treg[SET][j] : z;
      if (p.square) {
        half8 hv = __builtin_bit_cast(half8, val);
        hv = hv * hv;
        val = __builtin_bit_cast(u32x4, hv);
      }
      const int idx = j * 64 + lane;
      *reinterpret_cast<u32x4*>(tbuf + (idx >> 2) * PS5 + (idx & 3) * 16) = val;
    }

    const unsigned char* wch = wlds + ch * ntaps * WSL5 + lane * 16;
    for (int t = 0; t < ntaps; ++t) convk::mma_tap(acc, wch + t * WSL5, tbuf, base, 0);

    if (ch == nchunks - 1) {
      const int tile = convk::walk_tile(p, nbtiles, first, stride, tile_i);
      const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
      const int oy0 = ty * (WR * NWAVE) + wave * WR;
      if constexpr (SIMPLE == 4) {
        // lean + broadcast-add over the four slices at y (tdvc_conv_desc::bcast_T): the wave overwrites exactly the pixels whose
        // input channels it has finished reading (1x1: no halo; the prefetched stages belong to other pixels)
        convk::epilogue_lean_seq<WR, false, true>(p, acc, bias_s, tbuf, n, cb * 64, oy0, tx * TW5, lane, true, false);
      } else if constexpr (SIMPLE == 5) {
        // lean + the flow added to the rounded output (tdvc_conv_desc::flow)
        convk::epilogue_lean_seq<WR, false, false, false, true>(p, acc, bias_s, tbuf, n, cb * 64, oy0, tx * TW5, lane, true, false);
      } else if constexpr (SIMPLE) {
        // the private tile doubles as the transpose scratch (this wave's reads of it are complete:
        // every fragment read was waited for before its MFMA)
        if (SIMPLE == 2 && p.csum) convk::epilogue_lean_seq<WR, false, false, true>(p, acc, bias_s, tbuf, n, cb * 64, oy0, tx * TW5, lane, true, false, cs);
        else convk::epilogue_simple_rows<WR, false, SIMPLE>(p, acc, bias_s, tbuf, n, cb * 64, oy0, tx * TW5, lane, true);
      } else {
        convk::epilogue_regs(p, acc, n, oy0, tx * TW5 + r, cb * 2, hh);
        convk::zero_acc(acc);               // the next tile accumulates into the same registers
      }
    }
    if (S + 2 < nstages) issue(setc, S + 2);          // last vector-memory work of the stage
  };
  for (int S = 0; S < nstages; S += 2) {
    stage(I0{}, S);
    if (S + 1 < nstages) stage(I1{}, S + 1);
  }
  if (SIMPLE == 2 && p.csum) {
    // the eight lanes with the same lane & 7 hold the same channels: fixed-order butterfly, then one row per (workgroup, wave)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cs[j] += __shfl_xor(cs[j], 8);
      cs[j] += __shfl_xor(cs[j], 16);
      cs[j] += __shfl_xor(cs[j], 32);
    }
    if (lane < 8) {
      float* o = p.csum + (((long)n * gridDim.x + blockIdx.x) * NWAVE + wave) * 64 + lane * 8;
      *reinterpret_cast<f32x4*>(o) = f32x4{cs[0], cs[1], cs[2], cs[3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
    }
  }
}

inline int v5_lds_bytes(int ntaps, int nchunks) { return 512 + nchunks * ntaps * WSL5 + NWAVE * WTILE5; }

template <int SIMPLE>
constexpr auto launch_v5 = convk::launch_big_lds<&conv_mfma_v5_kernel<SIMPLE>, ConvParams, int>;

}  // namespace

bool conv_v5_eligible(const tdvc_conv_desc* d, int Ho, int Wo) {
  const int nchunks = (d->x.C + CK5 - 1) / CK5;
  const bool stride_ok = d->stride == 1 || (d->stride == 2 && d->pad == 0);   // ResidualBlockWithStride skips
  return d->ck == 32 && stride_ok && d->ntaps >= 1 && d->ntaps <= 9 && d->kh == 1 && d->kw == 1 && d->cout >= 64 &&
         d->x.C >= 32 && !d->s2d && ((long)Ho * Wo >= convk::LARGE_MAP_PIXELS || d->stride == 2) &&     // stride 2: the only ck = 32 kernel that takes it
         v5_lds_bytes(d->ntaps, nchunks) <= 160 * 1024;
}

// workgroups along x for a launch over `nbtiles` tiles (also the row count of tdvc_conv_desc::chan_sum: 8 waves per workgroup)
static int v5_grid_x(int nbtiles, int cout_blocks, int N) { return convk::persistent_grid_x(256, cout_blocks, N, nbtiles); }
int conv_v5_chan_sum_rows(int Ho, int Wo, int cout_blocks, int N) {
  const int nbtiles = ((Wo + TW5 - 1) / TW5) * ((Ho + WR * NWAVE - 1) / (WR * NWAVE));
  return v5_grid_x(nbtiles, cout_blocks, N) * NWAVE;
}

int launch_conv_v5(const ConvParams& p, int cout_blocks, int N, hipStream_t st) {
  ConvParams q = p;
  q.tiles_x = (p.Wo + TW5 - 1) / TW5;
  const int tiles_y = (p.Ho + WR * NWAVE - 1) / (WR * NWAVE);
  const int nbtiles = q.tiles_x * tiles_y;
  dim3 grid(v5_grid_x(nbtiles, cout_blocks, N), cout_blocks, N);
  if (p.flow.p && !(p.simple == 2 && !p.bcast_T && !p.csum)) {      // the dispatch (conv_flow_ok, conv_dispatch.hip) never sends such a launch here
    tdvc_set_error("conv v5: flow needs the lean epilogue without channel sums");
    return TDVC_EINVAL;
  }
  const auto go = p.bcast_T ? launch_v5<4> : (p.flow.p ? launch_v5<5> : convk::by_form(p.simple, launch_v5<0>, launch_v5<1>, launch_v5<2>));
  return go("tdvc_conv2d(v5)", 160 * 1024, grid, dim3(NTHR5), v5_lds_bytes(p.ntaps, p.nchunks), st, q, nbtiles);
}
