// conv_mfma_v7 — the dominant layer class of the TDVC path: 3x3, stride 1, pad 1, Cin in {32, 64},
// Cout >= 64 (the 64->64 / 64->216 convs), transposed fp16 epilogue.
//
// In-kernel stamps of its register-staged predecessor showed the stage time is set inside
// the CU, not by HBM: staging the tile global -> VGPR -> ds_write costs two barriers per stage, a publish
// pass, address arithmetic per load, and the compiler drains every outstanding load (vmcnt(0)) around
// it.  v7 removes the staging: tiles arrive by LDS-DMA through the shared halo-tile pipeline (conv_dma.h;
// DESIGN.md, "The shared halo-tile pipeline") with 8 loader waves and the weight-stationary LDS map.
// What is v7's own:
//   * one persistent 8-wave workgroup per CU; a wave computes 64 couts x (2 rows x 32 px); accumulators
//     initialised from the bias, fragment reads software-pipelined one half tap ahead;
//   * one barrier per stage + one per tile (the finished tile buffer becomes the epilogue scratch);
//   * the only compiler-tracked vector-memory operations in the loop are the epilogue's residual / GDN
//     loads and its stores, which are younger than the DMA they follow, so the compiler's own counted
//     waits stay valid.  The top-of-stage wait allows exactly the epilogue's 8 stores to stay in flight
//     (full tiles) or drains.
#include <type_traits>

#include "conv_dma.h"

using convk::ConvParams;
using convk::HaloExtra;
using convk::raw_barrier;
using convk::wslice_off;

namespace {

constexpr int TH7 = convk::HALO_TH, TW7 = convk::HALO_TW, TIW7 = convk::HALO_IW, NT7 = 2, NTHR7 = 512;
using Dma7 = convk::HaloDma<8, true, false>;
constexpr int DMA7 = Dma7::SLOTS;                                    // 5 per wave
constexpr int BUF1 = convk::WS_BUF1, WLO7 = convk::WS_WLO, MISC7 = convk::WS_MISC, LDS7 = convk::WS_LDS, WSL7 = convk::WS_WSL;
static_assert(8 * 32 * 144 <= WLO7, "epilogue scratch aliases a tile buffer");

static long long* g_stamp7 = nullptr;
static int g_stamp7_cap = 0;

template <bool STAMP = false>
__global__ __launch_bounds__(NTHR7, 1) void conv_mfma_v7_kernel(const ConvParams p, const HaloExtra e, long long* stamps = nullptr, int stamp_cap = 0) {
  long long stv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define ST7(i) do { if constexpr (STAMP) { if (S == 3) stv[i] = clock64(); } } while (0)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  float* bias_s = reinterpret_cast<float*>(smem + MISC7);   // 64 floats
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(smem));   // LDS byte address of the array (low 32 bits of the flat address)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, r = lane & 31;
  const int cb = blockIdx.y, n = blockIdx.z;
  const int nchunks = p.nchunks;

  int first, stride, my_tiles;                             // XCD-aware: one contiguous band of tiles per L2
  convk::xcd_tile_walk(e.ntiles, first, stride, my_tiles);
  const int nstages = my_tiles * nchunks;
  if (nstages <= 0) return;

  Dma7 dma;
  dma.init(p, e.zeros, n, wave, lane);
  auto issue_prep = [&](int S) {
    const int tile_i = S / nchunks, ch = S - tile_i * nchunks;
    const int tile = convk::walk_tile(p, e.ntiles, first, stride, tile_i);
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    dma.prep(p, ty, tx, ch);
  };

  // ---- prologue: first tile's DMA, then bias + resident weights (compiler-tracked loads, younger than the DMA)
  issue_prep(0);
#pragma unroll
  for (int j = 0; j < DMA7; ++j) dma.issue(p, j, lds0);

  convk::ws_load_bias_weights<NTHR7>(p, smem, cb, nchunks, tid);

  // ---- B-fragment read offsets (tile buffer 0, s2 = 0): pixel q = (2*wave + nt + dy) * 34 + r + dx, chunk hh
  int bq[NT7][9];
#pragma unroll
  for (int nt = 0; nt < NT7; ++nt)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int q = (wave * NT7 + nt + t / 3) * TIW7 + r + (t % 3);
      bq[nt][t] = convk::halo_frag_off(q, hh, 0);
    }

  __syncthreads();                       // bias and weights are visible (no DMA-aware wait here: see top of stage)

  f32x16 acc[2][NT7];
  auto init_acc = [&]() {                // accumulators start from the bias: LDS reads, no vector moves
#pragma unroll
    for (int nt = 0; nt < NT7; ++nt) {
      int o = hh * 4;
      asm volatile("" : "+v"(o));        // keep one read per accumulator (no register copies)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_s + mt * 32 + 8 * g + o);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[mt][nt][4 * g + i] = b4[i];
        }
    }
  };
  init_acc();

  bool stores_in_flight = false;         // the previous stage ended with exactly 8 epilogue stores (full tile)
  for (int S = 0; S < nstages; ++S) {
    const int tile_i = S / nchunks, ch = S - tile_i * nchunks;
    const unsigned bsel = (S & 1) ? BUF1 : 0;
    ST7(0);
    // This wave's DMA pieces of stage S have landed: they are older than the (at most 8) epilogue stores.
    if (stores_in_flight) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ST7(1);
    raw_barrier();                       // every wave's pieces landed; every wave is done with the other buffer
    ST7(2);
    const bool have_next = S + 1 < nstages;
    if (have_next) issue_prep(S + 1);
    const unsigned nbuf = lds0 + (bsel ^ BUF1);

    // matrix phase: 18 half taps, fragments double-buffered; one DMA piece of the next stage after each of
    // the first DMA7 half taps
    const unsigned char* tb = smem + bsel;
    const unsigned char* wlo = smem + (ch == 0 ? WLO7 : wslice_off(9) - 0 * WSL7) + lane * 16;              // taps 0..5 of this chunk
    const unsigned char* whi = smem + (ch == 0 ? wslice_off(6) - 6 * WSL7 : wslice_off(9)) + lane * 16;     // taps 6..8
    half8 fa[2][2], fb[2][NT7];
    auto frag = [&](int i, int buf) {
      const int t = i >> 1, s2 = i & 1;
      const unsigned char* wt = (t < 6 ? wlo : whi) + t * WSL7;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) fa[buf][mt] = *reinterpret_cast<const half8*>(wt + (mt * 2 + s2) * 1024);
#pragma unroll
      for (int nt = 0; nt < NT7; ++nt) fb[buf][nt] = *reinterpret_cast<const half8*>(tb + (bq[nt][t] ^ (s2 * 32)));
    };
    frag(0, 0);
#pragma unroll
    for (int i = 0; i < 18; ++i) {
      if (i + 1 < 18) frag(i + 1, (i + 1) & 1);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT7; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i & 1][mt], fb[i & 1][nt], acc[mt][nt], 0, 0, 0);
      // pin the software pipeline: all four fragment reads of half tap i+1 are issued BEFORE the four MFMAs
      // of half tap i (left alone, hipcc sinks them behind the second MFMA and the next group stalls on them)
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      if (i < DMA7 && have_next) dma.issue(p, i, nbuf);
    }
    ST7(3);
    stores_in_flight = false;
    if (ch != nchunks - 1) continue;

    const int tile = convk::walk_tile(p, e.ntiles, first, stride, tile_i);
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const bool full = (ty + 1) * TH7 <= p.Ho && (tx + 1) * TW7 <= p.Wo;
    raw_barrier();                       // all waves finished reading this tile buffer: it becomes epilogue scratch
    ST7(4);
    convk::epilogue_simple_rows<NT7, true, 1>(p, acc, bias_s, smem + bsel + wave * (32 * 144), n, cb * 64,
                                           ty * TH7 + wave * NT7, tx * TW7, lane, false, full);
    init_acc();
    stores_in_flight = full;
    ST7(5);
    if constexpr (STAMP) {
      if (S == 3 && lane == 0) {             // one record per wave: [block][wave][8 stamps]
        const int bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        if (bid * 8 + 7 < stamp_cap) for (int i = 0; i < 8; ++i) stamps[((long)bid * 8 + wave) * 8 + i] = stv[i];
      }
    }
  }
}

}  // namespace

extern "C" void tdvc_debug_set_stamp_buffer_v7(void* buf, int cap_blocks) { g_stamp7 = (long long*)buf; g_stamp7_cap = cap_blocks; }

bool conv_v7_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo) {
  // the counted vmcnt(8) of a full tile assumes every wave stored; a wave covers the 64 packed rows of its cout block (sub-pixel
  // store: inside one sub-pixel, cq % 64 == 0 by conv_is_simple)
  return convk::taps_dense(d, 3, 3, 1) && convk::all_waves_store(d, 64) && d->ck == 32 && d->stride == 1 && d->cout >= 64 &&
         (d->x.C == 32 || d->x.C == 64) && !d->s2d && !d->square_input && (long)Ho * Wo >= convk::LARGE_MAP_PIXELS && convk::conv_is_simple(p);
}

int launch_conv_v7(const ConvParams& p, int cout_blocks, int N, hipStream_t st) {
  ConvParams q;
  HaloExtra e;
  dim3 grid;
  if (const int rc = convk::halo_launch_setup(p, cout_blocks, N, q, e, grid)) return rc;
  const auto go = g_stamp7 ? convk::launch_big_lds<&conv_mfma_v7_kernel<true>, ConvParams, HaloExtra, long long*, int>
                           : convk::launch_big_lds<&conv_mfma_v7_kernel<false>, ConvParams, HaloExtra, long long*, int>;
  return go("tdvc_conv2d(v7)", 160 * 1024, grid, dim3(NTHR7), LDS7, st, q, e, g_stamp7, g_stamp7 ? g_stamp7_cap : 0);
}
