// The LDS-DMA halo-tile stage pipeline shared by conv_mfma_v7, v10 and v11 ("The shared halo-tile pipeline"), and the
// LDS-DMA instruction + raw barrier that conv_row and conv_pair use as well.  The layout invariants between the DMA (producer) and
// the B-fragment reads (consumer) are static_asserts at the end of the geometry section: they are evaluated at every build.
#pragma once
#include "conv_common.h"

namespace convk {

// One LDS-DMA piece: 64 lanes x 16 B from per-lane global addresses to LDS bytes [lds_dst + 16 * lane, + 16).  Issued from inline
// asm: the compiler neither counts nor drains it (the kernels' own s_waitcnt vmcnt retire it).
__device__ __forceinline__ void glds16(const half_t* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// drain this wave's LDS operations, then barrier unless `skip` (wave-uniform)
__device__ __forceinline__ void raw_barrier(bool skip = false) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (!skip) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- halo-tile geometry: a 16x32-pixel output tile of a 3x3 conv reads 18x34 input pixels, 32 channels (64 B) per stage -------
constexpr int HALO_TH = 16, HALO_TW = 32, HALO_CK = 32;
constexpr int HALO_IH = HALO_TH + 2, HALO_IW = HALO_TW + 2, HALO_NPIX = HALO_IH * HALO_IW;   // 612 halo pixels
constexpr int HALO_PX_BYTES = HALO_CK * 2;                                                   // 64 B per pixel per chunk: four 16-byte slots
constexpr int HALO_PIECE_BYTES = 1024, HALO_PIECE_PX = HALO_PIECE_BYTES / HALO_PX_BYTES;     // one DMA piece = 16 pixels
constexpr int HALO_PIECES = (HALO_NPIX + HALO_PIECE_PX - 1) / HALO_PIECE_PX;                 // 39 pieces hold pixels
constexpr int HALO_IMAGE_BYTES = HALO_PIECES * HALO_PIECE_BYTES;
constexpr int halo_slots(int nw) { return (HALO_PIECES + nw - 1) / nw; }                     // DMA slots per wave with nw loader waves

// Slot j of loader wave w is piece u = j * nw + w, which lands at LDS bytes [u * 1024, + 1024) of the tile image; lane l of the
// piece moves physical 16-byte slot (l & 3) of halo pixel 16 u + (l >> 2).
constexpr __host__ __device__ int halo_piece(int nw, int j, int w) { return j * nw + w; }
constexpr __host__ __device__ int halo_piece_pixel(int u, int lane) { return HALO_PIECE_PX * u + (lane >> 2); }

// The XOR swizzle that removes the bank conflicts of the B-fragment reads: the physical 16-byte slot in which the DMA places
// logical chunk c (channels 8c .. 8c + 7 of the stage) of halo pixel q.  An involution: physical slot s holds chunk
// halo_swz_slot(q, s), which is how the DMA applies it -- on its SOURCE address.
constexpr __host__ __device__ int halo_swz_slot(int q, int c) { return c ^ ((q >> 2) & 3); }
// byte offset in the tile image of B fragment (pixel q, lane half hh, k-half s2) = logical chunk 2 * s2 + hh.  The kernels keep
// the s2 = 0 offsets in registers and read the other half at `^ (s2 * 32)`.
constexpr __host__ __device__ int halo_frag_off(int q, int hh, int s2) { return q * HALO_PX_BYTES + (halo_swz_slot(q, 2 * s2 + hh) << 4); }

namespace halo_check {
// (a) over all (slot, wave, lane) every (halo pixel, 16-byte slot) is written exactly once, lane-linear: piece u at u * 1024 + lane * 16
constexpr bool dma_covers_once(int nw) {
  int cnt[HALO_NPIX * 4] = {};
  for (int j = 0; j < halo_slots(nw); ++j)
    for (int w = 0; w < nw; ++w)
      for (int lane = 0; lane < 64; ++lane) {
        const int u = halo_piece(nw, j, w), q = halo_piece_pixel(u, lane);
        if (u * HALO_PIECE_BYTES + lane * 16 != q * HALO_PX_BYTES + (lane & 3) * 16) return false;
        if (q < HALO_NPIX) ++cnt[q * 4 + (lane & 3)];
        else if (u < HALO_PIECES - 1) return false;           // only the last piece(s) may run past the image
      }
  for (int i = 0; i < HALO_NPIX * 4; ++i)
    if (cnt[i] != 1) return false;
  return true;
}
// (b) a fragment is read from where the DMA put its logical chunk, and the other k-half is the s2 = 0 offset ^ 32
constexpr bool reads_match_dma() {
  for (int q = 0; q < HALO_NPIX; ++q)
    for (int hh = 0; hh < 2; ++hh)
      for (int s2 = 0; s2 < 2; ++s2) {
        int at = -1;
        for (int s = 0; s < 4; ++s)                            // physical slot s of pixel q carries chunk halo_swz_slot(q, s)
          if (halo_swz_slot(q, s) == 2 * s2 + hh) at = q * HALO_PX_BYTES + s * 16;
        if (halo_frag_off(q, hh, s2) != at || halo_frag_off(q, hh, s2) != (halo_frag_off(q, hh, 0) ^ (s2 * 32))) return false;
      }
  return true;
}
// the chunk a lane carries does not depend on the piece: (q >> 2) & 3 == (lane >> 4) & 3 for q = 16 u + (lane >> 2)
constexpr bool lane_chunk_is_piece_free() {
  for (int u = 0; u < HALO_PIECES + 1; ++u)
    for (int lane = 0; lane < 64; ++lane)
      if (halo_swz_slot(halo_piece_pixel(u, lane), lane & 3) != halo_swz_slot(lane >> 2, lane & 3)) return false;
  return true;
}
}  // namespace halo_check
static_assert(halo_check::dma_covers_once(4) && halo_check::dma_covers_once(8), "every halo pixel slot is written exactly once");
static_assert(halo_check::reads_match_dma(), "B-fragment read offsets match the DMA swizzle");
static_assert(halo_check::lane_chunk_is_piece_free(), "per-lane chunk");

// ---- the halo-tile loader of NW loader waves.  CACHE_OFFSETS: the per-slot element offsets of interior tiles stay in registers
// (v7, v10) or are recomputed per slot (v11: ten of them spilled its 256-VGPR budget).  SKIP_EMPTY_PIECE: piece 39, which holds no
// pixel, is not issued (v11) or is (v7, v10: every wave issues the same number of pieces).  The two flags keep each kernel's DMA
// count and register budget where they were measured.
template <int NW, bool CACHE_OFFSETS, bool SKIP_EMPTY_PIECE>
struct HaloDma {
  static constexpr int SLOTS = halo_slots(NW);
  static constexpr int IMAGE_BYTES = SKIP_EMPTY_PIECE ? HALO_IMAGE_BYTES : SLOTS * NW * HALO_PIECE_BYTES;   // LDS bytes written per stage

  int wave, lane;                 // loader wave 0 .. NW - 1 (wave-uniform), lane of the wave
  int q0;                         // pixel(0)
  int csw;                        // logical chunk this lane moves
  int xrow;                       // elements per image row
  int it_off[CACHE_OFFSETS ? SLOTS : 1];   // interior_off() of every slot
  const half_t* xn;               // image n
  const half_t* zeros;            // >= 16 bytes of zeros: the DMA source of out-of-image halo pixels
  int iy0, ix0, ch;               // the stage being issued: first halo pixel, chunk
  bool interior;
  const half_t* base;             // only dereferenced when interior

  // halo pixel of this lane in slot j.  With cached offsets it is needed on border tiles only and is recomputed from (wave, lane);
  // without, slot 0's pixel stays in a register and slot j is 16 * NW * j further
  __device__ __forceinline__ int pixel(int j) const {
    if constexpr (CACHE_OFFSETS) return halo_piece_pixel(halo_piece(NW, j, wave), lane);
    else return q0 + HALO_PIECE_PX * NW * j;
  }
  // element offset of this lane's 16 bytes of slot j from the tile's first halo pixel, chunk 0 (interior tiles; a pixel
  // past the image re-reads the first one)
  __device__ __forceinline__ int interior_off(const ConvParams& p, int j) const {
    const int q = pixel(j);
    const int rr = q / HALO_IW, cc = q - rr * HALO_IW;
    return (q < HALO_NPIX ? rr * xrow + cc * p.x_sp : 0) + csw * 8;
  }
  // border tiles clamp per lane: the pixel's own address, or the page of zeros
  __device__ __forceinline__ const half_t* border_src(const ConvParams& p, int j) const {
    const int q = pixel(j);
    const int rr = q / HALO_IW;
    const int iy = iy0 + rr, ix = ix0 + (q - rr * HALO_IW);
    const bool ok = q < HALO_NPIX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    // ok: iy, ix and W are non-negative -- said to the compiler, the pixel index is one 32 x 32 -> 64-bit multiply-add
    const long pix = (long)((unsigned long)(unsigned)iy * (unsigned)p.W + (unsigned)ix);
    return ok ? xn + pix * p.x_sp + ch * HALO_CK + csw * 8 : zeros;
  }

  __device__ __forceinline__ void init(const ConvParams& p, const half_t* zeros_, int n, int wave_, int lane_) {
    wave = wave_;
    lane = lane_;
    q0 = halo_piece_pixel(wave_, lane_);
    csw = halo_swz_slot(lane_ >> 2, lane_ & 3);
    xrow = p.W * p.x_sp;
    xn = p.x + (long)n * p.x_sn;
    zeros = zeros_;
    iy0 = ix0 = ch = 0;
    interior = false;
    base = xn;
    if constexpr (CACHE_OFFSETS) {
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) it_off[j] = interior_off(p, j);
    }
  }
  // chunk ch of tile (ty, tx) is what the following issue() calls stream
  __device__ __forceinline__ void prep(const ConvParams& p, int ty, int tx, int ch_) {
    iy0 = ty * HALO_TH - 1;
    ix0 = tx * HALO_TW - 1;
    ch = ch_;
    interior = iy0 >= 0 && ix0 >= 0 && iy0 + HALO_IH <= p.H && ix0 + HALO_IW <= p.W;
    base = xn + ((long)iy0 * p.W + ix0) * p.x_sp + ch_ * HALO_CK;
  }
  // slot j (a compile-time constant at every call site) into the tile image at LDS byte address dst_buf
  __device__ __forceinline__ void issue(const ConvParams& p, int j, unsigned dst_buf) const {
    const int u = halo_piece(NW, j, wave);
    if constexpr (SKIP_EMPTY_PIECE) { if (u >= HALO_PIECES) return; }
    const half_t* src = base;
    if constexpr (CACHE_OFFSETS) src += it_off[j];
    else src += interior_off(p, j);
    if (!interior) src = border_src(p, j);          // uniform branch: 6 % of the tiles at 1080p
    glds16(src, dst_buf + u * HALO_PIECE_BYTES);
  }
};

// ---- the weight-stationary LDS map of v7 and v10 (bytes): [0, 40K) tile buffer 0 | [40K, 64K) weight slices 0..5 |
// [64K, 104K) tile buffer 1 | [104K, 152K) weight slices 6..17 | [152K, +512) bias, so that switching buffers is `addr ^ 0x10000`.
constexpr int WS_BUF1 = 0x10000, WS_WLO = 40 * 1024, WS_WHI = 104 * 1024, WS_MISC = 152 * 1024;
constexpr int WS_LDS = WS_MISC + 512;
constexpr int WS_WSL = 4096;             // one weight slice (chunk, tap) = [mt 2][s2 2][lane 64][8 halves]
// weight slice sl (= chunk * 9 + tap) -> LDS byte offset
__device__ __host__ constexpr int wslice_off(int sl) { return sl < 6 ? WS_WLO + sl * WS_WSL : WS_WHI + (sl - 6) * WS_WSL; }
// (c) the tile images fit their buffers (v11 states its own map in conv_mfma_v11.hip)
static_assert(HaloDma<8, true, false>::IMAGE_BYTES <= WS_WLO && HaloDma<4, true, false>::IMAGE_BYTES <= WS_WLO, "tile buffer 0");
static_assert(WS_BUF1 + WS_WLO <= WS_WHI && wslice_off(5) + WS_WSL <= WS_BUF1 && wslice_off(17) + WS_WSL <= WS_MISC, "weight-stationary LDS map");

// prologue of a weight-stationary workgroup of NTHR threads: the bias and all weights of cout block cb (compiler-tracked loads,
// younger than the first tile's DMA)
template <int NTHR>
__device__ __forceinline__ void ws_load_bias_weights(const ConvParams& p, unsigned char* smem, int cb, int nchunks, int tid) {
  if (tid < 64) reinterpret_cast<float*>(smem + WS_MISC)[tid] = p.bias[cb * 64 + tid];
  const int nslices = nchunks * 9;
  for (int i = tid; i < nslices * 256; i += NTHR) {
    const int sl = i >> 8, u = i & 255;            // u = q*64 + lane, q = mt*2 + s2
    const int qq = u >> 6, ln = u & 63;
    const half_t* src = p.w + ((((long)(cb * 2 + (qq >> 1)) * nslices + sl) * 2 + (qq & 1)) * 64 + ln) * 8;
    *reinterpret_cast<half8*>(smem + wslice_off(sl) + u * 16) = *reinterpret_cast<const half8*>(src);
  }
}

// ---- launch side ----------------------------------------------------------------------------------------------------------------
struct HaloExtra {
  int ntiles;
  const half_t* zeros;      // >= 16 bytes of zeros: the DMA source of out-of-image halo pixels
};

// What the launchers of the three kernels share: q = p with tiles_x, e.ntiles / e.zeros, and the persistent
// grid (256 workgroup slots).  Returns 0 or the error of the zeros page.
template <typename Extra>
inline int halo_launch_setup(const ConvParams& p, int cout_blocks, int N, ConvParams& q, Extra& e, dim3& grid) {
  const void* zeros = nullptr;
  if (const int zrc = tdvc_scratch_pages(&zeros, nullptr)) return zrc;
  q = p;
  q.tiles_x = (p.Wo + HALO_TW - 1) / HALO_TW;
  e.ntiles = q.tiles_x * ((p.Ho + HALO_TH - 1) / HALO_TH);
  e.zeros = reinterpret_cast<const half_t*>(zeros);
  grid = dim3(persistent_grid_x(256, cout_blocks, N, e.ntiles), cout_blocks, N);
  return 0;
}

}  // namespace convk
