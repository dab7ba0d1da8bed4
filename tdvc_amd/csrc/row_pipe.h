// The row pipeline shared by conv_row, lf_tail and conv_pair ("The shared row pipeline"): weights in registers, input rows
// streamed by LDS-DMA into a ring PF rows ahead, rotating accumulator rows, fp16 staging rows stored as full lines through the dump
// page, BI steps closed by one barrier and an exactly counted `s_waitcnt vmcnt`.  What stands here stands once: the LDS layouts, the ring
// inequalities, the counted wait, the ring slot, the run walk, pack / activation, the step rotation and the host-side parameter types.
// The layout invariants between the DMA (producer) and the B-fragment reads (consumer), the bank-conflict freedom of those reads and
// the ring inequalities are static_asserts: evaluated at every build.  The weight gather, the dense loader, the store phase and the
// step loops are still written out in conv_row.hip and lf_tail.hip: as shared functions they moved conv_row's vector-memory
// instructions and with them the compiler's own waits ("The shared row pipeline").
#pragma once
#include <type_traits>

#include "conv_dma.h"

namespace rowk {

// 1. Layout.  A ring row is pixel-major, PXB bytes per pixel in 16-byte positions; logical slot c (channels 8 c .. 8 c + 7) of ring
// pixel q sits at position c ^ term(q).  The DMA writes positions linearly (piece j at j * 1024 + 16 * lane), so the XOR sits on its
// SOURCE address: the lane that writes position pos of pixel q fetches slot pos ^ term(q).  A B fragment is read by ds_read_b128
// with lane (r, kb) = pixel p0 + lane_px(r), slot 4 kc + kb.
// fragment lane -> pixel of its 16-pixel block: lanes {0-3, 12-15} of a 16-lane group read the even pixels, {4-11} the odd ones
constexpr __host__ __device__ __forceinline__ int sigma(int r) { return r < 4 ? 2 * r : (r >= 12 ? 2 * r - 16 : 2 * r - 7); }
// staging-row swizzle term (and the 128-byte ring pixel's under SIGMA)
constexpr __host__ __device__ __forceinline__ int stage_g(int q) { return (q >> 1) & 7; }
// conv_pair's table G = {0, 1, 2, 4, 5, 6, 2, 6}[(q >> 1) & 7]: one of the 720 that keep the three windows conflict-free WITHOUT SIGMA
constexpr __host__ __device__ __forceinline__ int pair_term(int q) { return (int)((0x62654210u >> (4 * ((q >> 1) & 7))) & 7u); }

// PXB: 128 / 256 / 512 bytes per ring pixel.  TABLE: conv_pair's layout (fragment lane r reads pixel r, term from the table);
// otherwise the SIGMA layouts of conv_row and lf_tail: term = q & 12 | swap of bits 0 and 1 of q (pairs q with q ^ 2, same parity),
// for the 128-byte pixel (q >> 1) & 7.
template <int PXB_, bool TABLE_ = false>
struct RingLayout {
  static constexpr int PXB = PXB_;
  static constexpr bool TABLE = TABLE_;
  static constexpr int LPP = PXB / 16;             // 16-byte positions (= DMA lanes) per ring pixel
  static constexpr int PPX = 1024 / PXB;           // ring pixels per 1-KB DMA piece
  static constexpr int PERIOD = 16;                // term(q + 16) == term(q)
  static_assert(PXB == 128 || PXB == 256 || PXB == 512, "ring pixel");
  static_assert(!TABLE || PXB == 128, "the table serves the 128-byte pixel");
  static constexpr __host__ __device__ __forceinline__ int term(int q) {
    if (TABLE) return pair_term(q);
    return PXB == 128 ? stage_g(q) : ((q & 12) | ((q & 1) << 1) | ((q >> 1) & 1));
  }
  static constexpr __host__ __device__ __forceinline__ int lane_px(int r) { return TABLE ? r : sigma(r); }
  // byte offset in the ring row of logical slot `slot` of pixel q (a B fragment: slot = 4 kc + kb; kc is applied later as ^ (kc << 6))
  static constexpr __host__ __device__ __forceinline__ int slot_off(int q, int slot) {
    const int t = term(q);          // (the order of evaluation is the kernels' before they shared this: their listings did not move)
    return q * PXB + ((slot ^ t) << 4);
  }
  // the logical slot that DMA lane `lane` of piece `piece` fetches, and the ring pixel it belongs to
  static constexpr __host__ __device__ __forceinline__ int dma_px(int piece, int lane) { return PPX * piece + lane / LPP; }
  static constexpr __host__ __device__ __forceinline__ int dma_slot(int piece, int lane) { return (lane % LPP) ^ term(dma_px(piece, lane)); }
};
// C/D-layout offset (pack of a finished row, conv_pair's identity read): 16-byte slot c of pixel q of pitch `pitch` bytes under the staging
// term (TABLE: conv_pair's); a lane's four channels are the 8-byte half (kb & 1) of it: + 8 * (kb & 1)
template <bool TABLE = false>
constexpr __host__ __device__ __forceinline__ int cd_off(int pitch, int q, int c) {
  return q * pitch + ((c ^ (TABLE ? pair_term(q) : stage_g(q))) << 4);
}

namespace row_check {
// (a) over all (piece, lane) every (pixel, position) of a ring row of `npx` pixels is written once, and the B-fragment read of logical
// slot c of pixel q looks where the DMA put that slot
template <class L>
constexpr bool dma_matches_reads(int pieces, int npx) {
  int cnt[80 * 32] = {};
  if (npx > 80 || npx * L::PXB > pieces * 1024) return false;
  for (int j = 0; j < pieces; ++j)
    for (int lane = 0; lane < 64; ++lane) {
      const int q = L::dma_px(j, lane), pos = lane % L::LPP;
      if (j * 1024 + lane * 16 != q * L::PXB + pos * 16) return false;          // lane-linear piece
      if (q < npx) ++cnt[q * 32 + pos];
      const int c = L::dma_slot(j, lane);
      if (c < 0 || c >= L::LPP) return false;
      if (L::slot_off(q, c) != q * L::PXB + pos * 16) return false;             // the read of slot c finds this lane's bytes
    }
  for (int q = 0; q < npx; ++q)
    for (int pos = 0; pos < L::LPP; ++pos)
      if (cnt[q * 32 + pos] != 1) return false;
  // the period the loaders rely on: one per-lane source offset serves pieces whose pixels are a multiple of PERIOD apart
  for (int q = 0; q < npx; ++q)
    if (L::term(q) != L::term(q + L::PERIOD)) return false;
  return true;
}
// (b) the 16-lane groups in which gfx950 serves a ds_read_b128 (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32):
// every group of every B-fragment read -- windows dx < kw, 16-pixel column blocks cb < ncb, chunks kc -- touches 16 distinct
// 16-byte bank slots (64 banks x 4 B = 16 slots)
constexpr int group_lane(int g, int i) {
  const int base = (g >> 1) * 32;
  if ((g & 1) == 0) return base + (i < 4 ? i : (i < 8 ? 8 + i : 12 + i));        // 0-3, 12-15, 20-27
  return base + (i < 8 ? 4 + i : (i < 12 ? 8 + i : 16 + i));                      // 4-11, 16-19, 28-31
}
template <class L>
constexpr bool reads_conflict_free(int kw, int ncb) {
  for (int dx = 0; dx < kw; ++dx)
    for (int cb = 0; cb < ncb; ++cb)
      for (int kc = 0; kc < L::LPP / 4; ++kc)
        for (int g = 0; g < 4; ++g) {
          unsigned seen = 0;
          for (int i = 0; i < 16; ++i) {
            const int lane = group_lane(g, i), r16 = lane & 15, kb = lane >> 4;
            const int q = dx + 16 * cb + L::lane_px(r16);
            // the kernels form the offset of chunk kc as (chunk 0's) ^ (kc << 6): the same bytes as slot 4 kc + kb
            if ((L::slot_off(q, kb) ^ (kc << 6)) != L::slot_off(q, 4 * kc + kb)) return false;
            seen |= 1u << ((L::slot_off(q, 4 * kc + kb) >> 4) & 15);
          }
          if (seen != 0xFFFFu) return false;
        }
  return true;
}
constexpr bool groups_partition_the_wave() {
  unsigned long long seen = 0;
  for (int g = 0; g < 4; ++g)
    for (int i = 0; i < 16; ++i) seen |= 1ull << group_lane(g, i);
  return seen == ~0ull;
}
static_assert(groups_partition_the_wave(), "ds_read_b128 lane groups");
}  // namespace row_check

// 2. Ring timing.  Step k consumes ring row k; a workgroup barrier closes every BI-th step, so between two barriers two waves are at
// most BI - 1 steps apart and always in the same barrier interval.  The DMA of row k + PF is ISSUED in step k by a loader wave;
// land_wait() after step s leaves the DMA issued in steps s - HD + 1 .. s in flight.  A row r is first read in step r - EARLIEST and
// last read in step r + OLDEST.
template <int PIECES_, int XRING_, int PF_, int HD_, int BI_, int OLDEST_, int EARLIEST_>
struct RingTiming {
  static constexpr int PIECES = PIECES_, XRING = XRING_, PF = PF_, HD = HD_, BI = BI_, OLDEST = OLDEST_, EARLIEST = EARLIEST_;
  static constexpr int NP = PIECES / 4 + 1;        // DMA instructions a loader may issue per row: PIECES / 4 regular pieces + the odd one
  static_assert((PIECES % 4) == 1, "four loaders share the regular pieces; one odd piece");
  static_assert((BI & (BI - 1)) == 0 && OLDEST >= 0 && EARLIEST >= 0, "barrier interval");
  // write-after-read: the DMA issued in step k by the fastest loader overwrites row k + PF - XRING; the slowest wave of the interval
  // is at step >= k - (BI - 1) and its oldest read is the row OLDEST behind that step: k + PF - XRING < k - (BI - 1) - OLDEST
  static_assert(PF + BI + OLDEST <= XRING, "input ring, write-after-read: a DMA would land on a row that a wave BI - 1 steps behind has not read");
  // landing: a loader's own pieces of row r (issued in step r - PF) are known to have landed after its land_wait() of a step
  // s >= r - PF + HD; the other waves learn it at the next barrier.  The row's first read is in step r - EARLIEST, and the last barrier
  // before that step closes a step >= r - EARLIEST - BI: r - PF + HD <= r - EARLIEST - BI
  static_assert(PF >= HD + BI + EARLIEST, "landing: row r must be past land_wait()'s history window before the last barrier in front of its first read");
  // the counted wait: loader waves issue nothing but DMA.  HD = 4: the odd piece goes round the four loaders, 4 (NP - 1) + 1 over any
  // four consecutive steps.  HD = 2: loader 0 owns it, 2 NP, the others 2 (NP - 1).  Shorter histories (the first steps of a segment)
  // have fewer outstanding and pass without waiting.
  static_assert(HD == 4 || HD == 2, "land_wait(): four-step history with the odd piece going round the loaders, or two steps with a fixed owner");
  static constexpr int wait_count(bool owner) { return HD == 4 ? 4 * (NP - 1) + 1 : 2 * (owner ? NP : NP - 1); }
  static_assert(wait_count(true) <= 63, "vmcnt is a 6-bit counter");
};

// 3. ring slot of row kk: a mask for the power-of-two rings; the others divide by a constant -- on the scalar unit (kk is wave-uniform;
// left to itself hipcc did the multiply-high in vector registers, three more live registers in kernels at the 256-register limit)
template <int XRING> __device__ __forceinline__ int ring_slot(int kk) {
  if constexpr ((XRING & (XRING - 1)) == 0) return kk & (XRING - 1);
  else return __builtin_amdgcn_readfirstlane(kk) % XRING;
}

// 4. the counted wait of loader wq at the end of a step in which it issued nvm DMA instructions (0: issuing has stopped, everything lands)
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <class T> __device__ __forceinline__ void land_wait(int nvm, int wq) {
  if (!nvm) { wait_vmcnt<0>(); return; }
  if constexpr (T::HD == 4) {
    wait_vmcnt<T::wait_count(true)>();
  } else {
    if (wq == 0) wait_vmcnt<T::wait_count(true)>();
    else wait_vmcnt<T::wait_count(false)>();
  }
}
// 5. Run walk.  A launch's work is the flat sequence of (image, strip, row) = N * strips * H rows of one strip width; a cout block's S
// workgroup slots cut it into S equal runs (a run that crosses a strip end is two segments), so every workgroup gets the same number of
// rows whatever H and the strip count are.  Workgroup b sits on XCD b % 8: an XCD's slots take consecutive runs (neighbouring strips
// share their column halo in that XCD's L2); the cout block is fixed per workgroup (its weights are loaded once).
struct RunRange {
  int cbk;                  // cout block of this workgroup
  long begin, end;          // its rows of the flat sequence
};
__device__ __forceinline__ RunRange run_range(int ncb, int reverse, int N, int strips, int H) {
  const int nwg = (int)gridDim.x, b = (int)blockIdx.x;
  int cbk, pos_slot, nslots;
  if ((nwg & 7) == 0 && ((nwg >> 3) % ncb) == 0) {
    const int slot = b >> 3, per_xcd = (nwg >> 3) / ncb;
    cbk = slot % ncb;
    pos_slot = (b & 7) * per_xcd + slot / ncb;
    nslots = 8 * per_xcd;
  } else {
    cbk = b % ncb; pos_slot = b / ncb; nslots = nwg / ncb;
  }
  if (reverse) pos_slot = nslots - 1 - pos_slot;
  const long allrows = (long)N * strips * H;
  return {cbk, allrows * pos_slot / nslots, allrows * (pos_slot + 1) / nslots};
}
// the segment at `pos` of a run: rows [ra, rb) of strip `strip` of image n; advances pos behind it
struct Segment { int n, strip, ra, rb, rows; };
__device__ __forceinline__ Segment next_segment(long& pos, long run_end, int H, int strips) {
  const int sid = (int)(pos / H);            // (image, strip)
  const int ra = (int)(pos - (long)sid * H), rb = (int)min((long)H, ra + (run_end - pos));
  const int rows = rb - ra;
  pos += rows;
  const int n = sid / strips;
  return {n, sid - n * strips, ra, rb, rows};
}

// 6. Pack and activation: an accumulator row's four channels -> fp16 -> max(v, v * slope) in packed fp16 math (A: 0 none, 1 ReLU,
// 2 LeakyReLU as max(v, v * slope), slope 1 = none), what the unfused kernels compute
template <int A>
__device__ __forceinline__ half4 actk(half4 v, half4 sl) {
  if constexpr (A == 1) {
    const half4 z = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
    return __builtin_elementwise_max(v, z);
  } else if constexpr (A == 2) {
    return __builtin_elementwise_max(v, v * sl);
  } else {
    return v;
  }
}
template <int A>
__device__ __forceinline__ half4 pack_act(const f32x4 v, half4 sl) {
  const half4 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
  return actk<A>(h, sl);
}

// 7. Step sequencer.  step(PH, FULL, k): PH = k % KH is a compile-time constant (the accumulator rows rotate through registers),
// FULL the steady state in which every part of a step is active (straight-line code).  The kernels loop over groups of KH steps: edge
// groups up to the first steady-state step (a multiple of KH), full groups, edge groups to the end.
template <int KH, class Step, class Full>
__device__ __forceinline__ void steps_of(Step& step, Full fullc, int k0, int kend) {     // up to KH steps from k0 (k0 % KH == 0), while < kend
  static_assert(KH == 2 || KH == 3, "accumulator rotation");
  step(std::integral_constant<int, 0>{}, fullc, k0);
  if (k0 + 1 < kend) step(std::integral_constant<int, 1 % KH>{}, fullc, k0 + 1);
  if constexpr (KH == 3) {
    if (k0 + 2 < kend) step(std::integral_constant<int, 2 % KH>{}, fullc, k0 + 2);
  }
}

// Host side: what the three parameter structs and launchers share
template <class T> struct MapRef {
  T* p;
  long sn;                  // image stride (elements)
  int sp;                   // pixel stride (elements)
};
template <class T> inline MapRef<T> map_ref(const void* p, long sn, int sp) { return {reinterpret_cast<T*>(const_cast<void*>(p)), p ? sn : 0, p ? sp : 0}; }
struct ScratchPages {
  const half_t* zeros;      // >= 16 B of zeros: DMA source of out-of-image pixels
  half_t* dump;             // a page nobody reads: store target of items outside the image (keeps the store branch-free)
};
inline int scratch_pages(ScratchPages& pg) {
  const void* zeros = nullptr;
  void* dump = nullptr;
  if (const int zrc = tdvc_scratch_pages(&zeros, &dump)) return zrc;
  pg.zeros = reinterpret_cast<const half_t*>(zeros);
  pg.dump = reinterpret_cast<half_t*>(dump);
  return 0;
}

}  // namespace rowk
