// lf_tail — the tail of LoopFilter's Bottleneck3D as ONE inference-only launch (tdvc_lf_tail):
//
//   T   = W_t . [S_0 | S_1 | S_2]                 the temporal (3,1,1) conv: a 1x1 conv 192 -> 64 per pixel, no bias
//   s_j = lrelu(S_j + T),  j = 0..3               conv_mfma_v5's bcast_T epilogue (conv_common.h: epilogue_lean_seq<.., BCAST>)
//   o_j = conv3(s_j) + A_j                        conv_row's Cin = 64 geometry over the four slices as a batch of four images
//
// byte-equal to those two launches: each stage repeats the operations of the kernel it replaces in the same order.  The map `s`
// (1.07 GB written and read again at 1080p) never exists in memory.
//
// Structure: conv_row's row pipeline (conv_row.hip) with all four images of a pixel in one 512-byte ring pixel (the four slices are
// contiguous in memory: the ring shape of the space-to-depth geometry, 17 one-KB pieces per 34-pixel row, 6-row ring).  The conv3 weights
// are the same for the four images: wave (cg, ip) holds the 18 A fragments of output channels [16 cg, +16) once and computes image pair
// (2 ip, 2 ip + 1): 72 v_mfma_f32_16x16x32_f16 per step, 48 accumulator registers.  Per step k (one barrier):
//   * A1 (loader waves; wave (mt, nt) = 32 temporal channels x 32 ring pixels): T of ring row k + 2 from the RAW row, by the MFMA and in the
//     chunk order of conv_mfma_v5 (12 chained v_mfma_f32_32x32x16_f16 over channels 0..191, accumulator from zero, + the zero bias in
//     fp32, one rounding to fp16) into a small fp16 row buffer;
//   * A2 (all waves, elementwise): ring row k + 1 is rewritten IN PLACE in LDS as s_j = lrelu(S_j + T) with the T row of the step before
//     (fp32 add of the two fp16 values, s > 0 ? s : s * slope, one rounding);
//   * B: conv3's taps on ring row k for this wave's two images (groups in (chunk, dx) order, bias as the C operand of a chain's first
//     MFMA), the finished rows packed to a 2-row staging ring of 16 KB rows;
//   * storer waves send the row finished one step earlier as full 128-byte lines with A_j added as packed fp16, and pre-load the next
//     residual row; loader waves issue ring row k + PF.
// The three phases touch three different ring rows and two different T rows, so one workgroup barrier per step covers every hand-off:
// row r is raw until the barrier that closes step r - 3, read by A1 in step r - 2, rewritten by A2 in step r - 1, read by B in step r and
// overwritten by the DMA of step r + XRING - PF = r + 1.
// Zero padding belongs to s, the conv's input: out-of-image ring pixels are DMA'd zeros; their T is +0 (no bias) and lrelu(0 + 0) = +0.
#include "row_pipe.h"

using convk::glds16;
using convk::raw_barrier;

namespace {

constexpr int LT_SW = 32, LT_RPX = LT_SW + 2, LT_PXB = 512, LT_PIECES = 17, LT_ROWB = LT_PIECES * 1024;
constexpr int LT_XRING = 6, LT_PF = 5, LT_HD = 2;      // ring rows; rows the DMA runs ahead; land_wait leaves two steps of DMA in flight
constexpr int LT_SROW = LT_SW * LT_PXB;          // a staging row: 32 px x 4 images x 64 channels
constexpr int LT_TPS = 144, LT_TROW = LT_RPX * LT_TPS;      // a T row: 34 px x 64 channels fp16, 144-byte pixel pitch
constexpr int LT_X0 = 0, LT_S0 = LT_XRING * LT_ROWB, LT_T0 = LT_S0 + 2 * LT_SROW, LT_B0 = LT_T0 + 2 * LT_TROW, LT_LDS = LT_B0 + 256;
constexpr int LT_NTHR = 512;
static_assert(LT_RPX * LT_PXB == LT_ROWB, "a ring row is exactly 17 pieces");
// One barrier per step (BI = 1).  Ring row r is read by A1 in step r - LT_A1 (raw), rewritten in place by A2 in step r - LT_A2 and read by
// B in step r: the first read is LT_A1 steps before the row's own step, the last is in it.  The write-after-read and landing inequalities
// and the counted wait are RingTiming's (row_pipe.h); the three phases of one row lie in three different steps, so a barrier separates
// A1's read from A2's rewrite and A2's rewrite from B's read.
constexpr int LT_A1 = 2, LT_A2 = 1, LT_B = 0;
using LtTiming = rowk::RingTiming<LT_PIECES, LT_XRING, LT_PF, LT_HD, 1, LT_B, LT_A1>;
using LtLayout = rowk::RingLayout<LT_PXB>;
static_assert(LT_A1 > LT_A2 && LT_A2 > LT_B && LT_B == 0, "A1, A2 and B of a row in three consecutive steps: one barrier between each pair");
static_assert(rowk::row_check::dma_matches_reads<LtLayout>(LT_PIECES, LT_RPX), "the DMA writes every (pixel, slot) of a ring row once, where the fragment read looks for it");
static_assert(rowk::row_check::reads_conflict_free<LtLayout>(3, 2), "a 16-lane group of a B-fragment read touches 16 distinct bank slots");
static_assert((LT_T0 % 16) == 0 && LT_LDS <= 160 * 1024, "LDS");

struct TailParams {
  rowk::MapRef<const half_t> s;
  rowk::MapRef<const half_t> a;
  rowk::MapRef<half_t> y;
  const half_t* wt;         // temporal conv, standard blob (ck = 32, one tap): [cout tile 32][chunk 6][k-step 2][lane 64][8 halves]
  const half_t* w3;         // conv3, standard blob: [cout tile 32][chunk 2][k-step 18][lane 64][8 halves]
  const float* bias3;
  rowk::ScratchPages pg;    // zeros; dump: >= 16 KB
  int N, H, W, strips;
  float slope;
  float tzero;              // 0.f: the temporal conv's (absent) bias, added in fp32 as conv_mfma_v5 does
};

__global__ __launch_bounds__(LT_NTHR, 1) void lf_tail_kernel(const TailParams p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(smem));
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave < 4;                // wave-uniform roles: waves 0-3 issue the DMA and compute T, waves 4-7 store
  const int wq = wave & 3;
  const int cg = wave & 3, ip = wave >> 2;     // block of 16 output channels; image pair (2 ip, 2 ip + 1)
  const int r16 = lane & 15, kb = lane >> 4;

  // ---- workgroup -> run of rows of the flat sequence (batch item, strip, row), as conv_row does with one cout block
  const rowk::RunRange rr = rowk::run_range(1, 0, p.N, p.strips, p.H);
  const long run_begin = rr.begin, run_end = rr.end;

  // ---- conv3: this wave's 16 output channels as 18 A fragments (tap, chunk), exactly conv_row's gather from the standard blob
  half8 wf[18];
  {
    const int co = 16 * cg + r16;
    const half_t* wb = p.w3 + ((long)(co >> 5) * 2 * 18 * 64 + (kb & 1) * 32 + (co & 31)) * 8 + (long)(kb >> 1) * 512;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) wf[tap * 2 + kc] = *reinterpret_cast<const half8*>(wb + ((long)kc * 18 + tap * 2) * 512);
  }
  if (tid < 64) reinterpret_cast<float*>(smem + LT_B0)[tid] = p.bias3[tid];
  const int boff = LT_B0 + (16 * cg + 4 * kb) * 4;

  // ---- per-lane LDS offsets
  int foff[3];                                 // B fragment (dx), logical slot kb of column block 0; slot 8 j + 4 kc + kb: ^ ((8 j + 4 kc) << 4)
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    foff[dx] = LtLayout::slot_off(dx + rowk::sigma(r16), kb);
  }
  int doff[2];                                 // pack: pixel 16 cb + SIGMA(r16), image 2 ip, channels 16 cg + 4 kb .. + 3; image + 1: + 128
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int q = 16 * cb + rowk::sigma(r16), c = 16 * ip + 2 * cg + (kb >> 1);
    doff[cb] = rowk::cd_off(LT_PXB, q, c) + 8 * (kb & 1);
  }
  // A2 items: 34 px x 32 positions of 16 bytes; thread t owns position t & 31 of pixels (t >> 5) and (t >> 5) + 16, wave 7 also pixels 32, 33
  // (the swizzle term depends on q & 15 only: one logical slot per thread)
  const int a2_pos = tid & 31, a2_q = tid >> 5;
  const int a2_slot = a2_pos ^ LtLayout::term(a2_q);     // image a2_slot >> 3, channels 8 (a2_slot & 7) .. + 7
  const int a2_x = a2_q * LT_PXB + a2_pos * 16, a2_t = a2_q * LT_TPS + (a2_slot & 7) * 16;
  const bool a2_third = tid >= LT_NTHR - 64;   // wave 7: threads 448 .. 511 (a2_q = 14, 15) also own pixels 32, 33, whose swizzle term is that of pixels 0, 1
  const int a2_t3 = (a2_q + 18) * LT_TPS + ((a2_pos ^ LtLayout::term(a2_q - 14)) & 7) * 16;

  auto run = [&](auto LOADERc) __attribute__((always_inline)) {
  constexpr bool LOADER = decltype(LOADERc)::value;
  // ---- loader waves: DMA items.  Piece j of a row is ring pixels 2 j, 2 j + 1 (lane: position lane & 31 of pixel 2 j + (lane >> 5)); loader wq
  // sends pieces wq, wq + 4, wq + 8, wq + 12 and loader 0 piece 16.  Pieces 8 apart share their swizzle term: two per-lane source offsets.
  const int dq = 2 * wq + (lane >> 5);
  int soff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = dq + 8 * j;
    soff[j] = q * p.s.sp + (((lane & 31) ^ LtLayout::term(q)) << 3);
  }
  // ---- loader waves: the temporal conv.  Wave (mt, nt): channels [32 mt, +32) of ring pixels 32 nt + (lane & 31) (nt = 1: pixels 32, 33 only;
  // the other lanes re-read pixel 33 and write nothing).  Lane (r, hh) of k-step m holds channels 16 m + 8 hh .. + 7: logical slot 2 m + hh.
  const int mt = wq & 1, nt = wq >> 1;
  const int a1_q = min(32 * nt + (lane & 31), LT_RPX - 1), a1_hh = lane >> 5;
  const bool a1_ok = 32 * nt + (lane & 31) < LT_RPX;
  const int a1_x = a1_q * LT_PXB + ((a1_hh ^ LtLayout::term(a1_q)) << 4);
  const int a1_t = a1_q * LT_TPS + (32 * mt + 4 * a1_hh) * 2;
  half8 tw[LOADER ? 12 : 1];
  if constexpr (LOADER) {
#pragma unroll
    for (int m = 0; m < 12; ++m) tw[m] = *reinterpret_cast<const half8*>(p.wt + ((long)(mt * 12 + m) * 64 + lane) * 8);
  }
  // ---- storer waves: item it = (tid - 256) + 256 j: pixel it >> 5, position it & 31 of the staging row
  const int s_t = tid & 255;
  int s_px[4], s_co[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int it = s_t + 256 * j;
    s_px[j] = it >> 5;
    s_co[j] = ((it & 31) ^ rowk::stage_g(it >> 5)) << 3;
  }

  f32x4 acc[3][2][2];                          // [rotating output row][column block][image of the pair]
  half8 r1v[4] = {};

  for (long pos = run_begin; pos < run_end;) {
    const rowk::Segment sg = rowk::next_segment(pos, run_end, p.H, p.strips);      // of (batch item, strip)
    const int ra = sg.ra, rb = sg.rb, rows = sg.rows, n = sg.n;
    const int c0 = sg.strip * LT_SW;
    const int last_in = rows + 1;              // the last step that consumes an input row

    unsigned colok = 0;                        // bit j: this lane's pixel of its j-th piece is inside the image
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int col = c0 - 1 + dq + 8 * j;
      colok |= (col >= 0 && col < p.W) ? (1u << j) : 0u;
    }
    bool s_ok[4];
    int y_lo[4], r_lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + s_px[j], colc = min(col, p.W - 1);
      s_ok[j] = col < p.W;
      y_lo[j] = col * p.y.sp + s_co[j];        // element offsets fit 32 bits (checked by the host)
      r_lo[j] = colc * p.a.sp + s_co[j];
    }
    const half_t* const yimg = p.y.p + (long)n * p.y.sn;
    const half_t* const rimg = p.a.p + (long)n * p.a.sn;
    const long yrow_stride = (long)p.W * p.y.sp, rrow_stride = (long)p.W * p.a.sp, xrow_stride = (long)p.W * p.s.sp;
    const half_t* const xcol = p.s.p + (long)n * p.s.sn + (long)(c0 - 1) * p.s.sp;
#pragma unroll
    for (int s3 = 0; s3 < 3; ++s3)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) acc[s3][cb][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ring row ra - 1 + kk into ring slot kk % XRING; returns the number of DMA instructions issued
    auto issue_row = [&](int kk) __attribute__((always_inline)) -> int {
      const int row = ra - 1 + kk;
      const bool rowok = row >= 0 && row < p.H;
      const half_t* base = xcol + row * xrow_stride;
      const unsigned dst = lds0 + LT_X0 + rowk::ring_slot<LT_XRING>(kk) * LT_ROWB;
      const unsigned okb = rowok ? colok : 0u;
#pragma nounroll
      for (int j = 0; j < 4; ++j) {
        const half_t* src = base + (long)(16 * (j >> 1)) * p.s.sp + soff[j & 1];
        glds16(((okb >> j) & 1u) ? src : p.pg.zeros, dst + (wq + 4 * j) * 1024);
      }
      if (wq == 0) {
        glds16(((okb >> 4) & 1u) ? base + (long)32 * p.s.sp + soff[0] : p.pg.zeros, dst + (LT_PIECES - 1) * 1024);
        return 5;
      }
      return 4;
    };
    // A1: T of ring row kk (raw) -> T row kk & 1
    auto phase_a1 = [&](int kk) __attribute__((always_inline)) {
      if constexpr (LOADER) {
        const unsigned char* xb = smem + LT_X0 + rowk::ring_slot<LT_XRING>(kk) * LT_ROWB;
        unsigned char* tb = smem + LT_T0 + (kk & 1) * LT_TROW;
        f32x16 t;
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = 0.f;
        half8 bf[2];
        bf[0] = *reinterpret_cast<const half8*>(xb + a1_x);
#pragma unroll
        for (int m = 0; m < 12; ++m) {
          if (m + 1 < 12) bf[(m + 1) & 1] = *reinterpret_cast<const half8*>(xb + (a1_x ^ ((m + 1) << 5)));
          t = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[m], bf[m & 1], t, 0, 0, 0);
        }
        if (a1_ok) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float v0 = t[4 * g] + p.tzero, v1 = t[4 * g + 1] + p.tzero, v2 = t[4 * g + 2] + p.tzero, v3 = t[4 * g + 3] + p.tzero;
            *reinterpret_cast<half4*>(tb + a1_t + 16 * g) = half4{(half_t)v0, (half_t)v1, (half_t)v2, (half_t)v3};
          }
        }
      }
    };
    // A2: ring row kk in place: s_j = lrelu(S_j + T) with T row kk & 1
    auto phase_a2 = [&](int kk) __attribute__((always_inline)) {
      unsigned char* xb = smem + LT_X0 + rowk::ring_slot<LT_XRING>(kk) * LT_ROWB;
      const unsigned char* tb = smem + LT_T0 + (kk & 1) * LT_TROW;
      auto item = [&](int qadd, int toff) __attribute__((always_inline)) {
        unsigned char* xp = xb + a2_x + qadd * LT_PXB;
        const half8 xs = *reinterpret_cast<const half8*>(xp);
        const half8 v = *reinterpret_cast<const half8*>(tb + toff);
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float s = (float)xs[j] + (float)v[j];
          o[j] = (half_t)(s > 0.f ? s : s * p.slope);
        }
        *reinterpret_cast<half8*>(xp) = o;
      };
      item(0, a2_t);
      item(16, a2_t + 16 * LT_TPS);
      if (!LOADER && a2_third) item(18, a2_t3);
    };

    // ---- prologue: the first PF rows landed and visible; T of rows 0 and 1; row 0 rewritten
    if constexpr (LOADER) {
#pragma unroll
      for (int kk = 0; kk < LT_PF; ++kk)
        if (kk <= last_in) issue_row(kk);
    }
    rowk::wait_vmcnt<0>();
    raw_barrier();
    phase_a1(0);
    raw_barrier();
    phase_a1(1);
    phase_a2(0);
    raw_barrier();

    const int K = rows + 3;                    // steps: row k - 2 of the segment is finished in step k and stored in step k + 1
    auto step = [&](auto PHc, auto FULLc, int k) __attribute__((always_inline)) {
      constexpr int PH = decltype(PHc)::value;       // k % 3: tap row dy accumulates into slot (PH + 3 - dy) % 3
      constexpr bool FULL = decltype(FULLc)::value;
      constexpr int SD = (PH + 1) % 3;               // the finishing row: dy = 2
      if constexpr (!LOADER) {
        const int srow = ra + k - 3;
        if (FULL || (srow >= ra && srow < rb)) {
          const unsigned char* sb = smem + LT_S0 + ((k - 1) & 1) * LT_SROW;
          half_t* const yrow = const_cast<half_t*>(yimg) + srow * yrow_stride;      // wave-uniform
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            half8 yv = *reinterpret_cast<const half8*>(sb + (s_t + 256 * j) * 16);
            yv = yv + r1v[j];
            // no branch around the store (conv_row): lanes outside the image store into the dump page
            *reinterpret_cast<half8*>(s_ok[j] ? yrow + y_lo[j] : p.pg.dump + (s_t + 256 * j) * 8) = yv;
          }
        }
        const int nrow = srow + 1;
        const bool rok = FULL || (nrow >= ra && nrow < rb);
        const half_t* const rrow = rimg + (rok ? nrow : ra) * rrow_stride;          // wave-uniform; a row outside the segment reads a valid one
#pragma unroll
        for (int j = 0; j < 4; ++j) r1v[j] = *reinterpret_cast<const half8*>(rrow + r_lo[j]);
        if (FULL || k + LT_A2 <= last_in) phase_a2(k + LT_A2);       // storers: elementwise work first, under the loaders' MFMAs
      } else {
        if (FULL || k + LT_A1 <= last_in) phase_a1(k + LT_A1);
      }
      int nvm = 0;
      if (FULL || k <= last_in) {
        const unsigned char* xb = smem + LT_X0 + rowk::ring_slot<LT_XRING>(k) * LT_ROWB;
        // 12 groups (image of the pair, chunk, dx) of 6 MFMAs (3 output rows x 2 column blocks) on two B fragments, the next group's
        // fragments requested before this group's MFMAs
        half8 fb[2][2];
        auto load_group = [&](int gi, int buf) __attribute__((always_inline)) {
          const int jj = gi / 6, g = gi - 6 * jj, kc = g / 3, dx = g - 3 * kc;
          const unsigned char* b0 = xb + (foff[dx] ^ ((8 * (2 * ip + jj) + 4 * kc) << 4));
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) fb[buf][cb] = *reinterpret_cast<const half8*>(b0 + cb * 16 * LT_PXB);
        };
        const f32x4 bias4 = *reinterpret_cast<const f32x4*>(smem + boff);
        load_group(0, 0);
#pragma unroll
        for (int gi = 0; gi < 12; ++gi) {
          const int jj = gi / 6, g = gi - 6 * jj, kc = g / 3, dx = g - 3 * kc;
          if (gi + 1 < 12) load_group(gi + 1, (gi + 1) & 1);
#pragma unroll
          for (int dyo = 0; dyo < 3; ++dyo) {
            const int dy = 2 - dyo;            // the finishing row first
            const int slot = (PH + 3 - dy) % 3;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const bool first = dy == 0 && g == 0;
              acc[slot][cb][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[(dy * 3 + dx) * 2 + kc], fb[gi & 1][cb],
                                                                         first ? bias4 : acc[slot][cb][jj], 0, 0, 0);
            }
          }
        }
        if (LOADER && k + LT_PF <= last_in) nvm = issue_row(k + LT_PF);
        {
          // finished rows -> fp16 into staging row k & 1 (rows outside the segment are never stored)
          unsigned char* sb = smem + LT_S0 + (k & 1) * LT_SROW;
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              const f32x4 v = acc[SD][cb][jj];
              const half4 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
              *reinterpret_cast<half4*>(sb + doff[cb] + 128 * jj) = h;
            }
        }
      }
      if constexpr (LOADER) {
        if (FULL || k + LT_A2 <= last_in) phase_a2(k + LT_A2);       // loaders: behind their MFMAs, under the storers'
        rowk::land_wait<LtTiming>(nvm, wq);       // two steps of DMA stay in flight (loader 0: 2 x 5 instructions, the others 2 x 4)
      }
      raw_barrier();
    };
    int k = 0;
    for (; k < 3; k += 3) rowk::steps_of<3>(step, std::false_type{}, k, min(3, K));
    for (; k + 2 + 2 <= last_in; k += 3) rowk::steps_of<3>(step, std::true_type{}, k, k + 3);        // full: rows k - 3 .. stored, rows .. k + 4 consumed
    for (; k < K; k += 3) rowk::steps_of<3>(step, std::false_type{}, k, K);
  }
  };
  if (loader) run(std::true_type{});
  else run(std::false_type{});
}

// the two ranges [p, end) of an fmap's bytes do not meet
bool lt_disjoint(const tdvc_fmap& x, const tdvc_fmap& y) {
  const uintptr_t xa = (uintptr_t)x.p, ya = (uintptr_t)y.p;
  const uintptr_t xe = xa + 2 * ((uintptr_t)(x.N - 1) * x.sn + ((uintptr_t)x.H * x.W - 1) * x.sp + x.C);
  const uintptr_t ye = ya + 2 * ((uintptr_t)(y.N - 1) * y.sn + ((uintptr_t)y.H * y.W - 1) * y.sp + y.C);
  return !(xa < ye && ya < xe);
}

// nullptr when the descriptor is taken, else why not
const char* lt_refusal(const tdvc_lf_tail_desc* d) {
  if (!d) return "null descriptor";
  const tdvc_fmap &s = d->s, &a = d->a, &y = d->y;
  if (d->nslices != 4 || d->slice_stride != 64) return "four slices at channel offsets 0, 64, 128, 192";
  if (s.dtype != TDVC_F16 || a.dtype != TDVC_F16 || y.dtype != TDVC_F16) return "s, a and y must be fp16 maps";
  if (!fmap_ok16(s) || !fmap_ok16(a) || !fmap_ok16(y)) return "s, a and y must be 16-byte aligned maps with channels and strides in multiples of 8";
  if (s.C != 256 || a.C != 256 || y.C != 256) return "s, a and y must have 4 x 64 channels";
  if (a.N != s.N || a.H != s.H || a.W != s.W || y.N != s.N || y.H != s.H || y.W != s.W) return "s / a / y geometry mismatch";
  if ((long)s.H * s.W < convk::LARGE_MAP_PIXELS || s.H < 16) return "the map is under the floor (8192 pixels, 16 rows)";
  const long px = (long)s.H * s.W;
  if (px * s.sp >= (1L << 31) || px * a.sp >= (1L << 31) || px * y.sp >= (1L << 31)) return "element offsets within an image must fit 32 bits";
  if (!d->wt || !d->w3 || !d->bias3 || !aligned16(d->wt) || !aligned16(d->w3) || ((uintptr_t)d->bias3 & 3)) return "weights / conv3 bias missing or misaligned";
  if (d->bias_t) return "the temporal conv must have no bias (zero padding is applied behind it)";
  if (!lt_disjoint(s, y) || !lt_disjoint(a, y)) return "y overlaps s or a (the kernel is out of place)";
  return nullptr;
}

}  // namespace

extern "C" int tdvc_lf_tail_supported(const tdvc_lf_tail_desc* d) { return lt_refusal(d) ? 0 : 1; }

extern "C" int tdvc_lf_tail(const tdvc_lf_tail_desc* d, void* stream) {
  if (const char* why = lt_refusal(d)) {
    tdvc_set_error("tdvc_lf_tail: %s", why);
    return TDVC_EINVAL;
  }
  TailParams q;
  if (const int zrc = rowk::scratch_pages(q.pg)) return zrc;
  q.s = rowk::map_ref<const half_t>(d->s.p, d->s.sn, d->s.sp);
  q.a = rowk::map_ref<const half_t>(d->a.p, d->a.sn, d->a.sp);
  q.y = rowk::map_ref<half_t>(d->y.p, d->y.sn, d->y.sp);
  q.wt = reinterpret_cast<const half_t*>(d->wt);
  q.w3 = reinterpret_cast<const half_t*>(d->w3);
  q.bias3 = d->bias3;
  q.N = d->s.N; q.H = d->s.H; q.W = d->s.W;
  q.strips = (q.W + LT_SW - 1) / LT_SW;
  q.slope = d->slope;
  q.tzero = 0.f;
  const long allrows = (long)q.N * q.strips * q.H;
  const int grid = allrows < 256 ? (int)allrows : 256;       // one workgroup per CU
  const int rc = convk::launch_big_lds<&lf_tail_kernel>("tdvc_lf_tail", LT_LDS, dim3(grid), dim3(LT_NTHR), LT_LDS, reinterpret_cast<hipStream_t>(stream), q);
  // the launch stands for 1 + N launches of tdvc_conv2d (the temporal conv, conv3 per batch item): the convs behind it keep the walk
  // direction they had, and with it the bytes of feat_fusion's channel sums
  if (rc == TDVC_OK) tdvc_conv_walk_advance(1 + q.N);
  return rc;
}
