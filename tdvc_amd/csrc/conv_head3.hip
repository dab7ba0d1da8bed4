// conv_head3 -- the RGB head: 3x3 / stride 1 / pad 1, 64 input channels, <= 4 output channels, planar fp32 output
// (FeatureFix.featdown, main/model/pnet.py:262), at full resolution a 267 MB read with almost no arithmetic.
//
// conv_n16 runs this layer with one 8-wave workgroup per CU that stages an 8 x 64 tile plus halo (93 KB), computes it and stores it,
// one phase after the other between barriers: while the MFMAs and the stores run nothing is in flight, and no second workgroup
// fits next to the tile to hide that (1.35 TB/s).  Same tile, same LDS layout, same arithmetic here, with two changes:
//   * the NEXT tile's 16-byte loads are issued into registers (11 per thread) right after the barrier that publishes the current
//     tile, and written to LDS only after the barrier that ends the current tile's reads: the loads of a whole tile are in flight
//     under the MFMAs, the epilogue and the stores of the tile before;
//   * the planar rows leave as full lines: the 16-pixel column blocks of a wave's row are gathered across the lanes, so a store
//     instruction writes the row's 64 consecutive floats of one channel (conv_n16: 16 at a time, through the generic epilogue).
// It is a form of conv_n16, chosen by conv_n16's launcher (launch_conv_n16): the dispatch table and the name it reports do not change.
// Arithmetic, for byte-equal results with conv_n16's own kernel: v_mfma_f32_16x16x32_f16 over the flattened (tap, channel) order in 18 k-steps of
// 32, the same lane <-> k mapping, one fp32 accumulator chain per output starting at zero; then bias, activation, fp32 store.
#include "conv_common.h"

using convk::ConvParams;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int H3_TH = 8, H3_TW = 64, H3_NTHR = 512;       // 8 waves, one output row of 64 pixels each
constexpr int H3_CIN = 64, H3_KS = 18;                    // 9 taps x 64 channels / 32
constexpr int H3_TIW = H3_TW + 2, H3_TIH = H3_TH + 2;
constexpr int H3_PS = 2 * H3_CIN + 16;                    // LDS bytes per staged pixel (conv_n16's padding)
constexpr int H3_ITEMS = H3_TIH * H3_TIW * (H3_CIN / 8);  // 16-byte pieces of a halo tile: 5280
constexpr int H3_PER_THR = (H3_ITEMS + H3_NTHR - 1) / H3_NTHR;      // 11
constexpr int H3_A_BYTES = H3_KS * 1024;
constexpr int H3_LDS = H3_A_BYTES + H3_TIH * H3_TIW * H3_PS;        // 113 472 bytes

struct Head3Extra {
  int ntiles, tiles_x, tiles_per_img;
};

__global__ __launch_bounds__(H3_NTHR, 1) void conv_head3_kernel(const ConvParams p, const Head3Extra e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wl = smem;                                          // [kstep][lane 64][16 B]
  unsigned char* tile = wl + H3_A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int px = lane & 15, kg = lane >> 4;

  // A fragments, gathered from the standard packed blob exactly as conv_n16 does for one block of 16 output channels
  for (int i = tid; i < H3_KS * 64; i += H3_NTHR) {
    const int ln = i & 63, S = i >> 6;
    const int q = 4 * S + (ln >> 4), s = q >> 1, h = q & 1;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (s < p.steps) v = *reinterpret_cast<const half8*>(p.w + ((long)s * 64 + (ln & 15) + 32 * h) * 8);
    *reinterpret_cast<half8*>(wl + (long)i * 16) = v;
  }

  // ---- staging, split in two (issue early, write late): the pieces of a tile as registers between the halves
  u32x4 treg[H3_PER_THR];
  unsigned okmask = 0u;
  auto issue = [&](int tile_i) {
    const int n = tile_i / e.tiles_per_img, rem = tile_i - n * e.tiles_per_img;
    const int ty = rem / e.tiles_x, tx = rem - ty * e.tiles_x;
    const half_t* xn = p.x + (long)n * p.x_sn;
    const int iy0 = ty * H3_TH - 1, ix0 = tx * H3_TW - 1;
    unsigned m = 0u;
#pragma unroll
    for (int u = 0; u < H3_PER_THR; ++u) {
      const int idx = tid + u * H3_NTHR;
      const int pix = idx >> 3, c8 = idx & 7;
      const int rr = pix / H3_TIW, cc = pix - rr * H3_TIW;
      const int iy = iy0 + rr, ix = ix0 + cc;
      const bool ok = (int)(idx < H3_ITEMS) & (int)(iy >= 0) & (int)(iy < p.H) & (int)(ix >= 0) & (int)(ix < p.W);
      // unconditional load at a clamped address (pixel 0 of the image where the piece lies outside); zeroed when it is written
      const half_t* src = xn + ((long)(ok ? iy : 0) * p.W + (ok ? ix : 0)) * p.x_sp + c8 * 8;
      treg[u] = *reinterpret_cast<const u32x4*>(src);
      m |= (ok ? 1u : 0u) << u;
    }
    okmask = m;
  };
  auto publish = [&]() {
#pragma unroll
    for (int u = 0; u < H3_PER_THR; ++u) {
      const int idx = tid + u * H3_NTHR;
      const int pix = idx >> 3, c8 = idx & 7;
      const u32x4 z = {0u, 0u, 0u, 0u};
      const u32x4 val = ((okmask >> u) & 1u) ? treg[u] : z;
      if (idx < H3_ITEMS) *reinterpret_cast<u32x4*>(tile + pix * H3_PS + c8 * 16) = val;
    }
  };

  const int base = (wave * H3_TIW + px) * H3_PS;                     // this wave's row, this lane's pixel of column block 0
  constexpr int cstep = 16 * H3_PS;
  // the tile offset of the lane's tap in k-step S: tap = S / 2, channels 32 (S & 1) + 8 kg .. + 7
  auto frag_off = [&](int S) {
    const int tap = S >> 1;
    const int dy = tap / 3, dx = tap - dy * 3;
    return base + (dy * H3_TIW + dx) * H3_PS + (32 * (S & 1) + 8 * kg) * 2;
  };

  f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) b4 = *reinterpret_cast<const f32x4*>(p.bias);          // channels 0 .. 3 (the lanes of kg == 0 hold them)

  int tile_i = blockIdx.x;
  if (tile_i < e.ntiles) issue(tile_i);
  for (; tile_i < e.ntiles; tile_i += gridDim.x) {
    const int n = tile_i / e.tiles_per_img, rem = tile_i - n * e.tiles_per_img;
    const int ty = rem / e.tiles_x, tx = rem - ty * e.tiles_x;
    publish();
    __syncthreads();                                                 // the tile (and, the first time, the weights) is in LDS
    if (tile_i + (int)gridDim.x < e.ntiles) issue(tile_i + gridDim.x);      // in flight until the next publish

    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    half8 a0, b0[4], a1, b1[4];
    auto load = [&](int S, half8& a, half8 (&b)[4]) {
      const int off = frag_off(S);
      a = *reinterpret_cast<const half8*>(wl + (S * 64 + lane) * 16);
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const half8*>(tile + off + c * cstep);
    };
    auto mm = [&](const half8& a, half8 (&b)[4]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[c], acc[c], 0, 0, 0);
    };
    load(0, a0, b0);
#pragma unroll 1
    for (int S = 0; S < H3_KS; S += 2) {                             // fragments of the next k-step are read under this step's MFMAs
      load(S + 1, a1, b1);
      mm(a0, b0);
      load(min(S + 2, H3_KS - 1), a0, b0);
      mm(a1, b1);
    }

    // ---- epilogue.  A lane's accumulator: output channels 4 kg .. + 3 of pixel 16 c + px; the real channels are those of kg == 0.
    // Bias and activation as convk::epilogue4 applies them, then lane l takes pixel l of the row from lane l & 15's column block l >> 4.
    const int oy = ty * H3_TH + wave;
    const int ox = tx * H3_TW + lane;
    const bool st_ok = oy < p.Ho && ox < p.Wo;
    float* yrow = reinterpret_cast<float*>(p.y.p) + ((long)n * p.cout * p.Ho + oy) * p.Wo + ox;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch < p.cout) {                                             // wave-uniform
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = acc[c][ch];
          if (p.bias) v += b4[ch];
          if (p.act) v = act_apply(v, p.act, p.slope);
          const float got = __shfl(v, px);                           // from the lane of kg == 0 with this lane's px
          if (kg == c) mine = got;
        }
        if (st_ok) yrow[(long)ch * p.Ho * p.Wo] = mine;
      }
    }
    __syncthreads();                                                 // every wave is done reading the tile
  }
}

}  // namespace

// Asked by conv_n16's launcher about a layer that conv_n16_eligible has taken (dense window, stride 1, one channel chunk, a large map):
// the 3x3 / pad 1 window over 64 channels to at most 4 planar fp32 channels, bias and activation only
bool conv_head3_takes(const ConvParams& p) {
  return p.kh == 3 && p.kw == 3 && p.pad == 1 && p.ntaps == 9 && p.in_stride == 1 && p.Cin == H3_CIN && p.steps == 2 * H3_KS && p.cout >= 1 &&
         p.cout <= 4 && p.out_mode == TDVC_OUT_NCHW_F32 && !p.res.p && !p.res2.p && !p.round16 && !p.gdn && !p.square && !p.s2d;
}

int launch_conv_head3(const ConvParams& p, int N, hipStream_t st) {
  Head3Extra e;
  e.tiles_x = (p.Wo + H3_TW - 1) / H3_TW;
  e.tiles_per_img = e.tiles_x * ((p.Ho + H3_TH - 1) / H3_TH);
  e.ntiles = N * e.tiles_per_img;
  const int grid = e.ntiles < 256 ? e.ntiles : 256;
  return convk::launch_big_lds<&conv_head3_kernel, ConvParams, Head3Extra>("tdvc_conv2d(head3)", 160 * 1024, dim3(grid), dim3(H3_NTHR), H3_LDS, st, p, e);
}
