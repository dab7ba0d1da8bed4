// The forward deformable conv behind tdvc_dcn_fused, shared by csrc/dcn.hip (fp16 maps) and csrc/dcn_f32.hip (fp32 maps): the one
// statement of the sampling rule (dcn_corners), the gather sampler and the epilogue of every kernel, and the gather kernel itself
// as a template over the element type.  Operator: 8 deformable groups x 8 channels, 3x3, stride 1, pad 1, dilation 1, 64 -> 64.
#pragma once
#include "common.h"

#include <type_traits>

namespace {

constexpr int DCN_G = 8;                         // deformable groups, 8 channels each (the launcher refuses anything else)
constexpr int DCN_TPX = 8, DCN_TPY = 8;          // pixel tile of dcn_fused_kernel

// the 8 channels of a group are read and written 16 bytes at a time: one half8 (fp16) or two f32x4 (fp32)
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename T> using dcn_vec = std::conditional_t<std::is_same_v<T, float>, f32x4, half8>;
template <typename T> using dcn_vec2 = std::conditional_t<std::is_same_v<T, float>, f32x2, half2v>;
template <typename T> struct DcnGroup {
  static constexpr int NV = (int)sizeof(T) / 2, VL = 8 / NV;      // vectors per group, channels per vector
  dcn_vec<T> v[NV];
  __device__ __forceinline__ static DcnGroup load(const void* p) {
    DcnGroup g;
#pragma unroll
    for (int k = 0; k < NV; ++k) g.v[k] = reinterpret_cast<const dcn_vec<T>*>(p)[k];
    return g;
  }
  __device__ __forceinline__ void store(void* p) const {
#pragma unroll
    for (int k = 0; k < NV; ++k) reinterpret_cast<dcn_vec<T>*>(p)[k] = v[k];
  }
};

template <typename T>
struct DcnParams {
  const T* x; long x_sn; int x_sp; int H, W;
  const T* om; long om_sn; int om_sp;
  FMap y;
  const T* w; const float* bias;
  int act; float slope; int round16;
  long npix;          // H*W
  const T* xp;        // fp16 only: group-planar copy of x ([N][8][H][W][8]) or null
};

// The sampling rule (dcn_v2_im2col_cuda.cu:25-54: bilinear, zero outside; :180: open-interval test), branch-free: the four corner
// weights with the modulation mask folded in, zero for a corner outside the image or a position outside (-1, H) x (-1, W), and the
// corner coordinates clamped into the image, so that every corner can be loaded without a test.  The clamp before floorf keeps an
// infinite or huge position finite: it lies outside and contributes zero, never NaN.
// dcn_pos is the rule's first half, shared with the backward kernels (csrc/dcn_backward.hip), which need the fractions for the
// derivative weights: the open-interval test, the clamped position's integer corner and its fractions.
struct DcnPos {
  bool inside;               // the position lies in (-1, H) x (-1, W)
  int h_low, w_low;          // floor of the clamped position
  float lh, lw;              // fractions: weights (1 - lh, lh) x (1 - lw, lw) on rows h_low, h_low + 1 and columns w_low, w_low + 1
};

__device__ __forceinline__ DcnPos dcn_pos(int H, int W, float h_im, float w_im) {
  DcnPos q;
  q.inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  const float hc = fminf(fmaxf(h_im, -2.f), (float)H + 1.f), wc = fminf(fmaxf(w_im, -2.f), (float)W + 1.f);
  const float hf = floorf(hc), wf = floorf(wc);
  q.h_low = (int)hf; q.w_low = (int)wf;
  q.lh = hc - hf; q.lw = wc - wf;
  return q;
}

// the modulation mask of a logit: fp16 maps rcp(1 + __expf(-m)) (the bits the exact tests' dyadic grade pins), fp32 maps a true
// division of expf (logits +-60000 give exactly 1 and 0, logit 0 exactly 0.5)
template <typename T>
__device__ __forceinline__ float dcn_mask(float m) {
  if constexpr (std::is_same_v<T, float>) return 1.f / (1.f + expf(-m));
  else return __builtin_amdgcn_rcpf(1.f + __expf(-m));
}

struct DcnCorners {
  float w1, w2, w3, w4;      // (y0, x0), (y0, x1), (y1, x0), (y1, x1)
  int y0, y1, x0, x1;
};

__device__ __forceinline__ DcnCorners dcn_corners(int H, int W, float h_im, float w_im, float mask) {
  DcnCorners c;
  const DcnPos q = dcn_pos(H, W, h_im, w_im);
  const bool inside = q.inside;
  const int h_low = q.h_low, w_low = q.w_low, h_high = h_low + 1, w_high = w_low + 1;
  const float lh = q.lh, lw = q.lw, hh = 1.f - lh, hw = 1.f - lw;
  const bool hl = h_low >= 0 && h_low <= H - 1, hhg = h_high >= 0 && h_high <= H - 1;
  const bool wl = w_low >= 0 && w_low <= W - 1, whg = w_high >= 0 && w_high <= W - 1;
  c.w1 = (inside && hl && wl) ? hh * hw * mask : 0.f; c.w2 = (inside && hl && whg) ? hh * lw * mask : 0.f;
  c.w3 = (inside && hhg && wl) ? lh * hw * mask : 0.f; c.w4 = (inside && hhg && whg) ? lh * lw * mask : 0.f;
  c.y0 = min(max(h_low, 0), H - 1); c.y1 = min(max(h_high, 0), H - 1);
  c.x0 = min(max(w_low, 0), W - 1); c.x1 = min(max(w_high, 0), W - 1);
  return c;
}

// The gather sampler: the 8 channels of one group at the four corners, combined with 4 fused multiply-adds per channel.  fp16
// samples are converted inside the FMA (v_fma_mix_f32, ~40 vector instructions instead of ~100) and the result is rounded to fp16;
// fp32 samples stay fp32.
template <typename T>
__device__ __forceinline__ DcnGroup<T> dcn_sample8(const T* xg, int W, int sp, const DcnCorners& c) {
  using GV = DcnGroup<T>;
  const int r0 = c.y0 * W, r1 = c.y1 * W;                 // pixel indices fit 32 bits (checked by the host)
  const T* p1 = xg + (long)(r0 + c.x0) * sp;
  const T* p2 = xg + (long)(r0 + c.x1) * sp;
  const T* p3 = xg + (long)(r1 + c.x0) * sp;
  const T* p4 = xg + (long)(r1 + c.x1) * sp;
  const GV v1 = GV::load(p1), v2 = GV::load(p2), v3 = GV::load(p3), v4 = GV::load(p4);
  GV o;
#pragma unroll
  for (int j = 0; j < GV::VL; ++j)
#pragma unroll
    for (int k = 0; k < GV::NV; ++k)
      o.v[k][j] = (T)__builtin_fmaf(c.w1, (float)v1.v[k][j], __builtin_fmaf(c.w2, (float)v2.v[k][j], __builtin_fmaf(c.w3, (float)v3.v[k][j], c.w4 * (float)v4.v[k][j])));
  return o;
}

// Epilogue of every kernel: the 16 accumulators of lane (r, hh) of a 32x32 product are channels mt*32 + 8*gq + 4*hh + i of one
// pixel; + bias, one rounding to fp16 if round16 (the reference's `.half()`), the activation in fp32, then 4 channels per store.
// `yoff`: element offset of the pixel in y.  Y32: y may be an fp32 map (p.y.f32); an fp16 y takes one more rounding.
template <bool Y32>
__device__ __forceinline__ void dcn_store(const f32x16& acc, int mt, int hh, const float* bias, int round16, int act, float slope,
                                          const FMap& y, long yoff) {
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const int co = mt * 32 + 8 * gq + 4 * hh;
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + co);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[4 * gq + i] + b4[i];
      if (round16) v = (float)(half_t)v;
      o[i] = act_apply(v, act, slope);
    }
    if (Y32 && y.f32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(y.p) + yoff + co) = o;
    } else {
      half4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = (half_t)o[i];
      *reinterpret_cast<half4*>(reinterpret_cast<half_t*>(y.p) + yoff + co) = h;
    }
  }
}

// The gather kernel, T = half_t or float.  One 256-thread workgroup = an 8x8 pixel tile x all 64 output channels.
//   sampling phase: thread (pixel = tid>>3 [+32], group = tid&7) -> the 8 lanes of a pixel read one full NHWC line per bilinear
//     corner (coalesced), branch-free (clamped address, zeroed weight) so all corner loads of a tap are in flight together;
//     modulated samples go to an LDS column tile of one kernel row (3 taps) x 64 channels per pixel (stride +16 B: conflict-free).
//   matrix phase: wave (mt, nt) multiplies the 32-row weight tile mt with the 32-pixel half nt, 3 taps per barrier pair.  Weight
//     blob [cout tile 2][step 36][lane 64][8]; lane (r, hh) reads its 8 k-values of step (tap, s2) -- the 8 channels of group
//     2 s2 + hh of pixel r -- from the column tile.  fp16: one 32x32x16 MFMA per step.  fp32 (tdvc_pack_conv_weights_indexed_f32,
//     ck = 64): eight 32x32x2 MFMAs, MFMA j contracting channel j of groups 2 s2 (hh = 0) and 2 s2 + 1 (hh = 1).
// k order of a pixel's sum: tap 0..8 (row-major), inside a tap the group pairs (0,1), (2,3), (4,5), (6,7); fp32:
// inside a pair channel j = 0..7, inside one MFMA the even group before the odd one.  It depends on nothing but the operator.
// fp32 maps: x, offsets and mask logits are fp32, a sampling position is base + offset in fp32, the mask is 1 / (1 + expf(-logit))
// with a true division (logits +-60000 give exactly 1 and 0, logit 0 exactly 0.5), and nothing is rounded to fp16 before the
// epilogue; the kernel is bound by the fp32 matrix pipe (288 MFMAs of 64 cycles per wave and tile) at every map size.
template <typename T>
__global__ __launch_bounds__(256) void dcn_fused_kernel(const DcnParams<T> p) {
  constexpr bool F32 = std::is_same_v<T, float>;
  constexpr int GB = 8 * sizeof(T);                      // bytes of one group's 8 channels
  constexpr int PS = 3 * DCN_G * GB + 16;                // LDS bytes per pixel (3 taps x 64 channels + pad)
  extern __shared__ __attribute__((aligned(16))) unsigned char col[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, r = lane & 31;
  const int mt = wave & 1, nt = wave >> 1;
  const int tiles_x = (p.W + DCN_TPX - 1) / DCN_TPX;
  const int tile_id = tdvc_xcd_tile(blockIdx.x);
  const int tx = tile_id % tiles_x, ty = tile_id / tiles_x;
  const int n = blockIdx.y;

  // ---- sampling identity: two pixels per thread (pass 0: pixels 0..31, pass 1: 32..63)
  const int g = tid & 7;
  // gather source of this thread's group: the NHWC map (pixel stride x_sp: every 16-byte corner of every lane is a line
  // of its own -- the L1 takes one line per clock, profiles/r01_dcn_fused_1080p_pmc.txt) or, fp16 only, the group-planar copy
  // [n][g][H][W][8] (pixel stride 8: the 8 lanes of a group sample 8 neighbouring pixels, whose corners share lines)
  const T* xg = p.x + (long)n * p.x_sn + g * 8;
  int xsp = p.x_sp;
  if constexpr (!F32) {
    if (p.xp) { xg = p.xp + ((long)n * DCN_G + g) * p.npix * 8; xsp = 8; }
  }
  int soy[2], sox[2];
  dcn_vec2<T> off[2][9];
  float msk[2][9];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int pl = (tid >> 3) + 32 * ps;
    soy[ps] = ty * DCN_TPY + (pl >> 3);
    sox[ps] = tx * DCN_TPX + (pl & 7);
    const int cy = min(soy[ps], p.H - 1), cx = min(sox[ps], p.W - 1);     // an overhanging pixel samples for its clamped twin; never stored
    const T* omp = p.om + (long)n * p.om_sn + ((long)cy * p.W + cx) * p.om_sp;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      off[ps][t][0] = omp[g * 18 + 2 * t];
      off[ps][t][1] = omp[g * 18 + 2 * t + 1];
      const float m = (float)omp[18 * DCN_G + g * 9 + t];                 // sigmoid (dcn_v2_amp.py: mask = sigmoid(mask))
      msk[ps][t] = dcn_mask<T>(m);
    }
  }

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const T* wbase = p.w + ((long)mt * 36 * 64 + lane) * 8;
  const unsigned char* bcol = col + (nt * 32 + r) * PS + hh * GB;

  // The barrier between the two phases.  fp16: a fence for the instruction scheduler as well -- with the 36 k-steps unrolled it
  // otherwise moves the next row's corner loads into the matrix phase, which costs the L1-bound sampling 10 % at 1088 x 1920; the
  // fp32 kernel is 6 % faster without the fence (profiles/r17_dcn_refactor_ab.txt)
  auto phase_barrier = [] {
    if constexpr (!F32) __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if constexpr (!F32) __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll
  for (int chunk = 0; chunk < 3; ++chunk) {             // fully unrolled: tap registers are selected at compile time
    if (chunk > 0) phase_barrier();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
      for (int tc = 0; tc < 3; ++tc) {
        const dcn_vec2<T> o2 = off[ps][chunk * 3 + tc];
        const float h_im = (float)(soy[ps] - 1 + chunk) + (float)o2[0];      // tap = chunk*3 + tc: dy = chunk, dx = tc
        const float w_im = (float)(sox[ps] - 1 + tc) + (float)o2[1];
        const DcnCorners c = dcn_corners(p.H, p.W, h_im, w_im, msk[ps][chunk * 3 + tc]);
        const int pl = (tid >> 3) + 32 * ps;
        dcn_sample8<T>(xg, p.W, xsp, c).store(col + pl * PS + (tc * DCN_G + g) * GB);
      }
    }
    phase_barrier();
#pragma unroll
    for (int tc = 0; tc < 3; ++tc) {
#pragma unroll
      for (int s2 = 0; s2 < DCN_G / 2; ++s2) {
        const DcnGroup<T> a = DcnGroup<T>::load(wbase + (long)((chunk * 3 + tc) * (DCN_G / 2) + s2) * 512);
        const DcnGroup<T> b = DcnGroup<T>::load(bcol + (tc * DCN_G + 2 * s2) * GB);
        if constexpr (F32) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j >> 2][j & 3], b.v[j >> 2][j & 3], acc, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.v[0], b.v[0], acc, 0, 0, 0);
        }
      }
    }
  }

  const int pl = nt * 32 + r;
  const int oy = ty * DCN_TPY + (pl >> 3), ox = tx * DCN_TPX + (pl & 7);
  if (oy < p.H && ox < p.W)
    dcn_store<F32>(acc, mt, hh, p.bias, p.round16, p.act, p.slope, p.y, (long)n * p.y.sn + ((long)oy * p.W + ox) * p.y.sp);
}

// A launch with more dynamic LDS than the 64 KB every kernel may have by default: reserved once per device
template <auto KERNEL, int BYTES>
int dcn_reserve_lds() {
  if constexpr (BYTES > 64 * 1024) {
    static TdvcPerDeviceFlag attr_flags;
    bool& attr_done = attr_flags.flag();
    if (!attr_done) {
      const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
      TDVC_CHECK(err == hipSuccess, "tdvc_dcn_fused: cannot reserve %d bytes of LDS: %s", BYTES, hipGetErrorString(err));
      attr_done = true;
    }
  }
  return TDVC_OK;
}

// kernel parameters of a descriptor that dcn_validate (csrc/dcn.hip) has accepted (x_planar is null for fp32 maps)
template <typename T>
DcnParams<T> dcn_params(const tdvc_dcn_desc* d) {
  DcnParams<T> p;
  p.x = reinterpret_cast<const T*>(d->x.p); p.x_sn = d->x.sn; p.x_sp = d->x.sp; p.H = d->x.H; p.W = d->x.W;
  p.om = reinterpret_cast<const T*>(d->om.p); p.om_sn = d->om.sn; p.om_sp = d->om.sp;
  p.y = to_dev(d->y);
  p.w = reinterpret_cast<const T*>(d->w); p.bias = d->bias;
  p.act = d->act; p.slope = d->slope; p.round16 = d->round_before_act;
  p.npix = (long)d->x.H * d->x.W;
  p.xp = reinterpret_cast<const T*>(d->x_planar);
  return p;
}

template <typename T>
int launch_dcn_fused(const tdvc_dcn_desc* d, void* stream) {
  constexpr int LDS = DCN_TPX * DCN_TPY * (3 * DCN_G * 8 * (int)sizeof(T) + 16);      // fp16 25,600 B, fp32 50,176 B
  const DcnParams<T> p = dcn_params<T>(d);
  if (const int e = dcn_reserve_lds<&dcn_fused_kernel<T>, LDS>(); e != TDVC_OK) return e;
  dim3 grid((unsigned)(((d->x.W + DCN_TPX - 1) / DCN_TPX) * ((d->x.H + DCN_TPY - 1) / DCN_TPY)), d->x.N);
  hipLaunchKernelGGL(dcn_fused_kernel<T>, grid, dim3(256), LDS, reinterpret_cast<hipStream_t>(stream), p);
  return tdvc_launch_status(std::is_same_v<T, float> ? "tdvc_dcn_fused(f32)" : "tdvc_dcn_fused");
}

}  // namespace
