// dcn_f32 — tdvc_dcn_fused on fp32 maps: the deformable conv of the whole-model fp32 mode (`enable_amp: False` of the reference,
// VideoCompressor.model_fp32).  The operator and geometry of dcn_fused_kernel (csrc/dcn.hip): 8 groups x 8 channels, 3x3, stride 1,
// pad 1, 64 -> 64, channel windows and arbitrary batch / pixel strides -- with nothing rounded to fp16 before the epilogue:
//   * x, offsets and mask logits are fp32; a sampling position is base + offset in fp32;
//   * the sampling rule is sample8_bf's: open-interval inside test, a clamp before floorf (an infinite or huge offset lies outside
//     and contributes zero, never NaN), clamped addresses with zeroed weights, no branch around a load;
//   * the mask is 1 / (1 + expf(-logit)) with a true division (logits +-60000 give exactly 1 and 0, logit 0 exactly 0.5), folded into
//     the four fp32 corner weights;
//   * the modulated samples of an 8x8 pixel tile go to an fp32 LDS column tile, one kernel row (three taps) at a time, and are
//     contracted on v_mfma_f32_32x32x2_f32 with the fp32 weight packing (tdvc_pack_conv_weights_indexed_f32, ck = 64, 9 taps);
//   * epilogue: + bias, one rounding to fp16 if round_before_act (the reference's `.half()`), the activation in fp32, an fp32 store or
//     an fp16 store with one more rounding.
// k order of a pixel's sum: tap 0..8 (row-major), inside a tap the group pairs (0,1), (2,3), (4,5), (6,7), inside
// a pair channel j = 0..7, and inside one MFMA the even group before the odd one.  It depends on nothing but the operator: not on the
// tile walk, the map size or the batch.
// One kernel for every map size (this mode is bound by the fp32 matrix pipe: 288 MFMAs of 64 cycles per wave and tile).
#include "common.h"

namespace {

constexpr int DF_TPX = 8, DF_TPY = 8, DF_G = 8;
constexpr int DF_PS = 3 * DF_G * 8 * 4 + 16;          // LDS bytes per pixel: 3 taps x 64 floats + 16 (16-byte reads of 32 pixels spread over the banks)
constexpr int DF_LDS = DF_TPX * DF_TPY * DF_PS;      // 50,176 B

struct DcnF32FusedParams {
  const float* x; long x_sn; int x_sp; int H, W;
  const float* om; long om_sn; int om_sp;
  FMap y;
  const float* w; const float* bias;
  int act; float slope; int round16;
};

struct DfSample { f32x4 lo, hi; };

// sample8_bf (csrc/dcn.hip) on an fp32 map, the result kept in fp32
__device__ __forceinline__ DfSample df_sample8(const float* xg, int H, int W, int sp, float h_im, float w_im, float mask) {
  const bool inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  const float hc = fminf(fmaxf(h_im, -2.f), (float)H + 1.f), wc = fminf(fmaxf(w_im, -2.f), (float)W + 1.f);
  const float hf = floorf(hc), wf = floorf(wc);
  const int h_low = (int)hf, w_low = (int)wf, h_high = h_low + 1, w_high = w_low + 1;
  const float lh = hc - hf, lw = wc - wf, hh = 1.f - lh, hw = 1.f - lw;
  const bool hl = h_low >= 0 && h_low <= H - 1, hhg = h_high >= 0 && h_high <= H - 1;
  const bool wl = w_low >= 0 && w_low <= W - 1, whg = w_high >= 0 && w_high <= W - 1;
  const float w1 = (inside && hl && wl) ? hh * hw * mask : 0.f, w2 = (inside && hl && whg) ? hh * lw * mask : 0.f;
  const float w3 = (inside && hhg && wl) ? lh * hw * mask : 0.f, w4 = (inside && hhg && whg) ? lh * lw * mask : 0.f;
  const int y0 = min(max(h_low, 0), H - 1), y1 = min(max(h_high, 0), H - 1);
  const int x0 = min(max(w_low, 0), W - 1), x1 = min(max(w_high, 0), W - 1);
  const int r0 = y0 * W, r1 = y1 * W;                     // pixel indices fit 32 bits (checked by the host)
  const float* p1 = xg + (long)(r0 + x0) * sp;
  const float* p2 = xg + (long)(r0 + x1) * sp;
  const float* p3 = xg + (long)(r1 + x0) * sp;
  const float* p4 = xg + (long)(r1 + x1) * sp;
  const f32x4 a1 = *reinterpret_cast<const f32x4*>(p1), b1 = *reinterpret_cast<const f32x4*>(p1 + 4);
  const f32x4 a2 = *reinterpret_cast<const f32x4*>(p2), b2 = *reinterpret_cast<const f32x4*>(p2 + 4);
  const f32x4 a3 = *reinterpret_cast<const f32x4*>(p3), b3 = *reinterpret_cast<const f32x4*>(p3 + 4);
  const f32x4 a4 = *reinterpret_cast<const f32x4*>(p4), b4 = *reinterpret_cast<const f32x4*>(p4 + 4);
  DfSample o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o.lo[j] = __builtin_fmaf(w1, a1[j], __builtin_fmaf(w2, a2[j], __builtin_fmaf(w3, a3[j], w4 * a4[j])));
    o.hi[j] = __builtin_fmaf(w1, b1[j], __builtin_fmaf(w2, b2[j], __builtin_fmaf(w3, b3[j], w4 * b4[j])));
  }
  return o;
}

// One 256-thread workgroup = an 8x8 pixel tile x all 64 output channels.
//   sampling phase: thread (pixel = tid>>3 [+32], group = tid&7), as in dcn_fused_kernel;
//   matrix phase: wave (mt, nt) multiplies the 32-row weight tile mt with the 32-pixel half nt; lane (r, hh) supplies A[r][hh] and
//     B[hh][r]: k-step (tap, s2) is eight MFMAs, MFMA j contracting channel j of groups 2 s2 (hh = 0) and 2 s2 + 1 (hh = 1).
__global__ __launch_bounds__(256) void dcn_f32_fused_kernel(const DcnF32FusedParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char col[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, r = lane & 31;
  const int mt = wave & 1, nt = wave >> 1;
  const int tiles_x = (p.W + DF_TPX - 1) / DF_TPX;
  const int tile_id = tdvc_xcd_tile(blockIdx.x);
  const int tx = tile_id % tiles_x, ty = tile_id / tiles_x;
  const int n = blockIdx.y;
  const int g = tid & 7;
  const float* xg = p.x + (long)n * p.x_sn + g * 8;

  int soy[2], sox[2];
  float offy[2][9], offx[2][9], msk[2][9];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int pl = (tid >> 3) + 32 * ps;
    soy[ps] = ty * DF_TPY + (pl >> 3);
    sox[ps] = tx * DF_TPX + (pl & 7);
    const int cy = min(soy[ps], p.H - 1), cx = min(sox[ps], p.W - 1);     // an overhanging pixel samples for its clamped twin; never stored
    const float* omp = p.om + (long)n * p.om_sn + ((long)cy * p.W + cx) * p.om_sp;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      offy[ps][t] = omp[g * 18 + 2 * t];
      offx[ps][t] = omp[g * 18 + 2 * t + 1];
      msk[ps][t] = 1.f / (1.f + expf(-omp[18 * DF_G + g * 9 + t]));       // sigmoid (dcn_v2_amp.py: mask = sigmoid(mask)), true division
    }
  }

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const float* wbase = p.w + ((long)mt * 36 * 64 + lane) * 8;            // [cout tile 2][step 36][lane 64][8 floats]
  const unsigned char* bcol = col + (nt * 32 + r) * DF_PS + hh * 32;

#pragma unroll
  for (int chunk = 0; chunk < 3; ++chunk) {             // fully unrolled: tap registers are selected at compile time
    if (chunk > 0) __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
      for (int tc = 0; tc < 3; ++tc) {
        const float h_im = (float)(soy[ps] - 1 + chunk) + offy[ps][chunk * 3 + tc];      // tap = chunk*3 + tc: dy = chunk, dx = tc
        const float w_im = (float)(sox[ps] - 1 + tc) + offx[ps][chunk * 3 + tc];
        const DfSample v = df_sample8(xg, p.H, p.W, p.x_sp, h_im, w_im, msk[ps][chunk * 3 + tc]);
        const int pl = (tid >> 3) + 32 * ps;
        unsigned char* dst = col + pl * DF_PS + tc * (DF_G * 32) + g * 32;
        *reinterpret_cast<f32x4*>(dst) = v.lo;
        *reinterpret_cast<f32x4*>(dst + 16) = v.hi;
      }
    }
    __syncthreads();
#pragma unroll
    for (int tc = 0; tc < 3; ++tc) {
#pragma unroll
      for (int s2 = 0; s2 < DF_G / 2; ++s2) {
        const float* ap = wbase + (long)((chunk * 3 + tc) * (DF_G / 2) + s2) * 512;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
        const unsigned char* bp = bcol + tc * (DF_G * 32) + s2 * 64;
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc, 0, 0, 0);
      }
    }
  }

  const int pl = nt * 32 + r;
  const int oy = ty * DF_TPY + (pl >> 3), ox = tx * DF_TPX + (pl & 7);
  if (oy >= p.H || ox >= p.W) return;
  const long yoff = (long)n * p.y.sn + ((long)oy * p.W + ox) * p.y.sp;
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const int co = mt * 32 + 8 * gq + 4 * hh;
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + co);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[4 * gq + i] + b4[i];
      if (p.round16) v = (float)(half_t)v;
      o[i] = act_apply(v, p.act, p.slope);
    }
    if (p.y.f32) {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y.p) + yoff + co) = o;
    } else {
      half4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = (half_t)o[i];
      *reinterpret_cast<half4*>(reinterpret_cast<half_t*>(p.y.p) + yoff + co) = h;
    }
  }
}

// an fp32 map the kernel reads or writes with 16-byte accesses
inline bool df_map_ok(const tdvc_fmap& f) { return fmap_ok32(f) && aligned16(f.p) && (f.sp % 4) == 0 && (f.sn % 4) == 0; }

}  // namespace

// tdvc_dcn_fused forwards here when d->x.dtype == TDVC_F32 (csrc/dcn.hip); every check runs before anything touches the device
int tdvc_dcn_fused_f32(const tdvc_dcn_desc* d, void* stream) {
  TDVC_CHECK(d, "tdvc_dcn_fused: null descriptor");
  TDVC_CHECK(df_map_ok(d->x), "tdvc_dcn_fused(f32): x must be an fp32 fmap, 16-byte aligned, pixel and batch strides %% 4");
  TDVC_CHECK(d->om.dtype == TDVC_F32 && df_map_ok(d->om), "tdvc_dcn_fused(f32): with an fp32 x the offset/mask fmap must be fp32 too (16-byte aligned, strides %% 4)");
  TDVC_CHECK(d->y.dtype == TDVC_F32 ? df_map_ok(d->y) : fmap_ok16(d->y), "tdvc_dcn_fused(f32): y must be an fp32 (16-byte aligned, strides %% 4) or fp16 fmap");
  TDVC_CHECK(!d->x_planar, "tdvc_dcn_fused(f32): x_planar is an fp16 form; it must be NULL for fp32 maps");
  const int G = d->groups;
  TDVC_CHECK(G == DF_G, "tdvc_dcn_fused(f32): groups=%d unsupported (8 groups x 8 channels)", G);
  TDVC_CHECK(d->x.C == 8 * G && d->y.C == 8 * G, "tdvc_dcn_fused(f32): needs Cin = Cout = 8*groups (8 channels per group)");
  TDVC_CHECK(d->om.C >= 27 * G, "tdvc_dcn_fused(f32): offset/mask fmap needs >= 27*groups channels");
  TDVC_CHECK(d->x.N == d->y.N && d->x.N == d->om.N && d->x.H == d->y.H && d->x.W == d->y.W && d->om.H == d->x.H && d->om.W == d->x.W,
             "tdvc_dcn_fused(f32): geometry mismatch");
  TDVC_CHECK(d->w && aligned16(d->w) && d->bias && aligned16(d->bias), "tdvc_dcn_fused(f32): weights/bias null or unaligned");
  TDVC_CHECK((long)d->x.H * d->x.W < 2147483647L, "tdvc_dcn_fused(f32): image too large (pixel indices are 32-bit)");
  TDVC_CHECK(d->x.N <= 65535, "tdvc_dcn_fused(f32): batch too large");
  DcnF32FusedParams p;
  p.x = reinterpret_cast<const float*>(d->x.p); p.x_sn = d->x.sn; p.x_sp = d->x.sp; p.H = d->x.H; p.W = d->x.W;
  p.om = reinterpret_cast<const float*>(d->om.p); p.om_sn = d->om.sn; p.om_sp = d->om.sp;
  p.y = to_dev(d->y);
  p.w = reinterpret_cast<const float*>(d->w); p.bias = d->bias;
  p.act = d->act; p.slope = d->slope; p.round16 = d->round_before_act;
  static TdvcPerDeviceFlag attr_flags;
  bool& attr_done = attr_flags.flag();
  if (!attr_done) {
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&dcn_f32_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DF_LDS);
    TDVC_CHECK(err == hipSuccess, "tdvc_dcn_fused(f32): cannot reserve %d bytes of LDS: %s", DF_LDS, hipGetErrorString(err));
    attr_done = true;
  }
  dim3 grid((unsigned)(((d->x.W + DF_TPX - 1) / DF_TPX) * ((d->x.H + DF_TPY - 1) / DF_TPY)), d->x.N);
  hipLaunchKernelGGL(dcn_f32_fused_kernel, grid, dim3(256), DF_LDS, reinterpret_cast<hipStream_t>(stream), p);
  return tdvc_launch_status("tdvc_dcn_fused(f32)");
}
