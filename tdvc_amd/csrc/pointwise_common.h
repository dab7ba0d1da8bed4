// Helpers shared by the streaming (HBM-bound) kernels: 8-channel accesses on fp16 / fp32 fmaps, 1-D grids.
#pragma once
#include "common.h"

namespace {

constexpr int EW_BLOCK = 256;

__device__ __forceinline__ void load8(const FMap& f, int n, long pix, int c, float v[8]) {
  if (f.f32) {
    const float* p = reinterpret_cast<const float*>(f.p) + (long)n * f.sn + pix * f.sp + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (c + j < f.C) ? p[j] : 0.f;
  } else {
    const half8 h = *reinterpret_cast<const half8*>(reinterpret_cast<const half_t*>(f.p) + (long)n * f.sn + pix * f.sp + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
  }
}
__device__ __forceinline__ void store8(const FMap& f, int n, long pix, int c, const float v[8]) {
  if (f.f32) {
    float* p = reinterpret_cast<float*>(f.p) + (long)n * f.sn + pix * f.sp + c;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c + j < f.C) p[j] = v[j];
  } else {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
    *reinterpret_cast<half8*>(reinterpret_cast<half_t*>(f.p) + (long)n * f.sn + pix * f.sp + c) = h;
  }
}

inline dim3 grid1d(long total, int block = EW_BLOCK) { return dim3((unsigned)((total + block - 1) / block)); }

// ---- the item walk of a 1-D grid.  Work item i is (image n, pixel pix, index i % per_pixel inside the pixel), images outermost.  The
// launcher sizes the grid with the count the kernel bounds itself by; the caller names the chunk count, so C / 8 against (C + 7) / 8
// (fp32 maps with C % 8 != 0) is a choice made at the call site.
template <class M> __host__ __device__ __forceinline__ long pixel_items(const M& f) { return (long)f.N * f.H * f.W; }
template <class M> __host__ __device__ __forceinline__ long chunk_items(const M& f, int chunks) { return pixel_items(f) * chunks; }

struct Item { int n; long pix; int c; bool ok; };      // ok: the item exists; a missing one has n = pix = 0 (a lane may stay alive on it)
__device__ __forceinline__ Item sub_item(const FMap& f, int per_pixel) {      // c = index inside the pixel
  const long npix = (long)f.H * f.W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long t = i / per_pixel;
  Item it;
  it.ok = i < npix * f.N * per_pixel;      // chunk_items(f, per_pixel)
  const long tc = it.ok ? t : 0;
  it.c = (int)(i - t * per_pixel);         // the remainders from their quotients: two 64-bit divisions per item wherever the compiler puts them
  it.n = (int)(tc / npix);
  it.pix = tc - it.n * npix;
  return it;
}
__device__ __forceinline__ Item chunk_item(const FMap& f, int chunks) {       // c = first channel of the 8-channel chunk
  Item it = sub_item(f, chunks);
  it.c *= 8;
  return it;
}
struct PixelItem { int n; long pix; bool ok; };
__device__ __forceinline__ PixelItem pixel_item(const FMap& f) {
  const Item it = sub_item(f, 1);
  return PixelItem{it.n, it.pix, it.ok};
}

// ---- the two-stage channel sum of a 256-thread workgroup over C <= 256 channels (C % 8 == 0).  Stage 1: thread = (pixel lane pl,
// chunk ck) adds its pixels pl, pl + lanes, ... into acc[8] in that order (the caller's loop).  Stage 2: thread c < C adds the
// lanes' values of channel c in lane order.  The SE gate, the bias gradients and the FeatureFix pooling are bit-reproducible
// because of this order.
struct ChanLanes { int chunks, lanes, ck, pl; bool live; };
__device__ __forceinline__ ChanLanes chan_lanes(int C) {
  ChanLanes L;
  L.chunks = C / 8;            // <= 32
  L.lanes = 256 / L.chunks;
  L.ck = threadIdx.x % L.chunks;
  L.pl = threadIdx.x / L.chunks;
  L.live = L.pl < L.lanes;
  return L;
}
__device__ __forceinline__ void chan_lanes_sum(const ChanLanes& L, const float acc[8], int C, float* dst) {      // dst[c], c < C
  __shared__ float red[256][9];
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tid][j] = L.live ? acc[j] : 0.f;
  __syncthreads();
  if (tid < C) {
    const int cc = tid / 8, j = tid % 8;
    float s = 0.f;
    for (int l = 0; l < L.lanes; ++l) s += red[l * L.chunks + cc][j];
    dst[tid] = s;
  }
}
// pixels [p0, p1) of workgroup blockIdx.x when an image's pixels are cut into nblocks equal ranges (the last one shorter or empty)
struct PixRange { long p0, p1; };
__device__ __forceinline__ PixRange block_pixels(const FMap& x, int nblocks) {
  const long npix = (long)x.H * x.W;
  const long per = (npix + nblocks - 1) / nblocks;
  const long p0 = (long)blockIdx.x * per;
  return PixRange{p0, p0 + per < npix ? p0 + per : npix};
}
// partial[(n * nblocks + blk)][c] = sum over the block's pixels, channels c0 .. c0 + 255 of image blockIdx.y: the body of
// channel_sum_kernel (pointwise.hip, C <= 256) and of channel_sum_wide_kernel (backward_ops.hip, 256 channels per blockIdx.z)
__device__ __forceinline__ void channel_sum_block(const FMap& x, float* partial, int nblocks, int c0) {
  const int cw = min(256, x.C - c0);
  const ChanLanes L = chan_lanes(cw);
  const int n = blockIdx.y, lanes = L.lanes;
  const PixRange r = block_pixels(x, nblocks);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (L.live) {
    long pix = r.p0 + L.pl;
    for (; pix + 3 * lanes < r.p1; pix += 4 * lanes) {       // four independent 16-byte loads in flight per thread; summed in pixel order
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) load8(x, n, pix + u * lanes, c0 + L.ck * 8, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[u][j];
    }
    for (; pix < r.p1; pix += lanes) {
      float v[8];
      load8(x, n, pix, c0 + L.ck * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
  chan_lanes_sum(L, acc, cw, partial + ((long)n * nblocks + blockIdx.x) * x.C + c0);
}

// ---- sums over a workgroup: xor-shuffle tree inside each wave, then the waves' values in wave order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float waves_sum(const float* s, int nwaves, int stride = 1) {      // s[w * stride]: wave w's sum
  float t = s[0];
  for (int w = 1; w < nwaves; ++w) t += s[w * stride];
  return t;
}
__device__ __forceinline__ float block_sum(float v, float* sh) {      // 256 threads; every thread gets the sum
  const int tid = threadIdx.x;
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) sh[tid >> 6] = v;
  __syncthreads();
  return waves_sum(sh, 4);
}

// ---- resampling rules: an output coordinate o along one axis reads source samples i0 and i1 with weights 1 - w1 and w1.  A forward
// kernel and its adjoint call the same function, so the adjoint's weights are the forward's, bit for bit.
struct Tap { int i0, i1; float w1; };
// bilinear x2, half-pixel centres (align_corners = False); n source samples
__device__ __forceinline__ Tap tap_half2x(int o, int n) {
  const float s = fmaxf((o + 0.5f) * 0.5f - 0.5f, 0.f);
  const int i0 = (int)s;
  return Tap{i0, i0 + (i0 < n - 1), s - i0};
}
// bilinear to any size, half-pixel centres; r = source size / output size
__device__ __forceinline__ Tap tap_half(int o, float r, int n) {
  const float s = fmaxf(r * (o + 0.5f) - 0.5f, 0.f);
  const int i0 = (int)s < n - 1 ? (int)s : n - 1;
  return Tap{i0, i0 + (i0 < n - 1), s - i0};
}
// bilinear, align_corners = True; r = ac_ratio(source size, output size)
__device__ __forceinline__ float ac_ratio(int n_src, int n_out) { return (n_out > 1) ? (float)(n_src - 1) / (float)(n_out - 1) : 0.f; }
__device__ __forceinline__ Tap tap_ac(int o, float r, int n) {
  const float s = r * o;
  const int i0 = (int)s;
  return Tap{i0, i0 + (i0 < n - 1), s - i0};
}
__device__ __forceinline__ float bilerp(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {      // a b / c d = rows i0 / i1
  const float ly1 = ty.w1, lx1 = tx.w1, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}
// the adjoint's view: the weight with which the output coordinate of tap t reads source sample i
__device__ __forceinline__ float tap_weight(const Tap& t, int i) { return (t.i0 == i ? 1.f - t.w1 : 0.f) + (t.i1 == i ? t.w1 : 0.f); }

// One axis of grid_sample(bilinear, border, align_corners=True) at pixel x + flow f of an axis of n samples, through torch's
// normalise / unnormalise round trip: the clamped position, its two samples with their bounds tests, and d pos / d f (0 where the
// position was clamped: torch's clip_coordinates_set_grad).
struct WarpAxis { float pos; int i0, i1; bool ok0, ok1; float dpos; };
__device__ __forceinline__ WarpAxis warp_border_axis(int x, float f, int n) {
  const float g = (float)x + f;
  const float m = (float)(n - 1 > 1 ? n - 1 : 1);
  const float nrm = 2.0f * g / m - 1.0f;
  float p = ((nrm + 1.f) / 2.f) * (float)(n - 1);
  WarpAxis a;
  a.dpos = (p >= 0.f && p <= (float)(n - 1)) ? (float)(n - 1) / m : 0.f;
  p = fminf((float)(n - 1), fmaxf(p, 0.f));
  a.pos = p;
  a.i0 = (int)floorf(p);
  a.i1 = a.i0 + 1;
  a.ok0 = a.i0 >= 0 && a.i0 < n;
  a.ok1 = a.i1 >= 0 && a.i1 < n;
  return a;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- factorised-prior logits (compressai EntropyBottleneck._logits_cumulative, filters (3,3,3,3)), packed parameters
constexpr int EB_NP = 59;   // floats per channel: tdvc_eb_pack (backward_ops.hip), or tdvc_amd/model/coder.py::_packed_tensor in torch

__device__ __forceinline__ float eb_logits(const float* P, float v) {
  // filters (1,3,3,3,3,1): m0[3], m1..m3[9], m4[3] | b0..b3[3], b4[1] | f0..f3[3] | median
  const float* m = P;
  const float* b = P + 33;
  const float* f = P + 46;
  float l[3], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    l[i] = m[i] * v + b[i];
    l[i] += f[i] * tanhf(l[i]);
  }
#pragma unroll
  for (int k = 1; k <= 3; ++k) {
    const float* mk = m + 3 + (k - 1) * 9;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      t[i] = mk[i * 3 + 0] * l[0] + mk[i * 3 + 1] * l[1] + mk[i * 3 + 2] * l[2] + b[3 * k + i];
      t[i] += f[3 * k + i] * tanhf(t[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) l[i] = t[i];
  }
  return m[30] * l[0] + m[31] * l[1] + m[32] * l[2] + b[12];
}

inline bool fmap_any(const tdvc_fmap& f) { return f.dtype == TDVC_F32 ? fmap_ok32(f) : fmap_ok16(f); }
inline bool same_geom(const tdvc_fmap& a, const tdvc_fmap& b) { return a.N == b.N && a.H == b.H && a.W == b.W; }
// an fp32 map whose pixels can be moved as one aligned 4-float / 2-float word (the VEC kernels)
inline bool pix16(const tdvc_fmap& f) { return f.C >= 4 && (f.sp % 4) == 0 && (f.sn % 4) == 0 && aligned16(f.p); }
inline bool pix8(const tdvc_fmap& f) { return (f.sp % 2) == 0 && (f.sn % 2) == 0 && (((uintptr_t)f.p) & 7) == 0; }
#define ST(s) reinterpret_cast<hipStream_t>(s)

}  // namespace
