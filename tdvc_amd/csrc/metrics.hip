// Quality metrics of the evaluation loop (tools/predict.py:87-100 in the reference): one level of MS-SSIM
// (main/model/ms_ssim_torch.py:33-83: valid separable Gaussian of X, Y, X^2, Y^2, XY; cs and ssim maps; per-image
// means) and the 2x2 average pooling between levels (:178-180, padding = size % 2, zeros counted).
//
// HBM-bound: one pass reads X and Y once per level (8 B per pixel per channel) -- the reference runs ten depthwise
// convolutions over five full-size fp32 products.  fp32 throughout, like the reference on a float input.
#include <hip/hip_runtime.h>

#include "common.h"
#include "../../include/tdvc_hip.h"

namespace {

constexpr int MS_TW = 32, MS_TH = 16, MS_MAXWIN = 15;

struct SsimLevel {
  const float *x, *y;
  int N, C, H, W, win;
  float taps[MS_MAXWIN];
  float c1, c2;
  int tiles_x, tiles_y;
  float* partial;               // [N][C * tiles][2]  (sum ssim_map, sum cs_map)
};

__global__ __launch_bounds__(256) void ssim_level_kernel(const SsimLevel p) {
  extern __shared__ float sm[];
  const int IW = MS_TW + p.win - 1, IH = MS_TH + p.win - 1;
  float* tx = sm;                         // [IH][IW] X tile
  float* ty = tx + IH * IW;               // [IH][IW] Y tile
  float* hz = ty + IH * IW;               // [5][IH][MS_TW] horizontally filtered X, Y, XX, YY, XY
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int tcol = tile % p.tiles_x, trow = tile / p.tiles_x;
  const int Hv = p.H - p.win + 1, Wv = p.W - p.win + 1;
  const int oy0 = trow * MS_TH, ox0 = tcol * MS_TW;
  const float* xp = p.x + ((long)n * p.C + c) * p.H * p.W;
  const float* yp = p.y + ((long)n * p.C + c) * p.H * p.W;
  for (int i = tid; i < IH * IW; i += 256) {
    const int r = i / IW, q = i - r * IW;
    const int iy = oy0 + r, ix = ox0 + q;
    const bool ok = iy < p.H && ix < p.W;
    tx[i] = ok ? xp[(long)iy * p.W + ix] : 0.f;
    ty[i] = ok ? yp[(long)iy * p.W + ix] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < IH * MS_TW; i += 256) {
    const int r = i / MS_TW, q = i - r * MS_TW;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
    for (int k = 0; k < p.win; ++k) {
      const float w = p.taps[k], u = tx[r * IW + q + k], v = ty[r * IW + q + k];
      a += w * u; b += w * v; aa += w * (u * u); bb += w * (v * v); ab += w * (u * v);
    }
    hz[i] = a; hz[IH * MS_TW + i] = b; hz[2 * IH * MS_TW + i] = aa; hz[3 * IH * MS_TW + i] = bb; hz[4 * IH * MS_TW + i] = ab;
  }
  __syncthreads();
  float s_ssim = 0.f, s_cs = 0.f;
  for (int i = tid; i < MS_TH * MS_TW; i += 256) {
    const int r = i / MS_TW, q = i - r * MS_TW;
    if (oy0 + r >= Hv || ox0 + q >= Wv) continue;
    float mu1 = 0.f, mu2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
    for (int k = 0; k < p.win; ++k) {
      const float w = p.taps[k];
      const int o = (r + k) * MS_TW + q;
      mu1 += w * hz[o]; mu2 += w * hz[IH * MS_TW + o]; xx += w * hz[2 * IH * MS_TW + o]; yy += w * hz[3 * IH * MS_TW + o];
      xy += w * hz[4 * IH * MS_TW + o];
    }
    const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
    const float s1 = xx - mu1s, s2 = yy - mu2s, s12 = xy - mu12;
    const float cs = (2.f * s12 + p.c2) / (s1 + s2 + p.c2);
    s_cs += cs;
    s_ssim += ((2.f * mu12 + p.c1) / (mu1s + mu2s + p.c1)) * cs;
  }
  // block sum in a fixed order: lanes by shuffle, waves through LDS
  for (int o = 32; o > 0; o >>= 1) {
    s_ssim += __shfl_down(s_ssim, o);
    s_cs += __shfl_down(s_cs, o);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s_ssim; red[1][tid >> 6] = s_cs; }
  __syncthreads();
  if (tid == 0) {
    float* o = p.partial + (((long)n * p.C + c) * (p.tiles_x * p.tiles_y) + tile) * 2;
    o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// out[n] = sum over the image's partials / count, fixed order (one workgroup per image, double accumulation)
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const float* partial, int per_image, double inv_count, float* ssim, float* cs) {
  __shared__ double red[2][256];
  const int n = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = tid; i < per_image; i += 256) {
    a += (double)partial[((long)n * per_image + i) * 2];
    b += (double)partial[((long)n * per_image + i) * 2 + 1];
  }
  red[0][tid] = a; red[1][tid] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { ssim[n] = (float)(red[0][0] * inv_count); cs[n] = (float)(red[1][0] * inv_count); }
}

// F.avg_pool2d(x, kernel_size=2, padding=(H % 2, W % 2)): stride 2, zeros of the padding counted (divisor 4)
__global__ void avgpool2_pad_kernel(const float* x, long planes, int H, int W, int ph, int pw, int Ho, int Wo, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * Ho * Wo) return;
  const int ox = (int)(i % Wo);
  const long q = i / Wo;
  const int oy = (int)(q % Ho);
  const long pl = q / Ho;
  const float* xp = x + pl * H * W;
  float s = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int iy = 2 * oy - ph + dy, ix = 2 * ox - pw + dx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += xp[(long)iy * W + ix];
    }
  out[i] = 0.25f * s;
}

// ---------------------------------------------------------------------------------------------------- backward of one level
// d(g_ssim[n] * mean ssim_map + g_cs[n] * mean cs_map) / dX, Y constant (the maps are symmetric: dY = the same kernel with the
// operands swapped).  A gather: one workgroup per 32x16 tile of dX.  With R = win - 1 it loads X, Y on the tile + 2R apron,
// recomputes the five filtered statistics on the tile + R apron (every map position whose window covers a tile pixel), turns
// them into the three partial-derivative maps
//   P_mu = a cs (2 mu2 - 2 mu1 l) / B1 + k (2 mu1 cs - 2 mu2) / B2,   P_xx = -k cs / B2,   P_xy = 2 k / B2       (k = a l + b)
// (zero outside the valid map) and filters those back with the transposed window:
//   dX(q) = scale * sum_p w(q - p) [P_mu(p) + 2 X(q) P_xx(p) + Y(q) P_xy(p)]  +  0.25 g_pool((q + pad) / 2)
// the last term being the backward of the padded 2x2 average pooling towards the next (coarser) level.  No atomics, fixed
// summation order.  LDS at win = 11: X, Y 2 x 36x52, horizontal statistics 5 x 36x42 (re-used by the 3 x 16x42 vertically
// back-filtered maps), P maps 3 x 26x42: 57.3 KB, two workgroups per CU.
struct SsimLevelBwd {
  const float *x, *y, *g_ssim, *g_cs, *g_pool;
  float* dx;
  int N, C, H, W, win;
  float taps[MS_MAXWIN];
  float c1, c2, scale, inv_m;
  int tiles_x, Hp, Wp;
};

__global__ __launch_bounds__(256) void ssim_level_backward_kernel(const SsimLevelBwd p) {
  extern __shared__ float sm[];
  const int R = p.win - 1;
  const int IW = MS_TW + 2 * R, IH = MS_TH + 2 * R, PW = MS_TW + R, PH = MS_TH + R;
  float* tx = sm;                         // [IH][IW] X tile, origin (qy0 - R, qx0 - R)
  float* ty = tx + IH * IW;               // [IH][IW] Y tile
  float* hz = ty + IH * IW;               // [5][IH][PW] horizontally filtered X, Y, XX, YY, XY; later [3][MS_TH][PW] (vt)
  float* pm = hz + 5 * IH * PW;           // [3][PH][PW] P_mu, P_xx, P_xy, origin (qy0 - R, qx0 - R) in map coordinates
  float* vt = hz;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int tcol = tile % p.tiles_x, trow = tile / p.tiles_x;
  const int Hv = p.H - R, Wv = p.W - R;
  const int qy0 = trow * MS_TH, qx0 = tcol * MS_TW;
  const long plane = ((long)n * p.C + c) * p.H * p.W;
  const float* xp = p.x + plane;
  const float* yp = p.y + plane;
  for (int i = tid; i < IH * IW; i += 256) {
    const int r = i / IW, q = i - r * IW;
    const int iy = qy0 - R + r, ix = qx0 - R + q;
    const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    tx[i] = ok ? xp[(long)iy * p.W + ix] : 0.f;
    ty[i] = ok ? yp[(long)iy * p.W + ix] : 0.f;
  }
  __syncthreads();
  const int HS = IH * PW;
  for (int i = tid; i < HS; i += 256) {
    const int r = i / PW, q = i - r * PW;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
    for (int k = 0; k < p.win; ++k) {
      const float w = p.taps[k], u = tx[r * IW + q + k], v = ty[r * IW + q + k];
      a += w * u; b += w * v; aa += w * (u * u); bb += w * (v * v); ab += w * (u * v);
    }
    hz[i] = a; hz[HS + i] = b; hz[2 * HS + i] = aa; hz[3 * HS + i] = bb; hz[4 * HS + i] = ab;
  }
  __syncthreads();
  const float ga = p.g_ssim[n] * p.inv_m, gb = p.g_cs[n] * p.inv_m;
  const int PS = PH * PW;
  for (int i = tid; i < PS; i += 256) {
    const int r = i / PW, q = i - r * PW;
    const int py = qy0 - R + r, px = qx0 - R + q;
    float pmu = 0.f, pxx = 0.f, pxy = 0.f;
    if (py >= 0 && py < Hv && px >= 0 && px < Wv) {
      float mu1 = 0.f, mu2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
      for (int k = 0; k < p.win; ++k) {
        const float w = p.taps[k];
        const int o = (r + k) * PW + q;
        mu1 += w * hz[o]; mu2 += w * hz[HS + o]; xx += w * hz[2 * HS + o]; yy += w * hz[3 * HS + o]; xy += w * hz[4 * HS + o];
      }
      const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
      const float s1 = xx - mu1s, s2 = yy - mu2s, s12 = xy - mu12;
      const float rb1 = 1.f / (mu1s + mu2s + p.c1), rb2 = 1.f / (s1 + s2 + p.c2);
      const float l = (2.f * mu12 + p.c1) * rb1, cs = (2.f * s12 + p.c2) * rb2;
      const float k = ga * l + gb;
      pmu = ga * cs * (2.f * mu2 - 2.f * mu1 * l) * rb1 + k * (2.f * mu1 * cs - 2.f * mu2) * rb2;
      pxx = -k * cs * rb2;
      pxy = 2.f * k * rb2;
    }
    pm[i] = pmu; pm[PS + i] = pxx; pm[2 * PS + i] = pxy;
  }
  __syncthreads();                        // every read of hz is done: vt may overwrite it
  const int VS = MS_TH * PW;
  for (int i = tid; i < VS; i += 256) {
    const int r = i / PW, q = i - r * PW;
    float a = 0.f, b = 0.f, d = 0.f;
    for (int k = 0; k < p.win; ++k) {     // map row qy - k  ->  local row r + R - k
      const float w = p.taps[k];
      const int o = (r + R - k) * PW + q;
      a += w * pm[o]; b += w * pm[PS + o]; d += w * pm[2 * PS + o];
    }
    vt[i] = a; vt[VS + i] = b; vt[2 * VS + i] = d;
  }
  __syncthreads();
  const int ph = p.H & 1, pw = p.W & 1;
  for (int i = tid; i < MS_TH * MS_TW; i += 256) {
    const int r = i / MS_TW, q = i - r * MS_TW;
    const int qy = qy0 + r, qx = qx0 + q;
    if (qy >= p.H || qx >= p.W) continue;
    float a = 0.f, b = 0.f, d = 0.f;
    for (int k = 0; k < p.win; ++k) {     // map column qx - k  ->  local column q + R - k
      const float w = p.taps[k];
      const int o = r * PW + q + R - k;
      a += w * vt[o]; b += w * vt[VS + o]; d += w * vt[2 * VS + o];
    }
    const int t = (r + R) * IW + q + R;
    float g = p.scale * (a + 2.f * tx[t] * b + ty[t] * d);
    if (p.g_pool) {
      const long pp = ((long)n * p.C + c) * p.Hp * p.Wp;
      g += 0.25f * p.g_pool[pp + (long)((qy + ph) >> 1) * p.Wp + ((qx + pw) >> 1)];
    }
    p.dx[plane + (long)qy * p.W + qx] = g;
  }
}

// The scalar tail of MS-SSIM and its gradient (ms_ssim_torch.py:183-188), one thread per image:
//   ms[n] = prod_{l < L-1} cs_l^w_l * ssim^w_{L-1}      (the reference multiplies the ssim factor into every one of the L-1 terms)
// and, for an upstream gradient go[n] of ms[n], the gradients of the loss with respect to every level's RAW means (the
// inputs here are the means after (v + 1) / 2, hence the 1/2):  g_cs[l][n] = go w_l ms / (2 cs_l) for l < L-1,
// g_ssim[L-1][n] = go (L-1) w_{L-1} ms / (2 ssim); every other entry is zero.
struct MsssimGrads {
  const float *cs, *ssim, *grad_out;
  float *ms, *g_ssim, *g_cs;
  int L, N;
  float w[TDVC_MSSSIM_MAX_LEVELS];
};

__global__ __launch_bounds__(256) void msssim_level_grads_kernel(const MsssimGrads p) {
  for (int n = threadIdx.x; n < p.N; n += 256) {
    const int last = p.L - 1;
    const float s = p.ssim[n], ps = powf(s, p.w[last]);
    float ms = 1.f;
    for (int l = 0; l < last; ++l) ms *= powf(p.cs[(long)l * p.N + n], p.w[l]) * ps;
    const float go = p.grad_out ? p.grad_out[n] : 1.f;
    for (int l = 0; l < p.L; ++l) {
      p.g_ssim[(long)l * p.N + n] = 0.f;
      p.g_cs[(long)l * p.N + n] = l < last ? go * (0.5f * p.w[l] * ms / p.cs[(long)l * p.N + n]) : 0.f;
    }
    p.g_ssim[(long)last * p.N + n] = go * (0.5f * (float)last * p.w[last] * ms / s);
    p.ms[n] = ms;
  }
}

}  // namespace

extern "C" int64_t tdvc_ssim_level_work_floats(int N, int C, int H, int W, int win) {
  if (N <= 0 || C <= 0 || win < 1 || win > MS_MAXWIN || (win & 1) == 0 || H < win || W < win) return TDVC_EINVAL;
  const int tiles_x = (W - win + 1 + MS_TW - 1) / MS_TW, tiles_y = (H - win + 1 + MS_TH - 1) / MS_TH;
  return (int64_t)N * C * tiles_x * tiles_y * 2;
}

extern "C" int tdvc_ssim_level(const float* x, const float* y, int N, int C, int H, int W, const float* win, int win_size,
                               float c1, float c2, float* ssim_out, float* cs_out, float* work, int64_t work_floats, void* stream) {
  TDVC_CHECK(x && y && win && ssim_out && cs_out && work, "tdvc_ssim_level: null pointer");
  const int64_t need = tdvc_ssim_level_work_floats(N, C, H, W, win_size);
  TDVC_CHECK(need > 0, "tdvc_ssim_level: bad geometry (N %d C %d H %d W %d window %d: odd window <= %d, image >= window)", N, C, H, W, win_size, MS_MAXWIN);
  TDVC_CHECK(work_floats >= need, "tdvc_ssim_level: workspace too small");
  TDVC_CHECK(N <= 65535 && C <= 65535, "tdvc_ssim_level: too many images / channels for one launch");
  SsimLevel p;
  p.x = x; p.y = y; p.N = N; p.C = C; p.H = H; p.W = W; p.win = win_size;
  for (int k = 0; k < MS_MAXWIN; ++k) p.taps[k] = k < win_size ? win[k] : 0.f;        // `win` is HOST memory (the 1-D kernel)
  p.c1 = c1; p.c2 = c2;
  p.tiles_x = (W - win_size + 1 + MS_TW - 1) / MS_TW; p.tiles_y = (H - win_size + 1 + MS_TH - 1) / MS_TH;
  p.partial = work;
  const int IW = MS_TW + win_size - 1, IH = MS_TH + win_size - 1;
  const size_t lds = sizeof(float) * ((size_t)2 * IH * IW + (size_t)5 * IH * MS_TW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssim_level_kernel, dim3(p.tiles_x * p.tiles_y, C, N), dim3(256), lds, st, p);
  const int per_image = C * p.tiles_x * p.tiles_y;
  const double inv = 1.0 / ((double)C * (H - win_size + 1) * (W - win_size + 1));
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3(N), dim3(256), 0, st, work, per_image, inv, ssim_out, cs_out);
  return tdvc_launch_status("tdvc_ssim_level");
}

extern "C" int tdvc_avgpool2_pad_f32(const float* x, int64_t planes, int H, int W, float* out, void* stream) {
  TDVC_CHECK(x && out && planes > 0 && H > 0 && W > 0, "tdvc_avgpool2_pad_f32: bad arguments");
  const int ph = H % 2, pw = W % 2;
  const int Ho = (H + 2 * ph - 2) / 2 + 1, Wo = (W + 2 * pw - 2) / 2 + 1;
  const long total = planes * Ho * Wo;
  hipLaunchKernelGGL(avgpool2_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, (long)planes,
                     H, W, ph, pw, Ho, Wo, out);
  return tdvc_launch_status("tdvc_avgpool2_pad_f32");
}

extern "C" int tdvc_ssim_level_backward(const float* x, const float* y, int N, int C, int H, int W, const float* win, int win_size,
                                        float c1, float c2, const float* g_ssim, const float* g_cs, float scale, const float* g_pool,
                                        float* dx, void* stream) {
  TDVC_CHECK(x && y && win && g_ssim && g_cs && dx, "tdvc_ssim_level_backward: null pointer");
  TDVC_CHECK(N > 0 && C > 0 && win_size >= 1 && win_size <= MS_MAXWIN && (win_size & 1) == 1 && H >= win_size && W >= win_size,
             "tdvc_ssim_level_backward: bad geometry (N %d C %d H %d W %d window %d: odd window <= %d, image >= window)", N, C, H, W, win_size, MS_MAXWIN);
  TDVC_CHECK(N <= 65535 && C <= 65535, "tdvc_ssim_level_backward: too many images / channels for one launch");
  SsimLevelBwd p;
  p.x = x; p.y = y; p.g_ssim = g_ssim; p.g_cs = g_cs; p.g_pool = g_pool; p.dx = dx;
  p.N = N; p.C = C; p.H = H; p.W = W; p.win = win_size;
  for (int k = 0; k < MS_MAXWIN; ++k) p.taps[k] = k < win_size ? win[k] : 0.f;        // `win` is HOST memory (the 1-D kernel)
  p.c1 = c1; p.c2 = c2; p.scale = scale;
  p.inv_m = (float)(1.0 / ((double)C * (H - win_size + 1) * (W - win_size + 1)));
  p.tiles_x = (W + MS_TW - 1) / MS_TW;
  const int tiles_y = (H + MS_TH - 1) / MS_TH;
  p.Hp = (H + 2 * (H % 2) - 2) / 2 + 1; p.Wp = (W + 2 * (W % 2) - 2) / 2 + 1;
  const int R = win_size - 1, IW = MS_TW + 2 * R, IH = MS_TH + 2 * R, PW = MS_TW + R, PH = MS_TH + R;
  const size_t lds = sizeof(float) * ((size_t)2 * IH * IW + (size_t)5 * IH * PW + (size_t)3 * PH * PW);
  static TdvcPerDeviceFlag attr;
  if (!attr.flag()) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&ssim_level_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    if (err != hipSuccess) { tdvc_set_error("tdvc_ssim_level_backward: hipFuncSetAttribute failed: %s", hipGetErrorString(err)); return (int)err; }
    attr.flag() = true;
  }
  TDVC_CHECK(lds <= 96 * 1024, "tdvc_ssim_level_backward: LDS plan %zu bytes too large", lds);
  hipLaunchKernelGGL(ssim_level_backward_kernel, dim3(p.tiles_x * tiles_y, C, N), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), p);
  return tdvc_launch_status("tdvc_ssim_level_backward");
}

extern "C" int tdvc_msssim_level_grads(const float* cs, const float* ssim_last, const float* weights, int levels, int N, const float* grad_out,
                                       float* ms_out, float* g_ssim, float* g_cs, void* stream) {
  TDVC_CHECK(cs && ssim_last && weights && ms_out && g_ssim && g_cs, "tdvc_msssim_level_grads: null pointer");
  TDVC_CHECK(levels >= 1 && levels <= TDVC_MSSSIM_MAX_LEVELS && N > 0, "tdvc_msssim_level_grads: bad geometry (levels %d of at most %d, N %d)", levels,
             TDVC_MSSSIM_MAX_LEVELS, N);
  MsssimGrads p;
  p.cs = cs; p.ssim = ssim_last; p.grad_out = grad_out; p.ms = ms_out; p.g_ssim = g_ssim; p.g_cs = g_cs; p.L = levels; p.N = N;
  for (int l = 0; l < TDVC_MSSSIM_MAX_LEVELS; ++l) p.w[l] = l < levels ? weights[l] : 0.f;      // `weights` is HOST memory
  hipLaunchKernelGGL(msssim_level_grads_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return tdvc_launch_status("tdvc_msssim_level_grads");
}
