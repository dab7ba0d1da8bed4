// Implicit-GEMM convolution on MFMA for gfx950 — the conv analysis/synthesis transforms,
// feature extractors, SPyNet 7x7 stacks, masked context conv, GDN norm pools (SURVEY §8 a2-a9,
// a13-a15).  fp16 NHWC in, fp32 accumulate, fused epilogue.
//
//   D[cout][pixel] = sum_{tap, cin} W[cout][tap][cin] * X[pixel + tap][cin]
//
// MFMA roles: A = weights (rows = cout), B = activations (cols = pixels), so that a lane's 16
// accumulator registers hold 4 groups of 4 CONSECUTIVE output channels of ONE pixel -> 8-byte
// NHWC stores (v_mfma_f32_32x32x16_f16: C/D col = lane&31, row = (reg&3)+8*(reg>>2)+4*(lane>>5)).
//
// Work decomposition: one 256-thread workgroup (4 waves) = 8x32 output pixels x (MT*32) output
// channels; wave w owns output rows 2w, 2w+1.  The input halo tile of one channel chunk (CK
// channels) is staged once in LDS and re-read by every tap (9x / 25x / 49x reuse); LDS pixel
// stride is CK*2+16 bytes so that the 16-lane groups of ds_read_b128 hit 16 distinct 16-byte
// slots (conflict-free).  Stride-2 convs de-interleave columns by parity while staging so the
// same holds.  Weights are pre-packed on the host in MFMA fragment order: one wave-wide 1 KiB
// coalesced global_load_dwordx4 per fragment, served from L2 (a layer's weights are <= 0.6 MB).
#include "conv_common.h"

using convk::ConvParams;

namespace {

constexpr int TH = 8, TW = 32;

// LEAN (MT == 2 only, chosen on the host from ConvParams::simple == 2): the instantiation carries ONLY the lean
// transposed epilogue -- with both epilogue forms and the per-register fallback inlined the MT = 2 kernels sat at 256
// VGPRs (two workgroups per CU); the first layers (3x3 8->64 at 1080p, four per frame) are latency-bound there.
template <int CK8, int MT, int STRIDE, bool LEAN = false>
__global__ __launch_bounds__(256, LEAN ? 3 : 1) void conv_mfma_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CK = CK8 * 8;
  constexpr int PS = (CK8 == 1) ? 16 : CK * 2 + 16;  // LDS bytes per staged pixel
  int* tapoff = reinterpret_cast<int*>(smem);          // [49], first 256 bytes
  unsigned char* tile = smem + 256;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, r = lane & 31;
  const int tile_id = convk::block_tile(p);
  const int tx = tile_id % p.tiles_x, ty = tile_id / p.tiles_x;
  const int cb = blockIdx.y, n = blockIdx.z;

  const int TIH = (TH - 1) * STRIDE + p.kh;
  const int TIW = (TW - 1) * STRIDE + p.kw;
  const int HALFW = (TIW + 1) >> 1;
  const int TIWp = (STRIDE == 2) ? 2 * HALFW : TIW;

  if (tid < p.ntaps) {
    const int dy = p.tap_dy[tid], dx = p.tap_dx[tid];
    tapoff[tid] = (STRIDE == 2) ? (dy * TIWp + (dx & 1) * HALFW + (dx >> 1)) * PS : (dy * TIWp + dx) * PS;
  }

  int base[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) base[nt] = (((wave * 2 + nt) * STRIDE) * TIWp + r) * PS;

  f32x16 acc[MT][2];
  convk::zero_acc(acc);

  const half_t* xn = p.x + (long)n * p.x_sn;
  const int iy0 = ty * TH * STRIDE - p.pad, ix0 = tx * TW * STRIDE - p.pad;
  const int total = TIH * TIW * CK8;

  for (int ch = 0; ch < p.nchunks; ++ch) {
    if (ch > 0) __syncthreads();
    // ---- stage the halo tile of channels [ch*CK, ch*CK+CK) ------------------------------
    for (int idx = tid; idx < total; idx += 256) {
      const int c8 = idx % CK8;
      const int pix = idx / CK8;
      const int c = pix % TIW, rr = pix / TIW;
      const int iy = iy0 + rr, ix = ix0 + c;
      const int cg = ch * CK + c8 * 8;
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && cg < p.Cin)
        v = *reinterpret_cast<const half8*>(xn + ((long)iy * p.W + ix) * p.x_sp + cg);
      if (p.square) v = v * v;
      const int cpos = (STRIDE == 2) ? ((c & 1) * HALFW + (c >> 1)) : c;
      *reinterpret_cast<half8*>(tile + (rr * TIWp + cpos) * PS + c8 * 16) = v;
    }
    __syncthreads();

    // ---- MFMA over (tap, channel) for this chunk ------------------------------------------
    const half_t* wp[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      wp[mt] = p.w + ((((long)(cb * MT + mt) * p.nchunks + ch) * p.steps) * 64 + lane) * 8;

    if constexpr (CK8 == 1) {
      for (int s = 0; s < p.steps; ++s) {
        int tap = 2 * s + hh;
        tap = tap < p.ntaps ? tap : p.ntaps - 1;   // padded k-chunk: its weights are zero
        const int toff = tapoff[tap];
        half8 a[MT], b[2];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { a[mt] = *reinterpret_cast<const half8*>(wp[mt]); wp[mt] += 512; }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) b[nt] = *reinterpret_cast<const half8*>(tile + base[nt] + toff);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
      }
    } else {
      for (int tap = 0; tap < p.ntaps; ++tap) {
        const int toff = tapoff[tap] + hh * 16;
#pragma unroll
        for (int s2 = 0; s2 < CK8 / 2; ++s2) {
          half8 a[MT], b[2];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) { a[mt] = *reinterpret_cast<const half8*>(wp[mt]); wp[mt] += 512; }
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            b[nt] = *reinterpret_cast<const half8*>(tile + base[nt] + toff + s2 * 32);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue ------------------------------------------------------------------------------
  if constexpr (MT == 2 && LEAN) {
    __syncthreads();      // transposed full-line stores through LDS (the staging tile is dead now)
    convk::epilogue_simple_rows<2, false, 2>(p, acc, p.bias + cb * 64, tile + wave * (32 * 144), n, cb * 64,
                                             ty * TH + wave * 2, tx * TW, lane, false);
    return;
  } else if constexpr (MT == 2) {
    if (p.simple) {
      __syncthreads();
      convk::epilogue_simple_rows<2, false, 1>(p, acc, p.bias + cb * 64, tile + wave * (32 * 144), n, cb * 64,
                                               ty * TH + wave * 2, tx * TW, lane, false);
      return;
    }
  }
  convk::epilogue_regs(p, acc, n, ty * TH + wave * 2, tx * TW + r, cb * MT, hh);
}

template <int CK8, int MT, int STRIDE>
int launch(const ConvParams& p, dim3 grid, size_t lds, hipStream_t st) {
  if constexpr (MT == 2) {
    if (p.simple == 2) {
      hipLaunchKernelGGL((conv_mfma_kernel<CK8, MT, STRIDE, true>), grid, dim3(256), lds, st, p);
      return tdvc_launch_status("tdvc_conv2d");
    }
  }
  hipLaunchKernelGGL((conv_mfma_kernel<CK8, MT, STRIDE, false>), grid, dim3(256), lds, st, p);
  return tdvc_launch_status("tdvc_conv2d");
}

template <int CK8, int MT>
int launch_s(const ConvParams& p, int stride, dim3 grid, size_t lds, hipStream_t st) {
  return stride == 1 ? launch<CK8, MT, 1>(p, grid, lds, st) : launch<CK8, MT, 2>(p, grid, lds, st);
}

template <int CK8>
int launch_m(const ConvParams& p, int mt, int stride, dim3 grid, size_t lds, hipStream_t st) {
  return mt == 1 ? launch_s<CK8, 1>(p, stride, grid, lds, st) : launch_s<CK8, 2>(p, stride, grid, lds, st);
}

inline int lds_bytes(int ck, int kh, int kw, int stride) {
  const int ps = (ck == 8) ? 16 : ck * 2 + 16;
  const int tih = (TH - 1) * stride + kh, tiw = (TW - 1) * stride + kw;
  const int tiwp = stride == 2 ? 2 * ((tiw + 1) >> 1) : tiw;
  return 256 + tih * tiwp * ps;
}

inline int cout_tiles(int cout) { return cout <= 32 ? 1 : 2 * ((cout + 63) / 64); }

}  // namespace

extern "C" int tdvc_conv_plan(int cin, int kh, int kw, int stride) {
  if (cin <= 0 || (cin % 8) != 0 || kh < 1 || kw < 1 || kh > 7 || kw > 7 || (stride != 1 && stride != 2)) {
    tdvc_set_error("tdvc_conv_plan: unsupported geometry cin=%d k=%dx%d stride=%d", cin, kh, kw, stride);
    return TDVC_EINVAL;
  }
  const int cands[4] = {64, 32, 16, 8};
  for (int i = 0; i < 4; ++i) {
    const int ck = cands[i];
    if (ck > cin && ck != 8) {
      // do not stage more channels than exist unless cin is not a power-of-two multiple
      if (cin % ck != 0 && cin < ck) continue;
    }
    if (lds_bytes(ck, kh, kw, stride) <= 64 * 1024) return ck;
  }
  tdvc_set_error("tdvc_conv_plan: no LDS plan for k=%dx%d stride=%d", kh, kw, stride);
  return TDVC_EINVAL;
}

extern "C" int64_t tdvc_conv_packed_bytes(int cout, int cin, int ntaps, int ck) {
  if (cout <= 0 || cin <= 0 || ntaps <= 0 || ntaps > TDVC_MAX_TAPS || (ck != 8 && ck != 16 && ck != 32 && ck != 64)) return TDVC_EINVAL;
  const int ck8 = ck / 8;
  const int64_t nchunks = (cin + ck - 1) / ck;
  const int64_t steps = (ntaps * ck8 + 1) / 2;
  return (int64_t)cout_tiles(cout) * nchunks * steps * 64 * 8 * 2;
}

extern "C" int tdvc_pack_conv_weights(const float* w, int cout, int cin_real, int cin, int kh, int kw,
                                      int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, int ck, uint16_t* dst) {
  TDVC_CHECK(w && dst && tap_dy && tap_dx, "tdvc_pack_conv_weights: null pointer");
  TDVC_CHECK(tdvc_conv_packed_bytes(cout, cin, ntaps, ck) > 0, "tdvc_pack_conv_weights: bad geometry");
  TDVC_CHECK(cin_real <= cin, "tdvc_pack_conv_weights: cin_real > cin");
  const int ck8 = ck / 8;
  const int nchunks = (cin + ck - 1) / ck;
  const int steps = (ntaps * ck8 + 1) / 2;
  const int tiles = cout_tiles(cout);
  half_t* out = reinterpret_cast<half_t*>(dst);
  for (int t = 0; t < tiles; ++t)
    for (int ch = 0; ch < nchunks; ++ch)
      for (int s = 0; s < steps; ++s)
        for (int lane = 0; lane < 64; ++lane) {
          const int r = lane & 31, h = lane >> 5;
          const int co = t * 32 + r;
          const int kc = 2 * s + h;
          half_t* o = out + ((((int64_t)t * nchunks + ch) * steps + s) * 64 + lane) * 8;
          for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (kc < ntaps * ck8 && co < cout) {
              const int tap = kc / ck8, c8 = kc % ck8;
              const int ci = ch * ck + c8 * 8 + j;
              const int dy = tap_dy[tap], dx = tap_dx[tap];
              if (ci < cin_real && dy >= 0 && dy < kh && dx >= 0 && dx < kw)
                v = w[(((int64_t)co * cin_real + ci) * kh + dy) * kw + dx];
            }
            o[j] = (half_t)v;
          }
        }
  return TDVC_OK;
}

// the direct kernel as the dispatch table's last entry (conv_dispatch.hip)
int conv_direct_lds_bytes(const tdvc_conv_desc* d) { return lds_bytes(d->ck, d->kh, d->kw, d->stride); }
int conv_cout_tiles(int cout) { return cout_tiles(cout); }

int launch_conv_direct(const ConvParams& p, int ck8, int stride, int N, hipStream_t st) {
  const int tiles = cout_tiles(p.cout), mt = tiles == 1 ? 1 : 2;
  const int lds = lds_bytes(ck8 * 8, p.kh, p.kw, stride);
  const dim3 grid(p.tiles_x * ((p.Ho + TH - 1) / TH), tiles / mt, N);
  const size_t lds_v1 = (p.simple && lds < 256 + 4 * 32 * 144) ? 256 + 4 * 32 * 144 : lds;
  switch (ck8) {
    case 1: return launch_m<1>(p, mt, stride, grid, lds_v1, st);
    case 2: return launch_m<2>(p, mt, stride, grid, lds_v1, st);
    case 4: return launch_m<4>(p, mt, stride, grid, lds_v1, st);
    default: return launch_m<8>(p, mt, stride, grid, lds_v1, st);
  }
}
