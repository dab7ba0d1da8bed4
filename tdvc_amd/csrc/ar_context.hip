// Autoregressive context-model support kernels (compress / decompress): gather the causal 5x5
// neighbourhoods of a batch of independent positions, quantise them and scatter them back.
// The dense math in between (context conv as a 12*M -> 2M 1x1 conv, entropy_parameters) runs on the
// MFMA conv kernel.  All integer / index outputs are exact; nothing here uses atomics.
#include "common.h"
#include "rans_lane.h"

namespace {

// the 12 causal taps of the type-A 5x5 mask in raster order: (dy, dx) relative to the centre
__constant__ int8_t kTapDy[12] = {-2, -2, -2, -2, -2, -1, -1, -1, -1, -1, 0, 0};
__constant__ int8_t kTapDx[12] = {-2, -1, 0, 1, 2, -2, -1, 0, 1, 2, -2, -1};

__device__ __forceinline__ int scale_index(float s, const float* table, int n) {
  s = fmaxf(s, 0.11f);
  int idx = n - 1;
  for (int j = 0; j < n - 1; ++j) idx -= (s <= table[j]) ? 1 : 0;
  return idx;
}

__global__ void round_symbols_kernel(FMap z, const float* median, int32_t* out) {
  const long npix = (long)z.H * z.W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix * z.C * z.N) return;
  const int c = (int)(i % z.C);
  const long t = i / z.C;
  const long pix = t % npix;
  const int n = (int)(t / npix);
  out[i] = (int)rintf(reinterpret_cast<const float*>(z.p)[(long)n * z.sn + pix * z.sp + c] - median[c]);
}

// ---- a step's positions of the B = y_hat.N images of a call in one launch (a single image is B = 1).  The images share the
// position list; row b * npos + k of the staging maps x1 / pc / gp belongs to position k of image b (image-major), so a step is a
// (1, B * npos) map to the convs.  y / y_hat / params are fmaps with N = B, addressed through their own batch and pixel strides.
// T = half_t (default coders) or float (fp32 islands); VT = the 16-byte vector of T (8 halves / 4 floats)
template <typename T, typename VT>
__global__ void ar_gather_batch_kernel(FMap yh, FMap pr, const int32_t* pos, int npos, FMap x1, FMap pc) {
  constexpr int VE = 16 / sizeof(T);              // elements per 16-byte chunk
  const int MV = yh.C / VE;                       // 16-byte chunks per position
  const int per = 12 * MV + pr.C / VE;            // chunks to move per position
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)yh.N * npos * per) return;
  const long row = i / per;
  const int u = (int)(i % per);
  const int b = (int)(row / npos), k = (int)(row % npos);
  const int h = pos[2 * k], w = pos[2 * k + 1];
  if (u < 12 * MV) {
    const int t = u / MV, cv = u % MV;
    const int yy = h + kTapDy[t], xx = w + kTapDx[t];
    VT v;
#pragma unroll
    for (int j = 0; j < VE; ++j) v[j] = (T)0.f;
    if (yy >= 0 && xx >= 0 && xx < yh.W)
      v = *reinterpret_cast<const VT*>(reinterpret_cast<const T*>(yh.p) + (long)b * yh.sn + ((long)yy * yh.W + xx) * yh.sp + cv * VE);
    *reinterpret_cast<VT*>(reinterpret_cast<T*>(x1.p) + row * x1.sp + (t * MV + cv) * VE) = v;
  } else {
    const int cv = u - 12 * MV;
    const VT v = *reinterpret_cast<const VT*>(reinterpret_cast<const T*>(pr.p) + (long)b * pr.sn + ((long)h * pr.W + w) * pr.sp + cv * VE);
    *reinterpret_cast<VT*>(reinterpret_cast<T*>(pc.p) + row * pc.sp + cv * VE) = v;
  }
}

// cbase < 0: sym_in / sym / idx are raster arrays [B][H][W][M]; cbase >= 0: they are compact arrays [B][H * W][M] in the order of the
// position list, this launch's position k of image b at row cbase + k of block b (the wavefront-ordered decoder)
__global__ void ar_quantize_batch_kernel(FMap y, FMap gp, const int32_t* pos, int npos, const float* table, int ntable,
                                         const int32_t* sym_in, FMap yh, int32_t* sym, int32_t* idx, long cbase) {
  const int M = yh.C;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)yh.N * npos * M) return;
  const long row = i / M;
  const int c = (int)(i % M);
  const int b = (int)(row / npos), k = (int)(row % npos);
  const int h = pos[2 * k], w = pos[2 * k + 1];
  const float* g = reinterpret_cast<const float*>(gp.p) + row * gp.sp;
  const float scale = g[c], mean = g[M + c];
  const long o = ((long)b * yh.H * yh.W + (cbase >= 0 ? cbase + k : (long)h * yh.W + w)) * M + c;
  int q;
  if (sym_in) q = sym_in[o];
  else q = (int)rintf(reinterpret_cast<const float*>(y.p)[(long)b * y.sn + ((long)h * yh.W + w) * y.sp + c] - mean);
  const long oy = (long)b * yh.sn + ((long)h * yh.W + w) * yh.sp + c;
  if (yh.f32) reinterpret_cast<float*>(yh.p)[oy] = (float)q + mean;
  else reinterpret_cast<half_t*>(yh.p)[oy] = (half_t)((float)q + mean);
  sym[o] = q;
  idx[o] = scale_index(scale, table, ntable);
}

__global__ void ar_indexes_batch_kernel(FMap gp, const int32_t* pos, int npos, int B, const float* table, int ntable, int M, int H, int W,
                                        int32_t* idx, long cbase) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * npos * M) return;
  const long row = i / M;
  const int c = (int)(i % M);
  const int b = (int)(row / npos), k = (int)(row % npos);
  const int h = pos[2 * k], w = pos[2 * k + 1];
  const float* g = reinterpret_cast<const float*>(gp.p) + row * gp.sp;
  idx[((long)b * H * W + (cbase >= 0 ? cbase + k : (long)h * W + w)) * M + c] = scale_index(g[c], table, ntable);
}

// ---- lane-split y streams (rans_lane.h): the range decoder of one anti-diagonal on the device, one thread per lane.
// Lane state lives in a device buffer between the steps' launches: uint32 [L][4] = {x low, x high, next word, end word}
// per lane, then one sticky `bad` word (the only error channel: nothing here faults on a damaged stream, it flags it).
constexpr int kLaneStateWords = 4;

__device__ __forceinline__ void lane_store(const TdvcLane& st, uint32_t* state, int lane, int L) {
  uint32_t* s = state + lane * kLaneStateWords;
  s[0] = (uint32_t)st.x; s[1] = (uint32_t)(st.x >> 32); s[2] = st.pos; s[3] = st.end;
  if (st.bad) state[L * kLaneStateWords] = 1;                  // every writer stores the same value
}

// The CDF tables as the kernel reads them: every table's entries packed end to end as uint16 (table t at cdf16[starts[t]],
// sizes[t] entries; the last entry of a table is 1 << 16, which does not fit and is implied), n16 <= kLdsCdf entries in all.
// They are copied into LDS at the start of a launch -- the 64 tables of compressai's scale table have 27 256 entries -- so
// that the bin search's dependent probes are LDS reads; a larger table set is refused by tdvc_ar_decode_lanes_step_batch.
constexpr int kLdsCdf = 27648;                                  // 54 KB
constexpr int kChunkSyms = 6144;                                // symbols between two barriers: 48 positions of 128 channels
constexpr int kLanesLds = kLdsCdf * 2 + kChunkSyms * 4 + 64 * 4 * 4 + kChunkSyms;      // cdf | q | starts, sizes, offsets, scale table | ci
typedef __attribute__((address_space(3))) const uint16_t* lds_u16_ptr;
struct CdfDev {
  lds_u16_ptr lds;
  int start, size;
  __device__ __forceinline__ uint32_t operator()(int32_t i) const { return i == size - 1 ? 65536u : lds[start + i]; }
  __device__ __forceinline__ uint32_t inner(int32_t i) const { return lds[start + i]; }
};

// scale_index() over a copy of the scale table in LDS whose entries from ntable - 1 on are -inf (they never count): the same
// 63 comparisons, fetched as 16 independent 16-byte LDS reads instead of 63 dependent ones
__device__ __forceinline__ int scale_index_lds(float s, const float* tab64, int ntable) {
  s = fmaxf(s, 0.11f);
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < 64; j += 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(tab64 + j);
    cnt += (s <= t[0] ? 1 : 0) + (s <= t[1] ? 1 : 0) + (s <= t[2] ? 1 : 0) + (s <= t[3] ? 1 : 0);
  }
  return ntable - 1 - cnt;
}

// The B containers of a call sit in one device buffer `streams` of `stream_bytes` bytes; tab[b] = {byte offset of container b (a
// multiple of 16), 32-bit words of its payload}.  The table is device memory a host copy filled: a container that does not lie inside
// the buffer is given no words, so its lanes flag `bad` and nothing outside the buffer is read.  State: [B][L * 4 + 1] words, one
// sticky `bad` word per image.  Workgroup b of L threads works on image b.
struct LaneStream { const uint8_t* payload; uint32_t nwords; bool ok; };
__device__ __forceinline__ LaneStream lane_stream(const uint8_t* streams, long stream_bytes, const uint32_t* tab, int b, int L) {
  const uint32_t off = tab[2 * b], nw = tab[2 * b + 1];
  const long pay = (long)off + tdvc_lanes_payload_offset(L);
  const bool ok = (off & 15u) == 0 && pay + 4 * (long)nw <= stream_bytes;
  return {streams + (ok ? pay : 0), ok ? nw : 0u, ok};
}

__global__ void ar_lanes_init_batch_kernel(const uint8_t* streams, long stream_bytes, const uint32_t* tab, uint32_t* state) {
  const int L = (int)blockDim.x, lane = (int)threadIdx.x, b = (int)blockIdx.x;
  const LaneStream ls = lane_stream(streams, stream_bytes, tab, b, L);
  uint32_t* st_b = state + (long)b * (L * kLaneStateWords + 1);
  TdvcLane st;
  if (ls.ok) {
    const uint8_t* lt = ls.payload - 2 * L;                    // the container's length table
    uint32_t begin = 0;
    for (int j = 0; j < lane; ++j) begin += (uint32_t)lt[2 * j] | ((uint32_t)lt[2 * j + 1] << 8);
    const uint32_t len = (uint32_t)lt[2 * lane] | ((uint32_t)lt[2 * lane + 1] << 8);
    tdvc_lane_init(st, ls.payload, begin, len, ls.nwords);
  } else {
    st.x = 0; st.pos = 0; st.end = 0; st.bad = 1;
  }
  if (lane == 0) st_b[L * kLaneStateWords] = 0;
  __syncthreads();
  lane_store(st, st_b, lane, L);
}

// What ar_indexes_batch_kernel + the host range decoder + ar_quantize_batch_kernel do for one step of a wavefront-ordered stream, in
// three phases per chunk of positions.  A (all threads, coalesced): scale -> CDF index of every symbol, into LDS and `idx`.  B: lane
// `threadIdx.x` decodes its symbols (k, c), c % L == lane, in stream order (k, then c) -- the serial part; it touches LDS only,
// apart from the lane's own renormalisation words, so no wait of the state update covers another memory operation.  C (all
// threads, coalesced): sym at the compact row cbase + k of the image's block and y_hat(b, h, w, c) = q + mean.  T: y_hat's element type.
template <typename T>
__global__ void __launch_bounds__(128) ar_decode_lanes_batch_kernel(FMap gp, const int32_t* __restrict__ pos, int npos, const float* __restrict__ table,
                                                                    int ntable, const uint8_t* __restrict__ streams, long stream_bytes,
                                                                    const uint32_t* __restrict__ tab, const uint16_t* __restrict__ cdf16, int n16,
                                                                    const int32_t* __restrict__ cdf_starts, const int32_t* __restrict__ cdf_sizes,
                                                                    const int32_t* __restrict__ offsets, uint32_t* state, FMap yh,
                                                                    int32_t* __restrict__ sym, int32_t* __restrict__ idx, long cbase) {
  const int L = (int)blockDim.x, lane = (int)threadIdx.x, b = (int)blockIdx.x, M = yh.C;
  const LaneStream ls = lane_stream(streams, stream_bytes, tab, b, L);
  const float* __restrict__ gp0 = reinterpret_cast<const float*>(gp.p) + (long)b * npos * gp.sp;       // row 0 of image b's rows of gp
  T* __restrict__ yh0 = reinterpret_cast<T*>(yh.p) + (long)b * yh.sn;
  const long row0 = ((long)b * yh.H * yh.W + cbase) * M;       // image b's block of the compact arrays, row cbase
  sym += row0;
  idx += row0;
  state += (long)b * (L * kLaneStateWords + 1);
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint16_t* s_cdf = reinterpret_cast<uint16_t*>(s_raw);
  int32_t* s_q = reinterpret_cast<int32_t*>(s_raw + kLdsCdf * 2);
  int32_t* s_start = s_q + kChunkSyms;
  int32_t* s_size = s_start + 64;
  int32_t* s_off = s_size + 64;
  float* s_table = reinterpret_cast<float*>(s_off + 64);
  uint8_t* s_ci = reinterpret_cast<uint8_t*>(s_table + 64);
  if (lane < 64) s_table[lane] = lane < ntable - 1 ? table[lane] : -INFINITY;       // ntable <= 64 <= L
  if (lane < ntable) {
    const int start = cdf_starts[lane], size = cdf_sizes[lane];
    const bool ok = start >= 0 && size >= 0 && start <= n16 && size <= n16 - start;
    s_start[lane] = ok ? start : 0;
    s_size[lane] = ok ? size : 0;                              // a table outside the array has no entries: the decode flags it
    s_off[lane] = offsets[lane];
  }
  const int nchunk = n16 / 8;                                  // 16-byte chunks, 1 <= nchunk <= kLdsCdf / 8
  for (int c0 = lane; c0 < nchunk; c0 += L * 8) {              // eight loads in flight per thread, no branch between them:
    int ix[8];                                                 // an index past the end is clamped, which re-copies the last
    uint4 v[8];                                                // chunk onto itself
#pragma unroll
    for (int u = 0; u < 8; ++u) ix[u] = min(c0 + u * L, nchunk - 1);
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const uint4*>(cdf16)[ix[u]];
#pragma unroll
    for (int u = 0; u < 8; ++u) reinterpret_cast<uint4*>(s_cdf)[ix[u]] = v[u];
  }
  TdvcLane st;
  {
    const uint32_t* s = state + lane * kLaneStateWords;
    st.x = (uint64_t)s[0] | ((uint64_t)s[1] << 32);
    st.end = s[3] < ls.nwords ? s[3] : ls.nwords;                    // whatever the buffer holds, no read leaves the payload
    st.pos = s[2] < st.end ? s[2] : st.end;
    st.bad = 0;
  }
  __syncthreads();
  const int per = M / L, kc = kChunkSyms / M;                  // positions per chunk (M <= kChunkSyms)
  for (int k0 = 0; k0 < npos; k0 += kc) {
    const int nk = npos - k0 < kc ? npos - k0 : kc, ne = nk * M;
    for (int e = lane; e < ne; e += L) {                       // A
      const int k = k0 + e / M, c = e % M;
      const int ci = scale_index_lds((gp0 + (long)k * gp.sp)[c], s_table, ntable);
      s_ci[e] = (uint8_t)ci;
      idx[(long)k * M + c] = ci;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k)                               // B
      for (int j = 0; j < per; ++j) {
        const int e = k * M + lane + j * L, ci = s_ci[e];
        const int size = s_size[ci];
        const CdfDev cdf{(lds_u16_ptr)s_cdf, s_start[ci], size};
        s_q[e] = tdvc_lane_decode(st, ls.payload, cdf, size) + s_off[ci];
      }
    __syncthreads();
    for (int e = lane; e < ne; e += L) {                       // C
      const int k = k0 + e / M, c = e % M;
      const int h = pos[2 * k], w = pos[2 * k + 1], q = s_q[e];
      const float mean = (gp0 + (long)k * gp.sp)[M + c];
      yh0[((long)h * yh.W + w) * yh.sp + c] = (T)((float)q + mean);
      sym[(long)k * M + c] = q;
    }
    __syncthreads();                                           // s_ci / s_q are free for the next chunk
  }
  lane_store(st, state, lane, L);
}

// ---- the range ENCODER of the same format on the device: workgroup b of L threads codes image b, thread l lane l, straight
// from the context loop's raster arrays sym / idx [B][H][W][M], so the symbols never leave the device.  Three phases.  1: the
// packed CDFs into LDS.  2: per chunk of positions, walked from the LAST position of the wavefront list to the first, A (coalesced
// loads, twelve symbols in flight per thread) everything about a symbol that does not depend on the coder's state -- its bin's
// start and range, its escape value (tdvc_lane_symbol) -- into LDS, B thread l pushes its symbols c = j * L + l, j from M / L - 1
// down to 0, through tdvc_lane_push into its own scratch region, words downward from the region's end: the serial pass is the
// state update alone (a compare, three 16-bit division steps), fed by LDS reads whose addresses it knows in advance.  3: lane lengths to LDS, prefix-summed; header, length table and the sub-streams, lane by lane, all threads
// copying, into out + b * out_stride; info[b] = {container bytes, status}.  On a non-zero status nothing of the container is
// written.  Nothing outside scratch[b], out[b] and info[b] is written; plain loads and stores and LDS only.
constexpr int kEncMaxPos = 64;                                  // positions per chunk at most (their pixel offsets: one thread each)
constexpr int kEncLds = kLdsCdf * 2 + kChunkSyms * 8 + 64 * 4 * 3 + kEncMaxPos * 4 + (128 * 3 + 4) * 4 + kChunkSyms;  // cdf | start and range, escape value | starts, sizes, offsets | pixel | lane pos, len, offset, status | kind

__global__ void __launch_bounds__(128) ar_encode_lanes_batch_kernel(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx, int H, int W, int M,
                                                                    const int32_t* __restrict__ pos, int npos, const uint16_t* __restrict__ cdf16, int n16,
                                                                    const int32_t* __restrict__ cdf_starts, const int32_t* __restrict__ cdf_sizes,
                                                                    const int32_t* __restrict__ offsets, int ncdfs, uint32_t* __restrict__ scratch,
                                                                    uint32_t lane_words, uint8_t* __restrict__ out, long out_stride, uint32_t* __restrict__ info) {
  const int L = (int)blockDim.x, lane = (int)threadIdx.x, b = (int)blockIdx.x;
  sym += (long)b * H * W * M;
  idx += (long)b * H * W * M;
  scratch += (long)b * L * lane_words;                         // image b's L regions; thread l owns words [l * lane_words, (l + 1) * lane_words)
  out += (long)b * out_stride;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint16_t* s_cdf = reinterpret_cast<uint16_t*>(s_raw);
  uint32_t* s_sr = reinterpret_cast<uint32_t*>(s_raw + kLdsCdf * 2);
  uint32_t* s_esc = s_sr + kChunkSyms;
  int32_t* s_start = reinterpret_cast<int32_t*>(s_esc + kChunkSyms);
  int32_t* s_size = s_start + 64;
  int32_t* s_off = s_size + 64;
  int32_t* s_pix = s_off + 64;
  uint32_t* s_lpos = reinterpret_cast<uint32_t*>(s_pix + kEncMaxPos);
  uint32_t* s_llen = s_lpos + 128;
  uint32_t* s_loff = s_llen + 128;                              // 128 + 1 prefix sums, then the image's status
  uint8_t* s_kind = reinterpret_cast<uint8_t*>(s_loff + 128 + 4);
  // phase 1
  if (lane < 64) {
    int start = 0, size = 0, off = 0;
    if (lane < ncdfs) {
      start = cdf_starts[lane]; size = cdf_sizes[lane]; off = offsets[lane];
      if (!(start >= 0 && size >= 0 && start <= n16 && size <= n16 - start)) start = size = 0;      // a table outside the array has no entries: flagged
    }
    s_start[lane] = start; s_size[lane] = size; s_off[lane] = off;
  }
  const int nchunk = n16 / 8;                                  // as in the decoder: 16-byte chunks, clamped indexes
  for (int c0 = lane; c0 < nchunk; c0 += L * 8) {
    int ix[8];
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) ix[u] = min(c0 + u * L, nchunk - 1);
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const uint4*>(cdf16)[ix[u]];
#pragma unroll
    for (int u = 0; u < 8; ++u) reinterpret_cast<uint4*>(s_cdf)[ix[u]] = v[u];
  }
  // phase 2
  TdvcEncLane st;
  tdvc_enc_lane_init(st, (uint32_t)lane * lane_words, (uint32_t)(lane + 1) * lane_words);
  const int per = M / L;
  const int kc = kChunkSyms / M < kEncMaxPos ? kChunkSyms / M : kEncMaxPos;       // positions per chunk, 1 <= kc <= 64 <= L
  // pixel offset of position k, or -1 outside the image; thread t < kc fetches the NEXT chunk's while this one is coded
  auto pixel = [&](int k) -> int {
    if (k < 0) return -1;
    const int h = pos[2 * k], w = pos[2 * k + 1];
    return (h >= 0 && h < H && w >= 0 && w < W) ? h * W + w : -1;
  };
  int pix_next = lane < kc ? pixel(npos - 1 - lane) : -1;      // chunk-local slot t holds position k_hi - t
  for (int k_hi = npos - 1; k_hi >= 0; k_hi -= kc) {
    const int nk = k_hi + 1 < kc ? k_hi + 1 : kc;
    if (lane < kc) s_pix[lane] = pix_next;
    if (lane < kc) pix_next = pixel(k_hi - kc - lane);
    __syncthreads();                                           // also: the previous chunk's B is over, s_sr / s_esc / s_kind are free
    constexpr int U = 12;                                      // A: U symbols and U indexes in flight per thread
    const int ni = nk * per;                                   // a thread's elements: i -> slot i / per, channel (i % per) * L + lane
    for (int i0 = 0; i0 < ni; i0 += U) {
      int e[U], c[U], pix[U], q[U], ci[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = min(i0 + u, ni - 1), t = i / per;        // uniform over the workgroup; past the end: the last element again
        c[u] = (i - t * per) * L + lane;
        e[u] = t * M + c[u];
        pix[u] = s_pix[t];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long o = (long)(pix[u] < 0 ? 0 : pix[u]) * M + c[u];
        q[u] = sym[o]; ci[u] = idx[o];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        TdvcEncSym sy = {0, 0, kEncUnusable};
        if (pix[u] >= 0 && ci[u] >= 0 && ci[u] < ncdfs && ci[u] < 64) {
          const int size = s_size[ci[u]];
          sy = tdvc_lane_symbol(CdfDev{(lds_u16_ptr)s_cdf, s_start[ci[u]], size}, size, (int32_t)((uint32_t)q[u] - (uint32_t)s_off[ci[u]]));
        }
        s_kind[e[u]] = (uint8_t)sy.kind;
        s_sr[e[u]] = sy.start_range;
        s_esc[e[u]] = sy.raw;
      }
    }
    __syncthreads();
    for (int t = 0; t < nk; ++t)                               // B: slot 0 is the chunk's LAST position; only the state update is serial
      for (int j = per - 1; j >= 0; --j) {
        const int e = t * M + j * L + lane;
        tdvc_lane_push(st, scratch, s_kind[e], s_sr[e], s_esc[e]);
      }
  }
  // phase 3
  const uint32_t len = tdvc_enc_lane_finish(st, scratch);
  s_lpos[lane] = st.pos;
  s_llen[lane] = len;
  s_loff[lane] = tdvc_enc_lane_status(st, len);
  __syncthreads();                                             // every lane's words are written (workgroup scope) and its length is in LDS
  if (lane == 0) {
    uint32_t status = 0, words = 0;
    for (int l = 0; l < L; ++l) {
      const uint32_t s = s_loff[l];
      status = s > status ? s : status;
      s_loff[l] = words;
      words += s_llen[l];                                      // <= 128 * 65536: no overflow
    }
    s_loff[128] = words;
    s_loff[129] = status;
  }
  __syncthreads();
  const uint32_t status = s_loff[129];
  if (lane == 0) {
    info[2 * b] = status ? 0u : (uint32_t)tdvc_lanes_payload_offset(L) + 4u * s_loff[128];
    info[2 * b + 1] = status;
  }
  if (status) return;                                          // uniform: the whole workgroup leaves
  // every lane is at most min(lane_words, 65535) words here, and the entry point has checked out_stride against L such lanes
  if (lane == 0) *reinterpret_cast<uint32_t*>(out) = (uint32_t)kLanesMagic | ((uint32_t)kLanesVersion << 8) | ((uint32_t)L << 16);
  reinterpret_cast<uint16_t*>(out + kLanesHeaderBytes)[lane] = (uint16_t)len;
  uint32_t* payload = reinterpret_cast<uint32_t*>(out + tdvc_lanes_payload_offset(L));
  for (int l = 0; l < L; ++l) {
    const uint32_t* __restrict__ src = scratch + s_lpos[l];
    uint32_t* __restrict__ dst = payload + s_loff[l];
    const int n = (int)s_llen[l];
#pragma unroll 4
    for (int i = lane; i < n; i += L) dst[i] = src[i];
  }
}

#define ST(s) reinterpret_cast<hipStream_t>(s)
inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" int tdvc_round_symbols(const tdvc_fmap* z, const float* median, int32_t* out, void* stream) {
  TDVC_CHECK(z && median && out && fmap_ok32(*z), "tdvc_round_symbols: bad arguments");
  hipLaunchKernelGGL(round_symbols_kernel, g1((long)z->N * z->H * z->W * z->C), dim3(256), 0, ST(stream), to_dev(*z), median, out);
  return tdvc_launch_status("tdvc_round_symbols");
}

// ---- the context loop in native code: a step handles the step's positions of all B images of the call in the same launches (the
// images share the position list, the weights and the tables; nothing in a step couples one image to another).  Row b * n + k of
// x1 / pc / gp is position k of image b, a step is a (1, B * n) map to the convs; y / y_hat / params are fmaps with N = B.
namespace {
bool ar_fmap_ok(const tdvc_fmap& f, bool f32) { return f32 ? (fmap_ok32(f) && (f.C % 4) == 0 && (f.sp % 4) == 0 && (f.sn % 4) == 0 && aligned16(f.p)) : fmap_ok16(f); }
}  // namespace

extern "C" int tdvc_ar_gather_batch(const tdvc_fmap* y_hat, const tdvc_fmap* params, const int32_t* pos, int npos,
                                    const tdvc_fmap* x1, const tdvc_fmap* pc, void* stream) {
  TDVC_CHECK(y_hat && params && pos && x1 && pc && npos >= 1, "tdvc_ar_gather_batch: null / empty");
  const bool f32 = y_hat->dtype == TDVC_F32;
  TDVC_CHECK(ar_fmap_ok(*y_hat, f32) && ar_fmap_ok(*params, f32) && ar_fmap_ok(*x1, f32) && ar_fmap_ok(*pc, f32),
             "tdvc_ar_gather_batch: four fp16 fmaps, or four fp32 fmaps (fp32 islands), expected");
  TDVC_CHECK(params->N == y_hat->N && params->H == y_hat->H && params->W == y_hat->W, "tdvc_ar_gather_batch: params batch / geometry must match y_hat");
  const long rows = (long)y_hat->N * npos;
  TDVC_CHECK(x1->C == 12 * y_hat->C && x1->W >= rows && x1->H == 1 && x1->N == 1 && pc->C >= params->C && pc->W >= rows && pc->H == 1 && pc->N == 1,
             "tdvc_ar_gather_batch: x1 must be (1,1,>=B*npos,12*M), pc (1,1,>=B*npos,>=2M)");
  const int ve = f32 ? 4 : 8;
  const long total = rows * (12 * y_hat->C / ve + params->C / ve);
  if (f32) hipLaunchKernelGGL((ar_gather_batch_kernel<float, f32x4>), g1(total), dim3(256), 0, ST(stream), to_dev(*y_hat), to_dev(*params), pos, npos, to_dev(*x1), to_dev(*pc));
  else hipLaunchKernelGGL((ar_gather_batch_kernel<half_t, half8>), g1(total), dim3(256), 0, ST(stream), to_dev(*y_hat), to_dev(*params), pos, npos, to_dev(*x1), to_dev(*pc));
  return tdvc_launch_status("tdvc_ar_gather_batch");
}

extern "C" int tdvc_ar_quantize_batch(const tdvc_fmap* y, const tdvc_fmap* gp, const int32_t* pos, int npos, const float* scale_table, int ntable,
                                      const int32_t* symbols_in, const tdvc_fmap* y_hat, int32_t* symbols, int32_t* indexes, int64_t cbase, void* stream) {
  TDVC_CHECK(gp && pos && scale_table && y_hat && symbols && indexes && npos >= 1 && ntable >= 2, "tdvc_ar_quantize_batch: null / empty");
  TDVC_CHECK(symbols_in || (y && fmap_ok32(*y) && y->N == y_hat->N && y->H == y_hat->H && y->W == y_hat->W && y->C >= y_hat->C),
             "tdvc_ar_quantize_batch: need y (encoder, y_hat's batch and geometry) or symbols_in (decoder)");
  TDVC_CHECK(fmap_ok32(*gp) && (y_hat->dtype == TDVC_F32 ? fmap_ok32(*y_hat) : fmap_ok16(*y_hat)) && gp->C >= 2 * y_hat->C && gp->W >= (long)y_hat->N * npos,
             "tdvc_ar_quantize_batch: bad gp / y_hat");
  TDVC_CHECK(cbase < 0 || cbase + npos <= (int64_t)y_hat->H * y_hat->W, "tdvc_ar_quantize_batch: compact rows past the image's block");
  const FMap yd = y ? to_dev(*y) : to_dev(*y_hat);
  hipLaunchKernelGGL(ar_quantize_batch_kernel, g1((long)y_hat->N * npos * y_hat->C), dim3(256), 0, ST(stream), yd, to_dev(*gp), pos, npos, scale_table, ntable,
                     symbols_in, to_dev(*y_hat), symbols, indexes, (long)cbase);
  return tdvc_launch_status("tdvc_ar_quantize_batch");
}

extern "C" int tdvc_ar_indexes_batch(const tdvc_fmap* gp, const int32_t* pos, int npos, int B, const float* scale_table, int ntable,
                                     int M, int H, int W, int32_t* indexes, int64_t cbase, void* stream) {
  TDVC_CHECK(gp && pos && scale_table && indexes && npos >= 1 && B >= 1 && ntable >= 2 && M >= 1 && H >= 1 && W >= 1 && fmap_ok32(*gp) && gp->C >= 2 * M &&
             gp->W >= (long)B * npos && (cbase < 0 || cbase + npos <= (int64_t)H * W), "tdvc_ar_indexes_batch: bad arguments");
  hipLaunchKernelGGL(ar_indexes_batch_kernel, g1((long)B * npos * M), dim3(256), 0, ST(stream), to_dev(*gp), pos, npos, B, scale_table, ntable, M, H, W, indexes, (long)cbase);
  return tdvc_launch_status("tdvc_ar_indexes_batch");
}

// ---- lane-split y streams: the decoder's loop with the range decoder on the device.  Device buffer layout
// (tdvc_ar_lanes_batch_layout): the table uint32 [B][2] = {byte offset of container b, words of its payload}, padded to 16 bytes,
// then the containers, each at a 16-byte aligned offset.
extern "C" int64_t tdvc_ar_lanes_state_bytes(int L) { return L >= 1 ? (int64_t)sizeof(uint32_t) * ((int64_t)L * kLaneStateWords + 1) : TDVC_EINVAL; }
extern "C" int64_t tdvc_ar_lanes_batch_layout(const int64_t* nbytes, int B, int L, uint32_t* table_out) {
  if (!nbytes || B < 1 || B > 65535 || L < 1) { tdvc_set_error("tdvc_ar_lanes_batch_layout: null sizes, or B = %d / L = %d out of range", B, L); return TDVC_EINVAL; }
  int64_t off = ((int64_t)B * 8 + 15) / 16 * 16;
  const int64_t pay = tdvc_lanes_payload_offset(L);
  for (int b = 0; b < B; ++b) {
    if (nbytes[b] < pay || (nbytes[b] - pay) % 4 != 0 || (nbytes[b] - pay) / 4 > (int64_t)L * kLanesMaxWords) {
      tdvc_set_error("tdvc_ar_lanes_batch_layout: image %d: bad stream size %lld", b, (long long)nbytes[b]);
      return TDVC_EINVAL;
    }
    if (table_out) { table_out[2 * b] = (uint32_t)off; table_out[2 * b + 1] = (uint32_t)((nbytes[b] - pay) / 4); }
    off += (nbytes[b] + 15) / 16 * 16;
    if (off > 0xFFFFFFF0ll) { tdvc_set_error("tdvc_ar_lanes_batch_layout: the strings exceed 4 GB"); return TDVC_EINVAL; }
  }
  return off;
}

namespace {
int lanes_batch_args(const char* who, const uint8_t* streams_dev, int64_t stream_bytes, const uint32_t* table_dev, int B, int L, int M, const uint32_t* state_dev) {
  TDVC_CHECK(streams_dev && table_dev && state_dev && B >= 1 && B <= 65535, "%s: null stream / table / state buffer, or B = %d out of range", who, B);
  TDVC_CHECK((L == 64 || L == 128) && M >= L && M % L == 0, "%s: the device decoder takes 64 or 128 lanes that divide the channel count (L = %d, M = %d)", who, L, M);
  TDVC_CHECK(aligned16(streams_dev) && (((uintptr_t)table_dev) & 3) == 0 && (((uintptr_t)state_dev) & 3) == 0 && stream_bytes >= 16,
             "%s: the stream buffer must be 16-byte aligned, the table / state buffers 4-byte aligned", who);
  return TDVC_OK;
}
}  // namespace

extern "C" int tdvc_ar_lanes_init_batch(const uint8_t* streams_dev, int64_t stream_bytes, const uint32_t* table_dev, int B, int L, uint32_t* state_dev, void* stream) {
  if (const int rc = lanes_batch_args("tdvc_ar_lanes_init_batch", streams_dev, stream_bytes, table_dev, B, L, L, state_dev)) return rc;
  hipLaunchKernelGGL(ar_lanes_init_batch_kernel, dim3(B), dim3(L), 0, ST(stream), streams_dev, (long)stream_bytes, table_dev, state_dev);
  return tdvc_launch_status("tdvc_ar_lanes_init_batch");
}

extern "C" int tdvc_ar_decode_lanes_step_batch(const tdvc_fmap* gp, const int32_t* pos, int npos, const float* scale_table, int ntable,
                                               const uint8_t* streams_dev, int64_t stream_bytes, const uint32_t* table_dev, int L,
                                               const tdvc_cdf_tables_dev* tables, uint32_t* state_dev, const tdvc_fmap* y_hat,
                                               int32_t* symbols, int32_t* indexes, int64_t cbase, void* stream) {
  TDVC_CHECK(gp && pos && scale_table && tables && tables->cdf16 && tables->starts && tables->sizes && tables->offsets && y_hat && symbols && indexes && npos >= 1 &&
             cbase >= 0, "tdvc_ar_decode_lanes_step_batch: null / empty");
  const tdvc_cdf_tables_dev& t = *tables;
  TDVC_CHECK(ntable >= 2 && ntable <= 64 && t.ncdfs >= ntable, "tdvc_ar_decode_lanes_step_batch: 2..64 scale-table entries, one CDF per entry expected");
  TDVC_CHECK(t.n16 >= 8 && t.n16 % 8 == 0 && aligned16(t.cdf16), "tdvc_ar_decode_lanes_step_batch: the packed CDFs must be 16-byte aligned, a multiple of 8 entries long");
  TDVC_CHECK(t.n16 <= kLdsCdf, "tdvc_ar_decode_lanes_step_batch: %d packed CDF entries, the kernel's LDS holds %d", t.n16, kLdsCdf);
  const int B = y_hat->N;
  TDVC_CHECK(fmap_ok32(*gp) && (y_hat->dtype == TDVC_F32 ? fmap_ok32(*y_hat) : fmap_ok16(*y_hat)) && gp->C >= 2 * y_hat->C && gp->W >= (long)B * npos &&
             cbase + npos <= (int64_t)y_hat->H * y_hat->W, "tdvc_ar_decode_lanes_step_batch: bad gp / y_hat / rows");
  if (const int rc = lanes_batch_args("tdvc_ar_decode_lanes_step_batch", streams_dev, stream_bytes, table_dev, B, L, y_hat->C, state_dev)) return rc;
  TDVC_CHECK(y_hat->C <= kChunkSyms, "tdvc_ar_decode_lanes_step_batch: more than %d channels", kChunkSyms);
  static TdvcPerDeviceFlag attr;
  if (!attr.flag()) {
    for (const void* k : {reinterpret_cast<const void*>(&ar_decode_lanes_batch_kernel<float>), reinterpret_cast<const void*>(&ar_decode_lanes_batch_kernel<half_t>)}) {
      const hipError_t err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLanesLds);
      if (err != hipSuccess) { tdvc_set_error("tdvc_ar_decode_lanes_step_batch: cannot reserve %d bytes of LDS: %s", kLanesLds, hipGetErrorString(err)); return (int)err; }
    }
    attr.flag() = true;
  }
  if (y_hat->dtype == TDVC_F32)
    hipLaunchKernelGGL(ar_decode_lanes_batch_kernel<float>, dim3(B), dim3(L), kLanesLds, ST(stream), to_dev(*gp), pos, npos, scale_table, ntable, streams_dev,
                       (long)stream_bytes, table_dev, t.cdf16, t.n16, t.starts, t.sizes, t.offsets, state_dev, to_dev(*y_hat), symbols, indexes, (long)cbase);
  else
    hipLaunchKernelGGL(ar_decode_lanes_batch_kernel<half_t>, dim3(B), dim3(L), kLanesLds, ST(stream), to_dev(*gp), pos, npos, scale_table, ntable, streams_dev,
                       (long)stream_bytes, table_dev, t.cdf16, t.n16, t.starts, t.sizes, t.offsets, state_dev, to_dev(*y_hat), symbols, indexes, (long)cbase);
  return tdvc_launch_status("tdvc_ar_decode_lanes_step_batch");
}

// what the device encoder and its host twin (rans.cpp) check before anything is touched; `who` names the entry point
int tdvc_encode_lanes_args(const char* who, const tdvc_lanes_enc* enc, int32_t ncdfs);

extern "C" int tdvc_ar_encode_lanes_batch(const tdvc_lanes_enc* enc, const tdvc_cdf_tables_dev* tables, void* stream) {
  TDVC_CHECK(tables && tables->cdf16 && tables->starts && tables->sizes && tables->offsets, "tdvc_ar_encode_lanes_batch: null table pointer");
  const tdvc_cdf_tables_dev& t = *tables;
  if (const int rc = tdvc_encode_lanes_args("tdvc_ar_encode_lanes_batch", enc, t.ncdfs)) return rc;
  const tdvc_lanes_enc& e = *enc;
  TDVC_CHECK(t.n16 >= 8 && t.n16 % 8 == 0 && aligned16(t.cdf16), "tdvc_ar_encode_lanes_batch: the packed CDFs must be 16-byte aligned, a multiple of 8 entries long");
  TDVC_CHECK(t.n16 <= kLdsCdf, "tdvc_ar_encode_lanes_batch: %d packed CDF entries, the kernel's LDS holds %d", t.n16, kLdsCdf);
  TDVC_CHECK(e.M <= kChunkSyms, "tdvc_ar_encode_lanes_batch: more than %d channels", kChunkSyms);
  static TdvcPerDeviceFlag attr;
  if (!attr.flag()) {
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&ar_encode_lanes_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kEncLds);
    if (err != hipSuccess) { tdvc_set_error("tdvc_ar_encode_lanes_batch: cannot reserve %d bytes of LDS: %s", kEncLds, hipGetErrorString(err)); return (int)err; }
    attr.flag() = true;
  }
  hipLaunchKernelGGL(ar_encode_lanes_batch_kernel, dim3(e.B), dim3(e.L), kEncLds, ST(stream), e.symbols, e.indexes, e.H, e.W, e.M, e.pos, e.npos, t.cdf16, t.n16, t.starts,
                     t.sizes, t.offsets, t.ncdfs, e.scratch, (uint32_t)e.lane_words, e.out, (long)e.out_stride, e.info);
  return tdvc_launch_status("tdvc_ar_encode_lanes_batch");
}

// ---- the loop's one driver.  A call is: validate the tdvc_ar_loop and the back end's own arguments (all of it before anything
// touches a device), copy the conv descriptors, then per step gather -> convs over B * n rows -> the back end's step.  The back ends
// are what the three entry points differ in: what follows a step's convs and what brackets the loop.
namespace {
struct LoopCall { const char* who; const tdvc_ar_loop* l; void* stream; };      // the entry point's name (for the messages), its loop, its stream
struct LoopBackend {                                           // a back end adds step(call, pos, n, o): a step's n positions, `o` positions into the list, after its convs
  int check(const LoopCall&) { return TDVC_OK; }               // host only; the loop's own arguments are valid here
  int begin(const LoopCall&, int /* positions of the largest step */) { return TDVC_OK; }
  int end(const LoopCall&, int rc) { return rc; }              // rc: the loop's status so far -> the call's
};

// -> the largest step
int loop_args(const char* who, const tdvc_ar_loop* l, int* nmax_out) {
  TDVC_CHECK(l && l->y_hat.p && l->params.p && l->x1.p && l->pc.p && l->gp.p && l->convs && l->pos_dev && l->scale_table && l->idx_dev && l->sym_dev, "%s: null argument", who);
  const tdvc_fmap &yh = l->y_hat, &pr = l->params;
  TDVC_CHECK(pr.N == yh.N && pr.H == yh.H && pr.W == yh.W, "%s: y_hat and params must be fmaps of B images of one geometry (y_hat %d x %d x %d, params %d x %d x %d)", who,
             yh.N, yh.H, yh.W, pr.N, pr.H, pr.W);
  const long B = yh.N;
  TDVC_CHECK(B >= 1 && B <= 65535, "%s: 1 <= B <= 65535 images expected, got %ld", who, B);
  TDVC_CHECK(l->nconvs >= 1 && l->nconvs <= 8 && l->nsteps >= 1 && yh.C >= 1 && yh.C <= 4096 && yh.W >= 1 && yh.H >= 1, "%s: bad sizes", who);
  long total = 0;
  int nmax = 0;
  for (int s = 0; s < l->nsteps; ++s) {
    const long n = l->step_sizes ? l->step_sizes[s] : 1;       // no step list: one position per step (the raster order)
    TDVC_CHECK(n >= 1 && n <= (1 << 20), "%s: step %d has %ld positions", who, s, n);
    TDVC_CHECK(B * n <= l->x1.W && B * n <= l->pc.W && B * n <= l->gp.W, "%s: step %d: B * n = %ld rows exceed the staging buffers (x1 %d, pc %d, gp %d)", who, s, B * n,
               l->x1.W, l->pc.W, l->gp.W);
    total += n;
    nmax = n > nmax ? (int)n : nmax;
  }
  TDVC_CHECK(total == (long)yh.H * yh.W, "%s: the steps must cover every position once (%ld of %ld)", who, total, (long)yh.H * yh.W);
  *nmax_out = nmax;
  return TDVC_OK;
}

template <class Backend>
int run_loop(const LoopCall& c, Backend&& be) {
  const tdvc_ar_loop* l = c.l;
  int nmax = 0;
  if (const int rc = loop_args(c.who, l, &nmax)) return rc;
  if (const int rc = be.check(c)) return rc;
  tdvc_conv_desc d[8];
  for (int k = 0; k < l->nconvs; ++k) d[k] = l->convs[k];
  const int B = l->y_hat.N;
  int rc = be.begin(c, nmax);
  long o = 0;
  for (int s = 0; s < l->nsteps && rc == TDVC_OK; ++s) {
    const int n = l->step_sizes ? l->step_sizes[s] : 1;
    const int32_t* pos = l->pos_dev + 2 * o;
    rc = tdvc_ar_gather_batch(&l->y_hat, &l->params, pos, n, &l->x1, &l->pc, c.stream);
    for (int k = 0; k < l->nconvs && rc == TDVC_OK; ++k) {
      d[k].x.W = d[k].y.W = B * n;
      rc = tdvc_conv2d(&d[k], c.stream);
    }
    if (rc == TDVC_OK) rc = be.step(c, pos, n, o);
    o += n;
  }
  return be.end(c, rc);
}

// Encoder: quantise.  ~7 enqueues per step and no synchronisation (Python drove a step at ~0.5 ms: 0.33 s per 1080p frame for the
// two coders).  idx / sym are raster arrays.
struct EncoderSteps : LoopBackend {
  const tdvc_fmap* y;
  int step(const LoopCall& c, const int32_t* pos, int n, long) {
    return tdvc_ar_quantize_batch(y, &c.l->gp, pos, n, c.l->scale_table, c.l->ntable, nullptr, &c.l->y_hat, c.l->sym_dev, c.l->idx_dev, -1, c.stream);
  }
};

// Decoder on the B host range decoders of a call and their pinned staging buffer [2][B * nmax * M] indexes | symbols.  Per step:
// CDF indexes -> the step's indexes of all images to the host (one strided copy) and a stream wait, the B decoders in turn, the
// symbols back (one strided copy) -> quantise.  idx / sym are compact arrays in step order: image b's values of a step start H * W * M
// ints after image b - 1's on the device and are dense in `host`.  In raster order -- a step per position, 8160 strictly serial
// steps per coder at 1080p, compressai's bitstream -- compact row k is raster row h * W + w.  Driving that from Python cost ~230 us
// per position (3.7 s per 1080p frame); here a step is seven enqueues.  One image is one row, copied plainly: a hipMemcpy2DAsync
// costs ~8 us more than a hipMemcpyAsync, twice per step of a loop whose step is 50-100 us
struct HostDecoderSteps : LoopBackend {
  const uint8_t* const* data; const int64_t* nbytes; const tdvc_cdf_tables* t;
  void* dec[256] = {};
  int B = 0;
  long half = 0;
  int32_t* host = nullptr;
  ~HostDecoderSteps() {
    for (int b = 0; b < B; ++b) if (dec[b]) tdvc_rans_decoder_destroy(dec[b]);
    if (host) (void)hipHostFree(host);
  }
  int check(const LoopCall& c) {
    TDVC_CHECK(data && nbytes && t && t->cdfs && t->sizes && t->offsets, "%s: null argument: the decoder needs the strings, their sizes and the CDF tables", c.who);
    for (int b = 0; b < c.l->y_hat.N; ++b) TDVC_CHECK(data[b] && nbytes[b] >= 4, "%s: image %d: null / empty string", c.who, b);
    TDVC_CHECK(c.l->y_hat.N <= 256, "%s: the host range decoders take at most 256 images per call, got %d", c.who, c.l->y_hat.N);
    return TDVC_OK;
  }
  int begin(const LoopCall& c, int nmax) {
    B = c.l->y_hat.N;
    half = (long)B * nmax * c.l->y_hat.C;
    for (int b = 0; b < B; ++b)
      if (!(dec[b] = tdvc_rans_decoder_create(data[b], nbytes[b]))) return TDVC_EINVAL;
    const hipError_t err = hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(int32_t) * 2 * (size_t)half, hipHostMallocDefault);
    if (err != hipSuccess) { host = nullptr; tdvc_set_error("%s: hipHostMalloc failed: %s", c.who, hipGetErrorString(err)); return (int)err; }
    return TDVC_OK;
  }
  int step(const LoopCall& c, const int32_t* pos, int n, long o) {
    const tdvc_ar_loop* l = c.l;
    const tdvc_fmap& yh = l->y_hat;
    const int M = yh.C;
    hipStream_t st = ST(c.stream);
    int rc = tdvc_ar_indexes_batch(&l->gp, pos, n, B, l->scale_table, l->ntable, M, yh.H, yh.W, l->idx_dev, o, c.stream);
    if (rc != TDVC_OK) return rc;
    int32_t *idx_at = l->idx_dev + o * M, *sym_at = l->sym_dev + o * M;
    const long cnt = (long)n * M;
    const size_t wb = sizeof(int32_t) * (size_t)cnt, pb = sizeof(int32_t) * (size_t)yh.H * yh.W * M;
    hipError_t err = B == 1 ? hipMemcpyAsync(host, idx_at, wb, hipMemcpyDeviceToHost, st) : hipMemcpy2DAsync(host, wb, idx_at, pb, wb, (size_t)B, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);     // also: the previous step's upload has left `host`
    if (err != hipSuccess) { tdvc_set_error("%s: copy / sync failed: %s", c.who, hipGetErrorString(err)); return (int)err; }
    for (int b = 0; b < B; ++b)
      if ((rc = tdvc_rans_decoder_decode(dec[b], host + b * cnt, cnt, t->cdfs, t->stride, t->sizes, t->offsets, host + half + b * cnt))) return rc;
    err = B == 1 ? hipMemcpyAsync(sym_at, host + half, wb, hipMemcpyHostToDevice, st) : hipMemcpy2DAsync(sym_at, pb, host + half, wb, wb, (size_t)B, hipMemcpyHostToDevice, st);
    if (err != hipSuccess) { tdvc_set_error("%s: upload failed: %s", c.who, hipGetErrorString(err)); return (int)err; }
    return tdvc_ar_quantize_batch(nullptr, &l->gp, pos, n, l->scale_table, l->ntable, l->sym_dev, &yh, l->sym_dev, l->idx_dev, o, c.stream);
  }
  int end(const LoopCall& c, int rc) {
    (void)hipStreamSynchronize(ST(c.stream));                  // before the pinned buffer is freed
    return rc;
  }
};

// Decoder of lane-split streams with the range decoder on the device.  The B strings are validated and uploaded behind their table,
// B + 1 copies from the caller's memory, then per step ar_decode_lanes_batch_kernel (B workgroups): the encoder's enqueue count and
// like it no synchronisation until the images are done; then the B sticky `bad` words come back with the one stream wait of the
// call.  Nothing is allocated here (a pinned staging buffer per call cost 0.3-0.5 ms, a fifth of a 448 x 256 loop).
struct LaneDecoderSteps : LoopBackend {
  const uint8_t* const* data; const int64_t* nbytes; uint8_t* stream_dev; int64_t stream_cap; uint32_t* state_dev; const tdvc_cdf_tables_dev* t; int32_t* bad_image;
  int B = 0, L = 0;
  int64_t total = 0;
  uint32_t table[2 * 4096];
  int check(const LoopCall& c) {
    TDVC_CHECK(data && nbytes && stream_dev && state_dev && t && t->cdf16 && t->starts && t->sizes && t->offsets, "%s: null argument", c.who);
    B = c.l->y_hat.N;
    TDVC_CHECK(B <= 4096, "%s: at most 4096 images per call, got %d", c.who, B);
    for (int b = 0; b < B; ++b) {
      int Lb = 0;
      if (const char* why = tdvc_lanes_check(data[b], nbytes[b], c.l->y_hat.C, &Lb)) { tdvc_set_error("%s: image %d: %s", c.who, b, why); return TDVC_EINVAL; }
      TDVC_CHECK(b == 0 || Lb == L, "%s: image %d declares %d lanes, image 0 %d: all images of a call must have the same lane count", c.who, b, Lb, L);
      L = Lb;
    }
    TDVC_CHECK(L == 64 || L == 128, "%s: the device decoder takes 64 or 128 lanes (L = %d)", c.who, L);
    total = tdvc_ar_lanes_batch_layout(nbytes, B, L, table);
    if (total < 0) return (int)total;
    TDVC_CHECK(total <= stream_cap, "%s: the device stream buffer holds %lld bytes, the strings and their table need %lld", c.who, (long long)stream_cap, (long long)total);
    return TDVC_OK;
  }
  int begin(const LoopCall& c, int) {
    // table | containers; the padding between them stays as it is: the kernels read a container's length table and payload only
    hipError_t err = hipMemcpyAsync(stream_dev, table, sizeof(uint32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, ST(c.stream));
    for (int b = 0; b < B && err == hipSuccess; ++b) err = hipMemcpyAsync(stream_dev + table[2 * b], data[b], (size_t)nbytes[b], hipMemcpyHostToDevice, ST(c.stream));
    if (err != hipSuccess) { tdvc_set_error("%s: upload failed: %s", c.who, hipGetErrorString(err)); return (int)err; }
    return tdvc_ar_lanes_init_batch(stream_dev, total, reinterpret_cast<const uint32_t*>(stream_dev), B, L, state_dev, c.stream);
  }
  int step(const LoopCall& c, const int32_t* pos, int n, long o) {
    return tdvc_ar_decode_lanes_step_batch(&c.l->gp, pos, n, c.l->scale_table, c.l->ntable, stream_dev, total, reinterpret_cast<const uint32_t*>(stream_dev), L, t, state_dev,
                                           &c.l->y_hat, c.l->sym_dev, c.l->idx_dev, o, c.stream);
  }
  int end(const LoopCall& c, int rc) {
    hipStream_t st = ST(c.stream);
    const long sw = (long)L * kLaneStateWords + 1;             // state words per image
    uint32_t* bad = table;                                     // the table's place, once its upload is done (stream order): B words
    hipError_t err;
    if (rc == TDVC_OK) {
      err = hipMemcpy2DAsync(bad, sizeof(uint32_t), state_dev + (long)L * kLaneStateWords, sizeof(uint32_t) * (size_t)sw, sizeof(uint32_t), (size_t)B, hipMemcpyDeviceToHost, st);
      if (err != hipSuccess) { tdvc_set_error("%s: reading the error words failed: %s", c.who, hipGetErrorString(err)); rc = (int)err; }
    }
    err = hipStreamSynchronize(st);
    if (rc == TDVC_OK && err != hipSuccess) { tdvc_set_error("%s: stream wait failed: %s", c.who, hipGetErrorString(err)); rc = (int)err; }
    for (int b = 0; b < B && rc == TDVC_OK; ++b)
      if (bad[b]) {
        if (bad_image) *bad_image = b;
        tdvc_set_error("%s: image %d: corrupt or exhausted lane-split stream (a lane ran out of words or met an impossible code)", c.who, b);
        rc = TDVC_EINVAL;
      }
    return rc;
  }
};
}  // namespace

extern "C" int tdvc_ar_wavefront_batch(const tdvc_ar_loop* loop, const tdvc_fmap* y, const uint8_t* const* data, const int64_t* nbytes, const tdvc_cdf_tables* tables,
                                       void* stream) {
  TdvcLoopLaunches count;
  TDVC_CHECK((data != nullptr) != (y != nullptr), "tdvc_ar_wavefront_batch: give y (encoder) or data (decoder), not both");
  const LoopCall c = {"tdvc_ar_wavefront_batch", loop, stream};
  return y ? run_loop(c, EncoderSteps{{}, y}) : run_loop(c, HostDecoderSteps{{}, data, nbytes, tables});
}

extern "C" int tdvc_ar_decode_serial_batch(const tdvc_ar_loop* loop, const uint8_t* const* data, const int64_t* nbytes, const tdvc_cdf_tables* tables, void* stream) {
  TdvcLoopLaunches count;
  return run_loop({"tdvc_ar_decode_serial_batch", loop, stream}, HostDecoderSteps{{}, data, nbytes, tables});
}

extern "C" int tdvc_ar_wavefront_lanes_batch(const tdvc_ar_loop* loop, const uint8_t* const* data, const int64_t* nbytes, uint8_t* stream_dev, int64_t stream_cap,
                                             uint32_t* state_dev, const tdvc_cdf_tables_dev* tables, int32_t* bad_image, void* stream) {
  TdvcLoopLaunches count;
  if (bad_image) *bad_image = -1;
  return run_loop({"tdvc_ar_wavefront_lanes_batch", loop, stream}, LaneDecoderSteps{{}, data, nbytes, stream_dev, stream_cap, state_dev, tables, bad_image});
}
