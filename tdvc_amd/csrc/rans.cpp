// Host-side range coder of the entropy stage: rANS with a 64-bit state and 32-bit renormalisation
// words, 16-bit CDF precision and 4-bit "bypass" digits for out-of-table symbols — the published
// scheme of CompressAI's `ans` extension (BufferedRansEncoder / RansDecoder over ryg_rans' rans64),
// which `Cheng2020Anchor.compress` drives from main/model/pnet.py:46-49,70-73.  It is host code
// in the reference as well; the GPU produces the symbols and CDF indexes, this packs them.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/tdvc_hip.h"
#include "rans_lane.h"

void tdvc_set_error(const char* fmt, ...);

namespace {
constexpr uint64_t kL = 1ull << 31;
constexpr int kPrec = 16;
constexpr int kBypassBits = 4;
constexpr int kMaxBypass = (1 << kBypassBits) - 1;

struct Sym { uint16_t start, range; bool bypass; };
}  // namespace

extern "C" int64_t tdvc_rans_encode(const int32_t* symbols, const int32_t* indexes, int64_t n,
                                    const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                    const int32_t* offsets, uint8_t* out, int64_t cap) {
  if (!symbols || !indexes || !cdfs || !cdf_sizes || !offsets || !out || n < 0) {
    tdvc_set_error("tdvc_rans_encode: null argument");
    return TDVC_EINVAL;
  }
  std::vector<Sym> syms;
  syms.reserve((size_t)n + 16);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t ci = indexes[i];
    const int32_t* cdf = cdfs + (int64_t)ci * cdf_stride;
    const int32_t max_value = cdf_sizes[ci] - 2;
    int32_t value = symbols[i] - offsets[ci];
    uint32_t raw = 0;
    if (value < 0) {
      raw = (uint32_t)(-2 * value - 1);
      value = max_value;
    } else if (value >= max_value) {
      raw = (uint32_t)(2 * (value - max_value));
      value = max_value;
    }
    syms.push_back({(uint16_t)cdf[value], (uint16_t)(cdf[value + 1] - cdf[value]), false});
    if (value == max_value) {
      int32_t nb = 0;
      while (nb < 8 && (raw >> (nb * kBypassBits)) != 0) ++nb;       // 8 digits hold all of raw (and raw >> 32 is undefined: the loop did not end for raw >= 1 << 28)
      int32_t v = nb;
      while (v >= kMaxBypass) {
        syms.push_back({(uint16_t)kMaxBypass, (uint16_t)(kMaxBypass + 1), true});
        v -= kMaxBypass;
      }
      syms.push_back({(uint16_t)v, (uint16_t)(v + 1), true});
      for (int32_t j = 0; j < nb; ++j) {
        const int32_t d = (raw >> (j * kBypassBits)) & kMaxBypass;
        syms.push_back({(uint16_t)d, (uint16_t)(d + 1), true});
      }
    }
  }
  std::vector<uint32_t> words;
  words.reserve(syms.size() / 2 + 4);
  uint64_t x = kL;
  for (size_t k = syms.size(); k-- > 0;) {
    const Sym s = syms[k];
    if (!s.bypass) {
      const uint64_t x_max = ((kL >> kPrec) << 32) * s.range;
      if (x >= x_max) { words.push_back((uint32_t)x); x >>= 32; }
      x = ((x / s.range) << kPrec) + (x % s.range) + s.start;
    } else {
      const uint32_t freq = 1u << (16 - kBypassBits);
      const uint64_t x_max = ((kL >> 16) << 32) * freq;
      if (x >= x_max) { words.push_back((uint32_t)x); x >>= 32; }
      x = (x << kBypassBits) | s.start;
    }
  }
  words.push_back((uint32_t)(x >> 32));
  words.push_back((uint32_t)x);
  const int64_t nbytes = (int64_t)words.size() * 4;
  if (nbytes > cap) {
    tdvc_set_error("tdvc_rans_encode: output buffer too small (%lld > %lld)", (long long)nbytes, (long long)cap);
    return TDVC_EINVAL;
  }
  // stream order = reverse emission order, little-endian words
  for (size_t k = 0; k < words.size(); ++k) {
    const uint32_t w = words[words.size() - 1 - k];
    out[4 * k + 0] = (uint8_t)(w);
    out[4 * k + 1] = (uint8_t)(w >> 8);
    out[4 * k + 2] = (uint8_t)(w >> 16);
    out[4 * k + 3] = (uint8_t)(w >> 24);
  }
  return nbytes;
}

namespace {
struct Dec {
  const uint8_t* d; int64_t nwords; int64_t pos; uint64_t x; bool bad;
  uint32_t word() {
    if (pos >= nwords) { bad = true; return 0; }
    const uint8_t* p = d + 4 * pos++;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
  void renorm() { if (x < kL) x = (x << 32) | word(); }
  uint32_t bits(int nb) { const uint32_t v = (uint32_t)(x & ((1u << nb) - 1)); x >>= nb; renorm(); return v; }
};
}  // namespace

static int dec_run(Dec& dc, const int32_t* indexes, int64_t n, const int32_t* cdfs, int32_t cdf_stride,
                   const int32_t* cdf_sizes, const int32_t* offsets, int32_t* symbols_out);

extern "C" int tdvc_rans_decode(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t n,
                                const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                const int32_t* offsets, int32_t* symbols_out) {
  if (!data || !indexes || !cdfs || !cdf_sizes || !offsets || !symbols_out || nbytes < 8 || (nbytes & 3)) {
    tdvc_set_error("tdvc_rans_decode: bad arguments (stream must be >= 8 bytes, multiple of 4)");
    return TDVC_EINVAL;
  }
  Dec dc{data, nbytes / 4, 0, 0, false};
  const uint64_t lo = dc.word(), hi = dc.word();
  dc.x = lo | (hi << 32);
  return dec_run(dc, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, symbols_out);
}

// stateful decoder (compressai RansDecoder.set_stream / decode_stream): the autoregressive decoder
// learns the CDF indexes of a position only after the previous positions are decoded
extern "C" void* tdvc_rans_decoder_create(const uint8_t* data, int64_t nbytes) {
  if (!data || nbytes < 8 || (nbytes & 3)) {
    tdvc_set_error("tdvc_rans_decoder_create: stream must be >= 8 bytes, multiple of 4");
    return nullptr;
  }
  uint8_t* copy = new uint8_t[(size_t)nbytes];
  memcpy(copy, data, (size_t)nbytes);
  Dec* dc = new Dec{copy, nbytes / 4, 0, 0, false};
  const uint64_t lo = dc->word(), hi = dc->word();
  dc->x = lo | (hi << 32);
  return dc;
}
extern "C" int tdvc_rans_decoder_decode(void* handle, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                                        int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                        int32_t* symbols_out) {
  if (!handle || !indexes || !cdfs || !cdf_sizes || !offsets || !symbols_out) {
    tdvc_set_error("tdvc_rans_decoder_decode: null argument");
    return TDVC_EINVAL;
  }
  return dec_run(*static_cast<Dec*>(handle), indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, symbols_out);
}
extern "C" void tdvc_rans_decoder_destroy(void* handle) {
  if (!handle) return;
  Dec* dc = static_cast<Dec*>(handle);
  delete[] dc->d;
  delete dc;
}

static int dec_run(Dec& dc, const int32_t* indexes, int64_t n, const int32_t* cdfs, int32_t cdf_stride,
                   const int32_t* cdf_sizes, const int32_t* offsets, int32_t* symbols_out) {
  const uint32_t mask = (1u << kPrec) - 1;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t ci = indexes[i];
    const int32_t* cdf = cdfs + (int64_t)ci * cdf_stride;
    const int32_t max_value = cdf_sizes[ci] - 2;
    const uint32_t cum = (uint32_t)(dc.x & mask);
    int32_t s = 0;
    while (s <= max_value && (uint32_t)cdf[s + 1] <= cum) ++s;
    if (s > max_value) { tdvc_set_error("tdvc_rans_decode: corrupt stream at symbol %lld", (long long)i); return TDVC_EINVAL; }
    dc.x = (uint64_t)(cdf[s + 1] - cdf[s]) * (dc.x >> kPrec) + cum - (uint32_t)cdf[s];
    dc.renorm();
    int32_t value = s;
    if (value == max_value) {
      int32_t v = (int32_t)dc.bits(kBypassBits);
      int32_t nb = v;
      while (v == kMaxBypass) { v = (int32_t)dc.bits(kBypassBits); nb += v; if (dc.bad) break; }
      uint32_t raw = 0;
      for (int32_t j = 0; j < nb && j < 8; ++j) raw |= dc.bits(kBypassBits) << (j * kBypassBits);
      value = (int32_t)(raw >> 1);
      if (raw & 1) value = -value - 1; else value += max_value;
    }
    if (dc.bad) { tdvc_set_error("tdvc_rans_decode: stream exhausted at symbol %lld", (long long)i); return TDVC_EINVAL; }
    symbols_out[i] = value + offsets[ci];
  }
  return TDVC_OK;
}

// compressai `_CXX.pmf_to_quantized_cdf` (cpp_exts/ops/ops.cpp): round to 2^precision, renormalise with
// integer division, prefix-sum, force the last entry, then repair zero-width bins by stealing one count
// from the narrowest bin wider than 1.  cdf_out has n + 1 entries.
extern "C" int tdvc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out) {
  if (!pmf || !cdf_out || n < 1 || precision < 1 || precision > 16) {
    tdvc_set_error("tdvc_pmf_to_quantized_cdf: bad arguments");
    return TDVC_EINVAL;
  }
  std::vector<uint32_t> cdf((size_t)n + 1);
  cdf[0] = 0;
  for (int i = 0; i < n; ++i) {
    const float v = pmf[i] * (float)(1 << precision);
    cdf[i + 1] = (uint32_t)(v + 0.5f >= 0.f ? (long long)(v + 0.5f) : 0);     // std::round for v >= 0
    if ((float)cdf[i + 1] - v > 0.5f) cdf[i + 1] -= 1;                          // guard the float add
  }
  uint64_t total = 0;
  for (uint32_t c : cdf) total += c;
  if (total == 0) { tdvc_set_error("tdvc_pmf_to_quantized_cdf: empty pmf"); return TDVC_EINVAL; }
  for (auto& c : cdf) c = (uint32_t)((((uint64_t)1 << precision) * c) / total);
  for (size_t i = 1; i < cdf.size(); ++i) cdf[i] += cdf[i - 1];
  cdf.back() = 1u << precision;
  const int m = (int)cdf.size();
  for (int i = 0; i < m - 1; ++i) {
    if (cdf[i] == cdf[i + 1]) {
      uint32_t best_freq = ~0u;
      int best = -1;
      for (int j = 0; j < m - 1; ++j) {
        const uint32_t f = cdf[j + 1] - cdf[j];
        if (f > 1 && f < best_freq) { best_freq = f; best = j; }
      }
      if (best == -1) { tdvc_set_error("tdvc_pmf_to_quantized_cdf: cannot repair zero-width bin"); return TDVC_EINVAL; }
      if (best < i) { for (int j = best + 1; j <= i; ++j) cdf[j]--; }
      else { for (int j = i + 1; j <= best; ++j) cdf[j]++; }
    }
  }
  for (int i = 0; i < m; ++i) cdf_out[i] = (int32_t)cdf[i];
  return TDVC_OK;
}

// ---- lane-split y streams (rans_lane.h): the same coder over L independent sub-streams, symbol c of a position in lane c % L

extern "C" int64_t tdvc_rans_encode_lanes(const int32_t* symbols, const int32_t* indexes, int64_t npos, int M, int L,
                                          const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                          const int32_t* offsets, uint8_t* out, int64_t cap) {
  if (!symbols || !indexes || !cdfs || !cdf_sizes || !offsets || !out || npos < 0) {
    tdvc_set_error("tdvc_rans_encode_lanes: null argument");
    return TDVC_EINVAL;
  }
  if (L < 1 || L > 255 || M < 1 || M % L != 0) {
    tdvc_set_error("tdvc_rans_encode_lanes: the lane count (%d) must be in [1, 255] and divide the channel count (%d)", L, M);
    return TDVC_EINVAL;
  }
  int64_t o = tdvc_lanes_payload_offset(L);
  if (cap < o) { tdvc_set_error("tdvc_rans_encode_lanes: output buffer too small"); return TDVC_EINVAL; }
  out[0] = kLanesMagic; out[1] = kLanesVersion; out[2] = (uint8_t)L; out[3] = 0;
  const int per = M / L;
  const int64_t n = npos * per;                            // symbols per lane
  // one pass over the position-major input into lane-major arrays (64 strided passes over 8 MB cost 2 ms per 1080p coder)
  std::vector<int32_t> s((size_t)(n * L)), ix((size_t)(n * L));
  for (int64_t p = 0; p < npos; ++p)
    for (int j = 0; j < per; ++j)
      for (int l = 0; l < L; ++l) {
        s[(size_t)(l * n + p * per + j)] = symbols[p * M + (int64_t)j * L + l];
        ix[(size_t)(l * n + p * per + j)] = indexes[p * M + (int64_t)j * L + l];
      }
  for (int l = 0; l < L; ++l) {
    const int64_t nb = tdvc_rans_encode(s.data() + l * n, ix.data() + l * n, n, cdfs, cdf_stride, cdf_sizes, offsets, out + o, cap - o);
    if (nb < 0) return nb;
    if (nb / 4 > kLanesMaxWords) {
      tdvc_set_error("tdvc_rans_encode_lanes: lane %d needs %lld words, the length table holds at most %d", l, (long long)(nb / 4), kLanesMaxWords);
      return TDVC_EINVAL;
    }
    out[kLanesHeaderBytes + 2 * l] = (uint8_t)((nb / 4) & 0xFF);
    out[kLanesHeaderBytes + 2 * l + 1] = (uint8_t)((nb / 4) >> 8);
    o += nb;
  }
  return o;
}

// reference decoder: what ar_decode_lanes_kernel computes, on the host, through the same tdvc_lane_decode
extern "C" int tdvc_rans_decode_lanes(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t npos, int M,
                                      const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                                      const int32_t* offsets, int32_t* symbols_out) {
  if (!data || !indexes || !cdfs || !cdf_sizes || !offsets || !symbols_out || npos < 0) {
    tdvc_set_error("tdvc_rans_decode_lanes: null argument");
    return TDVC_EINVAL;
  }
  int L = 0;
  if (const char* why = tdvc_lanes_check(data, nbytes, M, &L)) {
    tdvc_set_error("tdvc_rans_decode_lanes: %s", why);
    return TDVC_EINVAL;
  }
  const uint8_t* payload = data + tdvc_lanes_payload_offset(L);
  const uint32_t nwords = (uint32_t)((nbytes - tdvc_lanes_payload_offset(L)) / 4);
  std::vector<TdvcLane> st((size_t)L);
  uint32_t begin = 0;
  for (int l = 0; l < L; ++l) {
    const uint32_t len = (uint32_t)data[kLanesHeaderBytes + 2 * l] | ((uint32_t)data[kLanesHeaderBytes + 2 * l + 1] << 8);
    tdvc_lane_init(st[(size_t)l], payload, begin, len, nwords);
    begin += len;
  }
  for (int64_t p = 0; p < npos; ++p)
    for (int c = 0; c < M; ++c) {
      TdvcLane& ln = st[(size_t)(c % L)];
      const int32_t ci = indexes[p * M + c];
      int32_t size = cdf_sizes[ci];
      if (size > cdf_stride) size = cdf_stride;
      const int32_t v = tdvc_lane_decode(ln, payload, TdvcCdf32{cdfs + (int64_t)ci * cdf_stride}, size);
      if (ln.bad) {
        tdvc_set_error("tdvc_rans_decode_lanes: corrupt or exhausted stream in lane %d at position %lld, channel %d", c % L, (long long)p, c);
        return TDVC_EINVAL;
      }
      symbols_out[p * M + c] = v + offsets[ci];
    }
  return TDVC_OK;
}

// ---- the encoder of lane-split streams that runs on the device (ar_context.hip: ar_encode_lanes_batch_kernel), its sizes and its
// host twin: the same encode-one-symbol routine (rans_lane.h), traversal, scratch layout and assembly, on host memory

extern "C" int64_t tdvc_ar_encode_lanes_scratch_words(int64_t npos, int M, int L) {
  if (npos < 0 || M < 1 || L < 1 || M % L != 0) { tdvc_set_error("tdvc_ar_encode_lanes_scratch_words: bad sizes (npos %lld, M %d, L %d)", (long long)npos, M, L); return TDVC_EINVAL; }
  return tdvc_lane_scratch_words(npos > kLanesScratchCap ? kLanesScratchCap : npos * (M / L));
}
extern "C" int64_t tdvc_ar_encode_lanes_out_bytes(int64_t npos, int M, int L) {
  const int64_t w = tdvc_ar_encode_lanes_scratch_words(npos, M, L);
  return w < 0 ? w : (tdvc_lanes_container_bound(L, w) + 15) / 16 * 16;
}

int tdvc_encode_lanes_args(const char* who, const tdvc_lanes_enc* enc, int32_t ncdfs) {
  const auto bad = [&](const char* what) { tdvc_set_error("%s: %s", who, what); return TDVC_EINVAL; };
  if (!enc) return bad("null argument");
  const tdvc_lanes_enc& e = *enc;
  if (!e.symbols || !e.indexes || !e.pos || !e.scratch || !e.out || !e.info) return bad("null argument");
  if (e.B < 1 || e.B > 65535 || e.H < 1 || e.W < 1 || e.M < 1 || e.npos < 1 || (int64_t)e.H * e.W > 0x7FFFFFFF)
    return bad("1 <= B <= 65535 images of H x W x M symbols and npos >= 1 positions expected");
  if ((e.L != 64 && e.L != 128) || e.M % e.L != 0) return bad("64 or 128 lanes that divide the channel count expected");
  if (ncdfs < 1 || ncdfs > 64) return bad("1..64 CDF tables expected");
  if (e.lane_words < 2 || e.lane_words > kLanesScratchCap || (int64_t)e.B * e.L * e.lane_words > e.scratch_cap_words)
    return bad("2..65536 scratch words per lane expected, B * L * lane_words of them inside the scratch buffer");
  if (e.out_stride % 16 != 0 || e.out_stride < tdvc_lanes_container_bound(e.L, e.lane_words) || (int64_t)e.B * e.out_stride > e.out_cap)
    return bad("the output stride must be a multiple of 16 that holds L lanes of min(lane_words, 65535) words behind header and length table, B strides inside the output buffer");
  if ((((uintptr_t)e.symbols) | ((uintptr_t)e.indexes) | ((uintptr_t)e.pos) | ((uintptr_t)e.scratch) | ((uintptr_t)e.info)) & 3 || ((uintptr_t)e.out) & 15)
    return bad("symbols / indexes / positions / scratch / info must be 4-byte aligned, the output buffer 16-byte aligned");
  return TDVC_OK;
}

extern "C" int tdvc_rans_encode_lanes_dev_ref(const tdvc_lanes_enc* enc, const tdvc_cdf_tables* tables) {
  if (!tables || !tables->cdfs || !tables->sizes || !tables->offsets || tables->stride < 1) { tdvc_set_error("tdvc_rans_encode_lanes_dev_ref: null table pointer"); return TDVC_EINVAL; }
  if (const int rc = tdvc_encode_lanes_args("tdvc_rans_encode_lanes_dev_ref", enc, tables->ncdfs)) return rc;
  const int B = enc->B, H = enc->H, W = enc->W, M = enc->M, npos = enc->npos, L = enc->L, ncdfs = tables->ncdfs, cdf_stride = tables->stride;
  const int32_t *symbols = enc->symbols, *indexes = enc->indexes, *pos = enc->pos, *cdfs = tables->cdfs, *cdf_sizes = tables->sizes, *offsets = tables->offsets;
  const int64_t lane_words = enc->lane_words, out_stride = enc->out_stride;
  uint32_t *scratch = enc->scratch, *info = enc->info;
  uint8_t* out = enc->out;
  const int per = M / L;
  std::vector<uint32_t> lpos((size_t)L), llen((size_t)L);
  for (int b = 0; b < B; ++b) {
    const int32_t* sym = symbols + (int64_t)b * H * W * M;
    const int32_t* idx = indexes + (int64_t)b * H * W * M;
    uint32_t* sc = scratch + (int64_t)b * L * lane_words;
    uint8_t* o = out + (int64_t)b * out_stride;
    uint32_t status = 0, words = 0;
    for (int l = 0; l < L; ++l) {
      TdvcEncLane st;
      tdvc_enc_lane_init(st, (uint32_t)(l * lane_words), (uint32_t)((l + 1) * lane_words));
      for (int p = npos - 1; p >= 0; --p) {
        const int h = pos[2 * p], w = pos[2 * p + 1];
        const bool inside = h >= 0 && h < H && w >= 0 && w < W;
        for (int j = per - 1; j >= 0; --j) {
          const int64_t e = inside ? ((int64_t)h * W + w) * M + (int64_t)j * L + l : 0;
          const int32_t ci = idx[e];
          if (!inside || ci < 0 || ci >= ncdfs) { st.bad = 1; continue; }
          int32_t size = cdf_sizes[ci];
          if (size > cdf_stride) size = cdf_stride;
          tdvc_lane_encode(st, sc, TdvcCdf32{cdfs + (int64_t)ci * cdf_stride}, size, (int32_t)((uint32_t)sym[e] - (uint32_t)offsets[ci]));
        }
      }
      const uint32_t len = tdvc_enc_lane_finish(st, sc);
      const uint32_t s = tdvc_enc_lane_status(st, len);
      status = s > status ? s : status;
      lpos[(size_t)l] = st.pos; llen[(size_t)l] = len;
      words += len;
    }
    info[2 * b] = status ? 0u : (uint32_t)tdvc_lanes_payload_offset(L) + 4u * words;
    info[2 * b + 1] = status;
    if (status) continue;                                      // nothing of the container is written
    o[0] = kLanesMagic; o[1] = kLanesVersion; o[2] = (uint8_t)L; o[3] = 0;
    uint8_t* q = o + tdvc_lanes_payload_offset(L);
    for (int l = 0; l < L; ++l) {
      o[kLanesHeaderBytes + 2 * l] = (uint8_t)(llen[(size_t)l] & 0xFF);
      o[kLanesHeaderBytes + 2 * l + 1] = (uint8_t)(llen[(size_t)l] >> 8);
      for (uint32_t i = 0; i < llen[(size_t)l]; ++i, q += 4) {
        const uint32_t w = sc[lpos[(size_t)l] + i];
        q[0] = (uint8_t)w; q[1] = (uint8_t)(w >> 8); q[2] = (uint8_t)(w >> 16); q[3] = (uint8_t)(w >> 24);
      }
    }
  }
  return TDVC_OK;
}
