// Lane-split y streams (order = "lanes"): the symbols of one image are split over L independent rANS sub-streams, symbol
// (step, k, c) of the wavefront sequence going to lane c % L.  This header holds what the host reference decoder
// (rans.cpp) and the device decoder (ar_context.hip: ar_decode_lanes_kernel) share: the container layout, the lane state
// and the decode-one-symbol routine.  The arithmetic is the single-stream coder's (rans64, 32-bit words, 16-bit CDF
// precision, 4-bit bypass digits); lane l's sub-stream is exactly what tdvc_rans_encode emits for lane l's symbols.
//
// Container: 4 bytes {'L', 1, L, 0}, L little-endian uint16 sub-stream lengths in 32-bit words, the L sub-streams.
//
// Every loop below is bounded independently of the stream's contents and no read leaves [lane begin, lane end): a read
// past the lane's end returns 0 and sets `bad`, a bypass digit count above 8 sets `bad` (the encoder never emits one:
// `raw` has 32 bits), and so does a symbol search that finds no bin.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define TDVC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TDVC_HD inline
#endif

constexpr int kLanesHeaderBytes = 4;
constexpr uint8_t kLanesMagic = 'L', kLanesVersion = 1;
constexpr int kLanesMaxWords = 65535;          // per lane: the length table holds uint16 values

struct TdvcLane {
  uint64_t x;          // rans64 state
  uint32_t pos, end;   // next word / one past the lane's last word, as word indexes into the payload
  uint32_t bad;        // sticky: the lane ran out of words or met an impossible code
};

// offset of the payload (the first lane's first word) in a container of L lanes
TDVC_HD int64_t tdvc_lanes_payload_offset(int L) { return kLanesHeaderBytes + 2 * (int64_t)L; }

TDVC_HD uint32_t tdvc_lane_word(TdvcLane& st, const uint8_t* payload) {
  if (st.pos >= st.end) { st.bad = 1; return 0; }
  const uint8_t* p = payload + 4 * (int64_t)st.pos++;
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const uint32_t*>(p);                  // the device payload is 4-byte aligned (L even), little-endian
#else
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

TDVC_HD void tdvc_lane_renorm(TdvcLane& st, const uint8_t* payload) {
  if (st.x < (1ull << 31)) st.x = (st.x << 32) | tdvc_lane_word(st, payload);
}

TDVC_HD uint32_t tdvc_lane_bits4(TdvcLane& st, const uint8_t* payload) {
  const uint32_t v = (uint32_t)(st.x & 15u);
  st.x >>= 4;
  tdvc_lane_renorm(st, payload);
  return v;
}

// lane l owns words [begin, begin + len) of the payload, clipped to the payload's `nwords`; its state starts as the
// single-stream decoder's does, from the sub-stream's first two words
TDVC_HD void tdvc_lane_init(TdvcLane& st, const uint8_t* payload, uint32_t begin, uint32_t len, uint32_t nwords) {
  st.x = 0; st.bad = 0;
  st.pos = begin < nwords ? begin : nwords;
  st.end = len <= nwords - st.pos ? st.pos + len : nwords;
  if (st.pos != begin || st.end != begin + len) st.bad = 1;
  const uint64_t lo = tdvc_lane_word(st, payload), hi = tdvc_lane_word(st, payload);
  st.x = lo | (hi << 32);
}

// A CDF table as the decode routine reads it: cdf(i) -> entry i, cdf.inner(i) -> the same for i < size - 1.  The host reads the coder's int32 rows; the kernel reads a
// packed uint16 copy out of LDS (ar_context.hip).
struct TdvcCdf32 {
  const int32_t* p;
  TDVC_HD uint32_t operator()(int32_t i) const { return (uint32_t)p[i]; }
  TDVC_HD uint32_t inner(int32_t i) const { return (uint32_t)p[i]; }          // an entry known not to be the table's last
};

// One symbol of table `cdf` (cdf_size entries, the last one 1 << 16) out of the lane: -> symbol value minus the table's
// offset, i.e. what tdvc_rans_decode returns before it adds offsets[ci].  The bin search is a binary search for the
// smallest s with cdf(s + 1) > cum: on a non-decreasing table that is the s the single-stream decoder's linear scan
// stops at (zero-width-repaired width-1 bins included), in at most 2 + log2(cdf_size) probes.  (An 8-ary search, seven
// independent probes per round and log8 rounds, was measured on the device and is slower: 123 against 112 ms per 1080p
// frame at 64 lanes.  One wave per SIMD is bound by the instructions it issues, not by the latency of an LDS probe.)
template <typename Cdf>
TDVC_HD int32_t tdvc_lane_decode(TdvcLane& st, const uint8_t* payload, const Cdf& cdf, int32_t cdf_size) {
  const int32_t max_value = cdf_size - 2;
  if (max_value < 0) { st.bad = 1; return 0; }
  const uint32_t cum = (uint32_t)(st.x & 0xFFFFu);
  int32_t lo = 0, hi = max_value;                          // the last bin needs no probe: it is what remains
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;                    // mid < max_value: entry mid + 1 is inside the table, and not its last
    if (cdf.inner(mid + 1) > cum) hi = mid; else lo = mid + 1;
  }
  if (!(cdf(lo + 1) > cum)) { st.bad = 1; return 0; }      // no bin holds cum (a table that does not end at 1 << 16)
  const uint32_t start = cdf(lo), range = cdf(lo + 1) - start;
  st.x = (uint64_t)range * (st.x >> 16) + cum - start;
  tdvc_lane_renorm(st, payload);
  int32_t value = lo;
  if (value == max_value) {                                // out-of-table symbol: digit count, then 4-bit digits
    const uint32_t nb = tdvc_lane_bits4(st, payload);
    if (nb > 8) { st.bad = 1; return 0; }
    uint32_t raw = 0;
    for (uint32_t j = 0; j < nb; ++j) raw |= tdvc_lane_bits4(st, payload) << (4 * j);
    value = (int32_t)(raw >> 1);
    if (raw & 1) value = -value - 1; else value += max_value;
  }
  return value;
}

// Host-side check of a container against its byte count and the channel count: -> NULL and L, or what is wrong.
inline const char* tdvc_lanes_check(const uint8_t* data, int64_t nbytes, int M, int* L_out) {
  if (!data || nbytes < kLanesHeaderBytes) return "shorter than its header";
  if (data[0] != kLanesMagic || data[1] != kLanesVersion || data[3] != 0) return "not a lane-split stream (magic / version)";
  const int L = data[2];
  if (L < 1 || M < 1 || M % L != 0) return "the lane count does not divide the channel count";
  const int64_t off = tdvc_lanes_payload_offset(L);
  if (nbytes < off) return "shorter than its length table";
  int64_t words = 0;
  for (int l = 0; l < L; ++l) {
    const int len = data[kLanesHeaderBytes + 2 * l] | (data[kLanesHeaderBytes + 2 * l + 1] << 8);
    if (len < 2) return "a lane is shorter than its 8-byte final state";
    words += len;
    if (off + 4 * words > nbytes) return "a lane's length exceeds the rest of the stream";
  }
  if (off + 4 * words != nbytes) return "the lanes' lengths do not add up to the stream's size";
  *L_out = L;
  return nullptr;
}
