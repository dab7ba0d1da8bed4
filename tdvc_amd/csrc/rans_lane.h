// Lane-split y streams (order = "lanes"): the symbols of one image are split over L independent rANS sub-streams, symbol
// (step, k, c) of the wavefront sequence going to lane c % L.  This header holds what the host reference decoder
// (rans.cpp) and the device decoder (ar_context.hip: ar_decode_lanes_kernel) share: the container layout, the lane state
// and the decode-one-symbol routine; further down, the same for the encoder of the format (host twin: rans.cpp
// tdvc_rans_encode_lanes_dev_ref, device: ar_encode_lanes_batch_kernel).  The arithmetic is the single-stream coder's (rans64, 32-bit words, 16-bit CDF
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

// ---- the encoder of the same format, one lane at a time (host twin: rans.cpp tdvc_rans_encode_lanes_dev_ref; device:
// ar_context.hip ar_encode_lanes_batch_kernel).  rANS emits its words in reverse stream order, so a lane visits its symbols last
// to first and writes its words DOWNWARD from the end of a scratch region [begin, end) of its own: when it is done its
// sub-stream is the contiguous range [pos, end), first word of the stream first.  The arithmetic is tdvc_rans_encode's, bit
// for bit.  Every loop is bounded independently of the data (a symbol is at most 1 table push + 1 count digit + 8 digits: `raw`
// has 32 bits) and no write leaves the region: a push that would sets `bad` and writes nothing.
struct TdvcEncLane {
  uint64_t x;                // rans64 state
  uint32_t pos, begin, end;  // lowest word written so far / the lane's scratch region, as word indexes into the scratch buffer
  uint32_t bad;              // sticky: the region is full, or a table is unusable
};

// Scratch words a lane of n symbols needs at most.  With w words emitted so far, (x + 1) * 2^(32 w) starts at 2^31 + 1 <= 2^32
// and grows by at most 2^16 per table push (x' = (x / r << 16) + x % r + start <= (x + 1) * 2^16 - 1) and 2^4 per bypass digit
// (x' = 16 x + d), so by at most 2^(16 + 4 * 9) = 2^52 per symbol; the state never falls below 2^31, hence
// 2^31 * 2^(32 w) <= 2^(32 + 52 n) and w <= (1 + 52 n) / 32.  The final state adds two words.  A lane above kLanesMaxWords is an
// error whatever the scratch holds, so the answer is capped at kLanesMaxWords + 1: a lane that fills such a region, or runs out
// of it, is known to be too long.
constexpr int kLanesScratchCap = kLanesMaxWords + 1;
TDVC_HD int64_t tdvc_lane_scratch_words(int64_t n) {
  if (n < 0) n = 0;
  if (n >= kLanesScratchCap) return kLanesScratchCap;        // 52 n / 32 > n: beyond the cap, and no overflow below
  const int64_t w = (31 + 52 * n) / 32 + 2;
  return w < kLanesScratchCap ? w : kLanesScratchCap;
}
// a container's size at most, from the per-lane scratch words the encoder is given: no lane of a valid container is longer
TDVC_HD int64_t tdvc_lanes_container_bound(int L, int64_t lane_words) {
  return tdvc_lanes_payload_offset(L) + 4 * (int64_t)L * (lane_words < kLanesMaxWords ? lane_words : kLanesMaxWords);
}

TDVC_HD void tdvc_enc_lane_init(TdvcEncLane& st, uint32_t begin, uint32_t end) {
  st.x = 1ull << 31; st.begin = begin; st.end = end; st.pos = end; st.bad = 0;
}
TDVC_HD void tdvc_enc_lane_word(TdvcEncLane& st, uint32_t* scratch, uint32_t w) {
  if (st.pos <= st.begin) { st.bad = 1; return; }
  scratch[--st.pos] = w;
}

// x / r and x % r for 1 <= r < 2^16 and x < r * 2^48 (the renormalised state: x < 2^47 * r), exactly: long division in three
// steps of 16 quotient bits whose partial dividends d = remainder * 2^16 + 16 more bits stay below r * 2^16 <= 2^32.  A step's
// quotient t = d / r < 2^16 is estimated in float: fl(d) and the product round by 2^-24 each, the reciprocal is within one ulp
// (2^-23; the host's division rounds correctly), so the estimate is within t * 2^-22 < 2^-6 of t and its integer part is
// floor(t) - 1, floor(t) or floor(t) + 1; the remainder d - q r, exact in 32 bits, says which, and one correction either way
// makes the step exact.  In place of a 64-bit division, which the device has no instruction for, and of three 32-bit ones:
// the reciprocal is shared by the steps and the products fit the 24-bit multiplier.
TDVC_HD uint32_t tdvc_div_step(uint32_t d, uint32_t r, float inv, uint32_t* rem) {
  uint32_t q = (uint32_t)((float)d * inv);
  int32_t m = (int32_t)(d - (q & 0x1FFFFu) * (r & 0xFFFFu));                   // q <= 2^16, r < 2^16: the masks change nothing and show the compiler a 24-bit product
  if (m < 0) { --q; m += (int32_t)r; }
  else if (m >= (int32_t)r) { ++q; m -= (int32_t)r; }
  *rem = (uint32_t)m;
  return q;
}
TDVC_HD uint64_t tdvc_divmod_u16(uint64_t x, uint32_t r, uint32_t* rem) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float inv = __builtin_amdgcn_rcpf((float)r);
#else
  const float inv = 1.0f / (float)r;
#endif
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  uint32_t r2, r1;
  const uint32_t q2 = tdvc_div_step(hi, r, inv, &r2);                          // hi < r * 2^16
  const uint32_t q1 = tdvc_div_step((r2 << 16) | (lo >> 16), r, inv, &r1);
  const uint32_t q0 = tdvc_div_step((r1 << 16) | (lo & 0xFFFFu), r, inv, rem);
  return ((uint64_t)q2 << 32) | ((uint64_t)q1 << 16) | q0;
}

TDVC_HD void tdvc_enc_lane_put(TdvcEncLane& st, uint32_t* scratch, uint32_t start, uint32_t range) {     // a table symbol, 1 <= range < 2^16
  if (st.x >= ((1ull << 31 >> 16) << 32) * range) { tdvc_enc_lane_word(st, scratch, (uint32_t)st.x); st.x >>= 32; }
  uint32_t rem;
  const uint64_t q = tdvc_divmod_u16(st.x, range, &rem);
  st.x = (q << 16) + rem + start;
}
TDVC_HD void tdvc_enc_lane_put4(TdvcEncLane& st, uint32_t* scratch, uint32_t digit) {                    // a 4-bit bypass digit
  if (st.x >= ((1ull << 31 >> 16) << 32) * (1u << 12)) { tdvc_enc_lane_word(st, scratch, (uint32_t)st.x); st.x >>= 32; }
  st.x = (st.x << 4) | digit;
}

// One symbol in two parts.  tdvc_lane_symbol: what does not depend on the lane's state -- table lookups, the escape value --
// from `value`, the symbol minus the table's offset (the kernel does this for a whole chunk of symbols at once, all threads,
// before the lanes' serial pass).  tdvc_lane_push: the pushes, tdvc_rans_encode's entries for the symbol in reverse (the caller
// walks the lane's symbols last to first): raw digits high to low, the digit count, the table symbol.
constexpr uint32_t kEncPlain = 0, kEncEscape = 1, kEncUnusable = 2;
struct TdvcEncSym {
  uint32_t start_range;      // start | range << 16: the single-stream coder holds both in 16 bits
  uint32_t raw;              // kEncEscape: the out-of-table value, -2v - 1 or 2 (v - max)
  uint32_t kind;
};
template <typename Cdf>
TDVC_HD TdvcEncSym tdvc_lane_symbol(const Cdf& cdf, int32_t cdf_size, int32_t value) {
  TdvcEncSym s = {0, 0, kEncUnusable};
  const int32_t max_value = cdf_size - 2;
  if (max_value < 0) return s;
  uint32_t kind = kEncPlain;
  if (value < 0 || value >= max_value) {
    s.raw = value < 0 ? (uint32_t)(-2 * (int64_t)value - 1) : 2u * (uint32_t)(value - max_value);
    kind = kEncEscape;
    value = max_value;
  }
  const uint32_t start = cdf(value), range = cdf(value + 1) - start;
  if (range < 1 || range > 0xFFFFu || start > 0xFFFFu) return s;
  s.start_range = start | (range << 16);
  s.kind = kind;
  return s;
}
TDVC_HD void tdvc_lane_push(TdvcEncLane& st, uint32_t* scratch, uint32_t kind, uint32_t start_range, uint32_t raw) {
  if (kind >= kEncUnusable) { st.bad = 1; return; }
  if (kind == kEncEscape) {
    int nb = 0;
    for (int j = 0; j < 8; ++j) if ((raw >> (4 * j)) != 0) nb = j + 1;
    for (int j = 7; j >= 0; --j) if (j < nb) tdvc_enc_lane_put4(st, scratch, (raw >> (4 * j)) & 15u);
    tdvc_enc_lane_put4(st, scratch, (uint32_t)nb);
  }
  tdvc_enc_lane_put(st, scratch, start_range & 0xFFFFu, start_range >> 16);
}
template <typename Cdf>
TDVC_HD void tdvc_lane_encode(TdvcEncLane& st, uint32_t* scratch, const Cdf& cdf, int32_t cdf_size, int32_t value) {
  const TdvcEncSym s = tdvc_lane_symbol(cdf, cdf_size, value);
  tdvc_lane_push(st, scratch, s.kind, s.start_range, s.raw);
}

// the lane is done: its final state, low word first in stream order -> the lane's length in words (its sub-stream is
// scratch[pos .. end))
TDVC_HD uint32_t tdvc_enc_lane_finish(TdvcEncLane& st, uint32_t* scratch) {
  tdvc_enc_lane_word(st, scratch, (uint32_t)(st.x >> 32));
  tdvc_enc_lane_word(st, scratch, (uint32_t)st.x);
  return st.end - st.pos;
}

// per-image status of the encoder: a lane that ran out of a region of kLanesScratchCap words is too long, not short of scratch
constexpr uint32_t kLanesEncOk = 0, kLanesEncTooLong = 1, kLanesEncScratch = 2;
TDVC_HD uint32_t tdvc_enc_lane_status(const TdvcEncLane& st, uint32_t len) {
  if (st.bad) return st.end - st.begin >= (uint32_t)kLanesScratchCap ? kLanesEncTooLong : kLanesEncScratch;
  return len > (uint32_t)kLanesMaxWords ? kLanesEncTooLong : kLanesEncOk;
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
