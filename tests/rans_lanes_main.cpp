// Stand-alone host program for the lane-split range coder (tdvc_rans_encode_lanes / tdvc_rans_decode_lanes in
// tdvc_amd/csrc/rans.cpp): round trips and damaged streams, meant to be compiled together with rans.cpp for the host
// with -fsanitize=address,undefined (tests/test_rans_lanes_cpu.py does that).  Exit status 0: everything as expected.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/tdvc_hip.h"

static char g_err[512];
void tdvc_set_error(const char* fmt, ...) {                 // lib.cpp's, which needs the HIP runtime
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                     // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 32);
}

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

int main() {
  // tables: random pmfs through tdvc_pmf_to_quantized_cdf, one wide Gaussian (width-1 bins repaired from width 0) among them
  const int ntab = 7, stride = 2100;
  std::vector<int32_t> cdfs((size_t)ntab * stride, 0), sizes(ntab), offsets(ntab);
  for (int t = 0; t < ntab; ++t) {
    const int n = t == ntab - 1 ? 2050 : 3 + (int)(rnd() % 40);
    std::vector<float> pmf((size_t)n);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
      const double d = (i - n / 2) / (t == ntab - 1 ? 120.0 : 4.0);
      pmf[(size_t)i] = (float)(1e-9 + (t == ntab - 1 ? 1.0 : (rnd() % 1000) / 1000.0) * __builtin_exp(-0.5 * d * d));
      sum += pmf[(size_t)i];
    }
    for (auto& p : pmf) p = (float)(p / sum);
    EXPECT(tdvc_pmf_to_quantized_cdf(pmf.data(), n, 16, &cdfs[(size_t)t * stride]) == 0, "cdf %d: %s", t, g_err);
    sizes[t] = n + 1;
    offsets[t] = -(int32_t)(rnd() % 12) - (t == ntab - 1 ? 1000 : 0);
  }
  const int M = 128;
  for (int L : {1, 64, 128})
    for (int npos : {1, 16, 600}) {
      const size_t N = (size_t)npos * M;
      std::vector<int32_t> sym(N), idx(N), dec(N, 0x7FFFFFFF);
      for (size_t i = 0; i < N; ++i) {
        const int t = (int)(rnd() % ntab);
        idx[i] = t;
        sym[i] = offsets[t] + (int32_t)(rnd() % (uint32_t)(sizes[t] - 1));
        if (rnd() % 100 < 3) sym[i] += (rnd() & 1) ? 30 + (int32_t)(rnd() % 100000) : -30 - (int32_t)(rnd() % 100000);   // bypass digits
      }
      std::vector<uint8_t> out(8 * N + 72 * (size_t)L + 64);
      const int64_t nb = tdvc_rans_encode_lanes(sym.data(), idx.data(), npos, M, L, cdfs.data(), stride, sizes.data(), offsets.data(), out.data(), (int64_t)out.size());
      EXPECT(nb > 0, "encode L=%d npos=%d: %s", L, npos, g_err);
      if (nb <= 0) continue;
      std::vector<uint8_t> s(out.begin(), out.begin() + nb);       // exact-size copy: a read past the end is the sanitizer's to find
      int rc = tdvc_rans_decode_lanes(s.data(), nb, idx.data(), npos, M, cdfs.data(), stride, sizes.data(), offsets.data(), dec.data());
      EXPECT(rc == 0 && dec == sym, "round trip L=%d npos=%d: rc %d %s", L, npos, rc, g_err);
      // single lane: the payload is the single-stream coder's string, and both decoders agree on it
      if (L == 1) {
        std::vector<uint8_t> one(8 * N + 64);
        const int64_t n1 = tdvc_rans_encode(sym.data(), idx.data(), (int64_t)N, cdfs.data(), stride, sizes.data(), offsets.data(), one.data(), (int64_t)one.size());
        EXPECT(n1 == nb - 6 && memcmp(one.data(), s.data() + 6, (size_t)n1) == 0, "L=1 payload differs from tdvc_rans_encode");
        std::vector<int32_t> d1(N);
        EXPECT(tdvc_rans_decode(one.data(), n1, idx.data(), (int64_t)N, cdfs.data(), stride, sizes.data(), offsets.data(), d1.data()) == 0 && d1 == dec, "L=1 decode");
      }
      // damaged streams: an error, never a crash or a success
      auto fails = [&](std::vector<uint8_t> d, int m, const char* what) {
        std::vector<int32_t> o(N);
        const int r = tdvc_rans_decode_lanes(d.data(), (int64_t)d.size(), idx.data(), npos, m, cdfs.data(), stride, sizes.data(), offsets.data(), o.data());
        EXPECT(r != 0, "%s (L=%d npos=%d) decoded without an error", what, L, npos);
      };
      fails(std::vector<uint8_t>(s.begin(), s.end() - 4), M, "truncated by 4 bytes");
      { auto d = s; d[4] = 0xFF; d[5] = 0xFF; fails(d, M, "length entry larger than the remainder"); }
      { auto d = s; d[0] = 'X'; fails(d, M, "wrong magic byte"); }
      { auto d = s; memset(d.data() + 4 + 2 * L, 0xFF, d.size() - 4 - 2 * (size_t)L); fails(d, M, "payload of 0xFF bytes"); }
      { // the last lane cut by one word, length table adjusted: passes the header check, the lane runs out of words
        auto d = std::vector<uint8_t>(s.begin(), s.end() - 4);
        const int len = (d[4 + 2 * (L - 1)] | (d[5 + 2 * (L - 1)] << 8)) - 1;
        d[4 + 2 * (L - 1)] = (uint8_t)(len & 0xFF); d[5 + 2 * (L - 1)] = (uint8_t)(len >> 8);
        fails(d, M, "last lane cut by one word");
      }
      if (L > 1) fails(s, M + 1, "L not dividing M");
      fails(std::vector<uint8_t>(s.begin(), s.begin() + 3), M, "3-byte stream");
    }
  std::vector<int32_t> z(96, 0);
  std::vector<uint8_t> o(4096);
  EXPECT(tdvc_rans_encode_lanes(z.data(), z.data(), 1, 96, 64, cdfs.data(), stride, sizes.data(), offsets.data(), o.data(), 4096) < 0, "L=64 with M=96 encoded");
  EXPECT(tdvc_rans_encode_lanes(z.data(), z.data(), 1, 96, 48, cdfs.data(), stride, sizes.data(), offsets.data(), o.data(), 16) < 0, "16-byte output buffer accepted");
  printf(g_fail ? "%d failures\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
