// Stand-alone host program for the encoder of lane-split streams that runs on the device, through its host twin
// tdvc_rans_encode_lanes_dev_ref (tdvc_amd/csrc/rans.cpp, over the encode routine of rans_lane.h): byte equality with
// tdvc_rans_encode_lanes, round trips, and a scratch region that is too small.  Meant to be compiled together with rans.cpp for
// the host with -fsanitize=address,undefined (tests/test_rans_lanes_enc_cpu.py does that); every buffer is a heap allocation of
// exactly the size handed to the coder, so a write past a region, the scratch or the output is the sanitizer's to find.
// Exit status 0: everything as expected.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
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

// the twin's call: the buffers as a tdvc_lanes_enc, the tables as a tdvc_cdf_tables
static int twin(const int32_t* sym, const int32_t* idx, int B, int H, int W, int M, const int32_t* pos, int npos, int L, const tdvc_cdf_tables& t, uint32_t* scratch,
                int64_t lane_words, int64_t scratch_cap_words, uint8_t* out, int64_t out_stride, int64_t out_cap, uint32_t* info) {
  const tdvc_lanes_enc e = {sym, idx, B, H, W, M, pos, npos, L, scratch, lane_words, scratch_cap_words, out, out_stride, out_cap, info};
  return tdvc_rans_encode_lanes_dev_ref(&e, &t);
}

int main() {
  // tables as in rans_lanes_main.cpp: random pmfs through tdvc_pmf_to_quantized_cdf, one wide Gaussian among them
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
  const tdvc_cdf_tables tabs = {cdfs.data(), sizes.data(), offsets.data(), stride, ntab};
  const int M = 128, B = 2;
  // 6 and 8 bypass digits; the extremes stay 4096 inside +-(1 << 30) so that tdvc_rans_encode's `2 * (value - max_value)` and
  // `-2 * value - 1`, int products, stay representable whatever the table's offset (the lane routine forms them wider)
  const int32_t extremes[4] = {1000000, -1000000, (1 << 30) - 4096, -(1 << 30) + 4096};
  for (int L : {64, 128})
    for (int grid = 0; grid < 3; ++grid) {
      const int H = grid == 0 ? 1 : grid == 1 ? 5 : 12, W = grid == 0 ? 1 : grid == 1 ? 7 : 20;
      std::vector<int32_t> pos;                             // anti-diagonals w + 3 h
      for (int t = 0; t < W + 3 * (H - 1); ++t)
        for (int h = 0; h < H; ++h)
          if (t - 3 * h >= 0 && t - 3 * h < W) { pos.push_back(h); pos.push_back(t - 3 * h); }
      const int npos = H * W;
      EXPECT((int)pos.size() == 2 * npos, "position list");
      const size_t N = (size_t)npos * M;
      std::vector<int32_t> sym(B * N), idx(B * N);
      for (size_t i = 0; i < B * N; ++i) {
        const int t = (int)(rnd() % ntab);
        idx[i] = t;
        sym[i] = offsets[t] + (int32_t)(rnd() % (uint32_t)(sizes[t] - 1));
        if (rnd() % 100 < 3) sym[i] += (rnd() & 1) ? 30 + (int32_t)(rnd() % 100000) : -30 - (int32_t)(rnd() % 100000);
        if (i >= N && rnd() % 100 < 5) sym[i] = extremes[rnd() % 4];        // the second image: 6 and 8 bypass digits too
      }
      const int64_t words = tdvc_ar_encode_lanes_scratch_words(npos, M, L), ostride = tdvc_ar_encode_lanes_out_bytes(npos, M, L);
      EXPECT(words >= 2 && ostride >= 4 + 2 * L + 8 * L && ostride % 16 == 0, "sizes: %lld %lld %s", (long long)words, (long long)ostride, g_err);
      std::vector<uint32_t> scratch((size_t)(B * L * words)), info(2 * B, 7);
      uint8_t* out = (uint8_t*)aligned_alloc(16, (size_t)(B * ostride));
      int rc = twin(sym.data(), idx.data(), B, H, W, M, pos.data(), npos, L, tabs, scratch.data(), words, (int64_t)scratch.size(), out, ostride, B * ostride, info.data());
      EXPECT(rc == 0, "twin L=%d %dx%d: %s", L, H, W, g_err);
      for (int b = 0; b < B && rc == 0; ++b) {
        EXPECT(info[2 * b + 1] == 0 && info[2 * b] > 0 && (int64_t)info[2 * b] <= ostride, "image %d: status %u, %u bytes", b, info[2 * b + 1], info[2 * b]);
        // the host coder's input: the position list's order
        std::vector<int32_t> gs(N), gi(N), dec(N, 0x7FFFFFFF);
        for (int p = 0; p < npos; ++p) {
          const size_t e = (size_t)b * N + ((size_t)pos[2 * p] * W + pos[2 * p + 1]) * M;
          memcpy(&gs[(size_t)p * M], &sym[e], M * sizeof(int32_t));
          memcpy(&gi[(size_t)p * M], &idx[e], M * sizeof(int32_t));
        }
        std::vector<uint8_t> ref(8 * N + 72 * (size_t)L + 64);
        const int64_t nb = tdvc_rans_encode_lanes(gs.data(), gi.data(), npos, M, L, cdfs.data(), stride, sizes.data(), offsets.data(), ref.data(), (int64_t)ref.size());
        EXPECT(nb == (int64_t)info[2 * b] && memcmp(ref.data(), out + b * ostride, (size_t)nb) == 0, "image %d L=%d %dx%d: twin differs from tdvc_rans_encode_lanes (%lld / %u bytes)",
               b, L, H, W, (long long)nb, info[2 * b]);
        std::vector<uint8_t> s(out + b * ostride, out + b * ostride + info[2 * b]);       // exact-size copy
        const int r = tdvc_rans_decode_lanes(s.data(), (int64_t)s.size(), gi.data(), npos, M, cdfs.data(), stride, sizes.data(), offsets.data(), dec.data());
        EXPECT(r == 0 && dec == gs, "round trip image %d L=%d %dx%d: rc %d %s", b, L, H, W, r, g_err);
      }
      free(out);
      // scratch deliberately too small: 4 words per lane, buffers of exactly that size
      if (grid > 0) {
        const int64_t w4 = 4, os4 = (4 + 2 * L + 4 * L * w4 + 15) / 16 * 16;
        std::vector<uint32_t> sc4((size_t)(B * L * w4)), info4(2 * B, 7);
        uint8_t* out4 = (uint8_t*)aligned_alloc(16, (size_t)(B * os4));
        memset(out4, 0xEE, (size_t)(B * os4));
        rc = twin(sym.data(), idx.data(), B, H, W, M, pos.data(), npos, L, tabs, sc4.data(), w4, (int64_t)sc4.size(), out4, os4, B * os4, info4.data());
        EXPECT(rc == 0, "small scratch L=%d: %s", L, g_err);
        for (int b = 0; b < B; ++b) EXPECT(info4[2 * b] == 0 && info4[2 * b + 1] == 2, "small scratch image %d: bytes %u status %u", b, info4[2 * b], info4[2 * b + 1]);
        for (int64_t i = 0; i < B * os4; ++i) if (out4[i] != 0xEE) { EXPECT(false, "small scratch: output byte %lld written", (long long)i); break; }
        free(out4);
      }
    }
  // arguments
  {
    std::vector<int32_t> z(128, 0);
    std::vector<uint32_t> sc(64 * 8), info(2);
    uint8_t* out = (uint8_t*)aligned_alloc(16, 4096);
    const int32_t pos[2] = {0, 0};
    EXPECT(twin(z.data(), z.data(), 1, 1, 1, 96, pos, 1, 64, tabs, sc.data(), 8, 512, out, 4096, 4096, info.data()) != 0, "L=64 with M=96 accepted");
    EXPECT(twin(z.data(), z.data(), 1, 1, 1, 128, pos, 1, 64, tabs, sc.data(), 8, 511, out, 4096, 4096, info.data()) != 0, "scratch capacity below B * L * lane_words accepted");
    EXPECT(twin(z.data(), z.data(), 1, 1, 1, 128, pos, 1, 64, tabs, sc.data(), 8, 512, out, 2048, 4096, info.data()) != 0, "output stride below the bound accepted");
    // a position outside the image and an index outside the tables: flagged, never read
    const int32_t far[2] = {3, 0};
    EXPECT(twin(z.data(), z.data(), 1, 1, 1, 128, far, 1, 64, tabs, sc.data(), 8, 512, out, 4096, 4096, info.data()) == 0 && info[1] == 2, "position outside the image: status %u", info[1]);
    std::vector<int32_t> wild(128, 1 << 20);
    EXPECT(twin(z.data(), wild.data(), 1, 1, 1, 128, pos, 1, 64, tabs, sc.data(), 8, 512, out, 4096, 4096, info.data()) == 0 && info[1] == 2, "index outside the tables: status %u", info[1]);
    EXPECT(tdvc_rans_encode_lanes_dev_ref(nullptr, &tabs) != 0 && tdvc_rans_encode_lanes_dev_ref(nullptr, nullptr) != 0, "null descriptors accepted");
    free(out);
  }
  printf(g_fail ? "%d failures\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
