// tdvc_conv2d: where every forward conv, data-gradient conv and GDN pool enters the library.  Validation, the kernel switches
// and the ONE ordered table that decides which of the conv kernels runs a descriptor.  The decision is host arithmetic on the
// descriptor alone: tdvc_conv_select answers it without a device, tdvc_conv2d launches what it answers.
#include <stdlib.h>

#include "conv_common.h"

using convk::ConvParams;
// each kernel's own conditions and its launcher live next to the kernel
bool conv_v2_eligible(const tdvc_conv_desc* d, int Ho, int Wo); int launch_conv_v2(const ConvParams& p, int cout_blocks, int N, hipStream_t st);
bool conv_v3_eligible(const tdvc_conv_desc* d, int Ho, int Wo); int launch_conv_v3(const ConvParams& p, int cout_blocks, int N, hipStream_t st);
bool conv_v5_eligible(const tdvc_conv_desc* d, int Ho, int Wo); int launch_conv_v5(const ConvParams& p, int cout_blocks, int N, hipStream_t st); int conv_v5_chan_sum_rows(int Ho, int Wo, int cout_blocks, int N);
bool conv_v7_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_conv_v7(const ConvParams& p, int cout_blocks, int N, hipStream_t st);
bool conv_v9_eligible(const tdvc_conv_desc* d, int Ho, int Wo, bool v3_ok); int launch_conv_v9(const ConvParams& p, int ck8, int cout_tiles32, int N, hipStream_t st);
bool conv_v10_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_conv_v10(const ConvParams& p, int cout_blocks, int N, hipStream_t st);
bool conv_v11_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_conv_v11(const ConvParams& p, int cout_blocks, int N, hipStream_t st);
int conv_row_geometry(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_conv_row(int geo, const ConvParams& p, int N, hipStream_t st);
bool conv_c8_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_conv_c8(const ConvParams& p, int N, hipStream_t st);
bool conv_n16_eligible(const tdvc_conv_desc* d, int Ho, int Wo); int launch_conv_n16(const ConvParams& p, int N, hipStream_t st);
bool gdn128_eligible(const tdvc_conv_desc* d, const ConvParams& p, int Ho, int Wo); int launch_gdn128(const ConvParams& p, int N, hipStream_t st);
int conv_direct_lds_bytes(const tdvc_conv_desc* d);
int conv_cout_tiles(int cout);
int launch_conv_direct(const ConvParams& p, int ck8, int stride, int N, hipStream_t st);
int conv_f32_validate(const tdvc_conv_desc* d, int& Ho, int& Wo);

// ---- kernel switches ---------------------------------------------------------------------------------------------------------
// TDVC_CONV_V1 switches every kernel but the direct one off (v2 has no variable of its own), TDVC_CONV_NO_<X> one of them.  The
// environment is read once and wins over the setters below, which tests, tools and A/B benchmarks use to send the same layers
// to the next kernel of the table.
namespace {
const char* const kSwitchEnv[convk::SW_COUNT] = {nullptr, "TDVC_CONV_NO_V3", "TDVC_CONV_NO_V5", "TDVC_CONV_NO_V7", "TDVC_CONV_NO_V9", "TDVC_CONV_NO_V10",
                                                 "TDVC_CONV_NO_V11", "TDVC_CONV_NO_ROW", "TDVC_CONV_NO_C8", "TDVC_CONV_NO_N16", "TDVC_CONV_NO_GDN128", "TDVC_CONV_NO_HEAD3"};
int g_enabled[convk::SW_COUNT] = {1, 1, 1, 1, 1, 1, 1, 15, 1, 1, 1, 1};       // conv_row: one bit per geometry (conv_row_geometry)
long g_v9_work_limit = 1L << 20;
}  // namespace

int convk::conv_on(int id) {
  static const struct EnvOff {
    bool off[convk::SW_COUNT];
    EnvOff() {
      const bool v1 = getenv("TDVC_CONV_V1") != nullptr;
      for (int i = 0; i < convk::SW_COUNT; ++i) off[i] = v1 || (kSwitchEnv[i] && getenv(kSwitchEnv[i]) != nullptr);
    }
  } env;
  return id == convk::SW_NONE ? 1 : (env.off[id] ? 0 : g_enabled[id]);
}
long convk::conv_v9_work_limit() { return g_v9_work_limit; }

extern "C" void tdvc_debug_enable_conv_v9(int enable) { g_enabled[convk::SW_V9] = enable != 0; }
extern "C" void tdvc_debug_enable_conv_v10(int enable) { g_enabled[convk::SW_V10] = enable != 0; }
extern "C" void tdvc_debug_enable_conv_v11(int enable) { g_enabled[convk::SW_V11] = enable != 0; }
extern "C" void tdvc_debug_enable_conv_row(int mask) { g_enabled[convk::SW_ROW] = mask; }
extern "C" void tdvc_debug_enable_conv_c8(int enable) { g_enabled[convk::SW_C8] = enable != 0; }
extern "C" void tdvc_debug_enable_conv_n16(int enable) { g_enabled[convk::SW_N16] = enable != 0; }
extern "C" void tdvc_debug_enable_gdn128(int enable) { g_enabled[convk::SW_GDN128] = enable != 0; }
// conv_n16's RGB-head form (conv_head3.hip): off, the layer runs on conv_n16's own kernel; the name the dispatch reports does not change
extern "C" void tdvc_debug_enable_conv_head3(int enable) { g_enabled[convk::SW_HEAD3] = enable != 0; }
extern "C" void tdvc_debug_set_conv_v9_work_limit(long v) { g_v9_work_limit = v; }

// ---- the table ---------------------------------------------------------------------------------------------------------------
namespace {

struct Pick {                 // what a launch needs besides ConvParams
  const tdvc_conv_desc* d;
  int Ho, Wo;
  int geo;                    // conv_row: geometry id
  int ck8() const { return d->ck / 8; }
  int N() const { return d->x.N; }
  int cout_blocks() const { return conv_cout_tiles(d->cout) / 2; }        // 64 output channels each
};

struct Entry {
  const char* name;           // as tdvc_last_conv_kernel() reports it
  int sw;                     // switched off: the entry is skipped
  bool (*eligible)(Pick& k, const ConvParams& p);
  int (*launch)(const Pick& k, const ConvParams& p, hipStream_t st);
  // `only` descriptors may run on this entry alone: when it does not take one (ineligible, or switched off), the descriptor is
  // rejected with `only_msg` instead of walking on
  bool (*only)(const tdvc_conv_desc* d);
  const char* only_msg;
};

bool v3_on_and_eligible(const Pick& k) { return convk::conv_on(convk::SW_V3) && conv_v3_eligible(k.d, k.Ho, k.Wo); }

// temporal 1x1 conv + broadcast add + LeakyReLU over the slices at y: conv_mfma_v5's lean epilogue in its BCAST form
bool bcast_eligible(Pick& k, const ConvParams& p) {
  const tdvc_conv_desc* d = k.d;
  return d->bcast_T == 4 && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0 && d->cout == 64 && d->y.C == 64 && d->y.sp >= 4 * 64 &&
         d->y.dtype == TDVC_F16 && d->out_mode == TDVC_OUT_NHWC && d->act == TDVC_ACT_NONE && !d->gdn && !d->res2.p &&
         // res: the SOURCE of the four slices (out-of-place form), never a residual
         (!d->res.p || (d->res.dtype == TDVC_F16 && d->res.C == 64 && d->res.sp >= 4 * 64 && d->res.N == d->y.N && d->res.H == d->y.H && d->res.W == d->y.W)) &&
         !d->square_input && !d->round_before_act && d->bias && d->bcast_slope >= 0.f && d->bcast_slope <= 1.f && conv_v5_eligible(d, k.Ho, k.Wo) &&
         convk::conv_is_lean(p);
}
int bcast_launch(const Pick& k, const ConvParams& p, hipStream_t st) {
  ConvParams q = p;
  q.simple = 2;
  q.slope = 1.f;
  return launch_conv_v5(q, 1, k.N(), st);
}
bool row_eligible(Pick& k, const ConvParams& p) { return (k.geo = conv_row_geometry(k.d, p, k.Ho, k.Wo)) >= 0; }

constexpr char kNameV5[] = "conv_mfma_v5", kNameDirect[] = "conv_mfma<%d,%d,%d>";       // the two entries conv2d_impl knows by name

const Entry kTable[] = {
    // ---- forms that one kernel alone implements
    {"conv_mfma_v5(bcast)", convk::SW_V5, bcast_eligible, bcast_launch, [](const tdvc_conv_desc* d) { return d->bcast_T != 0; },
     "tdvc_conv2d: bcast_T needs a plain 1x1 / stride 1 conv to 64 channels of >= 8192 pixels, y (and res, the optional source of the slices) a 64-channel window of a buffer with >= 4 slices, bcast_T == 4"},
    {"conv_row(s2d)", convk::SW_ROW, [](Pick& k, const ConvParams& p) { return k.d->s2d && row_eligible(k, p); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_row(k.geo, p, k.N(), st); }, nullptr, nullptr},
    {"conv_mfma_v3(s2d)", convk::SW_V3, [](Pick& k, const ConvParams&) { return k.d->s2d && conv_v3_eligible(k.d, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v3(p, k.cout_blocks(), k.N(), st); },
     [](const tdvc_conv_desc* d) { return d->s2d != 0; }, "tdvc_conv2d: s2d conv not eligible for the stage-pipelined kernel"},
    // ---- small maps: split-K over the channel chunks (<= LARGE_MAP_PIXELS output pixels over the batch)
    {"conv_mfma_v9", convk::SW_V9, [](Pick& k, const ConvParams&) { return conv_v9_eligible(k.d, k.Ho, k.Wo, v3_on_and_eligible(k)); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v9(p, k.ck8(), conv_cout_tiles(k.d->cout), k.N(), st); }, nullptr, nullptr},
    // ---- large maps, the most specific kernel first
    {"gdn128", convk::SW_GDN128, [](Pick& k, const ConvParams& p) { return gdn128_eligible(k.d, p, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_gdn128(p, k.N(), st); }, nullptr, nullptr},
    {kNameV5, convk::SW_V5, [](Pick& k, const ConvParams&) { return conv_v5_eligible(k.d, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v5(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    {"conv_c8", convk::SW_C8, [](Pick& k, const ConvParams& p) { return conv_c8_eligible(k.d, p, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_c8(p, k.N(), st); }, nullptr, nullptr},
    {"conv_n16", convk::SW_N16, [](Pick& k, const ConvParams&) { return conv_n16_eligible(k.d, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_n16(p, k.N(), st); }, nullptr, nullptr},
    {"conv_row", convk::SW_ROW, row_eligible,
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_row(k.geo, p, k.N(), st); }, nullptr, nullptr},
    {"conv_mfma_v10", convk::SW_V10, [](Pick& k, const ConvParams& p) { return conv_v10_eligible(k.d, p, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v10(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    {"conv_mfma_v7", convk::SW_V7, [](Pick& k, const ConvParams& p) { return conv_v7_eligible(k.d, p, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v7(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    {"conv_mfma_v11", convk::SW_V11, [](Pick& k, const ConvParams& p) { return conv_v11_eligible(k.d, p, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v11(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    // ---- any map: the tiled kernels, then the direct one
    {"conv_mfma_v3", convk::SW_V3, [](Pick& k, const ConvParams&) { return conv_v3_eligible(k.d, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v3(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    {"conv_mfma_v2", convk::SW_V2, [](Pick& k, const ConvParams&) { return conv_v2_eligible(k.d, k.Ho, k.Wo); },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_v2(p, k.cout_blocks(), k.N(), st); }, nullptr, nullptr},
    {kNameDirect, convk::SW_NONE, [](Pick& k, const ConvParams&) { return conv_direct_lds_bytes(k.d) <= 64 * 1024; },
     [](const Pick& k, const ConvParams& p, hipStream_t st) { return launch_conv_direct(p, k.ck8(), k.d->stride, k.N(), st); },
     [](const tdvc_conv_desc*) { return true; }, nullptr},
};

// The first entry that is switched on and takes the descriptor; nullptr: rejected, tdvc_last_error() says why.
const Entry* select(Pick& k, const ConvParams& p) {
  for (const Entry& e : kTable) {
    if (convk::conv_on(e.sw) && e.eligible(k, p)) return &e;
    if (e.only && e.only(k.d)) {
      if (e.only_msg) tdvc_set_error("%s", e.only_msg);
      else tdvc_set_error("tdvc_conv2d: LDS plan %d bytes too large for the direct kernel (use tdvc_conv_plan)", conv_direct_lds_bytes(k.d));
      return nullptr;
    }
  }
  return nullptr;
}

void kernel_name(const Entry* e, const Pick& k, char (&out)[48]) {
  if (e->name == kNameDirect) snprintf(out, sizeof(out), kNameDirect, k.ck8(), conv_cout_tiles(k.d->cout) == 1 ? 1 : 2, k.d->stride);
  else snprintf(out, sizeof(out), "%s", e->name);
}

// validation of the fp16 form -> TDVC_OK, the output map and the launch parameters (all but the walk direction)
int prepare(const tdvc_conv_desc* d, ConvParams& p, int& Ho, int& Wo) {
  TDVC_CHECK(fmap_ok16(d->x), "tdvc_conv2d: input must be an fp16 fmap with C,sp %% 8 == 0 and 16-byte aligned");
  TDVC_CHECK(d->w && aligned16(d->w), "tdvc_conv2d: weights null/unaligned");
  TDVC_CHECK(d->stride == 1 || d->stride == 2, "tdvc_conv2d: stride %d unsupported", d->stride);
  TDVC_CHECK(d->ntaps >= 1 && d->ntaps <= TDVC_MAX_TAPS && d->kh >= 1 && d->kh <= 7 && d->kw >= 1 && d->kw <= 7,
             "tdvc_conv2d: bad kernel %dx%d ntaps=%d", d->kh, d->kw, d->ntaps);
  TDVC_CHECK(d->ck == 8 || d->ck == 16 || d->ck == 32 || d->ck == 64, "tdvc_conv2d: bad ck %d", d->ck);
  TDVC_CHECK(d->cout >= 1, "tdvc_conv2d: cout");
  for (int t = 0; t < d->ntaps; ++t)
    TDVC_CHECK(d->tap_dy[t] >= 0 && d->tap_dy[t] < d->kh && d->tap_dx[t] >= 0 && d->tap_dx[t] < d->kw,
               "tdvc_conv2d: tap %d out of the %dx%d window", t, d->kh, d->kw);
  Ho = (d->x.H + 2 * d->pad - d->kh) / d->stride + 1;
  Wo = (d->x.W + 2 * d->pad - d->kw) / d->stride + 1;
  if (d->s2d) {
    TDVC_CHECK(d->kh == 2 && d->kw == 2 && d->stride == 1 && d->pad == 1 && d->ntaps == 4 && d->ck == 32 && !d->square_input && !d->gdn,
               "tdvc_conv2d: s2d expects the virtual 2x2 / stride 1 / pad 1 conv packed with ck=32");
    TDVC_CHECK((d->x.H % 2) == 0 && (d->x.W % 2) == 0 && (d->x.C % 32) == 0 && d->cout >= 64,
               "tdvc_conv2d: s2d needs even H, W, C %% 32 == 0 and cout >= 64 (got %dx%dx%d, cout %d)", d->x.H, d->x.W, d->x.C, d->cout);
    Ho = d->x.H / 2;
    Wo = d->x.W / 2;
  }
  TDVC_CHECK(Ho > 0 && Wo > 0, "tdvc_conv2d: empty output");
  TDVC_CHECK((long)Ho * Wo * 4 < 2147483647L && (long)d->x.H * d->x.W < 2147483647L, "tdvc_conv2d: image too large (pixel indices are 32-bit)");

  const int shuf = d->out_mode == TDVC_OUT_SHUFFLE2;
  if (d->out_mode == TDVC_OUT_NCHW_F32) {
    TDVC_CHECK(d->y.p && d->y.N == d->x.N, "tdvc_conv2d: NCHW output null / batch mismatch");
  } else {
    TDVC_CHECK(d->y.dtype == TDVC_F32 ? fmap_ok32(d->y) : fmap_ok16(d->y), "tdvc_conv2d: bad output fmap");
    TDVC_CHECK(d->y.N == d->x.N && d->y.H == (shuf ? 2 * Ho : Ho) && d->y.W == (shuf ? 2 * Wo : Wo),
               "tdvc_conv2d: output geometry %dx%d does not match conv result %dx%d%s", d->y.H, d->y.W, Ho, Wo,
               shuf ? " (x2 shuffle)" : "");
    if (shuf) TDVC_CHECK((d->cout % 128) == 0, "tdvc_conv2d: SHUFFLE2 needs cout %% 128 == 0");
    if (d->y.dtype == TDVC_F16) TDVC_CHECK((d->y.C % 8) == 0, "tdvc_conv2d: fp16 output C %% 8");
  }
  if (d->gdn) {
    TDVC_CHECK(fmap_ok16(d->aux) && d->aux.H == Ho && d->aux.W == Wo && d->aux.N == d->x.N && d->aux.C >= d->cout &&
                   !shuf && (d->cout % 64) == 0,
               "tdvc_conv2d: GDN aux fmap mismatch");
  }
  if (d->res.p) {
    TDVC_CHECK(d->res.dtype == TDVC_F32 ? fmap_ok32(d->res) : fmap_ok16(d->res), "tdvc_conv2d: bad residual fmap");
    TDVC_CHECK(d->res.N == d->x.N && d->res.H == (shuf ? 2 * Ho : Ho) && d->res.W == (shuf ? 2 * Wo : Wo),
               "tdvc_conv2d: residual geometry mismatch");
  }
  if (d->res2.p) {
    TDVC_CHECK(fmap_ok16(d->res2) && d->res2.N == d->x.N && d->res2.H == (shuf ? 2 * Ho : Ho) && d->res2.W == (shuf ? 2 * Wo : Wo),
               "tdvc_conv2d: bad second residual fmap");
  }
  if (d->bias) TDVC_CHECK(aligned16(d->bias), "tdvc_conv2d: bias unaligned");

  memset(&p, 0, sizeof(p));
  p.x = reinterpret_cast<const half_t*>(d->x.p); p.x_sn = d->x.sn; p.x_sp = d->x.sp;
  p.H = d->x.H; p.W = d->x.W; p.Cin = d->x.C;
  p.w = reinterpret_cast<const half_t*>(d->w); p.bias = d->bias;
  p.y = to_dev(d->y); p.Ho = Ho; p.Wo = Wo; p.cout = d->cout;
  p.aux = d->gdn ? to_dev(d->aux) : null_fmap();
  p.res = d->res.p ? to_dev(d->res) : null_fmap();
  p.res2 = d->res2.p ? to_dev(d->res2) : null_fmap();
  p.ntaps = d->ntaps; p.kh = d->kh; p.kw = d->kw; p.pad = d->pad;
  p.in_stride = d->stride;
  p.s2d = d->s2d; p.Corig = d->x.C;
  p.bcast_T = d->bcast_T; p.bcast_slope = d->bcast_slope;
  p.nchunks = d->s2d ? (4 * d->x.C) / d->ck : (d->x.C + d->ck - 1) / d->ck;
  p.steps = (d->ntaps * (d->ck / 8) + 1) / 2;
  p.square = d->square_input; p.gdn = d->gdn; p.act = d->act; p.slope = d->slope;
  p.round16 = d->round_before_act; p.out_mode = d->out_mode;
  memcpy(p.tap_dy, d->tap_dy, sizeof(p.tap_dy));
  memcpy(p.tap_dx, d->tap_dx, sizeof(p.tap_dx));
  p.tiles_x = (Wo + 31) / 32;                          // the direct kernel's 8 x 32 tiles; the other launchers set their own
  if (conv_cout_tiles(d->cout) > 1 && convk::conv_is_simple(p)) {
    p.simple = convk::conv_is_lean(p) ? 2 : 1;       // 2: the lean packed-fp16 form of the transposed epilogue (conv_common.h)
    p.slope = convk::conv_simple_slope(p);
  }
  return TDVC_OK;
}

thread_local char g_last_kernel[48] = "";

// Tile-walk direction.  The 256 MB Infinity Cache sits in front of HBM and every layer streams a map slightly larger
// than it (64 channels x 1088 x 1920 fp16 = 267 MB): when layer l+1 reads, in the same raster order, what layer l just
// wrote, the head of the map has already been pushed out by its tail and nothing hits.  Consecutive launches therefore
// walk the tile raster in OPPOSITE directions: the consumer starts on the producer's most recently written tiles (and on
// the tail of the residual the producer read), which are still resident.  Launch parity is per host thread (one stream
// of launches per rank); any order is correct, the alternation only decides what hits.
thread_local unsigned g_walk_parity = 0;
int g_walk_mode = -1;      // -1: read TDVC_CONV_WALK once (0 = always forward, 1 = alternate [default])
int next_walk_reverse() {
  if (g_walk_mode < 0) { const char* e = getenv("TDVC_CONV_WALK"); g_walk_mode = e ? atoi(e) : 1; }
  return g_walk_mode == 1 ? (int)(g_walk_parity++ & 1u) : 0;
}

// tdvc_conv_desc::flow: honoured by the lean epilogue of conv_mfma_v5 (any number of 64-channel blocks), not together with chan_sum
bool conv_flow_ok(const tdvc_conv_desc* d, const Entry* e, const ConvParams& p) {
  return e && e->name == kNameV5 && p.simple == 2 && !d->chan_sum;
}
// the map itself: fp32, >= 2 channels, the output's geometry
bool flow_map_ok(const tdvc_conv_desc* d, int Ho, int Wo) {
  return fmap_ok32(d->flow) && d->flow.C >= 2 && d->flow.N == d->x.N && d->flow.H == Ho && d->flow.W == Wo;
}
constexpr char kFlowMsg[] = "tdvc_conv2d: flow on a conv whose kernel does not add it (tdvc_conv_flow_supported() == 0), with chan_sum, or not an fp32 map of >= 2 channels and the output's geometry";

enum Query { LAUNCH = 0, QUERY_ROWS = 1, QUERY_FLOW = 2 };
// QUERY_ROWS / QUERY_FLOW: validate and select as tdvc_conv2d would, but return the rows of tdvc_conv_desc::chan_sum / whether the kernel
// honours tdvc_conv_desc::flow instead of launching
int conv2d_impl(const tdvc_conv_desc* d, void* stream, int query) {
  const bool query_rows = query == QUERY_ROWS;
  TDVC_CHECK(d, "tdvc_conv2d: null descriptor");
  if (d->x.dtype == TDVC_F32) {           // fp32 islands (pnet.py:33,57): fp32 activations + fp32 packing -> conv_f32.hip
    if (query != LAUNCH) return 0;
    TDVC_CHECK(!d->chan_sum, "tdvc_conv2d: chan_sum is not available on the fp32 path (tdvc_conv_chan_sum_rows() == 0)");
    TDVC_CHECK(!d->flow.p, "tdvc_conv2d: flow is not available on the fp32 path (tdvc_conv_flow_supported() == 0)");
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_f32");
    return tdvc_conv2d_f32(d, stream);
  }
  ConvParams p;
  Pick k = {d, 0, 0, -1};
  if (const int rc = prepare(d, p, k.Ho, k.Wo)) return rc;
  p.reverse = query != LAUNCH ? 0 : next_walk_reverse();      // once per launching call, never on a query
  const Entry* e = select(k, p);
  // fused channel sums (tdvc_conv_desc::chan_sum): the lean epilogue of conv_mfma_v5 with one block of 64 output channels
  const bool csum_ok = e && e->name == kNameV5 && k.cout_blocks() == 1 && p.simple == 2;
  if (query_rows) return csum_ok ? conv_v5_chan_sum_rows(k.Ho, k.Wo, 1, k.N()) : 0;
  if (query == QUERY_FLOW) return conv_flow_ok(d, e, p) && (!d->flow.p || flow_map_ok(d, k.Ho, k.Wo)) ? 1 : 0;
  TDVC_CHECK(!d->chan_sum || (csum_ok && (reinterpret_cast<uintptr_t>(d->chan_sum) & 15) == 0),
             "tdvc_conv2d: chan_sum on a conv whose kernel has no fused channel sum (tdvc_conv_chan_sum_rows() == 0) or unaligned");
  p.csum = d->chan_sum;
  if (!e) return TDVC_EINVAL;
  if (d->flow.p) {
    TDVC_CHECK(conv_flow_ok(d, e, p) && flow_map_ok(d, k.Ho, k.Wo), "%s", kFlowMsg);
    p.flow = to_dev(d->flow);
  }
  kernel_name(e, k, g_last_kernel);
  return e->launch(k, p, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

// A fused launch outside tdvc_conv2d that stands for `launches` of its launches (tdvc_lf_tail): the launches behind it walk in the
// direction they had behind the unfused sequence, so results that depend on the walk (tdvc_conv_desc::chan_sum partials) keep their bytes.
void tdvc_conv_walk_advance(int launches) { g_walk_parity += (unsigned)launches; }
// a conv entry point outside tdvc_conv2d (tdvc_conv2d_split) names its kernel for tdvc_last_conv_kernel()
void tdvc_set_last_conv_kernel(const char* name) { snprintf(g_last_kernel, sizeof(g_last_kernel), "%s", name); }

extern "C" void tdvc_debug_set_conv_walk(int mode) { g_walk_mode = mode; }
extern "C" int tdvc_conv2d(const tdvc_conv_desc* d, void* stream) { return conv2d_impl(d, stream, LAUNCH); }
extern "C" int tdvc_conv_chan_sum_rows(const tdvc_conv_desc* d) { return conv2d_impl(d, nullptr, QUERY_ROWS); }
extern "C" int tdvc_conv_flow_supported(const tdvc_conv_desc* d) { return conv2d_impl(d, nullptr, QUERY_FLOW); }
extern "C" const char* tdvc_last_conv_kernel(void) { return g_last_kernel; }

extern "C" const char* tdvc_conv_select(const tdvc_conv_desc* d) {
  static thread_local char name[48];
  if (!d) { tdvc_set_error("tdvc_conv_select: null descriptor"); return nullptr; }
  if (d->x.dtype == TDVC_F32) {
    int Ho, Wo;
    if (d->flow.p) { tdvc_set_error("%s", kFlowMsg); return nullptr; }
    return conv_f32_validate(d, Ho, Wo) == TDVC_OK ? "conv_f32" : nullptr;
  }
  ConvParams p;
  Pick k = {d, 0, 0, -1};
  if (prepare(d, p, k.Ho, k.Wo) != TDVC_OK) return nullptr;
  const Entry* e = select(k, p);
  if (!e) return nullptr;
  if (d->flow.p && !(conv_flow_ok(d, e, p) && flow_map_ok(d, k.Ho, k.Wo))) { tdvc_set_error("%s", kFlowMsg); return nullptr; }
  kernel_name(e, k, name);
  return name;
}
