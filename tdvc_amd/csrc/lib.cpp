// Library-level pieces of libtdvc_hip.so: ABI version, thread-local error text, per-device scratch pages.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include <map>
#include <mutex>
#include <utility>

#include "../../include/tdvc_hip.h"

static thread_local char g_err[512] = "";

void tdvc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// the descriptors of ABI 13 as tdvc_amd/_lib.py declares them to ctypes (tests/test_lib_abi.py asserts the same numbers there)
static_assert(sizeof(tdvc_cdf_tables) == 32 && offsetof(tdvc_cdf_tables, ncdfs) == 28, "tdvc_cdf_tables layout");
static_assert(sizeof(tdvc_cdf_tables_dev) == 40 && offsetof(tdvc_cdf_tables_dev, ncdfs) == 36, "tdvc_cdf_tables_dev layout");
static_assert(sizeof(tdvc_ar_loop) == 272 && offsetof(tdvc_ar_loop, sym_dev) == 264, "tdvc_ar_loop layout");
static_assert(sizeof(tdvc_lf_tail_desc) == 168 && offsetof(tdvc_lf_tail_desc, slope) == 160, "tdvc_lf_tail_desc layout");
static_assert(sizeof(tdvc_lanes_enc) == 104 && offsetof(tdvc_lanes_enc, info) == 96, "tdvc_lanes_enc layout");
static_assert(sizeof(tdvc_rate_chain) == 224 && offsetof(tdvc_rate_chain, bits) == 208, "tdvc_rate_chain layout");

extern "C" int tdvc_abi_version(void) { return 19; }   // 19: tdvc_rate_branch, tdvc_rate_join (tdvc_rate_chain): a coder's rate branch on a side stream; 18: tdvc_conv_wgrad_bias_split, tdvc_conv_wgrad_partials_split (conv_wgrad_split_kernel); 17: tdvc_conv2d_split, tdvc_pack_conv_weights_indexed_bf16x3 (csrc/conv_split.hip); 16: tdvc_dcn_columns / tdvc_dcn_col2im / tdvc_dcn_col2im_det take fp32 maps (all of one dtype), tdvc_dcn_col2im_tile, tdvc_add_flow_backward / tdvc_bcast_add_act_backward / tdvc_upsample2x_backward / tdvc_match_gather_backward take fp32 maps, tdvc_spynet_level_input_backward an fp32 dcat8; 15: tdvc_dcn_fused takes fp32 maps (x and om fp32, y fp32 or fp16, `w` the fp32 packing: csrc/dcn_f32.hip), tdvc_add_flow / tdvc_bcast_add_act / tdvc_upsample2x / tdvc_avgpool_k / tdvc_match_gather take fp32 maps, tdvc_spynet_level_input an fp32 cat8; 14: tdvc_lf_tail, tdvc_lf_tail_supported (tdvc_lf_tail_desc); 13: the context loop's arguments as descriptors (tdvc_ar_loop, tdvc_cdf_tables, tdvc_cdf_tables_dev, tdvc_lanes_enc): new parameter lists of tdvc_ar_wavefront_batch, tdvc_ar_decode_serial_batch, tdvc_ar_wavefront_lanes_batch, tdvc_ar_decode_lanes_step_batch, tdvc_ar_encode_lanes_batch, tdvc_rans_encode_lanes_dev_ref; 12: device encoder of lane-split streams (tdvc_ar_encode_lanes_*, tdvc_rans_encode_lanes_dev_ref); 11: tdvc_conv_desc::flow, tdvc_conv_flow_supported, tdvc_scale_act_res3, tdvc_avgpool2_pyramid; 10: a single image is B = y_hat->N = 1 of the tdvc_ar_*_batch entry points; removed: tdvc_ar_gather, tdvc_ar_quantize, tdvc_ar_indexes, tdvc_ar_lanes_init, tdvc_ar_decode_lanes_step, tdvc_ar_decode_serial, tdvc_ar_wavefront, tdvc_ar_wavefront_lanes; 9: batched context loop (tdvc_ar_*_batch), tdvc_ar_last_loop_launches; 8: per-image launch predicate, tdvc_frames_changed, out-of-place bcast_T; 7: launch predicate, tdvc_frame_changed; 6: lane-split y streams (tdvc_*_lanes*); 5: tdvc_conv_select; 4: tdvc_conv_desc::chan_sum; 3: tdvc_prepare_device, SE-pool conv epilogue, deterministic col2im
extern "C" const char* tdvc_last_error(void) { return g_err; }

// ---- launch predicate (tdvc_set_predicate): a device flag the predicated kernels (conv_c8, conv_pair, conv_row, avgpool_k) read at
// their top; a launcher of one of them takes it with tdvc_launch_predicate() right before its launch, and tdvc_launch_status() -- the
// tail of EVERY launching entry point -- closes the launch with tdvc_note_launch(): the query then says whether that launch carried it.
static thread_local const int* g_pred = nullptr;
static thread_local int g_pred_taken = 0, g_pred_last = 0;
// the per-image form (tdvc_set_predicate_images): n flags, one per image of a launch of exactly n images; the two forms exclude each other
static thread_local const int* g_pred_img = nullptr;
static thread_local int g_pred_img_n = 0;

extern "C" int tdvc_set_predicate(const int* flag) {
  if (reinterpret_cast<uintptr_t>(flag) & 3) { tdvc_set_error("tdvc_set_predicate: flag must be 4-byte aligned"); return TDVC_EINVAL; }
  if (flag && g_pred_img) { tdvc_set_error("tdvc_set_predicate: a per-image predicate is set (clear it first)"); return TDVC_EINVAL; }
  g_pred = flag;
  return TDVC_OK;
}
extern "C" int tdvc_set_predicate_images(const int* flags, int n) {
  if (!flags || n == 0) { g_pred_img = nullptr; g_pred_img_n = 0; return TDVC_OK; }
  if (reinterpret_cast<uintptr_t>(flags) & 3) { tdvc_set_error("tdvc_set_predicate_images: flags must be 4-byte aligned"); return TDVC_EINVAL; }
  if (n < 1 || n > TDVC_MAX_PREDICATE_IMAGES) { tdvc_set_error("tdvc_set_predicate_images: 1 <= n <= %d images, got %d", TDVC_MAX_PREDICATE_IMAGES, n); return TDVC_EINVAL; }
  if (g_pred) { tdvc_set_error("tdvc_set_predicate_images: a launch predicate is set (clear it first)"); return TDVC_EINVAL; }
  g_pred_img = flags; g_pred_img_n = n;
  return TDVC_OK;
}
const int* tdvc_launch_predicate_images(int N) {
  if (!g_pred_img || N != g_pred_img_n) return nullptr;      // a launch of another image count runs in full
  g_pred_taken = 1;
  return g_pred_img;
}
extern "C" int tdvc_last_launch_predicated(void) { return g_pred_last; }
const int* tdvc_launch_predicate() {
  g_pred_taken = g_pred != nullptr;
  return g_pred;
}
// ---- launch counter: kernel enqueues of this thread, for tdvc_ar_last_loop_launches().  tdvc_note_launch() counts the launch it closes.
static thread_local long g_launches = 0, g_loop_launches = 0;
void tdvc_note_launch() {
  g_pred_last = g_pred_taken;
  g_pred_taken = 0;
  ++g_launches;
}
long tdvc_launch_count() { return g_launches; }
void tdvc_set_loop_launches(long n) { g_loop_launches = n; }
extern "C" int64_t tdvc_ar_last_loop_launches(void) { return g_loop_launches; }

// ---- per-device scratch: a page of zeros nobody writes (DMA source of out-of-image halo pixels) and a dump page nobody
// reads (store target of lanes outside a strip).  One allocation per device, created under a mutex on the first launch that
// needs it on THAT device (a process driving several GPUs gets one page each); the allocation is synchronous, so a caller
// that captures launches into a graph calls tdvc_prepare_device() once before the capture.
namespace {
constexpr int kMaxDev = 64;
constexpr size_t kZeroBytes = 4096, kDumpBytes = 16384;
std::mutex g_scratch_mu;
unsigned char* g_scratch[kMaxDev] = {};
}  // namespace

// -> 0 and the two pointers, or a HIP error code (tdvc_last_error() says which)
int tdvc_scratch_pages(const void** zeros, void** dump) {
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess || dev < 0 || dev >= kMaxDev) {
    tdvc_set_error("scratch pages: hipGetDevice failed or device index %d out of range: %s", dev, hipGetErrorString(err));
    return err != hipSuccess ? (int)err : TDVC_EINVAL;
  }
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  if (!g_scratch[dev]) {
    unsigned char* p = nullptr;
    err = hipMalloc(reinterpret_cast<void**>(&p), kZeroBytes + kDumpBytes);
    if (err == hipSuccess) err = hipMemset(p, 0, kZeroBytes + kDumpBytes);
    if (err == hipSuccess) err = hipDeviceSynchronize();      // the fill runs on the null stream: complete before a launch on ANY stream reads the page
    if (err != hipSuccess) {
      if (p) (void)hipFree(p);
      tdvc_set_error("scratch pages: allocation on device %d failed: %s", dev, hipGetErrorString(err));
      return (int)err;
    }
    g_scratch[dev] = p;
  }
  if (zeros) *zeros = g_scratch[dev];
  if (dump) *dump = g_scratch[dev] + kZeroBytes;
  return TDVC_OK;
}

extern "C" int tdvc_prepare_device(void) { return tdvc_scratch_pages(nullptr, nullptr); }

// ---- a coder's rate branch on a side stream (tdvc_rate_branch / tdvc_rate_join).  One side stream per (device, main stream) with a fork
// event and a done event per slot, created on first use and never destroyed; `pending` says which done events a join has to wait for.
// All of it under one mutex: a call is ~20 enqueues, and two threads that share a main stream share its side stream.
namespace {
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, done[TDVC_RATE_BRANCHES] = {};
  bool pending[TDVC_RATE_BRANCHES] = {};
};
std::mutex g_side_mu;
std::map<std::pair<int, void*>, SideStream> g_side;

int hip_fail(const char* who, const char* what, hipError_t e) {
  tdvc_set_error("%s: %s failed: %s", who, what, hipGetErrorString(e));
  return (int)e;
}

// the side stream of (current device, main) with its events, created on first use; g_side_mu is held
int side_stream(const char* who, void* main, SideStream** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(who, "hipGetDevice", e);
  SideStream& s = g_side[{dev, main}];
  if (!s.stream) {
    SideStream n;
    e = hipStreamCreateWithFlags(&n.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&n.fork, hipEventDisableTiming);
    for (int i = 0; i < TDVC_RATE_BRANCHES && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&n.done[i], hipEventDisableTiming);
    if (e != hipSuccess) {
      for (hipEvent_t ev : n.done) if (ev) (void)hipEventDestroy(ev);
      if (n.fork) (void)hipEventDestroy(n.fork);
      if (n.stream) (void)hipStreamDestroy(n.stream);
      return hip_fail(who, "creating the side stream", e);
    }
    s = n;
  }
  *out = &s;
  return TDVC_OK;
}

int rate_chain_args(const tdvc_rate_chain* c) {
  if (!c || !c->convs || !c->eb_params || !c->eb_partial || !c->gc_partial || !c->bits || !c->z.p || !c->z_hat.p || !c->y.p || !c->gp.p) {
    tdvc_set_error("tdvc_rate_branch: null argument");
    return TDVC_EINVAL;
  }
  if (c->nconvs < 1 || c->nconvs > TDVC_RATE_MAX_CONVS || c->eb_after < 1 || c->eb_after > c->nconvs) {
    tdvc_set_error("tdvc_rate_branch: 1 <= eb_after <= nconvs <= %d expected, got eb_after %d, nconvs %d", TDVC_RATE_MAX_CONVS, c->eb_after, c->nconvs);
    return TDVC_EINVAL;
  }
  if (c->which < 0 || c->which >= TDVC_RATE_BRANCHES) {
    tdvc_set_error("tdvc_rate_branch: slot %d out of range (%d slots)", c->which, TDVC_RATE_BRANCHES);
    return TDVC_EINVAL;
  }
  return TDVC_OK;
}
}  // namespace

extern "C" int tdvc_rate_branch(const tdvc_rate_chain* c, void* main_stream) {
  if (const int rc = rate_chain_args(c)) return rc;
  std::lock_guard<std::mutex> lk(g_side_mu);
  SideStream* s = nullptr;
  if (const int rc = side_stream("tdvc_rate_branch", main_stream, &s)) return rc;
  if (s->pending[c->which]) {
    tdvc_set_error("tdvc_rate_branch: slot %d has a branch that was not joined (tdvc_rate_join)", c->which);
    return TDVC_EINVAL;
  }
  hipError_t e = hipEventRecord(s->fork, reinterpret_cast<hipStream_t>(main_stream));
  if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, s->fork, 0);
  if (e != hipSuccess) return hip_fail("tdvc_rate_branch", "the fork", e);      // nothing was enqueued on the side stream: nothing is pending
  void* side = s->stream;
  int rc = TDVC_OK;
  for (int k = 0; k < c->nconvs && rc == TDVC_OK; ++k) {
    rc = c->split ? tdvc_conv2d_split(&c->convs[k], side) : tdvc_conv2d(&c->convs[k], side);
    if (rc == TDVC_OK && k + 1 == c->eb_after)
      rc = tdvc_eb_forward(&c->z, c->eb_params, nullptr, &c->z_hat, c->bits + 1, c->eb_partial, c->eb_partial_cap, side);
  }
  if (rc == TDVC_OK) rc = tdvc_gc_forward(&c->y, &c->gp, nullptr, c->bits, c->gc_partial, c->gc_partial_cap, side);
  // whatever the launches said, the done event is recorded behind what did get enqueued: the join waits for exactly that
  e = hipEventRecord(s->done[c->which], s->stream);
  if (e != hipSuccess) return rc != TDVC_OK ? rc : hip_fail("tdvc_rate_branch", "recording the done event", e);
  s->pending[c->which] = true;
  return rc;
}

extern "C" int tdvc_rate_join(void* main_stream, int which) {
  if (which < 0 || which >= TDVC_RATE_BRANCHES) {
    tdvc_set_error("tdvc_rate_join: slot %d out of range (%d slots)", which, TDVC_RATE_BRANCHES);
    return TDVC_EINVAL;
  }
  std::lock_guard<std::mutex> lk(g_side_mu);
  if (g_side.empty()) return TDVC_OK;              // no branch was ever forked (also: no device)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TDVC_OK;
  const auto it = g_side.find({dev, main_stream});
  if (it == g_side.end() || !it->second.pending[which]) return TDVC_OK;
  it->second.pending[which] = false;               // a failed wait is not retried: the slot is free either way
  const hipError_t e = hipStreamWaitEvent(reinterpret_cast<hipStream_t>(main_stream), it->second.done[which], 0);
  return e == hipSuccess ? TDVC_OK : hip_fail("tdvc_rate_join", "hipStreamWaitEvent", e);
}
