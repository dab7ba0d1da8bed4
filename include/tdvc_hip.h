/*
 * tdvc_hip.h — C-ABI of libtdvc_hip.so: MI355X (gfx950) kernels for TDVC's per-P-frame
 * encode / reconstruct hot path (`main/model/pnet.py::VideoCompressor.forward`).
 *
 * Boundary rules
 *   - plain pointers, sizes and a `void* stream` (a hipStream_t; NULL = default stream);
 *     no torch types.  All device pointers must be 16-byte aligned.
 *   - every entry point ENQUEUES on `stream` and returns immediately (no host sync, no
 *     allocation, graph-capture safe) — the contract of the reference's only FFI crossing,
 *     `_ext.dcn_v2_forward`, which enqueues on the current CUDA stream
 *     (main/utils/dcnv2/src/cuda/dcn_v2_cuda.cu:78).
 *   - return value: 0 on success, a negative TDVC_E* code on invalid arguments, or the
 *     positive hipError_t of a failed launch.  (The reference only printf's launch failures,
 *     src/cuda/dcn_v2_im2col_cuda.cu:346-350; here they are returned.)
 *
 * Feature maps ("fmap") are channel-innermost: element (n, y, x, c) lives at
 *     base + n*sn + (y*W + x)*sp + c            (strides in ELEMENTS)
 * so a tensor may be a channel slice of a wider buffer (concatenation without copies).
 * fp16 fmaps need C, sp and the channel offset to be multiples of 8.
 *
 * Which reference function each entry replaces is stated per declaration (file:line under
 * /root/reference).
 */
#ifndef TDVC_HIP_H
#define TDVC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDVC_OK 0
#define TDVC_EINVAL (-1)   /* bad shape / alignment / unsupported configuration */
#define TDVC_ENOSUP (-2)

/* ---------------------------------------------------------------- descriptors */
typedef struct {
  void* p;      /* device pointer to element (0,0,0,0) of the view */
  int32_t N, H, W, C;
  int64_t sn;   /* batch stride (elements) */
  int32_t sp;   /* pixel stride (elements) */
  int32_t dtype; /* TDVC_F16 or TDVC_F32 */
} tdvc_fmap;

enum { TDVC_F16 = 0, TDVC_F32 = 1 };
enum { TDVC_ACT_NONE = 0, TDVC_ACT_RELU = 1, TDVC_ACT_LRELU = 2, TDVC_ACT_CLAMP01 = 3, TDVC_ACT_SIGMOID = 4 };
enum { TDVC_GDN_NONE = 0, TDVC_GDN_FWD = 1, TDVC_GDN_INV = 2 };
enum { TDVC_OUT_NHWC = 0,       /* y is an fmap (fp16 or fp32) */
       TDVC_OUT_SHUFFLE2 = 1,   /* PixelShuffle(2): out channel o -> (c=o/4, i=(o/2)&1, j=o&1), y has 2H x 2W */
       TDVC_OUT_NCHW_F32 = 2 }; /* planar fp32 [N][C][H][W] (module boundary) */

#define TDVC_MAX_TAPS 49

typedef struct {
  tdvc_fmap x;            /* input, fp16 */
  tdvc_fmap y;            /* output view (post-shuffle geometry for SHUFFLE2) */
  const void* w;          /* weights packed by tdvc_pack_conv_weights (fp16, MFMA fragment order) */
  const float* bias;      /* [cout_pad] fp32, may be NULL */
  int32_t cout;           /* real output channels */
  int32_t ntaps;          /* taps actually evaluated (masked taps are dropped at pack time) */
  int8_t tap_dy[TDVC_MAX_TAPS], tap_dx[TDVC_MAX_TAPS]; /* tap offsets in [0,KH) x [0,KW) */
  int32_t kh, kw, stride, pad;
  int32_t ck;             /* channel chunk staged in LDS per pass: 8,16,32 or 64 (from tdvc_conv_plan) */
  int32_t square_input;   /* 1: stage x^2 (GDN norm pool) */
  int32_t gdn;            /* TDVC_GDN_*: v = aux * rsqrt(v) (FWD) or aux * sqrt(v) (INV) */
  tdvc_fmap aux;          /* GDN multiplicand (same geometry as y pre-shuffle), fp16 */
  int32_t act; float slope;
  int32_t round_before_act; /* 1: round v to fp16 before the activation (DCN quirk, dcn_v2_amp.py:67-68) */
  tdvc_fmap res;          /* residual added AFTER the activation, at output coordinates; p==NULL: none */
  tdvc_fmap res2;         /* optional second residual (fp16), same rules */
  int32_t out_mode;
  int32_t s2d;            /* 1: `x` is read through a 2x2 space-to-depth view: the virtual input is
                             (H/2, W/2, 4C) with channel q*C + c = pixel (2Y + q/2, 2X + q%2), channel c.
                             A 3x3 stride-2 pad-1 conv becomes a 2x2 stride-1 conv (kh=kw=2, pad=1 on the
                             top/left only) over that view; weights are packed for the virtual conv
                             (tdvc_amd/ops.py::pack_conv(s2d=True)).  Needs H, W even and C % 32 == 0. */
  int32_t bcast_T;        /* ABI 3.  > 0: the conv result b (1x1, stride 1, cout == y.C == 64, no activation / residual / GDN) is not
                             stored but broadcast-added over the bcast_T channel slices of width y.C that start at y:
                             y[:, t] = lrelu(y[:, t] + b), in place (y's pixel stride covers the slices) -- Bottleneck3D's temporal
                             conv + `out + temporal` + LeakyReLU (pnet.py:304-314) as ONE pass over the 4-frame buffer.  The conv
                             input may be channels of the same buffer (a 1x1 conv reads only the pixels it then overwrites).
                             ABI 8: with `res` given (fp16, 64 channels, y's geometry, pixel stride >= 4 * 64) the four slices are READ
                             at res and WRITTEN at y -- the out-of-place form, same arithmetic and traffic; res is left as it was. */
  float bcast_slope;
  float* chan_sum;        /* ABI 4.  not NULL: next to storing y the launch writes partial per-channel sums of the STORED fp16 values,
                             chan_sum[n][row][cout] for row < tdvc_conv_chan_sum_rows(d) (fp32; every row is written) -- the
                             SELayer's global average pool (inflate.py:204) without a second pass over y.  Only the convs for which
                             tdvc_conv_chan_sum_rows() returns > 0 accept it. */
  tdvc_fmap flow;         /* ABI 11.  p != NULL: an fp32 map of >= 2 channels and the output's geometry whose channel 0 is added to the even
                             and channel 1 to the odd output channels of its pixel, AFTER the bias + activation + residuals + fp16 rounding
                             of today: stored = fp16(float(fp16 result) + flow) -- byte for byte the conv followed by tdvc_add_flow
                             (pnet.py:163), without the pass over y.  Only the convs for which tdvc_conv_flow_supported() returns 1
                             accept it (the lean epilogue of conv_mfma_v5), not together with chan_sum.  p == NULL: nothing changes. */
} tdvc_conv_desc;

/* ---------------------------------------------------------------- library */
/* Library/ABI version; bumps when a struct above changes. */
int tdvc_abi_version(void);
/* Human-readable description of the last error on this thread (never NULL). */
const char* tdvc_last_error(void);
/* Creates the current device's scratch pages (a zero page the halo DMA reads, a dump page masked stores go to).  The
 * launchers create them on first use, synchronously: call this once per device before capturing launches into a graph.
 * Thread-safe; one allocation per device for the life of the process. */
int tdvc_prepare_device(void);
/* Name of the kernel the last tdvc_conv2d call on this thread dispatched to ("conv_mfma_v7", "conv_mfma<4,2,1>",
 * ...; "" before the first call).  Diagnostic for profiles and benchmarks; never NULL. */
const char* tdvc_last_conv_kernel(void);

/* ---------------------------------------------------------------- launch predicate (ABI 7)
 * Device-side skipping of work whose inputs did not change, with no host synchronisation: `flag` is one int of device memory,
 * written on the stream by an earlier launch (tdvc_frame_changed).  While a predicate is set on the calling thread (NULL clears
 * it), the launches of the PREDICATED kernels -- conv_c8, conv_pair, conv_row (tdvc_conv2d / tdvc_conv_pair dispatching to them)
 * and both kernels of tdvc_avgpool_k -- carry the pointer: every workgroup reads *flag once at its top, before any barrier,
 * LDS-DMA or store, and returns when it is 0, leaving its outputs as they were.  Every other kernel launched under a
 * predicate runs in full (correct, only not shortened).  tdvc_last_launch_predicated(): 1 when the last launching entry point
 * on this thread passed the predicate into its kernel(s), else 0. */
int tdvc_set_predicate(const int* flag);
int tdvc_last_launch_predicated(void);
/* ABI 8.  Per-image form: `flags` are n <= TDVC_MAX_PREDICATE_IMAGES ints of device memory (tdvc_frames_changed writes them).  While set
 * (thread-local; NULL or n == 0 clears it; it and tdvc_set_predicate exclude each other), a launch of conv_c8 or conv_pair over
 * exactly N == n images computes image i only when flags[i] != 0 and leaves the other images' outputs as they were.  Every workgroup
 * reads the flags once at its top (plain loads, before any barrier, LDS-DMA, weight load or store), returns when no image is active
 * and otherwise walks the job space of the ACTIVE images alone, so no workgroup idles on a skipped image; results are byte-equal to
 * the full launch.  A launch that cannot honour the flags (another kernel, N != n) runs in full and
 * tdvc_last_launch_predicated() says 0. */
#define TDVC_MAX_PREDICATE_IMAGES 4
int tdvc_set_predicate_images(const int* flags, int n);
/* flag[0] = (cur != cache), compared exactly as 16-byte integer words (NaN payloads and signed zeros count); when they differ
 * `cache` becomes a copy of `cur`, else its bytes are not touched.  fp16 maps of one geometry (N, H, W, C), each with its own
 * pixel / batch strides.  Three enqueued steps: flag = 0, compare, conditional copy. */
int tdvc_frame_changed(const tdvc_fmap* cur, tdvc_fmap* cache, int* flag, void* stream);
/* ABI 8.  The same per image, for N <= TDVC_MAX_PREDICATE_IMAGES images: flags[n] = ((force_mask >> n) & 1) | (image n of cur != image n
 * of cache), then cache[n] = cur[n] for the images whose flag is set (the others' bytes are not touched).  Three enqueued steps for
 * all images: flags = 0, compare, conditional copy. */
int tdvc_frames_changed(const tdvc_fmap* cur, tdvc_fmap* cache, int* flags, unsigned force_mask, void* stream);

/* ---------------------------------------------------------------- conv transforms
 * Replaces every torch.nn.Conv2d / Conv3d(1,3,3) / Conv3d(3,1,1) / compressai
 * conv3x3 / subpel_conv3x3 / MaskedConv2d / GDN 1x1 call on the path:
 * main/model/pnet.py:93-96,132-166,180-184,213-262,278-292,309-317,327-332;
 * main/model/flownet.py:187-227; main/model/encoder_v3.py:17-40,46-69;
 * main/utils/utils.py:52-56; compressai layers (not in tree).                       */

/* Choose the LDS channel chunk for a geometry. Returns ck (8/16/32/64) or <0. */
int tdvc_conv_plan(int cin, int kh, int kw, int stride);
/* Size in bytes of the packed weight blob for (cout, cin, ntaps, ck). */
int64_t tdvc_conv_packed_bytes(int cout, int cin, int ntaps, int ck);
/* Host-side packing: w_oihw fp32 [cout][cin_real][kh][kw] -> fragment-ordered fp16 (host
 * memory, caller uploads).  tap list selects/permutes kernel positions; channels
 * cin_real..cin-1 are zero.  dst is uint16 (IEEE half bits). */
int tdvc_pack_conv_weights(const float* w_oihw, int cout, int cin_real, int cin, int kh, int kw,
                           int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, int ck, uint16_t* dst);
int tdvc_conv2d(const tdvc_conv_desc* d, void* stream);
/* Rows per image of tdvc_conv_desc::chan_sum this conv would write, 0 when its kernel has no fused channel sum (the caller then
 * runs tdvc_channel_sum over y), < 0 on a malformed descriptor.  `chan_sum` itself is ignored here. */
int tdvc_conv_chan_sum_rows(const tdvc_conv_desc* d);
/* ABI 11.  1 when the kernel tdvc_conv2d would dispatch this descriptor to honours tdvc_conv_desc::flow, else 0 (the caller then runs
 * tdvc_add_flow over y); < 0 on a malformed descriptor.  Asked with flow.p == NULL it answers for the kernel alone; with a map given,
 * the map's dtype, channels and geometry count too.  Same validation and selection as tdvc_conv2d, never touches the device. */
int tdvc_conv_flow_supported(const tdvc_conv_desc* d);
/* ABI 5.  Name of the kernel tdvc_conv2d would dispatch this descriptor to -- what tdvc_last_conv_kernel() reports after the
 * launch -- or NULL with tdvc_last_error() set when tdvc_conv2d would reject it.  Same validation and selection, no launch:
 * never touches the device (the pointers are only checked for alignment), the launch-parity state or tdvc_last_conv_kernel();
 * `chan_sum` is ignored.  The string belongs to the calling thread and is valid until its next call. */
const char* tdvc_conv_select(const tdvc_conv_desc* d);
/* The fp32 islands: main/model/pnet.py:33-49,57-73 run both coders with autocast OFF (and enabled_amp=False runs the
 * whole model fp32).  Same descriptor with an fp32 input fmap (C %% 8 == 0) and `w` = the fp32 packing below; fp32
 * accumulation on v_mfma_f32_32x32x2_f32; aux / residual / output fmaps fp32 or fp16.  tdvc_conv2d forwards here
 * when d->x.dtype == TDVC_F32, so fixed descriptor chains (tdvc_ar_decode_serial_batch) run in either precision. */
int tdvc_conv2d_f32(const tdvc_conv_desc* d, void* stream);
/* ABI 17.  tdvc_conv2d_f32's contract on the bf16 matrix pipe (csrc/conv_split.hip): the same descriptors are accepted and rejected, the
 * same epilogue runs, `w` = the three-plane bf16 packing (tdvc_pack_conv_weights_indexed_bf16x3).  Every fp32 operand is split exactly
 * into three bf16 parts (v == h + m + l for every normal fp32 value below bf16's overflow threshold of about 3.39e38; the l part of values below about 2^-110
 * underflows; an operand that is Inf, or finite above that threshold, yields NaN where tdvc_conv2d_f32 yields Inf or a finite sum) and a MAC is the
 * fp32 sum of six exact products on v_mfma_f32_32x32x16_bf16; the three dropped cross terms are below (2 u^3 + u^4) |x| |w| per product,
 * u = 2^-8.  Results are fp32-grade but NOT bit-equal to tdvc_conv2d_f32's.  Strictly opt-in: tdvc_conv2d and tdvc_conv_select never
 * choose it.  tdvc_last_conv_kernel() reports "conv_split". */
int tdvc_conv2d_split(const tdvc_conv_desc* d, void* stream);

/* ---------------------------------------------------------------- fused conv pair
 * y = act2(conv2(act1(conv1(x)))) [+ x] [+ res2] for two 3x3 / stride 1 / pad 1 / 64 -> 64 convs in one launch, the
 * intermediate map staying in LDS: `Res_Block.forward` (main/utils/utils.py:52-56: conv, ReLU, conv, + identity) and the
 * LeakyReLU conv pairs of main/model/pnet.py:132-166.  Results equal two tdvc_conv2d launches up to the fp32 summation
 * order (the intermediate is rounded to fp16 exactly as the stored map would be).  Inference path: nothing is kept for a
 * backward pass. */
typedef struct {
  tdvc_fmap x, y;         /* fp16 maps of 64 channels, same geometry; views (sp > 64) allowed; not in place */
  const void* w;          /* tdvc_pack_conv_pair_weights, on the device */
  const float* bias;      /* [2][64] on the device: conv1 | conv2 */
  int32_t act1; float slope1;   /* TDVC_ACT_NONE / RELU / LRELU after conv1 */
  int32_t act2; float slope2;   /* ... after conv2, before the additions */
  int32_t add_input;      /* 1: y += x */
  tdvc_fmap res2;         /* optional further residual (fp16, output geometry); p == NULL: none */
} tdvc_conv_pair_desc;
int64_t tdvc_conv_pair_packed_bytes(void);
/* host-side packing of the two fp32 OIHW [64][64][3][3] weights into per-wave v_mfma_f32_16x16x32_f16 A fragments
 * (layout in tdvc_amd/csrc/conv_pair.hip); dst: tdvc_conv_pair_packed_bytes() bytes of host memory, caller uploads */
int tdvc_pack_conv_pair_weights(const float* w1_oihw, const float* w2_oihw, uint16_t* dst);
/* 1 when tdvc_conv_pair takes this descriptor (geometry / size limits, LeakyReLU slopes in [0, 1], x and y not overlapping
 * except as disjoint channel windows of one buffer), 0: run the two convs through tdvc_conv2d.  y.p == x.p asks about the
 * geometry only (output not allocated yet); tdvc_conv_pair itself refuses that descriptor. */
int tdvc_conv_pair_supported(const tdvc_conv_pair_desc* d);
int tdvc_conv_pair(const tdvc_conv_pair_desc* d, void* stream);

/* ---------------------------------------------------------------- LoopFilter tail (ABI 14)
 * The tail of Bottleneck3D (main/model/pnet.py:304-317) in one inference-only launch, out of place:
 *   T = W_t . [s_0 | s_1 | s_2] per pixel (the temporal (3,1,1) conv, no bias), s'_j = lrelu(s_j + T, slope), y_j = conv3(s'_j) + a_j
 * for the four 64-channel slices j at channel offsets 0, 64, 128, 192 of a pixel of `s`, `a` and `y` (any pixel stride: dense 256-channel
 * buffers or windows of a ring of slots).  Byte for byte tdvc_conv2d with bcast_T = 4 and `res` (conv_mfma_v5) followed by tdvc_conv2d of
 * conv3 over the four slices with residual `a` (conv_row); the intermediate map never reaches memory.  `s` and `a` are only read. */
typedef struct {
  tdvc_fmap s, a, y;      /* fp16 maps of 256 channels, one geometry; y overlaps neither s nor a */
  int32_t nslices;        /* 4 */
  int32_t slice_stride;   /* 64: channel offset from one slice to the next */
  const void* wt;         /* temporal conv 192 -> 64 (1x1), packed by tdvc_pack_conv_weights with ck = 32 */
  const float* bias_t;    /* must be NULL: the zero padding of conv3's input is applied behind the temporal conv */
  const void* w3;         /* conv3 64 -> 64 (3x3, pad 1), packed with ck = 32 */
  const float* bias3;     /* [64] fp32 */
  float slope;            /* LeakyReLU slope of s' */
} tdvc_lf_tail_desc;
/* 1 when tdvc_lf_tail takes this descriptor (fp16, 4 x 64 channels, aligned, H * W >= 8192, H >= 16, no temporal bias), else 0.  The same
 * validation as the launch; never touches the device. */
int tdvc_lf_tail_supported(const tdvc_lf_tail_desc* d);
int tdvc_lf_tail(const tdvc_lf_tail_desc* d, void* stream);

/* ---------------------------------------------------------------- deformable conv (motion compensation)
 * Fused modulated deformable 3x3 conv, fp16 NHWC, no column buffer:
 * replaces DCN.forward's `_DCNv2.apply` (main/utils/dcnv2/dcn_v2_amp.py:219-234) =
 * dcn_v2_cuda_forward (src/cuda/dcn_v2_cuda.cu:20-95) + modulated_deformable_im2col
 * (src/cuda/dcn_v2_im2col_cuda.cu:125-195).
 * om: fp16 fmap with 27*G channels = raw conv_offset_mask output [o1 | o2 | mask_logits]
 * (sigmoid applied here, dcn_v2_amp.py:220-223). Cin = Cout = 8*G, 8 channels per group.
 * ABI 15.  fp32 maps: with x.dtype == TDVC_F32 the call runs dcn_fused_kernel<float> (csrc/dcn_common.h) -- fp32 samples, sampling
 * positions, mask (1 / (1 + expf(-logit)), a true division) and accumulation (v_mfma_f32_32x32x2_f32); nothing is rounded to
 * fp16 before the epilogue (bias, one fp16 rounding if round_before_act, activation in fp32).  Then om must be fp32 too, y is
 * fp32 or fp16 (one more rounding), x_planar must be NULL, `w` is the fp32 packing (tdvc_pack_conv_weights_indexed_f32,
 * ck = 64, 9 taps), and the fp32 maps are 16-byte aligned with pixel / batch strides that are multiples of 4. */
typedef struct {
  tdvc_fmap x, om, y;
  const void* w;        /* packed with tdvc_pack_conv_weights(ck = 64, 9 taps row-major) */
  const float* bias;
  int32_t groups;
  int32_t act; float slope; int32_t round_before_act;
  void* x_planar;       /* optional scratch of N*H*W*8*groups fp16 values (ABI v2): when non-NULL, x is first re-laid
                           group-planar ([n][g][H][W][8]) and the bilinear gathers read that copy (neighbouring pixels of a
                           group share 128-byte lines); NULL: gather from the NHWC map */
} tdvc_dcn_desc;
int tdvc_dcn_fused(const tdvc_dcn_desc* d, void* stream);

/* fp32 NCHW operator with the exact signature semantics of `_ext.dcn_v2_forward`
 * (src/vision.cpp:3-8, src/dcn_v2.h:9-45): contiguous fp32 tensors, output [B][Cout][Ho][Wo]. */
int tdvc_dcn_v2_forward_f32(const float* input, const float* weight, const float* bias,
                            const float* offset, const float* mask, float* output,
                            int B, int C, int H, int W, int Cout,
                            int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                            int deformable_group, void* stream);
/* `_ext.dcn_v2_backward` (src/dcn_v2.h:48-92, src/cuda/dcn_v2_cuda.cu:97-216). All grads
 * are OVERWRITTEN (zero-initialised inside). `columns` is caller-provided scratch of
 * C*kh*kw*Ho*Wo floats (per-sample column buffer, reused across the batch). */
int tdvc_dcn_v2_backward_f32(const float* input, const float* weight, const float* bias,
                             const float* offset, const float* mask, const float* grad_output,
                             float* grad_input, float* grad_offset, float* grad_mask,
                             float* grad_weight, float* grad_bias, float* columns,
                             int B, int C, int H, int W, int Cout,
                             int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                             int deformable_group, void* stream);

/* ---------------------------------------------------------------- layout / elementwise */
/* NCHW fp32 [N][C][H][W] -> fmap (fp16 or fp32), channels >= C zero-filled up to y.C. */
int tdvc_nchw_to_fmap(const float* src, int C, const tdvc_fmap* y, void* stream);
/* fmap (fp16/fp32) -> NCHW fp32, first C channels. */
int tdvc_fmap_to_nchw(const tdvc_fmap* x, int C, float* dst, void* stream);
/* y = act(a * gate[n][c] (optional) ) + r (optional) ; also y2 (optional, other dtype) gets the same value.
 * gate NULL => no scaling.  Used for SE scaling (main/model/inflate.py:204-208) and plain add/sub. */
int tdvc_scale_act_res(const tdvc_fmap* a, const float* gate, int act, float slope,
                       const tdvc_fmap* r, float r_sign, const tdvc_fmap* y, const tdvc_fmap* y2, void* stream);
/* ABI 11.  The same y, and a second result from it in the same pass: y3 = fp16(float(b) + b_sign * float(y)) on the ROUNDED y -- byte for
 * byte what tdvc_scale_act_res(b, NULL, NONE, 0, y, b_sign, y3, NULL) computes after reading y back (the residual the
 * residual coder codes, `f_cur - pred`, out of LoopFilter's last pass).  fp16 maps of one geometry and channel count (C % 8 == 0), each with its own strides;
 * y3 must not alias a, r or y. */
int tdvc_scale_act_res3(const tdvc_fmap* a, const float* gate, int act, float slope, const tdvc_fmap* r, float r_sign,
                        const tdvc_fmap* y, const tdvc_fmap* b, float b_sign, const tdvc_fmap* y3, void* stream);
/* offset[c] += flow[c & 1] (main/model/pnet.py:163); off fp16 or fp32 (ABI 15) in place, C % 8 == 0; flow an fp32 fmap whose first two
 * channels are read (C >= 2). */
int tdvc_add_flow(const tdvc_fmap* off, const tdvc_fmap* flow, void* stream);
/* x[:, t] = lrelu(x[:, t] + b) for the T channel-slices of width b.C (pnet.py:313-314). */
int tdvc_bcast_add_act(const tdvc_fmap* x, const tdvc_fmap* b, int T, float slope, void* stream);

/* ---------------------------------------------------------------- SE attention
 * main/model/inflate.py:159-208.  Deterministic two-stage mean: partial[N][nblocks][C] fp32
 * scratch, then the gate kernel sums the partials in fixed order, applies the two 1x1 convs
 * (ReLU, Sigmoid) and writes gate[N][C].  w1: [Cmid][C], w2: [C][Cmid]. */
int tdvc_channel_sum(const tdvc_fmap* x, float* partial, int nblocks, void* stream);
int tdvc_se_gate(const float* partial, int nblocks, float inv_count, int N, int C, int Cmid,
                 const float* w1, const float* b1, const float* w2, const float* b2,
                 float* gate, void* stream);

/* ---------------------------------------------------------------- resampling
 * bilinear x2 upsample, align_corners=False (nn.Upsample, main/model/pnet.py:117). fp16 or fp32 (ABI 15) fmaps, C % 8 == 0. */
int tdvc_upsample2x(const tdvc_fmap* x, const tdvc_fmap* y, void* stream);
/* 2x2 average pooling, fp32 fmap -> fp32 fmap (F.avg_pool2d, main/model/flownet.py:103-114). */
int tdvc_avgpool2(const tdvc_fmap* x, const tdvc_fmap* y, void* stream);
/* ABI 11.  Five chained tdvc_avgpool2 levels of two maps in ONE launch (SPyNet's two image pyramids, flownet.py:103-114): xa / xb are
 * fp32 maps of one geometry with H and W multiples of 32; ya / yb are arrays of five fp32 maps each, level k (0-based) of
 * (H >> (k + 1)) x (W >> (k + 1)) pixels, all of the same channel count C <= 4 (<= the inputs').  Every level is computed from the
 * fp32 values of the level above with tdvc_avgpool2's expression: byte for byte the ten chained calls. */
int tdvc_avgpool2_pyramid(const tdvc_fmap* xa, const tdvc_fmap* xb, const tdvc_fmap* ya, const tdvc_fmap* yb, void* stream);
/* One SPyNet level's input assembly — the "bilinear warp" of the path
 * (main/model/flownet.py:119-138 + flow_warp :8-48):
 *   flow_up = 2 * bilinear_x2(flow_lo, align_corners=True)   (zeros if flow_lo == NULL)
 *   warped  = grid_sample(supp, grid + flow_up, bilinear, border, align_corners=True)
 *   cat8    = [ref(3) | warped(3) | flow_up(2)] in cat8's dtype; flow_up is also kept in fp32.
 * ref/supp: fp32 fmaps with C>=3; flow_lo/flow_up: fp32 fmaps whose first two channels are used (C >= 2); cat8: fp16 or fp32 (ABI 15), C=8. */
int tdvc_spynet_level_input(const tdvc_fmap* ref, const tdvc_fmap* supp, const tdvc_fmap* flow_lo,
                            const tdvc_fmap* flow_up, const tdvc_fmap* cat8, void* stream);
/* generic bilinear resize, align_corners=False, fp32 fmaps, optional per-channel scale of the
 * output (flow rescale, flownet.py:153-173). */
int tdvc_resize_bilinear(const tdvc_fmap* x, const tdvc_fmap* y, const float* chscale, void* stream);

/* ---------------------------------------------------------------- in-loop filter matching
 * FeatureFix.forward, main/model/pnet.py:219-255. */
/* scale x scale average pooling (floor), fp16 or fp32 (ABI 15) fmap -> fp32 [N][hp][wp][C] (nn.AvgPool2d, :224-225).
 * Two order-fixed stages through `work` (>= tdvc_avgpool_k_work_floats(..) floats of device memory). */
int64_t tdvc_avgpool_k_work_floats(int N, int hp, int wp, int C, int scale);
int tdvc_avgpool_k(const tdvc_fmap* x, int scale, float* pooled, int hp, int wp, float* work, int64_t work_floats, void* stream);
/* 3x3 / stride-3 / pad-3 patches of both pooled maps, L2-normalise, cosine similarity, first
 * -index argmax over reference patches -> idx[N][L] int32, L = ((hp+3)/3+1)*((wp+3)/3+1)
 * (F.unfold + normalize + bmm + max, :230-236). */
int tdvc_patch_match(const float* pin, const float* pref, int N, int hp, int wp, int C,
                     int32_t* idx, void* stream);
/* gather full-resolution reference blocks by idx (unfold/gather/fold with kernel 3*scale,
 * :247-254), per-pixel cosine similarity with fin over channels (:255), write
 * cat = [fin*cor | out*cor] (128 channels) (:257).  fin, fref (64 channels) and cat are fp16 or fp32 (ABI 15) fmaps. */
int tdvc_match_gather(const tdvc_fmap* fin, const tdvc_fmap* fref, const int32_t* idx, int scale,
                      int hp, int wp, const tdvc_fmap* cat, void* stream);

/* ---------------------------------------------------------------- entropy model (rate terms)
 * compressai EntropyBottleneck.forward, called from main/model/pnet.py:34,58:
 *   z_hat = round(z - median) + median (eval)  |  z + noise (train, noise != NULL)
 *   lik   = |sigmoid(s*upper) - sigmoid(s*lower)|, logits chain over filters (3,3,3,3), >= 1e-9
 * z: fp32 fmap; params: [C][59] floats = softplus(matrix0..4) (33), bias0..4 (13),
 * tanh(factor0..3) (12), median (1); z_hat: fp16 or fp32 fmap.
 * *bits_out = sum(-log2 lik) as a double, by a deterministic two-stage reduction through
 * partial[partial_cap] (needs >= ceil(numel/256) floats). */
int tdvc_eb_forward(const tdvc_fmap* z, const float* params, const tdvc_fmap* noise,
                    const tdvc_fmap* z_hat, double* bits_out, float* partial, int partial_cap, void* stream);
/* compressai GaussianConditional likelihood:
 *   v   = |round(y - mean)| (eval) | |y + noise - mean| (train)
 *   lik = Phi((0.5-v)/s) - Phi((-0.5-v)/s), s = max(scale, 0.11), lik >= 1e-9
 * gp: fp32 fmap with 2C channels [scales | means]. */
int tdvc_gc_forward(const tdvc_fmap* y, const tdvc_fmap* gp, const tdvc_fmap* noise,
                    double* bits_out, float* partial, int partial_cap, void* stream);
/* y_hat = round(y) (half-to-even, torch.round) or y + noise. */
int tdvc_quantize(const tdvc_fmap* y, const tdvc_fmap* noise, const tdvc_fmap* y_hat, void* stream);

/* ---------------------------------------------------------------- a coder's rate branch on a side stream (ABI 19)
 * The rate branch of Cheng2020Anchor.forward -- h_a, tdvc_eb_forward, h_s, the context conv, entropy_parameters, tdvc_gc_forward --
 * feeds only `bits`, which the frame reads once at its end, while the synthesis transform needs y_hat alone: two chains of small
 * launches that do not depend on each other.  tdvc_rate_branch enqueues the whole branch on a SIDE stream, so that what the caller
 * enqueues on `main_stream` behind the call (g_s) runs beside it, and tdvc_rate_join makes the main stream wait for it.
 * tdvc_rate_chain: convs[0 .. nconvs) in launch order (1 <= nconvs <= TDVC_RATE_MAX_CONVS), tdvc_eb_forward's launch behind
 * convs[eb_after - 1] (1 <= eb_after <= nconvs), tdvc_gc_forward's behind the last conv; z / eb_params / z_hat / eb_partial and
 * y / gp / gc_partial are those calls' arguments (eval form: no noise), bits[0] the y bits and bits[1] the z bits.  `split` != 0:
 * the convs go through tdvc_conv2d_split (their `w` the three-plane packing) instead of tdvc_conv2d.  `which`: the branch's slot,
 * 0 <= which < TDVC_RATE_BRANCHES (one per coder of a frame); a slot whose branch has not been joined is refused.
 * The call validates the chain, records an event on `main_stream`, makes the side stream wait for it, makes the nconvs + 2 calls
 * there -- the entry points themselves, so every conv takes the kernel and the tile-walk direction it would take on the main stream
 * in this position -- and records the slot's done event.  Everything the branch reads must have been enqueued on `main_stream`
 * before the call; everything it touches must stay allocated, and untouched by later main-stream work that writes it, until the join
 * has been enqueued.  A failing launch ends the branch: the status is returned, the done event is recorded all the same, and the
 * slot is pending -- a join never waits for an event that was not recorded.
 * The side stream: one per (device, main stream), created on first use (non-blocking, its events without timing) and kept for the life
 * of the process.  No graph capture, no environment variable and no queue setting is involved.  Thread-safe. */
#define TDVC_RATE_MAX_CONVS 16
#define TDVC_RATE_BRANCHES 2
typedef struct tdvc_rate_chain {
  const tdvc_conv_desc* convs;
  int32_t nconvs, eb_after;
  tdvc_fmap z, z_hat;
  const float* eb_params;
  float* eb_partial;
  int32_t eb_partial_cap;
  int32_t gc_partial_cap;
  float* gc_partial;
  tdvc_fmap y, gp;
  double* bits;
  int32_t which, split;
} tdvc_rate_chain;
int tdvc_rate_branch(const tdvc_rate_chain* c, void* main_stream);
/* `main_stream` waits for the done event of slot `which` of ITS side stream (on the current device) and the slot is free again.
 * Nothing pending there -- joined already, never forked, no side stream, no device -- is a no-op: TDVC_OK, nothing enqueued. */
int tdvc_rate_join(void* main_stream, int which);

/* ---------------------------------------------------------------- range coder (host side)
 * compressai `ans` extension (rans64, 16-bit precision, 4-bit bypass) used by
 * Cheng2020Anchor.compress (main/model/pnet.py:46-49,70-73).  Pure host code, like the
 * reference's.  Returns number of bytes written to `out` (<= cap) or <0. */
int64_t tdvc_rans_encode(const int32_t* symbols, const int32_t* indexes, int64_t n,
                         const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                         const int32_t* offsets, uint8_t* out, int64_t cap);
int tdvc_rans_decode(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t n,
                     const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                     const int32_t* offsets, int32_t* symbols_out);

/* Stateful decoder (compressai RansDecoder.set_stream / decode_stream): create copies the stream;
 * decode continues where the previous call stopped. */
void* tdvc_rans_decoder_create(const uint8_t* data, int64_t nbytes);
int tdvc_rans_decoder_decode(void* handle, const int32_t* indexes, int64_t n, const int32_t* cdfs,
                             int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                             int32_t* symbols_out);
void tdvc_rans_decoder_destroy(void* handle);

/* Lane-split y stream (an extension like the wavefront order; the reference's decoder cannot read it): the symbols of one
 * image, given as [npos][M] in wavefront order, are split over L independent sub-streams ("lanes"), symbol c of a position
 * going to lane c % L.  Container: 4 bytes {'L', 1, L, 0}, L little-endian uint16 sub-stream lengths in 32-bit words, then
 * the L sub-streams, lane l's being exactly what tdvc_rans_encode emits for lane l's symbols in that order.  L must divide
 * M; the host entry points take 1 <= L <= 255, the device decoder (tdvc_ar_decode_lanes_step_batch) 64 or 128.
 * encode: -> bytes written or < 0 (a lane of more than 65 535 words included).  decode: the reference decoder, over the
 * decode routine the device kernel uses (csrc/rans_lane.h); validates the header and the length table against nbytes. */
int64_t tdvc_rans_encode_lanes(const int32_t* symbols, const int32_t* indexes, int64_t npos, int M, int L,
                               const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                               const int32_t* offsets, uint8_t* out, int64_t cap);
int tdvc_rans_decode_lanes(const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t npos, int M,
                           const int32_t* cdfs, int32_t cdf_stride, const int32_t* cdf_sizes,
                           const int32_t* offsets, int32_t* symbols_out);

/* compressai `_CXX.pmf_to_quantized_cdf` (used by EntropyModel._pmf_to_cdf inside update(),
 * main/model/pnet.py:47,71): pmf[n] -> quantised cdf[n+1] at `precision` bits, every bin >= 1. Host code. */
int tdvc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out);

/* ---------------------------------------------------------------- autoregressive context model: the context loop
 * `_compress_ar` / `_decompress_ar` of compressai's JointAutoregressiveHierarchicalPriors, called from
 * main/model/pnet.py:48,72.  Position (h, w) depends on rows h-2..h within +-2 columns, so positions
 * with equal w + 3h are independent: the encoder walks W + 3(H-1) anti-diagonal steps, each step a
 * batch of <= H positions whose 12-tap neighbourhoods are gathered into a dense matrix
 * (tdvc_ar_gather_batch), pushed through the context conv and entropy_parameters as 1x1 MFMA convs, then
 * quantised and written back (tdvc_ar_quantize_batch).
 * The loop is a chain of dependent tiny launches (at 1080p 321 steps per coder, at most 40 positions each): a step costs its
 * launches, not its arithmetic.  The images of a batch share the position list, the weights and the CDF tables and nothing in a
 * step couples one image to another, so every entry point handles a step's positions of all B images of the call in the SAME
 * launches.  A single image is B = y_hat->N = 1 and there is no other form: ABI 10 removed the single-image entry points of ABI <= 9
 * (tdvc_ar_gather, tdvc_ar_quantize, tdvc_ar_indexes, tdvc_ar_lanes_init, tdvc_ar_decode_lanes_step, tdvc_ar_decode_serial,
 * tdvc_ar_wavefront, tdvc_ar_wavefront_lanes); the *_batch entry points are those of ABI 9 (ABI 13: the drivers' arguments
 * come in descriptors).
 * Layout: y / y_hat / params are fmaps with N = B (their sn / sp strides are honoured: batch views and channel windows of larger
 * buffers work); `pos` is the shared position list, int32 [npos][2] = (h, w) on the device; row b * npos + k (image-major) of the
 * staging maps x1 / pc / gp belongs to position k of image b, so a step is a (1, B * npos) map to the convs; the raster arrays are
 * [B][H][W][M], the compact ones [B][H * W][M] with row cbase + k inside image b's block (cbase < 0 selects the raster form).  A
 * row's bits do not depend on the row count as long as tdvc_conv_select names the same kernel for the chain's descriptors
 * (conv_mfma_v9 and conv_f32 compute a pixel as one MFMA column with a K split that depends on the layer alone), so a batch's
 * result is byte for byte that of B calls of one image.
 * tdvc_ar_gather_batch.  y_hat: fp16 (or, fp32 islands, fp32) fmap (B, H, W, M); only causal -- already written -- neighbours are
 * read.  params: fmap (B, H, W, 2M) of y_hat's dtype (h_s output).  x1: fmap (1, 1, >= B * npos, 12*M), neighbourhoods in tap-major
 * order, zeros outside the image; pc: fmap (1, 1, >= B * npos, 4M): channels [0, 2M) receive params of the positions. */
int tdvc_ar_gather_batch(const tdvc_fmap* y_hat, const tdvc_fmap* params, const int32_t* pos, int npos,
                         const tdvc_fmap* x1, const tdvc_fmap* pc, void* stream);
/* gp: fp32 fmap (1, 1, >= B * npos, 2M) [scales | means].  Encoder (symbols_in == NULL): q = round(y - mean), y an fp32 fmap of
 * y_hat's batch and geometry; decoder: q = symbols_in[..][c].  Writes y_hat[b][h][w][c] = q + mean, symbols = q (int32) and
 * indexes = #{table entries < max(scale, 0.11)} clipped to ntable-1 (GaussianConditional.build_indexes) at the raster or compact
 * place of the position.  scale_table: ntable floats. */
int tdvc_ar_quantize_batch(const tdvc_fmap* y, const tdvc_fmap* gp, const int32_t* pos, int npos, const float* scale_table, int ntable,
                           const int32_t* symbols_in, const tdvc_fmap* y_hat, int32_t* symbols, int32_t* indexes, int64_t cbase, void* stream);
/* indexes only (decoder: needed before the symbols can be read from the stream). */
int tdvc_ar_indexes_batch(const tdvc_fmap* gp, const int32_t* pos, int npos, int B, const float* scale_table, int ntable,
                          int M, int H, int W, int32_t* indexes, int64_t cbase, void* stream);
/* ABI 13.  The context loop's arguments as descriptors: the groups every driver takes, each written once.
 * tdvc_cdf_tables: the CDF tables in HOST memory, rows as tdvc_rans_decode takes them (ncdfs rows of `stride` ints).
 * tdvc_cdf_tables_dev: the same tables in DEVICE memory, packed for the lane kernels (see tdvc_ar_decode_lanes_step_batch below).
 * tdvc_ar_loop: the chain and its staging buffers, the step list, the scale table and the index / symbol arrays.  B = y_hat.N
 * images, M = y_hat.C channels, W = y_hat.W: the maps are the one source of the sizes.  pos_dev: device int32 [H*W][2] in step
 * order, step s owning step_sizes[s] (HOST array) consecutive entries; step_sizes == NULL: nsteps steps of one position each (the
 * raster order).  x1 / pc / gp and the conv descriptors' x / y maps (convs[0 .. nconvs), nconvs <= 8: context conv over x1 into pc,
 * entropy_parameters into gp; fixed buffers) are (1, 1, >= B * largest step, C) staging buffers whose width is set to the step's
 * B * n rows per step. */
typedef struct tdvc_cdf_tables {
  const int32_t *cdfs, *sizes, *offsets;
  int32_t stride, ncdfs;
} tdvc_cdf_tables;
typedef struct tdvc_cdf_tables_dev {
  const uint16_t* cdf16;
  const int32_t *starts, *sizes, *offsets;
  int32_t n16, ncdfs;
} tdvc_cdf_tables_dev;
typedef struct tdvc_ar_loop {
  tdvc_fmap y_hat, params;
  tdvc_fmap x1, pc, gp;
  const tdvc_conv_desc* convs;
  int32_t nconvs;
  const int32_t* pos_dev;
  const int32_t* step_sizes;
  int32_t nsteps;
  const float* scale_table;
  int32_t ntable;
  int32_t *idx_dev, *sym_dev;
} tdvc_ar_loop;
/* The three drivers below are one loop -- per step gather -> convs -> the driver's back end -- and make every check (arguments,
 * sizes, B * n against the staging width, the steps covering H * W, the strings) before anything touches a device.  data / nbytes:
 * HOST arrays of the B strings and their sizes.
 * tdvc_ar_wavefront_batch, the loop over anti-diagonals in either direction.  Encoder (y given, data / nbytes / tables NULL;
 * replaces `_compress_ar`'s position loop, main/model/pnet.py:48,72): quantise per step; sym_dev / idx_dev are raster
 * [B][H][W][M]; nothing but enqueues, nothing synchronises.  Decoder (data given, y NULL) of streams whose symbols were emitted in
 * wavefront order (an extension: the reference's streams are raster-ordered), per step: indexes -> one device->host copy of the
 * B * n * M indexes, the B host range decoders in turn, one host->device copy -> quantise; one stream synchronisation per step;
 * sym_dev / idx_dev are [B][H*W][M] in step order. */
int tdvc_ar_wavefront_batch(const tdvc_ar_loop* loop, const tdvc_fmap* y, const uint8_t* const* data, const int64_t* nbytes,
                            const tdvc_cdf_tables* tables, void* stream);
/* The decoder's whole context loop for raster-ordered streams (compressai's bitstream): tdvc_ar_wavefront_batch's decoder over a
 * loop whose position list is the raster order, H * W steps of one position (step_sizes == NULL, nsteps = H * W), B rows per step.
 * idx_dev / sym_dev: device int32 [B][H][W][M]; y_hat is filled.  Synchronises the stream once per position (the stream order of
 * compressai's bitstream leaves no other choice). */
int tdvc_ar_decode_serial_batch(const tdvc_ar_loop* loop, const uint8_t* const* data, const int64_t* nbytes, const tdvc_cdf_tables* tables,
                                void* stream);
/* Device decoder of lane-split streams (tdvc_rans_encode_lanes).  B containers of ONE lane count L in one device buffer: a table
 * uint32 [B][2] = {byte offset of container b, 32-bit words of its payload}, padded to 16 bytes, then the containers at 16-byte
 * aligned offsets.  tdvc_ar_lanes_batch_layout: -> the bytes the buffer needs (or < 0) and, when table_out is not NULL, the table
 * (HOST memory, 2 * B words).  The kernels take the buffer (16-byte aligned, stream_bytes long) and the table in DEVICE memory (an
 * ordinary copy puts it there); a table entry that does not lie inside the buffer gives its image no words: flagged, never read.
 * state_dev: [B][L * 4 + 1] words, i.e. B blocks of tdvc_ar_lanes_state_bytes(L) holding the L lane states and one sticky error
 * word (the block's last uint32), which is the only error channel: a damaged stream is flagged, every read stays inside the
 * payload.  tdvc_cdf_tables_dev: the tables of tdvc_rans_decode in DEVICE memory, packed: cdf16 holds every table's entries end to
 * end as uint16 (the last entry of a table, 1 << 16, wraps to 0 and is implied), n16 entries in all (16-byte aligned, padded to a
 * multiple of 8); table t = sizes[t] entries from starts[t]; offsets[t]; ncdfs >= ntable tables.  The kernel keeps the
 * first 27 648 entries in LDS (compressai's 64 Gaussian tables have 27 256).
 * tdvc_ar_lanes_init_batch: lane states from the containers' length tables (and error words = 0).
 * tdvc_ar_decode_lanes_step_batch: one step of npos positions: B workgroups of L threads, thread l of workgroup b decoding the
 * symbols (k, c) of image b, c % L == l, in stream order; does what tdvc_ar_indexes_batch + the range decoder +
 * tdvc_ar_quantize_batch do: indexes / symbols at the compact rows cbase + k, y_hat(b, h, w, c) = q + mean in y_hat's dtype.  Lane
 * states carry over in state_dev.  No atomics, no spinning, nothing persistent. */
int64_t tdvc_ar_lanes_state_bytes(int L);
int64_t tdvc_ar_lanes_batch_layout(const int64_t* nbytes, int B, int L, uint32_t* table_out);
int tdvc_ar_lanes_init_batch(const uint8_t* streams_dev, int64_t stream_bytes, const uint32_t* table_dev, int B, int L, uint32_t* state_dev, void* stream);
int tdvc_ar_decode_lanes_step_batch(const tdvc_fmap* gp, const int32_t* pos, int npos, const float* scale_table, int ntable,
                                    const uint8_t* streams_dev, int64_t stream_bytes, const uint32_t* table_dev, int L,
                                    const tdvc_cdf_tables_dev* tables, uint32_t* state_dev, const tdvc_fmap* y_hat,
                                    int32_t* symbols, int32_t* indexes, int64_t cbase, void* stream);
/* tdvc_ar_wavefront_batch's decoder direction for lane-split streams: the B strings (HOST memory) are validated -- all of one
 * lane count -- and uploaded behind their table, B + 1 copies, into stream_dev (stream_cap >= tdvc_ar_lanes_batch_layout() bytes),
 * then tdvc_ar_lanes_init_batch and per step of the loop tdvc_ar_decode_lanes_step_batch with no synchronisation; after the
 * last step the error words are read back with the call's only stream wait.  TDVC_EINVAL when an image's error word is set: the
 * message and *bad_image (may be NULL; -1 otherwise) name the FIRST such image.  sym_dev / idx_dev are [B][H*W][M] in wavefront
 * order.  Allocates nothing. */
int tdvc_ar_wavefront_lanes_batch(const tdvc_ar_loop* loop, const uint8_t* const* data, const int64_t* nbytes, uint8_t* stream_dev,
                                  int64_t stream_cap, uint32_t* state_dev, const tdvc_cdf_tables_dev* tables, int32_t* bad_image, void* stream);
/* ABI 12.  Device ENCODER of lane-split streams: the container of tdvc_rans_encode_lanes, byte for byte, from the encoder loop's
 * raster arrays symbols / indexes [B][H][W][M] in DEVICE memory, so that the symbols never cross the bus.  pos: int32 [npos][2] =
 * (h, w), the wavefront position list; image b is coded by one workgroup of L threads (L = 64 or 128, L | M), thread l coding lane l
 * -- channels c = j * L + l of every position -- from the LAST position to the first (rANS emits its words in reverse stream
 * order) into a scratch region of its own, words [(b * L + l) * lane_words, + lane_words) of scratch, filled downward from its
 * end; then header, length table and sub-streams are assembled at out + b * out_stride and info[b] = {container bytes, status}:
 * 0 ok; 1 a lane exceeds 65 535 words (tdvc_rans_encode_lanes' error); 2 a lane ran out of its scratch region (or met an index
 * outside the tables or a position outside the image).  On a non-zero status the bytes are 0 and nothing of the container is
 * written; nothing outside scratch, out and info is written at all.
 * tdvc_ar_encode_lanes_scratch_words: the lane_words that suffice for every input: a lane of n = npos * M / L symbols starts
 * below 2^32, gains at most 16 + 4 * 9 = 52 bits per symbol and sheds 32 per word: (31 + 52 n) / 32 + 2 words, capped at 65 536 (a
 * lane that fills or leaves such a region is too long whatever follows: status 1).  tdvc_ar_encode_lanes_out_bytes: the out_stride
 * that goes with it (a multiple of 16).  A smaller lane_words is legal (status 2 where it does not suffice); out_stride must be a
 * multiple of 16 of at least 4 + 2 L + 4 L min(lane_words, 65 535).  Tables as in tdvc_ar_decode_lanes_step_batch, ncdfs <= 64.
 * Every check is made before a device is touched; enqueue-only, no atomics, no spinning, nothing persistent.
 * tdvc_rans_encode_lanes_dev_ref: the host twin -- the same encode routine (csrc/rans_lane.h), traversal, scratch layout and
 * assembly over HOST memory, tables as in tdvc_rans_encode (the first ncdfs rows).
 * tdvc_lanes_enc (ABI 13): the buffers and sizes above, the same for the kernel (DEVICE memory) and its host twin (HOST memory). */
int64_t tdvc_ar_encode_lanes_scratch_words(int64_t npos, int M, int L);
int64_t tdvc_ar_encode_lanes_out_bytes(int64_t npos, int M, int L);
typedef struct tdvc_lanes_enc {
  const int32_t *symbols, *indexes;
  int32_t B, H, W, M;
  const int32_t* pos;
  int32_t npos, L;
  uint32_t* scratch;
  int64_t lane_words, scratch_cap_words;
  uint8_t* out;
  int64_t out_stride, out_cap;
  uint32_t* info;
} tdvc_lanes_enc;
int tdvc_ar_encode_lanes_batch(const tdvc_lanes_enc* enc, const tdvc_cdf_tables_dev* tables, void* stream);
int tdvc_rans_encode_lanes_dev_ref(const tdvc_lanes_enc* enc, const tdvc_cdf_tables* tables);
/* Kernel enqueues of the last context-loop call on this thread (tdvc_ar_decode_serial_batch, tdvc_ar_wavefront_batch,
 * tdvc_ar_wavefront_lanes_batch), conv launches included: the launches the library's entry points closed during the call.  Copies
 * are not counted.  The count does not depend on B. */
int64_t tdvc_ar_last_loop_launches(void);
/* q[n][h][w][c] = round(z - median[c]) as int32 in the fmap's own order (factorised-prior symbols). */
int tdvc_round_symbols(const tdvc_fmap* z, const float* median, int32_t* out, void* stream);

/* ---------------------------------------------------------------- conv backward (training path)
 * torch.autograd's conv backward on the reference path (tools/train.py:142-159 drives loss.backward()):
 * dX runs on tdvc_conv2d with weights re-packed by tdvc_pack_conv_weights_indexed (tdvc_amd/convpack.py builds
 * the index tables); dW is tdvc_conv_wgrad; db is tdvc_channel_sum. */
/* Device-side packing: element (row r, channel c, tap t) of the packed conv = w[row_off[r] + chan_off[c] + tap_off[t]],
 * zero when row_off[r] < 0, chan_off[c] < 0 or tap_mask[t] & (row_mask[r] | chan_mask[c]).  All pointers are device
 * memory; `dst` has tdvc_conv_packed_bytes(cout, cin, ntaps, ck) bytes. */
int tdvc_pack_conv_weights_indexed(const float* w, const int32_t* row_off, const int32_t* chan_off, const int32_t* tap_off,
                                   const uint8_t* row_mask, const uint8_t* chan_mask, const uint8_t* tap_mask,
                                   int cout, int cin, int ntaps, int ck, void* dst, void* stream);
/* fp32 twin of the packing (same item order, 8 floats per item: 2 x tdvc_conv_packed_bytes bytes) for tdvc_conv2d_f32. */
int tdvc_pack_conv_weights_indexed_f32(const float* w, const int32_t* row_off, const int32_t* chan_off, const int32_t* tap_off,
                                       const uint8_t* row_mask, const uint8_t* chan_mask, const uint8_t* tap_mask,
                                       int cout, int cin, int ntaps, int ck, float* dst, void* stream);
/* ABI 17.  Split twin of the packing for tdvc_conv2d_split: same arguments and item order; per item (the 8 values of one lane) three 16-byte
 * bf16 fragments h = bf16(w), m = bf16(w - h), l = bf16((w - h) - m), round-to-nearest-even each, stored as
 * [cout tile][k-step = chunk * steps + step][plane h, m, l][lane 64][8 bf16]: 3 x tdvc_conv_packed_bytes bytes, every plane of a k-step one
 * contiguous 1 KB line. */
int tdvc_pack_conv_weights_indexed_bf16x3(const float* w, const int32_t* row_off, const int32_t* chan_off, const int32_t* tap_off,
                                          const uint8_t* row_mask, const uint8_t* chan_mask, const uint8_t* tap_mask,
                                          int cout, int cin, int ntaps, int ck, void* dst, void* stream);
/* The same for many layers in one launch (after an optimizer step every packed layer follows its parameters).  `jobs`
 * and `block_start` (njobs + 1 prefix sums of tdvc_pack_job_blocks) are DEVICE arrays; a job with bias_src also
 * gathers its bias: bias_dst[i] = bias_src[bias_perm ? bias_perm[i] : i], i < cout. */
typedef struct tdvc_pack_job {
  const float* w;
  const int32_t *row_off, *chan_off, *tap_off;
  const uint8_t *row_mask, *chan_mask, *tap_mask;
  void* dst;
  const float* bias_src;
  float* bias_dst;
  const int32_t* bias_perm;
  int32_t cout, cin, ntaps, ck;
} tdvc_pack_job;
int64_t tdvc_pack_job_blocks(int cout, int cin, int ntaps, int ck);
int tdvc_pack_conv_weights_batch(const tdvc_pack_job* jobs, const int32_t* block_start, int njobs, int total_blocks, void* stream);
/* dW[row_off[co] + chan_off[ci] + tap_off[t]] += scale * sum_{n,oy,ox} g[n,oy,ox,co] * x[n, oy*stride + dy_t - pad, ox*stride + dx_t - pad, ci]
 * for the forward conv y = conv(x, W); g = dL/dy (fp16 fmap, >= cout channels; for a sub-pixel conv the un-shuffled
 * gradient in packed-row order), dW the fp32 parameter gradient.  row_off[cout] / chan_off[x.C] / tap_off[ntaps] are the
 * layer's forward packing tables (device int32; negative row / channel entries are skipped); square_x contracts with
 * x^2 instead of x (GDN norm pool).  Two order-fixed stages
 * through `work` (>= tdvc_conv_wgrad_work_floats(cout, x.C, ntaps, N, Ho, Wo) floats of device memory). */
int64_t tdvc_conv_wgrad_work_floats(int cout, int cin, int ntaps, int N, int Ho, int Wo);
int tdvc_conv_wgrad(const tdvc_fmap* g, const tdvc_fmap* x, int cout, int kh, int kw, int stride, int pad,
                    int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, const int32_t* row_off, const int32_t* chan_off,
                    const int32_t* tap_off, int square_x, float scale, float* dw, float* work, int64_t work_floats, void* stream);
/* The same, and the bias gradient from the dY tiles the kernel already holds (saves a pass over dY):
 * db[bias_index ? bias_index[co] : co] += scale * sum_{n,oy,ox} g[n,oy,ox,co], co < cout; db == NULL skips it. */
int tdvc_conv_wgrad_bias(const tdvc_fmap* g, const tdvc_fmap* x, int cout, int kh, int kw, int stride, int pad,
                         int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, const int32_t* row_off, const int32_t* chan_off,
                         const int32_t* tap_off, int square_x, float scale, float* dw, const int32_t* bias_index, float* db,
                         float* work, int64_t work_floats, void* stream);

/* The two stages apart (training: ~220 layers per step, each reduce a 15 us launch of its own on the side stream): tdvc_conv_wgrad_partials
 * runs the first stage only and fills `job` (a HOST struct) with what the second stage needs; tdvc_wgrad_reduce_batch runs the second stage
 * of many layers in ONE launch.  `jobs` and `block_start` (njobs + 1 prefix sums of tdvc_wgrad_reduce_job::nblocks) are DEVICE arrays.
 * Jobs of one batch must write disjoint dw / db ranges (the sums are `+=` without atomics): a caller with several jobs for one parameter
 * (shared layers, per-image launches) issues them in successive batches, which also keeps the summation order fixed.  `work` must stay
 * alive and unmodified until the batch that reduces it has run. */
typedef struct tdvc_wgrad_reduce_job {
  const float* work;
  const float* bwork;
  const int32_t *row_off, *chan_off, *tap_off, *bias_index;
  float *dw, *db;
  float scale;
  int32_t nworkers, cow, ciw, ntaps, cout, cin, wblocks, nblocks;
} tdvc_wgrad_reduce_job;
int tdvc_conv_wgrad_partials(const tdvc_fmap* g, const tdvc_fmap* x, int cout, int kh, int kw, int stride, int pad,
                             int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, const int32_t* row_off, const int32_t* chan_off,
                             const int32_t* tap_off, int square_x, float scale, float* dw, const int32_t* bias_index, float* db,
                             float* work, int64_t work_floats, tdvc_wgrad_reduce_job* job, void* stream);
int tdvc_wgrad_reduce_batch(const tdvc_wgrad_reduce_job* jobs, const int32_t* block_start, int njobs, int total_blocks, void* stream);
/* The split forms of tdvc_conv_wgrad_bias / tdvc_conv_wgrad_partials (csrc/conv_backward.hip, conv_wgrad_split_kernel): fp32 g and x (both;
 * C % 8 == 0, 16-byte aligned pixels; anything else is an error before any launch), every value split exactly into three bf16 parts and a MAC
 * the fp32 sum of six products on the bf16 matrix pipe (tdvc_conv2d_split's arithmetic; db is the plain fp32 sum of g).  fp32-grade, not
 * bit-equal to the fp32 kernel.  Same workspace (tdvc_conv_wgrad_work_floats), same job, same second stage; a window / stride whose
 * three-plane tiles do not fit the LDS is refused. */
int tdvc_conv_wgrad_bias_split(const tdvc_fmap* g, const tdvc_fmap* x, int cout, int kh, int kw, int stride, int pad,
                               int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, const int32_t* row_off, const int32_t* chan_off,
                               const int32_t* tap_off, int square_x, float scale, float* dw, const int32_t* bias_index, float* db,
                               float* work, int64_t work_floats, void* stream);
int tdvc_conv_wgrad_partials_split(const tdvc_fmap* g, const tdvc_fmap* x, int cout, int kh, int kw, int stride, int pad,
                                   int ntaps, const int8_t* tap_dy, const int8_t* tap_dx, const int32_t* row_off, const int32_t* chan_off,
                                   const int32_t* tap_off, int square_x, float scale, float* dw, const int32_t* bias_index, float* db,
                                   float* work, int64_t work_floats, tdvc_wgrad_reduce_job* job, void* stream);

/* out = g * act'(z), ReLU / LeakyReLU, the sign of z taken from the stored output (y - res); out may alias g. */
int tdvc_act_backward(const tdvc_fmap* g, const tdvc_fmap* y, const tdvc_fmap* res, int act, float slope, const tdvc_fmap* out, void* stream);
/* out[n][Y][X][(i*2+j)*C + c] = y[n][2Y+i][2X+j][c] (adjoint of the PixelShuffle(2) store, packed-row order). */
int tdvc_pixel_unshuffle(const tdvc_fmap* y, const tdvc_fmap* out, void* stream);
/* db[dst_index[c] or c] += scale * sum_{n,h,w} g[n,h,w,c] for c < nvalid (two order-fixed stages through `work`). */
int64_t tdvc_bias_grad_work_floats(int N, int C);
int tdvc_bias_grad(const tdvc_fmap* g, int nvalid, const int32_t* dst_index, float scale, float* db, float* work, int64_t work_floats, void* stream);

/* ---------------------------------------------------------------- backward of the streaming operators (training path)
 * Adjoints of the kernels above; every gradient ACCUMULATES into its destination (tdvc_amd/autograd.py). */
/* dst[..., c] = c < src.C ? src[..., c] : 0 with dtype conversion (fp32 gradients -> the fp16 MFMA backward kernels). */
int tdvc_copy_cast(const tdvc_fmap* src, const tdvc_fmap* dst, void* stream);
/* g *= [0 < y < 1] (the reconstruction clamp, pnet.py:78). */
int tdvc_clamp01_backward(const tdvc_fmap* g, const tdvc_fmap* y, void* stream);
/* y = a * gate[n][c] (SELayer scaling, inflate.py:208): da += g * gate (da may be NULL), dgate[n][c] += sum_pix g * a. */
int64_t tdvc_gate_backward_work_floats(int N, int C);
int tdvc_gate_backward(const tdvc_fmap* g, const tdvc_fmap* a, const float* gate, const tdvc_fmap* da, float* dgate, float* work,
                       int64_t work_floats, void* stream);
/* backward of tdvc_se_gate: dmean[N][C] (written) and the four parameter gradients (+= scale * ...). */
int tdvc_se_gate_backward(const float* partial, int nblocks, float inv_count, int N, int C, int Cmid, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* gate, const float* dgate, float scale, float* dmean,
                          float* dw1, float* db1, float* dw2, float* db2, void* stream);
/* dx[n][pix][c] += v[n][c] * scale (adjoint of the global average pool). */
int tdvc_bcast_channel_add(const tdvc_fmap* dx, const float* v, float scale, void* stream);
/* adjoint of tdvc_add_flow: dflow[.., 0/1] += sum of the even / odd channels of doff (fp16, or fp32 with C % 8 == 0: ABI 16). */
int tdvc_add_flow_backward(const tdvc_fmap* doff, const tdvc_fmap* dflow, void* stream);
/* adjoint of tdvc_bcast_add_act: dx *= lrelu'(x) in place, db += sum over the T channel slices of dx.  fp16 or fp32 (ABI 16) fmaps. */
int tdvc_bcast_add_act_backward(const tdvc_fmap* dx, const tdvc_fmap* x, const tdvc_fmap* db, float slope, void* stream);
/* adjoint of tdvc_upsample2x: dx += U^T dy.  fp16 or fp32 (ABI 16) fmaps, C % 8 == 0. */
int tdvc_upsample2x_backward(const tdvc_fmap* dy, const tdvc_fmap* dx, void* stream);
/* adjoint of tdvc_resize_bilinear (flownet.py:153-173, the flow's way back from the x32-padded size): dx += R^T (chscale * dy),
 * fp32 maps, gathered per input pixel (reproducible).  Only reached when H or W is not a multiple of 32. */
int tdvc_resize_bilinear_backward(const tdvc_fmap* dy, const tdvc_fmap* dx, const float* chscale, void* stream);

/* backward of tdvc_spynet_level_input (flownet.py:82-140): dflow_up += flow channels of dcat8 + the warp gradient
 * (grid_sample bilinear / border / align_corners=True w.r.t. the flow), then dflow_lo += 2 * U^T dflow_up.  The images
 * need no gradient.  dflow_lo may be NULL (coarsest level).  dcat8: fp16 or fp32 (ABI 16), C = 8. */
int tdvc_spynet_level_input_backward(const tdvc_fmap* supp, const tdvc_fmap* flow_up, const tdvc_fmap* dcat8, const tdvc_fmap* dflow_up,
                                     const tdvc_fmap* dflow_lo, void* stream);

/* flat fp32 helpers of the DCN backward glue: out = sigmoid(x); g *= s*(1-s); dst += scale*src. */
int tdvc_sigmoid_f32(const float* x, float* out, int64_t n, void* stream);
int tdvc_sigmoid_backward_f32(float* g, const float* s, int64_t n, void* stream);
int tdvc_axpy_f32(float* dst, const float* src, float scale, int64_t n, void* stream);

/* backward of tdvc_match_gather (pnet.py:240-255): the matching indices carry no gradient; dfin += d(cat)/d(fin),
 * dfref += the gathered blocks' gradients in gather form (fixed summation order, no atomics).  The five fmaps are fp16 or fp32 (ABI 16). */
int tdvc_match_gather_backward(const tdvc_fmap* fin, const tdvc_fmap* fref, const int32_t* idx, int scale, int hp, int wp,
                               const tdvc_fmap* dcat, const tdvc_fmap* dfin, const tdvc_fmap* dfref, void* stream);

/* GDN / inverse GDN backward, elementwise part (y = x * n^(-1/2) | x * n^(+1/2), n = beta + gamma . x^2 recomputed in
 * fp32): dx += g * n^(-+1/2);  dn = g * x * (-+1/2) * n^(-+1/2 - 1) (fp16, feeds conv_dgrad / conv_wgrad of the norm pool). */
int tdvc_gdn_backward(const tdvc_fmap* g, const tdvc_fmap* x, const tdvc_fmap* n32, int inverse, const tdvc_fmap* dn, const tdvc_fmap* dx, void* stream);
/* dx += 2 * x * t (chain rule through x^2). */
int tdvc_mul2_accumulate(const tdvc_fmap* dx, const tdvc_fmap* x, const tdvc_fmap* t, void* stream);

/* backward of the rate terms in training mode (additive uniform noise), bits = -log2(likelihood):
 * tdvc_eb_backward: dz += gscale * dbits/dz, dparams[C][59] += gscale * dbits/d(packed parameters);
 * tdvc_gc_backward: dy += gscale * dbits/dy, dgp[.., 0:M] (scales) and dgp[.., M:2M] (means) likewise. */
int tdvc_eb_backward(const tdvc_fmap* z, const float* params, const tdvc_fmap* noise, float gscale, const tdvc_fmap* dz, float* dparams, void* stream);
int tdvc_gc_backward(const tdvc_fmap* y, const tdvc_fmap* gp, const tdvc_fmap* noise, float gscale, const tdvc_fmap* dy, const tdvc_fmap* dgp, void* stream);
/* The factorised prior's parameter-space work of a training step (compressai EntropyBottleneck: `_logits_cumulative`'s softplus / tanh
 * reparametrisation and `loss()`, the auxiliary quantile loss; the reference's tools/train.py:150-151 runs the latter through autograd).
 * `raw` / `grad`: DEVICE arrays of 14 pointers -- _matrix0..4, _bias0..4, _factor0..3, each [C][len] fp32 -- in the column order of the
 * packed table [C][59] that tdvc_eb_forward / tdvc_eb_backward read.
 * tdvc_eb_pack: packed = softplus(matrices) | biases | tanh(factors) | median (quantiles[c][1]).
 * tdvc_eb_param_chain: grad[k] += scale * dpacked * d packed / d raw (the median column is skipped).
 * tdvc_eb_aux: loss[0] = sum |logits_cumulative(quantiles) - (-target, 0, +target)|, dq[C][3] = its gradient (overwritten); 3 C <= 1024. */
int tdvc_eb_pack(const float* const* raw, const float* quantiles, float* packed, int C, void* stream);
int tdvc_eb_param_chain(const float* dpacked, const float* const* raw, float* const* grad, float scale, int C, void* stream);
int tdvc_eb_aux(const float* params, const float* quantiles, float target, float* dq, float* loss, int C, void* stream);

/* fp16 channel-innermost pieces of the fused DCN's backward (dcn_v2_cuda.cu:97-216 restructured): column channel
 * k = group*72 + tap*8 + j.  tdvc_dcn_columns: col = mask * bilinear samples (operand of dW = dY col^T, a 1x1
 * tdvc_conv_wgrad).  tdvc_dcn_col2im: from dcol = W^T dY (a 1x1 tdvc_conv2d): offset / mask gradients accumulate
 * into dom (fp16, the offset-mask conv's output gradient, mask through its sigmoid), the bilinear scatter into
 * dx32 (fp32 [N][H][W][8G], zero-initialised by the caller).  The scatter is privatised: one 32x32-pixel LDS window
 * per 16x16 tile and group, stored to `work` (tdvc_dcn_col2im_work_floats floats, 16-byte aligned) and summed per
 * pixel in a fixed order; only samples displaced by more than 8 pixels use float atomics (the reference's col2im
 * uses them for every sample).
 * ABI 16.  x, om, col / dcol and dom may all be fp32 maps instead (the whole-model fp32 training mode): the same kernels templated on
 * the element type, fp32 samples, offsets, columns and dom, the mask a true division of expf as in tdvc_dcn_fused on fp32 maps; fp32
 * maps need a 16-byte aligned base and pixel / batch strides that are multiples of 4.  A mix of fp16 and fp32 maps is refused before
 * any launch.  tdvc_dcn_col2im_tile: the side of the scatter's pixel tile (the LDS window reaches one tile further on every side). */
int tdvc_dcn_columns(const tdvc_fmap* x, const tdvc_fmap* om, int groups, const tdvc_fmap* col, void* stream);
int64_t tdvc_dcn_col2im_work_floats(int N, int H, int W, int groups);
int tdvc_dcn_col2im_tile(void);
int tdvc_dcn_col2im(const tdvc_fmap* x, const tdvc_fmap* om, const tdvc_fmap* dcol, int groups, float* dx32, const tdvc_fmap* dom,
                    float* work, int64_t work_floats, void* stream);
/* Run-to-run reproducible form (tdvc_amd.ops.DETERMINISTIC; the reproducible training run of the parity tests): samples
 * displaced out of their tile's window are recorded instead of added with float atomics -- far_keys[i] (unique: target
 * (n, y, x, group) << 27 | source pixel * 36 + tap * 4 + corner), far_vals[i][8]; *far_count (device, zeroed by the caller)
 * counts every such sample, records beyond far_cap are dropped (the caller checks the count).  The caller sorts the keys
 * (any stable device sort; `order` = the permutation) and tdvc_dcn_far_apply adds each target's records in key order. */
int tdvc_dcn_col2im_det(const tdvc_fmap* x, const tdvc_fmap* om, const tdvc_fmap* dcol, int groups, float* dx32, const tdvc_fmap* dom,
                        float* work, int64_t work_floats, int64_t* far_keys, float* far_vals, int32_t* far_count, int32_t far_cap, void* stream);
int tdvc_dcn_far_apply(const int64_t* keys_sorted, const int64_t* order, const float* far_vals, int32_t count, float* dx32, void* stream);

/* ---------------------------------------------------------------- quality metrics (evaluation loop)
 * One level of MS-SSIM as main/model/ms_ssim_torch.py:33-83 computes it on a float32 NCHW pair: valid separable
 * filter `win` (HOST array of win_size taps, odd, <= 15) of X, Y, X^2, Y^2, XY; ssim_out[n] / cs_out[n] = the means of
 * the ssim / cs maps over (C, H - win + 1, W - win + 1), BEFORE the reference's (v + 1) / 2.  x, y, outputs and `work`
 * (tdvc_ssim_level_work_floats floats) are device memory.  tdvc_avgpool2_pad_f32 is the pooling between levels
 * (:178-180): kernel 2, stride 2, padding (H % 2, W % 2) with the zeros counted; out is
 * [planes][(H + 2*(H%2) - 2) / 2 + 1][(W + 2*(W%2) - 2) / 2 + 1]. */
int64_t tdvc_ssim_level_work_floats(int N, int C, int H, int W, int win_size);
int tdvc_ssim_level(const float* x, const float* y, int N, int C, int H, int W, const float* win, int win_size,
                    float c1, float c2, float* ssim_out, float* cs_out, float* work, int64_t work_floats, void* stream);
int tdvc_avgpool2_pad_f32(const float* x, int64_t planes, int H, int W, float* out, void* stream);

/* ---------------------------------------------------------------- MS-SSIM as a training distortion: the backward half
 * tdvc_ssim_level_backward: dx = scale * d(sum_n g_ssim[n] * S[n] + g_cs[n] * CS[n]) / dx, where S[n] / CS[n] are the RAW
 * per-image means tdvc_ssim_level writes (before (v + 1) / 2) and y is held constant (both maps are symmetric in x and y:
 * swap the operands for the gradient with respect to y).  g_ssim / g_cs are DEVICE arrays of N floats and are never read
 * on the host; `win` is a HOST array as in tdvc_ssim_level.  g_pool, when not NULL, is the gradient of the next (coarser)
 * level, [N][C][(H + 2*(H%2) - 2) / 2 + 1][(W + 2*(W%2) - 2) / 2 + 1]: the backward of tdvc_avgpool2_pad_f32,
 * 0.25 * g_pool[(iy + H%2) / 2][(ix + W%2) / 2], is added (unscaled) in the same store, so the backward of the whole
 * pyramid is one launch per level, coarse to fine.  dx ([N][C][H][W]) is overwritten.  A gather with a fixed summation
 * order and no atomics: bit-reproducible.  All fp32.
 * tdvc_msssim_level_grads: the scalar tail (ms_ssim_torch.py:183-188) and its gradient.  cs: DEVICE [levels][N] cs means
 * and ssim_last: DEVICE [N] ssim means of the last level, both AFTER (v + 1) / 2; weights: HOST array of `levels`
 * (<= TDVC_MSSSIM_MAX_LEVELS) floats; grad_out: DEVICE [N] upstream gradient of the MS-SSIM value, NULL = ones.  Writes
 * ms_out[N] = prod_{l < levels-1} cs_l^w_l * ssim^w_last and g_ssim / g_cs ([levels][N] each): the gradients with respect
 * to the RAW means of every level, ready for tdvc_ssim_level_backward (only the last level's g_ssim is non-zero). */
#define TDVC_MSSSIM_MAX_LEVELS 8
int tdvc_ssim_level_backward(const float* x, const float* y, int N, int C, int H, int W, const float* win, int win_size,
                             float c1, float c2, const float* g_ssim, const float* g_cs, float scale, const float* g_pool,
                             float* dx, void* stream);
int tdvc_msssim_level_grads(const float* cs, const float* ssim_last, const float* weights, int levels, int N, const float* grad_out,
                            float* ms_out, float* g_ssim, float* g_cs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDVC_HIP_H */
