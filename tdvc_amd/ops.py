"""Host-side operator layer: torch tensors (device memory + streams only) -> C-ABI calls.

`FM` is a channel-innermost feature-map view ([N][H][W][C], fp16 or fp32) over a torch buffer;
channel slices of a wider buffer are views, so concatenations are never materialised.
Every function enqueues on torch's current HIP stream and returns immediately.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from . import convpack
from ._lib import (ACT_CLAMP01, ACT_LRELU, ACT_NONE, ACT_RELU, GDN_FWD, GDN_INV, GDN_NONE, OUT_NCHW_F32,  # noqa: F401
                   OUT_NHWC, OUT_SHUFFLE2)


# The launch stream.  `torch.cuda.current_stream()` costs ~8 us of Python per call (device-index and availability checks, an os.environ
# lookup, a Stream object): with ~2.4 k launches per training step it was a fifth of the HOST time that bounds the step
# (tools/train_host_bound.py, tools/train_host_profile.py); the raw handle comes from the same C++ call without the wrappers.
_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_dev = torch._C._cuda_getDevice
FORCE_STREAM = None       # a raw stream handle: every launch goes there instead of torch's current stream (Tape.off_path: the side
                          # stream without the ~10 us of a `with torch.cuda.stream(...)` block per weight-gradient launch)
FORCE_KEEP = None         # with FORCE_STREAM: a list that keeps temporaries of such launches alive (they were allocated by the main
                          # stream's pool, which must not reuse them before the streams have joined)


def _stream():
    if FORCE_STREAM is not None:
        return C.c_void_p(FORCE_STREAM)
    return C.c_void_p(_raw_stream(_cur_dev()))


# optional per-launch event trace (bench.py roofline leg): list of dicts, or None
PROFILE = None
# active autograd tape (tdvc_amd/autograd.py) or None: differentiable ops record their backward closure on it
TAPE = None
_IN_BACKWARD = False      # set by Tape.backward(): ops called from backward closures are not recorded


def _profiled(kernel, shape: str, flops: float, run, flops_real: float | None = None, bytes: float = 0.0, **more):
    """`run()`; under PROFILE between two events, as one row of the per-kernel table.  `kernel`: the row's name, or a callable that
    gives it behind the launch; `flops_real`: the algorithmic count where padding makes it differ from `flops`; `more`: further columns"""
    if PROFILE is None:
        return run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = run()
    e1.record()
    PROFILE.append(dict(kernel=kernel() if callable(kernel) else kernel, shape=shape, e0=e0, e1=e1, flops=flops,
                        flops_real=flops if flops_real is None else flops_real, bytes=bytes, **more))
    return r


# ----------------------------------------------------------------------------- launch predicate
_PRED_LOG = None          # inside `with predicate(flag)`: one tdvc_last_launch_predicated() answer per kernel conv / conv_pair / avgpool_k launched


class _predicate_block:
    """enter / exit of the two predicate forms: `_SET` is the library's setter, `_on()` its arguments inside the block, `_OFF` behind it"""

    def __enter__(self):
        global _PRED_LOG
        if _PRED_LOG is not None:
            raise L.TdvcHipError(f"ops.{type(self).__name__} does not nest")
        launch(self._SET, *self._on(), host=True)
        _PRED_LOG = []
        return _PRED_LOG

    def __exit__(self, *exc):
        global _PRED_LOG
        _PRED_LOG = None
        getattr(L.lib(), self._SET)(*self._OFF)
        return False


class predicate(_predicate_block):
    """`with ops.predicate(flag) as log:` -- the launches inside carry the device flag (int32 tensor of one element, written on
    this stream by `frame_changed`) wherever their kernel tests it (tdvc_set_predicate): conv_c8, conv_pair, conv_row and both
    kernels of avgpool_k return at once, outputs untouched, when the flag is 0; any other kernel runs in full.  `log` collects,
    per kernel launched by conv / conv_pair / avgpool_k, whether it carried the flag: a chain may only rely on the skipping
    when every entry is true (a skipped producer in front of a consumer that ran would feed it stale memory)."""
    _SET, _OFF = "tdvc_set_predicate", (None,)

    def __init__(self, flag: torch.Tensor):
        assert flag.dtype == torch.int32 and flag.is_cuda and flag.numel() >= 1
        self.flag = flag

    def _on(self):
        return (self.flag,)


class predicate_images(_predicate_block):
    """`with ops.predicate_images(flags) as log:` -- the per-image form (tdvc_set_predicate_images): `flags` is a contiguous int32 device
    tensor of n <= 4 elements (written on this stream by `frames_changed`); a conv_c8 or conv_pair launch over exactly n images computes
    image i only when flags[i] != 0 and leaves the others' outputs as they were, its workgroups sharing the active images' work.  Any
    other launch runs in full.  `log` as for `predicate`; the two forms do not nest, in themselves or in each other."""
    _SET, _OFF = "tdvc_set_predicate_images", (None, 0)

    def __init__(self, flags: torch.Tensor):
        assert flags.dtype == torch.int32 and flags.is_cuda and flags.dim() == 1 and flags.is_contiguous() and 1 <= flags.numel() <= 4
        self.flags = flags

    def _on(self):
        return (self.flags, self.flags.numel())


def _log_predicated(kernels=1):
    if _PRED_LOG is not None:
        _PRED_LOG.extend([bool(L.lib().tdvc_last_launch_predicated())] * kernels)


def frame_changed(cur: FM, cache: FM, flag: torch.Tensor) -> None:
    """flag[0] = (cur != cache) as exact 16-byte words, and cache = cur when they differ; all on the stream, no host wait"""
    launch("tdvc_frame_changed", cur, cache, flag)


def frames_changed(cur: FM, cache: FM, flags: torch.Tensor, force_mask: int = 0) -> None:
    """per image n of at most four: flags[n] = bit n of force_mask | (cur[n] != cache[n]) as exact 16-byte words, and cache[n] = cur[n]
    where the flag is set; all on the stream, no host wait"""
    assert flags.dtype == torch.int32 and flags.is_cuda and flags.is_contiguous() and flags.numel() >= cur.N
    launch("tdvc_frames_changed", cur, cache, flags, int(force_mask) & 0xF)


def _rec(name, *args):
    """record a differentiable op on the active tape (no-op outside `autograd.record()`)"""
    if TAPE is not None and not _IN_BACKWARD:
        from . import autograd
        getattr(autograd, "record_" + name)(TAPE, *args)


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


class FM:
    """Feature-map view over a torch buffer `t` of shape (N, H, W, Cbuf): N images of C channels
    starting `off` elements into the buffer, batch stride `sn`, pixel stride t.stride(2)."""

    __slots__ = ("t", "off", "N", "C", "H", "W", "sn", "sp", "_d")

    def __init__(self, t: torch.Tensor, off: int = 0, N: int | None = None, C_: int | None = None, sn: int | None = None):
        assert t.dim() == 4 and (t.shape[3] == 1 or t.stride(3) == 1)
        self.t, self.off = t, off
        self._d = None
        self.N = t.shape[0] if N is None else N
        self.C = t.shape[3] if C_ is None else C_
        self.H, self.W = t.shape[1], t.shape[2]
        # strides of size-1 dimensions are arbitrary in torch: derive them from the dense layout instead
        if self.W > 1:
            self.sp = t.stride(2)
        elif self.H > 1:
            self.sp = t.stride(1)
        else:
            self.sp = t.shape[3]
        assert self.H == 1 or t.stride(1) == self.W * self.sp, "rows of a feature map must be dense (row stride = W * pixel stride)"
        self.sn = (t.stride(0) if t.shape[0] > 1 else self.H * self.W * self.sp) if sn is None else sn

    @staticmethod
    def empty(N, H, W, C_, dtype=torch.float16, device="cuda"):
        return FM(torch.empty((N, H, W, C_), dtype=dtype, device=device))

    @staticmethod
    def zeros(N, H, W, C_, dtype=torch.float16, device="cuda"):
        return FM(torch.zeros((N, H, W, C_), dtype=dtype, device=device))

    @property
    def f32(self):
        return self.t.dtype == torch.float32

    def ch(self, c0, C_):
        """channel slice view"""
        assert 0 <= c0 and c0 + C_ <= self.C
        return FM(self.t, self.off + c0, self.N, C_, self.sn)

    def batch(self, n0, N):
        assert 0 <= n0 and n0 + N <= self.N
        return FM(self.t, self.off + n0 * self.sn, N, self.C, self.sn)

    def as_slices(self, b, T, Cs):
        """the T channel-slices (width Cs) of batch item b, viewed as a batch of T images"""
        assert self.C == T * Cs and 0 <= b < self.N
        return FM(self.t, self.off + b * self.sn, T, Cs, Cs)

    def desc(self) -> L.FMapDesc:
        d = self._d                          # an FM is immutable: built once (struct fields are copied on assignment into descriptors)
        if d is None:
            p = self.t.data_ptr() + self.off * self.t.element_size()
            d = self._d = L.FMapDesc(p, self.N, self.H, self.W, self.C, self.sn, self.sp, L.F32 if self.f32 else L.F16)
        return d

    def to_nchw(self, C_=None) -> torch.Tensor:
        C_ = self.C if C_ is None else C_
        out = torch.empty((self.N, C_, self.H, self.W), dtype=torch.float32, device=self.t.device)
        launch("tdvc_fmap_to_nchw", self, C_, out)
        return out


_NULL_FM = L.FMapDesc(None, 0, 0, 0, 0, 0, 0, 0)


# ----------------------------------------------------------------------------- the launch rule
class _Marshal(dict):
    """argument type -> how a wrapper's argument of that type becomes the C argument, resolved once per type: a map is its cached
    descriptor and a tensor its address; anything else (None, descriptor structures, ctypes arrays, raw addresses) passes as it is.
    `_lib.SIGNATURES` declares every argument, so ctypes itself passes a structure by reference, None as NULL, an int as a pointer"""
    __slots__ = ()

    def __missing__(self, t):
        rule = self[t] = FM.desc if issubclass(t, FM) else torch.Tensor.data_ptr if issubclass(t, torch.Tensor) else None
        return rule


_marshal = _Marshal()
_LAUNCHERS = {}           # entry point -> its launcher


def _launcher(name: str, host: bool):
    """the launcher of one entry point, written once from its declared argument types: an argument declared as a pointer goes through
    `_marshal`, a scalar passes untouched, and the launch stream (`_stream()`'s choice, as a raw handle) follows unless the entry point
    is a host one.  One expression per entry point instead of a loop over the arguments per call: the training step is bound by host time"""
    types = L.SIGNATURES[name][1]
    names = [f"a{i}" for i in range(len(types) - (not host))]
    call = [f"({a} if (f := _marshal[{a}.__class__]) is None else f({a}))" if (t is C.c_void_p or issubclass(t, C._Pointer)) else a
            for a, t in zip(names, types)]
    if not host:
        call.append("FORCE_STREAM if FORCE_STREAM is not None else _raw_stream(_cur_dev())")
    fn = _LAUNCHERS[name] = eval(f"lambda {', '.join(names)}: L.lib().{name}({', '.join(call)})", globals())
    return fn


def launch(name: str, *args, what: str | None = None, check: bool = True, host: bool = False) -> int:
    """call the library's entry point `name` with the wrapper's arguments, marshalled as `_launcher` says, and check its return code;
    `what` names the call in the error message (default: `name` without its prefix).  `host=True`: an entry point without a stream
    argument.  `check=False`: -> the return code, for the caller to read"""
    rc = (_LAUNCHERS.get(name) or _launcher(name, host))(*args)
    if rc and check:
        L.check(rc, what or name[5:])
    return rc


def from_nchw(x: torch.Tensor, Cpad: int | None = None, dtype=torch.float16, out: FM | None = None) -> FM:
    """(N,C,H,W) fp32 cuda tensor -> FM (channels zero-padded to Cpad)."""
    assert x.is_cuda and x.dtype == torch.float32
    x = x.contiguous()
    N, Cc, H, W = x.shape
    if out is None:
        out = FM.empty(N, H, W, pad8(Cc) if Cpad is None else Cpad, dtype=dtype, device=x.device)
    launch("tdvc_nchw_to_fmap", x, Cc, out)
    return out


# ----------------------------------------------------------------------------- conv
FORMS_CREATED = 0            # PackedConv objects built so far (train.refresh_packed: has a form appeared since the PackBatch was built?)


class _Keyed(dict):
    """slot -> (key, value): what was built for a slot is kept with the key it was built for and built again under another key"""
    __slots__ = ()

    def of(self, slot, key, build, *args):
        e = self.get(slot)
        if e is None or e[0] != key:
            e = self[slot] = (key, build(*args))
        return e[1]


@dataclass
class PackedConv:
    w: torch.Tensor          # device uint8 blob (fragment-ordered fp16)
    bias: torch.Tensor       # device fp32 [cout_pad]
    cout: int
    cin: int                 # padded input channels the kernel will see
    kh: int
    kw: int
    stride: int
    pad: int
    ck: int
    taps: list               # [(dy, dx)]
    shuffle: bool = False
    cin_real: int = 0        # un-padded input channels (algorithmic FLOP accounting)
    s2d: bool = False        # stride-2 3x3 conv executed as a 2x2 conv over a space-to-depth view
    flops_per_px: float = 0.0  # algorithmic FLOP per OUTPUT pixel of the ORIGINAL conv
    # --- provenance for re-packing after an optimizer step and for the backward pass (training path)
    wsrc: torch.Tensor | None = None       # the fp32 weight (nn.Parameter or tensor) on the device
    bsrc: torch.Tensor | None = None
    layout: convpack.WeightLayout | None = None
    tables: convpack.PackTables | None = None
    orig: dict | None = None               # geometry of the ORIGINAL conv: stride, pad, taps, cin_perm, kh, kw
    dgrad: "PackedConv | None" = None      # lazily built data-gradient conv (ops.conv_dgrad)
    param_w: torch.Tensor | None = None    # the nn.Parameters that own wsrc / bsrc (gradient accumulators live on them)
    param_b: torch.Tensor | None = None
    owner: object | None = None            # module that maps this layer's weight gradient to its own parameters (GDN)
    w32: torch.Tensor | None = None        # fp32 twin of `w` for the fp32 islands (conv_f32.hip), packed on first use
    w32_buf: torch.Tensor | None = None    # the buffer of a twin that a re-pack of `w` made stale: the next packed_f32() fills it again
    wsplit: torch.Tensor | None = None     # three-plane bf16 twin of `w` for ops.f32_split (conv_split.hip), packed on first use
    wsplit_buf: torch.Tensor | None = None  # as w32_buf
    column: "PackedConv | None" = None     # lazily built: the DCN weight as a 1x1 conv over sampled columns (ops.dcn_column_conv)
    plain: "PackedConv | None" = None      # lazily built: the plain stride-2 3x3 packing of a space-to-depth layer (ops._plain_form)
    # --- what is derived from the layer without being a packed form: nothing to re-pack
    bias_index: torch.Tensor | None = field(default=None, init=False, repr=False, compare=False)    # sub-pixel row order (ops._bias_index)
    tmpl: _Keyed = field(default_factory=_Keyed, init=False, repr=False, compare=False)    # weight dtype -> descriptor template
    wgrad: _Keyed = field(default_factory=_Keyed, init=False, repr=False, compare=False)   # weight-gradient tables and workspace size

    def __post_init__(self):
        global FORMS_CREATED
        FORMS_CREATED += 1                 # a layer or a derived form (dgrad, plain, column) is new: PackBatch tables are incomplete

    def forms(self, seen: set | None = None):
        """the packed forms derived from this layer (data gradient, column, plain) and from those, each once; `seen`: ids of forms
        met earlier in a walk over several layers.  The one list of what a re-pack has to follow"""
        seen = set() if seen is None else seen
        for f in (self.dgrad, self.column, self.plain):
            if f is not None and id(f) not in seen:
                seen.add(id(f))
                yield f
                yield from f.forms(seen)

    def packed_f32(self) -> torch.Tensor:
        """the same fragment order as `w`, as floats (tdvc_pack_conv_weights_indexed_f32).  Packed on first use and again on the first
        use after a re-pack of `w` (stale_f32()): into the same buffer, so training with fp32 coders allocates nothing per step"""
        if self.w32 is None:
            self.w32, self.w32_buf = _pack_from_tables_f32(self.wsrc, self.tables, self.w32_buf), None
        return self.w32

    def packed_split(self) -> torch.Tensor:
        """the same item order as `w`, every value split exactly into three bf16 parts (tdvc_pack_conv_weights_indexed_bf16x3: per k-step
        the h, m and l planes).  Built and made stale exactly as `packed_f32()`"""
        if self.wsplit is None:
            self.wsplit, self.wsplit_buf = _pack(self.wsrc, self.tables, self.wsplit_buf, "bf16x3"), None
        return self.wsplit

    def stale_f32(self):
        """`w` was re-packed from updated parameters: the fp32 twins (the float and the split one, if ever built) follow on their next use.
        No launch here: a default-mode training step never pays for twins it does not use"""
        if self.w32 is not None:
            self.w32_buf, self.w32 = self.w32, None
        if self.wsplit is not None:
            self.wsplit_buf, self.wsplit = self.wsplit, None

    def repack(self):
        """re-pack from the (updated) fp32 parameters, the derived forms too: per form one kernel launch, plus the bias gather"""
        for pc in (self, *self.forms()):
            _pack_from_tables(pc.wsrc, pc.tables, pc.w)
            pc.stale_f32()
            if pc.bsrc is not None:
                b = pc.bsrc.detach().float()
                pc.bias[:pc.cout] = b[torch.from_numpy(convpack.shuffle_perm(pc.cout)).to(b.device)] if pc.shuffle else b


def _cout_pad(cout):
    return 32 if cout <= 32 else 64 * ((cout + 63) // 64)


def _s2d_weights(w: torch.Tensor) -> torch.Tensor:
    """(cout, C, 3, 3) stride-2 pad-1 kernel -> (cout, 4C, 2, 2) stride-1 kernel over the 2x2
    space-to-depth view: virtual channel q*C + c = parity (py, px) = (q>>1, q&1); virtual tap (dy, dx)
    covers original kernel row ky = 2*dy + py - 1 (zero weight when outside 0..2).  Reference form of
    `convpack.forward_tables_s2d` (tests)."""
    cout, C_, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    w2 = torch.zeros(cout, 4 * C_, 2, 2)
    for py in range(2):
        for px in range(2):
            q = py * 2 + px
            for dy in range(2):
                for dx in range(2):
                    ky, kx = 2 * dy + py - 1, 2 * dx + px - 1
                    if 0 <= ky <= 2 and 0 <= kx <= 2:
                        w2[:, q * C_:(q + 1) * C_, dy, dx] = w[:, :, ky, kx]
    return w2


_PACK_FORMS = {"f16": "tdvc_pack_conv_weights_indexed", "f32": "tdvc_pack_conv_weights_indexed_f32", "bf16x3": "tdvc_pack_conv_weights_indexed_bf16x3"}


def _pack(wsrc: torch.Tensor, tb: convpack.PackTables, dst: torch.Tensor | None, form: str) -> torch.Tensor:
    """the weight in the tables' fragment order: as halves in a byte blob ("f16"), as floats ("f32") or as three bf16 planes per k-step
    ("bf16x3"); into `dst` when one is given"""
    nbytes = L.lib().tdvc_conv_packed_bytes(tb.cout, tb.cin, len(tb.taps), tb.ck)
    assert nbytes > 0
    w = wsrc.detach()
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    if form != "f16":                             # a passed buffer is reused only when it fits
        n, dt = (nbytes // 2, torch.float32) if form == "f32" else (3 * nbytes // 2, torch.bfloat16)      # per 8 halves: 8 floats / 3 x 8 bf16
        if dst is None or dst.numel() != n or dst.device != w.device:
            dst = torch.empty(n, dtype=dt, device=w.device)
    else:
        if dst is None:
            dst = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        assert dst.numel() == nbytes
    launch(_PACK_FORMS[form], w, tb.row_off, tb.chan_off, tb.tap_off,
           tb.row_mask, tb.chan_mask, tb.tap_mask, tb.cout, tb.cin, len(tb.taps), tb.ck, dst)
    return dst


def _pack_from_tables(wsrc: torch.Tensor, tb: convpack.PackTables, dst: torch.Tensor | None = None) -> torch.Tensor:
    return _pack(wsrc, tb, dst, "f16")


def _pack_from_tables_f32(wsrc: torch.Tensor, tb: convpack.PackTables, dst: torch.Tensor | None = None) -> torch.Tensor:
    return _pack(wsrc, tb, dst, "f32")


class _PackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("row_off", C.c_void_p), ("chan_off", C.c_void_p), ("tap_off", C.c_void_p),
                ("row_mask", C.c_void_p), ("chan_mask", C.c_void_p), ("tap_mask", C.c_void_p), ("dst", C.c_void_p),
                ("bias_src", C.c_void_p), ("bias_dst", C.c_void_p), ("bias_perm", C.c_void_p),
                ("cout", C.c_int32), ("cin", C.c_int32), ("ntaps", C.c_int32), ("ck", C.c_int32)]


class PackBatch:
    """Every PackedConv of a model (its forward, dgrad and column forms) re-packed from the fp32 parameters by ONE
    launch (`tdvc_pack_conv_weights_batch`): after an optimizer step ~400 small packing launches and ~200 bias copies
    become one kernel.  The job table lives on the device and is rebuilt when a tensor it points at has moved."""

    def __init__(self, pcs):
        self.pcs = []
        seen = set()
        self.forms = FORMS_CREATED                 # forms built after this walk (a layer's first dgrad, the plain form of an s2d layer the
        for pc in pcs:                             # first time it sees a small or an fp32 map) are not members: refresh_packed rebuilds
            if pc is not None and id(pc) not in seen:
                seen.add(id(pc))
                self.pcs.append(pc)
                self.pcs.extend(pc.forms(seen))
        self._build()

    def _tensors(self, pc):
        tb = pc.tables
        return [pc.wsrc, tb.row_off, tb.chan_off, tb.tap_off, tb.row_mask, tb.chan_mask, tb.tap_mask, pc.w] + \
               ([pc.bsrc, pc.bias] if pc.bsrc is not None else [])

    def _build(self):
        lib = L.lib()
        jobs = (_PackJob * len(self.pcs))()
        starts = [0]
        self._keep = []
        self._ptrs = []
        dev = self.pcs[0].w.device
        for j, pc in zip(jobs, self.pcs):
            tb = pc.tables
            w = pc.wsrc.detach()
            assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
            j.w, j.row_off, j.chan_off, j.tap_off = w.data_ptr(), tb.row_off.data_ptr(), tb.chan_off.data_ptr(), tb.tap_off.data_ptr()
            j.row_mask, j.chan_mask, j.tap_mask = tb.row_mask.data_ptr(), tb.chan_mask.data_ptr(), tb.tap_mask.data_ptr()
            j.dst = pc.w.data_ptr()
            j.cout, j.cin, j.ntaps, j.ck = tb.cout, tb.cin, len(tb.taps), tb.ck
            if pc.bsrc is not None:
                b = pc.bsrc.detach()
                assert b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() and pc.bias.dtype == torch.float32
                j.bias_src, j.bias_dst = b.data_ptr(), pc.bias.data_ptr()
                if pc.shuffle:
                    perm = torch.from_numpy(convpack.shuffle_perm(pc.cout).astype(np.int32)).to(dev)
                    self._keep.append(perm)
                    j.bias_perm = perm.data_ptr()
            nb = lib.tdvc_pack_job_blocks(tb.cout, tb.cin, len(tb.taps), tb.ck)
            assert nb > 0
            starts.append(starts[-1] + nb)
            self._ptrs.append([t.data_ptr() for t in self._tensors(pc)])
        self.total_blocks = starts[-1]
        self.jobs = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        self.starts = torch.tensor(starts, dtype=torch.int32, device=dev)

    def run(self):
        # a moved tensor (module.to(), a re-assigned parameter) invalidates the device job table.  The full check reads ~10 pointers of ~470
        # layers (4 k `data_ptr()` calls: 2-3 ms of a host-bound step); the parameter and the blob of every layer each time, everything
        # every 64th run
        self._runs = getattr(self, "_runs", 0) + 1
        full = (self._runs & 63) == 1
        for pc, ptrs in zip(self.pcs, self._ptrs):
            if (([t.data_ptr() for t in self._tensors(pc)] != ptrs) if full else (pc.wsrc.data_ptr() != ptrs[0] or pc.w.data_ptr() != ptrs[7])):
                self._build()
                break
        launch("tdvc_pack_conv_weights_batch", self.jobs, self.starts, len(self.pcs), self.total_blocks)
        for pc in self.pcs:
            pc.stale_f32()               # fp32 twins (fp32 islands, fp32-coder training) are re-packed from the parameters on next use


def _pick_ck(cin, cout, kh, kw, stride, pad):
    if (stride == 1 or (stride == 2 and kh == 1 and kw == 1 and pad == 0)) and cin >= 32 and cout >= 64:
        return 32            # the weight-stationary / pipelined kernels stream 32-channel chunks
    ck = L.lib().tdvc_conv_plan(cin, kh, kw, stride)
    L.check(0 if ck > 0 else ck, "conv_plan")
    return ck


def pack_conv(weight: torch.Tensor, bias: torch.Tensor | None, stride=1, pad=0, cin_pad: int | None = None,
              taps=None, shuffle=False, cin_perm=None, device="cuda", ck=None, allow_s2d=True,
              layout: convpack.WeightLayout | None = None, param_w: torch.Tensor | None = None,
              param_b: torch.Tensor | None = None) -> PackedConv:
    """weight (cout, cin, kh, kw) fp32 (moved to `device` if it is not there; an nn.Parameter on the device is
    referenced, not copied, so `PackedConv.repack()` sees optimizer updates).  `taps`: list of (dy,dx) to keep
    (masked convs); `shuffle`: rows permuted for the PixelShuffle(2) store; `cin_perm`: index list applied to
    input channels (free re-ordering of concatenated inputs); `layout`: how the logical weight sits in the
    parameter's storage when it is not the dense (cout, cin, kh, kw) order (Conv3d holders)."""
    wsrc = weight if (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()) else \
        weight.detach().float().contiguous().to(device)
    dev = wsrc.device
    if layout is None:
        cout, cin_real, kh, kw = weight.shape
        layout = convpack.WeightLayout.dense(cout, cin_real, kh, kw)
    cout, kh, kw = layout.cout, layout.kh, layout.kw
    cin_real = layout.cin if cin_perm is None else len(cin_perm)
    bsrc = None if bias is None else (bias if bias.is_cuda else bias.detach().float().to(dev))
    orig = dict(stride=stride, pad=pad, taps=taps, cin_perm=cin_perm, kh=kh, kw=kw)
    s2d = (allow_s2d and stride == 2 and (kh, kw) == (3, 3) and pad == 1 and cin_real % 32 == 0 and cout >= 64
           and taps is None and not shuffle and ck is None and cin_perm is None and cin_pad is None)
    if shuffle:
        assert cout % 4 == 0
    if s2d:
        tb = convpack.forward_tables_s2d(layout, ck=32, device=dev)
        cin, k_stride, k_pad = cin_real, 1, 1
    else:
        cin = pad8(cin_real) if cin_pad is None else cin_pad
        if taps is None:
            taps = [(dy, dx) for dy in range(kh) for dx in range(kw)]
        if ck is None:
            ck = _pick_ck(cin, cout, kh, kw, stride, pad)
        tb = convpack.forward_tables(layout, cin_pad=cin, taps=taps, pad=pad, ck=ck, shuffle=shuffle, cin_perm=cin_perm, device=dev)
        k_stride, k_pad = stride, pad
    orig["taps"] = [(dy, dx) for dy in range(kh) for dx in range(kw)] if orig["taps"] is None else list(orig["taps"])
    bp = torch.zeros(_cout_pad(cout), dtype=torch.float32, device=dev)
    pc = PackedConv(_pack_from_tables(wsrc, tb), bp, cout, cin, tb.kh, tb.kw, k_stride, k_pad, tb.ck, tb.taps, shuffle, cin_real,
                    s2d=s2d, flops_per_px=2.0 * cout * cin_real * 9 if s2d else 0.0,
                    wsrc=wsrc, bsrc=bsrc, layout=layout, tables=tb, orig=orig,
                    param_w=param_w if param_w is not None else (weight if isinstance(weight, torch.nn.Parameter) else None),
                    param_b=param_b if param_b is not None else (bias if isinstance(bias, torch.nn.Parameter) else None))
    if bsrc is not None:
        b = bsrc.detach().float()
        bp[:cout] = b[torch.from_numpy(convpack.shuffle_perm(cout)).to(dev)] if shuffle else b
    return pc


SMALL_MAP_PIXELS = 8192      # conv_mfma_v9's range: LARGE_MAP_PIXELS of csrc/conv_common.h


def _plain_form(pc: PackedConv) -> PackedConv:
    """the un-transformed stride-2 3x3 packing of a layer whose main form is the space-to-depth view (built on first use)"""
    if pc.plain is None:
        pc.plain = pack_conv(pc.wsrc, pc.bsrc, stride=2, pad=1, allow_s2d=False, layout=pc.layout, param_w=pc.param_w, param_b=pc.param_b)
    return pc.plain


def _conv_template(pc: PackedConv, wt: torch.Tensor) -> L.ConvDesc:
    """the layer's part of a `tdvc_conv_desc` (weights `wt`, bias, window, taps)"""
    t_ = L.ConvDesc()
    t_.w = wt.data_ptr()
    t_.bias = pc.bias.data_ptr()
    t_.cout, t_.ntaps = pc.cout, len(pc.taps)
    for i, (dy, dx) in enumerate(pc.taps):
        t_.tap_dy[i], t_.tap_dx[i] = dy, dx
    t_.kh, t_.kw, t_.stride, t_.pad, t_.ck = pc.kh, pc.kw, pc.stride, pc.pad, pc.ck
    t_.s2d = int(pc.s2d)
    return t_


F32_SPLIT = False         # inside `with f32_split(True)`: conv() runs fp32 maps on conv_split (six bf16 MFMA products) instead of conv_f32


class f32_split:
    """`with ops.f32_split(True):` -- every conv() of an fp32 map inside the block that no tape records launches `tdvc_conv2d_split`
    (csrc/conv_split.hip: each fp32 operand split exactly into three bf16 parts, a MAC the fp32 sum of six exact products on the bf16
    matrix pipe) with the layer's `packed_split()` weights instead of conv_f32.  fp32-grade, not bit-equal to conv_f32: an encoder and its
    decoder must run under the same setting.  fp16 maps, recorded (training) convs, `conv_desc()` and the native descriptor chains built
    from it are not affected.  Nests; `f32_split(False)` switches it off inside an enabled block."""

    def __init__(self, enable: bool):
        self.enable = bool(enable)

    def __enter__(self):
        global F32_SPLIT
        self.prev, F32_SPLIT = F32_SPLIT, self.enable
        return self

    def __exit__(self, *exc):
        global F32_SPLIT
        F32_SPLIT = self.prev
        return False


F32_SPLIT_TRAIN = False   # inside `with f32_split_train(True)`: the TRAINING convs of fp32 maps (recorded, data- and weight-gradient) on the bf16 pipe


class f32_split_train:
    """`with ops.f32_split_train(True):` -- the training form of `f32_split`, a switch of its own (`f32_split` keeps leaving recorded convs
    and the backward sweep on conv_f32).  Inside the block a conv() of an fp32 map that a tape records, a conv() issued by the backward
    sweep and every `conv_dgrad` launch `tdvc_conv2d_split` with the form's `packed_split()` weights, and a `conv_wgrad` of fp32 maps
    launches the split entry points (conv_wgrad_split_kernel, csrc/conv_backward.hip): the same six-product arithmetic for the forward,
    the data gradient and the weight gradient.  fp16 maps and un-recorded convs outside a backward sweep are not affected; no geometry
    falls back to the fp32 kernels.  Nests like `f32_split`."""

    def __init__(self, enable: bool):
        self.enable = bool(enable)

    def __enter__(self):
        global F32_SPLIT_TRAIN
        self.prev, F32_SPLIT_TRAIN = F32_SPLIT_TRAIN, self.enable
        return self

    def __exit__(self, *exc):
        global F32_SPLIT_TRAIN
        F32_SPLIT_TRAIN = self.prev
        return False


def conv_desc(x: FM, pc: PackedConv, out: FM | None = None, act=ACT_NONE, slope=0.0, res: FM | None = None,
              res2: FM | None = None, gdn=GDN_NONE, aux: FM | None = None, square=False, out_dtype=None,
              round16=False, nchw_out: torch.Tensor | None = None, bcast_T=0, bcast_slope=0.0, _wsplit: bool = False):
    """the `tdvc_conv_desc` a conv() call would launch, without launching it (native loops re-launch fixed descriptors:
    `tdvc_ar_decode_serial_batch`).  -> (descriptor, result FM / tensor, Ho, Wo, layer form used, layer as recorded)

    An fp32 input FM selects the fp32 form of the layer (fp32 weights, v_mfma_f32_32x32x2_f32: the fp32 islands of
    pnet.py:33,57); `out_dtype=None` allocates the output in the input's dtype."""
    assert x.C == pc.cin, f"conv: input has {x.C} channels, layer packed for {pc.cin}"
    rec_pc = pc                                   # the tape records the layer itself (its dgrad / wgrad forms hang off it)
    if out_dtype is None:
        out_dtype = torch.float32 if x.f32 else torch.float16
    if pc.s2d and (x.f32 or x.N * (x.H // 2) * (x.W // 2) <= SMALL_MAP_PIXELS):
        pc = _plain_form(pc)                      # small maps: the plain stride-2 form runs on the split-K kernel (fp32: always plain)
    if pc.s2d:
        if x.H % 2 or x.W % 2:
            raise L.TdvcHipError("conv: the space-to-depth stride-2 path needs even H, W")
        Ho, Wo = x.H // 2, x.W // 2
    else:
        Ho = (x.H + 2 * pc.pad - pc.kh) // pc.stride + 1
        Wo = (x.W + 2 * pc.pad - pc.kw) // pc.stride + 1
    # the layer's part of the descriptor (weights, bias, window, taps) is built once per layer and weight form and copied per call
    # (re-packing writes the same buffers in place; a re-allocated blob is caught by the pointer check)
    # `_wsplit` (conv() under f32_split_train): the split twin at once, so that a training step packs one twin per form, not two
    wt = pc.packed_split() if _wsplit else pc.packed_f32() if x.f32 else pc.w
    d = L.ConvDesc.from_buffer_copy(pc.tmpl.of(wt.dtype, wt.data_ptr(), _conv_template, pc, wt))
    d.x = x.desc()
    d.square_input, d.gdn = int(square), gdn
    d.aux = aux.desc() if aux is not None else _NULL_FM
    d.act, d.slope, d.round_before_act = act, slope, int(round16)
    d.res = res.desc() if res is not None else _NULL_FM
    d.res2 = res2.desc() if res2 is not None else _NULL_FM
    d.bcast_T, d.bcast_slope = int(bcast_T), float(bcast_slope)
    if nchw_out is not None:
        assert nchw_out.shape == (x.N, pc.cout, Ho, Wo) and nchw_out.dtype == torch.float32 and nchw_out.is_contiguous()
        d.out_mode = OUT_NCHW_F32
        d.y = L.FMapDesc(nchw_out.data_ptr(), x.N, Ho, Wo, pc.cout, pc.cout * Ho * Wo, 1, L.F32)
        ret = nchw_out
    else:
        if pc.shuffle:
            d.out_mode = OUT_SHUFFLE2
            if out is None:
                out = FM.empty(x.N, 2 * Ho, 2 * Wo, pad8(pc.cout // 4), dtype=out_dtype, device=x.t.device)
        else:
            d.out_mode = OUT_NHWC
            if out is None:
                out = FM.empty(x.N, Ho, Wo, pc.cout if (out_dtype == torch.float32 and not x.f32) else pad8(pc.cout),
                               dtype=out_dtype, device=x.t.device)
        d.y = out.desc()
        ret = out
    return d, ret, Ho, Wo, pc, rec_pc


def conv(x: FM, pc: PackedConv, out: FM | None = None, act=ACT_NONE, slope=0.0, res: FM | None = None,
         res2: FM | None = None, gdn=GDN_NONE, aux: FM | None = None, square=False, out_dtype=None,
         round16=False, nchw_out: torch.Tensor | None = None, bcast_T=0, bcast_slope=0.0, chan_sum: list | None = None,
         flow: FM | None = None, _dgrad: bool = False) -> FM | torch.Tensor:
    """`flow` (inference only): an fp32 flow map added to the stored output, x to even and y to odd channels -- in the conv's epilogue
    (tdvc_conv_desc::flow) when the kernel it dispatches to does that (tdvc_conv_flow_supported), else by `add_flow` behind it; the
    same bytes either way.
    `bcast_T` (inference only): the conv result is not stored but broadcast-added, with LeakyReLU(bcast_slope), over the
    bcast_T channel slices that start at `out` (tdvc_conv_desc::bcast_T); with `res` given the slices are read at `res` and written
    at `out` (out of place), else in place.
    `chan_sum` (inference only): a list; when the kernel this conv dispatches to can sum the values it stores per channel
    (tdvc_conv_desc::chan_sum), (partial [N][rows][cout] fp32, rows) is appended -- the input of `se_gate(..., partial=)`;
    left empty otherwise (the caller then sums with tdvc_channel_sum)."""
    # ops.f32_split: inference convs of fp32 maps on the bf16 matrix pipe; ops.f32_split_train: the recorded ones and the backward sweep's
    tsplit = split = False
    if x.f32:                                     # (one test per conv of an fp16 map, as before the training switch: the step is host-bound)
        tsplit = F32_SPLIT_TRAIN and (TAPE is not None or _IN_BACKWARD or _dgrad)
        split = tsplit or (F32_SPLIT and TAPE is None)
    entry = "tdvc_conv2d_split" if split else "tdvc_conv2d"
    d, ret, Ho, Wo, pc, rec_pc = conv_desc(x, pc, out, act, slope, res, res2, gdn, aux, square, out_dtype, round16, nchw_out, bcast_T, bcast_slope, tsplit)
    if split and not tsplit:                      # f32_split: conv_desc() built conv_f32's descriptor, and only this launch swaps the
        d.w = pc.packed_split().data_ptr()        # weights (the layer's form `pc`, as conv_desc chose it)
    if chan_sum is not None and TAPE is None and FUSE_CHAN_SUM:
        rows = L.lib().tdvc_conv_chan_sum_rows(d)
        if rows > 0:
            part = torch.empty((x.N, rows, pc.cout), dtype=torch.float32, device=x.t.device)
            d.chan_sum = part.data_ptr()
            chan_sum.append((part, rows))
    if bcast_T and TAPE is not None and not _IN_BACKWARD:
        raise L.TdvcHipError("conv: bcast_T is an inference-only fusion (under the tape use conv + bcast_add_act)")
    if flow is not None:
        if (TAPE is not None and not _IN_BACKWARD) or chan_sum is not None or nchw_out is not None:
            raise L.TdvcHipError("conv: flow is an inference-only fusion of an fmap output, not combined with chan_sum (use conv + add_flow)")
        d.flow = flow.desc()
        if L.lib().tdvc_conv_flow_supported(d) != 1:       # another kernel: the conv as it is, then one pass over its output
            d.flow = _NULL_FM
            launch(entry, d)
            _log_predicated()
            add_flow(ret, flow)
            return ret
    if PROFILE is None:
        launch(entry, d)
        _log_predicated()
    else:                                         # the kernel's name is known behind the launch; a profiled call does not log its predicate
        _profiled(lambda: L.lib().tdvc_last_conv_kernel().decode(),
                  f"{pc.kh}x{pc.kw} s{pc.stride} {x.C}->{pc.cout} @{x.H}x{x.W}" + (" f32out" if out_dtype == torch.float32 else "") + (" nchw" if nchw_out is not None else ""),
                  2.0 * x.N * Ho * Wo * pc.cout * x.C * len(pc.taps), lambda: launch(entry, d),
                  flops_real=(x.N * Ho * Wo * pc.flops_per_px) if pc.s2d else 2.0 * x.N * Ho * Wo * pc.cout * pc.cin_real * len(pc.taps),
                  bytes=2.0 * x.N * (x.H * x.W * x.C + Ho * Wo * pc.cout * (4 if pc.shuffle else 1) / (4 if pc.shuffle else 1)))
    _rec("conv", x, rec_pc, None if nchw_out is not None else ret, act, slope, res, res2, gdn, aux, square, nchw_out)
    return ret


class rgb_head_kernel:
    """`with ops.rgb_head_kernel(False):` -- conv_n16 runs the RGB head (3x3, 64 -> <= 4 planar fp32 channels) on its own kernel instead
    of its streamed form conv_head3 (the library's debug switch tdvc_debug_enable_conv_head3; process-wide, on by default and on again
    behind the block).  The same bytes either way.  For the A/B switch, the tests, training and profiled / traced calls."""

    def __init__(self, enable: bool):
        self.enable = bool(enable)

    def __enter__(self):
        if not self.enable:
            L.lib().tdvc_debug_enable_conv_head3(0)
        return self

    def __exit__(self, *exc):
        if not self.enable:
            L.lib().tdvc_debug_enable_conv_head3(1)
        return False


# ----------------------------------------------------------------------------- fused conv pair (inference)
class PackedConvPair:
    """two 3x3 64->64 convs packed for `tdvc_conv_pair` (per-wave v_mfma_f32_16x16x32_f16 A fragments + both biases)"""

    def __init__(self, w: torch.Tensor, bias: torch.Tensor):
        self.w, self.bias = w, bias


def pack_conv_pair(w1: torch.Tensor, b1: torch.Tensor | None, w2: torch.Tensor, b2: torch.Tensor | None) -> PackedConvPair:
    """weights (64, 64, 3, 3) on the device -> [conv][wave][tap*2 + chunk][lane][8] fp16 (the layout of
    tdvc_pack_conv_pair_weights: cout = 16 wave + (lane & 15), cin = 32 chunk + 8 (lane >> 4) + j)"""
    for w in (w1, w2):
        if tuple(w.shape) != (64, 64, 3, 3):
            raise L.TdvcHipError(f"pack_conv_pair: weights must be (64, 64, 3, 3), got {tuple(w.shape)}")
    frag = lambda w: w.detach().float().reshape(4, 16, 2, 4, 8, 9).permute(0, 5, 2, 3, 1, 4)
    w = torch.stack([frag(w1), frag(w2)]).contiguous().to(torch.float16)
    zb = lambda b_: torch.zeros(64, device=w1.device) if b_ is None else b_.detach().float()
    return PackedConvPair(w, torch.cat([zb(b1), zb(b2)]).contiguous())


def _pair_desc(x: FM, pp: PackedConvPair, out: FM, act1, slope1, act2, slope2, add_input, res2):
    d = L.ConvPairDesc()
    d.x, d.y = x.desc(), out.desc()
    d.w, d.bias = pp.w.data_ptr(), pp.bias.data_ptr()
    d.act1, d.slope1, d.act2, d.slope2 = act1, slope1, act2, slope2
    d.add_input = 1 if add_input else 0
    d.res2 = res2.desc() if res2 is not None else L.FMapDesc()
    return d


def conv_pair_supported(x: FM, out: FM | None = None, res2: FM | None = None) -> bool:
    """inference only (nothing is kept for a backward pass); geometry limits are the library's (tdvc_conv_pair_supported)"""
    if TAPE is not None or x.f32 or x.C != 64:
        return False
    d = L.ConvPairDesc()
    d.x = x.desc()
    d.y = out.desc() if out is not None else x.desc()
    d.res2 = res2.desc() if res2 is not None else L.FMapDesc()
    d.w = d.bias = 1            # presence only; never dereferenced by the query
    return bool(L.lib().tdvc_conv_pair_supported(d))


def conv_pair(x: FM, pp: PackedConvPair, out: FM | None = None, act1=ACT_RELU, slope1=0.0, act2=ACT_NONE, slope2=0.0,
              add_input=True, res2: FM | None = None) -> FM:
    """y = act2(conv2(act1(conv1(x)))) [+ x] [+ res2] in one launch (`tdvc_conv_pair`)"""
    if TAPE is not None:
        raise L.TdvcHipError("conv_pair: inference only (the intermediate map is not kept for the backward pass)")
    if out is None:
        out = FM.empty(x.N, x.H, x.W, 64, device=x.t.device)
    d = _pair_desc(x, pp, out, act1, slope1, act2, slope2, add_input, res2)
    if PROFILE is None:
        launch("tdvc_conv_pair", d)
        _log_predicated()
    else:                                         # as in conv: a profiled call does not log its predicate
        _profiled("conv_pair", f"2x(3x3 s1 64->64) @{x.H}x{x.W}", 2 * 2.0 * x.N * x.H * x.W * 64 * 64 * 9, lambda: launch("tdvc_conv_pair", d),
                  bytes=2.0 * x.N * x.H * x.W * 128)
    return out


# ----------------------------------------------------------------------------- LoopFilter tail (inference)
def _lf_tail_desc(S: FM, A: FM, out: FM, pct: PackedConv | None, pc3: PackedConv | None, slope: float):
    d = L.LfTailDesc()
    d.s, d.a, d.y = S.desc(), A.desc(), out.desc()
    d.nslices, d.slice_stride = 4, 64
    if pct is None:                               # the query: presence only, never dereferenced
        d.wt, d.bias_t, d.w3, d.bias3 = 16, None, 16, 16
    else:
        d.wt, d.bias_t = pct.w.data_ptr(), (None if pct.bsrc is None else pct.bias.data_ptr())
        d.w3, d.bias3 = pc3.w.data_ptr(), pc3.bias.data_ptr()
    d.slope = float(slope)
    return d


def lf_tail_supported(S: FM, A: FM, out: FM) -> bool:
    """inference only; S, A, out: fp16 views of 4 x 64 channels per pixel (dense buffers or ring windows), limits are the library's
    (tdvc_lf_tail_supported)"""
    if TAPE is not None or S.f32 or A.f32 or out.f32:
        return False
    return bool(L.lib().tdvc_lf_tail_supported(_lf_tail_desc(S, A, out, None, None, 0.0)))


def lf_tail(S: FM, A: FM, pct: PackedConv, pc3: PackedConv, out: FM, slope: float = 0.1) -> FM:
    """out_j = conv3(lrelu(S_j + temporal(S_0 | S_1 | S_2), slope)) + A_j over the four 64-channel slices of a pixel, in one launch
    (`tdvc_lf_tail`): byte for byte conv(bcast_T=4, res=S) followed by the conv of the four slices with residual A"""
    if TAPE is not None:
        raise L.TdvcHipError("lf_tail: inference only (the intermediate map is not kept for the backward pass)")
    if (pct.cin, pct.cout, pct.kh, pct.kw, pct.ck) != (192, 64, 1, 1, 32) or (pc3.cin, pc3.cout, pc3.kh, pc3.kw, pc3.ck, pc3.stride, pc3.pad) != (64, 64, 3, 3, 32, 1, 1):
        raise L.TdvcHipError("lf_tail: needs the 1x1 192 -> 64 temporal conv and the 3x3 64 -> 64 conv, both packed with ck = 32")
    launch("tdvc_lf_tail", _lf_tail_desc(S, A, out, pct, pc3, slope))
    _log_predicated()
    return out


# ----------------------------------------------------------------------------- conv backward (training path)
def act_backward(g: FM, y: FM, act, slope=0.0, res: FM | None = None, out: FM | None = None) -> FM:
    """g * act'(z); the sign of the pre-activation comes from the stored output y (minus its residual)"""
    out = g if out is None else out
    launch("tdvc_act_backward", g, y, res, act, slope, out)
    return out


def pixel_unshuffle(y: FM, out: FM | None = None) -> FM:
    """(N, 2H, 2W, C) -> (N, H, W, 4C), channel (i*2+j)*C + c: the gradient of a sub-pixel conv in packed-row order"""
    if out is None:
        out = FM.empty(y.N, y.H // 2, y.W // 2, 4 * y.C, dtype=y.t.dtype, device=y.t.device)
    launch("tdvc_pixel_unshuffle", y, out)
    return out


def _dgrad_conv(pc: PackedConv, g_channels: int, x_channels: int) -> PackedConv:
    """the conv that maps dY to dX for the layer `pc` (built once, re-packed with it)"""
    if pc.dgrad is None:
        o = pc.orig
        tb0 = dict(g_channels=g_channels, x_channels=x_channels, taps=o["taps"], pad=o["pad"], stride=o["stride"], shuffle=pc.shuffle,
                   cin_perm=o["cin_perm"], device=pc.w.device)
        rows = x_channels * (4 if o["stride"] == 2 else 1)
        kk = 3 if (o["stride"] == 2 and o["kh"] == 3) else o["kh"]
        ck = _pick_ck(g_channels, rows, kk, kk, 1, 1)
        tb = convpack.dgrad_tables(pc.layout, ck=ck, **tb0)
        bias = torch.zeros(_cout_pad(tb.cout), dtype=torch.float32, device=pc.w.device)
        pc.dgrad = PackedConv(_pack_from_tables(pc.wsrc, tb), bias, tb.cout, tb.cin, tb.kh, tb.kw, 1, tb.pad, tb.ck, tb.taps, tb.shuffle,
                              tb.cin, wsrc=pc.wsrc, tables=tb)
    assert pc.dgrad.cin == g_channels
    return pc.dgrad


def conv_dgrad(pc: PackedConv, g: FM, dx: FM, accumulate=True, extra: FM | None = None) -> FM:
    """dX (+)= dL/dx of y = conv(x, W) given g = dL/dy (pre-activation).  Runs on the forward conv kernels with
    the weights packed transposed / mirrored (`convpack.dgrad_tables`); for a sub-pixel layer `g` is the
    un-shuffled gradient (`pixel_unshuffle`), for a stride-2 layer the result is stored through PixelShuffle."""
    dpc = _dgrad_conv(pc, g.C, dx.C)
    if accumulate:
        return conv(g, dpc, out=dx, res=dx, res2=extra, _dgrad=True)
    return conv(g, dpc, out=dx, res=extra, _dgrad=True)          # `extra`: one more gradient of the same geometry added in the epilogue (Tape.add_identity)


class WgradBatch:
    """Deferred second stages of conv weight gradients (training: ~220 layers per step, each order-fixed reduce a 15 us launch of its own,
    3.4 ms of the side stream).  `conv_wgrad(..., defer=batch)` runs the first stage only; `flush()` reduces everything collected so far
    in ONE launch of `tdvc_wgrad_reduce_batch` per round, on the current stream (the one the first stages ran on).  Jobs that add to the
    same parameter (shared layers, per-image launches of one layer) go to successive rounds in their order of arrival, so the sums and
    their order are those of the immediate form: bit-identical gradients."""

    def __init__(self):
        self.items = []

    def add(self, job, keep):
        self.items.append((job, keep))

    def flush(self):
        if not self.items:
            return
        rounds, nxt = [], {}
        for job, _ in self.items:
            r = nxt.get(job.dw, 0)
            nxt[job.dw] = r + 1
            if len(rounds) <= r:
                rounds.append([])
            rounds[r].append(job)
        for jobs in rounds:
            n = len(jobs)
            arr = (L.WgradReduceJob * n)(*jobs)
            starts = (C.c_int32 * (n + 1))()
            for i, j in enumerate(jobs):
                starts[i + 1] = starts[i] + j.nblocks
            nb_j, nb_s = C.sizeof(arr), C.sizeof(starts)
            host = torch.empty((nb_j + nb_s,), dtype=torch.uint8, pin_memory=True)
            C.memmove(host.data_ptr(), arr, nb_j)
            C.memmove(host.data_ptr() + nb_j, starts, nb_s)
            dev = host.to(jobs_device(jobs), non_blocking=True)
            if torch.cuda.is_current_stream_capturing():
                _GRAPH_KEEP.append((host, dev))          # a captured copy node re-reads the pinned table at every replay
            launch("tdvc_wgrad_reduce_batch", dev, dev.data_ptr() + nb_j, n, int(starts[n]))
        self.items.clear()


_GRAPH_KEEP: list = []


def jobs_device(jobs):
    return torch.device("cuda", torch.cuda.current_device())


def _wgrad_tables(pc: PackedConv, cin: int, taps):
    """plain-geometry tables (also for layers that RUN in space-to-depth form) for an input of `cin` channels, and the tap arrays"""
    o = pc.orig
    return (convpack.forward_tables(pc.layout, cin_pad=cin, taps=taps, pad=o["pad"], ck=8, shuffle=pc.shuffle, cin_perm=o["cin_perm"], device=pc.w.device),
            (C.c_int8 * len(taps))(*[t[0] for t in taps]), (C.c_int8 * len(taps))(*[t[1] for t in taps]))


def _wgrad_static(pc: PackedConv, cin: int, N: int, Ho: int, Wo: int, taps):
    """what the weight-gradient launches of a layer at one geometry share -> (tables, the launch's arguments between its maps and
    `square_x`, workspace floats).  The tables are the layer's for `cin` input channels: another channel count builds them again"""
    o = pc.orig
    tb, dy, dxs = pc.wgrad.of("tables", cin, _wgrad_tables, pc, cin, taps)
    return (tb, (pc.cout, o["kh"], o["kw"], o["stride"], o["pad"], len(taps), dy, dxs, tb.row_off, tb.chan_off, tb.tap_off),
            L.lib().tdvc_conv_wgrad_work_floats(pc.cout, cin, len(taps), N, Ho, Wo))


def conv_wgrad(pc: PackedConv, g: FM, x: FM, dw: torch.Tensor, scale=1.0, square_x=False, db: torch.Tensor | None = None,
               defer: WgradBatch | None = None) -> None:
    """dW += scale * dL/dW (fp32, the parameter's own layout); `g` as in conv_dgrad.  With `db` the bias gradient
    (what `conv_bgrad` computes) comes out of the same launch: the kernel already holds the dY tiles.  `pc.orig["wgrad_taps"]` widens
    the tap list beyond the forward's (masked convs: the reference's autograd also fills the masked taps)."""
    o = pc.orig
    taps = o.get("wgrad_taps") or o["taps"]
    assert dw.is_cuda and dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == pc.wsrc.numel()
    Ho, Wo = g.H, g.W
    tb, static, nwork = pc.wgrad.of("launch", (x.C, x.N, Ho, Wo), _wgrad_static, pc, x.C, x.N, Ho, Wo, taps)
    work = torch.empty((nwork,), dtype=torch.float32, device=dw.device)
    if FORCE_KEEP is not None:
        FORCE_KEEP.append(work)
    bidx = None
    if db is not None:
        assert db.is_cuda and db.dtype == torch.float32 and db.is_contiguous() and db.numel() >= pc.cout
        bidx = _bias_index(pc, db.device)
    args = (g, x, *static, int(square_x), scale, dw, bidx, db, work, nwork)
    split = x.f32 and F32_SPLIT_TRAIN               # ops.f32_split_train: six bf16 MFMA products per MAC; every geometry, or an error
    if defer is not None and PROFILE is None:
        job = L.WgradReduceJob()
        launch("tdvc_conv_wgrad_partials_split" if split else "tdvc_conv_wgrad_partials", *args, job)
        defer.add(job, (work, dw, db, tb, bidx))             # the workspace and the tables live until the flush
        return
    _profiled("conv_wgrad_split" if split else "conv_wgrad_f32" if x.f32 else "conv_wgrad",
              f"{o['kh']}x{o['kw']} s{o['stride']} {x.C}->{pc.cout} @{x.N}x{x.H}x{x.W}",
              2.0 * x.N * Ho * Wo * pc.cout * x.C * len(taps),
              lambda: launch("tdvc_conv_wgrad_bias_split" if split else "tdvc_conv_wgrad_bias", *args, what="conv_wgrad_split" if split else "conv_wgrad"),
              flops_real=2.0 * x.N * Ho * Wo * pc.cout * pc.cin_real * len(taps),
              # geometry class (kh, kw, stride, cin, cout, shuffle, square_x, masked): the op-level test coverage guard
              geo=(o["kh"], o["kw"], o["stride"], pc.cin_real, pc.cout, bool(pc.shuffle), bool(square_x), "wgrad_taps" in o))


def _bias_index(pc: PackedConv, device):
    if pc.bias_index is None and pc.shuffle:
        pc.bias_index = torch.from_numpy(convpack.shuffle_perm(pc.cout)).to(torch.int32).to(device)
    return pc.bias_index


def conv_bgrad(pc: PackedConv, g: FM, db: torch.Tensor, scale=1.0) -> None:
    """db += scale * sum over batch and pixels of g (rows un-permuted for sub-pixel layers)"""
    nwork = L.lib().tdvc_bias_grad_work_floats(g.N, g.C)
    work = torch.empty((nwork,), dtype=torch.float32, device=db.device)
    launch("tdvc_bias_grad", g, pc.cout, _bias_index(pc, db.device), scale, db, work, nwork)


def gdn_backward(g: FM, x: FM, n32: FM, inverse: bool, dx: FM) -> FM:
    """-> dn (x's dtype); dx += g * n^(-+1/2)"""
    dn = FM.empty(g.N, g.H, g.W, g.C, dtype=x.t.dtype, device=g.t.device)
    launch("tdvc_gdn_backward", g, x, n32, int(inverse), dn, dx)
    return dn


def mul2_accumulate(dx: FM, x: FM, t: FM) -> None:
    launch("tdvc_mul2_accumulate", dx, x, t)


def copy_cast(src: FM, dst: FM) -> FM:
    launch("tdvc_copy_cast", src, dst)
    return dst


def cast_f32(x: FM) -> FM:
    """a recorded fp16 -> fp32 copy: the entry of an fp32 island (`estmv.float()`, pnet.py:34,58); its backward rounds the island's
    fp32 input gradient into the fp16 mirror"""
    out = copy_cast(x, FM.empty(x.N, x.H, x.W, x.C, dtype=torch.float32, device=x.t.device))
    _rec("cast", x, out)
    return out


def clamp01_backward(g: FM, y: FM) -> FM:
    launch("tdvc_clamp01_backward", g, y)
    return g


def gate_backward(g: FM, a: FM, gate: torch.Tensor, da: FM | None, dgate: torch.Tensor) -> None:
    nwork = L.lib().tdvc_gate_backward_work_floats(g.N, g.C)
    work = torch.empty((nwork,), dtype=torch.float32, device=gate.device)
    launch("tdvc_gate_backward", g, a, gate, da, dgate, work, nwork)


def se_gate_backward(p: "SEParams", partial: torch.Tensor, nblocks: int, npix: int, gate: torch.Tensor, dgate: torch.Tensor, scale: float,
                     grads) -> torch.Tensor:
    """-> dmean [N][C]; parameter gradients accumulate into `grads` = (dw1, db1, dw2, db2)"""
    N = gate.shape[0]
    dmean = torch.empty_like(gate)
    launch("tdvc_se_gate_backward", partial, nblocks, 1.0 / npix, N, p.C, p.Cmid, p.w1, p.b1, p.w2, p.b2, gate, dgate, scale, dmean, *grads[:4])
    return dmean


def bcast_channel_add(dx: FM, v: torch.Tensor, scale: float) -> None:
    launch("tdvc_bcast_channel_add", dx, v, scale)


def add_flow_backward(doff: FM, dflow: FM) -> None:
    launch("tdvc_add_flow_backward", doff, dflow)


def bcast_add_act_backward(dx: FM, x: FM, db: FM, slope: float) -> None:
    launch("tdvc_bcast_add_act_backward", dx, x, db, slope)


def upsample2x_backward(dy: FM, dx: FM) -> None:
    launch("tdvc_upsample2x_backward", dy, dx)


DCN_PLANAR_MIN_PIXELS = 1 << 16      # below this the map is L2-resident anyway and the extra pass does not pay
DCN_PLANAR = __import__("os").environ.get("TDVC_DCN_PLANAR", "0") == "1"


TRAIN_MODEL_FP32 = False      # inside `with train_model_fp32(True)`: dcn_fused on fp32 maps records under a tape


class train_model_fp32:
    """`with ops.train_model_fp32(on):` -- VideoCompressor.forward's whole-model fp32 training mode for the calls inside the block"""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        global TRAIN_MODEL_FP32
        self.prev, TRAIN_MODEL_FP32 = TRAIN_MODEL_FP32, self.on
        return self

    def __exit__(self, *exc):
        global TRAIN_MODEL_FP32
        TRAIN_MODEL_FP32 = self.prev
        return False


def dcn_fused(x: FM, om: FM, pc: PackedConv, out: FM, groups=8, act=ACT_NONE, slope=0.0, round16=True, planar: bool | None = None) -> FM:
    """`planar` (default: large maps): gather from a group-planar copy of x made by the same call (one extra pass over x;
    the 288 bilinear corner gathers per pixel then share 128-byte lines between neighbouring pixels of a group).
    An fp32 `x` selects the fp32 kernel (csrc/dcn_f32.hip: fp32 samples, offsets, mask and accumulation, the layer's fp32 weight
    packing); `om` is then fp32 too, `out` fp32 or fp16, and there is no planar form.  Under a tape fp32 maps are recorded only in the
    whole-model fp32 training mode (TRAIN_MODEL_FP32, VideoCompressor.train_model_fp32), with an fp16 `out` as the model calls it;
    otherwise the fp32 form is inference only."""
    if x.f32 and TAPE is not None and not (TRAIN_MODEL_FP32 and not out.f32):
        raise L.TdvcHipError("dcn_fused on fp32 maps is an inference form (no backward) outside the whole-model fp32 training mode")
    d = L.DcnDesc()
    d.x, d.om, d.y = x.desc(), om.desc(), out.desc()
    d.w, d.bias = (pc.packed_f32() if x.f32 else pc.w).data_ptr(), pc.bias.data_ptr()
    d.groups, d.act, d.slope, d.round_before_act = groups, act, slope, int(round16)
    if planar is None:
        planar = DCN_PLANAR and x.H * x.W >= DCN_PLANAR_MIN_PIXELS and not x.f32
    scratch = torch.empty((x.N, groups, x.H, x.W, 8), dtype=torch.float16, device=x.t.device) if planar else None
    d.x_planar = scratch.data_ptr() if scratch is not None else None
    launch("tdvc_dcn_fused", d)
    _rec("dcn_fused", x, om, pc, out, groups, act, slope)
    return out


def dcn_col2im_tile() -> int:
    """side of the pixel tile one workgroup of dcn_col2im scatters (its LDS window reaches one tile further on every side)"""
    return int(L.lib().tdvc_dcn_col2im_tile())


def dcn_columns(x: FM, om: FM, groups: int) -> FM:
    """the sampled, modulated columns (N, H, W, 72 groups) in the dtype of `x` (`om` must have it too)"""
    col = FM.empty(x.N, x.H, x.W, 72 * groups, dtype=x.t.dtype, device=x.t.device)
    _profiled("dcn_columns_f32" if x.f32 else "dcn_columns", f"G{groups} @{x.N}x{x.H}x{x.W}", 2.0 * 4 * 72 * groups * x.N * x.H * x.W,
              lambda: launch("tdvc_dcn_columns", x, om, groups, col))
    return col


# Run-to-run reproducible training (tests/test_model_gpu.py trains its operating-point model with it): the one operator whose
# result depends on arrival order -- the float atomics of the DCN's bilinear scatter for samples displaced out of their
# tile's window -- records those samples and adds them in sorted key order instead.  Costs a host synchronisation per step.
DETERMINISTIC = False


def dcn_col2im(x: FM, om: FM, dcol: FM, groups: int, dom: FM) -> FM:
    """-> dx as an fp32 FM (fresh; scatter through per-tile windows); offset / mask gradients accumulate into `dom`.  x, om, dcol and
    dom are all fp16 or all fp32 maps (a mix is refused before any launch)"""
    dx32 = FM.zeros(x.N, x.H, x.W, x.C, dtype=torch.float32, device=x.t.device)
    nwork = L.lib().tdvc_dcn_col2im_work_floats(x.N, x.H, x.W, groups)
    work = torch.empty((nwork,), dtype=torch.float32, device=x.t.device)
    entry, args = "tdvc_dcn_col2im", (x, om, dcol, groups, dx32.t, dom, work, nwork)
    if DETERMINISTIC:
        dev = x.t.device
        cap = max(1 << 16, x.N * x.H * x.W * groups * 36 // 8)          # an eighth of all samples far out of their window
        keys = torch.empty((cap,), dtype=torch.int64, device=dev)
        vals = torch.empty((cap, 8), dtype=torch.float32, device=dev)
        cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
        entry, args = "tdvc_dcn_col2im_det", args + (keys, vals, cnt, cap)
    _profiled("dcn_col2im_f32" if x.f32 else "dcn_col2im", f"G{groups} @{x.N}x{x.H}x{x.W}", 2.0 * 4 * 3 * 72 * groups * x.N * x.H * x.W,
              lambda: launch(entry, *args))
    if DETERMINISTIC:
        n = int(cnt.item())
        if n > cap:
            raise L.TdvcHipError(f"dcn_col2im (deterministic): {n} far samples exceed the record capacity {cap}")
        if n:
            ks, order = torch.sort(keys[:n], stable=True)
            launch("tdvc_dcn_far_apply", ks, order, vals, n, dx32.t)
    return dx32


def dcn_column_conv(pc: PackedConv, groups: int) -> PackedConv:
    """the DCN weight (cout, 8G, 3, 3) as a 1x1 conv over the 72G column channels k = g*72 + t*8 + j, input channel
    c = g*8 + j (weight offset c*9 + t)"""
    if pc.column is None:
        cin = 8 * groups
        chan = np.array([(g * 8 + j) * 9 + t for g in range(groups) for t in range(9) for j in range(8)], dtype=np.int64)
        lay = convpack.WeightLayout(pc.cout, 9 * cin, 1, 1, np.arange(pc.cout, dtype=np.int64) * cin * 9, chan, np.zeros(1, dtype=np.int64))
        pc.column = pack_conv(pc.wsrc, None, stride=1, pad=0, layout=lay, param_w=pc.param_w)
    return pc.column


def sigmoid_f32(x: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(x)
    launch("tdvc_sigmoid_f32", x, out, x.numel())
    return out


def sigmoid_backward_f32(g: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    launch("tdvc_sigmoid_backward_f32", g, s, g.numel())
    return g


def axpy_f32(dst: torch.Tensor, src: torch.Tensor, scale: float) -> None:
    assert dst.numel() == src.numel() and dst.dtype == src.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    launch("tdvc_axpy_f32", dst, src, scale, dst.numel())


# ----------------------------------------------------------------------------- elementwise / SE
def scale_act_res3(a: FM, out: FM, b: FM, out3: FM, b_sign=-1.0, gate: torch.Tensor | None = None, act=ACT_NONE, slope=0.0,
                   res: FM | None = None, res_sign=1.0) -> FM:
    """scale_act_res into `out`, and out3 = b + b_sign * out from the rounded `out` -- in the same launch (tdvc_scale_act_res3) when
    every map is fp16, else as a second launch; the same bytes either way.  Inference only."""
    if TAPE is not None and not _IN_BACKWARD:
        raise L.TdvcHipError("scale_act_res3 is an inference-only fusion (under the tape: two scale_act_res calls)")
    if not (a.f32 or out.f32 or b.f32 or out3.f32 or (res is not None and res.f32)):
        launch("tdvc_scale_act_res3", a, gate, act, slope, res, res_sign, out, b, b_sign, out3)
        return out
    scale_act_res(a, out, gate=gate, act=act, slope=slope, res=res, res_sign=res_sign)
    scale_act_res(b, out3, res=out, res_sign=b_sign)
    return out


def scale_act_res(a: FM, out: FM, gate: torch.Tensor | None = None, act=ACT_NONE, slope=0.0, res: FM | None = None,
                  res_sign=1.0, out2: FM | None = None) -> FM:
    launch("tdvc_scale_act_res", a, gate, act, slope, res, res_sign, out, out2)
    _rec("scale_act_res", a, out, gate, act, slope, res, res_sign, out2)
    return out


def clone(x: FM) -> FM:
    """a recorded copy: the in-place kernels below run on it under the tape, so that the producer of `x` still finds
    its own output (activation sign, weight-gradient operand) in the backward pass"""
    out = copy_cast(x, FM.empty(x.N, x.H, x.W, x.C, dtype=x.t.dtype, device=x.t.device))
    _rec("clone", x, out)
    return out


def add_flow(off: FM, flow: FM):
    launch("tdvc_add_flow", off, flow)
    _rec("add_flow", off, flow)


def bcast_add_act(x: FM, b: FM, T: int, slope: float):
    launch("tdvc_bcast_add_act", x, b, T, slope)
    _rec("bcast_add_act", x, b, slope)


@dataclass
class SEParams:
    w1: torch.Tensor
    b1: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    C: int
    Cmid: int
    params: tuple = ()       # the four nn.Parameters (gradient accumulators), same storage as w1 / b1 / w2 / b2


FUSE_CHAN_SUM = True           # A/B switch: the SELayer's channel sums from the producing conv's epilogue (conv(..., chan_sum=[]))


def se_gate(x: FM, p: SEParams, partial=None) -> torch.Tensor:
    """gate[N][C] fp32 (`main/model/inflate.py:204-208` without the final multiply).  `partial` = (tensor [N][rows][C], rows): the
    channel sums of `x` that its producer already wrote (conv(..., chan_sum=)); otherwise one pass over x (tdvc_channel_sum)."""
    npix = x.H * x.W
    gate = torch.empty((x.N, x.C), dtype=torch.float32, device=x.t.device)
    if partial is not None:
        partial, nblocks = partial
        assert tuple(partial.shape) == (x.N, nblocks, x.C) and partial.dtype == torch.float32
    else:
        nblocks = max(1, min(1024, npix // 256))      # 4 workgroups per CU at full resolution: 64 KB of loads in flight per CU
        partial = torch.empty((x.N, nblocks, x.C), dtype=torch.float32, device=x.t.device)
        launch("tdvc_channel_sum", x, partial, nblocks)
    launch("tdvc_se_gate", partial, nblocks, 1.0 / npix, x.N, p.C, p.Cmid, p.w1, p.b1, p.w2, p.b2, gate)
    _rec("se_gate", x, p, partial, nblocks, gate)
    return gate


# ----------------------------------------------------------------------------- resampling
def upsample2x(x: FM, out: FM | None = None) -> FM:
    if out is None:
        out = FM.empty(x.N, 2 * x.H, 2 * x.W, x.C, dtype=x.t.dtype, device=x.t.device)
    launch("tdvc_upsample2x", x, out)
    _rec("upsample2x", x, out)
    return out


def avgpool2(x: FM) -> FM:
    out = FM.empty(x.N, x.H // 2, x.W // 2, x.C, dtype=torch.float32, device=x.t.device)
    launch("tdvc_avgpool2", x, out)
    return out


def avgpool2_pyramid_supported(a: FM, b: FM) -> bool:
    return a.f32 and b.f32 and (a.N, a.H, a.W, a.C) == (b.N, b.H, b.W, b.C) and a.C <= 4 and a.H % 32 == 0 and a.W % 32 == 0


def avgpool2_pyramid(a: FM, b: FM) -> tuple:
    """five chained avgpool2 levels of both maps in one launch -> ([a/2, a/4, ..., a/32], [b/2, ..., b/32]), separate buffers"""
    lv = lambda x: [FM.empty(x.N, x.H >> k, x.W >> k, x.C, dtype=torch.float32, device=x.t.device) for k in range(1, 6)]
    la, lb = lv(a), lv(b)
    launch("tdvc_avgpool2_pyramid", a, b, (L.FMapDesc * 5)(*[f.desc() for f in la]), (L.FMapDesc * 5)(*[f.desc() for f in lb]))
    return la, lb


def spynet_level_input(ref: FM, supp: FM, flow_lo: FM | None, flow_up: FM, cat8: FM):
    launch("tdvc_spynet_level_input", ref, supp, flow_lo, flow_up, cat8)
    _rec("spynet_level_input", supp, flow_lo, flow_up, cat8)


def spynet_level_input_backward(supp: FM, flow_up: FM, dcat8: FM, dflow_up: FM, dflow_lo: FM | None) -> None:
    launch("tdvc_spynet_level_input_backward", supp, flow_up, dcat8, dflow_up, dflow_lo)


def resize_bilinear(x: FM, H: int, W: int, chscale: torch.Tensor | None = None) -> FM:
    if chscale is not None and (chscale.dtype != torch.float32 or chscale.numel() < x.C):
        raise ValueError(f"resize_bilinear: chscale needs one fp32 scale per channel ({x.C}), got {chscale.numel()} of {chscale.dtype}")
    out = FM.empty(x.N, H, W, x.C, dtype=torch.float32, device=x.t.device)
    launch("tdvc_resize_bilinear", x, out, chscale)
    _rec("resize_bilinear", x, out, chscale)
    return out


def resize_bilinear_backward(dy: FM, dx: FM, chscale: torch.Tensor | None = None) -> None:
    launch("tdvc_resize_bilinear_backward", dy, dx, chscale)


# ----------------------------------------------------------------------------- in-loop filter matching
def avgpool_k(x: FM, scale: int, out: torch.Tensor | None = None) -> torch.Tensor:
    hp, wp = x.H // scale, x.W // scale
    pooled = torch.empty((x.N, hp, wp, x.C), dtype=torch.float32, device=x.t.device) if out is None else out
    assert pooled.shape == (x.N, hp, wp, x.C) and pooled.dtype == torch.float32 and pooled.is_contiguous()
    nwork = L.lib().tdvc_avgpool_k_work_floats(x.N, hp, wp, x.C, scale)
    work = torch.empty((nwork,), dtype=torch.float32, device=x.t.device)
    launch("tdvc_avgpool_k", x, scale, pooled, hp, wp, work, nwork)
    _log_predicated(2)               # strip pass + final pass
    return pooled


def patch_match(pin: torch.Tensor, pref: torch.Tensor) -> torch.Tensor:
    N, hp, wp, Cc = pin.shape
    Lp = ((hp + 3) // 3 + 1) * ((wp + 3) // 3 + 1)
    idx = torch.empty((N, Lp), dtype=torch.int32, device=pin.device)
    launch("tdvc_patch_match", pin, pref, N, hp, wp, Cc, idx)
    return idx


def match_gather(fin: FM, fref: FM, idx: torch.Tensor, scale: int, cat: FM):
    launch("tdvc_match_gather", fin, fref, idx, scale, fin.H // scale, fin.W // scale, cat)
    _rec("match_gather", fin, fref, idx, scale, cat)


def match_gather_backward(fin: FM, fref: FM, idx: torch.Tensor, scale: int, dcat: FM, dfin: FM, dfref: FM) -> None:
    launch("tdvc_match_gather_backward", fin, fref, idx, scale, fin.H // scale, fin.W // scale, dcat, dfin, dfref)


# ----------------------------------------------------------------------------- entropy model
def eb_forward(z: FM, params: torch.Tensor, z_hat: FM, bits_out: torch.Tensor, noise: FM | None = None):
    numel = z.N * z.H * z.W * z.C
    cap = (numel + 255) // 256
    partial = torch.empty(cap, dtype=torch.float32, device=z.t.device)
    launch("tdvc_eb_forward", z, params, noise, z_hat, bits_out, partial, cap)
    _rec("eb_forward", z, params, z_hat, noise)


def eb_pack(raw_table: torch.Tensor, quantiles: torch.Tensor, packed: torch.Tensor, Cn: int) -> None:
    launch("tdvc_eb_pack", raw_table, quantiles, packed, Cn)


def eb_param_chain(dpacked: torch.Tensor, raw_table: torch.Tensor, grad_table: torch.Tensor, scale: float, Cn: int) -> None:
    assert dpacked.is_contiguous() and dpacked.dtype == torch.float32 and tuple(dpacked.shape) == (Cn, 59)
    launch("tdvc_eb_param_chain", dpacked, raw_table, grad_table, scale, Cn)


def eb_aux(params: torch.Tensor, quantiles: torch.Tensor, target: float, dq: torch.Tensor, loss: torch.Tensor, Cn: int) -> None:
    assert quantiles.is_contiguous() and dq.is_contiguous() and quantiles.numel() == 3 * Cn == dq.numel() and dq.dtype == torch.float32
    launch("tdvc_eb_aux", params, quantiles, target, dq, loss, Cn)


def eb_backward(z: FM, params: torch.Tensor, noise: FM, gscale: float, dz: FM, dparams: torch.Tensor) -> None:
    launch("tdvc_eb_backward", z, params, noise, gscale, dz, dparams)


def gc_backward(y: FM, gp: FM, noise: FM, gscale: float, dy: FM, dgp: FM) -> None:
    launch("tdvc_gc_backward", y, gp, noise, gscale, dy, dgp)


def gc_forward(y: FM, gp: FM, bits_out: torch.Tensor, noise: FM | None = None):
    numel = y.N * y.H * y.W * y.C
    cap = (numel + 255) // 256
    partial = torch.empty(cap, dtype=torch.float32, device=y.t.device)
    launch("tdvc_gc_forward", y, gp, noise, bits_out, partial, cap)
    _rec("gc_forward", y, gp, noise)


def rate_branch(descs: list, eb_after: int, z: FM, eb_params: torch.Tensor, z_hat: FM, y: FM, gp: FM, bits: torch.Tensor, which: int,
                split: bool = False) -> list:
    """a coder's rate branch on the side stream of the launch stream (`tdvc_rate_branch`): the convs `descs` (conv_desc()'s descriptors)
    in order, `eb_forward(z, eb_params, z_hat, bits[1:2])` behind descs[eb_after - 1] and `gc_forward(y, gp, bits[0:1])` behind the last,
    as slot `which`.  -> the tensors the call allocated (the two reductions' partial buffers): the caller keeps them, and everything
    else the branch touches, referenced until `rate_join(which)` has been enqueued -- the allocator of the launch stream owns them all
    and knows nothing of the side stream"""
    assert bits.dtype == torch.float64 and bits.numel() == 2 and bits.is_contiguous() and PROFILE is None and TAPE is None
    dev = z.t.device
    ecap, gcap = (z.N * z.H * z.W * z.C + 255) // 256, (y.N * y.H * y.W * y.C + 255) // 256
    epart = torch.empty(ecap, dtype=torch.float32, device=dev)
    gpart = torch.empty(gcap, dtype=torch.float32, device=dev)
    convs = (L.ConvDesc * len(descs))(*descs)
    chain = L.RateChainDesc(convs, len(descs), eb_after, z.desc(), z_hat.desc(), eb_params.data_ptr(), epart.data_ptr(), ecap, gcap,
                            gpart.data_ptr(), y.desc(), gp.desc(), bits.data_ptr(), which, int(split))
    launch("tdvc_rate_branch", chain)
    return [epart, gpart]


def rate_join(which: int) -> None:
    """the launch stream waits for slot `which` of its side stream (`tdvc_rate_join`); nothing pending there: a no-op"""
    L.check(L.lib().tdvc_rate_join(_stream(), which), "rate_join")


def quantize(y: FM, out: FM, noise: FM | None = None) -> FM:
    launch("tdvc_quantize", y, noise, out)
    _rec("quantize", y, out, noise)
    return out


# ----------------------------------------------------------------------------- entropy coding (host + AR kernels)
def pmf_to_quantized_cdf(pmf: np.ndarray, precision: int = 16) -> np.ndarray:
    p = np.ascontiguousarray(pmf, dtype=np.float32)
    out = np.zeros(p.size + 1, dtype=np.int32)
    launch("tdvc_pmf_to_quantized_cdf", p.ctypes.data, p.size, precision, out.ctypes.data, host=True)
    return out


class CdfTables:
    """host copies of an entropy model's quantised CDFs in the layout the range coder takes"""

    def __init__(self, cdf: torch.Tensor, lengths: torch.Tensor, offsets: torch.Tensor):
        self.cdf = np.ascontiguousarray(cdf.detach().cpu().numpy(), dtype=np.int32)
        self.sizes = np.ascontiguousarray(lengths.detach().cpu().numpy().reshape(-1), dtype=np.int32)
        self.offsets = np.ascontiguousarray(offsets.detach().cpu().numpy().reshape(-1), dtype=np.int32)
        self.stride = self.cdf.shape[1]
        self.desc = L.CdfTablesDesc(self.cdf.ctypes.data, self.sizes.ctypes.data, self.offsets.ctypes.data, self.stride, len(self.sizes))      # tdvc_cdf_tables
        self._dev = {}

    def device(self, dev) -> L.CdfTablesDevDesc:
        """the tables in device memory as the lane kernels read them (`tdvc_cdf_tables_dev`), made once per device: every table's
        entries end to end as uint16 (a table's last entry, 1 << 16, wraps to 0: the kernel implies it), padded to a multiple
        of 8; per table its start in that array, its size, its offset.  The descriptor's `keep` holds the four tensors."""
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._dev:
            starts = np.concatenate([[0], np.cumsum(self.sizes[:-1])]).astype(np.int32)
            n16 = (int(self.sizes.sum()) + 7) // 8 * 8
            packed = np.zeros(n16, dtype=np.uint16)
            for t, (o, n) in enumerate(zip(starts, self.sizes)):
                packed[o:o + n] = self.cdf[t, :n].astype(np.uint16)
            keep = (torch.from_numpy(packed.view(np.int16)).to(dev),) + tuple(torch.from_numpy(a).to(dev) for a in (starts, self.sizes, self.offsets))
            d = L.CdfTablesDevDesc(*[a.data_ptr() for a in keep], n16, len(self.sizes))
            d.keep = keep
            self._dev[key] = d
        return self._dev[key]


def rans_encode(symbols: np.ndarray, indexes: np.ndarray, t: CdfTables) -> bytes:
    s = np.ascontiguousarray(symbols.reshape(-1), dtype=np.int32)
    i = np.ascontiguousarray(indexes.reshape(-1), dtype=np.int32)
    out = np.empty(4 * s.size + 64, dtype=np.uint8)
    n = L.lib().tdvc_rans_encode(s.ctypes.data, i.ctypes.data, s.size, t.cdf.ctypes.data, t.stride, t.sizes.ctypes.data,
                                 t.offsets.ctypes.data, out.ctypes.data, out.size)
    if n < 0:
        L.check(int(n), "rans_encode")
    return out[:n].tobytes()


class RansDecoder:
    def __init__(self, data: bytes):
        self._buf = np.frombuffer(data, dtype=np.uint8)
        self._h = L.lib().tdvc_rans_decoder_create(self._buf.ctypes.data, self._buf.size)
        if not self._h:
            L.check(-1, "rans_decoder_create")

    def decode(self, indexes: np.ndarray, t: CdfTables) -> np.ndarray:
        i = np.ascontiguousarray(indexes.reshape(-1), dtype=np.int32)
        out = np.empty(i.size, dtype=np.int32)
        launch("tdvc_rans_decoder_decode", self._h, i.ctypes.data, i.size, t.cdf.ctypes.data, t.stride, t.sizes.ctypes.data, t.offsets.ctypes.data,
               out.ctypes.data, what="rans_decode", host=True)
        return out

    def close(self):
        if self._h:
            L.lib().tdvc_rans_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


LANE_COUNTS = (64, 128)          # what the device decoder of a lane-split stream takes


def rans_encode_lanes(symbols: np.ndarray, indexes: np.ndarray, t: CdfTables, lanes: int = 64) -> bytes:
    """symbols / indexes [npos][M] in wavefront order -> the lane-split container (`tdvc_rans_encode_lanes`): header, length
    table, `lanes` sub-streams; channel c of every position goes to lane c % lanes"""
    s = np.ascontiguousarray(symbols, dtype=np.int32)
    i = np.ascontiguousarray(indexes, dtype=np.int32)
    if s.ndim != 2 or s.shape != i.shape:
        raise ValueError("rans_encode_lanes: symbols and indexes must both be [npos][M]")
    out = np.empty(8 * s.size + 16 * int(lanes) + 64, dtype=np.uint8)          # a symbol: at most 16 + 4 + 32 bits
    n = L.lib().tdvc_rans_encode_lanes(s.ctypes.data, i.ctypes.data, s.shape[0], s.shape[1], int(lanes), t.cdf.ctypes.data, t.stride,
                                       t.sizes.ctypes.data, t.offsets.ctypes.data, out.ctypes.data, out.size)
    if n < 0:
        msg = L.lib().tdvc_last_error().decode("utf-8", "replace")
        raise ValueError(f"rans_encode_lanes: {msg}")
    return out[:n].tobytes()


def rans_decode_lanes(data: bytes, indexes: np.ndarray, t: CdfTables) -> np.ndarray:
    """the host reference decoder of a lane-split container (`tdvc_rans_decode_lanes`); indexes [npos][M] -> symbols [npos][M]"""
    buf = np.frombuffer(data, dtype=np.uint8)
    i = np.ascontiguousarray(indexes, dtype=np.int32)
    if i.ndim != 2:
        raise ValueError("rans_decode_lanes: indexes must be [npos][M]")
    out = np.empty(i.shape, dtype=np.int32)
    launch("tdvc_rans_decode_lanes", buf.ctypes.data if buf.size else None, buf.size, i.ctypes.data, i.shape[0], i.shape[1], t.cdf.ctypes.data,
           t.stride, t.sizes.ctypes.data, t.offsets.ctypes.data, out.ctypes.data, host=True)
    return out


LANES_ENC_STATUS = {1: "a lane needs more than 65535 words, the length table holds at most 65535",
                    2: "a lane ran out of its scratch region (or met an index outside the tables / a position outside the image)"}


def ar_encode_lanes_sizes(npos: int, M: int, lanes: int):
    """-> (scratch words per lane, bytes of one image's container at most) for the device encoder of lane-split streams
    (`tdvc_ar_encode_lanes_scratch_words`, `tdvc_ar_encode_lanes_out_bytes`)"""
    w = int(L.lib().tdvc_ar_encode_lanes_scratch_words(int(npos), int(M), int(lanes)))
    o = int(L.lib().tdvc_ar_encode_lanes_out_bytes(int(npos), int(M), int(lanes)))
    if w < 0 or o < 0:
        L.check(min(w, o), "ar_encode_lanes_sizes")
    return w, o


def _lanes_out_stride(lanes: int, lane_words: int) -> int:
    return (4 + 2 * lanes + 4 * lanes * min(lane_words, 65535) + 15) // 16 * 16


def lanes_check_status(info: np.ndarray, who: str) -> None:
    """info words [B][2] = {bytes, status} of an encoder call (host array): a status is an error: 1 the host coder's ValueError,
    2 a RuntimeError"""
    for b in range(info.shape[0]):
        status = int(info[b, 1])
        if status == 1:
            raise ValueError(f"{who}: image {b}: {LANES_ENC_STATUS[1]}")
        if status:
            raise RuntimeError(f"{who}: image {b}: {LANES_ENC_STATUS.get(status, f'status {status}')}")


def lanes_strings(out: np.ndarray, info: np.ndarray, who: str):
    """the containers of an encoder call from its output buffer [B][stride] and info words (host arrays), statuses checked"""
    lanes_check_status(info, who)
    return [out[b, :int(info[b, 0])].tobytes() for b in range(info.shape[0])]


def rans_encode_lanes_dev_ref(symbols: np.ndarray, indexes: np.ndarray, pos: np.ndarray, t: CdfTables, lanes: int = 64, lane_words: int | None = None,
                              raw: bool = False):
    """the host twin of the device encoder (`tdvc_rans_encode_lanes_dev_ref`): symbols / indexes [B][H][W][M] as the context loop
    leaves them, pos [npos][2] the wavefront position list -> the B containers.  `lane_words`: scratch words per lane (default: what
    always suffices).  `raw`: -> (out [B][stride] uint8, info [B][2] uint32, scratch [B][lanes][lane_words] uint32) untouched by
    any check of the status"""
    s = np.ascontiguousarray(symbols, dtype=np.int32)
    i = np.ascontiguousarray(indexes, dtype=np.int32)
    p = np.ascontiguousarray(pos, dtype=np.int32)
    if s.ndim != 4 or s.shape != i.shape or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("rans_encode_lanes_dev_ref: symbols and indexes must both be [B][H][W][M], pos [npos][2]")
    B, H, W, M = s.shape
    if lane_words is None:
        lane_words = ar_encode_lanes_sizes(p.shape[0], M, lanes)[0]
    stride = _lanes_out_stride(int(lanes), int(lane_words))
    scratch = np.zeros((B, int(lanes), int(lane_words)), dtype=np.uint32)
    out = np.zeros((B, stride), dtype=np.uint8)
    if out.ctypes.data % 16:                                          # numpy aligns to 16 in practice; the entry point insists
        out = np.zeros(B * stride + 16, dtype=np.uint8)
        out = out[(-out.ctypes.data) % 16:][:B * stride].reshape(B, stride)
    info = np.full((B, 2), 0xFFFFFFFF, dtype=np.uint32)
    enc = L.LanesEncDesc(s.ctypes.data, i.ctypes.data, B, H, W, M, p.ctypes.data, p.shape[0], int(lanes), scratch.ctypes.data, int(lane_words), scratch.size,
                         out.ctypes.data, stride, out.size, info.ctypes.data)
    tabs = L.CdfTablesDesc(t.cdf.ctypes.data, t.sizes.ctypes.data, t.offsets.ctypes.data, t.stride, len(t.sizes))      # `t`: a CdfTables or anything with its four fields
    launch("tdvc_rans_encode_lanes_dev_ref", enc, tabs, host=True)
    if raw:
        return out, info, scratch
    return lanes_strings(out, info, "rans_encode_lanes_dev_ref")


class LanesEncoding:
    """the buffers of one `ar_encode_lanes_batch` call: they belong to the kernel until it is done, so the object is kept until then
    (the symbols / indexes it read included: they may have been allocated on another stream than the kernel's)"""

    def __init__(self, out, info, scratch, keep):
        self.out, self.info, self.scratch, self.keep = out, info, scratch, keep


def ar_encode_lanes_batch(symbols: torch.Tensor, indexes: torch.Tensor, pos: torch.Tensor, t: CdfTables, lanes: int = 64, lane_words: int | None = None,
                          scratch: torch.Tensor | None = None, out: torch.Tensor | None = None) -> LanesEncoding:
    """the range encoder of lane-split y streams on the device (`tdvc_ar_encode_lanes_batch`), enqueue-only: symbols / indexes int32
    [B][H][W][M] as `ar_wavefront_batch` leaves them, pos int32 [npos][2] (the wavefront position list) -> LanesEncoding with
    out uint8 [B][stride] (image b's container at row b), info int32 [B][2] = {container bytes, status} (`lanes_strings` reads
    both once they are on the host).  `lane_words` / `scratch` / `out`: scratch words per lane and caller-provided buffers
    (default: what always suffices, allocated here)"""
    assert symbols.dtype == torch.int32 and indexes.dtype == torch.int32 and pos.dtype == torch.int32 and symbols.is_contiguous() and indexes.is_contiguous()
    assert symbols.dim() == 4 and symbols.shape == indexes.shape and pos.dim() == 2 and pos.shape[1] == 2 and pos.is_contiguous()
    B, H, W, M = symbols.shape
    dev = symbols.device
    if lane_words is None:
        lane_words = ar_encode_lanes_sizes(pos.shape[0], M, lanes)[0]
    stride = _lanes_out_stride(int(lanes), int(lane_words))
    if scratch is None:
        scratch = torch.empty((B, int(lanes), int(lane_words)), dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty((B, stride), dtype=torch.uint8, device=dev)
    assert scratch.dtype == torch.int32 and out.dtype == torch.uint8 and scratch.is_contiguous() and out.is_contiguous()
    info = torch.empty((B, 2), dtype=torch.int32, device=dev)
    td = t.device(dev)
    enc = L.LanesEncDesc(symbols.data_ptr(), indexes.data_ptr(), B, H, W, M, pos.data_ptr(), pos.shape[0], int(lanes), scratch.data_ptr(), int(lane_words),
                         scratch.numel(), out.data_ptr(), stride, out.numel(), info.data_ptr())
    launch("tdvc_ar_encode_lanes_batch", enc, td)
    return LanesEncoding(out, info, scratch, (symbols, indexes, pos, td))


def lanes_of(data: bytes) -> int:
    """the lane count a lane-split container declares"""
    if len(data) < 4 or data[0:2] != b"L\x01" or data[3] != 0:
        raise ValueError("not a lane-split y stream (order=\"lanes\")")
    return data[2]


# ---- the context loop (tdvc_ar_*_batch): a step's positions of all B images of a call in the same launches; one image is B = 1.
# y / y_hat / params are FMs with N = B; row b * npos + k of x1 / pc / gp is position k of image b; symbols / indexes are [B][H][W][M] or [B][H * W][M].
def ar_last_loop_launches() -> int:
    """kernel enqueues of this thread's last context-loop call (`tdvc_ar_last_loop_launches`), conv launches included"""
    return int(L.lib().tdvc_ar_last_loop_launches())


def ar_chain_kernels(descs: list, rows: int) -> tuple:
    """the kernels `tdvc_conv_select` names for the context loop's conv descriptors when a step has `rows` rows (None: rejected).
    Host arithmetic on the descriptors alone: needs no device."""
    out = []
    for d0 in descs:
        d = L.ConvDesc.from_buffer_copy(d0)
        d.x.W = d.y.W = rows
        name = L.lib().tdvc_conv_select(d)
        out.append(name.decode() if name else None)
    return tuple(out)


def ar_batch_ok(descs: list, g: int, nmax: int) -> bool:
    """may `g` images share the launches of a context loop whose largest step has `nmax` positions?  A row's bits must not depend
    on the row count (any encoder batch size decodes at any decoder batch size).  The kernels the chain runs on are row-count
    independent each (conv_mfma_v9, conv_f32: a pixel is one MFMA column, the K split depends on the layer alone); the SELECTION
    is not (conv_v9_eligible leaves v9 above LARGE_MAP_PIXELS pixels and, where v3 is eligible, above conv_v9_work_limit() pixels x
    cout).  So: one and the same kernel per descriptor at 1 row, at the largest single-image step and at g times that."""
    one = ar_chain_kernels(descs, 1)
    return g == 1 or (None not in one and one == ar_chain_kernels(descs, nmax) == ar_chain_kernels(descs, g * nmax))


def ar_batch_groups(descs: list, B: int, nmax: int) -> list:
    """B images as the largest groups `ar_batch_ok` allows, in order -> the group sizes (they add up to B)"""
    out, left = [], B
    while left > 0:
        g = next(g for g in range(left, 0, -1) if ar_batch_ok(descs, g, nmax))
        out.append(g)
        left -= g
    return out


def ar_gather_batch(y_hat: FM, params: FM, pos: torch.Tensor, npos: int, x1: FM, pc: FM):
    assert pos.numel() >= 2 * npos
    launch("tdvc_ar_gather_batch", y_hat, params, pos, npos, x1, pc)


def _ar_rows_ok(a: torch.Tensor, y_hat: FM, cbase: int, npos: int) -> bool:
    return a.dtype == torch.int32 and a.is_contiguous() and a.numel() >= y_hat.N * y_hat.H * y_hat.W * y_hat.C and cbase + npos <= y_hat.H * y_hat.W


def ar_quantize_batch(y: FM | None, gp: FM, pos: torch.Tensor, npos: int, table: torch.Tensor, y_hat: FM, symbols: torch.Tensor,
                      indexes: torch.Tensor, symbols_in: torch.Tensor | None = None, cbase: int = -1):
    """`cbase` < 0: the arrays are raster [B][H][W][M]; else compact [B][H * W][M], this call's position k at row cbase + k of a block"""
    assert pos.numel() >= 2 * npos and all(_ar_rows_ok(a, y_hat, cbase, npos) for a in (symbols, indexes) + ((symbols_in,) if symbols_in is not None else ()))
    launch("tdvc_ar_quantize_batch", y, gp, pos, npos, table, table.numel(), symbols_in, y_hat, symbols, indexes, cbase)


def ar_indexes_batch(gp: FM, pos: torch.Tensor, npos: int, B: int, table: torch.Tensor, M: int, H: int, W: int, indexes: torch.Tensor, cbase: int = -1):
    assert pos.numel() >= 2 * npos and indexes.dtype == torch.int32 and indexes.numel() >= B * H * W * M and cbase + npos <= H * W
    launch("tdvc_ar_indexes_batch", gp, pos, npos, B, table, table.numel(), M, H, W, indexes, cbase)


def _host_strings(strings):
    """the B strings of a batched decoder call as the drivers take them: (keep-alive buffers, pointer array, size array)"""
    bufs = [np.frombuffer(s, dtype=np.uint8) for s in strings]
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data if b.size else None for b in bufs])
    sizes = (C.c_int64 * len(bufs))(*[b.size for b in bufs])
    return bufs, ptrs, sizes


class ArLoop:
    """the fixed parts of a `tdvc_ar_loop`, kept between calls on images of one geometry: the staging maps x1 / pc / gp, the conv
    descriptors over them (`descs`; `convs`: their ctypes array, built once), what they point into (`packed`: the PackedConvs, which
    Cheng2020Anchor._ar_setup compares with the live ones; `keep`: the chain's inner buffers), the position list `pos` (device int32
    [H * W][2] in step order) and the steps' sizes (None: a step per position, the raster order).  `key`, `host` and `serial` are the
    coder's to fill: its cache key, compress()'s pinned buffers, the raster-order loop of the geometry."""

    def __init__(self, x1: FM, pc: FM, gp: FM, descs: list, packed: list, keep, pos: torch.Tensor, step_sizes=None):
        self.x1, self.pc, self.gp, self.descs, self.packed, self.keep, self.pos = x1, pc, gp, descs, packed, keep, pos
        ss = self.step_sizes = None if step_sizes is None else np.ascontiguousarray(step_sizes, dtype=np.int32)
        assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.dim() == 2 and pos.shape[1] == 2 and (ss is None or int(ss.sum()) == pos.shape[0])
        self.nsteps, self.nmax = (pos.shape[0], 1) if ss is None else (ss.size, int(ss.max()))        # steps, positions of the largest
        self.convs = (L.ConvDesc * len(descs))(*descs)
        self.pos_long = pos.long()                                     # for torch indexing with the list
        self.key = self.host = self.serial = None

    def desc(self, y_hat: FM, params: FM, scale_table: torch.Tensor, idx: torch.Tensor, sym: torch.Tensor) -> L.ArLoopDesc:
        """the loop over B = y_hat.N images; idx / sym: int32 arrays of B * H * W * M elements"""
        assert _ar_rows_ok(idx, y_hat, 0, 0) and _ar_rows_ok(sym, y_hat, 0, 0) and self.pos.shape[0] == y_hat.H * y_hat.W
        return L.ArLoopDesc(y_hat.desc(), params.desc(), self.x1.desc(), self.pc.desc(), self.gp.desc(), self.convs, len(self.descs), self.pos.data_ptr(),
                            self.step_sizes.ctypes.data if self.step_sizes is not None else None, self.nsteps, scale_table.data_ptr(), scale_table.numel(),
                            idx.data_ptr(), sym.data_ptr())


def ar_wavefront_batch(loop: ArLoop, strings, t: CdfTables | None, y: FM | None, y_hat: FM, params: FM, scale_table: torch.Tensor, idx: torch.Tensor,
                       sym: torch.Tensor) -> None:
    """the context loop of the B = y_hat.N images over the loop's steps in one pass (`tdvc_ar_wavefront_batch`): encoder with `y` (idx / sym
    raster [B][H][W][M]), decoder with `strings` (B byte strings) + `t` (idx / sym [B][H * W][M] in step order)"""
    assert strings is None or len(strings) == y_hat.N
    keep, ptrs, sizes = _host_strings(strings) if strings is not None else (None, None, None)
    launch("tdvc_ar_wavefront_batch", loop.desc(y_hat, params, scale_table, idx, sym), y, ptrs, sizes, t.desc if t else None)


def ar_decode_serial_batch(loop: ArLoop, strings, t: CdfTables, y_hat: FM, params: FM, scale_table: torch.Tensor, idx: torch.Tensor, sym: torch.Tensor) -> None:
    """the decoder's serial context loop for raster-ordered streams over the B = y_hat.N images at once, B rows per position
    (`tdvc_ar_decode_serial_batch`; `loop`: a raster position list, no step sizes); fills y_hat, idx / sym [B][H][W][M]"""
    assert len(strings) == y_hat.N and loop.step_sizes is None
    keep, ptrs, sizes = _host_strings(strings)
    launch("tdvc_ar_decode_serial_batch", loop.desc(y_hat, params, scale_table, idx, sym), ptrs, sizes, t.desc)


def ar_lanes_batch_layout(sizes, lanes: int):
    """-> (bytes of the device buffer that holds B lane-split containers behind their table, the table as uint32 [B][2] =
    {byte offset, payload words}) (`tdvc_ar_lanes_batch_layout`)"""
    n = (C.c_int64 * len(sizes))(*[int(v) for v in sizes])
    table = np.zeros((len(sizes), 2), dtype=np.uint32)
    total = int(L.lib().tdvc_ar_lanes_batch_layout(n, len(sizes), int(lanes), table.ctypes.data))
    if total < 0:
        L.check(total, "ar_lanes_batch_layout")
    return total, table


def ar_lanes_pack_batch(strings, lanes: int, device):
    """the B containers packed as the lane kernels read them -> (device uint8 buffer: table | containers, table as numpy)"""
    total, table = ar_lanes_batch_layout([len(s) for s in strings], lanes)
    host = np.zeros(total, dtype=np.uint8)
    host[:table.nbytes] = table.reshape(-1).view(np.uint8)
    for (off, _), s in zip(table, strings):
        host[off:off + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(host).to(device), table


def ar_lanes_state_batch(lanes: int, B: int, device) -> torch.Tensor:
    """[B][lanes * 4 + 1] int32: per image the lane states and the sticky error word (the row's last element)"""
    return torch.zeros((B, int(L.lib().tdvc_ar_lanes_state_bytes(int(lanes))) // 4), dtype=torch.int32, device=device)


def ar_lanes_init_batch(streams_dev: torch.Tensor, B: int, lanes: int, state: torch.Tensor) -> None:
    """lane states of B containers from their length tables; `streams_dev` as `ar_lanes_pack_batch` lays it out (table at its head)"""
    assert streams_dev.dtype == torch.uint8 and streams_dev.numel() >= 16 and state.numel() * 4 >= B * L.lib().tdvc_ar_lanes_state_bytes(int(lanes))
    launch("tdvc_ar_lanes_init_batch", streams_dev, streams_dev.numel(), streams_dev, B, int(lanes), state)


def ar_decode_lanes_step_batch(gp: FM, pos: torch.Tensor, npos: int, table: torch.Tensor, streams_dev: torch.Tensor, lanes: int, t: CdfTables,
                               state: torch.Tensor, y_hat: FM, symbols: torch.Tensor, indexes: torch.Tensor, cbase: int) -> None:
    """one step of the on-device decoder over B = y_hat.N lane-split streams (`tdvc_ar_decode_lanes_step_batch`), B workgroups: the
    range decoder, the CDF indexes and the quantiser's write-back of `npos` positions; symbols / indexes rows cbase .. cbase + npos
    of every image's block of [B][H * W][M]"""
    td = t.device(y_hat.t.device)
    assert streams_dev.dtype == torch.uint8 and state.numel() * 4 >= y_hat.N * L.lib().tdvc_ar_lanes_state_bytes(int(lanes))
    assert pos.numel() >= 2 * npos and _ar_rows_ok(symbols, y_hat, cbase, npos) and _ar_rows_ok(indexes, y_hat, cbase, npos)
    launch("tdvc_ar_decode_lanes_step_batch", gp, pos, npos, table, table.numel(), streams_dev, streams_dev.numel(), streams_dev, int(lanes), td, state,
           y_hat, symbols, indexes, cbase)


def ar_wavefront_lanes_batch(loop: ArLoop, strings, t: CdfTables, stream_dev: torch.Tensor, state: torch.Tensor, y_hat: FM, params: FM, scale_table: torch.Tensor,
                             idx: torch.Tensor, sym: torch.Tensor) -> None:
    """the decoder's context loop of B = y_hat.N lane-split streams of one lane count in one pass (`tdvc_ar_wavefront_lanes_batch`):
    the strings are uploaded once into `stream_dev`, every step's range decoding runs on the device, one stream wait at the end;
    a damaged stream raises TdvcStreamError (a ValueError) whose `image` is the first image of the call whose error word is set"""
    assert len(strings) == y_hat.N and stream_dev.dtype == torch.uint8 and state.numel() * 4 >= y_hat.N * L.lib().tdvc_ar_lanes_state_bytes(lanes_of(strings[0]))
    keep, ptrs, nbytes = _host_strings(strings)
    bad = C.c_int32(-1)
    rc = launch("tdvc_ar_wavefront_lanes_batch", loop.desc(y_hat, params, scale_table, idx, sym), ptrs, nbytes, stream_dev, stream_dev.numel(), state,
                t.device(y_hat.t.device), bad, check=False)
    if rc != 0 and bad.value >= 0:
        e = L.TdvcStreamError(L.lib().tdvc_last_error().decode("utf-8", "replace"))
        e.image = bad.value
        raise e
    L.check(rc, "ar_wavefront_lanes_batch")


def round_symbols(z: FM, median: torch.Tensor) -> torch.Tensor:
    out = torch.empty((z.N, z.H, z.W, z.C), dtype=torch.int32, device=z.t.device)
    launch("tdvc_round_symbols", z, median, out)
    return out


# ----------------------------------------------------------------------------- `_ext` operator
def dcn_v2_forward(input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group):
    """Same arity / semantics as `_ext.dcn_v2_forward` (src/vision.cpp:3-8): fp32 contiguous
    NCHW cuda tensors in, freshly allocated output out; raises RuntimeError on violations
    (the reference raises through AT_ASSERTM, src/cuda/dcn_v2_cuda.cu:38-62)."""
    ts = (input, weight, bias, offset, mask)
    for t in ts:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("dcn_v2_forward: all tensors must be CUDA/HIP tensors (Not compiled with CPU support)")
        if t.dtype != torch.float32:
            raise RuntimeError("dcn_v2_forward: fp32 tensors only")
    input, weight, bias, offset, mask = [t.contiguous() for t in ts]
    B, Cc, H, W = input.shape
    Cout, Ck, kh_, kw_ = weight.shape
    if (kh_, kw_) != (kh, kw):
        raise RuntimeError(f"Input shape and kernel shape wont match: ({kh} x {kw} vs {kh_} x {kw_}).")
    if Cc != Ck:
        raise RuntimeError(f"Input shape and kernel channels wont match: ({Cc} vs {Ck}).")
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if offset.shape != (B, 2 * deformable_group * kh * kw, Ho, Wo) or mask.shape != (B, deformable_group * kh * kw, Ho, Wo):
        raise RuntimeError("dcn_v2_forward: offset/mask shape mismatch")
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=input.device)
    with torch.cuda.device(input.device):
        launch("tdvc_dcn_v2_forward_f32", input, weight, bias, offset, mask, out, B, Cc, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group,
               what="dcn_v2_forward")
    return out
