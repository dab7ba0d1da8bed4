"""Deterministic sweep of `tdvc_conv_desc`s for the forward conv dispatch (tests/test_conv_dispatch_cpu.py and the recorder
tests/golden/make_conv_dispatch.py).  The descriptors sit over dummy 16-byte-aligned HOST addresses: they are only ever
validated and dispatched on a machine without a GPU, never launched."""
import ctypes as C

GOLDEN = "conv_dispatch.npz"
REJECTED = "rejected"

# dummy buffers: distinct, 16-byte aligned, never dereferenced
PX, PY, PW, PB, PAUX, PR1, PR2 = (0x10000000 * (i + 1) for i in range(7))

MAPS = [(8, 30), (16, 16), (68, 120), (64, 128), (90, 92), (15, 600), (272, 480), (1088, 1920)]
SOME_MAPS = [(8, 30), (68, 120), (64, 128), (15, 600), (272, 480)]
CINS = [8, 16, 32, 64, 128, 192, 256]
COUTS = [2, 16, 32, 64, 128, 192, 216, 256, 512]
MASK12 = [(dy, dx) for dy in range(5) for dx in range(5)][:12]          # the context model's causal 5x5 mask
# (kh, kw, stride, pad, taps or None for dense)
WINDOWS = [(1, 1, 1, 0, None), (3, 3, 1, 1, None), (5, 5, 1, 2, None), (7, 7, 1, 3, None), (5, 5, 1, 2, MASK12),
           (1, 1, 2, 0, None), (3, 3, 2, 1, None)]
# the debug switches, one setting each that turns ONE kernel (or one conv_row geometry) off: (setter, off value, on value)
SWITCHES = [("tdvc_debug_enable_conv_v9", 0, 1), ("tdvc_debug_enable_conv_v10", 0, 1), ("tdvc_debug_enable_conv_v11", 0, 1),
            ("tdvc_debug_enable_conv_row", 15 & ~1, 15), ("tdvc_debug_enable_conv_row", 15 & ~2, 15),
            ("tdvc_debug_enable_conv_row", 15 & ~4, 15), ("tdvc_debug_enable_conv_row", 15 & ~8, 15),
            ("tdvc_debug_enable_conv_c8", 0, 1), ("tdvc_debug_enable_conv_n16", 0, 1), ("tdvc_debug_enable_gdn128", 0, 1)]
# every outcome the dispatch has; the golden must hold each at least MIN_PER_OUTCOME times ("direct" = any conv_mfma<..> name)
OUTCOMES = ["conv_f32", "conv_mfma_v9", "gdn128", "conv_mfma_v5", "conv_mfma_v5(bcast)", "conv_c8", "conv_n16", "conv_row", "conv_row(s2d)",
            "conv_mfma_v10", "conv_mfma_v7", "conv_mfma_v11", "conv_mfma_v3", "conv_mfma_v3(s2d)", "conv_mfma_v2", "direct", REJECTED]
MIN_PER_OUTCOME = 5


def pad8(c):
    return (c + 7) // 8 * 8


def fmap(L, p, N, H, W, Cc, sp=None, dtype=None):
    sp = Cc if sp is None else sp
    return L.FMapDesc(p, N, H, W, Cc, H * W * sp, sp, L.F16 if dtype is None else dtype)


def desc(L, pick_ck, cin, cout, win, H, W, N, *, act=0, slope=0.0, res=None, res2=None, out="f16", narrow=0, bias=True, round16=False,
         x_f32=False, ck=None):
    """A conv over an (N, H, W, cin) input; `H, W` is the OUTPUT map for stride 1 and the input map for stride 2.
    res / res2: None | "f16" | "f32"; out: "f16" | "f32" | "shuffle" | "nchw"; narrow: y.C = cout - narrow inside a cout-wide buffer."""
    kh, kw, stride, pad, taps = win
    taps = [(dy, dx) for dy in range(kh) for dx in range(kw)] if taps is None else taps
    d = L.ConvDesc()
    d.x = fmap(L, PX, N, H, W, cin, dtype=L.F32 if x_f32 else L.F16)
    d.w, d.bias = PW, (PB if bias else None)
    d.cout, d.ntaps = cout, len(taps)
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i] = dy, dx
    d.kh, d.kw, d.stride, d.pad = kh, kw, stride, pad
    d.ck = pick_ck(cin, cout, kh, kw, stride, pad) if ck is None else ck
    d.act, d.slope, d.round_before_act = act, slope, int(round16)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    fill_outputs(L, d, N, Ho, Wo, cout, res, res2, out, narrow)
    return d


def fill_outputs(L, d, N, Ho, Wo, cout, res=None, res2=None, out="f16", narrow=0):
    if out == "nchw":
        d.out_mode = L.OUT_NCHW_F32
        d.y = L.FMapDesc(PY, N, Ho, Wo, cout, cout * Ho * Wo, 1, L.F32)
        yc, ysp, yh, yw = cout, cout, Ho, Wo
    else:
        shuf = out == "shuffle"
        d.out_mode = L.OUT_SHUFFLE2 if shuf else L.OUT_NHWC
        ysp = pad8(cout // 4 if shuf else cout)
        yc, yh, yw = ysp - narrow, (2 * Ho if shuf else Ho), (2 * Wo if shuf else Wo)
        d.y = fmap(L, PY, N, yh, yw, yc, ysp, L.F32 if out == "f32" else L.F16)
    if res:
        d.res = fmap(L, PR1, N, yh, yw, yc, ysp, L.F32 if res == "f32" else L.F16)
    if res2:
        d.res2 = fmap(L, PR2, N, yh, yw, yc, ysp, L.F32 if res2 == "f32" else L.F16)


def s2d_desc(L, cin, cout, Ho, Wo, N, **kw):
    """the space-to-depth form of a 3x3 stride-2 conv: the virtual 2x2 / stride 1 / pad 1 conv, ck 32, over the (2 Ho, 2 Wo) input"""
    d = desc(L, None, cin, cout, (2, 2, 1, 1, None), 2 * Ho, 2 * Wo, N, ck=32)
    d.s2d = 1
    d.act, d.slope = kw.pop("act", 0), kw.pop("slope", 0.0)
    fill_outputs(L, d, N, Ho, Wo, cout, **kw)
    return d


def gdn_desc(L, ch, H, W, N, gdn, aux_is_x=True, res=None):
    """the GDN call of ops.conv: 1x1 over x^2, multiplicand aux == x"""
    d = desc(L, lambda *a: 32, ch, ch, (1, 1, 1, 0, None), H, W, N, res=res)
    d.square_input, d.gdn = 1, gdn
    d.aux = fmap(L, PX if aux_is_x else PAUX, N, H, W, ch)
    return d


def bcast_desc(L, cin, H, W, N, T=4, act=0, y_sp=256):
    d = desc(L, lambda *a: 32, cin, 64, (1, 1, 1, 0, None), H, W, N, act=act)
    d.y = fmap(L, PY, N, H, W, 64, y_sp)
    d.bcast_T, d.bcast_slope = T, 0.2
    return d


def malformed(L, pick_ck):
    base = lambda: desc(L, pick_ck, 64, 64, WINDOWS[1], 272, 480, 1)
    out = []
    for edit in ("stride3", "ck24", "kh8", "ntaps0", "tap_out", "x_unaligned", "y_geometry", "w_null", "cin12", "bias_unaligned", "y_null",
                 "y_batch", "res_geometry", "x_null"):
        d = base()
        if edit == "stride3": d.stride = 3
        elif edit == "ck24": d.ck = 24
        elif edit == "kh8": d.kh = 8
        elif edit == "ntaps0": d.ntaps = 0
        elif edit == "tap_out": d.tap_dy[4] = 3
        elif edit == "x_unaligned": d.x.p = PX + 8
        elif edit == "y_geometry": d.y.H = 271
        elif edit == "w_null": d.w = None
        elif edit == "cin12": d.x.C = 12
        elif edit == "bias_unaligned": d.bias = PB + 4
        elif edit == "y_null": d.y.p = None
        elif edit == "y_batch": d.y.N = 2
        elif edit == "res_geometry": d.res = fmap(L, PR1, 1, 272, 479, 64)
        elif edit == "x_null": d.x.p = None
        out.append(d)
    return out


# what a layer can ask for besides its window: (keyword arguments of desc, condition on cout)
VARIANTS = [(dict(act=1), None), (dict(act=2, slope=0.1), None), (dict(res="f16"), None), (dict(res="f16", res2="f16", act=1), None),
            (dict(res2="f16"), None), (dict(res="f32"), None), (dict(out="f32"), None), (dict(out="nchw"), None),
            (dict(out="shuffle", act=2, slope=0.01), lambda co: co % 128 == 0), (dict(out="shuffle", res="f16"), lambda co: co % 128 == 0),
            (dict(narrow=32), lambda co: co > 32), (dict(narrow=64, act=1), lambda co: co > 64), (dict(bias=False), None),
            (dict(round16=True, act=2, slope=0.1), None), (dict(x_f32=True, out="f32"), None), (dict(act=2, slope=1.5), None)]


def sweep(L, pick_ck):
    """-> (descriptors in the order of the golden file, indices of the ones every debug switch is replayed on: a fixed stride through
    the sweep plus the layers the switched kernels are there for -- 1x1 / 3x3 / space-to-depth / GDN calls on a large map)"""
    out, focus = [], []
    FOCUS_MAPS = [(272, 480), (15, 600)]

    def add(d, hot):
        if hot or len(out) % 97 == 0:
            focus.append(len(out))
        out.append(d)
    acts = [dict(), dict(act=1), dict(act=2, slope=0.1)]
    i = 0
    for cin in CINS:                                    # every layer shape on every map, activations in turn
        for cout in COUTS:
            for win in WINDOWS:
                for (H, W) in MAPS:
                    for N in (1, 4):
                        add(desc(L, pick_ck, cin, cout, win, H, W, N, **acts[i % 3]),
                            N == 1 and (H, W) in FOCUS_MAPS and cin in (8, 16, 64, 128) and win in WINDOWS[:2])
                        i += 1
    for kw, cond in VARIANTS:                           # epilogue / output forms on a thinner grid
        for cin in (8, 32, 64, 128, 192):
            for cout in (16, 32, 64, 128, 256):
                if cond is not None and not cond(cout):
                    continue
                for win in WINDOWS:
                    for (H, W) in SOME_MAPS:
                        add(desc(L, pick_ck, cin, cout, win, H, W, 1, **kw), (H, W) == FOCUS_MAPS[0] and cin in (8, 64, 128) and cout in (64, 128, 256) and win in WINDOWS[:2])
    for cin in (64, 128):                               # space-to-depth form of the stride-2 3x3 convs
        for cout in (64, 128, 192, 256):
            for (H, W) in MAPS:
                for N in (1, 4):
                    for kw in (dict(), dict(act=1), dict(act=2, slope=0.1, res="f16"), dict(res="f16", res2="f16"), dict(out="f32"), dict(narrow=32)):
                        add(s2d_desc(L, cin, cout, H, W, N, **kw), N == 1 and (H, W) == FOCUS_MAPS[0])
    for ch in (128, 64, 192):                           # GDN / inverse GDN norm pools
        for (H, W) in MAPS:
            for N in (1, 4):
                for gdn in (L.GDN_FWD, L.GDN_INV):
                    add(gdn_desc(L, ch, H, W, N, gdn), N == 1 and (H, W) in FOCUS_MAPS)
                add(gdn_desc(L, ch, H, W, N, L.GDN_FWD, res="f16"), N == 1 and (H, W) in FOCUS_MAPS)
                add(gdn_desc(L, ch, H, W, N, L.GDN_FWD, aux_is_x=False), False)
    for cin in (32, 64, 128):                           # temporal 1x1 conv + broadcast add (legal, then illegal forms)
        for (H, W) in MAPS:
            for N in (1, 4):
                add(bcast_desc(L, cin, H, W, N), False)
        add(bcast_desc(L, cin, 272, 480, 1, T=3), False)
        add(bcast_desc(L, cin, 272, 480, 1, act=1), False)
        add(bcast_desc(L, cin, 272, 480, 1, y_sp=64), False)
    for d in malformed(L, pick_ck):
        add(d, False)
    return out, focus


def observe(lib, d):
    """(kernel name or REJECTED, chan_sum rows) through tdvc_conv2d + tdvc_last_conv_kernel: works on any commit, and only on a
    machine without a GPU -- the launch that follows the dispatch must fail."""
    rc = lib.tdvc_conv2d(C.byref(d), None)
    assert rc != 0, "a launch over dummy pointers succeeded: this must never run next to a GPU"
    name = REJECTED if rc == -1 else lib.tdvc_last_conv_kernel().decode()         # -1 = TDVC_EINVAL; the name is stale then
    return name, lib.tdvc_conv_chan_sum_rows(C.byref(d))


def outcome(name):
    return "direct" if name.startswith("conv_mfma<") else name
