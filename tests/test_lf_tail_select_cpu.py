"""CPU: `tdvc_lf_tail_supported` is host arithmetic on the descriptor: it takes the shapes and strides LoopFilter passes (dense 256-channel
buffers, windows of a ring of slots) and refuses everything the kernel does not compute, without a device."""
import ctypes as C

from tdvc_amd import _lib as L

PS, PA, PY, PW = 0x1000000000, 0x2000000000, 0x3000000000, 0x4000000000          # dummy 16-byte aligned addresses 64 GB apart, never dereferenced
SHAPES = [(65, 131), (64, 128), (280, 30), (16, 520), (1088, 1920)]


def _fmap(p, N, H, W, Cc=256, sp=None, dtype=L.F16):
    sp = Cc if sp is None else sp
    return L.FMapDesc(p, N, H, W, Cc, H * W * sp, sp, dtype)


def _desc(N=1, H=65, W=131, sp=256, win=0, **kw):
    d = L.LfTailDesc()
    d.s, d.a, d.y = _fmap(PS + 2 * 64 * win, N, H, W, sp=sp), _fmap(PA + 2 * 64 * win, N, H, W, sp=sp), _fmap(PY, N, H, W)
    d.nslices, d.slice_stride = 4, 64
    d.wt, d.bias_t, d.w3, d.bias3 = PW, None, PW + 4096, PW + 8192
    d.slope = 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ok(d):
    return L.lib().tdvc_lf_tail_supported(C.byref(d))


def test_layout_and_abi():
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 14
    assert C.sizeof(L.LfTailDesc) == 168 and L.LfTailDesc.slope.offset == 160 and L.LfTailDesc.nslices.offset == 3 * C.sizeof(L.FMapDesc)


def test_accepts_the_shapes_and_strides_in_use():
    for H, W in SHAPES:
        for N in (1, 2):
            assert _ok(_desc(N, H, W)) == 1, (H, W, N)                       # dense (B, H, W, 256)
            for p in (0, 3, 5):
                assert _ok(_desc(N, H, W, sp=64 * 9, win=p)) == 1, (H, W, N, p)      # ring windows: pixel stride 64 * 9, window start p


def test_rejects_what_the_kernel_does_not_compute():
    lib = L.lib()
    assert lib.tdvc_lf_tail_supported(None) == 0
    f32 = lambda p: _fmap(p, 1, 65, 131, dtype=L.F32)
    bad = {
        "fp32 s": _desc(s=f32(PS)), "fp32 a": _desc(a=f32(PA)), "fp32 y": _desc(y=f32(PY)),
        "three slices": _desc(nslices=3), "slice offset 128": _desc(slice_stride=128), "slice offset 32": _desc(slice_stride=32),
        "192 channels": _desc(s=_fmap(PS, 1, 65, 131, Cc=192, sp=256)), "320 channels": _desc(y=_fmap(PY, 1, 65, 131, Cc=320)),
        "128-channel a": _desc(a=_fmap(PA, 1, 65, 131, Cc=128, sp=256)),
        "misaligned s": _desc(s=_fmap(PS + 8, 1, 65, 131)), "misaligned a": _desc(a=_fmap(PA + 2, 1, 65, 131)),
        "misaligned y": _desc(y=_fmap(PY + 4, 1, 65, 131)), "misaligned weights": _desc(wt=PW + 8), "misaligned conv3": _desc(w3=PW + 4100),
        "odd pixel stride": _desc(s=_fmap(PS, 1, 65, 131, sp=260)),
        "temporal bias": _desc(bias_t=PW + 16384),
        "no weights": _desc(wt=None), "no conv3": _desc(w3=None), "no conv3 bias": _desc(bias3=None),
        "under the floor": _desc(H=64, W=127), "15 rows": _desc(H=15, W=600),
        "geometry": _desc(a=_fmap(PA, 1, 65, 132)), "batch": _desc(y=_fmap(PY, 2, 65, 131)),
        "in place": _desc(y=_fmap(PS, 1, 65, 131)), "y inside a": _desc(y=_fmap(PA + 4096, 1, 65, 131)),
    }
    for what, d in bad.items():
        assert _ok(d) == 0, what
        assert lib.tdvc_lf_tail(C.byref(d), None) == -1, what        # TDVC_EINVAL, before anything touches a device
        assert b"tdvc_lf_tail" in lib.tdvc_last_error(), what
    assert _ok(_desc()) == 1
