"""`ops.lf_tail` (tdvc_lf_tail): the temporal conv + broadcast add + LeakyReLU + conv3 + residual of LoopFilter's tail as one launch.
Every case is byte-equal (int16 words) to the two launches it replaces on the same inputs -- the out-of-place
`ops.conv(..., bcast_T=4, bcast_slope=0.1, res=...)` and the per-batch-item `ops.conv(s.as_slices(b, 4, 64), pc3, res=A...)` -- on dense
256-channel buffers and on windows of a ring of slots; one case has exact answers against float64 torch; one runs `LoopFilter` with the
switch on and off."""
import pytest
import torch

from util import randn, rnd16

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B          # "this memory was not written"
NAN16 = 0x7E00
RING = 9                   # slots of the ring windows: pixel stride 64 * 9


def _ops():
    from tdvc_amd import ops
    return ops


def _words(t):
    return t.view(torch.int16)


def _bits(fm):
    base = _words(fm.t).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


_LAYERS = {}


def _layers():
    """the two layers, packed once: temporal 1x1 192 -> 64 without bias, conv3 3x3 64 -> 64"""
    if not _LAYERS:
        ops = _ops()
        _LAYERS["t"] = ops.pack_conv(rnd16(randn(64, 192, 1, 1, seed=71) * 0.07), None, stride=1, pad=0)
        _LAYERS["3"] = ops.pack_conv(rnd16(randn(64, 64, 3, 3, seed=72) * 0.04), randn(64, seed=73) * 0.1, stride=1, pad=1)
    return _LAYERS["t"], _LAYERS["3"]


def _two_launches(S, A, pct, pc3, slope=0.1):
    """today's pair of launches on views S, A of 256 channels -> the int16 words of o (B, H, W, 256)"""
    ops = _ops()
    B, H, W = S.N, S.H, S.W
    s = ops.FM.empty(B, H, W, 256)
    ops.conv(S.ch(0, 192), pct, out=s.ch(0, 64), bcast_T=4, bcast_slope=slope, res=S.ch(0, 64))
    assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_mfma_v5(bcast)"
    o = ops.FM.empty(B, H, W, 256)
    for b in range(B):
        ops.conv(s.as_slices(b, 4, 64), pc3, out=o.as_slices(b, 4, 64), res=ops.FM(A.t, A.off + b * A.sn, 4, 64, 64))
        assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_row"
    return _bits(o)


def _poisoned_out(B, H, W):
    """o as a 256-channel window at channel 32 of a 320-channel buffer filled with NaN"""
    ops = _ops()
    buf = torch.empty((B, H, W, 320), dtype=torch.float16, device="cuda")
    _words(buf).fill_(NAN16)
    return buf, ops.FM(buf).ch(32, 256)


def _check_out(buf, o, want, what):
    got = _bits(o)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} words differ from the two launches"
    w = _words(buf)
    assert bool((w[..., :32] == NAN16).all()) and bool((w[..., 288:] == NAN16).all()), f"{what}: channels outside the four slices were written"


SHAPES = [(65, 131),       # ragged last strip, odd sizes, runs that cross strip ends
          (64, 128),       # exact strips
          (280, 30),       # one strip narrower than the strip width, many row segments per workgroup
          (16, 520)]       # the minimum height: prologue and drain overlap


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_dense_buffers(H, W, B):
    ops = _ops()
    pct, pc3 = _layers()
    S = ops.FM(rnd16(randn(B, H, W, 256, seed=80 + B)).half().cuda())
    A = ops.FM(rnd16(randn(B, H, W, 256, seed=90 + B)).half().cuda())
    assert ops.lf_tail_supported(S, A, ops.FM.empty(B, H, W, 256))
    want = _two_launches(S, A, pct, pc3)
    s0, a0 = _words(S.t).clone(), _words(A.t).clone()
    buf, o = _poisoned_out(B, H, W)
    ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
    _check_out(buf, o, want, f"{H}x{W} B={B}")
    assert torch.equal(_words(S.t), s0) and torch.equal(_words(A.t), a0), "S and A are only read"
    dense = ops.FM.empty(B, H, W, 256)                    # and into a dense 256-channel buffer, as _run_plain does
    _words(dense.t).fill_(NAN16)
    ops.lf_tail(S, A, pct, pc3, out=dense, slope=0.1)
    assert torch.equal(_bits(dense), want)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("p", [0, 3, 5])
def test_ring_windows(p, B):
    """S and A as LoopFilter's ring windows: slots p .. p + 3 of a ring of 9 (pixel stride 576); the other slots keep their pattern"""
    ops = _ops()
    pct, pc3 = _layers()
    H, W = 65, 131
    rings = []
    for seed in (101, 102):
        t = torch.empty((B, H, W, 64 * RING), dtype=torch.float16, device="cuda")
        _words(t).fill_(SENTINEL)
        t[..., 64 * p:64 * p + 256] = rnd16(randn(B, H, W, 256, seed=seed + p)).half().cuda()
        rings.append(t)
    S, A = ops.FM(rings[0]).ch(64 * p, 256), ops.FM(rings[1]).ch(64 * p, 256)
    assert S.sp == 64 * RING and ops.lf_tail_supported(S, A, ops.FM.empty(B, H, W, 256))
    want = _two_launches(S, A, pct, pc3)
    before = [_words(t).clone() for t in rings]
    buf, o = _poisoned_out(B, H, W)
    ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
    _check_out(buf, o, want, f"window {p} B={B}")
    for t, b4 in zip(rings, before):
        assert torch.equal(_words(t), b4), "S, A and the other ring slots are bit-unchanged"
        w = _words(t)
        assert bool((w[..., :64 * p] == SENTINEL).all()) and bool((w[..., 64 * p + 256:] == SENTINEL).all())


def test_signed_zeros():
    """exact zeros and negative zeros in S: T's accumulator starts at +0 and the zero bias is added in fp32, as conv_mfma_v5 does"""
    ops = _ops()
    pct, pc3 = _layers()
    H, W = 65, 131
    s = rnd16(randn(1, H, W, 256, seed=111)).half()
    kind = torch.randint(0, 4, (1, H, W, 256), generator=torch.Generator().manual_seed(112))
    s[kind == 0] = 0.0
    s[kind == 1] = -0.0
    s[:, 10:20, 40:90] = -0.0                              # whole pixels of negative zeros: T = 0 there
    s[:, 30:40, 40:90] = 0.0
    S = ops.FM(s.cuda())
    assert int((_words(S.t) == -32768).sum()) > 100000
    A = ops.FM(rnd16(randn(1, H, W, 256, seed=113)).half().cuda())
    want = _two_launches(S, A, pct, pc3)
    buf, o = _poisoned_out(1, H, W)
    ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
    _check_out(buf, o, want, "signed zeros")


def test_exact_small_integers():
    """small-integer weights and inputs, slope 0.5: every intermediate is exact in fp16 / fp32, so the float64 formulas are the answer"""
    ops = _ops()
    H, W = 65, 131
    g = torch.Generator().manual_seed(121)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    sparse = lambda *shape: ri(-1, 1, *shape) * (torch.rand(shape, generator=g) < 1 / 16).double()
    wt, w3, b3 = sparse(64, 192, 1, 1), sparse(64, 64, 3, 3), ri(-3, 3, 64)
    S, A = ri(-2, 2, 1, H, W, 256), ri(-4, 4, 1, H, W, 256)
    F = torch.nn.functional
    T = F.conv2d(S[..., :192].permute(0, 3, 1, 2), wt)                                           # (1, 64, H, W)
    want = torch.empty(1, H, W, 256, dtype=torch.float64)
    for j in range(4):
        sj = S[..., 64 * j:64 * j + 64].permute(0, 3, 1, 2) + T
        sj = torch.where(sj > 0, sj, sj * 0.5)
        assert float(sj.abs().max()) < 1024                                                      # multiples of 0.5 below 1024: exact in fp16
        c = F.conv2d(sj, w3, b3, padding=1)
        assert float(c.abs().max()) + 4 < 1024
        want[..., 64 * j:64 * j + 64] = (c + A[..., 64 * j:64 * j + 64].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert torch.equal(want, want.half().double()) and float(T.abs().max()) > 4
    pct = ops.pack_conv(wt.float(), None, stride=1, pad=0)
    pc3 = ops.pack_conv(w3.float(), b3.float(), stride=1, pad=1)
    Sf, Af = ops.FM(S.half().cuda()), ops.FM(A.half().cuda())
    o = ops.FM.empty(1, H, W, 256)
    _words(o.t).fill_(NAN16)
    ops.lf_tail(Sf, Af, pct, pc3, out=o, slope=0.5)
    got = o.t.double().cpu()
    assert torch.equal(got, want), f"max |error| {float((got - want).abs().max())}"
    assert torch.equal(_bits(o), _two_launches(Sf, Af, pct, pc3, slope=0.5))


def test_loopfilter_switch_bit_identical():
    """LoopFilter at 65x131 over a ring of calls, LOOPFILTER_TAIL on and off: prediction and residual byte-equal, reuse and plain path"""
    import tdvc_amd.model.modules as M
    from tdvc_amd.model.modules import LoopFilter
    from tdvc_amd.synth import fill_parameters, make_gop
    ops = _ops()
    H, W = 65, 131
    lf = LoopFilter()
    fill_parameters(lf)
    lf = lf.cuda().eval()
    pool = make_gop(78, 6, H, W)
    # [r-3, r-2, r-1]: a GOP, a restart.  An even number of calls: a call is an odd number of tdvc_conv2d launches, whose tile walk
    # alternates, and feat_fusion's channel sums follow the walk -- every pass over the calls starts in the same direction
    calls = [[0, 0, 0], [0, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [0, 0, 0], [0, 0, 5], [0, 5, 5]]
    xts = [rnd16(randn(1, H, W, 256, seed=300 + i) * 0.5).half().cuda() for i in range(len(calls))]
    cur = [rnd16(randn(1, H, W, 64, seed=320 + i) * 0.5).half().cuda() for i in range(len(calls))]
    launched = []
    real = ops.lf_tail

    def counting(*a, **kw):
        launched.append(1)
        return real(*a, **kw)

    def run_all():
        lf.__dict__.pop("_packed", None)
        outs = []
        for i, want in enumerate(calls):
            refs8 = ops.from_nchw(torch.stack([pool[0]] + [pool[k] for k in want]).cuda(), Cpad=8)
            out, out3 = ops.FM.empty(1, H, W, 64), ops.FM.empty(1, H, W, 64)
            lf.run(ops.FM(xts[i].clone()), refs8, out, then=(ops.FM(cur[i]), -1.0, out3))
            outs.append((_bits(out), _bits(out3)))
        return outs

    saved = (M.LOOPFILTER_TAIL, M.LOOPFILTER_REUSE)
    ops.lf_tail = counting
    try:
        res = {}
        for reuse in (True, False):
            for tail in (False, True):
                M.LOOPFILTER_TAIL, M.LOOPFILTER_REUSE = tail, reuse
                del launched[:]
                res[reuse, tail] = run_all()
                assert len(launched) == (len(calls) if tail else 0), "the fused tail runs exactly when the switch is on"
                assert (lf.reuse_state() is not None) == reuse
    finally:
        ops.lf_tail = real
        M.LOOPFILTER_TAIL, M.LOOPFILTER_REUSE = saved
        lf.__dict__.pop("_packed", None)
    for reuse in (True, False):
        for i, ((p0, r0), (p1, r1)) in enumerate(zip(res[reuse, False], res[reuse, True])):
            assert torch.equal(p0, p1), f"reuse={reuse} call {i + 1}: prediction differs with the fused tail"
            assert torch.equal(r0, r1), f"reuse={reuse} call {i + 1}: residual differs with the fused tail"
