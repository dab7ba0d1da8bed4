"""Device-predicated reuse of the I-frame features in FeatureFix: `tdvc_frame_changed` (exact compare + conditional refresh),
the launch predicate of conv_c8 / conv_pair / conv_row / avgpool_k (flag 0: outputs untouched, flag 1: byte-equal to the plain
launch), and the reuse in `FeatureFix.run` / `VideoCompressor` (byte-equal with the switch on and off)."""
import pytest
import torch

from util import randn, rnd16

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B          # int16 pattern no kernel output is checked against: "this memory was not written"


def _ops():
    from tdvc_amd import ops
    return ops


def _bits(fm):
    """the int16 words of an FM view, (N, H, W, C), as a copy"""
    base = fm.t.view(torch.int16 if fm.t.dtype == torch.float16 else torch.int32).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


def _rand16(*shape, seed):
    """fp16 tensor of random BIT patterns (NaNs, infinities and denormals included)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).cuda().view(torch.float16)


def _predicated():
    return _ops().L.lib().tdvc_last_launch_predicated()


# ------------------------------------------------------------------------------------------- tdvc_frame_changed
def _frame_pair(kind):
    """-> (cur FM, cache FM, cache's whole buffer)"""
    ops = _ops()
    H, W = 96, 128
    if kind == "n1":
        cur, buf = ops.FM(_rand16(1, H, W, 8, seed=1)), torch.empty((1, H, W, 8), dtype=torch.float16, device="cuda")
        return cur, ops.FM(buf), buf
    if kind == "n2":
        cur, buf = ops.FM(_rand16(2, H, W, 8, seed=2)), torch.empty((2, H, W, 8), dtype=torch.float16, device="cuda")
        return cur, ops.FM(buf), buf
    # the model's view: items 0 and 4 of a stack of 8 frames (pnet.py:_ref_views); the cache a channel slice of a wider buffer
    stack = ops.FM(_rand16(8, H, W, 8, seed=3))
    cur = ops.FM(stack.t, 0, 2, 8, 4 * stack.sn)
    buf = torch.empty((2, H, W, 24), dtype=torch.float16, device="cuda")
    return cur, ops.FM(buf).ch(8, 8), buf


def _set_cache(cur, cache, buf):
    """cache = cur bit for bit, the rest of its buffer = SENTINEL"""
    buf.view(torch.int16).fill_(SENTINEL)
    base = buf.view(torch.int16).reshape(-1)
    torch.as_strided(base, (cache.N, cache.H, cache.W, cache.C), (cache.sn, cache.W * cache.sp, cache.sp, 1), cache.off).copy_(_bits(cur))


@pytest.mark.parametrize("kind", ["n1", "n2", "strided"])
def test_frame_changed(kind):
    ops = _ops()
    cur, cache, buf = _frame_pair(kind)
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    _set_cache(cur, cache, buf)
    before = buf.view(torch.int16).clone()
    ops.frame_changed(cur, cache, flag)
    assert int(flag.item()) == 0
    assert torch.equal(buf.view(torch.int16), before), "equal frames: the cache's bytes must stay as they were"

    N, H, W = cur.N, cur.H, cur.W
    cb = torch.as_strided(buf.view(torch.int16).reshape(-1), (N, H, W, 8), (cache.sn, W * cache.sp, cache.sp, 1), cache.off)
    want = _bits(cur)
    for what, (n, y, x, c) in (("first word", (0, 0, 0, 0)), ("last word", (N - 1, H - 1, W - 1, 7))):
        _set_cache(cur, cache, buf)
        cb[n, y, x, c] ^= 1                                            # one bit of one word
        ops.frame_changed(cur, cache, flag)
        assert int(flag.item()) == 1, what
        assert torch.equal(_bits(cache), want), what
    # two NaNs with different payloads compare unequal (bits, not values)
    _set_cache(cur, cache, buf)
    curw = torch.as_strided(cur.t.view(torch.int16).reshape(-1), (N, H, W, 8), (cur.sn, W * cur.sp, cur.sp, 1), cur.off)
    curw[N - 1, 5, 7, 3] = 0x7E00
    cb[N - 1, 5, 7, 3] = 0x7E01
    ops.frame_changed(cur, cache, flag)
    assert int(flag.item()) == 1
    assert torch.equal(_bits(cache), _bits(cur))
    # and the cache's surroundings were never written
    if kind == "strided":
        whole = buf.view(torch.int16)
        assert bool((whole[..., :8] == SENTINEL).all()) and bool((whole[..., 16:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------- the predicated kernels
def _conv_case(name):
    """-> (launch(out), make_out(), kernel name the dispatch must report)"""
    ops = _ops()
    if name == "conv_c8":
        x = ops.from_nchw(rnd16(randn(1, 3, 96, 128, seed=11)).cuda(), Cpad=8)
        pc = ops.pack_conv(randn(64, 3, 3, 3, seed=12) * 0.2, randn(64, seed=13) * 0.1, stride=1, pad=1)
        return (lambda out: ops.conv(x, pc, out=out, act=ops.ACT_LRELU, slope=0.01)), (lambda: ops.FM.empty(1, 96, 128, 64)), "conv_c8"
    cin, cout, stride, H, W, res = {"conv_row_c64": (64, 64, 1, 96, 128, True), "conv_row_c128": (128, 128, 1, 96, 128, False),
                                    "conv_row_c128w": (128, 64, 1, 96, 128, False), "conv_row_s2d": (64, 128, 2, 192, 256, False)}[name]
    x = ops.from_nchw(rnd16(randn(1, cin, H, W, seed=21)).cuda())
    pc = ops.pack_conv(randn(cout, cin, 3, 3, seed=22) * 0.03, randn(cout, seed=23) * 0.1, stride=stride, pad=1)
    r = ops.from_nchw(rnd16(randn(1, cout, H // stride, W // stride, seed=24)).cuda()) if res else None
    return ((lambda out: ops.conv(x, pc, out=out, act=ops.ACT_RELU, res=r)), (lambda: ops.FM.empty(1, H // stride, W // stride, cout)),
            "conv_row(s2d)" if stride == 2 else "conv_row")


def _check_predicated(launch, make_out, kernels, after_launch=None):
    """sentinel survives under flag 0, flag 1 equals the plain launch, both report `predicated`"""
    ops = _ops()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(pred):
        out = make_out()
        t = out.t if isinstance(out, ops.FM) else out
        t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).fill_(SENTINEL)
        if pred is None:
            launch(out)
            log = None
        else:
            flag.fill_(pred)
            with ops.predicate(flag) as log:
                launch(out)
                assert _predicated() == 1
            log = list(log)
        if after_launch is not None:
            after_launch()
        return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).clone(), log

    ref, _ = run(None)
    assert not bool((ref == SENTINEL).all())
    skipped, log0 = run(0)
    assert bool((skipped == SENTINEL).all()), "flag 0: the output must not be written"
    full, log1 = run(1)
    assert torch.equal(full, ref), "flag 1: byte-equal to the launch without a predicate"
    assert log0 == [True] * kernels and log1 == [True] * kernels


@pytest.mark.parametrize("name", ["conv_c8", "conv_row_c64", "conv_row_c128", "conv_row_c128w", "conv_row_s2d"])
def test_predicated_conv(name):
    ops = _ops()
    launch, make_out, kernel = _conv_case(name)

    def named():
        assert ops.L.lib().tdvc_last_conv_kernel().decode() == kernel
    _check_predicated(launch, make_out, 1, after_launch=named)


@pytest.mark.parametrize("res_block", [True, False], ids=["resblock", "lrelu"])
def test_predicated_conv_pair(res_block):
    ops = _ops()
    x = ops.from_nchw(rnd16(randn(1, 64, 96, 128, seed=31)).cuda())
    assert ops.conv_pair_supported(x)
    pp = ops.pack_conv_pair((randn(64, 64, 3, 3, seed=32) * 0.05).cuda(), (randn(64, seed=33) * 0.1).cuda(),
                            (randn(64, 64, 3, 3, seed=34) * 0.05).cuda(), (randn(64, seed=35) * 0.1).cuda())
    kw = dict(act1=ops.ACT_RELU, act2=ops.ACT_NONE, add_input=True) if res_block else \
        dict(act1=ops.ACT_LRELU, slope1=0.1, act2=ops.ACT_LRELU, slope2=0.1, add_input=False)
    _check_predicated(lambda out: ops.conv_pair(x, pp, out=out, **kw), lambda: ops.FM.empty(1, 96, 128, 64), 1)


def test_predicated_avgpool_k():
    ops = _ops()
    x = ops.from_nchw(rnd16(randn(2, 64, 96, 128, seed=41)).cuda())
    _check_predicated(lambda out: ops.avgpool_k(x, 12, out=out), lambda: torch.empty((2, 8, 10, 64), dtype=torch.float32, device="cuda"), 2)


def test_other_kernels_run_in_full_under_a_predicate():
    """a 1x1 conv (conv_mfma_v5) and an elementwise pass are outside the predicated set: flag 0 does not stop them, the query says 0"""
    ops = _ops()
    x = ops.from_nchw(rnd16(randn(1, 64, 96, 128, seed=51)).cuda())
    pc = ops.pack_conv(randn(64, 64, 1, 1, seed=52) * 0.1, randn(64, seed=53) * 0.1)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref = _bits(ops.conv(x, pc))
    assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_mfma_v5"
    ref2 = _bits(ops.scale_act_res(x, ops.FM.empty(1, 96, 128, 64), act=ops.ACT_RELU))
    with ops.predicate(flag) as log:
        got = ops.conv(x, pc)
        assert _predicated() == 0
        got2 = ops.scale_act_res(x, ops.FM.empty(1, 96, 128, 64), act=ops.ACT_RELU)
        assert _predicated() == 0
    assert log == [False]
    assert torch.equal(_bits(got), ref) and torch.equal(_bits(got2), ref2)
    # the predicate ends with the block
    launch, make_out, _ = _conv_case("conv_c8")
    launch(make_out())
    assert _predicated() == 0


# ------------------------------------------------------------------------------------------- FeatureFix / VideoCompressor
def _switch(on):
    import tdvc_amd.model.modules as M
    M.FEATUREFIX_REUSE = on


@pytest.fixture()
def reuse_switch():
    yield _switch
    _switch(True)


def _frame8(seed, H=128, W=128):
    """a stack of 4 reference frames as the model converts it, and the I-frame view of it"""
    from tdvc_amd.model.pnet import _ref_views
    from tdvc_amd.synth import make_gop
    ops = _ops()
    refs8 = ops.from_nchw(make_gop(seed, 4, H, W).cuda(), Cpad=8)
    return refs8, _ref_views(refs8, 1)[1]


def test_featurefix_reuse_bit_identical(reuse_switch):
    from tdvc_amd.model.modules import FeatureFix
    from tdvc_amd.synth import fill_parameters
    ops = _ops()
    ff = FeatureFix()
    fill_parameters(ff)
    ff = ff.cuda().eval()
    xs = [ops.from_nchw(rnd16(randn(1, 64, 128, 128, seed=60 + i) * 0.5).cuda()) for i in range(4)]
    (_, fa), (_, fa2), (_, fb) = _frame8(70), _frame8(70), _frame8(71)      # fa2: the same I-frame in OTHER memory
    frames = [fa, fa2, fb, fb]
    assert torch.equal(_bits(fa), _bits(fa2)) and not torch.equal(_bits(fa), _bits(fb))
    out, logs = {}, []
    for on in (False, True):
        reuse_switch(on)
        ff.__dict__.pop("_packed", None)
        res = []
        for x, fr in zip(xs, frames):
            res.append(ff.run(x, fr, training=False).clone())
            if on:
                logs.append(list(ff.reuse_state().log))
        out[on] = res
        if not on:
            assert ff.reuse_state() is None
    for i in range(4):
        assert torch.equal(out[True][i].view(torch.int32), out[False][i].view(torch.int32)), f"call {i + 1}"
    for i in (1, 3):
        assert logs[i] == [True] * 6, f"call {i + 1}: all six launches (conv_c8, 2 x conv_pair, conv_row, 2 x avgpool_k) predicated"
    assert int(ff.reuse_state().flag.item()) == 0                           # call 4 was a hit
    # a forward in training mode keeps no state and leaves an existing one alone
    ff.__dict__.pop("_packed", None)
    ff.run(xs[0], fa, training=True)
    assert ff.reuse_state() is None


def _code_gop(m, g, n=3):
    from tdvc_amd.synth import ref_list
    refs, outs = [g[0:1]], []
    with torch.no_grad():
        for t in range(1, n + 1):
            recon, bpp_res, bpp_mv = m(g[t:t + 1], ref_list(refs), True)
            refs.append(recon)
            outs.append((recon.clone(), bpp_res.clone(), bpp_mv.clone()))
    return outs


def _same(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for fa, fb in zip(a, b) for u, v in zip(fa, fb))


def test_video_compressor_reuse_bit_identical(reuse_switch):
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.synth import fill_parameters, make_gop

    def model(scale=1.0):
        m = VideoCompressor()
        fill_parameters(m)
        if scale != 1.0:
            with torch.no_grad():
                for p in m.loopfilter.FeatureExtract_ref.parameters():
                    p.mul_(scale)
        return m

    g = make_gop(4321, 4, 128, 128).cuda()
    m = model().cuda().eval()
    reuse_switch(False)
    off = _code_gop(m, g)
    assert m.loopfilter.reuse_state() is None
    reuse_switch(True)
    m.clear_packed()
    on = _code_gop(m, g)
    st = m.loopfilter.reuse_state()
    assert st is not None and st.usable and st.log == [True] * 6 and int(st.flag.item()) == 0
    assert _same(on, off), "recon / bpp_res / bpp_mv must be byte-equal with the reuse on and off"

    # other weights through load_state_dict: the cached maps of the old weights must be gone
    other = model(0.5)
    m.load_state_dict(other.state_dict())
    assert m.loopfilter.reuse_state() is None
    got = _code_gop(m, g)
    fresh = _code_gop(other.cuda().eval(), g)
    assert _same(got, fresh) and not _same(got, on)

    # a .train() forward builds no cache
    m.clear_packed()
    m.train()
    from tdvc_amd.synth import ref_list
    m(g[1:2], ref_list([g[0:1]]), True)
    assert m.loopfilter.reuse_state() is None
    m.eval()
