"""Reuse of LoopFilter's per-reference-frame maps across P-frames: the per-image launch predicate of conv_c8 / conv_pair
(`tdvc_set_predicate_images`: skipped images untouched, computed images byte-equal to the plain launches), `tdvc_frames_changed`
(exact per-image compare + conditional refresh), the out-of-place form of the fused temporal conv, and the reuse in `LoopFilter.run` /
`VideoCompressor` (byte-equal with the switch on and off, flags as the slot model predicts)."""
import pytest
import torch

from util import randn, rnd16

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B          # int16 pattern no kernel output is checked against: "this memory was not written"
PATTERNS3 = ["000", "001", "010", "100", "101", "111"]            # character i: flag of image i
PATTERNS4 = ["0000", "0001", "0010", "0100", "0101", "0111", "1000", "1011", "1111"]


def _ops():
    from tdvc_amd import ops
    return ops


def _words(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _bits(fm):
    """the int16 words of an FM view, (N, H, W, C), as a copy"""
    base = _words(fm.t).reshape(-1)
    return torch.as_strided(base, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


def _rand16(*shape, seed):
    """fp16 tensor of random BIT patterns (NaNs, infinities and denormals included)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).cuda().view(torch.float16)


def _predicated():
    return _ops().L.lib().tdvc_last_launch_predicated()


def _flags(pattern):
    return torch.tensor([int(c) for c in pattern], dtype=torch.int32, device="cuda")


def _check_images(launch, make_out, N, patterns):
    """launch(x_first_image, n_images, out) runs the op on images [first, first + n) of the input into `out` (an FM of n images).
    Per pattern: skipped images keep the sentinel, computed ones equal the one-image launch and the unpredicated N-image launch."""
    ops = _ops()

    def fresh(n):
        out = make_out(n)
        _words(out.t).fill_(SENTINEL)
        return out

    full = fresh(N)
    launch(0, N, full)
    full = _bits(full)
    assert not bool((full == SENTINEL).all())
    for i in range(N):
        one = fresh(1)
        launch(i, 1, one)
        assert torch.equal(_bits(one)[0], full[i]), f"image {i}: one-image launch != its slice of the {N}-image launch"
    for pat in patterns:
        out = fresh(N)
        with ops.predicate_images(_flags(pat)) as log:
            launch(0, N, out)
            assert _predicated() == 1, pat
        assert log == [True], pat
        got = _bits(out)
        for i, c in enumerate(pat):
            if c == "1":
                assert torch.equal(got[i], full[i]), f"flags {pat}: image {i} differs from the unpredicated launch"
            else:
                assert bool((got[i] == SENTINEL).all()), f"flags {pat}: skipped image {i} was written"
    assert _predicated() == 1
    launch(0, N, fresh(N))                     # the flags end with the block
    assert _predicated() == 0


# ------------------------------------------------------------------------------------------- per-image predicate
def test_predicate_images_conv_c8():
    ops = _ops()
    x = ops.from_nchw(rnd16(randn(3, 3, 96, 128, seed=11)).cuda(), Cpad=8)
    pc = ops.pack_conv(randn(64, 3, 3, 3, seed=12) * 0.2, randn(64, seed=13) * 0.1, stride=1, pad=1)

    def launch(first, n, out):
        ops.conv(x.batch(first, n), pc, out=out, act=ops.ACT_LRELU, slope=0.1)
        assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_c8"
    _check_images(launch, lambda n: ops.FM.empty(n, 96, 128, 64), 3, PATTERNS3)


def _pair_weights():
    ops = _ops()
    return ops.pack_conv_pair((randn(64, 64, 3, 3, seed=32) * 0.05).cuda(), (randn(64, seed=33) * 0.1).cuda(),
                              (randn(64, 64, 3, 3, seed=34) * 0.05).cuda(), (randn(64, seed=35) * 0.1).cuda())


def _strip_columns(W):
    """the launcher's rule (tdvc_conv_pair): 62-column strips unless the 30-column ones waste clearly fewer columns"""
    waste = lambda pw: ((W + pw - 1) // pw) * (pw + 2) / W
    return 62 if waste(62) <= 1.12 * waste(30) else 30


PAIR_FORMS = {"slope": dict(act1=0, act2=2, slope2=0.1, add_input=False),           # conv02 + conv1 of LoopFilter (ACT_NONE, ACT_LRELU)
              "resblock": dict(act1=1, act2=0, add_input=True)}                      # ACT_RELU, ACT_NONE, + x


@pytest.mark.parametrize("W,strip", [(128, 30), (248, 62)])
@pytest.mark.parametrize("form", ["slope", "resblock"])
@pytest.mark.parametrize("N", [3, 4])
def test_predicate_images_conv_pair(N, form, W, strip):
    ops = _ops()
    assert _strip_columns(W) == strip
    x = ops.from_nchw(rnd16(randn(N, 64, 96, W, seed=31)).cuda())
    assert ops.conv_pair_supported(x)
    pp = _pair_weights()
    _check_images(lambda first, n, out: ops.conv_pair(x.batch(first, n), pp, out=out, **PAIR_FORMS[form]),
                  lambda n: ops.FM.empty(n, 96, W, 64), N, PATTERNS3 if N == 3 else PATTERNS4)


def _pair_jobs(n, H, strips):
    """the launcher's row-segment search (tdvc_conv_pair) for n images -> jobs"""
    best, best_eff, sg = 1, 0.0, 1
    while sg <= 64 and (H + sg - 1) // sg >= 16:
        sr = (H + sg - 1) // sg
        jobs = n * strips * ((H + sr - 1) // sr)
        eff = jobs / (((jobs + 255) // 256) * 256) * sr / (sr + 5.0)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, sg
        sg += 1
    sr = (H + best - 1) // best
    return n * strips * ((H + sr - 1) // sr)


def test_predicate_images_conv_pair_more_jobs_than_workgroups():
    """280x624, N = 4: the smallest map at which the compacted walk takes both of its other paths, as at 1080p -- with four active images
    484 jobs go round 256 workgroups (several jobs per workgroup, XCD-aware ranges), with one to three 198 / 242 / 231 jobs leave tail
    workgroups of the same 256-workgroup grid without a job"""
    ops = _ops()
    H, W, N = 280, 624, 4
    assert _strip_columns(W) == 62
    strips = (W + 61) // 62
    assert [_pair_jobs(a, H, strips) for a in (1, 2, 3, 4)] == [198, 242, 231, 484]
    x = ops.from_nchw(rnd16(randn(N, 64, H, W, seed=36)).cuda())
    pp = _pair_weights()
    _check_images(lambda first, n, out: ops.conv_pair(x.batch(first, n), pp, out=out, **PAIR_FORMS["slope"]),
                  lambda n: ops.FM.empty(n, H, W, 64), N, PATTERNS4)


def test_predicate_images_conv_pair_slot_windows():
    """x and y as LoopFilter's slot windows: four 64-channel images at channel offset 64 of 320-channel buffers (image stride 64)"""
    ops = _ops()
    H, W = 96, 128
    xbuf = ops.FM(rnd16(randn(1, H, W, 320, seed=41)).half().cuda())
    win = lambda buf, j0, n: ops.FM(buf.t, 64 * (1 + j0), n, 64, 64)
    pp = _pair_weights()
    dense = ops.FM.empty(4, H, W, 64)
    dense.t.copy_(_bits(win(xbuf, 0, 4)).view(torch.float16))
    ref = _bits(ops.conv_pair(dense, pp, **PAIR_FORMS["slope"]))
    for pat in PATTERNS4:
        ybuf = ops.FM.empty(1, H, W, 320)
        _words(ybuf.t).fill_(SENTINEL)
        with ops.predicate_images(_flags(pat)) as log:
            ops.conv_pair(win(xbuf, 0, 4), pp, out=win(ybuf, 0, 4), **PAIR_FORMS["slope"])
        assert log == [True], pat
        got = _bits(win(ybuf, 0, 4))
        for i, c in enumerate(pat):
            if c == "1":
                assert torch.equal(got[i], ref[i]), f"flags {pat}: image {i}"
            else:
                assert bool((got[i] == SENTINEL).all()), f"flags {pat}: skipped image {i} was written"
        assert bool((_words(ybuf.t)[..., :64] == SENTINEL).all()), f"flags {pat}: channels in front of the window were written"


def test_launches_that_cannot_honour_image_flags_run_in_full():
    ops = _ops()
    pp = _pair_weights()
    zeros3 = torch.zeros(3, dtype=torch.int32, device="cuda")
    # two images under three flags
    x2 = ops.from_nchw(rnd16(randn(2, 64, 96, 128, seed=51)).cuda())
    ref = _bits(ops.conv_pair(x2, pp, **PAIR_FORMS["slope"]))
    with ops.predicate_images(zeros3) as log:
        got = ops.conv_pair(x2, pp, **PAIR_FORMS["slope"])
        assert _predicated() == 0
    assert log == [False] and torch.equal(_bits(got), ref)
    # conv_row is outside the per-image set
    x3 = ops.from_nchw(rnd16(randn(3, 64, 96, 128, seed=52)).cuda())
    r3 = ops.from_nchw(rnd16(randn(3, 64, 96, 128, seed=53)).cuda())
    pc = ops.pack_conv(randn(64, 64, 3, 3, seed=54) * 0.03, randn(64, seed=55) * 0.1, stride=1, pad=1)
    ref = _bits(ops.conv(x3, pc, act=ops.ACT_RELU, res=r3))
    assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_row"
    with ops.predicate_images(zeros3) as log:
        got = ops.conv(x3, pc, act=ops.ACT_RELU, res=r3)
        assert _predicated() == 0
    assert log == [False] and torch.equal(_bits(got), ref)
    # the two forms exclude each other
    lib = ops.L.lib()
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    with ops.predicate(one):
        assert lib.tdvc_set_predicate_images(zeros3.data_ptr(), 3) != 0
    with ops.predicate_images(zeros3):
        assert lib.tdvc_set_predicate(one.data_ptr()) != 0
    assert lib.tdvc_set_predicate_images(zeros3.data_ptr(), 5) != 0


# ------------------------------------------------------------------------------------------- tdvc_frames_changed
def _frames(kind):
    """-> (cur FM of 3 images, cache FM, the cache's whole buffer)"""
    ops = _ops()
    H, W = 96, 128
    if kind == "contiguous":
        buf = torch.empty((3, H, W, 8), dtype=torch.float16, device="cuda")
        return ops.FM(_rand16(3, H, W, 8, seed=1)), ops.FM(buf), buf
    # the model's views: items 1..3 of a stack of 4 frames; the cache three slots in the middle of a ring of 5, in a wider buffer
    stack = ops.FM(_rand16(4, H, W, 8, seed=2))
    buf = torch.empty((5, H, W, 24), dtype=torch.float16, device="cuda")
    return stack.batch(1, 3), ops.FM(buf).ch(8, 8).batch(1, 3), buf


@pytest.mark.parametrize("kind", ["contiguous", "strided"])
def test_frames_changed(kind):
    ops = _ops()
    cur, cache, buf = _frames(kind)
    N, H, W = 3, cur.H, cur.W
    whole = _words(buf)
    cb = torch.as_strided(whole.reshape(-1), (N, H, W, 8), (cache.sn, W * cache.sp, cache.sp, 1), cache.off)
    want = _bits(cur)

    def set_cache():
        whole.fill_(SENTINEL)
        cb.copy_(want)
    flags = torch.full((4,), 7, dtype=torch.int32, device="cuda")

    set_cache()
    before = whole.clone()
    ops.frames_changed(cur, cache, flags[:3])
    assert flags.tolist() == [0, 0, 0, 7], "equal frames; the int behind the three flags is not written"
    assert torch.equal(whole, before), "equal frames: the cache's bytes must stay as they were"

    for what, (y, x, c) in (("first word", (0, 0, 0)), ("last word", (H - 1, W - 1, 7))):
        set_cache()
        cb[1, y, x, c] ^= 1                                            # one bit of one word of image 1
        ops.frames_changed(cur, cache, flags[:3])
        assert flags.tolist() == [0, 1, 0, 7], what
        assert torch.equal(_bits(cache), want), what
    set_cache()
    ops.frames_changed(cur, cache, flags[:3], force_mask=0b010)
    assert flags.tolist() == [0, 1, 0, 7], "the force mask sets a flag on equal frames"
    assert torch.equal(_bits(cache), want)
    set_cache()
    ops.frames_changed(cur, cache, flags[:3], force_mask=0b101)
    assert flags.tolist() == [1, 0, 1, 7]
    # two NaNs with different payloads compare unequal (bits, not values)
    set_cache()
    curw = torch.as_strided(_words(cur.t).reshape(-1), (N, H, W, 8), (cur.sn, W * cur.sp, cur.sp, 1), cur.off)
    curw[2, 5, 7, 3] = 0x7E00
    cb[2, 5, 7, 3] = 0x7E01
    ops.frames_changed(cur, cache, flags[:3])
    assert flags.tolist() == [0, 0, 1, 7]
    assert torch.equal(_bits(cache), _bits(cur))
    if kind == "strided":                                              # the cache's surroundings were never written
        assert bool((whole[..., :8] == SENTINEL).all()) and bool((whole[..., 16:] == SENTINEL).all())
        assert bool((whole[0] == SENTINEL).all()) and bool((whole[4] == SENTINEL).all())


# ------------------------------------------------------------------------------------------- out-of-place temporal conv
def test_bcast_out_of_place():
    ops = _ops()
    H, W = 128, 128
    src = ops.FM(rnd16(randn(1, H, W, 320, seed=61)).half().cuda())             # slices at channels 64 .. 319
    pc = ops.pack_conv(rnd16(randn(64, 192, 1, 1, seed=62) * 0.07), None, stride=1, pad=0)
    before = _words(src.t).clone()
    inplace = ops.FM.empty(1, H, W, 256)
    inplace.t.copy_(src.t[..., 64:])
    ops.conv(inplace.ch(0, 192), pc, out=inplace.ch(0, 64), bcast_T=4, bcast_slope=0.1)
    y = ops.FM.empty(1, H, W, 256)
    _words(y.t).fill_(SENTINEL)
    ops.conv(src.ch(64, 192), pc, out=y.ch(0, 64), bcast_T=4, bcast_slope=0.1, res=src.ch(64, 64))
    assert ops.L.lib().tdvc_last_conv_kernel().decode() == "conv_mfma_v5(bcast)"
    assert src.sp == 320 and y.sp == 256
    assert torch.equal(_bits(y), _bits(inplace))
    assert torch.equal(_words(src.t), before), "the source must stay as it was"


# ------------------------------------------------------------------------------------------- LoopFilter / VideoCompressor
@pytest.fixture()
def switches():
    import tdvc_amd.model.modules as M
    ring = M.LOOPFILTER_RING

    def set_(reuse=True, slots=ring):
        M.LOOPFILTER_REUSE, M.LOOPFILTER_RING = reuse, slots
    yield set_
    M.LOOPFILTER_REUSE, M.LOOPFILTER_RING = True, ring


def _ref_slices(refs):
    """[r-3, r-2, r-1] by synth.ref_list"""
    if len(refs) == 1:
        return [refs[0]] * 3
    if len(refs) == 2:
        return [refs[-2], refs[-1], refs[-1]]
    return refs[-3:]


def _expected_flags(slots, calls):
    """the slot model, independent of tdvc_amd/model/ring.py: per call the flags [f0, f1, f2] (1 = computed)"""
    holds, p, out = [None] * slots, 0, []
    for i, want in enumerate(calls):
        if i:
            p += 1
            if p > slots - 4:
                p, holds = 0, [None] * slots
        out.append([0 if holds[p + j] == want[j] else 1 for j in range(3)])
        holds[p:p + 3] = want
        holds[p + 3] = None
    return out


def test_loopfilter_reuse_bit_identical(switches):
    from tdvc_amd.model.modules import LoopFilter
    from tdvc_amd.synth import fill_parameters, make_gop
    ops = _ops()
    H = W = 128
    lf = LoopFilter()
    fill_parameters(lf)
    lf = lf.cuda().eval()
    pool = make_gop(77, 12, H, W)                          # frame ids -> frames
    ids = {"I0": 0, "x0.1": 1, "x0.2": 2, "x0.3": 3, "x0.4": 4, "I1": 5, "x1.1": 6, "x1.2": 7, "S": 8, "u1": 9, "u2": 10, "u3": 11}
    calls = []
    for g, nframes in ((0, 6), (1, 4)):                    # eight calls: five P-frames, a GOP restart, three more
        refs = [f"I{g}"]
        for t in range(1, nframes):
            calls.append(_ref_slices(refs))
            refs.append(f"x{g}.{t}")
    assert len(calls) == 8
    calls += [["S", "S", "S"]] * 3                        # a static sequence
    calls += [["u1", "u2", "u3"]]                          # an unrelated stack
    want_flags = _expected_flags(5, calls)
    assert want_flags[1] == [0, 1, 1] and want_flags[3] == [0, 0, 1] and want_flags[9] == [0, 0, 1]      # hits where the list slid / stood still
    xts = [rnd16(randn(1, H, W, 256, seed=200 + i) * 0.5).half().cuda() for i in range(len(calls))]

    def run_all(check_flags):
        outs = []
        for i, want in enumerate(calls):
            stack = torch.stack([pool[ids["I0"]]] + [pool[ids[k]] for k in want]).cuda()          # [I, r-3, r-2, r-1]
            refs8 = ops.from_nchw(stack, Cpad=8)
            out = ops.FM.empty(1, H, W, 64)
            lf.run(ops.FM(xts[i].clone()), refs8, out)
            outs.append(_bits(out))
            if check_flags:
                st = lf.reuse_state()
                assert st is not None and st.usable and st.log == [True] * 3, f"call {i + 1}: conv_c8 and both conv_pair launches carry the flags"
                assert st.flags[0].tolist() == want_flags[i] + [1], f"call {i + 1}"
        return outs

    switches(reuse=False)
    off = run_all(False)
    assert lf.reuse_state() is None
    switches(reuse=True, slots=5)
    lf.__dict__.pop("_packed", None)
    on = run_all(True)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), f"call {i + 1}: output differs with the reuse on"
    # a forward in training mode builds no state
    lf.__dict__.pop("_packed", None)
    lf.train()
    lf.run(ops.FM(xts[0].clone()), ops.from_nchw(torch.stack([pool[0]] * 4).cuda(), Cpad=8), ops.FM.empty(1, H, W, 64))
    assert lf.reuse_state() is None


def _code_gops(m, gops, n):
    from tdvc_amd.synth import ref_list
    outs = []
    with torch.no_grad():
        for g in gops:
            refs = [g[:, 0]]
            for t in range(1, n + 1):
                recon, bpp_res, bpp_mv = m(g[:, t], ref_list(refs), True)
                refs.append(recon)
                outs.append((recon.clone(), bpp_res.clone(), bpp_mv.clone()))
    return outs


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for fa, fb in zip(a, b) for u, v in zip(fa, fb))


def _model(scale=1.0):
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.synth import fill_parameters
    m = VideoCompressor()
    fill_parameters(m)
    if scale != 1.0:
        with torch.no_grad():
            for p in m.mcfilter.conv01.parameters():
                p.mul_(scale)
    return m


def test_video_compressor_reuse_bit_identical(switches):
    from tdvc_amd.synth import make_gop, ref_list
    gops = [make_gop(4321 + k, 7, 128, 128).cuda().unsqueeze(0) for k in range(2)]           # (B = 1, T, 3, H, W)
    m = _model().cuda().eval()
    switches(reuse=False)
    off = _code_gops(m, gops, 6)
    assert m.mcfilter.reuse_state() is None
    switches(reuse=True)
    m.clear_packed()
    on = _code_gops(m, gops, 6)
    st = m.mcfilter.reuse_state()
    assert st is not None and st.usable and st.log == [True] * 3
    assert st.flags[0].tolist() == [0, 0, 1, 1], "the last P-frame of a GOP finds two of its three reference slices"
    assert _same(on, off), "recon / bpp_res / bpp_mv must be byte-equal with the reuse on and off"

    # other weights through load_state_dict: the maps of the old weights must be gone
    other = _model(0.5)
    m.load_state_dict(other.state_dict())
    assert m.mcfilter.reuse_state() is None
    got = _code_gops(m, gops[:1], 3)
    fresh = _code_gops(other.cuda().eval(), gops[:1], 3)
    assert _same(got, fresh) and not _same(got, on[:3])

    # a .train() forward builds no state
    m.clear_packed()
    m.train()
    m(gops[0][:, 1], ref_list([gops[0][:, 0]]), True)
    assert m.mcfilter.reuse_state() is None
    m.eval()


def test_video_compressor_reuse_batch_of_two(switches):
    from tdvc_amd.synth import make_gop
    g = torch.stack([make_gop(555 + k, 5, 128, 128) for k in range(2)]).cuda()               # (B = 2, T, 3, H, W)
    m = _model().cuda().eval()
    switches(reuse=False)
    off = _code_gops(m, [g], 4)
    switches(reuse=True)
    m.clear_packed()
    on = _code_gops(m, [g], 4)
    st = m.mcfilter.reuse_state()
    assert st is not None and st.usable and st.log == [True] * 6
    assert st.flags.tolist() == [[0, 0, 1, 1]] * 2
    assert _same(on, off)
