"""The coders' rate branches on the side stream (tdvc_amd/model/modules.py: RATE_FORK; tdvc_rate_branch / tdvc_rate_join) in the whole
model: `VideoCompressor` in eval mode with filler weights.  The fork moves launches to another stream and changes none of them, so
recon, bpp_res and bpp_mv are byte-equal with the switch on and off -- at 64 x 64 (z is 1 x 1) and 128 x 192, for one image and two,
with the fp16-in coders and the fp32 islands, and over three calls in a row (the allocator hands the branch's buffers out again).  The
holders that keep those buffers alive are empty behind every forward, also one that raises between the fork and the join; profiled,
traced and training calls keep the one-stream sequence.

What "the off result" is: consecutive conv launches walk their tiles in opposite directions (tdvc_conv2d, a per-thread launch parity), and
feat_fusion's fused channel sums keep the order of the walk in their last bits.  A forward whose convs count odd (two images through fp32
coders at 128 x 192: conv_f32 does not take part in the alternation) therefore gives two results, call by call in turn, with or without
the fork.  The reference is the PAIR of results of two consecutive forwards with the switch off, and a later forward is held to the one
of its own parity; that the fork leaves every conv its place in the alternation is part of what the equality shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.synth import fill_parameters
    m = VideoCompressor()
    fill_parameters(m)
    return m.cuda().eval()


@pytest.fixture()
def fork():
    import tdvc_amd.model.modules as M

    def set_(on):
        M.RATE_FORK = bool(on)
    yield set_
    M.RATE_FORK = True


@pytest.fixture()
def entry_points(monkeypatch):
    """the library's entry points in launch order, as `ops.launch` is asked for them"""
    from tdvc_amd import ops
    names, real = [], ops.launch

    def launch(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)
    monkeypatch.setattr(ops, "launch", launch)
    return names


def _inputs(B, H, W):
    from tdvc_amd.synth import make_gop, ref_list
    g = torch.stack([make_gop(97 + b, 2, H, W) for b in range(B)]).cuda()          # (B, T, 3, H, W): I, P
    return g[:, 1], ref_list([g[:, 0]])


def _forward(m, x, refs, amp=True, **kw):
    with torch.no_grad():
        out = m(x, refs, amp, **kw)
    torch.cuda.synchronize()
    return [o.clone() for o in out[:3]]


def _off_pair(m, x, refs, amp=True):
    """the results of two consecutive forwards with the switch off: behind them forward k (k = 0, 1, ...) starts at the parity of pair[k % 2]"""
    return [_forward(m, x, refs, amp), _forward(m, x, refs, amp)]


def _same(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


@pytest.mark.parametrize("amp", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(64, 64), (128, 192)])
def test_forked_forward_gives_the_same_bytes(model, fork, entry_points, H, W, B, amp):
    x, refs = _inputs(B, H, W)
    fork(False)
    off = _off_pair(model, x, refs, amp)
    assert "tdvc_rate_branch" not in entry_points and entry_points.count("tdvc_gc_forward") == 4
    assert float(off[0][0].std()) > 0.01 and float(off[0][1].min()) > 0 and float(off[0][2].min()) > 0
    fork(True)
    for call in range(3):
        del entry_points[:]
        on = _forward(model, x, refs, amp)
        assert entry_points.count("tdvc_rate_branch") == 2 and "tdvc_gc_forward" not in entry_points and "tdvc_eb_forward" not in entry_points
        assert _same(on, off[call % 2]), f"call {call}: recon / bpp_res / bpp_mv differ with the rate branches on the side stream"
        assert not model.mvCoder.rate_hold and not model.resCoder.rate_hold


@pytest.mark.parametrize("raising", ["mvCoder", "resCoder"])
def test_a_forward_that_raises_behind_the_fork_leaves_nothing_pending(model, fork, monkeypatch, raising):
    x, refs = _inputs(1, 64, 64)
    fork(False)
    off = _off_pair(model, x, refs)
    fork(True)
    coder = getattr(model, raising)
    seen = []

    def run_g_s(*a, **kw):
        seen.append(len(coder.rate_hold))
        raise RuntimeError("injected behind the fork")
    with monkeypatch.context() as mp:
        mp.setattr(coder, "run_g_s", run_g_s)
        with pytest.raises(RuntimeError, match="injected behind the fork"):
            _forward(model, x, refs)
    assert seen and seen[0] > 0, "the branch was not forked in front of g_s"
    assert not model.mvCoder.rate_hold and not model.resCoder.rate_hold
    from tdvc_amd import ops
    ops.rate_join(0), ops.rate_join(1)                     # joined already: no-ops
    again = _forward(model, x, refs)                       # and the slots are free: the next forward forks again (the forward that
    assert _same(again, off[0]) or _same(again, off[1])    # raised stopped somewhere in the alternation: either parity)


@pytest.mark.parametrize("mode", ["profile", "trace", "train"])
def test_profiled_traced_and_training_calls_keep_the_one_stream_sequence(model, fork, entry_points, mode):
    from tdvc_amd import ops
    x, refs = _inputs(1, 64, 64)

    def run():
        del entry_points[:]
        if mode == "profile":
            ops.PROFILE = []
        elif mode == "train":
            model.train()
        try:
            out = _forward(model, x, refs, **(dict(trace={}) if mode == "trace" else {}))
        finally:
            ops.PROFILE = None
            model.eval()
        return out, list(entry_points)
    fork(False)
    run()
    off, want = run()                                      # two forwards further the parity is this one's again
    fork(True)
    run()
    on, got = run()
    assert got == want and "tdvc_rate_branch" not in got and got.count("tdvc_gc_forward") == 2
    if mode != "train":                                    # a training forward draws its quantisation noise
        assert _same(on, off)
    assert not model.mvCoder.rate_hold and not model.resCoder.rate_hold
