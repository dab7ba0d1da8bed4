"""The glue fusions of the P-frame forward (tdvc_amd/model/modules.py: PYRAMID_FUSED, FLOW_EPILOGUE, RESID_FUSED, RGB_HEAD) in the whole model:
`VideoCompressor` in eval mode at 128 x 192 with filler weights, two consecutive P-frames of one GOP.  recon, bpp_res and bpp_mv are
byte-equal with every switch on, every switch off and each switch alone; a traced call and a call under `ops.PROFILE` run the separate
launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCHES = ("PYRAMID_FUSED", "FLOW_EPILOGUE", "RESID_FUSED", "RGB_HEAD")
H, W = 128, 192


@pytest.fixture(scope="module")
def model():
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.synth import fill_parameters
    m = VideoCompressor()
    fill_parameters(m)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def gop():
    from tdvc_amd.synth import make_gop
    return make_gop(2468, 3, H, W).cuda().unsqueeze(0)                 # (B = 1, T, 3, H, W): I, P, P


@pytest.fixture()
def switches():
    import tdvc_amd.model.modules as M

    def set_(**kw):
        for s in SWITCHES:
            setattr(M, s, bool(kw.get(s, False)))
    yield set_
    for s in SWITCHES:
        setattr(M, s, True)


@pytest.fixture()
def launches(monkeypatch):
    """counts of the launches the switches trade against each other"""
    from tdvc_amd import ops
    n = dict(avgpool2=0, pyramid=0, add_flow=0, conv_flow=0, resid_fused=0, scale_act_res=0, head_streamed=0)
    real = {k: getattr(ops, k) for k in ("avgpool2", "avgpool2_pyramid", "add_flow", "conv", "scale_act_res")}

    def count(key, fn, pred=None):
        def f(*a, **kw):
            if pred is None or pred(kw):
                n[key] += 1
            return fn(*a, **kw)
        return f
    monkeypatch.setattr(ops, "avgpool2", count("avgpool2", real["avgpool2"]))
    monkeypatch.setattr(ops, "avgpool2_pyramid", count("pyramid", real["avgpool2_pyramid"]))
    monkeypatch.setattr(ops, "add_flow", count("add_flow", real["add_flow"]))
    monkeypatch.setattr(ops, "conv", count("conv_flow", real["conv"], lambda kw: kw.get("flow") is not None))
    monkeypatch.setattr(ops, "scale_act_res", count("scale_act_res", real["scale_act_res"]))
    monkeypatch.setattr(ops, "scale_act_res3", count("resid_fused", ops.scale_act_res3))
    real_head = ops.rgb_head_kernel

    def head(enable):
        n["head_streamed"] += int(bool(enable))
        return real_head(enable)
    monkeypatch.setattr(ops, "rgb_head_kernel", head)
    return n


def _two_p_frames(m, g, **kw):
    from tdvc_amd.synth import ref_list
    m.clear_packed()                                                    # every configuration starts without reuse state
    outs, refs = [], [g[:, 0]]
    with torch.no_grad():
        for t in (1, 2):
            recon, bpp_res, bpp_mv = m(g[:, t], ref_list(refs), True, **kw)
            refs.append(recon)
            outs += [recon.clone(), bpp_res.clone(), bpp_mv.clone()]
    torch.cuda.synchronize()
    return outs


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def test_every_switch_setting_gives_the_same_bytes(model, gop, switches, launches):
    switches()
    off = _two_p_frames(model, gop)
    assert launches == dict(avgpool2=20, pyramid=0, add_flow=2, conv_flow=0, resid_fused=0, scale_act_res=launches["scale_act_res"], head_streamed=0)
    n_sar = launches["scale_act_res"]
    for k in launches:
        launches[k] = 0
    switches(**{s: True for s in SWITCHES})
    on = _two_p_frames(model, gop)
    assert launches == dict(avgpool2=0, pyramid=2, add_flow=0, conv_flow=2, resid_fused=2, scale_act_res=n_sar - 4, head_streamed=2)      # per frame: LoopFilter's last pass and the residual's own launch
    assert _same(on, off), "recon / bpp_res / bpp_mv must be byte-equal with the fusions on and off"
    assert float(off[0].std()) > 0.01 and float(off[1]) > 0 and float(off[2]) > 0
    for s in SWITCHES:
        switches(**{s: True})
        assert _same(_two_p_frames(model, gop), off), f"{s} alone changes the result"


def test_traced_and_profiled_calls_keep_the_separate_launches(model, gop, switches, launches):
    from tdvc_amd import ops
    switches(**{s: True for s in SWITCHES})
    want = _two_p_frames(model, gop)
    for k in launches:
        launches[k] = 0
    traced = _two_p_frames(model, gop, trace={})
    assert (launches["avgpool2"], launches["pyramid"], launches["add_flow"], launches["conv_flow"], launches["resid_fused"], launches["head_streamed"]) == (20, 0, 2, 0, 0, 0)
    assert _same(traced, want)
    for k in launches:
        launches[k] = 0
    ops.PROFILE = []
    try:
        prof = _two_p_frames(model, gop)
    finally:
        ops.PROFILE = None
    assert (launches["avgpool2"], launches["pyramid"], launches["add_flow"], launches["conv_flow"], launches["resid_fused"], launches["head_streamed"]) == (20, 0, 2, 0, 0, 0)
    assert _same(prof, want)
