"""The fp32 islands on conv_split (`ops.f32_split`, `VideoCompressor.f32_split`): the coders' strings against the fp32 CPU oracle's up to
rounding ties, encoder / decoder agreement bit for bit, the model's PSNR and bpp within the project's parity gates of the conv_f32 islands,
the kernels the profile names, and training untouched."""
import math

import pytest
import torch

from test_entropy_coding_gpu import coders  # noqa: F401  (the fixture: oracle MVCoder + the GPU coder with its weights)
from tests import helpers_model_fp32 as M
from util import randn, rnd16, to_fm

pytestmark = pytest.mark.gpu

TIE = 2e-5            # the project's tie distance (test_fp32_island_bitstreams_equal_oracle)


def _model(**flags):
    from tdvc_amd import synth
    from tdvc_amd.model import VideoCompressor
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda().eval()
    assert m.f32_split is False
    for k, v in flags.items():
        setattr(m, k, v)
    return m


def _profiled(fn):
    from tdvc_amd import ops
    ops.PROFILE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [(e["kernel"], e["shape"]) for e in ops.PROFILE]
    finally:
        ops.PROFILE = None


def psnr(a, b):
    return 10 * math.log10(1.0 / float(((a - b) ** 2).mean()))


@pytest.mark.parametrize("H,W", [(64, 64), (128, 192)])
def test_split_island_strings_and_round_trip(coders, H, W, report):  # noqa: F811
    from tdvc_amd import ops
    ref, m = coders
    x = rnd16(randn(1, 64, H, W, seed=31, scale=0.5))
    xf = to_fm(x, ops)
    with torch.no_grad():
        enc_o = ref.compress(x)
    with ops.f32_split(True):
        enc = m.compress(xf, f32=True)
        dec = m.decompress(enc["strings"], enc["shape"], f32=True)
        x_hat_enc = m._g_s(enc["_debug"][0]["y_hat"], False)
    ys, zs = enc["strings"]
    d = enc["_debug"][0]
    assert zs[0] == enc_o["strings"][1][0], "z byte string differs from the oracle's compress()"
    sym = d["symbols"].cpu().view(-1)
    sym_o = torch.tensor(enc_o["_debug"][0]["symbols"])
    nflip = int((sym != sym_o).sum())
    report(f"split islands {H}x{W}: y symbols differing from the oracle's {nflip}/{sym.numel()}; y string {len(ys[0])} B (oracle {len(enc_o['strings'][0][0])})")
    if ys[0] != enc_o["strings"][0][0]:
        assert nflip, "same symbols, different y bytes"
        with torch.no_grad():
            y_o = ref.g_a(x)[0].permute(1, 2, 0).reshape(-1)                 # (h, w, c) order of the symbol list
        yh_o = enc_o["_debug"][0]["y_hat"]
        mean_o = yh_o[0].permute(1, 2, 0).reshape(-1) - sym_o.float()
        first = int((sym != sym_o).nonzero()[0])
        dist = abs(abs(float(y_o[first] - mean_o[first]) - float(sym_o[first])) - 0.5)
        report(f"split islands {H}x{W}: first differing symbol at flat index {first}: |y - mean - q| is {dist:.2e} from the rounding boundary")
        assert dist <= TIE, "the first differing symbol is not a rounding tie"
        assert bool((sym[:first] == sym_o[:first]).all())
    assert torch.equal(dec["y_hat"].t, d["y_hat"].t), "decoder y_hat differs from encoder y_hat"
    assert torch.equal(dec["x_hat"].t, x_hat_enc.t), "decoder x_hat differs from the encoder's"


@pytest.mark.parametrize("B", [1, 2])
def test_split_model_encode_decode(B):
    m = _model(coder_fp32=True, f32_split=True)
    (x0, r0), (x1, r1) = M.frame(), M.frame(1234)
    x, refs = torch.cat([x0, x1])[:B].cuda(), torch.cat([r0, r1])[:B].cuda()

    def round_trip():
        enc = m.encode(x, refs)
        return enc, m.decode(enc["strings"], enc["shapes"], refs)

    (enc, dec), prof = _profiled(round_trip)
    assert torch.equal(enc["recon"], dec) and bool(torch.isfinite(dec).all())
    assert any(k == "conv_split" for k, _ in prof)


@pytest.mark.parametrize("H,W", [(64, 64), (128, 192)])
def test_split_forward_parity_and_kernels(H, W, report):
    """enabled_amp=False: both coders are fp32 islands.  Flag on against flag off: the project's parity gates, and every conv of an fp32
    map on conv_split (a forward without compress() runs no native context chain: no conv_f32 row at all)"""
    m = _model()
    x, refs = M.frame(1234, H, W)
    x, refs = x.cuda(), refs.cuda()
    with torch.no_grad():
        off, prof_off = _profiled(lambda: m(x, refs, False))
        m.f32_split = True
        on, prof_on = _profiled(lambda: m(x, refs, False))
    k_off, k_on = [k for k, _ in prof_off], [k for k, _ in prof_on]
    assert "conv_split" not in k_off and "conv_f32" in k_off
    assert "conv_f32" not in k_on
    assert [("conv_f32" if k == "conv_split" else k, s) for k, s in prof_on] == prof_off              # the same launches, nothing else moved
    dp = psnr(on[0], x) - psnr(off[0], x)
    db = float(on[1] + on[2]) - float(off[1] + off[2])
    report(f"split islands forward {H}x{W}: dPSNR {dp:+.5f} dB, dbpp {db:+.6f} ({k_on.count('conv_split')} convs on conv_split)")
    assert abs(dp) <= 0.02 and abs(db) <= 0.001


def test_split_model_fp32_forward(report):
    m = _model(model_fp32=True)
    x, refs = M.frame()
    x, refs = x.cuda(), refs.cuda()
    with torch.no_grad():
        off = m(x, refs, True)
        m.f32_split = True
        on, prof = _profiled(lambda: m(x, refs, True))
    kern = [k for k, _ in prof]
    assert "conv_split" in kern
    dp = psnr(on[0], x) - psnr(off[0], x)
    db = float(on[1] + on[2]) - float(off[1] + off[2])
    report(f"model_fp32 + f32_split 64x64: dPSNR {dp:+.5f} dB, dbpp {db:+.6f} ({kern.count('conv_split')} convs on conv_split)")
    assert abs(dp) <= 0.02 and abs(db) <= 0.001


def test_split_flag_leaves_training_alone():
    """under the tape nothing changes: a TrainStep with fp32 coders launches the same kernels with the flag set on the model"""
    from tdvc_amd import synth
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.train import TrainStep
    net = VideoCompressor()
    synth.fill_parameters(net)
    net = net.cuda().train()
    x, refs = M.frame(1234)
    x, refs = x.cuda(), refs.cuda()
    step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0, coder_fp32=True)
    step(x, refs)
    _, before = _profiled(lambda: step(x, refs))
    net.f32_split = True
    _, after = _profiled(lambda: step(x, refs))
    assert after == before
    assert all(k != "conv_split" for k, _ in after) and any(k == "conv_f32" for k, _ in after)


def test_split_flag_is_ignored_by_a_train_mode_forward():
    """the model's flag is an inference / coding switch: a .train() forward with fp32 coders and no recording tape stays on conv_f32"""
    m = _model(f32_split=True)
    m.train_coder_fp32 = True
    m.train()
    x, refs = M.frame(1234)
    with torch.no_grad():
        _, prof = _profiled(lambda: m(x.cuda(), refs.cuda(), True))
    kern = [k for k, _ in prof]
    assert "conv_f32" in kern and "conv_split" not in kern
