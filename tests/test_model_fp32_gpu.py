"""`VideoCompressor.model_fp32 = True` (every stage on fp32 maps, the reference's `enable_amp: False`) against the CPU oracle's default
mode, which computes the same thing: fp32 everywhere but the deformable conv's fp16 output.

The pinned 64x64 frame (tests/helpers_model_fp32.py; its margins are asserted without a GPU by tests/test_model_fp32_cases_cpu.py):
  * |d(y - mu)| < 1e-4 in both coders, a quarter of the asserted margin; then no flipped y_hat symbol, equal CDF indexes and symbols
    of compress(), and the strings of forward(..., is_compress=True) byte for byte the oracle's;
  * stage gates: 4 x the relative L2 error measured on an MI355X when the mode was built (GATES below; profiles/r16_model_fp32.txt),
    none above its cap: 1e-4 in front of the quantisers (the fp16 path's best stage is 3.8e-4), 1e-3 behind them (the DCN's fp16 output
    rounding may move single elements by an fp16 ulp), 1e-4 relative for the two bpp terms.
128x192 and 192x320 (seed 1234): the gates in front of the quantisers, ff_idx, PSNR within 0.02 dB and bpp within 1e-3 + 0.5 %; flipped
symbols are only reported (the oracle has near-ties there: helpers_model_fp32's docstring).
Round trip, guards and the default of the flag at the end."""
import math

import pytest
import torch

from tests import helpers_model_fp32 as M
from util import fm_to_cpu

pytestmark = pytest.mark.gpu

# relative L2 against the oracle, measured on the pinned frame (128x192 and 192x320 give the same figures to 10 %)
MEASURED_PRE = {"f_cur": 5.19e-7, "f_ref": 5.19e-7, "estmv": 4.69e-7, "mv.y": 1.43e-6, "mv.z": 2.36e-6}
MEASURED_POST = {"mv_x_hat": 1.59e-6, "pred1": 8.44e-6, "pred": 7.94e-6, "resid": 6.75e-6, "recon_f": 4.62e-6, "recon": 1.56e-6}
MEASURED_BPP = {"bpp_res": 9.08e-8, "bpp_mv": 6.08e-8}                # 1 - 2 ulp of the fp32 value the model returns
CAP_PRE, CAP_POST, CAP_BPP = 1e-4, 1e-3, 1e-4
GATES = {**{k: 4 * v for k, v in MEASURED_PRE.items()}, **{k: 4 * v for k, v in MEASURED_POST.items()}, **{k: 4 * v for k, v in MEASURED_BPP.items()}}
assert all(GATES[k] <= CAP_PRE for k in MEASURED_PRE) and all(GATES[k] <= CAP_POST for k in MEASURED_POST) and all(GATES[k] <= CAP_BPP for k in MEASURED_BPP)


@pytest.fixture(scope="module")
def model():
    from tdvc_amd.model import VideoCompressor
    m = VideoCompressor()
    m.load_state_dict(M.oracle().state_dict(), strict=True)
    m = m.cuda().eval()
    assert m.model_fp32 is False
    m.model_fp32 = True
    return m


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def psnr(a, b):
    return 10 * math.log10(1.0 / float(((a - b) ** 2).mean()))


def _forward(m, seed, h, w, compress):
    x, refs = M.frame(seed, h, w)
    out_o, tr_o = M.oracle_frame(seed, h, w)
    tr_g = {}
    with torch.no_grad():
        out_g = m(x.cuda(), refs.cuda(), True, is_compress=compress, trace=tr_g)
    torch.cuda.synchronize()
    return x, out_o, tr_o, out_g, tr_g


def _stages(out_o, tr_o, out_g, tr_g):
    st = {k: rel(fm_to_cpu(tr_g[k]), tr_o[k].float()) for k in ("f_cur", "f_ref", "estmv", "mv_x_hat", "pred1", "pred", "resid", "recon_f")}
    st["recon"] = rel(out_g[0].cpu(), out_o[0])
    for c in ("mv", "res"):
        st[c + ".y"] = rel(fm_to_cpu(tr_g[c]["y"]), tr_o[c + "_dbg"]["y"])
        st[c + ".z"] = rel(fm_to_cpu(tr_g[c]["z"]), tr_o[c + "_dbg"]["z"])
    st["bpp_res"] = abs(float(out_g[1]) - float(out_o[1])) / float(out_o[1])
    st["bpp_mv"] = abs(float(out_g[2]) - float(out_o[2])) / float(out_o[2])
    return st


def _flips(tr_o, tr_g, c):
    return int((fm_to_cpu(tr_g[c]["y_hat"]) != tr_o[c + "_dbg"]["y_hat"]).sum())


def test_pinned_frame_symbols_strings_and_stages(model, report):
    m = model
    x, out_o, tr_o, out_g, tr_g = _forward(m, M.SEED, M.H, M.W, True)
    st = _stages(out_o, tr_o, out_g, tr_g)
    report(f"model_fp32 {M.H}x{M.W} seed {M.SEED}: " + " ".join(f"{k}={v:.2e}" for k, v in st.items()))
    for c, coder, key in (("mv", m.mvCoder, "estmv"), ("res", m.resCoder, "resid")):
        dbg, od = tr_o[c + "_dbg"], tr_o["strings"][c]["_debug"][0]
        yg, gp = fm_to_cpu(tr_g[c]["y"]), fm_to_cpu(tr_g[c]["gp"])
        d_fwd = float(((yg - gp[:, 128:]) - (dbg["y"] - dbg["means"])).abs().max())
        enc = coder.compress(tr_g[key], f32=True)                       # the debug record of the strings forward() produced
        d = enc["_debug"][0]
        q = d["symbols"].cpu().permute(2, 0, 1).unsqueeze(0).float()
        d_ar = float(((yg - (fm_to_cpu(d["y_hat"]) - q)) - M.y_minus_mu(dbg["y"], od)[0]).abs().max())
        report(f"   {c}: max |d(y - mu)| forward {d_fwd:.3e}, compress() {d_ar:.3e}")
        assert d_fwd < M.MARGIN / 4 and d_ar < M.MARGIN / 4, (c, d_fwd, d_ar)
        assert _flips(tr_o, tr_g, c) == 0, f"{c}: flipped forward y_hat symbols"
        assert torch.equal(d["symbols"].cpu().reshape(-1), torch.tensor(od["symbols"], dtype=torch.int32)), f"{c}: compress() symbols differ"
        assert torch.equal(d["indexes"].cpu().reshape(-1), torch.tensor(od["indexes"], dtype=torch.int32)), f"{c}: CDF indexes differ"
        assert enc["strings"][0][0] == tr_o["strings"][c]["strings"][0][0] and enc["strings"][1][0] == tr_o["strings"][c]["strings"][1][0]
        got, want = m.last_strings[c], tr_o["strings"][c]["strings"]
        assert got[0][0] == want[0][0] and got[1][0] == want[1][0], f"{c}: strings of forward(is_compress=True) differ from the oracle's"
    for k, g in GATES.items():
        assert st[k] < g, (k, st[k], g)
    assert torch.equal(tr_g["ff_idx"].cpu().long(), tr_o["ff_idx"])


@pytest.mark.parametrize("H,W", [(128, 192), (192, 320)])
def test_larger_frames(model, H, W, report):
    x, out_o, tr_o, out_g, tr_g = _forward(model, 1234, H, W, False)
    assert torch.equal(tr_g["ff_idx"].cpu().long(), tr_o["ff_idx"]), "in-loop filter patch argmax differs"
    st = _stages(out_o, tr_o, out_g, tr_g)
    report(f"model_fp32 {H}x{W} seed 1234: " + " ".join(f"{k}={v:.2e}" for k, v in st.items())
           + f" | flipped y_hat symbols mv {_flips(tr_o, tr_g, 'mv')} res {_flips(tr_o, tr_g, 'res')}")
    for k in MEASURED_PRE:
        assert st[k] < GATES[k], (k, st[k], GATES[k])
    p_o, p_g = psnr(out_o[0], x), psnr(out_g[0].cpu(), x)
    assert abs(p_o - p_g) <= 0.02, f"PSNR delta {p_o - p_g}"
    for i, name in ((1, "bpp_res"), (2, "bpp_mv")):
        assert abs(float(out_o[i]) - float(out_g[i])) <= 1e-3 + 5e-3 * float(out_o[i]), name


def test_encode_decode_round_trip(model):
    x, refs = M.frame()
    with torch.no_grad():
        enc = model.encode(x.cuda(), refs.cuda())
        dec = model.decode(enc["strings"], enc["shapes"], refs.cuda())
    assert torch.equal(enc["recon"], dec)
    assert bool(torch.isfinite(dec).all()) and dec.dtype == torch.float32 and tuple(dec.shape) == tuple(x.shape)


def test_encode_decode_batch_of_two(model):
    """B = 2 takes encode()'s / decode()'s batch forms: frame b's strings and reconstruction are those of a call with frame b alone"""
    (x0, r0), (x1, r1) = M.frame(), M.frame(1234)
    x, refs = torch.cat([x0, x1]).cuda(), torch.cat([r0, r1]).cuda()
    with torch.no_grad():
        enc = model.encode(x, refs)
        dec = model.decode(enc["strings"], enc["shapes"], refs)
        one = model.encode(x[1:2], refs[1:2])
    assert torch.equal(enc["recon"], dec)
    assert [s[1] for s in enc["strings"]] == [s[0] for s in one["strings"]] and torch.equal(enc["recon"][1:2], one["recon"])


def test_flag_defaults_and_guards(model):
    from tdvc_amd import autograd
    from tdvc_amd.model import VideoCompressor
    assert VideoCompressor().model_fp32 is False
    x, refs = M.frame()
    x, refs = x.cuda(), refs.cuda()
    model.train()
    try:
        with pytest.raises(ValueError):
            model(x, refs, True)
    finally:
        model.eval()
    with pytest.raises(ValueError):
        with autograd.record():
            model(x, refs, True)
