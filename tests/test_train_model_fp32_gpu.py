"""Whole-model fp32 training (TrainStep(model_fp32=True), VideoCompressor.train_model_fp32): the reference's `amp: False` branch
(tools/train.py:152-159) on the GPU.  The yardstick is the oracle's plain fp32 CPU path with torch autograd, which computes the same
thing: fp32 everywhere but the deformable conv's fp16 output (and, in the backward, that output's fp16 gradient).

Setup of the gradient test = tests/test_autograd_gpu.py::test_full_model_backward_and_steps: B = 1, 64 x 64, filler weights,
lambda = 2048, the three noise draws of each coder injected on both sides.  The op-level forms: tests/test_train_model_fp32_ops_gpu.py
(the mixed-dtype refusal of the DCN backward, with its sentinel check, is there too)."""
import warnings

import pytest
import torch

import test_model_fp32_gpu as EVAL
import test_train_fp32_coders_gpu as TC
from util import to_fm

pytestmark = pytest.mark.gpu

B, HH, WW, LAM = 1, 64, 64, 2048.0
SUBMODULES = ("mvCoder", "resCoder", "extra_fea", "motion_est", "mcnet", "loopfilter", "mcfilter")
FP32_KERNELS = {"conv_f32", "conv_wgrad_f32", "dcn_columns_f32", "dcn_col2im_f32"}
_CACHE = {}


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-300))


def _sample():
    from tdvc_amd import synth
    frames = synth.make_gop(1234, 7, HH, WW).float()
    return frames[3:4], torch.stack([frames[0], frames[0], frames[1], frames[2]]).unsqueeze(0)


def _noise():
    g = torch.Generator().manual_seed(71)
    u = lambda *s: torch.rand(*s, generator=g) - 0.5
    mk = lambda: {"z": u(B, 128, HH // 64, WW // 64), "y": u(B, 128, HH // 16, WW // 16), "y_lik": u(B, 128, HH // 16, WW // 16)}
    return {"mv": mk(), "res": mk()}


def oracle_sweep():
    """the oracle's fp32 forward and autograd on the fixed sample, once per session: losses, rate terms, parameter gradients"""
    if "oracle" not in _CACHE:
        from oracle.tdvc_ref.codec import VideoCompressor as RefVC
        from tdvc_amd import synth
        ref = RefVC()
        synth.fill_parameters(ref)
        ref.train()
        x, refs = _sample()
        recon, bpp_res, bpp_mv, _, _ = ref(x, refs, noise=_noise())
        loss = LAM * torch.nn.functional.mse_loss(recon, x) + bpp_res.mean() + bpp_mv.mean()
        loss.backward()
        _CACHE["oracle"] = dict(state=ref.state_dict(), loss=float(loss), bpp_res=float(bpp_res.mean()), bpp_mv=float(bpp_mv.mean()),
                                grads={k: (None if q.grad is None else q.grad.clone()) for k, q in ref.named_parameters()})
    return _CACHE["oracle"]


def _device_model():
    from tdvc_amd.model.pnet import VideoCompressor
    dev = VideoCompressor()
    dev.load_state_dict(oracle_sweep()["state"])
    return dev.cuda().train()


def device_sweep(fp32: bool, side: bool = False, profile: bool = False):
    """one taped forward + backward of the whole model on the fixed sample -> losses, gradients (cpu) and, if asked, the PROFILE rows"""
    from tdvc_amd import autograd, ops
    dev = _device_model()
    dev.train_model_fp32 = fp32
    x, refs = _sample()
    xc, rc = x.cuda(), refs.cuda()
    if profile:
        ops.PROFILE = []
    try:
        with autograd.record(side_stream=torch.cuda.Stream() if side else None) as tape:
            nf = {k: {kk: to_fm(v, ops, Cpad=128, dtype=torch.float32) for kk, v in d.items()} for k, d in _noise().items()}
            r, br, bm, _, _ = dev(xc, rc, True, noise=nf)
            diff = r - xc
            tape.grad_tensor(r).copy_(diff * (2.0 * LAM / diff.numel()))
            tape.rate_grad = 1.0 / float(B * HH * WW)
            tape.backward()
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
    return dict(loss=float(LAM * (diff * diff).mean() + br.mean() + bm.mean()), bpp_res=float(br.mean()), bpp_mv=float(bm.mean()), prof=prof,
                grads={k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in dev.named_parameters()})


def profiled_sweep():
    """the fp32 sweep under ops.PROFILE (shared with the op-level coverage guard)"""
    if "prof" not in _CACHE:
        _CACHE["prof"] = device_sweep(True, profile=True)
    return _CACHE["prof"]


def _whole(grads, ref):
    keys = [k for k, q in ref.items() if q is not None and not k.endswith(".quantiles")]
    return torch.cat([grads[k].reshape(-1) for k in keys]), torch.cat([ref[k].reshape(-1) for k in keys])


# ------------------------------------------------------------------------------------------------------------------ 1. gradient parity
def test_whole_model_gradients_against_the_fp32_oracle(report):
    """e16 = the default mode's whole-gradient relative L2 error against the fp32 oracle (existing code: the yardstick), e32 = the same with
    train_model_fp32.  Operand roundings are 2^-24 against 2^-11, so e32 <= e16 / 8 leaves orders of magnitude of headroom and fails only
    if some stage still runs fp16.  The losses: the two rate terms within the gates tests/test_model_fp32_gpu.py asserts for them
    (GATES["bpp_res"] = 3.6e-7, GATES["bpp_mv"] = 2.4e-7 relative) and rd_loss within its gate for the reconstruction, the value the
    distortion term is made of (GATES["recon"] = 6.2e-6 relative).
    Measured on MI355X: rd_loss 5.6e-7, bpp_res 8.6e-8, bpp_mv 1.8e-7 relative (the default mode: 3.4e-5, 8e-7,
    2.0e-4); e32 = 3.97e-4, e16 = 8.49e-3."""
    o = oracle_sweep()
    d32, d16 = device_sweep(True), device_sweep(False)
    for k in ("loss", "bpp_res", "bpp_mv"):
        report(f"model_fp32 training forward {k}: oracle {o[k]:.7f} fp32 {d32[k]:.7f} (rel {abs(d32[k] - o[k]) / abs(o[k]):.2e}) default {d16[k]:.7f}")
    for k, gate in (("bpp_res", EVAL.GATES["bpp_res"]), ("bpp_mv", EVAL.GATES["bpp_mv"]), ("loss", EVAL.GATES["recon"])):
        assert abs(d32[k] - o[k]) <= gate * abs(o[k]), f"{k}: fp32 {d32[k]!r} oracle {o[k]!r}, gate {gate:.2e} relative"
    for k, q in o["grads"].items():
        if k.endswith(".quantiles"):
            continue
        p = d32["grads"][k]
        if q is None:
            assert p is None or not bool(p.any()), f"{k}: the oracle gives no gradient, the fp32 sweep does"
        else:
            assert p is not None, f"{k}: no gradient from the fp32 sweep"
    g32, gr = _whole(d32["grads"], o["grads"])
    g16, _ = _whole(d16["grads"], o["grads"])
    e32, e16 = _rel(g32, gr), _rel(g16, gr)
    per = sorted((_rel(d32["grads"][k], q), k) for k, q in o["grads"].items()
                 if q is not None and float(q.norm()) > 0 and not k.endswith(".quantiles"))
    report(f"whole-model fp32 gradient parity (1x64x64, {gr.numel()} values in {len(per)} tensors): rel L2 err e32 = {e32:.3e}, e16 = {e16:.3e} "
           f"(ratio {e16 / max(e32, 1e-30):.1f}); per tensor median {per[len(per) // 2][0]:.3e}, 90% {per[int(0.9 * len(per))][0]:.3e}, "
           f"worst five {[(f'{e:.2e}', k) for e, k in per[-5:]]}")
    assert e32 <= e16 / 8, f"e32 = {e32:.3e}, e16 = {e16:.3e}"


def test_side_stream_sweep_is_bit_identical(report):
    """the fp32 sweep with the weight gradients on a side stream (Tape.off_path, what TrainStep does) against the single-stream sweep,
    under ops.DETERMINISTIC: a missing dependency between the streams would show"""
    from tdvc_amd import ops
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, True
    try:
        one = device_sweep(True)
        for rep in range(2):
            two = device_sweep(True, side=True)
            bad = [k for k, g in one["grads"].items() if (g is None) != (two["grads"][k] is None) or (g is not None and not torch.equal(g, two["grads"][k]))]
            assert not bad, f"side-stream fp32 sweep differs in {len(bad)} tensors, e.g. {bad[:4]}"
    finally:
        ops.DETERMINISTIC = prev
    report(f"model_fp32 sweep: side-stream weight gradients bit-identical to the single-stream sweep ({sum(g is not None for g in one['grads'].values())} tensors)")


# ------------------------------------------------------------------------------------------------------------------ 2. training steps
def _four_steps(tag):
    if tag in _CACHE:
        return _CACHE[tag]
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    x, refs = _sample()
    xc, rc = x.cuda(), refs.cuda()
    torch.manual_seed(0)
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, True
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            net = _device_model()
            before = {k: v.detach().clone() for k, v in net.named_parameters()}
            step = TrainStep(net, train_lambda=LAM, lr=1e-4, model_fp32=True)
            logs = [dict(step(xc, rc)) for _ in range(3)]
            ops.PROFILE = []
            try:
                logs.append(dict(step(xc, rc)))
                torch.cuda.synchronize()
                prof = [(e["kernel"], e["shape"]) for e in ops.PROFILE]
            finally:
                ops.PROFILE = None
    finally:
        ops.DETERMINISTIC = prev
    _CACHE[tag] = dict(net=net, step=step, before=before, after={k: v.detach().clone() for k, v in net.state_dict().items()}, logs=logs, prof=prof,
                       warned=[str(w.message) for w in caught])
    return _CACHE[tag]


def test_train_steps_with_model_fp32(report):
    r = _four_steps("a")
    for log in r["logs"]:
        assert not log["skipped"] and log["loss_scale"] == 1.0
        for k in ("rd_loss", "mse", "bpp_res", "bpp_mv", "aux_loss", "grad_norm"):
            assert log[k] == log[k] and abs(log[k]) != float("inf"), (k, log)
    report("model_fp32 train steps: " + "; ".join(f"rd {l['rd_loss']:.4f} |g| {l['grad_norm']:.3e}" for l in r["logs"]))
    assert r["logs"][-1]["rd_loss"] < r["logs"][0]["rd_loss"]
    for sub in SUBMODULES:
        moved = [k for k, v in r["before"].items() if k.startswith(sub + ".") and not torch.equal(v, r["after"][k])]
        assert moved, f"no parameter of {sub} moved in four steps"
    assert r["net"].train_model_fp32 is True and r["net"].train_coder_fp32 is True and r["step"].loss_scale == 1.0
    assert not [m for m in r["warned"] if "fp32" in m], r["warned"]


def test_model_fp32_steps_are_reproducible(report):
    a, b = _four_steps("a"), _four_steps("b")
    bad = [k for k in a["after"] if not torch.equal(a["after"][k], b["after"][k])]
    report(f"4 model_fp32 steps at 1x64x64, twice: {len(bad)}/{len(a['after'])} state tensors differ")
    assert not bad, f"fp32 training is not reproducible run to run: {bad[:4]}"
    assert [l["rd_loss"] for l in a["logs"]] == [l["rd_loss"] for l in b["logs"]]


def test_the_step_really_is_fp32(report):
    """ops.PROFILE of the fourth step: every conv, data-gradient and weight-gradient launch is an fp32 kernel and both launches of the DCN
    backward got fp32 maps"""
    kernels = [k for k, _ in _four_steps("a")["prof"]]
    count = {k: kernels.count(k) for k in sorted(set(kernels))}
    report(f"model_fp32 step at 1x64x64: launches per kernel {count}")
    assert set(kernels) == FP32_KERNELS, sorted(set(kernels) - FP32_KERNELS)
    assert count["dcn_columns_f32"] == 1 and count["dcn_col2im_f32"] == 1


# ------------------------------------------------------------------------------------------------------------------ 3. default untouched
def _profiled_step(step, x, refs):
    from tdvc_amd import ops
    ops.PROFILE = []
    try:
        log = step(x, refs)
        torch.cuda.synchronize()
        return [(e["kernel"], e["shape"]) for e in ops.PROFILE], log
    finally:
        ops.PROFILE = None


def test_default_training_mode_is_untouched(report):
    """a default TrainStep packs no fp32 twin and launches the same kernels before and after the model took model_fp32 steps; switching
    to model_fp32 and back works (forms created late follow the optimizer: the FORMS_CREATED / PackBatch path)"""
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    x, refs = TC._sample()
    net = TC._fresh_model()
    assert net.train_model_fp32 is False
    calls = []
    orig = ops._pack_from_tables_f32

    def counting(*args, **kw):
        calls.append(1)
        return orig(*args, **kw)
    ops._pack_from_tables_f32 = counting
    try:
        step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0)
        assert net.train_model_fp32 is False and step.loss_scale == 128.0 and step.dynamic_scale is True
        assert not step(x, refs)["skipped"]
        seq_a, log = _profiled_step(step, x, refs)
        assert not calls, f"a default-mode training step packed {len(calls)} fp32 weight twins"
        net.train_model_fp32 = True                   # set and unset: nothing sticks to the model
        net.train_model_fp32 = False
        seq_b, log = _profiled_step(step, x, refs)
        assert seq_a == seq_b and not calls
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            f32 = TrainStep(net, train_lambda=256.0, lr=1e-4, model_fp32=True)
            assert net.train_model_fp32 is True
            assert not f32(x, refs)["skipped"] and not f32(x, refs)["skipped"]
        assert calls and not [str(w.message) for w in caught if "fp32" in str(w.message)]
        nforms, ntwins = TC._assert_forms_current(net)
        n_f32 = len(calls)
        step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0)
        assert net.train_model_fp32 is False and net.train_coder_fp32 is False
        assert not step(x, refs)["skipped"]
        seq_c, log = _profiled_step(step, x, refs)
        assert len(calls) == n_f32, "a default-mode step after fp32 steps packed fp32 twins"
        assert seq_c == seq_a, "the default step launches other kernels after the model took model_fp32 steps"
        f32 = TrainStep(net, train_lambda=256.0, lr=1e-4, model_fp32=True)
        l = f32(x, refs)
        assert not l["skipped"] and l["rd_loss"] == l["rd_loss"]
        TC._assert_forms_current(net)
    finally:
        ops._pack_from_tables_f32 = orig
    report(f"default training mode: no fp32 twin packed, {len(seq_a)} profiled launches identical before and after model_fp32 steps; "
           f"{nforms} forms / {ntwins} fp32 twins current after the switch")


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    from tdvc_amd import autograd
    from tdvc_amd.train import TrainStep
    net = TC._fresh_model()
    x, refs = TC._sample()
    net.model_fp32 = True
    with pytest.raises(ValueError, match="inference / coding mode"):
        net(x, refs, True)
    net.eval()
    with pytest.raises(ValueError, match="inference / coding mode"):
        with autograd.record():
            net(x, refs, True)
    net.model_fp32 = False
    net.train()
    with pytest.raises(ValueError, match="model_fp32=True is not supported with graph=True"):
        TrainStep(net, model_fp32=True, graph=True)
    assert net.train_model_fp32 is False and net.train_coder_fp32 is False
