"""fp32 training on the bf16 matrix pipe: VideoCompressor.train_f32_split / TrainStep(f32_split=True) / ops.f32_split_train.  With the flag the
fp32 convs of a taped .train() forward and of its backward sweep run on conv_split, the fp32 conv weight gradients on conv_wgrad_split; without
it nothing changes.  Set-ups and yardsticks are tests/test_train_model_fp32_gpu.py's (whole model, the fp32 oracle) and
tests/test_train_fp32_coders_gpu.py's (one coder alone, the packed forms)."""
import warnings

import pytest
import torch

import test_model_fp32_gpu as EVAL
import test_train_fp32_coders_gpu as TC
import test_train_model_fp32_gpu as TM
from util import randn, rnd16, to_fm

pytestmark = pytest.mark.gpu

SPLIT_KERNELS = {"conv_split", "conv_wgrad_split", "dcn_columns_f32", "dcn_col2im_f32"}
_CACHE = {}


def split_sweep(side: bool = False, profile: bool = False):
    """TM.device_sweep(True) with `train_f32_split` set: one taped forward + backward of the whole model on the fixed sample"""
    from tdvc_amd import autograd, ops
    dev = TM._device_model()
    dev.train_model_fp32 = True
    dev.train_f32_split = True
    x, refs = TM._sample()
    xc, rc = x.cuda(), refs.cuda()
    if profile:
        ops.PROFILE = []
    try:
        with autograd.record(side_stream=torch.cuda.Stream() if side else None) as tape:
            nf = {k: {kk: to_fm(v, ops, Cpad=128, dtype=torch.float32) for kk, v in d.items()} for k, d in TM._noise().items()}
            r, br, bm, _, _ = dev(xc, rc, True, noise=nf)
            assert tape.f32_split_train and not ops.F32_SPLIT_TRAIN
            diff = r - xc
            tape.grad_tensor(r).copy_(diff * (2.0 * TM.LAM / diff.numel()))
            tape.rate_grad = 1.0 / float(TM.B * TM.HH * TM.WW)
            tape.backward()
        torch.cuda.synchronize()
        prof = ops.PROFILE
    finally:
        ops.PROFILE = None
    assert not ops.F32_SPLIT_TRAIN
    return dict(loss=float(TM.LAM * (diff * diff).mean() + br.mean() + bm.mean()), bpp_res=float(br.mean()), bpp_mv=float(bm.mean()), prof=prof,
                grads={k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in dev.named_parameters()})


# ------------------------------------------------------------------------------------------------------------------ 1. the whole-model sweep
def test_whole_model_sweep_on_the_split_kernels(report):
    """1 x 64 x 64, train_model_fp32 and train_f32_split: only split kernels in the profile; the whole-gradient relative L2 error against the
    fp32 oracle within the project's gate for the fp32 mode (e <= e16 / 8, e16 from the default mode in this test); loss and rate terms within
    the fp32 test's GATES.  e_split / e32 is recorded, not gated: e32 is dominated by the fp16-rounded DCN output."""
    o = TM.oracle_sweep()
    ds = split_sweep(profile=True)
    kernels = [e["kernel"] for e in ds["prof"]]
    count = {k: kernels.count(k) for k in sorted(set(kernels))}
    report(f"train_f32_split sweep at 1x64x64: launches per kernel {count}")
    assert "conv_split" in count and "conv_wgrad_split" in count
    assert "conv_f32" not in count and "conv_wgrad_f32" not in count
    assert set(kernels) == SPLIT_KERNELS, sorted(set(kernels) ^ SPLIT_KERNELS)
    d32, d16 = TM.device_sweep(True), TM.device_sweep(False)
    for k, gate in (("bpp_res", EVAL.GATES["bpp_res"]), ("bpp_mv", EVAL.GATES["bpp_mv"]), ("loss", EVAL.GATES["recon"])):
        report(f"train_f32_split forward {k}: oracle {o[k]:.7f} split {ds[k]:.7f} (rel {abs(ds[k] - o[k]) / abs(o[k]):.2e}; conv_f32: "
               f"{abs(d32[k] - o[k]) / abs(o[k]):.2e}, gate {gate:.2e})")
        assert abs(ds[k] - o[k]) <= gate * abs(o[k]), f"{k}: split {ds[k]!r} oracle {o[k]!r}, gate {gate:.2e} relative"
    for k, q in o["grads"].items():
        if not k.endswith(".quantiles") and q is not None:
            assert ds["grads"][k] is not None, f"{k}: no gradient from the split sweep"
    gs, gr = TM._whole(ds["grads"], o["grads"])
    g32, _ = TM._whole(d32["grads"], o["grads"])
    g16, _ = TM._whole(d16["grads"], o["grads"])
    es, e32, e16 = TM._rel(gs, gr), TM._rel(g32, gr), TM._rel(g16, gr)
    report(f"whole-model gradient parity (1x64x64, {gr.numel()} values): rel L2 err e_split = {es:.3e}, e32 = {e32:.3e}, e16 = {e16:.3e}; "
           f"e_split / e32 = {es / e32:.3f} (recorded), e16 / e_split = {e16 / es:.1f}; split against conv_f32 gradients: {TM._rel(gs, g32):.3e}")
    assert es <= e16 / 8, f"e_split = {es:.3e}, e16 = {e16:.3e}"


def test_side_stream_split_sweep_is_bit_identical(report):
    from tdvc_amd import ops
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, True
    try:
        one, two = split_sweep(), split_sweep(side=True)
    finally:
        ops.DETERMINISTIC = prev
    bad = [k for k, g in one["grads"].items() if (g is None) != (two["grads"][k] is None) or (g is not None and not torch.equal(g, two["grads"][k]))]
    assert not bad, f"side-stream split sweep differs in {len(bad)} tensors, e.g. {bad[:4]}"
    report(f"train_f32_split sweep: side-stream weight gradients bit-identical to the single-stream sweep ({sum(g is not None for g in one['grads'].values())} tensors)")


def test_one_coder_alone_under_the_ops_switch(report):
    """tests/test_train_fp32_coders_gpu.py's MVCoder set-up under ops.f32_split_train(True), no model flag: every conv and weight gradient it
    launches is a split kernel, as many as the fp32 kernels without the switch"""
    from tdvc_amd import autograd, ops, synth
    from tdvc_amd.model import coder as dc
    cd = dc.MVCoder(128)
    synth.fill_parameters(cd)
    cd = cd.cuda().train()
    runs = []
    for on in (False, True):
        ops.PROFILE = []
        try:
            with ops.f32_split_train(on), autograd.record() as tape:
                x_hat, _ = cd.run(to_fm(rnd16(randn(2, 64, 64, 64, seed=5) * 0.5), ops), training=True, f32=True)
                tape.grad(x_hat).t.fill_(1.0 / 64)
                tape.rate_grad = 1.0
                tape.backward()
            torch.cuda.synchronize()
            runs.append([e["kernel"] for e in ops.PROFILE])
        finally:
            ops.PROFILE = None
    off, on = runs
    assert set(off) == {"conv_f32", "conv_wgrad_f32"} and set(on) == {"conv_split", "conv_wgrad_split"}, (sorted(set(off)), sorted(set(on)))
    assert [{"conv_f32": "conv_split", "conv_wgrad_f32": "conv_wgrad_split"}[k] for k in off] == on
    report(f"one fp32 coder under ops.f32_split_train: {on.count('conv_split')} conv_split + {on.count('conv_wgrad_split')} conv_wgrad_split launches")


# ------------------------------------------------------------------------------------------------------------------ 2. training steps
def _steps(tag, mode):
    """mode "model": four TrainStep(model_fp32=True, f32_split=True) steps on TM's sample; "coder": three TrainStep(coder_fp32=True,
    f32_split=True) steps on TC's; under ops.DETERMINISTIC, the last step profiled; cached per (tag, mode)"""
    key = (tag, mode)
    if key in _CACHE:
        return _CACHE[key]
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, True
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            if mode == "model":
                x, refs = TM._sample()
                x, refs = x.cuda(), refs.cuda()
                torch.manual_seed(0)
                net = TM._device_model()
                step, n = TrainStep(net, train_lambda=TM.LAM, lr=1e-4, model_fp32=True, f32_split=True), 4
            else:
                x, refs = TC._sample()
                torch.manual_seed(1111)
                net = TC._fresh_model()
                step, n = TrainStep(net, train_lambda=256.0, lr=2e-4, loss_scale=128.0, coder_fp32=True, f32_split=True), 3
            assert net.train_f32_split is True and step.f32_split is True
            logs = [dict(step(x, refs)) for _ in range(n - 1)]
            ops.PROFILE = []
            try:
                logs.append(dict(step(x, refs)))
                torch.cuda.synchronize()
                prof = [e["kernel"] for e in ops.PROFILE]
            finally:
                ops.PROFILE = None
    finally:
        ops.DETERMINISTIC = prev
    _CACHE[key] = dict(net=net, step=step, logs=logs, prof=prof, after={k: v.detach().clone() for k, v in net.state_dict().items()},
                       warned=[str(w.message) for w in caught], sample=(x, refs))
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["model", "coder"])
def test_train_steps_with_f32_split(mode, report):
    r = _steps("a", mode)
    for log in r["logs"]:
        assert not log["skipped"]
        for k in ("rd_loss", "mse", "bpp_res", "bpp_mv", "aux_loss", "grad_norm"):
            assert log[k] == log[k] and abs(log[k]) != float("inf"), (k, log)
    report(f"f32_split train steps ({mode}_fp32): " + "; ".join(f"rd {l['rd_loss']:.4f} |g| {l['grad_norm']:.3e}" for l in r["logs"]))
    assert r["logs"][-1]["rd_loss"] < r["logs"][0]["rd_loss"]
    assert not [m for m in r["warned"] if "fp32" in m], r["warned"]
    kernels = set(r["prof"])
    assert "conv_split" in kernels and "conv_wgrad_split" in kernels and "conv_f32" not in kernels and "conv_wgrad_f32" not in kernels, sorted(kernels)
    if mode == "model":
        assert kernels == SPLIT_KERNELS, sorted(kernels ^ SPLIT_KERNELS)


@pytest.mark.parametrize("mode", ["model", "coder"])
def test_f32_split_steps_are_reproducible(mode, report):
    a, b = _steps("a", mode), _steps("b", mode)
    bad = [k for k in a["after"] if not torch.equal(a["after"][k], b["after"][k])]
    report(f"{len(a['logs'])} {mode}_fp32 + f32_split steps, twice: {len(bad)}/{len(a['after'])} state tensors differ")
    assert not bad, f"split training is not reproducible run to run: {bad[:4]}"
    assert [l["rd_loss"] for l in a["logs"]] == [l["rd_loss"] for l in b["logs"]]


# ------------------------------------------------------------------------------------------------------------------ 3. the split twins
def _split_twins(net):
    return [(name, pc) for name, pc in TC._forms(net) if pc.wsplit is not None or pc.wsplit_buf is not None]


@pytest.mark.parametrize("mode", ["model", "coder"])
def test_split_twins_follow_the_optimizer(mode, report):
    """after the steps (the optimizer ran last: every twin is stale) each layer's and each dgrad / plain / column form's packed_split() equals
    a fresh pack of the updated parameters; one more step packs them into the same buffers; no fp32 (float) twin was built"""
    from tdvc_amd import ops
    r = _steps("a", mode)
    net = r["net"]
    twins = _split_twins(net)
    kinds = {k: sum(1 for n, _ in twins if n.endswith(k)) for k in (" dgrad", " plain", " column")}
    assert len(twins) >= (60 if mode == "coder" else 100) and kinds[" dgrad"] >= 30, (len(twins), kinds)
    assert all(pc.wsplit is None for _, pc in twins), "a twin is current although the optimizer ran after its last use"
    floats = [n for n, pc in TC._forms(net) if pc.w32 is not None or pc.w32_buf is not None]
    if mode == "coder":                               # (the whole-model mode's fp32 deformable conv reads a float packing)
        assert not floats, f"a split step packed float twins: {floats[:4]}"
    ptrs = {n: pc.wsplit_buf.data_ptr() for n, pc in twins}
    assert not r["step"](*r["sample"])["skipped"]
    torch.cuda.synchronize()
    assert {n for n, _ in _split_twins(net)} == set(ptrs), "a step built a new twin"
    for n, pc in twins:
        got = pc.packed_split()
        assert got.data_ptr() == ptrs[n], f"{n}: the twin moved to a new buffer"
        assert torch.equal(got.view(torch.int16), ops._pack(pc.wsrc, pc.tables, None, "bf16x3").view(torch.int16)), f"{n}: stale split twin"
    n16, _ = TC._assert_forms_current(net)
    report(f"{mode}_fp32 + f32_split: {len(twins)} split twins ({kinds}) of {n16} forms equal a fresh packing after a step, in their old buffers")


# ------------------------------------------------------------------------------------------------------------------ 4. nothing else changes
def _profiled_step(step, x, refs):
    seq, log = TM._profiled_step(step, x, refs)
    assert not log["skipped"]
    return seq


def test_other_training_modes_are_untouched(report):
    """a default TrainStep and TrainStep(coder_fp32=True) launch the same profiled kernels before and after another model trained with the flag,
    build no split twin, and `net.f32_split = True` alone leaves a taped step on conv_f32"""
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    x, refs = TC._sample()
    torch.manual_seed(3)
    nets = {"default": TC._fresh_model(), "coder": TC._fresh_model()}
    steps = {"default": TrainStep(nets["default"], train_lambda=256.0, lr=1e-4, loss_scale=128.0),
             "coder": TrainStep(nets["coder"], train_lambda=256.0, lr=1e-4, loss_scale=128.0, coder_fp32=True)}
    before = {}
    for k, st in steps.items():
        assert st.f32_split is False and nets[k].train_f32_split is False
        assert not st(x, refs)["skipped"]
        before[k] = _profiled_step(st, x, refs)
    other = TC._fresh_model()
    flagged = TrainStep(other, train_lambda=256.0, lr=1e-4, loss_scale=128.0, coder_fp32=True, f32_split=True)
    seq_f = _profiled_step(flagged, x, refs)
    assert {"conv_split", "conv_wgrad_split"} <= {k for k, _ in seq_f} and not ops.F32_SPLIT_TRAIN
    for k, st in steps.items():
        assert _profiled_step(st, x, refs) == before[k], f"the {k} step launches other kernels after another model trained with f32_split"
        assert not _split_twins(nets[k]), f"the {k} step built split twins"
    names = {k: {kern for kern, _ in seq} for k, seq in before.items()}
    assert not names["default"] & {"conv_f32", "conv_split", "conv_wgrad_f32", "conv_wgrad_split"}
    assert {"conv_f32", "conv_wgrad_f32"} <= names["coder"] and not names["coder"] & {"conv_split", "conv_wgrad_split"}
    # the flagged step's list is the coder_fp32 step's with the fp32 kernels renamed
    ren = {"conv_f32": "conv_split", "conv_wgrad_f32": "conv_wgrad_split"}
    assert [(ren.get(kern, kern), shape) for kern, shape in before["coder"]] == seq_f
    nets["coder"].f32_split = True                    # the inference switch: a taped step stays on conv_f32
    assert _profiled_step(steps["coder"], x, refs) == before["coder"]
    assert not _split_twins(nets["coder"])
    # a later TrainStep without the flag writes it back
    TrainStep(other, train_lambda=256.0, lr=1e-4, loss_scale=128.0, coder_fp32=True)
    assert other.train_f32_split is False
    report(f"default ({len(before['default'])} launches) and coder_fp32 ({len(before['coder'])}) steps: identical kernel lists before and after "
           f"f32_split steps on another model, no split twin; net.f32_split alone leaves the taped step on conv_f32")


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    from tdvc_amd.train import TrainStep
    net = TC._fresh_model()
    with pytest.raises(ValueError, match="f32_split=True needs coder_fp32=True or model_fp32=True"):
        TrainStep(net, f32_split=True)
    with pytest.raises(ValueError):
        TrainStep(net, f32_split=True, graph=True)
    with pytest.raises(ValueError, match="not supported with graph=True"):
        TrainStep(net, coder_fp32=True, f32_split=True, graph=True)
    with pytest.raises(ValueError, match="not supported with graph=True"):
        TrainStep(net, model_fp32=True, f32_split=True, graph=True)
    assert net.train_f32_split is False and net.train_coder_fp32 is False and net.train_model_fp32 is False
