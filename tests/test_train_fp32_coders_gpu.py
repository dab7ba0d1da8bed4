"""Training with fp32 coders (TrainStep(coder_fp32=True), VideoCompressor.train_coder_fp32): the reference keeps mvCoder / resCoder
outside autocast in training too (main/model/pnet.py:33,57), so its tools/train.py optimises them in fp32."""
import inspect
import warnings

import pytest
import torch

from util import randn, rnd16, to_fm

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-12))


def _sample(B=2, H=64, W=64):
    from tdvc_amd import synth
    frames = synth.make_gop(1234, 7, H, W).float()
    x = frames[3:3 + B]
    refs = torch.stack([torch.stack([frames[0], frames[max(t - 3, 0)], frames[max(t - 2, 0)], frames[t - 1]]) for t in range(3, 3 + B)])
    return x.cuda(), refs.cuda()


def _fresh_model():
    from tdvc_amd import synth
    from tdvc_amd.model.pnet import VideoCompressor
    net = VideoCompressor()
    synth.fill_parameters(net)
    return net.cuda().train()


# ------------------------------------------------------------------------------------------------------------------ 1. gradient parity
def test_fp32_coder_gradients_against_the_fp32_oracle(report):
    """MVCoder(N=128), training mode, B = 2, 64 channels at 64 x 64, the three noise draws injected on both sides: the oracle coder in fp32
    with torch autograd against the tape, once with f32=True (e32) and once on the default fp16-in path (e16, the yardstick: existing
    code).  Operand roundings are 2^-24 against 2^-11, so e32 <= e16 / 8 leaves three orders of magnitude of headroom.
    The rate terms compare two fp32 evaluations of the same ~30-layer network, summed over 4096 (y) and 256 (z) positive terms
    -log2(likelihood).  A layer's fp32 contraction over ~1e3 products is off by about sqrt(1e3) u = 2e-6 (u = 2^-24) of its operand
    magnitudes; added up linearly (not in quadrature) over 30 layers that is at most ~6e-5 on a single term.  The errors of the terms are
    not aligned, so the sum averages them down by sqrt(256) = 16 or more: ~4e-6, and the summation itself adds a few u.  The bound is
    1e-5: an fp16 operand rounding anywhere in the rate path (2^-11 = 5e-4 per term) cannot pass it.
    Measured on MI355X: e32 = 5.99e-05, e16 = 1.43e-02."""
    from oracle.tdvc_ref import coder as oc
    from tdvc_amd import autograd, ops, synth
    from tdvc_amd.model import coder as dc
    ref = oc.MVCoder(128)
    synth.fill_parameters(ref)
    dev = dc.MVCoder(128)
    dev.load_state_dict(ref.state_dict())
    dev = dev.cuda().train()
    ref.train()
    B, H, W = 2, 64, 64
    g = torch.Generator().manual_seed(61)
    x = rnd16(torch.randn(B, 64, H, W, generator=g) * 0.5)
    u = lambda *s: torch.rand(*s, generator=g) - 0.5
    noise = {"z": u(B, 128, H // 64, W // 64), "y": u(B, 128, H // 16, W // 16), "y_lik": u(B, 128, H // 16, W // 16)}
    wgt = randn(B, 64, H, W, seed=62)
    kappa = 50.0
    o = ref(x, noise)
    bits = sum((-torch.log2(l)).sum() for l in o["likelihoods"].values())
    ((o["x_hat"] * wgt).sum() + kappa * bits).backward()
    bref = torch.stack([(-torch.log2(o["likelihoods"][k])).sum() for k in ("y", "z")]).double().detach()
    names = [k for k, q in ref.named_parameters() if q.grad is not None and not k.endswith(".quantiles")]
    gref = torch.cat([dict(ref.named_parameters())[k].grad.reshape(-1) for k in names])

    def device_grads(f32):
        for p in dev.parameters():
            p.grad = None
        with autograd.record() as tape:
            xf = to_fm(x, ops)
            nf = {k: to_fm(v, ops, Cpad=128, dtype=torch.float32) for k, v in noise.items()}
            x_hat, dbits = dev.run(xf, training=True, noise=nf, f32=f32)
            assert not x_hat.f32                                    # x_hat re-enters the fp16 path whatever the coder's precision
            ops.copy_cast(to_fm(wgt, ops), tape.grad(x_hat))
            tape.rate_grad = kappa
            tape.backward()
        torch.cuda.synchronize()
        named = dict(dev.named_parameters())
        assert all(named[k].grad is not None for k in names)
        return torch.cat([named[k].grad.reshape(-1).cpu() for k in names]), dbits.cpu()

    g32, b32 = device_grads(True)
    g16, b16 = device_grads(False)
    e32, e16 = _rel(g32, gref), _rel(g16, gref)
    eb32 = float(((b32 - bref).abs() / bref).max())
    eb16 = float(((b16 - bref).abs() / bref).max())
    report(f"fp32-coder gradient parity (MVCoder, 2x64x64, {gref.numel()} values): rel L2 err of the full parameter gradient "
           f"e32 = {e32:.3e}, e16 = {e16:.3e} (ratio {e16 / max(e32, 1e-30):.1f}); bits rel err fp32 {eb32:.3e}, fp16-in {eb16:.3e}")
    assert eb32 < 1e-5, f"rate terms: device {b32.tolist()} oracle {bref.tolist()}"
    assert e32 <= e16 / 8, f"e32 = {e32:.3e}, e16 = {e16:.3e}"


# ------------------------------------------------------------------------------------------------------------------ 2. + 4. steps
_RUNS = {}


def _three_steps(tag):
    """a fresh model, seed 1111, three coder_fp32 steps at 2 x 64 x 64 (the last one profiled); cached per tag"""
    if tag in _RUNS:
        return _RUNS[tag]
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    x, refs = _sample()
    torch.manual_seed(1111)
    ops.DETERMINISTIC = True
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            net = _fresh_model()
            before = {k: v.detach().clone() for k, v in net.named_parameters()}
            step = TrainStep(net, train_lambda=256.0, lr=2e-4, loss_scale=128.0, coder_fp32=True)
            logs = [dict(step(x, refs)) for _ in range(2)]
            ops.PROFILE = []
            try:
                logs.append(dict(step(x, refs)))
                torch.cuda.synchronize()
                prof = [(e["kernel"], e["shape"]) for e in ops.PROFILE]
            finally:
                ops.PROFILE = None
    finally:
        ops.DETERMINISTIC = False
    after = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _RUNS[tag] = dict(net=net, before=before, after=after, logs=logs, prof=prof, warned=[str(w.message) for w in caught])
    return _RUNS[tag]


def test_train_step_with_fp32_coders(report):
    """fails without the feature (TrainStep has no `coder_fp32`; a taped conv on an fp32 map raised): three steps, finite log, every coder
    parameter moved, no fp32-training warning, and the coders' convs / weight gradients on the fp32 kernels only"""
    from tdvc_amd import autograd, ops
    from tdvc_amd.model import coder as dc
    from tdvc_amd import synth
    r = _three_steps("a")
    for log in r["logs"]:
        assert not log["skipped"]
        for k in ("rd_loss", "mse", "bpp_res", "bpp_mv", "aux_loss", "grad_norm"):
            assert log[k] == log[k] and abs(log[k]) != float("inf"), (k, log)
    same = [k for k, v in r["before"].items() if k.startswith(("mvCoder.", "resCoder.")) and torch.equal(v, r["after"][k])]
    assert not same, f"coder parameters that did not move in three steps: {same[:6]}"
    assert not [m for m in r["warned"] if "fp32" in m], r["warned"]
    assert r["net"].train_coder_fp32 is True
    # one coder alone under the tape, fp32: EVERY conv and weight gradient it launches is an fp32 kernel ...
    cd = dc.MVCoder(128)
    synth.fill_parameters(cd)
    cd = cd.cuda().train()
    ops.PROFILE = []
    try:
        with autograd.record() as tape:
            x_hat, _ = cd.run(to_fm(rnd16(randn(2, 64, 64, 64, seed=5) * 0.5), ops), training=True, f32=True)
            tape.grad(x_hat).t.fill_(1.0 / 64)
            tape.rate_grad = 1.0
            tape.backward()
        torch.cuda.synchronize()
        alone = [e["kernel"] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert set(alone) == {"conv_f32", "conv_wgrad_f32"}, sorted(set(alone))
    n_conv, n_wg = alone.count("conv_f32"), alone.count("conv_wgrad_f32")
    # ... and the whole model's step runs exactly two coders' worth of them: no coder layer is left on an fp16 kernel
    kernels = [k for k, _ in r["prof"]]
    report(f"coder_fp32 step at 2x64x64: {kernels.count('conv_f32')} conv_f32 + {kernels.count('conv_wgrad_f32')} conv_wgrad_f32 launches "
           f"(one coder alone: {n_conv} + {n_wg}); fp16 conv / wgrad launches of the rest of the model: "
           f"{sum(1 for k in kernels if k not in ('conv_f32', 'conv_wgrad_f32'))}; rd_loss {[round(l['rd_loss'], 4) for l in r['logs']]}")
    # one weight gradient per conv layer and per GDN of the coder (the SE layers' two 1x1 convs are part of the gate kernel)
    from tdvc_amd.model.modules import ConvAct
    se_convs = {id(m.conv) for m in cd.modules() if isinstance(m, ConvAct)}
    n_layers = sum(1 for m in cd.modules() if (isinstance(m, torch.nn.Conv2d) and id(m) not in se_convs) or isinstance(m, dc.GDN))
    assert n_wg == n_layers, (n_wg, n_layers)
    assert kernels.count("conv_wgrad_f32") == 2 * n_wg and kernels.count("conv_f32") == 2 * n_conv


def test_fp32_coder_steps_are_reproducible(report):
    """the same seed and the same three steps, from scratch, twice: bit-identical parameters and losses"""
    a, b = _three_steps("a"), _three_steps("b")
    bad = [k for k in a["after"] if not torch.equal(a["after"][k], b["after"][k])]
    report(f"3 coder_fp32 steps at 2x64x64, twice: {len(bad)}/{len(a['after'])} state tensors differ")
    assert not bad, f"fp32-coder training is not reproducible run to run: {bad[:4]}"
    assert [l["rd_loss"] for l in a["logs"]] == [l["rd_loss"] for l in b["logs"]]


# ------------------------------------------------------------------------------------------------------------------ 3. re-pack
def test_fp32_twins_follow_the_optimizer(report):
    """after one coder_fp32 step the model's fp32-island inference equals that of a fresh model loaded with the stepped state: a stale
    fp32 weight twin (forward or dgrad form, GDN, plain stride-2 form) would show here"""
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.train import TrainStep
    x, refs = _sample()
    torch.manual_seed(7)
    net = _fresh_model()
    step = TrainStep(net, train_lambda=256.0, lr=1e-3, loss_scale=128.0, coder_fp32=True)
    assert not step(x, refs)["skipped"]
    net.eval()
    net.coder_fp32 = True
    fresh = VideoCompressor()
    fresh.load_state_dict(net.state_dict())
    fresh = fresh.cuda().eval()
    fresh.coder_fp32 = True
    with torch.no_grad():
        got, want = net(x, refs, True), fresh(x, refs, True)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (p, q) in enumerate(zip(got, want)):
        assert torch.equal(p, q), f"output {i} of the stepped model differs from a fresh model with the same state"
    report("fp32 twins after an optimizer step: fp32-island inference bit-identical to a freshly packed model")


def _forms(net):
    """every PackedConv of the model with the forms that hang off it: [(name, form)]"""
    from tdvc_amd import ops
    out, seen = [], set()

    def walk(name, pc):
        if pc is None or id(pc) in seen:
            return
        seen.add(id(pc))
        out.append((name, pc))
        walk(name + " dgrad", pc.dgrad)
        walk(name + " plain", pc.plain)
        walk(name + " column", pc.column)
    for mname, m in net.named_modules():
        for key, pc in m.__dict__.get("_packed", {}).items():
            if isinstance(pc, ops.PackedConv):
                walk(f"{mname}[{key}]", pc)
    return out


def _assert_forms_current(net):
    """the packed fp16 blob of EVERY form, and the fp32 twin of every form that has one, equal a fresh packing of the live weights"""
    from tdvc_amd import ops
    forms = _forms(net)
    twins = 0
    for name, pc in forms:
        assert torch.equal(pc.w, ops._pack_from_tables(pc.wsrc, pc.tables)), f"{name}: stale fp16 packing"
        if pc.w32 is not None or pc.w32_buf is not None:
            twins += 1
            assert torch.equal(pc.packed_f32(), ops._pack_from_tables_f32(pc.wsrc, pc.tables)), f"{name}: stale fp32 twin"
    return len(forms), twins


def _assert_dgrads_current(coder):
    """the fp32 data gradient of every layer of a coder that has taken a backward pass, on a small random dY, against the same layer
    with its dgrad form packed afresh from the live weights: bit-identical.  (An eval forward runs no dgrad conv.)"""
    import dataclasses
    from tdvc_amd import ops
    n = 0
    for name, pc in _forms(coder):
        if pc.dgrad is None or " " in name:                 # the layers themselves, not the forms that hang off them
            continue
        s = pc.orig["stride"]
        xc = pc.dgrad.cout // (4 if s == 2 else 1)
        g = to_fm(randn(1, pc.dgrad.cin, 3, 5, seed=900 + n), ops, dtype=torch.float32)
        fresh = dataclasses.replace(pc, dgrad=None, w32=None, w32_buf=None)
        got = ops.conv_dgrad(pc, g, ops.FM.empty(1, 3 * s, 5 * s, xc, dtype=torch.float32, device="cuda"), accumulate=False)
        want = ops.conv_dgrad(fresh, g, ops.FM.empty(1, 3 * s, 5 * s, xc, dtype=torch.float32, device="cuda"), accumulate=False)
        assert fresh.dgrad is not None and fresh.dgrad is not pc.dgrad
        assert torch.equal(got.t[..., :xc], want.t[..., :xc]), f"{name}: fp32 data gradient from a stale dgrad twin"
        assert float(want.t[..., :xc].abs().max()) > 0
        n += 1
    torch.cuda.synchronize()
    return n


def test_fp32_dgrad_twins_follow_the_optimizer(report):
    """two coder_fp32 steps, then every form of the model against a fresh packing and the fp32 data gradient of every coder layer
    against a freshly packed dgrad form"""
    from tdvc_amd.train import TrainStep
    x, refs = _sample()
    torch.manual_seed(8)
    net = _fresh_model()
    step = TrainStep(net, train_lambda=256.0, lr=1e-3, loss_scale=128.0, coder_fp32=True)
    assert not step(x, refs)["skipped"] and not step(x, refs)["skipped"]
    nforms, ntwins = _assert_forms_current(net)
    nd = _assert_dgrads_current(net.mvCoder) + _assert_dgrads_current(net.resCoder)
    report(f"after 2 coder_fp32 steps: {nforms} packed forms and {ntwins} fp32 twins equal a fresh packing; "
           f"{nd} fp32 layer data gradients equal those of freshly packed dgrad forms")
    assert ntwins >= 2 * 30 and nd >= 2 * 30


def test_switching_a_trained_model_to_fp32_coders(report):
    """default steps first, at a size where the stride-2 3x3 layers run in space-to-depth form (1 x 96 x 96 = 9216 half-resolution pixels
    > ops.SMALL_MAP_PIXELS), so their plain form -- the one fp32 uses -- does not exist when the model's batched re-pack is built.  Then
    coder_fp32 steps on the same model: the forms created late must follow the optimizer like all others.  Checked three ways: every
    form against a fresh packing, the coders' fp32 data gradients against fresh dgrad forms, and the fp32-island inference against a
    fresh model with the stepped state."""
    from tdvc_amd import ops
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.train import TrainStep
    x, refs = _sample(B=1, H=192, W=192)
    assert x.shape[0] * (x.shape[2] // 2) * (x.shape[3] // 2) > ops.SMALL_MAP_PIXELS
    torch.manual_seed(9)
    net = _fresh_model()
    step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0)
    assert not step(x, refs)["skipped"]
    batch = net.__dict__["_pack_batch"]
    assert not step(x, refs)["skipped"]
    assert net.__dict__["_pack_batch"] is batch, "a default-mode step rebuilt the batched re-pack although no layer form was new"
    late = [n for n, pc in _forms(net.mvCoder) + _forms(net.resCoder) if pc.s2d and pc.plain is None]
    assert late, "no coder layer is in space-to-depth form only: the case this test is about does not occur at this size"
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0, coder_fp32=True)
        assert not step(x, refs)["skipped"]
        rebuilt = net.__dict__["_pack_batch"]
        assert rebuilt is not batch and len(rebuilt.pcs) > len(batch.pcs)
        assert not step(x, refs)["skipped"]
        assert net.__dict__["_pack_batch"] is rebuilt
    assert not [str(w.message) for w in caught if "fp32" in str(w.message)]
    nforms, ntwins = _assert_forms_current(net)
    nd = _assert_dgrads_current(net.mvCoder) + _assert_dgrads_current(net.resCoder)
    net.eval()
    net.coder_fp32 = True
    fresh = VideoCompressor()
    fresh.load_state_dict(net.state_dict())
    fresh = fresh.cuda().eval()
    fresh.coder_fp32 = True
    with torch.no_grad():
        got, want = net(x, refs, True), fresh(x, refs, True)
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(got, want)):
        assert torch.equal(p, q), f"output {i}: the model switched to fp32 coders mid-training differs from a fresh model with its state"
    report(f"2 default + 2 coder_fp32 steps at 1x192x192: {len(late)} coder layers got their plain form after the switch; "
           f"{nforms} forms / {ntwins} fp32 twins / {nd} fp32 data gradients current; fp32-island inference equals a fresh model")


# ------------------------------------------------------------------------------------------------------------------ 5. default untouched
def test_default_training_mode_is_untouched(report):
    from tdvc_amd import ops
    from tdvc_amd.train import TrainStep
    assert inspect.signature(TrainStep.__init__).parameters["coder_fp32"].default is False
    x, refs = _sample()
    net = _fresh_model()
    assert net.train_coder_fp32 is False
    B, H, W = x.shape[0], 64, 64
    gen = torch.Generator().manual_seed(71)
    u = lambda *s: torch.rand(*s, generator=gen) - 0.5
    mk = lambda: {"z": u(B, 128, H // 64, W // 64), "y": u(B, 128, H // 16, W // 16), "y_lik": u(B, 128, H // 16, W // 16)}
    nf = {k: {kk: to_fm(v, ops, Cpad=128, dtype=torch.float32) for kk, v in mk().items()} for k in ("mv", "res")}
    with torch.no_grad():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            a = net(x, refs, False, noise=nf)
        assert [w for w in caught if "fp32-island coders are an inference / coding mode" in str(w.message)], [str(w.message) for w in caught]
        b = net(x, refs, True, noise=nf)
    for p, q in zip(a[:3], b[:3]):
        assert torch.equal(p, q)
    # a default TrainStep never packs an fp32 twin
    calls = []
    orig = ops._pack_from_tables_f32

    def counting(*args, **kw):
        calls.append(1)
        return orig(*args, **kw)
    ops._pack_from_tables_f32 = counting
    try:
        step = TrainStep(net, train_lambda=256.0, lr=1e-4, loss_scale=128.0)
        assert net.train_coder_fp32 is False
        logs = [step(x, refs) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        ops._pack_from_tables_f32 = orig
    assert all(l["rd_loss"] == l["rd_loss"] for l in logs)
    assert not calls, f"a default-mode training step packed {len(calls)} fp32 weight twins"
    report("default training mode: enabled_amp=False still warns and equals enabled_amp=True; no fp32 twin packed in 2 default steps")


def test_graph_capture_is_refused_at_construction():
    from tdvc_amd.train import TrainStep
    net = _fresh_model()
    with pytest.raises(ValueError, match="coder_fp32=True is not supported with graph=True"):
        TrainStep(net, coder_fp32=True, graph=True)
    assert net.train_coder_fp32 is False
