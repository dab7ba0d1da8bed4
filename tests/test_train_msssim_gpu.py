"""GPU: TrainStep(distortion=...): MS-SSIM as the training distortion (the reference's commented
`rd_loss = train_lambda * msssim + bpp`, tools/train.py:133,139), the callable hook, and the unchanged "mse" default.
B = 1 at 192x192 (the smallest multiple of 64 whose fifth pyramid level still holds the 11-tap window), seeded model,
synthetic frames."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 192
LAM = 32.0


def sample(size=H):
    from tdvc_amd import synth
    gop = synth.make_gop(4321, 7, size, size).float()
    return gop[3:4].cuda(), torch.stack([gop[0], gop[0], gop[1], gop[2]]).unsqueeze(0).cuda()


def msssim_hook(recon, target):
    """what distortion="ms-ssim" is documented to be, built on the public function"""
    from tdvc_amd import metrics
    n = recon.shape[0]
    ms, g = metrics.ms_ssim_value_and_grad(recon, target, data_range=1.0, grad_out=torch.full((n,), -1.0 / n, dtype=torch.float32, device=recon.device))
    return 1.0 - ms.mean(), g


def mse_hook(recon, target):
    diff = recon - target
    return (diff * diff).mean(), diff * (2.0 / diff.numel())


def run(distortion, steps, lam=LAM, deterministic=True, **kw):
    """-> (state dict, [log as a plain dict]) after `steps` steps on one sample; deterministic: the reproducible form of the DCN
    backward (it reads a counter on the host, so not under graph capture)"""
    from tdvc_amd import ops, synth
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.train import TrainStep
    x, refs = sample()
    torch.manual_seed(5)
    ops.DETERMINISTIC = deterministic
    try:
        m = VideoCompressor()
        synth.fill_parameters(m)
        m = m.cuda()
        step = TrainStep(m, train_lambda=lam, lr=1e-4, loss_scale=128.0, distortion=distortion, **kw)
        logs = [dict(step(x, refs)) for _ in range(steps)]
        torch.cuda.synchronize()
    finally:
        ops.DETERMINISTIC = False
    run.last_step = step
    return {k: v.detach().clone() for k, v in m.state_dict().items()}, logs


@functools.lru_cache(maxsize=None)
def builtin_two_steps():
    return run("ms-ssim", 2)


def same_logs(a, b):
    return all(set(p) == set(q) and all(p[k] == q[k] or (p[k] != p[k] and q[k] != q[k]) for k in p) for p, q in zip(a, b))


def test_builtin_mode_and_hook_are_one_path(report):
    sa, la = builtin_two_steps()
    sb, lb = run(msssim_hook, 2)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    report(f"ms-ssim training, built-in vs hook, 2 steps at 1x{H}x{W}: {len(bad)}/{len(sa)} state tensors differ; "
           f"rd_loss {[round(l['rd_loss'], 4) for l in la]} distortion {[round(l['distortion'], 5) for l in la]}")
    assert not bad, bad[:4]
    assert same_logs(la, lb), (la, lb)
    assert all(not l["skipped"] and 0.0 < l["distortion"] < 1.0 for l in la)


def test_two_fresh_runs_are_bit_identical():
    sa, la = builtin_two_steps()
    sb, lb = run("ms-ssim", 2)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, f"ms-ssim training is not reproducible run to run: {len(bad)} tensors differ, e.g. {bad[:4]}"
    assert same_logs(la, lb)


def test_mse_hook_matches_mse_mode(report):
    """a lost factor of lambda, loss_scale, 2 or 1 / numel in the hook's seeding shows as >= 2x; the rounding of the seed
    (two fp32 roundings per element against one) is orders of magnitude below the 1e-2 asked for here"""
    from tdvc_amd.train import StepLog
    _, (a,) = run("mse", 1, lam=2048.0)
    _, (b,) = run(mse_hook, 1, lam=2048.0)
    report(f"mse mode vs mse hook, first step: rd_loss {a['rd_loss']:.6f} / {b['rd_loss']:.6f}, grad_norm {a['grad_norm']:.6e} / {b['grad_norm']:.6e}")
    assert "distortion" not in a and set(a) == set(StepLog.KEYS) and len(a) == len(StepLog.KEYS)
    assert set(b) == set(StepLog.KEYS) | {"distortion"}
    assert abs(a["rd_loss"] - b["rd_loss"]) <= 1e-2 * abs(a["rd_loss"])
    assert abs(a["grad_norm"] - b["grad_norm"]) <= 1e-2 * abs(a["grad_norm"])
    assert abs(b["distortion"] - b["mse"]) <= 1e-5 * b["mse"]


def test_log_identities(report):
    """rd_loss = lambda * D + bpp_res + bpp_mv to fp32 rounding, and 1 - D is metrics.ms_ssim of the step's own reconstruction:
    the recon and target the TAPE holds, captured by a hook that otherwise is the built-in distortion (the first test shows
    the two are one path, logs included)"""
    from tdvc_amd import metrics
    seen = []

    def hook(recon, target):
        seen.append((recon.detach().clone(), target.detach().clone()))
        return msssim_hook(recon, target)

    _, (log,) = run(hook, 1)
    _, la = builtin_two_steps()
    assert log == la[0] or same_logs([log], la[:1])
    eps = 2.0 ** -23
    terms = (LAM * log["distortion"], log["bpp_res"], log["bpp_mv"])
    assert abs(log["rd_loss"] - sum(terms)) <= 4 * eps * sum(abs(t) for t in terms), (log, terms)
    recon, target = seen[0]
    ms = float(metrics.ms_ssim(recon, target, data_range=1.0))
    report(f"ms-ssim step log: distortion {log['distortion']:.7f}, 1 - ms_ssim(recon, input) {1 - ms:.7f}, mse {log['mse']:.6f}")
    assert abs((1.0 - log["distortion"]) - ms) <= 2 * eps
    assert 0.0 < log["mse"] < 1.0


def test_graph_replay_matches_eager(report):
    """the tolerance of tests/test_autograd_gpu.py::test_train_step_graph_replay_matches_eager (the noise draws differ): 5 %.
    graph_warmup=1 is raised to TrainStep's minimum of two eager steps, so the third step is the captured and replayed one"""
    _, eager = run("ms-ssim", 3, deterministic=False)
    _, graph = run("ms-ssim", 3, deterministic=False, graph=True, graph_warmup=1)
    report("ms-ssim train step, eager vs graph replay: " + "; ".join(f"{a['rd_loss']:.4f}/{b['rd_loss']:.4f}" for a, b in zip(eager, graph)))
    assert len(graph) == 3 and run.last_step._graph is not None
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert not b["skipped"] and 0.0 < b["distortion"] < 1.0
        assert abs(a["rd_loss"] - b["rd_loss"]) <= 0.05 * abs(a["rd_loss"]), (i, a["rd_loss"], b["rd_loss"])


def test_small_input_raises_and_leaves_the_model_alone():
    from tdvc_amd import synth
    from tdvc_amd.model.pnet import VideoCompressor
    from tdvc_amd.train import TrainStep
    x, refs = sample(128)
    torch.manual_seed(5)
    m = VideoCompressor()
    synth.fill_parameters(m)
    m = m.cuda()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = TrainStep(m, train_lambda=LAM, loss_scale=128.0, distortion="ms-ssim")
    with pytest.raises(ValueError):
        step(x, refs)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())
