"""Output bytes of the model layer (tdvc_amd/model: LoopFilter.run, VideoCompressor.forward / encode / decode, TrainStep) on fixed-seed
inputs from tdvc_amd.synth: one line `digest <case> <sha256>` per case, the launch list of every LoopFilter path at B = 1 (`launch ...`),
then the SHA-256 of all those lines.  Run it once per tree, each in a process of its own, both with the same built library (TDVC_LIB=path),
and compare the lists: equal lists mean equal bytes and equal launch lists.
  python tools/ab_model_bytes.py > tree.txt;  (cd /path/to/parent/worktree && TDVC_LIB=/path/to/libtdvc_hip.so python tools/ab_model_bytes.py) > parent.txt
It imports the tree it stands in, and only names every tree since the LoopFilter tail has.  `--only lf,forward,codec,train` picks cases.
Cases: (1) LoopFilter.run over the twelve-call reference sequence of tests/test_loopfilter_reuse_gpu.py at 64x128, 65x131 (the fused
forms) and 64x64 (the unfused form), B = 1, 2, under every setting of LOOPFILTER_REUSE / _TAIL / _PAIR / _BCAST and once under ops.PROFILE:
`out`, and `out` + `out3` with then= given; (2) an eval forward over 7-frame GOPs at 64x128, FEATUREFIX_REUSE on and off; (3) encode() and
decode() in the three stream orders, B = 1, 2; (4) two TrainStep iterations under ops.DETERMINISTIC, default and model_fp32."""
import argparse
import hashlib
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import _lib as L  # noqa: E402

if os.environ.get("TDVC_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["TDVC_LIB"])
from tdvc_amd import ops  # noqa: E402
from tdvc_amd.model import VideoCompressor  # noqa: E402
from tdvc_amd.model import modules as M  # noqa: E402
from tdvc_amd.synth import fill_parameters, make_gop, ref_list  # noqa: E402

LINES = []


def line(text):
    LINES.append(text)
    print(text, flush=True)


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t if isinstance(t, bytes) else t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def fm_bytes(fm):
    """the words of an FM view, (N, H, W, C), as a dense copy"""
    return torch.as_strided(fm.t.reshape(-1), (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.off).clone()


def rnd16(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half().cuda()


# ---- (1) LoopFilter.run, every path, with its launch list
LAUNCHES = None           # a list while a LoopFilter call is being recorded


def _wrap(name, is_conv=False):
    plain = getattr(ops, name)

    def f(*args, **kw):
        r = plain(*args, **kw)
        if LAUNCHES is not None:
            LAUNCHES.append(name + (" " + L.lib().tdvc_last_conv_kernel().decode() if is_conv else ""))
        return r
    setattr(ops, name, f)


def _ref_slices(refs):
    """[r-3, r-2, r-1] by synth.ref_list"""
    return [refs[0]] * 3 if len(refs) == 1 else ([refs[-2], refs[-1], refs[-1]] if len(refs) == 2 else refs[-3:])


def lf_calls():
    """the twelve calls of test_loopfilter_reuse_bit_identical as lists of frame ids"""
    ids = {"I0": 0, "x0.1": 1, "x0.2": 2, "x0.3": 3, "x0.4": 4, "I1": 5, "x1.1": 6, "x1.2": 7, "S": 8, "u1": 9, "u2": 10, "u3": 11}
    calls = []
    for g, nframes in ((0, 6), (1, 4)):
        refs = [f"I{g}"]
        for t in range(1, nframes):
            calls.append(_ref_slices(refs))
            refs.append(f"x{g}.{t}")
    calls += [["S", "S", "S"]] * 3 + [["u1", "u2", "u3"]]
    return [[ids[k] for k in c] for c in calls]


def case_lf():
    global LAUNCHES
    for name in ("conv", "conv_pair", "lf_tail", "bcast_add_act", "frames_changed"):
        _wrap(name, is_conv=name == "conv")
    lf = M.LoopFilter()
    fill_parameters(lf)
    lf = lf.cuda().eval()
    calls = lf_calls()
    saved = (M.LOOPFILTER_REUSE, M.LOOPFILTER_TAIL, M.LOOPFILTER_PAIR, M.LOOPFILTER_BCAST)
    settings = [s + (False,) for s in itertools.product((True, False), repeat=4)] + [(True, True, True, True, True)]
    for (H, W) in ((64, 128), (65, 131), (64, 64)):
        for B in (1, 2):
            pools = [make_gop(77 + b, 12, H, W) for b in range(B)]
            stacks = [ops.from_nchw(torch.cat([torch.stack([pools[b][0]] + [pools[b][k] for k in want]) for b in range(B)]).cuda(), Cpad=8) for want in calls]
            xts = [rnd16(B, H, W, 256, seed=200 + i, scale=0.5) for i in range(len(calls))]
            fcur = ops.FM(rnd16(B, H, W, 64, seed=300, scale=0.5))
            for reuse, tail, pair, bcast, profile in settings:
                M.LOOPFILTER_REUSE, M.LOOPFILTER_TAIL, M.LOOPFILTER_PAIR, M.LOOPFILTER_BCAST = reuse, tail, pair, bcast
                tag = f"lf {H}x{W} B{B} reuse{int(reuse)} tail{int(tail)} pair{int(pair)} bcast{int(bcast)}" + (" profile" if profile else "")
                for with_then in (False, True):
                    lf.__dict__.pop("_packed", None)
                    outs, record = [], []
                    ops.PROFILE = [] if profile else None
                    try:
                        for i in range(len(calls)):
                            out, out3 = ops.FM.empty(B, H, W, 64), ops.FM.empty(B, H, W, 64)
                            LAUNCHES = []
                            lf.run(ops.FM(xts[i].clone()), stacks[i], out, then=(fcur, -1.0, out3) if with_then else None)
                            record.append(LAUNCHES)
                            LAUNCHES = None
                            outs += [fm_bytes(out)] + ([fm_bytes(out3)] if with_then else [])
                    finally:
                        ops.PROFILE = None
                    line(f"digest {tag} {'out+out3' if with_then else 'out'} {sha(*outs)}")
                    if with_then:
                        continue
                    if B == 1:                    # the launch list: calls 1 and 2 in full, the twelve calls as a hash
                        for i in (0, 1):
                            for k, what in enumerate(record[i]):
                                line(f"launch {tag} call{i + 1} {k:2d} {what}")
                        line(f"launches {tag} 12 calls {hashlib.sha256(repr(record).encode()).hexdigest()}")
                    else:                         # the conv launches in front of feat_fusion set its walk direction
                        line(f"convs {tag} {[sum(w.startswith('conv ') for w in r) for r in record]}")
    M.LOOPFILTER_REUSE, M.LOOPFILTER_TAIL, M.LOOPFILTER_PAIR, M.LOOPFILTER_BCAST = saved


# ---- (2) eval forward over GOPs
def model():
    m = VideoCompressor()
    fill_parameters(m)
    return m.cuda().eval()


def case_forward():
    m = model()
    saved = M.FEATUREFIX_REUSE
    for B, ngops in ((1, 2), (2, 1)):
        gops = [torch.stack([make_gop(4321 + 10 * k + b, 7, 64, 128) for b in range(B)]).cuda() for k in range(ngops)]      # (B, T, 3, H, W)
        for ff in (True, False):
            M.FEATUREFIX_REUSE = ff
            m.clear_packed()
            with torch.no_grad():
                for k, g in enumerate(gops):
                    refs = [g[:, 0]]
                    for t in range(1, 7):
                        recon, bpp_res, bpp_mv = m(g[:, t], ref_list(refs), True)
                        refs.append(recon)
                        line(f"digest forward 64x128 B{B} featurefix_reuse{int(ff)} gop{k} frame{t} {sha(recon, bpp_res, bpp_mv)}")
    M.FEATUREFIX_REUSE = saved


# ---- (3) encode / decode
def case_codec():
    m = model()
    for (H, W) in ((64, 64), (64, 128)):
        for B in (1, 2):
            g = torch.stack([make_gop(1234 + 17 * b, 3, H, W) for b in range(B)]).cuda()
            rl, x = ref_list([g[:, 0], g[:, 1]]), g[:, 2]
            for order in ("raster", "wavefront", "lanes"):
                m.stream_order = order
                enc = m.encode(x, rl)
                dec = m.decode(enc["strings"], enc["shapes"], rl)
                tag = f"codec {H}x{W} B{B} {order}"
                for name, strs in zip(("mv_y", "mv_z", "res_y", "res_z"), enc["strings"]):
                    line(f"digest {tag} strings {name} {len(strs)} {sha(*[bytes(s) for s in strs])}")
                line(f"digest {tag} shapes {[tuple(s) for s in enc['shapes']]}")
                line(f"digest {tag} recon {tuple(enc['recon'].shape)} {sha(enc['recon'])}")
                line(f"digest {tag} decoded {tuple(dec.shape)} {sha(dec)}")


# ---- (4) training steps
def case_train():
    from tdvc_amd.train import TrainStep
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, True
    try:
        g = torch.stack([make_gop(1234 + 17 * b, 4, 64, 64) for b in range(2)]).cuda()
        x, refs = g[:, 3], torch.stack([g[:, 0], g[:, 0], g[:, 1], g[:, 2]], 1)
        for fp32 in (False, True):
            torch.manual_seed(0)
            net = VideoCompressor()
            fill_parameters(net)
            net = net.cuda().train()
            step = TrainStep(net, train_lambda=2048.0, lr=1e-4, **(dict(model_fp32=True) if fp32 else {}))
            for it in range(2):
                log = dict(step(x, refs))
                tag = f"train 64x64 B2 {'model_fp32' if fp32 else 'default'} step{it + 1}"
                line(f"digest {tag} log {' '.join(f'{k}={log[k]!r}' for k in sorted(log))}")
                grads = [p.grad if p.grad is not None else torch.zeros(0) for _, p in net.named_parameters()]
                line(f"digest {tag} grads {sum(p.grad is not None for p in net.parameters())} {sha(*grads)}")
    finally:
        ops.DETERMINISTIC = prev


CASES = {"lf": case_lf, "forward": case_forward, "codec": case_codec, "train": case_train}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(CASES))
    for name in ap.parse_args().only.split(","):
        CASES[name]()
    print(f"{len(LINES)} lines, digest of the list {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
