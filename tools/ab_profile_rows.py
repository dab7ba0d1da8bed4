"""The ops.PROFILE row lists of the tree this file stands in, as (kernel, shape, flops, flops_real, bytes, geo) per row: a profiled eval
forward and a profiled TrainStep at 1 x 64 x 64 in the default, coder_fp32 and model_fp32 modes, and one profiled conv_pair call at its
smallest supported map (no model path runs it under PROFILE).  Run it once per tree, each in a process of its own, both with the same
built library (TDVC_LIB=path), and compare the lists: equal lists mean the same rows in the same order.
  python tools/ab_profile_rows.py tree.txt;  (cd /path/to/parent/worktree && TDVC_LIB=/path/to/libtdvc_hip.so python tools/ab_profile_rows.py parent.txt)"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import _lib as L  # noqa: E402

if os.environ.get("TDVC_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["TDVC_LIB"])
from tdvc_amd import ops  # noqa: E402
from tdvc_amd.model import VideoCompressor  # noqa: E402
from tdvc_amd.synth import fill_parameters, make_gop, ref_list  # noqa: E402
from tdvc_amd.train import TrainStep  # noqa: E402

print("ops from", ops.__file__, "lib", L.LIB_PATH, flush=True)
LINES = []


def rows(tag, prof):
    for i, r in enumerate(prof):
        assert list(r)[:7] == ["kernel", "shape", "e0", "e1", "flops", "flops_real", "bytes"] and set(r) <= {"kernel", "shape", "e0", "e1", "flops", "flops_real", "bytes", "geo"}, list(r)
        assert r["e0"].elapsed_time(r["e1"]) >= 0
        LINES.append(f"{tag} {i} {(r['kernel'], r['shape'], r['flops'], r['flops_real'], r['bytes'], r.get('geo'))!r}")
    h = hashlib.sha256("\n".join(l for l in LINES if l.startswith(tag + " ")).encode()).hexdigest()
    print(f"rows {tag}: {len(prof)} rows, sha256 {h}", flush=True)


def data():
    g = make_gop(1000, 7, 64, 64).cuda()
    return g[3:4], ref_list([g[0:1], g[1:2], g[2:3]])


def profiled(fn):
    torch.cuda.synchronize()
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return ops.PROFILE
    finally:
        ops.PROFILE = None


x, refs = data()
for mode, kw in (("default", dict(loss_scale=128.0)), ("coder_fp32", dict(loss_scale=128.0, coder_fp32=True)), ("model_fp32", dict(model_fp32=True))):
    torch.manual_seed(0)
    m = VideoCompressor()
    fill_parameters(m)
    m = m.cuda().eval()
    with torch.no_grad():
        m(x, refs, True)
        rows(f"eval-forward[{mode}]", profiled(lambda: m(x, refs, True)))
    m.train()
    step = TrainStep(m, **kw)
    step(x, refs)
    rows(f"trainstep[{mode}]", profiled(lambda: step(x, refs)))
    del step, m

pp = ops.pack_conv_pair(torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(1)).cuda() * 0.05, None,
                        torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(2)).cuda() * 0.05, None)
for H, W in ((1, 1), (2, 2), (4, 4), (8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128)):
    xf = ops.FM(torch.zeros(1, H, W, 64, dtype=torch.float16, device="cuda"))
    if ops.conv_pair_supported(xf):
        rows(f"conv_pair[{H}x{W}]", profiled(lambda: ops.conv_pair(xf, pp)))
        break
else:
    raise SystemExit("no supported conv_pair map found")
print(f"{len(LINES)} rows in all, sha256 {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(LINES) + "\n")
