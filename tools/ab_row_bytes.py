"""Output bytes of the three row-pipeline kernels (csrc/conv_row.hip, lf_tail.hip, conv_pair.hip; shared pieces: csrc/row_pipe.h) on
fixed-seed inputs: one line `digest <case> <sha256>` per output buffer, then the SHA-256 of those lines.  Run it once per build of the
library, each in a process of its own (TDVC_LIB=path loads another build), and compare the lists: equal lists mean equal bytes.
  python tools/ab_row_bytes.py > tree.txt;  TDVC_LIB=/path/to/parent/libtdvc_hip.so python tools/ab_row_bytes.py > parent.txt
Cases: every conv_row and conv_pair case of tests/test_conv_exact_gpu.py (the stored window of every launch: both walk directions and the
forward walk, both strip geometries); all 30 instantiations of conv_row_kernel on random data at 65x131 (two launches each: both walk
directions); lf_tail on the shapes of tests/test_lf_tail_gpu.py with B = 1, 2, dense and as ring windows; conv_pair on random data in both
strip geometries, unpredicated and under per-image predicates."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import _lib as L  # noqa: E402

if os.environ.get("TDVC_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["TDVC_LIB"])
from tdvc_amd import ops  # noqa: E402
from tests import helpers_conv_exact as X  # noqa: E402
from tests import test_conv_exact_gpu as T  # noqa: E402

LINES = []


def digest(case, t):
    torch.cuda.synchronize()
    LINES.append(f"digest {case} {hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()}")
    print(LINES[-1], flush=True)


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half().cuda()


def last():
    return L.lib().tdvc_last_conv_kernel().decode()


# ---- the exact cases: the test's own launches, its check() also records the bytes it compared
_check = T.check


def recording_check(case, d, got, tag, report):
    digest(f"exact {case.id} [{tag}]", got)
    _check(case, d, got, tag, report)


T.check = recording_check
for case in X.CASES:
    if case.kernel.startswith("conv_row"):
        T.test_conv_exact(case, lambda msg: None)
for case in X.PAIR_CASES:
    T.test_conv_pair_exact(case, lambda msg: None)
T._call("tdvc_debug_set_pair_geometry", 0)
T._call("tdvc_debug_set_conv_walk", 1)

# ---- conv_row: geometry x activation x residual x store, random data
H, W = 65, 131
GEOS = [("c128", 128, 128, False), ("c128s", 128, 256, True), ("c64", 64, 64, False), ("c128w", 128, 64, False), ("s2d", 64, 128, False)]
seed = 1000
for name, cin, cout, shuf in GEOS:
    s2d = name == "s2d"
    hin, win = (2 * H, 2 * W) if s2d else (H, W)
    x = ops.FM(rnd(1, hin, win, cin, seed=seed))
    pc = ops.pack_conv(rnd(cout, cin, 3, 3, seed=seed + 1, scale=0.03).float().cpu(), rnd(cout, seed=seed + 2, scale=0.1).float().cpu(),
                       stride=2 if s2d else 1, pad=1, shuffle=shuf)
    oc, oh, ow = (cout // 4, 2 * H, 2 * W) if shuf else (cout, H, W)
    for act, slope in ((ops.ACT_NONE, 0.0), (ops.ACT_RELU, 0.0), (ops.ACT_LRELU, 0.25)):
        for with_res in (False, True):
            res = ops.FM(rnd(1, oh, ow, oc, seed=seed + 3)) if with_res else None
            for launch in (0, 1):
                y = ops.FM(torch.full((1, oh, ow, oc), 7.0, dtype=torch.float16, device="cuda"))
                ops.conv(x, pc, out=y, act=act, slope=slope, res=res)
                assert last().startswith("conv_row"), last()
                digest(f"conv_row {name} act{act} res{int(with_res)} launch{launch}", y.t)
    seed += 10

# ---- lf_tail
pct = ops.pack_conv(rnd(64, 192, 1, 1, seed=71, scale=0.07).float().cpu(), None, stride=1, pad=0)
pc3 = ops.pack_conv(rnd(64, 64, 3, 3, seed=72, scale=0.04).float().cpu(), rnd(64, seed=73, scale=0.1).float().cpu(), stride=1, pad=1)
for (h, w) in ((65, 131), (64, 128), (280, 30), (16, 520)):
    for B in (1, 2):
        S, A = ops.FM(rnd(B, h, w, 256, seed=80 + B)), ops.FM(rnd(B, h, w, 256, seed=90 + B))
        o = ops.FM(torch.full((B, h, w, 320), 7.0, dtype=torch.float16, device="cuda")).ch(32, 256)
        ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
        digest(f"lf_tail dense {h}x{w} B{B}", o.t)
RING = 9
for p in (0, 3, 5):
    for B in (1, 2):
        S = ops.FM(rnd(B, 65, 131, 64 * RING, seed=101 + p)).ch(64 * p, 256)
        A = ops.FM(rnd(B, 65, 131, 64 * RING, seed=102 + p)).ch(64 * p, 256)
        o = ops.FM(torch.full((B, 65, 131, 320), 7.0, dtype=torch.float16, device="cuda")).ch(32, 256)
        ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
        digest(f"lf_tail ring window {p} B{B}", o.t)

# ---- conv_pair: both strip geometries, with and without per-image predicates
w1, w2 = rnd(64, 64, 3, 3, seed=201, scale=0.04), rnd(64, 64, 3, 3, seed=202, scale=0.04)
b1, b2 = rnd(64, seed=203, scale=0.1).float(), rnd(64, seed=204, scale=0.1).float()
pp = ops.pack_conv_pair(w1.float(), b1, w2.float(), b2)
for (N, h, w) in ((1, 100, 131), (4, 65, 131), (2, 64, 160)):
    x, r2 = ops.FM(rnd(N, h, w, 64, seed=210 + N)), ops.FM(rnd(N, h, w, 64, seed=220 + N))
    for geo in (2, 4):
        T._call("tdvc_debug_set_pair_geometry", geo)
        for kw in (dict(act1=ops.ACT_RELU, add_input=True), dict(act1=ops.ACT_RELU, add_input=True, res2=r2), dict(act1=ops.ACT_RELU),
                   dict(act1=ops.ACT_LRELU, slope1=0.2, act2=ops.ACT_LRELU, slope2=0.05), dict(act1=ops.ACT_LRELU, slope1=0.2, act2=ops.ACT_LRELU, slope2=0.05, add_input=True, res2=r2)):
            tag = " ".join(f"{k}={v if not isinstance(v, ops.FM) else 1}" for k, v in kw.items())
            y = ops.FM(torch.full((N, h, w, 64), 7.0, dtype=torch.float16, device="cuda"))
            ops.conv_pair(x, pp, out=y, **kw)
            digest(f"conv_pair N{N} {h}x{w} geo{geo} {tag}", y.t)
            if N > 1:
                for pat in ((1, 0, 1, 1), (0, 0, 1, 0), (1, 1, 1, 1), (0, 1, 0, 0)):
                    flags = torch.tensor(pat[:N], dtype=torch.int32, device="cuda")
                    y = ops.FM(torch.full((N, h, w, 64), 7.0, dtype=torch.float16, device="cuda"))
                    with ops.predicate_images(flags):
                        ops.conv_pair(x, pp, out=y, **kw)
                    digest(f"conv_pair N{N} {h}x{w} geo{geo} {tag} flags{''.join(map(str, pat[:N]))}", y.t)
T._call("tdvc_debug_set_pair_geometry", 0)

print(f"{len(LINES)} lines, digest of the list {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
