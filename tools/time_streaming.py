"""Median time per launch of the streaming kernels that carry the milliseconds of a frame or a training step, at production shapes
(1088 x 1920, 64 channels unless the operator says otherwise).  One process per build of the library (TDVC_LIB=path loads another
build); compare builds in the order parent, parent, branch, parent, branch (profiles/r19_streaming_refactor_ab.txt).
  python tools/time_streaming.py LABEL
10 warm-up launches, then 7 timed loops of 30 launches between two device events; median, fastest and slowest loop."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import _lib as L, ops  # noqa: E402

if os.environ.get("TDVC_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["TDVC_LIB"])
lib = L.lib()
label = sys.argv[1] if len(sys.argv) > 1 else "build"
H, W = 1088, 1920
F16, F32 = torch.float16, torch.float32
torch.manual_seed(0)


def fm(N, h, w, c, dt=F16, pos=False):
    t = torch.randn(N, h, w, c, device="cuda", dtype=F32)
    return ops.FM((t.abs() + 0.5 if pos else t).to(dt))


def P(x):
    if isinstance(x, ops.FM):
        return C.byref(x.desc())
    return x.data_ptr() if isinstance(x, torch.Tensor) else x


def timeit(name, fn, args, loops=7, n=30):
    f = getattr(lib, fn)
    a = [P(x) for x in args] + [ops._stream()]
    for _ in range(10):
        L.check(f(*a), name)
    torch.cuda.synchronize()
    us = []
    for _ in range(loops):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            rc = f(*a)
        e1.record()
        torch.cuda.synchronize()
        L.check(rc, name)
        us.append(e0.elapsed_time(e1) / n * 1e3)
    print(f"time {label} {name}: median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f}  ({loops} loops)", flush=True)


a, r, y = fm(1, H, W, 64), fm(1, H, W, 64), fm(1, H, W, 64)
gate = torch.rand(1, 64, device="cuda")
timeit("scale_act_res16_kernel<4>", "tdvc_scale_act_res", [a, gate, 0, 0.0, r, 1.0, y, None])
partial = torch.empty(1, 1024, 64, device="cuda")
timeit("channel_sum_kernel", "tdvc_channel_sum", [a, partial, 1024])
xs = fm(1, H // 2, W // 2, 64)
timeit("upsample2x_kernel", "tdvc_upsample2x", [xs, y])
ref, supp, flo, fup, cat8 = fm(1, H, W, 4, F32), fm(1, H, W, 4, F32), fm(1, H // 2, W // 2, 2, F32), fm(1, H, W, 2, F32), fm(1, H, W, 8)
timeit("spynet_level_input_kernel<true>", "tdvc_spynet_level_input", [ref, supp, flo, fup, cat8])
scale, hp, wp = 136, 8, 14
nwork = lib.tdvc_avgpool_k_work_floats(1, hp, wp, 64, scale)
work, pooled = torch.empty(nwork, device="cuda"), torch.empty(1, hp, wp, 64, device="cuda")
timeit("avgpool_k (avgpool_k_strip_kernel + final)", "tdvc_avgpool_k", [a, scale, pooled, hp, wp, work, nwork])
nb = ((hp + 3) // 3 + 1) * ((wp + 3) // 3 + 1)
idx = torch.randint(0, nb, (1, nb), dtype=torch.int32).cuda()
cat = fm(1, H, W, 128)
timeit("match_gather_kernel", "tdvc_match_gather", [a, r, idx, scale, hp, wp, cat])
del cat
out = fm(1, H, W, 64)
timeit("act_backward_kernel", "tdvc_act_backward", [a, y, r, 2, 0.1, out])
nwork = lib.tdvc_gate_backward_work_floats(1, 64)
work, dgate = torch.empty(nwork, device="cuda"), torch.zeros(1, 64, device="cuda")
timeit("gate_backward (gate_backward_kernel + reduce)", "tdvc_gate_backward", [a, r, gate, out, dgate, work, nwork])
dx, x2, db = fm(1, H, W, 128), fm(1, H, W, 128), fm(1, H, W, 64)
timeit("bcast_add_act_backward_kernel T=2", "tdvc_bcast_add_act_backward", [dx, x2, db, 0.1])
del dx, x2
for g in (a, fm(1, H // 4, W // 4, 264), fm(4, 256, 256, 64), fm(4, 128, 128, 128)):
    nwork = lib.tdvc_bias_grad_work_floats(g.N, g.C)
    work, dbias = torch.empty(nwork, device="cuda"), torch.zeros(g.C, device="cuda")
    timeit(f"bias_grad {g.N}x{g.H}x{g.W}x{g.C} (channel_sum_wide_kernel + reduce_rows_kernel)", "tdvc_bias_grad", [g, g.C, None, 1.0, dbias, work, nwork])
timeit("scale_act_res16_kernel<4> again", "tdvc_scale_act_res", [a, gate, 0, 0.0, r, 1.0, y, None])
