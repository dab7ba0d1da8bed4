"""Per coder of a 1088 x 1920 P-frame, the time on the launch stream from the end of the analysis transform g_a -- where the rate branch
is forked with modules.RATE_FORK, and where it starts in line without it -- to the end of the synthesis transform g_s: HIP events around
`Cheng2020Anchor.run_g_a`'s return and `run`'s return, the median over the timed frames.  Without the fork the interval holds the rate
branch and g_s one after the other; with it g_s alone, the branch beside it.  Works on any commit that has both methods (an A/B against
a tree without the switch prints the same lines).  python tools/rate_fork_interval.py [frames] [fork: 0 | 1]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import tdvc_amd.model.modules as M  # noqa: E402
from tdvc_amd.model.coder import Cheng2020Anchor  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 12
if len(sys.argv) > 2 and hasattr(M, "RATE_FORK"):
    M.RATE_FORK = sys.argv[2] == "1"
dev = torch.device("cuda:0")
model = bench.build_model(dev)
runner = bench.GopRunner(model, bench.make_inputs(1234, dev))
log = []                                                  # (coder, start event, end event)
run_g_a, run = Cheng2020Anchor.run_g_a, Cheng2020Anchor.run


def timed_g_a(self, x):
    r = run_g_a(self, x)
    self.__dict__["_t_fork"] = e = torch.cuda.Event(enable_timing=True)
    e.record()
    return r


def timed_run(self, *a, **kw):
    r = run(self, *a, **kw)
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    log.append((type(self).__name__, self.__dict__["_t_fork"], e))
    return r


Cheng2020Anchor.run_g_a, Cheng2020Anchor.run = timed_g_a, timed_run
with torch.no_grad():
    for i in range(3 + frames):
        if i == 3:
            torch.cuda.synchronize()
            del log[:]
        runner.step()
torch.cuda.synchronize()
print(f"RATE_FORK = {getattr(M, 'RATE_FORK', 'absent')}; {frames} frames; g_a's end -> g_s's end on the launch stream, median [min .. max] us")
for name in ("MVCoder", "ResCoder"):
    us = [a.elapsed_time(b) * 1e3 for n, a, b in log if n == name]
    print(f"  {name}: {statistics.median(us):7.1f} [{min(us):7.1f} .. {max(us):7.1f}]")
