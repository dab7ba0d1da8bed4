"""run ONE fused LoopFilter tail (tdvc_lf_tail) repeatedly on ring windows as LoopFilter passes them (for rocprofv3 --pmc or a kernel
trace): python tools/one_lf_tail.py H W iters [two]   (`two`: the two launches it replaces instead -- conv_mfma_v5 bcast_T + conv_row)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import ops  # noqa: E402

H, W, iters = [int(v) for v in sys.argv[1:4]]
two = len(sys.argv) > 4 and sys.argv[4] == "two"
R, p = 9, 2
S = ops.FM(torch.randn(1, H, W, 64 * R, device="cuda").half()).ch(64 * p, 256)
A = ops.FM(torch.randn(1, H, W, 64 * R, device="cuda").half()).ch(64 * p, 256)
pct = ops.pack_conv(torch.randn(64, 192, 1, 1) * 0.07, None, stride=1, pad=0)
pc3 = ops.pack_conv(torch.randn(64, 64, 3, 3) * 0.04, torch.randn(64) * 0.1, stride=1, pad=1)
o = ops.FM.empty(1, H, W, 256)
s = ops.FM.empty(1, H, W, 256)
for _ in range(iters + 1):
    if two:
        ops.conv(S.ch(0, 192), pct, out=s.ch(0, 64), bcast_T=4, bcast_slope=0.1, res=S.ch(0, 64))
        ops.conv(s.as_slices(0, 4, 64), pc3, out=o.as_slices(0, 4, 64), res=ops.FM(A.t, A.off, 4, 64, 64))
    else:
        ops.lf_tail(S, A, pct, pc3, out=o, slope=0.1)
torch.cuda.synchronize()
