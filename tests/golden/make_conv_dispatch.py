"""Records tests/golden/conv_dispatch.npz: which kernel tdvc_conv2d dispatches every descriptor of
tests/helpers_conv_dispatch.sweep to, and its tdvc_conv_chan_sum_rows, with every debug switch on and then with each one off.

    python tests/golden/make_conv_dispatch.py [ROOT]

ROOT is the checkout whose built library is recorded (default: this one) -- the golden in git was recorded from the commit
BEFORE the dispatch table, so that the table is held to the cascade it replaced.  Only tdvc_conv2d, tdvc_last_conv_kernel and
tdvc_conv_chan_sum_rows are used.  The descriptors point at dummy host addresses: every launch must fail for want of a
device, so this refuses to run where there is one."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if torch.cuda.is_available():
    sys.exit("make_conv_dispatch.py: a GPU is visible; dummy pointers must never reach a real device")
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
from tdvc_amd import _lib as L, ops  # noqa: E402  (of ROOT)

spec = importlib.util.spec_from_file_location("helpers_conv_dispatch", os.path.join(os.path.dirname(HERE), "helpers_conv_dispatch.py"))
H = importlib.util.module_from_spec(spec)
spec.loader.exec_module(H)

lib = L.lib()
descs, subset = H.sweep(L, ops._pick_ck)
names = []


def record(ds):
    idx, rows = [], []
    for d in ds:
        name, r = H.observe(lib, d)
        if name not in names:
            names.append(name)
        idx.append(names.index(name))
        rows.append(r)
    return np.array(idx, dtype=np.uint8), np.array(rows, dtype=np.int32)


kernel, rows = record(descs)
sw_kernel, sw_rows = [], []
for setter, off, on in H.SWITCHES:
    getattr(lib, setter)(off)
    try:
        k, r = record([descs[i] for i in subset])
    finally:
        getattr(lib, setter)(on)
    sw_kernel.append(k)
    sw_rows.append(r)
np.savez_compressed(os.path.join(HERE, H.GOLDEN), names=np.array(names), kernel=kernel, rows=rows,
                    sw_kernel=np.stack(sw_kernel), sw_rows=np.stack(sw_rows))
count = {o: 0 for o in H.OUTCOMES}
for i in kernel:
    count[H.outcome(names[i])] += 1
print(len(descs), "descriptors,", len(subset), "per switch;", int((rows > 0).sum()), "with channel-sum rows")
for o, n in count.items():
    print(f"  {o:22s} {n}")
for (setter, off, _), k in zip(H.SWITCHES, sw_kernel):
    print(f"  {setter}({off}): {int((k != kernel[subset]).sum())} of {len(subset)} move")
