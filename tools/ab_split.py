#!/usr/bin/env python3
"""conv_f32 against conv_split (ops.f32_split) on the fp32 islands of a frame: `forward(..., enabled_amp=False)` with the flag off (the
islands as they were: conv_f32) and on.

  per layer   one process: the profiled forward of each mode (event timings per launch), summed per conv shape -- every coder layer of the
              frame, launch by launch, on both kernels
  per frame   a fresh process per run, flag off and on alternating, --runs of each: median ms per frame over --steps forwards

usage: python tools/ab_split.py [--height 1088 --width 1920 --steps 10 --warmup 3 --runs 3] [--out profiles/rNN_split_islands.txt]"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup(h, w):
    import torch
    from tdvc_amd import synth
    from tdvc_amd.model import VideoCompressor
    net = VideoCompressor()
    synth.fill_parameters(net)
    net = net.cuda().eval()
    g = synth.make_gop(1234, 2, h, w)
    return torch, net, g[1:2].cuda(), synth.ref_list([g[0:1]]).cuda()


def child(a):
    """one mode in this process: median ms per forward"""
    torch, net, x, refs = _setup(a.height, a.width)
    net.f32_split = a.child == "on"
    ms = []
    with torch.no_grad():
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net(x, refs, False)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"mode": a.child, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}), flush=True)


def layers(a, say):
    from tdvc_amd import ops
    torch, net, x, refs = _setup(a.height, a.width)
    rows = {}
    with torch.no_grad():
        for mode in ("off", "on"):
            net.f32_split = mode == "on"
            for _ in range(a.warmup):
                net(x, refs, False)
            acc = collections.defaultdict(list)
            for _ in range(a.steps):
                ops.PROFILE = []
                try:
                    net(x, refs, False)
                    torch.cuda.synchronize()
                    one = collections.defaultdict(float)
                    cnt = collections.Counter()
                    for e in ops.PROFILE:
                        if e["kernel"] in ("conv_f32", "conv_split"):
                            one[(e["shape"], e["flops"])] += e["e0"].elapsed_time(e["e1"]) * 1e3
                            cnt[(e["shape"], e["flops"])] += 1
                finally:
                    ops.PROFILE = None
                for k, v in one.items():
                    acc[k].append((v, cnt[k]))
            rows[mode] = {k: (statistics.median(t for t, _ in v), v[0][1]) for k, v in acc.items()}
    say(f"per layer shape, {a.height}x{a.width}, median of {a.steps} profiled forwards (us per frame over the n launches of the shape; TFLOP/s of conv_split)")
    say(f"{'shape':44s} {'n':>3s} {'conv_f32':>10s} {'conv_split':>10s} {'ratio':>6s} {'TFLOP/s':>8s}")
    tot = [0.0, 0.0]
    for k in sorted(rows["off"], key=lambda k: -rows["off"][k][0]):
        t0, n = rows["off"][k]
        t1 = rows["on"].get(k, (float("nan"), 0))[0]
        tot[0] += t0
        tot[1] += t1
        say(f"{k[0]:44s} {n:3d} {t0:10.1f} {t1:10.1f} {t1 / t0:6.2f} {n * k[1] / t1 / 1e6:8.1f}" + ("   SLOWER" if t1 > t0 else ""))
    say(f"{'all fp32 convs of the frame':44s}     {tot[0]:10.1f} {tot[1]:10.1f} {tot[1] / tot[0]:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("off", "on"), default=None)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            print(s, file=out, flush=True)

    if not a.no_layers:
        layers(a, say)
    say(f"\nper frame, forward(x, refs, enabled_amp=False) at {a.height}x{a.width}: a process per run, alternating, median of {a.steps} forwards")
    res = {"off": [], "on": []}
    for r in range(a.runs):
        for mode in ("off", "on"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--height", str(a.height), "--width", str(a.width),
                                "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                say(f"run {r} {mode}: exit {p.returncode}\n{p.stderr[-2000:]}")
                return 1
            j = json.loads(p.stdout.strip().splitlines()[-1])
            res[mode].append(j["ms_median"])
            say(f"run {r} f32_split {mode:3s}: {j['ms_median']:8.2f} ms  (min {j['ms_min']:.2f}, max {j['ms_max']:.2f})")
    for mode, name in (("off", "conv_f32 islands (parent)"), ("on", "conv_split islands")):
        v = res[mode]
        say(f"{name:28s}: median {statistics.median(v):7.2f} ms = {1e3 / statistics.median(v):6.2f} frames/s, spread {max(v) - min(v):.2f} ms over {len(v)} processes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
