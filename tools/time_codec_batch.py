"""Real coding of a batch of frames: per-frame wall time of VideoCompressor.encode / decode for B frames in one call, with the
batched context loop (coder.AR_BATCH) off and on, and the time of one step of the loop.

  python tools/time_codec_batch.py                                   # 1088x1920 and 448x256, B = 1 2 4 8, all orders
  python tools/time_codec_batch.py --sizes 448x256 --batches 1,4 --orders lanes64 --repo /path/to/another/checkout

One process.  A line per (size, order, AR_BATCH, B): encode / decode ms PER FRAME (the call's time over B; median over --frames
calls, the first call dropped) and the loop's time per step (one coder's context-loop call bracketed by stream waits, over its
steps).  Every step runs under its own time limit: a watchdog thread ends the process when a step exceeds --step-limit seconds.
`--repo`: import tdvc_amd from another checkout (a commit without AR_BATCH runs the `off` lines only)."""
import argparse
import faulthandler
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1088x1920,448x256")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--orders", default="raster,wavefront,lanes64,lanes128")
    ap.add_argument("--modes", default="off,on", help="coder.AR_BATCH settings to time")
    ap.add_argument("--frames", type=int, default=3, help="timed calls per line (one more is run first and dropped)")
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds a line may take before the process is ended")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="", help="prefix of every line (e.g. the commit)")
    a = ap.parse_args()
    sys.path.insert(0, a.repo)
    import torch
    from tdvc_amd import ops
    from tdvc_amd.codec_utils import pad
    from tdvc_amd.model import VideoCompressor
    from tdvc_amd.model import coder as cm
    from tdvc_amd.synth import fill_parameters, make_gop, ref_list

    has_switch = hasattr(cm, "AR_BATCH")
    net = VideoCompressor()
    fill_parameters(net)
    net = net.cuda().eval()
    loop_time = []
    loops = [n for n in ("ar_wavefront", "ar_wavefront_batch", "ar_wavefront_lanes", "ar_wavefront_lanes_batch", "ar_decode_serial", "ar_decode_serial_batch")
             if hasattr(ops, n)]
    plain = {n: getattr(ops, n) for n in loops}

    def timed(fn):
        def f(*args, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(*args, **kw)
            torch.cuda.synchronize()
            loop_time.append(time.perf_counter() - t)
        return f

    def instrument(on):
        for n in loops:
            setattr(ops, n, timed(plain[n]) if on else plain[n])

    med = lambda v: statistics.median(v) * 1e3
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        nsteps = {True: (H // 16) * (W // 16), False: W // 16 + 3 * (H // 16 - 1)}          # raster decode: a step per position
        for order in a.orders.split(","):
            net.stream_order = "lanes" if order.startswith("lanes") else order
            net.stream_lanes = int(order[5:]) if order.startswith("lanes") else 64
            for mode in a.modes.split(","):
                if mode == "on" and not has_switch:
                    continue
                if has_switch:
                    cm.AR_BATCH = mode == "on"
                for B in (int(v) for v in a.batches.split(",")):
                    faulthandler.dump_traceback_later(a.step_limit, exit=True)
                    gops = [pad(make_gop(1234 + 17 * k, 3, H, W).cuda(), 64) for k in range(B)]
                    rl = ref_list([torch.cat([g[0:1] for g in gops]), torch.cat([g[1:2] for g in gops])])
                    x = torch.cat([g[2:3] for g in gops])
                    te, td, equal = [], [], True
                    with torch.no_grad():
                        for it in range(a.frames + 1):
                            torch.cuda.synchronize(); t0 = time.perf_counter()
                            enc = net.encode(x, rl)
                            torch.cuda.synchronize(); t1 = time.perf_counter()
                            rec = net.decode(enc["strings"], enc["shapes"], rl)
                            torch.cuda.synchronize(); t2 = time.perf_counter()
                            equal = equal and torch.equal(rec, enc["recon"])
                            if it:
                                te.append((t1 - t0) / B); td.append((t2 - t1) / B)
                        # the loop alone: one more frame with every loop call bracketed by stream waits
                        instrument(True)
                        del loop_time[:]
                        enc = net.encode(x, rl)
                        n_enc = len(loop_time)
                        net.decode(enc["strings"], enc["shapes"], rl)
                        instrument(False)
                    enc_step = sum(loop_time[:n_enc]) / 2 / nsteps[False] * 1e6          # two coders; per-image loops add up
                    dec_step = sum(loop_time[n_enc:]) / 2 / nsteps[order == "raster"] * 1e6
                    nbytes = sum(len(s) for rec_ in enc["strings"] for s in rec_)
                    print(f"{a.tag}{H}x{W} {order:9s} AR_BATCH={mode:3s} B={B}: encode {med(te):8.2f} ms/frame (min {min(te) * 1e3:.2f} max {max(te) * 1e3:.2f})  "
                          f"decode {med(td):8.2f} ms/frame (min {min(td) * 1e3:.2f} max {max(td) * 1e3:.2f})  loop per step: encode {enc_step:6.1f} us "
                          f"decode {dec_step:6.1f} us (all {B} images)  {nbytes} B  equal {equal}", flush=True)
                    faulthandler.cancel_dump_traceback_later()
    if has_switch:
        cm.AR_BATCH = True


if __name__ == "__main__":
    main()
