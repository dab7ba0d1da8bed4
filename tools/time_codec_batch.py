"""Real coding of a batch of frames: per-frame wall time of VideoCompressor.encode / decode for B frames in one call, with the
batched context loop (coder.AR_BATCH) off and on, and the time of one step of the loop.

  python tools/time_codec_batch.py                                   # 1088x1920 and 448x256, B = 1 2 4 8, all orders
  python tools/time_codec_batch.py --sizes 448x256 --batches 1,4 --orders lanes64 --repo /path/to/another/checkout

One process.  A line per (size, order, AR_BATCH, B): encode / decode ms PER FRAME (the call's time over B; median over --frames
calls, the first call dropped) and the loop's time per step (one coder's context-loop call bracketed by stream waits, over its
steps).  Every step runs under its own time limit: a watchdog thread ends the process when a step exceeds --step-limit seconds.
`--repo`: import tdvc_amd from another checkout (a commit without AR_BATCH runs the `off` lines only).
`--range-coder device` (lanes orders only): the y streams' range encoder on the GPU (VideoCompressor.stream_coder).  Every line
also gives the process's CPU seconds per frame over the timed encode calls (time.process_time(): worker threads included), the y
bytes copied device-to-host per frame (coder.Y_BUS_BYTES; for a checkout without the counter, the host coder's symbols and indexes
from the shapes) and, for the device coder, the encode kernel's own duration per frame from events around its launches."""
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
    ap.add_argument("--range-coder", default="host", choices=("host", "device"))
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
    if a.range_coder == "device":
        net.stream_coder = "device"
    kern_events = []
    plain_enc = getattr(ops, "ar_encode_lanes_batch", None)

    def evented(*args, **kw):                                  # events on the stream the launch goes to (the coder's side stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = plain_enc(*args, **kw)
        e1.record()
        kern_events.append((e0, e1))
        return r

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
            if a.range_coder == "device" and net.stream_order != "lanes":
                continue
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
                    te, td, equal, cpu, bus = [], [], True, [], []
                    with torch.no_grad():
                        for it in range(a.frames + 1):
                            torch.cuda.synchronize(); t0 = time.perf_counter()
                            c0, b0 = time.process_time(), getattr(cm, "Y_BUS_BYTES", None)
                            enc = net.encode(x, rl)
                            torch.cuda.synchronize(); t1 = time.perf_counter()
                            if it:
                                cpu.append((time.process_time() - c0) / B)
                                bus.append((cm.Y_BUS_BYTES - b0) / B if b0 is not None else 2 * 2 * 4 * (H // 16) * (W // 16) * 128)
                            rec = net.decode(enc["strings"], enc["shapes"], rl)
                            torch.cuda.synchronize(); t2 = time.perf_counter()
                            equal = equal and torch.equal(rec, enc["recon"])
                            if it:
                                te.append((t1 - t0) / B); td.append((t2 - t1) / B)
                        # the loop alone: one more frame with every loop call bracketed by stream waits
                        instrument(True)
                        del loop_time[:], kern_events[:]
                        if plain_enc is not None:
                            ops.ar_encode_lanes_batch = evented
                        enc = net.encode(x, rl)
                        if plain_enc is not None:
                            ops.ar_encode_lanes_batch = plain_enc
                        n_enc = len(loop_time)
                        torch.cuda.synchronize()
                        kern = f"{sum(e0.elapsed_time(e1) for e0, e1 in kern_events) / B:.3f} ms/frame" if kern_events else "-"
                        net.decode(enc["strings"], enc["shapes"], rl)
                        instrument(False)
                    enc_step = sum(loop_time[:n_enc]) / 2 / nsteps[False] * 1e6          # two coders; per-image loops add up
                    dec_step = sum(loop_time[n_enc:]) / 2 / nsteps[order == "raster"] * 1e6
                    nbytes = sum(len(s) for rec_ in enc["strings"] for s in rec_)
                    print(f"{a.tag}{H}x{W} {order:9s} coder={a.range_coder:6s} AR_BATCH={mode:3s} B={B}: encode {med(te):8.2f} ms/frame (min {min(te) * 1e3:.2f} max {max(te) * 1e3:.2f})  "
                          f"decode {med(td):8.2f} ms/frame (min {min(td) * 1e3:.2f} max {max(td) * 1e3:.2f})  loop per step: encode {enc_step:6.1f} us "
                          f"decode {dec_step:6.1f} us (all {B} images)  {nbytes} B  equal {equal}  "
                          f"cpu {statistics.median(cpu):.4f} s/frame  y d2h {int(statistics.median(bus))} B/frame  encode kernels {kern}", flush=True)
                    faulthandler.cancel_dump_traceback_later()
    if has_switch:
        cm.AR_BATCH = True


if __name__ == "__main__":
    main()
