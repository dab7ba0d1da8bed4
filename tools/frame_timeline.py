"""Timeline of the LAST P-frame in a rocprofv3 kernel trace of bench.py (frames are delimited by patch_match_kernel, one per frame, as in
tools/last_frame.py): kernels, sum of their durations, span, per queue (= HIP stream) the busy time with its first start and last end, and
the union-busy time over the queues.  Sum of durations > union = kernels of two queues ran at the same time; the side queue's rows are the
coders' rate branches (tdvc_rate_branch).  python tools/frame_timeline.py kernel_trace.csv"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "patch_match_kernel" in r["Kernel_Name"]]
frame = rows[marks[-2] + 1:marks[-1] + 1]
qkey = "Queue_Id" if "Queue_Id" in frame[0] else ("Stream_Id" if "Stream_Id" in frame[0] else None)
iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[qkey] if qkey else "0", r["Kernel_Name"]) for r in frame)
t0, t1 = iv[0][0], max(e for _, e, _, _ in iv)


def union(spans):
    busy, (cs, ce) = 0, spans[0]
    for s, e in spans[1:]:
        if s > ce:
            busy, cs, ce = busy + ce - cs, s, e
        else:
            ce = max(ce, e)
    return busy + ce - cs


total = sum(e - s for s, e, _, _ in iv)
busy = union([(s, e) for s, e, _, _ in iv])
print(f"last frame: {len(iv)} kernels, sum of durations {total / 1e6:.3f} ms, span {(t1 - t0) / 1e6:.3f} ms, busy (union over queues) {busy / 1e6:.3f} ms, "
      f"overlapped {(total - busy) / 1e6:.3f} ms, queue column: {qkey}")
byq = collections.defaultdict(list)
for s, e, q, n in iv:
    byq[q].append((s, e, n))
for q, v in sorted(byq.items(), key=lambda kv: -len(kv[1])):
    print(f"queue {q}: {len(v)} kernels, busy {union([(s, e) for s, e, _ in v]) / 1e6:.3f} ms, first start +{(v[0][0] - t0) / 1e6:.3f} ms, "
          f"last end +{(max(e for _, e, _ in v) - t0) / 1e6:.3f} ms")
    if len(byq) > 1 and len(v) < len(iv) // 2:                 # a side queue: its bursts (a gap of > 1 ms starts a new one)
        burst = [v[0]]
        for k in v[1:] + [None]:
            if k is None or k[0] - burst[-1][1] > 1_000_000:
                bs, be = burst[0][0], max(e for _, e, _ in burst)
                print(f"      burst of {len(burst)} kernels +{(bs - t0) / 1e6:.3f} .. +{(be - t0) / 1e6:.3f} ms: {(be - bs) / 1e3:.0f} us long, "
                      f"{sum(e - s for s, e, _ in burst) / 1e3:.0f} us of kernels")
                burst = []
            if k is not None:
                burst.append(k)
