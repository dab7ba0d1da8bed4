"""The launches of LoopFilter's head in the LAST P-frame of a rocprofv3 kernel trace, one line per launch, and the per-image time of its
conv_pair launches.  The head is what sits between conv01's conv_c8 launch on the three reference frames and the fused temporal conv
(conv_mfma_v5): with the reuse on, tdvc_frames_changed's compare and refresh kernels, conv_c8, conv_pair (conv02 + conv1), the conv of prediction1's slice,
conv_pair (layer1.conv1 + spatial_conv3d); with it off the same without the first two.  A skipped image shortens its launch.  Then the
tail: the fused temporal conv and conv3's launches, or the single lf_tail_kernel launch that replaces them (LOOPFILTER_TAIL).
usage: python3 tools/lf_chain.py <kernel_trace.csv> [images computed by the first pair launch] [by the second]   (default 3 4)"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "patch_match_kernel" in r["Kernel_Name"]]
frame = rows[marks[-2] + 1:marks[-1] + 1]
# conv01 is the conv_c8 launch directly in front of a conv_pair launch of the slope form <*, 2, 2, ...> (FeaExtra's and
# FeatureExtract_ref's first convs feed Res_Block pairs <*, 1, 0, ...>)
short = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
c8 = [i for i, r in enumerate(frame) if "conv_c8_kernel" in r["Kernel_Name"]]
head = next(i for i in c8 if any("conv_pair_kernel" in frame[j]["Kernel_Name"] and ", 2, 2," in short(frame[j]) for j in range(i + 1, min(i + 3, len(frame)))))
first = head
while first > 0 and "frames_" in frame[first - 1]["Kernel_Name"]:
    first -= 1
is_tail = lambda r: "conv_mfma_v5" in r["Kernel_Name"] or "lf_tail_kernel" in r["Kernel_Name"]
last = next(i for i in range(head, len(frame)) if is_tail(frame[i]))
t0 = int(frame[first]["Start_Timestamp"])
pairs = []
for r in frame[first:last + 1]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if "conv_pair_kernel" in r["Kernel_Name"]:
        pairs.append((e - s) / 1e3)
    print(f"+{(s - t0) / 1e3:9.1f} us  {(e - s) / 1e3:8.1f} us  {short(r)[:90]}")
e_last = int(frame[max(i for i in range(first, last) if "conv_pair_kernel" in frame[i]["Kernel_Name"])]["End_Timestamp"])
print(f"head (first launch to the end of the last conv_pair): {(e_last - t0) / 1e3:.1f} us")
imgs = [int(a) for a in sys.argv[2:4]] or [3, 4]
for us, n in zip(pairs, imgs):
    print(f"conv_pair: {us:.1f} us for {n} image(s) = {us / max(n, 1):.1f} us per image")
# the tail: the fused temporal conv (conv_mfma_v5<4, ..>) and conv3's conv_row launches, or the one lf_tail_kernel launch in their place,
# up to and without feat_fusion's conv_mfma_v5 launch
tail_end = next(i for i in range(last + 1, len(frame)) if "conv_mfma_v5" in frame[i]["Kernel_Name"])
tail = frame[last:tail_end]
for r in tail:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print(f"tail +{(s - t0) / 1e3:9.1f} us  {(e - s) / 1e3:8.1f} us  {short(r)[:90]}")
print(f"tail: {len(tail)} launch(es), {sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in tail) / 1e3:.1f} us of kernel time")
span = int(frame[-1]["End_Timestamp"]) - int(frame[0]["Start_Timestamp"])
print(f"last frame: {len(frame)} kernels, span {span / 1e6:.3f} ms")
