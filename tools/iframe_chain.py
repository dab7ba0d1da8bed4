"""The launches around FeatureFix's I-frame chain in the LAST P-frame of a rocprofv3 kernel trace, one line per launch: the frame's last
conv_c8 launch is FeatureExtract_ref's first conv; in front of it sit tdvc_frame_changed's compare and refresh kernels (when the reuse is
on), behind it the two conv_pair launches, the conv_row launch and avgpool_k's two kernels.  On a hit frame the six show launch cost only.
usage: python3 tools/iframe_chain.py <kernel_trace.csv>"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "patch_match_kernel" in r["Kernel_Name"]]
frame = rows[marks[-2] + 1:marks[-1] + 1]
c8 = max(i for i, r in enumerate(frame) if "conv_c8_kernel" in r["Kernel_Name"])
t0 = int(frame[max(c8 - 3, 0)]["Start_Timestamp"])
for r in frame[max(c8 - 3, 0):c8 + 9]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")[:90]
    print(f"+{(s - t0) / 1e3:9.1f} us  {(e - s) / 1e3:8.1f} us  {name}")
span = int(frame[-1]["End_Timestamp"]) - int(frame[0]["Start_Timestamp"])
print(f"last frame: {len(frame)} kernels, span {span / 1e6:.3f} ms")
