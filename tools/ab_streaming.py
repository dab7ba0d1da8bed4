"""Output bytes of every C entry point of csrc/pointwise.hip and csrc/backward_ops.hip on fixed-seed inputs at small sizes:
one line `digest <case> <buffer> <sha256>` per output buffer, then the SHA-256 of those lines.  Run it once per build of the
library, each in a process of its own (TDVC_LIB=path loads another build), and compare the lists: equal lists mean equal
bytes, which the tolerance tests cannot see (a reordered fp32 sum passes them).
  python tools/ab_streaming.py > branch.txt;  TDVC_LIB=/path/to/parent/libtdvc_hip.so python tools/ab_streaming.py > parent.txt
The cases cover fp16 and fp32 maps, channel windows of wider buffers (C < sp), N = 2, fp32 maps with C % 8 != 0, the VEC and the
scalar forms of spynet_level_input / avgpool2_pyramid, both paths of scale_act_res / bcast_add_act, flow_lo / da / dflow_lo
present and absent, inverse 0 / 1, and pixel counts that are no multiple of the reductions' block ranges."""
import ctypes as C
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdvc_amd import _lib as L, ops  # noqa: E402

if os.environ.get("TDVC_LIB"):
    L.LIB_PATH = os.path.abspath(os.environ["TDVC_LIB"])
lib = L.lib()
F16, F32 = torch.float16, torch.float32
LINES = []
_seed = [0]


def rnd(*shape, scale=1.0, dt=F32):
    _seed[0] += 1
    g = torch.Generator().manual_seed(_seed[0])
    return (torch.randn(*shape, generator=g) * scale).to(dt).cuda().contiguous()


def fm(N, H, W, C_, dt=F16, win=False, scale=1.0, pos=False):
    """a random map; win: channels 8 .. 8 + C of a buffer 16 channels wider"""
    t = rnd(N, H, W, C_ + (16 if win else 0), scale=scale, dt=dt)
    if pos:
        t = t.abs() + 0.5
    return ops.FM(t).ch(8, C_) if win else ops.FM(t)


def P(x):
    """argument form of a map (or None), a tensor (or None) or a scalar"""
    if isinstance(x, ops.FM):
        return C.byref(x.desc())
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    return x


def run(case, fn, args, outs):
    """outs: {name: FM or tensor}; the whole underlying buffer is hashed, so a write outside a window shows"""
    L.check(getattr(lib, fn)(*[P(a) for a in args], ops._stream()), case)
    torch.cuda.synchronize()
    for name, o in outs.items():
        t = o.t if isinstance(o, ops.FM) else o
        h = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
        LINES.append(f"digest {case} {name} {h}")
        print(LINES[-1], flush=True)


N, H, W = 2, 13, 11
DTW = [(F16, False), (F16, True), (F32, False), (F32, True)]
tag = lambda dt, win: ("f16" if dt == F16 else "f32") + ("w" if win else "")

# ---------------------------------------------------------------- pointwise.hip
for dt, win in DTW:
    for Cs, Cm in ((5, 8), (3, 5)) if dt == F32 else ((5, 8),):
        src = rnd(N, Cs, H, W)
        y = fm(N, H, W, Cm, dt, win)
        run(f"nchw_to_fmap {tag(dt, win)} C{Cs}->{Cm}", "tdvc_nchw_to_fmap", [src, Cs, y], {"y": y})
        dst = rnd(N, Cs, H, W)
        run(f"fmap_to_nchw {tag(dt, win)} C{Cs}<-{Cm}", "tdvc_fmap_to_nchw", [y, Cs, dst], {"dst": dst})

for dt, win in DTW:
    for Cc in (16, 12) if dt == F32 else (16,):
        gate = rnd(N, Cc).sigmoid()
        for g, r, y2, act in ((None, False, False, 0), (gate, True, False, 2), (gate, True, True, 1), (None, True, True, 0)):
            a, y = fm(N, H, W, Cc, dt, win), fm(N, H, W, Cc, dt, win)
            rr = fm(N, H, W, Cc, dt, win) if r else None
            yy = fm(N, H, W, Cc, dt) if y2 else None
            run(f"scale_act_res {tag(dt, win)} C{Cc} gate{int(g is not None)} r{int(r)} y2{int(y2)} act{act}", "tdvc_scale_act_res",
                [a, g, act, 0.1, rr, -1.0, y, yy], {"y": y, **({"y2": yy} if y2 else {})})
# the generic kernel on mixed dtypes (fp16 in, fp32 out) and the fast one on a map larger than one grid-stride round
a, y = fm(N, H, W, 16, F16), fm(N, H, W, 16, F32)
run("scale_act_res f16->f32", "tdvc_scale_act_res", [a, None, 2, 0.1, None, 1.0, y, None], {"y": y})
a, r, y = fm(1, 96, 128, 64), fm(1, 96, 128, 64), fm(1, 96, 128, 64)
run("scale_act_res f16 96x128x64", "tdvc_scale_act_res", [a, rnd(1, 64).sigmoid(), 0, 0.0, r, 1.0, y, None], {"y": y})
for win in (False, True):
    for g, r in ((None, False), (rnd(N, 16).sigmoid(), True)):
        a, y, b, y3 = (fm(N, H, W, 16, F16, win) for _ in range(4))
        rr = fm(N, H, W, 16, F16, win) if r else None
        run(f"scale_act_res3 {tag(F16, win)} gate{int(g is not None)} r{int(r)}", "tdvc_scale_act_res3", [a, g, 2, 0.1, rr, 1.0, y, b, -1.0, y3], {"y": y, "y3": y3})

for dt, win in DTW:
    off, flow = fm(N, H, W, 16, dt, win), fm(N, H, W, 2, F32, win)
    run(f"add_flow {tag(dt, win)}", "tdvc_add_flow", [off, flow], {"off": off})
    for T in (4, 2):
        x, b = fm(N, H, W, T * 16, dt, win), fm(N, H, W, 16, dt, win)
        run(f"bcast_add_act {tag(dt, win)} T{T}", "tdvc_bcast_add_act", [x, b, T, 0.1], {"x": x})

# SE: 143 pixels in 3 ranges (48, 48, 47: the tail loop), 1073 pixels in 3 ranges (358: the four-loads loop and its tail), 1 range
for dt, win in DTW:
    for (h, w, nb) in ((13, 11, 3), (37, 29, 3), (13, 11, 1)):
        for Cc in (64, 16, 256):
            x = fm(N, h, w, Cc, dt, win)
            partial = rnd(N, nb, Cc)
            run(f"channel_sum {tag(dt, win)} {h}x{w} C{Cc} nb{nb}", "tdvc_channel_sum", [x, partial, nb], {"partial": partial})
for Cc, Cmid, nb in ((64, 4, 3), (128, 8, 37), (256, 16, 1)):
    partial, gate = rnd(N, nb, Cc), rnd(N, Cc)
    w1, b1, w2, b2 = rnd(Cmid, Cc, scale=0.2), rnd(Cmid), rnd(Cc, Cmid, scale=0.5), rnd(Cc)
    run(f"se_gate C{Cc} nb{nb}", "tdvc_se_gate", [partial, nb, 1.0 / 143, N, Cc, Cmid, w1, b1, w2, b2, gate], {"gate": gate})

for dt, win in DTW:
    x, y = fm(N, H, W, 16, dt, win), fm(N, 2 * H, 2 * W, 16, dt, win)
    run(f"upsample2x {tag(dt, win)}", "tdvc_upsample2x", [x, y], {"y": y})
x, y = fm(N, 1, 1, 8), fm(N, 2, 2, 8)
run("upsample2x 1x1", "tdvc_upsample2x", [x, y], {"y": y})
for win in (False, True):
    x, y = fm(N, 2 * H + 1, 2 * W, 5, F32, win), fm(N, H, W, 3, F32, win)
    run(f"avgpool2 {tag(F32, win)}", "tdvc_avgpool2", [x, y], {"y": y})

for vec in (True, False):
    Cp = 4 if vec else 3
    xa, xb = fm(N, 64, 96, Cp, F32), fm(N, 64, 96, Cp, F32)
    ya = [fm(N, 64 >> (k + 1), 96 >> (k + 1), Cp, F32) for k in range(5)]
    yb = [fm(N, 64 >> (k + 1), 96 >> (k + 1), Cp, F32) for k in range(5)]
    da, db = (L.FMapDesc * 5)(*[m.desc() for m in ya]), (L.FMapDesc * 5)(*[m.desc() for m in yb])
    run(f"avgpool2_pyramid vec{int(vec)}", "tdvc_avgpool2_pyramid", [xa, xb, da, db],
        {**{f"ya{k}": m for k, m in enumerate(ya)}, **{f"yb{k}": m for k, m in enumerate(yb)}})

for vec in (True, False):
    for lo in (True, False):
        for cdt in (F16, F32):
            Cp = 4 if vec else 3
            h, w = 14, 22
            ref, supp = fm(N, h, w, Cp, F32), fm(N, h, w, Cp, F32)
            flow_lo = fm(N, h // 2, w // 2, 2, F32, scale=3.0) if lo else None       # flows of a few pixels: some positions clamp at the border
            flow_up, cat8 = fm(N, h, w, 2, F32), fm(N, h, w, 8, cdt)
            run(f"spynet_level_input vec{int(vec)} lo{int(lo)} cat{tag(cdt, False)}", "tdvc_spynet_level_input", [ref, supp, flow_lo, flow_up, cat8],
                {"flow_up": flow_up, "cat8": cat8})

for (h0, w0, h1, w1) in ((13, 11, 7, 9), (7, 9, 13, 11), (5, 6, 20, 18), (13, 11, 13, 11)):
    for sc in (None, rnd(3)):
        x, y = fm(N, h0, w0, 3, F32), fm(N, h1, w1, 3, F32)
        run(f"resize_bilinear {h0}x{w0}->{h1}x{w1} chscale{int(sc is not None)}", "tdvc_resize_bilinear", [x, y, sc], {"y": y})

for dt, win in DTW:
    x = fm(N, 40, 52, 64, dt, win)
    scale, hp, wp = 10, 4, 5
    nwork = lib.tdvc_avgpool_k_work_floats(N, hp, wp, 64, scale)
    print(f"value avgpool_k_work_floats {nwork}")
    LINES.append(f"value avgpool_k_work_floats {nwork}")
    work, pooled = rnd(nwork), rnd(N, hp, wp, 64)
    run(f"avgpool_k {tag(dt, win)}", "tdvc_avgpool_k", [x, scale, pooled, hp, wp, work, nwork], {"pooled": pooled, "work": work})

for same in (True, False):
    cur = fm(N, H, W, 16)
    cache = ops.FM(cur.t.clone()) if same else fm(N, H, W, 16)
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    run(f"frame_changed same{int(same)}", "tdvc_frame_changed", [cur, cache, flag], {"cache": cache, "flag": flag})
    cache = ops.FM(cur.t.clone())
    if not same:
        cache.t[1, 3, 4, 5] += 1.0
    flags = torch.full((N,), 7, dtype=torch.int32, device="cuda")
    for mask in (0, 1):
        run(f"frames_changed same{int(same)} mask{mask}", "tdvc_frames_changed", [cur, cache, flags, mask], {"cache": cache, "flags": flags})

hp, wp, Cc = 9, 15, 8
pin, pref = rnd(N, hp, wp, Cc), rnd(N, hp, wp, Cc)
nph, npw = (hp + 3) // 3 + 1, (wp + 3) // 3 + 1
idx = torch.zeros((N, nph * npw), dtype=torch.int32, device="cuda")
run("patch_match", "tdvc_patch_match", [pin, pref, N, hp, wp, Cc, idx], {"idx": idx})
_seed[0] += 1
idx = torch.randint(0, nph * npw, (N, nph * npw), generator=torch.Generator().manual_seed(_seed[0]), dtype=torch.int32).cuda()
for dt, win in DTW:
    fin, fref, cat = fm(N, 18, 30, 64, dt, win), fm(N, 18, 30, 64, dt, win), fm(N, 18, 30, 128, dt, win)
    run(f"match_gather {tag(dt, win)}", "tdvc_match_gather", [fin, fref, idx, 2, hp, wp, cat], {"cat": cat})
    dcat, dfin, dfref = fm(N, 18, 30, 128, dt, win), fm(N, 18, 30, 64, dt, win), fm(N, 18, 30, 64, dt, win)
    run(f"match_gather_backward {tag(dt, win)}", "tdvc_match_gather_backward", [fin, fref, idx, 2, hp, wp, dcat, dfin, dfref], {"dfin": dfin, "dfref": dfref})


def eb_raw(Cc):
    lens = [3, 9, 9, 9, 3, 3, 3, 3, 3, 1, 3, 3, 3, 3]
    raw = [rnd(Cc, n, scale=0.5) for n in lens]
    table = torch.tensor([t.data_ptr() for t in raw], dtype=torch.int64).cuda()
    q = rnd(Cc, 3)
    return raw, table, q


Cc = 8
raw, table, quant = eb_raw(Cc)
packed = rnd(Cc, 59)
run("eb_pack", "tdvc_eb_pack", [table, quant, packed, Cc], {"packed": packed})
for win in (False, True):
    for noisy in (False, True):
        for zdt in (F16, F32):
            z, z_hat = fm(N, H, W, Cc, F32, win, scale=2.0), fm(N, H, W, Cc, zdt, win)
            noise = fm(N, H, W, Cc, F32, win, scale=0.3) if noisy else None
            nb = (N * H * W * Cc + 255) // 256
            bits, partial = torch.zeros(1, dtype=torch.float64, device="cuda"), rnd(nb)
            run(f"eb_forward {tag(F32, win)} noise{int(noisy)} zhat{tag(zdt, False)}", "tdvc_eb_forward", [z, packed, noise, z_hat, bits, partial, nb],
                {"z_hat": z_hat, "bits": bits, "partial": partial})
        y, gp = fm(N, H, W, Cc, F32, win, scale=2.0), fm(N, H, W, 2 * Cc, F32, win)
        noise = fm(N, H, W, Cc, F32, win, scale=0.3) if noisy else None
        bits, partial = torch.zeros(1, dtype=torch.float64, device="cuda"), rnd(nb)
        run(f"gc_forward {tag(F32, win)} noise{int(noisy)}", "tdvc_gc_forward", [y, gp, noise, bits, partial, nb], {"bits": bits, "partial": partial})
    z, noise, dz = fm(N, H, W, Cc, F32, win, scale=2.0), fm(N, H, W, Cc, F32, win, scale=0.3), fm(N, H, W, Cc, F32, win)
    dparams = rnd(Cc, 59)
    run(f"eb_backward {tag(F32, win)}", "tdvc_eb_backward", [z, packed, noise, 0.01, dz, dparams], {"dz": dz, "dparams": dparams})
    y, gp, noise = fm(N, H, W, Cc, F32, win, scale=2.0), fm(N, H, W, 2 * Cc, F32, win), fm(N, H, W, Cc, F32, win, scale=0.3)
    dy, dgp = fm(N, H, W, Cc, F32, win), fm(N, H, W, 2 * Cc, F32, win)
    run(f"gc_backward {tag(F32, win)}", "tdvc_gc_backward", [y, gp, noise, 0.01, dy, dgp], {"dy": dy, "dgp": dgp})
grads = [rnd(*t.shape) for t in raw]
gtable = torch.tensor([t.data_ptr() for t in grads], dtype=torch.int64).cuda()
run("eb_param_chain", "tdvc_eb_param_chain", [rnd(Cc, 59), table, gtable, 0.5, Cc], {f"g{k}": t for k, t in enumerate(grads)})
for Ca in (8, 128, 341):          # 24 threads (one wave), 384 (6 waves), 1023 (16 waves)
    rawa, tablea, qa = eb_raw(Ca)
    pk = rnd(Ca, 59)
    run(f"eb_pack C{Ca}", "tdvc_eb_pack", [tablea, qa, pk, Ca], {"packed": pk})
    dq, loss = rnd(Ca, 3), rnd(1)
    run(f"eb_aux C{Ca}", "tdvc_eb_aux", [pk, qa, 6.9, dq, loss, Ca], {"dq": dq, "loss": loss})

for dt, win in DTW:
    for Cc in (16, 12) if dt == F32 else (16,):
        y, noise, y_hat = fm(N, H, W, Cc, dt, win, scale=3.0), fm(N, H, W, Cc, dt, win, scale=0.3), fm(N, H, W, Cc, dt, win)
        run(f"quantize {tag(dt, win)} C{Cc} round", "tdvc_quantize", [y, None, y_hat], {"y_hat": y_hat})
        run(f"quantize {tag(dt, win)} C{Cc} noise", "tdvc_quantize", [y, noise, y_hat], {"y_hat": y_hat})

# ---------------------------------------------------------------- backward_ops.hip
for dt, win in DTW:
    for res in (False, True):
        for act in (1, 2):
            g, y, out = fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win)
            r = fm(N, H, W, 16, dt, win) if res else None
            run(f"act_backward {tag(dt, win)} res{int(res)} act{act}", "tdvc_act_backward", [g, y, r, act, 0.1, out], {"out": out})
    y, out = fm(N, 2 * H, 2 * W, 16, dt, win), fm(N, H, W, 64, dt, win)
    run(f"pixel_unshuffle {tag(dt, win)}", "tdvc_pixel_unshuffle", [y, out], {"out": out})
    g, y = fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win, scale=0.7)
    run(f"clamp01_backward {tag(dt, win)}", "tdvc_clamp01_backward", [g, y], {"g": g})
    dx, v = fm(N, H, W, 16, dt, win), rnd(N, 16)
    run(f"bcast_channel_add {tag(dt, win)}", "tdvc_bcast_channel_add", [dx, v, 0.25], {"dx": dx})
    doff, dflow = fm(N, H, W, 16, dt, win), fm(N, H, W, 2, F32, win)
    run(f"add_flow_backward {tag(dt, win)}", "tdvc_add_flow_backward", [doff, dflow], {"dflow": dflow})
    for T in (4, 1):
        dx, x, db = fm(N, H, W, T * 16, dt, win), fm(N, H, W, T * 16, dt, win), fm(N, H, W, 16, dt, win)
        run(f"bcast_add_act_backward {tag(dt, win)} T{T}", "tdvc_bcast_add_act_backward", [dx, x, db, 0.1], {"dx": dx, "db": db})
    dy, dx = fm(N, 2 * H, 2 * W, 16, dt, win), fm(N, H, W, 16, dt, win)
    run(f"upsample2x_backward {tag(dt, win)}", "tdvc_upsample2x_backward", [dy, dx], {"dx": dx})
    for inv in (0, 1):
        g, x, n32 = fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win), fm(N, H, W, 16, F32, win, pos=True)
        dn, dx = fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win)
        run(f"gdn_backward {tag(dt, win)} inverse{inv}", "tdvc_gdn_backward", [g, x, n32, inv, dn, dx], {"dn": dn, "dx": dx})
    dx, x, t = fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win), fm(N, H, W, 16, dt, win)
    run(f"mul2_accumulate {tag(dt, win)}", "tdvc_mul2_accumulate", [dx, x, t], {"dx": dx})
    # bias gradient: 35 pixels (one range), 2173 pixels (two ranges, 1087 + 1086); C = 264: a last 256-channel block of 8 channels
    for (h, w) in ((5, 7), (41, 53)):
        for Cc in (8, 216, 264):
            g = fm(N, h, w, Cc, dt, win)
            nwork = lib.tdvc_bias_grad_work_floats(N, Cc)
            for nvalid, perm in ((Cc, False), (Cc - 3, True)):
                db, work = rnd(Cc), rnd(nwork)
                _seed[0] += 1
                di = torch.randperm(Cc, generator=torch.Generator().manual_seed(_seed[0])).to(torch.int32)
                di[1] = -1
                run(f"bias_grad {tag(dt, win)} {h}x{w} C{Cc} nvalid{nvalid} index{int(perm)}", "tdvc_bias_grad",
                    [g, nvalid, di.cuda() if perm else None, 0.5, db, work, nwork], {"db": db, "work": work})
    for (h, w) in ((13, 11), (37, 29), (67, 53)):      # 1 range; 4 ranges of 269 (268 + ... uneven); 13 ranges
        for da_on in (False, True):
            g, a, gate = fm(N, h, w, 64, dt, win), fm(N, h, w, 64, dt, win), rnd(N, 64).sigmoid()
            da = fm(N, h, w, 64, dt, win) if da_on else None
            nwork = lib.tdvc_gate_backward_work_floats(N, 64)
            dgate, work = rnd(N, 64), rnd(nwork)
            run(f"gate_backward {tag(dt, win)} {h}x{w} da{int(da_on)}", "tdvc_gate_backward", [g, a, gate, da, dgate, work, nwork],
                {"dgate": dgate, "work": work, **({"da": da} if da_on else {})})
print(f"value bias_grad_work_floats {lib.tdvc_bias_grad_work_floats(N, 264)} gate_backward_work_floats {lib.tdvc_gate_backward_work_floats(N, 64)}")
LINES.append(f"value work_floats {lib.tdvc_bias_grad_work_floats(N, 264)} {lib.tdvc_gate_backward_work_floats(N, 64)}")

for (sdt, sC, ddt, dC) in ((F16, 8, F32, 8), (F16, 8, F32, 13), (F32, 5, F16, 8), (F32, 5, F32, 5), (F32, 5, F32, 11), (F16, 8, F16, 24)):
    for win in (False, True):
        src, dst = fm(N, H, W, sC, sdt, win), fm(N, H, W, dC, ddt, win)
        run(f"copy_cast {tag(sdt, win)} C{sC} -> {tag(ddt, win)} C{dC}", "tdvc_copy_cast", [src, dst], {"dst": dst})

Cc, Cmid, nb = 64, 4, 3
partial, gate, dgate = rnd(N, nb, Cc), rnd(N, Cc).sigmoid(), rnd(N, Cc)
w1, b1, w2, b2 = rnd(Cmid, Cc, scale=0.2), rnd(Cmid), rnd(Cc, Cmid, scale=0.5), rnd(Cc)
dmean, dw1, db1, dw2, db2 = rnd(N, Cc), rnd(Cmid, Cc), rnd(Cmid), rnd(Cc, Cmid), rnd(Cc)
run("se_gate_backward", "tdvc_se_gate_backward", [partial, nb, 1.0 / 143, N, Cc, Cmid, w1, b1, w2, b2, gate, dgate, 0.5, dmean, dw1, db1, dw2, db2],
    {"dmean": dmean, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2})

for (h0, w0, h1, w1_) in ((13, 11, 7, 9), (7, 9, 13, 11), (5, 6, 20, 18), (13, 11, 13, 11)):
    for sc in (None, rnd(3)):
        dy, dx = fm(N, h1, w1_, 3, F32), fm(N, h0, w0, 3, F32)
        run(f"resize_bilinear_backward {h0}x{w0}<-{h1}x{w1_} chscale{int(sc is not None)}", "tdvc_resize_bilinear_backward", [dy, dx, sc], {"dx": dx})

for lo in (True, False):
    for cdt in (F16, F32):
        for (h, w) in ((14, 22), (2, 2)):
            supp, flow_up = fm(N, h, w, 3, F32), fm(N, h, w, 2, F32, scale=3.0)
            dcat8, dflow_up = fm(N, h, w, 8, cdt), fm(N, h, w, 2, F32)
            dflow_lo = fm(N, h // 2, w // 2, 2, F32) if lo else None
            run(f"spynet_level_input_backward {h}x{w} lo{int(lo)} dcat{tag(cdt, False)}", "tdvc_spynet_level_input_backward",
                [supp, flow_up, dcat8, dflow_up, dflow_lo], {"dflow_up": dflow_up, **({"dflow_lo": dflow_lo} if lo else {})})

n = 1000
x, out = rnd(n, scale=3.0), rnd(n)
run("sigmoid_f32", "tdvc_sigmoid_f32", [x, out, n], {"out": out})
g = rnd(n)
run("sigmoid_backward_f32", "tdvc_sigmoid_backward_f32", [g, out, n], {"g": g})
dst = rnd(n)
run("axpy_f32", "tdvc_axpy_f32", [dst, x, 0.25, n], {"dst": dst})

print(f"{len(LINES)} lines, digest of the list {hashlib.sha256(chr(10).join(LINES).encode()).hexdigest()}")
