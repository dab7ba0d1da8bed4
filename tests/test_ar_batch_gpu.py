"""The context loop on the MI355X path (tdvc_ar_*_batch, coder.AR_BATCH): a step's positions of all B images in the same
launches, one image being B = 1.  All of it is exact arithmetic, so every comparison here is exact -- torch.equal, np.array_equal,
== on bytes -- against a torch reference of the kernels, the host range decoder and the per-image loop (B calls of one image)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from util import randn, rnd16, to_fm

pytestmark = pytest.mark.gpu

M = 128
DEV = "cuda"


@pytest.fixture(scope="module")
def coder():
    from tdvc_amd.model.coder import MVCoder
    from tdvc_amd.synth import fill_parameters
    m = MVCoder(N=128)
    h = torch.nn.Module(); h.add_module("mvCoder", m); fill_parameters(h)
    m = m.cuda().eval()
    m.update(force=True)
    return m


def adt_of(f32):
    return torch.float32 if f32 else torch.float16


# positions of an 8 x 8 grid that meet every border case of the 12 causal taps: the corners of row 0, rows 0 / 1 (taps at dy = -2, -1
# outside), columns 0, 1 and 6, 7 (taps at dx = -2, -1 / +1, +2 outside) and interior ones
POS = [(0, 0), (0, 7), (1, 0), (3, 4), (0, 1), (1, 1), (0, 6), (1, 7), (2, 0), (2, 6), (7, 7), (5, 1), (4, 3)]


def window(B, H, W, Cc, dtype, windowed, fill):
    """an FM of (B, H, W, Cc): dense, or a batch and channel window of a larger buffer (sn and sp larger than dense)"""
    from tdvc_amd import ops
    if not windowed:
        return ops.FM(fill(B, H, W, Cc).to(dtype).to(DEV).contiguous())
    big = torch.full((B + 2, H, W, Cc + 64), 777.0, dtype=dtype, device=DEV)
    big[1:B + 1, :, :, 32:32 + Cc] = fill(B, H, W, Cc).to(dtype).to(DEV)
    return ops.FM(big).batch(1, B).ch(32, Cc)


def dense(fm):
    """the (N, H, W, C) values an FM addresses, as a strided view of its buffer (writes go to the buffer)"""
    return torch.as_strided(fm.t, (fm.N, fm.H, fm.W, fm.C), (fm.sn, fm.W * fm.sp, fm.sp, 1), fm.t.storage_offset() + fm.off)


def with_b1(names, cases):
    """parametrise over `cases` and B in (3, 1).  B = 3 runs under the ids the cases had before a single image became B = 1 of the same
    kernels, B = 1 under the id with "-B1" appended"""
    return pytest.mark.parametrize(names + ",B", [pytest.param(*c, B, id="-".join(str(v) for v in c) + ("" if B == 3 else "-B1"))
                                                  for B in (3, 1) for c in cases])


# ---- what the kernels compute, in torch: moves, one fp32 subtraction, round half to even, one fp32 addition, comparisons -- all exact
TAPS = [(-2, -2), (-2, -1), (-2, 0), (-2, 1), (-2, 2), (-1, -2), (-1, -1), (-1, 0), (-1, 1), (-1, 2), (0, -2), (0, -1)]      # the type-A 5x5 mask


def ref_gather(y_hat, params, pos):
    """y_hat (B, H, W, M), params (B, H, W, 2M), pos [(h, w)] -> x1 rows (B * n, 12 * M), pc rows (B * n, 2M): row b * n + k, tap t =
    y_hat[b, h + dy_t, w + dx_t] if that lies in rows >= 0 and columns 0 .. W - 1, else zeros"""
    B, H, W, Mc = y_hat.shape
    x1 = torch.zeros((B, len(pos), 12, Mc), dtype=y_hat.dtype, device=y_hat.device)
    pc = torch.empty((B, len(pos), params.shape[3]), dtype=params.dtype, device=params.device)
    for k, (h, w) in enumerate(pos):
        for t, (dy, dx) in enumerate(TAPS):
            if h + dy >= 0 and 0 <= w + dx < W:
                x1[:, k, t] = y_hat[:, h + dy, w + dx]
        pc[:, k] = params[:, h, w]
    return x1.view(B * len(pos), 12 * Mc), pc.view(B * len(pos), -1)


def ref_scale_index(scale, table):
    """ntable - 1 - #{j < ntable - 1 : max(s, 0.11) <= table[j]} (tests/test_ar_lanes_gpu.py: host_scale_index)"""
    s = scale.float().clamp(min=0.11)
    return (table.numel() - 1 - (s[..., None] <= table[:-1]).sum(-1)).to(torch.int32)


def ref_quantize(y, gp_rows_, pos, table, adt, symbols_in=None):
    """y (B, H, W, M) fp32 or None, gp rows (B, n, 2M) [scales | means], symbols_in (B, n, M) or None
    -> per position of the list: q (B, n, M) int32, y_hat values (B, n, M) in `adt`, CDF indexes (B, n, M) int32"""
    Mc = gp_rows_.shape[2] // 2
    scale, mean = gp_rows_[..., :Mc], gp_rows_[..., Mc:]
    if symbols_in is not None:
        q = symbols_in
    else:
        ph, pw = [p[0] for p in pos], [p[1] for p in pos]
        q = torch.round(y[:, ph, pw] - mean).to(torch.int32)          # one fp32 subtraction, round half to even (rintf)
    return q, (q.float() + mean).to(adt), ref_scale_index(scale, table)


@with_b1("f32,windowed", [(f, w) for f in (False, True) for w in (False, True)])
def test_gather_batch(f32, windowed, B):
    """B = 1 with a windowed FM: a batch window whose sn is larger than dense, on one image"""
    from tdvc_amd import ops
    H, W, n = 8, 8, len(POS)
    adt = adt_of(f32)
    fill = lambda *s: randn(*s, seed=3 + len(s) + s[-1])
    y_hat, params = window(B, H, W, M, adt, windowed, fill), window(B, H, W, 2 * M, adt, windowed, fill)
    pos = torch.tensor(POS, dtype=torch.int32, device=DEV)
    cap = B * n + 5                                                       # wider than the step
    x1 = ops.FM(torch.full((1, 1, cap, 12 * M), -5.0, dtype=adt, device=DEV))
    pc = ops.FM(torch.full((1, 1, cap, 4 * M), -5.0, dtype=adt, device=DEV))
    ops.ar_gather_batch(y_hat, params, pos, n, x1, pc)
    want_x1, want_pc = ref_gather(dense(y_hat), dense(params), POS)
    for b in range(B):
        assert torch.equal(x1.t[0, 0, b * n:(b + 1) * n], want_x1[b * n:(b + 1) * n]), f"image {b}: neighbourhoods"
        assert torch.equal(pc.t[0, 0, b * n:(b + 1) * n, :2 * M], want_pc[b * n:(b + 1) * n]), f"image {b}: params rows"
        x1_b = x1.t[0, 0, b * n:(b + 1) * n]
        assert bool((x1_b == 0).any()) and bool((x1_b[3] != 0).all())                     # zero fill at the borders, none inside
    assert bool((x1.t[0, 0, B * n:] == -5).all()) and bool((pc.t[0, 0, :, 2 * M:] == -5).all())        # nothing else was written
    # the images differ, and the windows' surroundings were not read as data
    assert B == 1 or not torch.equal(x1.t[0, 0, :n], x1.t[0, 0, n:2 * n])
    assert not bool((x1.t[0, 0, :B * n] == 777).any())


def gp_rows(nrows, seed):
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.02), np.log(600.0), (nrows, M))).astype(np.float32)
    scale[0, :4] = [0.05, 0.11, 256.0, 1e4]
    mean = (rng.standard_normal((nrows, M)) * 3).astype(np.float32)
    return torch.from_numpy(np.concatenate([scale, mean], 1))


@with_b1("f32", [(False,), (True,)])
def test_quantize_and_indexes_batch(coder, f32, B):
    from tdvc_amd import ops
    table = coder._coder_tables()[2]
    H, W, n = 8, 8, len(POS)
    adt = adt_of(f32)
    pos = torch.tensor(POS, dtype=torch.int32, device=DEV)
    ph, pw = pos[:, 0].long(), pos[:, 1].long()
    y = window(B, H, W, M, torch.float32, True, lambda *s: randn(*s, seed=17, scale=4.0))
    gp = ops.FM(torch.zeros((1, 1, B * n + 3, 2 * M), dtype=torch.float32, device=DEV))
    gp.t[0, 0, :B * n] = gp_rows(B * n, 5).to(DEV)
    sym_in = torch.randint(-40, 40, (B, H, W, M), dtype=torch.int32, device=DEV)
    cbase = 7
    for use_in in (False, True):
        # the torch reference, scattered into raster arrays and a windowed y_hat whose surroundings stay as they were
        q, yv, ci = ref_quantize(dense(y), gp.t[0, 0, :B * n].view(B, n, 2 * M), POS, table, adt, symbols_in=sym_in[:, ph, pw] if use_in else None)
        want_yh = window(B, H, W, M, adt, True, lambda *s: torch.zeros(*s))
        dense(want_yh)[:, ph, pw] = yv
        want_sym = torch.full((B, H, W, M), -9, dtype=torch.int32, device=DEV)
        want_idx = torch.full_like(want_sym, -9)
        want_sym[:, ph, pw], want_idx[:, ph, pw] = q, ci
        for compact in (False, True):
            yh = window(B, H, W, M, adt, True, lambda *s: torch.zeros(*s))
            shape = (B, H * W, M) if compact else (B, H, W, M)
            sym, idx, idx2 = (torch.full(shape, -9, dtype=torch.int32, device=DEV) for _ in range(3))
            s_in = None
            if use_in:
                s_in = sym_in
                if compact:
                    s_in = torch.zeros(shape, dtype=torch.int32, device=DEV)
                    s_in[:, cbase:cbase + n] = sym_in[:, ph, pw]
            ops.ar_quantize_batch(None if use_in else y, gp, pos, n, table, yh, sym, idx, symbols_in=s_in, cbase=cbase if compact else -1)
            ops.ar_indexes_batch(gp, pos, n, B, table, M, H, W, idx2, cbase=cbase if compact else -1)
            what = f"symbols_in={use_in} compact={compact}"
            assert torch.equal(yh.t, want_yh.t), what
            if compact:
                ws, wi = torch.full(shape, -9, dtype=torch.int32, device=DEV), torch.full(shape, -9, dtype=torch.int32, device=DEV)
                ws[:, cbase:cbase + n], wi[:, cbase:cbase + n] = want_sym[:, ph, pw], want_idx[:, ph, pw]
            else:
                ws, wi = want_sym, want_idx
            assert torch.equal(sym, ws) and torch.equal(idx, wi) and torch.equal(idx2, wi), what
        assert bool((want_idx[:, ph, pw] >= 0).all()) and (B == 1 or not torch.equal(want_sym[0], want_sym[1]))          # written, and the images differ
        assert int(ci.min()) == 0 and int(ci.max()) == table.numel() - 1 and bool((dense(want_yh) != 0).any())            # both ends of the table


def lane_case(coder, seed):
    """tests/test_ar_lanes_gpu.py's kernel_case for one image: 44 positions in three steps (1, 3, 40) of an 8 x 8 grid, scales over the
    whole table and beyond both ends, symbols inside and outside their tables, at least one bypass symbol per channel (hence per lane)"""
    _, gct, table = coder._coder_tables()
    tab = table.cpu().numpy()
    rng = np.random.default_rng(seed)
    npos = 44
    scale = np.exp(rng.uniform(np.log(0.02), np.log(600.0), (npos, M))).astype(np.float32)
    scale[0, :4] = [0.05, 0.11, 256.0, 1e4]
    mean = (rng.standard_normal((npos, M)) * 3).astype(np.float32)
    s = np.maximum(scale, np.float32(0.11))
    idx = (tab.size - 1 - (s[..., None] <= tab[None, None, :-1]).sum(-1)).astype(np.int32)
    assert idx.min() == 0 and idx.max() == tab.size - 1
    size, off = gct.sizes[idx], gct.offsets[idx]
    sym = (off + rng.integers(0, size - 1)).astype(np.int32)
    out = rng.random((npos, M)) < 0.04
    out[rng.integers(0, npos, M), np.arange(M)] = True
    far = np.where(rng.random((npos, M)) < 0.5, off - rng.integers(1, 3000, (npos, M)), off + size - 2 + rng.integers(0, 3000, (npos, M)))
    sym = np.where(out, far, sym).astype(np.int32)
    v = sym - off
    return dict(scale=scale, mean=mean, idx=idx, sym=sym, bypass=(v < 0) | (v >= size - 2))


@with_b1("lanes,f32", [(l, f) for f in (False, True) for l in (64, 128)])
def test_lane_decoder_batch(coder, lanes, f32, B):
    from tdvc_amd import ops
    _, gct, table = coder._coder_tables()
    steps, npos = [1, 3, 40], 44
    adt = adt_of(f32)
    cases = [lane_case(coder, 11 + 7 * b) for b in range(B)]
    assert B == 1 or not np.array_equal(cases[0]["sym"], cases[1]["sym"])
    perm = np.random.default_rng(1).permutation(64)[:npos]
    pos = torch.from_numpy(np.stack([perm // 8, perm % 8], 1).astype(np.int32)).to(DEV)          # one list for all images
    datas = []
    for k in cases:
        assert k["bypass"].reshape(npos, M // lanes, lanes).any((0, 1)).all(), "a lane without a bypass symbol"
        datas.append(ops.rans_encode_lanes(k["sym"], k["idx"], gct, lanes))
    assert B == 1 or len({len(d) for d in datas}) > 1 or datas[0] != datas[1]
    rows = [torch.from_numpy(np.concatenate([k["scale"], k["mean"]], 1)).to(DEV) for k in cases]
    # every image alone: a call of B = 1 with its own packed buffer and state
    single = []
    for b in range(B):
        sd, _ = ops.ar_lanes_pack_batch([datas[b]], lanes, DEV)
        state = ops.ar_lanes_state_batch(lanes, 1, DEV)
        ops.ar_lanes_init_batch(sd, 1, lanes, state)
        gp = ops.FM.empty(1, 1, max(steps), 2 * M, dtype=torch.float32, device=DEV)
        yh = ops.FM.zeros(1, 8, 8, M, dtype=adt, device=DEV)
        sym_d = torch.full((64, M), -12345, dtype=torch.int32, device=DEV)
        idx_d = torch.full((64, M), -12345, dtype=torch.int32, device=DEV)
        o = 0
        for n in steps:
            gp.t.view(-1, 2 * M)[:n] = rows[b][o:o + n]
            ops.ar_decode_lanes_step_batch(gp, pos[o:], n, table, sd, lanes, gct, state, yh, sym_d, idx_d, o)
            o += n
        single.append((sym_d, idx_d, yh.t, state[0]))
        assert np.array_equal(sym_d[:npos].cpu().numpy(), cases[b]["sym"]) and np.array_equal(idx_d[:npos].cpu().numpy(), cases[b]["idx"])
        want_yh = (torch.from_numpy(cases[b]["sym"]).float() + torch.from_numpy(cases[b]["mean"])).to(adt)          # q + mean in fp32, then y_hat's type
        assert torch.equal(yh.t[0, pos[:, 0].long(), pos[:, 1].long()].cpu(), want_yh), f"image {b}: y_hat"
    # all images in one call: B workgroups, rows image-major, y_hat a batch window of a larger buffer
    streams, tab = ops.ar_lanes_pack_batch(datas, lanes, DEV)
    assert all(off % 16 == 0 for off, _ in tab)
    state = ops.ar_lanes_state_batch(lanes, B, DEV)
    state.fill_(-1)
    ops.ar_lanes_init_batch(streams, B, lanes, state)
    gp = ops.FM.empty(1, 1, B * max(steps) + 2, 2 * M, dtype=torch.float32, device=DEV)
    big = torch.zeros((B + 1, 8, 8, M), dtype=adt, device=DEV)
    yh = ops.FM(big).batch(1, B)
    sym_d = torch.full((B, 64, M), -12345, dtype=torch.int32, device=DEV)
    idx_d = torch.full((B, 64, M), -12345, dtype=torch.int32, device=DEV)
    o = 0
    for n in steps:
        for b in range(B):
            gp.t.view(-1, 2 * M)[b * n:(b + 1) * n] = rows[b][o:o + n]
        ops.ar_decode_lanes_step_batch(gp, pos[o:], n, table, streams, lanes, gct, state, yh, sym_d, idx_d, o)
        o += n
    torch.cuda.synchronize()
    for b in range(B):
        s_sym, s_idx, s_yh, s_state = single[b]
        assert torch.equal(sym_d[b], s_sym), f"image {b}: symbols"
        assert torch.equal(idx_d[b], s_idx), f"image {b}: indexes"
        assert torch.equal(big[1 + b:2 + b], s_yh), f"image {b}: y_hat"
        assert torch.equal(state[b], s_state), f"image {b}: final lane states"
        assert int(state[b, -1]) == 0
    assert bool((sym_d[:, npos:] == -12345).all()) and bool((big[0] == 0).all()) and bool((big[1:] != 0).any())


# ---------------------------------------------------------------- coder level
def batch_input(B, H, W, seed=37):
    from tdvc_amd import ops
    x = rnd16(randn(B, 64, H, W, seed=seed, scale=0.5))
    assert not torch.equal(x[0], x[1])
    return x, to_fm(x, ops)


def set_batch(monkeypatch, on):
    from tdvc_amd.model import coder as cm
    monkeypatch.setattr(cm, "AR_BATCH", on)


def dbg_equal(a, b):
    return all(torch.equal(x["y_hat"].t, y["y_hat"].t) and torch.equal(x["symbols"], y["symbols"]) and torch.equal(x["indexes"], y["indexes"])
               for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("H,W", [(64, 64), (128, 192)])
def test_coder_batched_equals_per_image(coder, monkeypatch, H, W, B, f32, report):
    """The hardware test of row-count independence: the batched loop (rows = B x n per step) against the per-image loop (rows = n),
    encoder and all three decoder orders, and crosswise: batched encoder -> one-image decoder, one-image encoder -> batched decoder."""
    from tdvc_amd import ops
    m = coder
    x, xf = batch_input(B, H, W)
    singles = [to_fm(x[b:b + 1], ops) for b in range(B)]
    for order in ("raster", "wavefront", "lanes"):
        set_batch(monkeypatch, True)
        enc_b = m.compress(xf, f32=f32, order=order)
        set_batch(monkeypatch, False)
        enc_s = m.compress(xf, f32=f32, order=order)
        assert enc_b["strings"] == enc_s["strings"], f"{order}: strings"
        assert len(enc_b["strings"][0]) == B and len(set(enc_b["strings"][0])) == B
        assert dbg_equal(enc_b["_debug"], enc_s["_debug"]), f"{order}: encoder y_hat / symbols / indexes"
        want = torch.cat([d["y_hat"].t for d in enc_s["_debug"]], 0)
        dec_s = m.decompress(enc_s["strings"], enc_s["shape"], synth=False, f32=f32, order=order)
        set_batch(monkeypatch, True)
        dec_b = m.decompress(enc_b["strings"], enc_b["shape"], synth=False, f32=f32, order=order)
        assert torch.equal(dec_b["y_hat"].t, dec_s["y_hat"].t) and torch.equal(dec_b["y_hat"].t, want), f"{order}: decoder y_hat"
        # crosswise, every image alone through compress() / decompress() (calls of B = 1): what the batched
        # encoder wrote decodes one image at a time, what one-image encoders wrote decodes as a batch
        for b in range(B):
            d1 = m.decompress([[enc_b["strings"][0][b]], [enc_b["strings"][1][b]]], enc_b["shape"], synth=False, f32=f32, order=order)
            assert torch.equal(d1["y_hat"].t, want[b:b + 1]), f"{order}: batched encoder, image {b} decoded alone"
        one = [m.compress(singles[b], f32=f32, order=order) for b in range(B)]
        dec_x = m.decompress([[o["strings"][0][0] for o in one], [o["strings"][1][0] for o in one]], enc_b["shape"], synth=False, f32=f32, order=order)
        assert torch.equal(dec_x["y_hat"].t, torch.cat([o["_debug"][0]["y_hat"].t for o in one], 0)), f"{order}: one-image encoders, batched decoder"
    report(f"batched context loop {H}x{W} B={B} f32={f32}: strings, y_hat, symbols, indexes equal the per-image loop's in all three orders, both directions")


LOOPS = ("ar_wavefront_batch", "ar_wavefront_lanes_batch", "ar_decode_serial_batch")


@pytest.fixture
def loop_calls(monkeypatch):
    """every context-loop call made through ops, with what tdvc_ar_last_loop_launches() says right after it"""
    from tdvc_amd import ops
    calls = []

    def wrap(name, fn):
        def f(*a, **kw):
            r = fn(*a, **kw)
            calls.append((name, ops.ar_last_loop_launches()))
            return r
        return f
    for name in LOOPS:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return calls


def test_launch_count(coder, monkeypatch, loop_calls, report):
    """a batch of 3 costs the launches of one image: six per step for the encoder (gather, four convs, quantise); the decoders: seven
    per step on the host range decoder (indexes and quantise apart), a step being a position in raster order, and six per step plus
    the lane-state initialisation with the range decoder on the device"""
    from tdvc_amd import ops
    m = coder
    x, xf = batch_input(3, 64, 64)
    one = to_fm(x[:1], ops)
    nsteps = len(m.wavefront_steps(4, 4))

    def run(fm, batched, order, dec):
        set_batch(monkeypatch, batched)
        enc = m.compress(fm, order=order)
        if dec:
            del loop_calls[:]
            m.decompress(enc["strings"], enc["shape"], synth=False, order=order)
        got = list(loop_calls)
        del loop_calls[:]
        return got
    for order, dec in (("wavefront", False), ("raster", True), ("wavefront", True), ("lanes", True)):
        (n1, c1), = run(one, True, order, dec)
        (nb, cb), = run(xf, True, order, dec)
        per_image = run(xf, False, order, dec)
        report(f"loop launches {'decode ' + order if dec else 'encode'}: B=1 {c1} ({n1}), B=3 batched {cb} ({nb}), B=3 per image {[c for _, c in per_image]}")
        assert c1 > 0 and cb == c1 and nb == n1
        assert per_image == [(n1, c1)] * 3 and sum(c for _, c in per_image) == 3 * c1
        if not dec:
            assert c1 == 6 * nsteps
        else:
            assert c1 == {"wavefront": 7 * nsteps, "raster": 7 * 4 * 4, "lanes": 6 * nsteps + 1}[order]


def test_mixed_lane_counts(coder, monkeypatch):
    m = coder
    set_batch(monkeypatch, True)
    _, xf = batch_input(3, 64, 64, seed=43)
    e64, e128 = m.compress(xf, order="lanes", lanes=64), m.compress(xf, order="lanes", lanes=128)
    ys = [e64["strings"][0][0], e128["strings"][0][1], e64["strings"][0][2]]
    assert [s[2] for s in ys] == [64, 128, 64]
    dec = m.decompress([ys, e64["strings"][1]], e64["shape"], synth=False, order="lanes")
    assert torch.equal(dec["y_hat"].t, torch.cat([d["y_hat"].t for d in e64["_debug"]], 0))


def test_damaged_stream_names_the_image(coder, monkeypatch):
    """image 1 of 3: the last lane cut by one word (length table adjusted, so the host's container check passes); the lane runs out
    of words on the device, image 1's sticky error word comes back as a ValueError naming it, and the next call is exact"""
    m = coder
    set_batch(monkeypatch, True)
    _, xf = batch_input(3, 64, 64, seed=47)
    lanes = 64
    enc = m.compress(xf, order="lanes", lanes=lanes)
    ys = enc["strings"][0][1]
    cut = bytearray(ys[:-4])
    e = 4 + 2 * (lanes - 1)
    cut[e:e + 2] = (int.from_bytes(ys[e:e + 2], "little") - 1).to_bytes(2, "little")
    bad = [enc["strings"][0][0], bytes(cut), enc["strings"][0][2]]
    with pytest.raises(ValueError, match="image 1 "):
        m.decompress([bad, enc["strings"][1]], enc["shape"], synth=False, order="lanes")
    dec = m.decompress(enc["strings"], enc["shape"], synth=False, order="lanes")
    assert torch.equal(dec["y_hat"].t, torch.cat([d["y_hat"].t for d in enc["_debug"]], 0))


# ---------------------------------------------------------------- model and tool level
def test_model_encode_decode_batch(loop_calls, report):
    """VideoCompressor.encode / decode of a batch of 2 against two calls of 1: the networks run image by image (the forward conv
    dispatch counts pixels over the batch: at 64 x 64 a 64 -> 216 conv is on conv_mfma_v9 alone and on conv_mfma_v3 in a batch of 2),
    the two coders' context loops once for both images"""
    from tdvc_amd import synth
    from tdvc_amd.model import VideoCompressor
    net = VideoCompressor()
    synth.fill_parameters(net)
    net = net.cuda().eval()
    net.stream_order, net.stream_lanes = "lanes", 64
    gops = [synth.make_gop(78 + 5 * k, 3, 64, 64).cuda() for k in range(2)]
    assert not torch.equal(gops[0], gops[1])
    refs1 = [synth.ref_list([g[0:1], g[1:2]]) for g in gops]
    one = [net.encode(g[2:3], r) for g, r in zip(gops, refs1)]
    del loop_calls[:]
    x, refs = torch.cat([g[2:3] for g in gops]), torch.cat(refs1)
    enc = net.encode(x, refs)
    assert [n for n, _ in loop_calls] == ["ar_wavefront_batch"] * 2, loop_calls                 # both coders took the batched path
    for i in range(4):
        assert enc["strings"][i] == [one[0]["strings"][i][0], one[1]["strings"][i][0]], f"record {i}: strings[i][b] is image b's string"
    assert enc["shapes"] == one[0]["shapes"]
    assert torch.equal(enc["recon"], torch.cat([o["recon"] for o in one]))
    del loop_calls[:]
    dec = net.decode(enc["strings"], enc["shapes"], refs)
    assert [n for n, _ in loop_calls] == ["ar_wavefront_lanes_batch"] * 2, loop_calls
    assert torch.equal(dec, enc["recon"]), "decoder / encoder reconstruction mismatch"
    report(f"frame round trip B=2 64x64 lanes: {[len(s) for s in enc['strings'][0]]} + {[len(s) for s in enc['strings'][2]]} y bytes, equal to two B=1 calls")


def test_predict_gop_batch(tmp_path, monkeypatch, capsys):
    from tdvc_amd.tools import predict
    out = {}
    for k in (1, 2):
        d = tmp_path / f"k{k}"
        monkeypatch.setattr(sys, "argv", ["predict", "--gops", "2", "--gop-size", "3", "--height", "64", "--width", "64", "--bitstream-dir", str(d),
                                          "--stream-order", "lanes", "--gop-batch", str(k)])
        predict.main()
        res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        out[k] = ({f: (d / f).read_bytes() for f in sorted(os.listdir(d))}, res)
    files1, files2 = out[1][0], out[2][0]
    assert sorted(files1) == [f"gop{g:03d}_frame{t:03d}.bin" for g in range(2) for t in (1, 2)]
    assert files1 == files2, "the files of --gop-batch 2 differ from those of --gop-batch 1"
    assert files1["gop000_frame001.bin"] != files1["gop001_frame001.bin"]
    r1, r2 = out[1][1], out[2][1]
    assert r1["frames"] == r2["frames"] == 4 and r1["bytes"] == r2["bytes"] and r1["bpp"] == r2["bpp"] and r1["psnr"] == r2["psnr"]
