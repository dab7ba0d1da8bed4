"""CPU: the encoder of lane-split y streams that runs on the device, through its host twin tdvc_rans_encode_lanes_dev_ref.

The twin runs the encode-one-symbol routine of csrc/rans_lane.h with the kernel's traversal (lane l: positions last to first,
channels j * L + l from the highest j down), scratch layout (a region per lane, words written downward from its end) and
assembly, so these tests exercise ar_encode_lanes_batch_kernel's logic: byte equality with tdvc_rans_encode_lanes (the oracle),
extreme bypass symbols, a table whose last bin ends at 1 << 16, a lane above the length table's limit, a scratch region that
is too small (bounded writes: canaries), argument checks, and a sanitizer run of a stand-alone program
(tests/rans_lanes_enc_main.cpp; host compilation only, nothing sanitised is loaded here)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tdvc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 128
CANARY = 0xA5C3F00D


class Tables:
    """what ops.CdfTables holds, from numpy arrays"""

    def __init__(self, cdf, sizes, offsets):
        self.cdf = np.ascontiguousarray(cdf, dtype=np.int32)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.stride = self.cdf.shape[1]


def random_tables():
    """random tables as in test_rans_lanes_cpu.py"""
    from oracle.tdvc_ref import coder as oc
    rng = np.random.default_rng(5)
    ntab, width = 6, 40
    cdfs = np.zeros((ntab, width), dtype=np.int32)
    sizes = np.zeros(ntab, dtype=np.int32)
    offsets = -rng.integers(1, 12, ntab).astype(np.int32)
    for i in range(ntab):
        n = int(rng.integers(3, width - 2))
        p = rng.random(n) ** 3 + 1e-9
        c = oc.pmf_to_quantized_cdf((p / p.sum()).tolist(), 16)
        cdfs[i, : len(c)] = c
        sizes[i] = len(c)
    return Tables(cdfs, sizes, offsets)


@pytest.fixture(scope="module")
def tables():
    return random_tables()


def symbols_for(t, shape, seed):
    """indexes and symbols of `shape`, 3 % of them below and 3 % above the table (bypass digits)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(t.sizes), shape).astype(np.int32)
    lo = t.offsets[idx] - np.where(rng.random(idx.shape) < 0.03, 30, 0)
    hi = t.offsets[idx] + t.sizes[idx] - 2 + np.where(rng.random(idx.shape) < 0.03, 30, 0)
    return idx, rng.integers(lo, hi).astype(np.int32)


def wavefront(H, W):
    """the encoder's position list: anti-diagonals w + 3 h (Cheng2020Anchor.wavefront_steps)"""
    return np.array([(h, t - 3 * h) for t in range(W + 3 * (H - 1)) for h in range(H) if 0 <= t - 3 * h < W], dtype=np.int32).reshape(-1, 2)


def gathered(a, pos):
    """[H][W][M] -> [npos][M] in the order of the position list: what the host coder is given"""
    return np.ascontiguousarray(a[pos[:, 0], pos[:, 1]])


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (5, 7), (20, 30)])
def test_twin_bytes_equal_the_host_encoder(tables, grid, B, lanes):
    from tdvc_amd import ops
    H, W = grid
    pos = wavefront(H, W)
    idx, sym = symbols_for(tables, (B, H, W, M), 1000 * H + 10 * B + lanes)
    got = ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes)
    assert len(got) == B
    for b in range(B):
        assert got[b] == ops.rans_encode_lanes(gathered(sym[b], pos), gathered(idx[b], pos), tables, lanes), f"image {b} differs from tdvc_rans_encode_lanes"
    assert B == 1 or got[0] != got[1]


def extremes_image(t, H, W, seed):
    """symbols far outside every table, of both signs: 6 to 8 bypass digits"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(t.sizes), (H, W, M)).astype(np.int32)
    sym = rng.choice(np.array([10 ** 6, -10 ** 6, 2 ** 30 - 1, -2 ** 30], dtype=np.int32), (H, W, M))
    return idx, sym


def in_table_image(t, H, W, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(t.sizes), (H, W, M)).astype(np.int32)
    return idx, rng.integers(t.offsets[idx], t.offsets[idx] + t.sizes[idx] - 2).astype(np.int32)


@pytest.mark.parametrize("lanes", [64, 128])
def test_extremes_and_all_in_table_round_trip(tables, lanes):
    from oracle.tdvc_ref import coder as oc
    from tdvc_amd import ops
    H, W = 5, 7
    pos = wavefront(H, W)
    i0, s0 = in_table_image(tables, H, W, 11)
    i1, s1 = extremes_image(tables, H, W, 12)
    idx, sym = np.stack([i0, i1]), np.stack([s0, s1])
    v = s0 - tables.offsets[i0]
    assert ((v >= 0) & (v < tables.sizes[i0] - 2)).all()
    raw = np.where(s1 < tables.offsets[i1], -2 * (s1.astype(np.int64) - tables.offsets[i1]) - 1, 2 * (s1.astype(np.int64) - tables.offsets[i1] - (tables.sizes[i1] - 2)))
    digits = np.ceil(np.log2(raw + 1) / 4).astype(int)
    assert set(np.unique(digits)) == {6, 8} and raw.max() < 2 ** 32
    got = ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes)
    for b in range(2):
        assert np.array_equal(ops.rans_decode_lanes(got[b], gathered(idx[b], pos), tables), gathered(sym[b], pos)), f"image {b} does not round-trip"
        assert got[b] == ops.rans_encode_lanes(gathered(sym[b], pos), gathered(idx[b], pos), tables, lanes)
    lens = np.frombuffer(got[0][4:4 + 2 * lanes], dtype="<u2")
    assert lens.max() <= 2 + (H * W * (M // lanes) * 16 + 31) // 32                 # all in the table: at most 16 bits a symbol
    # lane 0 of the extremes image against the oracle's python coder, which has no word size to trip over
    cdf, sizes, offsets = tables.cdf.tolist(), tables.sizes.tolist(), tables.offsets.tolist()
    s, i = gathered(sym[1], pos)[:, 0::lanes].reshape(-1), gathered(idx[1], pos)[:, 0::lanes].reshape(-1)
    n0 = int(np.frombuffer(got[1][4:6], dtype="<u2")[0]) * 4
    assert got[1][4 + 2 * lanes:4 + 2 * lanes + n0] == oc.rans_encode(s.tolist(), i.tolist(), cdf, sizes, offsets)


def test_wide_table_every_bin_and_the_last_one():
    """the 2 400-entry wide-Gaussian table of test_search_equals_linear_scan_on_a_wide_table: every bin at least once, the
    width-1 bins and the last bin (whose upper edge is 1 << 16: 0 as a uint16) included"""
    from tdvc_amd import ops
    n = 2400
    x = np.arange(n) - n // 2
    p = np.exp(-0.5 * (x / 150.0) ** 2)
    cdf = ops.pmf_to_quantized_cdf(p / p.sum())
    w = np.diff(cdf)
    assert cdf.size == n + 1 and (w >= 1).all() and int((w == 1).sum()) > 200 and cdf[-1] == 1 << 16
    t = Tables(cdf[None, :], [cdf.size], [-n // 2])
    rng = np.random.default_rng(7)
    H, W = 4, 5
    # bins 0 .. n - 2 are table symbols, bin n - 1 (the last) is the escape bin: out-of-table symbols use it
    sym = np.concatenate([np.arange(n - 1), rng.choice(n - 1, H * W * M - (n - 1) - 40, p=p[:-1] / p[:-1].sum()), np.full(40, 4000)]).astype(np.int32) - n // 2
    sym = rng.permutation(sym).reshape(1, H, W, M)
    idx = np.zeros_like(sym)
    used = np.unique(np.clip(sym + n // 2, 0, n - 1))
    assert used.size == n                                                        # every bin, the last one included
    pos = wavefront(H, W)
    for lanes in (64, 128):
        got = ops.rans_encode_lanes_dev_ref(sym, idx, pos, t, lanes)[0]
        assert got == ops.rans_encode_lanes(gathered(sym[0], pos), gathered(idx[0], pos), t, lanes)
        assert np.array_equal(ops.rans_decode_lanes(got, gathered(idx[0], pos), t), gathered(sym[0], pos))


def test_lane_above_the_length_table_limit(tables):
    """constant 10 ** 6 symbols: 6 bypass digits and a count digit are 28 bits, the escape bin adds its own: more than 3.5 bytes
    a symbol whatever the table (about 6 was the estimate; the count below is taken from the bound, so that it holds)"""
    from tdvc_amd import ops
    lanes = 64
    per = M // lanes
    npos = int(np.ceil(65536 * 4 / (3.5 * per))) + 64                             # certainly above 65 535 words a lane
    H, W = 1, npos
    pos = np.stack([np.zeros(npos, dtype=np.int32), np.arange(npos, dtype=np.int32)], 1)
    sym = np.full((1, H, W, M), 10 ** 6, dtype=np.int32)
    idx = np.zeros_like(sym)
    with pytest.raises(ValueError, match="length table"):
        ops.rans_encode_lanes(sym[0, 0], idx[0, 0], tables, lanes)
    out, info, _ = ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes, raw=True)
    assert info.tolist() == [[0, 1]]
    with pytest.raises(ValueError, match="length table"):
        ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes)


def test_scratch_too_small_is_status_2_and_no_write_leaves_a_region(tables):
    lib = L.lib()
    lanes, B, H, W, words = 64, 2, 4, 4, 4
    pos = wavefront(H, W)
    idx, sym = symbols_for(tables, (B, H, W, M), 77)
    stride = (4 + 2 * lanes + 4 * lanes * words + 15) // 16 * 16
    scratch = np.full(B * lanes * words + 8, CANARY, dtype=np.uint32)            # canaries after the last region
    outbuf = np.full(B * stride + 64, 0xEE, dtype=np.uint8)
    o0 = (-outbuf.ctypes.data) % 16
    out = outbuf[o0:o0 + B * stride]
    info = np.full((B, 2), 0xFFFFFFFF, dtype=np.uint32)
    enc = L.LanesEncDesc(sym.ctypes.data, idx.ctypes.data, B, H, W, M, pos.ctypes.data, len(pos), lanes, scratch.ctypes.data, words, B * lanes * words,
                         out.ctypes.data, stride, B * stride, info.ctypes.data)
    tabs = L.CdfTablesDesc(tables.cdf.ctypes.data, tables.sizes.ctypes.data, tables.offsets.ctypes.data, tables.stride, len(tables.sizes))
    rc = lib.tdvc_rans_encode_lanes_dev_ref(C.byref(enc), C.byref(tabs))
    assert rc == 0
    assert info.tolist() == [[0, 2]] * B
    assert (scratch[B * lanes * words:] == CANARY).all()
    assert (outbuf[:o0] == 0xEE).all() and (outbuf[o0 + B * stride:] == 0xEE).all()
    assert (out == 0xEE).all()                                                   # a failed image writes nothing of its container
    # The regions are contiguous (the word after lane l's region is lane l + 1's own), so a canary cannot sit between them; what
    # stands in for it is stronger: every word of every region must be what that lane alone emits -- the first 4 words it emits
    # with enough scratch -- so a write of any lane into any other lane's region shows.
    from tdvc_amd import ops
    out2, info2, scr2 = ops.rans_encode_lanes_dev_ref(sym, idx, pos, tables, lanes, raw=True)
    assert (info2[:, 1] == 0).all()
    regions = scratch[:B * lanes * words].reshape(B, lanes, words)
    assert np.array_equal(regions, scr2[:, :, -words:])
    # and with enough scratch the words below each lane's cursor are untouched
    lens = np.stack([np.frombuffer(out2[b, 4:4 + 2 * lanes].tobytes(), dtype="<u2") for b in range(B)])
    for b in range(B):
        for l in range(lanes):
            assert (scr2[b, l, :scr2.shape[2] - lens[b, l]] == 0).all()


def test_bad_arguments_abi_and_the_scratch_helper(tables):
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 12
    for npos, m, lanes in [(1, 128, 64), (1, 128, 128), (16, 128, 64), (8160, 128, 128), (8160, 128, 64), (8160, 192, 64), (30000, 128, 64), (10 ** 7, 128, 128)]:
        n = npos * (m // lanes)
        want = min((31 + 52 * n) // 32 + 2, 65536)
        assert lib.tdvc_ar_encode_lanes_scratch_words(npos, m, lanes) == want
        assert lib.tdvc_ar_encode_lanes_out_bytes(npos, m, lanes) == (4 + 2 * lanes + 4 * lanes * min(want, 65535) + 15) // 16 * 16
    assert lib.tdvc_ar_encode_lanes_scratch_words(4, 96, 64) < 0
    # the device entry point validates before it touches a GPU: none of these may reach a launch
    good = np.zeros(64, dtype=np.uint8)
    p = good.ctypes.data + (-good.ctypes.data) % 16
    words = lib.tdvc_ar_encode_lanes_scratch_words(1, 128, 64)
    stride = lib.tdvc_ar_encode_lanes_out_bytes(1, 128, 64)

    def call(sym=p, idx=p, B=1, H=1, W=1, m=128, pos=p, npos=1, lanes=64, cdf16=p, n16=8, starts=p, sizes=p, offsets=p, ncdfs=1, scratch=p, lane_words=words,
             scratch_cap=64 * words, out=p, out_stride=stride, out_cap=stride, info=p):
        enc = L.LanesEncDesc(sym, idx, B, H, W, m, pos, npos, lanes, scratch, lane_words, scratch_cap, out, out_stride, out_cap, info)
        return lib.tdvc_ar_encode_lanes_batch(C.byref(enc), C.byref(L.CdfTablesDevDesc(cdf16, starts, sizes, offsets, n16, ncdfs)), None)
    bad = [dict(sym=None), dict(idx=None), dict(pos=None), dict(cdf16=None), dict(starts=None), dict(sizes=None), dict(offsets=None), dict(scratch=None),
           dict(out=None), dict(info=None), dict(B=0), dict(H=0), dict(npos=0), dict(lanes=32), dict(lanes=96), dict(m=192, lanes=128), dict(ncdfs=0),
           dict(ncdfs=65), dict(lane_words=1), dict(lane_words=65537), dict(scratch_cap=64 * words - 1), dict(out_stride=stride - 16), dict(out_stride=stride + 4),
           dict(out_cap=stride - 1), dict(out=p + 4), dict(sym=p + 1), dict(scratch=p + 2), dict(n16=12), dict(n16=1 << 20), dict(cdf16=p + 2)]
    for kw in bad:
        assert call(**kw) != 0, f"{kw} was accepted"
        assert b"tdvc_ar_encode_lanes_batch" in lib.tdvc_last_error()
    tabs = C.byref(L.CdfTablesDevDesc(p, p, p, p, 8, 1))
    for enc, t in ((None, tabs), (C.byref(L.LanesEncDesc()), None)):              # no descriptor at all
        assert lib.tdvc_ar_encode_lanes_batch(enc, t, None) != 0 and b"tdvc_ar_encode_lanes_batch" in lib.tdvc_last_error()
    from tdvc_amd import ops
    with pytest.raises(L.TdvcHipError):
        ops.rans_encode_lanes_dev_ref(np.zeros((1, 1, 1, 96), np.int32), np.zeros((1, 1, 1, 96), np.int32), np.zeros((1, 2), np.int32), tables, 64)


def test_standalone_program_under_address_and_ub_sanitizers(tmp_path):
    """tests/rans_lanes_enc_main.cpp + csrc/rans.cpp, compiled for the host with -fsanitize=address,undefined, run as a child process"""
    src = [os.path.join(ROOT, "tests", "rans_lanes_enc_main.cpp"), os.path.join(ROOT, "tdvc_amd", "csrc", "rans.cpp")]
    exe = str(tmp_path / "rans_lanes_enc_main")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # the compiler probe and skip rule of test_rans_lanes_cpu.py: only a failed probe skips
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    cxx = None
    for cand, extra in (("/opt/rocm/lib/llvm/bin/clang++", []), (shutil.which("c++"), ["-static-libasan", "-static-libubsan"]),
                        (shutil.which("g++"), ["-static-libasan", "-static-libubsan"])):
        if not cand or not os.path.exists(cand):
            continue
        r = subprocess.run([cand, *flags, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if r.returncode == 0:
            cxx, flags = cand, flags + extra
            break
        print(f"{cand}: probe failed: {r.stderr[-500:]}")
    if cxx is None:
        pytest.skip("no host compiler here accepts -fsanitize=address,undefined with a static runtime")
    r = subprocess.run([cxx, *flags, *src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, f"{cxx} accepts the sanitizer flags but does not build the program:\n{r.stderr[-4000:]}"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, "the sanitised encoder program failed"
    assert r.stdout.strip().endswith("ok")
