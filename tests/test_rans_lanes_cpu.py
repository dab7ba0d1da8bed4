"""CPU: the lane-split y stream (order="lanes") on the host: tdvc_rans_encode_lanes / tdvc_rans_decode_lanes.

The host decoder runs the decode-one-symbol routine of csrc/rans_lane.h, which is also what ar_decode_lanes_kernel runs per
thread, so these tests exercise the kernel's logic: container layout, byte equality of every lane with the oracle's python
coder, equivalence of the O(log n) bin search with the single-stream decoder's linear scan, damaged streams, and a
sanitizer run of a stand-alone program (tests/rans_lanes_main.cpp; host compilation only, nothing sanitised is loaded here)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tdvc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 128


class Tables:
    """what ops.CdfTables holds, from numpy arrays"""

    def __init__(self, cdf, sizes, offsets):
        self.cdf = np.ascontiguousarray(cdf, dtype=np.int32)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.stride = self.cdf.shape[1]

    def lists(self):
        return self.cdf.tolist(), self.sizes.tolist(), self.offsets.tolist()


@pytest.fixture(scope="module")
def tables():
    """random tables as in test_lib_abi.py::test_rans_c_matches_oracle_bitstream"""
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


def symbols_for(t, npos, seed):
    """[npos][M] indexes and symbols, 3 % of them below and 3 % above the table (bypass digits)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(t.sizes), (npos, M)).astype(np.int32)
    lo = t.offsets[idx] - np.where(rng.random(idx.shape) < 0.03, 30, 0)
    hi = t.offsets[idx] + t.sizes[idx] - 2 + np.where(rng.random(idx.shape) < 0.03, 30, 0)
    return idx, rng.integers(lo, hi).astype(np.int32)


def split(data, lanes):
    """-> the lanes' payloads, after checking header and length table"""
    assert data[:4] == bytes([ord("L"), 1, lanes, 0])
    lens = np.frombuffer(data[4:4 + 2 * lanes], dtype="<u2").astype(np.int64) * 4
    assert 4 + 2 * lanes + int(lens.sum()) == len(data)
    o = np.concatenate([[0], np.cumsum(lens)]) + 4 + 2 * lanes
    return [data[o[l]:o[l + 1]] for l in range(lanes)]


@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("npos", [1, 16, 600])
def test_roundtrip_and_lane_bytes_equal_oracle(tables, npos, lanes):
    from oracle.tdvc_ref import coder as oc
    from tdvc_amd import ops
    idx, sym = symbols_for(tables, npos, 100 + npos)
    data = ops.rans_encode_lanes(sym, idx, tables, lanes)
    assert np.array_equal(ops.rans_decode_lanes(data, idx, tables), sym)
    cdf, sizes, offsets = tables.lists()
    parts = split(data, lanes)
    nbypass = 0
    for l, part in enumerate(parts):
        s, i = sym[:, l::lanes].reshape(-1), idx[:, l::lanes].reshape(-1)         # lane l: position by position, c = l, l + L, ...
        assert part == oc.rans_encode(s.tolist(), i.tolist(), cdf, sizes, offsets), f"lane {l} differs from the oracle coder"
        v = s - tables.offsets[i]
        nbypass += int(((v < 0) | (v >= tables.sizes[i] - 2)).any())
    if npos >= 600:
        assert nbypass > lanes // 2                                              # bypass digits occur in most lanes
    single = ops.rans_encode(sym, idx, tables)                                   # the "wavefront" string of the same symbols
    print(f"lanes={lanes} npos={npos}: {len(data)} B lane-split vs {len(single)} B single stream "
          f"(+{len(data) - len(single)}, bound +{4 + 14 * lanes}); lanes with bypass symbols {nbypass}/{lanes}")
    assert len(data) <= len(single) + 4 + 14 * lanes


def test_search_equals_linear_scan_on_a_wide_table():
    """a 2 400-entry table of a wide Gaussian: most tail bins come out of pmf_to_quantized_cdf with width 0 and are repaired to
    width 1; the binary search must land on the bin the single-stream decoder's linear scan finds"""
    from tdvc_amd import ops
    lib = L.lib()
    n = 2400
    x = np.arange(n) - n // 2
    p = np.exp(-0.5 * (x / 150.0) ** 2)
    cdf = ops.pmf_to_quantized_cdf(p / p.sum())
    w = np.diff(cdf)
    assert cdf.size == n + 1 and (w >= 1).all() and int((w == 1).sum()) > 200
    t = Tables(cdf[None, :], [cdf.size], [-n // 2])
    rng = np.random.default_rng(7)
    npos = 64
    idx = np.zeros((npos, M), dtype=np.int32)
    # every bin at least once (the width-1 ones included), the rest drawn from the distribution; some out of the table
    sym = np.concatenate([np.arange(n - 1), rng.choice(n - 1, npos * M - (n - 1), p=p[:-1] / p[:-1].sum())]).astype(np.int32) - n // 2
    sym[rng.random(sym.size) < 0.01] += 4000
    sym = rng.permutation(sym).reshape(npos, M)
    one = ops.rans_encode_lanes(sym, idx, t, 1)                                  # L = 1: host only
    assert one[:4] == bytes([ord("L"), 1, 1, 0]) and one[6:] == ops.rans_encode(sym, idx, t)
    want = np.zeros(sym.size, dtype=np.int32)
    buf = np.frombuffer(one[6:], dtype=np.uint8)
    assert lib.tdvc_rans_decode(buf.ctypes.data, buf.size, idx.ctypes.data, idx.size, t.cdf.ctypes.data, t.stride, t.sizes.ctypes.data,
                                t.offsets.ctypes.data, want.ctypes.data) == 0
    assert np.array_equal(want.reshape(sym.shape), sym)
    assert np.array_equal(ops.rans_decode_lanes(one, idx, t), want.reshape(sym.shape))
    for lanes in (64, 128):
        assert np.array_equal(ops.rans_decode_lanes(ops.rans_encode_lanes(sym, idx, t, lanes), idx, t), sym)


def test_damaged_streams_are_errors(tables):
    from tdvc_amd import ops
    lanes = 64
    idx, sym = symbols_for(tables, 16, 3)
    data = ops.rans_encode_lanes(sym, idx, tables, lanes)
    assert np.array_equal(ops.rans_decode_lanes(data, idx, tables), sym)
    off = 4 + 2 * lanes
    cut = bytearray(data[:-4])                                                   # last lane cut by a word, length table adjusted
    cut[4 + 2 * (lanes - 1):off] = (int.from_bytes(data[4 + 2 * (lanes - 1):off], "little") - 1).to_bytes(2, "little")
    damaged = {
        "truncated by 4 bytes": data[:-4],
        "length entry larger than the remainder": data[:4] + b"\xff\xff" + data[6:],
        "wrong magic byte": b"M" + data[1:],
        "wrong version": data[:1] + b"\x02" + data[2:],
        "payload of 0xFF bytes": data[:off] + b"\xff" * (len(data) - off),
        "last lane one word short": bytes(cut),
        "header only": data[:4],
        "empty": b"",
    }
    for what, d in damaged.items():
        with pytest.raises(RuntimeError):
            ops.rans_decode_lanes(d, idx, tables)
            print(f"{what}: decoded without an error")
    # L not dividing M: on both sides
    with pytest.raises(ValueError):
        ops.rans_encode_lanes(sym, idx, tables, 48)
    with pytest.raises(RuntimeError):
        ops.rans_decode_lanes(data[:2] + bytes([48]) + data[3:], idx, tables)
    with pytest.raises(RuntimeError):
        ops.rans_decode_lanes(data, idx[:, :96], tables)                         # M = 96 against 64 lanes
    assert np.array_equal(ops.rans_decode_lanes(data, idx, tables), sym)         # and the library is none the worse


def test_lane_length_limit_is_an_error(tables):
    """a lane of more than 65 535 words does not fit the uint16 length table"""
    from tdvc_amd import ops
    npos = 1200
    idx = np.zeros((npos, M), dtype=np.int32)
    sym = np.full((npos, M), 10 ** 6, dtype=np.int32)                            # 7 bypass digits each: ~6 bytes a symbol
    with pytest.raises(ValueError, match="length table"):
        ops.rans_encode_lanes(sym, idx, tables, 1)
    assert len(ops.rans_encode_lanes(sym, idx, tables, 128)) > 4 * 65535


def test_abi_version_covers_the_lane_entry_points():
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 6
    assert lib.tdvc_ar_lanes_state_bytes(64) == 4 * (4 * 64 + 1)
    # the device entry points validate before they touch the GPU
    assert lib.tdvc_ar_lanes_init_batch(None, 0, None, 1, 64, None, None) != 0
    assert lib.tdvc_ar_wavefront_lanes_batch(None, None, None, None, 0, None, None, None, None) != 0
    assert lib.tdvc_ar_wavefront_lanes_batch(C.byref(L.ArLoopDesc()), None, None, None, 0, None, None, None, None) != 0


def test_standalone_program_under_address_and_ub_sanitizers(tmp_path):
    """tests/rans_lanes_main.cpp + csrc/rans.cpp, compiled for the host with -fsanitize=address,undefined, run as a child process"""
    src = [os.path.join(ROOT, "tests", "rans_lanes_main.cpp"), os.path.join(ROOT, "tdvc_amd", "csrc", "rans.cpp")]
    exe = str(tmp_path / "rans_lanes_main")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    # A compiler qualifies if it builds an empty program with the flags and links the sanitizer runtime statically (clang's
    # default; gcc with -static-lib*san), so the child runs in this process's environment as it is.  Only a failed probe
    # skips; once a compiler qualified, a failed build of the real sources is a failure.
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
    assert r.returncode == 0, "the sanitised round-trip program failed"
    assert r.stdout.strip().endswith("ok")
