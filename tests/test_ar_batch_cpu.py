"""The context loop (tdvc_ar_*_batch; one image is B = 1), the parts that need no GPU: the ABI, the drivers' argument checks (every rejection is made before
anything touches a device: TDVC_EINVAL with a message, never a HIP error code) and the row-count guard -- the table of kernels
tdvc_conv_select names for the loop's four conv descriptors, and the grouping built on it."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_conv_dispatch as H
from tdvc_amd import _lib as L
from tdvc_amd import ops

M = 128
EINVAL = -1
BATCH_SYMBOLS = ["tdvc_ar_gather_batch", "tdvc_ar_quantize_batch", "tdvc_ar_indexes_batch", "tdvc_ar_wavefront_batch", "tdvc_ar_decode_serial_batch",
                 "tdvc_ar_lanes_batch_layout", "tdvc_ar_lanes_init_batch", "tdvc_ar_decode_lanes_step_batch", "tdvc_ar_wavefront_lanes_batch",
                 "tdvc_ar_last_loop_launches"]
# the single-image entry points ABI 10 removed: B = y_hat->N = 1 of the above is the single image
REMOVED_SYMBOLS = ["tdvc_ar_gather", "tdvc_ar_quantize", "tdvc_ar_indexes", "tdvc_ar_lanes_init", "tdvc_ar_decode_lanes_step", "tdvc_ar_decode_serial",
                   "tdvc_ar_wavefront", "tdvc_ar_wavefront_lanes"]


def test_abi_and_symbols():
    lib = L.lib()
    assert lib.tdvc_abi_version() >= 10
    for s in BATCH_SYMBOLS:
        assert hasattr(lib, s) and s in L.SIGNATURES, s
    for f in ("ar_gather_batch", "ar_quantize_batch", "ar_indexes_batch", "ar_wavefront_batch", "ar_decode_serial_batch", "ar_lanes_init_batch",
              "ar_decode_lanes_step_batch", "ar_wavefront_lanes_batch", "ar_last_loop_launches", "ar_batch_groups"):
        assert callable(getattr(ops, f))
    assert issubclass(L.TdvcStreamError, ValueError) and issubclass(L.TdvcStreamError, L.TdvcHipError)
    assert lib.tdvc_ar_last_loop_launches() >= 0


def test_single_image_entry_points_are_gone():
    lib = L.lib()
    for s in REMOVED_SYMBOLS:
        assert not hasattr(lib, s), f"{s} is still exported"
        assert s not in L.SIGNATURES, f"{s} still has a signature"
        assert not hasattr(ops, s[len("tdvc_"):]), f"ops.{s[len('tdvc_'):]} is still there"


# ---------------------------------------------------------------- driver validation
# an 8 x 8 grid, B = 3 or 1: fmaps over dummy addresses (never dereferenced: every call below is rejected before a device is touched)
HG, WG = 8, 8


def chain_descs(rows=1, f32=False):
    """the loop's four conv descriptors at M = 128 as Cheng2020Anchor._ar_chain builds them: context conv as a 1x1 over the 12
    gathered taps into pc[2M:4M], entropy_parameters 4M -> 10M/3 -> 8M/3 -> 2M (fp32 out)"""
    w1 = (1, 1, 1, 0, None)
    o = "f32" if f32 else "f16"
    d = [H.desc(L, ops._pick_ck, 12 * M, 2 * M, w1, 1, rows, 1, out=o, x_f32=f32),
         H.desc(L, ops._pick_ck, 4 * M, M * 10 // 3, w1, 1, rows, 1, act=2, slope=0.01, out=o, x_f32=f32),
         H.desc(L, ops._pick_ck, ops.pad8(M * 10 // 3), M * 8 // 3, w1, 1, rows, 1, act=2, slope=0.01, out=o, x_f32=f32),
         H.desc(L, ops._pick_ck, ops.pad8(M * 8 // 3), 2 * M, w1, 1, rows, 1, out="f32", x_f32=f32)]
    d[0].y.sp = 4 * M                                                 # a channel window of pc
    return d


def wavefront_sizes(h, w):
    return np.array([sum(1 for y in range(h) if 0 <= t - 3 * y < w) for t in range(w + 3 * (h - 1))], dtype=np.int32)


def lane_string(lanes, seed):
    """a valid lane-split container of HG * WG positions (host coder; two tables)"""
    rng = np.random.default_rng(seed)
    cdf = torch.tensor([[0, 20000, 50000, 65536, 0], [0, 1000, 30000, 60000, 65536]], dtype=torch.int32)
    t = ops.CdfTables(cdf, torch.tensor([4, 5]), torch.tensor([-1, -2]))
    idx = rng.integers(0, 2, (HG * WG, M)).astype(np.int32)
    sym = (t.offsets[idx] + rng.integers(0, 2, idx.shape)).astype(np.int32)
    return ops.rans_encode_lanes(sym, idx, t, lanes), t


class Call:
    """the arguments of one driver for B images, valid by default; `run()` -> (rc, message)"""

    def __init__(self, driver, B):
        self.driver = driver
        CAP = B * 3                                                   # staging rows: B x the largest step (3 positions at 8 x 8)
        self.fm = dict(y=H.fmap(L, H.PX, B, HG, WG, M, dtype=L.F32), y_hat=H.fmap(L, H.PY, B, HG, WG, M), params=H.fmap(L, H.PAUX, B, HG, WG, 2 * M),
                       x1=H.fmap(L, H.PR1, 1, 1, CAP, 12 * M), pc=H.fmap(L, H.PR2, 1, 1, CAP, 4 * M), gp=H.fmap(L, H.PW, 1, 1, CAP, 2 * M, dtype=L.F32))
        self.sizes = wavefront_sizes(HG, WG)
        self.B = B
        self.strings = None
        self.null = ()
        self.null_loop = False
        self.table = None
        if driver == "tdvc_ar_wavefront_lanes_batch":
            pairs = [lane_string(64, s) for s in range(B)]
            self.strings, self.table = [p[0] for p in pairs], pairs[0][1]
        elif driver == "tdvc_ar_decode_serial_batch":
            self.strings = [bytes(16)] * B
            self.sizes = np.ones(HG * WG, dtype=np.int32)

    def run(self):
        lib = L.lib()
        fm = {k: L.FMapDesc.from_buffer_copy(v) for k, v in self.fm.items()}
        for k in self.null:                                           # a null map: one whose p is NULL
            fm[k].p = None
        if self.B != self.fm["params"].N:                             # a bad B: the drivers read it from the maps' N
            for k in ("y", "y_hat", "params"):
                fm[k].N = self.B
        descs = chain_descs()
        arr = (L.ConvDesc * 4)(*descs)
        dummy = H.PB
        ss = np.ascontiguousarray(self.sizes, dtype=np.int32)
        serial = self.driver == "tdvc_ar_decode_serial_batch"         # raster order: no step list, a step per position
        loop = L.ArLoopDesc(fm["y_hat"], fm["params"], fm["x1"], fm["pc"], fm["gp"], arr, 4, dummy, None if serial else ss.ctypes.data,
                            int(ss.sum()) if serial else ss.size, dummy, 64, dummy, dummy)
        lp = None if self.null_loop else C.byref(loop)
        if self.strings is not None:
            keep, ptrs, nbytes = ops._host_strings(self.strings)
        tab = np.zeros((4, 8), dtype=np.int32)
        host = L.CdfTablesDesc(tab.ctypes.data, tab.ctypes.data, tab.ctypes.data, 8, 4)
        if self.driver == "tdvc_ar_wavefront_batch":                  # encoder direction
            rc = lib.tdvc_ar_wavefront_batch(lp, C.byref(fm["y"]), None, None, None, None)
        elif serial:
            rc = lib.tdvc_ar_decode_serial_batch(lp, ptrs, nbytes, C.byref(host), None)
        else:
            dev = L.CdfTablesDevDesc(dummy, dummy, dummy, dummy, 27256 // 8 * 8, 64)
            rc = lib.tdvc_ar_wavefront_lanes_batch(lp, ptrs, nbytes, dummy, 1 << 30, dummy, C.byref(dev), None, None)
        return rc, lib.tdvc_last_error().decode()


DRIVERS = ["tdvc_ar_wavefront_batch", "tdvc_ar_decode_serial_batch", "tdvc_ar_wavefront_lanes_batch"]


# B = 3 under the ids the cases had before a single image became B = 1 of these drivers; B = 1 as "<driver>-B1"
@pytest.mark.parametrize("driver,B", [pytest.param(d, B, id=d if B == 3 else d + "-B1") for B in (3, 1) for d in DRIVERS])
def test_driver_rejects_before_touching_a_device(driver, B):
    def rejected(c, word):
        rc, msg = c.run()
        assert rc == EINVAL, f"{driver}: rc {rc} ({msg}): a HIP error code means the call reached a device"
        assert driver in msg and word in msg, msg

    for name in ("y_hat", "params", "x1", "pc", "gp"):
        c = Call(driver, B)
        c.null = (name,)
        rejected(c, "null")
    c = Call(driver, B)                                               # no loop descriptor at all
    c.null_loop = True
    rejected(c, "null")
    for bad in (0, -2):
        c = Call(driver, B)
        c.B = bad
        rejected(c, "images expected")
    c = Call(driver, B)                                               # the steps do not cover H x W
    if driver == "tdvc_ar_decode_serial_batch":
        c.sizes = c.sizes[:-1]
    else:
        c.sizes = c.sizes.copy()
        c.sizes[5] -= 1
    rejected(c, "cover every position")
    c = Call(driver, B)                                               # B * n beyond the staging width
    width = B * int(c.sizes.max()) - 1                                # one row short of the largest step of the batch
    for k in ("x1", "pc", "gp"):
        c.fm[k].W = width
    rejected(c, "exceed the staging buffers")
    for k in ("x1", "pc", "gp"):                                      # each buffer alone, too
        c = Call(driver, B)
        c.fm[k].W = width
        rejected(c, "exceed the staging buffers")
    c = Call(driver, B)                                               # a batch of another size than the fmaps'
    c.fm["y_hat"].N = B - 1
    rejected(c, "fmaps of B")


def test_lanes_driver_rejects_unequal_lane_counts_and_bad_strings():
    c = Call("tdvc_ar_wavefront_lanes_batch", 3)
    c.strings[1] = lane_string(128, 9)[0]
    rc, msg = c.run()
    assert rc == EINVAL and "image 1 declares 128 lanes, image 0 64" in msg, (rc, msg)
    c = Call("tdvc_ar_wavefront_lanes_batch", 3)
    c.strings[2] = c.strings[2][:-4]                                  # the length table no longer adds up
    rc, msg = c.run()
    assert rc == EINVAL and "image 2" in msg, (rc, msg)


def test_lanes_batch_layout():
    total, table = ops.ar_lanes_batch_layout([4 + 128 + 400, 4 + 128 + 8, 4 + 128 + 4000], 64)
    assert table.tolist() == [[32, 100], [32 + 544, 2], [32 + 544 + 144, 1000]] and total == 32 + 544 + 144 + 4144
    assert all(off % 16 == 0 for off, _ in table)
    with pytest.raises(L.TdvcHipError):
        ops.ar_lanes_batch_layout([4 + 128 + 3], 64)                  # not a whole number of words


# ---------------------------------------------------------------- the row-count guard
V9_WORK_LIMIT = 1 << 20            # conv_v9_work_limit(): pixels x cout above which v9 yields to v3 WHERE v3 IS ELIGIBLE
LARGE_MAP_PIXELS = 8192            # conv_v9_eligible leaves v9 above this many pixels


def test_guard_table():
    """The guard, as a table.  One kernel for all four descriptors at 1 row, at 40 rows (the largest 1080p step) and at 4 and 8
    times that.  conv_mfma_v3 takes no 1x1 conv (it needs >= 2 taps), so the work limit never moves these four: one row past
    conv_v9_work_limit() / cout they are still on v9; what does move them is LARGE_MAP_PIXELS, which every such row count beyond
    8192 is past as well -- there the selection changes, and the grouping answers with smaller groups."""
    for f32, want in ((False, "conv_mfma_v9"), (True, "conv_f32")):
        d = chain_descs(f32=f32)
        for rows in (1, 40, 160, 320):
            assert ops.ar_chain_kernels(d, rows) == (want,) * 4, (f32, rows)
    d = chain_descs()
    couts = [x.cout for x in d]
    assert couts == [256, 426, 341, 256]
    for cout in couts:
        assert ops.ar_chain_kernels(d, V9_WORK_LIMIT // cout + 1) == ("conv_mfma_v9",) * 4
    assert ops.ar_chain_kernels(d, LARGE_MAP_PIXELS) == ("conv_mfma_v9",) * 4
    past = LARGE_MAP_PIXELS + 1
    assert past > V9_WORK_LIMIT // min(couts)
    assert all(k != "conv_mfma_v9" and k is not None for k in ops.ar_chain_kernels(d, past))
    # the fp32 islands have one kernel at any size
    assert ops.ar_chain_kernels(chain_descs(f32=True), past) == ("conv_f32",) * 4


def test_grouping():
    d = chain_descs()
    assert ops.ar_batch_groups(d, 1, 40) == [1]
    assert ops.ar_batch_groups(d, 8, 40) == [8]
    assert ops.ar_batch_groups(d, 8, 1024) == [8]                     # 8192 rows: still one kernel
    assert ops.ar_batch_groups(d, 8, 1100) == [7, 1]                  # 8800 rows would leave v9: 7 x 1100 = 7700 do not
    assert ops.ar_batch_groups(d, 8, 3000) == [2, 2, 2, 2]
    assert ops.ar_batch_groups(d, 3, 5000) == [1, 1, 1]
    assert ops.ar_batch_groups(d, 3, 9000) == [1, 1, 1]               # the single image is already past it: today's path
    assert ops.ar_batch_groups(chain_descs(f32=True), 8, 9000) == [8]
    assert not ops.ar_batch_ok(d, 2, 5000) and ops.ar_batch_ok(d, 2, 4096)
    # with the switch off every image is its own group
    from tdvc_amd.model import coder
    old = coder.AR_BATCH
    try:
        coder.AR_BATCH = False
        assert coder.Cheng2020Anchor._ar_groups(d, 4, 40) == [1] * 4
        coder.AR_BATCH = True
        assert coder.Cheng2020Anchor._ar_groups(d, 4, 40) == [4]
    finally:
        coder.AR_BATCH = old
