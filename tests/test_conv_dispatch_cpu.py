"""CPU: which kernel tdvc_conv2d picks is pure host arithmetic on the descriptor.  tdvc_conv_select (no device, no launch) and
tdvc_conv_chan_sum_rows are held, over the whole sweep of tests/helpers_conv_dispatch.py and with every debug switch turned off in
turn, to tests/golden/conv_dispatch.npz -- recorded by tests/golden/make_conv_dispatch.py from the `if` cascade that the dispatch
table replaced."""
import ctypes as C
import os

import numpy as np
import pytest

from tdvc_amd import _lib as L, ops

from tests import helpers_conv_dispatch as H


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", H.GOLDEN))
    return dict(names=[str(n) for n in g["names"]], kernel=g["kernel"], rows=g["rows"], sw_kernel=g["sw_kernel"], sw_rows=g["sw_rows"])


@pytest.fixture(scope="module")
def swept():
    return H.sweep(L, ops._pick_ck)


def select(lib, d):
    name = lib.tdvc_conv_select(C.byref(d))
    if name is None:
        assert lib.tdvc_last_error(), "a rejected descriptor leaves its reason in tdvc_last_error()"
        return H.REJECTED
    return name.decode()


def mismatches(lib, descs, names, kernel, rows):
    bad = []
    for i, d in enumerate(descs):
        got = (select(lib, d), lib.tdvc_conv_chan_sum_rows(C.byref(d)))
        want = (names[kernel[i]], int(rows[i]))
        if got != want:
            bad.append((i, got, want))
    return bad


def test_golden_reaches_every_outcome(golden, swept):
    descs, subset = swept
    assert len(golden["kernel"]) == len(golden["rows"]) == len(descs)                     # nothing skipped
    assert golden["sw_kernel"].shape == golden["sw_rows"].shape == (len(H.SWITCHES), len(subset))
    count = {o: 0 for o in H.OUTCOMES}
    for k in golden["kernel"]:
        count[H.outcome(golden["names"][k])] += 1
    assert min(count.values()) >= H.MIN_PER_OUTCOME, count
    assert (golden["rows"] > 0).any() and (golden["rows"][golden["kernel"] == golden["names"].index(H.REJECTED)] <= 0).all()
    for s, (setter, off, _) in enumerate(H.SWITCHES):                                     # every switch decides something in its subset
        assert (golden["sw_kernel"][s] != golden["kernel"][subset]).any(), (setter, off)


def test_selection_matches_the_recorded_dispatch(golden, swept):
    descs, _ = swept
    bad = mismatches(L.lib(), descs, golden["names"], golden["kernel"], golden["rows"])
    assert not bad, f"{len(bad)} of {len(descs)} descriptors differ, first (index, got, recorded): {bad[:5]}"


@pytest.mark.parametrize("s", range(len(H.SWITCHES)), ids=[f"{n[len('tdvc_debug_enable_'):]}={off}" for n, off, _ in H.SWITCHES])
def test_selection_with_one_kernel_switched_off(golden, swept, s):
    descs, subset = swept
    setter, off, on = H.SWITCHES[s]
    lib = L.lib()
    getattr(lib, setter)(off)
    try:
        bad = mismatches(lib, [descs[i] for i in subset], golden["names"], golden["sw_kernel"][s], golden["sw_rows"][s])
    finally:
        getattr(lib, setter)(on)
    assert not bad, f"{len(bad)} of {len(subset)} descriptors differ, first (index in the subset, got, recorded): {bad[:5]}"


def test_select_is_a_pure_query():
    """no launch is attempted (tdvc_conv2d on this descriptor would fail for want of a device, or launch), the name of the last
    launch is left alone, and a rejection reports NULL + reason instead of a stale name"""
    lib = L.lib()
    before = lib.tdvc_last_conv_kernel()
    d = H.desc(L, ops._pick_ck, 64, 64, H.WINDOWS[1], 272, 480, 1, act=1)
    assert lib.tdvc_conv_select(C.byref(d)) == b"conv_row"
    d.stride = 3
    assert lib.tdvc_conv_select(C.byref(d)) is None and b"stride" in lib.tdvc_last_error()
    assert lib.tdvc_conv_select(None) is None
    assert lib.tdvc_last_conv_kernel() == before
