"""LoopFilter's slot ring (tdvc_amd/model/ring.py): where a call's window lies and which of its slots are forced.  The model here is
independent of the class: it tracks, per slot, WHAT the slot holds (a frame id, prediction1's maps, or nothing)."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "tdvc_ring", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tdvc_amd", "model", "ring.py"))
ring = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ring)

EMPTY, PRED = "empty", "pred"


def _ref_lists(gops):
    """reference slices [r-3, r-2, r-1] of the P-frames of GOPs of the given lengths, by the rule of synth.ref_list"""
    calls = []
    for g, nframes in enumerate(gops):
        refs = [f"I{g}"]
        for t in range(1, nframes):
            if len(refs) == 1:
                calls.append([refs[0]] * 3)
            elif len(refs) == 2:
                calls.append([refs[-2], refs[-1], refs[-1]])
            else:
                calls.append(refs[-3:])
            refs.append(f"x{g}.{t}")
    return calls


def _drive(slots, calls):
    """-> per call (p, mask, hits): hits = slices whose slot is offered unforced AND holds that very frame"""
    r = ring.SlotRing(slots)
    holds = [EMPTY] * slots
    out = []
    for want in calls:
        p, mask = r.begin()
        assert 0 <= p and p + ring.WINDOW <= slots, "the window never exceeds the ring"
        hits = 0
        for j in range(3):
            forced = bool(mask >> j & 1)
            if not forced:
                assert holds[p + j] not in (EMPTY, PRED), f"slot {p + j} offered unforced while it holds {holds[p + j]}"
                hits += holds[p + j] == want[j]
            holds[p + j] = want[j]
        holds[p + 3] = PRED
        r.commit()
        out.append((p, mask, hits))
    return out


def test_sliding_sequence_ring9_matches_the_gop_of_the_benchmark():
    """7-frame GOPs, 9 slots: the window wraps exactly at the GOP boundary; hits 0 1 1 2 2 2 in every GOP"""
    got = _drive(9, _ref_lists([7, 7, 7]))
    assert [p for p, _, _ in got] == [0, 1, 2, 3, 4, 5] * 3
    assert [h for _, _, h in got] == [0, 1, 1, 2, 2, 2] * 3
    assert [m for _, m, _ in got] == [0b111, 0b100, 0b100, 0b100, 0b100, 0b100] * 3


def test_ring5_sliding_restart_and_wraps():
    """two window positions: every second call is a wrap and recomputes everything; in between the two older slices are offered"""
    calls = _ref_lists([6, 4, 9])                  # a GOP restart in the middle of a ring pass, several wraps
    got = _drive(5, calls)
    assert [p for p, _, _ in got] == [i % 2 for i in range(len(calls))]
    for i, (p, mask, hits) in enumerate(got):
        if p == 0:
            assert mask == 0b111 and hits == 0, f"call {i + 1}: the wrap forgets every slot"
        else:
            assert mask == 0b100, f"call {i + 1}: slot p + 2 held prediction1's maps"
    # what is offered is found where the list really slid by one: call 2 ([I,x1,x1] after [I,I,I]) finds its I, call 4 ([x1,x2,x3] after
    # [I,x1,x2]) both frames; the first call of a new GOP behind an odd call finds nothing
    assert got[1][2] == 1 and got[3][2] == 2
    first_of_gop2 = 5
    assert got[first_of_gop2][0] == 1 and got[first_of_gop2][2] == 0


def test_slot_that_held_prediction_is_never_offered():
    for slots in (5, 6, 9, 12):
        _drive(slots, _ref_lists([13, 2, 7, 30]))   # the assertion is inside _drive


def test_ring4_is_always_forced():
    got = _drive(4, _ref_lists([7, 7]))
    assert all(p == 0 and mask == 0b111 and hits == 0 for p, mask, hits in got)


def test_fewer_than_four_slots_is_refused():
    with pytest.raises(ValueError):
        ring.SlotRing(3)
