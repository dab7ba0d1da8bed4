"""Host-side bookkeeping of LoopFilter's slot ring (no GPU, no torch: tests/test_loopfilter_ring_cpu.py drives it alone).

The ring has `slots` slots of per-frame maps.  A call uses the window of four consecutive slots that starts at `p`: slot p + j serves
reference slice j (j = 0, 1, 2) and slot p + 3 takes the maps of prediction1.  The window slides by one slot per call, because the
reference list slides by one frame per P-frame: what a call left in slots p + 1 and p + 2 is what the next call looks for in ITS slots
p' + 0 and p' + 1.  Whether a slot's maps are reused is decided on the device by an exact compare of the frame with the slot's frame copy;
this class only places the data and says which slots hold nothing comparable (`force_mask`): slots never filled, and slots that held
prediction1's maps.  Past the last window position the window returns to slot 0 and every slot is forgotten (one full recompute per wrap).
Forgetting is a choice, not a need -- the device compare would reject a stale slot anyway.  The slots at the ring's head hold frames that
are slots - 3 calls old: in coding they never match again, and a match there comes only from content that repeats with the ring's period
(a benchmark that loops one GOP, where every slot would "hit" from the second pass on and the measured gain would be one that real
coding never sees).  Static content pays for this with one recompute per wrap.
"""
from __future__ import annotations

WINDOW = 4          # three reference slices + prediction1


class SlotRing:
    __slots__ = ("slots", "p", "valid", "_started")

    def __init__(self, slots: int):
        if slots < WINDOW:
            raise ValueError(f"SlotRing: the window needs {WINDOW} slots, got {slots}")
        self.slots = slots
        self.p = 0
        self.valid = [False] * slots
        self._started = False

    def begin(self) -> tuple[int, int]:
        """-> (window start p, force mask) of the call that starts now: bit j set = slot p + j holds no reference maps"""
        if self._started:
            self.p += 1
            if self.p > self.slots - WINDOW:          # wrap: the slots at the ring's head hold frames of long ago
                self.p = 0
                self.valid = [False] * self.slots
        self._started = True
        mask = 0
        for j in range(WINDOW - 1):
            if not self.valid[self.p + j]:
                mask |= 1 << j
        return self.p, mask

    def commit(self) -> None:
        """the call that `begin` opened has been enqueued: slots p .. p + 2 hold reference maps, slot p + 3 prediction1's"""
        for j in range(WINDOW - 1):
            self.valid[self.p + j] = True
        self.valid[self.p + WINDOW - 1] = False
