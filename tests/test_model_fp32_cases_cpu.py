"""Without a GPU: the frame that tests/test_model_fp32_gpu.py pins keeps its distance from every rounding boundary of both coders, on
the oracle alone.  A change of the synthetic filler (tdvc_amd/synth.py) that moves a y - mu next to a half-integer shows here, as a
failed precondition, and not as a kernel failure on the GPU."""
from tests import helpers_model_fp32 as M


def test_pinned_frame_margins():
    _, tr = M.oracle_frame()
    m = M.margins(tr)
    print(f"seed {M.SEED} {M.H}x{M.W} frame 1: smallest distance of y - mu from a rounding boundary: motion {m['mv']:.3e}, residual {m['res']:.3e}")
    assert m["mv"] >= M.MARGIN and m["res"] >= M.MARGIN, m
    # the symbols the GPU test holds to zero flips: round(y) of the forward pass and round(y - mu) of compress() stay farther from a
    # boundary than the discrepancy that test allows
    for c, (fwd, ar) in M.symbol_distances(tr).items():
        print(f"   {c}: round(y) {fwd:.3e}, compress() round(y - mu) {ar:.3e}")
        assert fwd >= M.MARGIN / 4 and ar >= M.MARGIN / 4, (c, fwd, ar)
