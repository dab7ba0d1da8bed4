"""CPU: the guard of tests/test_conv_exact_gpu.py.  Every case of tests/helpers_conv_exact.py names the kernel it is there for;
tdvc_conv_select (host arithmetic on the descriptor, no device) must answer with that kernel here, so a dispatch change cannot
silently move the GPU module off a kernel.  The table as a whole must reach every dispatch outcome, and every kernel that walks
its tiles in both directions must have a case with more tiles than workgroups and a case that is ragged in its own tile."""
import ctypes as C

import pytest

from tdvc_amd import _lib as L, ops

from tests import helpers_conv_dispatch as HD
from tests import helpers_conv_exact as X


def select(case):
    lib = L.lib()
    d = X.guard_desc(L, ops._pick_ck, case)
    for setter, off, _ in case.switches:
        getattr(lib, setter)(off)
    try:
        name = lib.tdvc_conv_select(C.byref(d))
        return HD.REJECTED + ": " + lib.tdvc_last_error().decode() if name is None else name.decode()
    finally:
        for setter, _, on in case.switches:
            getattr(lib, setter)(on)


@pytest.mark.parametrize("case", X.CASES, ids=[c.id for c in X.CASES])
def test_case_reaches_its_kernel(case):
    assert HD.outcome(select(case)) == case.kernel


def test_case_ids_are_unique_and_forms_known():
    ids = [c.id for c in X.CASES + X.PAIR_CASES]
    assert len(ids) == len(set(ids))
    for c in X.CASES:
        assert c.form in ("e4", "generic", "lean", "gdn", "gdn32") and c.grade in ("int", "dyadic", "f64"), c.id
        assert (c.form == "gdn32") == bool(c.gdn and c.x_f32), c.id
        assert (c.grade == "f64") == bool(c.gdn or c.act == X.ACT_SIGMOID), c.id       # float64 only where the operation is inexact


def test_table_reaches_every_outcome(report):
    named = {c.kernel for c in X.CASES}
    want = set(HD.OUTCOMES) - {HD.REJECTED}
    report("exact conv cases per dispatch outcome: " + ", ".join(f"{k} {sum(c.kernel == k for c in X.CASES)}" for k in HD.OUTCOMES if k != HD.REJECTED)
           + f"; conv_pair {len(X.PAIR_CASES)}")
    assert named == want, (want - named, named - want)
    for k in want:                       # each kernel: at least one ragged case
        assert any(c.ragged for c in X.CASES if c.kernel == k), k
    assert any(c.ragged for c in X.PAIR_CASES)


def test_reverse_walkers_have_multi_tile_and_ragged_cases(report):
    for k in X.REVERSE_WALKERS:
        mine = [c for c in X.CASES if c.kernel == k or (k == "conv_mfma_v3" and c.kernel == "conv_mfma_v3(s2d)") or (k == "conv_row" and c.kernel == "conv_row(s2d)")]
        multi, ragged = [c.id for c in mine if c.multi], [c.id for c in mine if c.ragged]
        report(f"{k}: multi-tile {multi}; ragged {len(ragged)} cases")
        assert multi and ragged, k


# tiles and persistent workgroups of the multi-tile cases, restated from the launchers (csrc/conv_*.hip: tile sizes, the slots of
# persistent_grid_x): a `multi` flag is only worth something if the arithmetic behind it is checked
PERSISTENT = {"conv_mfma_v3": (8, 32, 512), "conv_mfma_v3(s2d)": (8, 32, 512), "conv_mfma_v5": (16, 32, 256), "conv_mfma_v7": (16, 32, 256),
              "conv_mfma_v10": (16, 32, 256), "conv_mfma_v11": (16, 32, 256)}


@pytest.mark.parametrize("case", [c for c in X.CASES if c.multi and c.kernel in PERSISTENT], ids=lambda c: c.id)
def test_multi_tile_cases_have_an_uneven_tail(case):
    th, tw, slots = PERSISTENT[case.kernel]
    Ho, Wo = (case.H // 2, case.W // 2) if case.s2d else X.out_map(case)
    ntiles = -(-Ho // th) * -(-Wo // tw)
    blocks = -(-case.cout // 64)
    wgs = max(1, min(slots // (blocks * case.N), ntiles))
    assert ntiles > wgs and ntiles % wgs != 0, (ntiles, wgs)
    assert Ho % th and Wo % tw


def row_runs(case):
    """conv_row (launch_conv_row_t): the work is N * strips * Ho rows of one strip width, cut into equal runs for the 256 / ncb
    workgroup slots of a block of CO output channels -> (rows, slots)"""
    Ho, Wo = (case.H // 2, case.W // 2) if case.s2d else X.out_map(case)
    sw, co = (32, 128) if case.s2d else ((32, 128) if case.cin == 128 and case.cout % 128 == 0 else (64, 64))      # RowGeo: SW, CO = 16 NCG
    rows = case.N * -(-Wo // sw) * Ho
    return rows, min(256 // (case.cout // co), rows), Wo % sw


ROW_CASES = [c for c in X.CASES if c.kernel.startswith("conv_row")]


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c.id)
def test_conv_row_multi_flag_is_the_arithmetic(case):
    """`multi` on a conv_row case: more rows than slots, unevenly, so runs are longer than one row and differ in length"""
    rows, slots, ragged_w = row_runs(case)
    assert case.multi == (rows > slots and rows % slots != 0), (rows, slots)
    assert bool(ragged_w) == case.ragged


def test_conv_row_has_long_runs():
    """the steady-state row loop: at least one case whose runs are ten rows or more"""
    assert any(rows // slots >= 10 for rows, slots, _ in map(row_runs, ROW_CASES))


# ------------------------------------------------------------------------------------------------- conv_f32: the whole-model fp32 mode
F32 = [c for c in X.CASES if c.kernel == "conv_f32"]


def _npix(c):
    Ho, Wo = X.out_map(c)
    return c.N * Ho * Wo, Ho * Wo


def test_f32_rows_reach_every_instantiation_and_its_tails(report):
    """conv_f32_kernel<MT, NT> (csrc/conv_f32.hip:290-297): all four instantiations have an integer row and a dyadic row, a row whose last
    workgroup holds a partial first pixel block and an empty second one, and a batch whose first image ends inside a 32-pixel group"""
    by = {}
    for c in F32:
        assert c.x_f32 and c.ragged, c.id
        by.setdefault(X.f32_variant(c), []).append(c)
    report("conv_f32 rows per <MT, NT>: " + ", ".join(f"{v} {len(cs)}" for v, cs in sorted(by.items())))
    assert set(by) == {(1, 1), (1, 2), (2, 1), (2, 2)}, sorted(by)
    for (mt, nt), cs in by.items():
        assert {"int", "dyadic"} <= {c.grade for c in cs}, (mt, nt)
        assert all(_npix(c)[0] % (64 * nt) for c in cs), (mt, nt)                                     # `ragged` is the arithmetic
        assert any(0 < _npix(c)[0] % (64 * nt) < 32 * nt for c in cs), (mt, nt)
        assert any(32 < _npix(c)[0] % 64 < 64 for c in cs) or nt == 2, (mt, nt)                       # NT 1: a short second block as well
        assert any(c.N > 1 and _npix(c)[1] % 32 for c in cs), (mt, nt)
    assert any(32 < _npix(c)[0] % 64 < 64 for c in F32 if X.f32_variant(c)[1] == 1)


def test_f32_variant_restates_the_launcher():
    """X.f32_variant_of is a restatement: the two conditions it restates must stand in the launcher as cited (csrc/conv_f32.hip:290-297), so
    a changed threshold or a forced branch there fails here instead of silently moving the rows off an instantiation"""
    import os
    import tdvc_amd
    src = open(os.path.join(os.path.dirname(tdvc_amd.__file__), "csrc", "conv_f32.hip")).read()
    assert "const bool big = e.total_px >= 16384;" in src
    assert "inline int cout_tiles32(int cout) { return cout <= 32 ? 1 : 2 * ((cout + 63) / 64); }" in src
    for inst, cond in (("<1, 2>", "if (big)"), ("<1, 1>", "else"), ("<2, 2>", "if (big)"), ("<2, 1>", "else")):
        line = [ln for ln in src.splitlines() if "hipLaunchKernelGGL((conv_f32_kernel" + inst in ln]
        assert len(line) == 1 and line[0].strip().startswith(cond), inst
    assert X.f32_variant_of(32, 16383) == (1, 1) and X.f32_variant_of(33, 16384) == (2, 2)


def test_f32_rows_have_every_layer_of_the_fp32_mode():
    """every layer outside the coders that model_fp32 runs on fp32 maps (X.F32_LAYERS, which the GPU guard holds to production) has a row;
    no layer is claimed twice"""
    have = {X.f32_layer(X.conv_f32_class(L, X.guard_desc(L, ops._pick_ck, c))) for c in F32}
    assert X.F32_LAYERS <= have, sorted(X.F32_LAYERS - have, key=str)
    assert not (X.F32_LAYERS & X.F32_CODER_LAYERS)
    forms = {(c.res, c.res2) for c in F32}
    assert ("f32", "f32") in forms and ("f16", "f32") in forms                                        # the F32MAPS branch of res2
    assert any(c.res_c == 2 and c.cout == 2 for c in F32) and any(c.cout == 216 and c.views for c in F32) and any(c.out == "nchw" for c in F32)
    assert {(c.slices, c.act, c.res) for c in F32 if c.slices} == {("all", X.ACT_NONE, None), ("all", X.ACT_NONE, "f32"), ("all", X.ACT_LRELU, None),
                                                                    ("last1", X.ACT_LRELU, None)}          # the LoopFilter's calls on frame slices
    assert {(c.gdn, c.cin) for c in F32 if c.form == "gdn32"} == {(g, ch) for g in (X.GDN_FWD, X.GDN_INV) for ch in (64, 128)}


@pytest.mark.parametrize("case", X.F32_MODE_CASES, ids=lambda c: c.id)
def test_f32_mode_rows_meet_their_preconditions(case):
    """X.reference asserts check_exact on the reference (sums below 2^24 in the accumulator's unit, integer stages exact fp16 values); the
    float64 rows get a positive pool and a finite bound"""
    d = X.reference(case, X.make_data(case))
    _, yc = X.y_channels(case)
    assert d.ref.shape[1] == yc and bool(d.ref.isfinite().all())
    if case.grade == "f64":
        assert bool((d.tol >= 0).all()) and float(d.tol.max()) < 1e-5
    else:
        assert float(d.ref.abs().max()) > 0
