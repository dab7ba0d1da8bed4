"""CPU: the guard of tests/test_dcn_exact_gpu.py.  Everything here is computed from the inputs and the reference of
tests/helpers_dcn_exact.py alone: the reference is pinned independently of the oracle, every case's grade preconditions hold, and
the table reaches what it claims to reach -- the three regimes of the tile remap on both kernels, every border class of a sample
position, the interior fast path and the fallback gather of the LDS window, every activation form, views on every path."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_dcn_exact as X


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def test_table_is_well_formed():
    ids = [c.id for c in X.CASES] + [c.id for c in X.EXT_CASES]
    assert len(ids) == len(set(ids))
    for c in X.CASES:
        assert c.grade in ("int", "dyadic", "f64") and c.paths and set(c.paths) <= set(X.PATHS), c.id
        if "lds" in c.paths:                 # the LDS kernel's floor, and a reference that stays quick
            assert X.LDS_MIN_PIXELS <= c.H * c.W <= 20000, c.id
        assert c.views in (0, 1) or c.N > 1, c.id


# ------------------------------------------------------------------------------------------------- the reference, pinned without the oracle
def _int_operands(seed, N=2, H=11, W=14):
    g = torch.Generator().manual_seed(seed)
    x = X._ints(g, (N, X.CH, H, W), 2).double()
    w = X._ints(g, (X.CH, X.CH, 3, 3), 2).double()
    b = X._ints(g, (X.CH,), 8).double()
    return x, w, b


def test_reference_with_zero_offsets_is_the_convolution():
    x, w, b = _int_operands(1)
    N, _, H, W = x.shape
    got = X.dcn_ref(x, w, b, torch.zeros(N, 18 * X.G, H, W, dtype=torch.float64), torch.ones(N, 9 * X.G, H, W, dtype=torch.float64))
    assert torch.equal(got, F.conv2d(x, w, b, padding=1))


@pytest.mark.parametrize("dy,dx", [(3, -2), (-1, 4), (0, 1), (-13, 2)])
def test_reference_with_a_constant_integer_offset_is_the_convolution_of_the_shifted_map(dy, dx):
    """sample (y + dy, x + dx) of x = sample (y, x) of the map shifted by (-dy, -dx) with zeros moving in, conv padding included"""
    x, w, b = _int_operands(2)
    N, _, H, W = x.shape
    off = torch.zeros(N, X.G, 9, 2, H, W, dtype=torch.float64)
    off[:, :, :, 0], off[:, :, :, 1] = dy, dx
    got = X.dcn_ref(x, w, b, off.view(N, 18 * X.G, H, W), torch.ones(N, 9 * X.G, H, W, dtype=torch.float64))
    big = torch.zeros(N, X.CH, 3 * H + 32, 3 * W + 32, dtype=torch.float64)                  # x in the middle of a zero plane
    y0, x0 = H + 16, W + 16
    big[:, :, y0:y0 + H, x0:x0 + W] = x
    shifted = big[:, :, y0 + dy - 1:y0 + dy + H + 1, x0 + dx - 1:x0 + dx + W + 1]            # one ring for the 3x3 window
    assert torch.equal(got, F.conv2d(shifted, w, b))


def test_epilogue_is_the_identity_on_fp16_values():
    v = torch.arange(-2047, 2048, dtype=torch.float32)
    for r16 in (False, True):
        assert torch.equal(X.epilogue(v, X.ACT_NONE, 0.0, r16), v)
        assert torch.equal(X.epilogue(v, X.ACT_RELU, 0.0, r16), v.clamp_min(0))
        assert torch.equal(X.epilogue(v, X.ACT_LRELU, 0.25, r16), torch.where(v > 0, v, v / 4))
        assert torch.equal(X.epilogue(v / 8, X.ACT_NONE, 0.0, r16), v / 8)
    # and it is not the identity elsewhere: 0.1 is no fp16 value, and rounding first changes the product
    u = -torch.arange(1, 4097, dtype=torch.float32) / 512               # the dyadic grade's unit
    assert not torch.equal(X.epilogue(u, X.ACT_NONE, 0.0, False), u)
    assert not torch.equal(X.epilogue(u, X.ACT_LRELU, 0.1, True), X.epilogue(u, X.ACT_LRELU, 0.1, False))


# ------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("case", X.CASES, ids=[c.id for c in X.CASES])
def test_grade_preconditions_hold_on_the_reference(case):
    """X.reference asserts them (check_exact: exact fp32 partial sums, |out| < 2048 on the integer grade, fp16 offsets)"""
    d = X.reference(case)
    assert d.ref.shape == (case.N, X.CH, case.H, case.W) and bool(torch.isfinite(d.ref).all())
    if case.grade == "f64":
        assert float(d.tol.min()) >= X.TINY16 and bool((d.tol < 0.05 * (1 + d.ref.abs())).all())        # a bound, not a blanket
    else:
        assert d.ref.dtype == torch.float32 and torch.equal(d.ref.half().float(), d.ref)
        if case.grade == "dyadic":           # the grade is only worth its name if the epilogue's roundings decide bits
            pre = d.pre.float()
            assert bool((pre.half().float() != pre).any()), case.id
    if case.act == X.ACT_CLAMP01:            # all three branches of the clamp
        assert bool((d.pre < 0).any()) and bool((d.pre > 1).any()) and bool(((d.pre > 0) & (d.pre < 1)).any()), case.id
    if case.regime == "huge":
        off = d.om[..., :18 * X.G]
        assert int(torch.isinf(off).sum()) >= 150 and int((off.abs() == X.BIG).sum()) >= 150 and bool((off == -float("inf")).any())


@pytest.mark.parametrize("case", X.EXT_CASES, ids=[c.id for c in X.EXT_CASES])
def test_ext_cases_are_exact_in_fp32(case):
    x, w, b, off, mask, want = X.ext_reference(case)                     # asserts exactness on the reference
    Ho, Wo = X.ext_out_map(case)
    assert want.shape == (case.B, case.Cout, Ho, Wo) and case.kernel[0] * case.kernel[1] <= 49


def test_ext_table_reaches_the_paths_it_names():
    npix = [X.ext_out_map(c)[0] * X.ext_out_map(c)[1] for c in X.EXT_CASES]
    assert any(c.Cout > 64 and c.Cout % 64 for c in X.EXT_CASES)        # a second, partial pass of the cob loop
    assert any(c.kernel == (7, 7) for c in X.EXT_CASES)                  # all 49 LDS rows
    assert any(c.kernel[0] != c.kernel[1] and c.stride[0] != c.stride[1] and c.pad[0] != c.pad[1] and c.dil[0] != c.dil[1] for c in X.EXT_CASES)
    assert any(n < 64 for n in npix) and any(n > 64 and n % 64 for n in npix)
    assert {c.grade for c in X.EXT_CASES} == {"int", "dyadic"}


# ------------------------------------------------------------------------------------------------- the tile remap
def test_tile_remap_regimes_are_all_reached_on_both_kernels(report):
    seen = {"gather": {}, "lds": {}}
    for c, p in X.RUNS:
        kern = "lds" if p == "lds" else "gather"                         # planar runs dcn_fused_kernel too
        seen[kern].setdefault(X.xcd_regime(X.tile_count(c, p), c.N), []).append(f"{c.id} ({X.tile_count(c, p)} x {c.N})")
    for kern, regimes in seen.items():
        report(f"dcn exact, tile remap on the {kern} kernel: " + "; ".join(f"{r}: {len(v)} runs" for r, v in sorted(regimes.items())))
        assert set(regimes) == {"identity", "divisible", "remainder"}, (kern, sorted(regimes))
    # the remainder remap only differs from c * q + c + (b >> 3) from 8 tiles on: both kernels need such a count, the gather kernel
    # also on a small map
    rem = [(c, p) for c, p in X.RUNS if X.xcd_regime(X.tile_count(c, p), c.N) == "remainder" and X.tile_count(c, p) > 8]
    assert any(p == "lds" for _, p in rem) and any(p != "lds" and c.H * c.W < 1024 for c, p in rem)
    # the shapes the table is built around
    count = {(c.H, c.W, p): X.tile_count(c, p) for c, p in X.RUNS}
    assert count[(65, 131, "lds")] == 81 and count[(65, 131, "gather")] == 153 and count[(64, 128, "lds")] == 64
    assert count[(13, 21, "gather")] == 6 and count[(20, 28, "gather")] == 12 and count[(16, 32, "gather")] == 8


def test_tile_remap_is_a_bijection_for_every_tile_count():
    for gx, N in sorted({(X.tile_count(c, p), c.N) for c, p in X.RUNS}):
        assert sorted(X.xcd_tile(b, gx, N) for b in range(gx)) == list(range(gx)), (gx, N)


# ------------------------------------------------------------------------------------------------- sample positions
def test_edge_and_border_cases_reach_every_sample_class(report):
    """h == -1, -1 < h < 0, h == H-1, H-1 < h < H, h == H, beyond; the same in w; and every pair of them at once"""
    n = len(X.AXIS_CLASSES)
    total = torch.zeros(n, n, dtype=torch.long)
    rows, cols = torch.zeros(n, dtype=torch.long), torch.zeros(n, dtype=torch.long)
    for c in X.CASES:
        if c.regime not in ("edges", "border"):
            continue
        h, w = X.sample_positions(c, X.reference(c))
        ch, cw = X.axis_class(h, c.H).flatten(), X.axis_class(w, c.W).flatten()
        rows += torch.bincount(ch[ch >= 0], minlength=n)
        cols += torch.bincount(cw[cw >= 0], minlength=n)
        both = (ch >= 0) & (cw >= 0)
        pair = torch.bincount(ch[both] * n + cw[both], minlength=n * n).view(n, n)
        total += pair
        report(f"dcn exact {c.id}: samples per class in h {torch.bincount(ch[ch >= 0], minlength=n).tolist()}, in w {torch.bincount(cw[cw >= 0], minlength=n).tolist()}")
        if c.regime == "edges":              # each edges case on its own: every class of its grade (open intervals: dyadic only)
            need = range(n) if c.grade == "dyadic" else (0, 2, 4, 5)
            assert all(int((ch == i).sum()) and int((cw == i).sum()) for i in need), c.id
    assert bool((rows > 0).all()) and bool((cols > 0).all()), (rows.tolist(), cols.tolist())
    assert bool((total > 0).all()), total.tolist()


def test_lds_cases_reach_the_window_paths(report):
    """over the table: interior tiles with no fallback at all; more than half of the samples falling back; interior and other tiles
    in one map; a map with no interior tile.  Conditions on the inputs: a shape that misses one is the wrong shape"""
    stats = {}
    for c in X.CASES:
        if "lds" in c.paths:
            stats[c.id] = s = X.lds_window_stats(c, X.reference(c))
            report(f"dcn exact {c.id}: {s[1]} of {s[0]} LDS tiles interior, {s[5]} of {s[2]} samples fall back, {s[3]} of them inside the map ({s[4]} in interior tiles)")
    assert any(i > 0 and fa == 0 for _, i, _, _, _, fa in stats.values()), "interior tiles and no fallback"
    assert any(2 * f > n for _, _, n, f, _, _ in stats.values()), "more than half of the samples fall back, with a weight"
    assert any(0 < i < t for t, i, *_ in stats.values()), "interior and other tiles coexist"
    assert any(i == 0 for _, i, *_ in stats.values()), "no interior tile"
    assert any(fi > 0 for _, _, _, _, fi, _ in stats.values()), "fallback samples on the interior fast path"
    assert any(i == 0 and f > 0 for _, i, _, f, _, _ in stats.values()), "fallback samples off the interior fast path"
    t, i, *_ = stats["m9x911_dy_edges_clamp"]
    assert i == 0                                                        # 9 rows: the 20-row window never fits
    assert stats["m600x14_dy_half_none_r16"][1] == 0                     # 14 columns: the 28-column window never fits


# ------------------------------------------------------------------------------------------------- floors and coverage
def test_every_activation_form_runs_at_the_dyadic_grade_rounded_and_not():
    forms = {(c.act, c.slope, c.round16) for c in X.CASES if c.grade == "dyadic"}
    for act, slope in ((X.ACT_NONE, 0.0), (X.ACT_RELU, 0.0), (X.ACT_LRELU, 0.1), (X.ACT_LRELU, 0.25), (X.ACT_CLAMP01, 0.0)):
        for r16 in (False, True):
            assert (act, slope, r16) in forms, (act, slope, r16)


def test_views_and_grades_appear_on_every_path():
    for p in X.PATHS:
        mine = [c for c, q in X.RUNS if q == p]
        assert any(c.views for c in mine) and any(c.views and c.N == 2 for c in mine), p
        assert {c.grade for c in mine} == {"int", "dyadic", "f64"}, p
        assert {"edges", "border", "huge", "wild"} <= {c.regime for c in mine} or p != "lds", p
    assert any(c.views == 2 for c in X.CASES)                            # a batch stride wider than H*W*C
    assert any(c.regime == "coherent_int" and c.shift != (0, 0) for c, p in X.RUNS if p == "lds")
