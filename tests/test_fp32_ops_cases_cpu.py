"""CPU: the tables of tests/helpers_fp32_ops.py (run on the GPU by tests/test_fp32_ops_gpu.py).

  * every table reaches the forks and dtypes it is there for;
  * the preconditions of the references hold (match_gather: no pixel under the 1e-8 clamp except the deliberately zero sources);
  * sensitivity: for every row whose maps are all fp32 and that has a bound rather than a bit-exact check, the float64 reference of the
    same inputs ROUNDED TO fp16 misses the row's bound by at least 10x in max(|d| / bound) -- an fp16 branch taken by mistake, the fault the
    fp32 forms exist to exclude, cannot pass (tests/test_dcn_f32_cases_cpu.py does the same for the DCN).  avgpool_k: the scale-2 rows (at
    scale 17 the average of 289 values hides the rounding); channel_sum: the rows with per <= 64."""
import pytest
import torch

import test_forward_ops_gpu as FO
from tests import helpers_fp32_ops as H

SENSITIVITY = 10.0


def test_tables_reach_their_forks():
    assert {(r[5], r[6], r[4]) for r in H.BC_CASES} == {(x, b, T) for x in ("f32", "f16") for b in ("f32", "f16") for T in (2, 3, 4)}
    assert {r[3] for r in H.BC_CASES} == {8, 64} and {r[7] for r in H.BC_CASES} == {False, True}
    t4 = [r for r in H.BC_CASES if FO.cls_bcast(r[4], r[5], r[6])[1] == "t4"]
    assert [(r[4], r[5], r[6]) for r in t4] == [(4, "f16", "f16")]
    assert {(r[4], r[5]) for r in H.UP_CASES} == {("f32", "f32"), ("f32", "f16"), ("f16", "f32")}
    for pair in (("f32", "f32"), ("f32", "f16"), ("f16", "f32")):              # 1 x w, h x 1 and 1 x 1 in every dtype pair
        shapes = {(r[1] == 1, r[2] == 1) for r in H.UP_CASES if (r[4], r[5]) == pair}
        assert {(True, False), (False, True)} <= shapes and ((True, True) in shapes or pair == ("f32", "f16")), pair
    assert any(r[1] == 1 and r[2] == 1 for r in H.UP_CASES)
    assert {(r[4], r[3]) for r in H.SP_CASES} == {(4, True), (4, False), (3, True), (3, False)} and {r[5] for r in H.SP_CASES} == {False, True}
    assert any((r[1], r[2]) == (2, 2) for r in H.SP_CASES) and any(r[2] == 2 and r[1] > 2 for r in H.SP_CASES)
    assert {r[6] for r in H.AF_CASES} == {2, 4, 8} and {r[4] for r in H.AF_CASES} == {8, 64} and any(r[4] != r[5] for r in H.AF_CASES)
    assert any(r[7] or r[8] for r in H.CC_CASES)


def test_channel_sum_rows_are_the_arithmetic():
    seen = set()
    for name, dt, N, Hh, W, C_, nb, v in H.CS_CASES:
        npix, lanes = Hh * W, H.cs_lanes(C_)
        per = -(-npix // nb)
        seen.add((dt, C_, H.cls_channel_sum(dt, C_, npix, nb)[3]))
        assert ("loop" in name) == (per > 3 * lanes), name
    assert {c for _, c, _ in seen} == {8, 64, 128, 256}
    for dt in ("f16", "f32"):
        assert {k for d, _, k in seen if d == dt} == {"loop4", "tail"}, dt
    rows = [(Hh * W, nb, H.cs_lanes(C_)) for (_, _, _, Hh, W, C_, nb, _) in H.CS_CASES]
    assert any(npix % nb for npix, nb, _ in rows)
    assert any(0 < npix - (nb - 1) * -(-npix // nb) < lanes for npix, nb, lanes in rows)          # a last block shorter than `lanes`
    assert any(npix - (nb - 1) * -(-npix // nb) <= 0 for npix, nb, _ in rows)                     # and an empty one


def test_avgpool_k_rows_are_the_arithmetic():
    for dt in ("f16", "f32"):
        mine = [r for r in H.AK_CASES if r[1] == dt]
        assert {r[6] for r in mine} == {2, 8, 11, 17}, dt
        assert {-(-r[6] // 8) for r in mine} == {1, 2, 3}
        assert any(r[7] for r in mine) and any(r[3] % r[6] and r[4] % r[6] for r in mine)
    assert {r[5] for r in H.AK_CASES} == {8, 64, 256}
    assert 11 % 8 == 3 and 17 % 8 == 1                                                              # last strips of 3 rows and of 1 row


@pytest.mark.parametrize("row", H.MG_CASES, ids=[r[0] for r in H.MG_CASES])
def test_match_gather_rows(row):
    name, dts, N, Hh, W, scale, vr, vc = row
    ks, nbh, nbw = H.mg_grid(Hh, W, scale)
    hp, wp = Hh // scale, W // scale
    assert nbh == (hp + 3) // 3 + 1 and nbw == (wp + 3) // 3 + 1                                    # the launcher's own check (F.fold's grid)
    fin, fref, idx = H.mg_data(row)
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < nbh * nbw
    ref, bound, clamped, outside = H.mg_ref(row, fin, fref, idx)
    assert clamped == outside and 0 < outside < N * Hh * W
    zero = (ref[..., 64:] == 0).all(-1)
    assert int(zero.sum()) == outside and bool((ref[zero] == 0).all())                             # cor = 0 exactly where the source lies outside
    if scale > 1:
        assert Hh % ks and W % ks                                                                   # blocks overhang the frame


def test_match_gather_dtypes():
    assert {r[1] for r in H.MG_CASES} == {(a, b, c) for a in ("f16", "f32") for b in ("f16", "f32") for c in ("f16", "f32")}      # fmap_any x 3
    assert {(r[3], r[4], r[5]) for r in H.MG_CASES} >= {(88, 120, 11), (100, 150, 12), (8, 8, 1)}
    assert any(r[6] for r in H.MG_CASES) and any(r[7] for r in H.MG_CASES)


# ------------------------------------------------------------------------------------------------- sensitivity of the counted bounds
def _rows():
    out = [("upsample2x", r) for r in H.UP_CASES if (r[4], r[5]) == ("f32", "f32")]
    out += [("spynet", r) for r in H.SP_CASES]
    out += [("channel_sum", r) for r in H.CS_CASES if r[1] == "f32" and -(-(r[3] * r[4]) // r[6]) <= 64]
    out += [("avgpool_k", r) for r in H.AK_CASES if r[1] == "f32" and r[6] == 2]
    out += [("match_gather", r) for r in H.MG_CASES if r[1] == ("f32", "f32", "f32")]
    return out


def test_sensitivity_rows_exist():
    ops_ = {k for k, _ in _rows()}
    assert ops_ == {"upsample2x", "spynet", "channel_sum", "avgpool_k", "match_gather"}


@pytest.mark.parametrize("op,row", _rows(), ids=[f"{k}-{'x'.join(str(v) for v in r[:8])}" for k, r in _rows()])
def test_fp16_rounded_inputs_miss_the_bound(op, row, report):
    if op == "upsample2x":
        x = H.up_data(row)
        (ref, bound), (r16, _) = H.up_ref(row, x), H.up_ref(row, x, x16=True)
    elif op == "channel_sum":
        x = H.cs_data(row)
        (ref, bound), (r16, _) = H.cs_ref(row, x), H.cs_ref(row, x, x16=True)
    elif op == "avgpool_k":
        x = H.ak_data(row)
        (ref, bound), (r16, _) = H.ak_ref(row, x), H.ak_ref(row, x, x16=True)
    elif op == "match_gather":
        fin, fref, idx = H.mg_data(row)
        ref, bound = H.mg_ref(row, fin, fref, idx)[:2]
        r16 = H.mg_ref(row, fin, fref, idx, x16=True)[0]
    else:
        N, Hh, W, fl, Cs, win = row
        rf, sp, flo = H.sp_data(row)
        ref, up = FO._level_ref64(rf, sp, flo, Hh, W)
        bound = H.sp_bound32(FO._level_bound(ref, up, sp, Hh, W, flo)[0], ref)
        h = lambda t: None if t is None else t.half().float()
        r16 = FO._level_ref64(h(rf), h(sp), h(flo), Hh, W)[0]
    r = H.ratio(r16, ref, bound)
    report(f"sensitivity {op} {row[:8]}: fp16-rounded inputs give max(|d|/bound) = {r:.1f}")
    assert r >= SENSITIVITY, (op, row, r)
