"""The planted statistics of tests/test_gpu_update.py and
tests/test_gpu_repair.py are what those tests assume (no GPU): each pattern
has the property that names it, the NumPy record agrees with the oracle's
restatement of _update_centroids, and each repair case has the empties, the
picks and the window edges it is there for.  Without this an == on the GPU
could pass or fail for reasons of the test's own inputs.
"""
from fractions import Fraction

import numpy as np
import pytest

import update_data as ud
from oracle import kmeans_oracle as orc

ALL_CASES = [c for k, d in ud.SHAPES for p in ud.PATTERNS for c in ud.cases(k, d, p)]


def _table(plan, case):
    k, d = case.k, case.d
    T = plan["flat"][:k * (d + 1)].reshape(k, d + 1)
    return T[:, :d], T[:, d]


def test_the_grid_splits_at_update_one_ok():
    assert all(ud.update_one_ok(k, d) for k, d in ud.ONE_SHAPES)
    assert not any(ud.update_one_ok(k, d) for k, d in ud.TWO_SHAPES)
    # both sides of each condition: k = 64 / 65 and k d = 16384 / 16448
    assert (64, 256) in ud.ONE_SHAPES and (64, 257) in ud.TWO_SHAPES and (65, 1) in ud.TWO_SHAPES
    assert (8, 2048) in ud.ONE_SHAPES and (9, 2047) in ud.TWO_SHAPES
    # more clusters than the 16 waves / the 256 threads, more features than the 64 lanes, and fewer
    assert any(k > 16 for k, _ in ud.ONE_SHAPES) and any(k < 16 for k, _ in ud.ONE_SHAPES)
    assert any(k > 256 for k, _ in ud.TWO_SHAPES) and any(k % 256 for k, _ in ud.TWO_SHAPES if k > 256)
    assert any(d > 64 and d % 64 for _, d in ud.SHAPES) and any(d < 64 for _, d in ud.SHAPES)


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_exact_shift_moves_one_coordinate_by_delta(k, d):
    mv = ud.movers(k, d)
    assert {j for j, _ in mv} >= {0, k - 1} and {f for _, f in mv} >= {0, d - 1}
    if k > 16:
        assert {15, 16} <= {j for j, _ in mv}
    if k > 256:
        assert {255, 256} <= {j for j, _ in mv}
    if d > 64:
        assert {63, 64} <= {f for _, f in mv}
    for case in ud.cases(k, d, "exact_shift"):
        plan = ud.plant(case)
        S, cnt = _table(plan, case)
        C = plan["C_old"]
        j, f = case.variant
        # integers, exact products: S = cnt C everywhere but the mover
        assert (C == np.rint(C)).all() and (cnt == np.rint(cnt)).all() and (cnt > 0).all()
        diff = plan["rec"]["new"] - C
        assert diff[j, f] == ud.DELTA and np.count_nonzero(diff) == 1
        mask = np.ones((k, d), bool)
        mask[j, f] = False
        assert (S[mask] == (C * cnt[:, None])[mask]).all()
        assert Fraction(S[j, f]) == 4 * (Fraction(C[j, f]) + Fraction(ud.DELTA))      # no rounding in the plant
        # delta^2 = 2^-40 plus zeros: the same float in any order, its root exact
        assert plan["rec"]["shift"] == ud.DELTA and plan["rec"]["exact_shift"]
        assert plan["tols"] == [(ud.DELTA, 0), (np.nextafter(ud.DELTA, np.inf), 1)]
        assert plan["rec"]["n_empty"] == 0 and plan["rec"]["nonfinite"] == 0


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_noise_and_weighted(k, d):
    for p in ("noise", "weighted"):
        (case,) = ud.cases(k, d, p)
        plan = ud.plant(case)
        S, cnt = _table(plan, case)
        rec = plan["rec"]
        assert np.isfinite(plan["flat"]).all() and (cnt > 0).all() and (cnt == np.rint(cnt)).all()
        assert rec["n_empty"] == 0 and rec["nonfinite"] == 0 and rec["shift"] > 0 and not rec["exact_shift"]
        assert len(plan["flat"]) == k * (d + 1) + 1 + (k if p == "weighted" else 0)
        div = cnt
        if p == "weighted":
            div = plan["flat"][k * (d + 1) + 1:]
            assert (div != cnt).all() and (div != np.rint(div)).any()       # fractional, not the counts
            assert (rec["new"] != S / cnt[:, None]).any()                    # dividing by the count is wrong
        np.testing.assert_array_equal(rec["new"], S / div[:, None])
        (lo, s_lo), (hi, s_hi) = plan["tols"]
        assert lo < rec["shift"] < hi and (s_lo, s_hi) == (0, 1)
        # far from the shift by more than the bound of the comparison
        assert rec["shift"] - lo > 1e3 * ud.shift_rtol(d) * rec["shift"]


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_big_counts(k, d):
    (case,) = ud.cases(k, d, "big_counts")
    plan = ud.plant(case)
    S, cnt = _table(plan, case)
    ids, e = ud.big_ids(k)
    for j, c in zip(ids, ud.BIG):
        if ids.index(j) == max(i for i, v in enumerate(ids) if v == j):
            assert cnt[j] == c
    assert plan["rec"]["counts"].dtype == np.int64
    if k >= 4:
        assert len(set(ids)) == 3 and e is not None
        assert [int(v) for v in plan["rec"]["counts"][ids]] == [2 ** 31, 2 ** 32, 2 ** 40 + 1]
        assert plan["rec"]["n_empty"] == 1 and cnt[e] == 0
    else:
        assert e is None and plan["rec"]["n_empty"] == 0
    # exact products far below 2^53: new == C_old bit for bit, shift 0
    assert np.abs(S).max() < 2.0 ** 53
    live = cnt > 0
    assert all(Fraction(S[j, f]) == Fraction(cnt[j]) * Fraction(plan["C_old"][j, f])
               for j in np.nonzero(live)[0][:4] for f in range(min(d, 3)))
    np.testing.assert_array_equal(plan["rec"]["new"], plan["C_old"])
    assert plan["rec"]["shift"] == 0.0
    # a count that int32 cannot hold
    assert (plan["rec"]["counts"] > np.iinfo(np.int32).max).any()


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_empties(k, d):
    for case in ud.cases(k, d, "empties"):
        plan = ud.plant(case)
        S, cnt = _table(plan, case)
        ids = ud.empty_ids(k, case.variant)
        assert list(np.nonzero(cnt == 0)[0]) == ids and plan["rec"]["n_empty"] == len(ids)
        if case.variant == "ends":
            assert ids == sorted({0, k - 1})
        if case.variant == "all_but_one":
            assert len(ids) == k - 1
        if ids:
            assert S[ids].any()                                   # sums that must not be read
            np.testing.assert_array_equal(plan["rec"]["new"][ids], plan["C_old"][ids])
            assert (plan["rec"]["norms"][ids] == 0).all()
        assert [s for _, s in plan["tols"]] == ([2, 2] if ids else [0, 1])


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_nonfinite(k, d):
    seen = set()
    for case in ud.cases(k, d, "nonfinite"):
        val, pos, combo = case.variant
        plan = ud.plant(case)
        S, cnt = _table(plan, case)
        bad = np.argwhere(~np.isfinite(S))
        assert bad.tolist() == [[k - 1, d - 1] if pos == "last" else [0, 0]]
        j, f = bad[0]
        assert cnt[j] > 0 and (np.isnan(S[j, f]) if val == "nan" else S[j, f] == np.inf)
        assert plan["rec"]["nonfinite"] == 1
        if combo == "with_empty" and k > 1:
            assert plan["rec"]["n_empty"] == 1
        if combo == "below_tol":
            (tol, _), = plan["tols"]
            assert np.nanmax(np.delete(plan["rec"]["norms"], j), initial=0.0) < tol
        assert [s for _, s in plan["tols"]] == [3]
        seen.add(case.variant)
    assert len(seen) == 12


@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_range_edges(k, d):
    tiny, huge, over = (ud.plant(c) for c in ud.cases(k, d, "range"))
    assert 1e-151 < np.abs(tiny["C_old"]).min() and np.abs(tiny["C_old"]).max() < 1e-149
    diff = tiny["rec"]["new"] - tiny["C_old"]
    assert (diff > 0).all() and (diff * diff == 0).all()            # every square underflows
    assert tiny["rec"]["shift"] == 0.0 and tiny["tols"] == [(0.0, 0), (5e-324, 1)]
    assert 1e149 < np.abs(huge["C_old"]).min() and np.abs(huge["C_old"]).max() < 1e151
    sq = (huge["rec"]["new"] - huge["C_old"]) ** 2
    assert sq.min() > 1e300 and np.isfinite(sq.sum(axis=1)).all()   # near the top of the range, no overflow
    assert 1e150 < huge["rec"]["shift"] < 1e153 and not huge["rec"]["exact_shift"]
    assert [s for _, s in huge["tols"]] == [0, 1]
    with np.errstate(over="ignore"):
        assert np.isinf((over["rec"]["new"] - over["C_old"]) ** 2).all()            # every square overflows
    assert np.isfinite(over["rec"]["new"]).all() and over["rec"]["nonfinite"] == 0
    assert over["rec"]["shift"] == np.inf and over["tols"] == [(1e300, 0)]


def test_the_record_is_the_oracles_update():
    n = 0
    for case in ALL_CASES:
        if case.weighted or (case.pattern == "exact_shift" and case.variant != ud.movers(case.k, case.d)[-1]):
            continue
        plan = ud.plant(case)
        rec = plan["rec"]
        new, counts, empty = orc.update_centroids(ud.stats_dict(plan["C_old"], plan["flat"]), plan["C_old"],
                                                  lambda m: [])
        np.testing.assert_array_equal(new, rec["new"])
        assert [counts[j] for j in range(case.k)] == rec["counts"].tolist()
        assert len(empty) == rec["n_empty"]
        assert int(not np.all(np.isfinite(new))) == rec["nonfinite"]            # kmeans_spark.py:289
        if not np.isnan(new).any():
            with np.errstate(all="ignore"):
                assert np.max(np.linalg.norm(new - plan["C_old"], axis=1)) == rec["shift"]    # :293-294
        n += 1
    assert n > 300


# ------------------------------------------------------------------- the repair
def test_repair_cases_cover_the_grid():
    cs = ud.REPAIR_CASES
    assert {c.k for c in cs} == set(ud.REPAIR_K) and {c.d for c in cs} == {3, 17}
    assert {(c.k, c.empties) for c in cs} >= {(k, e) for k in ud.REPAIR_K for e in ud.EMPTY_PATTERNS
                                              if ud.repair_empties(k, e)}
    assert {(c.layout, c.seed) for c in cs} >= {(lay, s) for lay in ud.LAYOUTS for s in ud.SEEDS}
    assert ud.repair_empties(1000, "chunk_edges") == [3, 4, 255, 256, 511, 512, 999]
    assert ud.repair_empties(1000, "wave_edges") == list(range(252, 260))       # threads 63 and 64
    assert ud.repair_empties(5, "wave_edges") == [] and ud.repair_empties(64, "wave_edges") == [63]
    assert len(ud.LAYOUTS["many"]) > 256 and 0 in ud.LAYOUTS["skew"] and 1 in ud.LAYOUTS["skew"]
    assert len(cs) == len(set(cs))


@pytest.mark.parametrize("case", ud.REPAIR_CASES, ids=ud.repair_id)
def test_repair_case(case):
    layout = ud.LAYOUTS[case.layout]
    empty = ud.repair_empties(case.k, case.empties)
    plan = ud.plant_repair(case.k, case.d, empty, layout, case.big)
    k, d = case.k, case.d
    cnt = plan["flat"][:k * (d + 1)].reshape(k, d + 1)[:, d]
    assert list(np.nonzero(cnt == 0)[0]) == empty and plan["plain"]["n_empty"] == len(empty)
    total = sum(layout)
    assert 0 < len(empty) < total and plan["X"].shape == (total, d)
    X = plan["X"]
    assert (X == np.rint(X)).all() and (X.astype(np.float32) == X).all()
    gidx = ud.picks(layout, len(empty), case.seed)
    assert len(gidx) == len(empty) == len(set(gidx)) and all(0 <= g < total for g in gidx)
    rec = ud.repaired(plan, empty, gidx)
    live = np.setdiff1d(np.arange(k), empty)
    for j, g in zip(empty, gidx):
        np.testing.assert_array_equal(rec["new"][j], X[g])
    np.testing.assert_array_equal(rec["new"][live], plan["plain"]["new"][live])
    # which kind holds the maximum shift is planted, by a wide margin
    a, b = rec["norms"][live].max(), rec["norms"][empty].max()
    assert (a > 2 * b) if case.big else (b > 2 * a > 0 or b == 0)
    assert rec["shift"] == max(a, b) > 0 and rec["nonfinite"] == 0
    # the replacement rows' shifts are roots of integers (exact in any order)
    assert all(float(np.sqrt(((X[g] - plan["C_old"][j]) ** 2).sum())) == rec["norms"][j] for j, g in zip(empty, gidx))


def test_repair_cases_put_the_maximum_on_both_kinds():
    assert {c.big for c in ud.REPAIR_CASES} == {True, False}
    small = [c for c in ud.REPAIR_CASES if not c.big]
    assert {c.k <= 64 for c in small} == {True, False}


def test_some_pick_is_the_first_or_last_row_of_a_partition():
    edges = 0
    for case in ud.REPAIR_CASES:
        layout = ud.LAYOUTS[case.layout]
        bases = np.concatenate([[0], np.cumsum(layout)])
        first = {int(b) for b, s in zip(bases[:-1], layout) if s}
        last = {int(b + s - 1) for b, s in zip(bases[:-1], layout) if s}
        g = set(ud.picks(layout, len(ud.repair_empties(case.k, case.empties)), case.seed))
        edges += len(g & (first | last))
    assert edges >= 10


@pytest.mark.parametrize("layout", ud.EVERY_ROW_LAYOUTS)
def test_every_row_branch(layout):
    total = sum(layout)
    empty = list(range(1, 9))
    assert len(empty) >= total                                   # num >= total: takeSample returns every row
    for seed in ud.SEEDS:
        gidx = orc.take_sample_indices(list(layout), len(empty), seed)
        assert sorted(gidx) == list(range(total))


@pytest.mark.parametrize("d", [3, 17])
def test_mode2_windows_put_picks_on_all_four_edges(d):
    m = ud.MODE2
    layout = ud.LAYOUTS[m["layout"]]
    gidx = ud.picks(layout, len(m["empty"]), m["seed"])
    assert len(set(gidx)) == len(m["empty"]) >= 8
    w = ud.mode2_windows(gidx)
    row0, n = w["inner"]
    assert row0 in gidx and row0 + n - 1 in gidx                              # the first and the last owned row
    own = [g for g in gidx if row0 <= g < row0 + n]
    assert 2 <= len(own) < len(gidx)
    assert any(g < row0 for g in gidx) and any(g >= row0 + n for g in gidx)
    row0, n = w["outer"]
    assert n >= 1 and row0 - 1 in gidx and row0 + n in gidx                   # one row before, one row past
    assert row0 not in gidx and row0 + n - 1 not in gidx
    assert row0 >= 0 and row0 + n <= sum(layout)
