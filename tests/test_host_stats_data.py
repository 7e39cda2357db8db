"""The inputs of tests/test_gpu_stats.py are what those tests assume (no GPU):
the planted label is the exact nearest centroid with a wide margin, every
value is an integer within the bounds that make float64 sums order-free, and
each named label pattern has the property that names it.  Without this a
bit-for-bit GPU comparison could pass or fail for reasons of stage 1.
"""
import numpy as np
import pytest

import stats_data as sd


def _groups(lab):
    """The aligned groups of 64 rows (the waves of k_hist and k_scatter)."""
    return [lab[i:i + 64] for i in range(0, len(lab), 64)]


def _check_pattern(case, lab):
    n, k, p = len(lab), case.k, case.pattern
    counts = np.bincount(lab, minlength=k)
    full = [g for g in _groups(lab) if len(g) == 64]
    if p in ("balanced", "tail1", "tail63"):
        assert counts.max() - counts.min() <= 1
        if n > 2 * 64 and k > 64:
            assert (np.diff(lab) < 0).any()                      # shuffled, not sorted
    if p == "tail1":
        assert n % 64 == 1 and n > 64
    if p == "tail63":
        assert n % 64 == 63 and n > 64
    if p.startswith("one_"):
        owner = {"one_first": 0, "one_last": k - 1, "one_kr": min(case.kr, k) - 1}[p]
        assert counts[owner] == n and (np.delete(counts, owner) == 0).all()
        if p == "one_kr" and case.ncr > 1:
            assert owner // case.kr == 0 and (owner + 1) // case.kr == 1   # the last id of the first range
    if p == "straddle":
        a, b = sd.heavy_pair(case)
        assert b == a + 1 and counts[a] == counts[b] == n * 45 // 100
        if case.ncr > 1:
            assert a // case.kr == 0 and b // case.kr == 1       # the two sides of the first boundary
        rest = np.delete(counts, [a, b])
        assert rest.sum() == n - counts[a] - counts[b] and rest.max() - rest.min() <= 1
    if p == "singletons":
        assert n == k and (counts == 1).all() and (np.diff(lab) < 0).any()
    if p == "sorted_runs":
        assert (np.diff(lab) >= 0).all() and len(np.unique(lab)) > 1
        assert len(set(counts[counts > 0])) > 1                  # runs of several lengths
    if p == "pair":
        for g in full:
            assert len(set(g)) == 2 and g[0] != g[1] and (g[::2] == g[0]).all() and (g[1::2] == g[1]).all()
    if p == "five":
        for g in full:                                           # more groups than peel_labels<4> has rounds
            assert sorted(np.bincount(g)[np.unique(g)]) == [12, 13, 13, 13, 13]
    if p == "lonely_first":
        for g in full:                                           # the first pending lane is alone: no round peels
            assert (g[1:] == g[1]).all() and g[0] != g[1]
    if p == "distinct":
        for g in _groups(lab):
            assert len(set(g)) == len(g)
    if p in ("pair", "five", "lonely_first", "distinct"):
        assert len(full) >= 2 and len(np.unique(lab)) > 64       # the groups differ from wave to wave


@pytest.mark.parametrize("case", sorted(set(sd.ALL_CASES)), ids=sd.case_id)
def test_planted_case(case):
    b = sd.build(case)
    X, M, C, lab, w = b["X"], b["M"], b["C"], b["lab"], b["w"]
    n = len(lab)
    assert n == sd.rows_of(case) and 1 <= n <= sd.MAX_N
    assert X.shape == (n, case.d) and M.shape == (case.k, case.d) and X.dtype == np.float32
    # integers within the bounds: exact in fp16 and fp32, every squared residual <= d
    R = sd.radius(case.d)
    assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= R + 1 and np.abs(M).max() <= R
    assert np.array_equal(X.astype(np.float16).astype(np.float32), X)
    e = X.astype(np.int64) - M[lab]
    assert np.array_equal(e, b["noise"]) and np.abs(e).max() <= 1
    if case.weighted:
        assert np.array_equal(w, np.rint(w)) and w.min() >= 1 and w.max() <= sd.MAX_W
        multi = np.flatnonzero(np.bincount(lab) > 1)[:200]
        if len(multi):                                           # not constant within a cluster
            assert 2 * sum(len(set(w[lab == j])) > 1 for j in multi) > len(multi)
    else:
        assert w is None
    if case.tails:
        # |m| >= 1 and a tail below half an fp32 ulp: the fp32 image is m, the tail survives in float64
        assert np.abs(M).min() >= 1
        assert np.array_equal(C.astype(np.float32).astype(np.float64), M.astype(np.float64))
        t = (C - M) / sd.TAIL_SCALE
        assert np.array_equal(t, sd.tails(case.k, case.d)) and t.min() >= 1 and t.max() <= 7
    else:
        assert np.array_equal(C, M)
    # the planted label is the exact argmin, the runner-up at least 1024 farther
    arg, best, second = sd.top2(X, M)
    np.testing.assert_array_equal(arg, lab)
    assert np.array_equal(best, (e * e).sum(1)) and best.max() <= case.d
    assert (second - best).min() >= sd.MIN_GAP, (second - best).min()
    _check_pattern(case, lab)
    ref = sd.reference(case)
    assert ref["max_abs"] < 2 ** 30
    assert ref["counts"].sum() == n and ref["n_empty"] == int((np.bincount(lab, minlength=case.k) == 0).sum())
    # the reduceat sums against a plain accumulation
    plain = np.zeros((case.k, case.d), dtype=np.int64)
    if case.d <= 300:
        np.add.at(plain, lab, X.astype(np.int64) * (1 if w is None else w.astype(np.int64)[:, None]))
        np.testing.assert_array_equal(ref["sums"], plain)
    if not case.tails:
        assert ref["sse"] == float(((e * e).sum(1) * (1 if w is None else w)).sum())


def test_tail_sse_is_the_exact_value():
    # the closed form of reference() against a long-double sum of the residuals
    case = sd.TAIL_CASES[0]
    b = sd.build(case)
    r = b["X"].astype(np.longdouble) - b["C"][b["lab"]].astype(np.longdouble)
    np.testing.assert_allclose(sd.reference(case)["sse"], float((r * r).sum()), rtol=1e-12)
    # what the flush's correction supplies: the residuals to the fp32 images
    # alone miss the SSE by more than the 1e-9 it is held to
    for case in sd.TAIL_CASES:
        b = sd.build(case)
        w = 1 if b["w"] is None else b["w"]
        plain = float(((b["noise"].astype(np.float64) ** 2).sum(1) * w).sum())
        assert abs(plain / sd.reference(case)["sse"] - 1) > 4e-9, case


def test_expected_splits_follow_the_lds_budget():
    # kr = STATS_LDS / (8 (fr + slots)), clamped to k; the sort starts at three cluster ranges
    lds = 156 * 1024
    for c in sorted(set(sd.ALL_CASES)):
        if c.route == 0:
            continue
        slots = 2 if c.weighted else 1
        dp = next((v for v in (16, 32, 48, 64, 96, 128, 192, 256) if c.d <= v), (c.d + 15) // 16 * 16)
        assert c.fr * c.nfr == dp and c.fr % 4 == 0
        assert c.kr == min(c.k, lds // (8 * (c.fr + slots))) and c.ncr == -(-c.k // c.kr)
        if dp <= 256 and c.k <= 16384:
            assert (c.route == 2) == (c.ncr >= 3), c
        else:
            assert c.route == 1, c


def test_bisector_rows():
    X, C, lab, tied = sd.bisector_case()
    assert int(tied.sum()) == sd.BISECTOR_ROWS and X.shape == (8193, 64)
    arg, best, second = sd.top2(X, C)
    np.testing.assert_array_equal(arg, lab)                      # the lower index of the pair
    assert (best[tied] == second[tied]).all() and (lab[tied] == 100).all()
    assert (second - best)[~tied].min() >= sd.MIN_GAP
    assert not np.isin(lab[~tied], (100, 101)).any()
    assert np.array_equal(C[101] - C[100], 2.0 * (np.arange(64) == 0))


DELTA_GEOMETRIES = [(64, 256, 8193), (64, 1536, 8193)]


def delta_iterations(X, C0):
    """Exact labels of two iterations (centroids C0, then the means)."""
    X = X.astype(np.float64)
    lab1, b1, s1 = sd.top2(X, C0)
    cnt = np.bincount(lab1, minlength=len(C0))
    C1 = C0.copy()
    S = sd.cluster_sums(lab1, len(C0), X.astype(np.int64))
    C1[cnt > 0] = S[cnt > 0] / cnt[cnt > 0, None]
    lab2, b2, s2 = sd.top2(X, C1)
    return lab1, lab2, min((s1 - b1).min(), (s2 - b2).min())


@pytest.mark.parametrize("d,k,n", DELTA_GEOMETRIES)
def test_delta_situations(d, k, n):
    moved = {}
    for situation in ("none", "one", "blob"):
        X, C0 = sd.delta_case(d, k, n, situation)
        assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= 64
        lab1, lab2, gap = delta_iterations(X, C0)
        assert gap >= 8.0, gap                                   # no near-tie in either iteration
        moved[situation] = np.flatnonzero(lab1 != lab2)
        if situation == "blob":
            rows = moved[situation]
            assert len(rows) == 12 and (lab1[rows] == 0).all() and (lab2[rows] == 1).all()
            assert (X[rows, 0] == 10).all()
            assert (np.bincount(lab1, minlength=k)[2], np.bincount(lab2, minlength=k)[2]) == (0, 0)
        if situation == "one":
            rows = moved[situation]
            assert len(rows) == 1 and lab1[rows[0]] == 0 and lab2[rows[0]] == 1 and X[rows[0], 0] == 6
    assert len(moved["none"]) == 0
