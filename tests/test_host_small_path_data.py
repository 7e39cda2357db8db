"""The inputs of tests/test_gpu_small_instances.py have the properties those
tests rely on (no GPU): without them the GPU tests could pass vacuously --
"tied" rows that are not ties, ties that NumPy's own argmin would not give
to the lower index, near-ties among the rows that are meant to be clear.
"""
import numpy as np
import pytest

import small_path_data as spd
from oracle import kmeans_oracle as orc


def _exact_ties(X, C):
    D = orc.distances(X, C)
    part = np.partition(D, 1, axis=1)
    return part[:, 0] == part[:, 1]


def _check_tie_rows(X, C0, tied, faithful_rows):
    k = len(C0)
    labels, _, gap = orc.assign(X, C0)
    if k > 1:
        exact = _exact_ties(X, C0)
        assert exact[tied].all()                       # every flagged row is an exact top-2 tie
        assert int(exact.sum()) == int(tied.sum())     # ... and no other row is
        assert (labels[tied] % 2 == 0).all()           # np.argmin: the pair's lower index (2b)
        assert gap[~tied].min() > 1e-4, gap[~tied].min()
        # every other row stays 0.05 away from its pair's bisector in feature 0
        lab = labels[~tied]
        paired = lab < 2 * (k // 2)
        m0 = C0[lab, 0] + np.where(paired, np.where(lab % 2 == 0, -1.0, 1.0), 0.0)
        assert np.abs(X[~tied, 0] - m0)[paired].min() >= 0.05
    else:
        assert not tied.any()
    lf, _ = orc.assign_faithful(X[faithful_rows], C0)
    np.testing.assert_array_equal(labels[faithful_rows], lf)
    ref = orc.lloyd_fit(X, k, 1, 1e-300, 0, True, 1, init_centroids=C0)
    assert ref["records"][0]["empty"] == [] and min(ref["records"][0]["sizes"]) > 0
    return labels


@pytest.mark.parametrize("d,k", spd.QUEUE_SHAPES)
def test_queue_level_rows(d, k):
    X, C0, tied = spd.tie_rows(d, k, spd.QUEUE_GROUPS + [64], seed=100 + d + k)
    assert X.shape == (2624, d) and C0.shape == (k, d)
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    # the wave-aligned blocks hold exactly the requested number of tied rows
    assert [int(t.sum()) for t in tied.reshape(-1, 64)] == spd.QUEUE_GROUPS + [64]
    assert all(t[:c].all() for t, c in zip(tied.reshape(-1, 64), spd.QUEUE_GROUPS + [64]))
    _check_tie_rows(X, C0, tied, slice(None))
    # the two sizes the GPU test runs: the aligned 2560 and the ragged 2597
    for n in (2560, 2597):
        _check_tie_rows(X[:n], C0, tied[:n], slice(0, 0))


@pytest.mark.parametrize("d,k", spd.FOLD_SHAPES)
def test_fold_rows(d, k):
    X, C0, tied = spd.tie_rows(d, k, spd.FOLD_GROUPS, seed=200 + d + k)
    assert X.shape == (6400, d)
    _check_tie_rows(X, C0, tied, slice(None))
    # three iterations (the GPU test's count) empty no cluster
    ref = orc.lloyd_fit(X, k, 3, 1e-300, 0, True, 1, init_centroids=C0)
    assert all(r["empty"] == [] for r in ref["records"])


@pytest.mark.parametrize("d,k", spd.MANY_SHAPES)
def test_many_rows(d, k):
    # the GPU test sizes this input by the device's CU count; the construction
    # is the same per block, checked here at 32 CUs (66,313 rows)
    groups, n = spd.many_rows_groups(32)
    assert n == 256 * 8 * 32 + 777 and len(groups) == -(-n // 64)
    first = 256 * 8 * 32 // 64
    # a wave's two trips together: below, at and above the 32-row LDS queue
    both = [a + b for a, b in zip(groups[:13], groups[first:first + 13])]
    assert min(both) < 32 and 32 in both and max(both) > 64
    assert groups[first + 12] <= 777 - 64 * 12           # the last, partial block holds its tied rows
    X, C0, tied = spd.many_rows_case(d, 32)
    assert len(X) == n and C0.shape == (k, d)
    assert tied[:64 * 13].any() and tied[256 * 8 * 32:].any()
    _check_tie_rows(X, C0, tied, slice(0, None, 7))


def test_fp32_range_inputs():
    d, k = 33, 8
    for scale in spd.FP32_RANGE_SCALES:
        X, C0 = spd.fp32_range(3001, d, k, seed=9, scale=scale)
        assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
        assert np.isfinite(C0.astype(np.float32)).all() and (C0.astype(np.float32) != 0).all()
        ref = orc.lloyd_fit(X, k, 2, 1e-300, 0, True, 1, init_centroids=C0)
        assert np.isfinite(ref["centroids"]).all() and np.isfinite(ref["sse_history"]).all()
        assert all(s > 0 for s in ref["sse_history"])
        assert all(r["empty"] == [] for r in ref["records"])
        labels, _, _ = orc.assign(X, C0)
        np.testing.assert_array_equal(labels, orc.assign_faithful(X, C0)[0])
        # the fp32 form of the row's own squared distance: every term
        # overflows (1e20) or underflows to zero (1e-25) for most rows
        with np.errstate(over="ignore", under="ignore"):
            t = X.astype(np.float32) - C0.astype(np.float32)[labels]
            s32 = (t * t).sum(axis=1, dtype=np.float32)
        lost = np.isinf(s32) if scale > 1 else (s32 == 0)
        assert lost.mean() > 0.5, lost.mean()


@pytest.mark.parametrize("d,k", [(33, 8), (64, 32)])
def test_numeric_edge_inputs(d, k):
    n = 3001
    # exact duplicates: rows of blob 3 tie exactly between 3 and its copies
    X, C0 = spd.duplicate_centroids(n, d, k, seed=3)
    dup = spd.duplicate_indices(k)
    assert dup and all(np.array_equal(C0[j], C0[3]) for j in dup)
    labels, _, gap = orc.assign(X, C0)
    assert (labels == 3).sum() > 0 and not np.isin(labels, dup).any()
    assert (gap[labels == 3] == 0).all()
    # one-ulp duplicates: every row's top two are a centroid and its neighbour
    X, C0 = spd.ulp_duplicates(n, d, k, seed=4)
    nb = k // 2
    assert np.array_equal(C0[nb:2 * nb], np.nextafter(C0[:nb], np.inf))
    labels, _, gap = orc.assign(X, C0)
    assert gap.max() < 1e-12
    assert len(np.unique(labels)) > nb // 2        # both members of pairs win rows
    np.testing.assert_array_equal(labels, orc.assign_faithful(X, C0)[0])
    # zero rows sit exactly on the zero centroid (distance 0, lower index of the two)
    X, C0 = spd.zero_rows_and_centroids(n, d, k, seed=5)
    labels, mind, _ = orc.assign(X, C0)
    zero = ~X.any(axis=1)
    assert zero.sum() >= n // 11 and (labels[zero] == 2).all() and (mind[zero] == 0).all()
    # per-feature magnitudes span 12 decades; far-from-origin means near 1000
    X, C0 = spd.feature_magnitudes(n, d, k, seed=6)
    assert np.abs(X[:, 0]).max() < 1e-7 and np.abs(X[:, -1]).max() > 1e3
    X, C0 = spd.far_from_origin(n, d, k, seed=7)
    assert np.abs(X).max() > 500
