"""The inputs of tests/test_gpu_fp32_range.py have the properties those tests
rely on (no GPU): ordinary float32 numbers whose float64 distances are finite
and non-zero, labels that the ||c||^2 term decides (a screen that drops it
mislabels most rows), clear top-2 gaps (a screen, not the float64 resolver,
decides them at scale 1), no empty cluster in any iteration the GPU tests
run, and the scales on both sides of the row gate's range.
"""
import numpy as np
import pytest

import range_data as rd
from oracle import kmeans_oracle as orc

F32_TINY = float(np.finfo(np.float32).tiny)


def _representable(A):
    with np.errstate(under="ignore"):
        return np.isfinite(A.astype(np.float32)).all() and np.array_equal(A, A.astype(np.float32).astype(np.float64))


def _basic(X, C0, zero_centroids=()):
    """Finite, float32-representable, non-zero norms; finite float64
    distances, non-zero for every row that is not itself a centroid."""
    assert _representable(X) and _representable(C0)
    assert (np.sqrt((X * X).sum(axis=1)) > 0).all()
    cn = np.sqrt((C0 * C0).sum(axis=1))
    assert sorted(np.nonzero(cn == 0)[0]) == sorted(zero_centroids)
    labels, mind = rd.assign(X, C0)
    assert np.isfinite(mind).all()
    is_centroid = (X[:, None, :8] == C0[None, :, :8]).all(axis=2).any(axis=1)
    assert (mind[~is_centroid] > 0).all()
    return labels, mind


def _gaps(X, C0):
    """Relative top-2 distance gap per row, from a float64 product (good to
    1e-9 of the scale: enough for a 1e-3 threshold)."""
    D2 = (X * X).sum(axis=1)[:, None] - 2.0 * (X @ C0.T) + (C0 * C0).sum(axis=1)[None, :]
    two = np.sqrt(np.maximum(np.partition(D2, 1, axis=1)[:, :2], 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)


def test_narrowed_assign_is_the_oracles():
    # rd.assign / rd.lloyd against orc.assign / orc.lloyd_fit where the latter are affordable
    for name, scale in [("A", 1e-25), ("B", 1e20), ("G3", 1.0)]:
        X, C0 = rd.class_case(name, scale)
        labels, mind = rd.assign(X, C0)
        ol, om, _ = orc.assign(X, C0)
        np.testing.assert_array_equal(labels, ol)
        np.testing.assert_array_equal(mind, om)
    X, C0 = rd.class_case("A", 1e-22)
    ours = rd.lloyd(X, C0, rd.ITERS)
    for i, r in enumerate(ours):
        fit = orc.lloyd_fit(X, len(C0), i + 1, 1e-300, 0, True, 1, init_centroids=C0)
        assert fit["n_iter"] == i + 1
        np.testing.assert_array_equal(r["counts"], fit["records"][-1]["sizes"])
        np.testing.assert_allclose(r["new"], fit["centroids"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(r["sse"], fit["sse_history"][-1], rtol=1e-12)
    # ties go to the lowest index, as np.argmin gives them
    X, C0 = rd.mixed_case("outlier_row", "A")
    assert rd.assign(X, C0)[0][0] == orc.assign(X[:1], C0)[0][0] == 0


@pytest.mark.parametrize("name", list(rd.CLASSES))
def test_scale_sweep_inputs(name):
    n, d, k, dp, kp, _, _ = rd.CLASSES[name]
    assert dp == (d + 15) // 16 * 16 and kp == (k + 63) // 64 * 64 and (k > 32 or d > 64)
    first = None
    for scale in rd.SCALES:
        X, C0 = rd.class_case(name, scale)
        assert X.shape == (n, d) and C0.shape == (k, d)
        assert len(np.unique(C0, axis=0)) == k
        labels, _ = _basic(X, C0)
        # the label a screen gives when it drops the norm term
        dropped = np.argmin(-2.0 * (X @ C0.T), axis=1)
        assert (dropped != labels).mean() >= 0.5, (dropped != labels).mean()
        assert (_gaps(X, C0) > 1e-3).mean() >= 0.9
        assert np.bincount(labels, minlength=k).min() > 0
        # row norms spread over a decade, and what the fp32 forms lose
        rn = np.sqrt((X * X).sum(axis=1))
        assert rn.max() / rn.min() > 8
        c2 = (C0 * C0).sum(axis=1)
        with np.errstate(over="ignore", under="ignore"):
            c2f = c2.astype(np.float32)
        if scale <= 1e-22:
            assert (c2f < F32_TINY).all()              # denormal or zero before the scale is applied
        if scale >= 1e19:
            assert np.isinf(c2f).any()
        if scale == 1e18:
            # ||c||^2 up to 4 d 1e36: some centroids overflow and some do not for d >= 90
            assert np.isinf(c2f).any() == (d >= 90) and not np.isinf(c2f).all()
        if first is None:
            first = labels
        # (the same noise at every scale, rounded to float32 at each: nearly the same labels)
        assert (labels != first).mean() < 0.01


@pytest.mark.parametrize("name", rd.ITER_CLASSES)
def test_iteration_inputs(name):
    k = rd.CLASSES[name][2]
    for scale in rd.ITER_SCALES:
        X, C0 = rd.class_case(name, scale)
        for r in rd.lloyd(X, C0, rd.ITERS):
            assert r["counts"].min() > 0 and np.isfinite(r["new"]).all() and np.isfinite(r["sse"]) and r["sse"] > 0
        s = rd.s1_scale(np.abs(X).max(), np.abs(C0).max())
        assert not 2.0 ** -30 <= s <= 2.0 ** 30         # outside the row gate's range
    assert k == len(C0)


def test_gate_scale_inputs():
    want = {"s=2^30": 2.0 ** 30, "s=2^31": 2.0 ** 31, "s=2^-30": 2.0 ** -30, "s=2^-31": 2.0 ** -31}
    for inside, outside in rd.GATE_PAIRS:
        runs = {}
        for side in (inside, outside):
            X, C0 = rd.gate_scale(side)
            _basic(X, C0)
            m = max(np.abs(X).max(), np.abs(C0).max())
            assert m == 1.5 * 2.0 ** rd.GATE_SIDES[side]
            assert rd.s1_scale(np.abs(X).max(), np.abs(C0).max()) == want[side]
            runs[side] = (X, rd.lloyd(X, C0, rd.ITERS))
        assert 2.0 ** -30 <= want[inside] <= 2.0 ** 30 and not 2.0 ** -30 <= want[outside] <= 2.0 ** 30
        # the same rows up to an exact factor of two: the same labels in every iteration
        f = runs[outside][0][0, 0] / runs[inside][0][0, 0]
        assert f in (0.5, 2.0) and np.array_equal(runs[outside][0], runs[inside][0] * f)
        for a, b in zip(runs[inside][1], runs[outside][1]):
            np.testing.assert_array_equal(a["labels"], b["labels"])
            assert a["counts"].min() > 0
            assert np.array_equal(a["new"] * f, b["new"])
        # labels still move in the third pass (the gate has something to skip, not everything)
        moved = (runs[inside][1][2]["labels"] != runs[inside][1][1]["labels"]).mean()
        assert 0 < moved < 0.5, moved


@pytest.mark.parametrize("name", rd.MIXED_CLASSES)
def test_mixed_inputs(name):
    n, d, k = rd.CLASSES[name][:3]
    X, C0 = rd.mixed_case("outlier_row", name)
    labels, mind = _basic(X, C0)
    assert np.abs(X[0]).max() > 1e20 and np.abs(X[1:]).max() < 20 and np.abs(C0).max() < 20
    assert rd.s1_scale(np.abs(X).max(), np.abs(C0).max()) <= 2.0 ** -54
    assert len(np.unique(orc.distances(X[:1], C0))) == 1 and labels[0] == 0    # float64 cannot tell: a k-way tie
    assert np.bincount(labels, minlength=k).min() > 0

    X, C0 = rd.mixed_case("outlier_centroid", name)
    labels, _ = _basic(X, C0)
    counts = np.bincount(labels, minlength=k)
    assert counts[k // 2] == 0 and (np.delete(counts, k // 2) > 0).all()
    assert np.abs(C0[k // 2]).max() == float(np.float32(1e20)) and np.abs(X).max() < 20

    X, C0 = rd.mixed_case("tiny_rows", name)
    labels, mind = _basic(X, C0, zero_centroids=[3])
    tiny = np.arange(n) % 7 == 0
    assert np.abs(X[tiny]).max() < 2e-24 and np.abs(X[~tiny]).max() > 1
    assert (labels[tiny] == 3).all() and mind[tiny].max() < 1e-22
    assert np.bincount(labels, minlength=k).min() > 0

    X, C0 = rd.mixed_case("denormal_rows", name)
    labels, _ = _basic(X, C0)
    assert np.abs(X).max() < F32_TINY and np.abs(C0).max() < F32_TINY
    assert np.bincount(labels, minlength=k).min() > 0
    assert (_gaps(X, C0) > 1e-3).mean() >= 0.9
