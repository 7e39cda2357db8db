"""k_s1 (csrc/km_screen1.hip) on dense multi-tile waves: the state a wave
carries from one 16-row tile to the next -- the re-scoring ring's fill, the
queue cursors against the wave's segment, the change-list cursor, the row
buffers' rotation -- pinned bit-exact against the float64 oracle.

Reference: kmeans_spark.py:147-159 (np.argmin of np.linalg.norm(C - x,
axis=1), first minimum) and :169-206 (per-cluster sums, mean update).

The rows come from tests/s1_dense_data.py: twin centroids on well separated
sites, so that every row of a twin site has exactly two candidates (a ring
row), a few thousand distinct rows repeated to n = 5 n_cu waves 16 + 7 rows
(five tiles per wave of a full grid and a ragged last tile).  Its CPU
preconditions (check_ring_rows, fit_case; also run without a GPU in
tests/test_host_s1_dense.py) are asserted before a kernel is launched.  On
the twelve-wave geometries (c3: d 64, k 254; c4: d 32, k 1000) the ring has 12
slots and a tile adds 16 rows: the fill goes 0 -> 4 -> 8 -> 0 (two batches in
the third tile), which the kernel before km_s1_ring.h got wrong from the
fourth tile on.

Bars: labels bit-identical to the oracle's over every row; centroids and SSE
at rtol = atol = 1e-9 (tests/test_gpu_s1.py's bars).
"""
import functools

import numpy as np
import pytest

import s1_dense_data as sd
from oracle import kmeans_oracle as orc
from test_gpu_s1 import S1, _engine, _fit, _predict

pytestmark = pytest.mark.gpu

TILES = 5  # per wave (four reach the 12-slot ring's second batch: one to spare)
C3 = (64, 254, 8)    # d, k, offsets pattern: 12 waves, 12-slot ring, fp32 table in LDS
C4 = (32, 1000, 4)   # 12 waves, 12-slot ring, fp32 table in global memory
W8 = (64, 126, 8)    # 8 waves, 16-slot ring: the control


@functools.lru_cache(maxsize=None)
def _n_cu():
    eng = _engine()
    n_cu = eng.info()["n_cu"]
    eng.close()
    return n_cu


def _rows(d, k):
    return sd.rows_for_tiles(d, k, _n_cu(), TILES)


@functools.lru_cache(maxsize=None)
def _oracle_labels(d, k, kind, n_single, pattern):
    ds = sd.dense(d, k, kind, n_single, pattern=pattern)
    return orc.assign(ds.U, ds.C, chunk=sd.ORACLE_CHUNK)[0]


def _check_predict(d, k, pattern, kind, n_single=0):
    ds = sd.dense(d, k, kind, n_single, pattern=pattern)
    sd.check_ring_rows(ds)  # CPU preconditions first
    ref = _oracle_labels(d, k, kind, n_single, pattern)
    n = _rows(d, k)
    inverse = sd.expand(len(ds.U), n, seed=k + n_single)
    # (predict takes k_s1 on every geometry with an instance; screen() names
    # the screen of the next pass with statistics, checked by the fits below)
    labels, eng = _predict(ds.U.astype(np.float32)[inverse], ds.C)
    assert eng.info()["n"] == n
    np.testing.assert_array_equal(labels, ref[inverse])
    return ds, inverse, ref


# -- predict (MODE 0): every row a ring row, five tiles per wave ------------------------------

@pytest.mark.parametrize("kind", ["exact", "ulp", "near"])
def test_predict_c3_every_row_needy(kind):
    # exact and one-ulp twins leave the ring for the float64 pair re-rank
    # (kind 1: qn advances by 16 per tile), near twins are decided in it
    _check_predict(*C3, kind)


@pytest.mark.parametrize("kind", ["exact", "near"])
def test_predict_c4_every_row_needy(kind):
    _check_predict(*C4, kind)


@pytest.mark.parametrize("kind", ["exact", "near"])
def test_predict_c3_mixed_partial_fills(kind):
    # 118 twin sites and 18 single-centroid sites (87% of the rows on twin
    # sites), random order: 10..16 ring rows per tile, every ring fill
    ds, inverse, _ = _check_predict(*C3, kind, n_single=18)
    share = float(np.mean(ds.twin_rows[inverse]))
    assert 0.8 < share < 0.9, share


@pytest.mark.parametrize("kind", ["exact", "near"])
def test_predict_16_slot_ring_control(kind):
    # d 64, k 126: eight waves, 16 slots -- the same construction
    assert sd.geometry(W8[0], W8[1])["ring"] == 16 and sd.geometry(C3[0], C3[1])["ring"] == 12
    _check_predict(*W8, kind)


def test_predict_far_from_origin_dense_full_scans():
    # test_gpu_s1.test_predict_far_from_origin's rows and centroids at the
    # multi-tile n: most rows have more candidates than the kernel re-scores
    # and go to the float64 scan, so qf fills every wave's segment from the
    # back across its tiles
    X = sd.blobs(20000, 64, 128, seed=5, box=1000.0, std=1.0)
    C = X[np.random.default_rng(2).choice(len(X), 256, replace=False)]
    ref = orc.assign(X, C)[0]
    inverse = sd.expand(len(X), _rows(64, 256), seed=6)
    labels, eng = _predict(X.astype(np.float32)[inverse], C)
    np.testing.assert_array_equal(labels, ref[inverse])


# -- fits: three k_s1 delta iterations over rows that stay ring rows ------------------------------

def _check_dense_fit(d, k, pattern, compute_sse):
    iters = 4
    ds, C0, inverse, ref, info = sd.fit_case(d, k, iters=iters, n=_rows(d, k), pattern=pattern)
    X = ds.U[inverse]
    km = _fit(X, C0, iters, compute_sse=compute_sse)
    eng = km._runner.engine
    assert eng.screen() == S1, "k_s1 not selected for this geometry"
    assert eng.info()["delta_stats"] == 1
    assert km._runner.iterations_ran == iters
    np.testing.assert_allclose(km.centroids, ref["centroids"][iters], rtol=1e-9, atol=1e-9)
    # the last pass's labels: the oracle's at the centroids that pass read
    np.testing.assert_array_equal(eng.labels(), ref["labels"][iters - 1][inverse])
    np.testing.assert_array_equal(km._runner.last["counts"], np.bincount(eng.labels(), minlength=k))
    np.testing.assert_array_equal(km._runner.last["counts"], ref["counts"][iters - 1])
    if compute_sse:
        np.testing.assert_allclose(km.sse_history, ref["sse_history"], rtol=1e-9)
    return km


def test_fit_c3_near_twins_delta_iterations():
    # passes 2..4 are k_s1 with delta statistics (one of them the REV
    # instance); a quarter, then an eighth of the rows change sides
    _check_dense_fit(*C3, compute_sse=False)


def test_fit_c4_near_twins_delta_iterations():
    _check_dense_fit(*C4, compute_sse=False)


def test_fit_c3_near_twins_sse_delta_iterations():
    # the SSE instance: the residuals are added from inside the ring's batches
    _check_dense_fit(*C3, compute_sse=True)


def test_exact_twins_delta_pass_every_row_through_the_ring():
    # exact twins at fixed centroids (a fit would empty the higher twin and
    # repair it): a full-statistics pass, its update (not committed), then a
    # delta pass of k_s1 at the same centroids.  Every row leaves the ring as
    # kind 1, so the pair re-rank count equals the row count: direct evidence
    # that every row of every tile went through the ring; no label changes
    d, k, pattern = C3
    ds = sd.dense(d, k, "exact", pattern=pattern)
    sd.check_ring_rows(ds)
    ref = _oracle_labels(d, k, "exact", 0, pattern)
    n = _rows(d, k)
    inverse = sd.expand(len(ds.U), n, seed=k)
    eng = _engine()
    eng.load_host(ds.U.astype(np.float32)[inverse])
    eng.set_centroids(ds.C)
    eng.assign_stats()
    eng.update()
    assert eng.info()["delta_stats"] == 0
    np.testing.assert_array_equal(eng.labels(), ref[inverse])
    eng.assign_stats()
    assert eng.screen() == S1 and eng.info()["delta_stats"] == 1
    st, counts = eng.update()
    assert (st.q_rerank, st.q_full) == (n, 0)
    np.testing.assert_array_equal(eng.labels(), ref[inverse])
    np.testing.assert_array_equal(counts, np.bincount(ref[inverse], minlength=k))
