"""CPU tests of ``fit(..., sample_weight=w)``'s host side through the
``_engine_factory`` seam (tests/weighted_ref.py: the NumPy restatement and an
oracle engine with weights): validation, the unweighted result for None /
all-ones weights, per-rank slicing over two gloo ranks with uneven shards,
and the integer-weight identity on the restatement itself."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest

from conftest import ROOT
from oracle import kmeans_oracle as orc


def _ka():
    import kmeans_amd
    return kmeans_amd


@pytest.fixture
def weighted_engine():
    ka = _ka()
    import weighted_ref as wr
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(wr.factory)
    yield
    ka.KMeans._engine_factory = old


def _blobs(n, d, k, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10, 10, (k, d))
    lab = rng.integers(0, k, n)
    X = (centers[lab] + spread * rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)
    C0 = (centers + 0.05 * rng.standard_normal((k, d)))
    return X, C0


def _pinned(init, seed=7):
    ka = _ka()

    class Pinned(ka.KMeans):
        def _initialize_centroids(self, run):
            return init.copy()

        def _empty_seed(self):
            return seed
    return Pinned


def _fit(X, C0, w, slices=3, max_iter=6, sse=True, tol=1e-9):
    ka = _ka()
    sc = ka.LocalContext()
    rdd = sc.parallelize(X, slices)
    km = _pinned(C0)(k=len(C0), max_iter=max_iter, tolerance=tol, compute_sse=sse)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if w is None:
            km.fit(rdd, sc)
        else:
            km.fit(rdd, sc, sample_weight=w)
    return km, buf.getvalue()


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0, -1.0])
def test_weights_must_be_finite_and_positive(weighted_engine, bad):
    X, C0 = _blobs(200, 4, 3, 0)
    w = np.ones(len(X))
    w[17] = bad
    with pytest.raises(ValueError, match="sample_weight must be finite and positive"):
        _fit(X, C0, w)


@pytest.mark.parametrize("m", [199, 201, 0])
def test_wrong_length_names_both_lengths(weighted_engine, m):
    X, C0 = _blobs(200, 4, 3, 0)
    with pytest.raises(ValueError) as e:
        _fit(X, C0, np.ones(m))
    assert str(m) in str(e.value) and "200" in str(e.value)


def test_kmeans_parallel_with_weights_is_refused(weighted_engine):
    ka = _ka()
    X, _ = _blobs(200, 4, 3, 0)
    km = ka.KMeans(k=3, init="k-means||")
    with pytest.raises(ValueError, match=r"k-means\|\| with sample_weight is not supported yet"):
        km.fit(X, sample_weight=np.ones(len(X)))


# ------------------------------------------------- None / ones = unweighted
def test_none_and_ones_give_the_unweighted_result(weighted_engine):
    ka = _ka()
    import cpu_engine as ce
    X, C0 = _blobs(1500, 6, 5, 1, spread=2.0)
    a, out_a = _fit(X, C0, None)
    b, out_b = _fit(X, C0, np.ones(len(X)))
    assert a._runner.engine.w is None and b._runner.engine.w is not None
    ka.KMeans._engine_factory = staticmethod(ce.factory)   # the engine without load_weights at all
    c, out_c = _fit(X, C0, None)
    ref = orc.lloyd_fit(X, len(C0), 6, 1e-9, 42, True, 3, init_centroids=C0)
    for km in (a, b, c):
        np.testing.assert_allclose(km.centroids, ref["centroids"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(km.sse_history, ref["sse_history"], rtol=1e-12)
    assert out_a == out_c
    assert [ln.split("Cluster Sizes")[1] for ln in out_b.splitlines() if "Cluster Sizes" in ln] == \
           [ln.split("Cluster Sizes")[1] for ln in out_a.splitlines() if "Cluster Sizes" in ln]


def test_weighted_driver_matches_the_restatement(weighted_engine):
    import weighted_ref as wr
    X, C0 = _blobs(1501, 5, 4, 2, spread=2.5)
    C0[3] = 1e3                                           # one far-away centroid: empty at iteration 1
    w = np.exp(np.random.default_rng(3).uniform(-7, 7, len(X)))
    km, out = _fit(X, C0, w, slices=3, max_iter=5)
    lines = []
    sc = _ka().LocalContext()
    rdd = sc.parallelize(X, 3)
    sizes = [rdd.partition_len(i) for i in range(3)]
    ref = wr.weighted_lloyd_fit(X, w, 4, 5, 1e-9, True, sizes, C0, empty_seed=lambda: 7, log=lines.append)
    assert ref["records"][0]["empty"] == [3]
    np.testing.assert_allclose(km.centroids, ref["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(km.sse_history, ref["sse_history"], rtol=1e-9)
    assert out.splitlines() == lines


# ------------------------------------------- the identity on the restatement
def test_integer_weights_equal_repeated_rows_on_the_restatement():
    import weighted_ref as wr
    X, C0 = _blobs(900, 7, 6, 4)
    w = np.random.default_rng(5).integers(1, 4, len(X))
    gap, emptied = wr.top2_gap_and_empties(X, w, 6, 8, 1e-9, C0)
    assert gap > 1e-6 and not emptied
    a = wr.weighted_lloyd_fit(X, w.astype(np.float64), 6, 8, 1e-9, True, [len(X)], C0)
    Xr = np.repeat(X, w, axis=0)
    b = orc.lloyd_fit(Xr, 6, 8, 1e-9, 42, True, 1, init_centroids=C0)
    assert a["n_iter"] == b["n_iter"]
    np.testing.assert_allclose(a["centroids"], b["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(a["sse_history"], b["sse_history"], rtol=1e-9)
    np.testing.assert_array_equal(orc.predict(X, a["centroids"]), orc.predict(Xr, b["centroids"])[np.cumsum(w) - 1])
    # the weighted step's counts are rows, its W the repeated rows
    _, _, W, n, _, _ = wr.weighted_step(X, w, C0)
    assert W.sum() == len(Xr) and n.sum() == len(X)


def test_prefiltered_labels_equal_the_oracle_assignment():
    # weighted_ref.exact_labels' large-problem route against orc.assign on
    # rows with exact ties (duplicate centroids, midpoints) and near-ties
    import weighted_ref as wr
    rng = np.random.default_rng(8)
    C = rng.uniform(-3, 3, (40, 6)).astype(np.float32).astype(np.float64)
    C[7] = C[3]                                             # a duplicate: argmin keeps index 3
    X = (C[rng.integers(0, 40, 3000)] + 0.5 * rng.standard_normal((3000, 6))).astype(np.float32).astype(np.float64)
    X[:50] = 0.5 * (C[10] + C[11])                          # exact midpoints
    X[50:100] = 0.5 * (C[12] + C[13]) + 1e-7
    ref, _, ref_gap = orc.assign(X, C)
    lab, gap = wr.exact_labels(X, C, direct_limit=0, with_gap=True)
    np.testing.assert_array_equal(lab, ref)
    assert gap == pytest.approx(float(ref_gap.min()), abs=1e-7)
    np.testing.assert_array_equal(wr.exact_labels(X, C), ref)


# ------------------------------------------------- two gloo ranks, uneven shards
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


N_RANKS = 1001   # odd: the two ranks hold 500 and 501 rows, across 3 partitions


def _case():
    X, C0 = _blobs(N_RANKS, 5, 4, 11, spread=2.5)
    w = np.exp(np.random.default_rng(12).uniform(-7, 7, len(X)))
    return X, C0, w


def _rank_main(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmeans_amd as ka
        import weighted_ref as wr
        ka.KMeans._engine_factory = staticmethod(wr.factory)
        X, C0, w = _case()
        km, out = _fit(X, C0, w, slices=3, max_iter=5)
        run = km._runner
        q.put((rank, km.centroids, km.sse_history, run.pl.row0, run.pl.n_local, run.engine.weight_loads, out))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_slice_the_weights_and_match_one_rank():
    import torch.multiprocessing as mp
    import weighted_ref as wr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    X, C0, w = _case()
    rdd = _ka().LocalContext().parallelize(X, 3)
    sizes = [rdd.partition_len(i) for i in range(3)]
    ref = wr.weighted_lloyd_fit(X, w, 4, 5, 1e-9, True, sizes, C0, empty_seed=lambda: 7)
    assert [r[4] for r in res] == [500, 501] and [r[3] for r in res] == [0, 500]
    for rank, C, sse, row0, n_local, loads, out in res:
        assert len(loads) == 1
        np.testing.assert_array_equal(loads[0], w[row0:row0 + n_local])
        np.testing.assert_allclose(C, ref["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, ref["sse_history"], rtol=1e-9)
    assert res[0][6] and not res[1][6]
