"""Weighted k-means on the GPU (``fit(..., sample_weight=w)``; km_set_weights)
against the NumPy restatement of tests/weighted_ref.py.

1. one step per geometry (every statistics path: small, LDS table, feature
   ranges, counting sort, wide rows), compute_sse on and off;
2. the integer-weight identity against the existing unweighted path on
   ``np.repeat(X, w)``;
3. empty clusters inside batches, and the engine state around a weighted fit;
4. two gloo ranks on the GPU with uneven shards.
"""
import contextlib
import io
import os
import re
import socket

import numpy as np
import pytest

from conftest import ROOT
from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

# n, d, k: n < 64 and padded features; the small path; k_s1 labels + LDS
# table; the feature-range split; the sorted path; wide rows
GEOMETRIES = [(37, 5, 1), (5001, 16, 7), (20003, 64, 256), (20003, 32, 1024), (20003, 128, 4096), (2051, 300, 70)]


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


_cases = {}


def _case(n, d, k):
    """Data, initial centroids (k distinct rows plus a little noise), weights
    exp(uniform(-7, 7)) and the restatement's labels, computed once."""
    key = (n, d, k)
    if key not in _cases:
        import weighted_ref as wr
        rng = np.random.default_rng(1000 + n + d + k)
        centers = rng.uniform(-10, 10, (max(k // 4, 1), d))
        X = (centers[rng.integers(0, len(centers), n)] + rng.standard_normal((n, d)))
        X = X.astype(np.float32).astype(np.float64)
        C0 = X[rng.choice(n, k, replace=False)] + 0.01 * rng.standard_normal((k, d))
        w = np.exp(rng.uniform(-7, 7, n))
        _cases[key] = (X, C0, w, wr.exact_labels(X, C0))
    return _cases[key]


def _step(X, C0, w, sse):
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    if w is not None:
        eng.load_weights(w)
    eng.set_sse(sse)
    eng.set_centroids(C0)
    eng.assign_stats()
    st, counts = eng.update()
    out = {"labels": eng.labels(), "new": eng.get_centroids(1), "sse": st.sse, "counts": counts,
           "n_empty": st.n_empty, "info": eng.info()}
    eng.close()
    return out


# ------------------------------------------------------ 1. one step per geometry
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("n,d,k", GEOMETRIES)
def test_one_weighted_step_matches_the_restatement(n, d, k, sse):
    import weighted_ref as wr
    X, C0, w, labels = _case(n, d, k)
    got = _step(X, C0, w, sse)
    _, _, _, cnt, new, ref_sse = wr.weighted_step(X, w, C0, sse, labels)
    np.testing.assert_array_equal(got["labels"], labels)
    np.testing.assert_array_equal(got["counts"], np.bincount(labels, minlength=k))
    np.testing.assert_array_equal(got["counts"], cnt)
    assert got["n_empty"] == int((cnt == 0).sum())
    print(f"max |dC| = {np.abs(got['new'] - new).max():.3e}, sse {got['sse']!r} vs {ref_sse!r}")
    np.testing.assert_allclose(got["new"], new, rtol=1e-9, atol=1e-9)
    if sse:
        np.testing.assert_allclose(got["sse"], ref_sse, rtol=1e-9, atol=1e-9)
    assert got["info"]["delta_stats"] == 0


@pytest.mark.parametrize("n,d,k", [(20003, 64, 256), (5001, 16, 7)])
def test_equal_weights_give_the_unweighted_step(n, d, k):
    # w = 0.25 everywhere scales S and W by the same power of two: the
    # centroids are the unweighted ones up to the summation order, ~n_j 2^-53
    # of the data scale per coordinate (far inside 1e-12 of it)
    import weighted_ref as wr
    X, C0, _, labels = _case(n, d, k)
    w = np.full(n, 0.25)
    a = _step(X, C0, w, True)
    b = _step(X, C0, None, True)
    np.testing.assert_array_equal(a["labels"], b["labels"])
    np.testing.assert_array_equal(a["counts"], b["counts"])
    scale = float(np.abs(X).max())
    np.testing.assert_allclose(a["new"], b["new"], rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(a["sse"], 0.25 * b["sse"], rtol=1e-9)
    _, _, _, _, new, ref_sse = wr.weighted_step(X, w, C0, True, labels)
    np.testing.assert_allclose(a["new"], new, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(a["sse"], ref_sse, rtol=1e-9, atol=1e-9)


# ------------------------------------- 2. integer weights = repeated rows
def _separated(n, d, k, seed):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10, 10, (k, d))
    X = (centers[np.arange(n) % k] + 0.3 * rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)
    C0 = centers + 0.05 * rng.standard_normal((k, d))
    w = rng.integers(1, 4, n)
    return X, C0, w


def _pinned(C0, seed=1234):
    import kmeans_amd as ka

    class Pinned(ka.KMeans):
        def _initialize_centroids(self, run):
            return C0.copy()

        def _empty_seed(self):
            return seed
    return Pinned


def _fit(X, C0, w, max_iter, sse=True, tol=1e-9, verbose=False):
    km = _pinned(C0)(k=len(C0), max_iter=max_iter, tolerance=tol, compute_sse=sse)
    km.verbose = verbose
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if w is None:
            km.fit(X)
        else:
            km.fit(X, sample_weight=w)
    return km, buf.getvalue()


@pytest.mark.parametrize("n,d,k", [(6000, 16, 8), (20003, 64, 256)])
def test_integer_weights_equal_repeated_rows(n, d, k):
    import weighted_ref as wr
    X, C0, w = _separated(n, d, k, 77 + k)
    gap, emptied = wr.top2_gap_and_empties(X, w, k, 8, 1e-9, C0)
    assert gap > 1e-6 and not emptied, (gap, emptied)
    Xr = np.repeat(X, w, axis=0)
    a, _ = _fit(X, C0, w.astype(np.float64), 8)
    b, _ = _fit(Xr, C0, None, 8)
    assert a._runner.engine.info()["delta_stats"] == 0
    assert len(a.sse_history) == len(b.sse_history) and a._runner.iterations_ran == b._runner.iterations_ran
    np.testing.assert_allclose(a.centroids, b.centroids, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(a.sse_history, b.sse_history, rtol=1e-9, atol=1e-9)
    la = np.asarray(a.predict(X).collect())
    lb = np.asarray(b.predict(Xr).collect())
    np.testing.assert_array_equal(np.repeat(la, w), lb)


# ---------------------------------------- 3. empty clusters and engine state
def _numbers_out(text):
    return [re.sub(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", "#", ln) for ln in text.splitlines()]


def test_empty_cluster_in_a_weighted_fit_and_engine_state():
    import weighted_ref as wr
    n, d, k = 20003, 64, 256
    X, C0, _ = _separated(n, d, k, 5)
    C0 = C0.copy()
    C0[17] = 1e3                                          # far away: empty at the first update
    w = np.exp(np.random.default_rng(6).uniform(-7, 7, n))
    km, out = _fit(X, C0, w, 6, verbose=True)
    lines = []
    ref = wr.weighted_lloyd_fit(X, w, k, 6, 1e-9, True, [n], C0, empty_seed=lambda: 1234, log=lines.append)
    assert ref["records"][0]["empty"] == [17]
    np.testing.assert_allclose(km.centroids, ref["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(km.sse_history, ref["sse_history"], rtol=1e-9, atol=1e-9)
    assert "  WARNING: 1 empty cluster(s) detected. Reinitializing..." in out.splitlines()
    assert _numbers_out(out) == _numbers_out("\n".join(lines))
    run = km._runner
    # repaired on the device, inside the batch: no host round trip for it
    assert run.device_repairs == 1 and run.iterations_ran == ref["n_iter"] >= 2
    assert run.engine.info()["delta_stats"] == 0
    # an unweighted fit on a fresh model afterwards still runs delta statistics here
    km2, _ = _fit(X, C0, None, 4, sse=False)
    assert km2._runner.engine.info()["delta_stats"] == 1
    ref2 = orc.lloyd_fit(X, k, 4, 1e-9, 0, False, 1, init_centroids=C0, empty_seed=lambda: 1234)
    np.testing.assert_allclose(km2.centroids, ref2["centroids"], rtol=1e-9, atol=1e-9)


def test_clearing_weights_returns_to_the_unweighted_statistics():
    import ctypes
    X, C0, w, labels = _case(5001, 16, 7)
    eng = _engine()
    # KM_ERR_STATE (-3) before km_load_begin; KM_ERR_ARG (-1) past the rows
    pw = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert eng.lib.km_set_weights(eng.ctx, 0, pw, len(w)) == -3
    assert eng.lib.km_clear_weights(eng.ctx) == 0
    eng.load_host(X.astype(np.float32))
    assert eng.lib.km_set_weights(eng.ctx, 1, pw, len(w)) == -1
    with pytest.raises(ValueError):
        eng.load_weights(w[:-1])
    eng.load_weights(w)
    eng.set_centroids(C0)
    assert eng.stats_len() == 7 * 17 + 1 + 7
    eng.assign_stats()
    eng.update()
    eng.load_weights(None)
    assert eng.stats_len() == 7 * 17 + 1
    eng.assign_stats()
    _, counts = eng.update()
    new = eng.get_centroids(1)
    sums = np.zeros((7, 16))
    np.add.at(sums, labels, X)
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=7))
    np.testing.assert_allclose(new, sums / np.bincount(labels, minlength=7)[:, None], rtol=1e-9, atol=1e-9)
    eng.close()


# ------------------------------------------- 4. two gloo ranks, uneven shards
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_case(n, d, k):
    X, C0, _ = _separated(n, d, k, 31 + k)
    w = np.exp(np.random.default_rng(32).uniform(-7, 7, n))
    return X, C0, w


def _rank_main(rank, world, port, n, d, k, q):
    # rank 0 holds all rows but 500, rank 1 the last 500
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmeans_amd import dataset
        X, C0, w = _rank_case(n, d, k)
        dataset.rank_rows = lambda m, wd, r: (0, m - 500) if r == 0 else (m - 500, m)
        km, _ = _fit(X, C0, w, 5)
        eng = km._runner.engine
        assert eng.distributed and eng.weighted
        q.put((rank, km.centroids, km.sse_history, km._runner.pl.n_local, eng.info()["delta_stats"],
               int(eng._stats_t.numel())))
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e), None, None, None, None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n,d,k", [(6001, 16, 8), (20003, 64, 256)])
def test_two_ranks_weighted_match_one_rank(n, d, k):
    import torch.multiprocessing as mp
    import weighted_ref as wr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, n, d, k, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=110) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0, res
    X, C0, w = _rank_case(n, d, k)
    one, _ = _fit(X, C0, w, 5)
    ref = wr.weighted_lloyd_fit(X, w, k, 5, 1e-9, True, [n], C0, empty_seed=lambda: 1234)
    assert [r[3] for r in res] == [n - 500, 500]
    for rank, C, sse, _, dstat, slen in res:
        assert dstat == 0 and slen == k * (d + 1) + 1 + k
        np.testing.assert_allclose(C, one.centroids, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, one.sse_history, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(C, ref["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, ref["sse_history"], rtol=1e-9, atol=1e-9)
