"""The row gate with two ranks (torch.distributed over gloo, both on cuda:0)
holding uneven shards: rank 0 all rows but 500, rank 1 the last 500.  Their
k_s1 grids, work lists and segments differ, but the margins are stepped by the
same shifts on both (each rank measures them on the all-reduced centroids), so
the fit must match the oracle's (kmeans_spark.py:147-206) exactly as the
single-rank one does, with the gate active on both ranks."""
import os
import socket

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

D, K, ITERS = 64, 256, 7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(n=20000):
    # as test_gpu_s1_gate._split_blobs: 64 blob centres, 31 of them (twice the
    # weight) with one seed each, the other 33 split among 225 seeds; every
    # cluster keeps rows, so no repair moves a centroid mid-fit
    rng = np.random.default_rng(301)
    Cb = rng.uniform(-10, 10, (64, D))
    w = np.r_[np.full(31, 2.0), np.full(33, 1.0)]
    blob = rng.choice(64, n, p=w / w.sum())
    X = (Cb[blob] + rng.standard_normal((n, D))).astype(np.float32).astype(np.float64)
    lone = [int(np.nonzero(blob == b)[0][0]) for b in range(31)]
    rest = np.nonzero(blob >= 31)[0]
    C0 = X[np.r_[lone, rng.choice(rest, K - 31, replace=False)].astype(np.int64)].copy()
    return X, C0


def _rank(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmeans_amd as ka
        from kmeans_amd import dataset
        X, C0 = _data()
        dataset.rank_rows = lambda n, w, r: (0, n - 500) if r == 0 else (n - 500, n)

        class Pinned(ka.KMeans):
            def _initialize_centroids(self, run):
                return C0.copy()

            def _empty_seed(self):
                return 1234

        km = Pinned(k=K, max_iter=ITERS, tolerance=1e-12, compute_sse=False)
        km.verbose = False
        km.fit(X)
        eng = km._runner.engine
        info = eng.info()
        q.put((rank, km.centroids, info["delta_stats"], info["gated_rows"], km._runner.pl.n_local, eng.labels(),
               km._runner.last["counts"].copy()))
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e), None, None, None, None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_uneven_shards_gated_fit_matches_oracle():
    import torch.multiprocessing as mp
    from oracle import kmeans_oracle as orc
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=110) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0, res
    X, C0 = _data()
    n = len(X)
    assert [r[4] for r in res] == [n - 500, 500]
    ref = orc.lloyd_fit(X, K, ITERS, 1e-12, 0, False, 1, init_centroids=C0, empty_seed=lambda: 1234)
    C_prev = orc.lloyd_fit(X, K, ITERS - 1, 1e-12, 0, False, 1, init_centroids=C0,
                           empty_seed=lambda: 1234)["centroids"]
    lab = orc.assign(X, C_prev)[0]
    shards = [lab[:n - 500], lab[n - 500:]]
    for (rank, C, dstat, gated, n_local, labels, counts), want in zip(res, shards):
        assert dstat == 1, (rank, dstat)
        np.testing.assert_allclose(C, ref["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(labels, want)
        np.testing.assert_array_equal(counts, np.bincount(lab, minlength=K))
        assert 0 <= gated <= n_local, (rank, gated)
    # the large shard has rows to skip by the last iteration; the gate ran on both
    assert 0 < res[0][3] < n - 500, res[0][3]
