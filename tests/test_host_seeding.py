"""CPU tests of k-means|| seeding (``init="k-means||"``, seeding.py): the
public parameters, the hash, the weighted recluster, and the driver through a
test-only CPU engine (tests/seeding_ref.py) against a NumPy restatement of
the algorithm, on one rank and on two gloo ranks."""
import contextlib
import inspect
import io
import os
import re
import socket

import numpy as np
import pytest

from conftest import ROOT
from oracle import kmeans_oracle as orc


def _ka():
    import kmeans_amd
    return kmeans_amd


@pytest.fixture
def seed_engine():
    ka = _ka()
    import seeding_ref as ref
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(ref.factory)
    yield ref
    ka.KMeans._engine_factory = old


def _blobs(seed, n=4000, d=8, c=16, box=100.0, std=1.0):
    """Well-separated blobs: float32 rows, their centres and their blob ids."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-box, box, (c, d))
    lab = rng.integers(0, c, n)
    X = (centers[lab] + std * rng.standard_normal((n, d))).astype(np.float32)
    return X, centers, lab


def _fit(X, **kw):
    """(model, captured initial centroids, log) of a fit through the CPU engine."""
    ka = _ka()

    class Capturing(ka.KMeans):
        def _initialize_centroids(self, run):
            self.init_centroids = super()._initialize_centroids(run)
            return self.init_centroids

    km = Capturing(**kw)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(X)
    return km, km.init_centroids, buf.getvalue()


# ------------------------------------------------------------ public surface
def test_parameter_validation():
    ka = _ka()
    with pytest.raises(ValueError, match="init must be"):
        ka.KMeans(k=3, init="kmeans++")
    with pytest.raises(ValueError, match="init_rounds"):
        ka.KMeans(k=3, init="k-means||", init_rounds=0)
    with pytest.raises(ValueError, match="oversampling"):
        ka.KMeans(k=3, init="k-means||", oversampling=0)
    with pytest.raises(ValueError, match="oversampling"):
        ka.KMeans(k=3, oversampling=-1.5)
    km = ka.KMeans(k=3, init="k-means||", init_rounds=1, oversampling=0.5)
    assert (km.init, km.init_rounds, km.oversampling) == ("k-means||", 1, 0.5)


def test_new_parameters_are_keyword_only_after_the_reference_five():
    ka = _ka()
    sig = inspect.signature(ka.KMeans.__init__)
    names = list(sig.parameters)[1:]
    assert names == ["k", "max_iter", "tolerance", "seed", "compute_sse", "init", "init_rounds", "oversampling"]
    for n in names[5:]:
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["init"].default == "random"
    assert sig.parameters["init_rounds"].default == 5
    assert sig.parameters["oversampling"].default is None
    with pytest.raises(TypeError):
        ka.KMeans(3, 100, 1e-4, 42, False, "k-means||")


def test_default_init_is_the_reference_path(golden, seed_engine):
    # a model built without the new arguments: the golden run, log lines included
    from test_gpu_parity import assert_logs_match
    ka = _ka()
    g = golden("test_a")
    sc = ka.LocalContext()
    rdd = sc.parallelize(g["X"], int(g["slices"]))
    km = ka.KMeans(k=int(g["k"]), max_iter=int(g["max_iter"]), tolerance=float(g["tol"]), seed=int(g["seed"]),
                   compute_sse=bool(g["sse"]))
    assert km.init == "random"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(rdd, sc)
    np.testing.assert_allclose(km.centroids, g["centroids"], rtol=1e-9, atol=1e-9)
    assert_logs_match(buf.getvalue(), g["stdout"])
    assert "Initialization" not in buf.getvalue()


# --------------------------------------------------------------------- hash
def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    return z ^ (z >> 31)


def _u(seed, r, g):
    h = _splitmix64(_splitmix64((seed % 2 ** 64) ^ ((r * 0xD1B54A32D192ED03) % 2 ** 64)) ^ g)
    return (h >> 11) * 2.0 ** -53


def test_hash_matches_scalar_python():
    from kmeans_amd import seeding
    import seeding_ref as ref
    # SplitMix64's first output from state 0 (Steele, Lea & Flood; the published test vector)
    assert _splitmix64(0) == 0xE220A8397B1DCDAF == seeding.splitmix64(0)
    for seed, r, g in [(42, 1, 0), (42, 5, 20002), (0, 1, 1), (2 ** 63 + 11, 3, 2 ** 33 + 5), (-7, 2, 123456789),
                       (1_700_000_000, 4, 2 ** 40)]:
        want = _u(seed, r, g)
        assert 0.0 <= want < 1.0
        assert seeding.uniforms(seed, r, [g])[0] == want
        assert ref.uniforms(seed, r, [g])[0] == want
    # the NumPy form of the pick rule is the restatement's, infinities and NaN included
    d2 = np.array([0.0, 1.0, np.inf, np.nan, 5e-3, 2.0, 1e300])
    for ell, phi in [(4.0, 8.0), (1e6, 1e-300), (0.5, 1e300)]:
        np.testing.assert_array_equal(seeding.pick_rule(d2, 9, 2, 2 ** 33 + 5, ell, phi),
                                      ref.pick(d2, 9, 2, 2 ** 33 + 5, ell, phi)[0])


# ---------------------------------------------------------------- recluster
def test_recluster_distinct_deterministic_and_duplicates_last():
    from kmeans_amd import seeding
    rng = np.random.default_rng(5)
    C = rng.normal(size=(40, 6))
    w = rng.integers(1, 50, 40)
    a = seeding.recluster(C, w, 12, 42)
    assert len(a) == 12 and len(set(a)) == 12 and all(0 <= j < 40 for j in a)
    assert a == seeding.recluster(C, w, 12, 42)
    assert a != seeding.recluster(C, w, 12, 43)
    import seeding_ref as ref
    assert a == ref.recluster(C, w, 12, 42)
    # candidates 3 and 7 repeat candidate 1 (a tie keeps the earliest id: they get no rows)
    C2 = rng.normal(size=(8, 4))
    C2[3] = C2[1]
    C2[7] = C2[1]
    w2 = np.array([5, 9, 4, 0, 6, 3, 8, 0])
    for seed in range(6):
        order = seeding.recluster(C2, w2, 8, seed)
        assert sorted(order) == list(range(8))
        assert order[-2:] == [3, 7], order          # total weight 0: lowest id first
        assert order == ref.recluster(C2, w2, 8, seed)


# ------------------------------------------------------------ the driver
def test_fit_equals_restatement_then_oracle(seed_engine):
    ref = seed_engine
    X = _blobs(0, n=3001, d=7, c=9)[0].astype(np.float64)  # float64 input: centroids come back as float64
    k, seed = 9, 42
    want = ref.kmeans_parallel_ref(X, [len(X)], k, seed, rounds=4, oversampling=11.0)
    km, init, log = _fit(X, k=k, max_iter=20, tolerance=1e-6, seed=seed, compute_sse=True, init="k-means||",
                         init_rounds=4, oversampling=11.0)
    np.testing.assert_array_equal(init, want["centroids"])
    lines = log.splitlines()
    assert lines[0].startswith("Starting K-Means") and lines[1].startswith("SSE computation")
    assert lines[2] == f"Initialization: k-means|| (rounds={want['rounds']}, candidates={len(want['candidates'])})"
    assert lines[3].startswith("Iteration 1:")
    o = orc.lloyd_fit(X, k, 20, 1e-6, seed, True, 1, init_centroids=want["centroids"])
    np.testing.assert_allclose(km.centroids, o["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(km.sse_history, o["sse_history"], rtol=1e-9)
    np.testing.assert_array_equal(np.array(km.predict(X).collect()), orc.predict(X, o["centroids"]))


def test_pick_overflow_falls_back_to_the_numpy_rule():
    ka = _ka()
    import seeding_ref as ref
    X, _, _ = _blobs(1, n=1500, d=5, c=6)
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(ref.factory_small_cap)
    try:
        _, init, _ = _fit(X, k=6, max_iter=1, seed=3, init="k-means||")
    finally:
        ka.KMeans._engine_factory = old
    np.testing.assert_array_equal(init, ref.kmeans_parallel_ref(X, [len(X)], 6, 3)["centroids"])


def test_not_enough_rows_gives_the_reference_message(seed_engine):
    ka = _ka()
    X = np.arange(10.0).reshape(5, 2)
    with pytest.raises(ValueError, match=re.escape("Not enough data points (5) to initialize 6 clusters")):
        ka.KMeans(k=6, init="k-means||").fit(X)
    sc = ka.LocalContext()
    with pytest.raises(ValueError, match=re.escape("Not enough data points (0) to initialize 4 clusters")):
        ka.KMeans(k=4, init="k-means||").fit(sc.parallelize(np.zeros((0, 3)), 2), sc)


def test_non_finite_rows_raise(seed_engine):
    ka = _ka()
    X = np.random.default_rng(0).normal(size=(40, 3))
    X[:, 1] = np.nan
    with pytest.raises(ValueError, match=re.escape("Data contains NaN or Inf values")):
        ka.KMeans(k=3, init="k-means||").fit(X)


def test_fewer_candidates_than_k_are_topped_up(seed_engine):
    ref = seed_engine
    # three distinct rows, each many times: phi reaches 0 with at most a few candidates
    vals = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0]])
    X = vals[np.random.default_rng(2).integers(0, 3, 60)].astype(np.float32)
    k, seed = 8, 5
    want = ref.kmeans_parallel_ref(X, [len(X)], k, seed, oversampling=0.5)
    M = len(want["candidates"])
    assert M < k, "the case must exercise the top-up"
    _, init, log = _fit(X, k=k, max_iter=1, seed=seed, init="k-means||", oversampling=0.5)
    np.testing.assert_array_equal(init, want["centroids"])
    assert init.shape == (k, 2)
    assert f"candidates={M})" in log
    # the candidates come first, then takeSample's rows that are no candidates, in its order
    extra = [g for g in orc.take_sample_indices([len(X)], k, seed) if g not in set(want["candidates"])][:k - M]
    assert want["index"][M:] == extra and len(set(want["index"])) == k
    assert sorted(want["index"][:M]) == sorted(want["candidates"])


# ------------------------------------------------------------------ quality
def test_every_blob_gets_a_seed_where_takesample_misses_some(seed_engine):
    ref = seed_engine
    X, centers, lab = _blobs(0)
    k, seed = 16, 42
    X64 = X.astype(np.float64)
    # the blob radius: the farthest any row lies from its own centre
    radius = float(np.sqrt(((X64 - centers[lab]) ** 2).sum(1)).max())
    gap = np.sqrt(((centers[:, None] - centers[None]) ** 2).sum(-1))
    assert gap[gap > 0].min() > 4 * radius, "blobs must be well separated"

    def farthest(C):  # the largest distance from a centre to its nearest seed
        return float(np.sqrt(((centers[:, None, :] - C[None]) ** 2).sum(-1)).min(1).max())

    want = ref.kmeans_parallel_ref(X, [len(X)], k, seed)
    random_init = X64[orc.take_sample_indices([len(X)], k, seed)]
    # the restatement alone satisfies both claims
    assert farthest(want["centroids"]) <= radius
    assert farthest(random_init) > radius
    _, init, _ = _fit(X, k=k, max_iter=1, seed=seed, init="k-means||")
    assert farthest(init) <= radius
    _, init_r, _ = _fit(X, k=k, max_iter=1, seed=seed)
    np.testing.assert_array_equal(init_r, random_init)


# ------------------------------------------------------ two ranks over gloo
GLOO_CASE = dict(n=2501, d=6, c=7, k=7, seed=11, data_seed=4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
        import seeding_ref as ref
        ka.KMeans._engine_factory = staticmethod(ref.factory)
        c = GLOO_CASE
        X = _blobs(c["data_seed"], n=c["n"], d=c["d"], c=c["c"])[0]
        km, init, log = _fit(X, k=c["k"], max_iter=3, seed=c["seed"], init="k-means||")
        q.put((rank, init, km.centroids, km._runner.pl.row0, km._runner.pl.n_local, log))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_seed_like_one(seed_engine):
    import torch.multiprocessing as mp
    ref = seed_engine
    c = GLOO_CASE
    X = _blobs(c["data_seed"], n=c["n"], d=c["d"], c=c["c"])[0]
    one = ref.kmeans_parallel_ref(X, [len(X)], c["k"], c["seed"])
    half = len(X) // 2
    two = ref.kmeans_parallel_ref(X, [len(X)], c["k"], c["seed"], shards=[(0, half), (half, len(X))])
    # phi of two ranks differs from one rank's by rounding only: no pick decision may sit that close
    assert one["margin"] > 1e-9 and two["margin"] > 1e-9, (one["margin"], two["margin"])
    np.testing.assert_array_equal(one["centroids"], two["centroids"])
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
    assert [r[3] for r in res] == [0, half] and sum(r[4] for r in res) == len(X)
    for rank, init, cent, _, _, log in res:
        np.testing.assert_array_equal(init, one["centroids"])
        np.testing.assert_array_equal(cent, res[0][2])
        assert ("Initialization: k-means||" in log) == (rank == 0)
    _, init1, _ = _fit(X, k=c["k"], max_iter=3, seed=c["seed"], init="k-means||")
    np.testing.assert_array_equal(init1, one["centroids"])
