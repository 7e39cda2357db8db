"""CPU tests of the host side: C-ABI library loads and exports the header's
symbols, the takeSample policy, data placement, the KMeans driver (through a
test-only oracle engine) against the reference's golden vectors, and the
multi-rank path over gloo (world size 2)."""
import contextlib
import io
import json
import os
import re
import socket

import numpy as np
import pytest

from conftest import ROOT
from oracle import kmeans_oracle as orc

HEADER = os.path.join(ROOT, "include", "kmeans_amd.h")
INJECTED = ("empty", "ties", "tight", "tight_wide", "c5_poor")  # golden cases that inject their initial centroids


def _ka():
    import kmeans_amd
    return kmeans_amd


# --------------------------------------------------------------------- C-ABI
def test_library_exports_every_header_symbol():
    from kmeans_amd import _lib
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(km_\w+)\s*\(", text, re.M))
    assert declared, "no declarations parsed"
    lib = _lib.load()
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    assert lib.km_abi_version() == 6


def test_stats_route_is_bound_and_checks_its_arguments():
    # km_stats_route (added within ABI 6): five int32 outputs; a null context
    # is an argument error before anything touches a device
    import ctypes
    from kmeans_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["km_stats_route"]) == 6
    out = [ctypes.c_int32(-7) for _ in range(5)]
    assert lib.km_stats_route(None, *[ctypes.byref(v) for v in out]) == -1   # KM_ERR_ARG
    assert b"km_stats_route" in lib.km_last_error()
    assert [v.value for v in out] == [-7] * 5


def test_product_library_has_no_diagnostic_kernels():
    # the environment knobs exist only in the diagnostic build (make diag,
    # -DKM_DIAG); the timing-ablation variants of round 1-5 are gone (round 6)
    import subprocess
    from kmeans_amd import _lib
    syms = subprocess.run(["nm", "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    fused = re.findall(r"k_fused<\d+, \d+, (?:true|false), (?:true|false), (?:true|false)>", syms)
    mfma = re.findall(r"k_assign_mfma<\d+, \d+, (?:true|false)>", syms)
    assert fused and mfma, "kernel symbols not found"
    assert "k_fusedp" not in syms
    # the fast-screen experiment (k_fused1, k_prep_bal) is diagnostic-only too
    assert not re.search(r"k_fused1<", syms) and "k_prep_bal" not in syms
    # the two-MFMA pair screen is gone (round 6): k_fused16 has five template arguments
    assert re.findall(r"k_fused16<\d+, \d+, (?:true|false), (?:true|false), (?:true|false)>", syms)
    assert "k_pair_table" not in syms
    assert "getenv" not in subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True,
                                          text=True, check=True).stdout


def test_exact_helpers_forbid_contraction():
    # hipcc fuses `acc + t * t` into v_fma_f64 unless `#pragma clang fp
    # contract(off)` covers the add; a fused square is not NumPy's rounding
    # (kmeans_spark.py:153).  Every helper of km_exact.h that adds or
    # multiplies doubles opens with the pragma (the round-1 scan variant whose
    # own multi-point helper lacked it computed wrong norms; DESIGN.md section
    # 2).  Comparison-only helpers and sqrt wrappers over pragma'd sums are
    # listed explicitly.
    src = open(os.path.join(ROOT, "assignment--2-group7-distributed-k-means_amd", "csrc", "km_exact.h")).read()
    no_arith = {"np_better", "np_pick_second", "np_norm_d", "np_norm"}
    heads = list(re.finditer(r"__device__[^;{]*?\b(np_\w+)\s*\(", src))
    assert len(heads) >= 12, [m.group(1) for m in heads]
    for m in heads:
        name = m.group(1)
        body = src[src.index("{", m.end()) + 1:][:200]
        if name in no_arith:
            assert "+" not in body.split("}")[0].replace("++", "") or name.startswith("np_norm"), name
            continue
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), f"{name}: no contract(off) pragma"


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ka = _ka()
    with pytest.raises(RuntimeError):
        ka.KMeans(k=2).fit(np.random.default_rng(0).standard_normal((100, 4)))


# ------------------------------------------------------------------ sampling
@pytest.mark.parametrize("sizes,num,seed", [
    ([1000], 3, 42), ([250, 250, 250, 250], 6, 42), ([333, 333, 334], 5, 1700000000),
    ([40000, 40000], 256, 6), ([70000], 10, 123), ([5], 6, 42), ([0, 7, 0], 3, 9),
    ([100000, 1, 50000], 17, 2 ** 40 + 5),
])
def test_take_sample_matches_oracle_restatement(sizes, num, seed):
    from kmeans_amd import sampling
    assert sampling.take_sample(sizes, num, seed) == orc.take_sample_indices(sizes, num, seed)


def test_device_pass_keys_for_negative_and_huge_seeds():
    # the device pass gets abs(seed ^ p) as a uint64 MT key (what
    # random.Random(seed ^ p) seeds with); keys of 2^64 and more stay on the
    # host path.  The fake device draws from the key exactly as the host does.
    from kmeans_amd import sampling
    calls = []

    def fake_device(keys, sizes, bases, fraction):
        assert keys.dtype == np.uint64
        calls.append(keys.tolist())
        out = []
        for key, size, base in zip(keys.tolist(), sizes.tolist(), bases.tolist()):
            u = sampling._python_random_stream(int(key)).random_sample(size)
            out.append(np.nonzero(u < fraction)[0] + base)
        return np.concatenate(out)

    sizes = [40000, 30001, 0, 25000]
    for num, seed in [(5, -987654321), (17, -(2 ** 63)), (3, -1), (9, 2 ** 64 - 3)]:
        calls.clear()
        assert sampling.take_sample(sizes, num, seed, device=fake_device) == sampling.take_sample(sizes, num, seed)
        assert calls and calls[0] == [abs(seed ^ p) for p in (0, 1, 3)]
    calls.clear()
    for seed in (2 ** 64 + 5, -(2 ** 70)):
        assert sampling.take_sample(sizes, 4, seed, device=fake_device) == sampling.take_sample(sizes, 4, seed)
    assert not calls or all(max(c) < 2 ** 64 for c in calls)


# Literal outputs of CPython's own random module (3.10, MT19937 +
# init_by_array seeding + getrandbits rejection in randint), written down
# once: they pin the samplers to CPython independently of the oracle's
# restatement, so a drift shared by sampling.py and the oracle is caught.
CPYTHON_PICKS = [
    ([1000, 313, 1, 0, 700], 0.01, 42,
     [10, 115, 260, 281, 288, 359, 385, 418, 472, 675, 873, 1142, 1229, 1241, 1361, 1425, 1490, 1757, 1791,
      2013]),
    ([624, 623, 625], 0.02, 2 ** 40 + 7,
     [118, 151, 165, 201, 243, 309, 321, 493, 545, 546, 586, 601, 611, 735, 748, 765, 849, 881, 925, 1071,
      1113, 1123, 1148, 1180, 1235, 1312, 1340, 1365, 1401, 1444, 1526, 1563, 1603, 1674, 1678, 1708, 1779]),
]
CPYTHON_TAKESAMPLE = [
    ([250, 250, 250, 250], 6, 42, [646, 533, 479, 991, 705, 319]),
    ([40000, 40000], 12, 6, [35818, 44499, 38713, 65870, 12098, 30608, 29487, 57706, 18963, 59044, 14022, 7334]),
    ([333, 333, 334], 5, 1700000000, [210, 862, 94, 524, 953]),
]


@pytest.mark.parametrize("sizes,fraction,seed,want", CPYTHON_PICKS)
def test_bernoulli_pass_pinned_to_cpython_literals(sizes, fraction, seed, want):
    import random
    from kmeans_amd import sampling
    r = random.Random(12345)
    assert [r.random() for _ in range(3)] == [0.41661987254534116, 0.010169169457068361, 0.8252065092537432]
    assert sampling._bernoulli_pass_py(sizes, fraction, seed) == want
    bases = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    got = np.concatenate([sampling._partition_picks(p, int(bases[p]), sizes[p], fraction, seed)
                          for p in range(len(sizes)) if sizes[p] > 0])
    assert got.tolist() == want


@pytest.mark.parametrize("sizes,num,seed,want", CPYTHON_TAKESAMPLE)
def test_take_sample_pinned_to_cpython_literals(sizes, num, seed, want):
    from kmeans_amd import sampling
    assert sampling.take_sample(sizes, num, seed) == want
    assert orc.take_sample_indices(sizes, num, seed) == want


def test_vectorised_sampler_equals_python_sampler():
    from kmeans_amd import sampling
    sizes = [70001, 30000]
    for seed in (0, 1, 42, 99991):
        frac = sampling._fraction(50, sum(sizes))
        assert sampling._bernoulli_pass(sizes, frac, seed) == sampling._bernoulli_pass_py(sizes, frac, seed)


# ----------------------------------------------------------------- placement
class FakeComm:
    def __init__(self, rank, world):
        self.rank, self.world = rank, world


def test_placement_partitions_and_order():
    ka = _ka()
    from kmeans_amd.dataset import place
    X = np.arange(1000 * 3, dtype=np.float64).reshape(1000, 3)
    rdd = ka.LocalContext().parallelize(X, 5)
    pls = [place(rdd, FakeComm(r, 2)) for r in range(2)]
    assert pls[0].global_sizes == [200] * 5
    # balanced to one row across partition boundaries (rank 1 starts inside
    # partition 2); the takeSample layout stays the 5 partitions
    assert [p.n_local for p in pls] == [500, 500]
    np.testing.assert_array_equal(np.concatenate([p.local_rows for p in pls]), X)
    assert pls[1].row0 == 500 and pls[1].global_sizes == [200] * 5
    # the reference's own inputs have 1-4 partitions (kmeans_spark.py:418,
    # 561-568): 8 ranks over a 4-partition RDD leave no rank idle
    r4 = ka.LocalContext().parallelize(X, 4)
    p8 = [place(r4, FakeComm(r, 8)) for r in range(8)]
    assert [p.n_local for p in p8] == [125] * 8
    np.testing.assert_array_equal(np.concatenate([p.local_rows for p in p8]), X)
    # uneven partitions (one empty) and more ranks than rows in a partition
    r5 = ka.LocalRDD([X[:7], X[7:7], X[7:300], X[300:]])
    p3 = [place(r5, FakeComm(r, 3)) for r in range(3)]
    assert [p.n_local for p in p3] == [333, 333, 334]
    np.testing.assert_array_equal(np.concatenate([p.local_rows for p in p3]), X)
    # a bare array is one takeSample partition, cut into row blocks per rank
    pa = [place(X, FakeComm(r, 3)) for r in range(3)]
    assert pa[0].global_sizes == [1000]
    np.testing.assert_array_equal(np.concatenate([p.local_rows for p in pa]), X)
    # device blobs: rows split over the ranks; the takeSample layout is the
    # dataset's own partitioning, the same for any number of ranks
    pb = place(ka.DeviceBlobs(n=10, d=4, n_centers=2, partitions=4), FakeComm(1, 3))
    assert (pb.row0, pb.n_local, pb.global_sizes) == (3, 3, [2, 3, 2, 3])
    assert place(ka.DeviceBlobs(n=10, d=4, n_centers=2, partitions=4), FakeComm(0, 1)).global_sizes == [2, 3, 2, 3]


def test_parallelize_slices_like_pyspark():
    ka = _ka()
    rdd = ka.LocalContext().parallelize(list(range(10)), 3)
    assert [len(p) for p in rdd._parts] == [3, 3, 4]
    assert rdd.collect() == list(range(10))
    assert rdd.getNumPartitions() == 3


def test_constructor_validation_messages():
    ka = _ka()
    for kw, msg in [({"k": 0}, "k must be positive, got 0"), ({"max_iter": 0}, "max_iter must be positive, got 0"),
                    ({"tolerance": 0}, "tolerance must be positive, got 0"),
                    ({"k": -2}, "k must be positive, got -2")]:
        with pytest.raises(ValueError, match=re.escape(msg)):
            ka.KMeans(**kw)
    km = ka.KMeans(5, 10, 1e-3, 7, True)  # positional order of the reference (L37-38)
    assert (km.k, km.max_iter, km.tolerance, km.seed, km.compute_sse) == (5, 10, 1e-3, 7, True)
    assert km.centroids is None and km.sse_history == [] and km.iterations_run == 0


# ----------------------------------------------- driver through the CPU engine
@pytest.fixture
def cpu_engine():
    ka = _ka()
    import cpu_engine as ce
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(ce.factory)
    yield
    ka.KMeans._engine_factory = old


def _fit(g, inject=True):
    ka = _ka()
    init = g["init"]

    class Pinned(ka.KMeans):
        def _initialize_centroids(self, run):
            return init.copy() if inject else super()._initialize_centroids(run)

        def _empty_seed(self):
            return int(g["time_seed"])

    sc = ka.LocalContext()
    rdd = sc.parallelize(g["X"], int(g["slices"]))
    km = Pinned(k=int(g["k"]), max_iter=int(g["max_iter"]), tolerance=float(g["tol"]), seed=int(g["seed"]),
                compute_sse=bool(g["sse"]))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(rdd, sc)
    return km, buf.getvalue(), np.array(km.predict(rdd, sc).collect())


def test_init_errors_match_reference(cpu_engine):
    # kmeans_spark.py:72-80: takeSample returns [] for an empty RDD and fewer
    # than k rows for a small one; a NaN / Inf among the sampled rows raises
    ka = _ka()
    sc = ka.LocalContext()
    with pytest.raises(ValueError, match=re.escape("Not enough data points (0) to initialize 4 clusters")):
        ka.KMeans(k=4).fit(sc.parallelize(np.zeros((0, 3)), 2), sc)
    with pytest.raises(ValueError, match=re.escape("Not enough data points (0) to initialize 3 clusters")):
        ka.KMeans(k=3).fit(sc.parallelize([], 1), sc)
    with pytest.raises(ValueError, match=re.escape("Not enough data points (5) to initialize 6 clusters")):
        ka.KMeans(k=6).fit(sc.parallelize(np.arange(10.0).reshape(5, 2), 2), sc)
    X = np.random.default_rng(0).normal(size=(40, 3))
    X[:, 1] = np.nan  # every row non-finite: any takeSample pick carries a NaN
    with pytest.raises(ValueError, match=re.escape("Data contains NaN or Inf values")):
        ka.KMeans(k=3).fit(sc.parallelize(X, 4), sc)
    X[:, 1] = np.inf
    with pytest.raises(ValueError, match=re.escape("Data contains NaN or Inf values")):
        ka.KMeans(k=3).fit(sc.parallelize(X, 4), sc)


def test_predict_on_empty_dataset_is_empty(cpu_engine):
    # predict is a lazy map over the rows (kmeans_spark.py:343-350): no rows, no labels
    ka = _ka()
    sc = ka.LocalContext()
    X = np.random.default_rng(1).normal(size=(30, 2))
    km = ka.KMeans(k=2, max_iter=3)
    with contextlib.redirect_stdout(io.StringIO()):
        km.fit(sc.parallelize(X, 2), sc)
    out = km.predict(sc.parallelize(np.zeros((0, 2)), 1), sc)
    assert out.collect() == [] and out.count() == 0


@pytest.mark.parametrize("name", ["test_a", "test_d", "empty", "ties", "test_c", "tight", "tight_wide", "c5_poor"])
def test_driver_reproduces_reference_with_cpu_engine(golden, cpu_engine, name):
    from test_gpu_parity import assert_logs_match
    g = golden(name)
    km, out, labels = _fit(g, inject=(name in INJECTED))
    np.testing.assert_allclose(km.centroids, g["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(km.sse_history, g["sse_history"], rtol=1e-9)
    assert_logs_match(out, g["stdout"])
    np.testing.assert_array_equal(labels, g["labels"])


@pytest.mark.parametrize("name", ["f32_test_a", "f32_c1", "f32_c3_small", "f32_empty"])
def test_float32_rows_cpu_engine_vs_reference_float32(golden, cpu_engine, name):
    # host logic with a float32 RDD (centroid dtype, logs, SSE history)
    # through the CPU engine, against the reference's float32 run
    from conftest import check_float32_run
    ka = _ka()
    g = golden(name)
    init = g["init"]

    class Pinned(ka.KMeans):
        def _initialize_centroids(self, run):
            return init.copy()

        def _empty_seed(self):
            return int(g["time_seed"])

    sc = ka.LocalContext()
    rdd = sc.parallelize(g["X"].astype(np.float32), int(g["slices"]))
    km = Pinned(k=int(g["k"]), max_iter=int(g["max_iter"]), tolerance=float(g["tol"]), seed=int(g["seed"]),
                compute_sse=bool(g["sse"]))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(rdd, sc)
    labels = np.array(km.predict(rdd, sc).collect())
    check_float32_run(g, km.centroids, km.sse_history, labels, buf.getvalue())


def test_failure_inside_a_batch_closes_it():
    # an error between km_batch_begin and km_batch_end (here: the third
    # assign of a batch) must still close the batch, or the device gate stays
    # up and every later launch on the context is a silent no-op
    ka = _ka()
    import cpu_engine as ce

    class Boom(RuntimeError):
        pass

    engines = []

    class Flaky(ce.OracleEngine):
        calls = 0

        def assign_stats(self):
            Flaky.calls += 1
            if Flaky.calls == 3:
                raise Boom("injected failure")
            return super().assign_stats()

        def batch_end(self, m):
            self.closed = getattr(self, "closed", 0) + 1
            return super().batch_end(m)

    def factory(comm):
        engines.append(Flaky(comm))
        return engines[-1]

    class K(ka.KMeans):
        _engine_factory = staticmethod(factory)

    rng = np.random.default_rng(5)
    X = rng.standard_normal((400, 3))
    km = K(k=3, max_iter=10, seed=1)
    km.verbose = False
    with pytest.raises(Boom):
        km.fit(X)
    eng = engines[-1]
    assert eng.closed == 1 and not eng._batching
    # the same model fits again afterwards (a new context, no open batch)
    Flaky.calls = 10
    km.fit(X)
    assert km.centroids.shape == (3, 3) and np.all(np.isfinite(km.centroids))


def test_predict_reuses_fit_rows_only_for_the_same_object(cpu_engine):
    # predict reuses the runner (rows resident from fit) only for the very
    # object fit saw, compared with `is` through a weak reference; a new
    # dataset, even one allocated where the old one lived, gets its own rows
    import gc
    ka = _ka()
    rng = np.random.default_rng(0)
    A = rng.standard_normal((600, 4)) + np.repeat(np.eye(4) * 20, 150, axis=0)
    km = ka.KMeans(k=4, max_iter=5, seed=1)
    km.verbose = False
    km.fit(A)
    fitted = km._runner
    lab_a = np.asarray(km.predict(A).collect())
    assert km._runner is fitted
    B = -A[::-1].copy()
    lab_b = np.asarray(km.predict(B).collect())
    want_b = np.argmin(((B[:, None, :] - km.centroids[None]) ** 2).sum(-1), axis=1)
    np.testing.assert_array_equal(lab_b, want_b)
    assert not np.array_equal(lab_a, lab_b[::-1]) or np.array_equal(want_b, lab_a[::-1])
    # a dead referent matches nothing, whatever id() a new object gets
    from kmeans_amd.kmeans import _deref, _ref_to
    tmp = np.zeros(3)
    km._runner_src = _ref_to(tmp)
    del tmp
    gc.collect()
    assert _deref(km._runner_src) is None
    # a type without weak references (e.g. a list) is held by the model instead
    L = [1, 2]
    assert _deref(_ref_to(L)) is L


def test_speedup_table_from_bench_lines(tmp_path):
    # test_e counterpart (kmeans_spark.py:543-621): bench lines of 1/2/4/8
    # GPUs -> the reference's timing table and the ideal-vs-actual figure
    import importlib.util
    spec = importlib.util.spec_from_file_location("speedup", os.path.join(ROOT, "scripts", "speedup.py"))
    sp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sp)
    lines = [{"metric": "m", "value": v, "unit": "Lloyd it/s", "n_gpus": n, "ms_per_step": 1e3 / v}
             for n, v in [(1, 88.0), (2, 170.0), (4, 330.0), (8, 600.0)]]
    f1 = tmp_path / "n1_2.json"
    f1.write_text("\n".join(json.dumps(o) for o in lines[:2]))
    f2 = tmp_path / "scale.json"   # a driver-style wrapper holding the rest
    f2.write_text(json.dumps({"runs": [{"n": 4, "parsed": lines[2]}, {"n": 8, "tail": json.dumps(lines[3]) + "\n"}]}))
    rows = sp.speedup_table(sp.load_runs([str(f1), str(f2)]))
    assert [r[0] for r in rows] == [1, 2, 4, 8]
    np.testing.assert_allclose([r[2] for r in rows], [1.0, 170 / 88, 330 / 88, 600 / 88])
    np.testing.assert_allclose([r[3] for r in rows], [1.0, 170 / 176, 330 / 352, 600 / 704])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sp.print_table(rows)
        png = sp.plot(rows, str(tmp_path / "speedup_graph.png"), "Number of GPUs")
    assert "GPUs:  8 | Time:   0.0017s | Speedup: 6.8182x" in buf.getvalue()
    if png:
        assert os.path.getsize(png) > 1000


# ------------------------------------------------------ multi-rank over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, name, q, device_repair=False):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmeans_amd as ka
        import cpu_engine as ce
        from conftest import load_golden
        ka.KMeans._engine_factory = staticmethod(ce.factory_device_repair if device_repair else ce.factory)
        g = load_golden(name)
        km, out, labels = _fit(g, inject=(name in INJECTED))
        run = km._runner
        pred = km.predict(g["X"])
        views = {"root": np.asarray(labels), "everywhere": np.asarray(pred.collect(everywhere=True)),
                 "local": pred.local().copy(), "row0": run.pl.row0, "count": pred.count()}
        q.put((rank, km.centroids, km.sse_history, views, out, (run.device_repair, run.device_repairs)))
    finally:
        dist.destroy_process_group()


def _run_ranks(world, name, device_repair=False):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, name, q, device_repair)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("name", ["test_a", "test_d", "empty"])
def test_two_ranks_gloo_match_single_rank(golden, name):
    g = golden(name)
    res = _run_ranks(2, name)
    for rank, C, sse, v, out, _ in res:
        np.testing.assert_allclose(C, g["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, g["sse_history"], rtol=1e-9)
        # collect(): the driver (rank 0) gets every label, the others none;
        # everywhere=True: every rank; local(): the rank's own row block
        np.testing.assert_array_equal(v["root"], g["labels"] if rank == 0 else g["labels"][:0])
        np.testing.assert_array_equal(v["everywhere"], g["labels"])
        np.testing.assert_array_equal(v["local"], g["labels"][v["row0"]:v["row0"] + len(v["local"])])
        assert v["count"] == len(g["labels"])
    assert sum(len(r[3]["local"]) for r in res) == len(g["labels"])
    assert res[0][4] and not res[1][4]  # only rank 0 logs, like the single driver


@pytest.mark.parametrize("world,name", [(4, "c5_poor"), (4, "empty"), (1, "c5_poor")])
def test_device_repair_protocol_over_gloo_ranks(golden, world, name):
    # the device repair's host protocol (layout mode 2 with world > 1: the same
    # seeds on every rank, every rank picks the same takeSample rows, the
    # owners' rows meet in one all-reduce, the apply finishes the iteration;
    # mode 1 on one rank) with the CPU engine standing in for the device, on
    # the reference's own goldens (~509 empties at c5_poor's first update)
    from test_gpu_parity import assert_logs_match
    g = golden(name)
    res = _run_ranks(world, name, device_repair=True)
    for rank, C, sse, v, out, (mode, repairs) in res:
        assert mode == (2 if world > 1 else 1) and repairs >= 1, (mode, repairs)
        np.testing.assert_allclose(C, g["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, g["sse_history"], rtol=1e-9)
        np.testing.assert_array_equal(v["everywhere"], g["labels"])
        np.testing.assert_array_equal(v["root"], g["labels"] if rank == 0 else g["labels"][:0])
    assert_logs_match(res[0][4], g["stdout"])
    assert all(not r[4] for r in res[1:])


class SparkLikeRDD:
    """Duck-typed PySpark RDD: mapPartitions / mapPartitionsWithIndex run "on
    the executors" (here: over the partition lists) and collect() returns
    what reaches the calling rank; it records the partitions whose ROWS came
    back (count triples are not rows)."""

    def __init__(self, parts, log=None, fn=None):
        self._parts, self.log, self._fn = parts, (log if log is not None else []), fn

    def getNumPartitions(self):
        return len(self._parts)

    def cache(self):
        return self

    def mapPartitions(self, f):
        return SparkLikeRDD(self._parts, self.log, lambda i, it: f(it))

    def mapPartitionsWithIndex(self, f):
        return SparkLikeRDD(self._parts, self.log, f)

    def collect(self):
        out = []
        for i, p in enumerate(self._parts):
            got = list(self._fn(i, iter(p)))
            if any(isinstance(x, np.ndarray) for x in got):
                self.log.append((i, len(got)))
            out.extend(got)
        return out


def _shard_rank_main(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import kmeans_amd as ka
        import cpu_engine as ce
        from conftest import load_golden
        ka.KMeans._engine_factory = staticmethod(ce.factory)
        g = load_golden("test_d")
        X, P = g["X"], int(g["slices"])
        n = len(X)
        parts = [list(X[(i * n) // P:((i + 1) * n) // P]) for i in range(P)]
        res = {}
        # a PySpark-like RDD: rows reach this rank only from its partitions
        rdd = SparkLikeRDD(parts)
        km = ka.KMeans(k=int(g["k"]), max_iter=int(g["max_iter"]), tolerance=float(g["tol"]), seed=int(g["seed"]),
                       compute_sse=bool(g["sse"]))
        km.verbose = False
        km.fit(rdd)
        res["spark"] = (km.centroids, km.sse_history, sorted(set(e for e in rdd.log if e[1])))

        # the package's LocalRDD: only this rank's partitions are materialised
        touched = []

        class Tracked(ka.LocalRDD):
            def partition_array(self, i):
                touched.append(i)
                return super().partition_array(i)

        lrdd = Tracked([np.asarray(p) for p in parts])
        km2 = ka.KMeans(k=int(g["k"]), max_iter=int(g["max_iter"]), tolerance=float(g["tol"]), seed=int(g["seed"]),
                        compute_sse=bool(g["sse"]))
        km2.verbose = False
        km2.fit(lrdd)
        res["local"] = (km2.centroids, km2.sse_history, sorted(set(touched)))
        q.put((rank, P, [len(p) for p in parts], res))
    finally:
        dist.destroy_process_group()


def test_two_ranks_ingest_only_their_own_partitions(golden):
    # sharded ingestion (kmeans_spark.py:256 rdd.cache() -> HBM): rank r
    # materialises only global rows [r N/W, (r+1) N/W); the fit is unchanged
    import torch.multiprocessing as mp
    g = golden("test_d")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    from kmeans_amd.dataset import _segments, rank_rows
    for rank, P, sizes, r in res:
        segs = _segments(sizes, *rank_rows(sum(sizes), 2, rank))
        own = [i for i, _, _ in segs]
        C, sse, log = r["spark"]
        # exactly this rank's rows came back: its row block, cut at the
        # partition boundaries it spans
        assert log == [(i, hi - lo) for i, lo, hi in segs], (rank, log)
        np.testing.assert_allclose(C, g["centroids"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sse, g["sse_history"], rtol=1e-9)
        C2, sse2, touched = r["local"]
        assert touched == own, (rank, touched)
        np.testing.assert_allclose(C2, g["centroids"], rtol=1e-9, atol=1e-9)


def _sample_rank_main(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmeans_amd import sampling
        from kmeans_amd.comm import Communicator
        comm = Communicator()
        sizes = [40000, 30000, 0, 50001, 25000]
        q.put((rank, sampling.take_sample(sizes, 37, 2024, comm), sampling.take_sample(sizes, 5, 7, comm)))
    finally:
        dist.destroy_process_group()


def test_take_sample_split_over_ranks_is_identical():
    # partitions are independent streams: splitting them over ranks (and host
    # threads) must not change takeSample's answer (kmeans_spark.py:72, :196)
    import torch.multiprocessing as mp
    from kmeans_amd import sampling
    sizes = [40000, 30000, 0, 50001, 25000]
    want = (sampling.take_sample(sizes, 37, 2024), sampling.take_sample(sizes, 5, 7))
    assert want[0] == orc.take_sample_indices(sizes, 37, 2024)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sample_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, a, b in res:
        assert (a, b) == want


def test_graft_build_entry_matches_the_library_abi():
    # __graft_entry__.build() (the driver's build check) runs make (a no-op when
    # the library is current) and checks the loaded library's ABI version
    # against the package constant; a stale pin here once broke it
    import __graft_entry__ as g
    g.build()


# ------------------------------------------- distributed device repair (order)
def test_distributed_device_repair_enqueue_order():
    # layout mode 2 (rows spread over ranks): per iteration the runner must
    # enqueue assign -> stats all-reduce -> update (with ONE seed shared by the
    # ranks, broadcast only while the repair is armed) -> the repair rows'
    # all-reduce -> km_repair_apply_async, all without a host sync; a batch
    # that is not armed enqueues no repair collective (kmeans_spark.py:191-204)
    from kmeans_amd import _lib
    from kmeans_amd.dataset import Placement
    from kmeans_amd.kmeans import LloydRunner
    calls = []

    class Dist:
        @staticmethod
        def all_reduce(t, async_op=False):
            calls.append("allreduce_rows")

    class Comm:
        rank, world, dist = 0, 2, Dist

        def broadcast_obj(self, obj, src=0):
            calls.append(("bcast", obj))
            return [777 + i for i in range(len(obj))]  # one seed per iteration of the batch

        def allreduce_stats(self, eng):
            calls.append("allreduce_stats")

    class Eng:
        distributed = True
        armed, waiting = True, False

        def load_host(self, rows):
            pass

        def set_layout(self, sizes, row0, mode):
            calls.append(("layout", list(sizes), row0, mode))

        def repair_bind(self):
            calls.append("bind")

        def repair_state(self):
            return self.armed, self.waiting

        def batch_begin(self):
            calls.append("begin")

        def assign_stats(self):
            calls.append("assign")

        def update_async(self, tol, seed):
            calls.append(("update", seed))
            self.waiting = self.armed

        def repair_exchange(self, fn):
            fn(None, async_op=True)
            calls.append("apply")
            self.waiting = False

        def batch_end(self, m):
            st = _lib.KmStatus()
            st.ran = 1
            st.max_shift = 1.0
            self.armed = False          # a batch without empties disarms
            return [(st, np.ones(2, dtype=np.int64))] * m

        def commit(self):
            calls.append("commit")

    class Model:
        tolerance, compute_sse = 1e-300, False

        @staticmethod
        def _empty_seed():
            return 123

    pl = Placement(global_sizes=[6, 6], local_rows=np.zeros((6, 3)), row0=6, n_local=6, n_global=12, d=3,
                   dtype=np.float64)
    run = LloydRunner(Eng(), pl, Comm(), 2)
    run.load()
    assert run.device_repair == 2 and calls[0] == ("layout", [6, 6], 6, 2)
    run.batch = 2
    run.run(Model(), None, 4)
    it = [["assign", "allreduce_stats", ("update", 777 + i), "allreduce_rows", "apply"] for i in range(2)]
    assert calls[1:] == ["bind", ("bcast", [123, 123]), "begin"] + it[0] + it[1] + ["commit", "bind", "begin"] + \
        ["assign", "allreduce_stats", ("update", 123)] * 2 + ["commit"], calls


def test_fullscan_lockstep_updates_minima_with_selects():
    # The lockstep chunk pass of k_fullscan evaluates two queued points per
    # staged centroid value.  Written as branches
    #   if (have[g + 1] && np_better(vb, best[g + 1], ...)) { best[g + 1] = vb; ... }
    # the lane minima of the second point stay at their first-chunk values on
    # this toolchain (printf trace: per-chunk norms right, minima never
    # updated; branch exp/fullscan-lockstep-branchy), the
    # cause of the round-2 lockstep variant's wrong labels.  The GPU test
    # test_gpu_parity.py::test_one_step_vs_oracle[50000-64-256-256] catches
    # it at run time; this lint keeps the select form in the source.
    src = open(os.path.join(ROOT, "assignment--2-group7-distributed-k-means_amd", "csrc", "km_kernels.hip")).read()
    body = src[src.index("void k_fullscan("):]
    body = body[:body.index("hipError_t launch_resolve(")]
    body = re.sub(r"//[^\n]*", "", body)  # code only
    assert "np_pw2<2>(" in body
    assert "best[g + 1] = ub ? vb : best[g + 1];" in body
    assert re.search(r"if \(have\[g \+ 1\] && np_better", body) is None
    # the same defect class everywhere (the structurized
    # branch's copy for the not-taken lanes runs for every lane that reached
    # the comparison): no running minimum or argmin shuffle is updated under
    # an if in any kernel
    code = re.sub(r"//[^\n]*", "", src)
    assert re.search(r"if \([^;{]*np_better\(", code) is None
    assert re.search(r"if \(take\)", code) is None
