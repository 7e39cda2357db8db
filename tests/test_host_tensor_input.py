"""Torch tensors as the dataset of ``fit`` / ``predict``: the host side.

A CPU tensor takes the ndarray's route (``dataset.tensor_to_host``), so these
tests run the product's placement and driver through the injected CPU engine
of ``tests/cpu_engine.py`` and compare with the ndarray route on the same
values.  The GPU route (``km_load_device``) is ``tests/test_gpu_tensor_input.py``."""
import contextlib
import ctypes
import io
import os
import re
import socket

import numpy as np
import pytest
import torch

from conftest import ROOT

FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]


def _ka():
    import kmeans_amd
    return kmeans_amd


@pytest.fixture
def cpu_engine():
    ka = _ka()
    import cpu_engine as ce
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(ce.factory)
    yield ce
    ka.KMeans._engine_factory = old


def _blobs(seed=5, n=600, d=5, c=4, box=50.0):
    """Well-separated blobs whose values bfloat16 and float16 hold exactly
    (small integers), so every dtype carries the same rows."""
    rng = np.random.default_rng(seed)
    centers = np.round(rng.uniform(-box, box, (c, d)))
    lab = rng.integers(0, c, n)
    return (centers[lab] + rng.integers(-3, 4, (n, d))).astype(np.float64)


def _fit(X, **kw):
    ka = _ka()
    km = ka.KMeans(k=4, max_iter=8, tolerance=1e-9, seed=3, compute_sse=True)
    km._empty_seed = lambda: 0
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(X, **kw)
        labels = np.asarray(km.predict(X).collect())
    return km, labels, buf.getvalue()


@pytest.mark.parametrize("dtype", FLOATS, ids=lambda t: str(t).split(".")[1])
def test_cpu_tensor_equals_the_ndarray_route(cpu_engine, dtype):
    X = _blobs()
    t = torch.from_numpy(X).to(dtype)
    assert torch.equal(t.to(torch.float64), torch.from_numpy(X))   # the rows are exact in every dtype
    want_dtype = np.float64 if dtype == torch.float64 else np.float32
    a, la, out_a = _fit(t)
    b, lb, out_b = _fit(X.astype(want_dtype))
    assert a.centroids.dtype == want_dtype
    np.testing.assert_array_equal(a.centroids, b.centroids)
    assert a.sse_history == b.sse_history and len(a.sse_history) > 0
    assert out_a == out_b
    np.testing.assert_array_equal(la, lb)
    assert a._runner.pl.device_rows is None and a._runner.pl.local_rows is not None


def test_integer_and_bool_tensors_go_through_float64(cpu_engine):
    X = _blobs()
    a, la, _ = _fit(torch.from_numpy(X).to(torch.int32))
    b, lb, _ = _fit(X.astype(np.int32))
    assert a.centroids.dtype == np.float64
    np.testing.assert_array_equal(a.centroids, b.centroids)
    np.testing.assert_array_equal(la, lb)
    from kmeans_amd import dataset
    assert dataset.tensor_to_host(torch.tensor([[True, False]])).dtype == np.float64


def test_layout_of_a_tensor():
    from kmeans_amd import dataset
    for dtype, want in [(torch.float16, np.float32), (torch.bfloat16, np.float32), (torch.float32, np.float32),
                        (torch.float64, np.float64)]:
        sizes, d, dt = dataset._layout(torch.zeros(7, 3, dtype=dtype))
        assert sizes == [7] and d == 3 and np.dtype(dt) == np.dtype(want)
    for bad in (torch.zeros(5), torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError, match=r"input tensor must be 2-D \[n\]\[d\]"):
            dataset._layout(bad)
    with pytest.raises(TypeError, match="unsupported dataset type"):
        dataset._layout(torch.zeros(4, 2, dtype=torch.complex64))
    # the unsupported-type message names the tensor among the accepted inputs
    with pytest.raises(TypeError, match="torch.Tensor"):
        dataset._layout(object())


def test_placement_of_a_cpu_tensor_is_the_ndarrays(cpu_engine):
    from kmeans_amd import dataset
    from kmeans_amd.comm import Communicator
    X = _blobs(n=11)
    comm = Communicator()
    a = dataset.place(torch.from_numpy(X).to(torch.bfloat16), comm)
    b = dataset.place(X.astype(np.float32), comm)
    assert (a.global_sizes, a.row0, a.n_local, a.n_global, a.d) == (b.global_sizes, b.row0, b.n_local, b.n_global, b.d)
    assert a.dtype == b.dtype == np.float32 and a.device_rows is None and a.blobs is None
    assert a.local_rows.dtype == np.float32                       # bfloat16 has no NumPy dtype: widened
    np.testing.assert_array_equal(a.local_rows, b.local_rows)


def test_empty_tensor(cpu_engine):
    ka = _ka()
    km = ka.KMeans(k=3)
    km.verbose = False
    with pytest.raises(ValueError, match=r"Not enough data points \(0\) to initialize 3 clusters"):
        km.fit(torch.zeros(0, 4))
    fitted, _, _ = _fit(_blobs())
    out = fitted.predict(torch.zeros(0, 5))
    assert isinstance(out, ka.kmeans.LabelsRDD) and out.collect() == [] and out.count() == 0
    assert out.to_tensor().dtype == torch.int32 and out.to_tensor().numel() == 0


def test_complex_tensor_is_refused(cpu_engine):
    km = _ka().KMeans(k=2)
    with pytest.raises(TypeError):
        km.fit(torch.zeros(8, 2, dtype=torch.complex64))


def test_labels_of_a_host_input_come_back_as_a_cpu_tensor(cpu_engine):
    X = _blobs()
    km, labels, _ = _fit(X)
    for inp in (X, torch.from_numpy(X)):
        lt = km.predict(inp).to_tensor()
        assert lt.dtype == torch.int32 and lt.device.type == "cpu"
        np.testing.assert_array_equal(lt.numpy(), labels)


def test_predict_reuses_the_fitted_tensor(cpu_engine):
    t = torch.from_numpy(_blobs()).float()
    km, _, _ = _fit(t)
    run = km._runner
    km.predict(t)
    assert km._runner is run and km._runner_src() is t


def test_sample_weight_as_a_tensor():
    ka = _ka()
    import weighted_ref as wr
    old = ka.KMeans._engine_factory
    ka.KMeans._engine_factory = staticmethod(wr.factory)
    try:
        X = _blobs().astype(np.float32)
        w = np.random.default_rng(0).uniform(0.5, 4.0, len(X))
        a, la, out_a = _fit(X, sample_weight=torch.from_numpy(w))
        b, lb, out_b = _fit(X, sample_weight=w)
        c, _, _ = _fit(torch.from_numpy(X), sample_weight=torch.from_numpy(w).float())
        d, _, _ = _fit(X, sample_weight=w.astype(np.float32))
        e, _, _ = _fit(X)
    finally:
        ka.KMeans._engine_factory = old
    np.testing.assert_array_equal(a.centroids, b.centroids)
    assert a.sse_history == b.sse_history and out_a == out_b
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(c.centroids, d.centroids)
    assert not np.array_equal(a.centroids, e.centroids)            # the weights did count


def test_lib_binds_the_two_new_symbols():
    from kmeans_amd import _lib
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # km_load_device(ctx, int64 row0, const void* rows, int64 nrows, int64 stride, int32 dtype)
    assert _lib.SIGNATURES["km_load_device"] == [P, I64, P, I64, I64, I32]
    # km_labels_device(ctx, int32* dev_out): a device address, passed as an integer
    assert _lib.SIGNATURES["km_labels_device"] == [P, P]
    assert (_lib.KM_DT_F32, _lib.KM_DT_F64, _lib.KM_DT_F16, _lib.KM_DT_BF16) == (0, 1, 2, 3)
    header = open(_lib.HEADER).read()
    for line in ("#define KM_DT_F32 0", "#define KM_DT_F64 1", "#define KM_DT_F16 2", "#define KM_DT_BF16 3",
                 "#define KM_ABI_VERSION 6"):
        assert line in header
    lib = _lib.load()
    for name in ("km_load_device", "km_labels_device"):
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype == ctypes.c_int


def test_abi_version_is_still_6():
    from kmeans_amd import _lib
    assert _lib.KM_ABI_VERSION == 6 and _lib.load().km_abi_version() == 6


# ------------------------------------------------------ two ranks over gloo
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
        import cpu_engine as ce
        ka.KMeans._engine_factory = staticmethod(ce.factory)
        t = torch.from_numpy(_blobs(n=601)).to(torch.bfloat16)
        km, _, log = _fit(t)
        local = km.predict(t).local()
        q.put((rank, km.centroids, list(km.sse_history), km._runner.pl.row0, km._runner.pl.n_local, local, log))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_with_a_cpu_tensor_equal_one(cpu_engine):
    import torch.multiprocessing as mp
    X = _blobs(n=601)
    one, labels, log1 = _fit(torch.from_numpy(X).to(torch.bfloat16))
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
    assert [r[3] for r in res] == [0, 300] and [r[4] for r in res] == [300, 301]
    for rank, cent, sse, _, _, _, log in res:
        # the rows are small integers: the two ranks' partial sums add exactly
        np.testing.assert_array_equal(cent, one.centroids)
        # the SSE adds 601 float64 residuals in another order: n * 2^-53 relative
        np.testing.assert_allclose(sse, one.sse_history, rtol=601 * 2.0 ** -53)
        strip = re.compile(r"SSE = [0-9.]+")
        assert strip.sub("SSE", log) == (strip.sub("SSE", log1) if rank == 0 else "")
    np.testing.assert_array_equal(np.concatenate([r[5] for r in res]), labels)
