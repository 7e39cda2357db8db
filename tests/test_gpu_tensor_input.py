"""GPU-resident torch tensors as the dataset (``km_load_device``, k_ingest of
km_ingest.hip; ``km_labels_device``): the device route must leave in HBM
exactly what the host route leaves for the same float32 values.

1. stored rows bit for bit, every dtype x row width x row count; with them the
   column sums and one labels-only assignment against an engine loaded by
   ``load_host`` (the data maximum, the row norms and the zero padding columns
   all feed the distances);
2. the float64 -> float32 rounding at its edges, and the special values of
   every dtype;
3. strided, offset, misaligned and transposed views, and a view that ends at
   the last element of its buffer;
4. ``KMeans.fit`` / ``predict`` on a tensor against the ndarray route, one
   geometry per assignment path;
5. the labels stay on the device;
6. every misuse of the two entry points is a return code.
"""
import contextlib
import ctypes
import io
import re

import numpy as np
import pytest
import torch

from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
_name = lambda t: str(t).split(".")[1]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def engines():
    """Two engines for the whole module (a load replaces the previous one):
    [0] takes the device route, [1] the host route."""
    from kmeans_amd.engine import HipEngine
    pair = (HipEngine(0), HipEngine(0))
    yield pair
    for e in pair:
        e.close()


def _values(n, d, dtype, seed):
    """Rows on the CPU in ``dtype``: normal values of mixed magnitude, with a
    -0.0 and a +0.0 planted (the sign of zero must survive)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) * np.exp(rng.uniform(-3, 3, (n, d)))
    x.flat[rng.integers(0, n * d)] = -0.0
    x.flat[rng.integers(0, n * d)] = 0.0
    return torch.from_numpy(x).to(dtype)


def _f32(t):
    """What the host route stores for the tensor's values: float32, where
    float64 rounds as NumPy rounds it (bfloat16 has no NumPy dtype; widening
    it in torch is exact)."""
    t = t.detach().cpu()
    if t.dtype == torch.float64:
        return t.numpy().astype(np.float32)
    return t.to(torch.float32).numpy()


def _assert_same_bits(got64, want32):
    """``gather_rows`` returns the stored float32 as float64 (exact), so value
    equality with NaNs in the same places and equal sign bits is bit equality
    up to a NaN's payload."""
    want = want32.astype(np.float64)
    assert got64.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got64), np.isnan(want))
    np.testing.assert_array_equal(np.signbit(got64), np.signbit(want))
    np.testing.assert_array_equal(got64, want)


def _stored(eng):
    return eng.gather_rows(np.arange(eng.n))


def _assert_same_sums(a, b, want32):
    """Two ``sum_x()`` of identical row stores.  Not a bit comparison: k_sum_x
    folds its per-wave partial sums with float64 atomics, so the order of the
    additions differs between two engines and between two runs, and a sum of
    float32 values of mixed magnitude and sign is not always exact in float64.
    Each order's sum of the n terms of a column is within (n - 1) 2^-53
    sum|x| of the exact one, so two orders are within twice that.  (The rows
    themselves are compared bit for bit, and the labels cover the data maximum,
    the row norms and the padding.)"""
    w = want32.astype(np.float64)
    bar = 2 * max(len(w) - 1, 0) * 2.0 ** -53 * np.abs(w).sum(axis=0)
    assert a.shape == b.shape == bar.shape
    assert np.all(np.abs(a - b) <= bar), (np.abs(a - b).max(), bar.min())
    # and each within the same bound of NumPy's own (pairwise) sum
    assert np.all(np.abs(a - w.sum(axis=0)) <= bar + 2.0 ** -53 * np.abs(w).sum(axis=0))


# ------------------------------------------------- 1. stored rows, bit for bit
# every padding case of choose_dp (16, 32, 48, 64, 96, 128, 192, 256 and the
# wide rows' multiple of 16), rows whose byte length is and is not a multiple of
# the vector load for each element size; one row, a wave less one, a wave, a
# wave and one, more than one workgroup's worth of groups
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("d", [1, 3, 7, 8, 16, 33, 64, 100, 257])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stored_rows_bit_for_bit(engines, dtype, d, n):
    dev, host = engines
    cpu = _values(n, d, dtype, 7 * n + d)
    want = _f32(cpu)
    t = cpu.to(DEV)
    assert dev.load_device(t) == n and (dev.n, dev.d) == (n, d)
    _assert_same_bits(_stored(dev), want)
    host.load_host(want)
    _assert_same_sums(dev.sum_x(), host.sum_x(), want)
    # centroids between the rows: distances that a wrong norm, data maximum or a
    # non-zero padding column would change
    k = min(3, n)
    C = want[np.linspace(0, n - 1, k).astype(int)].astype(np.float64) * 1.25 + 0.5
    dev.set_centroids(C)
    host.set_centroids(C)
    la, lb = dev.predict(), host.predict()
    np.testing.assert_array_equal(la, lb)
    assert dev.info()["dp"] == host.info()["dp"] and dev.info()["path"] == host.info()["path"]


# ------------------------------------------------- 2. rounding and special values
def test_fp64_rounding_edges(engines):
    dev, _ = engines
    f32 = np.float32
    one, up = f32(1.0), np.nextafter(f32(1.0), f32(2.0))
    upup = np.nextafter(up, f32(2.0))
    half_even = (np.float64(one) + np.float64(up)) / 2      # tie: rounds to 1.0 (even mantissa)
    half_odd = (np.float64(up) + np.float64(upup)) / 2      # tie: rounds up, away from the odd neighbour
    fmax = np.float64(np.finfo(f32).max)
    over = fmax + 2.0 ** 103                                # halfway to 2^128: rounds to inf
    sub = np.float64(np.finfo(f32).smallest_subnormal)
    vals = []
    for h in (half_even, half_odd, -half_even, -half_odd):
        vals += [h, np.nextafter(h, np.inf), np.nextafter(h, -np.inf)]
    vals += [fmax, -fmax, np.nextafter(fmax, np.inf), -np.nextafter(fmax, np.inf), np.nextafter(over, 0.0), over,
             -over, 1e300, -1e300, sub, -sub, sub / 2, np.nextafter(sub / 2, 1.0), -sub / 2, 1.5 * sub, 2.5 * sub,
             sub / 4, 0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, np.finfo(f32).tiny * (1 - 2.0 ** -25)]
    x = np.array(vals, dtype=np.float64)
    for shape in ((len(x), 1), (1, len(x)), (len(x) // 4, 4)):
        rows = x[:shape[0] * shape[1]].reshape(shape)
        with np.errstate(over="ignore", under="ignore"):
            want = rows.astype(f32)
        dev.load_device(torch.from_numpy(rows).to(DEV))
        got = _stored(dev).astype(f32)                      # exact: the stored values are float32
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    # the planted cases are what they are meant to be
    assert f32(half_even) == one and f32(half_odd) == upup
    with np.errstate(over="ignore"):
        assert np.isinf(f32(over)) and np.isfinite(f32(np.nextafter(over, 0.0)))
    assert f32(sub / 2) == 0 and f32(np.nextafter(sub / 2, 1.0)) == f32(sub)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_special_values_of_every_dtype(engines, dtype):
    dev, _ = engines
    fi = torch.finfo(dtype)
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), fi.max, fi.min, fi.tiny, -fi.tiny,
            fi.smallest_normal / 2, fi.smallest_normal / 4, -fi.smallest_normal / 4, fi.eps, 1.0 + fi.eps, -1.0, 65504.0]
    cpu = torch.tensor(vals, dtype=torch.float64).to(dtype).reshape(4, 4)
    with np.errstate(over="ignore", under="ignore"):
        want = _f32(cpu)
    dev.load_device(cpu.to(DEV))
    _assert_same_bits(_stored(dev), want)
    if dtype in (torch.float16, torch.bfloat16):
        # widening is exact: the subnormals of the narrow type arrive unflushed
        assert want.reshape(-1)[9] != 0 and want.reshape(-1)[10] != 0


# ------------------------------------------------------------------- 3. views
VIEW_N, VIEW_D, VIEW_W = 65, 10, 24   # 24 elements: the row stride keeps every dtype's vector alignment


def _views(dtype):
    """name -> (view on the GPU, the same rows on the CPU)."""
    n, d, w = VIEW_N, VIEW_D, VIEW_W
    base = _values(2 * n + 5, w, dtype, 99).to(DEV)
    wide = _values(d, n, dtype, 98).to(DEV)
    stride = d + 3
    flat = _values(1, (n - 1) * stride + d, dtype, 97).reshape(-1).to(DEV)
    out = {
        "columns_0": base[:n, :d],                       # stride > d, aligned base
        "columns_1": base[:n, 1:1 + d],                  # misaligned base: the scalar instance
        "columns_4": base[:n, 4:4 + d],                  # base offset by one whole vector: still aligned
        "rows_5": base[5:5 + n, :d],                     # storage offset
        "every_other_row": base[::2][:n, :d],            # row skipping
        "transposed": wide.t(),                          # column stride != 1: made contiguous first
        "to_the_last_element": flat.as_strided((n, d), (stride, 1)),   # ends where its buffer ends
        "overlapping_rows": flat.as_strided((n, d), (d - 1, 1)),       # row stride < d: made contiguous first
    }
    return {k: (v, v.cpu()) for k, v in out.items()}


@pytest.mark.parametrize("view", ["columns_0", "columns_1", "columns_4", "rows_5", "every_other_row", "transposed",
                                  "to_the_last_element", "overlapping_rows"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_views_equal_their_contiguous_copy(engines, dtype, view):
    dev, other = engines
    v, cpu = _views(dtype)[view]
    assert v.shape == (VIEW_N, VIEW_D)
    if view not in ("transposed", "overlapping_rows"):
        assert not v.is_contiguous() and v.stride(1) == 1
    if view == "to_the_last_element":
        assert v.storage_offset() + (VIEW_N - 1) * v.stride(0) + VIEW_D == v.untyped_storage().nbytes() // v.element_size()
    dev.load_device(v)
    other.load_device(v.contiguous())
    got = _stored(dev)
    _assert_same_bits(got, _f32(cpu))
    assert got.tobytes() == _stored(other).tobytes()
    _assert_same_sums(dev.sum_x(), other.sum_x(), _f32(cpu))


# -------------------------------------------- 4. fit parity through KMeans
# n, d, k, seed, blobs: the small path, k_s1 / the fused kernel, wide rows.
# Blobs with centres uniform in (-40, 40)^d and unit deviation (k = 256 splits
# 32 blobs: with one blob per centroid takeSample leaves blobs unseeded and
# clusters empty out).  The oracle, run on the CPU with these seeds on the
# float32 and on the float16 rows when this test was written, meets no empty
# cluster in any of the 6 iterations; the test asserts it again from the
# product's own log, and the repair's seed is pinned anyway
FIT_CASES = [(5000, 16, 8, 1, 8), (20000, 64, 256, 2, 32), (3000, 300, 16, 3, 16)]
_fit_data = {}


def _fit_rows(n, d, k, seed, blobs):
    if (n, d, k) not in _fit_data:
        rng = np.random.default_rng(seed)
        centers = rng.uniform(-40, 40, (blobs, d))
        _fit_data[(n, d, k)] = (centers[rng.integers(0, blobs, n)] + rng.standard_normal((n, d))).astype(np.float32)
    return _fit_data[(n, d, k)]


def _fit(rows, k, seed):
    import kmeans_amd as ka

    class Pinned(ka.KMeans):
        def _empty_seed(self):
            return 12345

    km = Pinned(k=k, max_iter=6, tolerance=1e-6, seed=seed, compute_sse=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(rows)
        labels = km.predict(rows).collect()
    return km, labels, buf.getvalue()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=_name)
@pytest.mark.parametrize("n,d,k,seed,blobs", FIT_CASES)
def test_fit_on_a_tensor_equals_fit_on_the_array(n, d, k, seed, blobs, dtype):
    t = torch.from_numpy(_fit_rows(n, d, k, seed, blobs)).to(dtype).to(DEV)
    a, la, out_a = _fit(t, k, seed)
    b, lb, out_b = _fit(t.float().cpu().numpy(), k, seed)
    assert a.centroids.dtype == np.float32 and b.centroids.dtype == np.float32
    assert a.centroids.tobytes() == b.centroids.tobytes()
    # The SSE is not bit-reproducible between two identical fits of ONE route:
    # the kernels add the n float64 residuals with atomics, in an order that
    # varies from run to run (measured when this test was written: three host
    # fits of each case differ among themselves by up to 2.1e-15 relative,
    # device against host by up to 2.9e-15).  Each order's sum of n non-negative
    # terms is within (n - 1) 2^-53 relative of the exact sum, so two orders
    # are within twice that of each other; that is the bar (4.4e-12 at n = 20000).
    # The log prints the SSE with 4 decimals: the same bar plus one unit of
    # the last printed digit; everything else in the log is equal text.
    bar = 2 * (n - 1) * 2.0 ** -53
    assert len(a.sse_history) == len(b.sse_history) >= 2
    print("max relative SSE difference", max(abs(x - y) / y for x, y in zip(a.sse_history, b.sse_history)), "bar", bar)
    np.testing.assert_allclose(a.sse_history, b.sse_history, rtol=bar, atol=0)
    num = re.compile(r"SSE = ([0-9.]+)")
    assert num.sub("SSE", out_a) == num.sub("SSE", out_b) and "Iteration 2" in out_a
    for x, y in zip(num.findall(out_a), num.findall(out_b)):
        assert abs(float(x) - float(y)) <= bar * float(y) + 1.0001e-4, (x, y)
    assert "empty cluster" not in out_a
    assert la == lb
    assert a._runner.engine.info()["path"] == b._runner.engine.info()["path"]
    # loaded from HBM, and the view of the caller's tensor was let go after the load
    assert a._runner.from_device and a._runner.pl.device_rows is None and a._runner.pl.local_rows is None
    if dtype == torch.float32 and d == 16:   # the smallest case once more against the oracle itself
        ref = orc.lloyd_fit(t.cpu().numpy().astype(np.float64), k, 6, 1e-6, seed, True, 1)
        assert all(not r["empty"] for r in ref["records"])
        np.testing.assert_allclose(a.centroids, ref["centroids"], rtol=1e-5, atol=1e-5)


def test_float64_tensor_returns_float64_centroids():
    rows = _fit_rows(*FIT_CASES[0])
    a, la, _ = _fit(torch.from_numpy(rows.astype(np.float64) * (1 + 2.0 ** -30)).to(DEV), 8, 1)
    b, lb, _ = _fit(rows.astype(np.float64) * (1 + 2.0 ** -30), 8, 1)
    assert a.centroids.dtype == np.float64
    assert a.centroids.tobytes() == b.centroids.tobytes() and la == lb


# ------------------------------------------------- 5. labels stay on the device
def test_labels_stay_on_the_device():
    import kmeans_amd as ka
    rows = _fit_rows(*FIT_CASES[0])
    t = torch.from_numpy(rows).to(DEV)
    km, host_labels, _ = _fit(rows, 8, 1)
    out = km.predict(t)
    assert isinstance(out, ka.kmeans.LabelsRDD)
    lt = out.to_tensor()
    assert lt.dtype == torch.int32 and lt.device == t.device and lt.shape == (len(rows),)
    assert out._host is None                       # nothing reached the host for it
    assert out.count() == len(rows) and out._host is None
    np.testing.assert_array_equal(lt.cpu().numpy(), host_labels)
    assert out.collect() == host_labels and out.to_tensor() is lt
    np.testing.assert_array_equal(out.to_numpy(), host_labels)
    # an ndarray input: the labels come back as a CPU tensor
    ct = km.predict(rows).to_tensor()
    assert ct.device.type == "cpu" and ct.dtype == torch.int32
    np.testing.assert_array_equal(ct.numpy(), host_labels)


def test_predict_reuses_the_rows_fit_loaded():
    rows = _fit_rows(*FIT_CASES[0])
    t = torch.from_numpy(rows).to(DEV)
    km, labels, _ = _fit(t, 8, 1)
    run = km._runner
    t.zero_()                                      # mutated in place: predict still sees the resident rows
    again = km.predict(t)
    assert km._runner is run
    assert again.collect() == labels
    other = torch.from_numpy(rows).to(DEV)         # another object: loaded afresh, same labels
    assert km.predict(other).collect() == labels and km._runner is run


def test_the_model_does_not_keep_the_tensor_alive():
    import gc
    rows = _fit_rows(*FIT_CASES[0])
    gc.collect()
    before = torch.cuda.memory_allocated(0)
    t = torch.from_numpy(rows).to(DEV)
    assert torch.cuda.memory_allocated(0) >= before + rows.nbytes
    km, _, _ = _fit(t, 8, 1)
    assert km._runner is not None and km._runner.pl.device_rows is None
    del t
    gc.collect()
    assert torch.cuda.memory_allocated(0) <= before      # torch's share: the row store is the library's


def test_tensor_on_the_host_and_sample_weight_tensor():
    rows = _fit_rows(*FIT_CASES[0])
    w = np.random.default_rng(2).uniform(0.5, 2.0, len(rows))
    import kmeans_amd as ka
    a = ka.KMeans(k=8, max_iter=4, seed=1)
    b = ka.KMeans(k=8, max_iter=4, seed=1)
    a.verbose = b.verbose = False
    a.fit(torch.from_numpy(rows).to(DEV), sample_weight=torch.from_numpy(w).to(DEV))
    b.fit(rows, sample_weight=w)
    assert a.centroids.tobytes() == b.centroids.tobytes()
    c = ka.KMeans(k=8, max_iter=4, seed=1)
    c.verbose = False
    c.fit(torch.from_numpy(rows), sample_weight=w)  # a CPU tensor: the host route
    assert c.centroids.tobytes() == b.centroids.tobytes()


# ------------------------------------------------------------ 6. ABI errors
def test_misuse_is_a_return_code():
    from kmeans_amd import _lib
    from kmeans_amd.engine import HipEngine
    eng = HipEngine(0)
    lib, ctx = eng.lib, eng.ctx
    n, d = 8, 4
    t = _values(n, d + 2, torch.float32, 1).to(DEV)
    want = _f32(t.cpu())
    P = ctypes.c_void_p
    ptr = P(t.data_ptr())
    host = np.zeros((n, d + 2), dtype=np.float32)
    assert lib.km_load_device(ctx, 0, ptr, n, d + 2, _lib.KM_DT_F32) == _lib.KM_ERR_STATE     # before km_load_begin
    labels_dev = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    assert lib.km_labels_device(ctx, P(labels_dev.data_ptr())) == _lib.KM_ERR_STATE
    assert lib.km_load_begin(ctx, n, d) == _lib.KM_OK
    torch.cuda.synchronize()

    def good():
        assert lib.km_load_device(ctx, 0, ptr, n, d + 2, _lib.KM_DT_F32) == _lib.KM_OK
        eng.n, eng.d = n, d
        _assert_same_bits(_stored(eng), want[:, :d])

    refused = [
        ("dtype 7", (0, ptr, n, d + 2, 7)),
        ("negative dtype", (0, ptr, n, d + 2, -1)),
        ("stride < d", (0, ptr, n, d - 1, _lib.KM_DT_F32)),
        ("host pointer", (0, P(host.ctypes.data), n, d + 2, _lib.KM_DT_F32)),
        ("null pointer", (0, P(None), n, d + 2, _lib.KM_DT_F32)),
        ("rows past the end", (1, ptr, n, d + 2, _lib.KM_DT_F32)),
        ("negative row0", (-1, ptr, 1, d + 2, _lib.KM_DT_F32)),
        ("negative nrows", (0, ptr, -1, d + 2, _lib.KM_DT_F32)),
    ]
    good()
    for what, args in refused:
        assert lib.km_load_device(ctx, *args) == _lib.KM_ERR_ARG, what
        assert lib.km_last_error().decode().startswith("km_load_device"), what
        good()
    assert lib.km_load_device(ctx, 0, P(None), 0, d + 2, _lib.KM_DT_F32) == _lib.KM_OK          # nrows == 0: nothing
    assert lib.km_load_device(ctx, n, ptr, 0, d + 2, _lib.KM_DT_F32) == _lib.KM_OK
    good()

    # km_labels_device: the same pointer checks
    eng.set_centroids(want[:2, :d].astype(np.float64))
    labels = eng.predict()
    hl = np.zeros(n, dtype=np.int32)
    assert lib.km_labels_device(ctx, P(hl.ctypes.data)) == _lib.KM_ERR_ARG
    assert lib.km_labels_device(ctx, P(None)) == _lib.KM_ERR_ARG
    torch.cuda.synchronize()
    assert lib.km_labels_device(ctx, P(labels_dev.data_ptr())) == _lib.KM_OK
    np.testing.assert_array_equal(labels_dev.cpu().numpy(), labels)
    np.testing.assert_array_equal(eng.labels_tensor().cpu().numpy(), labels)
    good()
    eng.close()


def test_engine_refuses_what_it_cannot_load(engines):
    dev, _ = engines
    with pytest.raises(ValueError, match="cpu"):
        dev.load_device(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="2-D"):
        dev.load_device(torch.zeros(4, device=DEV))
    with pytest.raises(TypeError, match="int32"):
        dev.load_device(torch.zeros(4, 2, dtype=torch.int32, device=DEV))
    assert dev.load_device(torch.zeros(0, 3, device=DEV)) == 0 and dev.labels_tensor().numel() == 0
