"""k-means|| seeding on the GPU (km_seed_*, csrc/km_seed.hip) against the NumPy
restatement of tests/seeding_ref.py: D2 bitwise, near with the lowest id on
ties, phi within the summation bound and identical on a repeat, the pick rule
exactly, the histogram, the state errors, and one fit end to end."""
import contextlib
import ctypes
import io
import math

import numpy as np
import pytest

from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

KM_ERR_ARG, KM_ERR_STATE = -1, -3

# n, d, candidates of the first and of the second update
GEOMETRIES = {
    "small": (5001, 16, 7, 7),            # the small direct-form path
    "mfma": (20003, 64, 1, 300),          # one candidate, then the MFMA path with kp padded to 320
    "d128": (4099, 128, 130, 130),
    "wide": (2051, 300, 70, 70),          # wide rows: depth-5 pairwise sums
}


def _case(name):
    """Rows, two candidate batches and the restatement's state after each.
    Some rows are exact copies of candidates (D2 exactly 0 there), and the
    second batch repeats one candidate of the first (a tie: the lower id)."""
    import seeding_ref as ref
    n, d, m1, m2 = GEOMETRIES[name]
    rng = np.random.default_rng(n + d)
    centers = rng.uniform(-20, 20, (12, d))
    X = (centers[rng.integers(0, 12, n)] + rng.standard_normal((n, d))).astype(np.float32)
    X[n - 3] = X[5]                                 # duplicate rows
    X64 = X.astype(np.float64)

    def batch(m):
        # half data rows (float32 values), half free float64 points
        B = centers[rng.integers(0, 12, m)] + rng.standard_normal((m, d))
        take = rng.choice(n, size=(m + 1) // 2, replace=False)
        B[:len(take)] = X64[take]
        return B

    B1 = batch(m1)
    B2 = batch(m2)
    B2[m2 - 1] = B1[0]                              # the duplicated candidate
    D2, near = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    states = []
    ref.update(X64, D2, near, B1, 0)
    states.append((D2.copy(), near.copy()))
    ref.update(X64, D2, near, B2, m1)
    states.append((D2.copy(), near.copy()))
    return {"X": X, "B": (B1, B2), "first": (0, m1), "states": states, "m_total": m1 + m2}


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _case(name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def engine():
    import kmeans_amd  # noqa: F401
    from kmeans_amd.engine import HipEngine
    eng = HipEngine(0)
    yield eng
    eng.close()


def _run_updates(eng, c, upto=2):
    """Load the case and run its updates; [(phi, D2, near)] after each."""
    eng.load_host(c["X"])
    eng.seed_begin()
    out = []
    for B, first in list(zip(c["B"], c["first"]))[:upto]:
        eng.set_centroids(B)
        phi = eng.seed_update(first)
        d2, near = eng.seed_read()
        out.append((phi, d2, near))
    return out


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_fold_is_bitwise_the_restatement(engine, cases, name):
    c = cases(name)
    n = len(c["X"])
    got = _run_updates(engine, c)
    try:
        for (phi, d2, near), (D2, NEAR) in zip(got, c["states"]):
            assert np.array_equal(d2.view(np.uint64), D2.view(np.uint64)), \
                f"{np.count_nonzero(d2 != D2)} of {n} D2 differ"
            np.testing.assert_array_equal(near, NEAR)
            want = math.fsum(D2)
            # non-negative terms: any summation order is within (n - 1) 2^-53 relative
            assert abs(phi - want) <= n * 2.0 ** -52 * want, (phi, want)
        assert np.count_nonzero(c["states"][1][0] == 0.0) >= (len(c["B"][0]) + 1) // 2  # rows that are candidates
        # the duplicated candidate never takes a row from its earlier copy
        assert not np.any(got[1][2] == c["m_total"] - 1)
        # identical calls, identical bits (folding the same batch again changes no state)
        engine.set_centroids(c["B"][1])
        a = engine.seed_update(c["first"][1])
        b = engine.seed_update(c["first"][1])
        assert a == b == got[1][0]
        d2, near = engine.seed_read()
        np.testing.assert_array_equal(d2, c["states"][1][0])
        np.testing.assert_array_equal(near, c["states"][1][1])
        # the histogram
        w = engine.seed_weights(c["m_total"])
        np.testing.assert_array_equal(w, np.bincount(c["states"][1][1], minlength=c["m_total"]))
        assert int(w.sum()) == n
        np.testing.assert_array_equal(engine.seed_weights(c["m_total"] + 9000)[:c["m_total"]], w)  # no LDS table
        # the context is left as a predict leaves it: labels of the last batch
        np.testing.assert_array_equal(engine.labels(), orc.assign(c["X"].astype(np.float64), c["B"][1])[0])
    finally:
        engine.seed_end()


@pytest.mark.parametrize("name", ["small", "mfma"])
def test_pick_rule_is_exactly_the_restatement(engine, cases, name):
    import seeding_ref as ref
    c = cases(name)
    n = len(c["X"])
    assert n % 64 != 0
    _run_updates(engine, c)
    try:
        D2 = c["states"][1][0]
        phi = math.fsum(D2)
        many = 0
        for seed, rnd, row0, ell, ph in [
                (42, 1, 0, 16.0, phi), (42, 2, 0, 16.0, phi), (2 ** 63 + 9, 3, 2 ** 33 + 5, 600.0, phi),
                (7, 5, 12345, float(n), phi),            # ell D2 / phi > 1 for many rows
                (7, 1, 2 ** 33 + 5, 3.0, 1e-290),        # phi tiny: every row with D2 > 0
                (0, 4, 1, 0.25, phi * 1.0000000001), (-3 % 2 ** 64, 2, 77, 2048.0, phi)]:
            want = ref.pick(D2, seed, rnd, row0, ell, ph)[0]
            many += int(np.count_nonzero(ell * D2 > ph) > n // 10)
            got = engine.seed_sample(seed, rnd, row0, ell, ph, cap=n)
            assert got is not None
            np.testing.assert_array_equal(got, want)
        assert many >= 2
        # a cap below the pick count: the error, nothing written beyond cap
        want = ref.pick(D2, 42, 1, 0, 64.0, phi)[0]
        assert len(want) > 8
        cap = len(want) - 3
        out = np.full(len(want) + 16, -77, dtype=np.int64)
        cnt = ctypes.c_int64(-1)
        rc = engine.lib.km_seed_sample(engine.ctx, ctypes.c_uint64(42), 1, 0, 64.0, phi,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cap, ctypes.byref(cnt))
        assert rc == KM_ERR_ARG
        assert np.all(out[cap:] == -77)
        assert engine.seed_sample(42, 1, 0, 64.0, phi, cap=cap) is None
        got = engine.seed_sample(42, 1, 0, 64.0, phi, cap=len(want))   # exactly enough room
        np.testing.assert_array_equal(got, want)
    finally:
        engine.seed_end()


def test_state_errors_do_not_launch():
    from kmeans_amd.engine import HipEngine
    eng = HipEngine(0)
    lib, ctx = eng.lib, eng.ctx
    phi, cnt = ctypes.c_double(), ctypes.c_int64()
    out = np.zeros(8, dtype=np.int64)
    pout = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def all_but_begin():
        return [lib.km_seed_update(ctx, 0, ctypes.byref(phi)),
                lib.km_seed_sample(ctx, ctypes.c_uint64(1), 1, 0, 2.0, 1.0, pout, 8, ctypes.byref(cnt)),
                lib.km_seed_weights(ctx, 4, pout), lib.km_seed_read(ctx, None, None), lib.km_seed_end(ctx)]
    try:
        assert lib.km_seed_begin(ctx) == KM_ERR_STATE           # no rows loaded
        assert all_but_begin() == [KM_ERR_STATE] * 5
        eng.load_host(np.arange(12, dtype=np.float32).reshape(6, 2))
        assert all_but_begin() == [KM_ERR_STATE] * 5           # rows, but no km_seed_begin
        eng.seed_begin()
        assert lib.km_seed_update(ctx, 0, ctypes.byref(phi)) == KM_ERR_STATE   # no candidate batch set
        d2, near = eng.seed_read()
        assert np.all(np.isinf(d2)) and np.all(near == -1)
        eng.seed_end()
        assert lib.km_seed_end(ctx) == KM_ERR_STATE
        # loading new rows releases the state
        eng.seed_begin()
        eng.load_host(np.zeros((3, 2), dtype=np.float32))
        assert lib.km_seed_read(ctx, None, None) == KM_ERR_STATE
        # a context with no rows is valid: phi 0, no picks, zero counts
        eng.load_host(np.zeros((0, 2), dtype=np.float32))
        eng.seed_begin()
        eng.set_centroids(np.array([[1.0, 2.0]]))
        assert eng.seed_update(0) == 0.0
        assert len(eng.seed_sample(1, 1, 0, 2.0, 1.0)) == 0
        np.testing.assert_array_equal(eng.seed_weights(3), [0, 0, 0])
        eng.seed_end()
    finally:
        eng.close()


def test_seeding_state_is_independent_of_the_lloyd_state(engine, cases):
    # a Lloyd step between two updates neither disturbs D2 / near nor is disturbed
    c = cases("small")
    X64 = c["X"].astype(np.float64)
    _run_updates(engine, c, upto=1)
    try:
        C = X64[:5].copy()
        engine.set_centroids(C)
        engine.set_sse(True)
        engine.assign_stats()
        st, counts = engine.update()
        lab = orc.assign(X64, C)[0]
        np.testing.assert_array_equal(counts, np.bincount(lab, minlength=5))
        engine.set_sse(False)
        engine.set_centroids(c["B"][1])
        engine.seed_update(c["first"][1])
        d2, near = engine.seed_read()
        assert np.array_equal(d2.view(np.uint64), c["states"][1][0].view(np.uint64))
        np.testing.assert_array_equal(near, c["states"][1][1])
    finally:
        engine.seed_end()


def test_fit_end_to_end_matches_restatement_and_oracle():
    import kmeans_amd as ka
    import seeding_ref as ref
    rng = np.random.default_rng(21)
    centers = rng.uniform(-30, 30, (8, 64))
    X = (centers[rng.integers(0, 8, 20003)] + 2.0 * rng.standard_normal((20003, 64))).astype(np.float32)
    X = X.astype(np.float64)                      # float64 input: float64 centroids back
    k, seed = 8, 42
    want = ref.kmeans_parallel_ref(X, [len(X)], k, seed)
    # the device sums phi in another order: no pick decision may sit within its rounding
    assert want["margin"] > 1e-9, want["margin"]

    class Capturing(ka.KMeans):
        def _initialize_centroids(self, run):
            self.init_centroids = super()._initialize_centroids(run)
            return self.init_centroids

    km = Capturing(k=k, max_iter=12, tolerance=1e-6, seed=seed, compute_sse=True, init="k-means||")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        km.fit(X)
    assert np.array_equal(km.init_centroids.view(np.uint64), want["centroids"].view(np.uint64))
    assert f"Initialization: k-means|| (rounds={want['rounds']}, candidates={len(want['candidates'])})" \
        in buf.getvalue().splitlines()[2]
    o = orc.lloyd_fit(X, k, 12, 1e-6, seed, True, 1, init_centroids=want["centroids"])
    np.testing.assert_allclose(km.centroids, o["centroids"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(km.sse_history, o["sse_history"], rtol=1e-9)
    labels = np.array(km.predict(X).collect())
    np.testing.assert_array_equal(labels, orc.predict(X, o["centroids"]))
    assert km._runner.engine.info()["path"] in (1, 2)
