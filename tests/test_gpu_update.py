"""Stage 3 of an iteration on its own: the all-reduced statistics -> the next
centroids, the status record and the batch gate (kmeans_spark.py:176-206,
:289-294, :307-313), against a few lines of NumPy.

The kernels: k_update_one / update_one_body (k <= 64 and k d <= 16384),
k_update + k_finalize (every other shape), and around them km_update,
km_update_async and km_batch_end.  No assign kernel runs: the statistics
buffer bound into the context is written by the test (tests/update_data.py;
tests/test_host_update_data.py proves the planted properties without a GPU)
and the update reads it as it stands.

Centroids, counts, the SSE slot, n_empty, nonfinite, stop_reason, ran and
repaired are compared with ==.  max_shift is compared with == where the plant
makes it the same float in any summation order (a power of two, 0, inf) and
within (d + 4) 2^-53 relative elsewhere (derived in update_data.py).
"""
import ctypes

import numpy as np
import pytest

import update_data as ud

pytestmark = pytest.mark.gpu

_PI64 = ctypes.POINTER(ctypes.c_int64)


def _engine(d, weighted=False):
    """Four rows of width d (the rows are irrelevant to the update) and a
    torch statistics buffer bound at the first set_centroids."""
    from kmeans_amd.engine import HipEngine
    eng = HipEngine(0, distributed=True)
    eng.load_host(np.zeros((4, d), dtype=np.float32))
    if weighted:
        eng.load_weights(np.full(4, 1.5))       # weighted mode; the buffer is bound after it, with k more doubles
    return eng


def _plant(eng, flat):
    """Write the statistics, ordered before the update on the engine's stream."""
    import torch
    assert eng._stats_t.numel() == len(flat) == eng.stats_len()
    with torch.cuda.stream(eng._tstream):
        eng._stats_t.copy_(torch.from_numpy(np.ascontiguousarray(flat)))


def _set(eng, C_old, flat):
    eng.set_centroids(C_old)
    _plant(eng, flat)


def _assert_shift(got, rec, d, what):
    want = rec["shift"]
    print(f"{what}: max_shift {got!r} vs {want!r}")
    if rec.get("exact_shift") or not np.isfinite(want) or want == 0.0:
        assert got == want, (what, got, want)
    else:
        assert abs(got - want) <= ud.shift_rtol(d) * want, (what, got, want, (got - want) / want)


def _assert_record(st, counts, rec, d, stop, what, repaired=0):
    np.testing.assert_array_equal(counts, rec["counts"], err_msg=what)
    assert counts.dtype == np.int64
    assert st.sse == rec["sse"], (what, st.sse, rec["sse"])
    assert (st.n_empty, st.nonfinite, st.ran, st.stop_reason, st.repaired) == \
        (rec["n_empty"], rec["nonfinite"], 1, stop, repaired), \
        (what, st.n_empty, st.nonfinite, st.ran, st.stop_reason, st.repaired)
    _assert_shift(st.max_shift, rec, d, what)


def _single(eng, plan, d, what):
    """km_update: no batch, so no stop reason; KM_EMPTY exactly with empties."""
    from kmeans_amd import _lib
    _set(eng, plan["C_old"], plan["flat"])
    st = _lib.KmStatus()
    counts = np.zeros(eng.k, dtype=np.int64)
    rc = eng.lib.km_update(eng.ctx, ctypes.byref(st), counts.ctypes.data_as(_PI64))
    rec = plan["rec"]
    assert rc == (_lib.KM_EMPTY if rec["n_empty"] else _lib.KM_OK), (what, rc)
    _assert_record(st, counts, rec, d, 0, what)
    np.testing.assert_array_equal(eng.get_centroids(1), rec["new"], err_msg=what)
    np.testing.assert_array_equal(eng.get_centroids(0), plan["C_old"], err_msg=what)


def _batch_of_one(eng, plan, d, tol, stop, what):
    _set(eng, plan["C_old"], plan["flat"])
    eng.batch_begin()
    eng.update_async(tol)
    recs = eng.batch_end(1)
    assert len(recs) == 1, what
    _assert_record(recs[0][0], recs[0][1], plan["rec"], d, stop, what)
    # the state km_update would leave: the old set current, the new set beside it
    np.testing.assert_array_equal(eng.get_centroids(1), plan["rec"]["new"], err_msg=what)
    np.testing.assert_array_equal(eng.get_centroids(0), plan["C_old"], err_msg=what)


# ------------------------------------------------------------------ single updates
@pytest.mark.parametrize("pattern", ud.PATTERNS)
@pytest.mark.parametrize("k,d", ud.SHAPES)
def test_update_and_one_iteration_batch(k, d, pattern):
    eng = _engine(d, pattern == "weighted")
    try:
        for case in ud.cases(k, d, pattern):
            plan = ud.plant(case)
            what = ud.case_id(case)
            _single(eng, plan, d, what)
            for tol, stop in plan["tols"]:
                _batch_of_one(eng, plan, d, tol, stop, f"{what} tol={tol!r}")
    finally:
        eng.close()


# ----------------------------------------------------------------- gate and restore
@pytest.mark.parametrize("k,d", ud.TWO_SHAPES)
def test_gate_and_restore_two_kernels(k, d):
    # k_update + k_finalize leave the statistics alone: iteration 2 of a batch
    # over the same buffer divides the same sums, so its new set is iteration
    # 1's and its shift is exactly 0
    assert not ud.update_one_ok(k, d)
    plan = ud.plant(ud.Case(k, d, "noise", 0, False))
    rec = plan["rec"]
    still = dict(rec, shift=0.0, exact_shift=True)
    eng = _engine(d)
    try:
        _set(eng, plan["C_old"], plan["flat"])
        eng.batch_begin()
        for _ in range(5):
            eng.update_async(rec["shift"] / 2)
        recs = eng.batch_end(5)
        assert len(recs) == 2
        _assert_record(*recs[0], rec, d, 0, "iteration 1")
        _assert_record(*recs[1], still, d, 1, "iteration 2")
        # iteration 2's old set is iteration 1's new set, and so is its new set
        np.testing.assert_array_equal(eng.get_centroids(0), rec["new"])
        np.testing.assert_array_equal(eng.get_centroids(1), rec["new"])

        # tol = 0: 0 < 0 is false, nothing stops the batch
        _set(eng, plan["C_old"], plan["flat"])
        eng.batch_begin()
        for _ in range(5):
            eng.update_async(0.0)
        recs = eng.batch_end(5)
        assert len(recs) == 5
        _assert_record(*recs[0], rec, d, 0, "tol 0, iteration 1")
        for i in range(1, 5):
            _assert_record(*recs[i], still, d, 0, f"tol 0, iteration {i + 1}")
        np.testing.assert_array_equal(eng.get_centroids(0), rec["new"])
        np.testing.assert_array_equal(eng.get_centroids(1), rec["new"])

        # commit, then a further batch: as if its centroids had been set afresh
        eng.commit()
        flat2 = ud.plant(ud.Case(k, d, "noise", 1, False))["flat"]
        rec2 = ud.reference(rec["new"], flat2)
        assert rec2["shift"] > 0
        _plant(eng, flat2)
        eng.batch_begin()
        eng.update_async(rec2["shift"] / 2)
        recs = eng.batch_end(1)
        assert len(recs) == 1
        _assert_record(*recs[0], rec2, d, 0, "after commit")
        np.testing.assert_array_equal(eng.get_centroids(0), rec["new"])
        np.testing.assert_array_equal(eng.get_centroids(1), rec2["new"])
    finally:
        eng.close()


@pytest.mark.parametrize("k,d", ud.ONE_SHAPES)
def test_gate_and_restore_one_workgroup(k, d):
    # k_update_one clears the statistics it consumed (the next assign of a
    # batch accumulates into them): with no assign between, iteration 2 sees
    # every cluster empty, stops the batch and changes no centroid
    assert ud.update_one_ok(k, d)
    plan = ud.plant(ud.Case(k, d, "noise", 0, False))
    rec = plan["rec"]
    cleared = {"counts": np.zeros(k, dtype=np.int64), "sse": 0.0, "shift": 0.0, "exact_shift": True,
               "n_empty": k, "nonfinite": 0}
    eng = _engine(d)
    try:
        _set(eng, plan["C_old"], plan["flat"])
        eng.batch_begin()
        for _ in range(5):
            eng.update_async(rec["shift"] / 2)
        recs = eng.batch_end(5)
        assert len(recs) == 2
        _assert_record(*recs[0], rec, d, 0, "iteration 1")
        _assert_record(*recs[1], cleared, d, 2, "iteration 2")
        np.testing.assert_array_equal(eng.get_centroids(0), rec["new"])
        np.testing.assert_array_equal(eng.get_centroids(1), rec["new"])
    finally:
        eng.close()


# --------------------------------------------------------------------- batch limits
def test_batch_limits():
    from kmeans_amd import _lib
    assert _lib.KM_MAX_BATCH == ud.KM_MAX_BATCH == 32
    k, d = 65, 1
    plan = ud.plant(ud.Case(k, d, "noise", 0, False))
    rec = plan["rec"]
    still = dict(rec, shift=0.0, exact_shift=True)
    eng = _engine(d)
    try:
        _set(eng, plan["C_old"], plan["flat"])
        eng.batch_begin()
        for _ in range(32):
            eng.update_async(0.0)
        with pytest.raises(_lib.KmError, match=r"\(-1\)"):           # KM_ERR_ARG: a 33rd iteration
            eng.update_async(0.0)
        recs = eng.batch_end(33)
        assert len(recs) == 32
        _assert_record(*recs[0], rec, d, 0, "iteration 1")
        for i in range(1, 32):
            _assert_record(*recs[i], still, d, 0, f"iteration {i + 1}")
        np.testing.assert_array_equal(eng.get_centroids(1), rec["new"])

        _set(eng, plan["C_old"], plan["flat"])
        eng.batch_begin()
        with pytest.raises(_lib.KmError, match=r"\(-1\)"):           # KM_ERR_ARG: tol < 0
            eng.update_async(-1e-300)
        with pytest.raises(_lib.KmError, match=r"\(-1\)"):
            eng.update_async(float("nan"))
        assert eng.batch_end(1) == []
        np.testing.assert_array_equal(eng.get_centroids(0), plan["C_old"])
    finally:
        eng.close()
