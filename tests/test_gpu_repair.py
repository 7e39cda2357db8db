"""The empty-cluster repair on the device (kmeans_spark.py:191-204 inside a
batch: k_rep_bernoulli, k_rep_finish, k_rep_pick, k_rep_apply, and the arming
logic of km_set_layout / km_update_async / km_batch_end) against the oracle's
takeSample restatement, with planted empties and real rows.

The statistics are written by the test (tests/update_data.py), so the empty
clusters are exactly the planted ids; the rows are small integers, the same
in float32 and float64.  Each empty cluster, in ascending id order, must
hold the row takeSample(False, n_empty, seed) returns at its position, bit
for bit; the other clusters hold S / cnt.  tests/test_host_update_data.py
proves the cases' properties without a GPU.

Not reached (read only, DESIGN.md "Stage 3"): the stop after a Bernoulli pass
with too few picks (probability about e^-21.7 by takeSample's fraction) and
the stop after a partition overflowed its pick slots (more than four times
the expected picks).
"""
import numpy as np
import pytest

import update_data as ud
from oracle import kmeans_oracle as orc
from test_gpu_update import _assert_record, _plant

pytestmark = pytest.mark.gpu

NEAR = 2.0 ** -40        # "just above / below" a shift: far outside the (d + 4) 2^-53 of the comparison


def _engine(X, sizes, row0, mode):
    from kmeans_amd.engine import HipEngine
    eng = HipEngine(0, distributed=True)
    eng.load_host(X.astype(np.float32))
    eng.set_layout(sizes, row0, mode)
    return eng


def _batch(eng, flat, tol, seed, m=1):
    _plant(eng, flat)
    eng.batch_begin()
    for _ in range(m):
        eng.update_async(tol, seed)
    return eng.batch_end(m)


def _mode1(plan, layout, tol, seed):
    """One armed iteration with every row resident: (status, counts, new)."""
    eng = _engine(plan["X"], layout, 0, 1)
    try:
        assert eng.repair_state() == (True, False)
        eng.set_centroids(plan["C_old"])
        recs = _batch(eng, plan["flat"], tol, seed)
        assert len(recs) == 1
        np.testing.assert_array_equal(eng.get_centroids(0), plan["C_old"])
        return recs[0][0], recs[0][1], eng.get_centroids(1)
    finally:
        eng.close()


# -------------------------------------------------------------------------- mode 1
@pytest.mark.parametrize("case", ud.REPAIR_CASES, ids=ud.repair_id)
def test_device_repair_matches_take_sample(case):
    k, d = case.k, case.d
    layout = ud.LAYOUTS[case.layout]
    empty = ud.repair_empties(k, case.empties)
    plan = ud.plant_repair(k, d, empty, layout, case.big)
    gidx = ud.picks(layout, len(empty), case.seed)
    rec = ud.repaired(plan, empty, gidx)
    assert rec["n_empty"] == len(empty)
    runs = [(rec["shift"] * (1 + NEAR), 1), (rec["shift"] * (1 - NEAR), 0)]
    if not case.big:
        # the maximum is a replacement row's shift, the root of an integer: the same float in any
        # order, so max_shift == it and tol == it does not converge (the strict < of rep_apply)
        rec["exact_shift"] = True
        runs.append((rec["shift"], 0))
    eng = _engine(plan["X"], layout, 0, 1)
    try:
        assert eng.repair_state() == (True, False)
        for tol, stop in runs:
            eng.set_centroids(plan["C_old"])
            recs = _batch(eng, plan["flat"], tol, case.seed)
            assert len(recs) == 1
            _assert_record(*recs[0], rec, d, stop, f"stop {stop}", repaired=1)
            new = eng.get_centroids(1)
            for i, j in enumerate(empty):                # the row of its position in takeSample's order
                np.testing.assert_array_equal(new[j], plan["X"][gidx[i]], err_msg=f"empty[{i}] = {j}")
            np.testing.assert_array_equal(new, rec["new"])
            np.testing.assert_array_equal(eng.get_centroids(0), plan["C_old"])
            assert eng.repair_state() == (True, False)
    finally:
        eng.close()


# ------------------------------------------------- takeSample's every-row branch
@pytest.mark.parametrize("seed", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("layout", ud.EVERY_ROW_LAYOUTS)
def test_every_row_branch_is_left_to_the_host(layout, seed):
    k, d = 9, 3
    empty = list(range(1, 9))
    assert len(empty) >= sum(layout)
    plan = ud.plant_repair(k, d, empty, layout, False)
    eng = _engine(plan["X"], layout, 0, 1)
    try:
        eng.set_centroids(plan["C_old"])
        recs = _batch(eng, plan["flat"], 1e-9, seed, m=3)
        assert len(recs) == 1
        _assert_record(*recs[0], plan["plain"], d, 2, "every row")            # KM_STOP_EMPTY, repaired 0
        np.testing.assert_array_equal(eng.get_centroids(1), plan["plain"]["new"])
        assert eng.repair_state() == (True, False)
        # the host repairs by the same policy (kmeans_spark.py:196-204)
        want, _, listed = orc.update_centroids(
            ud.stats_dict(plan["C_old"], plan["flat"]), plan["C_old"],
            lambda m: [plan["X"][g] for g in orc.take_sample_indices(list(layout), m, seed)])
        assert listed == empty
        gidx = orc.take_sample_indices(list(layout), len(empty), seed)
        ids = empty[:len(gidx)]
        eng.replace_rows(ids, plan["X"][gidx[:len(ids)]])
        eng.commit()
        np.testing.assert_array_equal(eng.get_centroids(0), want)
    finally:
        eng.close()


# ----------------------------------------------------------- arming across batches
@pytest.mark.parametrize("k", [5, 65])
def test_arming_across_batches(k):
    d, layout, seed = 3, ud.LAYOUTS["one"], 42
    empty = ud.repair_empties(k, "chunk_edges")
    full = ud.plant_repair(k, d, (), layout, False)
    holes = ud.plant_repair(k, d, empty, layout, False)
    C0 = full["C_old"]
    eng = _engine(full["X"], layout, 0, 1)
    try:
        assert eng.repair_state() == (True, False)                  # 1. armed by the layout
        eng.set_centroids(C0)
        assert eng.repair_state() == (True, False)
        recs = _batch(eng, full["flat"], 0.0, seed)                 # 2. a batch without empties
        assert len(recs) == 1
        _assert_record(*recs[0], full["plain"], d, 0, "no empties")
        assert eng.repair_state() == (False, False)
        C1 = eng.get_centroids(0)
        np.testing.assert_array_equal(C1, C0)
        plain = ud.reference(C1, holes["flat"])
        recs = _batch(eng, holes["flat"], 1e-9, seed, m=3)          # 3. empties, not armed: the batch stops
        assert len(recs) == 1
        _assert_record(*recs[0], plain, d, 2, "not armed")
        np.testing.assert_array_equal(eng.get_centroids(1), plain["new"])
        np.testing.assert_array_equal(eng.get_centroids(0), C1)
        assert eng.repair_state() == (True, False)                  #    ... and arms again
        rec = ud.repaired({"plain": plain, "X": full["X"], "C_old": C1}, empty,
                          ud.picks(layout, len(empty), seed))
        recs = _batch(eng, holes["flat"], rec["shift"] * (1 + NEAR), seed, m=3)   # 4. repaired on the device
        assert len(recs) == 1
        _assert_record(*recs[0], rec, d, 1, "armed", repaired=1)
        np.testing.assert_array_equal(eng.get_centroids(1), rec["new"])
        assert eng.repair_state() == (True, False)
    finally:
        eng.close()


# ------------------------------------------------------- non-finite outranks repair
@pytest.mark.parametrize("k", [5, 257])
def test_nonfinite_outranks_repair(k):
    d, layout = 17, ud.LAYOUTS["twist"]
    empty = ud.repair_empties(k, "chunk_edges")
    plan = ud.plant_repair(k, d, empty, layout, False, nan=True)
    assert plan["plain"]["nonfinite"] == 1 and plan["plain"]["n_empty"] == len(empty)
    eng = _engine(plan["X"], layout, 0, 1)
    try:
        eng.set_centroids(plan["C_old"])
        assert eng.repair_state() == (True, False)
        recs = _batch(eng, plan["flat"], 1e-9, 42, m=2)
        assert len(recs) == 1
        _assert_record(*recs[0], plan["plain"], d, 3, "nan beside empties")   # KM_STOP_NONFINITE, repaired 0
        new = eng.get_centroids(1)
        np.testing.assert_array_equal(new, plan["plain"]["new"])
        np.testing.assert_array_equal(new[empty], plan["C_old"][empty])         # no centroid replaced
    finally:
        eng.close()


# ------------------------------------------------------------ mode 2 in one process
@pytest.mark.parametrize("window", ["inner", "outer"])
@pytest.mark.parametrize("d", [3, 17])
def test_mode2_ownership_window(d, window):
    import torch
    from kmeans_amd import _lib
    m = ud.MODE2
    k, seed, empty = m["k"], m["seed"], list(m["empty"])
    layout = ud.LAYOUTS[m["layout"]]
    plan = ud.plant_repair(k, d, empty, layout, False)
    gidx = ud.picks(layout, len(empty), seed)
    rec = ud.repaired(plan, empty, gidx)
    tol = rec["shift"] * (1 - NEAR)
    row0, n = ud.mode2_windows(gidx)[window]
    X = plan["X"]
    owned = [row0 <= g < row0 + n for g in gidx]
    mine, other = np.zeros((k, d)), np.zeros((k, d))
    for i, g in enumerate(gidx):
        (mine if owned[i] else other)[i] = X[g]
    eng = _engine(X[row0:row0 + n], layout, row0, 2)
    try:
        assert eng.repair_state() == (True, False)
        eng.set_centroids(plan["C_old"])
        eng.repair_bind()
        _plant(eng, plan["flat"])
        eng.batch_begin()
        eng.update_async(tol, seed)
        assert eng.repair_state() == (True, True)                   # waiting for the exchange
        with pytest.raises(_lib.KmError, match=r"\(-3\)"):          # KM_ERR_STATE
            eng.update_async(tol, seed)
        eng.sync()
        # the rows this context owns, zeros for the others
        np.testing.assert_array_equal(eng._rep_t.cpu().numpy().reshape(k, d)[:len(gidx)], mine[:len(gidx)])
        rest = torch.from_numpy(other.reshape(-1)).to("cuda:0")
        torch.cuda.synchronize()

        def allreduce(t, async_op=True):                            # the other ranks' contribution
            t.add_(rest)
            return None

        eng.repair_exchange(allreduce)
        assert eng.repair_state() == (True, False)
        recs = eng.batch_end(1)
        assert len(recs) == 1
        _assert_record(*recs[0], rec, d, 0, f"mode 2 {window}", repaired=1)
        new = eng.get_centroids(1)
        np.testing.assert_array_equal(new, rec["new"])
        assert eng.repair_state() == (True, False)
    finally:
        eng.close()
    # the mode-1 result, bit for bit
    st1, counts1, new1 = _mode1(plan, layout, tol, seed)
    st2 = recs[0][0]
    assert (st1.max_shift, st1.sse, st1.n_empty, st1.nonfinite, st1.stop_reason, st1.repaired) == \
        (st2.max_shift, st2.sse, st2.n_empty, st2.nonfinite, st2.stop_reason, st2.repaired)
    np.testing.assert_array_equal(counts1, recs[0][1])
    np.testing.assert_array_equal(new1, new)


# ------------------------------------------------------ a layout ends with its load
def test_a_layout_ends_with_its_load():
    # km_load_begin drops the takeSample layout with the rows it described.
    # Kept, an armed repair sampled the old layout after a reload with the same
    # k: picks beyond the new n, reported as a non-finite iteration
    k, d, layout = 5, 3, ud.LAYOUTS["one"]
    empty = ud.repair_empties(k, "chunk_edges")
    plan = ud.plant_repair(k, d, empty, layout, False)
    eng = _engine(plan["X"], layout, 0, 1)
    try:
        eng.set_centroids(plan["C_old"])
        assert eng.repair_state() == (True, False)
        eng.load_host(plan["X"][:300].astype(np.float32))          # same d, same k below, fewer rows
        eng.set_centroids(plan["C_old"])
        assert eng.repair_state() == (False, False)
        recs = _batch(eng, plan["flat"], 1e-9, 42, m=2)
        assert eng.repair_state()[0] is False
        assert len(recs) == 1
        _assert_record(*recs[0], plan["plain"], d, 2, "after the reload")      # KM_STOP_EMPTY, repaired 0
        np.testing.assert_array_equal(eng.get_centroids(1), plan["plain"]["new"])
    finally:
        eng.close()
