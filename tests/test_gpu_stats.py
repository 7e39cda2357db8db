"""Stage 2 of an iteration on its own: labels -> per-cluster float64 sums,
counts, SSE and sums of weights (reduceByKey + the SSE map of
kmeans_spark.py:169-173 and :224-237), bit for bit under skewed labels.

The kernels: k_stats<SSE, W> (W: weighted; an LDS table tiled over cluster
and feature ranges), the counting-sort route (k_hist, k_scan, k_scatter,
k_put_counts, k_segsum<L, W> for eight row widths), and the
tables the fused screen and k_rerank2 flush.  The inputs are planted integer
data (tests/stats_data.py; tests/test_host_stats_data.py proves their
properties without a GPU): every sum is an integer far below 2^53, so every
comparison here is assert_array_equal -- except the SSE of the cases whose
centroids carry a tail below the fp32 image's resolution, held to the
project's 1e-9.

Every case first asserts the route and the table split that km_stats_route
reports (engine.info()), so that a change of the dispatch cannot hide a
kernel from its test.
"""
import ctypes

import numpy as np
import pytest

import stats_data as sd
from test_host_stats_data import DELTA_GEOMETRIES, delta_iterations

pytestmark = pytest.mark.gpu


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


def _dp(d):
    return next((v for v in (16, 32, 48, 64, 96, 128, 192, 256) if d <= v), (d + 15) // 16 * 16)


def _bind(eng, length):
    import torch
    keep = torch.zeros(length, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.km_bind_stats_buffer(eng.ctx, ctypes.c_void_p(keep.data_ptr())) == 0
    return keep


def _load(X, C, sse, w=None, screen=None):
    eng = _engine()
    eng.load_host(X)
    if w is not None:
        eng.load_weights(w)
    eng.set_sse(sse)
    if screen is not None:
        eng.set_screen(screen)
    eng.set_centroids(C)
    return eng


def _assert_route(info, case):
    """The dispatch of the case, before anything runs."""
    want = {"path": 2, "dp": _dp(case.d), "kp": (case.k + 63) // 64 * 64, "fused_stats": int(case.route == 0),
            "stats_route": case.route, "stats_cluster_ranges": case.ncr, "stats_kr": case.kr,
            "stats_feature_ranges": case.nfr, "stats_fr": case.fr}
    got = {key: info.get(key) for key in want}
    assert got == want, (got, want)


def _step(case, sse, screen=None):
    """load, set centroids, assert the route, bind an external buffer, two
    sweeps on the same centroids, update."""
    b = sd.build(case)
    k, d = case.k, case.d
    eng = _load(b["X"], b["C"], sse, b["w"], screen)
    try:
        _assert_route(eng.info(), case)
        keep = _bind(eng, k * (d + 1) + 1 + (k if case.weighted else 0))
        sweeps = []
        for _ in range(2):
            eng.assign_stats()
            eng.sync()
            sweeps.append((eng.labels(), keep.cpu().numpy().copy()))
        st, counts = eng.update()
        return {"sweeps": sweeps, "counts": counts, "new": eng.get_centroids(1), "sse": st.sse,
                "q": st.q_rerank + st.q_full, "n_empty": st.n_empty, "nonfinite": st.nonfinite,
                "delta": eng.info()["delta_stats"]}
    finally:
        eng.close()


def _check(case, sse, out):
    b, ref = sd.build(case), sd.reference(case)
    k, d = case.k, case.d
    exact_sse = not case.tails
    for labels, flat in out["sweeps"]:
        np.testing.assert_array_equal(labels, b["lab"])
        tab = flat[:k * (d + 1)].reshape(k, d + 1)
        np.testing.assert_array_equal(tab[:, d], ref["counts"])
        np.testing.assert_array_equal(tab[:, :d], ref["sums"])
        slot = flat[k * (d + 1)]
        if not sse:
            assert slot == 0.0
        elif exact_sse:
            assert slot == ref["sse"], (slot, ref["sse"])
        else:
            print(f"sse {slot!r} vs {ref['sse']!r}: rel {slot / ref['sse'] - 1:.3e}")
            np.testing.assert_allclose(slot, ref["sse"], rtol=1e-9)
        if case.weighted:
            np.testing.assert_array_equal(flat[k * (d + 1) + 1:], ref["W"])
        else:
            assert len(flat) == k * (d + 1) + 1
    # the second sweep equals the first
    np.testing.assert_array_equal(out["sweeps"][1][1][:k * (d + 1)], out["sweeps"][0][1][:k * (d + 1)])
    np.testing.assert_array_equal(out["counts"], ref["counts"])
    assert out["n_empty"] == ref["n_empty"] and out["nonfinite"] == 0 and out["delta"] == 0
    if not sse:
        assert out["sse"] == 0.0
    elif exact_sse:
        assert out["sse"] == ref["sse"]
    else:
        np.testing.assert_allclose(out["sse"], ref["sse"], rtol=1e-9)
    # sums / counts, one rounding (k_update); an empty cluster keeps its centroid
    np.testing.assert_array_equal(out["new"], ref["new"])


# ------------------------------------------------- the range-tiled table (route 1)
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("case", sd.ROUTE1_CASES, ids=sd.case_id)
def test_range_tiled_statistics(case, sse):
    assert case.route == 1 and not case.weighted
    _check(case, sse, _step(case, sse))


# ---------------------------------------------------- the counting sort (route 2)
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("case", sd.ROUTE2_SHAPES, ids=sd.case_id)
def test_sorted_statistics_at_each_row_width(case, sse):
    assert case.route == 2
    _check(case, sse, _step(case, sse))


@pytest.mark.parametrize("case", sd.ROUTE2_CASES, ids=sd.case_id)
def test_sorted_statistics_patterns_and_edges(case):
    assert case.route == 2
    _check(case, True, _step(case, True))


# ------------------------------------------------------------- the weighted twins
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("case", sd.WEIGHTED_CASES, ids=sd.case_id)
def test_weighted_statistics(case, sse):
    assert case.weighted
    _check(case, sse, _step(case, sse))


# ---------------------------------------------------------------- SSE correction
@pytest.mark.parametrize("case", sd.TAIL_CASES, ids=sd.case_id)
def test_sse_correction_to_the_float64_centroid(case):
    # k_stats<true> takes the residuals to the fp32 image c' = m and corrects
    # them by the tail c - c' at the flush; the sort route reads c itself.
    # Sums, counts and labels stay exact; the SSE is held to 1e-9 of the
    # exact rational value (the residuals to c' alone miss it by > 4e-9)
    assert case.tails
    _check(case, True, _step(case, True))


# ------------------------------------------------- past the sort's capacity in k
@pytest.mark.parametrize("case", sd.BIG_K_CASES, ids=sd.case_id)
def test_more_clusters_than_the_sort_holds(case):
    # k = 16385: one cluster more than k_hist / k_scatter hold in 64 KiB of
    # LDS.  km_set_centroids accepts the geometry, so the statistics must not
    # choose the sort (it refused with KM_ERR_HIP): the range-tiled table
    # takes it, in 14 cluster ranges (15 with weights)
    assert case.k * 4 > 64 * 1024 and case.route == 1
    _check(case, True, _step(case, True))


# ------------------------------------------------ the fused kernel's table (route 0)
@pytest.mark.parametrize("screen", [0, -1])
@pytest.mark.parametrize("case", sd.FUSED_CASES, ids=sd.case_id)
def test_fused_table(case, screen):
    assert case.route == 0
    for sse in (True, False):
        _check(case, sse, _step(case, sse, screen))


@pytest.mark.parametrize("screen", [0, -1])
def test_bisector_rows_reach_the_statistics_through_the_resolver(screen):
    # 200 rows at equal (integer) distance from a centroid pair: no screen can
    # settle them, k_rerank2 / the full scans label them (the lower index) and
    # add them to the statistics through their own table
    X, C, lab, tied = sd.bisector_case()
    k, d = C.shape
    Xi = X.astype(np.int64)
    counts = np.bincount(lab, minlength=k)
    sums = sd.cluster_sums(lab, k, Xi).astype(np.float64)
    sse = float(((Xi - C[lab].astype(np.int64)) ** 2).sum())
    eng = _load(X, C, True, screen=screen)
    info = eng.info()
    assert (info["path"], info["fused_stats"], info["stats_route"]) == (2, 1, 0), info
    keep = _bind(eng, k * (d + 1) + 1)
    for _ in range(2):
        eng.assign_stats()
        eng.sync()
        flat = keep.cpu().numpy()
        np.testing.assert_array_equal(eng.labels(), lab)
        tab = flat[:-1].reshape(k, d + 1)
        np.testing.assert_array_equal(tab[:, d], counts)
        np.testing.assert_array_equal(tab[:, :d], sums)
        assert flat[-1] == sse
    st, cnt = eng.update()
    eng.close()
    assert st.q_rerank + st.q_full >= sd.BISECTOR_ROWS, (st.q_rerank, st.q_full)
    np.testing.assert_array_equal(cnt, counts)
    assert st.sse == sse and st.n_empty == 1            # the upper centroid of the pair owns nothing


# -------------------------------------------------------------------- delta folds
@pytest.mark.parametrize("situation", ["none", "one", "blob"])
@pytest.mark.parametrize("d,k,n", DELTA_GEOMETRIES)
def test_delta_buffer_is_the_difference_of_the_sums(d, k, n, situation):
    # assign, update, commit, assign: the second assign leaves only the moves
    # of rows between clusters in the buffer (km_assign_stats, delta
    # statistics).  The differences are integers whatever the centroids are
    X, C0 = sd.delta_case(d, k, n, situation)
    lab1, lab2, _ = delta_iterations(X, C0)
    Xi = X.astype(np.int64)
    s1, s2 = sd.cluster_sums(lab1, k, Xi), sd.cluster_sums(lab2, k, Xi)
    c1, c2 = np.bincount(lab1, minlength=k), np.bincount(lab2, minlength=k)
    eng = _load(X, C0, False)
    info = eng.info()
    assert (info["path"], info["dp"], info["kp"]) == (2, 64, k), info
    keep = _bind(eng, k * (d + 1) + 1)
    eng.assign_stats()
    eng.sync()
    first = keep.cpu().numpy().copy()
    np.testing.assert_array_equal(eng.labels(), lab1)
    np.testing.assert_array_equal(first[:-1].reshape(k, d + 1)[:, :d], s1.astype(np.float64))
    np.testing.assert_array_equal(first[:-1].reshape(k, d + 1)[:, d], c1)
    assert eng.info()["delta_stats"] == 0
    _, cnt = eng.update()
    np.testing.assert_array_equal(cnt, c1)
    eng.commit()
    eng.assign_stats()
    eng.sync()
    flat = keep.cpu().numpy().copy()
    assert eng.info()["delta_stats"] == 1
    np.testing.assert_array_equal(eng.labels(), lab2)
    tab = flat[:-1].reshape(k, d + 1)
    np.testing.assert_array_equal(tab[:, :d], (s2 - s1).astype(np.float64))
    np.testing.assert_array_equal(tab[:, d], c2 - c1)
    assert flat[-1] == 0.0
    if situation == "none":
        assert not flat.any()
    _, cnt = eng.update()
    eng.close()
    np.testing.assert_array_equal(cnt, c2)
