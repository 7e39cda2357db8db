"""The small path (k <= 32, d <= 64: k_assign_small, k_prep_small and the
update folded into the assign launch) at every row width, queue level and
edge, against the oracle.

kmeans_spark.py:147-206 (assign + reduceByKey + update), :224-237 (SSE) and
:343-350 (predict).  k_assign_small is compiled per padded row width
DP in {16, 32, 48, 64}, with SSE on and off; DP = 16 and DP > 16 are two code
shapes (waves per SIMD, row registers).  Rows the fp32 bound cannot settle
queue per wave in LDS (SMALL_QW = 32) and past that in the launch's global
queue, which the last workgroup drains; the float64 resolver reproduces
NumPy's pairwise norm, whose 8-accumulator loop has a remainder for
d = 17 ... 64 that d = 16 never has.

a. instance grid: one step at every DP, d = dp and d < dp, k from 1 to 32,
   statistics replicas R from 32 down to 1, both sweep directions;
b. queue levels 0, 1, 31, 32, 33 and 64 rows per wave at each width, with
   statistics (fuse = 1) and as predict (fuse = 0: another LDS layout);
c. more rows than threads: the row loop's second, partial trip;
d. the folded iteration against the two-launch form over three iterations
   (the fold writes the next iteration's fp32 images itself);
e. numeric edges, and inputs whose squared differences leave the fp32 range;
f. the two dispatch boundaries k = 32 | 33 and d = 64 | 65;
g. the weighted statistics pass behind path-1 labels.

The inputs come from tests/small_path_data.py; tests/test_host_small_path_data.py
checks (without a GPU) that they are what these tests assume.
"""
import ctypes

import numpy as np
import pytest

import small_path_data as spd
from oracle import kmeans_oracle as orc
from test_gpu_small_fold import _run

pytestmark = pytest.mark.gpu


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


def _dp(d):
    return (d + 15) // 16 * 16


def _load(X, C0, sse, path=1, dp=None, kp=None, fused=None, screen=None):
    """An engine holding X and C0; the dispatch is asserted first, so that a
    change of it cannot hide the kernel from the test.  screen: km_set_screen
    mode forced before the centroids are set (path 2)."""
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    eng.set_sse(sse)
    if screen is not None:
        eng.set_screen(screen)
    eng.set_centroids(C0)
    info = eng.info()
    assert info["path"] == path, info
    assert info["dp"] == (_dp(X.shape[1]) if dp is None else dp), info
    if kp is not None:
        assert info["kp"] == kp, info
    if fused is not None:
        assert info["fused_stats"] == fused, info
    return eng


def _bind(eng, k, d):
    import torch
    keep = torch.zeros(k * (d + 1) + 1, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.km_bind_stats_buffer(eng.ctx, ctypes.c_void_p(keep.data_ptr())) == 0
    return keep


def _step(X, C0, sse, sweeps=2, **geo):
    """assign_stats `sweeps` times on the same centroids (the sweep direction
    alternates), each read from an external statistics buffer, then update."""
    k, d = C0.shape
    eng = _load(X, C0, sse, **geo)
    keep = _bind(eng, k, d)
    outs = []
    for _ in range(sweeps):
        eng.assign_stats()
        eng.sync()
        outs.append((eng.labels(), keep.cpu().numpy().copy()))
    st, counts = eng.update()
    out = {"sweeps": outs, "counts": counts, "new": eng.get_centroids(1), "sse": st.sse,
           "q": st.q_rerank + st.q_full, "n_empty": st.n_empty, "nonfinite": st.nonfinite}
    eng.close()
    del keep
    return out


_refs = {}


def _reference(key, X, C0):
    """Oracle labels, counts, sums (accumulated in long double), SSE and the
    centroids after one step; computed once per input and left unchanged."""
    if key not in _refs:
        k = len(C0)
        labels, mind, _ = orc.assign(X, C0)
        sums = np.zeros(C0.shape, dtype=np.longdouble)
        np.add.at(sums, labels, X.astype(np.longdouble))
        counts = np.bincount(labels, minlength=k)
        ref = {"labels": labels, "counts": counts, "sums": sums.astype(np.float64),
               "sse": orc.partition_sse(mind)}
        if counts.min() > 0:
            fit = orc.lloyd_fit(X, k, 1, 1e-300, 0, True, 1, init_centroids=C0)
            ref["new"], ref["sse_fit"] = fit["centroids"], fit["sse_history"][0]
        else:  # (lloyd_fit would draw replacement rows; km_update keeps the old centroid and reports)
            new = C0.copy()
            new[counts > 0] = (sums[counts > 0] / counts[counts > 0, None]).astype(np.float64)
            ref["new"], ref["sse_fit"] = new, ref["sse"]
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _check_step(out, ref, sse, atol=0.0):
    """Labels and counts exact, sums, centroids and SSE to 1e-9 relative; the
    second sweep identical in labels and counts, its sums within 1e-12.
    atol: absolute slack of the sums and centroids, for inputs whose sums
    cancel (noise around the origin)."""
    k, d = ref["sums"].shape
    d1 = d + 1
    first = None
    for labels, flat in out["sweeps"]:
        np.testing.assert_array_equal(labels, ref["labels"])
        tab = flat[:-1].reshape(k, d1)
        np.testing.assert_array_equal(tab[:, d], ref["counts"])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.nanmax(np.where(ref["sums"] != 0, np.abs(tab[:, :d] / ref["sums"] - 1), 0.0))
        print(f"sums: max rel err {rel:.3e}; sse {flat[-1]!r} vs {ref['sse_fit']!r}")
        np.testing.assert_allclose(tab[:, :d], ref["sums"], rtol=1e-9, atol=atol)
        if sse:
            np.testing.assert_allclose(flat[-1], ref["sse_fit"], rtol=1e-9)
            np.testing.assert_allclose(flat[-1], ref["sse"], rtol=1e-9)
        else:
            assert flat[-1] == 0.0
        if first is None:
            first = tab
        else:
            np.testing.assert_array_equal(tab[:, d], first[:, d])
            np.testing.assert_allclose(tab[:, :d], first[:, :d], rtol=1e-12, atol=atol)
    np.testing.assert_array_equal(out["counts"], ref["counts"])
    assert out["n_empty"] == int((ref["counts"] == 0).sum()) and out["nonfinite"] == 0
    np.testing.assert_allclose(out["new"], ref["new"], rtol=1e-9, atol=atol)
    if sse:
        np.testing.assert_allclose(out["sse"], ref["sse_fit"], rtol=1e-9)


# ------------------------------------------------------------ a. instance grid
GRID = [(1, 1), (1, 2), (2, 3), (16, 32), (17, 5), (17, 32), (31, 17), (32, 31), (33, 2), (40, 10), (47, 32),
        (48, 1), (49, 7), (63, 3), (64, 32), (64, 1)]


@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("d,k", GRID)
def test_instance_grid_one_step(d, k, sse):
    # n = 3001: ragged, 12 workgroups, so the hand-off to the last one is real
    X, C0 = spd.blobs(3001, d, k, seed=1000 + 100 * d + k)
    ref = _reference(("grid", d, k), X, C0)
    assert ref["counts"].min() > 0
    _check_step(_step(X, C0, sse), ref, sse)


# ------------------------------------------------------------- b. queue levels
def _queue_case(d, k, n):
    X, C0, tied = spd.tie_rows(d, k, spd.QUEUE_GROUPS + [64], seed=100 + d + k)
    return X[:n], C0, tied[:n]


@pytest.mark.parametrize("n", [2560, 2560 + 37])
@pytest.mark.parametrize("d,k", spd.QUEUE_SHAPES)
def test_queue_levels_at_each_width(d, k, n):
    # n = 2560: every wave of either sweep direction holds one aligned block
    # of 64 rows, so its queued-row count is the block's tied count (0, 1,
    # 31, 32, 33, 64: the LDS-only level, both sides of SMALL_QW, a certain
    # overflow).  n = 2597: the reversed sweep's waves straddle the blocks
    X, C0, tied = _queue_case(d, k, n)
    ref = _reference(("queue", d, k, n), X, C0)
    out = _step(X, C0, True)
    _check_step(out, ref, True)           # the lower index wins every tie
    # a lower bound only: near-ties queue too
    print(f"queued {out['q']} rows, tied {int(tied.sum())}")
    assert out["q"] >= int(tied.sum())
    # predict: the same kernel without the statistics table (fuse = 0), the
    # wave queues at another LDS offset
    eng = _load(X, C0, True)
    for _ in range(2):                       # one sweep per direction
        np.testing.assert_array_equal(eng.predict(), ref["labels"])
    eng.close()
    out2 = _step(X, C0, False, sweeps=1)
    _check_step(out2, ref, False)
    assert out2["q"] >= int(tied.sum())


# -------------------------------------------------- c. more rows than threads
@pytest.mark.parametrize("d", [64, 20])
def test_more_rows_than_threads(d):
    # n = 256 * 8 * n_cu + 777: the grid is capped at 8 workgroups per CU, so
    # each thread's row loop and register prefetch take a second, partial
    # trip; tied rows sit in both trips of the same waves (the wave's queue
    # fills across trips and overflows in the second)
    probe = _engine()
    n_cu = probe.info()["n_cu"]
    probe.close()
    X, C0, tied = spd.many_rows_case(d, n_cu)
    assert len(X) == 256 * 8 * n_cu + 777
    labels, mind, _ = orc.assign(X, C0)
    counts = np.bincount(labels, minlength=4)
    sse = orc.partition_sse(mind)
    out = _step(X, C0, True)
    for got, flat in out["sweeps"]:          # one sweep per direction
        np.testing.assert_array_equal(got, labels)
        np.testing.assert_array_equal(flat[:-1].reshape(4, d + 1)[:, d], counts)
        np.testing.assert_allclose(flat[-1], sse, rtol=1e-9)
    np.testing.assert_array_equal(out["counts"], counts)
    np.testing.assert_allclose(out["sse"], sse, rtol=1e-9)
    assert out["q"] >= int(tied.sum())


# --------------------------------------------------- d. fold vs two launches
@pytest.mark.parametrize("d,k", spd.FOLD_SHAPES)
def test_fold_equals_two_launches_at_each_width(d, k):
    X, C0, tied = spd.tie_rows(d, k, spd.FOLD_GROUPS, seed=200 + d + k)
    probe = _load(X, C0, True)
    probe.close()
    a = _run(X, C0, 3, external=False)
    b = _run(X, C0, 3, external=True)
    # k = 1: the mean does not move after the first iteration, so the second
    # one's shift is 0 < tolerance and the batch stops there, as the
    # reference does (kmeans_spark.py:310) -- unless the sums of the two
    # sweeps differ in their last bit, which float64 atomics allow; every
    # iteration that ran is checked either way
    ran = a["ran"]
    assert ran == b["ran"] and (ran == 3 if k > 1 else ran in (2, 3))
    assert a["q"] == b["q"]
    assert a["q"][0][0] + a["q"][0][1] >= int(tied.sum())
    np.testing.assert_array_equal(a["labels"], b["labels"])
    for ca, cb in zip(a["counts"], b["counts"]):
        np.testing.assert_array_equal(ca, cb)
    np.testing.assert_allclose(a["C"], b["C"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a["sse"], b["sse"], rtol=1e-12)
    fit = [orc.lloyd_fit(X, k, i, 1e-300, 0, True, 1, init_centroids=C0) for i in (1, 2, 3)]
    assert fit[2]["n_iter"] == (3 if k > 1 else 2)
    sse = [f["sse_history"][-1] for f in fit][:ran]
    sizes = [f["records"][-1]["sizes"] for f in fit][:ran]
    before_last = fit[ran - 2]["centroids"]
    for r in (a, b):
        assert len(r["sse"]) == len(r["counts"]) == ran
        np.testing.assert_allclose(r["sse"], sse, rtol=1e-9)
        for cnt, ref_cnt in zip(r["counts"], sizes):
            np.testing.assert_array_equal(cnt, ref_cnt)
        # km_batch_end leaves the last iteration uncommitted: the current
        # centroids are those of the iterations before it (two of three),
        # and the last labels theirs.  A wrong fp32 image, pad or max ||c||
        # written by the folded update shows here: the next assign screens
        # with them
        np.testing.assert_allclose(r["C"], before_last, rtol=1e-9, atol=0)
        np.testing.assert_array_equal(r["labels"], orc.assign(X, before_last)[0])


# -------------------------------------------------------------- e. numeric edges
EDGES = {"far": spd.far_from_origin, "magnitudes": spd.feature_magnitudes, "zeros": spd.zero_rows_and_centroids,
         "duplicates": spd.duplicate_centroids, "ulp": spd.ulp_duplicates}


@pytest.mark.parametrize("d,k", [(33, 8), (64, 32)])
@pytest.mark.parametrize("edge", list(EDGES))
def test_numeric_edges(edge, d, k):
    X, C0 = EDGES[edge](3001, d, k, seed=3 + list(EDGES).index(edge))
    ref = _reference((edge, d, k), X, C0)
    if edge == "duplicates":
        assert not np.isin(ref["labels"], spd.duplicate_indices(k)).any()
    out = _step(X, C0, True)
    for labels, flat in out["sweeps"]:
        np.testing.assert_array_equal(labels, ref["labels"])
        np.testing.assert_allclose(flat[-1], ref["sse"], rtol=1e-9)
    np.testing.assert_array_equal(out["counts"], ref["counts"])
    np.testing.assert_allclose(out["sse"], ref["sse"], rtol=1e-9)
    assert out["nonfinite"] == 0
    if edge == "duplicates":
        assert out["n_empty"] == len(spd.duplicate_indices(k))


def _iterate(X, C0, iters, fold):
    """`iters` iterations with SSE: inside a batch (the update folded into
    the assign launch, which then writes the next fp32 images) or as separate
    assign / update / commit calls (k_prep_small writes them)."""
    eng = _load(X, C0, True)
    recs = []
    if fold:
        eng.batch_begin()
        for _ in range(iters):
            eng.assign_stats()
            eng.update_async(1e-300, 0)
        recs = [(st.sse, st.nonfinite, st.n_empty, cnt.copy()) for st, cnt in eng.batch_end(iters)]
    else:
        for i in range(iters):
            eng.assign_stats()
            st, cnt = eng.update()
            recs.append((st.sse, st.nonfinite, st.n_empty, cnt.copy()))
            if i + 1 < iters:
                eng.commit()
    return {"labels": eng.labels(), "old": eng.get_centroids(0), "new": eng.get_centroids(1), "recs": recs}


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("scale", spd.FP32_RANGE_SCALES)
def test_fp32_range_inputs(scale, fold):
    # (x - c)^2 overflows (1e20) or underflows (1e-25) float32: the fp32 form
    # cannot judge such rows, they belong in the float64 queue.  (Before the
    # bound had its underflow term, the 1e-25 rows all took label 0: every
    # score was 0, the bound too, and the keys' index bits decided)
    d, k = 33, 8
    X, C0 = spd.fp32_range(3001, d, k, seed=9, scale=scale)
    key = ("range", scale)
    if key not in _refs:
        _refs[key] = (orc.lloyd_fit(X, k, 1, 1e-300, 0, True, 1, init_centroids=C0),
                      orc.lloyd_fit(X, k, 2, 1e-300, 0, True, 1, init_centroids=C0))
    ref1, ref2 = _refs[key]
    out = _iterate(X, C0, 2, fold)
    assert len(out["recs"]) == 2
    print([r[0] for r in out["recs"]], ref2["sse_history"])
    np.testing.assert_array_equal(out["labels"], orc.assign(X, ref1["centroids"])[0])
    atol = 1e-9 * float(np.abs(X).max())
    np.testing.assert_allclose(out["old"], ref1["centroids"], rtol=1e-9, atol=atol)
    np.testing.assert_allclose(out["new"], ref2["centroids"], rtol=1e-9, atol=atol)
    np.testing.assert_allclose([r[0] for r in out["recs"]], ref2["sse_history"], rtol=1e-9)
    for (_, nonfinite, n_empty, cnt), rec in zip(out["recs"], ref2["records"]):
        assert nonfinite == 0 and n_empty == 0
        np.testing.assert_array_equal(cnt, rec["sizes"])


# ------------------------------------------------------ f. dispatch boundaries
def _boundary(d, k):
    # the same blobs on both sides of a boundary: 33 blobs in 20 features
    # (the 33rd centroid is the one k = 32 leaves out), 5 blobs in 65
    # features (d = 64 drops the last one)
    if d <= 20:
        X, C = spd.blobs(4000, 20, 33, seed=61)
        return X, C[:k]
    X, C = spd.blobs(4000, 65, 5, seed=62)
    return np.ascontiguousarray(X[:, :d]), np.ascontiguousarray(C[:, :d])


@pytest.mark.parametrize("d,k,path", [(20, 32, 1), (20, 33, 2), (64, 5, 1), (65, 5, 2)])
def test_dispatch_boundaries(d, k, path):
    X, C0 = _boundary(d, k)
    ref = _reference(("boundary", d, k), X, C0)
    assert ref["counts"].min() > 0
    geo = {"path": path}
    if path == 2:   # mostly pad on the far side
        geo["kp"] = 64
        if d == 65:
            geo["dp"] = 96
    for sse in (True, False):
        _check_step(_step(X, C0, sse, **geo), ref, sse)


@pytest.mark.parametrize("d,k", [(20, 33), (65, 5)])
def test_ulp_duplicates_past_the_boundaries(d, k):
    X, C0 = spd.ulp_duplicates(4000, d, k, seed=70 + k)
    ref = _reference(("boundary-ulp", d, k), X, C0)
    out = _step(X, C0, True, path=2, kp=64, dp=96 if d == 65 else None)
    for labels, flat in out["sweeps"]:
        np.testing.assert_array_equal(labels, ref["labels"])
        np.testing.assert_allclose(flat[-1], ref["sse"], rtol=1e-9)
    np.testing.assert_array_equal(out["counts"], ref["counts"])
    np.testing.assert_allclose(out["sse"], ref["sse"], rtol=1e-9)


# ---------------------------------------------------------- g. weights on path 1
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("n,d,k", [(3001, 33, 5), (3001, 64, 32)])
def test_weighted_step_on_the_small_path(n, d, k, sse):
    # the weighted pass reads the float64 centroids with stride d, not dp
    import weighted_ref as wr
    X, C0 = spd.blobs(n, d, k, seed=80 + d)
    w = np.random.default_rng(81 + d).uniform(0.5, 2.0, n)
    labels = wr.exact_labels(X, C0)
    _, _, _, cnt, new, ref_sse = wr.weighted_step(X, w, C0, sse, labels)
    eng = _load(X, C0, sse)
    eng.load_weights(w)
    eng.set_sse(sse)
    eng.set_centroids(C0)
    assert eng.info()["path"] == 1
    eng.assign_stats()
    st, counts = eng.update()
    got = eng.get_centroids(1)
    np.testing.assert_array_equal(eng.labels(), labels)
    np.testing.assert_array_equal(counts, np.bincount(labels, minlength=k))
    np.testing.assert_array_equal(counts, cnt)
    assert st.n_empty == int((cnt == 0).sum())
    print(f"max |dC| = {np.abs(got - new).max():.3e}, sse {st.sse!r} vs {ref_sse!r}")
    np.testing.assert_allclose(got, new, rtol=1e-9, atol=1e-9)
    if sse:
        np.testing.assert_allclose(st.sse, ref_sse, rtol=1e-9, atol=1e-9)
    assert eng.info()["delta_stats"] == 0
    eng.close()
