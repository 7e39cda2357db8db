"""The wide-row path (256 < d <= 2048: k_assign_wide with its resolver
instances k_rerank2<true> and k_fullscan<2, true>) at every feature piece,
centroid chunk and edge, against the oracle.

kmeans_spark.py:147-206 (assign + reduceByKey + update), :224-237 (SSE) and
:343-350 (predict).  k_assign_wide walks a row tile through pieces of 64
features (four K-steps of 16; the last piece may hold 1 to 4) and chunks of
256 centroids, double-buffered in LDS; a workgroup of 8 waves x 32 rows takes
tile groups blockIdx.x, blockIdx.x + gridDim.x, ... and prefetches the next
group's first piece during the last piece of the current one.  Rows its fp32
bound cannot settle queue per wave: pairs from the front of the wave's
segment, rows without a pair certificate from its back.

Most inputs are `wide_data.planted`: every row's decision is between two
centroids that differ in one feature of a chosen piece, 3 to 40 decision
thresholds apart.  Such a row must be decided by the screen (q == 0 is a
consequence of the kernel's own bound, not a measurement), and a screen that
lost a piece, a K-step or a centroid block mislabels or queues it.

a. width grid: every width of the last piece, the smallest and the largest
   dp, odd and even piece counts; one step with SSE on and off, two sweeps,
   then predict twice on the same engine;
b. chunk grid: k from 1 to 513 (one partial chunk to two full ones and a
   64-wide third);
c. row-count edges: below, at and past one tile and one tile group;
d. tile groups: more than 256 n_cu rows, so that every workgroup takes a
   second and some a third, partial trip (the prefetch across groups, the
   buffer parity carried over for odd and even piece counts, a queue segment
   filled over several trips);
e. queue segments filled completely from both ends;
f. the wide resolvers at every shape of NumPy's pairwise tree;
g. numeric edges;
h. three iterations (the images are prepared again with new centroids);
i. the dispatch boundaries d = 256 | 257 and d = 2048 | 2049.

The inputs come from tests/wide_data.py; tests/test_host_wide_data.py checks
(without a GPU) that they are what these tests assume.  The oracle is
wide_data.step: test_gpu_small_instances._reference in chunks of 128 rows
(orc.assign's default chunk holds n k d float64s at once).
"""
import numpy as np
import pytest

import wide_data as wd
from oracle import kmeans_oracle as orc
from test_gpu_small_instances import _bind, _check_step, _engine, _load, _step

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(key, X, C0, mult=None):
    """The oracle's step for an input, computed once and left unchanged."""
    if key not in _refs:
        ref = wd.step(X, C0, mult)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _geo(d, k):
    # asserted by _load before anything runs: a change of dispatch cannot
    # hide the kernel from the test
    return dict(path=2, dp=wd.dp_of(d), kp=wd.kp_of(k), fused=0)


def _step_predict(X, C0, sse, **geo):
    """_step (two sweeps read from an external statistics buffer, then the
    update), with the two queue counts apart and predict twice on the same
    engine afterwards: the update has prepared the images of the new
    centroids, predict prepares those of the current ones again."""
    k, d = C0.shape
    eng = _load(X, C0, sse, **geo)
    keep = _bind(eng, k, d)
    outs = []
    for _ in range(2):
        eng.assign_stats()
        eng.sync()
        outs.append((eng.labels(), keep.cpu().numpy().copy()))
    st, counts = eng.update()
    out = {"sweeps": outs, "counts": counts, "new": eng.get_centroids(1), "sse": st.sse,
           "q": st.q_rerank + st.q_full, "q_rerank": st.q_rerank, "q_full": st.q_full, "n_empty": st.n_empty,
           "nonfinite": st.nonfinite, "predict": [eng.predict(), eng.predict()]}
    eng.close()
    del keep
    return out


def _check_planted(X, C0, ref, **geo):
    for sse in (True, False):
        out = _step_predict(X, C0, sse, **geo)
        print(f"sse {sse}: queued {out['q']} of {len(X)}")
        _check_step(out, ref, sse)
        # a mislabel: the screen was confidently wrong; a queued row: a key
        # was off by more than its bound
        assert out["q"] == 0
        for labels in out["predict"]:
            np.testing.assert_array_equal(labels, ref["labels"])


# ---------------------------------------------------------------- a. width grid
@pytest.mark.parametrize("d", wd.WIDTHS)
def test_width_grid(d):
    X, C0, _ = wd.width_case(d)
    _check_planted(X, C0, _ref(("width", d), X, C0), **_geo(d, wd.WIDTH_K))


# ---------------------------------------------------------------- b. chunk grid
@pytest.mark.parametrize("k", list(wd.CHUNK_KP))
def test_chunk_grid(k):
    X, C0, _ = wd.chunk_case(k)
    geo = _geo(wd.CHUNK_D, k)
    assert geo["kp"] == wd.CHUNK_KP[k]
    _check_planted(X, C0, _ref(("chunk", k), X, C0), **geo)


# ------------------------------------------------------------ c. row-count edges
@pytest.mark.parametrize("n", wd.ROW_EDGES)
def test_row_count_edges(n):
    # seven of eight waves (or 31 of 32 lanes) compute on row n - 1 and drop
    # the result; below k rows some centroids own none
    X, C0, _ = wd.row_edge_case()
    X = X[:n]
    _check_planted(X, C0, _ref(("rows", n), X, C0), **_geo(260, 40))


# --------------------------------------------------------------- d. tile groups
@pytest.mark.parametrize("d,k,ps,ts", wd.GROUP_SHAPES)
def test_tile_groups(d, k, ps, ts):
    # n = 2 * 256 n_cu + 3 * 256 + 7: every workgroup makes two trips, the
    # first four a third one, and the fourth's third trip holds 7 rows in one
    # wave.  The rows repeat 1868 distinct ones (3/4 planted, 1/8 pair ties,
    # 1/8 triple ties), so the oracle runs on those and is expanded
    probe = _engine()
    n_cu = probe.info()["n_cu"]
    probe.close()
    Xb, C0, meta = wd.group_base(d, k, ps, ts)
    idx = wd.group_index(n_cu)
    assert len(idx) == wd.group_n(n_cu) > 2 * 256 * n_cu
    mult = np.bincount(idx, minlength=len(Xb))
    base = _ref(("group", d, k, n_cu), Xb, C0, mult)
    sse = orc.partition_sse(base["mind"][idx])
    ref = dict(base, labels=base["labels"][idx], sse=sse, sse_fit=sse)
    kind = meta["kind"][idx]
    X = Xb.astype(np.float32)[idx]
    out = _step_predict(X, C0, True, **_geo(d, k))
    print(f"queued {out['q_rerank']} + {out['q_full']}; tie rows {int((kind == 1).sum())} + {int((kind == 2).sum())}")
    _check_step(out, ref, True)
    for labels in out["predict"]:
        np.testing.assert_array_equal(labels, ref["labels"])
    # planted rows must be decided, tie rows cannot be (their gap is far
    # below 2 B0); a pair tie has a clear third key (kind 1: re-rank), a
    # triple tie has none (kind 2: full scan)
    assert out["q"] == int((kind != 0).sum())
    assert out["q_rerank"] == int((kind == 1).sum())
    assert out["q_full"] == int((kind == 2).sum())


# ---------------------------------------------------------- e. full segments
def test_full_segments_from_both_ends():
    # 96 tiles on 12 workgroups: one tile and a 32-entry segment per wave,
    # filled completely, 16 pairs from the front and 16 full scans from the back
    X, C0, kind = wd.segment_case()
    ref = _ref("segment", X, C0)
    for sse in (True, False):
        out = _step_predict(X, C0, sse, **_geo(wd.SEGMENT_D, 40))
        print(f"queued {out['q_rerank']} + {out['q_full']} of {len(X)}")
        _check_step(out, ref, sse)
        assert out["q"] == len(X)


# ------------------------------------------------------------------ f. resolvers
@pytest.mark.parametrize("copies", [2, 3])
@pytest.mark.parametrize("d", wd.TREE_WIDTHS)
def test_resolvers_at_every_tree_shape(d, copies):
    # centroids one float64 ulp apart: the float64 resolvers must return
    # np.argmin over np.linalg.norm bit for bit (kmeans_spark.py:153-156),
    # whose pairwise sum has remainders at other levels for each of these d
    X, C0 = wd.tree_case(d, copies)
    ref = _ref(("tree", d, copies), X, C0)
    out = _step(X, C0, True, **_geo(d, len(C0)))
    print(f"queued {out['q']} of {len(X)}")
    _check_step(out, ref, True)
    assert out["q"] > len(X) // 2


# --------------------------------------------------------------- g. numeric edges
@pytest.mark.parametrize("edge", list(wd.EDGES))
def test_numeric_edges(edge):
    n, k, make = wd.EDGES[edge]
    X, C0 = make()
    ref = _ref(("edge", edge), X, C0)
    if edge in wd.EDGE_DUPLICATE:
        assert not np.any(ref["labels"] == wd.EDGE_DUPLICATE[edge])
    out = _step(X, C0, True, **_geo(wd.EDGE_D, k))
    print(f"{edge}: queued {out['q']} of {n}")
    _check_step(out, ref, True)


# ------------------------------------------------------------ h. three iterations
@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("d,k,n", wd.ITER_SHAPES)
def test_three_iterations(d, k, n, sse):
    X, C0, _ = wd.iter_case(d, k, n)
    key = ("iter", d, k)
    if key not in _refs:
        _refs[key] = wd.lloyd(X, C0, wd.ITERS)
    eng = _load(X, C0, sse, **_geo(d, k))
    for i, ref in enumerate(_refs[key]):
        eng.assign_stats()
        st, cnt = eng.update()
        np.testing.assert_array_equal(eng.labels(), ref["labels"])
        np.testing.assert_array_equal(cnt, ref["counts"])
        assert st.n_empty == 0 and st.nonfinite == 0
        np.testing.assert_allclose(eng.get_centroids(1), ref["new"], rtol=1e-9, atol=0)
        if sse:
            print(f"iteration {i + 1}: sse {st.sse!r} vs {ref['sse']!r}")
            np.testing.assert_allclose(st.sse, ref["sse"], rtol=1e-9)
        assert eng.info()["delta_stats"] == 0
        if i + 1 < wd.ITERS:
            eng.commit()
    eng.close()


# ---------------------------------------------------------- i. dispatch boundaries
@pytest.mark.parametrize("d", [256, 257])
def test_dispatch_boundary_256_257(d):
    # the same planted columns on both sides: dp 256 is the narrow screen,
    # dp 272 k_assign_wide; each against the oracle of its own truncation
    X, C0, _ = wd.boundary_case(d)
    ref = _ref(("boundary", d), X, C0)
    for sse in (True, False):
        out = _step(X, C0, sse, **_geo(d, 40))
        _check_step(out, ref, sse)
        if d == 257:
            assert out["q"] == 0


def test_unsupported_width_is_an_error():
    # an error return: nothing is launched for d = 2049
    from kmeans_amd._lib import KmError
    rng = np.random.default_rng(12)
    X = rng.standard_normal((64, 2049)).astype(np.float32).astype(np.float64)
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    eng.set_sse(True)
    eng.set_centroids(X[:4].copy())
    assert eng.info()["path"] == 0
    with pytest.raises(KmError, match=r"no kernel for d=2049 \(supported: d <= 2048\)"):
        eng.assign_stats()
    with pytest.raises(KmError, match="unsupported geometry"):
        eng.predict()
    eng.close()
    # a supported load works afterwards
    X, C0, _ = wd.boundary_case(257)
    _check_step(_step(X, C0, True, sweeps=1, **_geo(257, 40)), _ref(("boundary", 257), X, C0), True)
