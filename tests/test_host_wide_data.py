"""The inputs of tests/test_gpu_wide.py have the properties those tests rely
on (no GPU): without them the GPU tests could pass vacuously -- planted rows
whose decision is so wide that a screen missing a feature piece would still
make it, or so narrow that a correct screen may queue them; feature pieces,
MFMA blocks or centroid chunks that no deciding pair and no winner touches;
"tie" rows that the screen could separate.
"""
import numpy as np
import pytest

import wide_data as wd
from oracle import kmeans_oracle as orc

LOW, HIGH = 3.0, 40.0     # the margin window of a planted row, in decision thresholds


def _is_f32(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


def _check_margins(X, C, meta, xabs=None):
    """Every planted row: 3 <= (k2 - k1) / thr2 and 3 <= (k3 - k1) / thr3, so
    a correct screen must decide it (each key errs by at most B0: it sees a
    gap of at least 3 thr2 - 2 B0 > thr2); a row of a pair also
    (k2 - k1) / thr2 <= 40, so an error a few bounds large changes its
    decision.  (A singleton's row -- k odd, or k = 1 -- has no partner and
    therefore no upper limit.)"""
    t = wd.thresholds(X, C, xabs=xabs)
    pl = meta["kind"][:len(X)] == 0
    own = meta["owner"][:len(X)]
    paired = pl & (own < 2 * (meta["kpl"] // 2))
    assert np.array_equal(t["first"][pl], own[pl])
    assert t["m2"][pl].min() >= LOW and t["m3"][pl].min() >= LOW, (t["m2"][pl].min(), t["m3"][pl].min())
    if paired.any():
        assert t["m2"][paired].max() <= HIGH, t["m2"][paired].max()
        # the gap is the planted one: s^2 4 delta^2
        np.testing.assert_allclose((t["k2"] - t["k1"])[paired], t["s"] ** 2 * 4.0 * meta["delta"] ** 2, rtol=1e-6)
        print(f"margin {t['m2'][paired].min():.2f} .. {t['m2'][paired].max():.2f}, delta {meta['delta']}")
    return t


def _check_planted(X, C, meta):
    """A planted input with at least k rows: the oracle's labels are the
    planted ones, every centroid owns a row, every feature piece holds a
    deciding feature, every MFMA block, register and lane half (j mod 256)
    and every centroid chunk wins a row, and the margins are in the window."""
    k, d = C.shape
    kpl = meta["kpl"]
    pl = meta["kind"] == 0
    assert _is_f32(X) and _is_f32(C[:kpl]) and len(X) >= k
    ref = wd.step(X, C)
    assert np.array_equal(ref["labels"][pl], meta["owner"][pl])
    assert ref["counts"].min() > 0
    nfc, npair = wd.nfc_of(d), kpl // 2
    f, p = meta["feature"], meta["piece"]
    assert np.all(f < d) and np.array_equal(f // wd.WIDE_FW, p)
    want = set(range(nfc)) if npair >= nfc else set(range(nfc - npair, nfc))
    assert set(p.tolist()) == want
    if npair:
        assert nfc - 1 in set(p.tolist())                                         # the last, partial piece
        last = f[p == nfc - 1]
        assert last.max() % wd.WIDE_FW // 16 == (d - 1) % wd.WIDE_FW // 16          # ... and its last K-step
    won = set(ref["labels"].tolist())
    assert {j % wd.WIDE_KC for j in won} >= set(range(min(k, wd.WIDE_KC)))
    assert {j // wd.WIDE_KC for j in won} == set(range(-(-k // wd.WIDE_KC)))
    _check_margins(X, C, meta)
    return ref


def test_threshold_restatement():
    # max(|x|, |c|) s in [2^13, 2^14) for any magnitude, and the key gap of
    # two centroids that differ by 2 delta in one feature the row shares
    for m in (1e-20, 0.7, 1.0, 9.99, 16.0, 3e9):
        s = wd.mfma_scale(m, m / 3)
        assert 2.0 ** 13 <= float(np.float32(m)) * s < 2.0 ** 14
    assert wd.mfma_scale(0.0, 0.0) == 1.0
    assert [wd.ceil_log2(v) for v in (64, 65, 128, 320, 512, 576)] == [6, 7, 7, 9, 9, 10]
    assert [wd.dp_of(d) for d in (257, 272, 273, 2033, 2048)] == [272, 272, 288, 2048, 2048]
    assert [wd.nfc_of(d) for d in (257, 300, 320, 321, 2048)] == [5, 5, 5, 6, 32]
    # B0 grows with each of its arguments (a bound that shrank would be a typo)
    b = wd.screen_b0(1e5, 1e5, 1e8, 304)
    assert b > 0 and all(wd.screen_b0(*a) > b for a in [(2e5, 1e5, 1e8, 304), (1e5, 2e5, 1e8, 304),
                                                          (1e5, 1e5, 2e8, 304), (1e5, 1e5, 1e8, 320)])


# ---------------------------------------------------------------- a. width grid
@pytest.mark.parametrize("d", wd.WIDTHS)
def test_width_grid_inputs(d):
    X, C, meta = wd.width_case(d)
    assert X.shape == (700 if d >= 1031 else 1400, d) and C.shape == (40, d) and wd.kp_of(40) == 64
    _check_planted(X, C, meta)


def test_width_grid_covers_every_last_piece_width():
    widths = {wd.dp_of(d) - (wd.nfc_of(d) - 1) * wd.WIDE_FW for d in wd.WIDTHS}
    assert widths == {16, 32, 48, 64}
    assert {wd.dp_of(d) for d in wd.WIDTHS} >= {272, 2048}
    # odd and even numbers of pieces per tile group (the buffer parity)
    assert {wd.nfc_of(d) % 2 for d in wd.WIDTHS} == {0, 1}
    # d that is no multiple of 4, within 16 of its dp
    assert any(d % 4 and wd.dp_of(d) - d < 16 for d in wd.WIDTHS)


# ---------------------------------------------------------------- b. chunk grid
@pytest.mark.parametrize("k", list(wd.CHUNK_KP))
def test_chunk_grid_inputs(k):
    X, C, meta = wd.chunk_case(k)
    assert X.shape == (max(1400, 4 * k), wd.CHUNK_D) and wd.kp_of(k) == wd.CHUNK_KP[k]
    if k // 2 >= wd.nfc_of(wd.CHUNK_D):
        _check_planted(X, C, meta)
    else:
        # k = 1, 2: too few pairs for every piece; everything else holds
        ref = wd.step(X, C)
        assert np.array_equal(ref["labels"], meta["owner"]) and ref["counts"].min() > 0
        assert _is_f32(X) and _is_f32(C)
        _check_margins(X, C, meta)


# ------------------------------------------------------------ c. row-count edges
def test_row_edge_inputs():
    X, C, meta = wd.row_edge_case()
    _check_planted(X, C, meta)
    for n in wd.ROW_EDGES:
        # max |x| is taken over the loaded rows: the scale and the bound are
        # those of the first n rows
        _check_margins(X[:n], C, meta)
        assert np.array_equal(wd.step(X[:n], C)["labels"], meta["owner"][:n])
    # one tile less one, one tile, one more; one tile group (8 waves x 32) likewise
    assert {wd.wide_layout(n, 256)["ntiles"] for n in wd.ROW_EDGES} == {1, 2, 8, 9, 16}
    assert [wd.wide_layout(n, 256)["nwt"] for n in (256, 257)] == [1, 2]


# --------------------------------------------------------------- d. tile groups
@pytest.mark.parametrize("d,k,ps,ts", wd.GROUP_SHAPES)
def test_tile_group_base(d, k, ps, ts):
    X, C, meta = wd.group_base(d, k, ps, ts)
    kind = meta["kind"]
    assert len(X) == sum(wd.GROUP_BASE) <= 2100 and len(C) == k
    assert [int((kind == i).sum()) for i in range(3)] == list(wd.GROUP_BASE)
    assert _is_f32(X)
    ref = wd.step(X, C)
    pl = kind == 0
    assert np.array_equal(ref["labels"][pl], meta["owner"][pl])
    assert ref["counts"][:meta["kpl"]].min() > 0
    t = _check_margins(X, C, meta)
    # tie rows: the top two (three) keys are far closer than 2 B0, which no
    # screen can separate; a pair tie's third key is clear, so it is a pair
    # (kind 1: re-rank) and not a full scan
    assert t["m2"][kind == 1].max() < 1e-3 and t["m3"][kind == 1].min() >= LOW
    assert t["m3"][kind == 2].max() < 1e-3
    kpl = meta["kpl"]
    assert np.all((ref["labels"][kind == 1] >= kpl) & (ref["labels"][kind == 1] < kpl + 2 * ps))
    assert np.all(ref["labels"][kind == 2] >= kpl + 2 * ps)
    npc = -(-wd.kp_of(k) // wd.WIDE_KC) * wd.nfc_of(d)
    assert npc == {40: 5, 300: 10}[k]            # odd: the buffer parity flips between groups; even: it does not


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_tile_group_row_arithmetic(n_cu):
    n = wd.group_n(n_cu)
    lay = wd.wide_layout(n, n_cu)
    assert lay["nb"] == n_cu and lay["nwt"] == 2 * n_cu + 4 and lay["seg"] == 96
    assert lay["ntiles"] == 16 * n_cu + 25
    # trips of workgroup b: tile groups b, b + nb, b + 2 nb, ...
    trips = [len(range(b, lay["nwt"], lay["nb"])) for b in range(lay["nb"])]
    assert trips[:4] == [3, 3, 3, 3] and set(trips[4:]) == {2}
    # workgroup 3's third trip: wave 0 holds 7 rows, waves 1 .. 7 none
    wt = 3 + 2 * n_cu
    rows = [max(0, min(32, n - 32 * (wt * wd.WIDE_WAVES + w))) for w in range(wd.WIDE_WAVES)]
    assert rows == [7, 0, 0, 0, 0, 0, 0, 0]
    # tie rows per (tile group, wave): every wave queues in each of its
    # trips, and both kinds fill a segment over several trips
    idx = wd.group_index(n_cu)
    assert len(idx) == n and idx.max() == sum(wd.GROUP_BASE) - 1
    kind = np.concatenate([np.full(c, i) for i, c in enumerate(wd.GROUP_BASE)])[idx]
    full = (n // 32) * 32
    per_tile = np.stack([(kind[:full].reshape(-1, 32) == i).sum(axis=1) for i in (1, 2)], axis=1)
    assert len(per_tile) == lay["ntiles"] - 1      # all but the last tile of 7 rows
    both = 0
    for b in range(4):                           # the workgroups with three trips
        for w in range(wd.WIDE_WAVES):
            tiles = [g * wd.WIDE_WAVES + w for g in range(b, lay["nwt"], lay["nb"])]
            tiles = [t for t in tiles if t < len(per_tile)]
            q = per_tile[tiles].sum(axis=0)
            assert q.sum() <= lay["seg"]
            both += int(len(tiles) >= 2 and all(per_tile[t].min() >= 1 for t in tiles))
    assert both >= 1
    # the multiplicities of the distinct rows
    mult = np.bincount(idx, minlength=sum(wd.GROUP_BASE))
    assert mult.min() >= n // sum(wd.GROUP_BASE) and mult.sum() == n


# ---------------------------------------------------------- e. full segments
def test_segment_case_rows():
    X, C, kind = wd.segment_case()
    assert X.shape == (wd.SEGMENT_N, wd.SEGMENT_D) and len(C) == 40 and _is_f32(X)
    lay = wd.wide_layout(len(X), 256)
    assert lay == {"ntiles": 96, "nwt": 12, "nb": 12, "seg": 32}
    assert np.array_equal(kind, np.tile([1, 2], wd.SEGMENT_N // 2))      # 16 + 16 per tile: qn + qf = seg
    t = wd.thresholds(X, C)
    assert t["m2"][kind == 1].max() < 1e-3 and t["m3"][kind == 1].min() >= LOW
    assert t["m3"][kind == 2].max() < 1e-3
    labels = wd.step(X, C)["labels"]
    assert np.all(labels[kind == 1] < 16) and np.all(labels[kind == 2] >= 16)


# ------------------------------------------------------------------ f. resolvers
@pytest.mark.parametrize("copies", [2, 3])
@pytest.mark.parametrize("d", wd.TREE_WIDTHS)
def test_tree_case_rows(d, copies):
    X, C = wd.tree_case(d, copies)
    assert X.shape == (wd.TREE_N, d) and len(C) == wd.TREE_SITES * copies and _is_f32(X)
    t = wd.thresholds(X, C)
    assert (t["m3"] if copies == 3 else t["m2"]).max() < 1e-3            # every row queues
    if copies == 2:
        assert t["m3"].min() >= LOW
    # the chunked oracle is np.argmin over np.linalg.norm bit for bit
    ref = wd.step(X, C)
    lf, mf = orc.assign_faithful(X, C)
    assert np.array_equal(ref["labels"], lf) and np.array_equal(ref["mind"], mf)
    # both the lower and a higher copy win rows: the float64 order decides
    assert len(set((ref["labels"] // wd.TREE_SITES).tolist())) >= 2


def test_tree_widths_reach_every_remainder_level():
    def halves(n):       # NumPy's pairwise sum: blocks of at most 128, the left half n / 2 rounded down to 8
        if n <= 128:
            return [n]
        h = (n // 2) - (n // 2) % 8
        return halves(h) + halves(n - h)
    leaves = {d: halves(d) for d in wd.TREE_WIDTHS}
    assert leaves[257] == [128, 129 // 2 - (129 // 2) % 8, 129 - 64] == [128, 64, 65]
    assert all(v == 128 for v in leaves[2048]) and len(leaves[2048]) == 16
    assert len(set(leaves[2047])) > 1 and any(v % 8 for v in leaves[2047])
    assert any(v % 8 for v in leaves[263]) and any(v % 8 for v in leaves[1031])


# --------------------------------------------------------------- g. numeric edges
@pytest.mark.parametrize("edge", list(wd.EDGES))
def test_edge_inputs(edge):
    n, k, make = wd.EDGES[edge]
    X, C = make()
    assert X.shape == (n, wd.EDGE_D) and C.shape == (k, wd.EDGE_D) and _is_f32(X)
    ref = wd.step(X, C)
    if edge in wd.EDGE_DUPLICATE:
        at = wd.EDGE_DUPLICATE[edge]
        assert np.array_equal(C[at], C[3]) and not np.any(ref["labels"] == at) and np.any(ref["labels"] == 3)
        assert at // wd.WIDE_KC == (1 if edge == "duplicate_chunks" else 0)
        assert int((ref["counts"] == 0).sum()) == 1
    else:
        assert ref["counts"].min() > 0
    if edge == "zeros":
        assert not C[2].any() and np.all(ref["labels"][::11] == 2) and not X[::11].any()
    if edge == "magnitudes":
        col = np.abs(X).max(axis=0)
        assert col[0] < 1e-7 and col[-1] > 1e3
    if edge == "far":
        assert np.abs(X).max() > 900
    # no sum cancels: a relative bound on it is a bound on the summation
    k_, d_ = C.shape
    absum = np.zeros((k_, d_))
    np.add.at(absum, ref["labels"], np.abs(X))
    own = ref["counts"] > 0
    assert np.all(np.abs(ref["sums"][own]) >= 1e-4 * absum[own])


# ------------------------------------------------------------ h. three iterations
@pytest.mark.parametrize("d,k,n", wd.ITER_SHAPES)
def test_iteration_inputs(d, k, n):
    X, C, meta = wd.iter_case(d, k, n)
    _check_planted(X, C, meta)
    refs = wd.lloyd(X, C, wd.ITERS)
    assert all(r["counts"].min() > 0 for r in refs)
    # the centroids move: the second iteration prepares new images
    assert np.abs(refs[0]["new"] - C).max() > 1e-3
    if k <= 70:     # (lloyd_fit holds n k d float64s at once)
        # (the planted labels are a fixed point: the reference's loop stops
        # after the second iteration, whose shift is 0; the third repeats it)
        fit = orc.lloyd_fit(X, k, 2, 1e-300, 0, True, 1, init_centroids=C)
        np.testing.assert_allclose(fit["centroids"], refs[1]["new"], rtol=1e-12)
        np.testing.assert_allclose(fit["sse_history"], [r["sse"] for r in refs[:2]], rtol=1e-12)
    assert np.array_equal(refs[1]["labels"], refs[2]["labels"])


# ---------------------------------------------------------- i. dispatch boundaries
def test_boundary_inputs():
    X, C, meta = wd.boundary_case(257)
    assert wd.dp_of(257) == 272
    _check_planted(X, C, meta)
    X6, C6, _ = wd.boundary_case(256)
    assert X6.shape == (1400, 256) and np.array_equal(X6, X[:, :256])
    ref = wd.step(X6, C6)
    # the pairs planted in feature 256 are exact duplicates without it: the
    # lower index takes their rows
    gone = np.nonzero(meta["feature"] == 256)[0]
    assert len(gone) >= 1
    for b in gone:
        assert np.array_equal(C6[2 * b], C6[2 * b + 1])
        assert ref["counts"][2 * b + 1] == 0 and ref["counts"][2 * b] == 70
