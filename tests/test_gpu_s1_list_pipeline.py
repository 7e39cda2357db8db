"""The list instance's entry pipeline and the lower totals in LDS (k_s1 with
GATED 1 / 2 in csrc/km_screen1.hip; DESIGN.md "Row gate / List instance").

Reference: kmeans_spark.py:147-159 (np.argmin of np.linalg.norm(C - x,
axis=1), first minimum) and :169-206 (per-cluster sums, mean update).

What is new under the same contract: a wave of the list instance fetches its
work-list entries 64 at a time (four tiles of 16), a whole group ahead, and a
tile takes its 16 by a cross-lane read; the clusters' lower totals (acc_dn)
are staged into an LDS table of kp floats at kernel start and the tail and the
re-score read them there.  Every bar is the dense kernel's: labels
bit-identical to the oracle's float64 argmin at the centroids each pass read,
counts equal to the label histogram, centroids at 1e-9 against the float64
means under those labels.  Two geometries: d = 64, k <= 256 (twelve waves per
workgroup) and d = 32, k <= 64 (eight).
"""
import numpy as np
import pytest

from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

S1 = 4
# (d, k, waves per workgroup on the geometry)
GEO12 = (64, 256, 12)
GEO8 = (32, 64, 8)


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _means_check(Xw, w, ref, counts, C_prev, C_new):
    """counts against the (weighted) label histogram, new centroids against the
    float64 means under `ref`; clusters without rows keep their centroid"""
    k = len(C_prev)
    cnt = np.bincount(ref, weights=w, minlength=k)
    np.testing.assert_array_equal(counts, cnt.astype(np.int64))
    sums = np.zeros_like(C_prev)
    np.add.at(sums, ref, Xw * w[:, None])
    nz = cnt > 0
    np.testing.assert_allclose(C_new[nz], sums[nz] / cnt[nz, None], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(C_new[~nz], C_prev[~nz])


# ---------------------------------------------------------------------------
# list-length edges
# ---------------------------------------------------------------------------
M_LIST = [0, 1, 15, 16, 17, 63, 64, 65, 127, 129]
SEG = 144            # rows per wave segment: holds the longest list, a multiple of 16


def _edge_pool(d, k, seed):
    """Distinct rows (float32-exact, float64) and the centroids they sit around.

    Centroids 0 .. k - 7 are quarter-integer points that stand still: cluster j
    has mirror pairs c_j + v, c_j - v, so its mean is c_j exactly, whatever the
    multiplicity of a pair.  Centroids 0 and 1 are siblings 16 apart (c_1 = c_0
    + 4 on the first 16 coordinates); rows mid + w with w zero on those
    coordinates are exact ties of the two (label 0, the lowest index; margin 0:
    listed at every pass), rows mid -+ 2^-10 along the axis sit within 1e-3 of
    the bisector on either side.  Each comes with its mirror image in its own
    centroid.  The last 6 centroids share one Gaussian blob: they keep moving,
    so every cluster's running total grows and the near rows' small margins
    are used up again and again.
    Returns (rows, C0, kinds) with kinds: dict name -> index array into rows;
    'tie' and 'near' rows are at even positions of their blocks, each followed
    by its mirror."""
    rng = np.random.default_rng(seed)
    ks = k - 6
    C = np.round(rng.uniform(-10, 10, (ks, d)) * 4) / 4
    C[1] = C[0]
    C[1, :16] += 4.0
    mid = 0.5 * (C[0] + C[1])
    rows, kinds, at = [], {}, 0

    def add(name, block):
        nonlocal at
        rows.append(block)
        kinds[name] = np.arange(at, at + len(block))
        at += len(block)

    V = np.round(rng.standard_normal((ks, 8, d)) * 2) / 4
    add("settled", np.stack([C[:, None, :] + V, C[:, None, :] - V], axis=2).reshape(-1, d))
    W = np.round(rng.standard_normal((192, d)) * 2) / 4
    W[:, :16] = 0.0
    tie = mid + W
    add("tie", np.stack([tie, 2 * C[0] - tie], axis=1).reshape(-1, d))
    e = np.zeros(d)
    e[:16] = 2.0 ** -12                      # |e| = 4 x 2^-12 = 2^-10 < 1e-3
    lo, hi = mid + W[:32] - e, mid + W[32:64] + e
    add("near", np.concatenate([np.stack([lo, 2 * C[0] - lo], axis=1).reshape(-1, d),
                                np.stack([hi, 2 * C[1] - hi], axis=1).reshape(-1, d)]))
    add("centre", C[2:10].copy())            # rows that are their centroid: no mean moves
    centre = np.full(d, 40.0)
    blob = _f32(centre + rng.standard_normal((10 * SEG, d)))
    add("moving", blob)
    R = np.concatenate(rows)
    assert np.array_equal(R, _f32(R))
    C0 = np.concatenate([C, blob[rng.choice(len(blob), 6, replace=False)]])
    return R, C0, kinds


@pytest.mark.parametrize("geo", [GEO12, GEO8], ids=["d64k256w12", "d32k64w8"])
def test_list_length_edges(geo):
    d, k, waves = geo
    probe = _engine()
    n_cu = probe.info()["n_cu"]
    probe.close()
    nw = n_cu * waves
    n = nw * SEG - 5                                  # the last wave's segment ends at n, mid-tile
    assert -(-(-(-n // 16)) // nw) * 16 == SEG        # k_s1's grid: every wave gets SEG rows
    R, C0, kinds = _edge_pool(d, k, seed=700 + d)
    rng = np.random.default_rng(701 + d)
    # rows as indices into the pool.  Waves 0 .. 9: the moving blob.  From wave
    # 10 on, wave w lists M_LIST[w % 10] bisector rows (every fifth a near one)
    # at random places of its segment; the last wave and every wave with
    # w % 10 == 0 none.  Everything else is filled with settled pairs and with
    # the mirrors that the bisector rows need to keep centroids 0 and 1 in place.
    idx = np.empty(nw * SEG, dtype=np.int64)
    idx[:10 * SEG] = kinds["moving"]
    free = np.ones(nw * SEG, dtype=bool)
    free[:10 * SEG] = False
    ties, nears, mirrors = kinds["tie"][0::2], kinds["near"][0::2], []
    n_tie = 0
    for w in range(10, nw):
        m = 0 if w == nw - 1 else M_LIST[w % 10]
        pos = w * SEG + rng.choice(SEG - 5 if w == nw - 1 else SEG, m, replace=False)
        pick = np.where(np.arange(m) % 5 == 4, rng.choice(nears, m), rng.choice(ties, m))
        idx[pos] = pick
        free[pos] = False
        mirrors.append(pick + 1)
        n_tie += int(np.sum(np.arange(m) % 5 != 4))
    mirrors = np.concatenate(mirrors)
    fpos = np.nonzero(free)[0]
    assert len(mirrors) < len(fpos)
    fill = np.empty(len(fpos), dtype=np.int64)
    fill[:len(mirrors)] = mirrors
    rest = len(fpos) - len(mirrors)
    pairs = rng.choice(kinds["settled"][0::2], rest // 2)
    fill[len(mirrors):len(mirrors) + 2 * (rest // 2)] = np.stack([pairs, pairs + 1], axis=1).ravel()
    if rest % 2:
        fill[-1] = kinds["centre"][0]
    idx[fpos] = fill[rng.permutation(len(fill))]
    idx = idx[:n]
    mult = np.bincount(idx, minlength=len(R)).astype(np.float64)
    eng = _engine()
    eng.load_host(R.astype(np.float32)[idx])
    eng.set_centroids(C0)
    assert eng.screen() in (1, S1)
    seen = []
    for i in range(6):
        C_prev = eng.get_centroids(0)
        eng.assign_stats()
        info = eng.info()
        labels = eng.labels()
        _st, counts = eng.update()
        C_new = eng.get_centroids(1)
        eng.commit()
        ref = orc.assign(R, C_prev)[0]
        np.testing.assert_array_equal(labels, ref[idx])
        _means_check(R, mult, ref, counts, C_prev, C_new)
        g = info["gated_rows"]
        seen.append(g)
        if i == 0:
            assert g == -1, seen
        elif i == 1:
            assert g == n, seen
        else:
            # the list path is the one under test, and every exact tie is on it
            assert 0 < g < n and g >= n_tie, (seen, n_tie)
    print("n", n, "waves", nw, "exact ties", n_tie, "rows listed:", seen)
    assert np.all(labels[idx == ties[0]] == 0)


# ---------------------------------------------------------------------------
# the lower totals' table in LDS
# ---------------------------------------------------------------------------
def _blobs(n, d, centers, seed, box=10.0, std=1.0):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-box, box, (centers, d))
    return _f32(C[rng.integers(0, centers, n)] + std * rng.standard_normal((n, d)))


def _pass(eng, X, ref_labels=None, nudge=None):
    """One iteration, checked: labels against the oracle at the centroids the
    pass read (or against `ref_labels`), counts and means under those labels"""
    C_prev = eng.get_centroids(0)
    eng.assign_stats()
    info = eng.info()
    labels = eng.labels()
    _st, counts = eng.update()
    C_new = eng.get_centroids(1)
    ref = orc.assign(X, C_prev)[0] if ref_labels is None else ref_labels(C_prev)
    np.testing.assert_array_equal(labels, ref)
    _means_check(X, np.ones(len(X)), ref, counts, C_prev, C_new)
    if nudge is not None:
        ids, rows = nudge(C_prev, C_new)
        eng.replace_rows(np.asarray(ids, dtype=np.int32), np.ascontiguousarray(rows))
    eng.commit()
    return dict(info=info, labels=labels, C_prev=C_prev, C_new=C_new)


@pytest.mark.parametrize("d,k", [(64, 250), (64, 256), (32, 33), (32, 64)])
def test_lower_totals_table(d, k):
    # k below and at the padded count kp (256 / 64): the table's pads are never
    # indexed, its last entry, label k - 1, is
    n = 6001
    X = _blobs(n, d, k, seed=900 + k)
    C0 = X[np.random.default_rng(901 + k).choice(n, k, replace=False)].copy()
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    eng.set_centroids(C0)
    assert eng.screen() in (1, S1)
    listed = []
    for i in range(4):
        s = _pass(eng, X)
        listed.append(s["info"]["gated_rows"])
    assert listed[0] == -1 and listed[1] == n and all(0 < g <= n for g in listed[2:]), listed
    assert np.any(s["labels"] == k - 1)
    # a NaN centroid through the repair's route (the gate stays armed): the
    # pass that reads it sees a non-finite shift, lists every row and stores
    # every base against the lower image 0.  The oracle's argmin takes the NaN
    # distance (np.argmin: the first NaN), so every row goes to cluster j; the
    # update makes its centroid the mean of all rows, and the repair's route
    # then puts it back where it was
    j = 3
    s = _pass(eng, X, nudge=lambda Cp, Cn: ([j], np.full((1, d), np.nan)))
    with np.errstate(all="ignore"):
        a = _pass(eng, X, nudge=lambda Cp, Cn: ([j], s["C_new"][j][None, :]))
    assert np.all(a["labels"] == j)
    assert a["info"]["delta_stats"] == 1 and a["info"]["gated_rows"] == n, a["info"]
    assert np.all(np.isfinite(eng.get_centroids(0)))
    # the centroid is finite again, the reference copy it is measured from is
    # not: one more non-finite shift, every row listed, oracle parity
    b = _pass(eng, X)
    assert b["info"]["delta_stats"] == 1 and b["info"]["gated_rows"] == n, b["info"]
    c = _pass(eng, X)
    assert c["info"]["delta_stats"] == 1 and 0 <= c["info"]["gated_rows"] <= n, c["info"]
    assert np.any(c["labels"] == k - 1)
    # new centroids: full statistics, then the dense sweep with margins starts
    # a new epoch (every row, totals 0), then the list instance
    C = eng.get_centroids(0)
    eng.set_centroids(C[::-1].copy())
    e0 = _pass(eng, X)
    assert e0["info"]["delta_stats"] == 0 and e0["info"]["gated_rows"] == -1
    e1 = _pass(eng, X)
    assert e1["info"]["delta_stats"] == 1 and e1["info"]["gated_rows"] == n
    e2 = _pass(eng, X)
    assert 0 <= e2["info"]["gated_rows"] < n      # (a converged fit lists no row at all)
    assert np.any(e2["labels"] == k - 1)


# ---------------------------------------------------------------------------
# drift: a long fit that never converges
# ---------------------------------------------------------------------------
def _one_split_blob(n=10001, shared=12, seed=5):
    """test_gpu_s1_gate's split blobs with the split concentrated: 244 blobs
    hold one seed each and 65 % of the rows (they settle at once, the gate
    skips them), one blob with 35 % of the rows is shared by 12 seeds.  About
    290 rows per moving centroid keep Lloyd's iteration going far longer than
    that module's 33 blobs of 7 seeds do: float64 Lloyd on the host stops
    moving after 7 iterations on those at 10,001 rows and after 20 at 40,001,
    and moves for more than 70 on these, so all 40 passes of the drift test
    see the running totals grow."""
    d, k = 64, 256
    rng = np.random.default_rng(seed)
    nl = k - shared
    Cb = rng.uniform(-10, 10, (nl + 1, d))
    Cb[nl] += 30.0
    w = np.r_[np.full(nl, 0.65 / nl), 0.35]
    blob = rng.choice(nl + 1, n, p=w)
    X = _f32(Cb[blob] + rng.standard_normal((n, d)))
    lone = [int(np.nonzero(blob == b)[0][0]) for b in range(nl)]
    rest = np.nonzero(blob == nl)[0]
    C0 = X[np.r_[lone, rng.choice(rest, shared, replace=False)].astype(np.int64)].copy()
    return X, C0


def test_drift_40_iterations_split_blobs():
    import test_gpu_s1_gate as tg

    X, C0 = _one_split_blob()
    n = len(X)
    eng = tg._loaded(X, C0)
    assert eng.screen() in (1, S1)
    steps = [tg._step(eng, X, bounds=True) for _ in range(40)]   # parity at every iteration, in _step
    for a, b in zip(steps, steps[1:]):
        np.testing.assert_array_equal(b["C_prev"], a["C_new"])
    # never converging: every one of the 40 updates moves a centroid, so every
    # gated pass tests the stored bases against totals that have grown
    moved = [not np.array_equal(s["C_new"], s["C_prev"]) for s in steps]
    assert all(moved), moved
    infos = [s["info"] for s in steps]
    assert infos[0]["gated_rows"] == -1 and infos[1]["gated_rows"] == n
    assert all(i["delta_stats"] == 1 and 0 < i["gated_rows"] <= n for i in infos[1:])
    assert all(0 < i["gated_rows"] < n for i in infos[6:])       # the list instance, on a real subset
    exact = tg._hamerly_shares(X, steps)                         # iterations 2 .. 40
    dev = [1.0 - i["gated_rows"] / n for i in infos[1:]]
    print("exact Hamerly skip share:", np.round(exact[5::6], 4))
    print("device skip share:       ", np.round(dev[5::6], 4))
    assert exact[-1] > 0.5, "the data must leave the exact test something to skip"
    # the existing bar of test_split_blob_fit_gate_is_active, held at every
    # iteration from the twelfth on
    for t in range(10, len(exact)):
        assert dev[t] >= 0.5 * exact[t], (t, dev[t], exact[t])
