"""The lean row gate (csrc/km_s1_gate.h "accumulated-drift form"; k_s1_gate,
k_s1_shift and the list instance of k_s1 in csrc/km_screen1.hip; DESIGN.md
"Row gate").

Reference: kmeans_spark.py:147-159 (np.argmin of np.linalg.norm(C - x,
axis=1), first minimum) and :169-206 (per-cluster sums, mean update).

What changed under the same contract: the gate reads a label and a stored base
per row and writes nothing back (the clusters' float64 running totals carry the
drift), it takes 4 consecutive rows per lane and S = 512 rows per wave and trip
(S1G_TRIP), its work-list entries carry {row, label}, and the list instance of
k_s1 reads neither the labels nor the row norms.  Every bar is the dense
kernel's: labels bit-identical to the oracle's float64 argmin after every
iteration, counts equal to the label histogram, centroids at 1e-9 against the
float64 means under those labels.  c3 geometry throughout: d = 64, k = 256.
"""
import numpy as np
import pytest

from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

S1 = 4
D, K = 64, 256
S = 512          # rows one wave takes per trip of k_s1_gate (S1G_TRIP: 2 loads of 4 rows per lane)
WAVES = 12       # waves per workgroup on this geometry


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


def _loaded(X, C0):
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    eng.set_centroids(C0)
    return eng


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _blobs(n, centers, seed, box=10.0, std=1.0):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-box, box, (centers, D))
    return _f32(C[rng.integers(0, centers, n)] + std * rng.standard_normal((n, D)))


def _check(X, C_prev, labels, counts, C_new, ref=None):
    """labels against the oracle at the centroids the pass read, counts against
    the label histogram, sums (counts x new centroids) against sum x by label"""
    if ref is None:
        ref = orc.assign(X, C_prev)[0]
    np.testing.assert_array_equal(labels, ref)
    cnt = np.bincount(ref, minlength=len(C_prev))
    np.testing.assert_array_equal(counts, cnt)
    sums = np.zeros_like(C_prev)
    np.add.at(sums, ref, X)
    nz = cnt > 0
    np.testing.assert_allclose(C_new[nz], sums[nz] / cnt[nz, None], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(C_new[~nz], C_prev[~nz])
    return ref


def _step(eng, X, nudge=None, ref=None):
    """One iteration (assign + statistics, update, commit), checked.  `nudge`
    (new centroids -> (ids, rows)) replaces centroid rows between the update
    and the commit, the host repair's route, which keeps the gate armed."""
    C_prev = eng.get_centroids(0)
    eng.assign_stats()
    info = eng.info()
    labels = eng.labels()
    _st, counts = eng.update()
    C_new = eng.get_centroids(1)
    ref = _check(X, C_prev, labels, counts, C_new, ref)
    if nudge is not None:
        ids, rows = nudge(C_new)
        eng.replace_rows(np.asarray(ids, dtype=np.int32), np.ascontiguousarray(rows))
    eng.commit()
    return dict(C_prev=C_prev, C_new=C_new, labels=labels, info=info, counts=counts, ref=ref)


def _bisector_gadget(centre):
    """34 rows and 2 centroids that stand still: quarter-integer centroids c0,
    c1, each with 8 mirror pairs c +- v, plus one row exactly halfway between
    them and its mirror image in c0.  All values are float32-exact and every
    sum exact in float64, so both means equal their centroids for ever, and
    the halfway row (label: the lower index) has margin 0: the gate lists it
    at every pass."""
    rng = np.random.default_rng(77)
    c0 = np.round(rng.uniform(-2, 2, D) * 4) / 4 + centre
    c1 = c0.copy()
    c1[:16] += 4.0
    V = np.round(rng.standard_normal((8, D)) * 2) / 4
    W = np.round(rng.standard_normal((8, D)) * 2) / 4
    mid = 0.5 * (c0 + c1)
    rows = np.concatenate([c0 + V, c0 - V, c1 + W, c1 - W, np.stack([mid, 2 * c0 - mid])])
    assert np.array_equal(rows, _f32(rows))
    return rows, np.stack([c0, c1])


# Small n: k_s1's grid gives a wave ceil(n / 16 / waves) tiles, so below
# n_cu x 12 x 16 rows every wave's segment is 16 rows (or empty, or the ragged
# last one).  These sizes run the gate's element-wise last trip alone, on
# lanes 0 .. 3, with waves that end mid-vector and empty waves; the full trips
# are test_gate_full_trips' below.
@pytest.mark.parametrize("n", [S - 1, S + 1, 2 * S + S // 2, WAVES * S * 3 + 5])
def test_gate_step_edges(n):
    G, CG = _bisector_gadget(np.r_[np.full(4, 30.0), np.zeros(D - 4)])
    Xb = _blobs(n - len(G), 8, seed=300 + n)
    rng = np.random.default_rng(400 + n)
    pos = np.sort(rng.choice(n, len(G), replace=False))   # the gadget's rows spread over the rows
    X = np.empty((n, D))
    mask = np.zeros(n, dtype=bool)
    mask[pos] = True
    X[mask], X[~mask] = G, Xb
    C0 = np.concatenate([CG, _blobs(K - 2, 8, seed=500 + n)])
    eng = _loaded(X, C0)
    assert eng.screen() in (1, S1)
    seen = []
    for i in range(6):
        s = _step(eng, X)
        g = s["info"]["gated_rows"]
        seen.append(g)
        np.testing.assert_array_equal(s["C_new"][:2], CG)
        if i == 0:
            assert g == -1, seen
        elif i == 1:
            assert g == n, seen
        else:
            assert 0 < g <= n, seen
    print("rows listed:", seen)


def _tiled_split_blobs(n, base_rows=8191, seed=5):
    """n rows that repeat a block of 8191 distinct rows (an odd period, so that
    a given row falls on every lane and trip position of the gate), fp32, and
    the block in float64: the oracle runs on the block, and a row's label is
    its block row's.  The block is test_gpu_s1_gate's split blobs: 31 blobs of
    double weight hold one seed each (their rows settle, the gate skips them),
    33 blobs share the other 225 seeds (their centroids keep moving)."""
    rng = np.random.default_rng(seed)
    Cb = rng.uniform(-10, 10, (64, D))
    w = np.r_[np.full(31, 2.0), np.full(33, 1.0)]
    blob = rng.choice(64, base_rows, p=w / w.sum())
    B = _f32(Cb[blob] + rng.standard_normal((base_rows, D)))
    lone = [int(np.nonzero(blob == b)[0][0]) for b in range(31)]
    rest = np.nonzero(blob >= 31)[0]
    C0 = B[np.r_[lone, rng.choice(rest, K - 31, replace=False)].astype(np.int64)].copy()
    B32 = B.astype(np.float32)
    reps = -(-n // base_rows)
    X32 = np.tile(B32, (reps, 1))[:n]
    return X32, B, C0


# One wave's segment is seg = ceil(n / 16 / (n_cu x 12)) x 16 rows, so n is
# sized from the device's CU count to make seg itself S - 16 (no full trip: the
# element-wise path on all 64 lanes), S + 16 (one full trip, then a tail of one
# vector of four lanes), 2 S + S / 2 (both register sets of the ping-pong, half
# a trip) and 3 S + 16 (the ping-pong wraps round to its first set).  n falls
# r = 0, 1 or 5 rows short of the grid, which ends the last wave on a vector
# boundary, one row short of it and mid-vector.
@pytest.mark.parametrize("seg,r", [(S - 16, 1), (S + 16, 0), (2 * S + S // 2, 5), (3 * S + 16, 1)])
def test_gate_full_trips(seg, r):
    probe = _engine()
    n_cu = probe.info()["n_cu"]
    probe.close()
    nw = n_cu * WAVES
    n = nw * seg - r
    assert -(-(-(-n // 16)) // nw) * 16 == seg   # k_s1's grid: every wave gets seg rows
    X32, B, C0 = _tiled_split_blobs(n)
    idx = np.arange(n) % len(B)
    mult = np.bincount(idx, minlength=len(B)).astype(np.float64)
    eng = _engine()
    eng.load_host(X32)
    del X32
    eng.set_centroids(C0)
    assert eng.screen() in (1, S1)
    seen = []
    for i in range(8):
        C_prev = eng.get_centroids(0)
        eng.assign_stats()
        info = eng.info()
        labels = eng.labels()
        _st, counts = eng.update()
        C_new = eng.get_centroids(1)
        eng.commit()
        # every row's label against the oracle's for its block row; counts and
        # sums against the block's, weighted by the rows' multiplicities
        ref = orc.assign(B, C_prev)[0]
        np.testing.assert_array_equal(labels, ref[idx])
        cnt = np.bincount(ref, weights=mult, minlength=K)
        np.testing.assert_array_equal(counts, cnt.astype(np.int64))
        sums = np.zeros((K, D))
        np.add.at(sums, ref, B * mult[:, None])
        nz = cnt > 0
        np.testing.assert_allclose(C_new[nz], sums[nz] / cnt[nz, None], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(C_new[~nz], C_prev[~nz])
        g = info["gated_rows"]
        seen.append(g)
        if i == 0:
            assert g == -1, seen
        elif i == 1:
            assert g == n, seen
        else:
            assert 0 < g <= n, seen
    print("seg", seg, "n", n, "rows listed:", seen)
    assert seen[-1] < n, seen   # kept and listed rows are mixed along the segments


def test_entries_carry_the_label():
    # 128 sites with two centroids each, 0.25 apart along the site's axis e, and
    # rows a few 1e-5 off their bisector (plus unit noise across it, in
    # antithetic pairs): the fp32 re-score cannot separate the pair, so the
    # float64 resolvers decide these rows, they keep base 0 and are listed at
    # every pass.  Each iteration the pairs are put back 0.25 apart around a
    # bisector moved by a few 1e-5, so rows between the old and the new
    # bisector change label from pass to pass -- by the resolvers, after the
    # gate has listed them with the label the previous pass's resolvers wrote.
    rng = np.random.default_rng(21)
    St = K // 2
    Gc = _f32(rng.uniform(-10, 10, (St, D)))
    e = rng.standard_normal((St, D))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    offs = np.array([-6e-5, -4e-5, -2e-5, 2e-5, 4e-5, 6e-5])
    noise = rng.standard_normal((St, len(offs), 2, D))
    noise -= (noise * e[:, None, None, :]).sum(-1, keepdims=True) * e[:, None, None, :]
    noise /= np.linalg.norm(noise, axis=-1, keepdims=True)
    base = Gc[:, None, None, :] + offs[None, :, None, None] * e[:, None, None, :]
    U = np.stack([base + noise, base - noise], axis=3).reshape(-1, D)
    X = _f32(np.concatenate([U, U[: 2 * S + 37]]))[rng.permutation(len(U) + 2 * S + 37)]
    n = len(X)

    def twins(shift):
        return _f32(np.concatenate([Gc + (shift - 0.125) * e, Gc + (shift + 0.125) * e]))

    shifts = [0.0, 3e-5, -3e-5, 5e-5, -5e-5, 1e-5, -1e-5, 0.0]
    eng = _loaded(X, twins(shifts[0]))
    changed, queued_listed = [], []
    prev = None
    for i in range(8):
        nxt = twins(shifts[(i + 1) % len(shifts)])
        s = _step(eng, X, nudge=lambda Cn, nxt=nxt: (np.arange(K), nxt))
        if prev is not None:
            changed.append(int(np.sum(prev != s["labels"])))
        prev = s["labels"]
        queued_listed.append(s["info"]["gated_rows"])
        assert int(s["counts"].sum()) == n
    print("rows that changed label per pass:", changed, "rows listed:", queued_listed)
    assert queued_listed[0] == -1 and queued_listed[1] == n
    assert all(0 < g <= n for g in queued_listed[2:])
    # the case is hit: labels do change between gated passes
    assert sum(c > 0 for c in changed[1:]) >= 4, changed


@pytest.mark.parametrize("nonfinite", [False, True])
def test_no_row_norm_read(nonfinite):
    # rows whose norm the list instance now bounds by itself: the zero row (on
    # the bisector of two centroids +-v: listed at every pass), two rows of norm
    # 1e4 next to two centroids that move at every pass, one row with a NaN and
    # one with an inf (non-finite: queued, base 0, listed at every pass; in a
    # case of their own, since an inf in the data widens the screen's bound for
    # every row).  The
    # labels must equal those of the full-statistics path (a second engine
    # given the same centroids afresh at every iteration), and the finite
    # rows' the oracle's.
    rng = np.random.default_rng(91)
    Xb = _blobs(3000, 256, seed=92)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    big = _f32(1e4 * u)
    spec = np.stack([np.zeros(D), big + _f32(0.5 * rng.standard_normal(D)), big - _f32(0.5 * rng.standard_normal(D)),
                     Xb[5].copy(), Xb[6].copy()])
    if nonfinite:
        spec[3, 7] = np.nan
        spec[4, 9] = np.inf
    at = np.array([100, 777, 1500, 2048, 2999])
    X = Xb.copy()
    X[at] = _f32(spec)
    n = len(X)
    fin = np.all(np.isfinite(X), axis=1)
    v = np.zeros(D)
    v[:4] = 1.5
    C = Xb[rng.choice(np.setdiff1d(np.arange(n), at), K, replace=False)].copy()

    def prescribed(t):
        r = np.random.default_rng(1000 + t)
        return _f32(np.stack([v * (1.0 + 0.01 * t), -v * (1.0 + 0.01 * t),
                              big + 0.3 * r.standard_normal(D), big - 0.3 * r.standard_normal(D)]))

    C[:4] = prescribed(0)
    eng = _loaded(X, C)
    full = _loaded(X, C)
    listed = []
    with np.errstate(all="ignore"):
        for t in range(6):
            C_prev = eng.get_centroids(0)
            eng.assign_stats()
            info = eng.info()
            labels = eng.labels()
            eng.update()
            C_new = eng.get_centroids(1)
            # the next centroids: the means, but the four prescribed ones, and
            # whatever the non-finite rows spoilt stays where it was
            nxt = np.where(np.isfinite(C_new).all(axis=1, keepdims=True), C_new, C_prev)
            nxt[:4] = prescribed(t + 1)
            eng.replace_rows(np.arange(K, dtype=np.int32), np.ascontiguousarray(nxt))
            eng.commit()
            full.set_centroids(C_prev)
            full.assign_stats()
            assert full.info()["delta_stats"] == 0
            np.testing.assert_array_equal(labels, full.labels())
            np.testing.assert_array_equal(labels[fin], orc.assign(X[fin], C_prev)[0])
            assert labels[at[0]] == 0          # the zero row: a tie, the lowest index
            assert set(labels[at[1:3]]) <= {2, 3}
            listed.append(info["gated_rows"])
    print("rows listed:", listed)
    assert listed[0] == -1 and listed[1] == n and all(3 <= g <= n for g in listed[2:]), listed


def test_long_fit_no_drift_then_epoch_reset():
    n = 20000
    X = _blobs(n, 256, seed=11)
    C0 = X[np.random.default_rng(12).choice(n, K, replace=False)].copy()
    eng = _loaded(X, C0)
    listed, ref, C_ref = [], None, None
    for i in range(300):
        C_prev = eng.get_centroids(0)
        # (the oracle's labels are reused while the centroids stand still)
        same = C_ref is not None and np.array_equal(C_prev, C_ref)
        s = _step(eng, X, ref=ref if same else None)
        ref, C_ref = s["ref"], C_prev
        listed.append(s["info"]["gated_rows"])
    print("rows listed at iterations 3, 10, 30, 100, 300:", [listed[i - 1] for i in (3, 10, 30, 100, 300)])
    np.testing.assert_array_equal(s["C_new"], s["C_prev"])   # converged: the shifts are 0
    assert all(0 <= g <= n for g in listed[2:])
    assert listed[299] <= listed[99] < n
    # new centroids, one of them moved by 100: full statistics, then the dense
    # sweep that starts a new epoch (every row, totals back to 0), then the gate
    C = eng.get_centroids(0)
    C[7] += 100.0 / np.sqrt(D)
    eng.set_centroids(C)
    a = _step(eng, X)
    assert a["info"]["delta_stats"] == 0 and a["info"]["gated_rows"] == -1
    b = _step(eng, X)
    assert b["info"]["delta_stats"] == 1 and b["info"]["gated_rows"] == n
    c = _step(eng, X)
    assert 0 <= c["info"]["gated_rows"] < n
