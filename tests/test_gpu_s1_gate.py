"""The row gate of k_s1's delta passes (csrc/km_s1_gate.h, k_s1_gate and the
gated instance of k_s1 in csrc/km_screen1.hip; DESIGN.md "Row gate").

Reference: kmeans_spark.py:147-159 (np.argmin of np.linalg.norm(C - x,
axis=1), first minimum) and :169-206 (per-cluster sums, mean update).

A row is left out of the screen only when its stored margin proves that its
label cannot have changed (Hamerly's test with rigorous rounding), so every
bar here is the one the dense kernel already meets: labels bit-identical to
the oracle's float64 argmin after every iteration, counts equal to the label
histogram, centroids at 1e-9 against the float64 means / the oracle's fit.
On top of that the gate must actually skip rows: at least half of what the
exact-distance Hamerly test skips on the same data.
"""
import numpy as np
import pytest

from oracle import kmeans_oracle as orc

pytestmark = pytest.mark.gpu

S1 = 4
SEED = 1234
D, K = 64, 256


def _engine():
    from kmeans_amd.comm import Communicator
    from kmeans_amd.engine import make_engine
    return make_engine(Communicator())


def _loaded(X, C0):
    eng = _engine()
    eng.load_host(X.astype(np.float32))
    eng.set_centroids(C0)
    return eng


def _step(eng, X, check=True, bounds=False):
    """One iteration through the engine (assign + statistics, update, commit);
    returns what it saw.  With check: the labels against the oracle at the
    centroids the pass read (orc.assign's argmin over orc.distances), the
    counts against the label histogram and the new centroids against the
    float64 means under those labels.  With bounds: also every row's two
    smallest exact distances (for the Hamerly simulation)."""
    C_prev = eng.get_centroids(0)
    eng.assign_stats()
    info = eng.info()
    labels = eng.labels()
    st, counts = eng.update()
    C_new = eng.get_centroids(1)
    eng.commit()
    out = dict(C_prev=C_prev, C_new=C_new, labels=labels, info=info, counts=counts)
    if check:
        if bounds:
            Dm = orc.distances(X, C_prev)
            ref = np.argmin(Dm, axis=1)
            part = np.partition(Dm, 1, axis=1)
            out["d1"], out["d2"] = part[:, 0].copy(), part[:, 1].copy()
        else:
            ref = orc.assign(X, C_prev)[0]
        np.testing.assert_array_equal(labels, ref)
        cnt = np.bincount(ref, minlength=len(C_prev))
        np.testing.assert_array_equal(counts, cnt)
        sums = np.zeros_like(C_prev)
        np.add.at(sums, ref, X)
        nz = cnt > 0
        np.testing.assert_allclose(C_new[nz], sums[nz] / cnt[nz, None], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(C_new[~nz], C_prev[~nz])
    return out


def _split_blobs(n=40001, seed=5):
    """64 blob centres for 256 clusters.  33 blobs hold 225 of the seeds (about
    seven each: split, their rows near the bisectors of sibling centroids and
    their centroids moving for many iterations); 31 blobs of twice the weight
    hold one seed each, so that more than half of the rows are provably
    settled once those blobs' centroids stand still."""
    rng = np.random.default_rng(seed)
    Cb = rng.uniform(-10, 10, (64, D))
    w = np.r_[np.full(31, 2.0), np.full(33, 1.0)]
    blob = rng.choice(64, n, p=w / w.sum())
    X = (Cb[blob] + rng.standard_normal((n, D))).astype(np.float32).astype(np.float64)
    lone = [int(np.nonzero(blob == b)[0][0]) for b in range(31)]
    rest = np.nonzero(blob >= 31)[0]
    C0 = X[np.r_[lone, rng.choice(rest, K - 31, replace=False)].astype(np.int64)].copy()
    return X, C0


def _hamerly_shares(X, steps):
    """Share of rows the exact-distance Hamerly test skips at each iteration
    after the first, for the centroid sequence of `steps`: bounds from exact
    float64 distances, a skipped row keeps its (loosened) bounds, every other
    row gets fresh ones.  No skipped row may change its label."""
    shares, ub, lb, lab_prev = [], None, None, None
    for s in steps:
        lab = np.asarray(s["labels"])
        if ub is not None:
            skip = (lb - ub) > 0
            assert np.all(lab[skip] == lab_prev[skip])
            shares.append(float(skip.mean()))
            ub, lb = np.where(skip, ub, s["d1"]), np.where(skip, lb, s["d2"])
        else:
            ub, lb = s["d1"].copy(), s["d2"].copy()
        lab_prev = lab
        sh = np.linalg.norm(s["C_new"] - s["C_prev"], axis=1)
        o = np.argsort(sh)[::-1]
        ub = ub + sh[lab]
        lb = lb - np.where(lab == o[0], sh[o[1]], sh[o[0]])
    return shares


@pytest.fixture(scope="module")
def split_fit():
    X, C0 = _split_blobs()
    eng = _loaded(X, C0)
    assert eng.screen() in (1, S1)
    steps = [_step(eng, X, bounds=True) for _ in range(12)]
    return X, C0, steps


def test_split_blob_fit_parity_every_iteration(split_fit):
    # every iteration's labels (oracle argmin at the centroids it read), counts
    # (label histogram) and new centroids (float64 means under the oracle's
    # labels, 1e-9) are checked in _step as the fit runs; here: the iterations
    # form one chain from C0, each reading what the last one wrote
    X, C0, steps = split_fit
    assert len(steps) == 12
    np.testing.assert_array_equal(steps[0]["C_prev"], C0)
    for a, b in zip(steps, steps[1:]):
        np.testing.assert_array_equal(b["C_prev"], a["C_new"])
    assert all(int(s["counts"].sum()) == len(X) for s in steps)


def test_split_blob_fit_gate_is_active(split_fit):
    X, C0, steps = split_fit
    n = len(X)
    infos = [s["info"] for s in steps]
    # iteration 1: full statistics; 2: the first gated pass lists every row
    assert infos[0]["delta_stats"] == 0 and infos[0]["gated_rows"] == -1
    assert infos[1]["delta_stats"] == 1 and infos[1]["gated_rows"] == n
    assert all(i["delta_stats"] == 1 and 0 < i["gated_rows"] <= n for i in infos[1:])
    assert all(0 < i["gated_rows"] < n for i in infos[6:])
    exact = _hamerly_shares(X, steps)          # iterations 2 .. 12
    dev = [1.0 - i["gated_rows"] / n for i in infos[1:]]
    print("exact Hamerly skip share:", np.round(exact, 4))
    print("device skip share:       ", np.round(dev, 4))
    assert exact[-1] > 0.5, "the data must leave the exact test something to skip"
    assert dev[-1] >= 0.5 * exact[-1]


def _small_blobs(n, centers, seed, box=10.0, std=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-box, box, (centers, D)) + offset
    return (C[rng.integers(0, centers, n)] + std * rng.standard_normal((n, D))).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def small():
    X = _small_blobs(6001, 256, seed=11)
    C0 = X[np.random.default_rng(12).choice(len(X), K, replace=False)].copy()
    return X, C0


def _warm(X, C0, iters=4):
    eng = _loaded(X, C0)
    for _ in range(iters):
        s = _step(eng, X)
    assert s["info"]["delta_stats"] == 1 and 0 < s["info"]["gated_rows"] < len(X), s["info"]
    return eng


def test_invalidation_set_centroids_mid_fit(small):
    X, C0 = small
    eng = _warm(X, C0)
    C = eng.get_centroids(0)
    eng.set_centroids(C[::-1].copy())   # every label changes its meaning
    a = _step(eng, X)
    assert a["info"]["delta_stats"] == 0 and a["info"]["gated_rows"] == -1
    b = _step(eng, X)
    assert b["info"]["delta_stats"] == 1 and b["info"]["gated_rows"] == len(X)
    c = _step(eng, X)
    assert 0 < c["info"]["gated_rows"] < len(X)


def test_invalidation_predict_between_iterations(small):
    X, C0 = small
    eng = _warm(X, C0)
    np.testing.assert_array_equal(eng.predict(), orc.assign(X, eng.get_centroids(0))[0])
    a = _step(eng, X)   # the labels are predict's: full statistics
    assert a["info"]["delta_stats"] == 0 and a["info"]["gated_rows"] == -1
    b = _step(eng, X)
    assert b["info"]["delta_stats"] == 1 and b["info"]["gated_rows"] == len(X)
    assert 0 < _step(eng, X)["info"]["gated_rows"] < len(X)


def test_invalidation_two_assign_stats_before_one_update(small):
    X, C0 = small
    eng = _warm(X, C0)
    eng.assign_stats()
    assert eng.info()["delta_stats"] == 1 and 0 < eng.info()["gated_rows"] < len(X)
    a = _step(eng, X)   # the second assign before the update: full statistics
    assert a["info"]["delta_stats"] == 0 and a["info"]["gated_rows"] == -1
    b = _step(eng, X)
    assert b["info"]["delta_stats"] == 1 and b["info"]["gated_rows"] == len(X)
    assert 0 < _step(eng, X)["info"]["gated_rows"] < len(X)


def _fit(X, C0, iters):
    import kmeans_amd as ka

    class Pinned(ka.KMeans):
        def _initialize_centroids(self, run):
            return C0.copy()

        def _empty_seed(self):
            return SEED

    km = Pinned(k=len(C0), max_iter=iters, tolerance=1e-12, compute_sse=False)
    km.verbose = False
    km.fit(X)
    return km


def test_invalidation_poor_seeds_device_repair():
    # 3 data rows + far points: 253 empties replaced on the device at
    # iteration 1; the pass right after it screens every row, later ones are
    # gated (the repair stays armed through these batches: each gated pass
    # reads the device word the repair would raise), all against the oracle's
    # whole loop (pinned repair seed)
    n = 12000
    X = _small_blobs(n, 64, seed=57)
    far = np.full((K - 3, D), 100.0) + np.arange(K - 3)[:, None]
    C0 = np.vstack([X[[0, 1, 2]], far])
    km = _fit(X, C0, 2)
    run, eng = km._runner, km._runner.engine
    assert run.device_repairs >= 1
    info = eng.info()
    assert info["delta_stats"] == 1 and info["gated_rows"] == n
    ref = orc.lloyd_fit(X, K, 2, 1e-12, 0, False, 1, init_centroids=C0, empty_seed=lambda: SEED)
    assert ref["records"][0]["empty"]
    np.testing.assert_allclose(km.centroids, ref["centroids"], rtol=1e-9, atol=1e-9)
    km.max_iter = 8
    run.run(km, None, 8, first=2)
    C7 = orc.lloyd_fit(X, K, 7, 1e-12, 0, False, 1, init_centroids=C0, empty_seed=lambda: SEED)["centroids"]
    lab = orc.assign(X, C7)[0]
    np.testing.assert_array_equal(eng.labels(), lab)
    cnt = np.bincount(lab, minlength=K)
    sums = np.zeros((K, D))
    np.add.at(sums, lab, X)
    assert np.all(cnt > 0)
    np.testing.assert_allclose(eng.get_centroids(0), sums / cnt[:, None], rtol=1e-9, atol=1e-9)
    assert 0 < eng.info()["gated_rows"] < n


@pytest.mark.parametrize("n", [1, 15, 17, 700])
def test_edges_tiny_n_and_empty_wave_segments(n):
    # fewer rows than waves (700 < the grid's waves x 16 at any n_cu: most
    # segments empty), a single partial tile, a tile and one row
    X = _small_blobs(n, 8, seed=20 + n)
    C0 = _small_blobs(K, 8, seed=40 + n)
    eng = _loaded(X, C0)
    for i in range(5):
        s = _step(eng, X)
        g = s["info"]["gated_rows"]
        assert g == -1 if i == 0 else g == n if i == 1 else 0 <= g <= n, (i, g)


def test_edges_survivor_counts_not_a_multiple_of_16(small):
    # the waves' lists end in partial tiles of every length: the per-iteration
    # parity of _step is the check; the totals below only show the case is hit
    X, C0 = small
    eng = _loaded(X, C0)
    rows = [_step(eng, X)["info"]["gated_rows"] for _ in range(8)]
    assert any(r > 0 and r % 16 for r in rows[2:]), rows


def test_edges_duplicate_centroids_and_rows_on_a_bisector():
    # A configuration that stays put, so that the ties are still there on the
    # gated passes: quarter-integer centroids, every cluster's rows in mirror
    # pairs c + v, c - v (float32-exact, so every float64 sum and mean is
    # exact and no centroid moves).  Centroid 200 duplicates centroid 10: the
    # lowest index takes the rows and their margin can never be positive.  One
    # row sits exactly halfway between centroids 20 and 100 (label 20, the
    # lowest index; its mirror image keeps cluster 20's mean in place).
    rng = np.random.default_rng(31)
    C0 = np.round(rng.uniform(-10, 10, (K, D)) * 4) / 4
    C0[200] = C0[10]
    rows = []
    for j in range(K):
        if j == 200:
            continue
        V = np.round(rng.standard_normal((8, D)) * 2) / 4
        rows += [C0[j] + V, C0[j] - V]
    mid = 0.5 * (C0[20] + C0[100])
    rows.append(np.stack([mid, 2 * C0[20] - mid]))
    X = np.concatenate(rows)
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    n = len(X)
    eng = _loaded(X, C0)
    for i in range(5):
        s = _step(eng, X)
        np.testing.assert_array_equal(s["C_new"], C0)
        assert np.all(s["labels"] != 200) and s["labels"][n - 2] == 20
        assert np.all(s["labels"][10 * 16:11 * 16] == 10)
        if i >= 2:
            # listed every time: the duplicate's 16 rows and the bisector row
            assert 17 <= s["info"]["gated_rows"] < n, s["info"]


def test_edges_a_centroid_moved_by_100(small):
    # a centroid displaced by 100 between two iterations (the host repair's
    # route: km_replace_rows on the update's new centroids, then commit): the
    # next pass lists every row and matches the oracle at the moved centroids
    X, C0 = small
    eng = _warm(X, C0)
    eng.assign_stats()
    eng.update()
    Cn = eng.get_centroids(1)
    moved = Cn[7] + 100.0 / np.sqrt(D)
    eng.replace_rows(np.array([7], dtype=np.int32), moved[None, :])
    eng.commit()
    np.testing.assert_array_equal(eng.get_centroids(0)[7], moved)
    s = _step(eng, X)
    assert s["info"]["delta_stats"] == 1 and s["info"]["gated_rows"] == len(X)
    assert 0 < _step(eng, X)["info"]["gated_rows"] <= len(X)


def test_edges_data_far_from_the_origin():
    # blobs around 1000 per coordinate (||x||^2 ~ 6e7 against within-cluster
    # distances ~ 64): the screen's bound is wide, margins mostly vanish, and
    # whatever the gate still skips must be right
    X = _small_blobs(6000, 256, seed=41, offset=1000.0)
    C0 = X[np.random.default_rng(42).choice(len(X), K, replace=False)].copy()
    eng = _loaded(X, C0)
    for _ in range(5):
        s = _step(eng, X)
    assert s["info"]["delta_stats"] == 1 and 0 < s["info"]["gated_rows"] <= len(X)
