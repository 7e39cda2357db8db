"""Inputs for the small-path tests (k <= 32, d <= 64: k_assign_small), plain
NumPy, no GPU.  tests/test_host_small_path_data.py checks the properties the
GPU tests rely on; tests/test_gpu_small_instances.py runs them.

Every generator returns float64 arrays whose rows are float32-representable
(the engine stores float32 rows and the oracle reads the same values).
"""
import numpy as np

QUEUE_GROUPS = [0, 1, 31, 32, 33, 64] * 6 + [64, 64, 0, 5]       # 40 waves, n = 2560
FOLD_GROUPS = [0, 1, 31, 32, 33, 64] * 16 + [64, 5, 0, 12]        # 100 waves, n = 6400

# (d, k) of every tie_rows input of the GPU file, by test group
QUEUE_SHAPES = [(17, 2), (33, 3), (50, 17), (64, 32), (48, 32), (2, 31)]
FOLD_SHAPES = [(17, 32), (33, 5), (50, 17), (64, 32), (64, 1)]
MANY_SHAPES = [(64, 4), (20, 4)]


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _means(rng, nb, d, box):
    """Blob means, float32-representable, every coordinate at least 1 from
    zero (a cluster's sum then never cancels: a relative bound on it is a
    bound on the summation, not on luck)."""
    m = rng.uniform(1.0, max(box, 2.0), (nb, d)) * rng.choice([-1.0, 1.0], (nb, d))
    return _f32(m)


def tie_rows(d, k, groups, seed, box=5.0, std=0.5):
    """(X, C0, tied) with n = 64 len(groups) rows.

    Centroids come in pairs m +- e_0 at indices (2b, 2b + 1), plus one
    singleton (index k - 1) when k is odd; m is float32-representable.  In the
    g-th aligned block of 64 rows the first groups[g] rows belong to a paired
    blob and have x_0 = m_0 exactly: (x_0 - c_0)^2 = 1 for both centroids of
    the pair and every other term is shared, an exact float64 tie that
    np.argmin gives to the lower index.  Every other row keeps
    |x_0 - m_0| >= 0.05.  For d <= 4 the means sit on a lattice
    (m_0 = 10 (b + 1), other features 3): random means in so few dimensions
    let another pair's centroid come closer than the row's own pair.
    With k = 1 there is no pair and no row is tied."""
    rng = np.random.default_rng(seed)
    npair, single = k // 2, k % 2
    nb = npair + single
    if d <= 4:
        m = np.full((nb, d), 3.0)
        m[:, 0] = 10.0 * (np.arange(nb) + 1)
    else:
        m = _means(rng, nb, d, box)
    n = 64 * len(groups)
    tied = np.zeros(n, dtype=bool)
    if npair:
        for g, cnt in enumerate(groups):
            tied[64 * g: 64 * g + cnt] = True
    blob = rng.integers(0, nb, n)
    if npair:
        blob[tied] = rng.integers(0, npair, int(tied.sum()))
    noise = std * rng.standard_normal((n, d))
    # |x_0 - m_0| >= 0.0625 before the float32 rounding of x_0 (|x_0| < 2^9:
    # the rounding moves it by less than 2^-15), so >= 0.05 after it
    noise[:, 0] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.0625 + np.abs(noise[:, 0]))
    noise[tied, 0] = 0.0
    X = _f32(m[blob] + noise)
    X[tied, 0] = m[blob[tied], 0]
    e0 = np.zeros(d)
    e0[0] = 1.0
    C0 = np.empty((k, d))
    C0[0:2 * npair:2] = m[:npair] + e0
    C0[1:2 * npair:2] = m[:npair] - e0
    if single:
        C0[k - 1] = m[nb - 1]
    return X, C0, tied


def many_rows_groups(n_cu):
    """groups for n = 256 * 8 * n_cu + 777 rows (every thread of the capped
    grid takes one row, the first 777 threads a second one): tied rows in the
    first 13 blocks and in the 13 blocks past the grid's first trip, which
    the same waves visit, so that a wave's queue fills across its two trips
    (20 + 20, 31 + 1, 32 + 0, 0 + 33, 5 + 27, ..., 4 + 22), and a sparse pattern in
    between.  Returns (groups, n); the caller truncates to n rows."""
    threads = 256 * 8 * n_cu
    n = threads + 777
    nblk = -(-n // 64)
    groups = [[0, 1, 0, 2, 0, 0, 33, 0][g % 8] for g in range(nblk)]
    head = [20, 31, 32, 0, 5, 16, 30, 1, 64, 4, 12, 3, 28]
    tail = [20, 1, 0, 33, 27, 16, 3, 31, 64, 22, 21, 30, 9]
    groups[:13] = head
    first = threads // 64
    groups[first:first + 13] = tail
    return groups, n


def many_rows_case(d, n_cu, seed=5):
    groups, n = many_rows_groups(n_cu)
    X, C0, tied = tie_rows(d, 4, groups, seed)
    return X[:n], C0, tied[:n]


def blobs(n, d, k, seed, box=10.0, std=1.0):
    """(X, C0): k blobs, rows dealt round-robin, initial centroids the true
    means moved by 0.05 std."""
    rng = np.random.default_rng(seed)
    m = _means(rng, k, d, box)
    X = _f32(m[np.arange(n) % k] + std * rng.standard_normal((n, d)))
    C0 = m + 0.05 * std * rng.standard_normal((k, d))
    return X, C0


def far_from_origin(n, d, k, seed):
    return blobs(n, d, k, seed, box=1000.0, std=1.0)


def feature_magnitudes(n, d, k, seed):
    """Blobs whose f-th feature is scaled by 10**linspace(-9, 3, d)[f]."""
    X, C0 = blobs(n, d, k, seed)
    s = 10.0 ** np.linspace(-9, 3, d)
    return _f32(X * s), C0 * s


def zero_rows_and_centroids(n, d, k, seed):
    """Blobs with every 11th row all zero, centroid 2 all zero (it owns the
    zero rows at distance exactly 0) and, for k > 5, centroid 5 all zero too
    (an exact duplicate of it that must stay empty)."""
    X, C0 = blobs(n, d, k, seed)
    X[::11] = 0.0
    C0 = C0.copy()
    C0[2] = 0.0
    if k > 5:
        C0[5] = 0.0
    return X, C0


def duplicate_centroids(n, d, k, seed):
    """Blobs with exact copies of centroid 3 at index 10 (k > 10) and k - 1:
    every row of blob 3 ties exactly between them; np.argmin keeps 3."""
    X, C0 = blobs(n, d, k, seed)
    C0 = C0.copy()
    for j in duplicate_indices(k):
        C0[j] = C0[3]
    return X, C0


def duplicate_indices(k):
    return [j for j in (10, k - 1) if 3 < j < k]


def ulp_duplicates(n, d, k, seed):
    """nb = k // 2 blobs; centroid j + nb is centroid j moved one float64 ulp
    up in every coordinate (plus one centroid of its own blob when k is odd).
    No fp32 bound separates such a pair: float64, in NumPy's order, decides
    every row."""
    nb = k // 2
    rng = np.random.default_rng(seed)
    m = _means(rng, nb + k % 2, d, 10.0)
    X = _f32(m[np.arange(n) % len(m)] + rng.standard_normal((n, d)))
    base = m + 0.05 * rng.standard_normal(m.shape)
    C0 = np.empty((k, d))
    C0[:nb] = base[:nb]
    C0[nb:2 * nb] = np.nextafter(base[:nb], np.inf)
    if k % 2:
        C0[k - 1] = base[nb]
    return X, C0


FP32_RANGE_SCALES = [1e20, 1e-25]


def fp32_range(n, d, k, seed, scale):
    """Blobs scaled by 1e20 or 1e-25: the rows and centroids are ordinary
    float32 numbers, but (x - c)^2 overflows (underflows) float32 while
    float64, and so the reference, stays finite and resolves every row."""
    X, C0 = blobs(n, d, k, seed)
    return _f32(X * scale), C0 * scale
