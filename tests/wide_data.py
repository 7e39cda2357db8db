"""Inputs for the wide-row tests (256 < d <= 2048: k_assign_wide and its
resolver instances k_rerank2<true> and k_fullscan<2, true>), plain NumPy, no
GPU.  tests/test_host_wide_data.py checks the properties the GPU tests rely
on; tests/test_gpu_wide.py runs them.

Every generator returns float64 arrays whose rows are float32-representable
(the engine stores float32 rows and the oracle reads the same values).

The main input is `planted`: centroids in pairs that differ in one feature of
a chosen feature piece, by a step whose effect on the screen's keys is a few
times the screen's own decision threshold (restated here from k_assign_wide,
mfma_scale and screen_b0 of km_kernels.hip).  A correct screen decides every
such row, and a screen that loses a feature piece, a K-step or a centroid
block ties or flips the rows of the pairs planted there.  Well-separated blobs
would not show that: their key gaps are thousands of thresholds wide.
"""
import numpy as np

import small_path_data as spd
from oracle import kmeans_oracle as orc

WIDE_FW = 64        # features per piece (four K-steps of 16)
WIDE_KC = 256       # centroids per chunk
WIDE_WAVES = 8      # waves per workgroup, one 32-row tile each per trip
U24 = 2.0 ** -24


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def dp_of(d):
    return (d + 15) // 16 * 16


def kp_of(k):
    return (k + 63) // 64 * 64


def nfc_of(d):
    return -(-dp_of(d) // WIDE_FW)


def _sites(rng, nb, d):
    """Site means, float32-representable, every coordinate uniform in
    +-[1, 10] (a cluster's sum then never cancels)."""
    return _f32(rng.uniform(1.0, 10.0, (nb, d)) * rng.choice([-1.0, 1.0], (nb, d)))


# ----------------------------------------------------------------- the kernel's bound
def mfma_scale(xabs, cabs):
    """s = 2^(14 - e) with max(xabs, cabs) < 2^e (mfma_scale)."""
    m = np.float32(max(xabs, cabs))
    if not (m > 0) or not (m < np.float32(3.0e38)):
        return 1.0
    _, e = np.frexp(m)
    return float(np.ldexp(1.0, 14 - int(e)))


def screen_b0(xn_s, cm_s, pm_s, dp):
    """screen_b0 of km_kernels.hip in its 32x32x16 shape (chain_err: 3 dp / 16
    MFMAs per block chain), evaluated in float64."""
    nm = 3.0 * dp / 16.0
    sq = np.sqrt(float(dp))
    slope = 1.5 * ((6.5 * 2.0 ** -22 + 0.5 * U24) * cm_s + nm * 2.0 * U24 * cm_s + U24 * sq)
    icpt = 1.5 * (U24 * cm_s * cm_s + nm * U24 * cm_s * cm_s + nm * 28.0 * U24 * pm_s + 2.0 * U24 * sq * cm_s)
    return slope * xn_s + icpt


def ceil_log2(v):
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def thresholds(X, C, xabs=None):
    """The decision of k_assign_wide for every row of X, restated in float64:
    the three smallest scaled keys K_j = s^2 (||c_j||^2 - 2 c_j.x) among the
    kp centroids (the pad rows carry ||c||^2 s^2 = 1e30 and a zero image, as
    k_prep_split writes them), the index of the smallest, and
    thr2 = 2 B0 + rho (|k1| + |k2|), thr3 likewise.  xabs: max |x| over the
    loaded rows where X is only a part of them."""
    k, d = C.shape
    dp, kp = dp_of(d), kp_of(k)
    xabs = float(np.abs(X).max()) if xabs is None else float(xabs)
    cabs = float(np.abs(C.astype(np.float32)).max())
    s = mfma_scale(xabs, cabs)
    cn2 = (C * C).sum(axis=1)
    cm = (float(np.float32(np.sqrt(cn2.max()))) * 1.0001 + 1e-30) * s
    pm = (cabs * s) * (xabs * s) * 1.0001
    xn = s * np.sqrt((X * X).sum(axis=1)) * 1.0001
    B0 = screen_b0(xn, cm, pm, dp)
    rho = 2.0 ** (ceil_log2(kp) - 2 - 23) * 1.01
    K = np.full((len(X), max(kp, 3)), 1e30)
    K[:, :k] = s * s * (cn2[None, :] - 2.0 * (X @ C.T))
    first = np.argmin(K, axis=1)
    part = np.partition(K, 2, axis=1)[:, :3]
    k1, k2, k3 = part[:, 0], part[:, 1], part[:, 2]
    thr2 = 2.0 * B0 + rho * (np.abs(k1) + np.abs(k2))
    thr3 = 2.0 * B0 + rho * (np.abs(k1) + np.abs(k3))
    return {"s": s, "B0": B0, "k1": k1, "k2": k2, "k3": k3, "thr2": thr2, "thr3": thr3, "first": first,
            "m2": (k2 - k1) / thr2, "m3": (k3 - k1) / thr3}


# ---------------------------------------------------------------------- tie sites
def tie_block(rng, d, sites, copies, n, std=0.5):
    """(C, X, site): `sites` site means, each with `copies` centroids one
    float64 ulp apart in every coordinate (base, then all second copies, then
    all third ones, as np.concatenate([base, up, ...]) orders them), and n
    rows dealt round-robin to the sites.  No fp32 bound separates the copies:
    float64, in NumPy's order, decides every such row."""
    m = _sites(rng, sites, d)
    base = m + 0.05 * rng.standard_normal(m.shape)
    cs = [base]
    for _ in range(copies - 1):
        cs.append(np.nextafter(cs[-1], np.inf))
    site = np.arange(n) % sites
    X = _f32(m[site] + std * rng.standard_normal((n, d)))
    return np.concatenate(cs), X, site


def ulp_ties(n, d, sites, copies, seed):
    """(X, C0): every row a tie among `copies` centroids one ulp apart."""
    rng = np.random.default_rng(seed)
    C, X, _ = tie_block(rng, d, sites, copies, n, std=1.0)
    return X, C


# ------------------------------------------------------------------ planted pairs
def pair_piece(b, npair, nfc):
    """The feature piece of pair b: b mod nfc.  With fewer pairs than pieces
    (k = 40 at dp 2048: 20 pairs, 32 pieces) the pairs count from the last
    piece down instead, so that the last piece -- the one whose width varies
    -- always holds one."""
    return b % nfc if npair >= nfc else nfc - 1 - b


def planted(n, d, k, seed=3, target=10.0, ties=(0, 0), tie_rows=(0, 0)):
    """(X, C0, meta): k centroids, n planted rows followed by the tie rows.

    The first kpl = k - 2 ties[0] - 3 ties[1] centroids are planted: pairs
    (2b, 2b + 1) = m_b -+ delta e_f around well-separated sites m_b, plus one
    singleton (index kpl - 1) when kpl is odd.  Pair b's feature f lies in
    feature piece `pair_piece` (the previous piece if that one holds no
    feature below d), the pairs of a piece taking its K-steps in turn, the
    last one first; delta is a power of two and m_b[f] a multiple of 2^-10,
    so the centroids are float32-representable.  Planted row i belongs to centroid
    i mod kpl: the centroid plus 0.5 standard normal noise in every feature
    but f, where it equals the centroid exactly -- the squared distances to
    the two members of the pair differ by exactly 4 delta^2, and delta is the
    power of two that brings s^2 4 delta^2 nearest to `target` times the
    median decision threshold thr2 of these rows (`thresholds`).

    Behind them sit ties[0] pair-tie sites and ties[1] triple-tie sites
    (`tie_block`) with tie_rows[0] and tie_rows[1] rows.  meta: "kind" per row
    (0 planted, 1 pair tie, 2 triple tie), "owner" (the planted centroid of a
    planted row, -1 elsewhere), "feature" and "piece" per pair, "delta"."""
    rng = np.random.default_rng(seed)
    dp = dp_of(d)
    nfc = nfc_of(d)
    kpl = k - 2 * ties[0] - 3 * ties[1]
    assert kpl >= 0 and (kpl > 0 or n == 0)
    npair, single = kpl // 2, kpl % 2
    m = _sites(rng, npair + single, d)
    feat = np.zeros(npair, dtype=np.int64)
    piece = np.zeros(npair, dtype=np.int64)
    for b in range(npair):
        p = pair_piece(b, npair, nfc)
        while p * WIDE_FW >= d:
            p -= 1
        lo, hi = p * WIDE_FW, min((p + 1) * WIDE_FW, d)
        ns = -(-(hi - lo) // 16)                   # K-steps of the piece that hold a feature below d
        t = (ns - 1 - b // nfc) % ns               # the piece's pairs take its K-steps in turn, the last one first
        feat[b] = rng.integers(lo + 16 * t, min(lo + 16 * t + 16, hi))
        piece[b] = p
        m[b, feat[b]] = np.round(m[b, feat[b]] * 1024.0) / 1024.0
    noise = 0.5 * rng.standard_normal((n, d))
    owner = np.arange(n) % max(kpl, 1)
    paired = owner < 2 * npair
    noise[paired, feat[owner[paired] // 2]] = 0.0
    Ct1, Xt1, _ = tie_block(rng, d, ties[0], 2, tie_rows[0]) if ties[0] else (np.zeros((0, d)), np.zeros((0, d)), None)
    Ct2, Xt2, _ = tie_block(rng, d, ties[1], 3, tie_rows[1]) if ties[1] else (np.zeros((0, d)), np.zeros((0, d)), None)

    def build(delta):
        C = np.empty((kpl, d))
        C[0:2 * npair:2] = m[:npair]
        C[1:2 * npair:2] = m[:npair]
        C[2 * np.arange(npair), feat] -= delta
        C[2 * np.arange(npair) + 1, feat] += delta
        if single:
            C[kpl - 1] = m[npair]
        X = _f32(C[owner] + noise) if n else np.zeros((0, d))
        return np.concatenate([X, Xt1, Xt2]), np.concatenate([C, Ct1, Ct2])

    delta = 1.0
    if npair and n:
        for _ in range(4):
            X, C = build(delta)
            t = thresholds(X[:n][paired], C, xabs=np.abs(X).max())
            want = target * float(np.median(t["thr2"])) / t["s"] ** 2     # 4 delta^2 in the data's units
            new = 2.0 ** int(np.round(0.5 * np.log2(want / 4.0)))
            if new == delta:
                break
            delta = new
    X, C = build(delta)
    assert np.array_equal(C[:kpl], _f32(C[:kpl])) and dp >= d
    kind = np.concatenate([np.zeros(n, dtype=np.int64), np.full(len(Xt1), 1), np.full(len(Xt2), 2)])
    own = np.concatenate([owner[:n], np.full(len(Xt1) + len(Xt2), -1)])
    meta = {"kind": kind, "owner": own, "feature": feat, "piece": piece, "delta": delta, "kpl": kpl}
    return X, C, meta


# --------------------------------------------------------------- the GPU file's cases
# a. width grid: (d, n), k = 40
WIDTHS = [257, 272, 273, 288, 300, 305, 320, 321, 519, 784, 1031, 2033, 2047, 2048]
WIDTH_K = 40


def width_case(d):
    return planted(700 if d >= 1031 else 1400, d, WIDTH_K, seed=3)


# b. chunk grid: d = 260, k -> kp
CHUNK_D = 260
CHUNK_KP = {1: 64, 2: 64, 33: 64, 64: 64, 65: 128, 256: 256, 257: 320, 300: 320, 512: 512, 513: 576}


def chunk_case(k):
    return planted(max(1400, 4 * k), CHUNK_D, k, seed=3)


# c. row-count edges: the first n rows of one planted input
ROW_EDGES = [1, 31, 32, 33, 255, 256, 257, 511]


def row_edge_case():
    return planted(1400, 260, 40, seed=4)


# d. tile groups: (d, k, pair-tie sites, triple-tie sites); 1400 planted rows
# (3/4 of the distinct rows), 234 pair-tie and 234 triple-tie rows (1/8 each)
GROUP_SHAPES = [(260, 40, 2, 2), (260, 300, 4, 4)]
GROUP_BASE = (1400, 234, 234)


def group_n(n_cu):
    return 2 * 256 * n_cu + 3 * 256 + 7


def group_base(d, k, ps, ts):
    """The distinct rows of the tile-group case and their centroids."""
    return planted(GROUP_BASE[0], d, k, seed=5, ties=(ps, ts), tie_rows=GROUP_BASE[1:])


def group_index(n_cu, seed=6):
    """Row i of the tile-group input is base[perm[i % len(base)]]."""
    nbase = sum(GROUP_BASE)
    perm = np.random.default_rng(seed).permutation(nbase)
    return perm[np.arange(group_n(n_cu)) % nbase]


def wide_layout(n, n_cu):
    """The launch geometry of k_assign_wide: tiles, tile groups, workgroups
    and the queue segment of a wave (launch_assign_mfma)."""
    ntiles = (n + 31) // 32
    nwt = (ntiles + WIDE_WAVES - 1) // WIDE_WAVES
    nb = min(nwt, n_cu)
    return {"ntiles": ntiles, "nwt": nwt, "nb": nb, "seg": 32 * ((nwt + nb - 1) // nb)}


# e. full segments: every row a tie row, pair and triple ties alternating
SEGMENT_N, SEGMENT_D = 3072, 300


def segment_case():
    X, C, meta = planted(0, SEGMENT_D, 40, seed=7, ties=(8, 8), tie_rows=(SEGMENT_N // 2, SEGMENT_N // 2))
    order = np.empty(SEGMENT_N, dtype=np.int64)
    order[0::2] = np.arange(SEGMENT_N // 2)
    order[1::2] = SEGMENT_N // 2 + np.arange(SEGMENT_N // 2)
    return X[order], C, meta["kind"][order]


# f. resolvers: d at every shape of NumPy's pairwise tree; (copies -> k, kp)
TREE_WIDTHS = [257, 263, 519, 1031, 1032, 2047, 2048]
TREE_N, TREE_SITES = 1200, 24


def tree_case(d, copies):
    return ulp_ties(TREE_N, d, TREE_SITES, copies, seed=11 + d + copies)


# g. numeric edges at d = 300
def magnitudes(n, d, k, seed):
    return spd.feature_magnitudes(n, d, k, seed)


def zeros(n, d, k, seed):
    """Blobs with every 11th row all zero and centroid 2 all zero: it owns
    the zero rows at distance exactly 0, and the rows of its own blob."""
    X, C0 = spd.blobs(n, d, k, seed)
    X[::11] = 0.0
    C0 = C0.copy()
    C0[2] = 0.0
    return X, C0


def duplicate(n, d, k, seed, at):
    """Blobs with an exact copy of centroid 3 at index `at`: np.argmin keeps 3."""
    X, C0 = spd.blobs(n, d, k, seed)
    C0 = C0.copy()
    C0[at] = C0[3]
    return X, C0


def far(n, d, k, seed):
    return spd.far_from_origin(n, d, k, seed)


EDGE_D = 300
EDGES = {
    "magnitudes": (1400, 70, lambda: magnitudes(1400, EDGE_D, 70, 21)),
    "zeros": (1400, 70, lambda: zeros(1400, EDGE_D, 70, 22)),
    "duplicate": (1400, 70, lambda: duplicate(1400, EDGE_D, 70, 23, 68)),
    "duplicate_chunks": (1500, 300, lambda: duplicate(1500, EDGE_D, 300, 24, 290)),
    "far": (1400, 70, lambda: far(1400, EDGE_D, 70, 25)),
}
EDGE_DUPLICATE = {"duplicate": 68, "duplicate_chunks": 290}

# h. three iterations: (d, k, n)
ITER_SHAPES = [(330, 70, 1400), (260, 300, 1500)]
ITERS = 3


def iter_case(d, k, n):
    return planted(n, d, k, seed=8)


# i. dispatch boundary: one planted input of 257 columns, truncated
def boundary_case(d):
    X, C, meta = planted(1400, 257, 40, seed=3)
    return np.ascontiguousarray(X[:, :d]), np.ascontiguousarray(C[:, :d]), meta


# ------------------------------------------------------------------------ the oracle
def step(X, C, mult=None):
    """One assignment and update in the oracle's terms (orc.assign in chunks
    of 128 rows: its default of 4096 holds n k d float64s at once): labels,
    counts, sums (accumulated in long double), SSE and the new centroids (an
    empty cluster keeps its centroid, as km_update does).  mult: how often
    each row occurs (the tile-group input repeats its distinct rows); the
    counts and sums are then weighted by it, and the SSE is left to the
    caller, who knows the order of the repeats."""
    k = len(C)
    labels, mind, _ = orc.assign(X, C, chunk=128)
    w = np.ones(len(X), dtype=np.int64) if mult is None else np.asarray(mult, dtype=np.int64)
    sums = np.zeros(C.shape, dtype=np.longdouble)
    np.add.at(sums, labels, X.astype(np.longdouble) * w[:, None])
    counts = np.bincount(labels, weights=w, minlength=k).astype(np.int64)
    new = C.copy()
    own = counts > 0
    new[own] = (sums[own] / counts[own, None]).astype(np.float64)
    sse = orc.partition_sse(mind) if mult is None else None
    return {"labels": labels, "counts": counts, "sums": sums.astype(np.float64), "sse": sse, "sse_fit": sse,
            "new": new, "mind": mind}


def lloyd(X, C0, iters):
    out, C = [], C0
    for _ in range(iters):
        out.append(step(X, C))
        C = out[-1]["new"]
    return out
