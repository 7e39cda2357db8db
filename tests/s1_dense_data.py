"""Inputs that keep k_s1's re-scoring ring full for many tiles per wave, and
the CPU checks that they do (tests/test_gpu_s1_dense.py, tests/test_host_s1_dense.py).

k_s1 (csrc/km_screen1.hip) sends a row with 2..8 candidate centroids to its
wave's ring; the ring fill, the queue cursors and the change-list cursor are
carried from one 16-row tile of the wave to the next.  The data here makes
(nearly) every row such a row, for as many tiles per wave as wanted:

  * S well separated sites G_i; a twin site carries two centroids, C[i] and
    C[St + i] (exact duplicates, float64 one-ulp duplicates, or near twins
    G_i -+ (delta / 2) e_i), a single site one centroid;
  * rows G_i + t e_i + n with a few offsets t along e_i and noise n orthogonal
    to e_i in antithetic pairs (n, -n): with equal weights on a pair the
    cluster means stay on the axis, so the twins stay ~delta apart after every
    update and the rows stay ring rows in every iteration;
  * a few thousand DISTINCT rows, repeated and permuted to n rows: the float64
    oracle runs on the distinct rows (`weighted_lloyd`), the kernel on all n.

`check_ring_rows` restates the kernel's own quantities on the CPU (the greedy
chain colouring of k_s1_color, the screen bound E = e1 ||x|| + e0 of
k_s1_prep, the fp32 re-score's bound width of k_s1's `decide`) and asserts,
with safety factors over them, that every twin-site row has exactly its two
twins as candidates, in different chains, and no open chain.  The factors 4, 8
and 10 are margins over the kernel's bounds, not measured values.
"""
import functools

import numpy as np

from oracle import kmeans_oracle as orc

U24 = 2.0 ** -24
U16 = 2.0 ** -11
TILE = 16
ORACLE_CHUNK = 256  # rows per block of the oracle's [rows][k][d] differences (k = 1000: 65 MB)


# -- the kernel's geometry (km_screen1.hip: s1_waves, s1_ring) -------------------------------

def geometry(d, k):
    dp = 32 * -(-d // 32)
    kp = 64 * -(-k // 64)
    waves = 12 if (dp, kp) in ((64, 256), (32, 1024)) else 8
    return {"dp": dp, "kp": kp, "ns2": dp // 32, "nb": kp // 32, "waves": waves, "ring": 12 if waves == 12 else 16}


def rows_for_tiles(d, k, n_cu, tiles_per_wave, ragged=7):
    """n = T n_cu waves 16 + 7: every wave of a full grid takes T tiles (and
    one wave a ragged last tile)."""
    return tiles_per_wave * n_cu * geometry(d, k)["waves"] * TILE + ragged


# -- restatements of k_s1_color and k_s1_prep -----------------------------------------------

def color_chains(C, nb):
    """chain (0..31) of every centroid: k_s1_color's greedy colouring.  In
    index order centroid j joins the non-full chain whose members' smallest
    fp32 squared distance to it is largest (an empty chain counts as +inf;
    ties: the lowest chain).  The distances are the kernel's fp32 fma chain in
    feature order (the square is exact in float64, so each step rounds once
    to float64 and once to fp32: the fp32 fma up to double rounding)."""
    C32 = np.asarray(C, dtype=np.float64).astype(np.float32)
    k, d = C32.shape
    D = np.zeros((k, k), dtype=np.float32)
    for f in range(d):
        df = (C32[:, None, f] - C32[None, :, f]).astype(np.float64)
        D = (df * df + D.astype(np.float64)).astype(np.float32)
    chain = np.full(k, -1, dtype=np.int64)
    cnt = np.zeros(32, dtype=np.int64)
    for j in range(k):
        cmin = np.full(32, np.inf, dtype=np.float32)
        if j:
            np.minimum.at(cmin, chain[:j], D[:j, j])
        c = int(np.argmax(np.where(cnt < nb, cmin, np.float32(-1.0))))  # first maximum: the lowest chain
        assert cnt[c] < nb
        chain[j] = c
        cnt[c] += 1
    return chain


def screen_bound(C, X, d, k):
    """(s, e1, e0): k_s1_prep's scale and screen error bound, E(x) = e1 ||x|| + e0
    on the keys s^2 (||c||^2 - 2 c.x)."""
    g = geometry(d, k)
    C = np.asarray(C, dtype=np.float64)
    cm = float(np.sqrt((C * C).sum(1)).max()) * (1.0 + 1e-6)
    ca = float(np.abs(C).max()) * (1.0 + U24) * (1.0 + 1e-6)
    xa = float(np.abs(X).max())
    m = max(xa, ca)
    s = 2.0 ** (14 - np.frexp(m)[1]) if 0.0 < m < 3.0e38 else 1.0
    s2, sq, nm = s * s, np.sqrt(g["dp"]) * 1.0001, float(g["ns2"])
    e1 = 1.25 * (2.0 * s2 * cm * (2.0 * U16 + U16 * U16 + 2.0 * U24) +
                 nm * 4.0 * U24 * 2.0 * s2 * cm * (1.0 + 2.0 * U16) +
                 2.0 ** -25 * s * sq * (1.0 + U16))
    e0 = 1.25 * (U24 * s2 * cm * cm + nm * (4.0 * U24 * s2 * cm * cm +
                                            28.0 * U24 * 2.0 * s2 * ca * xa * (1.0 + U16) * (1.0 + U16)) +
                 2.0 ** -24 * s * sq * cm)
    return s, e1 * 1.0001, e0 * 1.0001 + 1e-30


# -- the data -----------------------------------------------------------------------------------

DELTA = 0.25
# offsets t of the rows along e_i, and the shift of a fit's initial twins,
# G + (shift -+ DELTA / 2) e: off-centre, so that the twins' bisector crosses
# one or two offsets in each of the next two iterations (1-d 2-means on the
# offsets; no offset on a bisector).  Eight offsets where k is small, four
# where 2 k rows per offset already make thousands of distinct rows
PATTERNS = {8: ((-0.35, -0.25, -0.15, -0.05, 0.06, 0.16, 0.25, 0.35), 0.325),
            4: ((-0.3, 0.1, 0.2, 0.3), 0.225)}


class Dense:
    """Distinct rows U (float64 values of fp32 rows), centroids C, and for
    every distinct row its site; twin site i < St has centroids i and St + i,
    single site St + j has centroid 2 St + j."""

    def __init__(self, d, k, kind, n_single, seed, scale, pattern):
        assert kind in ("exact", "ulp", "near")
        assert (k - n_single) % 2 == 0
        rng = np.random.default_rng(seed)
        self.d, self.k, self.kind = d, k, kind
        offsets, self.shift = PATTERNS[pattern]
        St = self.St = (k - n_single) // 2
        S = St + n_single
        self.delta = DELTA * scale
        G = rng.uniform(-10.0, 10.0, (S, d)).astype(np.float32).astype(np.float64)
        e = rng.standard_normal((S, d))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        self.G, self.e = G, e
        if kind == "exact":
            twins = (G[:St], G[:St])
        elif kind == "ulp":
            twins = (G[:St], np.nextafter(G[:St], np.inf))
        else:
            twins = self.twins_at(0.0)
        self.C = np.concatenate([twins[0], twins[1], G[St:]])
        assert self.C.shape == (k, d)
        # rows: site-major, offset, then the antithetic pair (adjacent rows)
        noise = rng.standard_normal((S, len(offsets), d))
        noise -= (noise * e[:, None, :]).sum(-1, keepdims=True) * e[:, None, :]
        noise /= np.linalg.norm(noise, axis=-1, keepdims=True)
        t = np.asarray(offsets, dtype=np.float64) * scale
        base = G[:, None, :] + t[None, :, None] * e[:, None, :]
        U = np.stack([base + noise, base - noise], axis=2).reshape(-1, d)
        self.U = U.astype(np.float32).astype(np.float64)
        self.site = np.repeat(np.arange(S), 2 * len(offsets))
        self.scale = scale

    def twins_at(self, shift):
        """near twins G + (shift -+ delta / 2) e, rounded to fp32"""
        St = self.St
        lo = self.G[:St] + (shift - 0.5 * self.delta) * self.e[:St]
        hi = self.G[:St] + (shift + 0.5 * self.delta) * self.e[:St]
        return lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)

    def fit_start(self):
        """off-centre initial centroids of a fit (near twins only)"""
        assert self.kind == "near"
        lo, hi = self.twins_at(self.shift * self.scale)
        return np.concatenate([lo, hi, self.G[self.St:]])

    @property
    def twin_rows(self):
        return self.site < self.St


@functools.lru_cache(maxsize=None)
def dense(d, k, kind, n_single=0, seed=0, scale=1.0, pattern=8):
    return Dense(d, k, kind, n_single, seed, scale, pattern)


def expand(n_distinct, n, seed):
    """`inverse`: n row indices into the distinct rows, permuted.  Every
    distinct row is repeated n // U times and the remainder goes to the first
    rows in order, so the two rows of an antithetic pair (adjacent) get the
    same multiplicity, but for at most one pair."""
    order = np.arange(n_distinct)
    reps, rem = divmod(n, n_distinct)
    inv = np.concatenate([np.tile(order, reps), order[:rem]])
    assert len(inv) == n
    return np.random.default_rng(seed).permutation(inv)


# -- preconditions ------------------------------------------------------------------------------

def check_ring_rows(ds, C=None, kind=None, chains=None):
    """Assert on the CPU that k_s1 sends every twin-site row of `ds` through its
    ring at centroids C (default ds.C), and decides every single-site row by the
    screen alone.  `chains`: colourings (color_chains) that must all separate
    the twins, default C's own (a fit recolours once per batch of iterations,
    so any of the batch's centroid sets may be the one coloured).  Returns a
    dict of the tightest margins met."""
    C = ds.C if C is None else np.asarray(C, dtype=np.float64)
    kind = ds.kind if kind is None else kind
    U, St, k, d = ds.U, ds.St, ds.k, ds.d
    g = geometry(d, k)
    a, b = np.arange(St), St + np.arange(St)
    # (a) every twin pair in different chains
    if chains is None:
        chains = [color_chains(C, g["nb"])]
    for ch in chains:
        assert np.all(np.bincount(ch, minlength=32) <= g["nb"])
        assert np.all(ch[a] != ch[b]), "a twin pair shares a chain: change the seed"
    # exact scores s^2 (||c||^2 - 2 c.x) and the screen bound E(x)
    s, e1, e0 = screen_bound(C, U, d, k)
    K = (s * s) * ((C * C).sum(1)[None, :] - 2.0 * (U @ C.T))
    xn = np.sqrt((U * U).sum(1)) * (1.0 + 1e-6)
    E = e1 * xn + e0
    rows = np.arange(len(U))
    tw = ds.twin_rows
    si = ds.site
    own = np.where(tw, si, 2 * St + (si - St))       # first (or only) centroid of the row's site
    sec = np.where(tw, St + si, own)                 # its twin
    ka, kb = K[rows, own], K[rows, sec]
    best = np.minimum(ka, kb)
    # (b) the twins within E / 4 of each other, everything else 8 E above the best
    assert np.all(np.abs(ka - kb) <= 0.25 * E), float(np.max(np.abs(ka - kb) / E))
    rest = K.copy()
    rest[rows, own] = np.inf
    rest[rows, sec] = np.inf
    other = rest.min(1)
    assert np.all(other >= best + 8.0 * E), float(np.min((other - best) / E))
    # (d) no chain holds two centroids within 8 E of a row's best: no open chain
    close = K <= (best + 8.0 * E)[:, None]
    assert np.all(close.sum(1) == np.where(tw, 2, 1))
    for ch in chains:
        per = np.zeros((len(U), 32), dtype=np.int64)
        r, c = np.nonzero(close)
        np.add.at(per, (r, ch[c]), 1)
        assert per.max() <= 1
    out = {"twin_gap_over_E": float(np.max(np.abs(ka - kb) / E)), "rest_over_E": float(np.min((other - best) / E)),
           "E_unscaled": float(E.max() / (s * s))}
    da = np.sqrt(((U - C[own]) ** 2).sum(1))
    db = np.sqrt(((U - C[sec]) ** 2).sum(1))
    if kind == "near":
        # (c) decided by the fp32 re-score (kind 0): the distances differ by 10 x
        # its bound width 80 u dist + 2 u cmax
        cmax = float(np.sqrt((C * C).sum(1)).max())
        width = 80.0 * U24 * np.maximum(da, db) + 2.0 * U24 * cmax
        ratio = np.abs(da - db)[tw] / width[tw]
        assert np.all(ratio >= 10.0), float(ratio.min())
        out["near_gap_over_width"] = float(ratio.min())
    else:
        # duplicates: equal fp32 images, so the re-score cannot separate them
        # (kind 1, the float64 pair re-rank)
        C32 = C.astype(np.float32)
        assert np.array_equal(C32[a], C32[b])
    return out


# -- the float64 oracle on distinct rows with multiplicities -------------------------------------

def weighted_lloyd(U, w, C0, iters, tol=1e-12):
    """Lloyd iterations of the rows U repeated w times each, in float64:
    labels from the oracle's assign on U, means sum w x / sum w, SSE
    sum w mind^2, the oracle's stop rule.  No cluster may go empty."""
    C = np.array(C0, dtype=np.float64, copy=True)
    k, d = C.shape
    w = np.asarray(w, dtype=np.float64)
    out = {"centroids": [C.copy()], "labels": [], "sse_history": [], "counts": []}
    for _ in range(iters):
        lab, mind, _gap = orc.assign(U, C, chunk=ORACLE_CHUNK)
        sums = np.zeros((k, d))
        np.add.at(sums, lab, U * w[:, None])
        cnt = np.bincount(lab, weights=w, minlength=k)
        assert np.all(cnt > 0), "a cluster went empty: the oracle here has no repair"
        new = sums / cnt[:, None]
        out["labels"].append(lab)
        out["counts"].append(cnt.astype(np.int64))
        out["sse_history"].append(float(np.sum(w * mind * mind)))
        shift = float(np.max(np.linalg.norm(new - C, axis=1)))
        C = new
        out["centroids"].append(C.copy())
        if shift < tol:
            break
    return out


@functools.lru_cache(maxsize=None)
def fit_case(d, k, seed=0, scale=1.0, iters=4, n=None, pattern=8):
    """A near-twin fit of n rows (default: every distinct row once): the data,
    its start, `inverse`, the weighted oracle at the rows' multiplicities, and
    precondition (e): at least two iterations after the first move >= 5% of the
    rows while every twin-site row stays a ring row at every pass's centroids
    (under the colouring of any of them)."""
    ds = dense(d, k, "near", 0, seed, scale, pattern)
    C0 = ds.fit_start()
    inverse = expand(len(ds.U), len(ds.U) if n is None else n, seed + 1)
    w = np.bincount(inverse, minlength=len(ds.U))
    ref = weighted_lloyd(ds.U, w, C0, iters)
    assert len(ref["labels"]) == iters
    cents = ref["centroids"][:iters]  # the centroids each pass reads
    chains = [color_chains(Cc, geometry(d, k)["nb"]) for Cc in cents]
    margins = [check_ring_rows(ds, Cc, chains=chains) for Cc in cents]
    moved = [float(np.average(ref["labels"][i] != ref["labels"][i - 1], weights=w)) for i in range(1, iters)]
    assert sum(m >= 0.05 for m in moved) >= 2, moved
    return ds, C0, inverse, ref, {"moved": moved, "margins": margins}


def blobs(n, d, centers, seed, box=10.0, std=1.0):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-box, box, (centers, d))
    lab = rng.integers(0, centers, n)
    return (C[lab] + std * rng.standard_normal((n, d))).astype(np.float32).astype(np.float64)
