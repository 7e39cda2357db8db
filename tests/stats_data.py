"""Planted integer inputs for tests/test_gpu_stats.py (stage 2 of an iteration:
labels -> per-cluster float64 sums, counts, SSE and sums of weights).

Labels come first: a label pattern lab[n] (a function of the row index) and k
integer centroids with coordinates in [-R, R] (R = 100 for d <= 32, 30
above); row i is C[lab[i]] + noise, noise in {-1, 0, 1}^d.  Every value is a
small integer (|x| <= 101: exact in fp16 and fp32), every sum, count,
weighted sum and squared residual an integer far below 2^53, so any order of
float64 additions, atomics or FMAs gives the same bits and the GPU tests
compare with assert_array_equal.  The planted label is the nearest centroid
by a wide margin (tests/test_host_stats_data.py proves it for every case, and
that each pattern has the property that names it), so stage 1 cannot blur a
stage-2 finding.

A case also carries the statistics route and table split that the dispatch
is expected to choose (km_stats_route): kr = STATS_LDS / (8 (fr + slots))
clusters of fr features per LDS table, STATS_LDS = 156 KiB, slots = 1 (the
count) or 2 with weights (sum of weights and count).
"""
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

MAX_N = 1 << 15
MAX_W = 7
MIN_GAP = 1024          # squared distance of the runner-up beyond the planted centroid
TAIL_SCALE = 2.0 ** -30  # centroid tails of the SSE-correction cases: c = m + t 2^-30, t in 1..7

# route: 0 statistics inside the assign kernel, 1 range-tiled table, 2 counting sort
# ncr x kr: cluster ranges and clusters per range; nfr x fr: feature ranges and features per range
Case = namedtuple("Case", "d k n pattern weighted tails route ncr kr nfr fr")

PATTERNS = ("balanced", "one_first", "one_last", "one_kr", "straddle", "singletons", "sorted_runs", "pair", "five",
            "lonely_first", "distinct", "tail1", "tail63")


def case_id(c):
    return (f"d{c.d}-k{c.k}-n{c.n}-{c.pattern}" + ("-w" if c.weighted else "") + ("-tails" if c.tails else ""))


def radius(d):
    return 100 if d <= 32 else 30


def rows_of(case):
    """n of the case: singletons has one row per cluster, the tail patterns a
    last partial wave of 1 and of 63 rows."""
    if case.pattern == "singletons":
        return case.k
    if case.pattern == "tail1":
        return case.n // 64 * 64 + 1
    if case.pattern == "tail63":
        return case.n // 64 * 64 + 63
    return case.n


def heavy_pair(case):
    """The two heavy clusters of `straddle`: the two sides of the first range
    boundary (kr - 1, kr); with a single cluster range there is no boundary
    and the last two ids stand in."""
    return (case.kr - 1, case.kr) if case.kr < case.k else (case.k - 2, case.k - 1)


def labels(case, rng):
    n, k, p = rows_of(case), case.k, case.pattern
    i = np.arange(n)
    g, lane = i // 64, i % 64
    if p in ("balanced", "tail1", "tail63"):
        lab = rng.permutation(i % k)
    elif p == "one_first":
        lab = np.zeros(n, dtype=np.int64)
    elif p == "one_last":
        lab = np.full(n, k - 1)
    elif p == "one_kr":
        lab = np.full(n, min(case.kr, k) - 1)
    elif p == "straddle":
        a, b = heavy_pair(case)
        h = n * 45 // 100
        rest = np.setdiff1d(np.arange(k), [a, b])
        lab = np.concatenate([np.full(h, a), np.full(h, b), rest[np.arange(n - 2 * h) % len(rest)]])
        lab = rng.permutation(lab)
    elif p == "singletons":
        lab = rng.permutation(k)
    elif p == "sorted_runs":
        lab = np.sort(rng.integers(0, k, n))
    elif p == "pair":
        lab = (2 * g + lane % 2) % k
    elif p == "five":
        lab = (5 * g + lane % 5) % k
    elif p == "lonely_first":
        lab = (2 * g + (lane > 0)) % k
    elif p == "distinct":
        lab = (64 * g + lane) % k
    else:
        raise ValueError(p)
    return lab.astype(np.int32)


def weights(n):
    """Integer weights 1..7 by row index (not constant within a cluster)."""
    i = np.arange(n)
    return (1 + (3 * i + i // 64) % MAX_W).astype(np.float64)


def tails(k, d):
    return 1 + (np.arange(k)[:, None] + np.arange(d)[None, :]) % 7


_built = {}


def build(case):
    """The case's inputs, built once and left unchanged: X float32 [n][d], the
    integer centroids M and the float64 centroids C (M, plus the tails), lab
    int32, noise int8 and w float64 (or None)."""
    if case in _built:
        return _built[case]
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    R = radius(case.d)
    M = rng.integers(-R, R + 1, (case.k, case.d))
    C = M.astype(np.float64)
    if case.tails:
        M[M == 0] = 1            # |m| >= 1: the tail is below half an fp32 ulp, the fp32 image is m
        C = M.astype(np.float64) + tails(case.k, case.d) * TAIL_SCALE
    lab = labels(case, rng)
    n = len(lab)
    # (tails: one-sided noise, so that the cross term -2 t (x - m) of the
    # residual adds up to more than the 1e-9 the SSE is held to)
    noise = rng.integers(0 if case.tails else -1, 2, (n, case.d)).astype(np.int8)
    X = (M[lab] + noise).astype(np.float32)
    out = {"X": X, "M": M, "C": C, "lab": lab, "noise": noise, "w": weights(n) if case.weighted else None}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _built[case] = out
    return out


def cluster_sums(lab, k, V):
    """Per-cluster column sums of the int64 rows V by reduceat over the
    label-sorted order (exact; np.add.at is slow for wide rows)."""
    out = np.zeros((k, V.shape[1]), dtype=np.int64)
    if len(lab) == 0:
        return out
    order = np.argsort(lab, kind="stable")
    ls = lab[order]
    starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
    out[ls[starts]] = np.add.reduceat(V[order], starts, axis=0)
    return out


_refs = {}


def reference(case):
    """Exact statistics of the planted labels in integers: counts, sums of
    (w) x, sums of weights W, the SSE (an integer; with tails the exact
    rational value rounded once to float64) and the centroids after the
    update (one NumPy division per entry; empty clusters keep theirs)."""
    if case in _refs:
        return _refs[case]
    b = build(case)
    lab, k = b["lab"], case.k
    w = np.ones(len(lab), dtype=np.int64) if b["w"] is None else b["w"].astype(np.int64)
    Xi = b["X"].astype(np.int64)
    counts = np.bincount(lab, minlength=k).astype(np.int64)
    sums = cluster_sums(lab, k, Xi * w[:, None])
    W = np.bincount(lab, weights=w, minlength=k).astype(np.int64)
    e = b["noise"].astype(np.int64)
    A = int((w * (e * e).sum(1)).sum())
    if case.tails:
        # sum w (e - t 2^-30)^2 = A - 2 B 2^-30 + T 2^-60
        t = tails(k, case.d)[lab]
        B = int((w * (e * t).sum(1)).sum())
        T = int((w * (t * t).sum(1)).sum())
        sse = float(Fraction((A << 60) - (B << 31) + T, 1 << 60))
    else:
        sse = float(A)
    new = b["C"].copy()
    live = counts > 0
    new[live] = sums[live].astype(np.float64) / W[live, None].astype(np.float64)
    ref = {"counts": counts, "sums": sums.astype(np.float64), "W": W.astype(np.float64), "sse": sse, "new": new,
           "n_empty": int((~live).sum()), "max_abs": int(max(np.abs(sums).max(), W.max(), A))}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _refs[case] = ref
    return ref


def top2(X, C):
    """(argmin, smallest and second smallest squared distance) of every row,
    by |x|^2 - 2 x.c + |c|^2 in float64 matmul chunked over k: exact for
    integer inputs of these magnitudes; np.argmin's lowest index on ties."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    n, k = len(X), len(C)
    x2 = (X * X).sum(1)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    arg = np.zeros(n, dtype=np.int64)
    step = max(64, (1 << 23) // max(n, 1))
    for j0 in range(0, k, step):
        Cc = C[j0:j0 + step]
        D = x2[:, None] - 2.0 * (X @ Cc.T) + (Cc * Cc).sum(1)[None, :]
        a = D.argmin(1)
        m1 = D[np.arange(n), a]
        if D.shape[1] > 1:
            D[np.arange(n), a] = np.inf
            m2 = D.min(1)
        else:
            m2 = np.full(n, np.inf)
        better = m1 < best          # strict: an earlier chunk keeps a tie
        second = np.where(better, np.minimum(best, m2), np.minimum(second, m1))
        arg = np.where(better, a + j0, arg)
        best = np.where(better, m1, best)
    return arg, best, second


# --------------------------------------------------------------------- cases
def _c(d, k, n, pattern, split, weighted=False, tails=False):
    return Case(d, k, n, pattern, weighted, tails, *split)


# route-1 shapes: (d, k) -> (route, ncr, kr, nfr, fr); the smallest k with the named structure
ROUTE1 = {
    (16, 1175): (1, 2, 1174, 1, 16),     # the second range holds one cluster
    (16, 2348): (1, 2, 1174, 1, 16),     # two full ranges, the last k before the sort
    (32, 1024): (1, 1, 1024, 2, 16),     # the c4 split: two feature ranges, one cluster range
    (32, 1180): (1, 2, 605, 1, 32),      # fr = 16 would need two cluster ranges as well: the widest wins
    (32, 1211): (1, 2, 1174, 2, 16),     # 2 x 2: fr = 32 would need three cluster ranges
    (40, 408): (1, 1, 408, 2, 24),       # 6 lanes per row, 4 lanes idle
    (90, 300): (1, 1, 300, 2, 48),
    (128, 200): (1, 1, 200, 2, 64),
    (180, 150): (1, 1, 150, 2, 96),
    (200, 100): (1, 1, 100, 2, 128),
    # wide rows (dp > 256) never sort
    (300, 70): (1, 1, 70, 2, 152),       # 38 lanes per row, one row per instruction
    (784, 200): (1, 1, 200, 14, 56),     # fr = 196 and 112 need two cluster ranges, 56 is the first with one
    (2000, 40): (1, 1, 40, 10, 200),
    (272, 1200): (1, 2, 1174, 17, 16),
    (2048, 80): (1, 1, 80, 16, 128),
}
ROUTE1_PATTERNS = ("one_first", "one_last", "one_kr", "straddle", "sorted_runs", "pair", "distinct")
ROUTE1_CASES = [_c(d, k, 4097 if i % 2 else 8193, "balanced", s) for i, ((d, k), s) in enumerate(ROUTE1.items())]
ROUTE1_CASES += [_c(16, 1175, n, "balanced", ROUTE1[(16, 1175)]) for n in (1, 63, 64, 65, 12289)]
ROUTE1_CASES += [_c(d, k, 4097, p, ROUTE1[(d, k)]) for d, k in ((16, 1175), (128, 200)) for p in ROUTE1_PATTERNS]

# sorted route: one shape per k_segsum<L> instance at the smallest sorting k
ROUTE2 = {
    (16, 2349): (2, 3, 1174, 1, 16),
    (32, 2349): (2, 3, 1174, 2, 16),
    (40, 1597): (2, 3, 798, 2, 24),
    (64, 2349): (2, 3, 1174, 4, 16),
    (90, 1597): (2, 3, 798, 4, 24),
    (128, 2349): (2, 3, 1174, 8, 16),
    (180, 1597): (2, 3, 798, 8, 24),
    (200, 2349): (2, 3, 1174, 16, 16),
    (128, 4096): (2, 4, 1174, 8, 16),
    (16, 16384): (2, 14, 1174, 1, 16),   # the largest k_hist / k_scatter take: 64 KiB of LDS
}
ROUTE2_SHAPES = [_c(d, k, 8193, "balanced", ROUTE2[(d, k)]) for d, k in list(ROUTE2)[:8]]
_TWO = ((16, 2349), (128, 4096))
ROUTE2_CASES = [_c(d, k, 8193, p, ROUTE2[(d, k)]) for d, k in _TWO for p in PATTERNS if p != "balanced"]
ROUTE2_CASES += [_c(128, 4096, 8193, "balanced", ROUTE2[(128, 4096)])]
# SCAT_PER = 8192 rows per k_scatter workgroup; below n_cu * 32 rows most k_segsum waves get nothing
ROUTE2_CASES += [_c(d, k, n, "balanced", ROUTE2[(d, k)]) for d, k in _TWO for n in (1, 64, 8191, 8192, 16385)]
# k_scan: three clusters per thread with the last thread partial (k = 2349), sixteen per thread (k = 16384)
ROUTE2_CASES += [_c(16, k, 20000, "balanced", ROUTE2[(16, k)]) for k in (2349, 16384)]

# weighted twins: the table row has two slots beside the features
WEIGHTED = {
    (16, 1175): (1, 2, 1109, 1, 16),
    (128, 200): (1, 1, 200, 2, 64),
    (300, 70): (1, 1, 70, 2, 152),
    (16, 2349): (2, 3, 1109, 1, 16),
    (40, 1597): (2, 3, 768, 2, 24),
    (128, 4096): (2, 4, 1109, 8, 16),
}
WEIGHTED_CASES = [_c(d, k, 4097, p, s, weighted=True) for (d, k), s in WEIGHTED.items()
                  for p in ("balanced", "one_kr", "singletons", "five")]

# SSE correction: centroids with tails below the fp32 image's resolution
TAIL_CASES = [_c(16, 1175, 4097, "balanced", ROUTE1[(16, 1175)], tails=True),
              _c(300, 70, 4097, "balanced", ROUTE1[(300, 70)], tails=True),
              _c(16, 2349, 8193, "balanced", ROUTE2[(16, 2349)], tails=True),
              _c(16, 1175, 4097, "balanced", WEIGHTED[(16, 1175)], weighted=True, tails=True),
              _c(16, 2349, 4097, "balanced", WEIGHTED[(16, 2349)], weighted=True, tails=True)]

# past the sort's capacity (k * 4 bytes > 64 KiB of LDS): the range-tiled table
BIG_K_CASES = [_c(16, 16385, 20000, "balanced", (1, 14, 1174, 1, 16)),
               _c(16, 16385, 20000, "balanced", (1, 15, 1109, 1, 16), weighted=True)]

# the fused kernel's own table (route 0)
FUSED = (0, 0, 0, 0, 0)
FUSED_CASES = [_c(64, 256, 8193, p, FUSED) for p in ("one_last", "five", "balanced")]

ALL_CASES = ROUTE1_CASES + ROUTE2_SHAPES + ROUTE2_CASES + WEIGHTED_CASES + TAIL_CASES + BIG_K_CASES + FUSED_CASES


# ---------------------------------------------------------------- bisector rows
BISECTOR_ROWS = 200


def bisector_case():
    """d = 64, k = 256, n = 8193 with 200 rows exactly on the bisector of an
    integer centroid pair: c_b = c_a + 2 e_1, row = c_a + e_1 + noise on the
    other axes.  The two distances are equal integers, so the label is the
    lower index a, as np.argmin gives; no other row belongs to a or b.
    Returns (X, C, lab, tied)."""
    d, k, n = 64, 256, 8193
    rng = np.random.default_rng(6425)
    M = rng.integers(-30, 31, (k, d))
    a, b = 100, 101
    M[b] = M[a]
    M[b, 0] += 2
    others = np.setdiff1d(np.arange(k), [a, b])
    lab = others[rng.permutation(n) % len(others)]
    tied = np.zeros(n, dtype=bool)
    tied[rng.choice(n, BISECTOR_ROWS, replace=False)] = True
    lab[tied] = a
    noise = rng.integers(-1, 2, (n, d))
    noise[tied, 0] = 1
    X = (M[lab] + noise).astype(np.float32)
    return X, M.astype(np.float64), lab.astype(np.int32), tied


# ------------------------------------------------------------------ delta folds
def delta_case(d, k, n, situation):
    """Two iterations whose label changes are planted (delta statistics: after
    the second assign the buffer holds sums(labels2) - sums(labels1)).

    Blobs of integer rows around integer centres; centroid j starts at its
    blob's centre except where a situation moves it:
      "none":  every centroid at its centre: no row moves in iteration 2;
      "one":   one row of blob 0 sits at 6 on axis 0 between the centres 0 and
               10 of blobs 0 and 1, and centroid 1 starts at 14: the row goes
               to cluster 0 first (36 < 64) and, once centroid 1 has moved to
               its blob's mean near 10, to cluster 1 (16 < ~36);
      "blob":  along axis 0 blob P at 0 (many rows), Q at 10 (few), S at 16;
               centroids 0 and 1 start at 0 and 21 and own P + Q and S; after
               the update they sit near 10 |Q| / (|P| + |Q|) and 16, and Q
               moves to cluster 1 as a whole.
    The other blobs lie far away in the other axes.  Returns (X, C0)."""
    rng = np.random.default_rng(zlib.crc32(f"delta-{d}-{k}-{n}-{situation}".encode()))
    M = rng.integers(-30, 31, (k, d))
    M[:3, 1:] = M[0, 1:]
    M[:3, 0] = (0, 10, 16)
    lab = 3 + rng.permutation(n) % (k - 3)
    sizes = {"none": (40, 40, 40), "one": (40, 40, 40), "blob": (400, 12, 40)}[situation]
    at = rng.permutation(n)
    o = 0
    for j, s in enumerate(sizes):
        lab[at[o:o + s]] = j
        o += s
    noise = rng.integers(-1, 2, (n, d))
    if situation == "blob":
        noise[lab < 3, 0] = 0  # Q exactly at 10: 100 < 121 decides iteration 1
    X = M[lab] + noise
    C0 = M.astype(np.float64)
    if situation == "one":
        X[at[0], 0] = 6
        C0[1, 0] = 14.0
        C0[2, 0] = 30.0
        X[lab == 2, 0] += 14   # blob S out of the way, at 30
    elif situation == "blob":
        C0[1] = C0[2]
        C0[1, 0] = 21.0
        C0[2, 0] = 500.0       # a centroid that owns nothing in either iteration
    return X.astype(np.float32), C0
