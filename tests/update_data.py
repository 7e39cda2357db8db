"""Planted statistics for tests/test_gpu_update.py and tests/test_gpu_repair.py
(stage 3 of an iteration: the all-reduced sums -> the next centroids, the
status record, the batch gate and the empty-cluster repair;
kmeans_spark.py:176-206 and :289-313).

No assign kernel runs in those tests: the statistics buffer is written by the
test ([k][d+1] sums and counts, the SSE slot, with weights k sums of weights
more) and the update reads it as it stands.  This module builds the buffers
and states what the update must make of them in a few lines of NumPy
(`reference`); tests/test_host_update_data.py proves, without a GPU, the
property that names each pattern.

What is exact and what is not
  new = S / cnt is ONE correctly rounded division per coordinate, an empty
  cluster keeps its old centroid: centroids, counts, the SSE slot, n_empty,
  nonfinite and the stop reason are compared with ==.  max_shift is
  sqrt(max_j sum_f (new - old)^2): two sums of d non-negative squares differ
  by at most 2 d u relative whatever the order or the use of fma (u = 2^-53),
  the root halves that, each root rounds once, the squares round once each:
  (d + 4) u relative (`SHIFT_RTOL`), derived, not measured.  The patterns
  whose shift is a power of two, 0 or inf in ANY order are flagged
  `exact_shift` and compared with ==.

The range edges (pattern `range`), as NumPy gives them:
  tiny  C_old and the sums near 1e-150, every coordinate moving by one ulp
        (2^-551): each square is 2^-1102, far below the smallest subnormal,
        so the squared shift underflows and max_shift is 0.0;
  huge  C_old near 1e150, the sums its negation: the squares are near 1e302
        and their sum stays below the largest float64 (d <= 2048), so
        max_shift is a finite number near 1e151, held to the derived bound;
  overflow  the same at 1e160: each square overflows, so max_shift is inf
        while every centroid is finite (nonfinite == 0, and inf < tol is
        false: the batch goes on).

A NaN sum: kmeans_spark.py:289 raises before the shifts are taken (:293), so
the reference has no max_shift for such an iteration.  The record's value is
the maximum over the clusters whose shift is a number (np.fmax), which for
NaN-free statistics is np.linalg.norm(new - old, axis=1).max() itself.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import kmeans_oracle as orc

DELTA = 2.0 ** -20
U = 2.0 ** -53
KM_MAX_BATCH = 32

# update_one_ok: k <= 64 and k d <= 16384 -> k_update_one (16 waves over the
# clusters, 64 lanes over the features); else k_update (a wave per cluster) +
# k_finalize (256 threads over the clusters)
ONE_SHAPES = [(1, 1), (3, 63), (16, 64), (17, 65), (63, 129), (64, 256), (8, 2048)]
TWO_SHAPES = [(64, 257), (65, 1), (65, 64), (255, 65), (256, 16), (257, 130), (1000, 20), (9, 2047)]
SHAPES = ONE_SHAPES + TWO_SHAPES

Case = namedtuple("Case", "k d pattern variant weighted")


def update_one_ok(k, d):
    return k <= 64 and k * d <= 16384


def shift_rtol(d):
    return (d + 4) * U


def case_id(c):
    v = "-".join(str(x) for x in c.variant) if isinstance(c.variant, tuple) else str(c.variant)
    return f"k{c.k}-d{c.d}-{c.pattern}-{v}" + ("-w" if c.weighted else "")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the reference
def reference(C_old, flat, weighted=False):
    """The record of one update of `flat` over `C_old`."""
    k, d = C_old.shape
    T = flat[:k * (d + 1)].reshape(k, d + 1)
    S, cnt = T[:, :d], T[:, d]
    div = flat[k * (d + 1) + 1:] if weighted else cnt
    assert len(div) == k
    live = cnt > 0
    new = C_old.copy()
    with np.errstate(all="ignore"):
        new[live] = S[live] / div[live][:, None]
        norms = np.linalg.norm(new - C_old, axis=1)
    return {"new": new, "counts": cnt.astype(np.int64), "sse": float(flat[k * (d + 1)]),
            "norms": norms, "shift": float(np.fmax.reduce(norms, initial=0.0)),
            "n_empty": int((cnt == 0).sum()), "nonfinite": int(not np.isfinite(new).all())}


def stop_reason(rec, tol, repaired=False):
    """KM_STOP_* of the iteration in a batch; empty clusters stop it only when
    no repair replaced them."""
    if rec["nonfinite"]:
        return 3
    if rec["n_empty"] and not repaired:
        return 2
    return 1 if rec["shift"] < tol else 0


def stats_dict(C_old, flat):
    """The reduceByKey dictionary of the same statistics (kmeans_spark.py:174)."""
    k, d = C_old.shape
    T = flat[:k * (d + 1)].reshape(k, d + 1)
    return {j: (T[j, :d].copy(), T[j, d]) for j in range(k) if T[j, d] > 0}


# -------------------------------------------------------------------- the plants
def _flat(S, cnt, sse, wsum=None):
    k, d = S.shape
    out = np.empty(k * (d + 1) + 1 + (k if wsum is not None else 0))
    T = out[:k * (d + 1)].reshape(k, d + 1)
    T[:, :d], T[:, d] = S, cnt
    out[k * (d + 1)] = sse
    if wsum is not None:
        out[k * (d + 1) + 1:] = wsum
    return out


def _exact_base(k, d, rng):
    """S = cnt C_old as integers: new == C_old bit for bit, shift 0."""
    C = rng.integers(-8, 9, (k, d)).astype(np.float64)
    cnt = rng.integers(1, 1001, k).astype(np.float64)
    return C, C * cnt[:, None], cnt


def _noise_base(k, d, rng, spread=0.5):
    C = 3.0 * rng.standard_normal((k, d))
    cnt = rng.integers(1, 5001, k).astype(np.float64)
    return C, (C + spread * rng.standard_normal((k, d))) * cnt[:, None], cnt


def movers(k, d):
    """exact_shift: the moving cluster (first, last, the stride edges of the 16
    waves and of the 256 threads) x the moving feature (first, last, the edge
    of the 64 lanes)."""
    js = sorted({j for j in (0, k - 1, 15, 16, 255, 256) if j < k})
    fs = sorted({f for f in (0, d - 1, 63, 64) if f < d})
    return [(j, f) for j in js for f in fs]


def big_ids(k):
    """big_counts: (ids of 2^31, 2^32, 2^40 + 1; the empty cluster or None).
    On k < 4 the ids coincide (the last count wins) and no cluster is left to
    be empty."""
    ids = [0, k // 2, k - 1]
    free = [j for j in range(k) if j not in ids]
    return ids, (free[0] if free else None)


BIG = (2.0 ** 31, 2.0 ** 32, 2.0 ** 40 + 1.0)


def empty_ids(k, variant):
    if variant == "ends":
        return sorted({0, k - 1})
    if variant == "alternate":
        return list(range(0, k, 2))
    assert variant == "all_but_one"
    return [j for j in range(k) if j != k // 2]


NONFINITE_VARIANTS = [(v, p, c) for v in ("inf", "nan") for p in ("last", "first")
                      for c in ("alone", "with_empty", "below_tol")]


def variants(k, d, pattern):
    if pattern == "exact_shift":
        return movers(k, d)
    if pattern in ("noise", "weighted", "big_counts"):
        return [0]
    if pattern == "empties":
        return ["ends", "alternate", "all_but_one"]
    if pattern == "nonfinite":
        return NONFINITE_VARIANTS
    assert pattern == "range"
    return ["tiny", "huge", "overflow"]


PATTERNS = ("exact_shift", "noise", "weighted", "big_counts", "empties", "nonfinite", "range")


def cases(k, d, pattern):
    return [Case(k, d, pattern, v, pattern == "weighted") for v in variants(k, d, pattern)]


def plant(case):
    """C_old [k][d], the flat statistics, the expected record (`reference`) and
    `tols`: [(tol, stop_reason of a batch iteration)].  rec["exact_shift"]: the
    shift is the same float in any summation order."""
    k, d, p, v = case.k, case.d, case.pattern, case.variant
    rng = _rng(k, d, p, v)
    sse = float(rng.uniform(1.0, 1e6))
    wsum = None
    exact = False
    tols = None
    if p == "exact_shift":
        j, f = v
        C, S, cnt = _exact_base(k, d, rng)
        cnt[j] = 4.0
        S[j] = 4.0 * C[j]
        S[j, f] = 4.0 * (C[j, f] + DELTA)
        exact = True
        tols = [DELTA, float(np.nextafter(DELTA, np.inf))]
    elif p == "noise":
        C, S, cnt = _noise_base(k, d, rng)
    elif p == "weighted":
        C, S, cnt = _noise_base(k, d, rng)
        wsum = cnt * rng.uniform(0.5, 1.5, k)
        S = S * (wsum / cnt)[:, None]
    elif p == "big_counts":
        C, S, cnt = _exact_base(k, d, rng)
        ids, e = big_ids(k)
        for j, c in zip(ids, BIG):
            cnt[j] = c
        S = C * cnt[:, None]
        if e is not None:
            cnt[e] = 0.0
        exact = True
        tols = [0.0, 1e-300]
    elif p == "empties":
        C, S, cnt = _noise_base(k, d, rng)
        cnt[empty_ids(k, v)] = 0.0          # their sums stay: an empty cluster's sums are not read
    elif p == "nonfinite":
        val, pos, combo = v
        C, S, cnt = _exact_base(k, d, rng) if combo == "below_tol" else _noise_base(k, d, rng)
        j, f = (k - 1, d - 1) if pos == "last" else (0, 0)
        S[j, f] = np.inf if val == "inf" else np.nan
        if combo == "with_empty" and k > 1:
            cnt[(j + k // 2) % k if (j + k // 2) % k != j else (j + 1) % k] = 0.0
        tols = [1.0] if combo == "below_tol" else [1e-3]
    else:
        assert p == "range"
        sign = np.where(rng.random((k, d)) < 0.5, -1.0, 1.0)
        cnt = np.ones(k)
        exact = True
        if v == "tiny":
            C = sign * rng.integers(1, 9, (k, d)) * 1e-150
            S = np.nextafter(C, np.inf)
            tols = [0.0, 5e-324]
        elif v == "huge":
            C = sign * rng.integers(1, 9, (k, d)) * 1e150
            S = -C
            exact = False
        else:
            C = sign * rng.integers(1, 9, (k, d)) * 1e160
            S = -C
            tols = [1e300]
    flat = _flat(S, cnt, sse, wsum)
    rec = reference(C, flat, wsum is not None)
    rec["exact_shift"] = exact
    if tols is None:                         # one tolerance on each side of the shift, far from it
        tols = [rec["shift"] / 2, rec["shift"] * 2]
    return {"C_old": C, "flat": flat, "rec": rec, "tols": [(t, stop_reason(rec, t)) for t in tols]}


# ------------------------------------------------------------------- the repair
# takeSample layouts: one partition; a skewed one with a one-row and a
# zero-row partition; more partitions than the 256 threads of k_rep_finish; the
# twist-block edges of tests/test_gpu_sampling.py (624 words = 312 rows)
LAYOUTS = {"one": (1000,), "skew": (313, 1, 0, 70001), "many": (7,) * 300, "twist": (624, 623, 625, 311, 312)}
SEEDS = (0, 42, 2 ** 32 + 5, 2 ** 63 - 1)
REPAIR_K = (5, 64, 65, 256, 257, 1000)
EMPTY_PATTERNS = ("first", "last", "chunk_edges", "wave_edges", "all_but_one")

RepairCase = namedtuple("RepairCase", "k d empties layout seed big")


def repair_id(c):
    return f"k{c.k}-d{c.d}-{c.empties}-{c.layout}-s{c.seed}" + ("-big" if c.big else "")


def repair_empties(k, name):
    """Ids of the planted empties.  rep_select gives thread t of 256 the ids
    [t chunk, (t + 1) chunk), chunk = ceil(k / 256); a wave is 64 threads."""
    chunk = (k + 255) // 256
    ids = {"first": [0], "last": [k - 1],
           "chunk_edges": [chunk - 1, chunk, 255, 256, 511, 512, k - 1],
           "wave_edges": list(range(63 * chunk, 65 * chunk)),
           "all_but_one": [j for j in range(k) if j != k // 2]}[name]
    return sorted({j for j in ids if j < k})


def _repair_cases():
    out = []
    names = list(LAYOUTS)
    for i, k in enumerate(REPAIR_K):
        for j, e in enumerate(EMPTY_PATTERNS):
            if repair_empties(k, e):
                out.append(RepairCase(k, (3, 17)[(i + j) % 2], e, names[(i + j) % 4], SEEDS[(i + 2 * j + j // 2) % 4],
                                      bool((i + j // 2) % 2)))
    for i, lay in enumerate(names):          # every layout under every seed
        for j, s in enumerate(SEEDS):
            c = RepairCase(257, (3, 17)[(i + j) % 2], "chunk_edges", lay, s, bool(j % 2))
            if c not in out:
                out.append(c)
    return out


REPAIR_CASES = _repair_cases()


@lru_cache(maxsize=None)
def repair_rows(total, d):
    """The dataset: small integers, the same in float32 and float64."""
    return _rng("rows", total, d).integers(-9, 10, (total, d)).astype(np.float64)


@lru_cache(maxsize=None)
def picks(layout, num, seed):
    return tuple(orc.take_sample_indices(list(layout), num, seed))


def plant_repair(k, d, empty, layout, big, nan=False):
    """Integer C_old, noisy sums for the live clusters (big: their shift
    exceeds any replacement row's; else it is far below), count 0 for `empty`;
    X = repair_rows.  Returns C_old, flat, X and the record of the plain
    update."""
    total = int(sum(layout))
    rng = _rng("repair", k, d, tuple(empty), layout, big)
    C = rng.integers(-9, 10, (k, d)).astype(np.float64)
    cnt = rng.integers(1, 5001, k).astype(np.float64)
    S = (C + (100.0 if big else 0.01) * rng.standard_normal((k, d))) * cnt[:, None]
    cnt[list(empty)] = 0.0
    if nan:
        live = [j for j in range(k) if j not in empty]
        S[live[-1], d - 1] = np.nan
    flat = _flat(S, cnt, float(rng.uniform(1.0, 1e6)))
    return {"C_old": C, "flat": flat, "X": repair_rows(total, d), "plain": reference(C, flat)}


def repaired(plan, empty, gidx):
    """The record after rows X[gidx[i]] replaced clusters empty[i]."""
    rec = dict(plan["plain"])
    new = rec["new"].copy()
    for j, g in zip(empty, gidx):
        new[j] = plan["X"][g]
    norms = np.linalg.norm(new - plan["C_old"], axis=1)
    rec.update(new=new, norms=norms, shift=float(np.fmax.reduce(norms, initial=0.0)),
               nonfinite=int(not np.isfinite(new).all()))
    return rec


# takeSample's every-row branch (num >= total): k = 9, 8 empties
EVERY_ROW_LAYOUTS = ((8,), (5,), (3, 0, 5))

# mode 2 in one process: the engine holds global rows [row0, row0 + n)
MODE2 = {"k": 65, "layout": "twist", "seed": 42, "empty": tuple(range(2, 65, 5))}


def mode2_windows(gidx):
    """Two windows around the second smallest and second largest pick g1 < g2:
    `inner` owns both as its first and last row (row0 = g1, row0 + n - 1 = g2);
    `outer` misses both by one row (row0 - 1 = g1, row0 + n = g2)."""
    s = sorted(gidx)
    g1, g2 = s[1], s[-2]
    assert g2 - g1 >= 2
    return {"inner": (g1, g2 - g1 + 1), "outer": (g1 + 1, g2 - g1 - 1)}
