"""k-means|| seeding (Bahmani et al. 2012, "Scalable K-Means++"; the default
initialisation of Spark MLlib): ``KMeans(..., init="k-means||")``.

The reference's only initialisation is ``takeSample`` of k random rows
(kmeans_spark.py:58-82, ``sampling.py``); this module is the alternative.
The passes over the rows run on the GPU (``km_seed_*``, csrc/km_seed.hip);
the round loop, the NumPy form of the pick rule and the weighted recluster
are here.

The algorithm, fixed exactly (rows are the stored float32 rows; everything is
keyed by global row index, so the outcome does not depend on how the rows are
spread over ranks, except through the rounding of phi):

1. First candidate: the row ``sampling.take_sample(global_sizes, 1, seed)``
   returns.  Candidate ids are assigned in order of discovery, from 0.
2. State per local row: ``D2[i]`` (float64, +inf) and ``near[i]`` (int32, -1).
3. Update with a batch ``Cnew`` of m new candidates, ids
   ``first_id .. first_id + m - 1``:
   ``j = np.argmin(np.linalg.norm(Cnew - x, axis=1))`` (the reference's
   assignment rule: the exact kernels of the Lloyd iteration);
   ``t = np.add.reduce((Cnew[j] - x) * (Cnew[j] - x))`` in float64 (NumPy's
   pairwise order, no fused multiply-add);
   ``if t < D2[i]: D2[i], near[i] = t, first_id + j``.
   The strict ``<`` lets the earliest candidate keep ties, and a NaN never
   replaces a value.  phi is the sum of D2 over every rank's rows.
4. Rounds r = 1 .. init_rounds: the row with global index g is picked iff
   ``u * phi < ell * D2[i]`` (both products rounded in float64),
   ``u = (h >> 11) * 2**-53``,
   ``h = splitmix64(splitmix64(seed64 ^ (r * 0xD1B54A32D192ED03 mod 2**64)) ^ g)``,
   ``seed64 = seed mod 2**64``, ``ell = oversampling`` (default 2 k).  The
   ranks' picks, gathered in rank order (ascending global indices), are the
   round's batch for step 3.  A round without picks moves on; ``phi == 0``
   ends the rounds; a non-finite phi raises
   ``ValueError("Data contains NaN or Inf values")``.
5. Weights: ``w[j]`` = rows with ``near == j`` (device histogram, summed over
   ranks).
6. Recluster on the host (``recluster``): weighted k-means++ over the M
   candidates in float64 with ``np.random.RandomState(seed mod 2**32)``.
7. Fewer than k candidates: the rows of ``take_sample(global_sizes, k, seed)``
   in order, skipping global indices that are candidates already, top up.
8. N < k raises the reference's
   ``Not enough data points (N) to initialize k clusters``.
"""
from __future__ import annotations

import time
from typing import List, Tuple

import numpy as np

from . import sampling

MASK64 = 2 ** 64 - 1
ROUND_MULT = 0xD1B54A32D192ED03


def splitmix64(z: int) -> int:
    """The hash of csrc/km_internal.h (``k_gen_blobs``, ``k_seed_sample``)."""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _splitmix64_np(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def round_key(seed: int, rnd: int) -> int:
    """``splitmix64(seed64 ^ (r * ROUND_MULT mod 2**64))``: the round's key."""
    return splitmix64((int(seed) & MASK64) ^ ((int(rnd) * ROUND_MULT) & MASK64))


def uniforms(seed: int, rnd: int, gidx) -> np.ndarray:
    """u in [0, 1) of the rows with global indices ``gidx`` in round ``rnd``."""
    g = np.asarray(gidx, dtype=np.int64).astype(np.uint64)
    h = _splitmix64_np(np.uint64(round_key(seed, rnd)) ^ g)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pick_rule(d2: np.ndarray, seed: int, rnd: int, global_row0: int, ell: float, phi: float) -> np.ndarray:
    """Step 4 over one rank's rows in NumPy (what ``km_seed_sample`` computes):
    local indices, ascending."""
    d2 = np.asarray(d2, dtype=np.float64)
    u = uniforms(seed, rnd, np.arange(len(d2), dtype=np.int64) + int(global_row0))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.nonzero(u * float(phi) < float(ell) * d2)[0].astype(np.int64)


def _draw(rs: np.random.RandomState, p: np.ndarray) -> int:
    """An index with probability proportional to p (non-negative, sum > 0)."""
    c = np.cumsum(p)
    j = min(int(np.searchsorted(c, rs.random_sample() * c[-1], side="right")), len(p) - 1)
    while p[j] == 0:  # the product rounded up to the total
        j -= 1
    return j


def recluster(cands: np.ndarray, w: np.ndarray, k: int, seed: int) -> List[int]:
    """Step 6: weighted k-means++ over the candidates.  The first centre is
    drawn with p ~ w, each next one with p ~ w * (min squared distance to the
    centres chosen so far); when that total is 0 the not-yet-chosen candidate
    with the lowest id is taken.  Returns min(k, M) distinct candidate ids in
    the order chosen."""
    C = np.asarray(cands, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    M = len(C)
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    chosen: List[int] = []
    taken = np.zeros(M, dtype=bool)
    mind2 = np.full(M, np.inf)
    diff = np.empty_like(C)   # reused: the loop is k passes over the M candidates
    for _ in range(min(k, M)):
        if not chosen:
            p = w.copy()
        else:
            p = w * mind2
            p[taken] = 0.0
        total = float(p.sum())
        if total > 0.0 and np.isfinite(total):
            j = _draw(rs, p)
        else:
            j = int(np.nonzero(~taken)[0][0])
        chosen.append(j)
        taken[j] = True
        np.subtract(C, C[j], out=diff)
        np.multiply(diff, diff, out=diff)
        np.minimum(mind2, np.add.reduce(diff, axis=1), out=mind2)
    return chosen


def _fold(run, rows: np.ndarray, first_id: int) -> float:
    """Step 3 for one batch on every rank; the global phi."""
    run.engine.set_centroids(np.asarray(rows, dtype=np.float64))
    phi = float(run.comm.allreduce_np(np.array([run.engine.seed_update(first_id)], dtype=np.float64))[0])
    if not np.isfinite(phi):
        raise ValueError("Data contains NaN or Inf values")
    return phi


def kmeans_parallel(run, k: int, seed: int, rounds: int, oversampling=None) -> Tuple[np.ndarray, dict]:
    """Steps 1-8 on the rows ``run`` (a ``kmeans.LloydRunner``) holds: the k
    initial centroids (float64 [k][d]) and ``{"rounds", "candidates"}`` with
    the wall time of the rounds and of the recluster.
    Every rank calls it with the same arguments and gets the same result."""
    eng, comm, pl = run.engine, run.comm, run.pl
    if pl.n_global < k:
        raise ValueError(f"Not enough data points ({pl.n_global}) to initialize {k} clusters")
    ell = float(2 * k if oversampling is None else oversampling)
    cand_idx = [int(g) for g in sampling.take_sample(pl.global_sizes, 1, seed, comm, run.sampler)]
    batches = [np.asarray(run.rows(cand_idx), dtype=np.float64)]
    rounds_run = 0
    t0 = time.perf_counter()
    eng.seed_begin()
    try:
        phi = _fold(run, batches[0], 0)
        for r in range(1, int(rounds) + 1):
            if phi == 0.0:
                break
            rounds_run = r
            local = eng.seed_sample(seed, r, pl.row0, ell, phi)
            if local is None:  # more picks than the device pass holds: the same rule on the host
                local = pick_rule(eng.seed_read()[0], seed, r, pl.row0, ell, phi)
            gidx = np.concatenate(comm.allgather_array(np.asarray(local, dtype=np.int64) + pl.row0))
            if len(gidx) == 0:
                continue
            rows = np.asarray(run.rows(gidx), dtype=np.float64)
            phi = _fold(run, rows, len(cand_idx))
            cand_idx.extend(int(g) for g in gidx)
            batches.append(rows)
        M = len(cand_idx)
        w = np.rint(comm.allreduce_np(eng.seed_weights(M).astype(np.float64))).astype(np.int64)
    finally:
        eng.seed_end()
    t1 = time.perf_counter()
    cands = np.concatenate(batches)
    centroids = cands[recluster(cands, w, k, seed)]
    t2 = time.perf_counter()
    if M < k:
        have = set(cand_idx)
        extra = [g for g in sampling.take_sample(pl.global_sizes, k, seed, comm, run.sampler) if g not in have]
        centroids = np.concatenate([centroids, np.asarray(run.rows(extra[:k - M]), dtype=np.float64)])
    if not np.all(np.isfinite(centroids)):
        raise ValueError("Data contains NaN or Inf values")
    return centroids, {"rounds": rounds_run, "candidates": M, "device_passes_s": t1 - t0, "recluster_s": t2 - t1}
