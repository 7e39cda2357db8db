"""TEST-ONLY: a NumPy restatement of k-means|| seeding as the product fixes it
(steps 1-8 of ``seeding.py``'s docstring), written against the oracle and
without importing the product, plus a CPU engine with the six ``seed_*``
methods so the host logic runs without a GPU (``KMeans._engine_factory``).
"""
import math

import numpy as np

import cpu_engine
from oracle import kmeans_oracle as orc

M64 = 2 ** 64 - 1


def splitmix64_np(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, rnd, gidx):
    key = splitmix64_np(np.uint64((seed & M64) ^ ((rnd * 0xD1B54A32D192ED03) & M64)))
    h = splitmix64_np(key ^ np.asarray(gidx, dtype=np.int64).astype(np.uint64))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def update(X, D2, near, Cnew, first_id):
    """Step 3, in place, for the rows X (float64 values of the float32 rows)."""
    if len(X) == 0:
        return
    Cnew = np.asarray(Cnew, dtype=np.float64)
    j = orc.assign(X, Cnew)[0]                     # np.argmin(np.linalg.norm(Cnew - x, axis=1))
    diff = Cnew[j] - X
    t = np.add.reduce(diff * diff, axis=1)         # pairwise, products rounded
    better = t < D2
    D2[better] = t[better]
    near[better] = (first_id + j[better]).astype(near.dtype)


def pick(D2, seed, rnd, row0, ell, phi):
    """Step 4 over rows with global indices row0 ..: (local picks, relative
    margin |u phi - ell D2| / max of the two, per row)."""
    u = uniforms(seed, rnd, np.arange(len(D2), dtype=np.int64) + row0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lhs, rhs = u * float(phi), float(ell) * D2
        hit = lhs < rhs
        big = np.maximum(lhs, rhs)
        margin = np.where(big > 0, np.abs(lhs - rhs) / big, 1.0)
        margin = np.where(np.isfinite(margin), margin, 1.0)
    return np.nonzero(hit)[0].astype(np.int64), margin


def recluster(C, w, k, seed):
    """Step 6: weighted k-means++ over the candidates."""
    C = np.asarray(C, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    M = len(C)
    rs = np.random.RandomState(seed & 0xFFFFFFFF)
    chosen, taken, mind2 = [], np.zeros(M, bool), np.full(M, np.inf)
    for _ in range(min(k, M)):
        p = w.copy() if not chosen else w * mind2
        p[taken] = 0.0
        total = float(p.sum())
        if total > 0.0 and np.isfinite(total):
            c = np.cumsum(p)
            j = min(int(np.searchsorted(c, rs.random_sample() * c[-1], side="right")), M - 1)
            while p[j] == 0:
                j -= 1
        else:
            j = int(np.nonzero(~taken)[0][0])
        chosen.append(j)
        taken[j] = True
        mind2 = np.minimum(mind2, np.add.reduce((C - C[j]) * (C - C[j]), axis=1))
    return chosen


def kmeans_parallel_ref(X, sizes, k, seed, rounds=5, oversampling=None, shards=None):
    """Steps 1-8 for the rows X with takeSample layout ``sizes``.  ``shards``:
    the ranks' row ranges [(a, b), ...]: phi is then the sum of the shards'
    sums, as the all-reduce forms it.  Returns centroids, the candidates'
    global indices, rounds run, weights and the smallest relative margin of
    any pick decision (how close any row came to flipping)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    N = len(X)
    if N < k:
        raise ValueError(f"Not enough data points ({N}) to initialize {k} clusters")
    ell = float(2 * k if oversampling is None else oversampling)
    shards = shards or [(0, N)]
    D2, near = np.full(N, np.inf), np.full(N, -1, dtype=np.int64)

    def fold(Cnew, first_id):
        update(X, D2, near, Cnew, first_id)
        phi = 0.0
        for a, b in shards:
            phi = phi + math.fsum(D2[a:b])
        if not math.isfinite(phi):
            raise ValueError("Data contains NaN or Inf values")
        return phi

    cand = list(orc.take_sample_indices(sizes, 1, seed))
    phi = fold(X[cand], 0)
    ran, margin = 0, 1.0
    for r in range(1, rounds + 1):
        if phi == 0.0:
            break
        ran = r
        picks, mg = pick(D2, seed, r, 0, ell, phi)
        margin = min(margin, float(mg.min()))
        if len(picks) == 0:
            continue
        phi = fold(X[picks], len(cand))
        cand.extend(int(g) for g in picks)
    M = len(cand)
    w = np.bincount(near, minlength=M)
    chosen = recluster(X[cand], w, k, seed)
    idx = [cand[j] for j in chosen]
    if M < k:
        have = set(cand)
        extra = [g for g in orc.take_sample_indices(sizes, k, seed) if g not in have]
        idx += extra[:k - M]
    return {"centroids": X[idx], "index": idx, "candidates": cand, "rounds": ran, "weights": w,
            "margin": margin, "D2": D2, "near": near}


class SeedOracleEngine(cpu_engine.OracleEngine):
    """The OracleEngine with the km_seed_* protocol (mirror of HipEngine)."""

    def seed_begin(self):
        self._d2 = np.full(self.n, np.inf)
        self._near = np.full(self.n, -1, dtype=np.int32)

    def seed_update(self, first_id):
        update(self.X, self._d2, self._near, self.cur, first_id)
        return math.fsum(self._d2)

    def seed_sample(self, seed, rnd, global_row0, ell, phi, cap=None):
        cap = int(4.0 * ell) + 64 if cap is None else cap
        picks = pick(self._d2, seed, rnd, global_row0, ell, phi)[0]
        return None if len(picks) > cap else picks

    def seed_weights(self, m_total):
        return np.bincount(self._near[self._near >= 0], minlength=m_total).astype(np.int64)

    def seed_read(self):
        return self._d2.copy(), self._near.copy()

    def seed_end(self):
        del self._d2, self._near


def factory(comm):
    return SeedOracleEngine(comm)


class SmallCapEngine(SeedOracleEngine):
    """Every device pick pass "overflows": the driver must fall back to the
    NumPy form of the rule on seed_read's D2."""

    def seed_sample(self, *a, **kw):
        return None


def factory_small_cap(comm):
    return SmallCapEngine(comm)
