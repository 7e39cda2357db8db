"""TEST-ONLY restatement of weighted k-means (``fit(..., sample_weight=w)``)
in NumPy, built from the oracle's assignment and takeSample, and the
``OracleEngine`` with weights (for the host-logic tests).

Contract (README "Row weights"): labels are the unweighted float64 argmin
(``orc.assign``); per cluster S = sum w x (x the stored float32 row as
float64), W = sum w, n = the row count; the new centroid is S / W where
n > 0, else the old one, replaced by the reference's takeSample policy
(uniform over rows); SSE = sum w ||x - c_label||^2.  Shift, convergence, NaN
check and log lines are the reference's.
"""
import numpy as np

from cpu_engine import OracleEngine
from oracle import kmeans_oracle as orc


DIRECT_LIMIT = 1 << 28   # n k d products up to which orc.assign runs on every pair


def exact_labels(X, C, direct_limit=DIRECT_LIMIT, with_gap=False):
    """``orc.assign(X, C)[0]`` -- NumPy's float64 argmin, lowest index on ties
    (with_gap: and the smallest relative top-2 distance gap of any row).

    Small problems call ``orc.assign`` itself.  Large ones (the k = 4096
    geometry is 1e10 products, over a minute of NumPy) first bound every
    distance with a float64 matrix product and keep, per row, the centroids
    whose bound could still reach the minimum; ``orc.assign`` then decides
    among those only.  The margin is 1e-9 of (||x|| + max ||c||)^2, about a
    million times the product's rounding error (~(d + 2) 2^-52 of that scale),
    so no candidate that could win is dropped; extra candidates cost time only.
    The host tests check the two routes against each other."""
    n, (k, d) = len(X), C.shape
    if n * k * d <= direct_limit:
        lab, _, gap = orc.assign(X, C)
        return (lab, float(gap.min())) if with_gap else lab
    labels = np.empty(n, dtype=np.int64)
    gap = np.inf
    c2 = (C * C).sum(axis=1)
    cmax = float(np.sqrt(c2.max()))
    for s in range(0, n, 2048):
        Xs = X[s:s + 2048]
        x2 = (Xs * Xs).sum(axis=1)
        D2 = x2[:, None] - 2.0 * (Xs @ C.T) + c2[None, :]
        margin = 1e-9 * (np.sqrt(x2) + cmax) ** 2
        lo = D2.min(axis=1)
        cand = D2 <= (lo + 2.0 * margin)[:, None]
        if with_gap and k > 1:                                    # from the bounds: good to ~1e-9 of the scale
            two = np.sqrt(np.maximum(np.partition(D2, 1, axis=1)[:, :2], 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                gap = min(gap, float(np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0).min()))
        labels[s:s + 2048] = np.argmax(cand, axis=1)              # the only candidate of most rows
        for i in np.nonzero(cand.sum(axis=1) > 1)[0]:
            ids = np.nonzero(cand[i])[0]                          # ascending: argmin keeps the lowest index
            labels[s + i] = ids[orc.assign(Xs[i:i + 1], C[ids])[0][0]]
    return (labels, gap) if with_gap else labels


def weighted_step(X, w, C, compute_sse=True, labels=None):
    """One assignment + update without the empty-cluster repair (labels: the
    assignment if the caller already has it).
    Returns labels, S [k][d], W [k], n [k], new centroids, SSE (or None)."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    k, d = C.shape
    if labels is None:
        labels = exact_labels(X, C)
    S = np.zeros((k, d))
    np.add.at(S, labels, w[:, None] * X)
    W = np.bincount(labels, weights=w, minlength=k).astype(np.float64)
    n = np.bincount(labels, minlength=k)
    new = np.where(n[:, None] > 0, S / np.where(n > 0, W, 1.0)[:, None], C)
    sse = float((w * ((X - C[labels]) ** 2).sum(axis=1)).sum()) if compute_sse else None
    return labels, S, W, n, new, sse


def weighted_lloyd_fit(X, w, k, max_iter, tolerance, compute_sse, sizes, init_centroids, empty_seed=lambda: 0,
                       log=None):
    """``orc.lloyd_fit`` with weights: the same loop, messages and repair
    policy (``sizes``: the takeSample partition layout)."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    centroids = np.array(init_centroids, dtype=np.float64, copy=True)
    say = log or (lambda s: None)
    say(f"Starting K-Means with k={k}, max_iter={max_iter}, tolerance={tolerance}")
    say(f"SSE computation: {'ENABLED' if compute_sse else 'DISABLED (for performance)'}")
    sse_history, records, converged = [], [], False
    for iteration in range(max_iter):
        labels, S, W, n, new, sse = weighted_step(X, w, centroids, compute_sse)
        empty = [j for j in range(k) if n[j] == 0]
        if empty:
            say(f"  WARNING: {len(empty)} empty cluster(s) detected. Reinitializing...")
            gidx = orc.take_sample_indices(list(sizes), len(empty), empty_seed())
            for i, cid in enumerate(empty):
                if i < len(gidx):
                    new[cid] = X[gidx[i]]
        if compute_sse:
            sse_history.append(sse)
            if len(sse_history) > 1 and sse > sse_history[-2] + 1e-6:
                say(f"  WARNING: SSE increased from {sse_history[-2]:.4f} to {sse:.4f}")
        if not np.all(np.isfinite(new)):
            raise ValueError(f"NaN or Inf detected in centroids at iteration {iteration + 1}")
        max_shift = np.max(np.linalg.norm(new - centroids, axis=1))
        sizes_list = [int(v) for v in n]
        if compute_sse:
            say(f"Iteration {iteration + 1}: SSE = {sse_history[-1]:.4f}, "
                f"Max Shift = {max_shift:.6f}, Cluster Sizes = {sizes_list}")
        else:
            say(f"Iteration {iteration + 1}: Max Shift = {max_shift:.6f}, Cluster Sizes = {sizes_list}")
        records.append({"max_shift": float(max_shift), "sizes": sizes_list, "empty": empty, "sse": sse})
        centroids = new
        if max_shift < tolerance:
            say(f"Converged after {iteration + 1} iterations")
            converged = True
            break
    return {"centroids": centroids, "sse_history": sse_history, "records": records, "n_iter": len(records),
            "converged": converged}


def top2_gap_and_empties(X, w, k, max_iter, tolerance, init_centroids):
    """Over the iterations of a weighted fit: the smallest relative top-2
    distance gap of any row and whether any cluster went empty (the data of an
    identity test must keep both away)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(init_centroids, dtype=np.float64)
    gap, emptied = np.inf, False
    for _ in range(max_iter):
        labels, g = exact_labels(X, C, with_gap=True)
        gap = min(gap, g)
        _, _, _, n, new, _ = weighted_step(X, w, C, False, labels)
        emptied = emptied or bool((n == 0).any())
        shift = np.max(np.linalg.norm(new - C, axis=1))
        C = new
        if shift < tolerance:
            break
    return gap, emptied


class WeightedOracleEngine(OracleEngine):
    """``OracleEngine`` with ``load_weights``: the stats buffer grows by the k
    sums of weights (behind the SSE slot), the update divides by them."""

    def __init__(self, comm):
        super().__init__(comm)
        self.w = None
        self.weight_loads = []   # what load_weights received, for the slicing tests

    def load_host(self, rows):
        self.w = None
        return super().load_host(rows)

    def load_weights(self, w):
        if w is None:
            self.w = None
            return
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (self.n,):
            raise ValueError(f"weights of shape {w.shape} for {self.n} local rows")
        self.w = w
        self.weight_loads.append(w.copy())

    def assign_stats(self):
        if self.w is None:
            return super().assign_stats()
        if getattr(self, "_stopped", False):
            return
        import torch
        k, d = self.k, self.d
        S = np.zeros(k * (d + 1) + 1 + k)
        T = S[:k * (d + 1)].reshape(k, d + 1)
        if self.n:
            labels, Sw, W, n, _, sse = weighted_step(self.X, self.w, self.cur, self.sse)
            self._labels = labels
            T[:, :d] = Sw
            T[:, d] = n
            S[k * (d + 1)] = sse if self.sse else 0.0
            S[k * (d + 1) + 1:] = W
        else:
            self._labels = np.zeros(0, dtype=np.int64)
        self._stats_t = torch.from_numpy(S)

    def update(self):
        if self.w is None:
            return super().update()
        from cpu_engine import _Status
        k, d = self.k, self.d
        flat = self._stats_t.numpy()
        T = flat[:k * (d + 1)].reshape(k, d + 1)
        cnt, W = T[:, d], flat[k * (d + 1) + 1:]
        old = self.cur
        new = np.where(cnt[:, None] > 0, T[:, :d] / np.where(cnt > 0, W, 1.0)[:, None], old)
        self.new = new
        shift = np.sqrt(((new - old) ** 2).sum(axis=1))
        st = _Status(sse=float(flat[k * (d + 1)]), max_shift=float(shift.max()), n_empty=int((cnt == 0).sum()),
                     nonfinite=int(not np.all(np.isfinite(new))), q_rerank=0, q_full=0, ran=1, stop_reason=0)
        return st, cnt.astype(np.int64)


def factory(comm):
    return WeightedOracleEngine(comm)
