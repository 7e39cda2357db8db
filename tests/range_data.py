"""Inputs for the float32-range tests of the MFMA path (path 2), plain NumPy,
no GPU.  tests/test_host_range_data.py checks the properties the GPU tests
rely on; tests/test_gpu_fp32_range.py runs them.

Every generator returns float64 arrays whose rows and centroids are
float32-representable (the engine stores float32 rows, and centroids that are
data rows; the oracle reads the same values).

The rows are noise around the origin whose norms spread over a decade, and
the centroids are rows: the ||c||^2 term of the score ||c||^2 - 2 c.x then
decides most labels, so a screen that loses it (an fp32 ||c||^2 that
underflowed before the scale was applied) mislabels most rows.  Well
separated blobs would not show that: their -2 c.x term decides alone.
"""
import numpy as np

from oracle import kmeans_oracle as orc

SCALES = [1e-30, 1e-25, 1e-22, 1e-19, 1.0, 1e18, 1e19, 1e20]
ITER_SCALES = [1e-25, 1e-22, 1e18, 1e20]

# class -> (n, d, k, dp, kp, fused_stats, seed): every dispatch class of path 2
# at the smallest shape that reaches it; G has three shapes
CLASSES = {
    "A": (3000, 64, 40, 64, 64, 1, 3),       # k_fused16 + k_s1 + row gate (the c3 class)
    "B": (3000, 32, 40, 32, 64, 1, 2),       # k_fused16, two-key chains
    "C": (3000, 40, 40, 48, 64, 1, 3),       # k_fused 32x32x16 (dp not a multiple of 32)
    "D": (3000, 128, 40, 128, 64, 1, 4),     # k_fused16, dp 128
    "E": (3000, 64, 500, 64, 512, 0, 5),     # unfused + k_s1 (the c4 class)
    "F": (3000, 64, 300, 64, 320, 0, 6),     # one-MFMA k_assign_mfma16 + candidate lists
    "G": (3000, 90, 300, 96, 320, 0, 7),     # fp16x3 k_assign_mfma, generic row norms
    "G2": (3000, 20, 40, 32, 64, 1, 8),      # d < dp on B's geometry (dp 32, kp 64 is a fused instance)
    "G3": (3000, 20, 300, 32, 320, 0, 11),   # fp16x3 k_assign_mfma at dp 32: two-key chains, unfused
    "H": (3000, 300, 40, 304, 64, 0, 9),     # k_assign_wide
    "I": (4000, 128, 1803, 128, 1856, 0, 10),  # chunked centroid images (the c5 class)
}
ITER_CLASSES = ["A", "E", "F"]
MIXED_CLASSES = ["A", "F", "H"]
PREDICT_CLASSES = ["A", "B", "D", "E"]
ITERS = 3


def _f32(a):
    with np.errstate(under="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def noise(n, d, k, seed, scale):
    """(X, C0): rows standard_normal * uniform(0.2, 2) * scale, rounded to
    float32; C0 = k distinct rows of X."""
    rng = np.random.default_rng(seed)
    X = _f32(rng.standard_normal((n, d)) * rng.uniform(0.2, 2.0, (n, 1)) * scale)
    C0 = X[rng.choice(n, k, replace=False)].copy()
    return X, C0


def class_case(name, scale):
    n, d, k, _, _, _, seed = CLASSES[name]
    return noise(n, d, k, seed, scale)


def _unit(n, d, k, seed):
    rng = np.random.default_rng(seed)
    X = _f32(rng.standard_normal((n, d)) * rng.uniform(0.2, 2.0, (n, 1)))
    idx = rng.choice(n - 1, k, replace=False) + 1          # row 0 is never a centroid
    return X, idx


def outlier_row(n, d, k, seed):
    """Unit-scale noise with row 0 multiplied by 1e20: max |x| forces the
    screens' scale s to about 2^-55, and every other row is an fp16 zero in
    the image.  The row itself is farther than 1e20 from every centroid and
    float64 cannot tell them apart: an exact tie, label 0."""
    X, idx = _unit(n, d, k, seed)
    X[0] = _f32(X[0] * 1e20)
    return X, X[idx].copy()


def outlier_centroid(n, d, k, seed):
    """Unit-scale noise with centroid k // 2 at 1e20 e_0: max ||c|| and
    max |c| become huge, and that centroid owns no row."""
    X, idx = _unit(n, d, k, seed)
    C0 = X[idx].copy()
    C0[k // 2] = 0.0
    C0[k // 2, 0] = float(np.float32(1e20))
    return X, C0


def tiny_rows(n, d, k, seed):
    """Unit-scale noise with every 7th row multiplied by 1e-25 and centroid 3
    at the origin (it owns the tiny rows, at distances near 1e-25)."""
    X, _ = _unit(n, d, k, seed)
    ordinary = np.nonzero(np.arange(n) % 7)[0]             # centroids are ordinary rows
    idx = np.random.default_rng(seed + 1).choice(ordinary, k, replace=False)
    X[::7] = _f32(X[::7] * 1e-25)
    C0 = X[idx].copy()
    C0[3] = 0.0
    return X, C0


def denormal_rows(n, d, k, seed):
    """Noise at scale 1e-41: every stored value is a float32 denormal."""
    return noise(n, d, k, seed, 1e-41)


MIXED = {"outlier_row": outlier_row, "outlier_centroid": outlier_centroid, "tiny_rows": tiny_rows,
         "denormal_rows": denormal_rows}


def mixed_case(kind, name):
    n, d, k, _, _, _, seed = CLASSES[name]
    return MIXED[kind](n, d, k, seed + 40)


# gate_scale: max(|x|, |c|) = 1.5 * 2^e; the screens' scale is s = 2^(13 - e)
GATE_SIDES = {"s=2^30": -17, "s=2^31": -18, "s=2^-30": 43, "s=2^-31": 44}
GATE_PAIRS = [("s=2^30", "s=2^31"), ("s=2^-30", "s=2^-31")]   # (inside, outside) the row gate's range


def gate_scale(side):
    """Class A noise with max |x| = 1.5 exactly, times 2^e: the rows of the two
    sides of a boundary differ by an exact factor of two, so the oracle's
    labels are the same and its centroids differ by that factor."""
    n, d, k, _, _, _, seed = CLASSES["A"]
    rng = np.random.default_rng(seed + 80)
    X = rng.standard_normal((n, d)) * rng.uniform(0.2, 2.0, (n, 1))
    X = _f32(X / np.abs(X).max() * 1.5)
    assert np.abs(X).max() == 1.5
    X = np.ldexp(X, GATE_SIDES[side])
    assert np.array_equal(X, _f32(X))
    C0 = X[rng.choice(n, k, replace=False)].copy()
    return X, C0


def s1_scale(xabs, cabs):
    """The screens' power-of-two scale (mfma_scale / s1_scale of the HIP
    sources) restated: max(|x|, |c|) * s in [2^13, 2^14)."""
    m = np.float32(max(xabs, cabs))
    if not (m > 0) or not (m < np.float32(3.0e38)):
        return 1.0
    _, e = np.frexp(m)
    return float(np.ldexp(1.0, 14 - int(e)))


def assign(X, C):
    """(labels, min distance): orc.assign's, with the candidates of each row
    first narrowed by a float64 matrix product (class I is 1e9 products).
    |D2 - ||x - c||^2| <= 1e-9 (||x|| + ||c||)^2 per pair, about a million
    times the product's rounding error, so no centroid that could win is
    dropped; orc.assign decides among the kept ones (ascending: the lowest
    index wins a tie) and the distance is NumPy's norm of the difference."""
    n, k = len(X), len(C)
    labels = np.empty(n, dtype=np.int64)
    c2 = (C * C).sum(axis=1)
    cn = np.sqrt(c2)
    for s in range(0, n, 2048):
        Xs = X[s:s + 2048]
        x2 = (Xs * Xs).sum(axis=1)
        D2 = x2[:, None] - 2.0 * (Xs @ C.T) + c2[None, :]
        m = 1e-9 * (np.sqrt(x2)[:, None] + cn[None, :]) ** 2
        cand = (D2 - m) <= (D2 + m).min(axis=1)[:, None]
        labels[s:s + 2048] = np.argmax(cand, axis=1)
        for i in np.nonzero(cand.sum(axis=1) > 1)[0]:
            ids = np.nonzero(cand[i])[0]
            labels[s + i] = ids[orc.assign(Xs[i:i + 1], C[ids])[0][0]]
    diff = C[labels] - X
    mind = np.sqrt(np.add.reduce(diff * diff, axis=-1))
    return labels, mind


def step(X, C):
    """One assignment and update in the oracle's terms: labels, counts, sums
    (accumulated in long double), SSE, and the new centroids (an empty
    cluster keeps its centroid, as km_update does)."""
    k = len(C)
    labels, mind = assign(X, C)
    sums = np.zeros(C.shape, dtype=np.longdouble)
    np.add.at(sums, labels, X.astype(np.longdouble))
    counts = np.bincount(labels, minlength=k)
    new = C.copy()
    own = counts > 0
    new[own] = (sums[own] / counts[own, None]).astype(np.float64)
    sse = orc.partition_sse(mind)
    return {"labels": labels, "counts": counts, "sums": sums.astype(np.float64), "sse": sse, "sse_fit": sse,
            "new": new}


def lloyd(X, C0, iters):
    """`iters` steps, each from the previous one's centroids (orc.lloyd_fit
    without its stopping rule and empty-cluster repair; the host tests assert
    that no cluster empties and compare the two)."""
    out, C = [], C0
    for _ in range(iters):
        out.append(step(X, C))
        C = out[-1]["new"]
    return out
