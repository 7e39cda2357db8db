"""What k-means|| seeding costs and buys on the benchmark configs (one GPU).

    python scripts/seed_time.py --config c3 [--arms random,k-means||] [--max-iter 100]

Per arm (an initialisation of the same generated rows):
  * the wall time of the initialisation, also in units of the run's own
    steady-state Lloyd iteration;
  * k_seed_fold's time per launch (HIP events in its dispatch) and the bytes
    per second it streams (X, the labels and D2 read once per row);
  * the SSE after 20 iterations, the iterations to convergence
    (max shift < 1e-4, the reference's default) or the cap, the final SSE and
    the iterations that repaired empty clusters.
Arms: ``random`` (takeSample of k rows), ``poor`` (bench.py's c5_poor seeds:
3 sampled rows + k - 3 far points), ``k-means||``.  One JSON document on
stdout and in profiles/seeding_<config>.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (N, d, k, n_centers), bench.py's
    "c3": (100_000_000, 64, 256, 256),
    "c5": (50_000_000, 128, 4096, 4096),
    "c5_poor": (50_000_000, 128, 4096, 4096),
    "c3_small": (4_000_000, 64, 256, 256),
}
DEFAULT_ARMS = {"c3": "random,k-means||", "c3_small": "random,k-means||", "c5": "random,k-means||",
                "c5_poor": "poor,k-means||"}


def one_arm(arm, N, d, k, centers, max_iter, seed):
    import kmeans_amd
    from kmeans_amd.comm import Communicator

    class TimedKMeans(kmeans_amd.KMeans):
        def _empty_seed(self):
            return 20240607  # bench.py's pinned repair seed

    km = TimedKMeans(k=k, max_iter=max_iter, tolerance=1e-4, seed=seed, compute_sse=True,
                     init="k-means||" if arm == "k-means||" else "random")
    km.verbose = False
    comm = Communicator()
    data = kmeans_amd.DeviceBlobs(n=N, d=d, n_centers=centers, box=10.0, std=1.0, seed=2024)
    run = km._make_runner(data, comm)
    eng = run.engine
    eng.sync()
    eng.profile(True, phases=("seed", "assign", "resolve", "prep"))
    t0 = time.perf_counter()
    C0 = km._initialize_centroids(run)
    eng.sync()
    init_s = time.perf_counter() - t0
    fold_ms, folds = eng.prof_read("seed")
    phases = {ph: dict(zip(("ms", "launches"), eng.prof_read(ph))) for ph in ("assign", "resolve", "prep")}
    eng.profile(False)
    if arm == "poor":
        C0 = np.vstack([C0[:3], np.full((k - 3, d), 100.0) + np.arange(k - 3)[:, None]])
    out = {"arm": arm, "init_wall_s": init_s, "init": km._init_info}
    if folds:
        out["init_kernels"] = phases  # the assignment passes of the rounds (HIP events)
        info = eng.info()
        nbytes = N * (info["dp"] * 4 + 4 + 8)  # X row, label, D2
        out["k_seed_fold"] = {"launches": folds, "ms_per_launch": fold_ms / folds,
                              "bytes_per_launch": nbytes, "TB_per_s": nbytes / (fold_ms / folds * 1e-3) / 1e12,
                              "fraction_of_8_TB_s": nbytes / (fold_ms / folds * 1e-3) / 8e12}
    repairs = []

    def log(msg):
        if "empty cluster" in msg:
            repairs.append(msg.strip())

    eng.set_centroids(np.asarray(C0, dtype=np.float64))
    eng.set_sse(True)
    km.sse_history = []
    conv = run.run(km, log, min(3, max_iter))
    eng.sync()
    steady = None
    if not conv and max_iter > 3:
        ran0 = run.iterations_ran
        t0 = time.perf_counter()
        conv = run.run(km, log, min(20, max_iter), first=3)
        eng.sync()
        dt = time.perf_counter() - t0
        steady = dt / max(run.iterations_ran - ran0, 1)
    if not conv and max_iter > 20:
        conv = run.run(km, log, max_iter, first=20)
        eng.sync()
    h = km.sse_history
    out.update({"steady_ms_per_iteration": None if steady is None else steady * 1e3,
                "init_in_iterations": None if steady is None else init_s / steady,
                "sse_after_20": h[19] if len(h) >= 20 else None, "sse_first": h[0] if h else None,
                "sse_final": h[-1] if h else None, "iterations": len(h), "converged": bool(conv),
                "iterations_with_empty_repairs": len(repairs)})
    eng.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    p.add_argument("--arms", default=None, help="comma-separated: random, poor, k-means||")
    p.add_argument("--max-iter", type=int, default=100)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--rows", type=int, default=None, help="override N (rehearsals)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    N, d, k, centers = CONFIGS[a.config]
    N = a.rows or N
    arms = (a.arms or DEFAULT_ARMS[a.config]).split(",")
    doc = {"config": a.config, "N": N, "d": d, "k": k, "seed": a.seed, "tolerance": 1e-4, "max_iter": a.max_iter,
           "data": "synthetic Gaussian blobs generated in HBM (centers U(-10,10), std 1), as bench.py",
           "arms": [one_arm(arm, N, d, k, centers, a.max_iter, a.seed) for arm in arms]}
    text = json.dumps(doc, indent=1)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", f"seeding_{a.config}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
