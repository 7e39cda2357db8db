"""What the weighted statistics pass costs on the benchmark geometries (one GPU).

    python scripts/weighted_time.py --config c3 [--reps 12] [--steps 20]

With ``fit(..., sample_weight=w)`` an iteration is: the labels-only
assignment, then one weighted statistics pass over the rows (k_stats<SSE, true>, or the
counting sort + k_segsum<L, true>).  Per config this times, with HIP events around
the statistics phase (km_profile, KM_K_STATS), after warm-up and over
``--reps`` repeats of the same assignment (median, min, max reported):

  * the weighted pass, compute_sse off and on;
  * the unweighted statistics pass over the same labels, where the geometry
    has one (the unfused geometries: k_s1's labels, then k_stats).  The fused
    geometries (c3) sum inside the assignment kernel and have no labelled
    statistics pass to compare with; their assignment phase is reported
    instead, for both modes;
  * bytes moved by the weighted pass, n (4 dp + 12) (row, label, weight), and
    the fraction of 8 TB/s that is;
  * end-to-end iterations per second of the batched Lloyd loop, weighted and
    unweighted, same rows and initial centroids.

One JSON document on stdout and in profiles/weighted_<config>.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (N, d, k, n_centers); c4: bench.py's c4 geometry at a fifth of its rows (X as large as c3's)
    "c3": (100_000_000, 64, 256, 256),
    "c4": (200_000_000, 32, 1024, 1024),
    "c3_small": (4_000_000, 64, 256, 256),
    "c4_small": (2_000_000, 32, 1024, 1024),
}


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs": len(v)} if v else None


def time_passes(eng, C0, sse, warmup, reps):
    """Per repeat: new centroids (so every assignment computes full
    statistics, never deltas), one km_assign_stats; the statistics and
    assignment phases' event times."""
    eng.set_sse(sse)
    stats, assign = [], []
    for r in range(warmup + reps):
        eng.set_centroids(C0)
        eng.profile(True, phases=("stats", "assign"))
        eng.assign_stats()
        eng.sync()
        s_ms, s_n = eng.prof_read("stats")
        a_ms, _ = eng.prof_read("assign")
        eng.profile(False)
        if r >= warmup:
            if s_n:
                stats.append(s_ms)
            assign.append(a_ms)
    return spread(stats), spread(assign)


def its_per_s(km, run, C0, warmup, steps):
    eng = run.engine
    eng.set_centroids(C0)
    eng.set_sse(False)
    km.sse_history = []
    run.run(km, None, warmup)
    eng.sync()
    ran0 = run.iterations_ran
    t0 = time.perf_counter()
    run.run(km, None, warmup + steps, first=warmup)
    eng.sync()
    dt = time.perf_counter() - t0
    ran = run.iterations_ran - ran0
    return {"iterations": ran, "it_per_s": ran / dt if ran else None}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    p.add_argument("--reps", type=int, default=12)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--rows", type=int, default=None, help="override N (rehearsals)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    N, d, k, centers = CONFIGS[a.config]
    N = a.rows or N

    import kmeans_amd
    from kmeans_amd.comm import Communicator

    class TimedKMeans(kmeans_amd.KMeans):
        def _empty_seed(self):
            return 20240607

    km = TimedKMeans(k=k, max_iter=10 ** 6, tolerance=1e-300, seed=42, compute_sse=False)
    km.verbose = False
    data = kmeans_amd.DeviceBlobs(n=N, d=d, n_centers=centers, box=10.0, std=1.0, seed=2024)
    run = km._make_runner(data, Communicator())
    eng = run.engine
    C0 = np.asarray(km._initialize_centroids(run), dtype=np.float64)
    info = eng.info()
    dp = info["dp"]

    doc = {"config": a.config, "N": N, "d": d, "dp": dp, "k": k,
           "data": "synthetic Gaussian blobs generated in HBM (centers U(-10,10), std 1), as bench.py",
           "weights": "exp(uniform(-7, 7)), float64", "warmup": a.warmup}
    un = {}
    for sse in (False, True):
        s, asg = time_passes(eng, C0, sse, a.warmup, a.reps)
        un["sse_on" if sse else "sse_off"] = {"stats_pass": s, "assign_phase": asg}
    un["end_to_end"] = its_per_s(km, run, C0, a.warmup, a.steps)
    if un["sse_off"]["stats_pass"] is None:
        un["note"] = ("fused geometry: the assignment kernel sums the statistics itself, there is no labelled "
                      "unweighted statistics pass")
    doc["unweighted"] = un

    eng.load_weights(np.exp(np.random.default_rng(7).uniform(-7, 7, N)))
    we = {}
    for sse in (False, True):
        s, asg = time_passes(eng, C0, sse, a.warmup, a.reps)
        nbytes = N * (4 * dp + 12)
        med = s["median_ms"] * 1e-3
        we["sse_on" if sse else "sse_off"] = {"stats_pass": s, "assign_phase": asg, "bytes_moved": nbytes,
                                              "TB_per_s": nbytes / med / 1e12,
                                              "fraction_of_8_TB_s": nbytes / med / 8e12}
    we["end_to_end"] = its_per_s(km, run, C0, a.warmup, a.steps)
    doc["weighted"] = we

    us, ws = un["sse_off"]["stats_pass"], we["sse_off"]["stats_pass"]
    if us:
        byte_ratio = (4 * dp + 12) / (4 * dp + 4)
        doc["comparison_sse_off"] = {
            "time_ratio_weighted_over_unweighted": ws["median_ms"] / us["median_ms"],
            "byte_ratio": byte_ratio,
            "run_to_run_spread": max(ws["max_ms"] - ws["min_ms"], us["max_ms"] - us["min_ms"]) / us["median_ms"],
        }
    eng.close()
    text = json.dumps(doc, indent=1)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", f"weighted_{a.config}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
