"""What loading a GPU-resident tensor costs, against the host route (one GPU).

    python scripts/ingest_time.py --config c3 --dtype float32 [--rows N]

The rows are Gaussian blobs as bench.py's (centres U(-10, 10), std 1),
generated on the GPU with torch in ``--dtype``.  Per route, 2 warm-up and 7
timed loads (``--warmup`` / ``--reps``), median and min - max:

  * device route, ``engine.load_device(t)``: wall time of the whole call
    (km_load_begin's allocation and clearing, k_ingest, the data maximum and
    the row norms, the final synchronisation) and, from HIP events around the
    launch (km_profile, KM_K_PREP), k_ingest alone; its bytes
    n (d sizeof(T) + 4 dp) and the fraction of 8 TB/s that is;
  * the yardstick, ``torch.empty_like(x).copy_(x)`` of a float32 tensor of
    X's size [n][dp] (the runtime's own device copy, HIP events): 8 n dp bytes;
  * host route, what a torch user had to do before: ``t.float().cpu().numpy()``
    (timed once) and ``engine.load_host`` of that array (wall time).

One JSON document on stdout and in profiles/ingest_<config>.json (the dtypes
of one config accumulate in the file).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (N, d, n_centers), bench.py's
    "c3": (100_000_000, 64, 256),
    "c5": (50_000_000, 128, 4096),
}
ELEM = {"float16": 2, "bfloat16": 2, "float32": 4, "float64": 8}


def spread(v, unit="ms"):
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v), "runs": len(v)}


def blobs(torch, n, d, centers, dtype, dev, chunk=4_000_000):
    g = torch.Generator(device=dev)
    g.manual_seed(2024)
    C = (torch.rand(centers, d, generator=g, device=dev) * 2 - 1) * 10.0
    out = torch.empty(n, d, dtype=dtype, device=dev)
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        pick = torch.randint(0, centers, (m,), generator=g, device=dev)
        out[a:a + m] = (C[pick] + torch.randn(m, d, generator=g, device=dev)).to(dtype)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    p.add_argument("--dtype", default="float32", choices=sorted(ELEM))
    p.add_argument("--rows", type=int, default=None, help="override N (rehearsals)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--no-host", action="store_true", help="skip the host route")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    N, d, centers = CONFIGS[a.config]
    N = a.rows or N

    import torch
    from kmeans_amd.engine import HipEngine
    dev = torch.device("cuda", 0)
    dtype = getattr(torch, a.dtype)
    t = blobs(torch, N, d, centers, dtype, dev)
    torch.cuda.synchronize()
    eng = HipEngine(0)
    clk = time.perf_counter

    wall, kern = [], []
    for r in range(a.warmup + a.reps):
        eng.profile(True, phases=("prep",))
        t0 = clk()
        eng.load_device(t)
        w = (clk() - t0) * 1e3
        ms, launches = eng.prof_read("prep")
        eng.profile(False)
        assert launches == 1
        if r >= a.warmup:
            wall.append(w)
            kern.append(ms)
    dp = eng.info()["dp"]
    nbytes = N * (d * ELEM[a.dtype] + 4 * dp)
    med = statistics.median(kern) * 1e-3
    doc = {"config": a.config, "N": N, "d": d, "dp": dp, "dtype": a.dtype, "warmup": a.warmup,
           "data": "Gaussian blobs generated on the GPU with torch (centres U(-10,10), std 1), as bench.py's",
           "device_route": {"load_device_wall": spread(wall), "k_ingest": spread(kern), "k_ingest_bytes": nbytes,
                            "k_ingest_TB_per_s": nbytes / med / 1e12, "k_ingest_fraction_of_8_TB_s": nbytes / med / 8e12}}

    # the host route first needs the rows on the host (while X is still resident: what a user pays)
    if not a.no_host:
        t0 = clk()
        rows = t.float().cpu().numpy()
        to_host_s = clk() - t0
    eng.close()

    # yardstick: the runtime's own device copy of a float32 tensor of X's size
    x = torch.empty(N, dp, dtype=torch.float32, device=dev).normal_()
    y = torch.empty_like(x)
    copy = []
    for r in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            copy.append(e0.elapsed_time(e1))
    cbytes = 8 * N * dp
    cmed = statistics.median(copy) * 1e-3
    doc["device_copy_yardstick"] = {"copy": spread(copy), "bytes": cbytes, "TB_per_s": cbytes / cmed / 1e12,
                                    "fraction_of_8_TB_s": cbytes / cmed / 8e12}
    doc["k_ingest_rate_over_copy_rate"] = (nbytes / med) / (cbytes / cmed)
    del x, y
    torch.cuda.empty_cache()

    if not a.no_host:
        eng = HipEngine(0)
        hw = []
        for r in range(a.warmup + a.reps):
            t0 = clk()
            eng.load_host(rows)
            w = clk() - t0
            if r >= a.warmup:
                hw.append(w)
        eng.close()
        doc["host_route"] = {"tensor_to_numpy_s": to_host_s, "load_host_wall": spread(hw, "s"),
                             "bytes_over_the_host_link_each_way": 4 * N * d}
        doc["host_over_device_wall"] = (to_host_s + statistics.median(hw)) / (statistics.median(wall) * 1e-3)

    out = a.out or os.path.join(ROOT, "profiles", f"ingest_{a.config}.json")
    allruns = {}
    if os.path.exists(out):
        with open(out) as f:
            allruns = json.load(f)
    allruns[a.dtype] = doc
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(allruns, indent=1) + "\n")


if __name__ == "__main__":
    main()
