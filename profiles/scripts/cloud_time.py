"""Timing of the raw-cloud kernels on an MI355X: the grid kNN against the brute-force scan of the same kernel on the same
definition.  Writes profiles/cloud_time.json (--out).

    python profiles/scripts/cloud_time.py                  everything below
    python profiles/scripts/cloud_time.py --kernels-only   the grid calls alone (profiler runs:
                                                           `rocprofv3 --kernel-trace --stats -- python profiles/scripts/cloud_time.py --kernels-only --reps 5`)

The fixture: the geodesic fixture's body, its surface sampled (mesh_io.sample_surface) to 8 clouds x 300 000 points.  HIP-event time per call,
median / min / max over --reps calls after 3 warm-up calls, of ops.cloud_knn_mean (k = 16; the cell keys, the two sorts and the gather
included) in the grid form and with brute=True, ops.cloud_radius_count (r = 1 cm), ops.cloud_voxel_grid (1 cm), and cloud.prepare (statistical
filter, voxel grid, centre, pick of 5 000) end to end on the host clock.  Where one brute-force call at 300 000 points per cloud takes longer
than --brute-budget seconds for its 33 calls, both forms are also timed at 50 000 points per cloud and the ratio is stated at that size."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from etch_amd import cloud as C
from etch_amd import mesh_io, ops
from etch_amd.depth import Cloud
from etch_amd.inference_demo import Mesh

GOLDEN = os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz")
CLOUDS, K = 8, 16


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e))
    t = np.sort(np.array(t))
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t[0]), 4), "max_ms": round(float(t[-1]), 4), "reps": reps}


def sampled(body, n):
    _, _, _, p64 = mesh_io.sample_surface([body] * CLOUDS, n, list(range(1, CLOUDS + 1)), center=False, return_fp64=True)
    pts = p64.reshape(-1, 3).contiguous()
    off = (torch.arange(CLOUDS + 1, dtype=torch.int64) * n).to(torch.int32).cuda()
    idx = torch.arange(n, dtype=torch.int32).repeat(CLOUDS).cuda()
    return Cloud(pts, idx, off, off[1:] - off[:-1], None)


def ratio(grid, brute):
    spread = max(grid["max_ms"] - grid["min_ms"], brute["max_ms"] - brute["min_ms"])
    return {"brute_over_grid": round(brute["median_ms"] / grid["median_ms"], 1), "difference_ms": round(brute["median_ms"] - grid["median_ms"], 3),
            "larger_spread_ms": round(spread, 3), "difference_exceeds_twice_the_spread": bool(brute["median_ms"] - grid["median_ms"] > 2.0 * spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_time.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--brute-budget", type=float, default=150.0, help="seconds the brute-force leg may take at --points")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    z = np.load(GOLDEN)
    body = Mesh(z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64))
    cl = sampled(body, a.points)
    P, O = cl.points, cl.offsets
    res = {"clouds": CLOUDS, "points_per_cloud": a.points, "k": K, "device": torch.cuda.get_device_name(0)}
    grid, status, _, skeys, _ = ops.cloud_cell_grid(P, O, 0, K)
    cells = int((skeys[1:] != skeys[:-1]).sum()) + 1
    res["knn_cell_size_m"] = [round(float(x), 6) for x in grid[:, 3].tolist()]
    res["knn_points_per_occupied_cell"] = round(P.shape[0] / cells, 2)
    res["knn_grid"] = event_ms(lambda: ops.cloud_knn_mean(P, O, K), a.reps)
    res["radius_count_r_0.01"] = event_ms(lambda: ops.cloud_radius_count(P, O, 0.01), a.reps)
    res["voxel_grid_0.01"] = event_ms(lambda: ops.cloud_voxel_grid(P, O, 0.01), a.reps)
    if a.kernels_only:
        print(json.dumps(res))
        return
    res["cell_keys_and_sorts_alone"] = event_ms(lambda: ops.cloud_cell_grid(P, O, 0, K), a.reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mb, _ = ops.cloud_knn_mean(P, O, K, brute=True)
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    res["knn_brute_first_call_s"] = round(one, 3)
    mg, _ = ops.cloud_knn_mean(P, O, K)
    res["grid_and_brute_bit_equal"] = bool(torch.equal(mg.view(torch.int64), mb.view(torch.int64)))
    if one * (a.reps + 3) <= a.brute_budget:
        res["knn_brute"] = event_ms(lambda: ops.cloud_knn_mean(P, O, K, brute=True), a.reps)
        res["knn_ratio"] = dict(ratio(res["knn_grid"], res["knn_brute"]), points_per_cloud=a.points)
    else:
        small = sampled(body, 50000)
        g = event_ms(lambda: ops.cloud_knn_mean(small.points, small.offsets, K), a.reps)
        b = event_ms(lambda: ops.cloud_knn_mean(small.points, small.offsets, K, brute=True), a.reps)
        res["knn_at_50000"] = {"grid": g, "brute": b}
        res["knn_ratio"] = dict(ratio(g, b), points_per_cloud=50000,
                                note=f"one brute-force call at {a.points} points per cloud took {one:.2f} s: the brute-force leg is timed at 50 000; not extrapolated")
    t = []
    keys = list(range(CLOUDS))
    for _ in range(a.reps + 2):
        t0 = time.perf_counter()
        p32, c, clean = C.prepare(cl, 5000, keys, voxel=0.01, stat=(K, 2.0))
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(np.array(t[2:]))
    res["prepare"] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "points_picked": 5000,
                      "rows": {k: [int(x) for x in v] for k, v in clean.stages.items()},
                      "note": "host clock: offsets check, statistical filter (k = 16, ratio 2), compaction, voxel grid 1 cm, centre, pick, one readback"}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
