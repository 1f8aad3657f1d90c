"""Timing of the normals kernel and of the point-to-plane registration on an MI355X.  Writes profiles/cloud_normals_time.json
(--out).

    python profiles/scripts/cloud_normals_time.py

The fixture and the protocol of profiles/scripts/cloud_align_time.py: the geodesic fixture's body sampled to 8 target clouds x 300 000 points and
8 source clouds x 100 000 points (other samples), the sources displaced by 10 degrees / 5 cm; HIP-event time per call, median / min / max over
--reps calls after 3 warm-up calls.  Timed: etch_cloud_normals alone on a grid built before at k = 16 and k = 32, in the grid and the brute form
(the brute form as often as --brute-budget allows), against etch_cloud_knn_mean alone on the same grid; ops.cloud_normals with the grid, the sorts
and the gather; one align of 40 point steps, of 40 plane steps and of --plane-steps plane steps, the normals pass included, each with its rms and
its largest row distance from the truth."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import torch

from cloud_align_time import GOLDEN, PAIRS, event_ms, packed, ratio, rotation, sampled
from etch_amd import _lib
from etch_amd import cloud as C
from etch_amd import ops
from etch_amd.inference_demo import Mesh

ROOT = os.path.dirname(os.path.dirname(HERE))


def kernels_alone(tgt, k, brute):
    """etch_cloud_normals and etch_cloud_knn_mean on one grid built before: -> two callables and the normals' outputs."""
    B, M = PAIRS, tgt.points.shape[0]
    grid, status, sp, sk, order = ops.cloud_cell_grid(tgt.points, tgt.offsets, 0, k, 0.0, sort=not brute)
    normal = torch.zeros((M, 3), dtype=torch.float64, device="cuda")
    variation = torch.zeros((M,), dtype=torch.float64, device="cuda")
    flag = torch.zeros((M,), dtype=torch.int32, device="cuda")
    mean = torch.zeros((M,), dtype=torch.float64, device="cuda")
    pts = tgt.points if brute else sp
    fn = lambda: _lib.call("etch_cloud_normals", B, M, k, int(brute), pts, sk, order, tgt.offsets, grid, status, None, normal, variation, flag, None)
    knn = lambda: _lib.call("etch_cloud_knn_mean", B, M, k, int(brute), pts, sk, order, tgt.offsets, grid, status, mean)
    return fn, knn, normal, flag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_normals_time.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--target", type=int, default=300000)
    ap.add_argument("--source", type=int, default=100000)
    ap.add_argument("--plane-steps", type=int, default=8, help="the step count after which the oracle's pose stops improving (tests/test_normals_host.py)")
    ap.add_argument("--brute-budget", type=float, default=90.0, help="seconds the brute-force legs may take in all")
    a = ap.parse_args()
    z = np.load(GOLDEN)
    body = Mesh(z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64))
    R0, t0 = rotation([0.3, 1.0, 0.2], 10.0), np.array([0.05, -0.025, 0.05 / 3.0])
    tgt = packed(sampled(body, a.target, 1), a.target)
    truth = sampled(body, a.source, 101)
    src = packed(((truth - torch.from_numpy(t0).cuda()) @ torch.from_numpy(R0).cuda()).contiguous(), a.source)
    res = {"pairs": PAIRS, "target_rows_per_cloud": a.target, "source_rows_per_cloud": a.source, "start_pose": "10 degrees, 5 cm",
           "device": torch.cuda.get_device_name(0)}
    spent = 0.0
    for k in (16, 32):
        fn, knn, normal, flag = kernels_alone(tgt, k, False)
        res[f"normals_kernel_k{k}_grid"] = event_ms(fn, a.reps)
        res[f"knn_mean_kernel_k{k}_grid"] = event_ms(knn, a.reps)
        res[f"normals_over_knn_mean_k{k}"] = round(res[f"normals_kernel_k{k}_grid"]["median_ms"] / res[f"knn_mean_kernel_k{k}_grid"]["median_ms"], 3)
        res[f"normals_k{k}_flagged_rows"] = int((flag != 0).sum())
        res[f"ops_cloud_normals_k{k}_with_grid_sorts_gather"] = event_ms(lambda: ops.cloud_normals(tgt.points, tgt.offsets, k), a.reps)
        bf, _, bnormal, bflag = kernels_alone(tgt, k, True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        bf()
        torch.cuda.synchronize()
        one = time.perf_counter() - t1
        res[f"normals_kernel_k{k}_brute_first_call_s"] = round(one, 3)
        res[f"normals_k{k}_brute_equal"] = bool(torch.equal(bnormal, normal) and torch.equal(bflag, flag))
        left = a.brute_budget - spent - one
        reps = int(min(a.reps, left / max(one, 1e-6) - 1))
        spent += one
        if reps >= 2:
            res[f"normals_kernel_k{k}_brute"] = event_ms(bf, reps, warm=1)
            spent += one * (reps + 1)
        else:
            res[f"normals_kernel_k{k}_brute"] = {"median_ms": round(one * 1e3, 1), "min_ms": round(one * 1e3, 1), "max_ms": round(one * 1e3, 1), "reps": 1,
                                                 "note": "host clock, the first call alone: the budget allows no more"}
        res[f"normals_k{k}_ratio"] = ratio(res[f"normals_kernel_k{k}_grid"], res[f"normals_kernel_k{k}_brute"])
    args = C._check_align()
    want = torch.from_numpy(R0).cuda(), torch.from_numpy(t0).cuda()

    def quality(out):
        moved = ops.cloud_transform(src.points, src.offsets, out["R"], out["t"])
        return {"rms_m": [round(float(x), 6) for x in out["rms"].tolist()], "steps": out["steps"].tolist(),
                "largest_row_distance_from_the_truth_m": float(torch.sqrt(((moved - truth) ** 2).sum(1)).max())}

    point = lambda: C._align(torch, ops, src, tgt, args, None, None, False)
    res["align_point_40_steps"] = dict(event_ms(point, a.reps), **quality(point()))
    for steps in (40, a.plane_steps):
        ar = C._check_align(iters=steps)
        plane = lambda: C._align(torch, ops, src, tgt, ar, None, None, False, ops.cloud_normals(tgt.points, tgt.offsets, 16)[0])
        res[f"align_plane_{steps}_steps_with_the_normals_pass"] = dict(event_ms(plane, a.reps), **quality(plane()))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
