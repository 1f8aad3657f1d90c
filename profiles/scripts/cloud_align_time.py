"""Timing of the registration kernels on an MI355X.  Writes profiles/cloud_align_time.json (--out).

    python profiles/scripts/cloud_align_time.py

The fixture: the geodesic fixture's body, its surface sampled (mesh_io.sample_surface) to 8 target clouds x 300 000 points and 8 source clouds x
100 000 points (other samples of the same surface), the sources displaced by 10 degrees / 5 cm.  The protocol of profiles/scripts/cloud_time.py:
HIP-event time per call, median / min / max over --reps calls after 3 warm-up calls.  Timed: etch_cloud_nearest alone on a grid built before
(the kernel both forms share), in the grid and the brute form, at gates of 20 cm and 2 cm, converged and at the start pose, and at 20 cm with every other source row 1 m off the body (no partner: the
ring walk must end it, not a scan); ops.cloud_nearest with the grid,
the sorts and the gather; one whole cloud.align of 40 steps; cloud.register_views of 4 views of 100 000 points (host clock: it reads back once
per view).  The brute form runs at full size only where one call fits --brute-budget."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from etch_amd import _lib
from etch_amd import cloud as C
from etch_amd import mesh_io, ops
from etch_amd.depth import Cloud
from etch_amd.inference_demo import Mesh

GOLDEN = os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz")
PAIRS = 8


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


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    th = np.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def sampled(body, n, first_key, clouds=PAIRS):
    _, _, _, p64 = mesh_io.sample_surface([body] * clouds, n, list(range(first_key, first_key + clouds)), center=False, return_fp64=True)
    return p64.reshape(clouds * n, 3).contiguous()


def packed(points, n, clouds=PAIRS):
    off = (torch.arange(clouds + 1, dtype=torch.int64) * n).to(torch.int32).cuda()
    return Cloud(points, torch.arange(n, dtype=torch.int32).repeat(clouds).cuda(), off, off[1:] - off[:-1], None)


def nearest_alone(src, tgt, gate, brute, R, t):
    """etch_cloud_nearest on a grid built before: -> a callable, pair, d2."""
    grid, _, status, sp, sk, order = ops.cloud_align_grid(tgt.points, tgt.offsets, gate, sort=not brute)
    qorder = None if brute else ops._query_order(src.points, src.offsets, gate, 0.0)
    Ms = src.points.shape[0]
    pair = torch.full((Ms,), -1, dtype=torch.int32, device="cuda")
    d2 = torch.full((Ms,), np.inf, dtype=torch.float64, device="cuda")
    g = torch.tensor([gate], dtype=torch.float64, device="cuda")
    fn = lambda: _lib.call("etch_cloud_nearest", PAIRS, Ms, int(brute), src.points, src.offsets, qorder, tgt.points if brute else sp, sk, order,
                           tgt.offsets, grid, R, t, g, None, status, pair, d2)
    return fn, pair, d2


def ratio(grid, brute):
    spread = max(grid["max_ms"] - grid["min_ms"], brute["max_ms"] - brute["min_ms"])
    return {"brute_over_grid": round(brute["median_ms"] / grid["median_ms"], 1), "difference_ms": round(brute["median_ms"] - grid["median_ms"], 3),
            "larger_spread_ms": round(spread, 3), "grid_beats_brute_by_more_than_the_larger_spread": bool(brute["median_ms"] - grid["median_ms"] > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_align_time.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--target", type=int, default=300000)
    ap.add_argument("--source", type=int, default=100000)
    ap.add_argument("--brute-budget", type=float, default=120.0, help="seconds the brute-force legs may take in all")
    a = ap.parse_args()
    z = np.load(GOLDEN)
    body = Mesh(z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64))
    R0, t0 = rotation([0.3, 1.0, 0.2], 10.0), np.array([0.05, -0.025, 0.05 / 3.0])
    tgt = packed(sampled(body, a.target, 1), a.target)
    truth = sampled(body, a.source, 101)
    src = packed(((truth - torch.from_numpy(t0).cuda()) @ torch.from_numpy(R0).cuda()).contiguous(), a.source)
    placed = packed(truth, a.source)
    eye = torch.eye(3, dtype=torch.float64, device="cuda").repeat(PAIRS, 1, 1)
    zero = torch.zeros((PAIRS, 3), dtype=torch.float64, device="cuda")
    res = {"pairs": PAIRS, "target_rows_per_cloud": a.target, "source_rows_per_cloud": a.source, "start_pose": "10 degrees, 5 cm",
           "device": torch.cuda.get_device_name(0)}
    spent = 0.0
    for where, s in (("at_the_start_pose", src), ("converged", placed)):
        for gate in (0.2, 0.02):
            name = f"nearest_{where}_gate_{gate:g}"
            fn, gp, gd = nearest_alone(s, tgt, gate, False, eye, zero)
            res[name + "_grid"] = dict(event_ms(fn, a.reps), matched=int((gp >= 0).sum()))
            bf, bp, bd = nearest_alone(s, tgt, gate, True, eye, zero)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            bf()
            torch.cuda.synchronize()
            one = time.perf_counter() - t1
            res[name + "_brute_first_call_s"] = round(one, 3)
            res[name + "_equal"] = bool(torch.equal(bp, gp) and torch.equal(bd, gd))
            reps = a.reps if spent + one * (a.reps + 3) <= a.brute_budget else max(3, int((a.brute_budget - spent) / max(one, 1e-6) / 4) - 3)
            reps = max(3, min(a.reps, reps))
            spent += one * (reps + 3)
            res[name + "_brute"] = event_ms(bf, reps)
            res[name + "_ratio"] = ratio(res[name + "_grid"], res[name + "_brute"])
    # rows without a partner at the first gate, default cell: every other source row of the start pose lies 1 m off the body
    half = src.points.clone()
    half[::2, 0] += 1.0
    halved = packed(half, a.source)
    fn, gp, gd = nearest_alone(halved, tgt, 0.2, False, eye, zero)
    res["nearest_half_without_partner_gate_0.2_grid"] = dict(event_ms(fn, a.reps), matched=int((gp >= 0).sum()))
    bf, bp, bd = nearest_alone(halved, tgt, 0.2, True, eye, zero)
    res["nearest_half_without_partner_gate_0.2_brute"] = event_ms(bf, 5)
    res["nearest_half_without_partner_gate_0.2_equal"] = bool(torch.equal(bp, gp) and torch.equal(bd, gd))
    res["nearest_half_without_partner_gate_0.2_ratio"] = ratio(res["nearest_half_without_partner_gate_0.2_grid"], res["nearest_half_without_partner_gate_0.2_brute"])
    res["ops_cloud_nearest_gate_0.2_with_grid_sorts_gather"] = event_ms(lambda: ops.cloud_nearest(src.points, src.offsets, tgt.points, tgt.offsets, 0.2), a.reps)
    args = C._check_align()
    run = lambda: C._align(torch, ops, src, tgt, args, None, None, False)
    res["align_40_steps"] = event_ms(run, a.reps)
    out = run()
    res["align_steps_taken"] = out["steps"].tolist()
    res["align_matched"] = out["matched"].tolist()
    res["align_rms_m"] = [round(float(x), 6) for x in out["rms"].tolist()]
    Rg = out["R"].cpu().numpy()
    res["align_degrees_from_the_truth"] = [round(float(np.degrees(np.arccos(np.clip((np.trace(Rg[b] @ R0.T) - 1.0) / 2.0, -1.0, 1.0)))), 5) for b in range(PAIRS)]
    views = [packed(sampled(body, a.source, 201 + 10 * k, 1), a.source, 1) for k in range(4)]
    for k in range(1, 4):
        Rk, tk = rotation([0.3, 1.0, 0.2], 4.0 * k), np.array([0.02 * k, -0.01 * k, 0.005 * k])
        views[k] = packed(((views[k].points - torch.from_numpy(tk).cuda()) @ torch.from_numpy(Rk).cuda()).contiguous(), a.source, 1)
    t = []
    for _ in range(7):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        reg = C.register_views(views)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t1) * 1e3)
    t = np.sort(np.array(t[2:]))
    res["register_views_4_views"] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "reps": 5,
                                     "steps": [int(r.steps[0]) for r in reg], "matched": [int(r.matched[0]) for r in reg], "note": "host clock, one readback per view"}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
