"""Timing of the subject-isolation kernels on an MI355X: the RANSAC floor plane and the Euclidean clusters.  Writes
profiles/cloud_isolate_time.json (--out).

    python profiles/scripts/cloud_isolate_time.py

The fixture: the geodesic fixture's body, its surface sampled (mesh_io.sample_surface) to 8 clouds x 300 000 points, each standing on a floor
disc of radius 1.5 m with 100 000 samples and +-3 mm noise.  The protocol of profiles/scripts/cloud_time.py: HIP-event time per call, median /
min / max over --reps calls after 3 warm-up calls.  Timed: cloud.fit_plane's launches (H = 1 024, tau = 2 cm, up = +y within 10 degrees) and
etch_cloud_plane_score alone with and without the tilt limit (it evaluates the valid planes only); ops.cloud_components at r = 1 cm in the grid form (keys, sorts and gather included), etch_cloud_components alone on
the sorted grid next to etch_cloud_radius_count on the same grid, and the brute form (at 50 000 + 16 667 points per cloud where one call at full
size exceeds --brute-budget); cloud.prepare with every stage on the host clock."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from etch_amd import _lib
from etch_amd import cloud as C
from etch_amd import mesh_io, ops
from etch_amd.depth import Cloud
from etch_amd.inference_demo import Mesh

GOLDEN = os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz")
CLOUDS, H, TAU, R = 8, 1024, 0.02, 0.01
UP = (0.0, 1.0, 0.0)


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


def scene(body, n_body, n_floor):
    """CLOUDS clouds: n_body surface samples of the body standing on n_floor samples of a noisy floor disc, rows in one random order."""
    _, _, _, p64 = mesh_io.sample_surface([body] * CLOUDS, n_body, list(range(1, CLOUDS + 1)), center=False, return_fp64=True)
    b = p64.cpu().numpy()
    v = np.asarray(body.vertices)
    rng = np.random.default_rng(7)
    cx, cz = (v[:, 0].min() + v[:, 0].max()) / 2.0, (v[:, 2].min() + v[:, 2].max()) / 2.0
    clouds = []
    for k in range(CLOUDS):
        rad, ang = 1.5 * np.sqrt(rng.uniform(0.0, 1.0, n_floor)), rng.uniform(0.0, 2.0 * np.pi, n_floor)
        floor = np.stack([cx + rad * np.cos(ang), v[:, 1].min() - 0.003 + rng.uniform(-0.003, 0.003, n_floor), cz + rad * np.sin(ang)], 1)
        clouds.append(rng.permutation(np.concatenate([b[k], floor])))
    n = n_body + n_floor
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds))).cuda()
    off = (torch.arange(CLOUDS + 1, dtype=torch.int64) * n).to(torch.int32).cuda()
    idx = torch.arange(n, dtype=torch.int32).repeat(CLOUDS).cuda()
    return Cloud(pts, idx, off, off[1:] - off[:-1], None)


def components_alone(cl):
    """etch_cloud_components and etch_cloud_radius_count on one sorted mode-1 grid: -> two callables."""
    P, O = cl.points, cl.offsets
    B, M = O.numel() - 1, P.shape[0]
    _, status, sp, sk, order = ops.cloud_cell_grid(P, O, 1, 1, R)
    parent, label, size, count = (torch.zeros((M,), dtype=torch.int32, device=P.device) for _ in range(4))
    comp = lambda: _lib.call("etch_cloud_components", B, M, R, 0, sp, sk, order, O, status, parent, label, size)
    radius = lambda: _lib.call("etch_cloud_radius_count", B, M, R, 0, sp, sk, order, O, status, count)
    return comp, radius


def ratio(grid, brute):
    spread = max(grid["max_ms"] - grid["min_ms"], brute["max_ms"] - brute["min_ms"])
    return {"brute_over_grid": round(brute["median_ms"] / grid["median_ms"], 1), "difference_ms": round(brute["median_ms"] - grid["median_ms"], 3),
            "larger_spread_ms": round(spread, 3), "difference_exceeds_twice_the_spread": bool(brute["median_ms"] - grid["median_ms"] > 2.0 * spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_isolate_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--floor-points", type=int, default=100000)
    ap.add_argument("--brute-budget", type=float, default=60.0, help="seconds the brute-force leg may take at --points")
    a = ap.parse_args()
    z = np.load(GOLDEN)
    body = Mesh(z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64))
    cl = scene(body, a.points, a.floor_points)
    P, O = cl.points, cl.offsets
    keys = list(range(1, CLOUDS + 1))
    res = {"clouds": CLOUDS, "points_per_cloud": a.points + a.floor_points, "floor_points_per_cloud": a.floor_points, "hypotheses": H, "tau_m": TAU,
           "radius_m": R, "device": torch.cuda.get_device_name(0)}
    args = C._check_plane(CLOUDS, TAU, keys, H, UP, 10.0)
    res["fit_plane"] = event_ms(lambda: C._plane(torch, ops, cl, args), a.reps)
    plane, counts, found, _ = C._plane(torch, ops, cl, args)
    res["fit_plane_found"] = [int(x) for x in found.tolist()]
    res["fit_plane_counts"] = counts.tolist()
    free = C._check_plane(CLOUDS, TAU, keys, H)                      # without up every hypothesis of three distinct rows spanning a plane is valid
    res["fit_plane_without_up"] = event_ms(lambda: C._plane(torch, ops, cl, free), a.reps)
    out = torch.empty((CLOUDS, H, 3), dtype=torch.int32, device=P.device)
    for name, arg in (("plane_score_alone_up_10_degrees", args), ("plane_score_alone_without_up", free)):      # the kernel evaluates valid planes only
        planes, valid = ops.cloud_plane_hypotheses(P, O, torch.from_numpy(arg["keys"]).cuda(), H, up=arg["up"], cos_tilt=arg["cos_tilt"])
        t = event_ms(lambda: _lib.call("etch_cloud_plane_score", CLOUDS, P.shape[0], H, TAU, P, O, planes, valid, out), a.reps)
        ev = float(valid.sum()) * (a.points + a.floor_points)
        res[name] = dict(t, valid_planes=int(valid.sum()), evaluations=ev, evaluations_per_ns=round(ev / (t["median_ms"] * 1e6), 2))
    res["components_grid"] = event_ms(lambda: ops.cloud_components(P, O, R), a.reps)
    comp, radius = components_alone(cl)
    res["components_kernels_alone"] = event_ms(comp, a.reps)
    res["radius_count_kernel_alone_same_grid"] = event_ms(radius, a.reps)
    label, size, _ = ops.cloud_components(P, O, R)
    res["components_largest"] = [int(size[int(O[b]):int(O[b + 1])].max()) for b in range(CLOUDS)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bl, bs, _ = ops.cloud_components(P, O, R, brute=True)
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    res["components_brute_first_call_s"] = round(one, 3)
    res["grid_and_brute_equal"] = bool(torch.equal(bl, label) and torch.equal(bs, size))
    if one * (a.reps + 3) <= a.brute_budget:
        res["components_brute"] = event_ms(lambda: ops.cloud_components(P, O, R, brute=True), a.reps)
        res["components_ratio"] = dict(ratio(res["components_grid"], res["components_brute"]), points_per_cloud=a.points + a.floor_points)
    else:
        small = scene(body, 50000, 16667)
        g = event_ms(lambda: ops.cloud_components(small.points, small.offsets, R), a.reps)
        b = event_ms(lambda: ops.cloud_components(small.points, small.offsets, R, brute=True), a.reps)
        res["components_at_66667"] = {"grid": g, "brute": b}
        res["components_ratio"] = dict(ratio(g, b), points_per_cloud=66667,
                                       note=f"one brute-force call at {a.points + a.floor_points} points per cloud took {one:.2f} s: the brute-force leg is "
                                            "timed at 66 667; not extrapolated")
    t = []
    floor = dict(threshold=TAU, hypotheses=H, up=UP, max_tilt=10.0)
    for _ in range(a.reps + 2):
        t0 = time.perf_counter()
        p32, c, clean = C.prepare(cl, 5000, keys, voxel=0.01, stat=(16, 2.0), radius=(0.01, 2), floor=floor, cluster=(R, 100))
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(np.array(t[2:]))
    res["prepare"] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3), "points_picked": 5000,
                      "rows": {k: [int(x) for x in v] for k, v in clean.stages.items()},
                      "note": "host clock: offsets check, statistical filter (k = 16, ratio 2), radius filter (1 cm, 2), floor, largest cluster (1 cm), "
                              "voxel grid 1 cm, centre, pick, one readback"}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
