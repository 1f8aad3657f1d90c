"""Timing of the depth rasteriser against the ray caster it stands beside, on an MI355X.  Writes profiles/depth_time.json (--out).

    python profiles/scripts/depth_time.py                 everything below
    python profiles/scripts/depth_time.py --render-only   the render calls alone (profiler runs:
                                                          `rocprofv3 --kernel-trace --stats -- python profiles/scripts/depth_time.py --render-only --reps 5`)

  render        ops.render_depth of 8 views at 512 x 512 of the geodesic fixture's body with its faces midpoint-subdivided twice (220 416 faces), the
                batch already packed and uploaded; HIP-event time per call, median / min / max over --reps calls after 3 warm-up calls
  ray_first_hit the same 8 views through ops.ray_first_hit along the pixel-centre rays (262 144 rays per view): every view once, and view 0
                --ray-reps times for the spread
  full_image    the same call with a quad behind the body that fills every image (two faces through the large-face launch)
  partial_view_points   end to end on the host clock, 5 000 points per view: packing, upload, the six launches of render, compact, centre, pick, one readback
The rasteriser's and the ray caster's maps are compared and the differences recorded."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from etch_amd import depth as D
from etch_amd import mesh_io, ops
from etch_amd.inference_demo import Mesh

GOLDEN = os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz")
H = W = 512
VIEWS = 8


def subdivide(v, f):
    """Every face into four through its edge midpoints (shared edges share the midpoint)."""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, inv = np.unique(e, axis=0, return_inverse=True)
    mid = len(v) + inv.reshape(3, -1).T                           # (F,3): midpoints of edges 01, 12, 20
    v2 = np.concatenate([v, (v[uniq[:, 0]] + v[uniq[:, 1]]) / 2.0])
    a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], mid[:, 0], mid[:, 1], mid[:, 2]
    return v2, np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])


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


def uploaded(mesh, cams):
    v, f, voff, foff = mesh_io.pack_meshes([mesh])
    up = lambda a: torch.from_numpy(a).cuda()
    rows = np.stack([c.row() for c in cams])
    return (up(v), up(f), up(voff), up(foff), up(np.zeros(len(cams), np.int32)), up(rows)), int(foff[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_time.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ray-reps", type=int, default=3)
    ap.add_argument("--render-only", action="store_true")
    a = ap.parse_args()
    z = np.load(GOLDEN)
    v, f = z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)
    for _ in range(2):
        v, f = subdivide(v, f)
    body = Mesh(v, f)
    center = D.bbox_mid(v)
    cams = [D.Camera.orbit(center, 2.5, 2.0 * math.pi * k / VIEWS, math.radians(10.0), 45.0, H, W) for k in range(VIEWS)]
    args, F = uploaded(body, cams)
    render = lambda: ops.render_depth(*args, H, W, F)
    depth, face, _, dropped, status, large = render()
    res = {"faces": int(F), "views": VIEWS, "image": [H, W], "valid_pixels_per_view": [int(x) for x in torch.isfinite(depth).sum((1, 2)).tolist()],
           "large_faces_per_view": large.tolist(), "device": torch.cuda.get_device_name(0)}
    res["render"] = event_ms(render, a.reps)
    # a full-image face: a 20 m quad 1.5 m behind the body, seen from the front by all 8 views (slightly different elevations)
    n = len(v)
    quad = np.array([[-10.0, -10.0, -1.5], [10.0, -10.0, -1.5], [10.0, 10.0, -1.5], [-10.0, 10.0, -1.5]]) + center
    wall = Mesh(np.concatenate([v, quad]), np.concatenate([f, [[n, n + 1, n + 2], [n, n + 2, n + 3]]]))
    front = [D.Camera.orbit(center, 2.5, 0.0, math.radians(2.0 * k), 45.0, H, W) for k in range(VIEWS)]
    wargs, WF = uploaded(wall, front)
    wdepth, _, _, _, _, wlarge = ops.render_depth(*wargs, H, W, WF)
    assert bool(torch.isfinite(wdepth).all()) and wlarge.min() >= 2
    res["full_image"] = dict(event_ms(lambda: ops.render_depth(*wargs, H, W, WF), a.reps), large_faces_per_view=wlarge.tolist())
    fargs, _ = uploaded(body, front)
    res["full_image"]["same_views_without_the_quad"] = event_ms(lambda: ops.render_depth(*fargs, H, W, F), a.reps)
    if not a.render_only:
        dv, df = args[0], args[1]
        rays = []
        for c in cams:
            r, cc = np.divmod(np.arange(H * W), W)
            d = np.stack([(cc + 0.5 - c.cx) / c.fx, (r + 0.5 - c.cy) / c.fy, np.ones(H * W)], 1) @ c.R
            rays.append((torch.from_numpy(np.broadcast_to(c.eye, (H * W, 3)).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()))
        per_view, agree = [], []
        for k, (o, d) in enumerate(rays):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rf, rt, _, _ = ops.ray_first_hit(o, d, dv, df)
            e.record()
            torch.cuda.synchronize()
            per_view.append(round(s.elapsed_time(e), 3))
            # the two routes see the same image (the first call of view 0 also carries the code-object load: it is not the figure quoted)
            hit = (face[k].reshape(-1) >= 0) & (rf >= 0)
            agree.append([int(((face[k].reshape(-1) >= 0) != (rf >= 0)).sum()), int((face[k].reshape(-1) != rf).sum()),
                          float((depth[k].reshape(-1)[hit] - rt[hit]).abs().max())])
        again = event_ms(lambda: ops.ray_first_hit(*rays[0], dv, df), a.ray_reps, warm=0)
        res["ray_first_hit"] = {"per_view_ms_first_pass": per_view, "view0_again": again, "all_views_ms": round(float(sum(per_view[1:]) + again["median_ms"]), 3),
                                "ray_triangle_tests_per_view": H * W * F,
                                "against_the_rasteriser_per_view": {"coverage_face_differences_and_max_depth_difference": agree}}
        spread = max(res["render"]["max_ms"] - res["render"]["min_ms"], again["max_ms"] - again["min_ms"]) * VIEWS
        res["rasteriser_beats_ray_route_by_more_than_twice_the_spread"] = bool(res["ray_first_hit"]["all_views_ms"] - res["render"]["median_ms"] > 2.0 * spread)
        res["speedup"] = round(res["ray_first_hit"]["all_views_ms"] / res["render"]["median_ms"], 1)
        t = []
        keys = list(range(VIEWS))
        for _ in range(a.reps + 2):
            t0 = time.perf_counter()
            D.partial_view_points([body], cams, 5000, keys)
            t.append((time.perf_counter() - t0) * 1e3)
        t = np.sort(np.array(t[2:]))
        res["partial_view_points"] = {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3),
                                      "points_per_view": 5000, "note": "host clock: pack, upload, render, compact, centre, pick, one readback"}
        t0 = time.perf_counter()
        mesh_io.pack_meshes([body])
        res["partial_view_points"]["pack_on_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        cloud = D.unproject(depth, cams)
        cargs = (depth, torch.from_numpy(np.stack([c.row() for c in cams])).cuda())
        res["compact"] = event_ms(lambda: ops.depth_compact(*cargs), a.reps)
        dk = torch.arange(VIEWS, dtype=torch.int64).cuda()
        res["pick"] = event_ms(lambda: ops.depth_pick(cloud.offsets, cloud.index, cloud.points, dk, 5000), a.reps)
    if not a.render_only:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
