"""Point winding numbers, timed: the one pass of etch_cloud_winding_number (w, the nearest row and its d2) at 8 clouds x
300 000 rows x 6 890 queries and at the same clouds on 5 mm voxels, beside the mesh pair of passes it replaces (etch_mesh_winding_number +
etch_ragged_mesh_closest) on an 81 920-face mesh of the same subject; what building the oriented cloud costs (cloud.surface: normals, areas,
pack); and fit_surface's schedule per iteration at 32 bodies with the cloud refreshed every iteration (K = 1) and every tenth (K = 10), the shapes
of profiles/containment_time.json.  The subject is the ellipsoid of 0.9 x the body's bounding box, so part of the body pokes out.

HIP events on the stream; 3 warm-up calls, then the median [min, max] of 30 (of 5 for the refinement schedules, which are 20 iterations each).
Every measurement is a step of its own: without --step this program starts one child per step under that step's time limit, stops at the first
one that fails, and writes profiles/cloud_winding_time.json.

    python profiles/scripts/cloud_winding_time.py [--out profiles/cloud_winding_time.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
STEPS = {"cloud": 150, "voxel": 150, "mesh": 150, "surface": 150, "dense_only": 150, "contain_k1": 240, "contain_k10": 240}     # step -> its time limit, s

# The inner loop of cw_tile_kernel in the gfx950 disassembly (hipcc -O3 -ffp-contract=off; one iteration = one row against a thread's two queries):
# 95 vector-ALU instructions, of which 4 are quarter-rate (2 v_sqrt_f32, 2 v_rcp_f32) and 8 packed fp32, + 2 LDS reads (128 and 96 bit), 13 s_nop
# (17 wait states) and 8 scalar.  Issue cost per wave as DESIGN 18c counts it: 4 cycles a plain instruction, 8 a quarter-rate one, a packed one
# between 4 and 8.  One iteration serves 64 lanes x 2 queries = 128 pairs.
CW_VALU, CW_QUARTER, CW_PACKED, CW_PAIRS = 95, 4, 8, 128
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--rows", type=int, default=300000)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--fit_B", type=int, default=32)
ap.add_argument("--N", type=int, default=5000)
ap.add_argument("--subdiv", type=int, default=6)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--step", choices=sorted(STEPS), default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_winding_time.json"))
a = ap.parse_args()

if a.step is None:
    res = {"B": a.B, "rows": a.rows, "voxel": a.voxel, "fit_B": a.fit_B, "N": a.N, "iters": a.iters, "calls": "3 warm-up, then median [min, max] of 30 (fit: of 5)"}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step]
        cmd += [x for k in ("B", "rows", "voxel", "fit_B", "N", "subdiv", "iters") for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step} ran into its {limit} s limit: nothing further is started")
        if r.returncode != 0:
            sys.exit(f"step {step} failed with status {r.returncode}: nothing further is started\n{r.stderr[-2000:]}")
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"step {step}: {r.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
    cycles = {"all_4": CW_VALU * 4, "quarter_8": (CW_VALU - CW_QUARTER) * 4 + CW_QUARTER * 8}
    cycles["quarter_8_packed_8"] = cycles["quarter_8"] + CW_PACKED * 4
    res["cloud_bound_pairs_per_s"] = {k: SIMDS * CLOCK_HZ * CW_PAIRS / c for k, c in cycles.items()}
    pairs = a.B * a.rows * res["V"]
    res["cloud_bound_ms"] = {k: round(pairs / b * 1e3, 3) for k, b in res["cloud_bound_pairs_per_s"].items()}
    res["cloud_fraction_of_bound"] = {k: round(res["cloud_pairs_per_s"] / b, 3) for k, b in res["cloud_bound_pairs_per_s"].items()}
    res["cloud_pairs_per_s_with_idle_rows"] = res["cloud_pairs_per_s"] * (-(-res["V"] // 512) * 512) / res["V"]
    for k in ("contain_k1", "contain_k10"):
        for c in ("voxel", "rows"):
            res[f"{k}_{c}_over_dense_only"] = round(res[f"{k}_{c}_ms_per_iteration"][0] / res["dense_only_ms_per_iteration"][0], 3)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0)

import numpy as np
import torch

from etch_amd import cloud, ops
from etch_amd.models.chamfer_refine import _bm_tables
from etch_amd.utils.body_model import SyntheticSurfaceSMPL


def icosphere(subdiv):
    """Unit icosphere, 20 * 4^subdiv outward faces (profiles/scripts/containment_time.py's)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
                  (-t, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
                  (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(subdiv):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1) + len(v)
        v = np.concatenate([v, mid])
        ab, bc, ca = m
        f = np.concatenate([np.stack([f[:, 0], ab, ca], 1), np.stack([f[:, 1], bc, ab], 1), np.stack([f[:, 2], ca, bc], 1), np.stack([ab, bc, ca], 1)])
    return v, f.astype(np.int32)


dev = torch.device("cuda")
bm = SyntheticSurfaceSMPL(7)
db = _bm_tables(bm, dev)
faces = torch.from_numpy(bm.faces).to(dev)
rng = np.random.default_rng(0)
fit = a.step in ("dense_only", "contain_k1", "contain_k10")
B, N, V = (a.fit_B if fit else a.B), a.N, bm.num_verts
params0 = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
params0 = torch.from_numpy(params0.astype(np.float32)).to(dev)
verts = ops.smpl_lbs(db.lbs_consts, torch.cat([params0[:, 3:72], params0[:, 72:82], params0[:, :3], params0[:, 82:85]], 1).contiguous(), V, db.n_extra)[0].contiguous()
lo, hi = verts.amin(1).cpu().numpy().astype(np.float64), verts.amax(1).cpu().numpy().astype(np.float64)
axes, mid = 0.45 * (hi - lo), 0.5 * (hi + lo)                     # the subject of every body: the ellipsoid of 0.9 x its bounding box


def ellipsoid_normals(p, b):
    """The outward unit normal of ellipsoid b at (or near) its surface point p: the gradient of sum ((x - m) / a)^2."""
    g = (p - mid[b]) / (axes[b] * axes[b])
    return g / np.sqrt((g * g).sum(1))[:, None]


def sampled(rows):
    """rows points on every ellipsoid (directions uniform on the sphere, so denser where the ellipsoid is narrow: the areas take care of it) ->
    the packed Cloud and the normals by row."""
    pts, nrm = [], []
    for b in range(B):
        d = rng.standard_normal((rows, 3))
        d /= np.sqrt((d * d).sum(1))[:, None]
        pts.append(d * axes[b] + mid[b])
        nrm.append(ellipsoid_normals(pts[-1], b))
    return cloud.pack(pts, device=dev), np.concatenate(nrm)


def voxelised(packed):
    """The same clouds on a voxel grid: -> the Cloud of centroids and the ellipsoids' normals at them."""
    out, _ = cloud.voxel_downsample(packed, a.voxel)
    o = out.offsets.cpu().numpy()
    p = out.points.cpu().numpy()
    return out, np.concatenate([ellipsoid_normals(p[o[b]:o[b + 1]], b) for b in range(B)])


def timed(fn, reps=30, warm=3):
    """-> [median, min, max] ms of `reps` calls, each between two events, after `warm` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return [round(float(x), 4) for x in (np.median(ms), min(ms), max(ms))]


def per_iteration(fn):
    return [round(x / a.iters, 4) for x in timed(fn, reps=5, warm=1)]


if a.step in ("cloud", "voxel"):
    packed, nrm = sampled(a.rows)
    if a.step == "voxel":
        packed, nrm = voxelised(packed)
    oc = cloud.surface(packed, normals=nrm)
    rows = int(packed.points.shape[0])
    ms = timed(lambda: ops.cloud_winding_number(oc, verts))
    w, near, _ = ops.cloud_winding_number(oc, verts)
    out = {"V": V, a.step + "_rows_total": rows, a.step + "_rows_max": oc.max_rows, a.step + "_ms": ms,
           a.step + "_pairs_per_s": rows * V / (ms[0] * 1e-3), a.step + "_outside_share": round(float((w.abs() < 0.5).float().mean()), 4)}
elif a.step == "surface":
    packed, nrm = sampled(a.rows)
    sensors = torch.from_numpy(np.concatenate([np.repeat(mid[b:b + 1], a.rows, 0) for b in range(B)])).to(dev)
    far = (packed.points - sensors) * 4.0 + sensors                                # one sensor per row, outside, along the ray from the centre
    out = {"surface_given_normals_ms": timed(lambda: cloud.surface(packed, normals=nrm), reps=10),
           "surface_computed_normals_ms": timed(lambda: cloud.surface(packed, sensors=far), reps=10),
           "knn_kth_ms": timed(lambda: ops.cloud_knn_kth(packed.points, packed.offsets, 8), reps=10)}
elif a.step == "mesh":
    sv, sf = icosphere(a.subdiv)
    SF = len(sf)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)      # noqa: E731
    scan_v = np.concatenate([sv * axes[b] + mid[b] for b in range(B)]).astype(np.float32)
    scan = (t(scan_v, torch.float32), t(np.tile(sf, (B, 1)), torch.int32), t(np.arange(B + 1) * len(sv), torch.int32), t(np.arange(B + 1) * SF, torch.int32), SF)
    wn = timed(lambda: ops.mesh_winding_number(scan, verts))
    cl = timed(lambda: ops.ragged_mesh_closest(scan, verts))
    both = timed(lambda: (ops.mesh_winding_number(scan, verts), ops.ragged_mesh_closest(scan, verts)))
    out = {"mesh_faces": SF, "mesh_winding_ms": wn, "mesh_closest_ms": cl, "mesh_pair_of_passes_ms": both, "mesh_winding_pairs_per_s": B * V * SF / (wn[0] * 1e-3)}
else:
    pts = torch.stack([verts[b, torch.from_numpy(rng.choice(V, N)).to(dev)] for b in range(B)]) + 0.003 * torch.randn(B, N, 3, device=dev)
    pts = pts.contiguous()
    start = params0.clone()
    start[:, :72] += 0.03 * torch.randn(B, 72, device=dev)
    if a.step == "dense_only":
        out = {"dense_only_ms_per_iteration": per_iteration(lambda: ops.smpl_surface_refine(db.lbs_consts, faces, pts, start.clone(), iters=a.iters))}
    else:
        K = 1 if a.step == "contain_k1" else 10
        packed, nrm = sampled(a.rows)
        vox, vnrm = voxelised(packed)
        out = {}
        for name, (c, n) in (("voxel", (vox, vnrm)), ("rows", (packed, nrm))):
            oc = cloud.surface(c, normals=n)
            out[f"{a.step}_{name}_ms_per_iteration"] = per_iteration(
                lambda: ops.smpl_surface_refine_contain_cloud(db.lbs_consts, faces, pts, start.clone(), oc, iters=a.iters, contain_every=K))
            out[f"fit_{name}_rows_max"] = oc.max_rows
print(json.dumps(out))
