"""Containment timing at 32 scans x 6 890 body vertices x an 81 920-face closed scan mesh (an icosphere refined six times, scaled to the
body's bounding box): the winding-number kernel alone ((query, face) pairs per second, and its share of the bound counted from the gfx950
disassembly), the ragged closest-point pass, one refresh (both passes and the term), and fit_surface's schedule per iteration with
containment refreshed every iteration (K = 1) and every tenth (K = 10) beside the dense-only refinement through the entry point it always
used, in the same run.  Device events after a warm-up run.  Every measurement is a step of its own: without --step this program starts one
child per step under that step's time limit, stops at the first one that fails, and writes profiles/containment_time.json.

    python profiles/scripts/containment_time.py [--iters 20] [--out profiles/containment_time.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
STEPS = {"winding": 120, "closest": 120, "refresh": 120, "dense_only": 120, "contain_k1": 240, "contain_k10": 240}      # step -> its time limit in seconds

# The inner loop of wn_tile_kernel in the gfx950 disassembly (hipcc -O3 -ffp-contract=off, one 256-face-tile iteration = one face against a
# thread's two queries): 276 vector-ALU instructions, of which 8 are quarter-rate (6 v_sqrt_f32, 2 v_rcp_f32) and 73 packed-fp32
# (v_pk_mul / v_pk_add / v_pk_fma / v_pk_mov), + 5 LDS reads and 11 scalar.  Issue cost per wave: 4 cycles a plain instruction, 8 a
# quarter-rate one; a packed-fp32 instruction between 4 (lower bound) and 8 (if it issues as two passes).  One iteration serves 64 lanes x 2
# queries = 128 pairs.
WN_VALU, WN_QUARTER, WN_PACKED, WN_PAIRS = 276, 8, 73, 128
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--N", type=int, default=5000)
ap.add_argument("--subdiv", type=int, default=6)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--step", choices=sorted(STEPS), default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "containment_time.json"))
a = ap.parse_args()

if a.step is None:
    res = {"B": a.B, "N": a.N, "iters": a.iters}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ("B", "N", "subdiv", "iters", "reps") for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step} ran into its {limit} s limit: nothing further is started")
        if r.returncode != 0:
            sys.exit(f"step {step} failed with status {r.returncode}: nothing further is started\n{r.stderr[-2000:]}")
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    # cycles per iteration: every instruction at 4 (the floor of the count), quarter-rate ones at 8, packed ones at 8 too
    cycles = {"all_4": WN_VALU * 4, "quarter_8": (WN_VALU - WN_QUARTER) * 4 + WN_QUARTER * 8}
    cycles["quarter_8_packed_8"] = cycles["quarter_8"] + WN_PACKED * 4
    res["winding_bound_pairs_per_s"] = {k: SIMDS * CLOCK_HZ * WN_PAIRS / c for k, c in cycles.items()}
    res["winding_fraction_of_bound"] = {k: round(res["winding_pairs_per_s"] / b, 3) for k, b in res["winding_bound_pairs_per_s"].items()}
    # the launch computes whole 512-query blocks: the pairs the lanes actually evaluate, idle rows of the last block included
    res["winding_pairs_per_s_with_idle_rows"] = res["winding_pairs_per_s"] * (-(-res["V"] // 512) * 512) / res["V"]
    for k in ("contain_k1", "contain_k10"):
        res[k + "_over_dense_only"] = round(res[k + "_ms_per_iteration"] / res["dense_only_ms_per_iteration"], 3)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0)

import numpy as np
import torch

from etch_amd import ops
from etch_amd.models.chamfer_refine import _bm_tables
from etch_amd.utils.body_model import SyntheticSurfaceSMPL


def icosphere(subdiv):
    """Unit icosphere, 20 * 4^subdiv outward faces (vectorised midpoint subdivision)."""
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
B, N, V, F = a.B, a.N, bm.num_verts, len(bm.faces)
params0 = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
params0 = torch.from_numpy(params0.astype(np.float32)).to(dev)
verts = ops.smpl_lbs(db.lbs_consts, torch.cat([params0[:, 3:72], params0[:, 72:82], params0[:, :3], params0[:, 82:85]], 1).contiguous(), V, db.n_extra)[0].contiguous()
pts = torch.stack([verts[b, torch.from_numpy(rng.choice(V, N)).to(dev)] for b in range(B)]) + 0.003 * torch.randn(B, N, 3, device=dev)
pts = pts.contiguous()
start = params0.clone()
start[:, :72] += 0.03 * torch.randn(B, 72, device=dev)

# the scan of every body: the ellipsoid of 0.9 x its bounding box, so part of the body pokes out
sv, sf = icosphere(a.subdiv)
lo, hi = verts.amin(1).cpu().numpy().astype(np.float64), verts.amax(1).cpu().numpy().astype(np.float64)
scan_v = np.concatenate([sv * (0.45 * (hi[b] - lo[b])) + 0.5 * (hi[b] + lo[b]) for b in range(B)]).astype(np.float32)
SF = len(sf)
t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)
scan = (t(scan_v, torch.float32), t(np.tile(sf, (B, 1)), torch.int32), t(np.arange(B + 1) * len(sv), torch.int32), t(np.arange(B + 1) * SF, torch.int32), SF)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def refresh():
    w = ops.mesh_winding_number(scan, verts)
    face, bary, d2 = ops.ragged_mesh_closest(scan, verts)
    return ops.containment_energy_grad(verts, scan, w, face, bary, d2)


if a.step == "winding":
    ms = timed(lambda: ops.mesh_winding_number(scan, verts), 3)
    share = float((ops.mesh_winding_number(scan, verts).abs() < 0.5).float().mean())
    out = {"V": V, "scan_faces": SF, "winding_ms": round(ms, 3), "winding_pairs_per_s": B * V * SF / (ms * 1e-3), "outside_share_at_start": round(share, 4)}
elif a.step == "closest":
    ms = timed(lambda: ops.ragged_mesh_closest(scan, verts), 3)
    out = {"ragged_closest_ms": round(ms, 3), "ragged_closest_tests_per_s": B * V * SF / (ms * 1e-3)}
elif a.step == "refresh":
    out = {"refresh_ms": round(timed(refresh, 3), 3)}
elif a.step == "dense_only":
    ms = timed(lambda: ops.smpl_surface_refine(db.lbs_consts, faces, pts, start.clone(), iters=a.iters), a.reps)
    out = {"dense_only_ms_per_iteration": round(ms / a.iters, 4)}
else:
    K = 1 if a.step == "contain_k1" else 10
    ms = timed(lambda: ops.smpl_surface_refine_contain(db.lbs_consts, faces, pts, start.clone(), scan, iters=a.iters, contain_every=K), a.reps)
    out = {a.step + "_ms_per_iteration": round(ms / a.iters, 4)}
print(json.dumps(out))
