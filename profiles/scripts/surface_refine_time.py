"""Dense surface refinement timing at 32 scans x 5 000 inner points against SyntheticSurfaceSMPL (6 890 vertices, 13 776 faces): the
closest-point kernel alone (point-triangle tests per second), the whole refinement per iteration, and fit_cham's schedule at the same
shape beside it.  Device events after a warm-up run.  Every measurement is a step of its own: without --step this program starts one child
per step under that step's time limit, stops at the first one that fails, and writes profiles/surface_refine_time.json.

    python profiles/scripts/surface_refine_time.py [--iters 20] [--out profiles/surface_refine_time.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
STEPS = {"closest": 120, "surface_refine": 240, "fit_cham": 240}      # step -> its time limit in seconds

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--N", type=int, default=5000)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--step", choices=sorted(STEPS), default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_refine_time.json"))
a = ap.parse_args()

if a.step is None:
    res = {"B": a.B, "N": a.N, "iters": a.iters}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--B", str(a.B), "--N", str(a.N), "--iters", str(a.iters), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step} ran into its {limit} s limit: nothing further is started")
        if r.returncode != 0:
            sys.exit(f"step {step} failed with status {r.returncode}: nothing further is started\n{r.stderr[-2000:]}")
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    res["surface_over_fit_cham"] = round(res["surface_refine_ms_per_iteration"] / res["fit_cham_ms_per_iteration"], 3)
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

dev = torch.device("cuda")
bm = SyntheticSurfaceSMPL(7)
db = _bm_tables(bm, dev)
faces = torch.from_numpy(bm.faces).to(dev)
rng = np.random.default_rng(0)
B, N, V, F = a.B, a.N, bm.num_verts, len(bm.faces)
params0 = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
params0 = torch.from_numpy(params0.astype(np.float32)).to(dev)
verts = ops.smpl_lbs(db.lbs_consts, torch.cat([params0[:, 3:72], params0[:, 72:82], params0[:, :3], params0[:, 82:85]], 1).contiguous(), V, db.n_extra)[0]
pts = torch.stack([verts[b, torch.from_numpy(rng.choice(V, N)).to(dev)] for b in range(B)]) + 0.003 * torch.randn(B, N, 3, device=dev)
pts = pts.contiguous()
start = params0.clone()
start[:, :72] += 0.03 * torch.randn(B, 72, device=dev)


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


if a.step == "closest":
    ms = timed(lambda: ops.point_mesh_closest(pts, verts.contiguous(), faces), 5)
    out = {"V": V, "F": F, "closest_ms": round(ms, 4), "closest_tests_per_s": B * N * F / (ms * 1e-3)}
elif a.step == "surface_refine":
    ms = timed(lambda: ops.smpl_surface_refine(db.lbs_consts, faces, pts, start.clone(), iters=a.iters), a.reps)
    out = {"surface_refine_ms": round(ms, 3), "surface_refine_ms_per_iteration": round(ms / a.iters, 4)}
else:
    ms = timed(lambda: ops.smpl_chamfer_refine(db.lbs_consts, pts, start.clone(), V, iters=a.iters), a.reps)
    out = {"fit_cham_ms": round(ms, 3), "fit_cham_ms_per_iteration": round(ms / a.iters, 4)}
print(json.dumps(out))
