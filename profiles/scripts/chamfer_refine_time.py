"""Chamfer refinement timing: the two-way nearest-neighbour pass alone (pairs/s) and the whole 500-iteration refine per batch, at
32 scans x 5 000 scan points against SyntheticSMPL (6 890 vertices), device events after a warm-up run.  Kernel breakdown: run this
under `rocprofv3 --kernel-trace --stats -- python profiles/scripts/chamfer_refine_time.py --iters 20` as a separate step."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from etch_amd import ops
from etch_amd.models.chamfer_refine import _bm_tables
from etch_amd.utils.body_model import SyntheticSMPL

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=32)
ap.add_argument("--N", type=int, default=5000)
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda")
bm = SyntheticSMPL(7)
db = _bm_tables(bm, dev)
rng = np.random.default_rng(0)
B, N, V = a.B, a.N, bm.num_verts
params0 = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
params0 = torch.from_numpy(params0.astype(np.float32)).to(dev)
verts = ops.smpl_lbs(db.lbs_consts, torch.cat([params0[:, 3:72], params0[:, 72:82], params0[:, :3], params0[:, 82:85]], 1).contiguous(), V, db.n_extra)[0]
scan = torch.stack([verts[b, torch.from_numpy(rng.choice(V, N)).to(dev)] for b in range(B)]) + 0.003 * torch.randn(B, N, 3, device=dev)
scan = scan.contiguous()


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


nn_ms = timed(lambda: ops.nn_bidir(scan, verts), 20)
pairs = B * N * V
refine_ms = timed(lambda: ops.smpl_chamfer_refine(db.lbs_consts, scan, params0.clone(), V, iters=a.iters), a.reps)
res = {"B": B, "N": N, "V": V, "nn_bidir_ms": round(nn_ms, 4), "nn_pairs_per_s": pairs / (nn_ms * 1e-3), "iters": a.iters,
       "refine_ms_per_batch": round(refine_ms, 3), "refine_ms_per_iteration": round(refine_ms / a.iters, 4)}
print(json.dumps(res))
