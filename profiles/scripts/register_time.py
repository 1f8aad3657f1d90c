"""SMPL+D registration timing: the whole schedule at 8 scans x 20 000 scan points against SyntheticSMPL (6 890 vertices),
300 iterations, beside fit_cham's schedule at the same B and N -- timed in the same process, alternating, device events, one warm-up
each, the median of 5.  Writes profiles/register_time.json (--out to write elsewhere).  Kernel shares: run this under
`rocprofv3 --kernel-trace --stats -- python profiles/scripts/register_time.py --iters 20 --reps 1 --out /dev/null` as a separate step."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from etch_amd import ops
from etch_amd.models.chamfer_refine import _bm_tables
from etch_amd.models.register import _edges_of, smooth_schedule
from etch_amd.utils.body_model import SyntheticSMPL

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--N", type=int, default=20000)
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "register_time.json"))
a = ap.parse_args()
dev = torch.device("cuda")
bm = SyntheticSMPL(7)
db = _bm_tables(bm, dev)
rng = np.random.default_rng(0)
B, N, V = a.B, a.N, bm.num_verts
params = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
params = torch.from_numpy(params.astype(np.float32)).to(dev)
base, R, _ = ops.smpl_skin_frames(db.lbs_consts, params)
D_true = 0.01 * torch.sin(2 * np.pi * torch.arange(1, 4, device=dev)[None, None, :] * torch.arange(V, device=dev)[None, :, None] / V).expand(B, -1, -1).contiguous()
target = ops.smpld_apply(base, R, D_true.float().contiguous())
scan = torch.stack([target[b, torch.from_numpy(rng.choice(V, N)).to(dev)] for b in range(B)]) + 0.003 * torch.randn(B, N, 3, device=dev)
scan = scan.contiguous()
ptr, idx, ne = _edges_of(bm, dev)
lam = smooth_schedule(10.0, 0.1, a.iters)


def register():
    ops.smpld_register(base, R, torch.zeros_like(base), scan, ptr, idx, ne, lam, trunc=0.05)


def refine():
    ops.smpl_chamfer_refine(db.lbs_consts, scan, params.clone(), V, iters=a.iters)


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


register(), refine()
torch.cuda.synchronize()
t_reg, t_ref = [], []
for _ in range(a.reps):
    t_reg.append(once(register))
    t_ref.append(once(refine))
reg_ms, ref_ms = float(np.median(t_reg)), float(np.median(t_ref))
res = {"B": B, "N": N, "V": V, "iters": a.iters, "reps": a.reps, "register_ms": round(reg_ms, 3), "register_ms_per_iteration": round(reg_ms / a.iters, 4),
       "fit_cham_ms": round(ref_ms, 3), "fit_cham_ms_per_iteration": round(ref_ms / a.iters, 4), "register_over_fit_cham": round(reg_ms / ref_ms, 4),
       "register_ms_all": [round(t, 3) for t in t_reg], "fit_cham_ms_all": [round(t, 3) for t in t_ref]}
print(json.dumps(res))
with open(a.out, "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
