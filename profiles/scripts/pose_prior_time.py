"""Timing record of the pose prior in the LM fit: the default 30 + 50 fit on SyntheticSMPL(7), B = 32 with one workgroup
per scan and B = 1 with the split fit, MI355X.

    python profiles/scripts/pose_prior_time.py [--parent_lib PATH] [--reps 15] [--out profiles/pose_prior_time.json]

Three variants take turns inside every repeat, each called through the C ABI with the same Python in front of it:
    (a) parent    no prior, the PARENT commit's kernel: --parent_lib, a shared library linked from the parent commit's etch_amd/csrc/smpl_fit.hip
                  alone (hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I etch_amd/csrc -I include -shared).  Left out when the flag is absent.
    (b) none      no prior, this commit (etch_smpl_lm_fit_split)
    (c) prior     GMM G = 8, D = 69 plus the four angle terms, this commit (etch_smpl_lm_fit_pose_prior)
Host clock around calls that end in a device synchronise.  The condition is (b) against (a): within twice the run-to-run spread of (a)
(DESIGN section 7).  (c) has no target; it is a record."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def main():
    import _pose_prior_oracle as P
    from etch_amd import _lib, ops
    from etch_amd.models.fit_SMPL import _device_body
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", default="")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_prior_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("pose_prior_time.py measures on the GPU; there is nothing to time without one")
    new = _lib.lib()._cdll
    parent = ctypes.CDLL(a.parent_lib) if a.parent_lib else None
    if parent is not None:
        parent.etch_smpl_lm_fit_split.restype = ctypes.c_int
    t = P.fit_tables(P.mixture(8, 69, seed=5), 2e-3, angles=True, w_ang=1e-2)
    pp = ops.PosePrior(t["means"], t["precisions"], t["nll_weights"], t["w_gmm"], t["angle_idx"], t["angle_sign"], t["w_ang"], device="cuda")
    vp, cf = ctypes.c_void_p, ctypes.c_float
    res = {"note": "ms per 30 + 50 fit [median, min, max], host clock around calls that end in a synchronise, the variants alternating inside every "
                   "repeat; spread = max - min of the parent's runs", "reps": a.reps, "cases": {}}
    for B, G in ((32, 1), (1, ops.lm_split_default(1, 24))):
        bm, ms, mv, tgt, valid, _ = P.problem(B, seed=3)
        db = _device_body(bm, mv, torch.device("cuda"))
        m, v = tgt.cuda().contiguous(), valid.float().cuda().contiguous()
        x, x0 = torch.empty(B, 85, device="cuda"), torch.empty(B, 85, device="cuda")
        ws = None
        if G > 1:
            ws = torch.empty((new.etch_smpl_lm_split_workspace_bytes(B, 24, 10, G) // 8 + 1,), dtype=torch.float64, device="cuda")
        arr = (vp * 7)(*[c.data_ptr() for c in db.lm_consts])
        head = lambda: (B, 86, 24, 10, arr, vp(m.data_ptr()), vp(v.data_ptr()), 30, cf(0.5), cf(0.01), 50, cf(0.2), cf(1e-3), vp(x.data_ptr()),
                        vp(x0.data_ptr()), None, None, G, None if ws is None else vp(ws.data_ptr()))
        st = lambda: vp(torch.cuda.current_stream().cuda_stream)
        fns = {}
        if parent is not None:
            fns["parent"] = lambda: parent.etch_smpl_lm_fit_split(*head(), st())
        fns["none"] = lambda: new.etch_smpl_lm_fit_split(*head(), st())
        fns["prior"] = lambda: new.etch_smpl_lm_fit_pose_prior(*head(), None, None, None, pp._tables, pp.G, pp.D, pp.n_ang, cf(pp.w_gmm), cf(pp.w_ang),
                                                               st())
        outs = {}
        for k, fn in fns.items():                     # warm-up, and a look at what each variant computes
            for _ in range(3):
                assert fn() == 0, k
            torch.cuda.synchronize()
            outs[k] = x.clone()
        ms_ = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms_[k].append((time.perf_counter() - t0) * 1e3)
        stat = {k: [round(float(np.median(q)), 4), round(float(np.min(q)), 4), round(float(np.max(q)), 4)] for k, q in ms_.items()}
        case = {"workgroups_per_scan": G, "ms": stat, "prior_over_none": round(stat["prior"][0] / stat["none"][0], 4),
                "prior_moves_x_by": float((outs["prior"] - outs["none"]).abs().max())}
        if parent is not None:
            spread = stat["parent"][2] - stat["parent"][1]
            case.update(none_minus_parent_ms=round(stat["none"][0] - stat["parent"][0], 4), parent_spread_ms=round(spread, 4),
                        within_twice_the_spread=bool(abs(stat["none"][0] - stat["parent"][0]) <= 2 * spread),
                        none_equals_parent_bitwise=bool(torch.equal(outs["none"], outs["parent"])))
        res["cases"][f"B={B}"] = case
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
