"""Per-body time of the geodesic marker fields (etch_amd.geodesic.marker_fields: subdivision, intrinsic Delaunay flips, operators, 86 heat +
Poisson columns, min / argmin) on the committed 4D-Dress body at B = 1 and B = 8, with the iterations per column and the traffic model.

    python profiles/scripts/geodesic_time.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from etch_amd import geodesic as G  # noqa: E402


def main(out):
    z = np.load(os.path.join(ROOT, "tests", "golden", "geodesic_4ddress.npz"))
    v = z["vertices_q"].astype(np.int64) / 1e8
    f = z["faces"].astype(np.int64)
    mk = list(z["markers"])
    rng = np.random.default_rng(0)
    res = {}
    for B in (1, 8):
        verts = np.stack([v] + [v + rng.normal(0, 1e-3, v.shape) for _ in range(B - 1)])
        G.marker_fields(verts, f, mk, device="cuda")               # warm-up (topology caches, code objects)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = G.marker_fields(verts, f, mk, device="cuda")
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        it = r["iters"].numpy()
        res[f"B{B}"] = {"ms_total": 1e3 * min(ts), "ms_per_body": 1e3 * min(ts) / B, "heat_sweeps_mean": float(it[..., 0].mean()),
                        "heat_sweeps_max": int(it[..., 0].max()), "cg_iters_mean": float(it[..., 1].mean()), "cg_iters_max": int(it[..., 1].max()),
                        "flips": r["flips"]}
    V, E = r["vertices"].shape[1], 3 * len(f) * 4 // 2
    nnz = 2 * E
    # one sweep / CG iteration of a 4-column workgroup reads per nonzero: col (4 B) + w (8 B) + 4 neighbour values (32 B), per row ~ 100 B
    bytes_sweep = nnz * 44 + V * 100
    b1 = res["B1"]
    per_col_iters = b1["heat_sweeps_mean"] + b1["cg_iters_mean"] * 1.5
    res["model"] = {"V": int(V), "nnz": int(nnz), "bytes_per_workgroup_sweep": int(bytes_sweep),
                    "achieved_GBps_B1": bytes_sweep * per_col_iters * 22 / (b1["ms_total"] * 1e-3) / 1e9,
                    "achieved_GBps_B8": bytes_sweep * per_col_iters * 22 * 8 / (res["B8"]["ms_total"] * 1e-3) / 1e9}
    print(json.dumps(res))
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
