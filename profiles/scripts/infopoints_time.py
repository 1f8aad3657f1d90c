"""Info-point generation timing for one (scan, body) pair: the whole generate_infopoints call at 30 000 samples per scan (host sampling and
compaction included), and each ray query and the thinning alone with device events after a warm-up.  --scan_obj / --body_obj: a whole
frame (profiles/r08_infopoints_time.json: the reference's 4D-Dress frame 00122_Inner_Take2_00011, 80 000 scan faces, 13 776 body faces);
without them, the band of that frame kept in tests/golden/infopoints_4ddress.npz.  Ray/triangle tests per second = rays x faces / kernel time.  Kernel breakdown: run this under
`rocprofv3 --kernel-trace --stats -- python profiles/scripts/infopoints_time.py --reps 1` as a separate step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from etch_amd import infopoints as I
from etch_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--num_samples", type=int, default=30000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--scan_obj")
ap.add_argument("--body_obj")
a = ap.parse_args()


class M:
    def __init__(self, v, f):
        self.vertices, self.faces = v, f


if a.scan_obj and a.body_obj:
    from etch_amd.inference_demo import load_obj

    scan, body = load_obj(a.scan_obj), load_obj(a.body_obj)
else:
    d = np.load(os.path.join(ROOT, "tests", "golden", "infopoints_4ddress.npz"))
    scan, body = M(d["scan_vertices_e8"] / 1e8, d["scan_faces"]), M(d["body_vertices_e8"] / 1e8, d["body_faces"])
dev = torch.device("cuda")


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


S = a.num_samples
I.generate_infopoints(scan, body, num_samples=S, device=dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.reps):
    _, _, counts = I.generate_infopoints(scan, body, num_samples=S, device=dev)
torch.cuda.synchronize()
scan_s = (time.perf_counter() - t0) / a.reps

sv, sf = I.mesh_to_device(scan, dev)
bv, bf = I.mesh_to_device(body, dev)
pts, face, bary = I.sample_surface(body, S, seed=0)
s = torch.as_tensor(pts, device=dev)
n = I.interpolate_normals(ops.vertex_normals(bv, bf), bf, torch.as_tensor(face, device=dev), torch.as_tensor(bary, device=dev)).contiguous()
tm = torch.full((S,), 0.16, dtype=torch.float64, device=dev)
scan_ms = timed(lambda: ops.ray_first_hit(s, n, sv, sf, t_max=tm), 5)
body_ms = timed(lambda: ops.ray_first_hit(s, n, bv, bf, t_max=tm), 5)
cand = torch.as_tensor(I.sample_surface(body, 3 * S, seed=0)[0], device=dev)
thin_ms = timed(lambda: ops.remove_close(cand, 0.005), 5)
normals_ms = timed(lambda: ops.vertex_normals(bv, bf), 5)
close_ms = timed(lambda: ops.closest_point_on_mesh(s, bv, bf), 5)
F_s, F_b, C = sf.shape[0], bf.shape[0], cand.shape[0]
tests = 2 * S * F_s + S * F_b + (counts["samples"] - counts["rejected_test1"] - counts["rejected_test2"] - counts["rejected_test3"]) * F_b
res = {"num_samples": S, "scan_faces": F_s, "body_faces": F_b, "generate_s_per_scan": round(scan_s, 4), "counts": counts,
       "ray_tests_per_scan": tests, "ray_scan_ms": round(scan_ms, 4), "ray_scan_tests_per_s": S * F_s / (scan_ms * 1e-3),
       "ray_body_ms": round(body_ms, 4), "ray_body_tests_per_s": S * F_b / (body_ms * 1e-3), "thinning_ms": round(thin_ms, 4),
       "thinning_pairs_per_s": 2 * C * C / (thin_ms * 1e-3), "vertex_normals_ms": round(normals_ms, 4), "closest_point_ms": round(close_ms, 4),
       "closest_point_tests_per_s": S * F_b / (close_ms * 1e-3)}
print(json.dumps(res))
