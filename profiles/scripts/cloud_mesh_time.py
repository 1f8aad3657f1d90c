"""A mesh from the winding field, timed: cloud.reconstruct pass by pass -- the lattice, the field of every round, the face test,
the extraction, the components -- and as a whole call, on section 26e's 8 ellipsoid clouds on 5 mm voxels (at most 46 178 rows) at voxel 0.01 and
0.005, and on the three views of the fixture body (6 721 rows) at voxel 0.01.  The field's rate in pairs (node, row) per second stands next to
section 26e's etch_cloud_winding_number at 1.017e12.

HIP events on the stream; 3 warm-up calls, then the median [min, max] of 30.  Every shape is a step of its own: without --step this program starts
one child per step under that step's time limit, stops at the first one that fails, and writes profiles/cloud_mesh_time.json.

    python profiles/scripts/cloud_mesh_time.py [--out profiles/cloud_mesh_time.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = {"fixture_10mm": 300, "ellipsoids_10mm": 400, "ellipsoids_5mm": 600}     # step -> its time limit, s

# The inner loop of cm_field_kernel in the gfx950 disassembly (hipcc -O3 -ffp-contract=off; one iteration = one row against a thread's three nodes):
# 131 vector-ALU instructions, of which 6 are quarter-rate (3 v_sqrt_f32, 3 v_rcp_f32) and 12 packed fp32, + 2 LDS reads, 21 s_nop and 12 other
# scalar.  Issue cost per wave as DESIGN 18c and 26c count it: 4 cycles a plain instruction, 8 a quarter-rate one.  One iteration serves 64 lanes x 3
# nodes = 192 pairs, of which 729 / 768 are nodes of the block.
CM_VALU, CM_QUARTER, CM_PAIRS = 131, 6, 192
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9
WINDING_PAIRS_PER_S = 1.017e12

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--rows", type=int, default=300000)
ap.add_argument("--cloud_voxel", type=float, default=0.005)
ap.add_argument("--step", choices=sorted(STEPS), default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_mesh_time.json"))
a = ap.parse_args()

if a.step is None:
    cyc = (CM_VALU - CM_QUARTER) * 4 + CM_QUARTER * 8
    res = {"calls": "3 warm-up, then median [min, max] of 30", "field_loop": {"valu": CM_VALU, "quarter_rate": CM_QUARTER, "pairs": CM_PAIRS, "cycles": cyc},
           "field_bound_pairs_per_s": SIMDS * CLOCK_HZ * CM_PAIRS / cyc, "cloud_winding_number_pairs_per_s": WINDING_PAIRS_PER_S}
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--B", str(a.B), "--rows", str(a.rows), "--cloud_voxel", str(a.cloud_voxel)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step} ran into its {limit} s limit: nothing further is started")
        if r.returncode != 0:
            sys.exit(f"step {step} failed with status {r.returncode}: nothing further is started\n{r.stderr[-2000:]}")
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"step {step}: {r.stdout.strip().splitlines()[-1]}", file=sys.stderr, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0)

import numpy as np
import torch

from etch_amd import cloud, ops

dev = torch.device("cuda")


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


def ellipsoids():
    """Section 26e's subject: per body the ellipsoid of 0.9 x its bounding box, `rows` samples each, on a voxel grid of `cloud_voxel`."""
    from etch_amd.models.chamfer_refine import _bm_tables
    from etch_amd.utils.body_model import SyntheticSurfaceSMPL
    bm = SyntheticSurfaceSMPL(7)
    db = _bm_tables(bm, dev)
    rng = np.random.default_rng(0)
    B, V = a.B, bm.num_verts
    p0 = np.concatenate([rng.standard_normal((B, 72)) * 0.1, rng.standard_normal((B, 10)) * 0.5, np.zeros((B, 3)), np.ones((B, 1))], 1)
    p0 = torch.from_numpy(p0.astype(np.float32)).to(dev)
    verts = ops.smpl_lbs(db.lbs_consts, torch.cat([p0[:, 3:72], p0[:, 72:82], p0[:, :3], p0[:, 82:85]], 1).contiguous(), V, db.n_extra)[0]
    lo, hi = verts.amin(1).cpu().numpy().astype(np.float64), verts.amax(1).cpu().numpy().astype(np.float64)
    axes, mid = 0.45 * (hi - lo), 0.5 * (hi + lo)
    pts = []
    for b in range(B):
        d = rng.standard_normal((a.rows, 3))
        d /= np.sqrt((d * d).sum(1))[:, None]
        pts.append(d * axes[b] + mid[b])
    out, _ = cloud.voxel_downsample(cloud.pack(pts, device=dev), a.cloud_voxel)
    o, p = out.offsets.cpu().numpy(), out.points.cpu().numpy()
    nrm = []
    for b in range(B):
        g = (p[o[b]:o[b + 1]] - mid[b]) / (axes[b] * axes[b])
        nrm.append(g / np.sqrt((g * g).sum(1))[:, None])
    return cloud.surface(out, normals=np.concatenate(nrm))


def fixture():
    import _cloud_winding_oracle as WO
    p, n, flag, _, _ = WO.body_views()
    pos, moment, cap = WO.surface(p, n, 8, flag)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    return cloud.OrientedCloud(t(pos), t(moment), t(cap), t(np.array([0, len(pos)], np.int32)), len(pos))


oc = fixture() if a.step.startswith("fixture") else ellipsoids()
h = 0.005 if a.step.endswith("5mm") else 0.01
B = int(oc.offsets.numel()) - 1
rows = np.diff(oc.offsets.cpu().numpy())

# the rounds once, as cloud.reconstruct walks them, keeping every round's slots
lattice, status = ops.cloud_mesh_lattice(oc, h, 2)
lat = lattice.cpu().numpy().astype(np.int64)
toff_host = np.concatenate([[0], np.cumsum((lat[:, 3:] - lat[:, :3]).prod(1))]).astype(np.int64)
toff = torch.from_numpy(toff_host).to(dev)
table = torch.full((int(toff_host[-1]),), ops.MESH_TABLE_INACTIVE, dtype=torch.int32, device=dev)
ops.cloud_mesh_seed(oc, h, 0, lattice, status, toff, table)
per_round, n_slots = [], 0
while True:
    new = torch.nonzero(table == ops.MESH_TABLE_MARK, as_tuple=False)[:, 0]
    if new.numel() == 0:
        break
    of = torch.bucketize(new, toff[1:], right=True)
    sl = torch.stack([of, new - toff[of]], 1).to(torch.int32).contiguous()
    table[new] = torch.arange(n_slots, n_slots + new.numel(), dtype=torch.int32, device=dev)
    n_slots += int(new.numel())
    fld = ops.cloud_mesh_field(oc, h, 0.5, lattice, sl)
    before = table.clone()
    ops.cloud_mesh_grow(lattice, toff, sl, fld, table)
    per_round.append((sl, fld, before, of))

out = {"clouds": B, "rows_total": int(rows.sum()), "rows_max": int(rows.max()), "voxel": h, "blocks": n_slots, "lattice_blocks": int(toff_host[-1]),
       "nodes": n_slots * 729, "rounds": len(per_round) - 1, "lattice_ms": timed(lambda: ops.cloud_mesh_lattice(oc, h, 2)), "field_rounds": []}
pairs_all, field_ms_all = 0, 0.0
for sl, fld, before, of in per_round:
    pairs = int((torch.from_numpy(rows).to(dev)[of] * 729).sum())
    ms = timed(lambda: ops.cloud_mesh_field(oc, h, 0.5, lattice, sl))
    grow = timed(lambda: ops.cloud_mesh_grow(lattice, toff, sl, fld, before.clone()))
    out["field_rounds"].append({"blocks": int(sl.shape[0]), "pairs": pairs, "field_ms": ms, "pairs_per_s": pairs / (ms[0] * 1e-3), "grow_ms_with_a_table_copy": grow})
    pairs_all, field_ms_all = pairs_all + pairs, field_ms_all + ms[0]
out.update(pairs=pairs_all, field_ms_all_rounds=round(field_ms_all, 4), field_pairs_per_s=pairs_all / (field_ms_all * 1e-3))
out["field_over_cloud_winding_number"] = round(out["field_pairs_per_s"] / WINDING_PAIRS_PER_S, 3)
sl, fld = torch.cat([r[0] for r in per_round]), torch.cat([r[1] for r in per_round])
order = torch.argsort(sl[:, 0].long() * (1 << 32) + sl[:, 1].long())
sl, fld = sl[order].contiguous(), fld[order].contiguous()
out["extract_ms"] = timed(lambda: ops.cloud_mesh_extract(lattice, h, sl, fld))
counts, keys, fpos = ops.cloud_mesh_extract(lattice, h, sl, fld)
f_end = np.cumsum(torch.zeros((B,), dtype=torch.int64, device=dev).index_add_(0, sl[:, 0].long(), counts.sum(1, dtype=torch.int64)).cpu().numpy())
welded = [ops.cloud_mesh_weld(keys[(f_end[b - 1] if b else 0):f_end[b]], fpos[(f_end[b - 1] if b else 0):f_end[b]]) for b in range(B)]
out["weld_ms"] = timed(lambda: [ops.cloud_mesh_weld(keys[(f_end[b - 1] if b else 0):f_end[b]], fpos[(f_end[b - 1] if b else 0):f_end[b]]) for b in range(B)])
out["components_ms"] = timed(lambda: [ops.mesh_components(v.shape[0], f) for _, v, f in welded])
out["faces"], out["vertices"] = int(f_end[-1]), int(sum(v.shape[0] for _, v, _ in welded))
out["reconstruct_ms"] = timed(lambda: cloud.reconstruct(oc, h))
rec = cloud.reconstruct(oc, h)
out.update(closed=[bool(x) for x in rec.closed], components=[int(x) for x in rec.components], kept_faces=int(sum(len(m.faces) for m in rec.meshes)))
print(json.dumps(out))
