"""Timing of the native scan ingestion against the routines it stands beside, in one process, alternating.  Each mode adds its
section to the JSON file (--out, default profiles/ingest_time.json).

    python profiles/scripts/ingest_time.py host SCAN.obj BODY.obj     no GPU: mesh_io.read_obj vs load_obj, mesh_io.write_obj vs Mesh.export
    python profiles/scripts/ingest_time.py sampler                    MI355X: mesh_io.sample_surface, B = 1 and 32 scans of 80 000 faces, vs
                                                                      sample_points_from_mesh; host clock around calls that end in a readback
    python profiles/scripts/ingest_time.py eval                       MI355X: scans/s of evaluate_dataset on 32 synthetic 80 000-face scans at batch 8
                                                                      with ingest host / device prefetch 0 / device prefetch 1
Kernel times: `rocprofv3 --kernel-trace --stats -- python profiles/scripts/ingest_time.py sampler --reps 5 --no-baseline` as a run of its own.
The synthetic scan is a seeded, displaced 200 x 200 torus grid: 40 000 vertices, 80 000 faces, about the size of a 4D-Dress frame."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

from etch_amd import mesh_io
from etch_amd.inference_demo import Mesh, load_obj, sample_points_from_mesh


def median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def alternate(fns, reps):
    """{name: (median, min, max) ms}: the candidates take turns inside every repeat, so a change of the host's load meets all of them."""
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in t.items()}


def synthetic_scan(seed, n=200):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(n) * 2 * np.pi / n, np.arange(n) * 2 * np.pi / n, indexing="ij")
    r = 0.12 + 0.01 * rng.standard_normal((n, n))
    verts = np.stack([(0.3 + r * np.cos(v)) * np.cos(u), 0.9 * (0.3 + r * np.cos(v)) * np.sin(u) + 1.0, r * np.sin(v)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b, c, d = i * n + j, ((i + 1) % n) * n + j, ((i + 1) % n) * n + (j + 1) % n, i * n + (j + 1) % n
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return Mesh(np.round(verts, 8), faces.astype(np.int64))


def mode_host(a):
    out = {"note": "ms per call: [median, min, max]; one thread; the routines alternate inside every repeat", "reps": a.reps}
    tmp = tempfile.mkdtemp()
    for name, path in (("scan", a.paths[0]), ("body", a.paths[1])):
        mesh = load_obj(path)
        size = os.path.getsize(path)
        r = alternate({"load_obj": lambda: load_obj(path), "read_obj": lambda: mesh_io.read_obj(path)}, a.reps)
        w = alternate({"Mesh.export": lambda: mesh.export(os.path.join(tmp, "a.obj")), "write_obj": lambda: mesh_io.write_obj(mesh, os.path.join(tmp, "b.obj"))}, a.reps)
        data = open(path, "rb").read()
        parse_only = median_ms(lambda: mesh_io.parse_obj(data), a.reps)[0]
        out[name] = {"vertices": len(mesh.vertices), "faces": len(mesh.faces), "bytes": size, "read_ms": r, "write_ms": w,
                     "parse_only_ms": round(parse_only, 3), "parse_MB_per_s": round(size / parse_only / 1e3, 1),
                     "written_bytes": os.path.getsize(os.path.join(tmp, "b.obj"))}
    return {"host": out}


def mode_sampler(a):
    import torch

    from etch_amd import ops
    out = {"note": "ms per call: [median, min, max], host clock, every call ends in a readback; points per scan below", "points": a.points, "reps": a.reps}
    scans = [synthetic_scan(k) for k in range(32)]
    keys = list(range(100, 132))
    for B in (1, 32):
        batch = scans[:B]
        fns = {"sample_surface": lambda: mesh_io.sample_surface(batch, a.points, keys[:B], center=True)}
        if not a.no_baseline:
            fns["sample_points_from_mesh"] = lambda: [sample_points_from_mesh(m, a.points, seed=15) for m in batch]
        fns["sample_surface"]()
        res = alternate(fns, a.reps)
        # the device part alone: the batch already packed and uploaded, events around bbox + the three sampler launches
        v, f, voff, foff = mesh_io.pack_meshes(batch)
        dv, df, dvo, dfo = (torch.from_numpy(x).cuda() for x in (v, f, voff, foff))
        dk = torch.from_numpy(np.array(keys[:B], np.uint64).view(np.int64)).cuda()
        t0 = time.perf_counter()
        mesh_io.pack_meshes(batch)
        pack_ms = (time.perf_counter() - t0) * 1e3

        def device_part():
            c = ops.bbox_center(dv, dvo)
            return ops.sample_surface(dv, df, dvo, dfo, dk, a.points, int(foff[-1]), int(np.diff(foff).max()), center=c)
        device_part()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            device_part()
        e.record()
        torch.cuda.synchronize()
        out[f"B{B}"] = {"faces_per_scan": len(batch[0].faces), "call_ms": res, "pack_on_host_ms": round(pack_ms, 3),
                        "upload_MB": round((v.nbytes + f.nbytes) / 1e6, 2), "device_part_ms_4_launches": round(s.elapsed_time(e) / 20, 4)}
    return {"sampler": out}


def mode_eval(a):
    import torch

    from etch_amd import constants as K
    from etch_amd import eval as E
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.body_model import SyntheticSMPL
    from etch_amd.utils.weights import load_seeded
    root = tempfile.mkdtemp()
    bm = SyntheticSMPL(7)
    ids = [f"s_{k:04d}" for k in range(a.scans)]
    for k, i in enumerate(ids):
        for d in ("scan", "smpl"):
            os.makedirs(os.path.join(root, d, i))
        synthetic_scan(k).export(os.path.join(root, "scan", i, f"{i}.obj"))
        Mesh(np.asarray(bm.v_template, np.float64), np.asarray(bm.faces, np.int64)).export(os.path.join(root, "smpl", i, f"mesh_smpl_{i}.obj"))
        np.savez(os.path.join(root, "smpl", i, f"info_{i}.npz"), gender=np.array(k % 2))
    os.makedirs(os.path.join(root, "ip"))
    for i in ids:
        np.savez(os.path.join(root, "ip", f"{i}.npz"), info_points=np.zeros((4, 3)), info_vectors=np.zeros((4, 3)))
    with open(os.path.join(root, "ids.pkl"), "wb") as fh:
        pickle.dump(ids, fh)
    args = types.SimpleNamespace(output_folder=os.path.join(root, "out"), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"),
                                 markerset=K.default_markerset(), scale_magnitude=10, body_model=bm)
    model = load_seeded(GT_network_equiv(option=args), 1).cuda().eval()
    sets = {g: E.EvalDataset(os.path.join(root, "scan"), os.path.join(root, "smpl"), os.path.join(root, "ip"), os.path.join(root, "ids.pkl"),
                             num_point=a.points, seed=1, ingest=g) for g in ("host", "device")}
    runs = {"host": ("host", 1), "device_prefetch0": ("device", 0), "device_prefetch1": ("device", 1)}
    for g in ("host", "device"):
        E.evaluate_dataset(args, model, _head(sets[g], a.batch), batch_size=a.batch, output_folder=os.path.join(root, "warm"))
    t = {k: [] for k in runs}
    for rep in range(a.reps):
        for name, (g, pf) in runs.items():
            t0 = time.perf_counter()
            E.evaluate_dataset(args, model, sets[g], batch_size=a.batch, output_folder=os.path.join(root, f"out_{name}"), prefetch=pf)
            torch.cuda.synchronize()
            t[name].append(a.scans / (time.perf_counter() - t0))
    return {"eval": {"note": "scans/s of evaluate_dataset per repeat, the three settings alternating; outputs written to a temporary folder",
                     "scans": a.scans, "faces_per_scan": 80000, "batch": a.batch, "points": a.points,
                     "scans_per_s": {k: [round(x, 2) for x in v] for k, v in t.items()}}}


def _head(ds, n):
    """The dataset cut to its first n ids (warm-up: code objects, allocator, the body model's device tables)."""
    import copy
    d = copy.copy(ds)
    d.id_list = ds.id_list[:n]
    return d


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["host", "sampler", "eval"])
    ap.add_argument("paths", nargs="*", help="host: the scan's and the body's OBJ file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_time.json"))
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-baseline", action="store_true", help="sampler: leave sample_points_from_mesh out (profiler runs)")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = {"host": 7, "sampler": 15, "eval": 2}[a.mode]
    if a.mode == "host" and len(a.paths) != 2:
        ap.error("host needs SCAN.obj BODY.obj")
    res = {"host": mode_host, "sampler": mode_sampler, "eval": mode_eval}[a.mode](a)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.update(res)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
