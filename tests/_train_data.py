"""The two-id, num_point = 512 training dataset on disk that test_gpu_train_program.py builds for itself (the geodesic fixture's body, two offset
scans), as a helper for other test files: `build(root)` writes it under `root` and returns the flags that point python -m etch_amd.train at it."""
import json
import os
import pickle
import types

import numpy as np
import torch

import _geodesic_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")
NUM_POINT = 512
WEIGHTS = ["--direction_w", "2.5", "--magnitude_w", "30", "--part_label_w", "1", "--confidence_w", "50"]


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.writelines(f"v {x:.8f} {y:.8f} {z:.8f}\n" for x, y, z in v)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)


def build(root, device="cuda"):
    """-> namespace(root, flags): flags hold everything but --epochs / --output_root (batch_size 2, seed 3, no plots)."""
    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.inference_demo import Mesh, load_obj
    from etch_amd.infopoints import generate_infopoints, save_data

    root = str(root)
    z = O.load_fixture(GOLDEN)
    verts, faces = z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)
    ids = ["a_0001", "b_0002"]
    body = Mesh(verts, faces)
    n = ops.vertex_normals(torch.as_tensor(verts, device=device), torch.as_tensor(faces, device=device).to(torch.int32)).cpu().numpy()
    os.makedirs(os.path.join(root, "ip"))
    for k, i in enumerate(ids):
        off = np.random.default_rng(k).uniform(0.01, 0.03, (len(verts), 1))
        for d in ("scan", "smpl"):
            os.makedirs(os.path.join(root, d, i))
        _write_obj(os.path.join(root, "scan", i, f"{i}.obj"), verts + off * n, faces)
        _write_obj(os.path.join(root, "smpl", i, f"mesh_smpl_{i}.obj"), verts, faces)
        np.savez(os.path.join(root, "smpl", i, f"info_{i}.npz"), gender=np.array(k))
        ip, iv, _ = generate_infopoints(load_obj(os.path.join(root, "scan", i, f"{i}.obj")), body, num_samples=3000, seed=k, device=device)
        save_data(ip, iv, os.path.join(root, "ip", f"{i}.npz"))
    with open(os.path.join(root, "ids.pkl"), "wb") as fh:
        pickle.dump(ids, fh)
    with open(os.path.join(root, "markers.json"), "w") as fh:
        json.dump(K.default_markerset(), fh)
    flags = ["--activated_ids_path", os.path.join(root, "ids.pkl"), "--markerset_path", os.path.join(root, "markers.json"),
             "--infopoints_dir", os.path.join(root, "ip"), "--scan_dir", os.path.join(root, "scan"), "--smpl_dir", os.path.join(root, "smpl"),
             "--num_point", str(NUM_POINT), "--batch_size", "2", "--seed", "3", "--vis_loss", "false"] + WEIGHTS
    return types.SimpleNamespace(root=root, flags=flags)


def folder(output_root):
    """The experiment folder the program makes under --output_root for this dataset."""
    return os.path.join(str(output_root), f"EPN_layer_2_radius_0.4_num_point_{NUM_POINT}")
