"""Drop-in for the reference's training dataset, data_utils.GT_dataloader.GTDataset (src/data_utils/GT_dataloader.py:61-160): the same `args`
fields (seed, scan_dir, smpl_dir, infopoints_dir, activated_ids_path, num_point, markerset), the same id filtering and the same item keys,
dtypes and shapes, with every target built on the GPU: the tightness vectors by etch_amd.infopoints.tightness_vectors, the labels and
confidences by etch_amd.geodesic (csrc/geodesic.hip) in place of potpourri3d.

Items run on the GPU in the calling process.  The reference's DataLoader(num_workers=16) does not apply: use num_workers=0, or the "spawn"
start method (a forked worker cannot use the parent's HIP context).  A body never changes for an id, so its marker field (min distance and
label per subdivided vertex) is computed once and cached; `precompute(batch_size)` solves many bodies per call.

The scan points come from our seeded area-weighted sampler with seed + 15: trimesh.sample.sample_surface's distribution, not its points
(as etch_amd.eval.EvalDataset documents).  With `view` (an etch_amd.depth.ViewSpec) an item's points are, with the spec's probability,
what one depth camera sees of the scan; the targets come from the same code, which takes any points on the scan surface.
"""
import os
import pickle

import numpy as np
import torch

from . import geodesic as G
from .infopoints import tightness_vectors


class GTDataset:
    gender_dict = {0: "female", 1: "male"}                  # GT_dataloader.py:75

    def __init__(self, args, device=None, laplacian="intrinsic_delaunay", verbose=True, reader="python", view=None):
        if reader not in ("python", "native"):
            raise ValueError(f"reader must be 'python' or 'native', got {reader!r}")
        self.view = view                                      # an etch_amd.depth.ViewSpec: items seen by one random depth camera
        self.epoch = 0
        self.reader = reader                                  # "native": etch_amd.mesh_io.read_obj for an item's two meshes, the same arrays
        self.seed = args.seed
        self.scan_dir = args.scan_dir
        self.smpl_dir = args.smpl_dir
        self.infopoints_dir = args.infopoints_dir
        with open(args.activated_ids_path, "rb") as f:
            self.activated_ids = pickle.load(f)
        self.id_list = sorted(i for i in os.listdir(self.scan_dir)
                              if os.path.isdir(os.path.join(self.scan_dir, i)) and os.path.isdir(os.path.join(self.smpl_dir, i))
                              and os.path.isfile(os.path.join(self.infopoints_dir, f"{i}.npz")) and i in self.activated_ids)
        self.num_point = args.num_point
        self.markerset = args.markerset
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.laplacian = laplacian
        self._fields = {}
        if verbose:
            print(f"Num of data: {len(self.id_list)}")

    def __len__(self):
        return len(self.id_list)

    def set_epoch(self, epoch):
        """The epoch whose views the items show (with `view`): an item's camera is a function of (seed, epoch, index) alone."""
        self.epoch = int(epoch)

    def view_camera(self, index, scan=None):
        """The camera of item `index` in the current epoch, or None where the item keeps its full scan (always None without `view`)."""
        if self.view is None:
            return None
        from .depth import bbox_mid
        if scan is None:
            from .inference_demo import load_obj
            scan = load_obj(self._paths(self.id_list[index])[1])
        return self.view.camera(self.seed, self.epoch, index, bbox_mid(scan.vertices))

    def _view_points(self, index, scan, camera):
        """num_point points of what `camera` sees of the scan, float64 in the scan's own frame (no centring, like the full samples)."""
        from .depth import partial_view_points
        key = self.view.draw(self.seed, self.epoch, index)[3]
        return partial_view_points([scan], [camera], self.num_point, [key], center=False, device=self.device).points64[0].cpu().numpy()

    def _paths(self, i):
        return (os.path.join(self.infopoints_dir, f"{i}.npz"), os.path.join(self.scan_dir, i, f"{i}.obj"),
                os.path.join(self.smpl_dir, i, f"mesh_smpl_{i}.obj"), os.path.join(self.smpl_dir, i, f"info_{i}.npz"))

    def _body(self, i):
        from .inference_demo import load_obj
        return load_obj(self._paths(i)[2])

    def precompute(self, batch_size=8, ids=None):
        """Solve the marker fields of every id not cached yet (or of `ids`), batch_size bodies per GPU call (bodies of one face array)."""
        todo = [i for i in (self.id_list if ids is None else ids) if i not in self._fields]
        groups = {}
        for i in todo:
            body = self._body(i)
            groups.setdefault(np.asarray(body.faces, np.int64).tobytes(), []).append((i, body))
        for items in groups.values():
            for s in range(0, len(items), batch_size):
                chunk = items[s:s + batch_size]
                verts = np.stack([np.asarray(b.vertices, np.float64) for _, b in chunk])
                r = G.marker_fields(verts, chunk[0][1].faces, self.markerset, laplacian=self.laplacian, device=self.device)
                for k, (i, _) in enumerate(chunk):
                    self._fields[i] = (r["min_dist"][k].clone(), r["label"][k].clone(), r["vertices"][k].clone())

    def field(self, i):
        """(min_dist (V'), label (V') int64, subdivided vertices (V',3)) of id i on the device."""
        if i not in self._fields:
            self.precompute(1, [i])
        return self._fields[i]

    def __getitem__(self, index):
        from .inference_demo import load_obj, sample_points_from_mesh
        if self.reader == "native":
            from .mesh_io import read_obj as load_obj
        i = self.id_list[index]
        ip_path, scan_path, smpl_path, info_path = self._paths(i)
        assert os.path.isfile(ip_path) and os.path.isfile(scan_path) and os.path.isfile(smpl_path) and os.path.isfile(info_path)
        ipd = np.load(ip_path)
        scan = load_obj(scan_path)
        body = load_obj(smpl_path)
        camera = self.view_camera(index, scan)
        if camera is not None:
            sample_points = self._view_points(index, scan, camera)
        else:
            sample_points = sample_points_from_mesh(scan, self.num_point, seed=self.seed + 15)
        vectors, _ = tightness_vectors(sample_points, ipd["info_points"], ipd["info_vectors"], body, device=self.device)
        dmin, lab, sv = self.field(i)
        confidences, labels = G.geodesic_targets(sample_points, vectors, dmin, lab, sv, device=self.device)
        info = np.load(info_path)
        return {"id": i,
                "hitpts": torch.from_numpy(np.asarray(sample_points)).type(torch.float32),
                "vectors": torch.from_numpy(vectors).type(torch.float32),
                "confidences": torch.from_numpy(confidences).type(torch.float32),
                "labels": torch.from_numpy(labels).type(torch.long),
                "gender": self.gender_dict[int(np.asarray(info["gender"]).item())]}
