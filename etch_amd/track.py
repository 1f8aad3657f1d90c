"""python -m etch_amd.track: inference_demo.py for a SEQUENCE of scans of one subject.

    python -m etch_amd.track --scan_paths f000.obj f001.obj ... [--scan_list FILE] [the flags of inference_demo.py]
                             [--batch_size 8] [--temporal_w_pose W --temporal_w_orient W --temporal_w_transl W] [--shape_w W]
                             [--sweeps 2] [--refit_steps 10]

Every scan is ingested as inference_demo.py ingests it (--ingest host / device), stage 1 and get_markers run in batches of --batch_size, and
etch_amd.sequence.fit_sequence tracks all frames at once: shared shape, temporal smoothness, frames without usable markers filled from their
neighbours.  Per frame the files of inference_demo.py are written -- <name>_pred_smpl.obj in the world frame, <name>_output_smpl_info.npz with
inference_demo.py's keys and conventions (transl and joints relative to the scan's bounding-box centre) -- and once sequence_info.npz:
names, offsets (the centres: world = centred + offset), beta_mean, status (marker_status per frame: non-zero frames were filled), and the mean
frame-to-frame joint displacement in the world frame before and after tracking.  --sweeps 0 writes each frame exactly as inference_demo.py
would (the fit of a frame does not depend on its batch; with more than 8 frames the fit runs one workgroup per scan instead of a split one,
which may move the last bits)."""
import argparse
import json
import os

import numpy as np
import torch

from . import inference_demo as D
from . import mesh_io, ops, sequence
from .models.fit_SMPL import Mesh, get_markers


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--scan_paths", type=str, nargs="+", default=[], help="the sequence's OBJ files, in temporal order")
    parser.add_argument("--scan_list", type=str, default="", help="text file with one OBJ path per line (instead of, or after, --scan_paths)")
    D.add_flags(parser)
    parser.add_argument("--batch_size", type=int, default=8, help="scans per stage-1 batch")
    parser.add_argument("--temporal_w_pose", type=float, default=sequence.DEFAULT_TEMPORAL_W[0])
    parser.add_argument("--temporal_w_orient", type=float, default=sequence.DEFAULT_TEMPORAL_W[1])
    parser.add_argument("--temporal_w_transl", type=float, default=sequence.DEFAULT_TEMPORAL_W[2])
    parser.add_argument("--shape_w", type=float, default=sequence.DEFAULT_SHAPE_W)
    parser.add_argument("--sweeps", type=int, default=sequence.DEFAULT_SWEEPS, help="red-black refit sweeps; 0: independent fits only")
    parser.add_argument("--refit_steps", type=int, default=sequence.DEFAULT_REFIT_STEPS, help="LM iterations of every refit")
    args = parser.parse_args(argv)
    paths = list(args.scan_paths)
    if args.scan_list:
        with open(args.scan_list) as f:
            paths += [ln.strip() for ln in f if ln.strip()]
    if not paths:
        parser.error("no scan: give --scan_paths or --scan_list")
    if args.batch_size < 1:
        parser.error("--batch_size must be >= 1")
    if args.chamfer_refine != "none":
        parser.error("--chamfer_refine works on single scans (inference_demo.py); the tracker has no chamfer stage")
    names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    if len(set(names)) != len(names):
        parser.error("two scans share a file name: their outputs would overwrite each other")
    args.scan_paths, args.scan_names = paths, names
    return args


def _ingest(args):
    """-> points (T,N,3) float32 on the device, centres (T,3) float64 numpy: per scan what inference_demo.main feeds its network."""
    meshes = mesh_io.read_objs(args.scan_paths)                       # the arrays load_obj returns, bit for bit
    if getattr(args, "ingest", "host") == "device":
        points, _, centers = mesh_io.sample_surface(meshes, args.num_point, [args.seed], center=True, device=args.device)
        return points, centers.cpu().numpy()
    pts, centers = [], []
    for m in meshes:
        c = (np.min(m.vertices, axis=0) + np.max(m.vertices, axis=0)) / 2.0                # preprocess_scan
        pts.append(D.sample_points_from_mesh(Mesh(m.vertices - c, m.faces), args.num_point, args.seed))
        centers.append(c)
    return torch.from_numpy(np.stack(pts)).float().to(args.device), np.stack(centers)


def stage1_markers(args, model, points):
    """Stage 1 and get_markers in batches of args.batch_size -> markers (T,M,3), valid (T,M) bool."""
    mk, vd = [], []
    with torch.no_grad():
        for i in range(0, points.shape[0], args.batch_size):
            p = points[i:i + args.batch_size].contiguous()
            res, _ = model(p, pred_items=["confidence", "direction", "magnitude"], direction_mode="standard_vector")
            labels = ops.argmax_rows(res["part_labels"])
            inner = ops.inner_points(p, res["direction"], res["magnitude"], float(args.scale_magnitude))
            m, v = get_markers(args, inner, labels, res["confidences"])
            mk.append(m), vd.append(v)
    return torch.cat(mk).contiguous(), torch.cat(vd).contiguous()


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("etch_amd needs an AMD GPU (gfx950); there is no CPU path")
    args.cuda = True
    args.device = torch.device("cuda")
    if os.path.exists(args.markerset_path):
        with open(args.markerset_path) as f:
            args.markerset = json.load(f)
    else:
        from . import constants
        args.markerset = constants.default_markerset()
    D.resolve_body_model(args)
    from .utils.prior import pose_prior_from_args
    pose_prior = pose_prior_from_args(args, args.device)
    os.makedirs(args.output_folder, exist_ok=True)
    model = D.load_model(args)
    export = mesh_io.write_obj if getattr(args, "ingest", "host") == "device" else Mesh.export
    points, centers = _ingest(args)
    markers, valid = stage1_markers(args, model, points)
    offsets = torch.from_numpy(centers).float().to(args.device)
    fit = sequence.fit_sequence(args, markers, valid, args.gender, offsets=offsets,
                                temporal_w=(args.temporal_w_pose, args.temporal_w_orient, args.temporal_w_transl), shape_w=args.shape_w,
                                sweeps=args.sweeps, refit_steps=args.refit_steps, pose_prior=pose_prior)
    nj, nb = fit["nj"], fit["nb"]
    npose = 3 * (nj - 1)
    x, verts, joints = fit["x"].cpu().numpy(), fit["verts"].cpu().numpy(), fit["joints"].cpu().numpy()
    for t, name in enumerate(args.scan_names):
        export(Mesh(verts[t] + centers[t], fit["faces"]), os.path.join(args.output_folder, f"{name}_pred_smpl.obj"))
        pose = x[t, :npose].reshape(-1, 3)
        np.savez(os.path.join(args.output_folder, f"{name}_output_smpl_info.npz"), body_pose=pose[:21], hand_pose=pose[21:23],
                 betas=x[t, npose:npose + nb].copy(), global_orient=x[t, npose + nb:npose + nb + 3].copy(),
                 transl=x[t, npose + nb + 3:npose + nb + 6].copy(), joints=joints[t])
    if args.sweeps > 0:
        from .models.fit_SMPL import _device_body, _resolve_body_model
        db = _device_body(_resolve_body_model(args, args.gender), list(args.markerset.values()), args.device)
        _, joints_before = ops.smpl_lbs(db.lbs_consts, fit["x_independent"].contiguous(), db.V, db.n_extra, nj=nj, nb=nb)
    else:
        joints_before = fit["joints"]
    np.savez(os.path.join(args.output_folder, "sequence_info.npz"), names=np.array(args.scan_names), offsets=centers,
             beta_mean=fit["beta_mean"].cpu().numpy(), status=fit["status"].cpu().numpy(),
             joint_displacement_before=sequence.joint_displacement(joints_before, offsets),
             joint_displacement_after=sequence.joint_displacement(fit["joints"], offsets))
    print(f"Tracked {len(args.scan_names)} frames; SMPL meshes and smpl info saved under {args.output_folder}")
    return fit


if __name__ == "__main__":
    main()
