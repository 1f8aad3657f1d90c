"""MI355X counterpart of /root/reference/src/inference_demo.py: same CLI flags, same `load_model`,
`preprocess_scan`, `sample_points_from_mesh`, `predict_smpl`, same output files
(`<scan>_pred_smpl.obj`, `<scan>_output_smpl_info.npz` with body_pose, hand_pose, betas, global_orient, transl, joints).

Differences forced by the environment (no trimesh here): OBJ parsing and area-weighted surface sampling are
small numpy routines (the reference's sampling is unseeded, inference_demo.py:38; ours takes --seed), and the SMPL
body model comes from --body_model (a chumpy-free SMPL pickle) or --synthetic_body (seeded SMPL-shaped stand-in).
"""
import argparse
import json
import os

import numpy as np
import torch

from . import ops
from .models.fit_SMPL import Mesh, fit_smpl, stage2_from_stage1
from .models.models_pointcloud import GT_network_equiv


def load_model(args):
    """inference_demo.py:12-17."""
    model = GT_network_equiv(option=args).to(args.device)
    if args.model_path:
        model.load_state_dict(torch.load(args.model_path, map_location="cpu"))
    model.eval()
    return model


def load_obj(path):
    vs, fs = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                vs.append([float(t) for t in line.split()[1:4]])
            elif line.startswith("f "):
                idx = [int(t.split("/")[0]) - 1 for t in line.split()[1:]]
                for k in range(1, len(idx) - 1):
                    fs.append([idx[0], idx[k], idx[k + 1]])
    return Mesh(np.asarray(vs, np.float64), np.asarray(fs, np.int64))


def preprocess_scan(scan_path):
    """inference_demo.py:19-34: centre on the bounding-box mid-point."""
    scan_mesh = load_obj(scan_path)
    v = scan_mesh.vertices
    scan_center = (np.min(v, axis=0) + np.max(v, axis=0)) / 2.0
    centered = scan_mesh.copy()
    centered.vertices = v - scan_center
    return centered, scan_center


def sample_points_from_mesh(mesh, num_points=5000, seed=0):
    """inference_demo.py:36-39 (trimesh.sample.sample_surface): area-weighted faces + uniform barycentric coordinates."""
    rng = np.random.default_rng(seed)
    tri = mesh.vertices[mesh.faces]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    face = rng.choice(len(area), size=num_points, p=area / area.sum())
    r = rng.random((num_points, 2))
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    t = tri[face]
    return t[:, 0] + r[:, :1] * (t[:, 1] - t[:, 0]) + r[:, 1:] * (t[:, 2] - t[:, 0])


def predict_smpl_batch(args, model, points_tensor, gender="neutral", inner_out=None, **fit_kwargs):
    """inference_demo.py:41-66 for a batch (B,N,3) already on the device: stage 1 -> labels / inner points -> stage 2.
    inner_out: a dict that receives stage 1's inner points (B,N,3) under "inner" (the dense surface refinement fits the body to them)."""
    if getattr(args, "fit_pose_prior", None) is not None:       # --pose_prior (main): the marker fit under the mixture prior
        fit_kwargs.setdefault("pose_prior", args.fit_pose_prior)
    with torch.no_grad():
        if inner_out is None:
            # nobody asks for all inner points: the direction head runs at the markers' points only (fit_SMPL.markers_from_stage1; same bits)
            results, ctx = model.forward_for_fit(points_tensor)
            return stage2_from_stage1(args, model, points_tensor, results, ctx, gender, fit=fit_smpl, **fit_kwargs)
        results, _ = model(points_tensor, pred_items=["confidence", "direction", "magnitude"], direction_mode="standard_vector")
        labels = ops.argmax_rows(results["part_labels"])
        inner = ops.inner_points(points_tensor.contiguous(), results["direction"], results["magnitude"], float(args.scale_magnitude))
        inner_out["inner"] = inner
        return fit_smpl(args, inner, labels, results["confidences"], gender, **fit_kwargs)


def predict_smpl(args, model, points, gender="neutral"):
    """inference_demo.py:41-66."""
    points_tensor = torch.from_numpy(points).float().unsqueeze(0).to(args.device)
    meshes, _, _, info = predict_smpl_batch(args, model, points_tensor, gender)
    return meshes[0], info


def add_flags(parser):
    """Every flag of this command but --scan_path (etch_amd.track takes the same ones for a list of scans)."""
    parser.add_argument("--gender", type=str, default="neutral", choices=["neutral", "male", "female"])
    parser.add_argument("--model_path", type=str, default="", help="Path to trained model")
    parser.add_argument("--markerset_path", default="datafolder/useful_data_4d-dress/superset_smpl.json", type=str)
    parser.add_argument("--output_folder", type=str, default="output")
    parser.add_argument("--num_point", type=int, default=5000)
    parser.add_argument("--scale_magnitude", type=int, default=10)
    parser.add_argument("--EPN_input_radius", type=float, default=0.4)
    parser.add_argument("--EPN_layer_num", type=int, default=2, choices=[1, 2, 3, 4],
                        help="encoder depth (models_pointcloud.py:34-48: feature widths 32 / 64 / 128 / 256); the release uses 2")
    parser.add_argument("--body_model", type=str, default="", help="chumpy-free SMPL .pkl (else the reference's gender paths)")
    parser.add_argument("--synthetic_body", action="store_true", help="use the seeded SMPL-shaped stand-in body model")
    parser.add_argument("--seed", type=int, default=0, help="surface-sampling seed (the reference is unseeded)")
    parser.add_argument("--chamfer_refine", type=str, default="none", choices=["none", "both", "partial", "clutter"],
                        help="after the marker fit, refine the body against the centred scan's vertices (chamfer_refine.py:fit_cham): "
                             "both directions, scan -> body only (partial scans) or body -> scan only (cluttered scans)")
    parser.add_argument("--refine_iters", type=int, default=500, help="Adam iterations of --chamfer_refine")
    # absent unless given (the namespace of a run without the flag is what it always was): main() reads it with "host" as the default
    parser.add_argument("--ingest", type=str, default=argparse.SUPPRESS, choices=["host", "device"],
                        help="host (default): the Python OBJ reader / writer and the numpy sampler; device: the native reader and writer and "
                             "the GPU sampler keyed by --seed (etch_amd.mesh_io; same distribution, other points)")
    from .utils.prior import add_pose_prior_flags
    add_pose_prior_flags(parser)
    return parser


def add_surface_refine_flags(parser):
    """--surface_refine and its settings (this command and etch_amd.eval).  Absent unless given, like --ingest: surface_refine_settings reads them."""
    parser.add_argument("--surface_refine", action="store_true", default=argparse.SUPPRESS,
                        help="after the marker fit, fit the body SURFACE to all of stage 1's inner points (models/surface_refine.py:fit_surface; the "
                             "aggregated markers stay in the loss).  With --synthetic_body the stand-in body is SyntheticSurfaceSMPL, whose faces are a surface")
    parser.add_argument("--surface_iters", type=int, default=argparse.SUPPRESS, help="Adam iterations of --surface_refine (200)")
    parser.add_argument("--surface_trunc", type=float, default=argparse.SUPPRESS,
                        help="inner points farther than this from the body (metres) are left out of an iteration's dense term (0.05; negative: none are)")
    parser.add_argument("--surface_w", type=float, default=argparse.SUPPRESS, help="weight of the dense term of --surface_refine (1e2)")
    parser.add_argument("--surface_contain", action="store_true", default=argparse.SUPPRESS,
                        help="with --surface_refine: keep the body inside the scan's mesh (etch_amd/containment.py: vertices whose generalised winding "
                             "number says they are outside are pulled back to the scan's surface) and print how much of it lies outside before and after")
    parser.add_argument("--contain_w", type=float, default=argparse.SUPPRESS, help="weight of the containment term of --surface_contain (1e2)")
    parser.add_argument("--contain_every", type=int, default=argparse.SUPPRESS,
                        help="iterations between two recomputations of which vertices are outside and where they are pulled to (10)")


def surface_refine_settings(args, parser=None):
    """None without --surface_refine, else fit_surface's keyword arguments from --surface_iters / --surface_trunc / --surface_w.  Both
    refinements at once, or a setting without the flag, is an argument error."""
    given = [k for k in ("surface_iters", "surface_trunc", "surface_w") if hasattr(args, k)]
    err = parser.error if parser is not None else argparse.ArgumentParser().error
    if not getattr(args, "surface_refine", False):
        if given:
            err("--" + given[0] + " needs --surface_refine")
        return None
    if getattr(args, "chamfer_refine", "none") != "none":
        err("--surface_refine and --chamfer_refine are two refinements of the same fit: give one")
    if getattr(args, "surface_iters", 200) < 1:
        err("--surface_iters must be at least 1")
    return dict(iterations=getattr(args, "surface_iters", 200), trunc=getattr(args, "surface_trunc", 0.05), w_dense=getattr(args, "surface_w", 1e2))


def surface_contain_settings(args, parser=None):
    """None without --surface_contain, else fit_surface's containment keyword arguments from --contain_w / --contain_every.  The flag without
    --surface_refine, or a setting without the flag, is an argument error."""
    given = [k for k in ("contain_w", "contain_every") if hasattr(args, k)]
    err = parser.error if parser is not None else argparse.ArgumentParser().error
    if not getattr(args, "surface_contain", False):
        if given:
            err("--" + given[0] + " needs --surface_contain")
        return None
    if not getattr(args, "surface_refine", False):
        err("--surface_contain is a term of the surface refinement: it needs --surface_refine")
    if getattr(args, "contain_every", 10) < 1:
        err("--contain_every must be at least 1")
    if not getattr(args, "contain_w", 1e2) >= 0:
        err("--contain_w must not be negative")
    return dict(w_contain=getattr(args, "contain_w", 1e2), contain_every=getattr(args, "contain_every", 10))


def format_containment(m):
    return f"outside_share {m['outside_share']:.4f} protrusion_rms_mm {m['protrusion_rms_mm']:.3f} protrusion_max_mm {m['protrusion_max_mm']:.3f}"


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--scan_path", type=str, required=True, help="Path to input scan OBJ file")
    add_surface_refine_flags(parser)      # this command and etch_amd.eval only: track, depth and animate share add_flags, not the refinement
    return add_flags(parser)


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    surface_refine_settings(args, parser)
    surface_contain_settings(args, parser)
    return args


def fit_and_refine(args, model, points, centered_mesh, report=None):
    """The marker fit of points (N,3), then with --chamfer_refine fit_cham against the centred scan's vertices (the script's `vertices_scan`).
    -> the fit's meshes, the body model, the refined vertices (None without --chamfer_refine) and the parameters as fit_cham's dict (without
    --chamfer_refine its `init`, the marker fit's).  With --surface_refine the refinement is fit_surface on stage 1's inner points instead.
    With --surface_contain, centered_mesh may be a cloud.OrientedCloud in the frame of the points (etch_amd.cloud); report: a dict that then
    receives contain_before and contain_after, the metrics that are printed."""
    from .models.chamfer_refine import fit_cham, init_from_fit
    from .models.fit_SMPL import _resolve_body_model

    points_tensor = torch.from_numpy(points).float().unsqueeze(0).to(args.device)
    surface = surface_refine_settings(args)
    if surface is not None:
        inner = {}
        meshes, _, _, _, dev = predict_smpl_batch(args, model, points_tensor, args.gender, return_trace=True, inner_out=inner)
    else:
        meshes, _, _, _, dev = predict_smpl_batch(args, model, points_tensor, args.gender, return_trace=True)
    bm = _resolve_body_model(args, args.gender)
    verts, prm = None, init_from_fit(dev)
    if surface is not None:
        from .models.surface_refine import fit_surface
        contain = surface_contain_settings(args)
        if contain is not None:
            # the centred mesh the command ingested (either --ingest mode) is the frame of the points and so of the fit
            from .containment import _is_cloud, containment_metrics, pack_scans
            scans = centered_mesh if _is_cloud(centered_mesh) else pack_scans([centered_mesh], args.device)
            before = containment_metrics(scans, np.asarray(meshes[0].vertices, np.float32)[None])[0]
            surface = dict(surface, scan=scans, **contain)
        verts, prm = fit_surface(bm, inner["inner"], prm, markers=dev["markers"], valid=dev["valid"], marker_vids=list(args.markerset.values()), **surface)
        if contain is not None:
            after = containment_metrics(scans, verts)[0]
            print("containment before the refinement: " + format_containment(before))
            print("containment after the refinement:  " + format_containment(after))
            if report is not None:
                report.update(contain_before=before, contain_after=after)
    elif args.chamfer_refine != "none":
        scan = torch.from_numpy(np.asarray(centered_mesh.vertices, np.float32)).unsqueeze(0).to(args.device)
        verts, prm = fit_cham(bm, scan, prm, prior=None, bidir=args.chamfer_refine, iterations=args.refine_iters)
    return meshes, bm, verts, prm


def _refine_and_save(args, model, points, centered_mesh, original_center, scan_name, export=Mesh.export, report=None):
    """--chamfer_refine / --surface_refine: the OBJ is the refined mesh moved back by the scan centre; the .npz holds the refined parameters, `scale`, and the
    joints in the centred scan's frame ((joints + trans) * scale, the frame the LM joints of an unrefined run are written in)."""
    meshes, _, verts, prm = fit_and_refine(args, model, points, centered_mesh, report=report)
    final = Mesh(verts[0] + original_center, meshes[0].faces)
    export(final, os.path.join(args.output_folder, f"{scan_name}_pred_smpl.obj"))
    pose = prm["pose"][0].cpu().numpy()
    body = pose[3:].reshape(-1, 3)
    scale = prm["scale"][0].cpu().numpy()
    trans = prm["trans"][0].cpu().numpy()
    joints = (prm["joints"][0].cpu().numpy() + trans) * scale
    np.savez(os.path.join(args.output_folder, f"{scan_name}_output_smpl_info.npz"), body_pose=body[:21], hand_pose=body[21:23],
             betas=prm["beta"][0].cpu().numpy(), global_orient=pose[:3], transl=trans, scale=scale, joints=joints)


def resolve_body_model(args):
    """--synthetic_body / --body_model -> args.body_model (a BodyModel, or None = the reference's gender paths)."""
    if args.synthetic_body:
        from .utils.body_model import SyntheticSMPL, SyntheticSurfaceSMPL
        # SyntheticSMPL's faces are a strip for OBJ export, no surface: the surface refinement gets the stand-in that has one
        args.body_model = SyntheticSurfaceSMPL(7) if getattr(args, "surface_refine", False) else SyntheticSMPL(7)
    elif args.body_model:
        from .utils.body_model import load_smpl_pkl, load_smplx
        # an SMPL-X model file (SMPLX_*.npz / .pkl) selects the 55-joint, 20-coefficient fit; anything else is read as an SMPL pickle
        args.body_model = load_smplx(args.body_model) if "smplx" in os.path.basename(args.body_model).lower() else load_smpl_pkl(args.body_model)
    else:
        args.body_model = None


def _ingest_device(args):
    """--ingest device: preprocess_scan and sample_points_from_mesh on the native path -> (points (1,N,3) float32 on the device, the centred
    mesh, the centre)."""
    from . import mesh_io
    scan_mesh = mesh_io.read_obj(args.scan_path)
    points, _, center = mesh_io.sample_surface([scan_mesh], args.num_point, [args.seed], center=True, device=args.device)
    center = center[0].cpu().numpy()
    return points, Mesh(scan_mesh.vertices - center, scan_mesh.faces), center


def prepare_common(args):
    """The part of prepare() that does not touch the scan: the device, the markerset, the body model, the pose prior and the output folder
    into args -> the network."""
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
    resolve_body_model(args)
    from .utils.prior import pose_prior_from_args
    args.fit_pose_prior = pose_prior_from_args(args, args.device)
    os.makedirs(args.output_folder, exist_ok=True)
    return load_model(args)


def prepare(args):
    """What a single-scan command does between parsing its flags and the fit: prepare_common; the scan read, centred and sampled (--ingest).
    -> model, the OBJ writer, points (N,3) float32 numpy, the centred mesh, the centre, the scan's name."""
    model = prepare_common(args)
    export = Mesh.export
    if getattr(args, "ingest", "host") == "device":
        from .mesh_io import write_obj as export
        points_tensor, centered_mesh, original_center = _ingest_device(args)
        points = points_tensor[0].cpu().numpy()
    else:
        centered_mesh, original_center = preprocess_scan(args.scan_path)
        points = sample_points_from_mesh(centered_mesh, args.num_point, args.seed)
    scan_name = os.path.splitext(os.path.basename(args.scan_path))[0]
    return model, export, points, centered_mesh, original_center, scan_name


def main(argv=None):
    args = parse_args(argv)
    model, export, points, centered_mesh, original_center, scan_name = prepare(args)
    if args.chamfer_refine != "none" or getattr(args, "surface_refine", False):
        _refine_and_save(args, model, points, centered_mesh, original_center, scan_name, export)
        print(f"Predicted SMPL mesh and smpl info saved under {args.output_folder}")
        return
    pred_smpl_mesh, smpl_info = predict_smpl(args, model, points, args.gender)
    final = pred_smpl_mesh.copy()
    final.vertices = pred_smpl_mesh.vertices + original_center
    export(final, os.path.join(args.output_folder, f"{scan_name}_pred_smpl.obj"))
    np.savez(os.path.join(args.output_folder, f"{scan_name}_output_smpl_info.npz"), body_pose=smpl_info[0][0, :21, :],
             hand_pose=smpl_info[0][0, 21:23, :], betas=smpl_info[1][0], global_orient=smpl_info[2][0], transl=smpl_info[3][0],
             joints=smpl_info[4][0])
    print(f"Predicted SMPL mesh and smpl info saved under {args.output_folder}")


if __name__ == "__main__":
    main()
