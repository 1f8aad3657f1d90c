"""Batch evaluation harness around the hot path -- MI355X counterpart of the inference part of
/root/reference/src/eval.py:
  * per-gender batching of fit_smpl (eval.py:186-209): one call when the batch has a single gender, otherwise per gender
    group (the reference falls back to per-sample calls; grouping by gender gives the same per-sample results because
    every LM problem is independent, and keeps the batches large),
  * V2V = mean_v || v_gt - v_pred ||_2 over the 6 890 vertices (eval.py:235-237),
  * MPJPE over the first 22 joints (scripts/experiment_scripts/compute_mpjpe_error.py:23-24),
  * the per-sample output_smpl_info npz (eval.py:240-247) and v2v_score.txt lines (eval.py:254-256).
  * `EvalDataset` reads the reference's on-disk layout (README.md:74-90; src/data_utils/GT_dataloader_mixed.py:110-161,259-274):
    scans `<scan_dir>/<id>/<id>.obj`, body models `<smpl_dir>/<id>/{info_<id>.npz, mesh_smpl_<id>.obj}`, per-id `<infopoints_dir>/<id>.npz`
    and the pickled list of activated ids -- the inference-side fields only (points sampled on the scan, gender, ground-truth SMPL
    vertices / joints).  The training targets of that loader (vectors, geodesic confidences, labels) are built by
    etch_amd.datasets.GTDataset (DESIGN sections 9 and 10); eval.py's visualisation exports are out of scope.
  * `evaluate_dataset` is eval.py's loop (:76-265): batches, per-sample outputs, v2v_score.txt with its summary block.
  * `python -m etch_amd.eval` is eval.py's command line (:270-315) on top of it.  With ingest="device" (the command's default)
    the meshes are read by the native OBJ reader on worker threads, one batch ahead of the GPU, sampled on the device per batch and written by
    the native writer."""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from .models.fit_SMPL import Mesh, fit_smpl


class EvalDataset:
    """Inference-side view of the reference's GTDataset (GT_dataloader_mixed.py:110-161).  Items:
    {id, hitpts (num_point,3) float32, gender "female" | "male", gt_vertices (V,3), gt_joints (J,3) or None}.
    ingest="device": the meshes come from the native reader and an item carries `scan` (the parsed Mesh) in place of `hitpts`; the points are
    sampled on the device per batch (evaluate_dataset), every scan under the key seed + 15."""

    gender_dict = {0: "female", 1: "male"}                # GT_dataloader_mixed.py:133

    def __init__(self, scan_dir, smpl_dir, infopoints_dir, activated_ids_path=None, num_point=5000, seed=0, ingest="host"):
        import pickle
        if ingest not in ("host", "device"):
            raise ValueError(f"ingest must be 'host' or 'device', got {ingest!r}")
        self.ingest = ingest
        self.scan_dir, self.smpl_dir, self.infopoints_dir = scan_dir, smpl_dir, infopoints_dir
        activated = None
        if activated_ids_path:
            with open(activated_ids_path, "rb") as f:
                activated = set(pickle.load(f))
        self.id_list = sorted(i for i in os.listdir(scan_dir)
                              if os.path.isdir(os.path.join(scan_dir, i)) and os.path.isdir(os.path.join(smpl_dir, i))
                              and os.path.isfile(os.path.join(infopoints_dir, f"{i}.npz")) and (activated is None or i in activated))
        self.num_point, self.seed = num_point, seed

    def __len__(self):
        return len(self.id_list)

    def __getitem__(self, index):
        from .inference_demo import load_obj, sample_points_from_mesh
        if self.ingest == "device":
            from .mesh_io import read_obj as load_obj
        i = self.id_list[index]
        scan = load_obj(os.path.join(self.scan_dir, i, f"{i}.obj"))
        smpl = load_obj(os.path.join(self.smpl_dir, i, f"mesh_smpl_{i}.obj"))
        info = np.load(os.path.join(self.smpl_dir, i, f"info_{i}.npz"))
        item = {"id": i, "gender": self.gender_dict[int(np.asarray(info["gender"]).item())], "gt_vertices": np.asarray(smpl.vertices, np.float32),
                "gt_joints": np.asarray(info["joints"], np.float32) if "joints" in info.files else None}
        if self.ingest == "device":
            item["scan"] = scan                                # sampled on the device with its batch (evaluate_dataset)
        else:
            # the reference samples with trimesh.sample.sample_surface(scan, num_point, seed = self.seed + 15) (:201-203); same
            # distribution (area-weighted faces, uniform barycentric coordinates) from our seeded sampler
            item["hitpts"] = sample_points_from_mesh(scan, self.num_point, seed=self.seed + 15).astype(np.float32)
        return item


def _device_batches(dataset, batch_size, prefetch):
    """Batches of an ingest="device" dataset: the items of a batch are read on worker threads, and with prefetch >= 1 the reads of the next
    `prefetch` batches are already running while the caller works on the current one."""
    starts = list(range(0, len(dataset), batch_size))
    depth = max(int(prefetch), 0)
    with ThreadPoolExecutor(max_workers=min(16, batch_size)) as pool:
        submit = lambda s: [pool.submit(dataset.__getitem__, k) for k in range(s, min(s + batch_size, len(dataset)))]
        queue = [submit(s) for s in starts[:depth]]
        for n, s in enumerate(starts):
            if depth == 0:
                queue.append(submit(s))
            elif n + depth < len(starts):
                queue.append(submit(starts[n + depth]))
            yield [f.result() for f in queue.pop(0)]


def view_cameras(view, scans):
    """--view_azimuth: one camera per scan, orbiting the scan's own bounding-box centre.  view = {azimuth, elevation (degrees), distance, fov,
    size (H, W)}."""
    import math

    from .depth import Camera, bbox_mid
    return [Camera.orbit(bbox_mid(s.vertices), view["distance"], math.radians(view["azimuth"]), math.radians(view["elevation"]), view["fov"],
                         int(view["size"][0]), int(view["size"][1])) for s in scans]


def _evaluate_dataset_device(args, model, dataset, batch_size, output_folder, prefetch, view=None):
    from .mesh_io import sample_surface, write_obj
    recs = []
    for items in _device_batches(dataset, batch_size, prefetch):
        scans = [it["scan"] for it in items]
        # every id under one key, as the reference gives each the sampler seed self.seed + 15 (GT_dataloader_mixed.py:201-203)
        if view is not None:
            # the points one virtual camera sees of each scan, in the scan's own frame like the full samples: the scores stay comparable
            from .depth import partial_view_points
            hitpts = partial_view_points(scans, view_cameras(view, scans), dataset.num_point, [dataset.seed + 15], center=False, device=args.device).points
        else:
            hitpts, _, _ = sample_surface(scans, dataset.num_point, [dataset.seed + 15], center=False, device=args.device)
        gtj = [it["gt_joints"] for it in items]
        recs += evaluate_batch(args, model, hitpts, [it["gender"] for it in items], ids=[it["id"] for it in items],
                               gt_vertices=[it["gt_vertices"] for it in items], gt_joints=None if any(j is None for j in gtj) else gtj,
                               output_folder=output_folder, export=write_obj, scans=scans)
    return recs


def evaluate_dataset(args, model, dataset, batch_size=8, output_folder=None, ingest=None, prefetch=1, view=None):
    """eval.py:76-265: the whole dataset in batches through `evaluate_batch`; v2v_score.txt ends with the reference's summary block.
    Returns (records, average v2v).  ingest (default: the dataset's): "host" = items sampled by the dataset one at a time in this thread;
    "device" = native reader on worker threads `prefetch` batches ahead (0: none), device sampler per batch, native writer.  view (ingest
    "device" only): every scan is scored from the points one virtual camera sees of it (view_cameras), against the full ground-truth body."""
    ingest = ingest or getattr(dataset, "ingest", "host")
    if view is not None and ingest != "device":
        raise ValueError("a virtual view (--view_azimuth) is rendered on the device: it needs ingest='device'")
    if ingest != getattr(dataset, "ingest", "host"):
        raise ValueError(f"ingest={ingest!r} needs a dataset built with the same ingest (it has {getattr(dataset, 'ingest', 'host')!r})")
    output_folder = output_folder or args.output_folder
    os.makedirs(output_folder, exist_ok=True)
    score = os.path.join(output_folder, "v2v_score.txt")
    if os.path.exists(score):
        os.remove(score)                                   # eval.py:82-84
    from .inference_demo import surface_contain_settings
    if surface_contain_settings(args) is not None:
        if ingest != "device":
            raise ValueError("--surface_contain needs the scans' meshes: host-ingest items carry none, use ingest='device'")
        if view is not None:
            raise ValueError("a single view is half a shell and has no inside: --surface_contain cannot be combined with a virtual view")
        if os.path.exists(os.path.join(output_folder, "containment.txt")):
            os.remove(os.path.join(output_folder, "containment.txt"))
    if ingest == "device":
        recs = _evaluate_dataset_device(args, model, dataset, batch_size, output_folder, prefetch, view)
    else:
        recs = []
        for s in range(0, len(dataset), batch_size):
            items = [dataset[k] for k in range(s, min(s + batch_size, len(dataset)))]
            hitpts = torch.from_numpy(np.stack([it["hitpts"] for it in items])).to(args.device)
            gtj = [it["gt_joints"] for it in items]
            recs += evaluate_batch(args, model, hitpts, [it["gender"] for it in items], ids=[it["id"] for it in items],
                                   gt_vertices=[it["gt_vertices"] for it in items], gt_joints=None if any(j is None for j in gtj) else gtj,
                                   output_folder=output_folder)
    total = float(sum(r["v2v"] for r in recs))
    n = len(recs)
    with open(score, "a") as f:                            # eval.py:258-265
        f.write("==========\n")
        f.write(f"average v2v: {total / max(n, 1)}\n")
        f.write(f"total v2v: {total}\n")
        f.write(f"sample num: {n}\n")
    return recs, total / max(n, 1)


def v2v(gt_vertices, pred_vertices):
    """eval.py:237."""
    return float(np.mean(np.linalg.norm(np.asarray(gt_vertices) - np.asarray(pred_vertices), axis=1)))


def mpjpe(gt_joints, pred_joints, joints_num_considered=22):
    """compute_mpjpe_error.py:23-24."""
    return float(np.linalg.norm(np.asarray(pred_joints)[:joints_num_considered] - np.asarray(gt_joints)[:joints_num_considered], axis=-1).mean())


def fit_smpl_by_gender(args, pred_inner_points, pred_part_labels, pred_confidences, gender_list, **fit_kwargs):
    """eval.py:186-209 with the same return layout as fit_smpl for the whole batch."""
    B = pred_inner_points.shape[0]
    assert len(gender_list) == B
    if len(set(gender_list)) == 1:
        return fit_smpl(args, pred_inner_points, pred_part_labels, pred_confidences, gender_list[0], **fit_kwargs)
    meshes = [None] * B
    markers = torch.zeros((B, len(args.markerset), 3), dtype=torch.float32, device=pred_inner_points.device)
    valid = torch.zeros((B, len(args.markerset)), dtype=torch.bool, device=pred_inner_points.device)
    info = None
    for g in sorted(set(gender_list)):
        sel = [i for i, x in enumerate(gender_list) if x == g]
        idx = torch.tensor(sel, device=pred_inner_points.device)
        m, mk, vm, inf = fit_smpl(args, pred_inner_points[idx].contiguous(), pred_part_labels[idx].contiguous(),
                                  pred_confidences[idx].contiguous(), g, **fit_kwargs)
        if info is None:
            info = [np.zeros((B,) + a.shape[1:], a.dtype) for a in inf]
        for k, i in enumerate(sel):
            meshes[i] = m[k]
            for a, src in zip(info, inf):
                a[i] = src[k]
        markers[idx] = mk
        valid[idx] = vm
    return meshes, markers, valid, info


def surface_refine_fits(args, settings, inner, labels, confidences, gender_list, scans=None, contain=None, contain_out=None, **fit_kwargs):
    """--surface_refine: the marker fit per gender, then fit_surface on the same scans' inner points with the aggregated markers and the marker
    fit as init (models/surface_refine.py) -> fit_smpl's return layout for the whole batch, the meshes and parameters being the refined ones
    (joints in the scan's frame: (joints + trans) * scale, as inference_demo writes them).  contain (--surface_contain: fit_surface's
    containment arguments) with scans = the batch's scan meshes in the frame of the points: the term joins the loss, and contain_out (a list
    of B slots) receives per scan (metrics of the marker fit, metrics of the refined body) from containment.containment_metrics."""
    from .models.chamfer_refine import init_from_fit
    from .models.fit_SMPL import _resolve_body_model
    from .models.surface_refine import fit_surface
    B = inner.shape[0]
    meshes, info = [None] * B, None
    markers = torch.zeros((B, len(args.markerset), 3), dtype=torch.float32, device=inner.device)
    valid = torch.zeros((B, len(args.markerset)), dtype=torch.bool, device=inner.device)
    for g in sorted(set(gender_list)):
        sel = [i for i, x in enumerate(gender_list) if x == g]
        idx = torch.tensor(sel, device=inner.device)
        pts = inner[idx].contiguous()
        m0, mk, vm, _, dev = fit_smpl(args, pts, labels[idx].contiguous(), confidences[idx].contiguous(), g, return_trace=True, **fit_kwargs)
        extra = {}
        if contain is not None:
            from .containment import containment_metrics, pack_scans
            packed = pack_scans([scans[i] for i in sel], inner.device)
            before = containment_metrics(packed, np.stack([np.asarray(m.vertices, np.float32) for m in m0]))
            extra = dict(scan=packed, **contain)
        verts, prm = fit_surface(_resolve_body_model(args, g), pts, init_from_fit(dev), markers=mk, valid=vm, marker_vids=list(args.markerset.values()),
                                 **settings, **extra)
        if contain is not None and contain_out is not None:
            for i, mb, ma in zip(sel, before, containment_metrics(packed, verts)):
                contain_out[i] = (mb, ma)
        pose, beta, trans = (prm[k].cpu().numpy() for k in ("pose", "beta", "trans"))
        joints = (prm["joints"].cpu().numpy() + trans[:, None]) * prm["scale"].cpu().numpy()[:, None]
        inf = [pose[:, 3:].reshape(len(sel), -1, 3), beta, pose[:, :3], trans, joints]
        if info is None:
            info = [np.zeros((B,) + a.shape[1:], a.dtype) for a in inf]
        for k, i in enumerate(sel):
            meshes[i] = Mesh(verts[k], dev["faces"])
            for a, src in zip(info, inf):
                a[i] = src[k]
        markers[idx] = mk
        valid[idx] = vm
    return meshes, markers, valid, info


def evaluate_batch(args, model, hitpts, gender_list, ids=None, gt_vertices=None, gt_joints=None, output_folder=None, export=Mesh.export, scans=None):
    """One eval.py iteration (eval.py:87-99,181-256) on a batch (B,K,3) already on the device.
    Returns a list of per-sample dicts {id, v2v, mpjpe, valid_full} (metrics only when ground truth is given).  export(mesh, path) writes the
    predicted bodies (default Mesh.export).  With --surface_contain, scans = the batch's scan meshes (in the frame of hitpts): each record
    gains outside_share, protrusion_rms_mm, protrusion_max_mm of the refined body and the same three with the suffix _before for the
    marker fit, and containment.txt beside v2v_score.txt a line per sample."""
    B = hitpts.shape[0]
    ids = list(ids) if ids is not None else [str(i) for i in range(B)]
    with torch.no_grad():
        results, _ = model(hitpts, pred_items=["confidence", "direction", "magnitude"], direction_mode="standard_vector")
        labels = ops.argmax_rows(results["part_labels"])
        inner = ops.inner_points(hitpts.contiguous(), results["direction"], results["magnitude"], float(args.scale_magnitude))
        pp = getattr(args, "fit_pose_prior", None)              # --pose_prior (main)
        from .inference_demo import format_containment, surface_contain_settings, surface_refine_settings
        surface = surface_refine_settings(args)
        contain = surface_contain_settings(args)
        if contain is not None and scans is None:
            raise ValueError("--surface_contain needs the scans' meshes (evaluate_batch's scans)")
        contained = [None] * B
        fit_kwargs = {} if pp is None else {"pose_prior": pp}
        if surface is None:
            meshes, markers, valid, info = fit_smpl_by_gender(args, inner, labels, results["confidences"], gender_list, **fit_kwargs)
        else:
            meshes, markers, valid, info = surface_refine_fits(args, surface, inner, labels, results["confidences"], gender_list, scans=scans,
                                                               contain=contain, contain_out=contained, **fit_kwargs)
    out = []
    vsum = valid.sum(1).tolist()
    for j in range(B):
        rec = {"id": ids[j], "valid_full": int(vsum[j]) == valid.shape[1]}
        if gt_vertices is not None:
            rec["v2v"] = v2v(gt_vertices[j], meshes[j].vertices)
        if gt_joints is not None:
            rec["mpjpe"] = mpjpe(gt_joints[j], info[4][j])
        if contained[j] is not None:
            rec.update(contained[j][1])
            rec.update({k + "_before": v for k, v in contained[j][0].items()})
            if output_folder is not None:
                with open(os.path.join(output_folder, "containment.txt"), "a") as f:
                    f.write(f"{ids[j]}: {format_containment(contained[j][1])} (marker fit: {format_containment(contained[j][0])})\n")
        if output_folder is not None:
            d = os.path.join(output_folder, f"{ids[j]}")
            os.makedirs(d, exist_ok=True)
            export(meshes[j], os.path.join(d, f"forwarded_smpl_mesh_on_pred_{ids[j]}.obj"))
            np.savez(os.path.join(d, f"output_smpl_info_{ids[j]}.npz"), body_pose=info[0][j][:21, :], hand_pose=info[0][j][21:23, :],
                     betas=info[1][j], global_orient=info[2][j], transl=info[3][j], joints=info[4][j])
            if "v2v" in rec:
                with open(os.path.join(output_folder, "v2v_score.txt"), "a") as f:
                    f.write(f"{ids[j]}: {rec['v2v']}{'' if rec['valid_full'] else '  attention, the valid mask is not full'}\n")
        out.append(rec)
    return out


def build_parser():
    """eval.py:270-289's flags with their defaults, then this program's own."""
    parser = argparse.ArgumentParser(description="ETCH evaluation on one MI355X (etch_amd)")
    parser.add_argument("--activated_ids_path", type=str, default="datafolder/useful_data_4d-dress/val_ids_sampled_ratio10.pkl", help="pickled list of the ids to evaluate")
    parser.add_argument("--scale_magnitude", type=int, default=10, help="factor between the magnitude head and metres")
    parser.add_argument("--markerset_path", default="datafolder/useful_data_4d-dress/superset_smpl.json", type=str)
    parser.add_argument("--seed", type=int, default=1, metavar="S", help="seed; every scan is sampled under seed + 15")
    parser.add_argument("--infopoints_dir", type=str, default="datafolder/gt_4D-Dress_data/npz", help="folder of the per-id info-point files <id>.npz")
    parser.add_argument("--scan_dir", type=str, default="datafolder/4D-DRESS/data_processed/model", help="folder of the scans, <id>/<id>.obj")
    parser.add_argument("--smpl_dir", type=str, default="datafolder/4D-DRESS/data_processed/smplh", help="folder of the ground-truth bodies, <id>/{mesh_smpl_<id>.obj, info_<id>.npz}")
    parser.add_argument("--model_path", type=str, default=None, help="state dict of the trained model; without it the seeded initial weights are scored, with a warning")
    parser.add_argument("--batch_size", type=int, default=3, metavar="N")
    parser.add_argument("--num_point", type=int, default=5000, metavar="N", help="points sampled on each scan")
    parser.add_argument("--EPN_input_radius", type=float, default=0.4)
    parser.add_argument("--EPN_layer_num", type=int, default=2, metavar="N")
    parser.add_argument("--i", type=str, default=None, help="suffix of the output folder eval_outputs_<i>")
    # this program's own
    parser.add_argument("--body_model", type=str, default="", help="chumpy-free SMPL .pkl (else the reference's gender paths)")
    parser.add_argument("--synthetic_body", action="store_true", help="use the seeded SMPL-shaped stand-in body model")
    parser.add_argument("--output_root", type=str, default="./all_experiments/experiments")
    parser.add_argument("--ingest", type=str, default="device", choices=["host", "device"],
                        help="device: native OBJ reader one batch ahead on worker threads, GPU surface sampler, native writer; host: the Python "
                             "reader and writer and the numpy sampler, one scan at a time")
    parser.add_argument("--prefetch", type=int, default=1, help="--ingest device: batches read ahead of the GPU (0: none)")
    parser.add_argument("--view_azimuth", type=float, default=None, metavar="DEG",
                        help="score every scan from one virtual depth camera at this azimuth around the scan's bounding-box centre (--ingest device)")
    parser.add_argument("--view_elevation", type=float, default=0.0, metavar="DEG")
    parser.add_argument("--view_distance", type=float, default=2.5, metavar="M")
    parser.add_argument("--view_fov", type=float, default=45.0, metavar="DEG")
    parser.add_argument("--view_size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"))
    from .inference_demo import add_surface_refine_flags
    add_surface_refine_flags(parser)
    from .utils.prior import add_pose_prior_flags
    add_pose_prior_flags(parser)
    return parser


def view_from_args(parser, args):
    """--view_* -> the dict view_cameras takes, or None without --view_azimuth; a parser error for a view the device path cannot render."""
    if args.view_azimuth is None:
        return None
    if args.ingest != "device":
        parser.error("--view_azimuth renders on the device: it needs --ingest device")
    if not -90.0 < args.view_elevation < 90.0 or not args.view_distance > 0.0 or not 0.0 < args.view_fov < 180.0 or min(args.view_size) < 1:
        parser.error("--view_elevation must lie inside (-90, 90), --view_distance be positive, --view_fov inside (0, 180), --view_size at least 1 1")
    return {"azimuth": args.view_azimuth, "elevation": args.view_elevation, "distance": args.view_distance, "fov": args.view_fov,
            "size": tuple(args.view_size)}


def contain_from_args(parser, args, view):
    """--surface_contain's argument errors: inference_demo's, and what this command adds -- it needs the scans' meshes, which only --ingest
    device items carry, and a closed surface, which a single view is not (half a shell: its winding number is ~0.5 everywhere behind it)."""
    from .inference_demo import surface_contain_settings
    contain = surface_contain_settings(args, parser)
    if contain is not None and args.ingest != "device":
        parser.error("--surface_contain needs the scans' meshes: host-ingest items carry none, use --ingest device")
    if contain is not None and view is not None:
        parser.error("--surface_contain and --view_azimuth: a single view is half a shell and has no inside")
    return contain


def main(argv=None):
    """eval.py:270-315.  Returns (records, average v2v)."""
    from .inference_demo import load_model, resolve_body_model
    from .train import default_stuff

    parser = build_parser()
    args = parser.parse_args(argv)
    view = view_from_args(parser, args)
    from .inference_demo import surface_refine_settings
    surface_refine_settings(args, parser)
    contain_from_args(parser, args, view)
    if not torch.cuda.is_available():
        raise RuntimeError("etch_amd.eval needs a GPU: etch_amd has no CPU path")
    args.cuda = True
    args.device = torch.device("cuda")
    default_stuff(args.seed)
    args.output_folder = os.path.join(args.output_root, f"eval_outputs_{args.i}")
    os.makedirs(args.output_folder, exist_ok=True)
    with open(args.markerset_path, "r") as f:
        args.markerset = json.load(f)
    resolve_body_model(args)
    from .utils.prior import pose_prior_from_args
    args.fit_pose_prior = pose_prior_from_args(args, args.device)
    if not args.model_path:
        print("WARNING: no --model_path: scoring the seeded INITIAL weights, not a trained model (smoke runs only)", file=sys.stderr)
        args.model_path = ""
    model = load_model(args)
    dataset = EvalDataset(args.scan_dir, args.smpl_dir, args.infopoints_dir, args.activated_ids_path, num_point=args.num_point, seed=args.seed,
                          ingest=args.ingest)
    print(f"Num of data: {len(dataset)}")
    recs, avg = evaluate_dataset(args, model, dataset, batch_size=args.batch_size, prefetch=args.prefetch, view=view)
    print(f"average v2v: {avg} over {len(recs)} samples; outputs under {args.output_folder}")
    return recs, avg


if __name__ == "__main__":
    main()
