"""Fit, register and animate one scan:

    python -m etch_amd.animate --scan_path scan.obj --new_pose poses.npz [--carry scan] [inference_demo's flags]

The fit is inference_demo's (with --chamfer_refine the refined one); the registration deforms the SMPL topology onto the scan (SMPL+D,
models/register.py); every pose of --new_pose re-poses the registered body and, with --carry scan, the scan itself.  Written to
--output_folder: smpld_<name>.obj, registration_<name>.npz (offsets, params, energy), smpld_<name>_<k>.obj and with --carry scan
scan_<name>_<k>.obj (all scan vertices, the scan's faces) and scan_<name>_<k>_filtered.obj (the faces animate.py:30-53 keeps).

This is what the reference's src/animate.py is for; that file cannot run (its skin-weight-transfer submodule is absent).  Here the skinning
weights of a scan vertex are those of its closest point on the registered surface, so nothing is transferred by thresholds or inpainted."""
import os

import numpy as np
import torch

from . import inference_demo as demo
from . import mesh_io
from .models.fit_SMPL import Mesh


def read_pose_file(path, nj=24):
    """--new_pose: an .npz, or a .pt dict (loaded with weights_only=True).  body_pose (K, 3 (nj - 1)) or (K, nj - 1, 3) (a single pose may
    drop K); global_orient and transl (K,3) or (3,), optional.  -> {body_pose (K, 3 (nj - 1)), global_orient (K,3) or None, transl (K,3) or
    None} float32 numpy.  Whatever is None keeps the fit's value, as betas always do (animate.py:144-149)."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            raw = {k: z[k] for k in z.files}
    else:
        raw = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(raw, dict):
            raise ValueError(f"{path}: expected a dict with body_pose")
    if "body_pose" not in raw:
        raise ValueError(f"{path}: no body_pose")
    arr = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float32)
    w = 3 * (nj - 1)
    bp = arr(raw["body_pose"])
    if bp.shape in ((w,), (nj - 1, 3)):
        bp = bp.reshape(1, w)
    if not (bp.ndim >= 2 and bp.shape[0] >= 1 and (bp.shape[1:] == (w,) or bp.shape[1:] == (nj - 1, 3))):
        raise ValueError(f"{path}: body_pose must be (K,{w}) or (K,{nj - 1},3), got {bp.shape}")
    bp = np.ascontiguousarray(bp.reshape(-1, w))
    K = bp.shape[0]
    out = dict(body_pose=bp, global_orient=None, transl=None)
    for k in ("global_orient", "transl"):
        if k in raw and raw[k] is not None:
            a = arr(raw[k]).reshape(-1, 3)
            if a.shape[0] not in (1, K):
                raise ValueError(f"{path}: {k} must be (3,) or ({K},3), got {a.shape}")
            out[k] = np.array(np.broadcast_to(a, (K, 3)))
    return out


def new_params(params, poses, nj, nb):
    """The fit's packed params (1,P) with every pose of read_pose_file's dict put in -> (K,P)."""
    K = poses["body_pose"].shape[0]
    p = params.reshape(1, -1).repeat(K, 1).clone()
    put = lambda a: torch.from_numpy(a).to(p)
    p[:, 3:3 * nj] = put(poses["body_pose"])
    if poses["global_orient"] is not None:
        p[:, :3] = put(poses["global_orient"])
    if poses["transl"] is not None:
        p[:, 3 * nj + nb:3 * nj + nb + 3] = put(poses["transl"])
    return p.contiguous()


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--scan_path", type=str, required=True, help="Path to input scan OBJ file")
    demo.add_flags(parser)
    parser.add_argument("--new_pose", type=str, required=True, help=".npz or .pt with body_pose (K,69) or (K,23,3) [, global_orient, transl]")
    parser.add_argument("--register_points", type=int, default=20000, help="surface samples of the scan the registration runs against")
    parser.add_argument("--register_iters", type=int, default=300)
    parser.add_argument("--smooth_w", type=float, nargs=2, default=(10.0, 0.1), metavar=("L0", "L1"), help="first and last smoothness weight")
    parser.add_argument("--trunc", type=float, default=0.05, help="body vertices further than this (m) from the scan do not pull; < 0: off")
    parser.add_argument("--carry", type=str, default="none", choices=["scan", "none"], help="scan: also re-pose the scan's own vertices")
    return parser.parse_args(argv)


def _drop_unreferenced(verts, faces):
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[faces]


def main(argv=None):
    from .models import register as RG

    args = parse_args(argv)
    model, export, points, centered, center, name = demo.prepare(args)
    out = lambda f: os.path.join(args.output_folder, f)

    # 1. the fit (and its refinement): inference_demo's
    _, bm, _, prm = demo.fit_and_refine(args, model, points, centered)
    nj, nb = bm.num_joints, bm.num_betas
    params = RG.pack_params({k: prm[k] for k in ("pose", "beta", "trans", "scale")}, nj, nb, args.device, 1)

    # 2. the registration, against a sample of the centred scan's surface
    pts, _, _ = mesh_io.sample_surface([centered], args.register_points, [args.seed], center=False, device=args.device)
    reg = RG.register_smpld(bm, pts, params, iterations=args.register_iters, smooth_w=tuple(args.smooth_w), trunc=None if args.trunc < 0 else args.trunc)
    export(Mesh(reg["verts"][0].cpu().numpy().astype(np.float64) + center, bm.faces), out(f"smpld_{name}.obj"))
    np.savez(out(f"registration_{name}.npz"), offsets=reg["offsets"][0].cpu().numpy(), params=params[0].cpu().numpy(), energy=reg["energy"][0].cpu().numpy())

    # 3. every new pose: the registered body, and the scan bound to it
    poses = read_pose_file(args.new_pose, nj)
    p_new = new_params(params, poses, nj, nb)
    K = p_new.shape[0]
    v_new = RG.repose(bm, p_new, reg["offsets"].expand(K, -1, -1)).cpu().numpy().astype(np.float64)
    for k in range(K):
        export(Mesh(v_new[k] + center, bm.faces), out(f"smpld_{name}_{k}.obj"))
    if args.carry == "scan":
        raw = torch.from_numpy(np.asarray(centered.vertices, np.float64)).to(args.device)
        faces = np.asarray(centered.faces, np.int64)
        face, bary = RG.bind_scan(reg["verts"][0], bm.faces, raw)
        for k in range(K):
            moved = RG.carry_scan(bm, params, p_new[k:k + 1], face, bary, raw)
            keep = RG.filter_faces(raw, moved, faces).cpu().numpy()
            moved = moved.cpu().numpy() + center
            export(Mesh(moved, faces), out(f"scan_{name}_{k}.obj"))
            export(Mesh(*_drop_unreferenced(moved, faces[keep])), out(f"scan_{name}_{k}_filtered.obj"))
    print(f"Registration and {K} re-posed meshes saved under {args.output_folder}")


if __name__ == "__main__":
    main()
