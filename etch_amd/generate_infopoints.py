"""MI355X counterpart of scripts/generate_infopoints.py: the tightness info points of (scan, fitted body) pairs, same flags, same output layout.

    python -m etch_amd.generate_infopoints [-m 0] [-f_m MODEL_DIR] [-f_s SMPL_DIR] [-f_p PLY_DIR] [-f_n NPZ_DIR]
    python -m etch_amd.generate_infopoints -m 1 -s scan.obj -b body.obj          (writes <scan name>.ply / .npz in the working directory)

Mode 0 walks the ids present in both -f_m and -f_s (sorted) and writes <-f_p>/<id>.ply and <-f_n>/<id>.npz.  Scans run one at a time on one
stream; -p / --parallel (the reference's 32-process pool) is accepted and ignored.  Added: --seed (the reference's sampling is unseeded) and
--self_face (etch_amd.infopoints: "exclude" by default, "reference" for the reference's self-hit rule).
"""
import argparse
import os
import sys

from .inference_demo import load_obj
from .infopoints import SELF_FACE_MODES, generate_infopoints, write_outputs


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-p", "--parallel", default=True, help="accepted and ignored: scans run one at a time on the GPU", type=bool)
    parser.add_argument("-m", "--mode", default=0, help="0: walk -f_m / -f_s, 1: one pair from -s / -b", type=int)
    parser.add_argument("-l", "--ray_length", default=0.16, type=float)
    parser.add_argument("-l_ops", "--ray_length_ops", default=0.025, type=float)
    parser.add_argument("--num_samples", default=30000, type=int)
    parser.add_argument("-f_m", "--folder_model", default="datafolder/4D-DRESS/data_processed/model", help="folder of <id>/<id>.obj scans", type=str)
    parser.add_argument("-f_s", "--folder_smpl", default="datafolder/4D-DRESS/data_processed/smplh", help="folder of <id>/mesh_smpl_<id>.obj bodies",
                        type=str)
    parser.add_argument("-f_p", "--folder_ply", default="datafolder/gt_4D-Dress_data/ply", help="output folder of <id>.ply", type=str)
    parser.add_argument("-f_n", "--folder_npz", default="datafolder/gt_4D-Dress_data/npz", help="output folder of <id>.npz", type=str)
    parser.add_argument("-s", "--scan_obj", help="mode 1: scan obj file", type=str)
    parser.add_argument("-b", "--body_obj", help="mode 1: body obj file", type=str)
    parser.add_argument("--seed", default=0, type=int, help="seed of the body sampling")
    parser.add_argument("--self_face", default="exclude", choices=SELF_FACE_MODES, help="test 3: skip the sample's own face (default) or not")
    return parser.parse_args(argv)


def pair_ids(folder_model, folder_smpl):
    """Ids with a directory in both folders, sorted."""
    def dirs(d):
        return {i for i in os.listdir(d) if os.path.isdir(os.path.join(d, i))}
    return sorted(dirs(folder_model) & dirs(folder_smpl))


def run_pair(args, scan_path, body_path, ply_path, npz_path):
    ip, iv, counts = generate_infopoints(load_obj(scan_path), load_obj(body_path), num_samples=args.num_samples, ray_length=args.ray_length,
                                         ray_length_ops=args.ray_length_ops, seed=args.seed, self_face=args.self_face)
    write_outputs(ip, iv, ply_path, npz_path)
    return counts


def main(argv=None):
    args = parse_args(argv)
    print(f"\n ray_length={args.ray_length}, ray_length_ops={args.ray_length_ops}\n")
    if args.mode == 0:
        os.makedirs(args.folder_ply, exist_ok=True)
        os.makedirs(args.folder_npz, exist_ok=True)
        for i in pair_ids(args.folder_model, args.folder_smpl):
            counts = run_pair(args, os.path.join(args.folder_model, i, f"{i}.obj"), os.path.join(args.folder_smpl, i, f"mesh_smpl_{i}.obj"),
                              os.path.join(args.folder_ply, f"{i}.ply"), os.path.join(args.folder_npz, f"{i}.npz"))
            print(i, counts, flush=True)
    elif args.mode == 1:
        # The reference's mode 1 passes the undefined names model_path / smpl_path (and a fixed id "abcd"); here it reads -s / -b and names
        # the outputs after the scan file.
        if not args.scan_obj or not args.body_obj:
            raise SystemExit("mode 1 needs -s/--scan_obj and -b/--body_obj")
        i = os.path.splitext(os.path.basename(args.scan_obj))[0]
        print(i, run_pair(args, args.scan_obj, args.body_obj, f"{i}.ply", f"{i}.npz"), flush=True)
    else:
        raise SystemExit(f"unknown mode {args.mode}")


if __name__ == "__main__":
    main(sys.argv[1:])
