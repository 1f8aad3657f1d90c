"""The training program: the reference's src/train.py (and train_mixed.py's --aug / PRED_ITEMS) on this package's kernels.

    python -m etch_amd.train --activated_ids_path ids.pkl --markerset_path superset_smpl.json --infopoints_dir npz --scan_dir model \\
        --smpl_dir smplh --direction_w 2.5 --magnitude_w 30 --part_label_w 1 --confidence_w 50

One step = forward of GT_network_equiv in train() mode, the four losses and their gradients in one launch (etch_amd.losses), backward through
etch_amd.autograd / autograd_pt, and Adam with train.py:111-125's NaN guards in two launches (etch_amd.optim.GuardedAdam), then ONE readback
(GuardedAdam.report) for the progress line and the epoch means.  `--reference_step` runs train.py:81-125 literally instead -- torch-op losses, the
per-tensor `param.grad.sum().isnan()` loop with its ~1 900 blocking reads, torch.optim.Adam -- for comparison and for tests.

Files, as the reference names them, under <output_root>/EPN_layer_{L}_radius_{r}_num_point_{n}[_{i}]/: training_args.json, model_epochs_{epoch:08d}.pth
(model.state_dict(): what inference_demo --model_path loads), log_all/train/losses.json (+ the loss PNGs if matplotlib imports) and
train_state_{epoch:08d}.pth (optimizer state, epoch, generator states), which `--resume` reads together with the model file beside it.

`--gpus N` trains data-parallel as the reference's DataParallel (train.py:212-214) does, one process per GPU (from a plain interpreter the program
launches its ranks itself; under torch.distributed.run it uses the ranks it is given), and `--accumulate K` cuts a global batch into micro-batches
on one device.  `--batch_size` stays the GLOBAL batch: it is cut into gpus * accumulate micro-batches of batch_size / (gpus * accumulate) items, and
rank r runs micro-batches r K ... r K + K - 1, one forward / backward each.  Every contribution's gradients are packed, times 1 / (gpus * accumulate),
into one flat buffer (GuardedAdam.accumulate), ONE SUM all-reduce combines the ranks (parallel.reduce_flat), and Adam's guards run on the combined
gradient; a NaN total in any contribution skips the step.  The sequence of global batches and the --aug angles depend on --seed, --batch_size and the
dataset alone -- never on --gpus or --accumulate -- so `--gpus 2` and `--accumulate 2` see the same micro-batches and a state saved under one resumes
under another.  Normalisation statistics are DataParallel's: train-mode BatchNorm normalises per micro-batch, every rank keeps running statistics of
its own (updated once per micro-batch under --accumulate) and rank 0's are saved, as DataParallel keeps replica 0's; in train() mode no parameter
depends on them.  Rank 0 alone writes files and prints.  `--gpus 1 --accumulate 1` is the plain step above, unchanged.

Not ported: train_mixed.py's TensorBoard writer and its use_dynamic_label_confidence branch.
"""
import argparse
import json
import math
import os
import sys
import time
from collections import defaultdict

import numpy as np
import torch

from . import losses as L

PRED_ITEMS = ("confidence", "direction", "magnitude")       # train.py:76


def default_stuff(seed: int):
    """train.py:22-26."""
    torch.backends.cudnn.allow_tf32 = False
    torch.set_printoptions(precision=8, linewidth=10000, edgeitems=10, threshold=5000)
    torch.manual_seed(seed + 1)
    np.random.seed(seed + 10)


def vis_loss(all_epochs_losses, log_dir, plots=True):
    """losses.json always; train.py:28-58's PNG per loss if `plots` and matplotlib imports."""
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "losses.json"), "w") as f:
        json.dump({k: list(v) for k, v in all_epochs_losses.items()}, f, indent=4)
    if not plots:
        return
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return
    for name, values in all_epochs_losses.items():
        plt.figure()
        plt.plot(values, label=f"{name} Loss")
        plt.xlabel("Epoch")
        plt.ylabel("Loss")
        plt.title(f"{name} Loss")
        plt.legend()
        margin = max(values) * 0.1
        if math.isfinite(margin) and margin > 0:
            plt.ylim(0, max(values) + margin)
        plt.xlim(0, len(values))
        last_epoch, last_loss = len(values) - 1, values[-1]
        if math.isfinite(last_loss):
            plt.annotate(f"{last_loss:.6f}", xy=(last_epoch, last_loss), xytext=(last_epoch, last_loss + (margin if math.isfinite(margin) else 0) * 0.05),
                         arrowprops=dict(facecolor="black", shrink=0.05), fontsize=8, ha="center")
        plt.savefig(os.path.join(log_dir, f"{name}.png"))
        plt.close()


def aug_angles(generator, batch_size):
    """--aug: one angle in [0, 2 pi) per item of the batch from the seeded generator (GT_dataloader_mixed.py:189)."""
    return torch.rand((batch_size,), generator=generator, dtype=torch.float64) * (2.0 * math.pi)


def rotate_y(x, theta):
    """x (B,N,3) @ R(theta_b)^T with R = [[c,0,s],[0,1,0],[-s,0,c]] (GT_dataloader_mixed.py:190-199), on x's device.  The reference rotates the meshes
    and info points and then samples; the sampler's seed is fixed per id and labels / confidences do not change under a rotation, so rotating the
    finished item's points and vectors is the same up to rounding."""
    c, s = torch.cos(theta).to(x.device, x.dtype).view(-1, 1), torch.sin(theta).to(x.device, x.dtype).view(-1, 1)
    return torch.stack([c * x[..., 0] + s * x[..., 2], x[..., 1], c * x[..., 2] - s * x[..., 0]], -1)


def _weights(args):
    return (args.direction_w, args.magnitude_w, args.confidence_w, args.part_label_w)


def _reference_step(args, model, optimizer, results, selected_indexs, vectors, confidences, labels):
    """train.py:81-125, literally.  (On a NaN total the reference sets all_loss = 0.0 and fails in `.backward()`; here that step is left out.)"""
    losses = L.reference_losses(results, selected_indexs, vectors, confidences, labels, _weights(args), args.scale_magnitude)
    all_loss = 0.0
    for key in losses.keys():
        all_loss = all_loss + losses[key]
    if all_loss.isnan().any():
        print("Loss is NaN issue")
        return {key: losses[key].item() for key in losses}
    optimizer.zero_grad()
    all_loss.backward()
    for nm, param in model.named_parameters():
        if param.grad is None:
            pass
        elif param.grad.sum().isnan():
            param.grad = torch.zeros_like(param.grad)
    optimizer.step()
    return {key: losses[key].item() for key in losses}


def _fused_step(args, model, optimizer, results, selected_indexs, vectors, confidences, labels):
    optimizer.zero_grad()
    total, parts = L.train_losses(results, selected_indexs, vectors, confidences, labels, _weights(args), args.scale_magnitude, status=optimizer.status)
    total.backward()
    optimizer.step()
    return _report(args, optimizer, parts, results)


def _report(args, optimizer, parts, results):
    """The step's one readback, and what follows from it."""
    rep = optimizer.report(parts)
    if rep["bad_label"]:
        raise ValueError("a part label outside [0, num_parts) (or a gather index outside the targets) reached the loss")
    skipped = rep["skipped_steps"] - getattr(args, "_skipped_steps", 0)
    if skipped:
        if getattr(args, "rank", 0) == 0:
            print("Loss is NaN issue")
        args._skipped_steps = rep["skipped_steps"]
    present = {"direction_loss": "direction" in results, "magnitude_loss": "magnitude" in results, "confidence_loss": "confidences" in results,
               "part_label_loss": "part_labels" in results}
    return {key: v for key, v in zip(L.KEYS, rep["losses"]) if present[key]}


def micro_batch_size(batch_size, gpus=1, accumulate=1):
    """Items per micro-batch: a global batch of `batch_size` is cut into gpus * accumulate equal micro-batches.  ValueError for anything else."""
    if gpus < 1 or accumulate < 1:
        raise ValueError(f"--gpus and --accumulate must be at least 1, got {gpus} and {accumulate}")
    if batch_size < 1 or batch_size % (gpus * accumulate):
        raise ValueError(f"--batch_size {batch_size} (the global batch) must be a positive multiple of gpus * accumulate = {gpus} * {accumulate}")
    return batch_size // (gpus * accumulate)


def micro_batches(batch_size, gpus, accumulate, rank):
    """The (start, stop) positions within a global batch of the micro-batches rank `rank` runs, in order: micro-batches rank K ... rank K + K - 1."""
    mb = micro_batch_size(batch_size, gpus, accumulate)
    if not 0 <= rank < gpus:
        raise ValueError(f"rank {rank} outside [0, {gpus})")
    return [((rank * accumulate + k) * mb, (rank * accumulate + k + 1) * mb) for k in range(accumulate)]


def batch_plan(num_items, batch_size, generator):
    """One epoch's global batches (lists of dataset indices) exactly as DataLoader(dataset, batch_size, shuffle=True, drop_last=True,
    generator=generator) draws them, advancing `generator` as that loader's epoch does: the plan knows nothing of --gpus / --accumulate."""
    from torch.utils.data import DataLoader
    return [list(b) for b in DataLoader(range(num_items), batch_size=batch_size, shuffle=True, drop_last=True, num_workers=0, generator=generator,
                                        collate_fn=list)]


class PlannedLoader:
    """The loader of the accumulated / data-parallel path: per epoch it draws the plan every rank draws, solves (batched) the marker fields of the
    ids THIS rank will touch and has not cached, and yields per global batch this rank's items only, collated, marked `local`."""

    def __init__(self, dataset, batch_size, gpus, accumulate, rank, generator):
        self.dataset, self.batch_size, self.generator = dataset, batch_size, generator
        self.spans = micro_batches(batch_size, gpus, accumulate, rank)

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def __iter__(self):
        from torch.utils.data import default_collate
        plan = batch_plan(len(self.dataset), self.batch_size, self.generator)
        mine = [[i for a, b in self.spans for i in batch[a:b]] for batch in plan]
        self.dataset.precompute(ids=sorted({self.dataset.id_list[i] for items in mine for i in items}))
        for items in mine:
            batch = default_collate([self.dataset[i] for i in items])
            batch["local"] = True
            yield batch


def _flat_path(args):
    """True when the step goes through the flat gradient buffer: more than one contribution per step, or a process group forced on one rank."""
    from . import parallel as P
    return getattr(args, "gpus", 1) * getattr(args, "accumulate", 1) > 1 or (P.forced() and torch.distributed.is_initialized())


def _accumulated_step(args, model, optimizer, pred_items, hitpts, vectors, confidences, labels):
    """The step over this rank's micro-batches (tensors of accumulate * micro-batch items): forward / losses / backward / pack each, one all-reduce
    of the flat buffer, Adam from it, ONE readback.  Returns (losses, last micro-batch's results, its selected_indexs)."""
    from . import parallel as P
    K = getattr(args, "accumulate", 1)
    scale = 1.0 / (getattr(args, "gpus", 1) * K)
    mb = hitpts.shape[0] // K
    for k in range(K):
        sl = slice(k * mb, (k + 1) * mb)
        results, selected_indexs = model(hitpts[sl], pred_items=pred_items, direction_mode="standard_vector")
        optimizer.zero_grad()
        total, parts = L.train_losses(results, selected_indexs, vectors[sl], confidences[sl], labels[sl], _weights(args), args.scale_magnitude,
                                      status=optimizer.status)
        total.backward()
        optimizer.accumulate(scale, first=k == 0, losses=parts)
    P.reduce_flat(optimizer.flat_gradients()[0])
    optimizer.step()
    return _report(args, optimizer, optimizer.flat_losses, results), results, selected_indexs


def train(args, model, optimizer, train_loader):
    """One epoch (train.py:60-140); returns the epoch's mean losses keyed as the reference keys them.  Stops early once args.max_steps optimizer
    steps have been taken over the run.  `args.on_step`, if set, is called after every step with a dict of what the step saw.  With args.gpus *
    args.accumulate > 1 a batch of `train_loader` is a GLOBAL batch, of which this rank (args.rank) takes its micro-batches -- or, marked `local`
    (PlannedLoader), this rank's items of it; the dict then holds this rank's tensors, the last micro-batch's results and "flat_gradients" =
    optimizer.flat_gradients() with the combined gradient."""
    model.train()
    try:
        import tqdm
        pbar = tqdm.tqdm(train_loader, disable=True if getattr(args, "rank", 0) != 0 else None)
    except ImportError:
        pbar = train_loader
    flat = not getattr(args, "reference_step", False) and _flat_path(args)
    gpus, accumulate, rank = getattr(args, "gpus", 1), getattr(args, "accumulate", 1), getattr(args, "rank", 0)
    epoch_losses = defaultdict(float)
    num_batches = 0
    pred_items = list(getattr(args, "pred_items", PRED_ITEMS))
    step_fn = _reference_step if getattr(args, "reference_step", False) else _fused_step
    max_steps = getattr(args, "max_steps", None)
    on_step = getattr(args, "on_step", None)
    for batch_data in pbar:
        if max_steps is not None and getattr(args, "steps_done", 0) >= max_steps:
            break
        t0 = time.perf_counter()
        hitpts = batch_data["hitpts"].to(args.device)               # (B,N,3)
        vectors = batch_data["vectors"].to(args.device)             # (B,N,3)
        confidences = batch_data["confidences"].to(args.device)     # (B,N,1)
        labels = batch_data["labels"].to(args.device)               # (B,N)
        seen = {}
        if flat:
            local = bool(batch_data.get("local", False))
            mine = hitpts.shape[0] if local else accumulate * micro_batch_size(hitpts.shape[0], gpus, accumulate)
            first = rank * mine                                      # this rank's items are [first, first + mine) of the global batch
            if not local:
                hitpts, vectors, confidences, labels = (t[first:first + mine] for t in (hitpts, vectors, confidences, labels))
            if getattr(args, "aug", False):                          # the angles of the GLOBAL batch, sliced: the generator advances alike on every rank
                theta = aug_angles(args.aug_generator, mine * gpus)[first:first + mine]
                hitpts, vectors = rotate_y(hitpts, theta), rotate_y(vectors, theta)
            values, results, selected_indexs = _accumulated_step(args, model, optimizer, pred_items, hitpts, vectors, confidences, labels)
            seen["flat_gradients"] = optimizer.flat_gradients()
        else:
            if getattr(args, "aug", False):
                theta = aug_angles(args.aug_generator, hitpts.shape[0])
                hitpts, vectors = rotate_y(hitpts, theta), rotate_y(vectors, theta)
            results, selected_indexs = model(hitpts, pred_items=pred_items, direction_mode="standard_vector")
            values = step_fn(args, model, optimizer, results, selected_indexs, vectors, confidences, labels)
        if hasattr(pbar, "set_description"):
            pbar.set_description("Batch losses: " + "".join(f"{key}: {v:.05f}, " for key, v in values.items()))
        num_batches += 1
        for key, v in values.items():
            epoch_losses[key] += v
        args.steps_done = getattr(args, "steps_done", 0) + 1
        if hasattr(args, "step_seconds"):
            args.step_seconds.append(time.perf_counter() - t0)       # ends behind the step's readback: the device has finished the step
        if on_step is not None:
            on_step({"hitpts": hitpts, "vectors": vectors, "confidences": confidences, "labels": labels, "results": results,
                     "selected_indexs": selected_indexs, "losses": values, **seen})
    for key in epoch_losses.keys():
        epoch_losses[key] /= max(num_batches, 1)
    return epoch_losses


def _bool(s):
    if isinstance(s, bool):
        return s
    if s.lower() in ("1", "true", "yes", "y"):
        return True
    if s.lower() in ("0", "false", "no", "n"):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {s}")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m etch_amd.train", description=__doc__.split("\n\n")[0])
    # train.py:146-172, with its defaults
    parser.add_argument("--activated_ids_path", type=str, default="datafolder/useful_data_4d-dress/train_ids.pkl", help="activated ids")
    parser.add_argument("--scale_magnitude", type=int, default=10, help="scaling ratio for magnitude")
    parser.add_argument("--markerset_path", default="datafolder/useful_data_4d-dress/superset_smpl.json", type=str)
    parser.add_argument("--vis_loss", type=_bool, default=True, help="whether visualize loss when training or not")
    parser.add_argument("--infopoints_dir", type=str, default="datafolder/gt_4D-Dress_data/npz", help="data dir path of npy files")
    parser.add_argument("--scan_dir", type=str, default="datafolder/4D-DRESS/data_processed/model", help="data dir path of obj files")
    parser.add_argument("--smpl_dir", type=str, default="datafolder/4D-DRESS/data_processed/smplh", help="data dir path of smpl files")
    parser.add_argument("--batch_size", type=int, default=1, metavar="N", help="input batch size for training")
    parser.add_argument("--epochs", type=int, default=30, metavar="N", help="number of epochs to train")
    parser.add_argument("--lr", type=float, default=1e-4, metavar="N", help="learning rate")
    parser.add_argument("--seed", type=int, default=1, metavar="S", help="random seed (default: 1)")
    parser.add_argument("--num_point", type=int, default=5000, metavar="N", help="point num sampled from mesh surface")
    parser.add_argument("--EPN_input_radius", type=float, default=0.4)
    parser.add_argument("--EPN_layer_num", type=int, default=2, metavar="N")
    parser.add_argument("--direction_w", type=float, default=1.0)
    parser.add_argument("--magnitude_w", type=float, default=1.0)
    parser.add_argument("--part_label_w", type=float, default=1.0)
    parser.add_argument("--confidence_w", type=float, default=1.0)
    parser.add_argument("--i", type=str, default=None, help="suffix of the experiment folder")
    # train_mixed.py
    parser.add_argument("--aug", type=_bool, nargs="?", const=True, default=False, help="rotate every item about y by a seeded random angle")
    parser.add_argument("--pred_items", type=str, default=",".join(PRED_ITEMS), help="comma list of the heads to train: confidence, direction, magnitude")
    # this program's own
    parser.add_argument("--resume", type=str, default=None, metavar="PATH", help="a train_state_{epoch:08d}.pth to continue from (the model file beside it is loaded)")
    parser.add_argument("--max_steps", type=int, default=None, metavar="N", help="stop after N optimizer steps (smoke runs)")
    parser.add_argument("--output_root", type=str, default="./all_experiments/experiments")
    parser.add_argument("--reference_step", action="store_true", help="the reference's literal step (torch-op losses, the per-tensor Python guard loop, "
                        "torch.optim.Adam): for comparison and tests")
    parser.add_argument("--gpus", type=int, default=1, help="devices to train on, one process each: --batch_size is split over them (DataParallel)")
    parser.add_argument("--accumulate", type=int, default=1, metavar="K", help="micro-batches per device and step: --batch_size (the global batch) is "
                        "cut into gpus * K micro-batches whose gradients are averaged")
    parser.add_argument("--partial_views", type=float, default=0.0, metavar="P", help="probability that an item's points are what one random depth camera "
                        "sees of the scan (etch_amd.depth.ViewSpec); the camera depends on (seed, epoch, item) only")
    parser.add_argument("--view_elevation", type=float, nargs=2, default=(-10.0, 30.0), metavar=("LO", "HI"), help="degrees")
    parser.add_argument("--view_distance", type=float, default=2.5, metavar="M")
    parser.add_argument("--view_fov", type=float, default=45.0, metavar="DEG")
    parser.add_argument("--view_size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
    return parser


def view_spec_from_args(args):
    """--partial_views P and the --view_* flags -> the dataset's ViewSpec, or None for P = 0 (the dataset of a run without the flags)."""
    if not args.partial_views:
        return None
    from .depth import ViewSpec
    return ViewSpec(probability=args.partial_views, elevation_range=tuple(args.view_elevation), distance=args.view_distance, fov_deg=args.view_fov,
                    size=tuple(args.view_size))


def make_model(args):
    from .models.models_pointcloud import GT_network_equiv
    if getattr(args, "rank", 0) != 0:
        # the constructor dumps EPN_model_setting_json into option.output_folder: that file is rank 0's, the other ranks' copy goes to a scratch folder
        import copy
        import tempfile
        with tempfile.TemporaryDirectory() as scratch:
            option = copy.copy(args)
            option.output_folder = scratch
            return GT_network_equiv(option=option).to(args.device)
    return GT_network_equiv(option=args).to(args.device)


def make_optimizer(args, model):
    if args.reference_step:
        return torch.optim.Adam(model.parameters(), lr=args.lr)
    from .optim import GuardedAdam
    return GuardedAdam(model.parameters(), lr=args.lr)


def _generator_states(args, loader_generator):
    return {"torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(args.device), "numpy": np.random.get_state(),
            "loader": loader_generator.get_state(), "aug": args.aug_generator.get_state()}


def _set_generator_states(args, loader_generator, st):
    torch.set_rng_state(st["torch"])
    torch.cuda.set_rng_state(st["cuda"], args.device)
    np.random.set_state(st["numpy"])
    loader_generator.set_state(st["loader"])
    args.aug_generator.set_state(st["aug"])


def main(argv=None):
    from torch.utils.data import DataLoader

    from .datasets import GTDataset

    from . import parallel as P

    parser = build_parser()
    args = parser.parse_args(argv)
    # argument errors first: nothing below them has touched a GPU or started a process
    try:
        micro_batch_size(args.batch_size, args.gpus, args.accumulate)
    except ValueError as e:
        parser.error(str(e))
    if args.gpus > P.MAX_RANKS:
        parser.error(f"--gpus {args.gpus}: at most {P.MAX_RANKS} ranks")
    if args.reference_step and args.gpus * args.accumulate > 1:
        parser.error("--reference_step is the reference's literal single-device step: it takes --gpus 1 --accumulate 1")
    try:
        view = view_spec_from_args(args)
    except ValueError as e:
        parser.error(f"--partial_views: {e}")
    args.pred_items = [s.strip() for s in args.pred_items.split(",") if s.strip()]
    if not args.pred_items or any(s not in PRED_ITEMS for s in args.pred_items):
        raise ValueError(f"--pred_items must be a comma list out of {PRED_ITEMS}")
    if args.gpus > 1 and "RANK" not in os.environ:
        # a plain interpreter: this process launches the ranks and never touches the GPU itself
        rc = P.launch_ranks([sys.executable, "-m", "etch_amd.train"] + list(sys.argv[1:] if argv is None else argv), args.gpus)
        if rc:
            raise SystemExit(rc)
        return {}
    rank, world, local = P.env_rank_world()
    if world != args.gpus:
        parser.error(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if world > 1:
        try:
            P.pin_to_local_cores(local, world)                   # before the GPU runtime starts its helper threads
        except Exception as e:                                  # an unreadable / unexpected topology must not stop the job
            print(f"[train] rank {rank}: CPU pinning skipped ({type(e).__name__}: {e})", file=sys.stderr)
    if not torch.cuda.is_available():
        raise RuntimeError("etch_amd.train needs a GPU: etch_amd has no CPU path")
    args.rank = rank
    say = print if rank == 0 else (lambda *a, **k: None)          # rank 0 alone prints and writes files
    args_dict = dict(vars(args))
    del args_dict["rank"]

    default_stuff(args.seed)
    if os.environ.get("ETCH_ALL_RANKS_DEVICE0"):                  # the multi-rank control flow on a 1-GPU box (with ETCH_DIST_BACKEND=gloo)
        local = 0
    torch.cuda.set_device(local)
    args.device = torch.device("cuda", local)
    P.init()
    flat = not args.reference_step and _flat_path(args)

    exps_folder = "EPN_layer_{}_radius_{}".format(args.EPN_layer_num, args.EPN_input_radius) + f"_num_point_{args.num_point}"
    if args.i is not None:
        exps_folder = exps_folder + f"_{args.i}"
    output_folder = os.path.join(args.output_root, exps_folder)
    args.output_folder = output_folder
    log_dir = os.path.join(output_folder, "log_all")
    if rank == 0:
        os.makedirs(output_folder, exist_ok=True)
        os.makedirs(log_dir, exist_ok=True)
        args_save_path = os.path.join(output_folder, "training_args.json")
        with open(args_save_path, "w") as f:
            json.dump(args_dict, f, indent=4)
        print(f"Training args saved to {args_save_path}")

    with open(args.markerset_path, "r") as f:
        args.markerset = json.load(f)

    model = make_model(args)
    say("======== Running on single GPU ========" if world == 1 else f"======== Running on {world} GPUs ========")
    optimizer = make_optimizer(args, model)
    if flat:
        backend = torch.distributed.get_backend() if torch.distributed.is_initialized() else "none"
        say(f"======== Flat gradient path: {args.gpus * args.accumulate} contribution(s) per step, all-reduce backend {backend}, world {world} ========")

    dataset = GTDataset(args, device=args.device, verbose=rank == 0, view=view)
    loader_generator = torch.Generator().manual_seed(args.seed)
    args.aug_generator = torch.Generator().manual_seed(args.seed + 100)
    if flat:
        train_loader = PlannedLoader(dataset, args.batch_size, args.gpus, args.accumulate, rank, loader_generator)
    else:
        dataset.precompute()
        train_loader = DataLoader(dataset, batch_size=args.batch_size, shuffle=True, drop_last=True, num_workers=0, generator=loader_generator)

    all_epochs_losses = defaultdict(list)
    first_epoch = 0
    args.steps_done, args.step_seconds = 0, []
    if args.resume:
        state = torch.load(args.resume, map_location="cpu", weights_only=False)
        model_path = os.path.join(os.path.dirname(os.path.abspath(args.resume)), f"model_epochs_{state['epoch']:08d}.pth")
        model.load_state_dict(torch.load(model_path, map_location=args.device))
        optimizer.load_state_dict(state["optimizer"])
        _set_generator_states(args, loader_generator, state["generators"])
        all_epochs_losses.update({k: list(v) for k, v in state["losses"].items()})
        first_epoch, args.steps_done = state["epoch"] + 1, state["steps_done"]
        say(f"Resumed from {args.resume}: epoch {state['epoch']} done")

    average_epoch_losses = {}
    for epoch in range(first_epoch, args.epochs):
        if args.max_steps is not None and args.steps_done >= args.max_steps:
            break
        say(f"====== Epoch {epoch} start! ====== \n")
        dataset.set_epoch(epoch)
        average_epoch_losses = train(args, model, optimizer, train_loader)
        say(f"===== Average losses of Epoch {epoch} are: " + "".join(f"{k}: {v:.05f}, " for k, v in average_epoch_losses.items()) + "======\n")
        for key in average_epoch_losses.keys():
            all_epochs_losses[key].append(average_epoch_losses[key])
        if rank != 0:
            continue
        vis_loss(all_epochs_losses, os.path.join(log_dir, "train"), plots=args.vis_loss)
        torch.save(model.state_dict(), os.path.join(output_folder, f"model_epochs_{epoch:08d}.pth"))
        torch.save({"epoch": epoch, "steps_done": args.steps_done, "optimizer": optimizer.state_dict(),
                    "generators": _generator_states(args, loader_generator), "losses": dict(all_epochs_losses)},
                   os.path.join(output_folder, f"train_state_{epoch:08d}.pth"))
    if len(args.step_seconds) > 10:
        # wall time per step behind the readback, the first five (code-object loads, allocator growth) left out
        ms = np.sort(np.array(args.step_seconds[5:])) * 1e3
        say(f"step wall time over {len(ms)} steps: median {np.median(ms):.2f} ms, p10 {ms[int(0.1 * (len(ms) - 1))]:.2f} ms, "
              f"p90 {ms[int(math.ceil(0.9 * (len(ms) - 1)))]:.2f} ms")
    if torch.distributed.is_initialized():
        P.barrier()                                               # rank 0's last files are written before any rank leaves
        torch.distributed.destroy_process_group()
    return dict(average_epoch_losses)


if __name__ == "__main__":
    main()
