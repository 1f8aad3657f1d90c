#!/usr/bin/env python3
"""Headline benchmark of the ETCH hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

N > 1: one rank per GPU.  Either the driver launches the ranks (`python -m torch.distributed.run --nproc-per-node N bench.py ...`:
RANK / LOCAL_RANK / WORLD_SIZE are then in the environment) or a plain `python bench.py --gpus N` launches them itself: the parent
process -- which never touches the GPU -- starts N children with the rank environment, relays rank 0's JSON line and exits with
the children's return code.  Every rank pins itself to the cores of its GPU's NUMA node before initialising the GPU.

One step = one pass of the full hot path over one batch of synthetic scans already resident in HBM:
  stage 1  GT_network_equiv.forward (EPN encoder + confidence / direction / magnitude heads)
  glue     argmax labels, inner points = points - direction * magnitude / 10
  stage 2  get_markers + (30 + 50)-iteration LM SMPL fit + final full-mesh LBS
Workload (BASELINE.json configs[2], the configuration the metric is quoted on): 32 scans x 5000 points per GPU
(weak scaling: every rank processes its own 32 scans; no collective on the data path; one RCCL all_gather of the
per-scan result rows at the end of the job).  Every step gets its own, distinct batch of scans (all resident in HBM before the
timed region).  `--forward-only` measures BASELINE.json configs[1] (equivariant forward only) instead.  Prints ONE JSON line on rank 0.

A plain run does only what the headline figure needs: set up, warm up, time the K steps, write --dump-outputs, print the line.  `--full` adds
every other leg: the single-scan latency (one of it in a child process of its own), the synchronous schedule, the well-posed-marker leg, the
instrumented roofline pass, the stage-2 latency and the CPU baseline with its parity numbers (with --train: the phase split and the CPU step).
"""
import argparse
import collections
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix peak (v_mfma_f32_*_f32)
F16_MFMA_PEAK_TFLOPS = 2500.0      # MI355X_MICROARCH.md: dense bf16 / fp16 matrix peak (v_mfma_f32_32x32x16_{f16,bf16}); measured there 2495
HBM_PEAK_GBS = 8000.0


def synth_scan(global_index, n):
    """rng(1000 + b).standard_normal((N,3)) * (0.14, 0.31, 0.085), fp32."""
    return (np.random.default_rng(1000 + global_index).standard_normal((n, 3)) * np.array([0.14, 0.31, 0.085])).astype(np.float32)


def build(device, seed=1, body="smpl"):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.body_model import SyntheticSMPL, SyntheticSMPLX
    from etch_amd.utils.weights import load_seeded

    bm = SyntheticSMPL(7) if body == "smpl" else SyntheticSMPLX(7)
    args = types.SimpleNamespace(output_folder=os.path.join("/tmp", f"etch_bench_{os.getpid()}"), EPN_input_radius=0.4, EPN_layer_num=2,
                                 device=device, markerset=K.default_markerset(), scale_magnitude=10, body_model=bm)
    model = load_seeded(GT_network_equiv(option=args), seed).to(device).eval()
    return args, model


# ------------------------------------------------------------------------------------------------ roofline
SOURCE_OF_KERNEL = {"inter_so3conv_y_kernel": "so3conv_y.hip", "inter_so3conv_x_kernel": "so3conv_x.hip", "inter_so3conv_kernel": "so3conv.hip", "gemm_nt_kernel": "gemm.hip",
                    "mhsa_layer_kernel": "mhsa_layer.hip", "mhsa_layer_kernel<3>": "mhsa_layer.hip", "mhsa_interp_layer_kernel": "mhsa_layer.hip", "linear_relu_dot_ws_kernel": "fused_dense.hip"}


def algorithmic_flops(name, a):
    """Algorithmic FLOPs of one C-ABI call from its integer arguments (DESIGN.md 'work per launch')."""
    v = [x.value if hasattr(x, "value") else x for x in a]
    if name == "etch_linear":
        R, K, O = v[0], v[1], v[2]
        return 2.0 * R * K * O, f"gemm_nt_kernel"
    if name in ("etch_linear_relu_dot", "etch_linear_relu_dot_split", "etch_linear_relu_dot_f16"):
        R, K, G, J = v[0], v[1], v[2], v[3]
        ws = name.endswith("f16") or (name.endswith("split") and K <= 128 and (G >= 8 or G == 1))          # the dispatch of etch_linear_relu_dot_split
        return 2.0 * R * G * J * (K + 1), ("linear_relu_dot_ws_kernel" if ws else "linear_relu_dot_bx_kernel") if not name.endswith("dot") else "linear_relu_dot_kernel"
    if name in ("etch_inter_so3conv", "etch_inter_so3conv_ordered", "etch_inter_so3conv_split"):
        b, cin, cout, p1, p2, nn = v[0:6]
        kern = "inter_so3conv_c1_kernel" if cin == 1 else f"inter_so3conv_kernel<{cin},{cout},{(nn + 15) // 16 if nn <= 32 else 4}{',split' if name.endswith('split') else ''}>"
        return 2.0 * b * p2 * 60 * 24 * (cin * nn + cout * cin), kern
    if name in ("etch_inter_so3conv_planes", "etch_inter_so3conv_planes32"):     # both contractions on the bf16 matrix cores (csrc/so3conv_x.hip)
        b, cin, cout, p1, p2, nn = v[0:6]
        kern = f"inter_so3conv_x32_kernel<{cin},{cout},{nn // 32}>" if name.endswith("32") else f"inter_so3conv_x_kernel<{cin},{cout},{nn // 32}>"
        return 2.0 * b * p2 * 60 * 24 * (cin * nn + cout * cin), kern
    if name == "etch_inter_so3conv_planes_kq":     # round 5: two fp16 planes per operand, weights' pre-activation on the matrix cores (csrc/so3conv_y.hip)
        b, cin, cout, p1, p2, nn = v[0:6]
        return 2.0 * b * p2 * 60 * 24 * (cin * nn + cout * cin), f"inter_so3conv_y_kernel<{cin},{cout},{nn // 32}>"
    if name == "etch_inter_so3conv32":
        b, cin, cout, p1, p2, nn = v[0:6]
        return 2.0 * b * p2 * 60 * 24 * (cin * nn + cout * cin), f"inter_so3conv32_kernel<{cin},{cout},{(nn + 7) // 8}>"
    if name in ("etch_intra_so3conv", "etch_intra_so3conv_stats", "etch_intra_so3conv32", "etch_intra_so3conv_split", "etch_intra_so3conv_f16"):
        b, c, cout, p = v[0:4]
        kern = "intra_so3conv_ws_kernel" if name.endswith(("split", "f16")) else "intra_so3conv32_kernel" if name.endswith("32") else "intra_so3conv_kernel"
        return 2.0 * b * p * 60 * 12 * c * cout, kern + f"<{c},{cout}>"
    if name == "etch_mhsa_layer":
        T, mode = v[0], v[7]
        return T * (2.0 * 60 * 64 * 192 + 8 * (2.0 * 60 * 60 * 8 * 2) + (2.0 * 60 * 64 * 64 if mode != 2 else 0.0)), "mhsa_layer_kernel"
    if name == "etch_mhsa_layer_dirtail":    # heads of the last layer + the folded tail (64 -> 128 hidden -> 1 per token) in mhsa_layer_kernel<3>
        return v[0] * (2.0 * 60 * 64 * 192 + 8 * (2.0 * 60 * 60 * 8 * 2) + 2.0 * 60 * 64 * 128 + 2.0 * 60 * 128), "mhsa_layer_kernel<3>"
    if name == "etch_mhsa_interp_layer":   # mode-0 layer on tokens interpolated in the kernel
        return float(v[0]) * v[1] * (2.0 * 60 * 64 * 192 + 8 * (2.0 * 60 * 60 * 8 * 2) + 2.0 * 60 * 64 * 64), "mhsa_interp_layer_kernel"
    if name == "etch_pt_attention_mfma":     # the c -> c/8 -> c/8 MLP of linear_w over the n * ns (point, neighbour) rows
        n, c, ns = v[0:3]
        return float(n) * ns * (2.0 * c * (c // 8) + 2.0 * (c // 8) ** 2), "pt_attention_mfma_kernel"
    if name == "etch_mhsa_attention":
        T = v[0]
        return T * 8 * (2.0 * 60 * 60 * 8 * 2), "mhsa_attention_kernel"
    return 0.0, KERNEL_OF_ENTRY.get(name, name.replace("etch_", "") + "_kernel")


# C-ABI entry -> the kernel it launches (entries without a flop model; `kernel_breakdown_ms` names kernels, not entry points)
KERNEL_OF_ENTRY = {
    "etch_smpl_lm_fit": "smpl_lm_fit_kernel", "etch_smpl_lm_fit_split": "smpl_lm_fit_kernel (one workgroup per scan above 8 scans)", "etch_smpl_lbs": "smpl_lbs_kernel",
    "etch_furthest_point_sampling": "fps_kernel", "etch_furthestsampling": "fps_kernel", "etch_ball_query": "ball_query_kernel", "etch_knnquery": "knn_wave_kernel",
    "etch_instnorm_act_add_planes": "instnorm_act_add_kernel", "etch_instnorm_act_add_planes_f16": "instnorm_act_add_kernel", "etch_instnorm_stats": "instnorm_partial_kernel + instnorm_final_kernel",
    "etch_instnorm_from_partials": "instnorm_from_partials_kernel", "etch_get_markers": "get_markers_kernel", "etch_so3_mean_dir": "so3_mean_dir_kernel",
    "etch_prop3nn": "prop3nn_kernel", "etch_prop_interp": "prop_interp_kernel", "etch_token_mean": "token_mean_kernel", "etch_spatial_order": "spatial_order_kernel",
    "etch_pt_down_gather_max": "pt_down_gather_max_kernel", "etch_pt_interp_add": "pt_interp_add_kernel", "etch_gather_points_forward": "gather_points_kernel",
}


def blob_hash(path):
    """git's blob hash of a file (sha1 over 'blob <size>\\0' + content): the profile summaries under profiles/ record it for the kernel sources
    they were collected from, bench.py marks a quoted counter `stale` when the source has changed since."""
    import hashlib
    data = open(path, "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def profile_pass(run_step):
    """One instrumented step: every C-ABI call bracketed by HIP events on the stream it is launched on."""
    from etch_amd import _lib

    rec = []

    def prof(name, args, fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        st = fn(*args)
        e.record()
        rec.append((name, args, s, e))
        return st

    lib = _lib.lib()
    lib.profiler = prof
    try:
        run_step()
        torch.cuda.synchronize()
    finally:
        lib.profiler = None
    agg = collections.OrderedDict()
    for name, args, s, e in rec:
        fl, kern = algorithmic_flops(name, args)
        d = agg.setdefault(kern, dict(calls=0, ms=0.0, flops=0.0))
        d["calls"] += 1
        d["ms"] += s.elapsed_time(e)
        d["flops"] += fl
    return agg, rec


def single_scan_latency(args, model, device, n_points, reps=15):
    """BASELINE configs[0]'s shape (ONE scan, the reference's inference_demo.py:41-66): wall time of the whole hot path, host copy of the
    result included, eager (~430 launches from Python).  Same caveat as the pipeline's stage 2: with the bench's random weights the
    marker fit freezes early; add stage2_latency's batch_1 figure for a well-posed fit.  (The same path as ONE HIP graph,
    etch_amd.graph.GraphedHotPath, measures 9.5 ms against 10.2 ms in a fresh process -- profiles/scripts/graph_time3.py; it is not timed here
    because a process that already owns the pipeline's streams maps the graph's branches onto shared hardware queues.)"""
    from etch_amd.inference_demo import predict_smpl_batch
    pts = torch.from_numpy(synth_scan(777, n_points)[None]).to(device)
    predict_smpl_batch(args, model, pts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        predict_smpl_batch(args, model, pts)
    torch.cuda.synchronize()
    return {"eager_ms": round((time.perf_counter() - t0) / reps * 1e3, 3), "points": n_points}


def well_posed_markers(args, device, batch, seed=5, noise=0.002):
    """Per-scan WELL-POSED marker targets: the body model at a random pose / shape / translation, its 86 marker vertices + 2 mm noise, all
    valid.  -> (markers (B,M,3), valid_f (B,M) float, valid_b (B,M) bool, generating vertices (B,V,3)) on the device."""
    from etch_amd import ops
    from etch_amd.models.fit_SMPL import _device_body
    bm = args.body_model
    mv = np.array(list(args.markerset.values()))
    db = _device_body(bm, mv, device)
    rng = np.random.default_rng(seed)
    npose, nb = 3 * (bm.num_joints - 1), bm.num_betas
    x = np.concatenate([rng.standard_normal((batch, npose)) * 0.2, rng.standard_normal((batch, nb)) * 0.8, rng.standard_normal((batch, 3)) * 0.2,
                        rng.standard_normal((batch, 3)) * 0.05], 1).astype(np.float32)
    verts, _ = ops.smpl_lbs(db.lbs_consts, torch.from_numpy(x).to(device), db.V, db.n_extra, nj=db.nj, nb=db.nb)
    tgt = verts[:, torch.from_numpy(mv).to(device).long()] + torch.from_numpy(rng.standard_normal((batch, len(mv), 3)).astype(np.float32) * noise).to(device)
    valid = torch.ones((batch, len(mv)), dtype=torch.float32, device=device)
    return tgt.contiguous(), valid, valid.bool(), verts


def graph_latency_child(points, reps=30):
    """Runs in a CHILD process that the parent starts before it touches the GPU (and waits for): the whole hot path of ONE scan with
    well-posed markers, captured as one HIP graph and replayed -- no eager multi-stream pipeline in the same process sharing the hardware
    queues.  Prints one JSON line."""
    from etch_amd.graph import GraphedHotPath
    from etch_amd.inference_demo import predict_smpl_batch
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    args, model = build(device)
    mk = well_posed_markers(args, device, 1)[:3]
    pts = torch.from_numpy(synth_scan(777, points)[None]).to(device)
    out = {"points": points, "markers": "86 valid, body model at a random pose + 2 mm noise (fit runs its full 30+50 schedule)"}
    for name, kw in (("well_posed", dict(markers_override=mk)), ("network_markers", {})):
        for _ in range(3):
            predict_smpl_batch(args, model, pts, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            predict_smpl_batch(args, model, pts, **kw)
        torch.cuda.synchronize()
        out[f"eager_ms_{name}"] = round((time.perf_counter() - t0) / reps * 1e3, 3)
    g = GraphedHotPath(args, model, 1, points, markers_override=mk)
    for _ in range(3):
        g(pts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        g(pts)                                   # host copy of the mesh included
    torch.cuda.synchronize()
    out["graph_ms_well_posed"] = round((time.perf_counter() - t0) / reps * 1e3, 3)
    print(json.dumps(out), flush=True)


def stage2_latency(args, device, iters, batch):
    """The LM fit kernel alone on WELL-POSED markers (all 86 valid, 2 mm noise, drawn from the body model at a random pose): with the
    bench's seeded random network weights most labels never win the argmax, a scan keeps ~2 valid markers and its fit freezes early
    (per-sample convergence test of the reference's LM), so the pipeline's own stage-2 time understates a trained network's.  Reported:
    the full schedule at the bench batch and at batch 1 (latency of a single-scan caller)."""
    from etch_amd import ops
    from etch_amd.models.fit_SMPL import _device_body
    bm = args.body_model
    mv = np.array(list(args.markerset.values()))
    db = _device_body(bm, mv, device)
    rng = np.random.default_rng(5)
    npose, nb = 3 * (bm.num_joints - 1), bm.num_betas
    out = {}
    for bsz in (batch, 1):
        x = np.concatenate([rng.standard_normal((bsz, npose)) * 0.2, rng.standard_normal((bsz, nb)) * 0.8, rng.standard_normal((bsz, 3)) * 0.2,
                            rng.standard_normal((bsz, 3)) * 0.05], 1).astype(np.float32)
        verts, _ = ops.smpl_lbs(db.lbs_consts, torch.from_numpy(x).to(device), db.V, db.n_extra, nj=db.nj, nb=db.nb)
        tgt = verts[:, torch.from_numpy(mv).to(device).long()] + torch.from_numpy(rng.standard_normal((bsz, len(mv), 3)).astype(np.float32) * 0.002).to(device)
        valid = torch.ones((bsz, len(mv)), dtype=torch.float32, device=device)
        def timed(split):
            best, tr = None, None
            for _ in range(3):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                _, _, tr = ops.smpl_lm_fit(db.lm_consts, tgt.contiguous(), valid, iters[0], 0.5, 0.01, iters[1], 0.2, 1e-3, True, nj=db.nj, nb=db.nb,
                                           split=split)
                e.record()
                torch.cuda.synchronize()
                best = s.elapsed_time(e) if best is None else min(best, s.elapsed_time(e))
            return best, tr
        best, tr = timed(None)                     # the default: split over LM_SPLIT_WGS workgroups per scan for small batches
        frozen = float((tr[:, 1:] == tr[:, :-1]).sum(1).float().mean())
        out[f"batch_{bsz}"] = {"ms": round(best, 3), "us_per_iteration": round(best * 1e3 / (iters[0] + iters[1] + 2), 1),
                               "iterations_skipped_by_the_convergence_freeze": frozen,
                               "workgroups_per_scan": ops.lm_split_default(bsz, db.nj)}
        if bsz <= ops.LM_SPLIT_MAX_BATCH:
            one, _ = timed(1)
            out[f"batch_{bsz}"]["ms_one_workgroup_per_scan"] = round(one, 3)
    out["schedule"] = f"{iters[0]}+{iters[1]} iterations, 86 valid markers with 2 mm noise"
    return out


# ------------------------------------------------------------------------------------------------ CPU baseline
def cpu_baseline(n_points, gpu_pts, gpu_results, gpu_fit_aux, args, seed=1, threads=None, forward_only=False, iters=(30, 50), refit=None):
    """The oracle (CPU restatement = "port") timed on this box's host cores on ONE scan of the same workload:
    full stage 1 and the full 30 + 50 iteration LM fit.  Also returns parity numbers for that scan.  `threads`: torch CPU
    threads (default 32 or the core count if smaller: on the 128-thread GPU box the oracle's small-matrix stages run SLOWER
    with every hardware thread than with 32, profiles/r02_cpu_baseline_threads.txt)."""
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import seeded_state_dict
    from oracle import stage1 as S1
    from oracle import stage2 as S2

    cores = threads or min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    cargs = types.SimpleNamespace(**{**vars(args), "device": torch.device("cpu")})
    sd = seeded_state_dict(GT_network_equiv(option=cargs), seed)
    table = S1.build_layer_table()
    x = gpu_pts[:1].cpu()
    t0 = time.time()
    out = S1.forward(sd, x, table, num_markers=len(args.markerset))
    t1 = time.time() - t0
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
    parity = {k: rel(gpu_results[k][:1].cpu(), out[k]) for k in ("part_labels", "confidences", "magnitude")}
    labels = out["part_labels"].argmax(-1)
    parity["label_agreement"] = float((gpu_results["part_labels"][:1].cpu().argmax(-1) == labels).float().mean())
    if forward_only:
        return dict(value=1.0 / t1, unit="scans/s", cores=cores, kind="port",
                    sample=f"1 scan x {n_points} pts: oracle stage 1 ({t1:.1f} s), torch CPU fp32, {cores} threads"), parity
    inner = x - out["direction"] * out["magnitude"] / args.scale_magnitude
    mv = np.array(list(args.markerset.values()))
    # bounded sample: the autograd LM differentiates the full mesh (~0.15 s / iteration for SMPL, ~1 s for the SMPL-X-sized model), so
    # long schedules are timed on a prefix of both stages and scaled to the full iteration count
    full = iters[0] + iters[1]
    run = iters if full <= 80 else (4, 6)
    t0 = time.time()
    mk, valid = S2.get_markers(len(args.markerset), inner, labels, out["confidences"])
    fit = S2.fit_smpl(args.body_model, mv, mk, valid, steps_stage0=run[0], steps_stage1=run[1])
    t2 = (time.time() - t0) * full / (run[0] + run[1])
    # fitter-only parity: the oracle LM on the GPU's own markers of scan 0 (same, possibly shortened, schedule on both sides)
    gm, gv = gpu_fit_aux["markers"][:1].cpu(), gpu_fit_aux["valid"][:1].cpu()
    fit_g = S2.fit_smpl(args.body_model, mv, gm, gv, steps_stage0=run[0], steps_stage1=run[1])
    if run != tuple(iters):
        gpu_fit_aux = refit(run)
    v2v = (gpu_fit_aux["verts"][:1].cpu() - fit_g["verts"]).norm(dim=-1).mean()
    parity["v2v_mm_gpu_vs_oracle_same_markers"] = float(v2v * 1e3)
    # pose / shape deltas vs the CPU oracle on identical inputs = the two fits of the same markers.  (A whole-pipeline
    # marker comparison is ill-posed with seeded random weights: the confidences of a label's points are tied to ~1e-6, so the
    # top-3 selection of fit_SMPL.py:42-57 differs between any two fp32 implementations; the stage-1 outputs themselves agree
    # to ~1e-6, see the entries above.)
    gx = gpu_fit_aux["x"][:1].cpu()
    npose, nbt = fit_g["pose"].shape[1], fit_g["betas"].shape[1]
    parity["pose_delta_rad_same_markers"] = float((gx[:, :npose] - fit_g["pose"]).abs().max())
    parity["betas_delta_same_markers"] = float((gx[:, npose:npose + nbt] - fit_g["betas"]).abs().max())
    how = f"full {iters[0]}+{iters[1]}-iteration" if run == tuple(iters) else f"{run[0]}+{run[1]} of {iters[0]}+{iters[1]} iterations timed, scaled to the full schedule:"
    return dict(value=1.0 / (t1 + t2), unit="scans/s", cores=cores, kind="port",
                sample=f"1 scan x {n_points} pts: oracle stage 1 ({t1:.1f} s) + get_markers + {how} autograd LM fit ({t2:.1f} s), torch CPU fp32, {cores} threads"), parity


# ------------------------------------------------------------------------------------------------ launcher
def train_bench(a):
    """`bench.py --train`: what train.py:77-124 times per iteration -- forward of GT_network_equiv in train() mode (the differentiable path: hand-written
    backward kernels behind torch.autograd, train-mode BatchNorm), the four losses of train.py:81-101, backward, one torch.optim.Adam step (lr 1e-4,
    train.py:219) -- on synthetic scans at train.py's batch shape (batch_size x num_point, defaults 1 x 5000; --batch / --points override); with --full
    also one step with its phases bracketed and the oracle's CPU autograd step (oracle/train_step.py, ONE step, bounded).  SURVEY 8 f-3.  Prints one JSON
    line (not the driver's metric)."""
    import types
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded, seeded_state_dict
    device = torch.device("cuda:0")
    B, N, depth = a.batch or 1, a.points or 5000, a.train_depth
    args = types.SimpleNamespace(output_folder="/tmp/etch_bench_train", EPN_input_radius=0.4, EPN_layer_num=depth, device=device, markerset=K.default_markerset(),
                                 scale_magnitude=10)
    model = load_seeded(GT_network_equiv(option=args), 1).to(device).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    rng = np.random.default_rng(11)
    pts_np = np.stack([synth_scan(b, N) for b in range(B)])
    vec_np = (rng.standard_normal((B, N, 3)) * 0.05).astype(np.float32)
    conf_np = rng.uniform(0.0, 1.0, (B, N, 1)).astype(np.float32)
    lab_np = rng.integers(0, len(args.markerset), (B, N))
    pts, vec, conf, labels = (torch.from_numpy(x).to(device) for x in (pts_np, vec_np, conf_np, lab_np))
    items = ["confidence", "direction", "magnitude"]

    def step():
        res, _ = model(pts, items, "standard_vector")
        cos = 1 - torch.nn.functional.cosine_similarity(vec, res["direction"], dim=-1)
        loss = (cos.mean() + torch.nn.functional.mse_loss(torch.norm(vec, dim=-1, keepdim=True) * 10, res["magnitude"])
                + torch.nn.functional.mse_loss(res["confidences"], conf)
                + torch.nn.functional.cross_entropy(res["part_labels"].permute(0, 2, 1).contiguous(), labels))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(device)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if a.dump_outputs:
            dump_outputs(host_arrays(loss), a.dump_outputs)
        if a.full:
            # the same step with the phases bracketed (one extra, untimed in `value`)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            res, _ = model(pts, items, "standard_vector")
            l2 = ((1 - torch.nn.functional.cosine_similarity(vec, res["direction"], dim=-1)).mean()
                  + torch.nn.functional.mse_loss(torch.norm(vec, dim=-1, keepdim=True) * 10, res["magnitude"])
                  + torch.nn.functional.mse_loss(res["confidences"], conf) + torch.nn.functional.cross_entropy(res["part_labels"].permute(0, 2, 1).contiguous(), labels))
            ev[1].record()
            opt.zero_grad()
            l2.backward()
            ev[2].record()
            opt.step()
            ev[3].record()
            torch.cuda.synchronize()
    ms = dt / a.steps * 1e3
    out = {"metric": "training steps/s (train.py:77-124: forward in train() mode + 4 losses + backward + Adam)", "value": round(a.steps / dt, 3), "unit": "steps/s",
           "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"train.py batch shape: batch_size {B} x num_point {N}, EPN_layer_num {depth}, seeded random weights, Adam lr 1e-4, all four losses",
                      "path": "etch_amd.autograd / autograd_pt (un-fused differentiable kernels, train-mode BatchNorm on batch statistics)"},
           "scans_per_s": round(B * a.steps / dt, 3), "final_loss": round(float(loss.detach()), 6),
           "peak_hbm_gib": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2), "vs_baseline": None}
    if a.full:
        out["phase_ms"] = {"forward + losses": round(ev[0].elapsed_time(ev[1]), 2), "backward": round(ev[1].elapsed_time(ev[2]), 2),
                           "adam": round(ev[2].elapsed_time(ev[3]), 2)}
    if a.full and not a.no_cpu_baseline:
        from oracle import train_step as OT
        threads = a.cpu_threads or min(32, os.cpu_count() or 1)
        torch.set_num_threads(threads)
        sd = {k: v.cpu() for k, v in seeded_state_dict(model, 1).items()}
        names = [k for k, _ in model.named_parameters()]
        nb = 1                                               # bounded sample: ONE scan of the batch, one step
        parts, tf, tb, ta = OT.train_step(sd, names, torch.from_numpy(pts_np[:nb]), torch.from_numpy(vec_np[:nb]), torch.from_numpy(conf_np[:nb]),
                                          torch.from_numpy(lab_np[:nb]), depth=depth)
        out["cpu_baseline"] = {"value": round(1.0 / (tf + tb + ta), 4), "unit": "steps/s", "cores": threads, "kind": "port",
                               "sample": f"1 step of 1 x {N} points: oracle forward {tf:.1f} s + torch.autograd backward {tb:.1f} s + Adam {ta:.2f} s, torch CPU fp32"}
    print(json.dumps(out), flush=True)


DUMP_BUDGET_BYTES = 60 * 2 ** 20       # "at most 64 MB": 62.9 MB of data leaves room for the .npy headers


def host_arrays(result):
    """What a caller of the timed path receives from one step, as named float32 / float64 host arrays:
    the pipeline's / predict_smpl_batch's (meshes, markers, valid, smpl_info) tuple, the model's result dict (--forward-only), a loss tensor (--train)."""
    def host(v):
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        return v.astype(np.float64 if v.dtype == np.float64 else np.float32)

    if isinstance(result, dict):
        return {k: host(v) for k, v in sorted(result.items()) if isinstance(v, (torch.Tensor, np.ndarray))}
    if isinstance(result, tuple):
        meshes, markers, valid, info = result[:4]
        out = {"vertices": host(np.stack([m.vertices for m in meshes])), "markers": host(markers), "valid": host(valid)}
        out.update(zip(("pose", "betas", "global_orient", "transl", "joints"), (host(x) for x in info)))
        return out
    return {"output": host(result)}


def dump_outputs(arrays, out_dir, budget=DUMP_BUDGET_BYTES):
    """Write DIR/<name>.npy.  Past `budget` bytes in all, the arrays with a per-point axis (axis 1 of the largest extent) keep a fixed, seeded sample of
    the points (the same for every run and every build: rng(0)); its indices are written as sample_point_index.npy."""
    total = sum(v.nbytes for v in arrays.values())
    if total > budget:
        n = max(v.shape[1] for v in arrays.values() if v.ndim >= 2)
        per_point = {k for k, v in arrays.items() if v.ndim >= 2 and v.shape[1] == n}
        rest = sum(v.nbytes for k, v in arrays.items() if k not in per_point) + 8 * n
        keep = int(n * (budget - rest) / sum(arrays[k].nbytes for k in per_point))
        idx = np.sort(np.random.default_rng(0).choice(n, max(1, keep), replace=False))
        arrays = {k: (np.ascontiguousarray(v[:, idx]) if k in per_point else v) for k, v in arrays.items()}
        arrays["sample_point_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    print(f"bench.py: wrote {len(arrays)} arrays ({sum(v.nbytes for v in arrays.values()) / 2 ** 20:.1f} MiB) of the last timed step to {out_dir}",
          file=sys.stderr)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script as child processes and relay rank 0's output.
    The parent must not (and does not) initialise the GPU; nothing is exec'ed.  Returns the exit code."""
    import subprocess
    import tempfile
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    with tempfile.TemporaryFile("w+") as out0:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL, stderr=None))
        bad = []
        while any(p.poll() is None for p in procs):
            bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
            if bad:                                  # a rank died: its peers would wait in the next barrier for ever -> stop them (own children, by PID)
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                for p in procs:
                    try:
                        p.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        p.kill()
                break
            time.sleep(0.05)
        bad = bad or [(r, p.returncode) for r, p in enumerate(procs) if p.returncode != 0]
        out0.seek(0)
        sys.stdout.write(out0.read())
        sys.stdout.flush()
    if bad:
        print(f"bench.py: ranks failed (rank, rc): {bad}", file=sys.stderr)
        return bad[0][1] if bad[0][1] and bad[0][1] > 0 else 1
    return 0


def preflight(a):
    """`bench.py --gpus N --preflight`: one JSON line describing the N-rank job (no GPU call, no process group, no child process)."""
    from etch_amd import parallel as P
    cfg = {"batch": 8, "points": 20000} if a.config == 4 else {"batch": 32, "points": 5000}
    B, N, world = a.batch or cfg["batch"], a.points or cfg["points"], a.gpus
    ranks = []
    for r in range(world):
        s0, s1 = P.shard_range(B * world, r, world)
        try:
            cpus = sorted(P.local_cpu_set(r, world)) if world > 1 and not a.no_pin else None
            cpu_note = None
        except Exception as e:                       # unreadable topology: the run itself would go on unpinned and say so
            cpus, cpu_note = None, f"{type(e).__name__}: {e}"
        ranks.append({"rank": r, "local_rank": r, "device": f"cuda:{r}", "scans": [s0, s1], "scan_seeds": [1000 + s0, 1000 + s1 - 1],
                      "cpu_set": None if cpus is None else f"{len(cpus)} cpus: {cpus[0]}..{cpus[-1]}", "cpu_pinning_error": cpu_note})
    env_keys = ("HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG", "NCCL_SOCKET_IFNAME", "NCCL_IB_DISABLE", "RCCL_MSCCL_ENABLE", "HIP_VISIBLE_DEVICES",
                "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_MAX_HW_QUEUES", "MASTER_ADDR", "MASTER_PORT", "WORLD_SIZE", "RANK", "LOCAL_RANK",
                "ETCH_DIST_BACKEND", "ETCH_FORCE_DIST")
    out = {"preflight": True, "n_gpus": world, "config": a.config, "scans_per_gpu": B, "points": N, "global_batch": B * world, "scaling": "weak",
           "launcher": "torchrun/env" if "TORCHELASTIC_RUN_ID" in os.environ else ("self: bench.py starts its own ranks" if world > 1 else "single process"),
           "rendezvous": {"addr": os.environ.get("MASTER_ADDR", "127.0.0.1"), "port": os.environ.get("MASTER_PORT", "chosen at launch")},
           "collective": {"backend": os.environ.get("ETCH_DIST_BACKEND", "nccl (= RCCL)") if world > 1 else None,
                          "calls": "1 barrier + 1 all_reduce(MAX) of the timing + 1 all_gather of 7 floats per scan at the end of the job; none on the data path"},
           "child_env_overrides": {"HSA_ENABLE_IPC_MODE_LEGACY": "0", "MASTER_ADDR": "127.0.0.1"} if world > 1 and "RANK" not in os.environ else {},
           "env": {k: os.environ[k] for k in env_keys if k in os.environ},
           "host": {"cpus_online": os.cpu_count(), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None), "gpus_visible": torch.cuda.device_count()},
           "ranks": ranks}
    print(json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=2, choices=[1, 2, 4], help="BASELINE.json configs[k]: 2 (default, the configuration the metric is "
                    "quoted on) = 32 x 5000 pts per GPU, forward + 30+50-iteration SMPL fit; 1 = the same batch, equivariant forward only; "
                    "4 = the per-GPU shard of the 64 x 20000-pt stress config: 8 dense scans per GPU + 200-iteration (75+125) fit of the "
                    "SMPL-X-sized 188-DoF body model")
    ap.add_argument("--batch", type=int, default=0, help="scans per GPU (default: the config's)")
    ap.add_argument("--points", type=int, default=0, help="points per scan (default: the config's)")
    ap.add_argument("--forward-only", action="store_true", help="BASELINE.json configs[1]: a step is the equivariant forward only")
    ap.add_argument("--same-batch", action="store_true", help="feed the same resident batch every step (default: a distinct batch per step)")
    ap.add_argument("--full", action="store_true", help="also run every leg beside the headline figure: single-scan latency, synchronous schedule, "
                    "well-posed markers, roofline pass, stage-2 latency, CPU baseline (default: set up, warm up, time the steps, print the line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the well-posed / stage2_latency / single_scan_latency legs (profiling "
                    "runs: their launches of other batch sizes would mix into the per-kernel averages of the trace)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="torch CPU threads of the cpu_baseline leg (0: min(32, cores))")
    ap.add_argument("--no-pin", action="store_true", help="do not pin ranks to the cores of their GPU's NUMA node (N > 1 only)")
    ap.add_argument("--sync", action="store_true", help="synchronous steps (stage 2 of a batch finishes before stage 1 of the next starts). Default: the "
                    "stream pipeline of etch_amd.pipeline (3 batches in flight) -- stage 2 of step i (32 persistent workgroups, 1/8 of the chip) runs on a second "
                    "HIP stream next to stage 1 of step i+1; every one of the K steps still completes inside the timed region")
    ap.add_argument("--schedule", default="eager", choices=["eager", "graph"], help="how a pipelined step reaches the GPU: eager (default: five streams, the launches "
                    "come from Python) or graph (A/B: one HIP-graph replay per batch slot -- immune to a busy host, but 25 %% slower on a quiet one: "
                    "profiles/r06_schedule_ab.txt)")
    ap.add_argument("--serial", action="store_true", help="profiling schedule: synchronous steps and every kernel on one stream")
    ap.add_argument("--unfused-interp", action="store_true", help="A/B: separate 3-NN interpolation kernel in front of the direction head")
    ap.add_argument("--stage1-streams", type=int, default=1, help="stage-1 streams the pipeline alternates over (batches in flight = this + 2; ETCH_MAX_IN_FLIGHT overrides)")
    ap.add_argument("--concurrent-heads", type=int, default=1, help="1: confidence / magnitude nets on their own streams next to the direction head")
    ap.add_argument("--train", action="store_true", help="time one training step (forward in train() mode + the four losses + backward + Adam, train.py:77-124) instead "
                    "of the inference metric; --batch / --points = train.py's batch_size / num_point (defaults 1 x 5000)")
    ap.add_argument("--train-depth", type=int, default=2, choices=[1, 2, 3, 4], help="EPN_layer_num of the --train model")
    ap.add_argument("--graph-latency-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--preflight", action="store_true", help="print, WITHOUT touching a GPU, what each of the --gpus N ranks would do: its shard of the "
                    "global batch, the CPU set it would pin itself to, the rendezvous and the RCCL-relevant environment -- so that a failed scaling run "
                    "can be diagnosed from its log")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed path computed in its last step (the "
                    "arrays its caller receives) as DIR/<name>.npy, float32 / float64, at most 64 MB in all (rank 0); the inputs depend on the arguments only")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    # The GPU phases need ONE host thread; torch's CPU pool (128 threads on the pool's hosts) spinning beside it exhausts the container's CPU quota and freezes
    # the enqueueing thread for up to 100 ms at a time (etch_amd/pipeline.py limit_host_threads; profiles/r06_host_throttling.txt).  The cpu_baseline leg sets
    # its own thread count when it runs, after the timed region.
    from etch_amd.pipeline import limit_host_threads
    limit_host_threads()
    # batches in flight: with 2 the host submits batch i+1 only after batch i-1 has finished stage 2 -- whose start waits for that batch's Point-Transformer
    # nets, which trail into the next batch's encoder -- so that every other step's index ops were enqueued late and its first conv idled 3.5 ms on them
    # (profiles/r04_stream_timeline.txt); with 3 the step boundary is a steady 0.3 ms
    in_flight = int(os.environ.get("ETCH_MAX_IN_FLIGHT", a.stage1_streams + 2))
    if a.graph_latency_child:
        graph_latency_child(a.points or 5000)
        return
    if a.preflight:
        preflight(a)
        return
    if a.train:
        train_bench(a)
        return
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(launch_ranks(a.gpus, sys.argv[1:]))          # parent: no GPU call before or after this point
    if a.serial:
        a.sync, a.concurrent_heads = True, 0
    if a.config == 1:
        a.forward_only = True
    cfg = {"body": "smplx", "iters": (75, 125), "batch": 8, "points": 20000} if a.config == 4 else {"body": "smpl", "iters": (30, 50), "batch": 32, "points": 5000}
    a.batch, a.points = a.batch or cfg["batch"], a.points or cfg["points"]
    a.pipeline = not a.sync and not a.forward_only

    from etch_amd import parallel as P

    rank, world, local = P.env_rank_world()
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    pinned = None
    if world > 1 and not a.no_pin:
        try:
            pinned = P.pin_to_local_cores(local, world)         # before the GPU runtime starts its helper threads
        except Exception as e:                                  # an unreadable / unexpected topology must not stop the job
            print(f"[bench] rank {rank}: CPU pinning skipped ({type(e).__name__}: {e})", file=sys.stderr)
    latency_child = None
    if a.full and world == 1 and a.config == 2 and not a.forward_only and not a.no_extras and not os.environ.get("ETCH_BENCH_DRY"):
        # single-scan latency as ONE HIP graph, measured in a child process that owns the GPU alone: started (and finished) BEFORE this
        # process makes its first GPU call, so neither side shares hardware queues with the other
        import subprocess
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--graph-latency-child", "--points", str(a.points or 5000)],
                               capture_output=True, text=True, timeout=900)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            latency_child = json.loads(lines[-1]) if r.returncode == 0 and lines else {"error": (r.stderr or "no output")[-400:]}
        except (subprocess.TimeoutExpired, OSError, ValueError) as e:     # a hung or unstartable child must not abort the bench: the error is reported
            latency_child = {"error": f"{type(e).__name__}: {str(e)[-300:]}"}
    dry = bool(os.environ.get("ETCH_BENCH_DRY"))                # control-flow test of the N > 1 path without a GPU (tests/test_parallel_gloo.py)
    if dry and os.environ.get("ETCH_BENCH_DRY_FAIL_RANK") == str(rank):
        sys.exit(3)                                             # failure injection for the launcher test
    P.init("gloo" if dry else None)
    if dry:
        device = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("bench.py needs an MI355X: the product path has no CPU fallback")
        if os.environ.get("ETCH_ALL_RANKS_DEVICE0"):      # smoke of the multi-rank control flow on a 1-GPU box (with ETCH_DIST_BACKEND=gloo)
            local = 0
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    sync = (lambda: None) if dry else torch.cuda.synchronize
    B, N = a.batch, a.points
    s0, _ = P.shard_range(B * world, rank, world)
    # a distinct batch per timed step, all resident before the timed region: step k of rank r reads scans
    # 1000 + k * (B * world) + [s0, s0 + B)  (k = 0 is the batch of the warm-up, the roofline pass and parity_scan0)
    nbatch = 1 if a.same_batch else a.steps + 1
    batches = [torch.from_numpy(np.stack([synth_scan(k * B * world + s0 + i, N) for i in range(B)])).to(device) for k in range(nbatch)]
    pts = batches[0]
    timed = [batches[(k + 1) % nbatch] for k in range(a.steps)]
    last = {}
    final = {}                  # what the caller of the timed path received from its latest step (--dump-outputs)
    sched_report = {"schedule": "none"}
    if dry:
        def step(p=pts):
            time.sleep(0.002)
            last.update(err=p[:, :, 0].mean(1).abs(), valid=torch.ones(B, 86, dtype=torch.bool), x=p[:, :85, 0].contiguous(),
                        status=torch.zeros(B, dtype=torch.int32), frozen=torch.zeros(B, dtype=torch.int64))
            final["result"] = dict(last)

        def run_steps(bs):
            for p in bs:
                step(p)
    else:
        from etch_amd.inference_demo import predict_smpl_batch
        from etch_amd.pipeline import HotPathPipeline
        args, model = build(device, body=cfg["body"])
        fit_kw = dict(steps_stage0=cfg["iters"][0], steps_stage1=cfg["iters"][1])
        model.concurrent_heads = bool(a.concurrent_heads)
        if a.serial:
            model.overlap_index_ops = False
        model_results = {}

        def stage1_only(p=pts):
            with torch.no_grad():
                r, _ = model(p, ["confidence", "direction", "magnitude"], "standard_vector")
            model_results.update(r)
            final["result"] = r

        def full_step(p=pts):
            meshes, markers, valid, info, aux = predict_smpl_batch(args, model, p, "neutral", return_trace=True, **fit_kw)
            tr = aux["err_trace"]
            final["result"] = (meshes, markers, valid, info)
            last.update(markers=markers, valid=valid, verts=aux["verts"], x=aux["x"], err=tr[:, -1], status=aux["status"],
                        frozen=(tr[:, 1:] == tr[:, :-1]).sum(1))

        step = stage1_only if a.forward_only else full_step
        from etch_amd.pipeline import choose_pipeline
        pipe = None
        if a.pipeline:
            for _ in range(max(1, a.warmup)):      # the model's caches (folded weights, fragments, device body tables) fill before anything is captured / timed
                (stage1_only if a.forward_only else full_step)()
            pipe, sched_report = choose_pipeline(args, model, pts, "neutral", max_in_flight=in_flight, schedule="eager" if a.forward_only else a.schedule,
                                                 stage1_streams=a.stage1_streams, want_trace=True, log=lambda m: print(m, file=sys.stderr), **fit_kw)

        def run_steps(bs):
            """One step per batch of `bs`; with the pipeline, stage 2 of step i overlaps stage 1 of step i+1 (all finish inside the call)."""
            if not a.pipeline:
                for p in bs:
                    step(p)
                return
            for res in pipe.run(iter(bs)):
                final["result"] = res

    for _ in range(a.warmup):
        step()
    run_steps([pts] * min(2, a.warmup))
    P.barrier()
    sync()
    import gc
    if os.environ.get("ETCH_BENCH_GC", "1") == "0":
        gc.collect(); gc.disable()
    seg0 = torch.cuda.memory_stats().get("segment.all.allocated", 0) if device.type == "cuda" else 0
    gc0 = [g["collections"] for g in gc.get_stats()]
    t0 = time.perf_counter()
    run_steps(timed)
    sync()
    P.barrier()
    dt = P.max_over_ranks(time.perf_counter() - t0, device)
    if a.dump_outputs and rank == 0:
        dump_outputs(host_arrays(final["result"]), a.dump_outputs)
    if os.environ.get("ETCH_PIPE_TIMING") == "1" and device.type == "cuda":
        print("timed region: allocator segments allocated %d, gc collections per generation %s" % (
            torch.cuda.memory_stats().get("segment.all.allocated", 0) - seg0, [g["collections"] - c for g, c in zip(gc.get_stats(), gc0)]), file=sys.stderr)
    gc.enable()
    if a.pipeline and not dry and getattr(pipe, "host_times", None) and hasattr(pipe, "gap_report"):
        gr = pipe.gap_report(last=a.steps)
        if gr:
            f = lambda v: " ".join("%.2f" % x for x in v)
            print("stage-1 stream timeline of the timed steps (HIP events, no tracer; ms):\n  stage-1 span per batch  %s\n  idle gap to the next batch's stage 1  %s\n"
                  "  batch done behind its stage 1  %s\n  period (stage-1 end to stage-1 end)  %s\n  medians: span %.2f  gap %.2f  period %.2f" %
                  (f(gr["stage1_span_ms"]), f(gr["stage1_gap_ms"]), f(gr["stage2_lag_ms"]), f(gr["period_ms"]), float(np.median(gr["stage1_span_ms"])),
                   float(np.median(gr["stage1_gap_ms"])), float(np.median(gr["period_ms"]))), file=sys.stderr)
    if a.pipeline and not dry and getattr(pipe, "host_times", None):
        ht = np.array(pipe.host_times[-a.steps:])
        print("host ms per submit (wait for the oldest ticket / finalize it / enqueue the batch): median %s, max %s; enqueue ms per step: %s"
              % (np.round(np.median(ht, 0), 2), np.round(ht.max(0), 2), " ".join("%.0f" % v for v in ht[:, 2])), file=sys.stderr)
    # --full: the first (up to 5) of the K steps without the cross-step overlap (untimed in `value`; reported next to the headline for transparency)
    sync()
    ts = time.perf_counter()
    unpipelined = timed[:5] if a.full else []
    for p in unpipelined:
        step(p)
    step(pts)           # batch 0 last: it provides the per-scan result rows for the end-of-job gather and parity_scan0
    sync()
    sync_ms = (time.perf_counter() - ts) / (len(unpipelined) + 1) * 1e3

    # second, labelled leg (--full): the same K steps with the pipeline's stage 2 consuming WELL-POSED per-scan markers (stage 1 unchanged; get_markers
    # still runs on the network's output): with the bench's seeded random weights the network's own markers leave ~2 of 86 valid and the
    # fit freezes early, so this is the figure a trained network's markers would give
    wp = None
    if a.full and not dry and not a.forward_only and not a.no_extras:
        mk_wp = well_posed_markers(args, device, B)
        pipe_wp, _ = choose_pipeline(args, model, pts, "neutral", max_in_flight=in_flight, schedule=sched_report["schedule"] if a.pipeline else "eager",
                                     stage1_streams=a.stage1_streams, want_trace=True, markers_override=mk_wp[:3], **fit_kw)
        for r_ in pipe_wp.run(iter([pts] * 2)):
            pass
        P.barrier()
        sync()
        t1 = time.perf_counter()
        last_wp = None
        for r_ in pipe_wp.run(iter(timed)):
            last_wp = r_
        sync()
        P.barrier()
        dt_wp = P.max_over_ranks(time.perf_counter() - t1, device)
        wp = {"value": round(world * B * a.steps / dt_wp, 3), "unit": "scans/s", "ms_per_step": round(dt_wp / a.steps * 1e3, 3),
              "markers": "86 valid per scan: body model at a random pose + 2 mm noise; full 30+50 (75+125) LM schedule runs"}
        gen = mk_wp[3]
        fitted = torch.from_numpy(np.stack([m.vertices for m in last_wp[0]])).to(device)
        wp["v2v_mm_fit_vs_generating_body_mean"] = round(float((fitted - gen).norm(dim=-1).mean() * 1e3), 4)
        wp["_last"] = (mk_wp, fitted)

    # end-of-batch metric reduction (north_star: the only collective): ONE all_gather of per-scan result rows
    #   [final LM error 0.5*|r|^2, #valid markers, RMS marker residual (mm), |pose| (rad), |betas|]
    if a.forward_only and not dry:
        conf = model_results["confidences"][..., 0]
        rows = torch.stack([conf.mean(1), conf.amax(1), model_results["magnitude"][..., 0].mean(1)], 1)
        row_names = ["mean confidence", "max confidence", "mean magnitude"]
    else:
        nv = last["valid"].float().sum(1)
        npose = last["x"].shape[1] - (26 if a.config == 4 else 16)
        rows = torch.stack([last["err"], nv, (2.0 * last["err"] / nv.clamp_min(1)).sqrt() * 1e3, last["x"][:, :npose].norm(dim=1),
                            last["x"][:, npose:-6].norm(dim=1), last["status"].float(), last["frozen"].float()], 1)
        row_names = ["final LM error", "valid markers", "rms marker residual mm", "pose norm rad", "betas norm", "status word",
                     "LM iterations skipped after the convergence freeze"]
    allrows = P.gather_rows(rows)

    if rank != 0:
        return
    value = world * B * a.steps / dt
    finite = torch.isfinite(allrows).all(1)
    cfg_name = (f"configs[1]: batch={B}/GPU synthetic {N}-pt Gaussian-blob scans, equivariant forward only (encoder + confidence / direction / "
                "magnitude heads), seeded random weights" if a.forward_only else
                f"configs[4] per-GPU shard: batch={B}/GPU dense synthetic {N}-pt scans, full pipeline (eq-net + 75+125-iter LM fit of the SMPL-X-sized "
                "188-DoF body: 55 joints, 20 shape+expression coefficients, 10475 vertices), seeded random weights, 86 markers" if a.config == 4 else
                f"configs[2]: batch={B}/GPU synthetic {N}-pt Gaussian-blob scans, full pipeline (eq-net + 30+50-iter LM SMPL fit), "
                "seeded random weights, seeded SMPL-shaped body model, 86-marker superset")
    sched = ("serial: synchronous steps, one stream" if a.serial else "synchronous steps") if not a.pipeline else \
        (f"stream pipeline, {in_flight} batches in flight: stage 2 of step i overlaps stage 1 of step i+1, the host enqueues two steps ahead"
         if sched_report.get("schedule") != "graph" else
         f"graph-replay pipeline, {in_flight} batches in flight: every batch's device work (stage 1, glue, marker fit, LBS: one stream) is one HIP graph per "
         "slot, replayed with one host call; stage 2 of step i overlaps stage 1 of step i+1") + \
        (f"; --schedule {a.schedule}" if a.schedule != "eager" else "")
    metric = "scans/s (5k pts, eq-net forward only)" if a.forward_only else "scans/s (5k pts, eq-net + 50-iter SMPL fit)"
    if a.config == 4:
        metric = "scans/s (20k pts, eq-net + 200-iter SMPL-X-sized fit)"
    out = {"metric": metric,
           "value": round(value, 3), "unit": "scans/s", "n_gpus": world,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32 (matrix operands: 2 x fp16 planes per fp32 value, fp32 accumulate)", "data": "synthetic",
           "config": {"workload": cfg_name, "schedule": sched, "global_batch": B * world, "points": N, "parallelism": f"scan-sharded x{world}",
                      "distinct_batches": nbatch, "launcher": "torchrun/env" if "TORCHELASTIC_RUN_ID" in os.environ else ("self" if world > 1 else "single"),
                      "cpu_pinning": None if pinned is None else f"rank 0 on {len(pinned)} NUMA-local cores",
                      # the box's 1-minute load average and hardware threads when the line was written: the host enqueues ~300 launches per step (8.5 ms of
                      # Python undisturbed); on a box whose cores are busy with other tenants that becomes the bound
                      "host_load": {"loadavg_1m": round(os.getloadavg()[0], 1), "hardware_threads": os.cpu_count()},
                      "collective_backend": (torch.distributed.get_backend() + (" (forced world-size-1 group: ETCH_FORCE_DIST)" if world == 1 else ""))
                      if torch.distributed.is_initialized() else None},
           "gathered_rows": {"columns": row_names, "scans_reported": int(allrows.shape[0]), "finite_scans": int(finite.sum()),
                             "mean": [float(v) for v in allrows[finite].mean(0)] if bool(finite.any()) else None}}
    if a.full:
        out["ms_per_step_synchronous"] = round(sync_ms, 3)
    if dry:
        out["dry_run"] = True
        print(json.dumps(out), flush=True)
        return
    out["peak_hbm_gib"] = round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)
    out["allocator_reserved_gib"] = round(getattr(pipe, "reserved_gib", 0.0), 2)       # free blocks handed to the streams' allocator pools up front (pipeline._reserve_allocator)
    if N == 5000 and not a.forward_only:
        # 152.4 GFLOP matmul / conv + 5.2 GFLOP kernel-weight generation per 5 000-point scan -> 1.0 ms at the fp32-MFMA
        # peak, HBM-side 0.05 ms: ceiling ~ 1 030 scans/s per GPU for the whole path
        # ceiling_mixed (the lead): the products that run as two fp16 planes (everything but the first conv's VALU work and the kernel-weight generation:
        # 140.7 + 11.7 of the 152.4 GFLOP since round 5 moved the attention scores / P V too) at the dense fp16 peak / 3 cross terms, the weight generation
        # (5.2 GFLOP) at the fp32 peak
        t_mixed = 152.4e9 / (F16_MFMA_PEAK_TFLOPS / 3.0 * 1e12) + 5.2e9 / (FP32_MFMA_PEAK_TFLOPS * 1e12)
        out["path_roofline"] = {"ceiling_mixed": round(1.0 / t_mixed), "frac_mixed": round(value / world * t_mixed, 4),
                                "ceiling_scans_per_s_per_gpu_fp32_matrix_peak": 1030, "frac_vs_fp32_matrix_peak": round(value / world / 1030.0, 4),
                                "note": "frac_mixed (lead) = value / ceiling_mixed: 152.4 GFLOP of products per scan at the dense fp16 matrix peak / 3 cross terms (833 TFLOP/s) "
                                        "+ 5.2 GFLOP weight generation at the fp32 peak; the second pair prices everything at the fp32 matrix peak, the unit SURVEY 8d's "
                                        "1 030 scans/s ceiling is written in (the path no longer runs on that pipe)"}
    if not a.full:                      # the legs below run with --full only
        print(json.dumps(out), flush=True)
        return

    # roofline of the dominant kernel: one instrumented pass of the same step (HIP events on the launch stream).
    # the instrumented pass runs the step on ONE stream (no heads / index ops on side streams): with kernels of several
    # streams resident at once a HIP-event bracket measures contention, not the kernel (`bench.py --serial` runs the whole
    # job in that schedule; profiles/*_serial_kernel_stats.txt is its rocprofv3 summary)
    saved = (model.concurrent_heads, model.overlap_index_ops)
    model.concurrent_heads, model.overlap_index_ops = False, False
    with torch.no_grad():
        step()
        torch.cuda.synchronize()
        agg, agg_calls = profile_pass(step)
        model.concurrent_heads, model.overlap_index_ops = saved
        stage1_only()
    tot_ms = sum(d["ms"] for d in agg.values())
    # dominant kernel = the kernel FUNCTION with the largest share of the step (template instantiations of one kernel are
    # one kernel: the three inter_so3conv_kernel<CIN,COUT,MAXT> launches of a step are priced together)
    def family(k):      # the inter conv of a step is ONE kernel family: its 16x16x32 (32 input channels) and 32x32x16 (64 input channels) instantiations are priced together
        return "inter_so3conv_x_kernel" if k.startswith("inter_so3conv_x32_kernel") else k.split("<")[0].split(" (")[0]
    fam = collections.OrderedDict()
    for k, v in agg.items():
        f = fam.setdefault(family(k), dict(calls=0, ms=0.0, flops=0.0, members=[]))
        for key in ("calls", "ms", "flops"):
            f[key] += v[key]
        f["members"].append(k)
    # ... among the chip-wide kernels: the LM fit and FPS run one workgroup per scan (8 - 32 of 256 CUs) and are bound by their
    # dependent iterations, not by a chip-level roofline; when one of them is the longest launch (the 8-scan dense shard of configs[4])
    # it is named in `longest_kernel` and the roofline stays with the widest arithmetic kernel
    longest = max(fam.items(), key=lambda kv: kv[1]["ms"])[0]
    kern, d = max(((k, v) for k, v in fam.items() if v["flops"] > 0), key=lambda kv: kv[1]["ms"])
    achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
    # HBM bytes per launch of that kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
    # runs of this same command, corrected as profiles/pmc_traffic.py documents); counters cannot be read inside this process
    traffic, counter_files = None, {}
    import glob

    def stamp(path):      # which committed file a counter comes from, and whether the kernel source has changed since it was collected
        src = os.path.join(ROOT, "etch_amd", "csrc", SOURCE_OF_KERNEL.get(kern, ""))
        rec = {"file": os.path.basename(path), "file_blob": blob_hash(path)[:12]}
        side = path + ".sources.json"
        if os.path.isfile(src):
            rec["kernel_source"] = os.path.basename(src)
            rec["kernel_source_blob"] = blob_hash(src)[:12]
            then = json.load(open(side)).get(os.path.basename(src)) if os.path.exists(side) else None
            rec["stale"] = then is None or then[:12] != rec["kernel_source_blob"]
        return rec

    for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):     # newest round / pass first
        tab = json.load(open(pmc))
        ents = [v for k, v in tab.items() if family(k.replace(" ", "")) == kern]     # template variants of the kernel: launch-weighted mean
        if ents:
            n = sum(e["launches_profiled"] for e in ents)
            traffic = round(sum(e["bytes_per_launch"] * e["launches_profiled"] for e in ents) / n)
            counter_files["traffic"] = stamp(pmc)
            break
    # algorithmic HBM bytes per launch of the dominant kernel (unique input + output): the gathered rows once (three bf16 planes = 6 bytes per
    # element for the planes kernels, 4 otherwise), the output once; and the matrix-pipe busy share of its instantiations from the newest committed counter pass
    alg_bytes = None
    if kern.startswith("inter_so3conv"):
        tot_b, n_b = 0.0, 0
        for name_, args_, _, _ in agg_calls:
            if name_.startswith("etch_inter_so3conv"):
                v_ = [x.value if hasattr(x, "value") else x for x in args_]
                b_, cin_, cout_, p1_, p2_, nn_ = v_[0:6]
                if cin_ > 1:
                    tot_b += b_ * p1_ * 60.0 * cin_ * (4 if name_.endswith("planes_kq") else 6 if "planes" in name_ else 4) + b_ * p2_ * 60.0 * cout_ * 4 + b_ * p2_ * nn_ * 4.0
                    n_b += 1
        alg_bytes = round(tot_b / n_b) if n_b else None
    pipe_busy = None
    for f_ in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_mfma.txt")), reverse=True):
        got = {}
        for ln in open(f_):
            if "matrix pipe busy" in ln and not ln.startswith("#"):
                nm = ln.split(" launches")[0].replace("void ", "").strip()
                if family(nm.replace(" ", "")) == kern:
                    got[nm] = float(ln.split("matrix pipe busy")[1].split()[0])
        if got:
            pipe_busy = {"source": os.path.basename(f_), "per_instantiation": got}
            counter_files["matrix_pipe_busy"] = stamp(f_)
            break
    # the roofline is priced on the pipe the kernel RUNS on.  inter_so3conv_y_kernel forms every fp32-equivalent product as three
    # fp16 x fp16 cross terms on v_mfma_f32_32x32x16_f16, so its ceiling in algorithmic (fp32-equivalent) FLOP/s is the guide's dense fp16 matrix
    # peak / 3 = 833 TFLOP/s; the bf16 six-term kernels (rounds 3 - 4) have 2 500 / 6; an fp32-MFMA kernel has 157.3.  `frac` = achieved / that peak,
    # reproducible from profiles/r06_serial_kernel_stats.txt as  sum_k 2 B p 60 24 (cin nn + cout cin) / sum_k avg duration / peak  (DESIGN 3, 5).
    # The fraction of the fp32 matrix peak SURVEY 8d wrote its ceiling in is kept beside it as `frac_vs_fp32_matrix_peak` (it can exceed 1).
    y_kernel = kern == "inter_so3conv_y_kernel"
    cross_terms = 3 if y_kernel else 6 if kern.startswith("inter_so3conv_x") else None
    peak = F16_MFMA_PEAK_TFLOPS / cross_terms if cross_terms else FP32_MFMA_PEAK_TFLOPS
    out["roofline"] = {"bound": "mfma", "kernel": kern, "instantiations": d["members"], "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                       "frac": round(achieved / peak, 4), "traffic": traffic, "algorithmic_bytes_per_launch": alg_bytes,
                       "traffic_over_algorithmic": round(traffic / alg_bytes, 2) if traffic and alg_bytes else None,
                       "matrix_pipe_busy": pipe_busy, "counter_files": counter_files,
                       "launches_per_step": d["calls"], "avg_launch_ms": round(d["ms"] / d["calls"], 4),
                       "algorithmic_gflop_per_launch": round(d["flops"] / d["calls"] / 1e9, 3),
                       "share_of_step": round(d["ms"] / tot_ms, 3),
                       "peak_is": (f"dense fp16 matrix peak {F16_MFMA_PEAK_TFLOPS:.0f} TFLOP/s (MI355X_MICROARCH.md) / {cross_terms} cross terms per fp32-equivalent product"
                                   if cross_terms else "dense fp32 matrix peak (MI355X_MICROARCH.md)"),
                       "executed_mfma_tflops": round(achieved * (cross_terms or 1), 1),
                       "frac_vs_fp32_matrix_peak": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4),
                       "arithmetic": "fp32 results and accumulators throughout.  "
                                     + ("The inter conv (csrc/so3conv_y.hip) runs both contractions on v_mfma_f32_32x32x16_f16 with TWO fp16 planes per operand (h = fp16(x), l = "
                                        "fp16(x - h), both to nearest; three cross products; operands brought to a known power-of-two range first; the fp32 MFMA's error against fp64, "
                                        "profiles/r05_f16_two_plane_split.txt) and forms the kernel weights' pre-activation on v_mfma_f32_32x32x16_bf16 from exactly split factors; "
                                        if y_kernel else "")
                                     + "the intra conv, the attention layers, the confidence head and the fused direction tail use the same two-plane fp16 form; the small-weight "
                                     "Linear layers run as exact 3 x bf16 operand splits with six cross products (profiles/r03_bf16x3_split.txt)"}
    if longest != kern:
        out["roofline"]["longest_kernel"] = {"kernel": longest, "ms": round(fam[longest]["ms"], 3), "note": "one workgroup per scan: latency-bound"}
    out["kernel_breakdown_ms"] = {k: round(v["ms"], 3) for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])[:8]}
    total_flops = sum(v["flops"] for v in agg.values())
    # the whole step's algorithmic FLOPs against the same two ceilings: the two-plane fp16 pipe (lead) and the fp32 matrix peak (SURVEY 8d's unit)
    out["whole_step_mfma_frac"] = round(total_flops / (dt / a.steps) / 1e12 / (F16_MFMA_PEAK_TFLOPS / 3.0), 4)
    out["whole_step_frac_vs_fp32_matrix_peak"] = round(total_flops / (dt / a.steps) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4)
    if not a.forward_only and not a.no_extras:
        out["stage2_latency"] = stage2_latency(args, device, cfg["iters"], B)
    if wp is not None:
        mk_wp, fitted = wp.pop("_last")
        out["value_well_posed_fit"] = wp["value"]
        out["well_posed_fit"] = wp
        if world == 1 and not a.no_cpu_baseline:
            # the metric's "V2V mm vs ref" for the bench workload: the oracle's LM on the SAME markers of two scans (bounded: the autograd LM of
            # the SMPL-X-sized model is timed on a prefix elsewhere; here SMPL only)
            if a.config == 2:
                from oracle import stage2 as S2
                mv = np.array(list(args.markerset.values()))
                ids = [0, B - 1]
                ref = S2.fit_smpl(args.body_model, mv, mk_wp[0][ids].cpu(), mk_wp[2][ids].cpu(), steps_stage0=cfg["iters"][0], steps_stage1=cfg["iters"][1])
                v2v = (fitted[ids].cpu() - ref["verts"]).norm(dim=-1).mean(1) * 1e3
                wp["v2v_mm_gpu_vs_oracle_same_markers"] = [round(float(v), 5) for v in v2v]
                wp["v2v_scans"] = ids
    if world == 1 and a.config == 2 and not a.forward_only and not a.no_extras:
        out["single_scan_latency"] = single_scan_latency(args, model, device, N)
        if latency_child is not None:
            out["single_scan_latency"]["own_process"] = latency_child
    if world == 1 and not a.no_cpu_baseline:
        def refit(run):          # the GPU fit of batch 0 with a shortened schedule (parity partner of the bounded oracle run)
            _, mk_, va_, _, aux_ = predict_smpl_batch(args, model, pts, "neutral", return_trace=True, steps_stage0=run[0], steps_stage1=run[1])
            return dict(markers=mk_, valid=va_, verts=aux_["verts"], x=aux_["x"])
        cb, parity = cpu_baseline(N, pts, model_results, last, args, threads=a.cpu_threads or None, forward_only=a.forward_only,
                                  iters=cfg["iters"], refit=refit)
        out["cpu_baseline"] = cb
        out["parity_scan0"] = parity
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
