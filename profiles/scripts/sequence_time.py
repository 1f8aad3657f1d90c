"""Timing record of the sequence tracker: pass 0 alone (the independent two-stage fit of all frames, fit_sequence with
sweeps = 0) against the full tracker at the default sweeps, T = 64 synthetic frames, MI355X.

    python profiles/scripts/sequence_time.py [--frames 64] [--reps 15] [--out profiles/sequence_time.json]

Host clock around calls that end in a device synchronise (fit_sequence reads the status words back, so the time includes its launches' gaps);
both candidates are warmed up and then take turns inside every repeat.  The sequence: SyntheticSMPL(7), pose and translation linear in t,
constant betas, 2 mm marker noise, one frame without markers and one with 26 of 86 -- the inputs of tests/test_gpu_sequence.py, longer.
There is no target for the ratio; it is a record."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def synthetic_sequence(T, seed=21):
    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.models.fit_SMPL import _device_body
    from etch_amd.utils.body_model import SyntheticSMPL
    bm = SyntheticSMPL(7)
    ms = K.default_markerset()
    mv = list(ms.values())
    db = _device_body(bm, mv, torch.device("cuda"))
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32)[:, None]
    pose = torch.randn(1, 72, generator=g) * 0.2 + t * (torch.randn(1, 72, generator=g) * (0.03 * 4 / max(T - 1, 1)))
    betas = (torch.randn(1, 10, generator=g) * 0.8).expand(T, -1)
    world_t = torch.randn(1, 3, generator=g) * 0.05 + t * torch.tensor([[0.03, 0.0, 0.015]]) * (4 / max(T - 1, 1))
    offsets = world_t + torch.randn(T, 3, generator=g) * 0.01
    x = torch.cat([pose[:, 3:], betas, pose[:, :3], world_t - offsets], 1).contiguous().cuda()
    verts, _ = ops.smpl_lbs(db.lbs_consts, x, db.V, db.n_extra)
    markers = verts[:, torch.tensor(mv, device="cuda")] + (torch.randn(T, 86, 3, generator=g) * 0.002).cuda()
    valid = torch.ones(T, 86, dtype=torch.bool)
    valid[T // 2] = False
    valid[T // 2 + 1, torch.randperm(86, generator=g)[:60]] = False
    args = types.SimpleNamespace(markerset=ms, device=torch.device("cuda"), body_model=bm)
    return args, markers.contiguous(), valid.cuda(), offsets.cuda()


def main():
    from etch_amd import sequence as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("sequence_time.py measures on the GPU; there is nothing to time without one")
    args, markers, valid, offsets = synthetic_sequence(a.frames)
    fns = {"pass0": lambda: S.fit_sequence(args, markers, valid, "neutral", offsets=offsets, sweeps=0),
           "tracker": lambda: S.fit_sequence(args, markers, valid, "neutral", offsets=offsets)}
    for fn in fns.values():                       # warm-up: code objects, the body model's device tables, the allocator
        fn(), fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    stat = {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in t.items()}
    res = {"note": "ms per call [median, min, max], host clock around calls that end in a synchronise, the two alternating inside every repeat",
           "frames": a.frames, "reps": a.reps, "schedule": {"pass0": [30, 50], "sweeps": S.DEFAULT_SWEEPS, "refit_steps": S.DEFAULT_REFIT_STEPS},
           "temporal_w": list(S.DEFAULT_TEMPORAL_W), "shape_w": S.DEFAULT_SHAPE_W, "ms": stat,
           "tracker_over_pass0": round(stat["tracker"][0] / stat["pass0"][0], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
