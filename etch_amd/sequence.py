"""Track a sequence of scans: the two-stage LM fit of every frame, then red-black refits warm-started at each frame's own parameters under
diagonal Gaussian priors -- pose / orient / transl towards the mean of the temporal neighbours, betas towards the sequence's shape mean.

The reference fits every frame alone from x = 0 (fit_SMPL.py:161-249); its datasets are sequences.  Everything here runs through the LM
kernel's warm start and prior (ops.smpl_lm_fit x_init / prior, csrc/smpl_fit.hip); the bookkeeping between launches is torch on the device.

Frames: markers are in each frame's own centred frame (what stage 1 emits), `offsets` are the frames' bounding-box centres.  All kernel calls
stay in the centred frames; world translation = transl + offset, and a translation prior reaches frame t as mu_world - offset_t.

DEFAULT_TEMPORAL_W / DEFAULT_SHAPE_W were chosen on the synthetic sequence of tests/test_gpu_sequence.py; nobody has measured
them on real captures.
"""
import math

import torch

from . import ops

DEFAULT_TEMPORAL_W = (0.05, 0.5, 5.0)     # pose, orient, transl: weight of ONE neighbour (an interior frame has two)
DEFAULT_SHAPE_W = 1.0
DEFAULT_SWEEPS = 2
DEFAULT_REFIT_STEPS = 10


def nearest_rotvec(theta, ref):
    """Of the rotation vectors equivalent to `theta` (..., 3) -- theta (1 + 2 pi k / |theta|), k in {-1, 0, 1}: the same rotation -- the one
    nearest `ref` (..., 3).  Axis-angle is a many-to-one chart: two neighbouring frames may describe nearly the same rotation by vectors
    2 pi apart, and their mean would be a rotation neither of them has.  Pure torch; runs on any device.  |theta| = 0 is returned as is."""
    theta, ref = torch.broadcast_tensors(theta, ref)
    n = theta.norm(dim=-1, keepdim=True)
    safe = n > 1e-12
    unit = theta / torch.where(safe, n, torch.ones_like(n))
    best, best_d = theta, (theta - ref).norm(dim=-1, keepdim=True)
    for k in (-1.0, 1.0):
        cand = torch.where(safe, theta + (2.0 * math.pi * k) * unit, theta)
        d = (cand - ref).norm(dim=-1, keepdim=True)
        take = d < best_d
        best, best_d = torch.where(take, cand, best), torch.where(take, d, best_d)
    return best


def _rot_slices(nj, nb):
    """x layout pose | betas | orient | transl -> (pose, betas, orient, transl) slices."""
    npose = 3 * (nj - 1)
    return slice(0, npose), slice(npose, npose + nb), slice(npose + nb, npose + nb + 3), slice(npose + nb + 3, npose + nb + 6)


def _aligned(xn, xref, nj, nb):
    """Neighbour parameters `xn` with every joint's (and the global) rotation vector moved next to the one in `xref`."""
    sp, _, so, _ = _rot_slices(nj, nb)
    out = xn.clone()
    out[..., sp] = nearest_rotvec(xn[..., sp].reshape(*xn.shape[:-1], nj - 1, 3), xref[..., sp].reshape(*xref.shape[:-1], nj - 1, 3)).reshape(xn[..., sp].shape)
    out[..., so] = nearest_rotvec(xn[..., so], xref[..., so])
    return out


def fill_dead_frames(x, live, offsets, nj, nb):
    """x (T,DOF) with the rows of the dead frames (`live` (T,) bool, host) replaced by the mean of the nearest live frames before and after
    (one of them at the ends of the sequence): rotation vectors aligned to the earlier neighbour's, translation averaged in the world frame."""
    T = x.shape[0]
    st = _rot_slices(nj, nb)[3]
    live = [bool(v) for v in live]
    out = x.clone()
    for t in range(T):
        if live[t]:
            continue
        nbrs = [next((u for u in rng if live[u]), None) for rng in (range(t - 1, -1, -1), range(t + 1, T))]
        nbrs = [u for u in nbrs if u is not None]
        rows = torch.stack([_aligned(x[u], x[nbrs[0]], nj, nb) for u in nbrs])
        rows[:, st] = rows[:, st] + offsets[nbrs]
        out[t] = rows.mean(0)
        out[t, st] = out[t, st] - offsets[t]
    return out


def shape_mean(x, valid_f, nj, nb):
    """Mean of the frames' betas weighted by their valid-marker counts (dead frames: their valid rows are zero) -> (nb,)."""
    sb = _rot_slices(nj, nb)[1]
    n = valid_f.sum(1, keepdim=True)
    return (torch.where(n > 0, x[:, sb], torch.zeros_like(x[:, sb])) * n).sum(0) / n.sum().clamp_min(1.0)


def sweep_prior(x, idx, offsets, beta_mean, temporal_w, shape_w, nj, nb):
    """Prior (mean, weight), each (len(idx), DOF), of the frames `idx` (long tensor) from the CURRENT x of their existing neighbours t +- 1."""
    T, dof = x.shape
    sp, sb, so, st = _rot_slices(nj, nb)
    own = x[idx]
    acc = torch.zeros_like(own)
    cnt = torch.zeros((idx.numel(), 1), dtype=x.dtype, device=x.device)
    for step in (-1, 1):
        j = idx + step
        has = ((j >= 0) & (j < T)).to(x.dtype)[:, None]
        j = j.clamp(0, T - 1)
        nbr = _aligned(x[j], own, nj, nb)
        nbr[:, st] = nbr[:, st] + offsets[j]
        acc, cnt = acc + has * nbr, cnt + has
    mean = acc / cnt.clamp_min(1.0)
    mean[:, st] = mean[:, st] - offsets[idx]
    mean[:, sb] = beta_mean
    weight = torch.zeros_like(own)
    weight[:, sp], weight[:, so], weight[:, st] = temporal_w[0] * cnt, temporal_w[1] * cnt, temporal_w[2] * cnt
    weight[:, sb] = shape_w
    return mean.contiguous(), weight.contiguous()


def fit_sequence(args, markers, valid, gender, offsets=None, temporal_w=DEFAULT_TEMPORAL_W, shape_w=DEFAULT_SHAPE_W, sweeps=DEFAULT_SWEEPS,
                 refit_steps=DEFAULT_REFIT_STEPS, steps_stage0=30, steps_stage1=50, lr_stage0=5e-1, lr_stage1=2e-1, want_trace=False, pose_prior=None):
    """markers (T,M,3), valid (T,M) bool -> the dict of fit_smpl_device (x, verts, joints, ... of the TRACKED sequence; x_stage0 / err_trace of
    pass 0) + x_independent (pass 0's x: bitwise fit_smpl_device's on the same markers), beta_mean (nb,) and status (T,) int32.

    0. pass 0: the independent two-stage fit of all T frames, one launch.
    1. frames with marker_status != 0 are dead: valid row zeroed, x = mean of the nearest live frames' x.
    2. beta_mean = mean of the betas weighted by the frames' valid-marker counts.
    3. `sweeps` red-black sweeps: for parity p in (0, 1) the frames t = p (mod 2) are refitted in one launch from their own x, stage 1 only
       (`refit_steps` iterations), prior mean = mean of the neighbours t +- 1 (weight temporal_w[group] x number of neighbours) for pose /
       orient / transl and beta_mean (weight shape_w) for betas; beta_mean is recomputed after every full sweep.
    4. the final LBS from the final x.
    pose_prior: an ops.PosePrior handed to pass 0 and to every refit, on top of the temporal prior.
    sweeps = 0 returns pass 0 untouched.  Synchronises (the dead frames are decided on the host): not a pipelined path."""
    from .models.fit_SMPL import _device_body, _resolve_body_model
    temporal_w = tuple(float(w) for w in temporal_w)
    shape_w = float(shape_w)
    if len(temporal_w) != 3 or not all(math.isfinite(w) and w >= 0 for w in temporal_w + (shape_w,)):
        raise ValueError("temporal_w = (pose, orient, transl) and shape_w must be finite and >= 0")
    if int(sweeps) < 0 or int(refit_steps) < 0:
        raise ValueError("sweeps and refit_steps must be >= 0")
    if markers.dim() != 3 or markers.shape[2] != 3 or tuple(valid.shape) != tuple(markers.shape[:2]):
        raise ValueError(f"markers (T,M,3) and valid (T,M) expected, got {tuple(markers.shape)} and {tuple(valid.shape)}")
    T, M = valid.shape
    if M != len(args.markerset):
        raise ValueError(f"{M} markers per frame, but the marker set has {len(args.markerset)}")
    dev = markers.device
    offsets = torch.zeros((T, 3), dtype=torch.float32, device=dev) if offsets is None else torch.as_tensor(offsets, dtype=torch.float32, device=dev)
    if tuple(offsets.shape) != (T, 3):
        raise ValueError(f"offsets must have shape ({T}, 3), got {tuple(offsets.shape)}")
    bm = _resolve_body_model(args, gender)
    db = _device_body(bm, list(args.markerset.values()), dev)
    nj, nb = db.nj, db.nb
    markers = markers.contiguous()
    valid_b = valid.bool().contiguous()
    valid_f = valid_b.float().contiguous()
    x, x0, trace = ops.smpl_lm_fit(db.lm_consts, markers, valid_f, steps_stage0, lr_stage0, 0.01, steps_stage1, lr_stage1, 1e-3, want_trace,
                                   nj=nj, nb=nb, pose_prior=pose_prior)
    status = ops.marker_status(markers, valid_f)
    x_independent = x
    live = (status == 0).cpu()
    if int(sweeps) > 0 and bool(live.any()):
        lv = live.to(dev)
        fit_valid = torch.where(lv[:, None], valid_f, torch.zeros_like(valid_f)).contiguous()
        fit_markers = torch.where(lv[:, None, None], markers, torch.zeros_like(markers)).contiguous()     # 0 * NaN is NaN in the residual
        x = fill_dead_frames(x, live.tolist(), offsets, nj, nb) if not bool(live.all()) else x.clone()
        beta_mean = shape_mean(x, fit_valid, nj, nb)
        for _ in range(int(sweeps)):
            for p in (0, 1):
                idx = torch.arange(p, T, 2, device=dev)
                if idx.numel() == 0:
                    continue
                mean, weight = sweep_prior(x, idx, offsets, beta_mean, temporal_w, shape_w, nj, nb)
                xi, _, _ = ops.smpl_lm_fit(db.lm_consts, fit_markers[idx].contiguous(), fit_valid[idx].contiguous(), 0, lr_stage0, 0.01,
                                           int(refit_steps), lr_stage1, 1e-3, nj=nj, nb=nb, x_init=x[idx].contiguous(), prior=(mean, weight),
                                           check=False, pose_prior=pose_prior)      # finite by construction: live or filled frames, weights validated above
                x = x.index_copy(0, idx, xi)
            beta_mean = shape_mean(x, fit_valid, nj, nb)
    else:
        lv = live.to(dev)
        beta_mean = shape_mean(torch.where(lv[:, None], x, torch.zeros_like(x)), torch.where(lv[:, None], valid_f, torch.zeros_like(valid_f)), nj, nb)
    x = x.contiguous()
    verts, joints = ops.smpl_lbs(db.lbs_consts, x, db.V, db.n_extra, nj=nj, nb=nb)
    return dict(markers=markers, valid=valid_b, x=x, x_stage0=x0, err_trace=trace, verts=verts, joints=joints, faces=db.faces, status=status,
                nj=nj, nb=nb, x_independent=x_independent, beta_mean=beta_mean)


def joint_displacement(joints, offsets=None):
    """Mean over frames and joints of |joint_t+1 - joint_t| in the world frame: the jitter figure track.py records.  joints (T,J,3)."""
    j = joints if offsets is None else joints + offsets[:, None, :]
    if j.shape[0] < 2:
        return 0.0
    return float((j[1:] - j[:-1]).norm(dim=-1).mean())
