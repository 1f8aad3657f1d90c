"""Oracle side of the warm-started / prior LM fit and of the sequence tracker (tests/test_gpu_fit_prior.py, tests/test_gpu_sequence.py).

The oracle is the committed oracle.stage2.lm, unmodified: it is generic in the residual function and in the starting x.  The prior enters
as extra residual rows, f_aug = cat([f(x, markers, mask), sqrt(w) (x - mu)]), with target = (markers, mu, w) as a tuple (vmap maps pytrees);
0.5 |f_aug|^2 is then the full objective, which is what the kernel's trace and freeze see.  Stage 0 works on the reduced vector (betas[:2]),
stage 1 on the full one, started at [x0 pose, x0 betas[:2], init betas[2:], x0 orient, x0 transl]."""
import math

import numpy as np
import torch

DOF_GROUPS = {"body pose": slice(0, 63), "hands": slice(63, 69), "betas[:2]": slice(69, 71), "betas[2:]": slice(71, 79), "orient": slice(79, 82),
              "transl": slice(82, 85)}
DOF_GROUPS_X = {"pose": slice(0, 162), "betas[:2]": slice(162, 164), "betas[2:]": slice(164, 182), "orient": slice(182, 185), "transl": slice(185, 188)}


def problem(B, seed=0, model="smpl"):
    """A seeded fit problem on the synthetic body (built like _problem of tests/test_gpu_stage2.py): noisy markers of random bodies, scan 0
    missing 1 marker and the last scan missing 4.  -> bm, markerset, marker vertex ids, markers (B,86,3), valid (B,86), x_gt (B,DOF)."""
    from etch_amd import constants as K
    from etch_amd.utils.body_model import SyntheticSMPL, SyntheticSMPLX
    from oracle import stage2 as S2
    bm = SyntheticSMPL(7) if model == "smpl" else SyntheticSMPLX(7)
    ms = K.default_markerset()
    mv = np.array(list(ms.values()))
    tb = S2.TorchBody(bm)
    g = torch.Generator().manual_seed(seed)
    gt_pose = torch.randn(B, 3 * bm.num_joints, generator=g) * 0.2
    gt_b = torch.randn(B, bm.num_betas, generator=g) * 0.8
    gt_t = torch.randn(B, 3, generator=g) * 0.05
    with torch.no_grad():
        vgt = S2.lbs(tb, gt_b, gt_pose, gt_t)[0]
    tgt = vgt[:, mv] + torch.randn(B, 86, 3, generator=g) * 0.002
    valid = torch.ones(B, 86, dtype=torch.bool)
    valid[0, 5] = False
    valid[B - 1, 40:44] = False
    x_gt = torch.cat([gt_pose[:, 3:], gt_b, gt_pose[:, :3], gt_t], 1)
    return bm, ms, mv, tgt, valid, x_gt


def _aug(f):
    def g(x, target, mask):
        markers, mu, w = target
        return torch.cat([f(x, markers, mask), torch.sqrt(w) * (x - mu)])

    return g


def fit(bm, mv, markers, valid, it0, it1, init=None, prior=None, dtype=torch.float32, lr0=0.5, lr1=0.2):
    """The two-stage fit through oracle.stage2.lm with a starting point and a prior.  -> dict(x (B,DOF), x_stage0 (B,DOF) in the kernel's
    layout (inactive betas = their init values), trace (B, it0+it1+2))."""
    from _parity import oracle_trace
    from oracle import stage2 as S2
    with torch.no_grad():
        tb = S2.TorchBody(bm, dtype)
        mvt = torch.as_tensor(np.asarray(mv)).long()
        npose, nbt = 3 * (tb.J - 1), tb.S.shape[2]
        dof = npose + nbt + 6
        B = markers.shape[0]
        markers, mask = markers.to(dtype), valid.to(dtype)
        init = torch.zeros(B, dof, dtype=dtype) if init is None else init.to(dtype)
        mu, w = (torch.zeros(B, dof, dtype=dtype), torch.zeros(B, dof, dtype=dtype)) if prior is None else (prior[0].to(dtype), prior[1].to(dtype))
        keep = list(range(npose + 2)) + list(range(npose + nbt, dof))
        t0, t1 = [], []
        x0 = S2.lm(_aug(S2.residual_fn(tb, mvt, 2)), init[:, keep], (markers, mu[:, keep], w[:, keep]), mask, it0, lr0, 0.01, t0)
        xs0 = torch.cat([x0[:, :npose + 2], init[:, npose + 2:npose + nbt], x0[:, npose + 2:]], 1)
        x1 = S2.lm(_aug(S2.residual_fn(tb, mvt, nbt)), xs0, (markers, mu, w), mask, it1, lr1, 1e-3, t1)
        return dict(x=x1, x_stage0=xs0, trace=oracle_trace([t0, t1], it0, it1))


def assert_fit_parity(got_x, got_x0, got_trace, ref32, run64, groups=DOF_GROUPS, npose=69):
    """The bars of test_lm_fit_vs_oracle: every DoF within 1e-4, trace within 2e-3 rt + 1e-7 and 1e-4 of its maximum, x_stage0's pose within
    1e-4.  A DoF group that misses 1e-4 falls under the project's entitled-error rule (tests/_parity.py, the conditioning stress test): it must
    be as close to the oracle's fp64 run as the oracle's own fp32 run is, x 2.  run64: callable -> the fp64 run (evaluated only then)."""
    x, xr = got_x.cpu().numpy().astype(np.float64), ref32["x"].numpy().astype(np.float64)
    assert np.isfinite(x).all()
    dev = np.abs(x - xr)
    print("parameter deviation vs oracle (fp32):", {k: float(dev[:, sl].max()) for k, sl in groups.items()})
    r64 = None
    for name, sl in groups.items():
        if dev[:, sl].max() < 1e-4:
            continue
        r64 = run64() if r64 is None else r64
        x64 = r64["x"].numpy()
        gpu, ref = float(np.abs(x[:, sl] - x64[:, sl]).max()), float(np.abs(xr[:, sl] - x64[:, sl]).max())
        print(f"entitled error, {name}: gpu {gpu:.2e}, oracle fp32 {ref:.2e}")
        assert gpu <= 2.0 * ref, (name, gpu, ref)
    if got_trace is not None:
        gt, rt = got_trace.cpu().numpy(), ref32["trace"]
        assert gt.shape == rt.shape, (gt.shape, rt.shape)
        assert np.abs(gt - rt).max() / rt.max() < 1e-4
        assert (np.abs(gt - rt) <= 2e-3 * rt + 1e-7).all()
    if got_x0 is not None:
        assert np.abs(got_x0.cpu().numpy()[:, :npose] - ref32["x_stage0"].numpy()[:, :npose]).max() < 1e-4


# ------------------------------------------------------------------------------------------------------------------ the tracker's schedule
def nearest_rotvec_ref(theta, ref):
    """Per 3-vector, by enumeration (numpy, fp64 norms): the equivalent rotation vector nearest `ref`."""
    theta, ref = np.asarray(theta), np.asarray(ref)
    out = theta.copy().reshape(-1, 3)
    for i, (a, r) in enumerate(zip(theta.reshape(-1, 3), ref.reshape(-1, 3))):
        n = float(np.linalg.norm(a.astype(np.float64)))
        if n <= 1e-12:
            continue
        cands = [a * (1.0 + 2.0 * math.pi * k / n) for k in (0, -1, 1)]
        out[i] = min(cands, key=lambda c: float(np.linalg.norm(c - r))).astype(theta.dtype)
    return out.reshape(theta.shape)


def sequence_problem(T=5, seed=21):
    """T frames of a smooth motion on SyntheticSMPL(7): pose and translation linear in t, constant betas, 2 mm marker noise; frame 2 has no
    valid marker and frame 3 keeps 26 of 86.  Markers are in each frame's own frame (world markers minus the frame's offset)."""
    from etch_amd import constants as K
    from etch_amd.utils.body_model import SyntheticSMPL
    from oracle import stage2 as S2
    bm = SyntheticSMPL(7)
    ms = K.default_markerset()
    mv = np.array(list(ms.values()))
    tb = S2.TorchBody(bm)
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32)[:, None]
    pose = torch.randn(1, 72, generator=g) * 0.2 + t * (torch.randn(1, 72, generator=g) * 0.03)
    betas = (torch.randn(1, 10, generator=g) * 0.8).expand(T, -1).contiguous()
    world_t = torch.randn(1, 3, generator=g) * 0.05 + t * torch.tensor([[0.03, 0.0, 0.015]])
    offsets = world_t + torch.randn(T, 3, generator=g) * 0.01            # bbox centres: near the body, not on its path
    with torch.no_grad():
        v = S2.lbs(tb, betas, pose, world_t)[0]
    markers = v[:, mv] + torch.randn(T, 86, 3, generator=g) * 0.002 - offsets[:, None]
    valid = torch.ones(T, 86, dtype=torch.bool)
    valid[2] = False
    drop = torch.randperm(86, generator=g)[:60]
    valid[3, drop] = False
    assert int(valid[3].sum()) == 26
    return bm, ms, mv, markers.contiguous(), valid, offsets.contiguous()


def track(bm, mv, markers, valid, offsets, temporal_w, shape_w, sweeps, refit_steps, it0, it1, dtype=torch.float32):
    """etch_amd.sequence.fit_sequence's schedule, frame by frame, through `fit`: pass 0, dead-frame filling, the weighted shape mean, red-black
    sweeps (stage 1 only, warm-started, prior from the neighbours' current x).  -> dict(x, x_independent, beta_mean)."""
    T = markers.shape[0]
    npose, nb = 3 * (bm.num_joints - 1), bm.num_betas
    st, so = slice(npose + nb + 3, npose + nb + 6), slice(npose + nb, npose + nb + 3)
    off = offsets.to(dtype)
    x_ind = fit(bm, mv, markers, valid, it0, it1, dtype=dtype)["x"]
    x = x_ind.clone()
    valid = valid.clone()
    live = [bool(valid[t].any()) and bool(torch.isfinite(markers[t][valid[t]]).all()) for t in range(T)]

    def align(row, ref):
        row = row.clone()
        row[:npose] = torch.from_numpy(nearest_rotvec_ref(row[:npose].numpy().reshape(-1, 3), ref[:npose].numpy().reshape(-1, 3)).reshape(-1))
        row[so] = torch.from_numpy(nearest_rotvec_ref(row[so].numpy(), ref[so].numpy()))
        return row

    def world(row, t):
        row = row.clone()
        row[st] = row[st] + off[t]
        return row

    for t in range(T):
        if live[t]:
            continue
        valid[t] = False
        left = next((u for u in range(t - 1, -1, -1) if live[u]), None)
        right = next((u for u in range(t + 1, T) if live[u]), None)
        nbrs = [u for u in (left, right) if u is not None]
        rows = torch.stack([world(align(x_ind[u], x_ind[nbrs[0]]), u) for u in nbrs])
        x[t] = rows.mean(0)
        x[t, st] -= off[t]
    markers = torch.where(torch.tensor(live)[:, None, None], markers, torch.zeros_like(markers))
    counts = valid.sum(1).to(dtype)

    def beta_mean():
        return (x[:, npose:npose + nb] * counts[:, None]).sum(0) / counts.sum()

    bmean = beta_mean()
    for _ in range(sweeps):
        for p in (0, 1):
            idx = list(range(p, T, 2))
            if not idx:
                continue
            mu, w = torch.zeros(len(idx), x.shape[1], dtype=dtype), torch.zeros(len(idx), x.shape[1], dtype=dtype)
            for i, t in enumerate(idx):
                nbrs = [u for u in (t - 1, t + 1) if 0 <= u < T]
                if nbrs:
                    mu[i] = torch.stack([world(align(x[u], x[t]), u) for u in nbrs]).mean(0)
                    mu[i, st] -= off[t]
                w[i, :npose], w[i, so], w[i, st] = temporal_w[0] * len(nbrs), temporal_w[1] * len(nbrs), temporal_w[2] * len(nbrs)
                mu[i, npose:npose + nb], w[i, npose:npose + nb] = bmean, shape_w
            x[idx] = fit(bm, mv, markers[idx], valid[idx], 0, refit_steps, init=x[idx], prior=(mu, w), dtype=dtype)["x"]
        bmean = beta_mean()
    return dict(x=x, x_independent=x_ind, beta_mean=bmean, live=live)


def world_joints(bm, x, offsets):
    """Joints (T,J,3) of parameters x (T,DOF) in the world frame, through the oracle's LBS."""
    from oracle import stage2 as S2
    npose, nb = 3 * (bm.num_joints - 1), bm.num_betas
    with torch.no_grad():
        _, j = S2.smpl_forward(S2.TorchBody(bm, x.dtype), x[:, npose:npose + nb], x[:, :npose], x[:, npose + nb:npose + nb + 3], x[:, npose + nb + 3:])
    return j + offsets.to(x.dtype)[:, None]


def shape_spread(x, live, npose=69, nb=10):
    """Max over coefficients of the std over the live frames' betas."""
    b = np.asarray(x, np.float64)[np.asarray(live, bool), npose:npose + nb]
    return float(b.std(0).max())


def jitter(joints):
    """Mean frame-to-frame joint displacement."""
    j = np.asarray(joints, np.float64)
    return float(np.linalg.norm(j[1:] - j[:-1], axis=-1).mean())
