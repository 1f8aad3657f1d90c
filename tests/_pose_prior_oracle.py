"""Oracle side of the pose prior of the marker fits (tests/test_gpu_pose_prior.py, tests/test_pose_prior_host.py).

The LM oracle is the committed oracle.stage2.lm, unmodified, as in tests/_fit_prior_oracle.py: the max-mixture GMM and the joint-angle terms
enter as extra residual rows,

    sqrt(w_gmm) L_k*^T d_k*  (P = L L^T),    sqrt(2 w_gmm (-log c_k*)),    sqrt(2 w_ang) exp(s_t x[a_t]),

so that 0.5 |f_aug|^2 is the full objective (what the kernel's trace and freeze see) and J^T J / J^T r are the kernel's additions.  Under
vmap(jacrev(.)) the component is selected with a detached one-hot mask.  The oracle is driven one iteration per call, so that the component
and the margin of its selection can be recorded at every linearisation point; a run in which the oracle's per-sample freeze would have
triggered is refused, so the chain of calls IS the single call.

The Adam oracle is oracle.stage2.fit_smpl_adam restated with the reference's two extra loss terms (fit_SMPL_Adam.py:141-153, 202-214)."""
import math

import numpy as np
import torch

from _fit_prior_oracle import DOF_GROUPS, DOF_GROUPS_X, assert_fit_parity, problem  # noqa: F401  (re-exported to the tests)

ANGLE_IDX = (52, 55, 9, 12)          # SMPLifyAnglePrior's elbows / knees with the global orientation removed
ANGLE_SIGN = (1.0, -1.0, -1.0, -1.0)


# ------------------------------------------------------------------------------------------------------------------ the synthetic mixture
def mixture(G=4, D=69, seed=5):
    """Seeded mixture in fp64 numpy: means 0.25 randn, covariances Q_k diag(sigma^2) Q_k^T with the SAME sigma = linspace(0.15, 0.5, D) permuted
    per component (equal determinants: the selection is decided by the quadratic form and the weights), weights softmax(randn).
    -> dict(means (G,D), covars (G,D,D), weights (G)): the content of a gmm_XX.pkl."""
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(G, D, generator=g, dtype=torch.float64) * 0.25
    covs = []
    for _ in range(G):
        Q, _r = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
        sig = torch.linspace(0.15, 0.5, D, dtype=torch.float64)[torch.randperm(D, generator=g)]
        covs.append(Q @ torch.diag(sig ** 2) @ Q.T)
    covs = torch.stack(covs)
    covs = 0.5 * (covs + covs.transpose(1, 2))
    w = torch.softmax(torch.randn(G, generator=g, dtype=torch.float64), 0)
    return dict(means=means.numpy(), covars=covs.numpy(), weights=w.numpy())


def buffers_fp64(gmm, np_dtype=np.float32, epsilon=1e-16):
    """MaxMixturePrior's buffers from a {means, covars, weights} dict, restated from the reference's constructor (src/utils/prior.py:131-171):
    tables cast to np_dtype, precisions = inverse of the cast covariances, nll_weights = weights / ((2 pi)^(69/2) sqrt(det) / min sqrt(det))
    from the UNCAST covariances (the 69 is the reference's literal), cov_dets = log(det(cast cov) + epsilon)."""
    means = gmm["means"].astype(np_dtype)
    covs = gmm["covars"].astype(np_dtype)
    precisions = np.stack([np.linalg.inv(c) for c in covs]).astype(np_dtype)
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in gmm["covars"]])
    nll = np.asarray(gmm["weights"] / ((2 * np.pi) ** (69 / 2.0) * (sqrdets / sqrdets.min())))
    cov_dets = np.array([np.log(np.float64(np.linalg.det(c)) + epsilon) for c in covs])
    return dict(means=means, covs=covs, precisions=precisions, nll_weights=nll.astype(np_dtype)[None], weights=gmm["weights"].astype(np_dtype)[None],
                cov_dets=cov_dets.astype(np_dtype), pi_term=np.asarray(np.log(2 * np.pi)).astype(np_dtype))


def fit_tables(gmm=None, w_gmm=0.0, angles=False, w_ang=0.0):
    """What the host hands the kernel, as CPU tensors: fp32 means, precisions symmetrised in fp64 and rounded to fp32, fp32 nll_weights.
    -> dict(means, precisions, nll_weights, w_gmm, angle_idx, angle_sign, w_ang); a part that is absent is None."""
    t = dict(means=None, precisions=None, nll_weights=None, w_gmm=float(w_gmm), angle_idx=None, angle_sign=None, w_ang=float(w_ang))
    if gmm is not None:
        b = buffers_fp64(gmm)
        P = torch.from_numpy(b["precisions"]).double()
        t.update(means=torch.from_numpy(b["means"]), precisions=(0.5 * (P + P.transpose(1, 2))).float(), nll_weights=torch.from_numpy(b["nll_weights"][0]))
    if angles:
        t.update(angle_idx=torch.tensor(ANGLE_IDX, dtype=torch.int32), angle_sign=torch.tensor(ANGLE_SIGN))
    return t


def brackets(pose, t, dtype=torch.float64):
    """(B, G) brackets 0.5 d^T P_k d - log c_k on pose (B, D) in `dtype`."""
    mu, P, lc = t["means"].to(dtype), t["precisions"].to(dtype), -torch.log(t["nll_weights"].to(dtype))
    d = pose.to(dtype)[:, None, :] - mu[None]
    return 0.5 * torch.einsum("bgi,gij,bgj->bg", d, P, d) + lc


def selection(pose, t, dtype):
    """-> component (B,) and the relative gap between the best and the second-best bracket (B,) (inf for one component)."""
    q = brackets(pose, t, dtype)
    s = q.sort(1).values
    gap = (s[:, 1] - s[:, 0]) / s[:, 0].abs() if q.shape[1] > 1 else torch.full((q.shape[0],), math.inf, dtype=dtype)
    return q.argmin(1), gap


# ------------------------------------------------------------------------------------------------------------------ the LM oracle
def _aug(f, t, dtype):
    has_gmm, has_ang = t["means"] is not None, t["angle_idx"] is not None
    if has_gmm:
        D = t["means"].shape[1]
        mu, lc = t["means"].to(dtype), -torch.log(t["nll_weights"].to(dtype))
        L = torch.linalg.cholesky(t["precisions"].to(dtype))
        assert bool((lc > 0).all())                  # the constant row needs -log c > 0
    if has_ang:
        idx, sg = t["angle_idx"].long(), t["angle_sign"].to(dtype)

    def g(x, target, mask):
        markers, pmu, pw = target
        rows = [f(x, markers, mask), torch.sqrt(pw) * (x - pmu)]
        if has_gmm:
            d = x[:D][None] - mu                                       # (G, D)
            y = torch.einsum("gji,gj->gi", L, d)                       # L_k^T d_k
            q = 0.5 * (y * y).sum(1) + lc
            sel = (q.detach() == q.detach().min()).to(dtype)           # one-hot (the margins asserted by the tests exclude ties)
            rows.append(math.sqrt(t["w_gmm"]) * (sel[:, None] * y).sum(0))
            rows.append(torch.sqrt(2.0 * t["w_gmm"] * (sel * lc).sum())[None])
        if has_ang:
            rows.append(math.sqrt(2.0 * t["w_ang"]) * torch.exp(sg * x[idx]))
        return torch.cat(rows)

    return g


def _lm_logged(S2, f, x, target, mask, iters, step, damping, trace, log, t, dtype):
    """oracle.stage2.lm, one iteration per call; the selection at every linearisation point goes to `log`."""
    def note(x):
        if t["means"] is not None:
            log.append(selection(x[:, :t["means"].shape[1]], t, dtype))

    if iters == 0:
        note(x)
        return S2.lm(f, x, target, mask, 0, step, damping, trace)
    for it in range(iters):
        note(x)
        tr = []
        x = S2.lm(f, x, target, mask, 1, step, damping, tr)
        assert len(tr) == 2
        a = (tr[0] - tr[1]).abs()
        assert not bool(((a < 1e-10) | (a / tr[0] < 1e-8)).any()), "the oracle's freeze would trigger: the chained calls are not the single call"
        trace.extend(tr if it == 0 else tr[1:])
    note(x)
    return x


def fit(bm, mv, markers, valid, it0, it1, tables, init=None, prior=None, dtype=torch.float32, lr0=0.5, lr1=0.2):
    """The two-stage fit of _fit_prior_oracle.fit under the pose prior `tables` (fit_tables).  -> dict(x, x_stage0 (kernel layout), trace
    (B, it0+it1+2), comp / gap (it0+it1+2, B): the selected component and its relative margin at every linearisation point, or None)."""
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
        t0, t1, log = [], [], []
        x0 = _lm_logged(S2, _aug(S2.residual_fn(tb, mvt, 2), tables, dtype), init[:, keep], (markers, mu[:, keep], w[:, keep]), mask, it0, lr0, 0.01,
                        t0, log, tables, dtype)
        xs0 = torch.cat([x0[:, :npose + 2], init[:, npose + 2:npose + nbt], x0[:, npose + 2:]], 1)
        x1 = _lm_logged(S2, _aug(S2.residual_fn(tb, mvt, nbt), tables, dtype), xs0, (markers, mu, w), mask, it1, lr1, 1e-3, t1, log, tables, dtype)
        comp = torch.stack([c for c, _ in log]) if log else None
        gap = torch.stack([g for _, g in log]) if log else None
        return dict(x=x1, x_stage0=xs0, trace=oracle_trace([t0, t1], it0, it1), comp=comp, gap=gap)


def assert_margins(r32, r64, min_gap=1e-3, want_switch=True):
    """The conditions under which a parity test on a max-mixture objective hides nothing: every selection of the fp64 run has a margin, the fp32
    run selects the same components, a scan changes component during the run and two components are in use at the end."""
    assert r64["gap"].shape == r32["gap"].shape and r64["gap"].numel() > 0
    print("smallest relative gap:", float(r64["gap"].min()), "components:", r64["comp"].T.tolist())
    assert float(r64["gap"].min()) >= min_gap
    assert torch.equal(r32["comp"], r64["comp"])
    if want_switch:
        assert bool((r64["comp"] != r64["comp"][0]).any()), "no scan changes its component"
        assert len(set(r64["comp"][-1].tolist())) >= 2, "one component serves every scan at the end"


# ------------------------------------------------------------------------------------------------------------------ the problem
def mixture_problem(gmm, seed=11, B=3):
    """SyntheticSMPL(7), default marker set: body pose of scan b = mean of component (1, 2, 3)[b] + 0.05 randn, orient 0.2 randn, betas 0.8 randn,
    translation 0.05 randn, 2 mm marker noise; scan 0 lacks marker 5, the last scan keeps 26 of 86.
    -> bm, marker vertex ids, markers (B,86,3), valid (B,86), x_gt (B,85)."""
    from etch_amd import constants as K
    from etch_amd.utils.body_model import SyntheticSMPL
    from oracle import stage2 as S2
    bm = SyntheticSMPL(7)
    mv = np.array(list(K.default_markerset().values()))
    tb = S2.TorchBody(bm)
    g = torch.Generator().manual_seed(seed)
    means = torch.from_numpy(gmm["means"]).float()
    body = torch.stack([means[c] for c in (1, 2, 3)[:B]]) + torch.randn(B, 69, generator=g) * 0.05
    orient = torch.randn(B, 3, generator=g) * 0.2
    gt_b = torch.randn(B, 10, generator=g) * 0.8
    gt_t = torch.randn(B, 3, generator=g) * 0.05
    with torch.no_grad():
        tgt = S2.lbs(tb, gt_b, torch.cat([orient, body], 1), gt_t)[0][:, mv] + torch.randn(B, 86, 3, generator=g) * 0.002
    valid = torch.ones(B, 86, dtype=torch.bool)
    valid[0, 5] = False
    valid[B - 1, torch.randperm(86, generator=g)[:60]] = False
    assert int(valid[B - 1].sum()) == 26
    return bm, mv, tgt.contiguous(), valid, torch.cat([body, gt_b, orient, gt_t], 1)


# ------------------------------------------------------------------------------------------------------------------ the Adam oracle
def fit_adam(bm, mv, markers, valid, it0, it1, tables, pose_prior_w, mean_shape_w, lr=1e-2, dtype=torch.float32):
    """oracle.stage2.fit_smpl_adam with loss += mean_shape_w * mean(shape^2) + pose_prior_w * sum_b min_k [.] (tables None: no pose term).
    -> dict(x (B,DOF) kernel layout, verts of the last forward, trace (it0+it1), comp / gap (it0+it1, B))."""
    from oracle import stage2 as S2
    tb = S2.TorchBody(bm, dtype)
    mvt = torch.as_tensor(np.asarray(mv)).long()
    B = markers.shape[0]
    npose, nbt = 3 * (tb.J - 1), tb.S.shape[2]
    markers = markers.to(dtype)
    pose = torch.nn.Parameter(torch.zeros(B, npose, dtype=dtype))
    shape_opt = torch.nn.Parameter(torch.zeros(B, 2, dtype=dtype))
    shape_frozen = torch.zeros(B, nbt - 2, dtype=dtype)
    orient = torch.nn.Parameter(torch.zeros(B, 3, dtype=dtype))
    transl = torch.nn.Parameter(torch.zeros(B, 3, dtype=dtype))
    trace, log = [], []
    D = None if tables is None else tables["means"].shape[1]

    def run(params, betas_fn, shape_fn, steps):
        opt = torch.optim.Adam(params, lr=lr)
        verts = None
        for _ in range(steps):
            opt.zero_grad()
            verts, _j = S2.lbs(tb, betas_fn(), torch.cat([orient, pose], 1), transl)
            loss = torch.nn.functional.mse_loss(verts[:, mvt][valid], markers[valid])
            if mean_shape_w:
                loss = loss + mean_shape_w * torch.mean(shape_fn() ** 2)
            if tables is not None:
                loss = loss + pose_prior_w * brackets(pose[:, :D], tables, dtype).min(1).values.sum()
                with torch.no_grad():
                    log.append(selection(pose[:, :D], tables, dtype))
            trace.append(float(loss.detach()))
            loss.backward()
            opt.step()
        return verts

    verts = run([shape_opt, orient, pose, transl], lambda: torch.cat([shape_opt, shape_frozen], 1), lambda: shape_opt, it0)
    shape = torch.nn.Parameter(torch.cat([shape_opt, shape_frozen], 1).detach())
    v1 = run([shape, orient, pose, transl], lambda: shape, lambda: shape, it1)
    verts = v1 if v1 is not None else verts
    x = torch.cat([pose, shape, orient, transl], 1).detach()
    return dict(x=x, verts=None if verts is None else verts.detach(), trace=np.asarray(trace),
                comp=torch.stack([c for c, _ in log]) if log else None, gap=torch.stack([g for _, g in log]) if log else None)
