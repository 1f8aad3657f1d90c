"""The pose prior of the marker fits: the max-mixture GMM and the joint-angle terms in the LM kernel, the two extra loss
terms of the Adam kernel, and the device function they share, in isolation.  The LM oracle is the committed oracle.stage2.lm, unmodified, with
the prior as extra residual rows (tests/_pose_prior_oracle.py); the mixture is a seeded synthetic one generated here."""
import math
import types

import numpy as np
import pytest
import torch

import _pose_prior_oracle as P

pytestmark = pytest.mark.gpu

W_GMM, W_ANG = 2e-3, 1e-2


def _db(bm, mv):
    from etch_amd.models.fit_SMPL import _device_body
    return _device_body(bm, mv, torch.device("cuda"))


def _pp(t, **kw):
    from etch_amd import ops
    a = dict(t)
    a.update(kw)
    return ops.PosePrior(a["means"], a["precisions"], a["nll_weights"], a["w_gmm"], a["angle_idx"], a["angle_sign"], a["w_ang"], device="cuda")


def _run(db, tgt, valid, it0, it1, pp=None, init=None, prior=None, **kw):
    from etch_amd import ops
    c = lambda t: None if t is None else t.cuda().contiguous()
    return ops.smpl_lm_fit(db.lm_consts, c(tgt), c(valid.float()), it0, 0.5, 0.01, it1, 0.2, 1e-3, True, nj=db.nj, nb=db.nb, x_init=c(init),
                           prior=None if prior is None else (c(prior[0]), c(prior[1])), pose_prior=pp, **kw)


@pytest.fixture(scope="module")
def mix():
    """The seeded mixture (G = 4, D = 69), the problem built on it, and the oracle's 6 + 10 run under GMM + angle terms in fp32 and fp64."""
    gmm = P.mixture(4, 69, seed=5)
    t = P.fit_tables(gmm, W_GMM, angles=True, w_ang=W_ANG)
    bm, mv, tgt, valid, x_gt = P.mixture_problem(gmm, seed=11)
    assert valid.sum(1).tolist() == [85, 86, 26]
    r32 = P.fit(bm, mv, tgt, valid, 6, 10, t)
    r64 = P.fit(bm, mv, tgt, valid, 6, 10, t, dtype=torch.float64)
    return types.SimpleNamespace(gmm=gmm, t=t, bm=bm, mv=mv, tgt=tgt, valid=valid, x_gt=x_gt, db=_db(bm, mv), r32=r32, r64=r64)


# ------------------------------------------------------------------------------------------------------------------ 1. the device function alone
def _eval_ref(pose, t):
    d = pose.double()[:, None, :] - t["means"].double()[None]                        # (B, G, D)
    Pm = t["precisions"].double()
    pd = torch.einsum("gij,bgj->bgi", Pm, d)
    lc = -torch.log(t["nll_weights"].double())
    q = 0.5 * (pd * d).sum(-1) + lc
    mag = 0.5 * torch.einsum("bgi,gij,bgj->bg", d.abs(), Pm.abs(), d.abs()) + lc.abs()
    gmag = torch.einsum("gij,bgj->bgi", Pm.abs(), d.abs())
    return q, pd, mag, gmag


@pytest.mark.parametrize("G,D", [(4, 69), (16, 69), (1, 69), (4, 63), (3, 1)])
def test_pose_prior_eval_vs_fp64(G, D):
    """Value, component and gradient of the bracket against fp64 torch on the same fp32 inputs.  The kernel sums <= 4 830 fp64 terms
    (n 2^-53 ~ 5e-13 of the sum of magnitudes); the bar is 1e-10 of that sum, 200 x the bound."""
    from etch_amd import ops
    t = P.fit_tables(P.mixture(G, D, seed=40 + G + D), 1.0)
    g = torch.Generator().manual_seed(G * 100 + D)
    pose = (t["means"][torch.arange(5) % G] + 0.3 * torch.randn(5, D, generator=g)).contiguous()
    val, comp, grad = ops.pose_prior_eval(pose.cuda(), _pp(t))
    q, pd, mag, gmag = _eval_ref(pose, t)
    k = q.argmin(1)
    assert val.dtype == torch.float64 and comp.dtype == torch.int32 and grad.dtype == torch.float64 and grad.shape == (5, D)
    assert torch.equal(comp.cpu().long(), k)
    r = torch.arange(5)
    ev, eg = (val.cpu() - q[r, k]).abs(), (grad.cpu() - pd[r, k]).abs()
    print("value error / bar:", float((ev / (1e-10 * mag[r, k])).max()), "gradient:", float((eg / (1e-10 * gmag[r, k])).max()))
    assert bool((ev <= 1e-10 * mag[r, k]).all())
    assert bool((eg <= 1e-10 * gmag[r, k]).all())


def test_pose_prior_eval_tie_selects_the_lowest_index(mix):
    from etch_amd import ops
    t = dict(mix.t)
    for key in ("means", "precisions", "nll_weights"):
        v = t[key].clone()
        v[0] = v[2]                               # components 0 and 2 are the same: an exact tie wherever they win
        t[key] = v
    pose = (t["means"][[2, 2, 1]] + 0.02 * torch.randn(3, 69, generator=torch.Generator().manual_seed(3))).contiguous()
    q = _eval_ref(pose, t)[0]
    assert q.argmin(1).tolist()[:2] == [0, 0] and bool((q[:2, 0] == q[:2, 2]).all())
    val, comp, grad = ops.pose_prior_eval(pose.cuda(), _pp(t))
    assert comp.tolist() == [0, 0, 1]


def test_max_mixture_prior_forward_is_the_kernel(mix, tmp_path):
    import pickle

    from etch_amd import ops
    from etch_amd.utils.prior import MaxMixturePrior
    with open(tmp_path / "gmm_04.pkl", "wb") as f:
        pickle.dump(mix.gmm, f)
    m = MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=4).cuda()
    pose = mix.x_gt[:, :69].contiguous().cuda()
    out = m(pose, None)
    val, _, _ = ops.pose_prior_eval(pose, m.as_fit_prior(1.0))
    assert out.dtype == torch.float32 and out.shape == (3,) and torch.equal(out, val.float())
    q = _eval_ref(pose.cpu(), P.fit_tables(mix.gmm, 1.0))[0].min(1).values
    assert float((out.cpu().double() - q).abs().max()) <= 1e-6 * float(q.abs().max())        # fp32 rounding of the output


# ------------------------------------------------------------------------------------------------------------------ 2. LM parity
def test_the_oracle_run_has_margins(mix):
    """What keeps the parity test below from hiding a failure: see _pose_prior_oracle.assert_margins.  No scan is excluded anywhere."""
    P.assert_margins(mix.r32, mix.r64)
    assert float((mix.r32["x"].double() - mix.r64["x"]).abs().max()) < 1e-4


def test_lm_fit_with_gmm_and_angle_terms_vs_oracle(mix):
    P.assert_margins(mix.r32, mix.r64)
    x, x0, tr = _run(mix.db, mix.tgt, mix.valid, 6, 10, _pp(mix.t))
    assert tr.shape == (3, 18)
    P.assert_fit_parity(x, x0, tr, mix.r32, lambda: mix.r64)
    xn, _, _ = _run(mix.db, mix.tgt, mix.valid, 6, 10)
    assert float((xn - x).abs().max()) > 1e-3


def _short_case(mix, t, it0=2, it1=3):
    """fp32 oracle only: its brackets carry ~1e-6 relative rounding, so a margin >= 1e-3 on that run leaves the selection unambiguous."""
    ref = P.fit(mix.bm, mix.mv, mix.tgt, mix.valid, it0, it1, t)
    if ref["gap"] is not None:
        assert float(ref["gap"].min()) >= 1e-3
    x, x0, tr = _run(mix.db, mix.tgt, mix.valid, it0, it1, _pp(t))
    P.assert_fit_parity(x, x0, tr, ref, lambda: P.fit(mix.bm, mix.mv, mix.tgt, mix.valid, it0, it1, t, dtype=torch.float64))
    xn, _, _ = _run(mix.db, mix.tgt, mix.valid, it0, it1)
    assert float((xn - x).abs().max()) > 1e-3


def test_lm_fit_gmm_only_vs_oracle(mix):
    _short_case(mix, P.fit_tables(mix.gmm, W_GMM))


def test_lm_fit_angle_terms_only_vs_oracle(mix):
    t = P.fit_tables(None, 0.0, angles=True, w_ang=W_ANG)
    assert t["means"] is None
    _short_case(mix, t)


# ------------------------------------------------------------------------------------------------------------------ 3. the 188-DoF instantiation
def test_188_dof_model_vs_oracle():
    bm, ms, mv, tgt, valid, x_gt = P.problem(2, seed=2, model="smplx")
    db = _db(bm, mv)
    t = P.fit_tables(P.mixture(4, 63, seed=6), W_GMM, angles=True, w_ang=W_ANG)
    ref = P.fit(bm, mv, tgt, valid, 2, 3, t)
    assert float(ref["gap"].min()) >= 1e-3
    x, x0, tr = _run(db, tgt, valid, 2, 3, _pp(t))
    assert x.shape == (2, 188) and tr.shape == (2, 7)
    P.assert_fit_parity(x, x0, tr, ref, lambda: P.fit(bm, mv, tgt, valid, 2, 3, t, dtype=torch.float64), groups=P.DOF_GROUPS_X, npose=162)
    xn, _, _ = _run(db, tgt, valid, 2, 3)
    assert float((xn - x).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------------ 4. with x_init and prior=
def _noisy(x_gt, seed):
    """As test_gpu_fit_prior._noisy (SMPL)."""
    g = torch.Generator().manual_seed(seed)
    B, dof = x_gt.shape
    init = x_gt + torch.randn(B, dof, generator=g) * 0.03
    mu = x_gt + torch.randn(B, dof, generator=g) * 0.03
    w = torch.zeros(B, dof)
    w[:, :69] = 0.1 + 0.2 * torch.rand(B, 69, generator=g)
    w[:, 9:21] = 0.0
    w[:, 69:79] = 50.0
    w[:, 82:] = 2.0
    return init.contiguous(), mu.contiguous(), w.contiguous()


def test_with_x_init_and_diagonal_prior_vs_oracle(mix):
    init, mu, w = _noisy(mix.x_gt, 41)
    ref = P.fit(mix.bm, mix.mv, mix.tgt, mix.valid, 5, 10, mix.t, init=init, prior=(mu, w))
    assert float(ref["gap"].min()) >= 1e-3
    x, x0, tr = _run(mix.db, mix.tgt, mix.valid, 5, 10, _pp(mix.t), init=init, prior=(mu, w))
    P.assert_fit_parity(x, x0, tr, ref, lambda: P.fit(mix.bm, mix.mv, mix.tgt, mix.valid, 5, 10, mix.t, init=init, prior=(mu, w), dtype=torch.float64))
    assert torch.equal(x0[:, 71:79].cpu(), init[:, 71:79])
    xn, _, _ = _run(mix.db, mix.tgt, mix.valid, 5, 10, init=init, prior=(mu, w))
    assert float((xn - x).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------------ 5. split fit
def test_split_fit_matches_one_workgroup_per_scan_and_repeats_bitwise(mix):
    pp = _pp(mix.t)
    tgt, valid = mix.tgt[:2], mix.valid[:2]
    x1, x01, tr1 = _run(mix.db, tgt, valid, 5, 10, pp, split=1)
    x3, x03, tr3 = _run(mix.db, tgt, valid, 5, 10, pp, split=3)
    assert torch.isfinite(x3).all()
    assert float((tr3 - tr1).abs().max()) <= 1e-6 * float(tr1.max())
    assert float((x3 - x1).abs().max()) < 2e-6 and float((x03 - x01).abs().max()) < 2e-6
    x3b, x03b, tr3b = _run(mix.db, tgt, valid, 5, 10, pp, split=3)
    assert torch.equal(x3b, x3) and torch.equal(x03b, x03) and torch.equal(tr3b, tr3)


# ------------------------------------------------------------------------------------------------------------------ 6. zero weights
def test_zero_weights_equal_the_default_fit(mix):
    pp = _pp(mix.t, w_gmm=0.0, w_ang=0.0)
    x, x0, tr = _run(mix.db, mix.tgt, mix.valid, 30, 50)
    xp, x0p, trp = _run(mix.db, mix.tgt, mix.valid, 30, 50, pp)
    assert torch.isfinite(x).all() and tr.shape == (3, 82)
    assert bool((xp == x).all()) and bool((x0p == x0).all()) and bool((trp == tr).all())


# ------------------------------------------------------------------------------------------------------------------ 7. a scan without markers
def test_scan_without_markers_is_held_by_the_mixture(mix):
    t = P.fit_tables(mix.gmm, W_GMM)
    tgt, valid = mix.tgt[:2], mix.valid[:2].clone()
    valid[0] = False
    g = torch.Generator().manual_seed(43)
    init = mix.x_gt[:2].clone()
    init[:, :69] = t["means"][[1, 2]] + 0.08 * torch.randn(2, 69, generator=g)          # off the mean
    init = init.contiguous()
    ref = P.fit(mix.bm, mix.mv, tgt, valid, 0, 10, t, init=init)
    assert float(ref["gap"].min()) >= 1e-3 and ref["comp"][:, 0].tolist() == [1] * 12
    x, x0, tr = _run(mix.db, tgt, valid, 0, 10, _pp(t), init=init)
    assert torch.isfinite(x).all() and torch.equal(x0.cpu(), init)
    P.assert_fit_parity(x, x0, tr, ref, lambda: P.fit(mix.bm, mix.mv, tgt, valid, 0, 10, t, init=init, dtype=torch.float64))
    mu1 = t["means"][1]
    assert float((x[0, :69].cpu() - mu1).norm()) < float((init[0, :69] - mu1).norm())


# ------------------------------------------------------------------------------------------------------------------ 8. the Adam fitter
def test_adam_fitter_with_pose_prior_and_mean_shape_vs_oracle(mix):
    """The bars of test_adam_fitter_vs_oracle.  Margins on the oracle's run: every selection has a relative gap >= 1e-3 and the fp32 and fp64
    runs select alike.  100 Adam steps of 1e-2 move the pose by less than the distance between two means of this mixture, so no scan changes
    component here (measured on the oracle: all three stay on the component nearest the zero pose, smallest gap 9.8e-2); the re-selection is
    covered by the LM case."""
    from etch_amd import ops
    it0, it1, wpp, wms = 40, 60, 1e-3, 1e-2
    t = P.fit_tables(mix.gmm, 0.0)
    ref = P.fit_adam(mix.bm, mix.mv, mix.tgt, mix.valid, it0, it1, t, wpp, wms)
    r64 = P.fit_adam(mix.bm, mix.mv, mix.tgt, mix.valid, it0, it1, t, wpp, wms, dtype=torch.float64)
    P.assert_margins(ref, r64, want_switch=False)
    db = mix.db
    mk, vf = mix.tgt.cuda().contiguous(), mix.valid.float().cuda().contiguous()
    x, xl, tr = ops.smpl_adam_fit(db.lm_consts, mk, vf, it0, it1, 1e-2, want_trace=True, nj=db.nj, nb=db.nb, pose_prior=_pp(t), pose_prior_w=wpp,
                                  mean_shape_w=wms)
    loss, rt = tr.cpu().numpy().sum(0), ref["trace"]
    assert loss.shape == rt.shape == (it0 + it1,)
    print("Adam loss deviation / max:", float(np.abs(loss - rt).max() / rt.max()), "parameters:", float((x.cpu() - ref["x"]).abs().max()))
    assert np.abs(loss - rt).max() / rt.max() < 1e-4
    assert float((x.cpu() - ref["x"]).abs().max()) < 2e-4
    verts, _ = ops.smpl_lbs(db.lbs_consts, xl, db.V, db.n_extra, nj=db.nj, nb=db.nb)
    assert float((verts.cpu() - ref["verts"]).abs().max()) < 1e-4
    xp, _, _ = ops.smpl_adam_fit(db.lm_consts, mk, vf, it0, it1, 1e-2, nj=db.nj, nb=db.nb)
    assert float((xp - x).abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------------------------ 9. the Python layers
def test_fit_smpl_and_fit_sequence_hand_the_prior_through(mix):
    from etch_amd import constants as K
    from etch_amd import ops, sequence
    from etch_amd.models.fit_SMPL import fit_smpl
    pp = _pp(mix.t)
    args = types.SimpleNamespace(markerset=K.default_markerset(), device=torch.device("cuda"), body_model=mix.bm)
    mk, vb = mix.tgt.cuda().contiguous(), mix.valid.cuda().contiguous()
    vf = vb.float().contiguous()
    over = (mk, vf, vb)
    pts, labels, conf = mk.clone(), torch.arange(86, device="cuda").repeat(3, 1), torch.ones(3, 86, 1, device="cuda")
    meshes, markers, vmask, info, dev = fit_smpl(args, pts, labels, conf, "neutral", 4, 5, return_trace=True, markers_override=over, pose_prior=pp)
    x, x0, tr = ops.smpl_lm_fit(mix.db.lm_consts, mk, vf, 4, 0.5, 0.01, 5, 0.2, 1e-3, True, nj=24, nb=10, pose_prior=pp)
    assert len(meshes) == 3 and info[0].shape == (3, 23, 3) and np.isfinite(meshes[0].vertices).all()
    assert torch.equal(dev["x"], x) and torch.equal(dev["err_trace"], tr)
    seq = sequence.fit_sequence(args, mk, vb, "neutral", sweeps=1, refit_steps=4, steps_stage0=4, steps_stage1=5, pose_prior=pp)
    assert seq["x"].shape == (3, 85) and torch.isfinite(seq["x"]).all() and seq["verts"].shape[0] == 3
    assert torch.equal(seq["x_independent"], x)
    # the sweep by hand: red (frames 0, 2), then black (frame 1), each refitted under the temporal prior AND the pose prior
    xs = x.clone()
    off = torch.zeros(3, 3, device="cuda")
    bmean = sequence.shape_mean(xs, vf, 24, 10)
    for p in (0, 1):
        idx = torch.arange(p, 3, 2, device="cuda")
        mean, weight = sequence.sweep_prior(xs, idx, off, bmean, sequence.DEFAULT_TEMPORAL_W, sequence.DEFAULT_SHAPE_W, 24, 10)
        xi, _, _ = ops.smpl_lm_fit(mix.db.lm_consts, mk[idx].contiguous(), vf[idx].contiguous(), 0, 0.5, 0.01, 4, 0.2, 1e-3, nj=24, nb=10,
                                   x_init=xs[idx].contiguous(), prior=(mean, weight), check=False, pose_prior=pp)
        xs = xs.index_copy(0, idx, xi)
    assert torch.equal(seq["x"], xs)
    seq0 = sequence.fit_sequence(args, mk, vb, "neutral", sweeps=1, refit_steps=4, steps_stage0=4, steps_stage1=5)
    assert float((seq0["x"] - seq["x"]).abs().max()) > 1e-3


def test_adam_fit_smpl_takes_the_reference_switches(mix, tmp_path):
    import pickle

    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.models import fit_SMPL_Adam as FA
    from etch_amd.utils.prior import MaxMixturePrior
    with open(tmp_path / "gmm_04.pkl", "wb") as f:
        pickle.dump(mix.gmm, f)
    m = MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=4).cuda()
    args = types.SimpleNamespace(markerset=K.default_markerset(), device=torch.device("cuda"), body_model=mix.bm)
    B = 3
    pts, labels, conf = mix.tgt.clone(), torch.arange(86).repeat(B, 1), torch.ones(B, 86, 1)
    for b in range(B):
        labels[b, (~mix.valid[b]).nonzero().flatten()] = int(mix.valid[b].nonzero()[0])
    conf[~mix.valid] = 1e-3
    meshes, markers, vmask, aux = FA.fit_smpl(args, pts.cuda(), labels.cuda(), conf.cuda(), steps_stage0=5, steps_stage1=6, return_aux=True,
                                              pose_prior=m, pose_prior_w=1e-3, mean_shape_w=1e-2)
    assert np.array_equal(vmask.cpu().numpy(), mix.valid.numpy()) and len(meshes) == B and np.isfinite(meshes[0].vertices).all()
    assert m.fit_tables() is m.fit_tables()                      # built once
    x, xl, tr = ops.smpl_adam_fit(mix.db.lm_consts, markers, vmask.float().contiguous(), 5, 6, 1e-2, want_trace=True, pose_prior=m.fit_tables(),
                                  pose_prior_w=1e-3, mean_shape_w=1e-2)
    assert torch.equal(aux["x"], x) and torch.equal(aux["loss_trace"], tr)
    _, _, _, plain = FA.fit_smpl(args, pts.cuda(), labels.cuda(), conf.cuda(), steps_stage0=5, steps_stage1=6, return_aux=True)
    assert float((plain["x"] - x).abs().max()) > 1e-5


# ------------------------------------------------------------------------------------------------------------------ 10. argument errors
def test_argument_errors_raise_before_any_launch(mix, monkeypatch):
    from etch_amd import _lib, ops
    t, db = mix.t, mix.db
    mk, vf = mix.tgt.cuda(), mix.valid.float().cuda()
    good = _pp(t)
    wide = _pp(P.fit_tables(P.mixture(2, 75, seed=8), W_GMM))                 # D = 75 > SMPL's 69 pose variables (fine for the 188-DoF model)
    far = ops.PosePrior(None, None, None, 0.0, torch.tensor([3, 69]), torch.tensor([1.0, -1.0]), 1e-2, device="cuda")     # index 69 = NPOSE
    on_cpu = ops.PosePrior(t["means"], t["precisions"], t["nll_weights"], W_GMM, device="cpu")
    pose = mix.x_gt[:, :69].contiguous().cuda()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    E = _lib.EtchHipError
    fit = lambda **kw: ops.smpl_lm_fit(db.lm_consts, mk, vf, 2, 0.5, 0.01, 2, 0.2, 1e-3, nj=db.nj, nb=db.nb, **kw)
    adam = lambda **kw: ops.smpl_adam_fit(db.lm_consts, mk, vf, 2, 2, nj=db.nj, nb=db.nb, **kw)
    for pp in (wide, far, on_cpu, (t["means"], t["precisions"]), t):
        with pytest.raises(E):
            fit(pose_prior=pp)
    for kw in (dict(pose_prior=wide), dict(pose_prior=on_cpu), dict(pose_prior=far), dict(pose_prior=good, pose_prior_w=-1.0),
               dict(mean_shape_w=float("nan"))):
        with pytest.raises(E):
            adam(**kw)
    for bad_pose in (pose[:, :68].contiguous(), pose.double(), pose.cpu(), pose[:, None, :]):
        with pytest.raises(E):
            ops.pose_prior_eval(bad_pose, good)
    with pytest.raises(E):
        ops.pose_prior_eval(pose, far)
    # at construction
    m, Pm, c = t["means"], t["precisions"], t["nll_weights"]
    g17 = P.fit_tables(P.mixture(17, 3, seed=9), W_GMM)
    nan_mean = m.clone()
    nan_mean[1, 4] = float("nan")
    zero_c = c.clone()
    zero_c[2] = 0.0
    indef = Pm.clone()
    indef[3] = indef[3] - 2.0 * float(torch.linalg.eigvalsh(indef[3].double()).min()) * torch.eye(69)      # its smallest eigenvalue changes sign
    nine = (torch.arange(9), torch.ones(9))
    for a in (dict(means=g17["means"], precisions=g17["precisions"], nll_weights=g17["nll_weights"]), dict(w_gmm=-1e-3), dict(w_ang=-1.0),
              dict(w_gmm=float("inf")), dict(means=nan_mean), dict(nll_weights=zero_c), dict(nll_weights=-c), dict(precisions=indef),
              dict(precisions=Pm[:, :, :68]), dict(precisions=Pm.cuda().double()[:3]), dict(means=m[:, :68]), dict(nll_weights=c[:3]),
              dict(angle_idx=nine[0], angle_sign=nine[1]), dict(angle_idx=torch.tensor([-1, 3, 4, 5])), dict(angle_sign=None),
              dict(angle_idx=torch.tensor([0.5, 1.0, 2.0, 3.0])), dict(means=None), dict(means=None, precisions=None, nll_weights=None, angle_idx=None,
                                                                                      angle_sign=None)):
        with pytest.raises(E):
            _pp(t, **a)
    with pytest.raises(AttributeError):
        good.w_gmm = 1.0
    assert math.isclose(good.w_gmm, W_GMM)
