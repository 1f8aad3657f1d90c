"""GPU checks of the chamfer refinement (csrc/chamfer_fit.hip): the two-way nearest-neighbour kernel, chamfer_distance and its
gradients, the full-mesh LBS vector-Jacobian product, fit_cham against the fp64 restatement (tests/_chamfer_oracle.py), its
determinism, and the demo's --chamfer_refine."""
import numpy as np
import pytest
import torch

import _chamfer_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _np_sqdist(p, q):
    """The kernel's bit-defined fp32 distance ((dx*dx)+(dy*dy))+(dz*dz), every op rounded (numpy float32 never fuses)."""
    d = (p - q).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _check_dir(P, Q, idx, dist, rows):
    """rows of P: returned distance = fp32 distance of the returned pair; it is the fp32 minimum, and the lowest index attaining it
    (the documented tie rule); within 2e-6 (relative to 1 + d) of the fp64 minimum."""
    for i in rows:
        d32 = _np_sqdist(P[i][None], Q)
        j = int(idx[i])
        assert dist[i] == d32[j], (i, dist[i], d32[j])
        m = d32.min()
        assert j == int(np.flatnonzero(d32 == m)[0]), (i, j)
        d64 = ((P[i][None].astype(np.float64) - Q.astype(np.float64)) ** 2).sum(1).min()
        assert abs(float(dist[i]) - d64) <= 2e-6 * (1 + d64), (i, float(dist[i]), d64)


@pytest.mark.parametrize("B,N,V,ragged,full", [(1, 1, 7, False, True), (3, 7, 1, False, True), (3, 300, 517, True, True),
                                                (32, 5000, 6890, True, False), (1, 40002, 6890, False, False)])
def test_nn_bidir_exact_ties_and_padding(B, N, V, ragged, full):
    from etch_amd import ops

    rng = np.random.default_rng(N + V)
    X = rng.standard_normal((B, N, 3)).astype(np.float32) * 0.4
    Y = rng.standard_normal((B, V, 3)).astype(np.float32) * 0.4
    if V > 2:
        Y[:, V // 2] = Y[:, 1]                            # duplicated points: exact ties, both directions
        X[:, -1] = Y[:, 1]
    if N > 2:
        X[:, N // 2] = X[:, 0]
    xl = rng.integers(max(1, N // 2), N + 1, B) if ragged else np.full(B, N)
    yl = rng.integers(max(1, V // 2), V + 1, B) if ragged else np.full(B, V)
    xt, yt = torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV)
    ixy, dxy, iyx, dyx = (t.cpu().numpy() for t in ops.nn_bidir(xt, yt, torch.from_numpy(xl), torch.from_numpy(yl)))
    rows = lambda n: range(n) if full else rng.choice(n, min(n, 60), replace=False)
    for b in range(B) if full else (0, B - 1):
        Xb, Yb = X[b, :xl[b]], Y[b, :yl[b]]
        _check_dir(Xb, Yb, ixy[b], dxy[b], rows(xl[b]))
        _check_dir(Yb, Xb, iyx[b], dyx[b], rows(yl[b]))
        assert (ixy[b, xl[b]:] == -1).all() and (iyx[b, yl[b]:] == -1).all() and (dxy[b, xl[b]:] == 0).all()
    # padding changes nothing, bitwise: garbage past the lengths (points ON the real ones) vs. every scan alone
    if ragged:
        Xg, Yg = X.copy(), Y.copy()
        for b in range(B):
            Xg[b, xl[b]:] = Y[b, 0]
            Yg[b, yl[b]:] = X[b, 0]
        got = [t.cpu().numpy() for t in ops.nn_bidir(torch.from_numpy(Xg).to(DEV), torch.from_numpy(Yg).to(DEV), torch.from_numpy(xl), torch.from_numpy(yl))]
        for a, g in zip((ixy, dxy, iyx, dyx), got):
            assert np.array_equal(a, g)
        for b in (0, B - 1):
            one = [t.cpu().numpy()[0] for t in ops.nn_bidir(torch.from_numpy(X[b:b + 1, :xl[b]].copy()).to(DEV), torch.from_numpy(Y[b:b + 1, :yl[b]].copy()).to(DEV))]
            assert np.array_equal(one[0], ixy[b, :xl[b]]) and np.array_equal(one[1], dxy[b, :xl[b]])
            assert np.array_equal(one[2], iyx[b, :yl[b]]) and np.array_equal(one[3], dyx[b, :yl[b]])


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
@pytest.mark.parametrize("batch_reduction", ["mean", "sum", None])
def test_chamfer_distance_matches_fp64_autograd(single, point_reduction, batch_reduction):
    from etch_amd import ops
    from etch_amd.models.chamfer_refine import chamfer_distance

    rng = np.random.default_rng(5)
    B, N, M = 3, 400, 700
    X = rng.standard_normal((B, N, 3)).astype(np.float32)
    Y = rng.standard_normal((B, M, 3)).astype(np.float32)
    xl, yl = np.array([400, 250, 311]), np.array([700, 699, 420])
    x = torch.from_numpy(X).to(DEV).requires_grad_(True)
    y = torch.from_numpy(Y).to(DEV).requires_grad_(True)
    loss, _ = chamfer_distance(x, y, torch.from_numpy(xl), torch.from_numpy(yl), single, point_reduction, batch_reduction)
    go = torch.linspace(0.5, 1.5, B, device=DEV) if batch_reduction is None else torch.tensor(1.3, device=DEV)
    gx, gy = torch.autograd.grad(loss, (x, y), go)
    ixy, _, iyx, _ = (t.cpu().long() for t in ops.nn_bidir(x.detach(), y.detach(), torch.from_numpy(xl), torch.from_numpy(yl)))
    # fp64 autograd with the kernel's neighbour assignment
    x6 = torch.from_numpy(X).double().requires_grad_(True)
    y6 = torch.from_numpy(Y).double().requires_grad_(True)
    per = []
    for b in range(B):
        cx = ((x6[b, :xl[b]] - y6[b][ixy[b, :xl[b]]]) ** 2).sum()
        cy = ((y6[b, :yl[b]] - x6[b][iyx[b, :yl[b]]]) ** 2).sum()
        if point_reduction == "mean":
            cx, cy = cx / xl[b], cy / yl[b]
        per.append(cx if single else cx + cy)
    per = torch.stack(per)
    ref = per.sum() if batch_reduction == "sum" else per.sum() / B if batch_reduction == "mean" else per
    rx, ry = torch.autograd.grad(ref, (x6, y6), go.cpu().double())
    rel = lambda a, r: float((a.detach().cpu().double() - r).abs().max() / r.abs().max().clamp_min(1e-30))
    assert rel(loss, ref.detach()) < 1e-5
    assert rel(gx, rx) < 1e-5 and rel(gy, ry) < 1e-5


def _random_params(bm, B, seed):
    rng = np.random.default_rng(seed)
    nj, nb = bm.num_joints, bm.num_betas
    return np.concatenate([rng.standard_normal((B, 3 * nj)) * 0.3, rng.standard_normal((B, nb)), rng.standard_normal((B, 3)) * 0.1,
                           1.0 + 0.1 * rng.standard_normal((B, 1))], 1).astype(np.float32)


@pytest.mark.parametrize("size", ["smpl", "smplx"])
def test_lbs_vjp_matches_fp64_autograd(size):
    from etch_amd import ops
    from etch_amd.models.chamfer_refine import _bm_tables
    from etch_amd.utils.body_model import SyntheticSMPL, SyntheticSMPLX

    bm = SyntheticSMPL(7) if size == "smpl" else SyntheticSMPLX(7)
    db = _bm_tables(bm, torch.device(DEV))
    B = 2
    p = _random_params(bm, B, 11)
    g = np.random.default_rng(12).standard_normal((B, bm.num_verts, 3)).astype(np.float32)
    got = ops.smpl_lbs_vjp(db.lbs_consts, torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV), nj=db.nj, nb=db.nb, n_extra=db.n_extra).cpu().numpy()
    r64 = O.lbs_vjp(bm, p, g, torch.float64)
    r32 = O.lbs_vjp(bm, p, g, torch.float32)
    s = np.abs(r64).max()
    err, ent = np.abs(got - r64).max() / s, np.abs(r32 - r64).max() / s
    assert err <= max(2 * ent, 1e-4), (err, ent)


def _scan_of(bm, p, n, seed, noise=0.002):
    from oracle import stage2 as S2
    tb = S2.TorchBody(bm, torch.float64)
    v, _ = O.forward(tb, torch.from_numpy(p).double(), bm.num_joints, bm.num_betas)
    v = v.numpy()
    rng = np.random.default_rng(seed)
    out = np.stack([v[b, rng.choice(v.shape[1], n, replace=False)] for b in range(p.shape[0])])
    return (out + noise * rng.standard_normal(out.shape)).astype(np.float32)


@pytest.mark.parametrize("bidir", [0, 1, -1])
@pytest.mark.parametrize("with_prior", [False, True])
def test_fit_cham_20_iterations_vs_fp64(bidir, with_prior):
    from etch_amd.models.chamfer_refine import fit_cham
    from etch_amd.utils.body_model import SyntheticSMPL

    bm = SyntheticSMPL(7, V=1200)
    B, n, iters = 2, 300, 20
    truth = _random_params(bm, B, 21)
    scans = _scan_of(bm, truth, n, 22)
    lengths = [n, 241]
    p0 = truth.copy()
    p0[:, :72] += 0.05 * np.random.default_rng(23).standard_normal((B, 72)).astype(np.float32)
    p0[:, -1] = 1.0
    # precisions x 1e7: the 1e-8-weighted prior is O(1) in the loss (~2) and the gradient (~0.8), and a skew part checks 0.5 (P + P^T) d
    prior = O.random_prior(24, prec_scale=1e7, skew=0.2) if with_prior else None
    init = dict(pose=p0[:, :72], beta=p0[:, 72:82], trans=p0[:, 82:85], scale=p0[:, 85:])
    st = torch.from_numpy(scans).to(DEV)
    _, prm = fit_cham(bm, st, init, prior=prior, bidir=bidir, iterations=iters, scan_lengths=lengths, want_trace=True)
    tr = prm["loss_trace"].cpu().numpy()
    pg = torch.cat([prm["pose"], prm["beta"], prm["trans"], prm["scale"]], 1).cpu().numpy()
    t64, p64 = O.fit_cham(bm, scans, lengths, p0, bidir, iters, prior=prior, dtype=torch.float64)
    t32, p32 = O.fit_cham(bm, scans, lengths, p0, bidir, iters, prior=prior, dtype=torch.float32)
    for got, r64, r32 in ((tr, t64, t32), (pg, p64, p32)):
        s = np.abs(r64).max()
        err, ent = np.abs(got - r64).max() / s, np.abs(r32 - r64).max() / s
        assert err <= max(2 * ent, 1e-4), (err, ent)
    if with_prior:
        # the prior term of the first forward, directly: loss with the prior - loss without it = 1e-8 prior_nll(pose[3:]) in fp64
        _, prm0 = fit_cham(bm, st, init, prior=None, bidir=bidir, iterations=1, scan_lengths=lengths, want_trace=True)
        nll = O.prior_nll(torch.from_numpy(p0[:, 3:72]).double(), *(torch.from_numpy(a).double() for a in prior)).numpy()
        term = tr[:, 0].astype(np.float64) - prm0["loss_trace"].cpu().numpy()[:, 0]
        assert np.abs(term - 1e-8 * nll).max() <= 1e-5 * np.abs(1e-8 * nll).max(), (term, 1e-8 * nll)
        # and the comparison above can see the prior: without it the fp64 trajectory lands far outside the tolerance
        t64n, p64n = O.fit_cham(bm, scans, lengths, p0, bidir, iters, prior=None, dtype=torch.float64)
        assert np.abs(pg - p64n).max() / np.abs(p64n).max() > 100 * max(2 * ent, 1e-4)
    assert abs(float(prm["loss"]) - float(tr[:, -1].sum())) <= 1e-6 * abs(float(prm["loss"]))


def test_fit_cham_recovers_a_known_body_and_is_deterministic():
    from etch_amd.models.chamfer_refine import fit_cham
    from etch_amd.utils.body_model import SyntheticSMPL
    from oracle import stage2 as S2

    bm = SyntheticSMPL(7)
    B, n = 4, 5000
    rng = np.random.default_rng(31)
    truth = _random_params(bm, B, 32)
    truth[:, -1] = 1.0
    scans = _scan_of(bm, truth, n, 33)
    p0 = truth.copy()
    p0[:, :72] += 0.03 * rng.standard_normal((B, 72)).astype(np.float32)
    p0[:, 82:85] += 0.01 * rng.standard_normal((B, 3)).astype(np.float32)
    init = lambda p: dict(pose=p[:, :72], beta=p[:, 72:82], trans=p[:, 82:85], scale=p[:, 85:])
    st = torch.from_numpy(scans).to(DEV)
    v1, prm1 = fit_cham(bm, st, init(p0), bidir=0, iterations=500, want_trace=True)
    v2, prm2 = fit_cham(bm, st, init(p0), bidir=0, iterations=500, want_trace=True)
    assert np.array_equal(v1, v2) and torch.equal(prm1["loss_trace"], prm2["loss_trace"])          # two runs: bitwise
    v3, prm3 = fit_cham(bm, st[2:3].contiguous(), init(p0[2:3]), bidir=0, iterations=500, want_trace=True)
    assert np.array_equal(v1[2], v3[0]) and torch.equal(prm1["loss_trace"][2], prm3["loss_trace"][0])   # scan b alone: bitwise
    tb = S2.TorchBody(bm, torch.float64)
    vt = O.forward(tb, torch.from_numpy(truth).double(), 24, 10)[0].numpy()
    v0 = O.forward(tb, torch.from_numpy(p0).double(), 24, 10)[0].numpy()
    e0 = np.linalg.norm(v0 - vt, axis=-1).mean(1)
    e1 = np.linalg.norm(v1 - vt, axis=-1).mean(1)
    tr = prm1["loss_trace"].cpu().numpy()
    print("per-vertex error mm: start", e0 * 1e3, "refined", e1 * 1e3, "loss", tr[:, 0], "->", tr[:, -1])
    assert (e1 < 2e-3).all() and (e1 < 0.5 * e0).all(), (e0, e1)      # stated bound: 2 mm mean per-vertex error (measured 0.6 mm), and at least halved
    assert (tr[:, -1] <= tr[:, 0]).all()


def test_cli_chamfer_refine(tmp_path):
    from etch_amd import inference_demo as D

    rng = np.random.default_rng(3)
    obj = tmp_path / "scan.obj"
    v = rng.standard_normal((400, 3)) * np.array([0.15, 0.45, 0.1]) + np.array([0.3, 1.0, -0.2])
    f = rng.integers(0, 400, (700, 3))
    obj.write_text("".join("v %f %f %f\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    # a seeded checkpoint: without --model_path the weights are torch's unseeded default init and two runs differ
    import types

    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded

    a = types.SimpleNamespace(output_folder=str(tmp_path / "ckpt_model"), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device(DEV),
                              markerset=K.default_markerset(), scale_magnitude=10, body_model=None)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({k: v.cpu() for k, v in load_seeded(GT_network_equiv(option=a), 1).state_dict().items()}, ckpt)
    outs = {}
    for name, extra in (("plain", []), ("none", ["--chamfer_refine", "none"]), ("both", ["--chamfer_refine", "both", "--refine_iters", "20"])):
        out = tmp_path / name
        D.main(["--scan_path", str(obj), "--synthetic_body", "--output_folder", str(out), "--num_point", "1024", "--markerset_path", "missing.json",
                "--model_path", str(ckpt)] + extra)
        outs[name] = ((out / "scan_pred_smpl.obj").read_bytes(), (out / "scan_output_smpl_info.npz").read_bytes())
    assert outs["plain"] == outs["none"]
    z = np.load(tmp_path / "both" / "scan_output_smpl_info.npz")
    assert "scale" in z.files and z["joints"].shape == (45, 3) and np.isfinite(z["joints"]).all()
    assert len([l for l in outs["both"][0].split(b"\n") if l.startswith(b"v ")]) == 6890


def test_one_sided_gradient_and_argument_checks():
    from etch_amd import _lib, ops
    from etch_amd.models.chamfer_refine import fit_cham
    from etch_amd.utils.body_model import SyntheticSMPL

    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.standard_normal((2, 300, 3)).astype(np.float32)).to(DEV)
    y = torch.from_numpy(rng.standard_normal((2, 500, 3)).astype(np.float32)).to(DEV)
    ixy, _, iyx, _ = ops.nn_bidir(x, y)
    w1, w2 = torch.tensor([0.3, 0.7], device=DEV), torch.tensor([1.1, 0.2], device=DEV)
    gx, gy = ops.chamfer_grad(x, y, ixy, iyx, w1, w2)
    # asking for one side skips the other side's scatter; the side asked for is bitwise the same
    assert torch.equal(ops.chamfer_grad(x, y, ixy, iyx, w1, w2, want_x=False)[1], gy)
    assert torch.equal(ops.chamfer_grad(x, y, ixy, iyx, w1, w2, want_y=False)[0], gx)
    with pytest.raises(_lib.EtchHipError):
        ops.nn_bidir(x, y[:1].contiguous())
    with pytest.raises(_lib.EtchHipError):
        ops.chamfer_grad(x, y, ixy[:, :10].contiguous(), iyx, w1, w2)
    bm = SyntheticSMPL(7, V=300)
    init = dict(pose=np.zeros((2, 72), np.float32), beta=np.zeros((2, 10), np.float32), trans=np.zeros((2, 3), np.float32),
                scale=np.ones((2, 1), np.float32))
    with pytest.raises(ValueError):
        fit_cham(bm, x, init, iterations=2, scan_lengths=[300, 0])       # an empty scan: sqrt(S) at 0 has no gradient
