"""GPU checks of the dense surface refinement (csrc/surface_fit.hip): the closest-point kernel bit for bit against the fp32 restatement of
the region test and against the reference's own point-mesh distance, the energy and its gradient against fp64 autograd, fit_surface
against the fp64 restatement of its schedule (tests/_surface_oracle.py), recovery of a known body, determinism, and the demo's
--surface_refine."""
import functools

import numpy as np
import pytest
import torch

import _chamfer_oracle as CO
import _surface_oracle as O
from tests._pt_fp64 import check

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _soup():
    z = np.load(O.GOLDEN)
    verts, faces, pts, lengths = z["verts"], z["faces"], z["points"], z["lengths"]
    return verts, faces, pts, lengths, z["ref32"], z["ref64"], O.closest_batch(pts, lengths, verts, faces)


def _closest(pts, verts, faces, lengths=None):
    from etch_amd import ops
    return tuple(t.cpu().numpy() for t in ops.point_mesh_closest(_dev(pts), _dev(verts), _dev(faces), None if lengths is None else _dev(lengths)))


def test_closest_is_bitwise_the_fp32_restatement():
    """B = 3, N = 257, lengths (257, 64, 0), V = 40, F = 70 (no multiple of any tile): shared vertices, two zero-area faces, a duplicated
    face, crafted points in all seven regions, and three points equidistant from faces 0 and 1 across their shared edge."""
    verts, faces, pts, lengths, _, _, (rf, rb, rd, rr) = _soup()
    tri = verts[0][faces[:2].astype(np.int64)]
    for row in (254, 255, 256):                                                    # the tie between two DIFFERENT faces, in the restatement
        _, d01, reg = O.closest_on_triangles(pts[0, row][None, :], tri[:, 0], tri[:, 1], tri[:, 2])
        assert reg.tolist() == [2, 2] and d01.view(np.uint32)[0] == d01.view(np.uint32)[1] == rd[0, row].view(np.uint32) and rf[0, row] == 0
    assert pts.shape == (3, 257, 3) and verts.shape == (3, 40, 3) and faces.shape == (70, 3) and lengths.tolist() == [257, 64, 0]
    assert set(np.unique(rr[rr >= 0]).tolist()) == set(range(7))                   # every region of the test is some point's answer
    assert (rf == 3).any() and not (rf == 69).any()                               # the duplicated face: ties go to the lower one
    face, bary, d2 = _closest(pts, verts, faces, lengths)
    assert face.dtype == np.int32 and bary.dtype == np.float32 and d2.dtype == np.float32
    assert np.array_equal(face, rf) and (face[0, 254:] == 0).all()                 # equal d2 on faces 0 and 1: the lower face
    assert np.array_equal(bary.view(np.uint32), rb.view(np.uint32)) and np.array_equal(d2.view(np.uint32), rd.view(np.uint32))
    for b in range(3):                                                             # padding rows
        n = lengths[b]
        assert (face[b, n:] == -1).all() and (bary[b, n:] == 0).all() and (d2[b, n:] == 0).all()
    again = _closest(pts, verts, faces, lengths)                                   # two runs
    assert all(np.array_equal(a, g) for a, g in zip((face, bary, d2), again))
    for b in (0, 1):                                                               # scan b alone
        n = lengths[b]
        one = _closest(pts[b:b + 1, :n].copy(), verts[b:b + 1], faces)
        assert np.array_equal(one[0][0], face[b, :n]) and np.array_equal(one[1][0], bary[b, :n]) and np.array_equal(one[2][0], d2[b, :n])
    garbage = pts.copy()                                                           # what lies past the lengths changes nothing
    garbage[1, 64:] = verts[1, 0]
    garbage[2] = np.nan
    assert all(np.array_equal(a, g) for a, g in zip((face, bary, d2), _closest(garbage, verts, faces, lengths)))


def test_closest_more_than_one_chunk_and_block():
    """F = 2500 faces (three 1024-face chunks merged through the keys) and N = 700 points (two 512-point blocks), sampled rows."""
    rng = np.random.default_rng(3)
    V, F, N = 300, 2500, 700
    verts = rng.uniform(-1, 1, (1, V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[2499] = faces[5]
    pts = rng.uniform(-1, 1, (1, N, 3)).astype(np.float32)
    face, bary, d2 = _closest(pts, verts, faces)
    rows = np.concatenate([np.arange(0, N, 9), [511, 512, 699]])
    rf, rb, rd, _ = O.closest_point_on_mesh(pts[0, rows], verts[0], faces)
    assert np.array_equal(face[0, rows], rf) and np.array_equal(bary[0, rows], rb) and np.array_equal(d2[0, rows], rd)
    assert (face >= 0).all() and face.max() >= 2048


def test_closest_against_the_reference_function():
    """sqrt(d2) within 2 e_32 + 1e-6 of the reference's my_point_mesh_face_distance in fp64 (tests/golden/point_mesh_unit_soup.npz, written
    by tests/_make_surface_fixture.py from the reference itself); e_32 = the reference's own fp32 error."""
    verts, faces, pts, _, ref32, ref64, _ = _soup()
    _, _, d2 = _closest(pts, verts, faces)
    e32 = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(np.sqrt(d2.astype(np.float64)) - ref64).max())
    print(f"PIN point_mesh vs reference: e_gpu {err:.3e}, e_32 {e32:.3e}")
    assert err <= 2 * e32 + 1e-6, (err, e32)


# --------------------------------------------------------------------------------------------- a small body with a real surface
@functools.lru_cache(maxsize=None)
def _body():
    from etch_amd.utils.body_model import SyntheticSurfaceSMPL
    bm = SyntheticSurfaceSMPL(7, rings=20, segs=24)
    assert bm.num_verts == 482 and bm.faces.shape == (960, 3)
    return bm


def _params(B, seed, pose=0.2, beta=1.0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal((B, 72)) * pose, rng.standard_normal((B, 10)) * beta, rng.standard_normal((B, 3)) * 0.1,
                           np.ones((B, 1))], 1).astype(np.float32)


def _verts64(bm, p):
    from oracle import stage2 as S2
    return CO.forward(S2.TorchBody(bm, torch.float64), torch.from_numpy(np.asarray(p)).double(), 24, 10)[0].numpy()


def _surface_points(bm, verts, n, seed, noise):
    """n points per scan on the surface of verts (B,V,3) (area-blind: a random face, uniform barycentric weights) + noise along all axes."""
    rng = np.random.default_rng(seed)
    out = []
    for v in verts:
        f = bm.faces[rng.integers(0, len(bm.faces), n)]
        w = rng.dirichlet(np.ones(3), n)
        out.append((w[:, :, None] * v[f]).sum(1) + noise * rng.standard_normal((n, 3)))
    return np.stack(out).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _energy_problem():
    bm = _body()
    B, N = 2, 300
    verts = _verts64(bm, _params(B, 51)).astype(np.float32)
    pts = _surface_points(bm, verts, N, 52, 0.02)
    rng = np.random.default_rng(53)
    w = rng.uniform(0.0, 2.0, (B, N)).astype(np.float32)
    w[:, ::7] = 0.0
    return bm, verts, pts, np.array([300, 211], np.int32), w, 0.03


def _energy(pts, verts, faces, lengths, w, trunc, **kw):
    from etch_amd import ops
    p, v, f = _dev(pts), _dev(verts), _dev(faces)
    nl = _dev(lengths)
    face, bary, d2 = ops.point_mesh_closest(p, v, f, nl)
    terms, g, _ = ops.point_mesh_energy_grad(p, v, f, face, bary, d2, None if w is None else _dev(w), trunc, nl, **kw)
    return face.cpu().numpy(), bary.cpu().numpy(), d2.cpu().numpy(), terms.cpu().numpy(), g.cpu().numpy()


def test_energy_and_gradient_vs_fp64():
    bm, verts, pts, lengths, w, trunc = _energy_problem()
    B, N = pts.shape[:2]
    face, bary, d2, terms, g = _energy(pts, verts, bm.faces, lengths, w, trunc, w_dense=1e2)
    t2 = np.float32(trunc) * np.float32(trunc)
    valid = np.arange(N)[None] < lengths[:, None]
    m = valid & (d2 <= t2)
    assert 0.2 < m[valid].mean() < 0.95 and (w[m] == 0).any()                     # the mask and the weights are both at work
    want = np.stack([(w.astype(np.float64) * m * d2.astype(np.float64)).sum(1), (w.astype(np.float64) * m).sum(1)], 1)
    rel = np.abs(terms - want) / np.abs(want)
    print("PIN point_mesh terms: max relative error", rel.max())
    assert terms.dtype == np.float64 and (rel <= 1e-12).all(), (terms, want)
    # the gradient of w_dense S1 / S0 by autograd with the kernel's correspondences, in fp64 and in fp32
    faces = torch.from_numpy(bm.faces.astype(np.int64))

    def ref(dt):
        v = torch.from_numpy(verts).to(dt).requires_grad_(True)
        tot = 0
        for b in range(B):
            n = lengths[b]
            S1, S0 = O.dense_terms(v[b], faces, torch.from_numpy(pts[b, :n]).to(dt), torch.from_numpy(face[b, :n]).long(),
                                   torch.from_numpy(bary[b, :n]).to(dt), torch.from_numpy(w[b, :n]).to(dt), trunc)
            tot = tot + 1e2 * S1 / S0
        tot.backward()
        return v.grad.numpy()

    check("point_mesh dL/dverts", g, ref(torch.float64), ref(torch.float32))


def test_zero_weight_and_truncated_points_change_nothing():
    bm, verts, pts, lengths, w, trunc = _energy_problem()
    B, N = pts.shape[:2]
    full = np.array([N, N], np.int32)
    *_, terms, g = _energy(pts, verts, bm.faces, full, w, trunc, w_dense=1e2)
    rng = np.random.default_rng(54)
    extra = np.concatenate([_surface_points(bm, verts, 40, 55, 0.01), (verts[:, :40] * 3.0 + 1.0).astype(np.float32)], 1)   # near; far beyond trunc
    we = np.concatenate([np.zeros((B, 40), np.float32), rng.uniform(0.5, 2.0, (B, 40)).astype(np.float32)], 1)
    _, _, d2e, terms2, g2 = _energy(np.concatenate([pts, extra], 1), verts, bm.faces, full + 80, np.concatenate([w, we], 1), trunc, w_dense=1e2)
    assert (d2e[:, N + 40:] > trunc * trunc).all() and (d2e[:, N:N + 40] <= trunc * trunc).any()
    assert np.array_equal(terms, terms2) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))


def test_point_mesh_face_distance_autograd():
    """The autograd Function: value and both gradients against fp64 autograd, every reduction."""
    from etch_amd import ops
    from etch_amd.models.surface_refine import point_mesh_face_distance
    bm, verts, pts, lengths, w, trunc = _energy_problem()
    B = len(pts)
    faces = torch.from_numpy(bm.faces.astype(np.int64))
    face, bary, _ = (t.cpu() for t in ops.point_mesh_closest(_dev(pts), _dev(verts), _dev(bm.faces), _dev(lengths)))
    for pr, br in (("mean", "mean"), ("sum", "sum"), ("mean", None)):
        v = _dev(verts).requires_grad_(True)
        p = _dev(pts).requires_grad_(True)
        loss = point_mesh_face_distance(v, bm.faces, p, lengths, _dev(w), trunc, pr, br)
        go = torch.linspace(0.5, 1.5, B, device=DEV) if br is None else torch.tensor(1.3, device=DEV)
        gv, gp = torch.autograd.grad(loss, (v, p), go)
        v6 = torch.from_numpy(verts).double().requires_grad_(True)
        p6 = torch.from_numpy(pts).double().requires_grad_(True)
        per = []
        for b in range(B):
            n = lengths[b]
            S1, S0 = O.dense_terms(v6[b], faces, p6[b, :n], face[b, :n].long(), bary[b, :n].double(), torch.from_numpy(w[b, :n]).double(), trunc)
            per.append(S1 / S0 if pr == "mean" else S1)
        per = torch.stack(per)
        r = per.sum() if br == "sum" else per.sum() / B if br == "mean" else per
        rv, rp = torch.autograd.grad(r, (v6, p6), go.cpu().double())
        rel = lambda a, x: float((a.detach().cpu().double() - x).abs().max() / x.abs().max())
        assert rel(loss, r.detach()) < 1e-5 and rel(gv, rv) < 1e-5 and rel(gp, rp) < 1e-5, (pr, br)
        assert (gp[1, lengths[1]:] == 0).all()


# --------------------------------------------------------------------------------------------- the refinement
def _init(p):
    return dict(pose=p[:, :72], beta=p[:, 72:82], trans=p[:, 82:85], scale=p[:, 85:])


def _packed(prm):
    return torch.cat([prm["pose"], prm["beta"], prm["trans"], prm["scale"]], 1).cpu().numpy()


@pytest.mark.parametrize("extras", [False, True])
def test_fit_surface_20_iterations_vs_fp64(extras):
    """Every column of loss_trace and the final parameters against the oracle's fp64 run: err <= max(2 ent, 1e-4), ent = the oracle's own fp32
    run, each relative to the largest magnitude of its own column.

    Two trajectories can be compared only while no point switches to another closest LOCATION (or crosses the mask) between them: a point
    near the medial axis of the surface has two closest locations whose squared distances differ by less than 4 d eps, eps ~ 6e-7 m being
    what fp32 skinned vertices resolve, and which one wins is then decided by rounding.  The switch moves the closest point by about
    d theta (theta: the crease angle there), changes that point's share of the gradient accordingly, and Adam carries the difference on
    at about lr per step.  On the crinkled body of the other tests (betas ~ N(0, 1): 3 cm of per-vertex noise on 4 cm edges) at the
    default lr, one such switch (a point 2.9 mm from the surface, its two locations 2.8 mm apart, squared distances 1e-9 m^2 apart,
    iteration 2) moves the final betas by 3.6e-4 with both runs correct: the kernels' parameter gradient is within 1e-6 of fp64 autograd at
    the iterates before and after it (profiles/surface_refine_pins.txt).  This test therefore fits a SMOOTH body (zero betas, pose 0.05
    rad: crease angles ~0.08 rad, a switch moves a closest point by a twelfth of what it does there) at a quarter of the step, which keeps
    what a switch can do well below the tolerance; every kernel and every term of the loss runs."""
    from etch_amd.models.surface_refine import fit_surface
    bm = _body()
    B, n, iters, lr = 2, 300, 20, 5e-3
    truth = _params(B, 61, pose=0.05, beta=0.0)
    pts = _surface_points(bm, _verts64(bm, truth), n, 62, 0.003)
    lengths = [n, 241]
    rng = np.random.default_rng(63)
    p0 = truth.copy()
    p0[:, :72] += 0.03 * rng.standard_normal((B, 72)).astype(np.float32)
    p0[:, 72:82] += 0.05 * rng.standard_normal((B, 10)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, (B, n)).astype(np.float32)
    kw, okw = {}, {}
    if extras:
        vids = rng.choice(bm.num_verts, 30, replace=False)
        mk = (_verts64(bm, truth)[:, vids] + 0.002 * rng.standard_normal((B, 30, 3))).astype(np.float32)
        valid = rng.random((B, 30)) < 0.7
        mk[~valid] = np.nan                                                    # an invalid marker's position is never read
        # precisions x 1e6: the 1e-7-weighted prior is O(0.1) in the loss and visible in the gradient; a skew part checks 0.5 (P + P^T) d
        prior = CO.random_prior(64, prec_scale=1e6, skew=0.2)
        kw = dict(markers=mk, valid=valid, marker_vids=vids, prior=prior)
        okw = dict(markers=(vids, np.nan_to_num(mk), valid), prior=prior)
    _, prm = fit_surface(bm, _dev(pts), _init(p0), weights=w, lengths=lengths, iterations=iters, lr=lr, want_trace=True, **kw)
    tr, pg = prm["loss_trace"].cpu().numpy(), _packed(prm)
    assert tr.shape == (B, iters, 4)
    t64, p64 = O.fit_surface(bm, pts, lengths, p0, iters, lr, weights=w, dtype=torch.float64, **okw)
    t32, p32 = O.fit_surface(bm, pts, lengths, p0, iters, lr, weights=w, dtype=torch.float32, **okw)
    cols = [(f"trace[{q}]", tr[:, :, q], t64[:, :, q], t32[:, :, q]) for q in range(4) if extras or q in (0, 2)]     # every term by its own scale
    for name, got, r64, r32 in cols + [("params", pg, p64, p32)]:
        s = np.abs(r64).max()
        err, ent = np.abs(got - r64).max() / s, np.abs(r32 - r64).max() / s
        print(f"PIN fit_surface {name} extras={extras}: err {err:.3e}, ent {ent:.3e}")
        assert err <= max(2 * ent, 1e-4), (name, err, ent)
    assert (pg[:, -1] == p0[:, -1]).all()                                          # scale stays where it started
    # the loss of the last forward is the last row of the trace, per scan and summed
    last = tr[:, -1].astype(np.float64).sum(1)
    assert np.abs(prm["loss_per_scan"].cpu().numpy() - last).max() <= 1e-6 * np.abs(last).max()
    assert abs(float(prm["loss"]) - last.sum()) <= 1e-6 * abs(last.sum())
    assert (tr[:, :, 1] > 0).all() == extras and (tr[:, :, 3] != 0).all() == extras and (tr[:, :, 0] > 0).all() and (tr[:, :, 2] > 0).all()
    if extras:                                                                     # the comparison can see the markers and the prior
        _, p64n = O.fit_surface(bm, pts, lengths, p0, iters, lr, weights=w, dtype=torch.float64)
        assert np.abs(pg - p64n).max() / np.abs(p64n).max() > 100 * max(2 * ent, 1e-4)


@functools.lru_cache(maxsize=None)
def _recovery():
    """N = 400 points on the true surface with 1 mm noise, the dense term only, 150 iterations from the truth with 0.03 rad added to every pose
    component, 0.3 to every beta and 1 cm to every translation component (a coherent error: the rotations add up along the kinematic chains,
    4.4 - 6.5 cm per vertex at the start); two runs of the batch and scan 1 alone."""
    from etch_amd.models.surface_refine import fit_surface
    bm = _body()
    B, n = 2, 400
    truth = _params(B, 71, pose=0.3)
    vt = _verts64(bm, truth)
    pts = _surface_points(bm, vt, n, 72, 0.001)
    p0 = truth.copy()
    p0[:, :72] += 0.03
    p0[:, 72:82] += 0.3
    p0[:, 82:85] += 0.01
    pd = _dev(pts)
    run = lambda p, q: fit_surface(bm, p, _init(q), iterations=150, w_beta=0.0, want_trace=True)
    return bm, vt, pd, p0, run(pd, p0), run(pd, p0), run(pd[1:2].contiguous(), p0[1:2])


def test_fit_surface_is_deterministic():
    _, _, _, _, (v1, prm1), (v2, prm2), (v3, prm3) = _recovery()
    assert np.array_equal(v1, v2) and torch.equal(prm1["loss_trace"], prm2["loss_trace"])              # two runs: bitwise
    assert np.array_equal(v1[1], v3[0]) and torch.equal(prm1["loss_trace"][1], prm3["loss_trace"][0])  # scan b alone: bitwise
    tr = prm1["loss_trace"].cpu().numpy()
    assert (tr[:, -1, 0] < tr[:, 0, 0]).all() and np.isfinite(v1).all()


def test_fit_surface_recovers_a_known_body():
    """The mean squared distance falls at least tenfold and the mean per-vertex error at least halves.  tests/_surface_oracle.py in fp64 on
    the CPU, same start: rms distance 23.5 / 22.5 mm -> 2.48 / 3.08 mm (mean d2 x 89.5 / 53.3), per-vertex error 61.4 / 61.4 mm -> 13.7 /
    15.5 mm (x 4.49 / 3.96); with truth poses of 0.2 rad or another seed it gives x 29 - 154 and x 2.2 - 12.6.  From offsets drawn at
    random with these magnitudes (2.6 cm per vertex at the start, no coherent part) the same restatement gives only x 1.6 - 37 and
    x 0.8 - 6.3: the conditions belong to the coherent start.  The MI355X figures are in profiles/surface_refine_pins.txt."""
    from etch_amd import ops
    bm, vt, pd, p0, (v1, _), _, _ = _recovery()
    v0 = _verts64(bm, p0)
    f = _dev(bm.faces)
    d2_0 = ops.point_mesh_closest(pd, _dev(v0.astype(np.float32)), f)[2].double().mean(1).cpu().numpy()
    d2_1 = ops.point_mesh_closest(pd, _dev(v1), f)[2].double().mean(1).cpu().numpy()
    e0, e1 = np.linalg.norm(v0 - vt, axis=-1).mean(1), np.linalg.norm(v1 - vt, axis=-1).mean(1)
    print("PIN fit_surface recovery: rms distance mm", np.sqrt(d2_0) * 1e3, "->", np.sqrt(d2_1) * 1e3, "(mean d2 x", d2_0 / d2_1,
          "); per-vertex error mm", e0 * 1e3, "->", e1 * 1e3, "(x", e0 / e1, ")")
    assert (d2_1 * 10 <= d2_0).all() and (e1 * 2 <= e0).all(), (d2_0, d2_1, e0, e1)


def test_argument_checks():
    from etch_amd import _lib, ops
    from etch_amd.models.surface_refine import fit_surface, point_mesh_face_distance
    bm = _body()
    p = _dev(np.zeros((2, 10, 3), np.float32))
    v = _dev(np.zeros((2, bm.num_verts, 3), np.float32))
    with pytest.raises(_lib.EtchHipError):
        ops.point_mesh_closest(p, v[:1].contiguous(), _dev(bm.faces))
    with pytest.raises(ValueError):
        point_mesh_face_distance(v, bm.faces, p, point_reduction="max")
    with pytest.raises(ValueError):
        fit_surface(bm, p, _init(_params(2, 1)), markers=np.zeros((2, 3, 3), np.float32))         # markers without their mask and ids
    # no usable point (all beyond trunc) and no marker: those terms and their gradients are 0, the parameters move by the regulariser only
    far = _dev(np.full((1, 5, 3), 50.0, np.float32))
    _, prm = fit_surface(bm, far, _init(_params(1, 2)), iterations=2, want_trace=True)
    tr = prm["loss_trace"].cpu().numpy()
    assert (tr[:, :, 0] == 0).all() and (tr[:, :, 1] == 0).all() and np.isfinite(_packed(prm)).all()
    assert torch.equal(prm["pose"].cpu(), torch.from_numpy(_params(1, 2)[:, :72]))


def test_cli_surface_refine(tmp_path):
    import types

    from etch_amd import constants as K
    from etch_amd import inference_demo as D
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded

    rng = np.random.default_rng(3)
    obj = tmp_path / "scan.obj"
    v = rng.standard_normal((400, 3)) * np.array([0.15, 0.45, 0.1]) + np.array([0.3, 1.0, -0.2])
    f = rng.integers(0, 400, (700, 3))
    obj.write_text("".join("v %f %f %f\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    a = types.SimpleNamespace(output_folder=str(tmp_path / "ckpt_model"), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device(DEV),
                              markerset=K.default_markerset(), scale_magnitude=10, body_model=None)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({k: v.cpu() for k, v in load_seeded(GT_network_equiv(option=a), 1).state_dict().items()}, ckpt)
    outs = {}
    for name, extra in (("plain", []), ("none", ["--chamfer_refine", "none"]), ("surface", ["--surface_refine", "--surface_iters", "5"])):
        out = tmp_path / name
        D.main(["--scan_path", str(obj), "--synthetic_body", "--output_folder", str(out), "--num_point", "1024", "--markerset_path", "missing.json",
                "--model_path", str(ckpt)] + extra)
        outs[name] = ((out / "scan_pred_smpl.obj").read_bytes(), (out / "scan_output_smpl_info.npz").read_bytes())
    assert outs["plain"] == outs["none"]
    lines = outs["plain"][0].split(b"\n")
    assert len([l for l in lines if l.startswith(b"v ")]) == 6890 and [l for l in lines if l.startswith(b"f ")][0] == b"f 1 2 3"   # the strip body
    z = np.load(tmp_path / "surface" / "scan_output_smpl_info.npz")
    assert "scale" in z.files and z["joints"].shape == (45, 3) and np.isfinite(z["joints"]).all() and np.isfinite(z["betas"]).all()
    lines = outs["surface"][0].split(b"\n")
    assert len([l for l in lines if l.startswith(b"v ")]) == 6890 and len([l for l in lines if l.startswith(b"f ")]) == 13776
    with pytest.raises(SystemExit):
        D.main(["--scan_path", str(obj), "--synthetic_body", "--surface_refine", "--chamfer_refine", "both"])


def test_eval_surface_refine_fits_mixed_genders():
    """eval --surface_refine: the per-gender marker fit followed by fit_surface, in fit_smpl's return layout for the whole batch."""
    import types

    from etch_amd import constants as K
    from etch_amd import eval as E
    from etch_amd.models.fit_SMPL import fit_smpl
    from etch_amd.utils.body_model import SyntheticSurfaceSMPL
    from oracle import stage2 as S2

    bm = SyntheticSurfaceSMPL(7)
    ms = K.default_markerset()
    vids = np.array(list(ms.values()))
    args = types.SimpleNamespace(markerset=ms, body_model={"male": bm, "female": bm}, surface_refine=True, surface_iters=3)
    B, n = 3, 1024
    truth = _params(B, 91, pose=0.1, beta=0.3)
    vt = CO.forward(S2.TorchBody(bm, torch.float64), torch.from_numpy(truth).double(), 24, 10)[0].numpy()
    pts = _surface_points(bm, vt, n, 92, 0.002)
    labels = np.stack([((pts[b][:, None] - vt[b][vids][None]) ** 2).sum(-1).argmin(1) for b in range(B)])
    conf = np.random.default_rng(93).uniform(0.6, 1.0, (B, n)).astype(np.float32)
    inner, lab, cf = _dev(pts), _dev(labels.astype(np.int64)), _dev(conf)
    genders = ["male", "female", "male"]
    from etch_amd.inference_demo import surface_refine_settings
    settings = surface_refine_settings(args)
    assert settings == dict(iterations=3, trunc=0.05, w_dense=1e2)
    meshes, markers, valid, info = E.surface_refine_fits(args, settings, inner, lab, cf, genders)
    assert len(meshes) == B and all(m.vertices.shape == (6890, 3) and m.faces.shape == (13776, 3) and np.isfinite(m.vertices).all() for m in meshes)
    assert markers.shape == (B, len(ms), 3) and valid.shape == (B, len(ms)) and bool(valid.any(1).all())
    assert [a.shape for a in info] == [(B, 23, 3), (B, 10), (B, 3), (B, 3), (B, 45, 3)] and all(np.isfinite(a).all() for a in info)
    # scan 1 ("female") alone through the same path is bitwise scan 1 of the mixed batch, and the refinement moved the marker fit
    one, _, _, inf1 = E.surface_refine_fits(args, settings, inner[1:2].contiguous(), lab[1:2].contiguous(), cf[1:2].contiguous(), ["female"])
    assert np.array_equal(one[0].vertices, meshes[1].vertices) and all(np.array_equal(a[0], b[1]) for a, b in zip(inf1, info))
    plain = fit_smpl(args, inner[1:2].contiguous(), lab[1:2].contiguous(), cf[1:2].contiguous(), "female")[0][0]
    assert np.abs(plain.vertices - meshes[1].vertices).max() > 1e-4
