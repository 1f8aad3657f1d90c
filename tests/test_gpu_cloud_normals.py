"""Raw-cloud normals and the point-to-plane registration on the GPU.  csrc/cloud_normals.hip against tests/_normals_oracle.py:
the neighbour sets (through the covariance) and the flags by bits in every form, the normal against numpy's eigh within the Jacobi's backward
error, the two sign rules, the status and the argument checks.  The plane step of csrc/cloud_align.hip against tests/_plane_oracle.py: one step
from given pairs within derived bounds, the loop on the exact-copy, partial-overlap and sampled-surface cases, register_views and the command.
Clouds of at most 12 000 points."""
import os
import types

import numpy as np
import pytest
import torch

import _align_oracle as AO
import _cloud_oracle as CO
import _normals_oracle as NO
import _plane_oracle as PO
import _train_data
from etch_amd import _lib, cloud

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = NO.U
CELLS = (0.07, 1.3)
# tests/test_normals_host.py derives it: at most 30 rotations of backward error 8 u |C|_F each, and 16 for the normalisation and the reference
C_JACOBI = 256.0


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


@pytest.fixture(scope="module")
def batch():
    """One packed batch, left unchanged: the body's vertices, the stray fixture (far points: the whole-cloud scan), two lattices scaled by 2^-4 (ties
    in d2 everywhere: the tie rule decides the set), collinear rows, and clouds of 3, 2, 1 and 0 rows (ke < k, FEW, empty).  With every cloud's
    32 nearest rows from the oracle, of which a smaller k takes a prefix."""
    rng = np.random.default_rng(7)
    clouds = [CO.body_vertices(), CO.stray_fixture()[0], NO.lattice(7, 7, 1), NO.lattice(5, 5, 5), NO.collinear(9), rng.standard_normal((3, 3)),
              rng.standard_normal((2, 3)), rng.standard_normal((1, 3)), np.zeros((0, 3))]
    return clouds, [NO.neighbours(p, 32) for p in clouds], cloud.pack(clouds, device=DEV)


def _split(values, clouds):
    o = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    v = _np(values)
    assert len(v) == o[-1]
    return [v[a:b] for a, b in zip(o[:-1], o[1:])]


@pytest.mark.parametrize("k", [3, 16, 32])
def test_normals_equal_the_oracle_in_every_form(batch, k):
    clouds, nbrs, packed = batch
    got = cloud.normals(packed, k=k, return_cov=True)
    for kw in [dict(cell=c) for c in CELLS] + [dict(brute=True)]:
        other = cloud.normals(packed, k=k, return_cov=True, **kw)
        for a, b, name in zip(got, other, ("normal", "variation", "flag", "cov")):
            assert _same(a, b), (kw, name)
    normal, variation, flag, cov = (_split(x, clouds) for x in got)
    worst_angle = worst_res = 0.0
    for c, (p, nbr) in enumerate(zip(clouds, nbrs)):
        onrm, ovar, oflag, ocov, _ = NO.normals(p, k, nbr=nbr)
        assert _same(cov[c], ocov), f"cloud {c}: covariance (the neighbour sets)"
        assert np.array_equal(flag[c], oflag), f"cloud {c}: flags"
        assert (normal[c][flag[c] != 0] == 0).all()
        ok = flag[c] == 0
        if not ok.any():
            continue
        n = normal[c][ok]
        assert (np.abs(np.sqrt((n * n).sum(1)) - 1.0) <= 4 * U).all()
        lead = n[np.arange(len(n)), np.abs(n).argmax(1)]
        assert (lead > 0).all()
        lam, vec, a = NO.eigh_reference(cov[c][ok])
        norm = np.sqrt((a * a).sum((1, 2)))
        res = np.sqrt(((np.einsum("nij,nj->ni", a, n) - lam[:, :1] * n) ** 2).sum(1))
        sin = np.sqrt((np.cross(n, vec) ** 2).sum(1))
        gap = lam[:, 1] - lam[:, 0]
        worst_res, worst_angle = max(worst_res, (res / (U * norm)).max()), max(worst_angle, (sin * gap / (U * norm)).max())
        assert (res <= C_JACOBI * U * norm).all() and (sin <= C_JACOBI * U * norm / gap).all(), (c, worst_res, worst_angle)
        tr = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        assert (np.abs(variation[c][ok] - lam[:, 0] / tr) <= 2 * C_JACOBI * U * norm / tr).all()
    print(f"k={k}: worst residual / (u |C|_F) = {worst_res:.3g}, worst sin(angle) gap / (u |C|_F) = {worst_angle:.3g}, bound {C_JACOBI}")
    # what the fixtures are there for
    assert (flag[2] == 0).all() and (normal[2] == [0.0, 0.0, 1.0]).all()                                # the lattice plane: exact
    assert (flag[4] == NO.FLAG_AMBIGUOUS).all()                                                         # collinear
    assert (flag[5] == 0).all() and (flag[6] == 3).all() and (flag[7] == 3).all()                       # 3, 2 and 1 rows
    if k == 32:
        assert flag[3][(2 * 5 + 2) * 5 + 2] == NO.FLAG_AMBIGUOUS                                       # the 5^3 lattice's centre: isotropic


def test_sign_rules(batch):
    clouds, nbrs, packed = batch
    plain = _split(cloud.normals(packed, k=16)[0], clouds)
    view = np.zeros((len(clouds), 3))
    view[0], view[1] = [0.3, 0.2, 4.0], [-3.0, 0.5, 0.1]
    view[2] = [5.0, -3.0, 0.0]                                            # in the lattice plane: n.(v - p) is exactly 0, the first rule stays
    view[3] = [0.1, 0.1, -2.0]
    normal, variation, flag = cloud.normals(packed, k=16, viewpoint=view)
    for kw in (dict(brute=True), dict(cell=CELLS[0])):
        assert _same(cloud.normals(packed, k=16, viewpoint=view, **kw)[0], normal)
    normal = _split(normal, clouds)
    for c in (0, 1, 3):
        s = (normal[c] * (view[c] - clouds[c])).sum(1)
        assert (s >= 0).all() and (np.abs(normal[c]) == np.abs(plain[c])).all()
        onrm = NO.normals(clouds[c], 16, viewpoint=view[c], nbr=nbrs[c])[0]
        assert np.array_equal(np.sign(normal[c]), np.sign(onrm))
        assert (normal[c] != plain[c]).any()
    assert (normal[2] == [0.0, 0.0, 1.0]).all()
    under = view.copy()
    under[2] = [0.1, 0.1, -2.0]
    assert (_split(cloud.normals(packed, k=16, viewpoint=under)[0], clouds)[2] == [0.0, 0.0, -1.0]).all()
    one = cloud.normals(packed, k=16, viewpoint=[0.3, 0.2, 4.0])[0]       # one position for every cloud
    assert _same(_split(one, clouds)[0], normal[0])


def test_non_finite_row_raises_naming_its_cloud_and_bad_arguments_raise(batch):
    clouds, _, packed = batch
    bad = [c.copy() for c in clouds]
    bad[3][17, 1] = np.nan
    with pytest.raises(_lib.EtchHipError, match="cloud 3"):
        cloud.normals(cloud.pack(bad, device=DEV), k=16)
    bad[3][17, 1] = np.inf
    with pytest.raises(_lib.EtchHipError, match="cloud 3"):
        cloud.normals(cloud.pack(bad, device=DEV), k=8, brute=True)
    for kw in (dict(k=2), dict(k=33), dict(k=16.5), dict(k=0), dict(cell=0.0), dict(cell=float("nan")), dict(viewpoint=np.zeros((2, 3))),
               dict(viewpoint=np.zeros(4)), dict(viewpoint=np.zeros((len(clouds), 3, 1))), dict(viewpoint=[np.nan, 0.0, 0.0])):
        with pytest.raises(ValueError):
            cloud.normals(packed, **kw)
    from etch_amd import ops
    with pytest.raises(_lib.EtchHipError, match="3 .. 32"):
        ops.cloud_normals(packed.points, packed.offsets, 2)
    with pytest.raises(_lib.EtchHipError, match="viewpoint"):
        ops.cloud_normals(packed.points, packed.offsets, 16, viewpoint=torch.zeros((2, 3), dtype=torch.float64, device=DEV))


# ---- the point-to-plane step from given pairs -----------------------------------------------------------------------------------------------------------
def _step_cases(batch):
    """(name, source, target, target normals, pair, R, t, degenerate): the step cases of test_gpu_cloud_align.py (its clouds, built the same way)
    with normals, and cases where some or all target normals are zero."""
    rng = np.random.default_rng(11)
    [rng.standard_normal(s) for s in ((256, 3), (1, 3), (9, 3), (33, 3))]                     # the draws in front of r257 there
    nine = np.random.default_rng(5).standard_normal((9, 3))
    q = rng.standard_normal((257, 3)) * [0.2, 0.5, 0.1] + [5.0, -3.0, 0.5]                     # centred at (5, -3, 0.5): the centring is exercised
    nq = NO.normals(q, 8)[0]
    rng = np.random.default_rng(29)
    p = AO.displaced(q, 20.0, 0.1)[0] + rng.standard_normal((257, 3)) * 1e-3
    pair = np.arange(257, dtype=np.int32)
    pair[::7] = -1
    src, tgt = AO.exact_copy_case()
    nbody = NO.normals(tgt, 16, nbr=batch[1][0])[0]                                            # the body's vertices are the batch's cloud 0
    Rb, tb = AO.start_pose(3.0, 0.01)
    flat = q.copy()
    flat[:, 2] = 0.5
    nflat = NO.normals(flat, 8)[0]
    assert (nflat == [0.0, 0.0, 1.0]).all()
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    eye, zero = np.eye(3), np.zeros(3)
    two = np.full(257, -1, np.int32)
    two[[5, 9]] = [5, 9]
    some = nq.copy()
    some[::5] = 0.0
    return [("offset cloud", p, q, nq, pair, eye, zero, False),
            ("body", AO.displaced(src, 5.0, 0.02)[0], tgt, nbody, (2 * np.arange(3445)).astype(np.int32), Rb, tb, False),
            ("exact plane, exact normals", AO.displaced(flat, 20.0, 0.1)[0], flat, nflat, np.arange(257, dtype=np.int32), eye, zero, True),
            ("collinear", AO.displaced(line, 20.0, 0.1)[0], line, np.tile([0.0, 0.6, 0.8], (3, 1)), np.arange(3, dtype=np.int32), Rb, tb, True),
            ("two pairs", p, q, nq, two, Rb, tb, True), ("no pair", nine, nine, np.tile([1.0, 0.0, 0.0], (9, 1)), np.full(9, -1, np.int32), Rb, tb, True),
            ("some normals zero", p, q, some, pair, eye, zero, False), ("all normals zero", p, q, np.zeros((257, 3)), pair, Rb, tb, True)]


def test_one_plane_step_from_given_pairs_within_the_derived_bounds(batch):
    """Sums: the same terms as the oracle's in another order, within m u sum|term| of math.fsum (test_gpu_cloud_align.py states why).  Solve: in
    the scaled unknowns z = y / D both sides solve Abar z = -gbar from sums that differ by at most that bound, dA and dg; to first order
    |dz| / |z| <= cond (|dA|_F / |Abar|_2 + |dg| / |gbar|), doubled for the two sides, and 128 u cond covers the two solvers' own backward
    error (tests/test_normals_host.py)."""
    from etch_amd import ops
    cases = _step_cases(batch)
    s, t = cloud.pack([c[1] for c in cases], DEV), cloud.pack([c[2] for c in cases], DEV)
    tn = torch.from_numpy(np.concatenate([c[3] for c in cases])).to(DEV)
    pair = torch.from_numpy(np.concatenate([c[4] for c in cases])).to(DEV)
    R = torch.from_numpy(np.stack([c[5] for c in cases])).to(DEV)
    tt = torch.from_numpy(np.stack([c[6] for c in cases])).to(DEV)
    dR, dt, m, sums, y, status, Rn, tnew = (_np(x) for x in ops.cloud_align_step_plane(s.points, s.offsets, t.points, t.offsets, tn, pair, R=R, t=tt))
    for b, (name, p, q, nq, pr, R0, t0, degenerate) in enumerate(cases):
        w = PO.step(p, q, nq, pr, R0, t0)
        assert m[b] == w["m"] == ((pr >= 0) & (nq[np.maximum(pr, 0)] != 0).any(1)).sum(), name
        err, bound = np.abs(sums[b] - w["sums"]), w["m"] * U * w["abs_sums"]
        print(f"PIN plane step {name}: m {m[b]}, worst sum error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (name, err, bound)
        assert bool(status[b] & cloud.STATUS_DEGENERATE) == degenerate == (not w["ok"]), (name, status[b])
        if degenerate:
            assert _same(Rn[b], R0) and _same(tnew[b], t0) and np.array_equal(dR[b], np.eye(3)) and not dt[b].any() and not y[b].any(), name
            continue
        mm = w["m"]
        Abar, gbar, D = PO.scaled_system(mm, w["sums"], w["rho"])
        dA, dg, _ = PO.scaled_system(mm, bound, w["rho"])
        rel = 2.0 * w["cond"] * (np.sqrt((dA * dA).sum()) / np.linalg.norm(Abar, 2) + np.sqrt((dg * dg).sum()) / np.sqrt((gbar * gbar).sum())) + 128 * U * w["cond"]
        z, oz = y[b] / D, w["y"] / D
        got = np.sqrt(((z - oz) ** 2).sum()) / np.sqrt((oz * oz).sum())
        print(f"PIN plane step {name}: cond {w['cond']:.3g}, |z - z_oracle| / |z| {got:.3e}, bound {rel:.3e}")
        assert got <= rel, (name, got, rel)
        assert abs(np.linalg.det(dR[b]) - 1.0) <= 16 * U and np.abs(dR[b].T @ dR[b] - np.eye(3)).max() <= 16 * U, name
        assert np.abs(dR[b] - PO.quat_rotation(y[b, :3])).max() <= 16 * U, name
        x_g, x_w = AO.apply(Rn[b], tnew[b], p), AO.apply(w["R"], w["t"], p)
        reach = float(np.abs(np.concatenate([p, q])).max())
        zn = float(np.sqrt((oz * oz).sum()))                                        # |d omega| <= rel |z| / rho, |d tau| <= rel |z|
        assert np.abs(x_g - x_w).max() <= 2.0 * rel * zn * (reach / w["rho"] + 1.0) + 64 * U * reach, name


def test_sixty_composed_plane_steps_stay_a_rotation(batch):
    """The bound of test_gpu_cloud_align.py's test: dR is the matrix of a normalised quaternion, orthogonal to 8 u whatever the data, and one
    composition adds at most 32 u to the defect of R^T R."""
    from etch_amd import ops
    rng = np.random.default_rng(31)
    p = _step_cases(batch)[0][2]
    n = NO.normals(p, 8)[0]
    s = cloud.pack([p], DEV)
    pair = torch.arange(257, dtype=torch.int32, device=DEV)
    R, t = torch.eye(3, dtype=torch.float64, device=DEV)[None], torch.zeros((1, 3), dtype=torch.float64, device=DEV)
    Rw, tw = np.eye(3), np.zeros(3)
    for k in range(60):
        Rk, tk = AO.rotation(rng.standard_normal(3), 7.0 + 4.0 * rng.random()), rng.standard_normal(3) * 0.05
        Rw, tw = Rk @ Rw, Rk @ tw + tk
        q = cloud.pack([AO.apply(Rw, tw, p)], DEV)
        nq = torch.from_numpy(np.ascontiguousarray(n @ Rw.T)).to(DEV)
        _, _, m, _, _, status, R, t = ops.cloud_align_step_plane(s.points, s.offsets, q.points, q.offsets, nq, pair, R=R, t=t)
    Rg = _np(R)[0]
    det, orth = abs(np.linalg.det(Rg) - 1.0), float(np.abs(Rg.T @ Rg - np.eye(3)).max())
    print(f"PIN 60 composed plane steps: det R - 1 {det:.3e}, max |R^T R - I| {orth:.3e}, bound {60 * 32 * U:.3e}; {AO.angle_between(Rg, Rw):.3e} deg from the truth")
    assert int(m[0]) == 257 and int(status[0]) == 0 and det <= 60 * 32 * U and orth <= 60 * 32 * U


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------------------
def _loop(name, moved, tgt, nq, R0, t0, **kw):
    """The GPU loop with the oracle's normals handed in, against the oracle's loop: same steps and matched; the poses agree within the step bound
    compounded -- every step's solve agrees within 256 u cond relative (above), the steps are at most 1 in the scaled unknowns."""
    w = PO.align(moved, tgt, nq, **kw)
    s, t = cloud.pack([moved], DEV), cloud.pack([tgt], DEV)
    res = cloud.align(s, t, metric="plane", normals=nq, **kw)
    R, tt = _np(res.R)[0], _np(res.t)[0]
    reach = float(np.abs(np.concatenate([moved, tgt])).max())
    diff = float(np.abs(AO.apply(R, tt, moved) - AO.apply(w["R"], w["t"], moved)).max())
    bound = w["steps"] * 256 * U * w["cond"] * reach
    print(f"PIN plane loop {name}: {res.steps[0]} steps (oracle {w['steps']}), {res.matched[0]} matched (oracle {w['matched']}), rms {res.rms[0]:.3e} m, "
          f"moved rows differ from the oracle's by {diff:.3e} m, bound {bound:.3e}; {PO.row_error(moved, R, tt, R0, t0):.3e} m from the truth "
          f"(oracle {PO.row_error(moved, w['R'], w['t'], R0, t0):.3e})")
    assert res.steps[0] == w["steps"] and res.matched[0] == w["matched"] and res.status[0] == w["status"] == 0
    assert diff <= bound
    brute = cloud.align(s, t, metric="plane", normals=nq, brute=True, **kw)
    assert _same(brute.R, res.R) and _same(brute.t, res.t) and _same(brute.pair, res.pair) and brute.steps[0] == res.steps[0] and brute.matched[0] == res.matched[0]
    return res, w


def test_the_plane_loop_on_the_exact_copy_and_partial_overlap_cases(batch):
    nbr = batch[1][0]
    src, tgt = AO.exact_copy_case()
    moved, R0, t0 = AO.displaced(src, 10.0, 0.05)
    res, w = _loop("exact copy", moved, tgt, NO.normals(tgt, 16, nbr=nbr)[0], R0, t0)
    assert res.steps[0] < 40 and res.rms[0] < 1e-9
    src, tgt = AO.partial_case()
    moved, R0, t0 = AO.displaced(src, 10.0, 0.05)
    _loop("partial overlap", moved, tgt, NO.normals(tgt, 16)[0], R0, t0, gate=0.2, gate_min=0.01, decay=0.85, iters=60)


def test_the_plane_loop_on_two_samplings_of_the_surface():
    """4 000 rows against 12 000, 10 deg / 5 cm, 8 steps: the GPU's largest row error to the truth is at most 1.5 x the oracle's.  A pair that flips
    at rounding level changes the path, but moves the pose by far less than the sampling distance."""
    p, q = PO.sampled_case()
    nq = NO.normals(q, 16, nbr=NO.neighbours_fast(q, 16))[0]
    moved, R0, t0 = AO.displaced(p, 10.0, 0.05)
    w = PO.align(moved, q, nq, iters=8)
    res = cloud.align(cloud.pack([moved], DEV), cloud.pack([q], DEV), iters=8, metric="plane", normal_k=16)
    got, own = PO.row_error(moved, _np(res.R)[0], _np(res.t)[0], R0, t0), PO.row_error(moved, w["R"], w["t"], R0, t0)
    print(f"PIN sampled surface, 8 plane steps from 10 deg / 5 cm: {got:.3e} m from the truth (oracle {own:.3e} m), {res.matched[0]} matched, rms {res.rms[0]:.3e} m")
    assert res.steps[0] == 8 and res.status[0] == 0 and got <= 1.5 * own


# ---- views, arguments, the command ---------------------------------------------------------------------------------------------------------------------
def _view_error(res, k):
    R0, t0 = AO.start_pose(*AO.VIEW_POSES[k])
    return AO.angle_between(_np(res[k].R)[0], R0), float(np.sqrt(((_np(res[k].t)[0] - t0) ** 2).sum()))


def test_register_views_with_the_plane_metric():
    views = AO.three_views()
    moved = [AO.displaced(v, d, s)[0] for v, (d, s) in zip(views, AO.VIEW_POSES)]
    packed = [cloud.pack([m], DEV) for m in moved]
    point = cloud.register_views(packed, **AO.VIEW_SETTINGS)
    plane = cloud.register_views(packed, metric="plane", **AO.VIEW_SETTINGS)
    named = cloud.register_views(packed, metric="point", normal_k=7, **AO.VIEW_SETTINGS)
    for k in (1, 2):
        (a1, s1), (a0, s0) = _view_error(plane, k), _view_error(point, k)
        print(f"PIN view {k}: plane {a1:.3e} deg, {s1:.3e} m from the truth in {plane[k].steps[0]} steps; point {a0:.3e} deg, {s0:.3e} m in {point[k].steps[0]} steps")
        assert a1 <= a0 and s1 <= s0 and plane[k].steps[0] <= point[k].steps[0] and plane[k].status[0] == 0
        assert _same(named[k].R, point[k].R) and _same(named[k].t, point[k].t) and _same(named[k].pair, point[k].pair) and named[k].steps[0] == point[k].steps[0]
    one = cloud.align(packed[1], packed[0], **AO.VIEW_SETTINGS)                                 # the point metric: the path of align as it was
    assert _same(one.R, point[1].R) and _same(one.t, point[1].t)


def test_bad_metric_arguments_raise_before_any_launch(batch):
    nine = cloud.pack([np.random.default_rng(2).standard_normal((9, 3))], DEV)
    for kw, match in ((dict(metric="surface"), "metric must be"), (dict(normals=np.zeros((9, 3))), "metric='point' takes none"),
                      (dict(metric="plane", normals=np.zeros((8, 3))), "normals must be"), (dict(metric="plane", normals=np.zeros((9, 2))), "normals must be"),
                      (dict(metric="plane", normal_k=2), "k must be"), (dict(metric="plane", normal_k=33), "k must be")):
        with pytest.raises(ValueError, match=match):
            cloud.align(nine, nine, **kw)
    with pytest.raises(ValueError, match="metric must be"):
        cloud.register_views([nine, nine], metric="planes")
    with pytest.raises(ValueError, match="k must be"):
        cloud.register_views([nine, nine], metric="plane", normal_k=40)
    from etch_amd import ops
    with pytest.raises(_lib.EtchHipError, match="tgt_normals"):
        ops.cloud_align(nine.points, nine.offsets, nine.points, nine.offsets, [0.2], 0.0, 0.0, tgt_normals=torch.zeros((8, 3), dtype=torch.float64, device=DEV))


@pytest.fixture(scope="module")
def common(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    data = _train_data.build(tmp_path_factory.mktemp("normals_data"), DEV)
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return ["--model_path", path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]


def test_the_command_with_the_plane_metric(common, tmp_path):
    from etch_amd import mesh_io
    views = AO.three_views()
    moved = [AO.displaced(v, d, s)[0] for v, (d, s) in zip(views, AO.VIEW_POSES)]
    for n, m in zip("abc", moved):
        mesh_io.write_ply(m, str(tmp_path / f"{n}.ply"))
    base = ["--cloud_path", str(tmp_path / "a.ply"), "--more_views", str(tmp_path / "b.ply"), str(tmp_path / "c.ply"), "--align_gate_min", "0.01",
            "--align_decay", "0.85", "--align_iters", "60", "--fuse_voxel", "0.005"]
    cloud.main(base + ["--align_metric", "plane", "--align_normal_k", "12", "--output_folder", str(tmp_path / "plane")] + common)
    rep = np.load(tmp_path / "plane" / "a_cloud.npz")
    assert str(rep["view_metric"]) == "plane" and not rep["view_status"].any() and (rep["view_steps"][1:] <= 60).all()
    for k in (1, 2):
        R0, t0 = AO.start_pose(*AO.VIEW_POSES[k])
        assert AO.angle_between(rep["view_pose"][k, :3, :3], R0) < 0.01 and np.abs(rep["view_pose"][k, :3, 3] - t0).max() < 1e-4
    cloud.main(base + ["--output_folder", str(tmp_path / "point")] + common)                    # without the new flags: the point metric, as before
    was = np.load(tmp_path / "point" / "a_cloud.npz")
    res = cloud.register_views([cloud.pack([m], DEV) for m in moved], **AO.VIEW_SETTINGS)
    assert str(was["view_metric"]) == "point" and sorted(set(was.files) - set(rep.files)) == []
    for k in (1, 2):
        assert _same(was["view_pose"][k, :3, :3], res[k].R[0]) and _same(was["view_pose"][k, :3, 3], res[k].t[0]) and was["view_steps"][k] == res[k].steps[0]
    with pytest.raises(SystemExit):
        cloud.parse_args(base + ["--align_metric", "plane", "--align_normal_k", "2"] + common)
