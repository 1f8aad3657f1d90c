"""Registering raw clouds on the GPU: the gated nearest rows of csrc/cloud_align.hip against tests/_align_oracle.py by bits
in every form, one rigid step from given pairs against the oracle's SVD Kabsch within derived bounds, the loop on the fixture body's exact-copy
and partial-overlap cases, register_views / fuse on three displaced views, and the command.  Clouds of at most 6 890 points."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _align_oracle as AO
import _cloud_oracle as CO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"
CELLS = (0.25, 0.07, 1.3)
U = 2.0 ** -53


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _split(values, clouds):
    o = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    v = _np(values)
    assert len(v) == o[-1]
    return [v[a:b] for a, b in zip(o[:-1], o[1:])]


@pytest.fixture(scope="module")
def small():
    """The small clouds of test_gpu_cloud.py, by name, left unchanged."""
    rng = np.random.default_rng(11)
    g = np.arange(-2, 3) * 0.25
    body = rng.standard_normal((256, 3)) * [0.15, 0.4, 0.1]
    ints = np.concatenate([np.stack(np.meshgrid(np.arange(0, 12, 3.0), np.arange(-4, 8, 4.0), [0.0, 5.0], indexing="ij"), -1).reshape(-1, 3),
                           [[3.0, 4.0, 0.0], [-5.0, 0.0, 0.0], [0.0, -3.0, 4.0]]])
    return {"one": rng.standard_normal((1, 3)), "nine": rng.standard_normal((9, 3)), "r33": rng.standard_normal((33, 3)) * [0.2, 0.5, 0.1],
            "r257": rng.standard_normal((257, 3)) * [0.2, 0.5, 0.1] + [5.0, -3.0, 0.5], "copies": np.repeat(rng.standard_normal((1, 3)), 40, 0),
            "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), "body": body,
            "far": np.concatenate([body[:100], [[1000.0, 0.0, 0.0]], body[100:]]), "ints": ints, "empty": np.zeros((0, 3))}


def _pairs(small):
    """(name, source, target, gate) of every nearest case."""
    s = small
    rng = np.random.default_rng(23)
    lat_q = np.concatenate([s["lattice"] + [0.5, -0.25, 0.0], s["lattice"][::3] * -1.0 - [0.0, 0.0, 0.75]])      # on cell walls, half of them outside the box
    ints_q = np.concatenate([s["ints"] + [5.0, 0.0, 0.0], s["ints"] + [0.0, 3.0, 4.0], s["ints"] - [3.0, 4.0, 0.0], s["ints"] * 0.5, [[30.0, 30.0, 30.0], [9.0, 4.0, 10.0 + 1e-9]]])
    cop = s["copies"]
    cop_q = np.concatenate([cop[:2], cop[:3] + [0.1, 0.0, 0.0], cop[:1] + [0.0, 0.4, 0.0]])
    return [("lattice", lat_q, s["lattice"], 0.25), ("ints", ints_q, s["ints"], 5.0), ("far source", s["far"] + [0.01, 0.02, -0.01], s["body"], 0.3),
            ("far target", s["body"][::2] + [0.02, 0.0, 0.01], s["far"], 0.3), ("copies", cop_q, cop, 0.3), ("one", s["nine"], s["one"], 3.0),
            ("nine", s["one"], s["nine"], 3.0), ("empty source", s["empty"], s["nine"], 0.3), ("empty target", s["nine"], s["empty"], 0.3),
            ("r257", s["r257"][::2] + rng.standard_normal((129, 3)) * 0.05, s["r257"], 0.1)]


def _nearest(srcs, tgts, gate, **kw):
    from etch_amd import cloud as C
    return C.nearest(C.pack(srcs, DEV), C.pack(tgts, DEV), gate, **kw)


@pytest.mark.parametrize("gate", [0.25, 0.3, 5.0, 3.0, 0.1])
def test_nearest_equals_the_oracle_by_bits_in_every_form(small, gate):
    cases = [c for c in _pairs(small) if c[3] == gate]
    names, srcs, tgts = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    want = [AO.nearest(p, q, gate) for p, q in zip(srcs, tgts)]
    pair, d2 = _nearest(srcs, tgts, gate)
    assert pair.dtype == torch.int32 and d2.dtype == torch.float64
    for n, gp, gd, (wp, wd) in zip(names, _split(pair, srcs), _split(d2, srcs), want):
        assert np.array_equal(gp, wp) and _same(gd, wd), n
        if n in ("lattice", "ints"):
            assert (wd == gate * gate).sum() >= 3 and (wp == -1).any(), n                  # rows exactly on the gate, rows without a partner
        if n == "copies":
            assert wp.tolist() == [0, 0, 0, 0, 0, -1]                                       # forty coincident rows: the lowest
        if n == "far source":
            assert wp[100] == -1 and (wp >= 0).sum() >= 200
        if n == "empty target":
            assert (wp == -1).all() and np.isinf(wd).all()
    for kw in [dict(cell=c) for c in CELLS] + [dict(brute=True)]:
        gp, gd = _nearest(srcs, tgts, gate, **kw)
        assert _same(gp, pair) and _same(gd, d2), kw                                        # the same bits for any cell size and from the whole scan
    for n, p, q, gp, gd in zip(names, srcs, tgts, _split(pair, srcs), _split(d2, srcs)):     # a pair alone = the same pair in the batch
        ap, ad = _nearest([p], [q], gate)
        assert _same(ap, gp) and _same(ad, gd), n
    rev = _nearest(srcs[::-1], tgts[::-1], gate)[0]
    assert _same(np.concatenate(_split(rev, srcs[::-1])[::-1]), pair)


def test_nearest_under_a_transform_and_on_the_body(small):
    R0, t0 = AO.start_pose(20.0, 0.1)
    R1, t1 = AO.start_pose(-35.0, 0.4)
    src, tgt = AO.partial_case()
    moved = AO.displaced(src, 20.0, 0.1)[0]
    srcs, tgts = [moved, AO.displaced(small["r257"][::2], -35.0, 0.4)[0], small["nine"]], [tgt, small["r257"], small["one"]]
    Rs, ts = np.stack([R0, R1, R1]), np.stack([t0, t1, t1])
    for gate in (0.2, 0.02):
        want = [AO.nearest(p, q, gate, R, t) for p, q, R, t in zip(srcs, tgts, Rs, ts)]
        pair, d2 = _nearest(srcs, tgts, gate, R=Rs, t=ts)
        for gp, gd, (wp, wd) in zip(_split(pair, srcs), _split(d2, srcs), want):
            assert np.array_equal(gp, wp) and _same(gd, wd)
        assert 0 < (want[0][0] >= 0).sum() < len(moved)                                     # a partial overlap: some rows have no partner
        for kw in (dict(cell=0.013), dict(cell=0.3), dict(brute=True)):
            gp, gd = _nearest(srcs, tgts, gate, R=Rs, t=ts, **kw)
            assert _same(gp, pair) and _same(gd, d2), kw
        a = _nearest(srcs[:1], tgts[:1], gate, R=Rs[:1], t=ts[:1])
        assert _same(a[0], _split(pair, srcs)[0]) and _same(a[1], _split(d2, srcs)[0])


def test_the_default_cell_puts_the_last_ring_beyond_the_gate(small):
    """A row without a partner inside the gate must end its ring walk by lim^2 > g^2, not fall through to the whole-cloud scan.  Both give the
    same bits, so the result cannot show which ran: the check is the kernel's own arithmetic on the grid's h.  At 2 m and 7 m the gate term of
    the cell rule wins, as it does at 20 cm on clouds of 300 000 rows."""
    from etch_amd import cloud as C
    from etch_amd import _lib, ops
    rings = 8
    assert f"#define ETCH_ALIGN_MAX_RINGS {rings} " in open(_lib.HEADER).read()
    tgt = AO.partial_case()[1]
    t = C.pack([tgt, small["r257"], small["nine"], small["one"]], DEV)
    for gate in (0.02, 0.2, 2.0, 7.0):
        h = _np(ops.cloud_align_grid(t.points, t.offsets, gate, sort=False)[0])[:, 3]
        lim = (float(rings) * h) * (1.0 - 2.0 ** -20)
        assert (lim * lim > gate * gate).all(), (gate, h)
        if gate >= 2.0:
            assert h[0] == gate / (rings - 1)                                               # 4 057 rows: the gate term wins
        away = [tgt[::3] + [100.0, 0.0, 0.0], small["r257"] + [0.0, -50.0, 3.0], small["nine"], small["nine"]]
        pair, d2 = C.nearest(C.pack(away, DEV), t, gate)
        want = [AO.nearest(p, q, gate) for p, q in zip(away, [tgt, small["r257"], small["nine"], small["one"]])]
        assert np.array_equal(_np(pair), np.concatenate([w[0] for w in want])) and _same(d2, np.concatenate([w[1] for w in want]))
        assert (_np(pair)[:len(away[0]) + 257] == -1).all()


def test_non_finite_rows_raise_naming_the_cloud(small):
    from etch_amd import _lib
    bad = small["nine"].copy()
    bad[4, 1] = np.nan
    with pytest.raises(_lib.EtchHipError, match="nearest: cloud 1: a coordinate is not finite"):
        _nearest([small["r33"], bad], [small["r33"], small["nine"]], 0.3)
    with pytest.raises(_lib.EtchHipError, match="nearest: cloud 1: a coordinate is not finite"):
        _nearest([small["r33"], small["nine"]], [small["r33"], bad], 0.3, brute=True)
    from etch_amd import cloud as C
    bad[4, 1] = np.inf
    with pytest.raises(_lib.EtchHipError, match="align: cloud 0: a coordinate is not finite"):
        C.align(C.pack([bad], DEV), C.pack([small["nine"]], DEV), iters=3)


# ---- one step from given pairs ------------------------------------------------------------------------------------------------------------------------

def _step_cases(small):
    """(name, source, target, pair, R, t, degenerate)."""
    rng = np.random.default_rng(29)
    q = small["r257"]                                                                      # centred at (5, -3, 0.5): the centring is exercised
    p = AO.displaced(q, 20.0, 0.1)[0] + rng.standard_normal((257, 3)) * 1e-3
    pair = np.arange(257, dtype=np.int32)
    pair[::7] = -1
    src, tgt = AO.exact_copy_case()
    Rb, tb = AO.start_pose(3.0, 0.01)
    flat = small["r257"].copy()
    flat[:, 2] = 0.5
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    eye, zero = np.eye(3), np.zeros(3)
    two = np.full(257, -1, np.int32)
    two[[5, 9]] = [5, 9]
    return [("offset cloud", p, q, pair, eye, zero, False), ("body", AO.displaced(src, 5.0, 0.02)[0], tgt, (2 * np.arange(3445)).astype(np.int32), Rb, tb, False),
            ("planar patch", AO.displaced(flat, 20.0, 0.1)[0], flat, np.arange(257, dtype=np.int32), eye, zero, False),
            ("collinear", AO.displaced(line, 20.0, 0.1)[0], line, np.arange(3, dtype=np.int32), Rb, tb, True),
            ("two pairs", p, q, two, Rb, tb, True), ("no pair", small["nine"], small["nine"], np.full(9, -1, np.int32), Rb, tb, True)]


def _gpu_step(cases):
    from etch_amd import cloud as C
    from etch_amd import ops
    s, t = C.pack([c[1] for c in cases], DEV), C.pack([c[2] for c in cases], DEV)
    pair = torch.from_numpy(np.concatenate([c[3] for c in cases])).to(DEV)
    R = torch.from_numpy(np.stack([c[4] for c in cases])).to(DEV)
    tt = torch.from_numpy(np.stack([c[5] for c in cases])).to(DEV)
    return [_np(x) for x in ops.cloud_align_step(s.points, s.offsets, t.points, t.offsets, pair, R=R, t=tt)]


def test_one_step_from_given_pairs_within_the_derived_bounds(small):
    """The bounds.  Sums: the product adds the same terms as the oracle (one rounding per operation on both sides) in another order; any order of m
    terms is within (m - 1) u sum|term| of the exact sum to first order, and math.fsum is the exact sum rounded: m u sum|term| covers both.
    Rotation: the centred cross-covariance C = S - sx sq^T / m inherits dC_ab <= m u (A_ab + (a_a |sq_b| + |sx_a| a_b) / m) + 4 u (|S_ab| + |sx_a sq_b| / m)
    (A, a: the sums of the absolute terms; the last part: the division, the product and the subtraction on either side).  The rotation that
    maximises tr(R C) moves by at most |dC|_F / (s2 + e s3) radians to first order -- the smallest gap of Horn's matrix is 2 (s2 + e s3) and the
    quaternion's angle is half the rotation's, hence the factor 2 that cancels the 2 of the gap and the factor 2 kept for the two sides.  Both
    solvers (cyclic Jacobi here, LAPACK's SVD there) are backward stable: 16 u s1 / (s2 + e s3) covers their own error."""
    from etch_amd import cloud as C
    cases = _step_cases(small)
    dR, dt, m, sums, status, Rn, tn = _gpu_step(cases)
    for b, (name, p, q, pair, R, t, degenerate) in enumerate(cases):
        w = AO.step(p, q, pair, R, t)
        assert m[b] == w["m"] == (pair >= 0).sum(), name
        err = np.abs(sums[b] - w["sums"])
        bound = w["m"] * U * w["abs_sums"]
        print(f"PIN step {name}: m {m[b]}, worst sum error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (name, err, bound)
        assert bool(status[b] & C.STATUS_DEGENERATE) == degenerate == (not w["ok"]), (name, status[b])
        if degenerate:
            assert _same(Rn[b], R) and _same(tn[b], t) and np.array_equal(dR[b], np.eye(3)) and np.array_equal(dt[b], np.zeros(3)), name
            continue
        mm, A, S = w["m"], w["abs_sums"], w["sums"]
        dC = np.array([[mm * U * (A[6 + 3 * a + e] + (A[a] * abs(S[3 + e]) + abs(S[a]) * A[3 + e]) / mm) + 4 * U * (abs(S[6 + 3 * a + e]) + abs(S[a] * S[3 + e]) / mm)
                        for e in range(3)] for a in range(3)])
        gap = w["S"][1] + w["sign"] * w["S"][2]
        bound = 2.0 * float(np.sqrt((dC * dC).sum())) / gap + 16 * U * w["S"][0] / gap
        ang = math.radians(AO.angle_between(dR[b], w["dR"]))
        x_g, x_w = AO.apply(Rn[b], tn[b], p), AO.apply(w["R"], w["t"], p)
        reach = float(np.abs(np.concatenate([p, q])).max())
        print(f"PIN step {name}: rotation {ang:.3e} rad from the SVD Kabsch, bound {bound:.3e}; det dR - 1 {np.linalg.det(dR[b]) - 1.0:.2e}; moved rows differ by {np.abs(x_g - x_w).max():.3e} m")
        assert ang <= bound, (name, ang, bound)
        assert abs(np.linalg.det(dR[b]) - 1.0) <= 16 * U and np.abs(dR[b].T @ dR[b] - np.eye(3)).max() <= 16 * U, name
        assert np.abs(x_g - x_w).max() <= 4.0 * bound * reach + 64 * U * reach, name       # the transforms agree where the rows are
    flat = [c for c in cases if c[0] == "planar patch"][0]
    assert AO.angle_between(Rn[2], AO.start_pose(20.0, 0.1)[0]) < 1e-10 and flat[2][:, 2].std() == 0.0      # rank 2 is enough


def test_sixty_composed_steps_stay_a_rotation(small):
    """Every step composes a genuine turn of 7 to 11 degrees.  One composition rounds every entry of R within 3 u |row| |column| <= 3 u (1 + defect), and dR
    itself is orthogonal to 8 u (the unit quaternion's matrix): the defect of R^T R grows by at most 32 u a step, to first order."""
    from etch_amd import cloud as C
    from etch_amd import ops
    rng = np.random.default_rng(31)
    p = small["r257"]
    s = C.pack([p], DEV)
    pair = torch.arange(257, dtype=torch.int32, device=DEV)
    R, t = torch.eye(3, dtype=torch.float64, device=DEV)[None], torch.zeros((1, 3), dtype=torch.float64, device=DEV)
    Rw, tw = np.eye(3), np.zeros(3)
    for k in range(60):
        Rk, tk = AO.rotation(rng.standard_normal(3), 7.0 + 4.0 * rng.random()), rng.standard_normal(3) * 0.05
        Rw, tw = Rk @ Rw, Rk @ tw + tk
        q = C.pack([AO.apply(Rw, tw, p)], DEV)
        _, _, m, _, status, R, t = ops.cloud_align_step(s.points, s.offsets, q.points, q.offsets, pair, R=R, t=t)
    Rg, tg = _np(R)[0], _np(t)[0]
    det, orth = abs(np.linalg.det(Rg) - 1.0), float(np.abs(Rg.T @ Rg - np.eye(3)).max())
    print(f"PIN 60 composed steps: det R - 1 {det:.3e}, max |R^T R - I| {orth:.3e}, bound {60 * 32 * U:.3e}; {AO.angle_between(Rg, Rw):.3e} deg from the truth")
    assert int(m[0]) == 257 and int(status[0]) == 0 and det <= 60 * 32 * U and orth <= 60 * 32 * U
    assert AO.angle_between(Rg, Rw) < 1e-10 and np.abs(AO.apply(Rg, tg, p) - AO.apply(Rw, tw, p)).max() < 1e-11


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------------------

def test_the_loop_on_the_exact_copy_case():
    from etch_amd import cloud as C
    src, tgt = AO.exact_copy_case()
    starts = ((10.0, 0.05), (20.0, 0.10))
    moved = [AO.displaced(src, d, s)[0] for d, s in starts]
    res = C.align(C.pack(moved, DEV), C.pack([tgt, tgt], DEV))
    pairs = _split(res.pair, moved)
    for b, (d, s) in enumerate(starts):
        w = AO.align(moved[b], tgt)
        own = float(np.abs(AO.apply(w["R"], w["t"], moved[b]) - tgt[::2]).max())
        got = float(np.abs(AO.apply(_np(res.R)[b], _np(res.t)[b], moved[b]) - tgt[::2]).max())
        print(f"PIN exact copy from {d} deg / {s} m: residual {got:.3e} m, bound {4 * own + 1e-14:.3e} m (the oracle's own {own:.3e}); steps {res.steps[b]} (oracle {w['steps']})")
        assert res.matched[b] == 3445 and np.array_equal(pairs[b], 2 * np.arange(3445)) and res.status[b] == 0
        assert got <= 4 * own + 1e-14
        assert res.steps[b] < 40 and res.rms[b] < 1e-9
    one = C.align(C.pack(moved[1:], DEV), C.pack([tgt], DEV))                               # a pair alone = the same pair in the batch
    assert _same(one.R[0], res.R[1]) and _same(one.t[0], res.t[1]) and one.steps[0] == res.steps[1]


def test_the_loop_on_the_partial_overlap_case_and_its_brute_form():
    from etch_amd import cloud as C
    src, tgt = AO.partial_case()
    moved, R0, t0 = AO.displaced(src, 10.0, 0.05)
    kw = dict(gate=0.2, gate_min=0.01, decay=0.85, iters=60)
    w = AO.align(moved, tgt, **kw)
    own_ang, own_sh = AO.angle_between(w["R"], R0), float(np.sqrt(((w["t"] - t0) ** 2).sum()))
    s, t = C.pack([moved], DEV), C.pack([tgt], DEV)
    res = C.align(s, t, **kw)
    R, tt = _np(res.R)[0], _np(res.t)[0]
    ang, sh = AO.angle_between(R, R0), float(np.sqrt(((tt - t0) ** 2).sum()))
    print(f"PIN partial overlap from 10 deg / 0.05 m: {ang:.3e} deg and {sh:.3e} m from the truth (the oracle's own {own_ang:.3e} deg, {own_sh:.3e} m); "
          f"{res.matched[0]} matched (oracle {w['matched']}), rms {res.rms[0]:.3e} m, {res.steps[0]} steps (oracle {w['steps']})")
    assert ang <= 2 * own_ang and sh <= 2 * own_sh and res.status[0] == 0
    brute = C.align(s, t, brute=True, **kw)
    assert _same(brute.R, res.R) and _same(brute.t, res.t) and brute.matched[0] == res.matched[0] and brute.steps[0] == res.steps[0]
    assert _same(brute.pair, res.pair)
    start = C.align(s, t, init=(R0[None], t0[None]), **kw)                                  # from the truth: it stays there
    assert AO.angle_between(_np(start.R)[0], R0) <= 2 * own_ang and start.steps[0] <= res.steps[0]


# ---- views --------------------------------------------------------------------------------------------------------------------------------------------

def test_register_views_and_fuse_leave_every_surface_once():
    from etch_amd import cloud as C
    from etch_amd.depth import Cloud
    views = AO.three_views()
    moved = [AO.displaced(v, d, s)[0] for v, (d, s) in zip(views, AO.VIEW_POSES)]
    want = AO.occupied(np.concatenate(views), 0.005)
    packed = [C.pack([m], DEV) for m in moved]
    res = C.register_views(packed, **AO.VIEW_SETTINGS)
    fused = C.fuse(packed, res, voxel=0.005)
    eye = [(np.eye(3)[None], np.zeros((1, 3)))] * 3
    rough = C.fuse(packed, eye, voxel=0.005)
    got, bad = fused.points.shape[0], rough.points.shape[0]
    for k in (1, 2):
        R0, t0 = AO.start_pose(*AO.VIEW_POSES[k])
        print(f"PIN view {k}: {AO.angle_between(_np(res[k].R)[0], R0):.3e} deg from the truth, {res[k].matched[0]} matched, rms {res[k].rms[0]:.3e} m, {res[k].steps[0]} steps")
    print(f"PIN occupied 5 mm cells: undisplaced union {want}, registered and fused {got}, rough poses fused {bad}")
    assert abs(got - want) <= 0.01 * want and bad > 1.5 * want                              # the host test measured the margin: 13 069 against 6 422
    assert np.array_equal(_np(res[0].R)[0], np.eye(3)) and isinstance(fused, Cloud) and fused.offsets.tolist() == [0, got]
    plain = C.fuse(packed, res)
    assert plain.points.shape[0] == sum(len(m) for m in moved) and _same(plain.points[:len(moved[0])], moved[0])
    pts, c, clean = C.prepare(fused, 512, [3])
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (1, 512, 3) and isinstance(clean, Cloud) and c.shape == (1, 3)
    two = C.register_views([C.pack([m, moved[0]], DEV) for m in moved[:2]], **AO.VIEW_SETTINGS)      # two subjects per view
    assert _same(two[1].R[0], res[1].R[0]) and AO.angle_between(_np(two[1].R)[1], np.eye(3)) < 1e-9


def test_bad_arguments_raise_before_any_launch(small):
    from etch_amd import cloud as C
    one, two = C.pack([small["nine"]], DEV), C.pack([small["nine"], small["one"]], DEV)
    for kw, match in ((dict(gate=0.0), "gate must be positive"), (dict(gate=0.1, gate_min=0.2), "gate_min must not exceed"), (dict(decay=0.0), "decay must lie"),
                      (dict(decay=1.01), "decay must lie"), (dict(iters=0), "iters must be")):
        with pytest.raises(ValueError, match=match):
            C.align(one, one, **kw)
    with pytest.raises(ValueError, match="same number of clouds"):
        C.align(one, two)
    with pytest.raises(ValueError, match="same number of clouds"):
        C.register_views([one, two])
    with pytest.raises(ValueError, match="gate must be positive"):
        C.nearest(one, one, -1.0)


# ---- the command --------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def common(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    data = _train_data.build(tmp_path_factory.mktemp("align_data"), DEV)
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return ["--model_path", path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]


def _write_ply(path, p):
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\nend_header\n"
    path.write_bytes(head.encode() + p.astype("<f8").tobytes())


def test_the_command_registers_more_views_and_is_unchanged_without_them(common, tmp_path):
    from etch_amd import cloud as C
    views = AO.three_views()
    moved = [AO.displaced(v, d, s)[0] for v, (d, s) in zip(views, AO.VIEW_POSES)]
    for n, m in zip("abc", moved):
        _write_ply(tmp_path / f"{n}.ply", m)
    out, alone = tmp_path / "out", tmp_path / "alone"
    C.main(["--cloud_path", str(tmp_path / "a.ply"), "--more_views", str(tmp_path / "b.ply"), str(tmp_path / "c.ply"), "--align_gate_min", "0.01",
            "--align_decay", "0.85", "--align_iters", "60", "--fuse_voxel", "0.005", "--output_folder", str(out)] + common)
    rep = np.load(out / "a_cloud.npz")
    assert rep["view_pose"].shape == (3, 4, 4) and np.array_equal(rep["view_pose"][0], np.eye(4)) and (rep["view_pose"][:, 3] == [0, 0, 0, 1]).all()
    for k in (1, 2):
        R0, t0 = AO.start_pose(*AO.VIEW_POSES[k])
        assert AO.angle_between(rep["view_pose"][k, :3, :3], R0) < 0.01 and np.abs(rep["view_pose"][k, :3, 3] - t0).max() < 1e-4
    assert (rep["view_matched"][1:] > 2000).all() and (rep["view_rms"][1:] < 1e-3).all() and (rep["view_steps"][1:] <= 60).all() and not rep["view_status"].any()
    want = AO.occupied(np.concatenate(views), 0.005)
    assert abs(int(rep["rows_input"][0]) - want) <= 0.01 * want and {"a_pred_smpl.obj", "a_output_smpl_info.npz"} <= set(os.listdir(out))
    C.main(["--cloud_path", str(tmp_path / "a.ply"), "--output_folder", str(alone)] + common)          # without --more_views: what the command wrote before
    got = np.load(alone / "a_cloud.npz")
    p32, c, clean = C.prepare(C.pack([moved[0]], DEV), 1024, [4])                                        # the path of the command as it was
    old = dict(keep=_np(clean.keep), center=_np(c[0]), points=_np(p32[0]), removed=np.int64(0), rows_output=np.array([len(moved[0])]),
               rows_input=clean.stages["input"])
    assert sorted(got.files) == sorted(old) and all(got[k].dtype == np.asarray(v).dtype and np.array_equal(got[k], v) for k, v in old.items())
    assert sorted(f for f in os.listdir(alone) if f.startswith("a_")) == ["a_cloud.npz", "a_output_smpl_info.npz", "a_pred_smpl.obj"]
    from etch_amd import inference_demo as demo                                                            # ... and the two files of the fit, by the same path
    from etch_amd.models.fit_SMPL import Mesh
    before = tmp_path / "before"
    args = C.parse_args(["--cloud_path", str(tmp_path / "a.ply"), "--output_folder", str(before)] + common)
    model = demo.prepare_common(args)
    pred, info = demo.predict_smpl(args, model, _np(p32[0]), args.gender)
    final = pred.copy()
    final.vertices = pred.vertices + _np(c[0])
    Mesh.export(final, os.path.join(str(before), "a_pred_smpl.obj"))
    assert (before / "a_pred_smpl.obj").read_bytes() == (alone / "a_pred_smpl.obj").read_bytes()
    fit = np.load(alone / "a_output_smpl_info.npz")
    was = dict(body_pose=info[0][0, :21, :], hand_pose=info[0][0, 21:23, :], betas=info[1][0], global_orient=info[2][0], transl=info[3][0], joints=info[4][0])
    assert sorted(fit.files) == sorted(was) and all(_same(fit[k], np.asarray(v)) and fit[k].shape == np.asarray(v).shape for k, v in was.items())
