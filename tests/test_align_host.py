"""Registration of raw clouds on the host: tests/_align_oracle.py against itself on the fixture body -- the conditions of the
cases the GPU tests use, pinned before any GPU is involved -- then the ABI, the build entry and the argument checks, which need no device."""
import numpy as np
import pytest

import _align_oracle as AO
from etch_amd import _lib


def test_nearest_ties_gate_and_the_tree_shortcut():
    q = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [3.0, 4.0, 0.0], [0.0, -3.0, 4.0], [10.0, 0.0, 0.0]])
    p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [6.0, 8.0, 0.0], [10.0, 5.0, 0.0], [10.0, 5.0 + 1e-9, 0.0], [1.5, 2.0, 0.0]])
    pair, d2 = AO.nearest(p, q, 5.0)
    assert pair.tolist() == [0, 1, 1, 4, -1, 0] and d2[:4].tolist() == [0.0, 0.0, 25.0, 25.0] and d2[4] == np.inf      # on the gate: in; a tie: the lowest row
    assert AO.nearest(p, q[:0], 5.0)[0].tolist() == [-1] * 6 and len(AO.nearest(p[:0], q, 5.0)[0]) == 0
    R, t = AO.start_pose(10.0, 0.05)
    src, tgt = AO.partial_case()
    from scipy.spatial import cKDTree
    a, b = AO.nearest(src[:700], tgt, 0.05, R, t), AO.nearest(src[:700], tgt, 0.05, R, t, tree=cKDTree(tgt))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and 0 < (a[0] >= 0).sum() < 700


def test_one_step_recovers_a_known_motion_and_reports_degenerate_pairs():
    rng = np.random.default_rng(23)
    q = rng.standard_normal((300, 3)) * [0.2, 0.6, 0.1] + [5.0, -3.0, 0.5]
    p, R0, t0 = AO.displaced(q, 20.0, 0.1)
    s = AO.step(p, q, np.arange(300), np.eye(3), np.zeros(3))
    assert s["ok"] and s["m"] == 300 and AO.angle_between(s["R"], R0) < 1e-12 and np.abs(s["t"] - t0).max() < 1e-13
    assert abs(np.linalg.det(s["dR"]) - 1.0) < 1e-14
    flat = q.copy()
    flat[:, 2] = 0.5                                                # a planar patch has rank 2: the step is defined
    pf, _, _ = AO.displaced(flat, 20.0, 0.1)
    s = AO.step(pf, flat, np.arange(300), np.eye(3), np.zeros(3))
    assert s["ok"] and s["S"][2] < 1e-12 * s["S"][0] and AO.angle_between(s["R"], R0) < 1e-12
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    s = AO.step(AO.displaced(line, 20.0, 0.1)[0], line, np.arange(3), np.eye(3), np.zeros(3))
    assert not s["ok"] and np.array_equal(s["R"], np.eye(3)) and np.array_equal(s["dR"], np.eye(3))
    assert not AO.step(p, q, np.concatenate([[0, 1], np.full(298, -1)]), np.eye(3), np.zeros(3))["ok"]      # two pairs


@pytest.mark.parametrize("degrees,shift", [(5.0, 0.02), (10.0, 0.05), (20.0, 0.10), (30.0, 0.15)])
def test_exact_copy_case_converges_to_rounding(degrees, shift):
    src, tgt = AO.exact_copy_case()
    p, R0, t0 = AO.displaced(src, degrees, shift)
    r = AO.align(p, tgt)
    res = float(np.abs(AO.apply(r["R"], r["t"], p) - tgt[::2]).max())
    print(f"exact copy from {degrees} deg / {shift} m: {r['steps']} steps, residual {res:.3e} m")
    assert r["matched"] == 3445 and np.array_equal(r["pair"], 2 * np.arange(3445)) and r["steps"] < 40 and res < 1e-13 and r["status"] == 0


@pytest.mark.parametrize("degrees,shift", [(10.0, 0.05), (20.0, 0.10)])
def test_partial_overlap_case_converges_inside_the_basin(degrees, shift):
    """From 30 degrees / 15 cm the loop stays 30 degrees away with a few hundred rows matched: that start is outside the basin, and is no test."""
    src, tgt = AO.partial_case()
    assert (len(src), len(tgt)) == (5119, 4057)
    p, R0, t0 = AO.displaced(src, degrees, shift)
    r = AO.align(p, tgt, gate=0.2, gate_min=0.01, decay=0.85, iters=60)
    ang, sh = AO.angle_between(r["R"], R0), float(np.sqrt(((r["t"] - t0) ** 2).sum()))
    print(f"partial overlap from {degrees} deg / {shift} m: {r['steps']} steps, {r['matched']} matched, rms {r['rms']:.3e} m, {ang:.3e} deg and {sh:.3e} m from the truth")
    assert r["matched"] == 2954 and ang < 2e-3 and sh < 2e-5 and r["rms"] < 3e-4


def test_three_views_double_the_surface_until_they_are_registered():
    views = AO.three_views()
    moved = [AO.displaced(v, d, s)[0] for v, (d, s) in zip(views, AO.VIEW_POSES)]
    want = AO.occupied(np.concatenate(views), 0.005)
    rough = AO.occupied(np.concatenate(moved), 0.005)
    placed = [moved[0]]
    for v in moved[1:]:
        r = AO.align(v, np.concatenate(placed), **AO.VIEW_SETTINGS)
        placed.append(AO.apply(r["R"], r["t"], v))
    got = AO.occupied(np.concatenate(placed), 0.005)
    print(f"occupied 5 mm cells: undisplaced union {want}, rough poses concatenated {rough}, registered {got}")
    assert rough > 1.5 * want and abs(got - want) <= 0.01 * want


def test_the_abi_declares_the_align_calls_and_the_package_binds_them():
    names = _lib.declared_symbols()
    for n in ("etch_cloud_align_grid", "etch_cloud_nearest", "etch_cloud_align_step", "etch_cloud_align", "etch_cloud_transform"):
        assert n in names, n
    from etch_amd import build as B
    assert B.EXTRA["cloud_align.hip"] == ["-ffp-contract=off"] and "cloud_align.hip" in B.sources()
    from etch_amd import cloud, ops
    for f in ("cloud_nearest", "cloud_align_step", "cloud_align", "cloud_transform"):
        assert callable(getattr(ops, f)), f
    for f in ("nearest", "align", "transform", "register_views", "fuse"):
        assert callable(getattr(cloud, f)), f
    hdr = open(_lib.HEADER).read()
    assert f"#define ETCH_ALIGN_STATUS_DEGENERATE {cloud.STATUS_DEGENERATE}" in hdr and cloud.STATUS_DEGENERATE == ops.ALIGN_STATUS_DEGENERATE == AO.DEGENERATE
    assert AO.RANK_EPS == 1e-9 and "#define ETCH_ALIGN_RANK_EPS 1e-9\n" in hdr


def test_bad_arguments_raise_before_any_launch_and_the_flags_default_to_off():
    """ValueError without a GPU: the checks run before the first launch (here there is no device to launch on)."""
    from etch_amd import cloud as C
    one = C.pack([np.zeros((4, 3))], device="cpu")
    two = C.pack([np.zeros((4, 3)), np.ones((2, 3))], device="cpu")
    for kw, match in ((dict(gate=0.0), "gate must be positive"), (dict(gate=-1.0), "gate must be positive"), (dict(gate=0.1, gate_min=0.2), "gate_min must not exceed"),
                      (dict(decay=0.0), "decay must lie"), (dict(decay=1.5), "decay must lie"), (dict(iters=0), "iters must be"), (dict(iters=2.5), "iters must be")):
        with pytest.raises(ValueError, match=match):
            C.align(one, one, **kw)
        with pytest.raises(ValueError, match=match):
            C.register_views([one, one], **kw)
    with pytest.raises(ValueError, match="same number of clouds"):
        C.align(one, two)
    with pytest.raises(ValueError, match="same number of clouds"):
        C.nearest(two, one, 0.1)
    with pytest.raises(ValueError, match="gate must be positive"):
        C.nearest(one, one, 0.0)
    with pytest.raises(ValueError, match="same number of clouds"):
        C.register_views([one, two])
    with pytest.raises(ValueError, match="R and t together"):
        C.nearest(one, one, 0.1, R=np.eye(3)[None])
    with pytest.raises(ValueError, match="R and t together"):
        C.transform(one, None, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="one transform per view"):
        C.fuse([one, one], [None])
    a = C.build_parser().parse_args(["--cloud_path", "x.ply"])
    assert (a.more_views, a.align_gate, a.align_gate_min, a.align_decay, a.align_iters, a.view_init, a.fuse_voxel) == (None, 0.2, 0.02, 0.9, 40, None, 0.0)
    for bad in (["--align_gate", "0"], ["--align_decay", "1.5"], ["--align_iters", "0"], ["--fuse_voxel", "-1"], ["--view_init", "p.npz"]):
        with pytest.raises(SystemExit):
            C.parse_args(["--cloud_path", "x.ply"] + bad)
