"""GPU checks of the info-point generation (csrc/raycast.hip, etch_amd.infopoints): the kernels bit for bit against the fp64 restatement
(tests/_raycast_oracle.py) on random and crafted cases, the pipeline against the reference's own output on the fixture's band of the 4D-Dress frame,
the acceptance of both self-face rules, determinism, the scan-point targets and the CLI."""
import os

import numpy as np
import pytest
import torch

import _raycast_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infopoints_4ddress.npz")


@pytest.fixture(scope="module")
def fx():
    return O.load_fixture(GOLDEN)


def _t(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype).contiguous()


def _soup(rng, F):
    v = rng.uniform(-1, 1, (3 * F, 3))
    return v, np.arange(3 * F).reshape(F, 3)


def _ray_gpu(o, d, v, f, excl=None, tmax=None):
    from etch_amd import ops

    out = ops.ray_first_hit(_t(o), _t(d), _t(v), _t(f, torch.int32), None if excl is None else _t(excl, torch.int32),
                            None if tmax is None else _t(tmax))
    return [x.cpu().numpy() for x in out]


def _assert_same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:8], g.dtype)


def test_ray_first_hit_random_soup_exact():
    rng = np.random.default_rng(11)
    v, f = _soup(rng, 4096)
    R = 640
    o = rng.uniform(-1.5, 1.5, (R, 3))
    d = rng.uniform(-1, 1, (R, 3)) - o * 0.5
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    excl = np.where(rng.random(R) < 0.5, rng.integers(0, 4096, R), -1)
    tmax = np.where(rng.random(R) < 0.5, rng.uniform(0.1, 3, R), np.inf)
    want = O.ray_first_hit(o, d, v, f, excl, tmax)
    got = _ray_gpu(o, d, v, f, excl, tmax)
    assert (want[0] >= 0).sum() > R // 2
    _assert_same(got, want)
    # the first hit excluded: the same rays find the next one, as the oracle does
    ex2 = np.where(want[0] >= 0, want[0], -1)
    _assert_same(_ray_gpu(o, d, v, f, ex2), O.ray_first_hit(o, d, v, f, ex2))


def test_ray_first_hit_crafted_cases():
    # a 2 x 2 grid of unit squares on z = 0 (8 triangles, listed so that shared edges / vertices meet faces of higher and lower index), a
    # plane at z = -1 underneath
    g = np.array([[x, y, 0.0] for y in range(3) for x in range(3)])
    v = np.concatenate([g, [[-5.0, -5, -1], [5, -5, -1], [0, 5, -1]]])
    quads = [(0, 1, 4, 3), (1, 2, 5, 4), (3, 4, 7, 6), (4, 5, 8, 7)]
    f = []
    for a, b, c, dd in reversed(quads):
        f += [[a, b, c], [a, c, dd]]
    f.append([9, 10, 11])
    f = np.array(f)
    down = [0.0, 0, -1]
    o = np.array([[0.5, 0.5, 1], [1.0, 1.0, 1], [1.0, 0.5, 1], [-1.0, 0.5, 0], [0.5, 0.5, -2], [0.25, 0.75, 1], [0.25, 0.75, 1], [0.25, 0.75, 1]])
    d = np.array([down, down, down, [1.0, 0, 0], down, down, down, down])
    excl = np.array([-1, -1, -1, -1, -1, -1, -1, -1])
    tmax = np.full(8, np.inf)
    tmax[6], tmax[7] = 1.0, 1.5
    want = O.ray_first_hit(o, d, v, f)
    # diagonal edge of one square (faces 6, 7) -> 6; centre vertex (every square) -> the lowest face touching it; edge between squares
    hits_centre = [i for i, tri in enumerate(f) if 4 in tri]
    assert want[0][0] == 6 and want[0][1] == min(hits_centre) and want[1][0] == 1.0
    assert want[0][3] == -1 and want[0][4] == -1        # parallel; behind the origin
    got = _ray_gpu(o, d, v, f, excl, tmax)
    _assert_same(got, O.ray_first_hit(o, d, v, f, excl, tmax))
    assert got[0][6] == -1 and got[0][7] >= 0 and got[1][7] == 1.0      # t < t_max is strict
    excl[5] = got[0][5]
    got = _ray_gpu(o, d, v, f, excl)
    assert got[0][5] == 8 and got[1][5] == 2.0          # the excluded face lets the ray reach the plane below
    _assert_same(got, O.ray_first_hit(o, d, v, f, excl))


def test_closest_point_random_soup_and_regions_exact():
    from etch_amd import ops

    rng = np.random.default_rng(12)
    v, f = _soup(rng, 4096)
    p = rng.uniform(-1.5, 1.5, (512, 3))
    got = [x.cpu().numpy() for x in ops.closest_point_on_mesh(_t(p), _t(v), _t(f, torch.int32))]
    _assert_same(got, O.closest_point_on_mesh(p, v, f))
    # the seven regions of one triangle (with a far-away second face so the chunk merge is exercised)
    tv = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [50, 50, 50], [51, 50, 50], [50, 51, 50]])
    tf = np.array([[0, 1, 2], [3, 4, 5]])
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [0.5, -1, 0.25], [-0.5, 2, 0], [-1, 0.5, 0], [1, 1, 0.5], [0.25, 0.25, 0.5]])
    _, _, _, region = O.closest_on_triangles(pts, tv[0], tv[1], tv[2])
    assert region.tolist() == list(range(7))
    got = [x.cpu().numpy() for x in ops.closest_point_on_mesh(_t(pts), _t(tv), _t(tf, torch.int32))]
    assert got[0].tolist() == [0] * 7
    _assert_same(got, O.closest_point_on_mesh(pts, tv, tf))


def test_vertex_normals_fixture_body(fx):
    from etch_amd import ops

    b = fx["body"]
    bv, bf = _t(b.vertices), _t(b.faces, torch.int32)
    n1 = ops.vertex_normals(bv, bf).cpu().numpy()
    n2 = ops.vertex_normals(bv, bf).cpu().numpy()
    assert np.array_equal(n1, n2)
    assert np.abs(n1 - O.vertex_normals(b.vertices, b.faces)).max() <= 1e-15


def test_thinning_flags_match_restatement(fx):
    from etch_amd import ops
    from etch_amd.infopoints import sample_surface

    pts, _, _ = sample_surface(fx["body"], 20000, seed=5)
    r = 0.012
    deg, rem = ops.remove_close(_t(pts), r)
    wdeg, wrem = O.remove_close(pts, r * r)
    assert wrem.sum() > 1000
    assert np.array_equal(deg.cpu().numpy(), wdeg) and np.array_equal(rem.cpu().numpy(), wrem)


def test_reference_samples_reproduced(fx):
    """The reference's own info points: each body point s = p - v located on the body (closest-point kernel), then tests 1-4 for it."""
    from etch_amd import ops
    from etch_amd.infopoints import interpolate_normals, mesh_to_device, trace_samples

    P, Vv = fx["info_points"], fx["info_vectors"]
    s = P - Vv
    scan_dev, body_dev = mesh_to_device(fx["scan"], DEV), mesh_to_device(fx["body"], DEV)
    face, bary, _, d2 = ops.closest_point_on_mesh(_t(s), *body_dev)
    assert float(d2.max()) <= 1e-18
    n = interpolate_normals(ops.vertex_normals(*body_dev), body_dev[1], face, bary).cpu().numpy()
    cosang = np.clip((n * Vv).sum(1) / np.linalg.norm(Vv, axis=1), -1, 1)
    angle = np.degrees(np.arccos(cosang))
    keep, ip, _, counts = trace_samples(scan_dev, body_dev, s, face, bary)
    keep, ip = keep.cpu().numpy(), ip.cpu().numpy()
    close = np.linalg.norm(ip - P[keep], axis=1) <= 1e-6
    good = np.zeros(len(P), bool)
    good[keep[close]] = True
    good &= angle <= 1e-4
    print("reference samples:", counts, "reproduced", good.mean())
    assert good.mean() >= 0.995, (good.mean(), counts)


def _generate(fx, self_face, seed=0, num_samples=1000):
    """generate_infopoints for samples drawn on the fixture's inner band (the faces whose rays see the whole frame's geometry)."""
    from etch_amd.infopoints import mesh_to_device, sample_surface_even, trace_samples

    pts, face, bary = sample_surface_even(fx["body_inner"], num_samples, seed=seed, device=DEV)
    _, ip, iv, counts = trace_samples(mesh_to_device(fx["scan"], DEV), mesh_to_device(fx["body"], DEV), pts, fx["inner_faces"][face], bary,
                                      self_face=self_face)
    return ip.cpu().numpy(), iv.cpu().numpy(), counts


@pytest.fixture(scope="module")
def runs(fx):
    return {"exclude": _generate(fx, "exclude"), "reference": _generate(fx, "reference"), "again": _generate(fx, "exclude")}


def test_acceptance_bands(runs):
    """Bands from the fp64 CPU restatement of the same pipeline (tests/_raycast_oracle.py in place of the kernels) on this band at 1 000
    samples, seeds 0-3: acceptance 0.691-0.706 with "exclude", 0.349-0.365 with "reference"."""
    e, r = runs["exclude"][2], runs["reference"][2]
    print("exclude", e, "reference", r)
    assert e["samples"] == r["samples"] == 1000
    assert 0.66 <= e["accepted"] / 1000 <= 0.74, e
    assert 0.31 <= r["accepted"] / 1000 <= 0.40, r
    assert min(e["rejected_test1"], e["rejected_test2"], e["rejected_test3"]) > 0       # the band exercises every test
    ip, iv, _ = runs["exclude"]
    assert ip.dtype == iv.dtype == np.float64 and ip.shape == iv.shape == (e["accepted"], 3)


def test_generation_is_bitwise_repeatable(runs):
    a, b = runs["exclude"], runs["again"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_batch_equals_uneven_chunks(fx):
    from etch_amd.infopoints import mesh_to_device, sample_surface

    pts, face, bary = sample_surface(fx["body"], 30000, seed=9)
    rng = np.random.default_rng(9)
    d = rng.standard_normal((30000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    excl = face.astype(np.int32)
    tmax = np.full(30000, 0.2)
    sv, sf = mesh_to_device(fx["scan"], DEV)
    from etch_amd import ops

    whole = [x.cpu().numpy() for x in ops.ray_first_hit(_t(pts), _t(d), sv, sf, _t(excl, torch.int32), _t(tmax))]
    cuts = [0, 1, 4097, 9000, 15555, 22222, 29999, 30000]
    parts = [[x.cpu().numpy() for x in ops.ray_first_hit(_t(pts[a:b]), _t(d[a:b]), sv, sf, _t(excl[a:b], torch.int32), _t(tmax[a:b]))]
             for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(4):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))
    assert (whole[0] >= 0).sum() > 1000
    sub = rng.choice(30000, 48, replace=False)
    _assert_same([w[sub] for w in whole], O.ray_first_hit(pts[sub], d[sub], fx["scan"].vertices, fx["scan"].faces, excl[sub], tmax[sub]))


def test_tightness_vectors_match_restatement(fx):
    from etch_amd.inference_demo import sample_points_from_mesh
    from etch_amd.infopoints import tightness_vectors

    x = sample_points_from_mesh(fx["scan"], 5000, seed=15)
    ip, iv = fx["info_points"], fx["info_vectors"]
    vec, use = tightness_vectors(x, ip, iv, fx["body"], device=DEV)
    # nearest info point by the bit-defined fp32 distance (lowest index on a tie), the 1 cm test on the fp64 distance to it
    x32, ip32 = x.astype(np.float32), ip.astype(np.float32)
    j = np.empty(len(x), np.int64)
    for a in range(0, len(x), 256):
        dd = (x32[a:a + 256, None] - ip32[None]).astype(np.float32)
        dist = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        j[a:a + 256] = dist.argmin(1)
    want_use = np.linalg.norm(x - ip[j], axis=1) < 0.01
    assert np.array_equal(use, want_use) and 0.05 < use.mean() < 0.95
    assert np.abs(vec[use] - iv[j[use]]).max() <= 1e-12
    far = np.flatnonzero(~use)
    _, _, q, _ = O.closest_point_on_mesh(x[far], fx["body"].vertices, fx["body"].faces)
    assert np.abs(vec[far] - (x[far] - q)).max() <= 1e-12


def _write_obj(path, m):
    with open(path, "w") as f:
        for p in m.vertices:
            f.write("v " + " ".join(repr(float(c)) for c in p) + "\n")
        for t in m.faces:
            f.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")


def test_cli_mode0_matches_api(fx, tmp_path):
    from etch_amd.generate_infopoints import main
    from etch_amd.inference_demo import load_obj
    from etch_amd.infopoints import generate_infopoints, write_outputs

    i = "00122_Inner_Take2_00011"
    os.makedirs(tmp_path / "model" / i)
    os.makedirs(tmp_path / "smplh" / i)
    _write_obj(tmp_path / "model" / i / f"{i}.obj", fx["scan"])
    _write_obj(tmp_path / "smplh" / i / f"mesh_smpl_{i}.obj", fx["body"])
    assert np.array_equal(load_obj(str(tmp_path / "smplh" / i / f"mesh_smpl_{i}.obj")).vertices, fx["body"].vertices)
    main(["-m", "0", "--num_samples", "6000", "-f_m", str(tmp_path / "model"), "-f_s", str(tmp_path / "smplh"), "-f_p", str(tmp_path / "ply"),
          "-f_n", str(tmp_path / "npz")])
    ip, iv, _ = generate_infopoints(fx["scan"], fx["body"], num_samples=6000, device=DEV)
    write_outputs(ip, iv, str(tmp_path / "api.ply"), str(tmp_path / "api.npz"))
    assert (tmp_path / "ply" / f"{i}.ply").read_bytes() == (tmp_path / "api.ply").read_bytes()
    a, b = np.load(tmp_path / "npz" / f"{i}.npz"), np.load(tmp_path / "api.npz")
    assert sorted(a.keys()) == sorted(b.keys()) == ["info_points", "info_vectors"]
    assert all(np.array_equal(a[k], b[k]) for k in a.keys()) and len(a["info_points"]) > 500
