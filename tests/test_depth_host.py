"""Single-view scans, the parts that need no GPU: cameras, the numpy oracle's self-check against an independent ray cast, depth-file loading, the
flags of `python -m etch_amd.depth` / eval / train, and the training views' determinism."""
import math
import os

import numpy as np
import pytest

import _depth_oracle as DO
import _raycast_oracle as RC

from etch_amd import depth as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")
H, W, F = 48, 64, 70.0
AZIMUTHS = (0.0, 1.1, 2.5)


def body():
    z = np.load(GOLDEN)
    return z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)


def issue_camera(verts, az):
    """64 x 48, fx = fy = 70, 2.5 m out, 0.25 m up, looking at the bounding-box centre."""
    c = (verts.min(0) + verts.max(0)) / 2.0
    return D.Camera.look_at(c + 2.5 * np.array([math.sin(az), 0.1, math.cos(az)]), c, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, width=W, height=H)


def _check_rotation(cam, target):
    assert np.abs(cam.R @ cam.R.T - np.eye(3)).max() < 1e-14
    assert abs(np.linalg.det(cam.R) - 1.0) < 1e-14
    uv, z = cam.project(np.asarray(target, np.float64)[None])
    assert np.abs(uv[0] - [cam.cx, cam.cy]).max() < 1e-9 and z[0] > 0


def test_look_at_and_orbit_are_rigid_and_centre_the_target():
    rng = np.random.default_rng(5)
    for _ in range(20):
        eye, target = rng.normal(size=3) * 3, rng.normal(size=3)
        cam = D.Camera.look_at(eye, target, fx=500.0, cx=320.0, cy=240.0, width=640, height=480)
        _check_rotation(cam, target)
        assert np.abs(cam.eye - eye).max() < 1e-12
        c = rng.normal(size=3)
        az, el = rng.uniform(0, 2 * math.pi), rng.uniform(-1.2, 1.2)
        cam = D.Camera.orbit(c, 2.0, az, el, fov_deg=50.0, height=48, width=64)
        _check_rotation(cam, c)
        assert abs(np.linalg.norm(cam.eye - c) - 2.0) < 1e-12
        assert cam.fx == cam.fy == 24.0 / math.tan(math.radians(25.0)) and (cam.cx, cam.cy) == (32.0, 24.0)
        want = c + 2.0 * np.array([math.sin(az) * math.cos(el), math.sin(el), math.cos(az) * math.cos(el)])
        assert np.abs(cam.eye - want).max() < 1e-12
    # y-up data, image y down: a point above the target lands above the principal point
    cam = D.Camera.orbit([0, 0, 0], 2.0, 0.0)
    assert cam.project(np.array([[0.0, 0.5, 0.0]]))[0][0, 1] < cam.cy
    assert cam.project(np.array([[0.5, 0.0, 0.0]]))[0][0, 0] > cam.cx        # seen from +z, +x is to the right
    with pytest.raises(ValueError):
        D.Camera.look_at([0, 0, 0], [0, 1, 0])
    with pytest.raises(ValueError):
        D.Camera.look_at([0, 0, 0], [0, 0, 0])


def test_camera_matches_the_oracles_own_look_at():
    v, _ = body()
    c = (v.min(0) + v.max(0)) / 2.0
    for az in AZIMUTHS:
        eye = c + 2.5 * np.array([math.sin(az), 0.1, math.cos(az)])
        assert np.array_equal(issue_camera(v, az).row(), DO.look_at_row(eye, c, F, F, W / 2.0, H / 2.0))


@pytest.mark.parametrize("az", AZIMUTHS)
def test_oracle_rasteriser_agrees_with_a_ray_cast(az):
    """The oracle of the GPU tests against Moller-Trumbore along the pixel-centre rays (tests/_raycast_oracle.py): the same covered pixels, the
    same face at every pixel, depths within 1e-12."""
    v, f = body()
    cam = issue_camera(v, az).row()
    depth, face, bary, dropped, status, _ = DO.render(v, f, cam, H, W)
    o, d = DO.pixel_rays(cam, H, W)
    rf, rt, _, _ = RC.ray_first_hit(o, d, v, f, block=128)
    hit = np.isfinite(depth).reshape(-1)
    print(f"azimuth {az}: {hit.sum()} valid pixels, {(hit != (rf >= 0)).sum()} coverage and {(face.reshape(-1) != rf).sum()} face differences, "
          f"max depth difference {np.abs(depth.reshape(-1)[hit] - rt[hit]).max():.2e}, {dropped} dropped")
    assert hit.sum() > 250 and dropped == 0 and status == 0
    assert np.array_equal(hit, rf >= 0)
    assert np.array_equal(face.reshape(-1), rf)
    assert np.abs(depth.reshape(-1)[hit] - rt[hit]).max() <= 1e-12
    b = bary.reshape(-1, 3)[hit]
    assert np.abs(b.sum(1) - 1.0).max() < 1e-12 and b.min() >= 0.0
    # the barycentrics carry the face's vertices to the point the ray hits
    p = (v[f[face.reshape(-1)[hit]]] * b[:, :, None]).sum(1)
    assert np.abs(p - (o[hit] + rt[hit, None] * d[hit])).max() < 1e-12


def test_oracle_unproject_and_pick_invert_the_projection():
    v, f = body()
    cam = issue_camera(v, 1.1)
    depth = DO.render(v, f, cam.row(), H, W)[0]
    index, world = DO.unproject(depth, cam.row())
    assert np.array_equal(index, np.flatnonzero(np.isfinite(depth).reshape(-1)))
    uv, z = cam.project(world)
    assert np.abs(uv - np.stack([index % W + 0.5, index // W + 0.5], 1)).max() < 1e-9
    assert np.abs(z - depth.reshape(-1)[index]).max() < 1e-12
    _, p32, pixel, rank = DO.pick(index, world, 64, 77)
    assert (np.diff(rank) >= 0).all() and rank.min() >= 0 and rank.max() < len(index) and np.array_equal(pixel, index[rank])
    assert p32.dtype == np.float32


def test_load_depth_and_scale(tmp_path):
    a = np.random.default_rng(0).uniform(0.5, 3.0, (5, 7))
    np.save(tmp_path / "a.npy", a)
    assert np.array_equal(D.load_depth(str(tmp_path / "a.npy")), a)
    mm = (a * 1000).astype(np.uint16)
    np.savez(tmp_path / "mm.npz", mm)
    got = D.load_depth(str(tmp_path / "mm.npz"), 0.001)
    assert got.dtype == np.float64 and np.array_equal(got, mm.astype(np.float64) * 0.001)
    np.savez(tmp_path / "two.npz", depth=mm, mask=mm)
    assert np.array_equal(D.load_depth(str(tmp_path / "two.npz"), 0.001), got)
    np.savez(tmp_path / "bad.npz", x=mm, y=mm)
    np.save(tmp_path / "cube.npy", np.zeros((2, 3, 4)))
    for name, scale in (("bad.npz", 1.0), ("cube.npy", 1.0), ("a.npy", 0.0), ("a.npy", math.nan)):
        with pytest.raises(ValueError):
            D.load_depth(str(tmp_path / name), scale)
    with pytest.raises(ValueError):
        D.load_depth(str(tmp_path / "a.png"))
    E = np.eye(4)
    E[:3, 3] = [1, 2, 3]
    np.save(tmp_path / "E.npy", E)
    R, t = D.load_extrinsics(str(tmp_path / "E.npy"))
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, [1, 2, 3])
    np.save(tmp_path / "E33.npy", np.eye(3))
    with pytest.raises(ValueError):
        D.load_extrinsics(str(tmp_path / "E33.npy"))


FRAME = ["--depth_path", "d.npy", "--intrinsics", "70", "70", "32", "24"]
VIEW = ["--scan_path", "s.obj", "--view_azimuth", "30"]


@pytest.mark.parametrize("argv", [[], FRAME + VIEW, ["--depth_path", "d.npy"], ["--scan_path", "s.obj"], FRAME + ["--view_azimuth", "3"],
                                  VIEW + ["--intrinsics", "1", "1", "0", "0"], VIEW + ["--depth_scale", "0.001"], VIEW + ["--view_elevation", "90"],
                                  VIEW + ["--view_size", "0", "4"], VIEW + ["--view_fov", "180"], FRAME + ["--depth_scale", "0"],
                                  FRAME + ["--depth_range", "2", "1"], ["--depth_path", "d.npy", "--intrinsics", "0", "70", "1", "1"],
                                  VIEW + ["--num_point", "0"], VIEW + ["--chamfer_refine", "sideways"]])
def test_depth_command_rejects_bad_flags(argv, capsys):
    with pytest.raises(SystemExit) as e:
        D.parse_args(argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_depth_command_flags():
    a = D.parse_args(VIEW)
    assert a.chamfer_refine == "none" and a.view_elevation == 0.0 and tuple(a.view_size) == (512, 512) and a.num_point == 5000
    assert D.parse_args(VIEW + ["--chamfer_refine"]).chamfer_refine == "partial"             # a single view is a partial scan
    assert D.parse_args(VIEW + ["--chamfer_refine", "both"]).chamfer_refine == "both"
    a = D.parse_args(FRAME + ["--depth_scale", "0.001", "--depth_range", "0.3", "4", "--extrinsics", "E.npy", "--synthetic_body"])
    assert a.intrinsics == [70.0, 70.0, 32.0, 24.0] and a.depth_range == [0.3, 4.0] and a.synthetic_body and a.depth_scale == 0.001


def test_view_spec_is_a_pure_function_of_seed_epoch_index():
    spec = D.ViewSpec(probability=1.0, elevation_range=(-10.0, 30.0), distance=2.5, fov_deg=40.0, size=(48, 64))
    c = np.array([0.1, -0.3, 0.0])
    a, b = spec.camera(3, 0, 1, c), spec.camera(3, 0, 1, c)
    assert np.array_equal(a.row(), b.row()) and spec.draw(3, 0, 1) == spec.draw(3, 0, 1)
    assert (a.height, a.width) == (48, 64)
    for other in ((3, 1, 1), (3, 0, 0), (4, 0, 1)):
        assert not np.array_equal(spec.camera(*other, c).row(), a.row())
    taken, az, el, key = spec.draw(3, 0, 1)
    assert taken and 0.0 <= az < 2 * math.pi and math.radians(-10.0) <= el <= math.radians(30.0) and 0 <= key < 2 ** 63
    assert abs(np.linalg.norm(a.eye - c) - 2.5) < 1e-12
    # the probability thins the views without moving the ones that stay
    half = D.ViewSpec(probability=0.5, size=(48, 64), fov_deg=40.0)
    kept = [half.camera(3, 0, i, c) for i in range(200)]
    assert 60 < sum(k is not None for k in kept) < 140
    assert all(k is None or np.array_equal(k.row(), spec.camera(3, 0, i, c).row()) for i, k in enumerate(kept))
    assert all(D.ViewSpec(probability=0.0).camera(3, 0, i, c) is None for i in range(20))
    for bad in (dict(probability=1.5), dict(elevation_range=(30.0, -10.0)), dict(elevation_range=(0.0, 90.0)), dict(distance=0.0), dict(fov_deg=180.0),
                dict(size=(0, 4))):
        with pytest.raises(ValueError):
            D.ViewSpec(**bad)


def test_train_and_eval_view_flags():
    from etch_amd import eval as E
    from etch_amd import train as T
    a = T.build_parser().parse_args([])
    assert a.partial_views == 0.0 and T.view_spec_from_args(a) is None                       # unset: the dataset of today
    a = T.build_parser().parse_args(["--partial_views", "0.5", "--view_elevation", "-5", "20", "--view_distance", "3", "--view_fov", "50", "--view_size", "64", "48"])
    assert T.view_spec_from_args(a) == D.ViewSpec(0.5, (-5.0, 20.0), 3.0, 50.0, (64, 48))
    p = E.build_parser()
    assert E.view_from_args(p, p.parse_args([])) is None
    v = E.view_from_args(p, p.parse_args(["--view_azimuth", "45", "--view_size", "64", "48"]))
    assert v == {"azimuth": 45.0, "elevation": 0.0, "distance": 2.5, "fov": 45.0, "size": (64, 48)}
    with pytest.raises(SystemExit):
        E.view_from_args(p, p.parse_args(["--view_azimuth", "45", "--ingest", "host"]))
    with pytest.raises(ValueError, match="ingest"):
        E.evaluate_dataset(None, None, type("DS", (), {"ingest": "host"})(), view=v)
    cams = E.view_cameras(v, [type("M", (), {"vertices": np.array([[0.0, 0, 0], [2, 2, 2]])})()])
    assert np.abs(cams[0].eye - (np.array([1.0, 1, 1]) + 2.5 * np.array([math.sin(math.pi / 4), 0, math.cos(math.pi / 4)]))).max() < 1e-12
