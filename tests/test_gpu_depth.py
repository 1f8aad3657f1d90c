"""Single-view scans on the GPU: the depth rasteriser, the back-projection and the stratified pick against tests/_depth_oracle.py
bit for bit, an independent cross-check through ops.ray_first_hit, partial_view_points, GTDataset(view=...), and the train / depth / eval commands
on the two-id dataset of tests/_train_data.py.  Images are 64 x 48 (one case 33 x 17), at most 4 views per call."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _depth_oracle as DO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")
H, W, F = 48, 64, 70.0
AZIMUTHS = (0.0, 1.1, 2.5)
KEYS = [15, 2 ** 63 + 5, 2 ** 64 - 1]


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _camera(verts, az, f=F, h=H, w=W):
    from etch_amd.depth import Camera
    c = (verts.min(0) + verts.max(0)) / 2.0
    return Camera.look_at(c + 2.5 * np.array([math.sin(az), 0.1, math.cos(az)]), c, fx=f, fy=f, cx=w / 2.0, cy=h / 2.0, width=w, height=h)


def _check_render(got, want, k=0):
    """got: RenderResult; want: DO.render's tuple for view k."""
    assert _same(got.depth[k], want[0]), "depth"
    assert _same(got.face[k], want[1]), "face"
    if got.bary is not None:
        assert _same(got.bary[k], want[2]), "bary"
    assert int(got.dropped[k]) == want[3] and int(got.large[k]) == want[5]


@pytest.fixture(scope="module")
def scene():
    """The fixture body (13 776 faces), its three cameras and the oracle's maps and clouds of them, computed once and left unchanged."""
    from etch_amd.inference_demo import Mesh
    z = np.load(GOLDEN)
    v, f = z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)
    cams = [_camera(v, az) for az in AZIMUTHS]
    want = [DO.render(v, f, c.row(), H, W) for c in cams]
    clouds = [DO.unproject(w[0], c.row()) for w, c in zip(want, cams)]
    assert all(w[3] == 0 and w[4] == 0 for w in want) and min(len(c[0]) for c in clouds) > 250
    rng = np.random.default_rng(5)
    sv = rng.standard_normal((67, 3)) * [0.3, 0.5, 0.2] + (v.min(0) + v.max(0)) / 2.0
    strip = Mesh(sv, np.stack([np.arange(65), np.arange(65) + 1, np.arange(65) + 2], 1))
    return types.SimpleNamespace(v=v, f=f, body=Mesh(v, f), cams=cams, want=want, clouds=clouds, strip=strip, center=(v.min(0) + v.max(0)) / 2.0)


@pytest.fixture(scope="module")
def rendered(scene):
    from etch_amd.depth import render
    return render([scene.body], scene.cams, bary=True, device=DEV)


def test_three_views_in_one_call_equal_the_oracle(scene, rendered):
    assert rendered.depth.shape == (3, H, W) and rendered.depth.dtype == torch.float64 and rendered.face.dtype == torch.int32
    assert rendered.bary.shape == (3, H, W, 3)
    for k in range(3):
        _check_render(rendered, scene.want[k], k)
    miss = rendered.face.cpu().numpy() < 0
    assert np.isposinf(rendered.depth.cpu().numpy()[miss]).all() and not rendered.bary.cpu().numpy()[miss].any()


def test_one_view_per_call_and_a_ragged_batch_give_the_same_bits(scene, rendered):
    from etch_amd.depth import render
    for k, cam in enumerate(scene.cams):
        one = render([scene.body], [cam], bary=True, device=DEV)
        assert _same(one.depth[0], rendered.depth[k]) and _same(one.face[0], rendered.face[k]) and _same(one.bary[0], rendered.bary[k])
    cams = [scene.cams[0], scene.cams[1], scene.cams[1], scene.cams[2]]
    rag = render([scene.strip, scene.body], cams, view_mesh=[1, 0, 1, 1], bary=True, device=DEV)
    for k, src in ((0, 0), (2, 1), (3, 2)):
        assert _same(rag.depth[k], rendered.depth[src]) and _same(rag.face[k], rendered.face[src]) and _same(rag.bary[k], rendered.bary[src])
    want = DO.render(scene.strip.vertices, scene.strip.faces, scene.cams[1].row(), H, W)
    assert np.isfinite(want[0]).sum() > 100
    _check_render(rag, want, 1)
    nob = render([scene.strip, scene.body], cams, view_mesh=[1, 0, 1, 1], device=DEV)            # bary=False skips the output, nothing else
    assert nob.bary is None and _same(nob.depth, rag.depth) and _same(nob.face, rag.face)


def test_odd_image_size(scene):
    """33 x 17: neither side a multiple of anything, 561 pixels = two full blocks of 256 and a part of a third."""
    from etch_amd.depth import render
    cams = [_camera(scene.v, az, f=25.0, h=17, w=33) for az in (0.4, 3.0)]
    got = render([scene.body, scene.strip], cams, view_mesh=[0, 1], bary=True, device=DEV)
    for k, m in enumerate((scene.body, scene.strip)):
        want = DO.render(m.vertices, m.faces, cams[k].row(), 17, 33)
        assert np.isfinite(want[0]).sum() > 40
        _check_render(got, want, k)


def test_exact_ties_report_the_lower_face(scene, rendered):
    from etch_amd.depth import render
    from etch_amd.inference_demo import Mesh
    n = len(scene.f)
    got = render([Mesh(scene.v, np.concatenate([scene.f, scene.f[::-1]]))], scene.cams, bary=True, device=DEV)
    assert _same(got.depth, rendered.depth) and _same(got.bary, rendered.bary)
    face = got.face.cpu().numpy()
    assert face.max() < n and _same(got.face, rendered.face)


def test_reversed_winding(scene, rendered):
    from etch_amd.depth import render
    from etch_amd.inference_demo import Mesh
    rev = np.ascontiguousarray(scene.f[:, ::-1])
    got = render([Mesh(scene.v, rev)], scene.cams, bary=True, device=DEV)
    for k, cam in enumerate(scene.cams):
        _check_render(got, DO.render(scene.v, rev, cam.row(), H, W), k)
    assert np.array_equal(got.face.cpu().numpy() >= 0, rendered.face.cpu().numpy() >= 0)             # two-sided: the same pixels are covered


def test_large_faces_and_clamping(scene):
    from etch_amd import ops
    from etch_amd.depth import render
    from etch_amd.inference_demo import Mesh
    assert ops.depth_large_threshold() == 256
    c = scene.center
    # the body seen from +z with a 20 m quad 1.5 m behind it: both triangles overfill the image
    quad = np.array([[-10.0, -10.0, -1.5], [10.0, -10.0, -1.5], [10.0, 10.0, -1.5], [-10.0, 10.0, -1.5]]) + c
    v = np.concatenate([scene.v, quad])
    n = len(scene.v)
    f = np.concatenate([scene.f, [[n, n + 1, n + 2], [n, n + 2, n + 3]]])
    got = render([Mesh(v, f)], [scene.cams[0]], bary=True, device=DEV)
    want = DO.render(v, f, scene.cams[0].row(), H, W)
    assert want[5] == 2 and np.isfinite(want[0]).all() and (want[1] >= len(scene.f)).sum() > 2000
    _check_render(got, want)
    assert int(got.large[0]) == 2                                                                   # the quad took the large-face launch
    # zoomed in: the body overflows the image and candidate boxes are clamped at its border; at 10 x the faces are still small (about 10 pixels
    # across), at 29 x the image lies inside the torso and 25 faces are large
    for f_zoom, large in ((700.0, 0), (2000.0, 25)):
        zoom = _camera(scene.v, 0.0, f=f_zoom)
        got = render([scene.body], [zoom], bary=True, device=DEV)
        want = DO.render(scene.v, scene.f, zoom.row(), H, W)
        assert want[5] == large and np.isfinite(want[0]).sum() > 2800
        _check_render(got, want)


def test_near_plane_drops_whole_faces_and_a_nan_vertex_raises(scene, rendered):
    from etch_amd._lib import EtchHipError
    from etch_amd.depth import render
    from etch_amd.inference_demo import Mesh
    cam = scene.cams[0]
    eye = cam.eye
    # a quad beside the camera, from 1 m in front of it to 1 m behind: every triangle has a corner behind the near plane
    quad = np.array([[0.5, -0.2, -1.0], [0.5, 0.2, -1.0], [0.5, 0.2, 1.0], [0.5, -0.2, 1.0]]) + eye
    n = len(scene.v)
    v = np.concatenate([scene.v, quad])
    f = np.concatenate([scene.f, [[n, n + 1, n + 2], [n, n + 2, n + 3]]])
    got = render([Mesh(v, f)], [cam], bary=True, device=DEV)
    assert int(got.dropped[0]) == 2 == DO.render(v, f, cam.row(), H, W)[3]
    assert _same(got.depth[0], rendered.depth[0]) and _same(got.face[0], rendered.face[0]) and _same(got.bary[0], rendered.bary[0])
    bad = scene.strip.vertices.copy()
    bad[10, 1] = np.nan
    with pytest.raises(EtchHipError, match="view 1.*not finite"):
        render([scene.body, Mesh(bad, scene.strip.faces)], [cam, cam], device=DEV)
    with pytest.raises(ValueError):
        render([scene.body], [cam, _camera(scene.v, 0.0, h=17, w=33)], device=DEV)                 # all views of a call share H and W
    with pytest.raises(ValueError):
        render([scene.body, scene.strip], [cam, cam, cam], device=DEV)                              # which mesh does each view look at?
    with pytest.raises(ValueError):
        render([scene.body], [cam], near=0.0, device=DEV)


@pytest.fixture(scope="module")
def cloud(scene, rendered):
    from etch_amd.depth import unproject
    return unproject(rendered.depth, scene.cams)


def test_unproject_equals_the_oracle(scene, cloud):
    off = cloud.offsets.cpu().numpy()
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(c[0]) for c in scene.clouds])]).tolist()
    assert cloud.count.cpu().numpy().tolist() == [len(c[0]) for c in scene.clouds] and len(cloud.points) == off[-1]
    for k, (index, world) in enumerate(scene.clouds):
        p, i = cloud.view(k)
        assert _same(i, index) and _same(p, world)


@pytest.mark.parametrize("N", [256, 512])
def test_pick_equals_the_oracle(scene, cloud, N):
    """N = 256 <= n on every view (277, 452, 375 valid pixels) and N = 512 > n on every view."""
    from etch_amd.depth import pick
    p32, p64, pixel = pick(cloud, N, KEYS)
    assert p32.shape == (3, N, 3) and p32.dtype == torch.float32 and p64.dtype == torch.float64 and pixel.dtype == torch.int32
    for k, (index, world) in enumerate(scene.clouds):
        assert (len(index) >= N) == (N == 256)
        w64, w32, wpix, _ = DO.pick(index, world, N, KEYS[k])
        assert _same(p64[k], w64) and _same(p32[k], w32) and _same(pixel[k], wpix)
        assert _same(p32[k], p64[k].cpu().numpy().astype(np.float32))                                 # the fp32 copy is the rounded fp64
        uv, z = scene.cams[k].project(p64[k].cpu().numpy())
        px = pixel[k].cpu().numpy()
        assert np.abs(uv - np.stack([px % W + 0.5, px // W + 0.5], 1)).max() <= 1e-9
        assert np.abs(z - scene.want[k][0].reshape(-1)[px]).max() <= 1e-9


def test_pick_with_enough_pixels_picks_none_twice(scene, cloud):
    """N = 256 on views of 277, 452 and 375 valid pixels: the strata [floor(j n / N), floor((j + 1) n / N)) are disjoint and none is empty, so
    every pick is another pixel, and the picks keep the row-major order."""
    from etch_amd.depth import pick
    _, _, pixel = pick(cloud, 256, KEYS)
    distinct = [len(np.unique(pixel[k].cpu().numpy())) for k in range(3)]
    print("distinct pixels of 256 picks per view:", distinct, "valid pixels:", [len(c[0]) for c in scene.clouds])
    assert distinct == [256, 256, 256]
    assert all((np.diff(pixel[k].cpu().numpy()) > 0).all() for k in range(3))


def test_empty_view_raises_and_a_callers_frame_is_compacted_by_the_validity_rule(scene, rendered):
    from etch_amd._lib import EtchHipError
    from etch_amd.depth import pick, unproject
    depth = rendered.depth.clone()
    depth[1] = math.inf
    c = unproject(depth, scene.cams)
    assert c.count.cpu().numpy().tolist() == [len(scene.clouds[0][0]), 0, len(scene.clouds[2][0])]
    with pytest.raises(EtchHipError, match="view 1.*no pixel"):
        pick(c, 16, KEYS)
    # a caller's 33 x 17 frame (numpy, float32) with zeros, negatives, NaN, inf and values on both sides of [near, far]
    rng = np.random.default_rng(3)
    frame = rng.uniform(0.0, 4.0, (2, 17, 33)).astype(np.float32)
    frame[0, ::3, ::2] = 0.0
    frame[0, 5, 5], frame[0, 6, 6], frame[1, 0, 0], frame[1, 16, 32] = np.nan, np.inf, -1.0, -np.inf
    frame[1, 2, 3], frame[1, 2, 4] = 0.5, 3.0                                                        # the bounds themselves are outside
    cams = [_camera(scene.v, az, f=25.0, h=17, w=33) for az in (0.4, 3.0)]
    c = unproject(frame, cams, near=0.5, far=3.0, device=DEV)
    off = c.offsets.cpu().numpy()
    for k in range(2):
        index, world = DO.unproject(frame[k].astype(np.float64), cams[k].row(), near=0.5, far=3.0)
        assert 100 < len(index) < 561 and off[k + 1] - off[k] == len(index)
        p, i = c.view(k)
        assert _same(i, index) and _same(p, world)
    with pytest.raises(ValueError):
        unproject(frame, cams[:1])
    with pytest.raises(ValueError):
        unproject(frame, cams, near=1.0, far=1.0)


def _pixel_rays(cam):
    o, d = DO.pixel_rays(cam.row(), cam.height, cam.width)
    return torch.from_numpy(o).to(DEV), torch.from_numpy(np.ascontiguousarray(d)).to(DEV)


def _mesh_tensors(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(DEV), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV)


def test_ray_caster_sees_the_same_image(scene, rendered):
    """The independent cross-check: ops.ray_first_hit (Moller-Trumbore, csrc/raycast.hip) along the pixel-centre rays of the 64 x 48 view at
    1.1 rad.  The rays have camera-frame direction (., ., 1), so t d_z = t is the depth."""
    from etch_amd import ops
    o, d = _pixel_rays(scene.cams[1])
    face, t, _, _ = ops.ray_first_hit(o, d, *_mesh_tensors(scene.v, scene.f))
    face, t = face.cpu().numpy(), t.cpu().numpy()
    z, zf = rendered.depth[1].cpu().numpy().reshape(-1), rendered.face[1].cpu().numpy().reshape(-1)
    hit = zf >= 0
    print(f"{hit.sum()} covered pixels, {(hit != (face >= 0)).sum()} coverage and {(zf != face).sum()} face differences, max |z - t| {np.abs(z[hit] - t[hit]).max():.2e}")
    assert np.array_equal(hit, face >= 0) and np.array_equal(zf, face)
    assert np.abs(z[hit] - t[hit]).max() <= 1e-12


def _assert_visible(points, eye, v, f, tol=1e-9):
    """Every point is what its camera sees along the ray through it: the first hit of the ray from the eye lies within tol of the point."""
    from etch_amd import ops
    p = torch.from_numpy(np.ascontiguousarray(points, np.float64)).to(DEV)
    o = torch.from_numpy(np.broadcast_to(eye, points.shape).copy()).to(DEV)
    face, t, _, loc = ops.ray_first_hit(o, (p - o).contiguous(), *_mesh_tensors(v, f))
    assert (face.cpu().numpy() >= 0).all()
    err = float((loc - p).norm(dim=1).max())
    assert err <= tol, err


def test_partial_view_points(scene):
    from etch_amd._lib import EtchHipError
    from etch_amd.depth import Camera, partial_view_points
    N = 256
    pv = partial_view_points([scene.body], scene.cams, N, KEYS, device=DEV)
    assert pv.points.shape == (3, N, 3) and pv.points.dtype == torch.float32 and pv.dropped.cpu().numpy().tolist() == [0, 0, 0]
    assert pv.cloud.offsets.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(c[0]) for c in scene.clouds])]).tolist()
    for k, (index, world) in enumerate(scene.clouds):
        c = DO.bbox_mid(world)
        assert _same(pv.centers[k], c)
        assert _same(pv.cloud.view(k)[0], world)
        w64, w32, wpix, _ = DO.pick(index, world, N, KEYS[k], center=c)
        assert _same(pv.points64[k], w64) and _same(pv.points[k], w32) and _same(pv.pixel[k], wpix)
        _assert_visible(pv.points64[k].cpu().numpy() + c, scene.cams[k].eye, scene.v, scene.f)
    raw = partial_view_points([scene.body], scene.cams, N, KEYS, center=False, device=DEV)
    assert raw.centers is None
    for k, (index, world) in enumerate(scene.clouds):
        assert _same(raw.points64[k], DO.pick(index, world, N, KEYS[k])[0])
    away = Camera.look_at(scene.center + [0.0, 0.0, 2.5], scene.center + [0.0, 0.0, 5.0], fx=F, cx=W / 2.0, cy=H / 2.0, width=W, height=H)
    with pytest.raises(EtchHipError, match="view 1.*no pixel"):
        partial_view_points([scene.body], [scene.cams[0], away], N, KEYS[:2], device=DEV)
    with pytest.raises(ValueError):
        partial_view_points([scene.body], scene.cams, N, [1, 2], device=DEV)                         # three views, two keys


# ---- the data set and the commands ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return _train_data.build(tmp_path_factory.mktemp("depth_data"), DEV)


def _dataset(data, view):
    from etch_amd import train
    from etch_amd.datasets import GTDataset
    import json
    args = train.build_parser().parse_args(data.flags)
    with open(args.markerset_path) as fh:
        args.markerset = json.load(fh)
    return GTDataset(args, device=DEV, verbose=False, view=view)


def test_gtdataset_items_seen_by_one_camera(data):
    from etch_amd.depth import ViewSpec
    from etch_amd.inference_demo import load_obj
    full, ds = _dataset(data, None), _dataset(data, ViewSpec(probability=1.0, distance=2.5, fov_deg=45.0, size=(96, 128)))
    today, again = full[1], _dataset(data, None)[1]
    item = ds[1]
    assert list(item.keys()) == list(today.keys()) and item["id"] == today["id"] and item["gender"] == today["gender"]
    for k in ("hitpts", "vectors", "confidences", "labels"):
        assert item[k].dtype == today[k].dtype and item[k].shape == today[k].shape
        assert torch.equal(today[k], again[k])                                                       # view=None is the item of today, bit for bit
        assert torch.isfinite(item[k].double()).all()
    assert not torch.equal(item["hitpts"], today["hitpts"])
    scan = load_obj(os.path.join(data.root, "scan", item["id"], f"{item['id']}.obj"))
    cam = ds.view_camera(1)
    # hitpts are the fp32 rounding of the picked fp64 points, and those are visible (an fp32 point is off the surface by up to 2e-7 m, which a
    # ray that grazes its face turns into any distance along the ray: the test of visibility is made on the points before the rounding)
    p64 = ds._view_points(1, scan, cam)
    assert np.array_equal(item["hitpts"].numpy(), p64.astype(np.float32))
    _assert_visible(p64, cam.eye, scan.vertices, scan.faces)
    twice = ds[1]
    assert all(torch.equal(item[k], twice[k]) for k in ("hitpts", "vectors", "confidences", "labels"))
    ds.set_epoch(1)
    assert not np.array_equal(ds.view_camera(1).row(), cam.row()) and not torch.equal(ds[1]["hitpts"], item["hitpts"])
    ds.set_epoch(0)
    assert torch.equal(ds[1]["hitpts"], item["hitpts"])
    assert full.view_camera(1) is None


def test_train_program_with_partial_views(data, tmp_path, monkeypatch):
    import json
    from etch_amd import train
    from etch_amd.models.models_pointcloud import GT_network_equiv
    # the model announces its train() mode path once per process, and test_gpu_train.py asserts that announcement: hand the switch back afterwards
    monkeypatch.setattr(GT_network_equiv, "_warned_switch", GT_network_equiv._warned_switch)
    last = train.main(data.flags + ["--epochs", "2", "--output_root", str(tmp_path), "--partial_views", "1", "--view_size", "96", "128", "--max_steps", "2"])
    assert last and all(math.isfinite(v) for v in last.values()), last
    with open(os.path.join(_train_data.folder(tmp_path), "training_args.json")) as fh:
        saved = json.load(fh)
    assert saved["partial_views"] == 1.0 and saved["view_size"] == [96, 128] and saved["view_elevation"] == [-10.0, 30.0]


@pytest.fixture(scope="module")
def model_path(data):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return path


def test_depth_command_from_a_virtual_view_and_from_its_depth_frame(data, model_path, tmp_path):
    from etch_amd import depth as D
    scan = os.path.join(data.root, "scan", "a_0001", "a_0001.obj")
    common = ["--model_path", model_path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]
    a, b = tmp_path / "a", tmp_path / "b"
    D.main(["--scan_path", scan, "--view_azimuth", "30", "--view_elevation", "10", "--view_size", "96", "128", "--output_folder", str(a)] + common)
    assert {"a_0001_view.npz", "a_0001_pred_smpl.obj", "a_0001_output_smpl_info.npz"} <= set(os.listdir(a))
    va = np.load(a / "a_0001_view.npz")
    assert va["depth"].shape == (96, 128) and va["points"].shape == (1024, 3) and va["points"].dtype == np.float32 and va["camera"].shape == (16,)
    assert np.isfinite(va["depth"]).sum() > 500
    np.save(tmp_path / "frame.npy", va["depth"])                                                     # background is +inf: not finite, so background
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = va["camera"][4:13].reshape(3, 3), va["camera"][13:]
    np.save(tmp_path / "E.npy", E)
    D.main(["--depth_path", str(tmp_path / "frame.npy"), "--intrinsics"] + [repr(float(x)) for x in va["camera"][:4]] +
           ["--extrinsics", str(tmp_path / "E.npy"), "--output_folder", str(b)] + common)
    assert {"frame_view.npz", "frame_pred_smpl.obj", "frame_output_smpl_info.npz"} <= set(os.listdir(b))
    vb = np.load(b / "frame_view.npz")
    for k in ("points", "pixel", "center", "depth", "camera"):
        assert _same(va[k], vb[k]), k
    ia, ib = np.load(a / "a_0001_output_smpl_info.npz"), np.load(b / "frame_output_smpl_info.npz")
    assert sorted(ia.files) == sorted(ib.files) == ["betas", "body_pose", "global_orient", "hand_pose", "joints", "transl"]
    assert all(np.isfinite(ia[k]).all() for k in ia.files)


def test_eval_command_under_a_virtual_camera(data, tmp_path):
    from etch_amd import eval as E
    flags = ["--activated_ids_path", os.path.join(data.root, "ids.pkl"), "--markerset_path", os.path.join(data.root, "markers.json"),
             "--infopoints_dir", os.path.join(data.root, "ip"), "--scan_dir", os.path.join(data.root, "scan"), "--smpl_dir", os.path.join(data.root, "smpl"),
             "--num_point", "512", "--batch_size", "2", "--seed", "3", "--synthetic_body", "--output_root", str(tmp_path)]
    recs, avg = E.main(flags + ["--i", "view", "--view_azimuth", "30", "--view_size", "96", "128"])
    assert [r["id"] for r in recs] == ["a_0001", "b_0002"] and math.isfinite(avg) and all(math.isfinite(r["v2v"]) for r in recs)
    with pytest.raises(SystemExit):
        E.main(flags + ["--i", "host", "--view_azimuth", "30", "--ingest", "host"])
