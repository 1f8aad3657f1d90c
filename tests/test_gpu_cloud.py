"""Raw point clouds on the GPU: the grid kNN mean distance, the radius counts, the statistical filter, the compaction and
the voxel grid of csrc/cloud_filter.hip against tests/_cloud_oracle.py, the grid against the brute-force form of the same kernels, and the
cloud / depth commands on the fixture body with stray points.  Clouds of at most 7 030 points; every oracle result is computed once."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _cloud_oracle as CO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (1, 8, 32)
CELLS = (0.25, 0.07, 1.3)


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _np(t):
    return t.cpu().numpy()


def _split(values, clouds):
    o = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    v = _np(values)
    assert len(v) == o[-1]
    return [v[a:b] for a, b in zip(o[:-1], o[1:])]


@pytest.fixture(scope="module")
def small():
    """The small clouds, by name, left unchanged."""
    rng = np.random.default_rng(11)
    g = np.arange(-2, 3) * 0.25
    line = rng.uniform(-1.0, 1.0, 100)[:, None] * np.array([1.0, 2.0, -0.5]) + [0.3, -0.2, 0.1]
    body = rng.standard_normal((256, 3)) * [0.15, 0.4, 0.1]
    ints = np.concatenate([np.stack(np.meshgrid(np.arange(0, 12, 3.0), np.arange(-4, 8, 4.0), [0.0, 5.0], indexing="ij"), -1).reshape(-1, 3),
                           [[3.0, 4.0, 0.0], [-5.0, 0.0, 0.0], [0.0, -3.0, 4.0]]])
    return {"one": rng.standard_normal((1, 3)), "two": rng.standard_normal((2, 3)), "nine": rng.standard_normal((9, 3)),
            "r33": rng.standard_normal((33, 3)) * [0.2, 0.5, 0.1], "r257": rng.standard_normal((257, 3)) * [0.2, 0.5, 0.1] + [5.0, -3.0, 0.5],
            "copies": np.repeat(rng.standard_normal((1, 3)), 40, 0),
            "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3),            # exact multiples of the cell size 0.25, negative ones too
            "line": line, "far": np.concatenate([body[:100], [[1000.0, 0.0, 0.0]], body[100:]]),     # one point 1 000 m from 256 others
            "ints": ints}                                                                          # pairs at exactly d2 == 25: (3,4,0), (5,0,0), (0,3,4) offsets


@pytest.fixture(scope="module")
def fixture_cloud():
    p, stray = CO.stray_fixture()
    return types.SimpleNamespace(p=p, stray=stray)


def _knn(clouds, k, **kw):
    from etch_amd import cloud as C
    return C.knn_mean_distance(C.pack(clouds, DEV), k, **kw)


@pytest.mark.parametrize("k", KS)
def test_knn_mean_distance_equals_the_oracle_in_every_form(small, k):
    names = list(small)
    clouds = [small[n] for n in names]
    assert {len(c) for c in clouds} >= {1, 2, k + 1}                        # n = 1, 2 and k + 1 are among them for every k
    want = [CO.knn_mean(c, k) for c in clouds]
    got = _knn(clouds, k)
    worst = 0.0
    for n, g, w in zip(names, _split(got, clouds), want):
        err = np.abs(g - w)
        worst = max(worst, float((err / np.maximum(w, 1e-300)).max()))
        assert (err <= 1e-13 * w + 1e-300).all(), (n, float(err.max()))                # the rule that assumes nothing about the device's sqrt
        assert _same(g, w), n                                                           # measured: the device's fp64 sqrt rounds correctly, so the bits
    print(f"k={k}: largest relative difference from the oracle {worst:.3e}")
    assert (_split(got, clouds)[names.index("copies")] == 0.0).all() and _split(got, clouds)[0][0] == 0.0
    for kw in [dict(cell=c) for c in CELLS] + [dict(brute=True)]:
        assert _same(_knn(clouds, k, **kw), got), kw                         # the same bits for any cell size and from the brute-force scan
    assert _same(_knn(clouds, k), got)                                       # two runs
    for n in ("far", "lattice", "two"):                                      # a cloud alone = the same cloud in the batch
        assert _same(_knn([small[n]], k), _split(got, clouds)[names.index(n)]), n
    far = _split(got, clouds)[names.index("far")]
    assert far[100] > 990.0 and far.max() == far[100]                        # the far point took the fallback, and finished


def test_knn_ragged_batch_equals_each_cloud_alone(small):
    rng = np.random.default_rng(12)
    big = rng.standard_normal((5000, 3)) * [0.2, 0.6, 0.12]
    clouds = [small["one"], small["r257"], big]
    got = _knn(clouds, 16)
    parts = _split(got, clouds)
    for c, g in zip(clouds, parts):
        assert _same(_knn([c], 16), g)
    assert _same(_knn(clouds, 16, brute=True), got) and _same(_knn(clouds[::-1], 16)[:5000], parts[2])
    w = CO.knn_mean(big, 16)
    assert _same(parts[2], w)


def test_radius_counts_equal_the_oracle_exactly(small, fixture_cloud):
    from etch_amd import cloud as C
    for names, r in ((["one", "two", "r33", "r257", "copies", "line", "far"], 0.3), (["lattice", "one"], 0.25), (["ints", "nine"], 5.0)):
        clouds = [small[n] for n in names]
        want = [CO.radius_count(c, r) for c in clouds]
        got = C.radius_neighbour_count(C.pack(clouds, DEV), r)
        assert got.dtype == torch.int32
        for n, g, w in zip(names, _split(got, clouds), want):
            assert np.array_equal(g, w), n
        assert _same(C.radius_neighbour_count(C.pack(clouds, DEV), r, brute=True), got)
    d2 = CO.d2_rows(small["ints"], np.arange(len(small["ints"])))
    assert (d2 == 25.0).sum() >= 6 and (CO.d2_rows(small["lattice"], np.arange(125)) == 0.0625).sum() >= 100    # pairs sit exactly on the radius
    p = fixture_cloud.p
    got = C.radius_neighbour_count(C.pack([p], DEV), 0.03)
    assert np.array_equal(_np(got), CO.radius_count(p, 0.03))
    kept, keep = C.remove_radius_outliers(C.pack([p, small["r33"]], DEV), 0.03, 3)
    want_keep = [CO.radius_count(p, 0.03) >= 3, CO.radius_count(small["r33"], 0.03) >= 3]
    pts, idx, off = CO.compact([p, small["r33"]], want_keep)
    assert np.array_equal(_np(keep), np.concatenate(want_keep)) and _same(kept.points, pts) and np.array_equal(_np(kept.index), idx)
    assert np.array_equal(_np(kept.offsets), off)


@pytest.mark.parametrize("k,ratio,stray_removed,margin", [(8, 1.0, 140, 1.9e-2), (16, 2.0, 129, 3.3e-3)])
def test_statistical_filter_on_the_fixed_fixture(fixture_cloud, small, k, ratio, stray_removed, margin):
    from etch_amd import cloud as C
    p, stray = fixture_cloud.p, fixture_cloud.stray
    assert p.shape == (7030, 3) and stray.sum() == 140
    m = CO.knn_mean(p, k)
    keep, mu, s, got_margin = CO.stat_keep(m, ratio)
    # the fixture's guard: the oracle's own counts, and no m_i near enough to the threshold for a rounding to flip it
    assert (~keep & stray).sum() == stray_removed and (~keep & ~stray).sum() == 0 and got_margin > 1e-6
    assert got_margin == pytest.approx(margin, rel=0.05)
    other = small["r257"]
    keep2 = CO.stat_keep(CO.knn_mean(other, k), ratio)[0]
    out, gkeep, stats = C.remove_statistical_outliers(C.pack([other, p], DEV), k=k, ratio=ratio, return_stats=True)
    assert gkeep.dtype == torch.bool and np.array_equal(_np(gkeep), np.concatenate([keep2, keep]))           # the masks, exactly
    gmu, gs = _np(stats)[1]
    print(f"k={k} ratio={ratio}: mu {gmu!r} (oracle {mu!r}), s {gs!r} (oracle {s!r})")
    assert abs(gmu - mu) <= 1e-12 * mu and abs(gs - s) <= 1e-12 * s
    pts, idx, off = CO.compact([other, p], [keep2, keep])
    assert _same(out.points, pts) and np.array_equal(_np(out.index), idx) and np.array_equal(_np(out.offsets), off)
    assert np.array_equal(_np(out.count), np.diff(off))
    alone, akeep = C.remove_statistical_outliers(C.pack([p], DEV), k=k, ratio=ratio)
    assert np.array_equal(_np(akeep), keep) and _same(alone.points, p[keep])


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_voxel_grid_equals_the_oracle(fixture_cloud, small):
    from etch_amd import cloud as C
    from etch_amd._lib import EtchHipError
    clouds = [small["r33"], fixture_cloud.p, small["one"], small["lattice"]]
    for voxel in (0.05, 0.25):
        out, count = C.voxel_downsample(C.pack(clouds, DEV), voxel)
        cells, cents, counts, lows = zip(*[CO.voxel_grid(c, voxel) for c in clouds])
        off = np.concatenate([[0], np.cumsum([len(c) for c in cells])])
        assert np.array_equal(_np(out.offsets), off)
        assert np.array_equal(_np(out.cell), np.concatenate(cells))                                       # the cell set and its order
        assert np.array_equal(_np(count), np.concatenate(counts)) and np.array_equal(_np(out.index), np.concatenate(lows))
        got, want = _np(out.points), np.concatenate(cents)
        ulps = _ulps(got, want)
        print(f"voxel {voxel}: centroids differ from the oracle's same-order sums by at most {np.nanmax(ulps[want != 0.0], initial=0.0)} ulp")
        assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all()
        for b, c in enumerate(clouds):
            assert counts[b].sum() == len(c) == _np(count)[off[b]:off[b + 1]].sum()
        single = np.flatnonzero(np.concatenate(counts) == 1)
        rows = np.concatenate([c[l] for c, l in zip(clouds, lows)])
        assert len(single) > 50 and _same(got[single], rows[single])                                      # a single-point cell returns the point's bits
    alone, count1 = C.voxel_downsample(C.pack([fixture_cloud.p], DEV), 0.05)
    c1 = CO.voxel_grid(fixture_cloud.p, 0.05)
    assert np.array_equal(_np(alone.cell), c1[0]) and np.array_equal(_np(count1), c1[2])
    with pytest.raises(EtchHipError, match="cloud 1.*2\\^21"):
        C.voxel_downsample(C.pack([small["copies"], fixture_cloud.p], DEV), 5e-7)                         # 1.7 m / 5e-7 m > 2^21 cells; cloud 0 has one cell
    with pytest.raises(EtchHipError, match="cloud 1.*no point"):
        C.voxel_downsample(C.pack([small["r33"], np.zeros((0, 3))], DEV), 0.1)


def test_errors(small):
    from etch_amd import cloud as C
    from etch_amd import ops
    from etch_amd._lib import EtchHipError
    bad = small["r257"].copy()
    bad[200, 1] = np.nan
    clouds = [small["r33"], bad, small["line"]]
    packed = C.pack(clouds, DEV)
    for call in (lambda: C.knn_mean_distance(packed, 8), lambda: C.radius_neighbour_count(packed, 0.3), lambda: C.remove_statistical_outliers(packed, 8, 1.0),
                 lambda: C.voxel_downsample(packed, 0.1), lambda: C.prepare(packed, 64, [1], stat=(8, 1.0))):
        with pytest.raises(EtchHipError, match="cloud 1: a coordinate is not finite"):
            call()
    mean, status = ops.cloud_knn_mean(packed.points, packed.offsets, 8)
    assert _np(status).tolist() == [0, C.STATUS_NONFINITE, 0]
    parts = _split(mean, clouds)
    assert _same(parts[0], _knn([clouds[0]], 8)) and _same(parts[2], _knn([clouds[2]], 8))                # clouds 0 and 2 are still correct
    good = C.pack([small["r33"], small["line"]], DEV)
    for call in (lambda: C.knn_mean_distance(good, 0), lambda: C.knn_mean_distance(good, 33), lambda: C.remove_radius_outliers(good, 0.0, 2),
                 lambda: C.radius_neighbour_count(good, 0.0), lambda: C.voxel_downsample(good, 0.0), lambda: C.remove_statistical_outliers(good, k=33),
                 lambda: C.knn_mean_distance(good, 8, cell=0.0), lambda: C.prepare(good, 16, [1, 2, 3])):
        with pytest.raises(ValueError):
            call()
    good.offsets = torch.tensor([0, 100, 33], dtype=torch.int32, device=DEV)                             # descending offsets
    entered = []
    from etch_amd import _lib
    lib = _lib.lib()
    lib.profiler = lambda name, args, fn: entered.append(name) or fn(*args)
    try:
        for call in (lambda: C.knn_mean_distance(good, 8), lambda: C.voxel_downsample(good, 0.1), lambda: C.knn_mean_distance(packed, 0)):
            with pytest.raises(ValueError):
                call()
    finally:
        lib.profiler = None
    assert entered == []                                                                                  # ... before any launch


def test_prepare_filters_then_voxels_then_picks(fixture_cloud, small):
    from etch_amd import cloud as C
    from etch_amd.depth import bbox_mid
    p, stray = fixture_cloud.p, fixture_cloud.stray
    other = small["r257"]
    pts, centers, clean = C.prepare(C.pack([p, other], DEV), 512, [5, 6], voxel=0.02, stat=(8, 1.0), radius=(0.05, 1))
    k1 = [CO.stat_keep(CO.knn_mean(c, 8), 1.0)[0] for c in (p, other)]
    s1 = [p[k1[0]], other[k1[1]]]
    k2 = [CO.radius_count(c, 0.05) >= 1 for c in s1]
    s2 = [c[k] for c, k in zip(s1, k2)]
    vox = [CO.voxel_grid(c, 0.02) for c in s2]
    keep = [k.copy() for k in k1]
    for a, b in zip(keep, k2):
        a[np.flatnonzero(a)] = b
    assert np.array_equal(_np(clean.keep), np.concatenate(keep)) and not (keep[0] & stray).any()
    assert clean.stages["input"].tolist() == [7030, 257] and clean.stages["statistical"].tolist() == [len(c) for c in s1]
    assert clean.stages["radius"].tolist() == [len(c) for c in s2] and clean.stages["voxel"].tolist() == [len(v[0]) for v in vox]
    want = np.concatenate([v[1] for v in vox])
    got = _np(clean.points)
    assert got.shape == want.shape and (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all()
    for b in range(2):
        mid = bbox_mid(vox[b][1])
        assert np.abs(_np(centers)[b] - mid).max() <= 1e-15
        picked = _np(pts)[b].astype(np.float64) + mid                        # every picked point is a voxel centroid (to fp32), in cell order
        d = np.abs(picked[:, None, :] - vox[b][1][None, :, :]).max(2)
        assert pts.dtype == torch.float32 and (d.min(1) < 1e-6).all() and (np.diff(d.argmin(1)) >= 0).all()
    raw, c_raw, same = C.prepare(C.pack([p], DEV), 512, [5])
    assert np.abs(_np(c_raw)[0] - bbox_mid(p)).max() <= 1e-15 and same.keep.all() and _same(same.points, p)


# ---- the commands -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return _train_data.build(tmp_path_factory.mktemp("cloud_data"), DEV)


@pytest.fixture(scope="module")
def common(data):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return ["--model_path", path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]


def test_cloud_command_on_a_big_endian_ply_with_stray_points(fixture_cloud, common, tmp_path):
    from etch_amd import cloud as C
    from etch_amd.depth import bbox_mid
    p, stray = fixture_cloud.p, fixture_cloud.stray
    head = f"ply\nformat binary_big_endian 1.0\ncomment body with stray points\nelement vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\nend_header\n"
    (tmp_path / "scan.ply").write_bytes(head.encode() + p.astype(">f8").tobytes())
    a, b = tmp_path / "a", tmp_path / "b"
    C.main(["--cloud_path", str(tmp_path / "scan.ply"), "--outlier_k", "8", "--outlier_ratio", "1.0", "--voxel", "0.02", "--output_folder", str(a)] + common)
    assert {"scan_cloud.npz", "scan_pred_smpl.obj", "scan_output_smpl_info.npz"} <= set(os.listdir(a))
    rep = np.load(a / "scan_cloud.npz")
    body_centroids = CO.voxel_grid(p[~stray], 0.02)[1]                       # the filter leaves the body's rows, in their order
    assert np.abs(rep["center"] - bbox_mid(body_centroids)).max() <= 1e-15
    assert int(rep["removed"]) == 140 and np.array_equal(rep["keep"], ~stray)
    assert rep["rows_input"].tolist() == [7030] and rep["rows_statistical"].tolist() == [6890] and rep["rows_voxel"].tolist() == [len(body_centroids)]
    info = np.load(a / "scan_output_smpl_info.npz")
    assert all(np.isfinite(info[k]).all() for k in info.files) and rep["points"].shape == (1024, 3) and np.isfinite(rep["points"]).all()
    from etch_amd.mesh_io import read_obj
    assert np.isfinite(read_obj(a / "scan_pred_smpl.obj").vertices).all()
    C.main(["--cloud_path", str(tmp_path / "scan.ply"), "--output_folder", str(b)] + common)                # the same command without the flags
    raw = np.load(b / "scan_cloud.npz")
    assert np.abs(raw["center"] - bbox_mid(p)).max() <= 1e-15 and int(raw["removed"]) == 0
    assert np.abs(raw["center"] - rep["center"]).max() > 1e-3                                            # the flags act


def test_depth_command_drops_flying_pixels(fixture_cloud, common, tmp_path):
    from etch_amd import depth as D
    z = np.load(CO.GOLDEN)
    v, f = CO.body_vertices(), z["faces"].astype(np.int64)
    H, W, F = 48, 64, 70.0
    c = bbox_mid = (v.min(0) + v.max(0)) / 2.0
    cam = D.Camera.look_at(c + 2.5 * np.array([math.sin(0.4), 0.1, math.cos(0.4)]), c, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, width=W, height=H)
    from etch_amd.inference_demo import Mesh
    frame = _np(D.render([Mesh(v, f)], [cam], device=DEV).depth[0]).copy()
    assert np.isfinite(frame).sum() > 250
    flying = [(3, 5), (8, 55), (40, 7), (44, 60), (24, 2), (20, 61)]                                      # mid-air depths, far from the body and each other
    for i, (r, col) in enumerate(flying):
        assert not np.isfinite(frame[r, col])
        frame[r, col] = 1.0 + 0.1 * i
    np.save(tmp_path / "frame.npy", frame)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = cam.R, cam.t
    np.save(tmp_path / "E.npy", E)
    flags = ["--depth_path", str(tmp_path / "frame.npy"), "--intrinsics"] + [repr(float(x)) for x in cam.row()[:4]] + ["--extrinsics", str(tmp_path / "E.npy")]
    D.main(flags + ["--output_folder", str(tmp_path / "a"), "--outlier_k", "8", "--outlier_ratio", "1.0"] + common)
    D.main(flags + ["--output_folder", str(tmp_path / "b")] + common)
    pix = {r * W + col for r, col in flying}
    with_filter, without = np.load(tmp_path / "a" / "frame_view.npz"), np.load(tmp_path / "b" / "frame_view.npz")
    assert not pix & set(with_filter["pixel"].tolist()) and len(pix & set(without["pixel"].tolist())) >= 1
    assert np.isfinite(with_filter["points"]).all() and with_filter["points"].shape == (1024, 3)
    assert np.abs(with_filter["center"] - without["center"]).max() > 1e-2
    assert {"frame_pred_smpl.obj", "frame_output_smpl_info.npz"} <= set(os.listdir(tmp_path / "a"))
