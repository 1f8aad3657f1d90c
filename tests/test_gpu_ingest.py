"""Native scan ingestion on the GPU: the surface sampler and the bounding-box centre against tests/_sampler_oracle.py, bit for
bit; GTDataset(reader="native"); `python -m etch_amd.eval` and `inference_demo --ingest device` end to end on a two-id dataset on disk (built as
test_gpu_train_program builds its own: the geodesic fixture's body, whose 6 890 vertices are what the synthetic body model fits; 1 024 points)."""
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import _geodesic_oracle as GO
import _raycast_oracle as RO
import _sampler_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
BAND = os.path.join(HERE, "golden", "infopoints_4ddress.npz")
BODY = os.path.join(HERE, "golden", "geodesic_4ddress.npz")
NUM_POINT = 1024
KEYS = [15, 2 ** 63 + 5, 2 ** 64 - 1, 7]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.fixture(scope="module")
def batch():
    """The ragged batch: a single face; 65 faces (a full tile and one); 127 faces of which the first and the whole second tile (the last face
    with it) have no area; the 7 035-face band.  The oracle's result for every N and both centre settings is computed once and shared."""
    from etch_amd.inference_demo import Mesh
    rng = np.random.default_rng(5)
    strip = lambda n: np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)
    m0 = Mesh(np.array([[0.25, -1.0, 2.0], [1.5, 0.5, 2.25], [-0.75, 0.125, 3.0]]), np.array([[2, 0, 1]]))
    m1 = Mesh(rng.standard_normal((67, 3)) * [0.3, 0.9, 0.2] + [0.1, 1.0, -0.2], strip(65))
    f2 = strip(127)
    f2[0] = [3, 3, 9]
    f2[64:] = np.stack([np.arange(63), np.arange(63), np.arange(63) + 1], 1)
    m2 = Mesh(rng.standard_normal((129, 3)), f2)
    band = RO.load_fixture(BAND)["scan"]
    m3 = Mesh(band.vertices, band.faces)
    meshes = [m0, m1, m2, m3]
    assert [len(m.faces) for m in meshes] == [1, 65, 127, 7035]
    centers = np.stack([S.bbox_center(m.vertices) for m in meshes])
    want = {}
    for n in (1, 65, 1000):
        for c in (False, True):
            want[n, c] = [S.sample_surface(m.vertices, m.faces, KEYS[k], n, centers[k] if c else None) for k, m in enumerate(meshes)]
    return types.SimpleNamespace(meshes=meshes, centers=centers, want=want)


def _check(got, want_rows, centers, center):
    p32, face, c, p64 = got
    if center:
        assert np.array_equal(_bits(c.cpu().numpy()), _bits(centers))
    else:
        assert c is None
    assert p32.dtype == torch.float32 and p64.dtype == torch.float64 and face.dtype == torch.int32
    for k, (w64, w32, wface, _) in enumerate(want_rows):
        assert np.array_equal(face[k].cpu().numpy(), wface), k
        assert np.array_equal(_bits(p64[k].cpu().numpy()), _bits(w64)), k
        assert np.array_equal(_bits(p32[k].cpu().numpy()), _bits(w32)), k


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_sampler_equals_the_oracle_bit_for_bit(batch, n, center):
    from etch_amd import mesh_io
    got = mesh_io.sample_surface(batch.meshes, n, KEYS, center=center, device=DEV, return_fp64=True)
    _check(got, batch.want[n, center], batch.centers, center)
    face = got[1].cpu().numpy()
    for k, m in enumerate(batch.meshes):
        _, e1, e2 = S.corners(m.vertices, m.faces, batch.centers[k] if center else None)
        assert np.all(S.face_areas(e1, e2)[face[k]] > 0.0), k              # a face without area is never drawn
    assert face[2].max() < 64 and face[2].min() >= 1


def test_a_scan_does_not_depend_on_its_batch(batch):
    from etch_amd import mesh_io
    n = 1000
    for k, m in enumerate(batch.meshes):
        got = mesh_io.sample_surface([m], n, [KEYS[k]], center=True, device=DEV, return_fp64=True)
        _check(got, [batch.want[n, True][k]], batch.centers[k:k + 1], True)
    got = mesh_io.sample_surface(batch.meshes[::-1], n, KEYS[::-1], center=True, device=DEV, return_fp64=True)
    _check(got, batch.want[n, True][::-1], batch.centers[::-1], True)
    # one key for all: every scan under the same key
    p32, face, _ = mesh_io.sample_surface(batch.meshes[:2], 65, 15, center=False, device=DEV)
    for k in range(2):
        assert np.array_equal(face[k].cpu().numpy(), S.sample_surface(batch.meshes[k].vertices, batch.meshes[k].faces, 15, 65)[2])


def test_points_lie_on_their_face(batch):
    """Recomputed on the host from the face id: the point is within 1e-12 of the face's plane, and inside the triangle.  The barycentric
    coordinates are solved from the point, so they carry its rounding (a few ulp of coordinates below 4, < 2e-15) over the triangle's smallest
    altitude: the bound is 1e-14 / altitude per face."""
    from etch_amd import mesh_io
    _, face, _, p64 = mesh_io.sample_surface(batch.meshes, 1000, KEYS, center=False, device=DEV, return_fp64=True)
    for k, m in enumerate(batch.meshes):
        f = face[k].cpu().numpy()
        p = p64[k].cpu().numpy()
        tri = m.vertices[m.faces[f]]
        e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], p - tri[:, 0]
        nrm = np.cross(e1, e2)
        area2 = np.linalg.norm(nrm, axis=1)
        assert np.all(np.abs(np.einsum("ij,ij->i", d, nrm / area2[:, None])) <= 1e-12), k
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        b1, b2 = (d * e1).sum(1), (d * e2).sum(1)
        det = g11 * g22 - g12 * g12
        u1, u2 = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
        longest = np.sqrt(np.maximum(np.maximum(g11, g22), ((e2 - e1) ** 2).sum(1)))
        tol = 1e-14 / (area2 / longest)
        assert np.all(u1 >= -tol) and np.all(u2 >= -tol) and np.all(u1 + u2 <= 1 + tol), k


def test_status_word_and_host_validation(batch):
    from etch_amd import mesh_io
    from etch_amd._lib import EtchHipError
    from etch_amd.inference_demo import Mesh
    good = batch.meshes[1]
    flat = Mesh(good.vertices, np.stack([np.arange(65), np.arange(65), np.arange(65) + 1], 1))       # only faces without area
    with pytest.raises(EtchHipError, match="mesh 1.*area"):
        mesh_io.sample_surface([good, flat], 65, KEYS[:2], device=DEV)
    v = np.vstack([good.vertices, [[0.0, np.inf, 0.0]]])           # a vertex no face names: the areas stay finite, only the vertex scan sees it
    with pytest.raises(EtchHipError, match="mesh 0.*not finite"):
        mesh_io.sample_surface([Mesh(v, good.faces), good], 65, KEYS[:2], device=DEV)
    v = good.vertices.copy()
    v[5, 2] = np.nan
    with pytest.raises(EtchHipError, match="mesh 1"):
        mesh_io.sample_surface([good, Mesh(v, good.faces)], 65, KEYS[:2], device=DEV)
    # an index outside the scan is refused on the host, before any launch: ValueError, which EtchHipError (a RuntimeError) is not
    for bad in (67, -1):
        f = good.faces.copy()
        f[64, 2] = bad
        with pytest.raises(ValueError, match="mesh 1"):
            mesh_io.sample_surface([good, Mesh(good.vertices, f)], 65, KEYS[:2], device=DEV)
    with pytest.raises(ValueError):
        mesh_io.sample_surface([good, Mesh(good.vertices, np.zeros((0, 3), np.int64))], 65, KEYS[:2], device=DEV)
    # and the sampler still works afterwards
    _, face, _ = mesh_io.sample_surface([good], 65, [KEYS[1]], center=False, device=DEV)
    assert np.array_equal(face[0].cpu().numpy(), batch.want[65, False][1][2])


# ------------------------------------------------------------------------------------------------ the dataset on disk and the programs
def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.writelines(f"v {x:.8f} {y:.8f} {z:.8f}\n" for x, y, z in v)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.inference_demo import Mesh, load_obj
    from etch_amd.infopoints import generate_infopoints, save_data
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded

    root = tmp_path_factory.mktemp("ingest_data")
    z = GO.load_fixture(BODY)
    verts, faces = z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)
    ids = ["a_0001", "b_0002"]
    body = Mesh(verts, faces)
    n = ops.vertex_normals(torch.as_tensor(verts, device=DEV), torch.as_tensor(faces, device=DEV).to(torch.int32)).cpu().numpy()
    os.makedirs(root / "ip")
    for k, i in enumerate(ids):
        off = np.random.default_rng(k).uniform(0.01, 0.03, (len(verts), 1))
        for d in ("scan", "smpl"):
            os.makedirs(root / d / i)
        _write_obj(root / "scan" / i / f"{i}.obj", verts + off * n, faces)
        _write_obj(root / "smpl" / i / f"mesh_smpl_{i}.obj", verts, faces)
        np.savez(root / "smpl" / i / f"info_{i}.npz", gender=np.array(k), joints=np.random.default_rng(10 + k).standard_normal((24, 3)))
        ip, iv, _ = generate_infopoints(load_obj(str(root / "scan" / i / f"{i}.obj")), body, num_samples=3000, seed=k, device=DEV)
        save_data(ip, iv, str(root / "ip" / f"{i}.npz"))
    with open(root / "ids.pkl", "wb") as fh:
        pickle.dump(ids, fh)
    with open(root / "markers.json", "w") as fh:
        json.dump(K.default_markerset(), fh)
    opt = types.SimpleNamespace(output_folder=str(root / "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), str(root / "model.pth"))
    flags = ["--activated_ids_path", str(root / "ids.pkl"), "--markerset_path", str(root / "markers.json"), "--infopoints_dir", str(root / "ip"),
             "--scan_dir", str(root / "scan"), "--smpl_dir", str(root / "smpl"), "--num_point", str(NUM_POINT), "--batch_size", "1", "--seed", "3",
             "--synthetic_body", "--model_path", str(root / "model.pth"), "--output_root", str(root / "out")]
    return types.SimpleNamespace(root=root, flags=flags, ids=ids)


def test_gtdataset_native_reader_gives_the_same_items(data):
    from etch_amd import constants as K
    from etch_amd.datasets import GTDataset
    args = types.SimpleNamespace(seed=3, scan_dir=str(data.root / "scan"), smpl_dir=str(data.root / "smpl"), infopoints_dir=str(data.root / "ip"),
                                 activated_ids_path=str(data.root / "ids.pkl"), num_point=NUM_POINT, markerset=K.default_markerset())
    a = GTDataset(args, device=DEV, verbose=False)
    b = GTDataset(args, device=DEV, verbose=False, reader="native")
    a.precompute(batch_size=2)
    b._fields = a._fields                                          # the marker fields do not go through the reader under test
    assert len(a) == len(b) == 2
    for k in range(2):
        x, y = a[k], b[k]
        assert set(x) == set(y) and x["id"] == y["id"] and x["gender"] == y["gender"]
        for key in ("hitpts", "vectors", "confidences", "labels"):
            assert x[key].dtype == y[key].dtype and torch.equal(x[key], y[key]), (k, key)
    with pytest.raises(ValueError):
        GTDataset(args, device=DEV, verbose=False, reader="fast")


def _outputs(folder, ids):
    """-> {relative name: bytes, or the arrays of an .npz} of an evaluation folder.  np.savez stamps each zip member with the wall clock, so two
    runs' .npz files differ in those bytes whatever the program does: they are compared array by array, exactly."""
    out = {"v2v_score.txt": open(os.path.join(folder, "v2v_score.txt"), "rb").read()}
    for i in ids:
        assert sorted(os.listdir(os.path.join(folder, i))) == [f"forwarded_smpl_mesh_on_pred_{i}.obj", f"output_smpl_info_{i}.npz"]
        out[f"{i}.obj"] = open(os.path.join(folder, i, f"forwarded_smpl_mesh_on_pred_{i}.obj"), "rb").read()
        z = np.load(os.path.join(folder, i, f"output_smpl_info_{i}.npz"))
        out[f"{i}.npz"] = {k: z[k] for k in z.files}
    return out


def _same_outputs(a, b):
    assert set(a) == set(b)
    for name in a:
        if name.endswith(".npz"):
            assert set(a[name]) == set(b[name]) == {"body_pose", "hand_pose", "betas", "global_orient", "transl", "joints"}
            for k in a[name]:
                assert a[name][k].dtype == b[name][k].dtype and np.array_equal(a[name][k], b[name][k]), (name, k)
        else:
            assert a[name] == b[name], name


def test_eval_command_with_host_ingest_equals_a_direct_call(data):
    from etch_amd import eval as E
    from etch_amd.inference_demo import load_model, resolve_body_model
    from etch_amd.train import default_stuff
    recs, avg = E.main(data.flags + ["--i", "host", "--ingest", "host"])
    assert [r["id"] for r in recs] == data.ids and all("mpjpe" in r for r in recs) and avg == pytest.approx(np.mean([r["v2v"] for r in recs]))
    args = E.build_parser().parse_args(data.flags + ["--i", "direct"])
    args.device = torch.device(DEV)
    direct = args.output_folder = str(data.root / "out" / "direct")
    default_stuff(args.seed)
    with open(args.markerset_path) as fh:
        args.markerset = json.load(fh)
    resolve_body_model(args)
    model = load_model(args)
    ds = E.EvalDataset(args.scan_dir, args.smpl_dir, args.infopoints_dir, args.activated_ids_path, num_point=NUM_POINT, seed=args.seed)
    recs2, avg2 = E.evaluate_dataset(args, model, ds, batch_size=1, output_folder=direct)
    assert avg2 == avg and recs2 == recs
    _same_outputs(_outputs(str(data.root / "out" / "eval_outputs_host"), data.ids), _outputs(direct, data.ids))


def test_eval_command_with_device_ingest(data, monkeypatch):
    from etch_amd import eval as E
    from etch_amd import mesh_io
    from etch_amd.inference_demo import load_obj
    seen, written = [], []
    real_batch, real_write = E.evaluate_batch, mesh_io.write_obj
    monkeypatch.setattr(E, "evaluate_batch", lambda args, model, hitpts, *a, **k: (seen.append(hitpts.clone()), real_batch(args, model, hitpts, *a, **k))[1])
    monkeypatch.setattr(mesh_io, "write_obj", lambda mesh, path: (written.append((mesh.copy(), path)), real_write(mesh, path))[1])
    recs, _ = E.main(data.flags + ["--i", "dev1", "--prefetch", "1"])                   # --ingest device is the command's default
    assert [r["id"] for r in recs] == data.ids and len(seen) == 2 and len(written) == 2
    out1 = _outputs(str(data.root / "out" / "eval_outputs_dev1"), data.ids)
    for k, i in enumerate(data.ids):
        # the points the model saw: the oracle's for the scan as load_obj reads it, every id under the key seed + 15, not centred
        scan = load_obj(str(data.root / "scan" / i / f"{i}.obj"))
        want = S.sample_surface(scan.vertices, scan.faces, 3 + 15, NUM_POINT)[1]
        assert seen[k].shape == (1, NUM_POINT, 3) and np.array_equal(_bits(seen[k][0].cpu().numpy()), _bits(want))
        mesh, path = written[k]
        assert path.endswith(f"forwarded_smpl_mesh_on_pred_{i}.obj")
        mesh.export(str(data.root / "python_export.obj"))
        assert open(str(data.root / "python_export.obj"), "rb").read() == out1[f"{i}.obj"]
    E.main(data.flags + ["--i", "dev0", "--prefetch", "0"])
    _same_outputs(out1, _outputs(str(data.root / "out" / "eval_outputs_dev0"), data.ids))


def test_inference_demo_with_device_ingest(data, tmp_path):
    from etch_amd import inference_demo as D
    from etch_amd import mesh_io
    i = data.ids[0]
    D.main(["--scan_path", str(data.root / "scan" / i / f"{i}.obj"), "--model_path", str(data.root / "model.pth"), "--markerset_path",
            str(data.root / "markers.json"), "--output_folder", str(tmp_path), "--num_point", str(NUM_POINT), "--synthetic_body", "--seed", "4",
            "--ingest", "device"])
    assert {f"{i}_output_smpl_info.npz", f"{i}_pred_smpl.obj"} <= set(os.listdir(tmp_path))
    got, want = mesh_io.read_obj(str(tmp_path / f"{i}_pred_smpl.obj")), D.load_obj(str(tmp_path / f"{i}_pred_smpl.obj"))
    assert got.vertices.shape == (6890, 3) and got.faces.shape == (13776, 3)
    assert np.array_equal(_bits(got.vertices), _bits(want.vertices)) and np.array_equal(got.faces, want.faces)
    assert set(np.load(tmp_path / f"{i}_output_smpl_info.npz").files) == {"body_pose", "hand_pose", "betas", "global_orient", "transl", "joints"}
