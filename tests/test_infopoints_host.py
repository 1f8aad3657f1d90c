"""CPU checks of the info-point generation: the reference's output files from the fixture's reference arrays, the CLI's argument set, the
thinning rule and the fp64 restatement (tests/_raycast_oracle.py) on hand-computed cases, and the wrappers' refusal of host tensors."""
import os

import numpy as np
import pytest
import torch

import _raycast_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infopoints_4ddress.npz")


def test_fixture_keys_and_dtypes():
    d = np.load(GOLDEN)
    assert d["scan_vertices_e8"].dtype == d["body_vertices_e8"].dtype == np.int32
    assert d["scan_faces"].dtype == d["body_faces"].dtype == np.int32
    fx = O.load_fixture(GOLDEN)
    K = len(fx["records"])
    assert fx["info_points"].shape == fx["info_vectors"].shape == (K, 3) and fx["info_points"].dtype == np.float64 and K > 500
    assert len(fx["ply_lines"]) == K and len(fx["scan"].faces) > 5000 and len(fx["body_inner"].faces) > 500
    # every kept record's body point lies in the band the fixture was cut for
    y0, y1, _ = fx["band"]
    s = fx["info_points"] - fx["info_vectors"]
    assert (s[:, 1] >= y0).all() and (s[:, 1] <= y1).all()


def test_ply_reproduces_reference_bytes(tmp_path):
    """The reference .ply's header (counts aside) and, for every kept record, its two vertex lines, byte for byte."""
    from etch_amd.infopoints import save_points_with_vector

    fx = O.load_fixture(GOLDEN)
    K = len(fx["records"])
    p = tmp_path / "x.ply"
    save_points_with_vector(None, fx["info_points"], fx["info_vectors"], str(p))
    ours = p.read_bytes().split(b"\n")
    ref_header = fx["ply_header"].replace(b"element vertex 23752\n", b"element vertex %d\n" % (2 * K)).replace(b"element edge 11876\n",
                                                                                                             b"element edge %d\n" % K)
    assert b"\n".join(ours[:13]) + b"\n" == ref_header
    for i in range(K):
        assert ours[13 + i] + b"\n" + ours[13 + K + i] + b"\n" == fx["ply_lines"][i], i
    assert ours[13 + 2 * K:] == [b"%d %d" % (i, K + i) for i in range(K)] + [b""]


def test_npz_keys_and_dtypes(tmp_path):
    from etch_amd.infopoints import save_data

    fx = O.load_fixture(GOLDEN)
    K = len(fx["records"])
    p = tmp_path / "x.npz"
    save_data(fx["info_points"], fx["info_vectors"], str(p))
    g = np.load(p)
    assert sorted(g.keys()) == ["info_points", "info_vectors"]
    for k in g.keys():
        assert g[k].dtype == np.float64 and g[k].shape == (K, 3)
        assert np.array_equal(g[k], fx[k])
    save_data(np.zeros((0, 3)), np.zeros((0, 3)), str(tmp_path / "empty.npz"))
    assert np.load(tmp_path / "empty.npz")["info_points"].shape == (0, 3)


def test_cli_parses_reference_arguments():
    from etch_amd.generate_infopoints import parse_args

    a = parse_args(["-p", "1", "-m", "0", "-l", "0.2", "-l_ops", "0.01", "--num_samples", "123", "-f_m", "M", "-f_s", "S", "-f_p", "P", "-f_n",
                    "N", "-s", "scan.obj", "-b", "body.obj"])
    assert (a.mode, a.ray_length, a.ray_length_ops, a.num_samples) == (0, 0.2, 0.01, 123)
    assert (a.folder_model, a.folder_smpl, a.folder_ply, a.folder_npz, a.scan_obj, a.body_obj) == ("M", "S", "P", "N", "scan.obj", "body.obj")
    assert (a.seed, a.self_face) == (0, "exclude")
    d = parse_args([])
    assert (d.mode, d.ray_length, d.ray_length_ops, d.num_samples) == (0, 0.16, 0.025, 30000)
    assert parse_args(["--seed", "3", "--self_face", "reference"]).self_face == "reference"
    with pytest.raises(SystemExit):
        parse_args(["--self_face", "neither"])


def test_pair_ids_sorted_intersection(tmp_path):
    from etch_amd.generate_infopoints import pair_ids

    for d, ids in (("m", ["b", "a", "c"]), ("s", ["c", "a", "d"])):
        for i in ids:
            os.makedirs(tmp_path / d / i)
    (tmp_path / "m" / "file").write_text("")
    assert pair_ids(str(tmp_path / "m"), str(tmp_path / "s")) == ["a", "c"]


def test_thinning_rule_by_hand():
    # points on a line, r = 1: pairs (0,1) (1,2) (3,4) (5,6); 7 alone.  Degrees 1 2 1 1 1 1 1 0.
    # (0,1): deg 1 < 2 -> remove 1; (1,2): 2 > 1 -> remove 1; (3,4): tie -> remove 3 (the i of the pair); (5,6): tie -> remove 5.
    x = np.array([0.0, 1.0, 2.0, 10.0, 11.0, 20.0, 21.0, 30.0])
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    deg, removed = O.remove_close(pts, 1.0)
    assert deg.tolist() == [1, 2, 1, 1, 1, 1, 1, 0]
    assert np.flatnonzero(~removed).tolist() == [0, 2, 4, 6, 7]
    # a triangle of mutual neighbours: degrees 2 2 2, every pair a tie -> 0 (pairs (0,1), (0,2)) and 1 (pair (1,2)) go
    tri = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.25, 0.4, 0]])
    deg, removed = O.remove_close(tri, 1.0)
    assert deg.tolist() == [2, 2, 2] and np.flatnonzero(~removed).tolist() == [2]


def test_oracle_ray_by_hand():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, -1], [2, 0, -1], [0, 2, -1]])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]])
    o = np.array([[0.5, 0.5, 1.0], [0.75, 0.25, 1.0], [0.25, 0.25, -2.0], [-1.0, 0.25, 0.0]])
    d = np.array([[0.0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, 0]])
    face, t, bary, loc = O.ray_first_hit(o, d, v, f)
    assert face.tolist() == [0, 0, -1, -1]             # diagonal shared by faces 0 and 1 -> 0; behind the origin; parallel
    assert t[0] == 1.0 and bary[1].tolist() == [0.25, 0.5, 0.25] and loc[1].tolist() == [0.75, 0.25, 0.0]
    face, t, _, _ = O.ray_first_hit(o[:1], d[:1], v, f, excl=np.array([0]))
    assert face[0] == 1
    face, t, _, _ = O.ray_first_hit(o[:1], d[:1], v, f[[0, 2]], excl=np.array([0]))
    assert face[0] == 1 and t[0] == 2.0
    face, _, _, _ = O.ray_first_hit(o[:1], d[:1], v, f, t_max=np.array([1.0]))
    assert face[0] == -1


def test_oracle_closest_point_regions_by_hand():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [0.5, -1, 0.25], [-0.5, 2, 0], [-1, 0.5, 0], [1, 1, 0.5], [0.25, 0.25, 0.5]])
    q, bary, d2, region = O.closest_on_triangles(pts, a, b, c)
    assert region.tolist() == list(range(7))
    assert q.tolist() == [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]]
    assert bary[2].tolist() == [0.5, 0.5, 0] and bary[5].tolist() == [0, 0.5, 0.5] and bary[6].tolist() == [0.5, 0.25, 0.25]
    assert d2[6] == 0.25 and d2[0] == 2.25


def test_oracle_vertex_normals_of_a_tetrahedron():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    n = O.vertex_normals(v, f)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3), atol=1e-15)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-15)


def test_wrappers_refuse_host_tensors():
    from etch_amd import _lib, ops

    z = torch.zeros(4, 3, dtype=torch.float64)
    fz = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(_lib.EtchHipError):
        ops.ray_first_hit(z, z, z, fz)
    with pytest.raises(_lib.EtchHipError):
        ops.closest_point_on_mesh(z, z, fz)
    with pytest.raises(_lib.EtchHipError):
        ops.vertex_normals(z, fz)
    with pytest.raises(_lib.EtchHipError):
        ops.remove_close(z, 0.1)
