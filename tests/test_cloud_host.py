"""Raw point clouds, host side: the PLY reader and writer, read_cloud's dispatch, the numpy oracle of the cloud kernels
against a second formulation of itself, and the C ABI's new names.  No GPU call."""
import os
import struct

import numpy as np
import pytest

import _cloud_oracle as CO

from etch_amd import _lib, mesh_io

RNG = np.random.default_rng(7)
V64 = RNG.standard_normal((23, 3))
V64[0] = [1e-300, -0.0, 1.0 + 2.0 ** -52]                    # values a text or fp32 detour would change
FACES = np.array([[0, 1, 2], [2, 3, 4], [22, 21, 20]], np.int64)
FMT = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}
CODE = {"char": "b", "uchar": "B", "short": "h", "ushort": "H", "int": "i", "uint": "I", "float": "f", "double": "d"}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def make_ply(fmt, elements):
    """elements: [(name, [(property, type) or (property, count type, item type)], rows)]; a row is a list with one value per property (a list
    value for a list property).  Written by hand, independently of mesh_io.format_ply."""
    head = ["ply", f"format {fmt} 1.0", "comment made by the test", "obj_info nothing"]
    for name, props, rows in elements:
        head.append(f"element {name} {len(rows)}")
        head += [f"property list {p[1]} {p[2]} {p[0]}" if len(p) == 3 else f"property {p[1]} {p[0]}" for p in props]
    out = ("\n".join(head + ["end_header"]) + "\n").encode()
    e = FMT[fmt]
    for name, props, rows in elements:
        for row in rows:
            if e is None:
                txt = []
                for p, val in zip(props, row):
                    txt += [str(len(val))] + [repr(x) for x in val] if len(p) == 3 else [repr(val)]
                out += (" ".join(txt) + "\n").encode()
            else:
                for p, val in zip(props, row):
                    if len(p) == 3:
                        out += struct.pack(e + CODE[p[1]], len(val)) + struct.pack(e + CODE[p[2]] * len(val), *val)
                    else:
                        out += struct.pack(e + CODE[p[1]], val)
    return out


def _vertex_rows(v, dtype):
    return [[dtype(x).item() for x in row] for row in v]


@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("vtype", ["float", "double"])
def test_ply_round_trip_and_hand_written_files(tmp_path, fmt, vtype):
    dt = np.float32 if vtype == "float" else np.float64
    v = V64.astype(dt)
    # our writer -> our reader (binary and ascii forms of the writer; the big-endian form is covered by the hand-written file below)
    if fmt != "binary_big_endian":
        path = tmp_path / "w.ply"
        mesh_io.write_ply(mesh_io.Mesh(v, FACES), path, binary=fmt != "ascii")
        got = mesh_io.read_ply(path)
        assert np.array_equal(_bits(got.vertices), _bits(v.astype(np.float64))) and got.vertices.dtype == np.float64      # exact, -0 and 1e-300 included
        assert np.array_equal(got.faces, FACES) and got.faces.dtype == np.int64 and got.normals is None and got.colors is None
        mesh_io.write_ply(v, path, binary=fmt != "ascii")                 # points alone: no face element
        got = mesh_io.read_ply(path)
        assert np.array_equal(_bits(got.vertices), _bits(v.astype(np.float64))) and got.faces.shape == (0, 3)
    # a hand-written file in every format
    path = tmp_path / "h.ply"
    props = [("x", vtype), ("y", vtype), ("z", vtype)]
    path.write_bytes(make_ply(fmt, [("vertex", props, _vertex_rows(v, dt)), ("face", [("vertex_indices", "uchar", "int")], [[list(map(int, f))] for f in FACES])]))
    got = mesh_io.read_ply(path)
    assert np.array_equal(_bits(got.vertices), _bits(v.astype(np.float64))) and np.array_equal(got.faces, FACES)


@pytest.mark.parametrize("fmt", list(FMT))
def test_ply_shuffled_properties_extra_elements_and_polygons(tmp_path, fmt):
    v = V64.astype(np.float32)
    n = RNG.standard_normal((23, 3)).astype(np.float32)
    rgba = RNG.integers(0, 256, (23, 4))
    props = [("nz", "float"), ("y", "float"), ("quality", "short"), ("red", "uchar"), ("x", "float"), ("alpha", "uchar"), ("nx", "float"),
             ("z", "float"), ("blue", "uchar"), ("ny", "float"), ("green", "uchar")]
    col = {"x": v[:, 0], "y": v[:, 1], "z": v[:, 2], "nx": n[:, 0], "ny": n[:, 1], "nz": n[:, 2], "red": rgba[:, 0], "green": rgba[:, 1],
           "blue": rgba[:, 2], "alpha": rgba[:, 3], "quality": np.arange(23) - 5}
    rows = [[col[p[0]][i].item() for p in props] for i in range(23)]
    extra = [("weights", "uchar", "float"), ("tag", "int"), ("ids", "ushort", "uint")]            # lists of varying length before `vertex`
    extra_rows = [[[0.5] * (i % 3), i, list(range(i))] for i in range(4)]
    polys = [[[0, 1, 2, 3, 4]], [[5, 6, 7]], [[8, 9]], [[10, 11, 12, 13]]]                         # a pentagon, a triangle, a 2-gon (dropped), a quad
    tail = [("edge", [("a", "int"), ("b", "int")], [[1, 2], [3, 4]])]
    path = tmp_path / "s.ply"
    for face_types, face_name in ((("uchar", "int"), "vertex_indices"), (("uint", "uint"), "vertex_index")):
        path.write_bytes(make_ply(fmt, [("camera", extra, extra_rows), ("vertex", props, rows), ("face", [(face_name,) + face_types], polys)] + tail))
        got = mesh_io.read_ply(path)
        assert np.array_equal(_bits(got.vertices), _bits(v.astype(np.float64)))
        assert np.array_equal(got.normals, n.astype(np.float64)) and np.array_equal(got.colors, rgba) and got.colors.shape == (23, 4)
        want = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 6, 7], [10, 11, 12], [10, 12, 13]]               # fanned (i0, ik, ik+1), as read_obj fans
        assert np.array_equal(got.faces, want)
    # red green blue without alpha
    path.write_bytes(make_ply(fmt, [("vertex", [p for p in props if p[0] != "alpha"], [[x for p, x in zip(props, r) if p[0] != "alpha"] for r in rows])]))
    assert mesh_io.read_ply(path).colors.shape == (23, 3)


def test_malformed_ply_files_name_the_file_and_the_defect(tmp_path):
    v = V64[:5]
    props = [("x", "double"), ("y", "double"), ("z", "double")]
    face = ("face", [("vertex_indices", "uchar", "int")], [[[0, 1, 4]]])
    path = tmp_path / "bad.ply"

    def check(data, match):
        path.write_bytes(data)
        with pytest.raises(ValueError, match=match) as e:
            mesh_io.read_ply(path)
        assert "bad.ply" in str(e.value)

    for fmt in FMT:
        good = make_ply(fmt, [("vertex", props, _vertex_rows(v, np.float64)), face])
        path.write_bytes(good)
        assert len(mesh_io.read_ply(path).vertices) == 5
        check(good[:-3] if fmt != "ascii" else good[:good.rfind(b"4")], "truncated")                 # a truncated body
        check(good[:good.find(b"end_header") + 11 + 20], "truncated")
        check(make_ply(fmt, [("vertex", [("u", "double"), ("y", "double"), ("z", "double")], _vertex_rows(v, np.float64))]), "missing x|no property x")
        check(good.replace(b"property double y", b"property half y"), "unknown type `half`")
        check(good.replace(b"element vertex 5", b"element vertex -5"), "does not fit")
        check(good.replace(b"element vertex 5", b"element vertex 99999999999"), "does not fit")
        check(good.replace(b"element vertex 5", b"element vertex five"), "does not fit")
        check(make_ply(fmt, [("vertex", props, _vertex_rows(v, np.float64)), ("face", face[1], [[[0, 1, 5]]])]), "index 5 is out of range")
        check(make_ply(fmt, [("vertex", props, _vertex_rows(v, np.float64)), ("face", face[1], [[[0, -1, 2]]])]), "index -1 is out of range")
    check(b"plx\n", "not a PLY")
    check(b"ply\nformat ascii 1.0\nelement vertex 0\n", "end_header")
    check(b"ply\nformat binary_middle_endian 1.0\nend_header\n", "unsupported format")


def test_read_cloud_dispatches_on_the_extension(tmp_path):
    v = V64
    mesh_io.write_ply(v, tmp_path / "c.ply")
    mesh_io.write_obj(mesh_io.Mesh(v, FACES), tmp_path / "c.obj")
    np.save(tmp_path / "c.npy", v.astype(np.float32))
    np.savez(tmp_path / "c.npz", points=v, other=np.zeros(3))
    np.savez(tmp_path / "one.npz", anything=v)
    (tmp_path / "c.xyz").write_text("# x y z intensity\n" + "".join(f"{a!r} {b!r} {c!r} 7\n" for a, b, c in v.tolist()))
    (tmp_path / "c.txt").write_text("".join(f"{a!r} {b!r} {c!r}\n" for a, b, c in v.tolist()))
    for name in ("c.ply", "c.npz", "one.npz", "c.xyz", "c.txt"):
        got = mesh_io.read_cloud(tmp_path / name)
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(v)), name
    assert np.array_equal(mesh_io.read_cloud(tmp_path / "c.npy"), v.astype(np.float32).astype(np.float64))
    assert np.allclose(mesh_io.read_cloud(tmp_path / "c.obj"), v, atol=1e-8, rtol=0)                 # the OBJ writer keeps 8 decimals
    np.save(tmp_path / "flat.npy", np.zeros(9))
    np.savez(tmp_path / "two.npz", a=v, b=v)
    (tmp_path / "c.stl").write_text("solid")
    for name, match in (("flat.npy", r"\(M,3\)"), ("two.npz", "name the cloud"), ("c.stl", r"\.ply")):
        with pytest.raises(ValueError, match=match) as e:
            mesh_io.read_cloud(tmp_path / name)
        assert name in str(e.value)


def test_oracle_against_a_second_formulation_of_itself():
    import torch
    p = np.random.default_rng(3).standard_normal((300, 3)) * [0.2, 0.6, 0.1]
    p[17] = p[3]                                                          # a coincident pair counts, at distance 0
    for k in (1, 8, 32):
        d = torch.cdist(torch.from_numpy(p), torch.from_numpy(p), compute_mode="donot_use_mm_for_euclid_dist")
        d[torch.arange(300), torch.arange(300)] = float("inf")
        want = d.topk(k, dim=1, largest=False).values.sum(1).numpy() / k
        got = CO.knn_mean(p, k)
        assert np.abs(got - want).max() <= 1e-12 * want.max()
        assert got[17] == got[3] and (k > 1 or got[17] == 0.0)
    assert np.array_equal(CO.knn_mean(p[:1], 8), [0.0]) and np.array_equal(CO.knn_mean(p[:2], 8), np.full(2, np.sqrt(CO.d2_rows(p, [0])[0, 1])))
    r = 0.08
    d = torch.cdist(torch.from_numpy(p), torch.from_numpy(p), compute_mode="donot_use_mm_for_euclid_dist").numpy()
    near = np.abs(d - r) < 1e-9                                           # no pair sits on the radius, so the two counts must agree exactly
    assert not near.any() and np.array_equal(CO.radius_count(p, r), (d <= r).sum(1) - 1)
    for voxel in (0.05, 0.31):
        cell, cent, count, lowest = CO.voxel_grid(p, voxel)
        u, first, inv, cnt = np.unique(CO.voxel_cells(p, voxel), axis=0, return_index=True, return_inverse=True, return_counts=True)
        assert np.array_equal(cell, u) and np.array_equal(count, cnt) and np.array_equal(lowest, first) and count.sum() == 300
        mean = np.stack([np.bincount(inv.reshape(-1), p[:, a]) for a in range(3)], 1) / cnt[:, None]
        assert np.abs(cent - mean).max() < 1e-15
        single = np.flatnonzero(count == 1)
        assert len(single) and np.array_equal(_bits(cent[single]), _bits(p[lowest[single]]))
    m = CO.knn_mean(p, 8)
    keep, mu, s, margin = CO.stat_keep(m, 1.5)
    assert mu == pytest.approx(np.mean(m), rel=1e-14) and s == pytest.approx(np.std(m, ddof=1), rel=1e-13) and margin > 0
    assert np.array_equal(keep, m <= np.mean(m) + 1.5 * np.std(m, ddof=1)) and 0 < keep.sum() < 300
    pts, idx, off = CO.compact([p, p[:5]], [keep, [1, 0, 0, 1, 1]])
    assert off.tolist() == [0, keep.sum(), keep.sum() + 3] and idx[-3:].tolist() == [0, 3, 4] and np.array_equal(pts[-3:], p[[0, 3, 4]])


def test_the_abi_declares_the_cloud_calls_and_the_package_binds_them():
    names = _lib.declared_symbols()
    for n in ("etch_cloud_cell_keys", "etch_cloud_knn_mean", "etch_cloud_radius_count", "etch_cloud_stat_keep", "etch_cloud_compact",
              "etch_cloud_voxel_grid"):
        assert n in names, n
    from etch_amd import build as B
    assert B.EXTRA["cloud_filter.hip"] == ["-ffp-contract=off"]
    from etch_amd import cloud, ops
    for f in ("cloud_knn_mean", "cloud_radius_count", "cloud_stat_keep", "cloud_compact", "cloud_voxel_grid"):
        assert callable(getattr(ops, f)), f
    for f in ("pack", "knn_mean_distance", "remove_statistical_outliers", "remove_radius_outliers", "voxel_downsample", "prepare"):
        assert callable(getattr(cloud, f)), f
    hdr = open(_lib.HEADER).read()
    assert all(f"#define ETCH_CLOUD_STATUS_{n} {v}" in hdr for n, v in (("NONFINITE", cloud.STATUS_NONFINITE), ("RANGE", cloud.STATUS_RANGE),
                                                                        ("EMPTY", cloud.STATUS_EMPTY)))


def test_bad_arguments_raise_before_any_launch_and_flags_default_to_off():
    """ValueError without a GPU: the argument checks run before the first launch (here there is no device to launch on)."""
    from etch_amd import cloud, depth
    a = cloud.build_parser().parse_args(["--cloud_path", "x.ply"])
    assert (a.voxel, a.outlier_k, a.outlier_radius, a.chamfer_refine) == (0.0, 0, 0.0, "none") and cloud.filter_args(a) == (None, None)
    assert cloud.build_parser().parse_args(["--cloud_path", "x.ply", "--chamfer_refine"]).chamfer_refine == "partial"
    d = depth.build_parser().parse_args(["--scan_path", "s.obj", "--view_azimuth", "0"])
    assert (d.outlier_k, d.outlier_ratio, d.outlier_radius, d.outlier_min_neighbours) == (0, 2.0, 0.0, 2)
    with pytest.raises(SystemExit):
        cloud.parse_args(["--cloud_path", "x.ply", "--outlier_k", "33"])
    with pytest.raises(SystemExit):
        depth.parse_args(["--scan_path", "s.obj", "--view_azimuth", "0", "--outlier_k", "40"])
    for k in (0, 33, 2.5):
        with pytest.raises(ValueError, match="k must"):
            cloud._check_k(k)
    with pytest.raises(ValueError, match="radius must be positive"):
        cloud._check_radius(0.0, 2)
    with pytest.raises(ValueError, match="voxel must be positive"):
        cloud._check_positive(-1.0, "voxel")
    with pytest.raises(ValueError, match="cloud 1"):
        cloud.pack([np.zeros((2, 3)), np.zeros((2, 2))], device="cpu")
