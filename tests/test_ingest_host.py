"""Host side of the native scan ingestion, no GPU: the OBJ reader against inference_demo.load_obj, the writer against
Mesh.export, read_objs, a sanitizer build of csrc/obj_io.h driven by tests/host/obj_io_main.cpp, and self-checks of tests/_sampler_oracle.py
(the restatement the GPU tests compare the sampler with)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _raycast_oracle as RO
import _sampler_oracle as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "infopoints_4ddress.npz")

# a quad and a pentagon, v/vt/vn, v//vn and v/vt tokens, colours after xyz, CRLF and LF ends, comments, blank lines, vn and vt lines, an indented
# line and "v<TAB>" (both skipped), exponent and '+' forms, a two-token face, a forward reference (vertex 6) and no final newline
GOOD = (b"# a comment\r\n"
        b"\r\n"
        b"v 0 0 0 0.5 0.25 1.0\r\n"
        b"v 1.0 0 0\n"
        b"v +1 1e0 0\r\n"
        b"v 0 1.5E+0 -0\n"
        b"v 5e-1 2 .5\r\n"
        b"vn 0 0 1\r\n"
        b"vt 0.5 0.5\n"
        b"  v 9 9 9\r\n"
        b"v\t9 9 9\r\n"
        b"\n"
        b"f 1 2 3 4\r\n"
        b"f 1/1/1 2/2/1 3/3/1 4/4/1 5/5/1\n"
        b"f 1//1 2//1 3//1\r\n"
        b"f 1/1 2/2 6/3\r\n"
        b"f 1 2\n"
        b"# the vertex the face above already names\n"
        b"v 2 2 2\r\n"
        b"f 6 5 4")

# name -> (text, the 1-based line of the error)
MALFORMED = {
    "index_0": (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", 4),
    "index_nv_plus_1": (b"v 0 0 0\nv 1 0 0\nv 0 1 0\n\nf 1 2 4\n", 5),
    "negative_index": (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -1\n", 4),
    "two_coordinates": (b"v 0 0 0\nv 1 2\n", 2),
    "bad_coordinate": (b"# c\nv 1 x 3\n", 2),
    "bad_face_token": (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3abc\n", 4),
    "index_of_30_digits": (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 " + b"1" * 30 + b"\n", 4),
    "hex_float": (b"v 0x1p3 0 0\n", 1),
}


@pytest.fixture(scope="module")
def fx():
    return RO.load_fixture(GOLDEN)


def _same(a, b):
    assert a.vertices.dtype == b.vertices.dtype == np.float64 and a.faces.dtype == b.faces.dtype == np.int64
    assert a.vertices.shape == b.vertices.shape and a.faces.shape == b.faces.shape
    assert np.array_equal(a.vertices.view(np.int64), b.vertices.view(np.int64)) and np.array_equal(a.faces, b.faces)


def test_reader_equals_load_obj_on_an_exported_scan(fx, tmp_path):
    from etch_amd import mesh_io
    from etch_amd.inference_demo import Mesh, load_obj
    path = str(tmp_path / "scan.obj")
    Mesh(fx["scan"].vertices, fx["scan"].faces).export(path)
    got = mesh_io.read_obj(path)
    assert got.vertices.shape == (3562, 3) and got.faces.shape == (7035, 3)
    _same(got, load_obj(path))


def test_reader_equals_load_obj_on_a_hand_written_text(tmp_path):
    from etch_amd import mesh_io
    from etch_amd.inference_demo import load_obj
    path = str(tmp_path / "hand.obj")
    with open(path, "wb") as fh:
        fh.write(GOOD)
    want = load_obj(path)
    assert want.vertices.shape == (6, 3) and want.faces.shape == (2 + 3 + 1 + 1 + 1, 3)      # the two-token face yields nothing
    _same(mesh_io.read_obj(path), want)
    _same(mesh_io.parse_obj(GOOD), want)


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_text_raises_with_file_and_line(name, tmp_path):
    from etch_amd import mesh_io
    text, line = MALFORMED[name]
    path = str(tmp_path / f"{name}.obj")
    with open(path, "wb") as fh:
        fh.write(text)
    with pytest.raises(ValueError) as e:
        mesh_io.read_obj(path)
    assert path in str(e.value) and f"line {line}:" in str(e.value)


def _export_bytes(mesh, path):
    mesh.export(path)
    with open(path, "rb") as fh:
        return fh.read()


def test_writer_is_byte_identical_to_mesh_export(fx, tmp_path):
    from etch_amd import mesh_io
    from etch_amd.inference_demo import Mesh
    body = Mesh(fx["body"].vertices, fx["body"].faces)
    mesh_io.write_obj(body, str(tmp_path / "native.obj"))
    with open(tmp_path / "native.obj", "rb") as fh:
        assert fh.read() == _export_bytes(body, str(tmp_path / "python.obj"))
    # rounding and sign: ties of the ninth decimal, negative zero and values that round to it, large magnitudes, float32 input
    v = np.array([[-0.0, 1e-9, 123456.123456789], [-2.5e-9, 0.5, -1.0], [0.000000005, 0.000000015, -0.000000025], [1e15, -1e22, 1e-300],
                  [2.0 ** -27, 1 / 3, -2 / 3]])
    f = np.array([[0, 1, 2], [4, 3, 0]])
    for mesh in (Mesh(v, f), Mesh(v.astype(np.float32), f.astype(np.int32)), Mesh(np.array([[1e300, -1e300, 1.7976931348623157e308]]), np.zeros((0, 3), np.int64))):
        assert mesh_io.format_obj(mesh) == _export_bytes(mesh, str(tmp_path / "values.obj"))


def test_read_objs_returns_every_file_in_order(fx, tmp_path):
    from etch_amd import mesh_io
    from etch_amd.inference_demo import Mesh
    paths = []
    for k in range(8):
        paths.append(str(tmp_path / f"copy_{k}.obj"))
        Mesh(fx["body"].vertices + k, fx["body"].faces).export(paths[-1])      # the copies differ by a shift, so a swapped order shows
    meshes = mesh_io.read_objs(paths)
    assert len(meshes) == 8
    for k, m in enumerate(meshes):
        _same(m, mesh_io.read_obj(paths[k]))
        assert np.array_equal(m.faces, fx["body"].faces) and abs(m.vertices[0, 0] - (fx["body"].vertices[0, 0] + k)) < 1e-7
    assert mesh_io.MAX_WORKERS == 16


def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_obj_io_header_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/obj_io.h compiled alone by the host compiler with -fsanitize=address,undefined into a program of its own (no sanitizer is ever loaded
    into python): the good text, every malformed text and every truncation of the good text's first 200 bytes."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "obj_io_main")
    src = os.path.join(HERE, "host", "obj_io_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "etch_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", exe]
    # the sanitizer runtimes linked into the program where the compiler has them as archives (g++; clang links them so by default)
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    files = [str(tmp_path / "good.obj")] + [str(tmp_path / f"{n}.obj") for n in sorted(MALFORMED)]
    for p, text in zip(files, [GOOD] + [MALFORMED[n][0] for n in sorted(MALFORMED)]):
        with open(p, "wb") as fh:
            fh.write(text)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and lines[0] == f"{files[0]} rc=0 line=0 nv=6 nf=8"
    for p, n, out in zip(files[1:], sorted(MALFORMED), lines[1:]):
        rc, line = (int(t.split("=")[1]) for t in out[len(p) + 1:].split()[:2])
        assert rc in (-3, -4, -5) and line == MALFORMED[n][1], out


def test_oracle_philox_known_answer():
    r = S.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [int(x) for x in r] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # Random123's second vector: counter and key all ones
    r = S.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(x) for x in r] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    uf, u1, u2 = S.uniforms(15, 4096)
    assert uf.min() >= 0.0 and uf.max() < 1.0 and u1.min() > 0.0 and u1.max() < 1.0 and u2.min() > 0.0 and u2.max() < 1.0


def test_oracle_cumulative_areas_are_monotone(fx):
    _, e1, e2 = S.corners(fx["scan"].vertices, fx["scan"].faces)
    area = S.face_areas(e1, e2)
    cum = S.cumulative_areas(area)
    assert len(cum) == 7035 and np.all(np.diff(cum) >= 0.0) and cum[0] == area[0]
    assert abs(cum[-1] - area.sum()) <= 1e-12 * cum[-1]
    assert np.array_equal(S.cumulative_areas(area[:64]), np.cumsum(area[:64]))          # one tile is a plain running sum


@pytest.mark.parametrize("key", [15, 16, 17, 18])
def test_oracle_draws_faces_by_area(key):
    """Two triangles of areas 3 : 1, 4 096 samples: face 0 is drawn 3 072 +- 139 times (5 sigma of the binomial, sigma = sqrt(4096 * 3/4 * 1/4))."""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [1, 0, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 2]])
    p, p32, face, cum = S.sample_surface(v, f, key, 4096)
    assert cum[0] == 3.0 and cum[1] == 4.0
    assert abs(int((face == 0).sum()) - 3072) <= 139
    assert np.all(p[:, 2] == 0.0) and np.all(p[:, 0] >= 0) and np.all(p[:, 1] >= 0) and np.all(p[:, 0] / 3 + p[:, 1] / 2 <= 1 + 1e-15)
