"""Host side of the raw-cloud normals, no GPU: self-checks of tests/_normals_oracle.py (the restatement the GPU tests compare
the kernel with), csrc/cloud_normal_solve.h built by the host compiler under the address and undefined-behaviour sanitizers and driven by
tests/host/cloud_solve_main.cpp, and normals through write_ply / read_ply / read_cloud."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _normals_oracle as NO
from etch_amd import mesh_io

HERE = os.path.dirname(os.path.abspath(__file__))
U = NO.U


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------------
def test_oracle_tie_goes_to_the_lower_row():
    """3 x 3 x 1 lattice, row = 3 ix + iy: the centre (row 4) has rows 1, 3, 5, 7 at d2 = 2^-8 and the corners at 2^-7; the corner row 0 has rows 1
    and 3 at 2^-8, row 4 at 2^-7 and rows 2 and 6 at 2^-6."""
    p = NO.lattice(3, 3, 1)
    nbr = NO.neighbours(p, 3)
    assert nbr[4].tolist() == [1, 3, 5] and nbr[0].tolist() == [1, 3, 4]
    assert NO.neighbours(p, 4)[0].tolist() == [1, 3, 4, 2] and NO.neighbours(p, 6)[4].tolist() == [1, 3, 5, 7, 0, 2]
    # a permutation of the rows moves the tie with it: the set is a function of the row numbers, not of the positions alone
    perm = np.array([8, 7, 6, 5, 4, 3, 2, 1, 0])
    assert NO.neighbours(p[perm], 3)[4].tolist() == [1, 3, 5]
    assert sorted(perm[NO.neighbours(p[perm], 3)[4]].tolist()) == [3, 5, 7]


def test_oracle_lattice_plane_has_the_exact_normal():
    p = NO.lattice(7, 7, 1)
    for k in (3, 8, 16, 32):
        nrm, var, flag, cov, _ = NO.normals(p, k)
        assert not flag.any() and (cov[:, [2, 4, 5]] == 0.0).all()
        assert (nrm == np.array([0.0, 0.0, 1.0])).all() and (var == 0.0).all()
    # towards a viewpoint under the plane the normal points down; one IN the plane keeps the first rule
    assert (NO.normals(p, 8, viewpoint=[0.1, 0.1, -2.0])[0] == np.array([0.0, 0.0, -1.0])).all()
    assert (NO.normals(p, 8, viewpoint=[5.0, -3.0, 0.0])[0] == np.array([0.0, 0.0, 1.0])).all()


def test_oracle_sphere_normal_is_radial_to_second_order():
    """Unit sphere (curvature 1), near-uniform sample: over a neighbourhood of radius r the surface leaves its tangent plane by r^2 / 2, and on a
    sample that is symmetric to first order the fitted plane tilts by the third-moment term, below r^2; r = the distance to the k-th neighbour."""
    p = NO.sphere(2000)
    nrm, var, flag, _, nbr = NO.normals(p, 16)
    assert not flag.any()
    r = np.sqrt(((p[nbr[:, -1]] - p) ** 2).sum(1))
    cosang = np.abs((nrm * p).sum(1))
    ang = np.arccos(np.minimum(cosang, 1.0))
    assert r.max() < 0.25 and (ang <= r * r).all(), (ang.max(), (ang / (r * r)).max())
    assert (var > 0).all() and (var < r * r).all()
    out = NO.normals(p, 16, viewpoint=[0.0, 0.0, 0.0], nbr=nbr)[0]                   # from the centre every normal points inward
    assert ((out * p).sum(1) < 0).all()
    lead = np.abs(nrm).argmax(1)
    assert (nrm[np.arange(len(p)), lead] > 0).all()


def test_oracle_flags_collinear_coincident_isotropic_and_few():
    nrm, var, flag, _, _ = NO.normals(NO.collinear(9), 4)
    assert (flag == NO.FLAG_AMBIGUOUS).all() and (nrm == 0).all()
    nrm, var, flag, cov, _ = NO.normals(np.repeat([[0.3, -1.0, 2.0]], 12, 0), 5)
    assert (flag == NO.FLAG_AMBIGUOUS).all() and (nrm == 0).all() and (cov == 0).all() and (var == 0).all()
    lat = NO.lattice(5, 5, 5)
    nrm, var, flag, cov, _ = NO.normals(lat, 32)
    centre = (2 * 5 + 2) * 5 + 2                                                 # 26 rows of the 3 x 3 x 3 block and the 6 at distance 2: isotropic
    assert flag[centre] == NO.FLAG_AMBIGUOUS and cov[centre, 0] == cov[centre, 3] == cov[centre, 5] and (cov[centre, [1, 2, 4]] == 0).all()
    for n, want in ((3, 0), (2, NO.FLAG_FEW | NO.FLAG_AMBIGUOUS), (1, NO.FLAG_FEW | NO.FLAG_AMBIGUOUS)):
        q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])[:n]
        nrm, _, flag, _, nbr = NO.normals(q, 16)
        assert nbr.shape == (n, n - 1) and (flag == want).all()
        assert (nrm == ([0.0, 0.0, 1.0] if want == 0 else [0.0, 0.0, 0.0])).all()
    assert NO.normals(np.zeros((0, 3)), 16)[0].shape == (0, 3)


# ---- csrc/cloud_normal_solve.h under the sanitizers ------------------------------------------------------------------------------------------------
def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _matrices():
    """(ke, cov6) cases: random covariances and random symmetric matrices, repeated eigenvalues, rank 1, zero, NaN."""
    rng = np.random.default_rng(41)
    pick = lambda a: a[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    out = []
    for i in range(300):
        a = rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-3, 3)
        out.append((16, pick(a @ a.T if i % 2 else (a + a.T))))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    for d in ((1.0, 1.0, 2.0), (1.0, 2.0, 2.0), (3.0, 3.0, 3.0), (0.0, 0.0, 5.0), (0.0, 1.0, 1.0)):
        out.append((16, pick(np.diag(d))))
        out.append((16, pick(q @ np.diag(d) @ q.T)))
    for _ in range(10):
        v = rng.standard_normal(3)
        out.append((16, pick(np.outer(v, v))))
    out.append((16, np.zeros(6)))
    out.append((1, pick(np.diag([1.0, 2.0, 3.0]))))
    out.append((0, np.zeros(6)))
    out.append((16, np.array([1.0, np.nan, 0.0, 1.0, 0.0, 2.0])))
    out.append((16, np.array([np.inf, 0.0, 0.0, 1.0, 0.0, 2.0])))
    return out


# The Jacobi's backward error.  One rotation replaces six entries by c a - s b with c, s carrying a few u each: the computed matrix is the exact
# rotation of A + E_r with |E_r|_F <= 8 u |A|_F.  At most NORMAL_JACOBI_SWEEPS x 3 = 30 rotations run, so eigenvalues and vectors are exact for
# A + E, |E|_F <= 240 u |A|_F; normalising the vector and the reference's own (LAPACK) error stay inside the remaining 16.  An eigenvalue then
# moves by at most |E|, and the eigenvector of lambda0 turns by at most |E| / (lambda1 - lambda0) to first order.
C_JACOBI = 256.0


def test_solve_header_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/cloud_normal_solve.h compiled alone by the host compiler with -fsanitize=address,undefined into a program of its own (no sanitizer is
    ever loaded into python).  Flags and eigenvalues equal the oracle's restatement by bits; eigenvalues, the residual and the angle to numpy's
    eigh stay within the Jacobi's backward error."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cloud_solve_main")
    src = os.path.join(HERE, "host", "cloud_solve_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "etch_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = _matrices()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as fh:
        for ke, c in cases:
            fh.write("J %d %s\n" % (ke, " ".join(repr(float(x)) for x in c)))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(cases) + 1
    got = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[:-1]])
    flag, lam, nrm, var = got[:, 0].astype(np.int32), got[:, 1:4], got[:, 4:7], got[:, 7]
    worst = 0.0
    for i, (ke, c) in enumerate(cases):
        with np.errstate(all="ignore"):
            olam, onrm, ovar, oflag = NO.solve(c[None], ke)
        assert flag[i] == oflag[0], (i, flag[i], oflag[0])
        assert np.array_equal(lam[i], olam[0], equal_nan=True) and np.array_equal(nrm[i], onrm[0]) and np.array_equal(var[i], ovar[0], equal_nan=True), i
        if not np.isfinite(c).all():
            assert flag[i] & NO.FLAG_AMBIGUOUS and (nrm[i] == 0).all()
            continue
        elam, evec, a = NO.eigh_reference(c[None])
        norm = np.sqrt((a[0] * a[0]).sum())
        assert (np.abs(lam[i] - elam[0]) <= C_JACOBI * U * norm).all(), (i, lam[i], elam[0])
        if flag[i]:
            assert (nrm[i] == 0).all()
            continue
        assert abs(np.sqrt((nrm[i] * nrm[i]).sum()) - 1.0) <= 4 * U
        assert np.sqrt(((a[0] @ nrm[i] - lam[i, 0] * nrm[i]) ** 2).sum()) <= C_JACOBI * U * norm, i
        gap = elam[0, 1] - elam[0, 0]
        sin = np.sqrt((np.cross(nrm[i], evec[0]) ** 2).sum())
        assert sin <= C_JACOBI * U * norm / gap, (i, sin, C_JACOBI * U * norm / gap)
        worst = max(worst, sin * gap / (U * norm))
    print(f"worst angle * gap / (u |C|_F) = {worst:.3g} of {C_JACOBI}")
    by = {tuple(np.round(c, 12)): f for (ke, c), f in zip(cases, flag)}
    pick = lambda d: tuple(np.round(np.diag(d)[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], 12))
    assert by[pick((1.0, 1.0, 2.0))] == NO.FLAG_AMBIGUOUS and by[pick((1.0, 2.0, 2.0))] == 0 and by[pick((3.0, 3.0, 3.0))] == NO.FLAG_AMBIGUOUS
    assert by[pick((0.0, 0.0, 5.0))] == NO.FLAG_AMBIGUOUS and by[pick((0.0, 1.0, 1.0))] == 0
    assert flag[-5] == NO.FLAG_AMBIGUOUS and flag[-4] == (NO.FLAG_FEW) and flag[-3] == (NO.FLAG_FEW | NO.FLAG_AMBIGUOUS)
    assert (flag[-15:-5] == NO.FLAG_AMBIGUOUS).all()                                # rank 1: two zero eigenvalues


# ---- normals in PLY files ------------------------------------------------------------------------------------------------------------------------------
def _cloud(dtype):
    rng = np.random.default_rng(3)
    p = rng.standard_normal((57, 3)).astype(dtype)
    n = rng.standard_normal((57, 3))
    n = (n / np.sqrt((n * n).sum(1))[:, None]).astype(dtype)
    n[5] = 0.0
    return p, n


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ply_normals_round_trip_is_exact(tmp_path, binary, dtype):
    p, n = _cloud(dtype)
    path = str(tmp_path / "c.ply")
    mesh_io.write_ply(p, path, binary=binary, normals=n)
    ply = mesh_io.read_ply(path)
    assert np.array_equal(ply.vertices, p.astype(np.float64)) and np.array_equal(ply.normals, n.astype(np.float64)) and len(ply.faces) == 0
    q, m = mesh_io.read_cloud(path, return_normals=True)
    assert q.dtype == m.dtype == np.float64 and np.array_equal(q, p.astype(np.float64)) and np.array_equal(m, n.astype(np.float64))
    assert np.array_equal(mesh_io.read_cloud(path), q)
    head = open(path, "rb").read().split(b"end_header")[0]
    t = b"float" if dtype == np.float32 else b"double"
    assert [ln for ln in head.split(b"\n") if ln.startswith(b"property")] == [b"property %s %s" % (t, a) for a in (b"x", b"y", b"z", b"nx", b"ny", b"nz")]


def test_ply_normals_big_endian_and_mesh(tmp_path):
    p, n = _cloud(np.float64)
    data = mesh_io.format_ply(p, True, n)
    head, body = data.split(b"end_header\n")
    big = head.replace(b"binary_little_endian", b"binary_big_endian") + b"end_header\n" + np.frombuffer(body, "<f8").astype(">f8").tobytes()
    path = str(tmp_path / "big.ply")
    open(path, "wb").write(big)
    q, m = mesh_io.read_cloud(path, return_normals=True)
    assert np.array_equal(q, p) and np.array_equal(m, n)
    faces = np.array([[0, 1, 2], [2, 3, 56]])
    mesh = mesh_io.PlyData(p, faces)
    for binary in (True, False):
        mesh_io.write_ply(mesh, str(tmp_path / "m.ply"), binary=binary, normals=n)
        ply = mesh_io.read_ply(str(tmp_path / "m.ply"))
        assert np.array_equal(ply.vertices, p) and np.array_equal(ply.normals, n) and np.array_equal(ply.faces, faces)


def test_ply_without_normals_is_unchanged_and_bad_normals_raise(tmp_path):
    p, n = _cloud(np.float64)
    faces = np.array([[0, 1, 2], [2, 3, 4]])
    for obj in (p, p.astype(np.float32), mesh_io.PlyData(p, faces)):
        v = getattr(obj, "vertices", obj)
        t = b"float" if v.dtype == np.float32 else b"double"
        for binary in (True, False):
            head = [b"ply", b"format binary_little_endian 1.0" if binary else b"format ascii 1.0", b"element vertex 57"]
            head += [b"property %s %s" % (t, a) for a in (b"x", b"y", b"z")]
            if obj is not p and v is p:
                head += [b"element face 2", b"property list uchar int vertex_indices"]
            head = b"\n".join(head + [b"end_header"]) + b"\n"
            if binary:
                body = v.astype("<" + v.dtype.str[1:]).tobytes()
                if b"face" in head:
                    body += b"".join(b"\x03" + np.asarray(f, "<i4").tobytes() for f in faces)
            else:
                body = "".join(f"{repr(float(a))} {repr(float(b))} {repr(float(c))}\n" for a, b, c in v.astype(np.float64)).encode()
                if b"face" in head:
                    body += b"3 0 1 2\n3 2 3 4\n"
            assert mesh_io.format_ply(obj, binary) == head + body == mesh_io.format_ply(obj, binary, None)
    path = str(tmp_path / "plain.ply")
    mesh_io.write_ply(p, path)
    assert mesh_io.read_cloud(path, return_normals=True)[1] is None
    np.save(str(tmp_path / "c.npy"), p)
    q, m = mesh_io.read_cloud(str(tmp_path / "c.npy"), return_normals=True)
    assert m is None and np.array_equal(q, p)
    for bad in (n[:-1], n[:, :2], n.astype(str)):
        with pytest.raises(ValueError, match="normals"):
            mesh_io.write_ply(p, path, normals=bad)


# ---- the 6 x 6 point-to-plane solve of csrc/cloud_align_solve.h under the sanitizers ---------------------------------------------------------------
def _plane_systems():
    """(name, m, rho, c, sums32) cases: random well-posed systems at several scales, a tiny step (the series branch), an exact plane with exact
    normals, a zero-diagonal system, too few rows, rho = 0 and a NaN."""
    import _plane_oracle as PO
    rng = np.random.default_rng(77)
    out = []

    def sums_of(xc, n, r):
        J = np.concatenate([np.cross(xc, n), n], 1)
        cols = [J[:, i] * J[:, j] for i, j in PO.TRI] + [J[:, i] * r for i in range(6)] + [r * r, r * r, xc[:, 0], xc[:, 1], xc[:, 2]]
        return np.stack(cols, 1).sum(0)

    for i in range(200):
        m = int(rng.integers(6, 400))
        scale = 10.0 ** rng.uniform(-2, 2)
        xc = rng.standard_normal((m, 3)) * scale
        n = rng.standard_normal((m, 3))
        n /= np.sqrt((n * n).sum(1))[:, None]
        r = rng.standard_normal(m) * scale * (1e-7 if i % 5 == 0 else 0.05)
        out.append(("random", m, scale * 1.7, rng.standard_normal(3) * scale, sums_of(xc, n, r)))
    xc = rng.standard_normal((50, 3))
    flat = np.tile([0.0, 0.0, 1.0], (50, 1))
    out.append(("plane", 50, 1.5, np.zeros(3), sums_of(xc, flat, rng.standard_normal(50) * 0.01)))
    out.append(("zero", 10, 1.0, np.zeros(3), np.zeros(32)))
    good = out[3]
    out.append(("few", 5, good[2], good[3], good[4]))
    out.append(("rho", good[1], 0.0, good[3], good[4]))
    nan = good[4].copy()
    nan[7] = np.nan
    out.append(("nan", good[1], good[2], good[3], nan))
    line = np.outer(np.linspace(-1, 1, 40), [1.0, 2.0, 0.5])                       # collinear rows, one normal: rank 2
    out.append(("collinear", 40, 1.2, np.zeros(3), sums_of(line, np.tile([0.6, 0.0, 0.8], (40, 1)), np.linspace(-1, 1, 40) * 0.01)))
    return out


def test_plane_solve_header_under_address_and_undefined_sanitizers(tmp_path):
    """The 6 x 6 solve of csrc/cloud_align_solve.h in the same stand-alone program: z = y / D against numpy's LU solve of the scaled system within
    the backward error of a 6 x 6 LDL^T (at most 6^2 = 36 products and sums per entry, 2 u each: 128 u covers it with the right-hand side) times
    the condition number; dR a rotation to rounding, equal to Rodrigues' matrix of omega; dt and the degenerate cases."""
    import _plane_oracle as PO
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cloud_solve_main")
    src = os.path.join(HERE, "host", "cloud_solve_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "etch_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = _plane_systems()
    path = str(tmp_path / "systems.txt")
    with open(path, "w") as fh:
        for _, m, rho, c, sums in cases:
            fh.write("S %d %s\n" % (m, " ".join(repr(float(x)) for x in [rho, *c, *sums])))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(cases) + 1
    worst = 0.0
    for ln, (name, m, rho, c, sums) in zip(lines, cases):
        v = [float(x) for x in ln.split()[1:]]
        ok, y, dR, dt, angle, shift = int(v[0]), np.array(v[1:7]), np.array(v[7:16]).reshape(3, 3), np.array(v[16:19]), v[19], v[20]
        oR, odt, ook, oy, oangle, oshift, cond = PO.solve(m, sums, c, rho)
        assert ok == int(ook) == (1 if name == "random" else 0), (name, ok, ook)
        if not ok:
            assert np.array_equal(dR, np.eye(3)) and not dt.any() and not y.any() and angle == 0.0 and shift == 0.0, name
            continue
        D = np.array([1.0 / rho] * 3 + [1.0] * 3)
        z, oz = y / D, oy / D
        err = np.sqrt(((z - oz) ** 2).sum()) / np.sqrt((oz ** 2).sum())
        worst = max(worst, err / (U * cond))
        assert err <= 128 * U * cond, (name, err, cond)
        assert np.abs(dR.T @ dR - np.eye(3)).max() <= 8 * U and abs(np.linalg.det(dR) - 1.0) <= 8 * U
        assert np.abs(dR - PO.quat_rotation(y[:3])).max() <= 16 * U
        assert np.abs(dt - (c - dR @ c + y[3:])).max() <= 8 * U * (np.abs(c).max() * 2 + np.abs(y[3:]).max())
        assert angle == np.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
        assert abs(shift - np.sqrt((((dR - np.eye(3)) @ (sums[29:32] / m) + y[3:]) ** 2).sum())) <= 64 * U * (np.abs(sums[29:32] / m).max() + np.abs(y[3:]).max())
    print(f"worst |z - z_ref| / (u cond |z_ref|) = {worst:.3g} of 128")


# ---- convergence: conditions on the oracle alone ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampled():
    import _plane_oracle as PO
    p, q = PO.sampled_case()
    return p, q, NO.normals(q, 16, nbr=NO.neighbours_fast(q, 16))[0]


@pytest.mark.parametrize("degrees,shift", [(10.0, 0.05), (20.0, 0.10)])
def test_plane_metric_converges_in_a_few_steps_where_the_point_metric_needs_tens(sampled, degrees, shift):
    """Two samplings of the body's surface, 4 000 rows against 12 000, default gates, normals from k = 16: the plane metric puts every source row
    within 1 mm of the truth within 6 steps, and after 8 steps it is no further from the truth than the point metric after 40.
    Measured (profiles/cloud_normals_pins.txt): see there."""
    import _align_oracle as AO
    import _plane_oracle as PO
    p, q, nq = sampled
    moved, R0, t0 = AO.displaced(p, degrees, shift)
    plane, point = [], []
    PO.align(moved, q, nq, iters=8, metric="plane", history=plane)
    PO.align(moved, q, nq, iters=40, metric="point", history=point)
    eplane = [PO.row_error(moved, R, t, R0, t0) for R, t in plane]
    epoint = [PO.row_error(moved, R, t, R0, t0) for R, t in point]
    first = next((k + 1 for k, e in enumerate(eplane) if e < 1e-3), None)
    first_point = next((k + 1 for k, e in enumerate(epoint) if e < 1e-3), None)
    print(f"{degrees} deg / {shift} m: plane under 1 mm at step {first}, after 8 steps {eplane[-1]:.3g} m; point under 1 mm at step {first_point}, "
          f"after 8 steps {epoint[7]:.3g} m, after 40 steps {epoint[-1]:.3g} m")
    assert len(eplane) == 8 and len(epoint) == 40
    assert first is not None and first <= 6, eplane
    assert eplane[-1] <= epoint[-1], (eplane[-1], epoint[-1])
