"""Point winding numbers without a GPU: the oracle of tests/_cloud_winding_oracle.py on a sphere and on the fixture body seen
from three sides (and from one, which must fail), csrc/cloud_winding_solve.h built by the host compiler under the address and undefined-behaviour
sanitizers and driven by tests/host/cloud_winding_main.cpp, the ABI, the flags and the argument errors, and orient_normals and the view ids of
fuse on hand-made cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _cloud_winding_oracle as WO
import _containment_oracle as CT

HERE = os.path.dirname(os.path.abspath(__file__))
R = 0.5


def _f64(cloud):
    return tuple(a.astype(np.float64) for a in cloud)


def test_the_abi_declares_the_entry_points_and_the_file_is_built_without_contraction():
    from etch_amd import _lib, build as B
    names = _lib.declared_symbols()
    for n in ("etch_cloud_knn_kth", "etch_cloud_surface_pack", "etch_cloud_winding_number", "etch_cloud_winding_number_workspace",
              "etch_cloud_containment_energy_grad", "etch_cloud_containment_energy_grad_workspace", "etch_smpl_surface_refine_contain_cloud",
              "etch_smpl_surface_refine_contain_cloud_workspace"):
        assert n in names, n
    assert B.EXTRA["cloud_winding.hip"] == ["-ffp-contract=off"] and "cloud_winding.hip" in B.sources()
    from etch_amd import ops
    for n in ("cloud_knn_kth", "cloud_surface_pack", "cloud_winding_number", "cloud_containment_energy_grad", "smpl_surface_refine_contain_cloud"):
        assert callable(getattr(ops, n)), n


# ---- the sphere ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16])
def test_a_sampled_sphere_has_an_inside(k):
    """2 000 rows on a Fibonacci sphere of radius 0.5 with analytic normals, the oracle in fp64: w >= 0.85 at every query within 0.9 R (the shell
    at 0.9 R itself included), w <= 0.15 beyond 1.1 R, the areas add up to the sphere's within a tenth, reversed normals negate w."""
    p, n = WO.fibonacci_sphere(2000, R)
    a = WO.areas(p, k)
    ratio = a.sum() / (4.0 * np.pi * R * R)
    cloud = _f64(WO.pack(p, n, a))
    inside = np.concatenate([WO.sphere_queries(R, 0.0, 0.9, 400, 1), WO.sphere_queries(R, 0.9, 0.9, 400, 2)])
    outside = np.concatenate([WO.sphere_queries(R, 1.1, 3.0, 400, 3), WO.sphere_queries(R, 1.1, 1.1, 400, 4)])
    wi, wo = WO.winding(*cloud, inside)[0], WO.winding(*cloud, outside)[0]
    print(f"k={k}: worst inside error {np.abs(wi - 1).max():.3f}, worst outside error {np.abs(wo).max():.3f}, area ratio {ratio:.3f}")
    assert (wi >= 0.85).all() and (wo <= 0.15).all()
    assert 0.9 <= ratio <= 1.1
    rev = _f64(WO.pack(p, -n, a))
    assert np.array_equal(WO.winding(*rev, inside)[0], -wi) and np.array_equal(WO.winding(*rev, outside)[0], -wo)


def test_the_area_rules():
    p, _ = WO.fibonacci_sphere(50, R)
    assert (WO.areas(p[:1], 8) == 0).all()                                    # one row: no neighbour
    a = WO.areas(p[:4], 8)                                                    # ke = 3 < k
    assert np.array_equal(a, (WO.PI * WO.kth_d2(p[:4], 3)) / 3.0)
    flag = np.zeros(50, np.int32)
    flag[7] = 2
    q = p.copy()
    q[9, 1] = np.nan
    with np.errstate(all="ignore"):
        a = WO.areas(q, 8, flag)
    assert a[7] == 0 and a[9] == 0 and (a[[0, 1, 2]] > 0).all()
    d = np.concatenate([p[:5], p[:5]])                                        # every row twice: the nearest is at 0, the third is not
    assert (WO.kth_d2(d, 3) > 0).all() and (WO.areas(d, 3) > 0).all()
    assert (WO.areas(np.repeat(p[:1], 5, 0), 3) == 0).all()                   # five copies of one row: every neighbour at 0, no area


# ---- the fixture body from three sides, and from one ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body_refs():
    """600 body vertices pushed 1 cm out and 1 cm in along the mesh normal, with the mesh oracle's inside flags."""
    v, f = WO.body_mesh()
    out, ins = WO.body_queries(600, 0.01)
    return [(q, np.abs(CT.winding_number(v, f, q)) >= 0.5) for q in (out, ins)]


@pytest.mark.parametrize("k", [8, 16])
def test_three_views_of_the_body_agree_with_its_mesh(body_refs, k):
    p, n, flag, _, view = WO.body_views()
    assert len(p) == WO.BODY_ROWS and sorted(set(view.tolist())) == [0, 1, 2]
    cloud = _f64(WO.surface(p, n, k, flag))
    got = []
    for q, ref in body_refs:
        got.append(float(((np.abs(WO.winding(*cloud, q)[0]) >= 0.5) == ref).mean()))
    print(f"k={k}: the cloud's inside flag agrees with the mesh's for {got[0]:.4f} of the queries 1 cm outside and {got[1]:.4f} of those 1 cm inside")
    assert min(got) >= 0.95, got


def test_a_single_view_has_no_inside(body_refs):
    """The evidence for the command's refusal: of the queries the mesh calls inside, the view from azimuth 0 alone calls fewer than 0.6 inside."""
    p, n, flag, _, _ = WO.body_views((0.0,))
    cloud = _f64(WO.surface(p, n, 8, flag))
    for q, ref in body_refs:
        if not ref.any():
            continue
        share = float((np.abs(WO.winding(*cloud, q)[0]) >= 0.5)[ref].mean())
        print(f"a single view: {share:.3f} of the mesh's inside queries are inside")
        assert share < 0.6


# ---- the header -----------------------------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _bits32(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


def test_the_header_agrees_with_the_oracle_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/cloud_winding_solve.h compiled alone by the host compiler with -fsanitize=address,undefined into a program of its own (no sanitizer is
    ever loaded into python): the area, the packed row, d2 and the pair term and the key equal the oracle's by bits."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cloud_winding_main")
    src = os.path.join(HERE, "host", "cloud_winding_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "etch_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(11)
    num = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1))      # noqa: E731
    lines, want = [], []
    for i in range(60):                                                              # A: areas
        d2k, ke, flag = float(rng.uniform(0, 1e-3)), int(rng.integers(0, 33)), int(i % 7 == 0)
        p = rng.standard_normal(3)
        if i % 11 == 0:
            p[i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
        lines.append(f"A {d2k!r} {ke} {flag} {num(p)}")
        ok = ke > 0 and not flag and np.isfinite(p).all()
        want.append(("A", [(WO.PI * d2k) / ke if ok else 0.0]))
    for i in range(60):                                                              # P: packed rows
        p, c, n = rng.standard_normal(3) * 3, rng.standard_normal(3), rng.standard_normal(3)
        n /= np.sqrt((n * n).sum())
        a = np.array([float(rng.uniform(0, 1e-3)) if i % 5 else 0.0])
        pos, mom, cap = WO.pack(p[None], n[None], a, c)
        lines.append(f"P {num(p)} {num(c)} {num(n)} {num(a)}")
        want.append(("P", [_bits32(x) for x in (*pos[0], *mom[0], cap[0])]))
    special = [np.float32(x) for x in (0.0, 1e-30, 1e-42, 3e38, np.inf, np.nan)]
    for i in range(120):                                                             # T: pair terms
        q, p, m = (rng.standard_normal(3).astype(np.float32) for _ in range(3))
        cap = np.float32(rng.uniform(0, 0.1)) if i % 4 else np.float32(0)
        if i % 9 == 0:
            p = q.copy()                                                             # the query on the row: d2 = 0, the cap decides
        if i % 13 == 0:
            p[i % 3] = special[i % len(special)]
        if i % 17 == 0:
            cap = special[(i // 17) % len(special)]
        term, d2 = WO.pair_terms(q[None], p[None], m[None], np.array([cap], np.float32))
        lines.append(f"T {num(q)} {num(p)} {num(m)} {num(cap)}")
        want.append(("T", [_bits32(d2[0, 0]), _bits32(term[0, 0])]))
    keys = []
    for d2 in (0.0, 1e-42, 1e-30, 0.5, 1.0, 3e38, np.inf, np.nan, -1.0):              # K: keys
        for row in (0, 1, 1023, 2 ** 31 - 1, -1):
            f = np.float32(d2)
            has = bool(f >= 0) and row >= 0
            key = (_bits32(f) << 32 | row) if has else 2 ** 64 - 1
            keys.append(key)
            lines.append(f"K {float(f)!r} {row}")
            want.append(("K", [key, row if has else -1, _bits32(f) if has else 0]))
    for a in keys[::3]:                                                              # M: merges
        for b in keys[1::7]:
            lines.append(f"M {a} {b}")
            want.append(("M", [min(a, b)]))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out[-1] == "done" and len(out) == len(want) + 1
    nan32 = lambda b: (b & 0x7f800000) == 0x7f800000 and (b & 0x007fffff) != 0       # noqa: E731
    for i, (ln, (kind, vals)) in enumerate(zip(out, want)):
        tok = ln.split()
        assert tok[0] == kind, (i, ln)
        if kind == "A":
            assert float(tok[1]) == vals[0], (i, lines[i], ln)
        elif kind == "T":
            got = [int(t) for t in tok[1:]]
            for g, w in zip(got, vals):                                              # a NaN is a NaN, whatever its payload
                assert g == w or (nan32(g) and nan32(w)), (i, lines[i], ln, vals)
        else:
            assert [int(t) for t in tok[1:]] == vals, (i, lines[i], ln, vals)


# ---- flags, argument errors, hand-made cases -------------------------------------------------------------------------------------------------------
def test_the_command_has_the_flags_and_refuses_what_has_no_inside(tmp_path, capsys):
    from etch_amd import cloud
    base = ["--cloud_path", "x.ply"]
    a = cloud.parse_args(base)
    assert not hasattr(a, "surface_refine") and not hasattr(a, "surface_contain") and a.contain_normal_k == 16 and a.contain_area_k == 8
    a = cloud.parse_args(base + ["--more_views", "y.ply", "--align_global", "--surface_refine", "--surface_contain", "--contain_area_k", "12"])
    assert a.surface_refine and a.surface_contain and a.contain_area_k == 12
    for bad in (["--surface_contain"], ["--contain_w", "3"], ["--surface_iters", "5"], ["--surface_refine", "--chamfer_refine"],
                ["--surface_refine", "--surface_contain", "--contain_area_k", "2"], ["--surface_refine", "--surface_contain", "--contain_normal_k", "33"],
                ["--surface_refine", "--surface_contain", "--contain_every", "0"]):
        with pytest.raises(SystemExit):
            cloud.parse_args(base + bad)
    capsys.readouterr()
    # one view, a file without normals: refused before anything is loaded
    path = str(tmp_path / "one.npy")
    np.save(path, np.random.default_rng(0).standard_normal((30, 3)))
    with pytest.raises(SystemExit):
        cloud.main(["--cloud_path", path, "--surface_refine", "--surface_contain"])
    assert "half a shell" in capsys.readouterr().err


def test_surface_and_areas_check_their_arguments_before_any_launch():
    from etch_amd import cloud
    c = cloud.pack([np.random.default_rng(1).standard_normal((20, 3))], device="cpu")
    nrm = np.tile([0.0, 0.0, 1.0], (20, 1))
    for kw in (dict(), dict(sensors=(0, 0, 1), normals=nrm), dict(sensors=(0, 0, 1), area_k=2), dict(sensors=(0, 0, 1), area_k=33),
               dict(sensors=(0, 0, 1), normal_k=2), dict(sensors=(0, 0), ), dict(sensors=np.zeros((3, 3))), dict(sensors=(0, np.nan, 1)),
               dict(normals=nrm[:5]), dict(normals=nrm, center=(0, 1)), dict(normals=nrm, center=(0, np.inf, 1)), dict(normals=nrm, area_k=8.5)):
        with pytest.raises(ValueError):
            cloud.surface(c, **kw)
    for kw in (dict(k=2), dict(k=33), dict(k=8, cell=0.0), dict(k=8, cell=float("nan"))):
        with pytest.raises(ValueError):
            cloud.areas(c, **kw)


def test_orient_normals_on_a_hand_made_case():
    from etch_amd import cloud
    pts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [5, 5, 5]])
    c = cloud.pack([pts[:3], pts[3:]], device="cpu")
    n = np.array([[0.0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, 0, 0]])
    one = cloud.orient_normals(c, n, (0.0, 0.0, 10.0)).numpy()                        # one sensor above everything
    assert np.array_equal(one, [[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 0]])      # dot 0 is not flipped; the zero normal stays
    per_cloud = cloud.orient_normals(c, n, [[0.0, 0, -10], [0, -10, 3]]).numpy()
    assert np.array_equal(per_cloud, [[0, 0, -1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0, 0, 0]])
    rows = np.array([[0.0, 0, 10], [1, 0, 10], [-4, 2, 0], [0, 9, 3], [0, 0, 0]])
    per_row = cloud.orient_normals(c, torch.from_numpy(n), rows).numpy()
    assert np.array_equal(per_row, [[0, 0, 1], [0, 0, 1], [-1, 0, 0], [0, 1, 0], [0, 0, 0]])
    assert np.array_equal(per_row, WO.orient(pts, n, rows))
    for bad in ((0, 0), np.zeros((3, 3)), np.zeros((4, 3))):
        with pytest.raises(ValueError):
            cloud.orient_normals(c, n, bad)
    with pytest.raises(ValueError):
        cloud.orient_normals(c, n[:4], (0, 0, 1))


def test_the_view_ids_of_a_fused_cloud_on_a_hand_made_case():
    """fuse(return_view=True) is two index computations around the kernels (the whole call runs in tests/test_gpu_cloud_winding.py): the view of
    every row of the union -- per subject, view after view --, and under a voxel grid the view of each cell's lowest row."""
    from etch_amd import cloud
    offsets = [np.array([0, 2, 3]), np.array([0, 1, 4]), np.array([0, 0, 2])]         # three views of two subjects: 2 + 1 + 0 and 1 + 3 + 2 rows
    ids = cloud._view_ids(torch, offsets, "cpu")
    assert ids.dtype == torch.int32 and ids.tolist() == [0, 0, 1, 0, 1, 1, 1, 2, 2]
    union_offsets = torch.tensor([0, 3, 9], dtype=torch.int32)
    index = torch.tensor([2, 0, 5, 1, 4], dtype=torch.int32)                          # lowest rows, local: subject 0 has two cells, subject 1 three
    out_offsets = torch.tensor([0, 2, 5], dtype=torch.int32)
    assert cloud._lowest_view(torch, ids, union_offsets, index, out_offsets).tolist() == [1, 0, 2, 1, 2]
