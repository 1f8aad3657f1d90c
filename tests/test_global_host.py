"""Global registration without a GPU: the oracle of tests/_global_oracle.py against itself, csrc/cloud_global_solve.h built by
the host compiler under the address and undefined-behaviour sanitizers and driven by tests/host/cloud_global_main.cpp, the conditions the
end-to-end fixtures must meet before any ICP, and seeded defects that the comparisons of tests/test_gpu_cloud_global.py must catch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _align_oracle as AO
import _cloud_oracle as CO
import _global_oracle as GO
import _normals_oracle as NO

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def patch():
    """Every fourth row of the 60 degree view with its descriptors at k = 16."""
    p, cam = GO.view(60.0)
    p = np.ascontiguousarray(p[::4])
    return p, cam, GO.features(p, 16, cam)


def test_the_abi_declares_the_entry_points_and_the_file_is_built_without_contraction():
    from etch_amd import _lib
    from etch_amd import build as B
    names = _lib.declared_symbols()
    for n in ("etch_cloud_fpfh", "etch_cloud_feature_match", "etch_cloud_global_hypotheses", "etch_cloud_global_score", "etch_cloud_global_select",
              "etch_cloud_global_inliers"):
        assert n in names, n
    assert B.EXTRA["cloud_global.hip"] == ["-ffp-contract=off"] and "cloud_global.hip" in B.sources()
    head = open(_lib.HEADER).read()
    assert "#define ETCH_GLOBAL_BINS 11 " in head and "#define ETCH_GLOBAL_FEATURES 33 " in head and "#define ETCH_GLOBAL_MAX_H 262144 " in head


def test_descriptors_do_not_change_under_a_rigid_motion_of_cloud_and_viewpoint(patch):
    """Every feature is an angle between directions that turn together.  The lists must stay as they are, the counts may move only as the edge
    rule allows (a rigid motion changes a feature by a few u, far inside the rule's 1e-9) -- except in rows with a pair whose source is tied, where
    the motion decides the sign of phi --, and F agrees to rounding wherever the counts it is built from stayed: 33 k terms of relative error
    ~16 u each, 1e-12 with room."""
    p, cam, (F, has, s, c, lists, nrm, flag) = patch
    R, t = AO.rotation([0.4, -0.3, 0.8], 107.0), np.array([0.7, -1.1, 0.4])
    q, cam2 = AO.apply(R, t, p), AO.apply(R, t, cam[None])[0]
    F2, has2, s2, c2, lists2, nrm2, flag2 = GO.features(q, 16, cam2)
    assert np.array_equal(lists, lists2) and np.array_equal(flag, flag2) and np.abs(nrm2 - nrm @ R.T).max() < 1e-9
    _, _, b, edge, counted = GO.spfh(p, nrm, flag, lists)
    firm = ~GO.source_ties(p, nrm, flag, lists).any(1)                                     # a tied source negates phi on the last bit: not steady
    why, share = GO.edge_rule(s2[firm], c2[firm], s[firm], c[firm], b[firm], edge[firm], counted[firm])
    assert why is None, why
    same = (s == s2).all(1)
    steady = same & np.where(lists >= 0, same[np.where(lists >= 0, lists, 0)], True).all(1)
    print(f"rows with an edge pair {share:.4f}, rows without a tied source {firm.mean():.4f}, rows whose counts stayed {steady.mean():.4f}, "
          f"worst |F - F'| there {np.abs(F - F2)[steady].max():.3e}")
    # two rows that share a neighbourhood (each other included) share a normal to rounding: 3 % of the pairs here, a quarter of the rows
    assert firm.mean() > 0.5 and steady.mean() > 0.25 and np.array_equal(has[steady], has2[steady]) and has.mean() > 0.9
    assert np.abs(F - F2)[steady].max() <= 1e-12 * 100.0
    assert np.allclose(F[has].reshape(-1, 3, 11).sum(2), 100.0, rtol=0, atol=1e-10)


def test_the_oracles_own_share_of_rows_with_an_edge_pair_is_below_one_percent():
    for name, (p, cam), k in (("body", (CO.body_vertices(), None), 16), ("view 0", GO.view(0.0), 32), ("view 60", GO.view(60.0), 32)):
        cam = p.mean(0) + [0.0, 0.0, 3.0] if cam is None else cam
        nbr = NO.neighbours_fast(p, k) if _has_scipy() else NO.neighbours(p, k)
        nrm, _, flag, _, _ = NO.normals(p, k, cam, nbr=nbr)
        _, _, _, edge, counted = GO.spfh(p, nrm, flag, GO.pad(nbr, k))
        share = float((edge & counted[..., None]).any((1, 2)).mean())
        print(f"{name}: {len(p)} rows, {int(counted.sum())} pairs, share of rows with an edge pair {share:.5f}")
        assert share <= 0.01, name


def _has_scipy():
    try:
        import scipy.spatial  # noqa: F401
        return True
    except ImportError:
        return False


# ---- csrc/cloud_global_solve.h under the sanitizers --------------------------------------------------------------------------------------------------
def _host_compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _pair_cases(patch):
    p, _, (_, _, _, _, lists, nrm, flag) = patch
    rng = np.random.default_rng(43)
    rows = rng.choice(np.flatnonzero(flag == 0), 300, replace=False)
    out = [(p[i], nrm[i], p[j], nrm[j]) for i in rows for j in lists[i, :3] if flag[j] == 0]
    e = np.array([0.0, 0.0, 1.0])
    out.append((p[0], e, p[0] + 0.1 * e, e))                               # d parallel to u: d x u = 0, not counted
    out.append((p[0], nrm[0], p[0], nrm[0]))                               # d2 = 0: not counted
    out.append((np.zeros(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])))      # alpha = 0, phi = 0, theta = 0 exactly
    out.append((np.zeros(3), np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0])))     # theta = +-pi: the last or the first bin
    return out


def _triple_cases():
    rng = np.random.default_rng(47)
    out = []
    for i in range(200):
        a = rng.standard_normal((3, 3)) * 0.3 + rng.standard_normal(3)
        R, t = AO.rotation(rng.standard_normal(3), rng.uniform(0, 180)), rng.standard_normal(3)
        b = AO.apply(R, t, a) * (1.0 + (0.08 * rng.standard_normal() if i % 2 else 0.0)) + rng.standard_normal((3, 3)) * (0.01 if i % 3 == 0 else 0.0)
        out.append((a, b, 0.9, 0.05 if i % 5 else 0.4))
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])
    out.append((line, line + 1.0, 0.9, 0.05))                              # collinear: the edges pass, the solve is degenerate
    out.append((line[[0, 0, 1]], line[[0, 0, 1]], 0.9, 0.0))               # a zero edge with min_edge = 0: 0 >= 0 passes, the solve does not
    return out


def test_the_header_agrees_with_the_oracle_under_address_and_undefined_sanitizers(patch, tmp_path):
    """csrc/cloud_global_solve.h compiled alone by the host compiler with -fsanitize=address,undefined into a program of its own (no sanitizer is
    ever loaded into python).  Counted flags, alpha, phi, their bins, the triple's validity, its centre and its 16 sums and the Philox draws
    equal the oracle's by bits or integers; theta agrees within 4 u pi (two math libraries' atan2) and its bin wherever the oracle sees no edge;
    the triple's rotation lies within the bound of section 23 of the oracle's SVD Kabsch."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cloud_global_main")
    src = os.path.join(HERE, "host", "cloud_global_main.cpp")
    inc = os.path.join(os.path.dirname(HERE), "etch_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, src, "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    pairs, triples = _pair_cases(patch), _triple_cases()
    draws = [(key, h, n) for key in (0, 7, 2 ** 32 + 5, 2 ** 64 - 1) for h in (0, 1, 63, 4095, 262143) for n in (0, 1, 3, 257, 3499)]
    path = str(tmp_path / "cases.txt")
    num = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1))      # noqa: E731
    with open(path, "w") as fh:
        for c in pairs:
            fh.write("P " + " ".join(num(x) for x in c) + "\n")
        for a, b, e, m in triples:
            fh.write(f"T {num(a)} {num(b)} {e!r} {m!r}\n")
        for key, h, n in draws:
            fh.write(f"H {key} {h} {n}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "done" and len(lines) == len(pairs) + len(triples) + len(draws) + 1
    got = [[float(x) for x in ln.split()[1:]] for ln in lines[:-1]]
    counted = 0
    for i, (pi, ni, pj, nj) in enumerate(pairs):
        ok, f, b, edge = GO.pair_features(np.stack([pi, pj]), np.stack([ni, nj]), np.zeros(2, np.int32), np.array([[1], [-1]]))
        g = got[i]
        assert bool(g[0]) == bool(ok[0, 0]), i
        counted += int(ok[0, 0])
        assert g[2] == f[0, 0, 1] and g[3] == f[0, 0, 2] and [int(g[5]), int(g[6])] == b[0, 0, 1:].tolist() or not ok[0, 0], (i, g, f[0, 0], b[0, 0])
        assert abs(g[1] - f[0, 0, 0]) <= 4 * U * np.pi, (i, g[1], f[0, 0, 0])
        assert int(g[4]) == b[0, 0, 0] or edge[0, 0, 0] or not ok[0, 0], (i, g, b[0, 0])
    assert counted == len(pairs) - 2 and got[len(pairs) - 2][1:4] == [0.0, 0.0, 0.0] and [int(x) for x in got[len(pairs) - 2][4:7]] == [5, 5, 5]
    assert int(got[len(pairs) - 1][4]) in (0, 10)
    seen = {(0, 0): 0, (1, 0): 0, (1, 1): 0}
    for i, (a, b, e, m) in enumerate(triples):
        g = got[len(pairs) + i]
        idx = np.array([[0, 1, 2]])
        valid = bool(GO.triple_valid(a, b, np.arange(3), idx, e, m)[0])
        assert bool(g[0]) == valid, i
        w = AO.step(a, b, np.arange(3), np.eye(3), np.zeros(3), exact=False)
        terms, c = AO.moment_terms(a, b, np.arange(3), np.eye(3), np.zeros(3))
        sums = np.zeros(16)
        for row in terms:
            sums = sums + row
        assert np.array_equal(np.array(g[14:17]), c) and np.array_equal(np.array(g[17:33]), sums), i
        assert bool(g[1]) == w["ok"], (i, g[1], w["S"])
        seen[(int(valid), int(w["ok"]))] = seen.get((int(valid), int(w["ok"])), 0) + 1
        R, t = np.array(g[2:11]).reshape(3, 3), np.array(g[11:14])
        if not w["ok"]:
            assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3)), i
            continue
        bound = _step_bound(w)
        ang = np.radians(AO.angle_between(R, w["dR"]))
        reach = float(np.abs(np.concatenate([a, b])).max())
        assert ang <= bound, (i, ang, bound)
        assert abs(np.linalg.det(R) - 1.0) <= 16 * U and np.abs(AO.apply(R, t, a) - AO.apply(w["dR"], w["dt"], a)).max() <= 4.0 * bound * reach + 64 * U * reach, i
    assert seen[(1, 1)] >= 20 and seen[(0, 1)] >= 20 and seen[(1, 0)] >= 2, seen
    for i, (key, h, n) in enumerate(draws):
        want = GO.hypothesis_rows(key, h + 1, n)[h]
        assert [int(x) for x in got[len(pairs) + len(triples) + i]] == want.tolist(), (key, h, n)


def _step_bound(w):
    """The rotation bound of test_gpu_cloud_align.test_one_step_from_given_pairs_within_the_derived_bounds, from an AO.step result."""
    mm, A, S = w["m"], w["abs_sums"], w["sums"]
    dC = np.array([[mm * U * (A[6 + 3 * a + e] + (A[a] * abs(S[3 + e]) + abs(S[a]) * A[3 + e]) / mm) + 4 * U * (abs(S[6 + 3 * a + e]) + abs(S[a] * S[3 + e]) / mm)
                    for e in range(3)] for a in range(3)])
    gap = w["S"][1] + w["sign"] * w["S"][2]
    return 2.0 * float(np.sqrt((dC * dC).sum())) / gap + 16 * U * w["S"][0] / gap


# ---- the fixture conditions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["60", "90"])
def test_the_oracle_alone_lands_inside_half_the_basin_on_the_fixture(name):
    """The end-to-end fixtures of the GPU test are only fair if the definitions themselves, run by the oracle, end within 10 degrees and 5 cm
    (worst row) of the truth before any ICP: half of the basin section 23 measured, the other half being ICP's margin."""
    src, vs, tgt, vt, R0, t0, k = GO.fixture(name)
    r = GO.global_align(src, vs, tgt, vt, GO.FIXTURE_KEY, k=k, H=GO.FIXTURE_H, tau=GO.FIXTURE_TAU)
    ang, worst = GO.pose_error(r["R"], r["t"], R0, t0, src)
    print(f"PIN oracle fixture {name}: {len(src)} / {len(tgt)} rows, {r['correspondences']} correspondences, {int(r['valid'].sum())} valid hypotheses, "
          f"{r['inliers']} inliers, {ang:.3f} deg and {worst * 100:.2f} cm (worst row) from the truth")
    assert r["found"] and ang <= 10.0 and worst <= 0.05
    assert AO.angle_between(np.eye(3), R0) > 90.0                                          # the start is far outside the basin


# ---- seeded defects -----------------------------------------------------------------------------------------------------------------------------------
def test_seeded_defects_fail_the_comparisons_the_gpu_tests_use(patch):
    p, cam, (F, has, s, c, lists, nrm, flag) = patch
    _, _, b, edge, counted = GO.spfh(p, nrm, flag, lists)
    assert GO.edge_rule(s, c, s, c, b, edge, counted)[0] is None
    shifted, c2, _, _, _ = GO.spfh(p, nrm, flag, lists, shift=1)                           # a bin shifted by one
    assert np.array_equal(c, c2) and GO.edge_rule(shifted, c2, s, c, b, edge, counted)[0] is not None
    ft, ht = np.concatenate([F[:50], F[10:12]]), np.concatenate([has[:50], has[10:12]])   # rows 50, 51 coincide with rows 10, 11
    assert has[10] and has[11]
    low, dl = GO.match(F[:50], has[:50], ft, ht)
    high, dh = GO.match(F[:50], has[:50], ft, ht, highest=True)                            # a tie broken to the higher row
    assert low[10] == 10 and high[10] == 50 and np.array_equal(dl, dh) and not np.array_equal(low, high)
    a = GO.hypothesis_rows(7, 64, 500)
    assert not np.array_equal(a, GO.hypothesis_rows(7, 64, 500, word=1))                   # the stream of the plane fit instead of its own
    assert (a >= 0).all() and (a < 500).all() and np.array_equal(a, GO.hypothesis_rows(7, 4096, 500)[:64])


def test_the_recorded_three_view_figures_are_what_the_oracle_reaches():
    """VIEWS_UNION_CELLS and VIEWS_FUSED_CELLS[7] of the oracle file, recomputed: the bound of the GPU's three-view test stands on them."""
    parts = [GO.view(az) for az in (0.0, 60.0, -60.0)]
    moved = [GO.moved(p, cam, turn, cam) for (p, cam), turn in zip(parts, (0.0, 150.0, -120.0))]
    views = [m[0] for m in moved]
    R00, t00 = moved[0][2], moved[0][3]
    truth = [(R00.T @ m[2], R00.T @ (m[3] - t00)) for m in moved]
    want = AO.occupied(np.concatenate([AO.apply(R, t, v) for (R, t), v in zip(truth, views)]), 0.005)
    poses, starts = GO.register_views(views, [np.zeros(3)] * 3, GO.FIXTURE_KEY, **AO.VIEW_SETTINGS)
    got = AO.occupied(np.concatenate([AO.apply(R, t, v) for (R, t), v in zip(poses, views)]), 0.005)
    for k in (1, 2):
        e0, e1 = GO.pose_error(*starts[k], *truth[k], views[k]), GO.pose_error(*poses[k], *truth[k], views[k])
        print(f"PIN oracle view {k}: global {e0[0]:.3f} deg / {e0[1] * 100:.2f} cm, refined {e1[0]:.4f} deg / {e1[1] * 1e3:.3f} mm")
        assert e0[0] <= 10.0 and e0[1] <= 0.05
    print(f"PIN oracle occupied 5 mm cells: undisplaced union {want}, registered and fused {got} ({abs(got - want) / want:.4f})")
    assert want == GO.VIEWS_UNION_CELLS and got == GO.VIEWS_FUSED_CELLS[GO.FIXTURE_KEY] and 0.3 < GO.VIEWS_BOUND < 0.33
