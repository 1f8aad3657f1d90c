"""Isolating the subject of a raw cloud, the part that needs no GPU: the numpy oracle against a second implementation, the
Philox rows, the argument checks (which come before any library call), the flags of both commands, and the end-to-end fixture judged by the
oracle alone -- so that the GPU test is never the first thing to meet an ill-chosen fixture."""
import collections

import numpy as np
import pytest

import _cloud_oracle as CO
import _isolate_oracle as IO
from _sampler_oracle import philox4x32_10


def _bfs_components(p, r):
    """Labels and sizes by breadth-first search over the dense adjacency matrix: shares nothing with the oracle's union-find."""
    n = len(p)
    adj = CO.d2_rows(p, np.arange(n)) <= float(r) * float(r)
    label = np.full(n, -1, np.int32)
    for s in range(n):                                               # ascending: the first unvisited row of a component is its lowest
        if label[s] >= 0:
            continue
        queue = collections.deque([s])
        label[s] = s
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(adj[i] & (label < 0)):
                label[j] = s
                queue.append(j)
    return label, np.bincount(label, minlength=n)[label].astype(np.int32)


def test_oracle_components_equal_a_breadth_first_search():
    rng = np.random.default_rng(3)
    g = np.arange(-2, 3) * 0.25
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    chain = np.arange(300)[::-1, None] * np.array([0.09, 0.0, 0.0])
    for p, r in ((rng.uniform(0, 1, (400, 3)), 0.08), (rng.uniform(0, 1, (400, 3)), 0.2), (lattice, 0.25), (lattice, 0.2499), (chain, 0.1),
                 (np.zeros((1, 3)), 1.0), (np.repeat(rng.standard_normal((1, 3)), 7, 0), 0.5)):
        label, size = IO.components(p, r)
        want_label, want_size = _bfs_components(p, r)
        assert np.array_equal(label, want_label) and np.array_equal(size, want_size)
        assert (label <= np.arange(len(p))).all() and (label[label] == label).all()
    assert len(set(IO.components(lattice, 0.25)[0])) == 1 and len(set(IO.components(lattice, 0.2499)[0])) == 125
    assert IO.components(np.zeros((0, 3)), 1.0)[0].shape == (0,)


@pytest.mark.parametrize("n", [1, 3, 2 ** 31 - 1])
def test_hypothesis_rows_come_from_the_shared_philox_and_stay_inside_the_cloud(n):
    key, H = 0xFEDCBA9876543210, 4096
    rows = IO.hypothesis_rows(key, H, n)
    assert rows.shape == (H, 3) and rows.min() >= 0 and rows.max() < n
    ctr = np.zeros((H, 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = np.arange(H), 1
    r = philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))
    want = np.array([[(int(x) * n) >> 32 for x in row[:3]] for row in r[:64]])                     # Python integers: no width to overflow
    assert np.array_equal(rows[:64], want)
    pick = np.zeros((H, 4), np.uint32)
    pick[:, 0] = np.arange(H)
    assert not np.array_equal(philox4x32_10(pick, (key & 0xFFFFFFFF, key >> 32)), r)               # the pick's stream (j, 0, 0, 0) is another one
    if n == 2 ** 31 - 1:
        assert rows.max() > 2 ** 30                                                                # the product needs its 63 bits


def test_oracle_plane_conventions():
    rng = np.random.default_rng(4)
    p = np.concatenate([np.stack([rng.uniform(-1, 1, 300), rng.uniform(-1e-3, 1e-3, 300), rng.uniform(-1, 1, 300)], 1),
                        rng.uniform(-1, 1, (60, 3)) * [0.2, 0.5, 0.2] - [0.0, 0.6, 0.0]])            # a floor, and a blob UNDER it
    plane, counts, found = IO.ransac(p, 9, 64, 0.01)
    assert found and plane[1] < -0.99 and counts[1] >= counts[2]                                   # without up: towards the bulk, which is below
    plane_up, counts_up, _ = IO.ransac(p, 9, 64, 0.01, up=(0.0, 1.0, 0.0), cos_tilt=np.cos(np.radians(10.0)))
    assert plane_up[1] > 0.99 and counts_up[0] == counts[0] and counts_up[1] == counts[2]
    assert abs(np.sqrt((plane[:3] ** 2).sum()) - 1.0) < 1e-15
    planes, valid = IO.hypotheses(p, 9, 64, up=(0.0, 1.0, 0.0), cos_tilt=1.0)                      # max_tilt 0: next to nothing is that level
    assert valid.sum() <= 1 and (planes[valid == 0] == 0.0).all()
    line = np.arange(50)[:, None] * np.array([[0.5, 1.0, -0.25]])
    assert IO.hypotheses(line, 1, 256)[1].sum() == 0 and not IO.ransac(line, 1, 256, 0.01)[2]
    assert not IO.ransac(p[:2], 1, 16, 0.01)[2] and not IO.ransac(p, 9, 64, 0.01, min_inliers=10 ** 6)[2]


def _no_library(monkeypatch):
    from etch_amd import _lib
    entered = []

    def call(name, *args):
        entered.append(name)
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    return entered


def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    from etch_amd import cloud as C
    rng = np.random.default_rng(5)
    packed = C.pack([rng.standard_normal((40, 3)), rng.standard_normal((9, 3))], device="cpu")
    entered = _no_library(monkeypatch)
    nan, inf = float("nan"), float("inf")
    bad_plane = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf), dict(hypotheses=0), dict(hypotheses=65537),
                 dict(hypotheses=2.5), dict(up=(0.0, 0.0, 0.0)), dict(up=(0.0, nan, 1.0)), dict(up=(inf, 0.0, 0.0)), dict(up=(0.0, 1.0)),
                 dict(up=(0.0, 1.0, 0.0), max_tilt=-1.0), dict(up=(0.0, 1.0, 0.0), max_tilt=90.5), dict(up=(0.0, 1.0, 0.0), max_tilt=nan),
                 dict(max_tilt=10.0), dict(min_inliers=-1), dict(keys=[1, 2, 3])]
    for kw in bad_plane:
        args = {"threshold": 0.02, "keys": [1, 2], **kw}
        for call in (lambda: C.fit_plane(packed, **args), lambda: C.remove_plane(packed, **args), lambda: C.prepare(packed, 16, [1, 2], floor=args)):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: C.cluster(packed, 0.0), lambda: C.cluster(packed, -0.1), lambda: C.cluster(packed, nan), lambda: C.keep_clusters(packed, 0.0),
                 lambda: C.keep_clusters(packed, 0.1, min_points=0), lambda: C.keep_clusters(packed, 0.1, min_points=1.5),
                 lambda: C.prepare(packed, 16, [1, 2], cluster=(0.0, 1)), lambda: C.prepare(packed, 16, [1, 2], cluster=(0.1, 0)),
                 lambda: C.prepare(packed, 16, [1, 2], cluster=(inf, 1))):
        with pytest.raises(ValueError):
            call()
    assert entered == []


def test_isolate_flags_parse_on_both_commands():
    from etch_amd import cloud as C
    from etch_amd import depth as D
    on = ["--floor_threshold", "0.02", "--floor_hypotheses", "256", "--floor_up", "0", "1", "0", "--floor_max_tilt", "10", "--floor_min_inliers", "50",
          "--cluster_radius", "0.05", "--cluster_min_points", "100"]
    for parse, base in ((C.parse_args, ["--cloud_path", "scan.ply"]), (D.parse_args, ["--scan_path", "scan.obj", "--view_azimuth", "30"])):
        off = parse(base)
        assert C.isolate_args(off) == (None, None) and off.floor_threshold == 0.0 and off.cluster_radius == 0.0
        a = parse(base + on)
        floor, cluster = C.isolate_args(a)
        assert floor == dict(threshold=0.02, hypotheses=256, up=[0.0, 1.0, 0.0], max_tilt=10.0, min_inliers=50) and cluster == (0.05, 100)
        assert C.isolate_args(parse(base + ["--cluster_radius", "0.05"])) == (None, (0.05, 1))
        for bad in (["--floor_threshold", "-1"], ["--floor_threshold", "0.02", "--floor_hypotheses", "0"], ["--floor_up", "0", "0", "0"],
                    ["--floor_max_tilt", "10"], ["--floor_up", "0", "1", "0", "--floor_max_tilt", "91"], ["--cluster_radius", "-1"],
                    ["--cluster_radius", "0.05", "--cluster_min_points", "0"], ["--floor_min_inliers", "-2"]):
            with pytest.raises(SystemExit):
                parse(base + bad)


@pytest.fixture(scope="module")
def fixture():
    p, kind = IO.isolate_fixture()
    k1, s1, plane, found = IO.isolate_pipeline(p, 5)
    return p, kind, k1, s1, plane, found


def test_the_end_to_end_fixture_meets_its_conditions_under_the_oracle(fixture):
    """The guard of tests/test_gpu_cloud_isolate.py's end-to-end test: statistical filter (8, 1.0), floor with tau = 2 cm, up = +y, 10 degrees and
    256 hypotheses under key 5, clusters at 5 cm.  With the plane refitted by numpy.linalg.eigh (the device's differs from it by ~1e-16) the
    result holds no floor, clutter or stray row and every body row more than tau above the plane; no row is nearer than 1e-7 m to the
    threshold, so no rounding of the refit flips one; the bounding-box centre moves by less than 1 cm (9.6 mm: the cut of the soles)."""
    p, kind, k1, s1, plane, found = fixture
    assert p.shape == (11430, 3) and np.bincount(kind).tolist() == [6890, 4000, 400, 140]
    assert found and plane[1] > 0.9999 and abs(plane[3]) < 0.003 and (k1 | (kind != 0)).all()       # the filter takes no body row
    refit, w, m = IO.refit_eigh(s1, plane, 0.02)
    assert m > 3000 and w[0] < 1e-3 * w[1]                                                           # a wide gap: the refit is well conditioned
    for pl in (plane, refit):
        keep, rows = IO.after_plane(p, k1, s1, pl, True)
        s = IO.signed(p, pl)
        assert not keep[kind != 0].any() and np.array_equal(keep[kind == 0], s[kind == 0] > 0.02)
        assert rows[0] > rows[1] > rows[2] == keep.sum() > 6600
        assert np.abs(np.abs(IO.signed(s1, pl)) - 0.02).min() > 1e-7
    v = CO.body_vertices()
    bare = (v.min(0) + v.max(0)) / 2.0 + [0.0, IO.LIFT - v[:, 1].min(), 0.0]
    q = p[keep]
    assert np.linalg.norm((q.min(0) + q.max(0)) / 2.0 - bare) < 0.01
    assert (kind != 0).mean() > 0.35                                                                 # without the stages, 4 of 10 picked points are no body
