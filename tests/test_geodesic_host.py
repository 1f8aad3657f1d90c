"""CPU checks of the geodesic restatement (tests/_geodesic_oracle.py) and of the host half of etch_amd.geodesic: subdivision known answers, one
flip against the law of cosines, the heat method against analytic distances, and the committed fixture reproduced from its body."""
import os

import numpy as np

import _geodesic_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")


def test_subdivision_two_triangles():
    from etch_amd import geodesic as G

    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    sv, sf = O.subdivide(v, f)
    gv, gf = G.subdivide(v, f)
    assert np.array_equal(sv, gv) and np.array_equal(sf, gf)
    assert np.array_equal(sv[:4], v)
    # unique edges (a < b) in order of (b, a): (0,1) (0,2) (1,2) (0,3) (2,3) -> midpoints 4..8
    assert np.array_equal(sv[4:], [[0.5, 0, 0], [0.5, 0.5, 0], [1, 0.5, 0], [0, 0.5, 0], [0.5, 1, 0]])
    assert np.array_equal(sf[:4], [[0, 4, 5], [4, 1, 6], [5, 6, 2], [4, 6, 5]])
    assert np.array_equal(sf[4:], [[0, 5, 7], [5, 2, 8], [7, 8, 3], [5, 8, 7]])
    n = np.cross(sv[sf[:, 1]] - sv[sf[:, 0]], sv[sf[:, 2]] - sv[sf[:, 0]])
    assert np.all(n[:, 2] > 0)                                    # winding kept
    m = O.EdgeMesh(sv, sf)
    assert len(sv) - m.E + len(sf) == 1                           # a disc
    s2, f2 = O.icosphere(2)
    assert len(s2) - O.EdgeMesh(s2, f2).E + len(f2) == 2


def test_one_flip_law_of_cosines():
    # quad a-b-d-c around the diagonal bc: a and d close to bc, so bc is not Delaunay
    a, b, c, d = np.array([0.5, 0.2, 0]), np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.5, -0.15, 0])
    v = np.stack([a, b, c, d])
    f = np.array([[0, 1, 2], [3, 2, 1]])
    m = O.EdgeMesh(v, f)
    e = int(np.flatnonzero((m.ev == [1, 2]).all(1))[0])
    assert O.edge_cot_sums(m)[e] < 0
    assert O.flip_to_delaunay(m) == 1
    lab, lbd = np.linalg.norm(a - b), np.linalg.norm(b - d)
    ang = np.arccos(np.dot(a - b, c - b) / (lab * np.linalg.norm(c - b))) + np.arccos(np.dot(d - b, c - b) / (lbd * np.linalg.norm(c - b)))
    want = np.sqrt(lab ** 2 + lbd ** 2 - 2 * lab * lbd * np.cos(ang))
    assert abs(m.el[e] - want) < 1e-14 and abs(want - np.linalg.norm(a - d)) < 1e-14
    assert sorted(m.ev[e]) == [0, 3] and O.edge_cot_sums(m).min() >= 0
    assert sorted(map(sorted, m.fv.tolist())) == [[0, 1, 3], [0, 2, 3]]


def test_heat_distance_sphere_and_plane():
    v, f = O.icosphere(4)
    d = O.HeatSolver(v, f).distance(0)
    gc = np.arccos(np.clip(v @ v[0], -1, 1))
    assert np.abs(d - gc).max() < 0.04                           # 2 562 vertices on the unit sphere, distances up to pi
    g, gf = O.planar_grid(33)
    c = 16 * 33 + 16
    dg = O.HeatSolver(g, gf).distance(c)
    eu = np.linalg.norm(g - g[c], axis=1)
    assert np.abs(dg - eu)[eu < 0.3].max() < 0.015               # spacing 1/32, away from the boundary


def test_fixture_regenerates_from_its_body():
    z = O.load_fixture(GOLDEN)
    v = z["vertices_q"].astype(np.int64) / 1e8
    dmin, lab, margin, cols, s = O.marker_fields(v, z["faces"].astype(np.int64), list(z["markers"]), keep=(0,))
    assert s.flips == int(z["flips"])
    assert np.abs(dmin - z["min_dist"]).max() <= 1e-12
    assert np.abs(cols[0] - z["dist0"]).max() <= 1e-12
    ok = z["margin"] > 1e-9
    assert np.array_equal(lab[ok], z["label"][ok].astype(np.int64))
