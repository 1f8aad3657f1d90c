"""Isolating the subject of a raw cloud on the GPU: the plane hypotheses, scores, selection, refit and removal and the
connected components of csrc/cloud_isolate.hip against tests/_isolate_oracle.py -- bits wherever the definition is exact, the perturbation
bound for the refitted normal alone --, the grid against the brute-force components, prepare() with the new stages on the body-on-a-floor
fixture, and the cloud / depth commands.  Clouds of at most 11 430 points; every oracle result is computed once.  The refit cases print `PIN`
lines; profiles/cloud_isolate_pins.txt is the record of a run."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _cloud_oracle as CO
import _isolate_oracle as IO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"


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
    """The small clouds of tests/test_gpu_cloud.py, rebuilt, and the ones the components need; left unchanged."""
    rng = np.random.default_rng(11)
    g = np.arange(-2, 3) * 0.25
    line = rng.uniform(-1.0, 1.0, 100)[:, None] * np.array([1.0, 2.0, -0.5]) + [0.3, -0.2, 0.1]
    body = rng.standard_normal((256, 3)) * [0.15, 0.4, 0.1]
    ints = np.concatenate([np.stack(np.meshgrid(np.arange(0, 12, 3.0), np.arange(-4, 8, 4.0), [0.0, 5.0], indexing="ij"), -1).reshape(-1, 3),
                           [[3.0, 4.0, 0.0], [-5.0, 0.0, 0.0], [0.0, -3.0, 4.0]]])
    out = {"one": rng.standard_normal((1, 3)), "two": rng.standard_normal((2, 3)), "nine": rng.standard_normal((9, 3)),
           "r33": rng.standard_normal((33, 3)) * [0.2, 0.5, 0.1], "r257": rng.standard_normal((257, 3)) * [0.2, 0.5, 0.1] + [5.0, -3.0, 0.5],
           "copies": np.repeat(rng.standard_normal((1, 3)), 40, 0),
           "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3),
           "line": line, "far": np.concatenate([body[:100], [[1000.0, 0.0, 0.0]], body[100:]]), "ints": ints}
    rng = np.random.default_rng(31)
    out["three"] = rng.standard_normal((3, 3))
    out["xline"] = np.arange(100)[:, None] * np.array([[0.5, 1.0, -0.25]]) + [0.25, -2.0, 1.0]   # collinear in fp64 too: every product is exact
    out["r1025"] = rng.standard_normal((1025, 3)) * [0.5, 0.05, 0.5]                              # one row over a tile of the score kernel
    out["r4100"] = rng.standard_normal((4100, 3)) * [0.5, 0.05, 0.5] + [0.0, 2.0, 0.0]            # four rows over a workgroup's share
    t = 2.0 * np.pi * np.arange(200) / 200.0
    a, b = np.stack([np.cos(t), np.sin(t), 0 * t], 1), np.stack([1.0 + np.cos(t), 0 * t, np.sin(t)], 1)
    out["rings"] = np.stack([a, b], 1).reshape(-1, 3)                                             # two linked rings, rows interleaved, always 1 m apart
    out["chain"] = np.arange(700)[::-1, None] * np.array([[0.9 * 0.3, 0.0, 0.0]])                 # 0.9 r apart at r = 0.3, the lowest row at the far end
    return out


def _pack(clouds):
    from etch_amd import cloud as C
    return C.pack(clouds, DEV)


def _key_tensor(keys):
    from etch_amd import mesh_io
    return torch.from_numpy(mesh_io._keys(keys, len(keys))).to(DEV)


# ---- hypotheses ---------------------------------------------------------------------------------------------------------------------------
UP_RAW = (0.1, -0.2, 1.0)                                          # near the thin axis of the random clouds: the tilt limits admit some planes


@pytest.mark.parametrize("H", [1, 64, 1000])
def test_hypotheses_equal_the_oracle(small, H):
    from etch_amd import cloud as C
    from etch_amd import ops
    names = ["one", "two", "three", "r33", "r257", "line", "copies", "xline"]
    clouds = [small[n] for n in names]
    assert [len(c) for c in clouds][:5] == [1, 2, 3, 33, 257]
    keys = [7, 2 ** 64 - 1, 0, 0x123456789ABCDEF, 5, 6, 2 ** 63, 9]
    packed = _pack(clouds)
    for up, tilt in ((None, None), (UP_RAW, 0.0), (UP_RAW, 10.0), (UP_RAW, 90.0), (UP_RAW, None)):
        a = C._check_plane(len(clouds), 0.01, keys, H, up, tilt)
        planes, valid = ops.cloud_plane_hypotheses(packed.points, packed.offsets, _key_tensor(keys), H, up=a["up"], cos_tilt=a["cos_tilt"])
        assert planes.shape == (len(clouds), H, 4) and valid.dtype == torch.int32
        nvalid = 0
        for b, (n, c) in enumerate(zip(names, clouds)):
            wp, wv = IO.hypotheses(c, keys[b], H, a["up"], a["cos_tilt"])
            assert np.array_equal(_np(valid)[b], wv), (n, up, tilt)
            assert _same(planes[b], wp), (n, up, tilt)
            if n in ("one", "two", "copies", "xline"):                                           # `line` is rounded: a third of its triples span a sliver
                assert wv.sum() == 0
            nvalid += int(wv.sum())
        if H >= 64 and tilt != 0.0:
            assert nvalid > 0
        if up is not None and H >= 64:
            u = np.array(a["up"])
            g = _np(planes)[_np(valid) != 0]
            assert (IO.dot3(g[:, :3], u[None]) >= 0.0).all()                                     # oriented along up
    if H == 1000:                                                                                # a wider tilt admits more planes: the flag acts
        count = lambda tilt: int(IO.hypotheses(small["r257"], 5, H, C._check_plane(1, 0.01, [5], H, UP_RAW, tilt)["up"],
                                               C._check_plane(1, 0.01, [5], H, UP_RAW, tilt)["cos_tilt"])[1].sum())
        assert 0 <= count(0.0) < count(10.0) < count(90.0) <= H
    plane, counts, found = C.fit_plane(_pack([small["xline"], small["copies"], small["two"], np.zeros((0, 3))]), 0.01, [1], hypotheses=H)
    assert found.dtype == torch.bool and not _np(found).any() and not _np(plane).any() and not _np(counts).any()


# ---- score ------------------------------------------------------------------------------------------------------------------------------------
def _score(clouds, planes, tau, valid=None):
    from etch_amd import ops
    packed = _pack(clouds)
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.int32)).to(DEV)
    return _np(ops.cloud_plane_score(packed.points, packed.offsets, torch.from_numpy(np.ascontiguousarray(planes, np.float64)).to(DEV), tau, valid=v))


def test_score_counts_rows_exactly_on_the_threshold_as_inliers(small):
    lattice = small["lattice"]
    s2 = math.sqrt(0.5)
    hand = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.25], [0.0, 1.0, 0.0, -0.5], [s2, s2, 0.0, 0.0], [0.0, 0.0, 1.0, 7.0]])
    for tau, first in ((0.25, [75, 25, 25]), (0.2499, [25, 50, 50])):
        got = _score([lattice], hand[None], tau)[0]
        assert got.dtype == np.int32 and np.array_equal(got, IO.score(lattice, hand, tau))
        assert got[0].tolist() == first and got[1].tolist() == first and (got.sum(1) == 125).all()
    at = _score([lattice], hand[None], 0.25)[0]
    assert at[2].tolist() == [75, 50, 0] and at[3].tolist() == [50, 0, 75] and at[5].tolist() == [0, 125, 0]      # x + 0.25, y - 0.5, z + 7


@pytest.fixture(scope="module")
def scored(small):
    """1 000 planes (not a multiple of the workgroup's 512), three of them flagged invalid among valid ones, and the oracle's counts for four
    clouds, computed once."""
    planes, valid = IO.hypotheses(small["r1025"], 77, 1000)
    assert valid.sum() > 990
    valid = valid.copy()
    valid[[3, 511, 999]] = 0
    names = ["r1025", "lattice", "r33", "r4100"]
    want = {n: IO.score(small[n], planes, 0.03, valid) for n in names}
    return planes, valid, names, want


def test_score_equals_the_oracle_past_a_tile_and_skips_invalid_planes(small, scored):
    planes, valid, names, want = scored
    for n in ("r1025", "r4100"):
        got = _score([small[n]], planes[None], 0.03, valid[None])[0]
        assert np.array_equal(got, want[n]), n
        assert (got[[3, 511, 999]] == 0).all() and (got[valid != 0].sum(1) == len(small[n])).all()
    assert want["r1025"][:, 0].max() > 100
    every = _score([small["r1025"]], planes[None], 0.03)[0]                                        # no flags: every plane counts
    assert every[[3, 511, 999]].sum(1).tolist() == [1025] * 3 and np.array_equal(every[valid != 0], want["r1025"][valid != 0])
    assert np.array_equal(_score([small["r1025"]], planes[None], 0.03, valid[None])[0], want["r1025"])   # two runs


def test_score_of_a_ragged_batch_equals_each_cloud_alone(small, scored):
    planes, valid, names, want = scored
    clouds = [small["r1025"], np.zeros((0, 3)), small["lattice"], small["r33"], small["r4100"]]
    B = len(clouds)
    got = _score(clouds, np.repeat(planes[None], B, 0), 0.03, np.repeat(valid[None], B, 0))
    assert not got[1].any()
    for b, n in ((0, "r1025"), (2, "lattice"), (3, "r33"), (4, "r4100")):
        assert np.array_equal(got[b], want[n]), n


# ---- select -----------------------------------------------------------------------------------------------------------------------------------
def _select(planes, valid, counts, **kw):
    from etch_amd import ops
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a, d)).to(DEV)
    return [_np(x) for x in ops.cloud_plane_select(t(planes, np.float64), t(valid, np.int32), t(counts, np.int32), **kw)]


def test_select_takes_the_lowest_of_equal_planes_and_respects_min_inliers(small):
    rng = np.random.default_rng(41)
    H = 1500
    base, _ = IO.hypotheses(small["r1025"], 3, 40)
    planes = base[rng.integers(0, 40, H)]                                                        # every plane many times over
    valid = np.ones(H, np.int32)
    valid[rng.integers(0, H, 100)] = 0
    counts = IO.score(small["r1025"], planes, 0.03, valid)
    best = counts[:, 0].max()
    ties = np.flatnonzero(counts[:, 0] == best)
    assert len(ties) > 5                                                                         # duplicated planes tie
    for min_inliers, has_up in ((3, False), (3, True), (best, False), (best + 1, False)):
        plane, c, found = _select(planes[None], valid[None], counts[None], min_inliers=int(min_inliers), has_up=has_up)
        wp, wc, wf = IO.select(planes, valid, counts, int(min_inliers), has_up)
        assert bool(found[0]) == wf == (min_inliers <= best) and _same(plane[0], wp) and np.array_equal(c[0], wc)
    # hand-made counts tell which h won: equal inliers at h = 7, 3 and 900, h = 2 better but invalid
    planes = np.arange(4 * H, dtype=np.float64).reshape(H, 4)
    valid = np.ones(H, np.int32)
    counts = np.zeros((H, 3), np.int32)
    counts[[7, 3, 900], 0] = 50
    counts[2, 0], valid[2] = 60, 0
    counts[:, 1], counts[:, 2] = np.arange(H), 7
    plane, c, found = _select(planes[None], valid[None], counts[None], has_up=True)
    assert found[0] == 1 and _same(plane[0], planes[3]) and c[0].tolist() == [50, 3, 7]
    plane, c, found = _select(planes[None], valid[None], counts[None], has_up=False)               # below (7) > above (3): negated and swapped
    assert _same(plane[0], -planes[3]) and c[0].tolist() == [50, 7, 3]
    counts[1400, 0] = 50
    counts[:, 2] = 0
    plane, c, found = _select(np.stack([planes, planes]), np.stack([valid, 0 * valid]), np.stack([counts, counts]), has_up=False)
    assert found.tolist() == [1, 0] and _same(plane[0], planes[3]) and not plane[1].any() and not c[1].any()      # above >= below stays; no valid plane


# ---- refit ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def discs():
    """Noisy floor discs with something standing on them: the gap between the smallest eigenvalue and the next is wide."""
    rng = np.random.default_rng(51)
    out = []
    for n, noise, normal in ((3000, 0.003, (0.0, 1.0, 0.0)), (1500, 0.001, (0.2, 0.9, -0.3)), (5000, 0.005, (-0.05, 0.02, 1.0))):
        w = np.array(normal) / np.linalg.norm(normal)
        e1 = np.cross(w, [1.0, 0.3, 0.2])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(w, e1)
        rad, ang = 1.5 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        floor = (rad * np.cos(ang))[:, None] * e1 + (rad * np.sin(ang))[:, None] * e2 + rng.uniform(-noise, noise, n)[:, None] * w
        blob = rng.standard_normal((n // 3, 3)) * 0.15 + 0.6 * w
        out.append(rng.permutation(np.concatenate([floor, blob])) + rng.uniform(-2, 2, 3))
    return out


def test_refit_stays_within_the_perturbation_bound_and_its_counts_are_exact(discs):
    from etch_amd import cloud as C
    tau, H, keys = 0.02, 128, [11, 12, 13]
    packed = _pack(discs)
    p0, c0, f0 = C.fit_plane(packed, tau, keys, hypotheses=H, refit=False)
    p1, c1, f1 = C.fit_plane(packed, tau, keys, hypotheses=H)
    out, keep, p2, f2 = C.remove_plane(packed, tau, keys, hypotheses=H)
    assert _np(f0).all() and _np(f1).all() and _same(p1, p2)
    keeps = _split(keep, discs)
    for b, p in enumerate(discs):
        wp, wc, wf = IO.ransac(p, keys[b], H, tau)
        assert wf and _same(p0[b], wp) and np.array_equal(_np(c0)[b], wc)                         # before the refit: bits
        got = _np(p1)[b]
        assert np.array_equal(_np(c1)[b], IO.score(p, got[None], tau)[0])                         # the counts and the mask on the returned plane's bits
        assert np.array_equal(keeps[b], IO.keep_above(p, got, True, tau))
        ref, w, m = IO.refit_eigh(p, wp, tau)
        assert m == wc[0] and w[1] - w[0] > 0.5 * w[1]
        bound = 16.0 * m * 2.0 ** -53 * w[2] / (w[1] - w[0])
        angle = math.atan2(np.linalg.norm(np.cross(got[:3], ref[:3])), float(got[:3] @ ref[:3]))
        extent = float(np.linalg.norm(p.max(0) - p.min(0)))
        print(f"PIN refit cloud {b}: m {m}, eigenvalues {w[0]:.4e} {w[1]:.4e} {w[2]:.4e}, angle {angle:.3e} rad (bound {bound:.3e}), "
              f"|d - d_ref| {abs(got[3] - ref[3]):.3e} (bound {bound * extent:.3e}), |n| - 1 {abs(np.linalg.norm(got[:3]) - 1.0):.1e}")
        assert angle <= bound and abs(got[3] - ref[3]) <= bound * extent
        assert float(got[:3] @ wp[:3]) > 0.999 and np.abs(IO.signed(p, got)[np.abs(IO.signed(p, wp)) <= tau]).mean() < 0.006
    assert np.array_equal(_np(out.offsets), np.concatenate([[0], np.cumsum([k.sum() for k in keeps])]))
    assert _same(out.points, np.concatenate([p[k] for p, k in zip(discs, keeps)]))
    alone = C.fit_plane(_pack([discs[1]]), tau, [12], hypotheses=H)
    assert _same(alone[0][0], p1[1]) and np.array_equal(_np(alone[1])[0], _np(c1)[1])              # a cloud alone = the same cloud in the batch
    again = C.fit_plane(packed, tau, keys, hypotheses=H)
    assert _same(again[0], p1)                                                                     # two runs: the sums have one order


# ---- components ---------------------------------------------------------------------------------------------------------------------------------
def _components(clouds, r, **kw):
    from etch_amd import cloud as C
    label, size = C.cluster(_pack(clouds), r, **kw)
    assert label.dtype == torch.int32 and size.dtype == torch.int32
    return _split(label, clouds), _split(size, clouds)


@pytest.fixture(scope="module")
def component_oracle(small):
    names = ["one", "two", "copies", "lattice", "ints", "far", "chain", "rings", "r257"]
    return names, {n: IO.components(small[n], 0.3) for n in names}


def test_components_equal_the_oracle_in_both_forms(small, component_oracle):
    for names, r in ((["one", "two", "copies", "lattice"], 0.25), (["lattice"], 0.2499), (["ints", "nine"], 5.0)):
        clouds = [small[n] for n in names]
        want = [IO.components(c, r) for c in clouds]
        for kw in (dict(), dict(brute=True)):
            labels, sizes = _components(clouds, r, **kw)
            for n, l, s, w in zip(names, labels, sizes, want):
                assert np.array_equal(l, w[0]) and np.array_equal(s, w[1]), (n, r, kw)
    l, s = _components([small["lattice"]], 0.25)
    assert (l[0] == 0).all() and (s[0] == 125).all()                                               # one component through d2 == r r edges
    l, s = _components([small["lattice"]], 0.2499)
    assert np.array_equal(l[0], np.arange(125)) and (s[0] == 1).all()
    l, s = _components([small["ints"]], 5.0)
    assert (CO.d2_rows(small["ints"], np.arange(len(small["ints"]))) == 25.0).sum() >= 6 and len(set(l[0])) < len(l[0])
    l, s = _components([small["copies"], small["one"]], 0.25)
    assert (l[0] == 0).all() and (s[0] == 40).all() and l[1].tolist() == [0] and s[1].tolist() == [1]


def test_components_of_a_ragged_batch_equal_each_cloud_alone(small, component_oracle):
    names, want = component_oracle
    clouds = [small[n] for n in names]
    labels, sizes = _components(clouds, 0.3)
    blabels, bsizes = _components(clouds, 0.3, brute=True)
    for n, l, s, bl, bs in zip(names, labels, sizes, blabels, bsizes):
        assert np.array_equal(l, want[n][0]) and np.array_equal(s, want[n][1]), n
        assert np.array_equal(bl, l) and np.array_equal(bs, s), n
    for n in ("chain", "rings", "far", "two"):
        l1, s1 = _components([small[n]], 0.3)
        assert np.array_equal(l1[0], want[n][0]) and np.array_equal(s1[0], want[n][1]), n
    at = dict(zip(names, zip(labels, sizes)))
    assert (at["chain"][0] == 0).all() and (at["chain"][1] == 700).all()                           # hooked from the far end through three workgroups
    assert np.array_equal(at["rings"][0], np.arange(400) % 2) and (at["rings"][1] == 200).all()    # linked, never within r of each other
    assert at["far"][0][100] == 100 and at["far"][1][100] == 1                                     # the far point is a singleton
    rl, rs = _components(clouds[::-1], 0.3)
    assert np.array_equal(rl[-1], labels[0]) and np.array_equal(rl[1], labels[-2])                 # the batch in another order


# ---- keep ---------------------------------------------------------------------------------------------------------------------------------------
def test_keep_clusters_ties_thresholds_and_emptied_clouds():
    from etch_amd import cloud as C
    from etch_amd._lib import EtchHipError
    rng = np.random.default_rng(61)
    blob = lambda n, c: rng.uniform(-0.05, 0.05, (n, 3)) + c
    a, b, c3 = blob(20, [0, 0, 0]), blob(20, [3, 0, 0]), blob(12, [0, 3, 0])
    tied = np.concatenate([c3[:5], np.stack([b, a], 1).reshape(-1, 3), c3[5:]])                    # rows 0-4: c3; then b, a interleaved: b owns row 5
    other = np.concatenate([blob(30, [1, 1, 1]), blob(7, [5, 5, 5])])
    clouds = [tied, other]
    want = [IO.components(x, 0.2) for x in clouds]
    assert sorted(set(want[0][1])) == [12, 20] and sorted(set(want[0][0])) == [0, 5, 6]
    for largest, min_points in ((True, 1), (False, 12), (False, 13), (False, 20), (True, 20), (False, 7), (False, 8)):
        out, keep = C.keep_clusters(_pack(clouds), 0.2, largest=largest, min_points=min_points)
        wk = [IO.component_keep(l, s, largest, min_points)[0] for l, s in want]
        assert keep.dtype == torch.bool and np.array_equal(_np(keep), np.concatenate(wk)), (largest, min_points)
        pts, idx, off = CO.compact(clouds, wk)
        assert _same(out.points, pts) and np.array_equal(_np(out.index), idx) and np.array_equal(_np(out.offsets), off)
    out, keep = C.keep_clusters(_pack(clouds), 0.2)
    k0 = _np(keep)[:len(tied)]
    assert k0.sum() == 20 and k0[5] and not k0[6] and not k0[:5].any()                             # of the two clusters of 20 the one with the lowest row
    with pytest.raises(EtchHipError, match="keep_clusters: cloud 0: no row is left"):
        C.keep_clusters(_pack(clouds), 0.2, largest=False, min_points=21)                          # the first cloud's clusters have 20, 20 and 12 rows
    with pytest.raises(EtchHipError, match="keep_clusters: cloud 1: no row is left"):
        C.keep_clusters(_pack(clouds[::-1]), 0.2, largest=True, min_points=21)
    flat = np.stack(np.meshgrid(np.arange(10) * 0.1, [0.0], np.arange(10) * 0.1, indexing="ij"), -1).reshape(-1, 3)
    hill = np.concatenate([flat, blob(60, [0.5, 0.4, 0.5])])
    with pytest.raises(EtchHipError, match="remove_plane: cloud 1: no row is left"):
        C.remove_plane(_pack([hill, flat]), 0.01, [1], hypotheses=64, up=(0, 1, 0), max_tilt=5.0)  # nothing stands on the second floor
    out, keep, plane, found = C.remove_plane(_pack([hill, flat[:2]]), 0.01, [1], hypotheses=64, up=(0, 1, 0), max_tilt=5.0)
    assert _np(found).tolist() == [True, False] and _np(keep).tolist() == [False] * 100 + [True] * 62   # no plane found: every row stays


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    p, kind = IO.isolate_fixture()
    k1, s1, plane, found = IO.isolate_pipeline(p, 5)
    return types.SimpleNamespace(p=p, kind=kind, k1=k1, s1=s1, plane=plane, found=found)


FLOOR = dict(threshold=0.02, hypotheses=256, up=IO.UP, max_tilt=10.0)


def test_prepare_isolates_the_body_with_one_readback(scene, small, monkeypatch):
    from etch_amd import cloud as C
    p, kind = scene.p, scene.kind
    other = small["r257"]
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: reads.append(tuple(self.shape)) or cpu(self, *a, **k))
    plain = C.prepare(_pack([p, other]), 512, [5, 6], stat=(8, 1.0))
    before = len(reads)
    pts, centers, clean = C.prepare(_pack([p, other]), 512, [5, 6], stat=(8, 1.0), floor=dict(FLOOR, min_inliers=500), cluster=(0.05, 1))
    assert len(reads) - before == before == 2                                                      # the offsets check of the input, and THE readback
    monkeypatch.undo()
    assert clean.plane.is_cuda and clean.plane_found.is_cuda and clean.keep.is_cuda and plain[2].plane is None and plain[2].plane_found is None
    assert list(clean.stages) == ["input", "statistical", "floor", "cluster"] and _np(clean.plane_found).tolist() == [True, False]
    plane = _np(clean.plane)
    assert abs(np.linalg.norm(plane[0, :3]) - 1.0) < 1e-15 and float(plane[0, :3] @ scene.plane[:3]) > 0.9999 and not plane[1].any()
    keep, rows = IO.after_plane(p, scene.k1, scene.s1, plane[0], True)                            # the oracle on the returned plane's bits
    k1o = CO.stat_keep(CO.knn_mean(other, 8), 1.0)[0]
    keep_o, rows_o = IO.after_plane(other, k1o, other[k1o], np.zeros(4), False)                    # a blob has no floor of 500 rows: it passes through
    got = _np(clean.keep)
    assert np.array_equal(got, np.concatenate([keep, keep_o]))
    g0 = got[:len(p)]
    assert not g0[kind != 0].any()                                                                 # no floor, clutter or stray row
    assert np.array_equal(g0[kind == 0], IO.signed(p, plane[0])[kind == 0] > 0.02) and g0.sum() > 6600     # every body row more than tau above the plane
    assert clean.stages["input"].tolist() == [len(p), 257]
    for i, name in enumerate(("statistical", "floor", "cluster")):
        assert clean.stages[name].tolist() == [rows[i], rows_o[i]], name
    assert rows_o[1] == rows_o[0] and _same(clean.points, np.concatenate([p[keep], other[keep_o]]))
    assert np.array_equal(_np(clean.offsets), [0, rows[2], rows[2] + rows_o[2]])
    v = CO.body_vertices()
    bare = (v.min(0) + v.max(0)) / 2.0 + [0.0, IO.LIFT - v[:, 1].min(), 0.0]
    assert np.linalg.norm(_np(centers)[0] - bare) < 0.01                                           # within 1 cm of the bare body's centre
    assert pts.shape == (2, 512, 3) and pts.dtype == torch.float32
    picked = _np(pts)[0].astype(np.float64) + _np(centers)[0]
    assert (IO.signed(picked, plane[0]) > 0.02 - 1e-6).all()                                       # the network sees nothing of the floor
    same = C.prepare(_pack([p, other]), 512, [5, 6], stat=(8, 1.0))
    assert _same(same[0], plain[0]) and _same(same[2].points, plain[2].points)


# ---- the commands ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return _train_data.build(tmp_path_factory.mktemp("isolate_data"), DEV)


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


def _arrays_equal(a, b):
    za, zb = np.load(a), np.load(b)
    return sorted(za.files) == sorted(zb.files) and all(za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes()
                                                 for k in za.files)


def _same_folders(a, b):
    """The same files; every array of an .npz with the same bits (the archive itself carries the time it was written), other files byte for byte."""
    names = sorted(os.listdir(a))
    return names == sorted(os.listdir(b)) and all(_arrays_equal(a / n, b / n) if n.endswith(".npz") else (a / n).read_bytes() == (b / n).read_bytes()
                                                  for n in names)


ISOLATE_FLAGS = ["--floor_threshold", "0.02", "--floor_hypotheses", "256", "--floor_up", "0", "1", "0", "--floor_max_tilt", "10", "--cluster_radius", "0.05"]


def test_cloud_command_isolates_the_body_and_is_unchanged_without_the_flags(scene, common, tmp_path):
    from etch_amd import cloud as C
    from etch_amd import mesh_io
    p, kind = scene.p, scene.kind
    mesh_io.write_ply(p, tmp_path / "scene.ply")
    base = ["--cloud_path", str(tmp_path / "scene.ply"), "--outlier_k", "8", "--outlier_ratio", "1.0"]
    a, b, c, d = (tmp_path / x for x in "abcd")
    C.main(base + ISOLATE_FLAGS + ["--output_folder", str(a)] + common)
    rep = np.load(a / "scene_cloud.npz")
    assert {"plane", "plane_found", "rows_floor", "rows_cluster", "rows_statistical", "keep"} <= set(rep.files)
    _, _, clean = C.prepare(C.pack([p], DEV), 1024, [4], stat=(8, 1.0), floor=FLOOR, cluster=(0.05, 1))
    assert _same(rep["plane"], clean.plane) and rep["plane_found"].tolist() == [True] and np.array_equal(rep["keep"], _np(clean.keep))
    assert rep["rows_floor"].tolist() == clean.stages["floor"].tolist() and rep["rows_cluster"].tolist() == [int(rep["keep"].sum())] == rep["rows_output"].tolist()
    assert rep["rows_input"][0] > rep["rows_statistical"][0] > rep["rows_floor"][0] > rep["rows_cluster"][0] > 6600
    assert not rep["keep"][kind != 0].any() and int(rep["removed"]) == len(p) - int(rep["keep"].sum())
    assert {"scene_pred_smpl.obj", "scene_output_smpl_info.npz"} <= set(os.listdir(a))
    info = np.load(a / "scene_output_smpl_info.npz")
    assert all(np.isfinite(info[k]).all() for k in info.files)
    # without the new flags.  What can be checked in-tree: the report holds exactly the keys it held before the flags existed, and its arrays are those
    # of prepare(stat=) alone -- the stages tests/test_gpu_cloud.py holds to its oracle, unchanged.  The run with the flags spelled out as 0 takes the
    # same branch as the run without them, so their equality only shows that 0 means off and that two runs agree.
    C.main(base + ["--output_folder", str(b)] + common)
    C.main(base + ["--floor_threshold", "0", "--cluster_radius", "0", "--output_folder", str(c)] + common)
    assert _same_folders(b, c)
    old = np.load(b / "scene_cloud.npz")
    assert sorted(old.files) == ["center", "keep", "points", "removed", "rows_input", "rows_output", "rows_statistical"]
    p32, cen, plain = C.prepare(C.pack([p], DEV), 1024, [4], stat=(8, 1.0))
    assert _same(old["points"], p32[0]) and _same(old["center"], cen[0]) and np.array_equal(old["keep"], _np(plain.keep))
    assert np.abs(old["center"] - rep["center"]).max() > 1e-3 and old["keep"][kind == 1].sum() > 3000     # the flags act: the floor was in


def test_depth_command_drops_the_floor_under_a_rendered_body(common, tmp_path):
    from etch_amd import depth as D
    from etch_amd.inference_demo import Mesh
    from etch_amd.mesh_io import write_obj
    v = CO.body_vertices()
    f = np.load(CO.GOLDEN)["faces"].astype(np.int64)
    y0 = v[:, 1].min()
    cx, cz = (v[:, 0].min() + v[:, 0].max()) / 2.0, (v[:, 2].min() + v[:, 2].max()) / 2.0
    quad = np.array([[cx - 1.5, y0, cz - 1.5], [cx - 1.5, y0, cz + 1.5], [cx + 1.5, y0, cz + 1.5], [cx + 1.5, y0, cz - 1.5]])
    mesh = Mesh(np.concatenate([v, quad]), np.concatenate([f, len(v) + np.array([[0, 1, 2], [0, 2, 3]])]))
    write_obj(mesh, tmp_path / "stand.obj")
    view = ["--scan_path", str(tmp_path / "stand.obj"), "--view_azimuth", "60", "--view_elevation", "25", "--view_distance", "3.5", "--view_size", "120", "160"]
    flags = ["--floor_threshold", "0.02", "--floor_hypotheses", "256", "--floor_up", "0", "1", "0", "--floor_max_tilt", "10", "--cluster_radius", "0.12"]
    D.main(view + flags + ["--output_folder", str(tmp_path / "a")] + common)
    D.main(view + ["--output_folder", str(tmp_path / "b")] + common)
    D.main(view + ["--floor_threshold", "0", "--cluster_radius", "0", "--output_folder", str(tmp_path / "c")] + common)
    rep, old = np.load(tmp_path / "a" / "stand_view.npz"), np.load(tmp_path / "b" / "stand_view.npz")
    # the keys the view file had before the flags existed; 0 means off (both runs take one branch: this shows no more than that, and that two runs agree)
    assert sorted(old.files) == ["camera", "center", "depth", "pixel", "points", "size"] and _same_folders(tmp_path / "b", tmp_path / "c")
    assert {"plane", "plane_found", "rows_floor", "rows_cluster"} <= set(rep.files) and rep["plane_found"].tolist() == [True]
    plane = rep["plane"][0]
    assert plane[1] > 0.9999 and abs(plane[3] + y0) < 2e-3                                         # the quad's plane: y = y0
    seen = int(np.isfinite(rep["depth"]).sum())
    assert seen > rep["rows_floor"][0] >= rep["rows_cluster"][0] > 300 and seen - rep["rows_floor"][0] > 1000     # the floor was most of the view
    height = lambda z: z["points"].astype(np.float64)[:, 1] + z["center"][1] - y0
    assert (height(rep) > 0.02 - 1e-5).all() and (height(old) < 0.01).sum() > 100                  # picked points: none on the floor / many on it
    assert {"stand_pred_smpl.obj", "stand_output_smpl_info.npz"} <= set(os.listdir(tmp_path / "a"))
