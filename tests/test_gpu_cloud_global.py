"""Global registration of raw clouds on the GPU: csrc/cloud_global.hip against tests/_global_oracle.py -- neighbour lists,
pair-feature counts (by the edge rule), descriptors, matches, hypotheses, scores and the selection by integers or bits, the triple's pose within
the bound of section 23 of an SVD Kabsch -- and the whole of global_align, align(init="global"), register_views(init="global") and the command
on views of the fixture body that start 150 degrees and a metre apart.  Clouds of at most 6 890 rows."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _align_oracle as AO
import _global_oracle as GO
import _normals_oracle as NO
import _train_data

pytestmark = pytest.mark.gpu
DEV = "cuda"
CELLS = (0.07, 1.3)
U = 2.0 ** -53
EYE = (0.3, -0.2, 10.0)                                            # the viewpoint of the small clouds


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.int64, 4: np.int32, 1: np.int8}[a.dtype.itemsize])


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


@pytest.fixture(scope="module")
def clouds():
    """The small clouds of test_gpu_cloud_align.py, rebuilt, and the two views of the first fixture; (name, points, viewpoint), left unchanged."""
    rng = np.random.default_rng(11)
    g = np.arange(-2, 3) * 0.25
    body = rng.standard_normal((256, 3)) * [0.15, 0.4, 0.1]
    small = {"one": rng.standard_normal((1, 3)), "nine": rng.standard_normal((9, 3)), "r33": rng.standard_normal((33, 3)) * [0.2, 0.5, 0.1],
             "r257": rng.standard_normal((257, 3)) * [0.2, 0.5, 0.1] + [5.0, -3.0, 0.5], "copies": np.repeat(rng.standard_normal((1, 3)), 40, 0),
             "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), "body": body, "empty": np.zeros((0, 3))}
    out = [(n, small[n], np.array(EYE)) for n in ("r33", "r257", "lattice", "copies", "one", "empty", "body")]
    for az in (0.0, 60.0):
        p, cam = GO.view(az)
        out.append((f"view {az:g}", p, cam))
    return out


@pytest.fixture(scope="module")
def lists32(clouds):
    """The oracle's neighbour lists at k = 32, computed once: the list at a smaller k is its prefix."""
    return [NO.neighbours(p, 32) for _, p, _ in clouds]


def _features(clouds, k, **kw):
    from etch_amd import cloud as C
    c = C.pack([p for _, p, _ in clouds], DEV)
    return c, C.features(c, k, viewpoint=np.stack([v for _, _, v in clouds]), return_spfh=True, **kw)


def _split(values, clouds):
    o = np.concatenate([[0], np.cumsum([len(c[1]) for c in clouds])])
    v = _np(values)
    assert len(v) == o[-1]
    return [v[a:b] for a, b in zip(o[:-1], o[1:])]


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 16, 32])
def test_descriptors_equal_the_oracle_in_every_form(clouds, lists32, k):
    from etch_amd import cloud as C
    pack, (F, has, spfh, c, nbr) = _features(clouds, k)
    assert F.dtype == torch.float64 and has.dtype == torch.bool and spfh.dtype == torch.int32 and c.dtype == torch.int32 and nbr.dtype == torch.int32
    assert tuple(F.shape) == (pack.points.shape[0], 33) and tuple(nbr.shape) == (pack.points.shape[0], k)
    for kw in [dict(cell=x) for x in CELLS] + [dict(brute=True)]:                           # the same bits for any cell size and from the whole scan
        _, other = _features(clouds, k, **kw)
        assert all(_same(a, b) for a, b in zip(other, (F, has, spfh, c, nbr))), kw
    nrm, _, flag = C.normals(pack, k, viewpoint=np.stack([v for _, _, v in clouds]))
    parts = [_split(x, clouds) for x in (F, has, spfh, c, nbr, nrm, flag)]
    for i, (name, p, cam) in enumerate(clouds):
        gF, gh, gs, gc, gn, gnrm, gflag = (x[i] for x in parts)
        want = GO.pad(lists32[i][:, :max(min(k, len(p) - 1), 0)], k)
        assert np.array_equal(gn, want), name                                              # the lists, by integers
        ws, wc, b, edge, counted = GO.spfh(p, gnrm, gflag, want)
        why, share = GO.edge_rule(gs, gc, ws, wc, b, edge, counted)
        print(f"PIN descriptors k={k} {name}: {len(p)} rows, {int(counted.sum())} pairs counted, share of rows with an edge pair {share:.5f}, "
              f"rows whose counts differ from the oracle's {int((gs != ws).any(1).sum())}, rows with a feature {int(gh.sum())}")
        assert why is None, (name, why)
        if name == "body" or name.startswith("view"):
            assert share <= 0.01, (name, share)
        wF, wh = GO.fpfh(p, gs, gc, gn.astype(np.int64), gflag)                            # pass 2 on the GPU's own counts and lists: by bits
        assert _same(gF, wF) and np.array_equal(gh, wh), name
        if name in ("copies", "one"):
            assert not gh.any() and (gc == 0).all(), name
        if name.startswith("view") and k >= 16:
            assert gh.mean() > 0.95 and np.allclose(gF[gh].reshape(-1, 3, 11).sum(2), 100.0, rtol=0, atol=1e-9), name
    assert sum(len(p) for _, p, _ in clouds) == F.shape[0] and clouds[5][0] == "empty"      # an empty cloud passes through


def test_rows_with_a_flagged_normal_have_no_feature_and_count_in_no_pair(clouds):
    from etch_amd import cloud as C
    name, p, cam = clouds[1]
    pack = C.pack([p], DEV)
    nrm, _, flag = C.normals(pack, 16, viewpoint=cam)
    given = _np(nrm).copy()
    gone = [3, 40, 41, 200]
    given[gone] = 0.0
    F, has, spfh, c, nbr = C.features(pack, 16, normals=given, return_spfh=True)
    wflag = _np(flag).copy()
    wflag[gone] = 2
    ws, wc, b, edge, counted = GO.spfh(p, given, wflag, _np(nbr).astype(np.int64))
    assert GO.edge_rule(_np(spfh), _np(c), ws, wc, b, edge, counted)[0] is None
    assert not _np(has)[gone].any() and (_np(c)[gone] == 0).all() and _np(has).sum() >= 200
    full = C.features(pack, 16, viewpoint=cam, return_spfh=True)
    near = np.isin(_np(nbr), gone).any(1)
    assert (_np(c)[near & ~np.isin(np.arange(257), gone)] < _np(full[3])[near & ~np.isin(np.arange(257), gone)]).all() and near.sum() > 4
    assert _same(full[0], C.features(pack, 16, normals=nrm)[0])                             # given normals = the same normals computed


# ---- matching ---------------------------------------------------------------------------------------------------------------------------------------------
def test_matches_equal_the_oracle_by_bits(clouds):
    from etch_amd import ops
    _, (F, has, _, _, _) = _features(clouds, 16)
    Fs, hs = _split(F, clouds), _split(has, clouds)
    v0, v60, r257, body = Fs[7], Fs[8], Fs[1], Fs[6]
    h0, h60, h257, hb = hs[7], hs[8], hs[1], hs[6]
    dup_t, dup_h = np.concatenate([r257[:50], r257[10:12], r257[50:]]), np.concatenate([h257[:50], h257[10:12], h257[50:]])
    assert h257[10] and h257[11]
    cases = [("views", v60, h60, v0, h0), ("coincident features", r257, h257, dup_t, dup_h), ("target without a feature", body, hb, r257, np.zeros(257, bool)),
             ("source without a feature", body, np.zeros(256, bool), r257, h257), ("empty target", body, hb, r257[:0], h257[:0]),
             ("empty source", body[:0], hb[:0], r257, h257), ("tile edge", r257, h257, body[:65], hb[:65])]
    off = lambda parts: _dev(np.concatenate([[0], np.cumsum([len(x) for x in parts])]), np.int32)      # noqa: E731
    fs, fh = _dev(np.concatenate([c[1] for c in cases])), _dev(np.concatenate([c[2] for c in cases]), np.int32)
    ft, th = _dev(np.concatenate([c[3] for c in cases])), _dev(np.concatenate([c[4] for c in cases]), np.int32)
    so, to = off([c[1] for c in cases]), off([c[3] for c in cases])
    match, dist = ops.cloud_feature_match(fs, fh, so, ft, th, to)
    assert match.dtype == torch.int32 and dist.dtype == torch.float64
    o = _np(so)
    for i, (name, a, ha, b, hb_) in enumerate(cases):
        wm, wd = GO.match(a, ha, b, hb_)
        gm, gd = _np(match)[o[i]:o[i + 1]], _np(dist)[o[i]:o[i + 1]]
        assert np.array_equal(gm, wm) and _same(gd, wd), name
        if name == "views":
            assert (gm >= 0).mean() > 0.95 and len(np.unique(gm)) > 500
        if name == "coincident features":
            assert gm[10] == 10 and gm[11] == 11 and gd[10] == 0.0 and (gm[50:][ha[50:]] == np.arange(52, 259)[ha[50:]]).all()      # the lower of two equal rows
        if "without" in name or "empty" in name:
            assert (gm == -1).all() and np.isinf(gd).all(), name


# ---- hypotheses -------------------------------------------------------------------------------------------------------------------------------------------
def _correspondence_cases(clouds):
    """(name, a, b, target rows): exact copies moved rigidly with a share of outliers and repeated target rows; fewer than three; none."""
    rng = np.random.default_rng(53)
    v60 = clouds[8][1]
    R0, t0 = AO.rotation([0.3, 1.0, 0.2], 150.0), np.array([0.3, 0.9, 0.3])
    b = AO.apply(R0, t0, v60)
    rows = np.arange(len(v60))
    wrong = rng.random(len(v60)) < 0.4
    rows[wrong] = rng.integers(0, len(v60), int(wrong.sum()))
    big = ("view", v60, b[rows], rows)
    r257 = clouds[1][1]
    rows2 = np.arange(257)
    rows2[::3] = rows2[1::3][:len(rows2[::3])]                                             # every third correspondence repeats its neighbour's target row
    small = ("repeated rows", r257, AO.apply(R0, t0, r257)[rows2], rows2)
    return [big, small, ("two", r257[:2], r257[:2], np.arange(2)), ("none", r257[:0], r257[:0], np.arange(0))]


def _corr_tensors(cases):
    return (_dev(np.concatenate([c[1] for c in cases])), _dev(np.concatenate([c[2] for c in cases])), _dev(np.concatenate([c[3] for c in cases]), np.int32),
            _dev(np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]), np.int32))


@pytest.mark.parametrize("H", [64, 4096])
def test_hypotheses_equal_the_oracle(clouds, H):
    from etch_amd import ops
    cases = _correspondence_cases(clouds)
    a, b, rows, off = _corr_tensors(cases)
    for keys in ([7, 2 ** 40 + 3, 5, 9], [2 ** 63 + 11, 0, 1, 2]):
        key = _dev(np.array(keys, np.uint64).view(np.int64))
        T, valid, triples = ops.cloud_global_hypotheses(a, b, rows, off, key, H)
        assert tuple(T.shape) == (4, H, 12) and valid.dtype == torch.int32 and triples.dtype == torch.int32
        T, valid, triples = _np(T), _np(valid), _np(triples)
        for i, (name, pa, pb, rr) in enumerate(cases):
            idx, wvalid, wT = GO.hypotheses(pa, pb, rr, keys[i], H)
            assert np.array_equal(triples[i], idx) and np.array_equal(valid[i], wvalid), (name, keys[i])
            if name in ("two", "none"):
                assert not valid[i].any()
            assert np.array_equal(T[i][valid[i] == 0], np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (int((valid[i] == 0).sum()), 1))), name
            worst = 0.0
            for h in np.flatnonzero(valid[i])[:200]:
                w = AO.step(pa[idx[h]], pb[idx[h]], np.arange(3), np.eye(3), np.zeros(3))
                mm, A, S = w["m"], w["abs_sums"], w["sums"]
                dC = np.array([[mm * U * (A[6 + 3 * x + e] + (A[x] * abs(S[3 + e]) + abs(S[x]) * A[3 + e]) / mm) + 4 * U * (abs(S[6 + 3 * x + e]) + abs(S[x] * S[3 + e]) / mm)
                                for e in range(3)] for x in range(3)])
                gap = w["S"][1] + w["sign"] * w["S"][2]
                bound = 2.0 * float(np.sqrt((dC * dC).sum())) / gap + 16 * U * w["S"][0] / gap
                R, t = T[i, h, :9].reshape(3, 3), T[i, h, 9:]
                ang = math.radians(AO.angle_between(R, w["dR"]))
                reach = float(np.abs(np.concatenate([pa[idx[h]], pb[idx[h]]])).max())
                assert w["ok"] and ang <= bound, (name, h, ang, bound)
                assert abs(np.linalg.det(R) - 1.0) <= 16 * U and np.abs(AO.apply(R, t, pa[idx[h]]) - AO.apply(w["dR"], w["dt"], pa[idx[h]])).max() <= 4.0 * bound * reach + 64 * U * reach
                worst = max(worst, ang / bound)
            print(f"PIN hypotheses H={H} key={keys[i]} {name}: {int(valid[i].sum())} valid, worst rotation error / bound {worst:.3f}")
        if H == 4096:
            assert valid[0].sum() > 100 and valid[1].sum() > 100
            r = cases[1][3][triples[1]]                                                     # the target rows of the small case's triples
            twice = (r[:, 0] == r[:, 1]) | (r[:, 0] == r[:, 2]) | (r[:, 1] == r[:, 2])
            distinct = (triples[1][:, 0] != triples[1][:, 1]) & (triples[1][:, 0] != triples[1][:, 2]) & (triples[1][:, 1] != triples[1][:, 2])
            assert (twice & distinct).sum() >= 5 and not valid[1][twice].any()              # distinct correspondences onto one target row: invalid


# ---- scores and the selection --------------------------------------------------------------------------------------------------------------------------------
def test_scores_and_selection_equal_the_oracle_by_integers(clouds):
    from etch_amd import ops
    cases = _correspondence_cases(clouds)
    rng = np.random.default_rng(59)
    ints = np.concatenate([np.stack(np.meshgrid(np.arange(0, 12, 3.0), np.arange(-4, 8, 4.0), [0.0, 5.0], indexing="ij"), -1).reshape(-1, 3),
                           [[3.0, 4.0, 0.0], [-5.0, 0.0, 0.0], [0.0, -3.0, 4.0]]])
    cases = cases[:2] + [("ints", ints, ints + [3.0, 4.0, 0.0], np.arange(len(ints)))] + cases[2:]
    a, b, rows, off = _corr_tensors(cases)
    H, tau = 601, 5.0                                                                      # 601: not a multiple of the 512 hypotheses a workgroup owns
    key = _dev(np.array([7, 8, 9, 10, 11], np.int64))
    T, valid, _ = ops.cloud_global_hypotheses(a, b, rows, off, key, H)
    T = T.clone()
    flat = lambda R, t: np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)])      # noqa: E731
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    exact = [flat(np.eye(3), [0, 0, 0]), flat(np.eye(3), [3, 4, 0]), flat(np.eye(3), [6, 8, 0]), flat(np.eye(3), [6, 8, 1e-6]), flat(np.eye(3), [3, 4, 5]),
             flat(quarter, [0, 0, 0]), flat(quarter @ quarter, [3, 4, 0])]
    T[2, :len(exact)] = _dev(np.stack(exact))
    v2 = valid.clone()
    v2[2] = 1
    v2[2, 5] = 0
    for tau_, vv in ((tau, v2), (0.03, valid), (0.03, None), (tau, None)):
        got = _np(ops.cloud_global_score(a, b, off, T, tau_, valid=vv))
        assert got.dtype == np.int32 and got.shape == (5, H)
        for i, (name, pa, pb, _) in enumerate(cases):
            want = GO.score(pa, pb, _np(T)[i], tau_, None if vv is None else _np(vv)[i])
            assert np.array_equal(got[i], want), (name, tau_)
        if vv is v2:
            n = len(ints)
            assert got[2, :7].tolist()[:5] == [n, n, n, 0, n] and got[2, 5] == 0            # d2 == tau^2 exactly counts, a last bit beyond does not
        if vv is valid and tau_ == 0.03:
            assert got[0].max() > 0.5 * len(cases[0][1]) and (got[0][_np(valid)[0] == 0] == 0).all() and not got[3].any() and not got[4].any()
            counts = got
    R, t, best, best_h, found = (_np(x) for x in ops.cloud_global_select(T, valid, _dev(counts), min_inliers=6))
    for i, (name, pa, pb, _) in enumerate(cases):
        h, ok = GO.select(_np(valid)[i], counts[i], 6)
        assert bool(found[i]) == ok and best_h[i] == h, name
        if ok:
            assert best[i] == counts[i, h] and _same(np.concatenate([R[i].reshape(9), t[i]]), _np(T)[i, h]), name
        else:
            assert best[i] == 0 and np.array_equal(R[i], np.eye(3)) and not t[i].any(), name
    assert found[:2].all() and not found[3:].any()
    tied = np.zeros((5, H), np.int32)
    tied[0, [5, 90, 600]] = 40                                                             # ties: the lowest valid h
    tied[1, [3, 4]] = [5, 5]                                                               # fewer than min_inliers
    tied[2, 7] = 9
    vt = np.ones((5, H), np.int32)
    vt[0, 5] = 0
    vt[2] = 0                                                                              # the best count belongs to an invalid hypothesis
    _, _, best, best_h, found = (_np(x) for x in ops.cloud_global_select(T, _dev(vt), _dev(tied), min_inliers=6))
    assert best_h.tolist() == [90, -1, -1, -1, -1] and found.tolist() == [1, 0, 0, 0, 0] and best.tolist() == [40, 0, 0, 0, 0]
    for i in range(5):
        assert (best_h[i], bool(found[i])) == GO.select(vt[i], tied[i], 6)
    _, _, best, best_h, found = (_np(x) for x in ops.cloud_global_select(T, _dev(vt), _dev(tied), min_inliers=0))
    assert best_h.tolist()[3:] == [0, 0] and found.tolist() == [1, 1, 0, 1, 1]              # every count 0 and min_inliers 0: the lowest h


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _global_kw(k):
    return dict(voxel=None, feature_k=k, hypotheses=GO.FIXTURE_H, tau=GO.FIXTURE_TAU)


@pytest.mark.parametrize("name", ["60", "90"])
def test_views_150_degrees_apart_are_registered_from_nothing(name):
    """Before any ICP global_align ends within 10 degrees and 5 cm (worst row) of the truth -- half of the basin section 23 measured, the bound
    the oracle alone meets on the CPU (test_global_host.py).  From there align(metric="plane") must end no further from the truth than twice what
    the same call reaches from section 23's 10 degree / 5 cm start: the partner sets differ on a partial overlap.  Plain align from the identity
    does not come within 10 degrees: the test needs the feature."""
    from etch_amd import cloud as C
    src, vs, tgt, vt, R0, t0, k = GO.fixture(name)
    s, t = C.pack([src], DEV), C.pack([tgt], DEV)
    g = C.global_align(s, t, [GO.FIXTURE_KEY], viewpoint=(vs, vt), **_global_kw(k))
    ang, worst = GO.pose_error(_np(g.R)[0], _np(g.t)[0], R0, t0, src)
    print(f"PIN global {name}: {len(src)} / {len(tgt)} rows, {g.correspondences[0]} correspondences, {g.inliers[0]} inliers, {ang:.3f} deg and {worst * 100:.2f} cm "
          f"(worst row) from the truth before any ICP")
    assert g.found[0] and ang <= 10.0 and worst <= 0.05
    kw = dict(metric="plane", **AO.VIEW_SETTINGS)
    res = C.align(s, t, init="global", keys=[GO.FIXTURE_KEY], viewpoint=(vs, vt), global_kw=_global_kw(k), **kw)
    Rp, tp = AO.start_pose(10.0, 0.05)
    ref = C.align(s, t, init=((Rp @ R0)[None], (Rp @ t0 + tp)[None]), **kw)
    plain = C.align(s, t, **kw)
    e_res = GO.pose_error(_np(res.R)[0], _np(res.t)[0], R0, t0, src)
    e_ref = GO.pose_error(_np(ref.R)[0], _np(ref.t)[0], R0, t0, src)
    e_plain = GO.pose_error(_np(plain.R)[0], _np(plain.t)[0], R0, t0, src)
    print(f"PIN align {name}: init='global' ends {e_res[0]:.4f} deg / {e_res[1] * 1e3:.3f} mm from the truth ({res.matched[0]} matched, {res.steps[0]} steps); "
          f"from the 10 deg / 5 cm start {e_ref[0]:.4f} deg / {e_ref[1] * 1e3:.3f} mm ({ref.matched[0]} matched); init=None {e_plain[0]:.1f} deg / {e_plain[1]:.3f} m")
    assert res.status[0] == 0 and res.start.found[0] and _same(res.start.R, g.R) and _same(res.start.t, g.t)
    assert e_res[0] <= 2.0 * e_ref[0] and e_res[1] <= 2.0 * e_ref[1]
    assert e_plain[0] > 10.0


def test_nothing_to_find_is_a_result_and_the_status_records_it(clouds):
    from etch_amd import cloud as C
    one, r33 = clouds[4][1], clouds[0][1]
    s, t = C.pack([one, r33], DEV), C.pack([r33, r33], DEV)
    g = C.global_align(s, t, [3, 4], voxel=None, feature_k=16, viewpoint=(EYE, EYE), hypotheses=64, tau=0.01, min_inliers=200)
    assert not g.found.any() and (g.inliers == 0).all() and g.correspondences[0] == 0 and g.correspondences[1] > 0
    assert np.array_equal(_np(g.R), np.tile(np.eye(3), (2, 1, 1))) and not _np(g.t).any()
    res = C.align(s, t, init="global", keys=[3, 4], viewpoint=(EYE, EYE), iters=2, global_kw=dict(voxel=None, feature_k=16, hypotheses=64, tau=0.01, min_inliers=200))
    assert (res.status & C.STATUS_GLOBAL_NOT_FOUND).all()
    same = C.global_align(s, t, [3, 4], voxel=None, feature_k=16, viewpoint=(EYE, EYE), hypotheses=64, tau=0.01, mutual=True)
    assert (same.correspondences <= g.correspondences).all() and same.found[1] and AO.angle_between(_np(same.R)[1], np.eye(3)) < 1e-6


def test_bad_arguments_raise_before_any_launch(clouds):
    from etch_amd import cloud as C
    one, two = C.pack([clouds[0][1]], DEV), C.pack([clouds[0][1], clouds[1][1]], DEV)
    with pytest.raises(ValueError, match="oriented normals"):
        C.features(one, 16)
    with pytest.raises(ValueError, match="not both"):
        C.features(one, 16, viewpoint=EYE, normals=np.zeros((33, 3)))
    for k in (2, 33, 3.5):
        with pytest.raises(ValueError, match="k must be an integer in 3 .. 32"):
            C.features(one, k, viewpoint=EYE)
    with pytest.raises(ValueError, match="viewpoint must be"):
        C.features(one, 16, viewpoint=[0.0, 1.0])
    with pytest.raises(ValueError, match="normals must be"):
        C.features(one, 16, normals=np.zeros((32, 3)))
    good = dict(viewpoint=(EYE, EYE))
    for kw, match in ((dict(voxel=0.0), "voxel must be positive"), (dict(hypotheses=0), "hypotheses must be"), (dict(hypotheses=262145), "hypotheses must be"),
                      (dict(tau=-1.0), "tau must be positive"), (dict(voxel=None), "give tau"), (dict(edge_similarity=0.0), "edge_similarity"),
                      (dict(edge_similarity=1.5), "edge_similarity"), (dict(min_edge=-0.1), "min_edge"), (dict(min_inliers=-1), "min_inliers"),
                      (dict(refit_steps=-1), "refit_steps"), (dict(feature_k=2), "k must be an integer"), (dict(viewpoint=None), "viewpoint must be"),
                      (dict(viewpoint=(EYE, None)), "viewpoint must give")):
        with pytest.raises(ValueError, match=match):
            C.global_align(one, one, [1], **{**good, **kw})
    with pytest.raises(ValueError, match="same number of clouds"):
        C.global_align(one, two, [1], **good)
    with pytest.raises(ValueError):
        C.global_align(two, two, [1, 2, 3], **good)                                        # one key per pair, or one for all
    with pytest.raises(ValueError, match="needs keys"):
        C.align(one, one, init="global", viewpoint=(EYE, EYE))
    with pytest.raises(ValueError, match="init must be"):
        C.align(one, one, init="rough")
    with pytest.raises(ValueError, match="belong to init='global'"):
        C.align(one, one, keys=[1])


# ---- views and the command ----------------------------------------------------------------------------------------------------------------------------------
VIEW_TURNS = (0.0, 150.0, -120.0)                                   # degrees about (0.3, 1, 0.2): the views 1 and 2 start more than 90 degrees away


def _camera_views():
    """Three views of the body (azimuths 0, 60, -60), each in a frame whose origin is its camera and which is turned by VIEW_TURNS.
    -> the views, the undisplaced rows, the true poses (R, t) into the frame of view 0."""
    parts = [GO.view(az) for az in (0.0, 60.0, -60.0)]
    moved = [GO.moved(p, cam, turn, cam) for (p, cam), turn in zip(parts, VIEW_TURNS)]
    assert all(np.abs(m[1]).max() < 1e-12 for m in moved)                                  # every camera sits at its view's origin
    R00, t00 = moved[0][2], moved[0][3]
    truth = [(R00.T @ m[2], R00.T @ (m[3] - t00)) for m in moved]
    return [m[0] for m in moved], [p for p, _ in parts], truth


def test_register_views_from_nothing_and_fuse_leave_every_surface_once():
    """Section 23's measure: the occupied 5 mm cells of the fused views against those of the undisplaced union, within 1 %.  The refinement is
    section 23's too, the point metric with its partial-overlap settings: the views are exact copies of vertices, which the point metric brings
    onto each other to rounding.  The plane metric stops 3 - 5 mm (worst row) from the truth on these back-face-culled views -- from the global
    start and from section 23's 10 degree / 5 cm start alike, test_views_150_degrees_apart_are_registered_from_nothing prints both -- and that is a
    cell's width: it measured 6 652 cells against 5 237, which says nothing about the start.
    The bound.  The oracle's pipeline alone (tests/_global_oracle.py register_views, on the CPU) does not meet 1 % on these back-face-culled views:
    it fuses to 5 630 cells against the union's 5 237 under the keys 7 and 8 (7.50 %: a row without a true partner still finds a wrong one
    inside the last gate of 1 cm, which leaves the poses 0.9 and 1.3 mm off) and to 6 957 under key 9, where the third view's 3 % of inliers
    lose to a mirrored pose (32.84 %).  As the issue rules for that case the bound is what the oracle reaches plus its spread over the three keys,
    7.50 % + 25.34 % = 32.84 %; and because that says little, the count must also lie within 1 % of the oracle's own count under the same key."""
    from etch_amd import cloud as C
    views, flat, truth = _camera_views()
    want = AO.occupied(np.concatenate([AO.apply(truth[0][0], truth[0][1], views[0])] + [AO.apply(R, t, v) for (R, t), v in zip(truth[1:], views[1:])]), 0.005)
    packed = [C.pack([v], DEV) for v in views]
    res = C.register_views(packed, init="global", keys=[GO.FIXTURE_KEY], viewpoints=[(0.0, 0.0, 0.0)] * 3, global_kw=_global_kw(32), **AO.VIEW_SETTINGS)
    fused = C.fuse(packed, res, voxel=0.005)
    rough = C.fuse(packed, [(np.eye(3)[None], np.zeros((1, 3)))] * 3, voxel=0.005)
    got, bad = fused.points.shape[0], rough.points.shape[0]
    for k in (1, 2):
        e0 = GO.pose_error(_np(res[k].start.R)[0], _np(res[k].start.t)[0], *truth[k], views[k])
        e1 = GO.pose_error(_np(res[k].R)[0], _np(res[k].t)[0], *truth[k], views[k])
        print(f"PIN view {k}: global {e0[0]:.3f} deg / {e0[1] * 100:.2f} cm ({res[k].start.inliers[0]} inliers of {res[k].start.correspondences[0]}), refined "
              f"{e1[0]:.4f} deg / {e1[1] * 1e3:.3f} mm, {res[k].matched[0]} matched, {res[k].steps[0]} steps")
        assert res[k].start.found[0] and res[k].status[0] == 0 and e0[0] <= 10.0 and e0[1] <= 0.05
        assert AO.angle_between(truth[k][0], np.eye(3)) > 90.0
    print(f"PIN occupied 5 mm cells: undisplaced union {want}, registered from nothing and fused {got}, as given {bad}")
    assert want == GO.VIEWS_UNION_CELLS and abs(got - want) <= GO.VIEWS_BOUND * want and bad > 1.3 * want
    # the operative assertion: VIEWS_BOUND (32.8 %) is the issue's rule and wide enough to pass a mirrored pose; 1 % of the oracle's own count under
    # the same key is not, and the 10 degree / 5 cm assertions on every view's start above are not either
    assert abs(got - GO.VIEWS_FUSED_CELLS[GO.FIXTURE_KEY]) <= 0.01 * GO.VIEWS_FUSED_CELLS[GO.FIXTURE_KEY]
    with pytest.raises(ValueError, match="one sensor position per view"):
        C.register_views(packed, init="global", keys=[1], viewpoints=[(0.0, 0.0, 0.0)])
    with pytest.raises(ValueError, match="needs keys"):
        C.register_views(packed, init="global", viewpoints=[(0.0, 0.0, 0.0)] * 3)


@pytest.fixture(scope="module")
def common(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    data = _train_data.build(tmp_path_factory.mktemp("global_data"), DEV)
    opt = types.SimpleNamespace(output_folder=os.path.join(data.root, "model"), EPN_input_radius=0.4, EPN_layer_num=2, markerset=K.default_markerset(),
                                device=torch.device(DEV))
    path = os.path.join(data.root, "model.pth")
    torch.save(load_seeded(GT_network_equiv(option=opt), 1).state_dict(), path)
    return ["--model_path", path, "--markerset_path", os.path.join(data.root, "markers.json"), "--num_point", "1024", "--synthetic_body", "--seed", "4"]


def _write_ply(path, p):
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\nend_header\n"
    path.write_bytes(head.encode() + p.astype("<f8").tobytes())


def test_the_command_registers_views_from_nothing_and_is_unchanged_without_the_flag(common, tmp_path):
    """The views 0 and 60 degrees, each in its camera's frame, the second turned by 150 degrees, under the command's defaults (2 cm voxels, k = 32,
    65 536 hypotheses, the key = --seed 4).  The oracle alone lands 1.36 degrees / 2.9 cm from the truth there on the CPU; with the third view
    (-60 degrees) it lands 7.9 degrees / 19 cm off on 2 cm voxels, outside the fixture condition, so the command's fixture has two views."""
    from etch_amd import cloud as C
    views, _, truth = _camera_views()
    views, truth = views[:2], truth[:2]
    for n, m in zip("ab", views):
        _write_ply(tmp_path / f"{n}.ply", m)
    base = ["--cloud_path", str(tmp_path / "a.ply"), "--more_views", str(tmp_path / "b.ply"), "--align_gate_min", "0.01", "--align_decay", "0.85",
            "--align_iters", "60", "--align_metric", "plane", "--fuse_voxel", "0.005"]
    out, given = tmp_path / "out", tmp_path / "given"
    C.main(base + ["--align_global", "--output_folder", str(out)] + common)
    rep = np.load(out / "a_cloud.npz")
    assert rep["view_global_found"].tolist() == [True, True] and rep["view_global_pose"].shape == (2, 4, 4) and rep["view_global_inliers"].shape == (2,)
    assert np.array_equal(rep["view_global_pose"][0], np.eye(4)) and (rep["view_global_inliers"][1:] >= 6).all() and not rep["view_status"].any()
    for k in (1,):
        e0 = GO.pose_error(rep["view_global_pose"][k, :3, :3], rep["view_global_pose"][k, :3, 3], *truth[k], views[k])
        e1 = GO.pose_error(rep["view_pose"][k, :3, :3], rep["view_pose"][k, :3, 3], *truth[k], views[k])
        print(f"PIN command view {k}: global {e0[0]:.3f} deg / {e0[1] * 100:.2f} cm, refined {e1[0]:.4f} deg / {e1[1] * 1e3:.3f} mm")
        assert e0[0] <= 10.0 and e0[1] <= 0.05 and e1[0] <= 1.0 and e1[1] <= 0.02
    poses = np.tile(np.eye(4), (1, 1, 1))                                                  # without the flag: what the command wrote before
    poses[0, :3, :3], poses[0, :3, 3] = truth[1]
    np.savez(tmp_path / "poses.npz", poses=poses)
    C.main(base + ["--view_init", str(tmp_path / "poses.npz"), "--output_folder", str(given)] + common)
    got = np.load(given / "a_cloud.npz")
    assert not [f for f in got.files if f.startswith("view_global")]
    packed = [C.pack([v], DEV) for v in views]
    res = C.register_views(packed, init=[None, poses[0:1]], gate=0.2, gate_min=0.01, decay=0.85, iters=60, metric="plane", normal_k=16)
    fused = C.fuse(packed, res, voxel=0.005)
    pose = np.tile(np.eye(4), (2, 1, 1))
    for k, r in enumerate(res):
        pose[k, :3, :3], pose[k, :3, 3] = _np(r.R)[0], _np(r.t)[0]
    p32, c, clean = C.prepare(C.pack([_np(fused.points)], DEV), 1024, [4])
    old = dict(keep=_np(clean.keep), center=_np(c[0]), points=_np(p32[0]), removed=np.int64(0), rows_output=np.array([fused.points.shape[0]]),
               rows_input=clean.stages["input"], view_pose=pose, view_matched=np.array([int(r.matched[0]) for r in res]),
               view_rms=np.array([float(r.rms[0]) for r in res]), view_steps=np.array([int(r.steps[0]) for r in res]),
               view_status=np.array([int(r.status[0]) for r in res]), view_metric=np.array("plane"))
    assert sorted(got.files) == sorted(old) and all(got[k].dtype == np.asarray(v).dtype and np.array_equal(got[k], v) for k, v in old.items())
    with pytest.raises(SystemExit):
        C.parse_args(base + ["--align_global", "--view_init", str(tmp_path / "poses.npz")] + common)
    with pytest.raises(SystemExit):
        C.parse_args(["--cloud_path", str(tmp_path / "a.ply"), "--align_global"] + common)
