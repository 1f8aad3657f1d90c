"""The definitions of DESIGN section 25 restated with numpy, brute force, for one cloud or one pair of clouds at a time -- the checker of
etch_amd.cloud's global registration, never the product.  Arithmetic is float64 with one rounding per operation (numpy's element-wise operations
do not fuse), every sum is accumulated in an explicit loop in the order the definition names; the rigid step is an SVD Kabsch, a second method
beside the product's quaternion."""
import math

import numpy as np

import _align_oracle as AO
import _cloud_oracle as CO
import _normals_oracle as NO
from _sampler_oracle import philox4x32_10

BINS, FEATURES = 11, 33
EDGE = 1e-9                                  # a feature this close to a bin edge, in its own units, may fall on either side
WIDTH = (2.0 * np.pi / BINS, 2.0 / BINS, 2.0 / BINS)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def d2_pairs(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ---- the view fixture ---------------------------------------------------------------------------------------------------------------------------
def view(az, cosine=0.1, distance=3.0):
    """The vertices of the fixture body a camera sees: those whose area-weighted outward vertex normal has cosine > 0.1 with the direction to a
    camera that stands 3 m from the vertex mean at azimuth `az` degrees about the y axis.  -> points (n,3), the camera (3) = the viewpoint."""
    z = np.load(CO.GOLDEN)
    v, f = CO.body_vertices(), z["faces"].astype(np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])           # twice the area times the unit normal
    vn = np.zeros_like(v)
    for c in range(3):
        np.add.at(vn, f[:, c], fn)
    vn = vn / np.sqrt((vn * vn).sum(1))[:, None]
    a = math.radians(az)
    cam = v.mean(0) + distance * np.array([math.sin(a), 0.0, math.cos(a)])
    to = cam[None, :] - v
    to = to / np.sqrt((to * to).sum(1))[:, None]
    return np.ascontiguousarray(v[(vn * to).sum(1) > cosine]), cam


def moved(p, cam, degrees, shift, axis=(0.3, 1.0, 0.2)):
    """A view carried into a frame of its own: rows R0^T (p - t0), so that (R0, t0) brings it back.  -> points, viewpoint, R0, t0."""
    R0, t0 = AO.rotation(axis, degrees), np.asarray(shift, np.float64)
    return np.ascontiguousarray((np.asarray(p) - t0) @ R0), (np.asarray(cam) - t0) @ R0, R0, t0


FIXTURES = {"60": dict(az=(0.0, 60.0), k=32, shift=(0.3, 0.9, 0.3)), "90": dict(az=(0.0, 90.0), k=16, shift=(0.6, -0.3, 0.8))}
FIXTURE_KEY, FIXTURE_H, FIXTURE_TAU, FIXTURE_TURN = 7, 20000, 0.03, 150.0


def fixture(name):
    """-> source (moved away by 150 degrees and the fixture's shift), its viewpoint, target, its viewpoint, R0, t0 (the truth), k."""
    f = FIXTURES[name]
    tgt, vt = view(f["az"][0])
    src, vs = view(f["az"][1])
    src, vs, R0, t0 = moved(src, vs, FIXTURE_TURN, f["shift"])
    return src, vs, tgt, vt, R0, t0, f["k"]


def pose_error(R, t, R0, t0, p):
    """-> the angle between R and R0 in degrees, the worst distance between a row of p moved by (R, t) and by (R0, t0)."""
    d = AO.apply(R, t, p) - AO.apply(R0, t0, p)
    return AO.angle_between(R, R0), float(np.sqrt((d * d).sum(1)).max()) if len(p) else 0.0


# ---- descriptors ------------------------------------------------------------------------------------------------------------------------------------
def pad(nbr, k):
    """Neighbour lists (n, ke) -> (n, k) with -1 behind the ke-th, as the product writes them."""
    out = np.full((len(nbr), int(k)), -1, np.int64)
    out[:, :nbr.shape[1]] = nbr
    return out


def pair_features(p, nrm, flag, nbr, shift=0):
    """For every row i and every slot of its list nbr (n,k) (-1: empty): counted (n,k) bool, f (n,k,3) = theta, alpha, phi, bin (n,k,3) int,
    edge (n,k,3) bool = the feature lies within EDGE of a bin edge.  shift: a seeded defect, every bin moved by that much."""
    p, nrm = np.asarray(p, np.float64), np.asarray(nrm, np.float64)
    n, k = nbr.shape
    j = np.where(nbr >= 0, nbr, 0)
    pi, pj, ni, nj = p[:, None, :], p[j], np.broadcast_to(nrm[:, None, :], (n, k, 3)), nrm[j]
    d2 = d2_pairs(pi, pj)
    ok = (nbr >= 0) & (np.asarray(flag)[:, None] == 0) & (np.asarray(flag)[j] == 0) & (d2 > 0.0)
    with np.errstate(all="ignore"):
        d = (pj - pi) / np.sqrt(d2)[..., None]
        ai, aj = dot3(ni, d), dot3(nj, d)
        first = (np.abs(ai) >= np.abs(aj))[..., None]
        u, t, d = np.where(first, ni, nj), np.where(first, nj, ni), np.where(first, d, -d)
        c = cross3(d, u)
        cl2 = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
        ok &= cl2 > 0.0
        v = c / np.sqrt(cl2)[..., None]
        w = cross3(u, v)
        f = np.stack([np.arctan2(dot3(w, t), dot3(u, t)), dot3(v, t), dot3(u, d)], -1)
        x = np.stack([(11.0 * (f[..., 0] + np.pi)) / (2.0 * np.pi), (11.0 * (f[..., 1] + 1.0)) / 2.0, (11.0 * (f[..., 2] + 1.0)) / 2.0], -1)
        x = np.where(ok[..., None], x, 0.0)
        b = np.floor(x)
        b = np.where(b >= 0.0, b, 0.0)
        b = np.where(b > BINS - 1.0, BINS - 1.0, b).astype(np.int64)
        edge = ok[..., None] & (np.abs(x - np.round(x)) * np.array(WIDTH) <= EDGE)
    if shift:
        b = np.clip(b + shift, 0, BINS - 1)
    return ok, np.where(ok[..., None], f, 0.0), b, edge


def source_ties(p, nrm, flag, nbr):
    """(n,k) bool: the pairs whose two candidates for the source are tied, | |a_i| - |a_j| | <= EDGE (equal normals, for one).  The rule then
    decides by the last bit, and the other choice negates phi: such a pair is defined to the bit, but not steady under a motion of the cloud."""
    p, nrm = np.asarray(p, np.float64), np.asarray(nrm, np.float64)
    j = np.where(nbr >= 0, nbr, 0)
    with np.errstate(all="ignore"):
        d = (p[j] - p[:, None, :]) / np.sqrt(d2_pairs(p[:, None, :], p[j]))[..., None]
        return (nbr >= 0) & (np.abs(np.abs(dot3(nrm[:, None, :], d)) - np.abs(dot3(nrm[j], d))) <= EDGE)


def spfh(p, nrm, flag, nbr, shift=0):
    """Pass 1.  -> spfh (n,33) int32, c (n) int32, bin (n,k,3), edge (n,k,3), counted (n,k)."""
    ok, _, b, edge = pair_features(p, nrm, flag, nbr, shift)
    n, k = nbr.shape
    out = np.zeros((n, FEATURES), np.int32)
    rows = np.broadcast_to(np.arange(n)[:, None], (n, k))
    for blk in range(3):
        np.add.at(out, (rows[ok], BINS * blk + b[..., blk][ok]), 1)
    return out, ok.sum(1).astype(np.int32), b, edge, ok


def edge_rule(got, got_c, want, want_c, b, edge, counted):
    """The comparison of pass 1.  Rows without an edge pair must be equal exactly; a row with edge pairs may differ only by moving those pairs
    between adjacent bins.  -> the message of the first violation or None, the share of rows with an edge pair."""
    if not np.array_equal(got_c, want_c):
        return f"c differs in rows {np.flatnonzero(got_c != want_c)[:5]}", 0.0
    has = (edge & counted[..., None]).any((1, 2))
    diff = np.asarray(got, np.int64) - np.asarray(want, np.int64)
    bad = np.flatnonzero((diff != 0).any(1) & ~has)
    if len(bad):
        return f"rows without an edge pair differ: {bad[:5]}", float(has.mean()) if len(has) else 0.0
    for i in np.flatnonzero(has & (diff != 0).any(1)):
        for blk in range(3):
            dd = diff[i, BINS * blk:BINS * (blk + 1)]
            e = edge[i, :, blk] & counted[i]
            allowed = np.zeros(BINS, bool)
            for s in b[i, e, blk]:
                allowed[max(s - 1, 0):min(s + 2, BINS)] = True
            if dd[~allowed].any() or dd.sum() != 0 or np.abs(dd).sum() > 2 * int(e.sum()):
                return f"row {i}, block {blk}: {dd} with {int(e.sum())} edge pairs in bins {b[i, e, blk]}", float(has.mean())
    return None, float(has.mean()) if len(has) else 0.0


def fpfh(p, spf, c, nbr, flag):
    """Pass 2 from given counts and lists (n,k) (-1: empty).  -> F (n,33), has_feature (n) bool."""
    p, spf, c = np.asarray(p, np.float64), np.asarray(spf), np.asarray(c)
    n, k = nbr.shape
    F = np.zeros((n, FEATURES))
    for u in range(k):
        j = np.where(nbr[:, u] >= 0, nbr[:, u], 0)
        d2 = d2_pairs(p, p[j])
        use = (nbr[:, u] >= 0) & (c[j] > 0) & (d2 > 0.0)
        with np.errstate(all="ignore"):
            term = (1.0 / d2)[:, None] * ((100.0 * spf[j].astype(np.float64)) / c[j].astype(np.float64)[:, None])
        F = F + np.where(use[:, None], term, 0.0)
    ok = np.ones(n, bool)
    for blk in range(3):
        s = np.zeros(n)
        for f in range(BINS):
            s = s + F[:, BINS * blk + f]
        pos = s > 0.0
        ok &= pos
        with np.errstate(all="ignore"):
            F[:, BINS * blk:BINS * (blk + 1)] = np.where(pos[:, None], (100.0 * F[:, BINS * blk:BINS * (blk + 1)]) / s[:, None], 0.0)
    return F, (np.asarray(flag) == 0) & (c > 0) & ok


def features(p, k, viewpoint=None, normals=None, flags=None, nbr=None):
    """The whole descriptor of one cloud.  -> F (n,33), has (n) bool, spfh, c, lists (n,k), normals, flags."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if nbr is None:
        nbr = NO.neighbours(p, k)
    if normals is None:
        normals, _, flags, _, _ = NO.normals(p, k, viewpoint, nbr=nbr)
    lists = pad(nbr, k)
    s, c, _, _, _ = spfh(p, normals, flags, lists)
    F, has = fpfh(p, s, c, lists, flags)
    return F, has, s, c, lists, normals, flags


# ---- matching -----------------------------------------------------------------------------------------------------------------------------------------
def match(fs, hs, ft, ht, chunk=256, highest=False):
    """-> match (ns) int32, dist (ns): the target row with a feature and the least (D, row), D summed sequentially over f; -1 and inf without one.
    highest: a seeded defect, a tie goes to the higher row."""
    fs, ft = np.asarray(fs, np.float64).reshape(-1, FEATURES), np.asarray(ft, np.float64).reshape(-1, FEATURES)
    out, dist = np.full(len(fs), -1, np.int32), np.full(len(fs), np.inf)
    if len(ft) == 0 or not np.asarray(ht).any() or len(fs) == 0:
        return out, dist
    for a in range(0, len(fs), chunk):
        D = np.zeros((len(fs[a:a + chunk]), len(ft)))
        for f in range(FEATURES):
            e = fs[a:a + chunk, f][:, None] - ft[None, :, f]
            D = D + e * e
        D[:, ~np.asarray(ht, bool)] = np.inf
        j = (D.shape[1] - 1 - D[:, ::-1].argmin(1)) if highest else D.argmin(1)
        out[a:a + chunk], dist[a:a + chunk] = j, D[np.arange(len(j)), j]
    none = ~np.asarray(hs, bool) | ~np.isfinite(dist)
    out[none], dist[none] = -1, np.inf
    return out, dist


def correspondences(ps, pt, m):
    """-> a (n_c,3), b (n_c,3), the matched target rows (n_c), the source rows (n_c), in ascending source row order."""
    rows = np.flatnonzero(np.asarray(m) >= 0)
    return np.asarray(ps, np.float64)[rows], np.asarray(pt, np.float64)[np.asarray(m)[rows]], np.asarray(m)[rows].astype(np.int64), rows


# ---- hypotheses, scores, selection ----------------------------------------------------------------------------------------------------------------------
def hypothesis_rows(key, H, n, word=2):
    """The correspondences i0, i1, i2 of hypotheses 0 .. H-1: Philox counter (h, 2, 0, 0) under the uint64 key, i = (r n) >> 32.  (H,3) int64."""
    ctr = np.zeros((H, 4), np.uint32)
    ctr[:, 0] = np.arange(H, dtype=np.uint32)
    ctr[:, 1] = word
    r = philox4x32_10(ctr, (int(key) & 0xFFFFFFFF, int(key) >> 32))[:, :3].astype(np.uint64)
    return ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def triple_valid(a, b, brow, idx, e=0.9, min_edge=0.05):
    """The tests on a triple that need no solve: distinct correspondences, distinct target rows, similar and long enough edges.  (H) bool."""
    if len(a) < 3:
        return np.zeros(len(idx), bool)
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    ok = (i0 != i1) & (i0 != i2) & (i1 != i2)
    r = brow[idx]
    ok &= (r[:, 0] != r[:, 1]) & (r[:, 0] != r[:, 2]) & (r[:, 1] != r[:, 2])
    e2, m2 = float(e) * float(e), float(min_edge) * float(min_edge)
    for x, y in ((0, 1), (1, 2), (2, 0)):
        ls2, lt2 = d2_pairs(a[idx[:, x]], a[idx[:, y]]), d2_pairs(b[idx[:, x]], b[idx[:, y]])
        ok &= (ls2 >= e2 * lt2) & (lt2 >= e2 * ls2) & (ls2 >= m2)
    return ok


def kabsch_triples(a3, b3):
    """The least-squares rigid motion of stacks of three pairs by SVD.  a3, b3 (H,3,3) -> R (H,3,3), t (H,3), ok (H): the rank test of section 23."""
    ca, cb = a3.mean(1), b3.mean(1)
    C = np.einsum("hki,hkj->hij", a3 - ca[:, None, :], b3 - cb[:, None, :])
    U, S, Vt = np.linalg.svd(C)
    e = np.where(np.linalg.det(U) * np.linalg.det(Vt) >= 0.0, 1.0, -1.0)
    D = np.zeros_like(C)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = e
    R = np.swapaxes(Vt, 1, 2) @ D @ np.swapaxes(U, 1, 2)
    l1 = S[:, 0] + S[:, 1] + e * S[:, 2]
    ok = (l1 > 0.0) & (2.0 * (S[:, 1] + e * S[:, 2]) > AO.RANK_EPS * l1)
    return R, cb - np.einsum("hij,hj->hi", R, ca), ok


def hypotheses(a, b, brow, key, H, e=0.9, min_edge=0.05, word=2):
    """-> idx (H,3) int64, valid (H) int32, transforms (H,12) (the identity where invalid)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    idx = hypothesis_rows(key, H, len(a), word)
    ok = triple_valid(a, b, np.asarray(brow), idx, e, min_edge)
    T = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (H, 1))
    rows = np.flatnonzero(ok)
    if len(rows):
        R, t, good = kabsch_triples(a[idx[rows]], b[idx[rows]])
        ok[rows] = good
        T[rows[good], :9], T[rows[good], 9:] = R[good].reshape(-1, 9), t[good]
    return idx, ok.astype(np.int32), T


def score(a, b, T, tau, valid=None, chunk=256):
    """inliers (H) int32 = #{c : d2(R a_c + t, b_c) <= tau tau}, the transform applied as section 23 defines it; 0 where valid is 0."""
    a, b, T = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3), np.asarray(T, np.float64).reshape(-1, 12)
    out, t2 = np.zeros(len(T), np.int32), float(tau) * float(tau)
    for s in range(0, len(T), chunk):
        R, t = T[s:s + chunk, :9].reshape(-1, 3, 3), T[s:s + chunk, 9:]
        x = np.stack([((R[:, r, 0, None] * a[None, :, 0] + R[:, r, 1, None] * a[None, :, 1]) + R[:, r, 2, None] * a[None, :, 2]) + t[:, r, None] for r in range(3)], -1)
        out[s:s + chunk] = (d2_pairs(x, b[None, :, :]) <= t2).sum(1)
    if valid is not None:
        out[np.asarray(valid) == 0] = 0
    return out


def select(valid, counts, min_inliers=6):
    """-> h (-1 without one), found: the valid hypothesis with the most inliers, a tie to the lowest h."""
    ok = np.flatnonzero(np.asarray(valid) != 0)
    if len(ok) == 0:
        return -1, False
    h = int(ok[np.argmax(np.asarray(counts)[ok])])
    return (h, True) if counts[h] >= min_inliers else (-1, False)


def refit(a, b, R, t, tau, steps=2):
    """Up to `steps` least-squares steps on the inliers, each followed by a recount; the last pose whose count did not fall stays."""
    best = int(score(a, b, np.concatenate([R.reshape(9), t])[None], tau)[0])
    for _ in range(steps):
        x = AO.apply(R, t, a)
        pair = np.where(d2_pairs(x, b) <= tau * tau, np.arange(len(a)), -1)
        s = AO.step(a, b, pair, R, t, exact=False)
        if not s["ok"]:
            break
        c = int(score(a, b, np.concatenate([s["R"].reshape(9), s["t"]])[None], tau)[0])
        if c < best:
            break
        R, t, best = s["R"], s["t"], c
    return R, t, best


def global_align(ps, vs, pt, vt, key, k=32, H=20000, tau=0.03, e=0.9, min_edge=0.05, min_inliers=6, refit_steps=2, word=2):
    """The whole pipeline on one pair.  -> a dict: R, t, found, inliers, correspondences, match."""
    fs, hs = features(ps, k, vs)[:2]
    ft, ht = features(pt, k, vt)[:2]
    m, _ = match(fs, hs, ft, ht)
    a, b, brow, _ = correspondences(ps, pt, m)
    idx, valid, T = hypotheses(a, b, brow, key, H, e, min_edge, word)
    counts = score(a, b, T, tau, valid)
    h, found = select(valid, counts, min_inliers)
    R, t, n = np.eye(3), np.zeros(3), 0
    if found:
        R, t, n = refit(a, b, T[h, :9].reshape(3, 3), T[h, 9:], tau, refit_steps)
    return dict(R=R, t=t, found=found, inliers=n, correspondences=len(a), match=m, valid=valid, counts=counts)


# ---- several views ---------------------------------------------------------------------------------------------------------------------------------
# What this file's register_views reaches on the three camera-frame views of tests/test_gpu_cloud_global.py (azimuths 0, 60, -60, turned by 0, 150,
# -120 degrees; vertex copies, k = 32, 20 000 hypotheses, tau = 3 cm, section 23's partial-overlap settings), recorded from the CPU: the occupied
# 5 mm cells of the undisplaced union, and of the registered and fused views under three keys (key 9: the third view takes a mirrored pose).
VIEWS_UNION_CELLS = 5237
VIEWS_FUSED_CELLS = {7: 5630, 8: 5630, 9: 6957}
# the bound of the GPU test: what the oracle reaches under the fixture's key plus its spread over the three keys, as a share of the union's cells
VIEWS_BOUND = abs(VIEWS_FUSED_CELLS[7] - VIEWS_UNION_CELLS) / VIEWS_UNION_CELLS + (max(VIEWS_FUSED_CELLS.values()) - min(VIEWS_FUSED_CELLS.values())) / VIEWS_UNION_CELLS


def register_views(views, cams, key, k=32, H=FIXTURE_H, tau=FIXTURE_TAU, **icp):
    """The pipeline of register_views(init="global") on one subject: the descriptors of every view once in its own frame, view i matched against the
    rows of the views before it as placed, the pose by hypotheses, scores, selection and refit, then section 23's point-metric loop against the union.
    -> a list of (R, t), the list of the global poses."""
    feats = [features(v, k, c)[:2] for v, c in zip(views, cams)]
    placed, poses, starts = [np.asarray(views[0], np.float64)], [(np.eye(3), np.zeros(3))], [(np.eye(3), np.zeros(3))]
    for i in range(1, len(views)):
        union = np.concatenate(placed)
        ft, ht = np.concatenate([f for f, _ in feats[:i]]), np.concatenate([h for _, h in feats[:i]])
        m, _ = match(feats[i][0], feats[i][1], ft, ht)
        a, b, brow, _ = correspondences(views[i], union, m)
        _, valid, T = hypotheses(a, b, brow, key, H)
        counts = score(a, b, T, tau, valid)
        h, found = select(valid, counts)
        R, t = (refit(a, b, T[h, :9].reshape(3, 3), T[h, 9:], tau)[:2]) if found else (np.eye(3), np.zeros(3))
        starts.append((R, t))
        w = AO.align(views[i], union, R=R, t=t, **icp)
        poses.append((w["R"], w["t"]))
        placed.append(AO.apply(w["R"], w["t"], views[i]))
    return poses, starts
