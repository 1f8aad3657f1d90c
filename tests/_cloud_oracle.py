"""The definitions of DESIGN section 19 restated with numpy, brute force, for one cloud (n,3) float64 at a time -- the checker of
etch_amd.cloud, never the product.  Arithmetic is float64 with one rounding per operation (numpy's element-wise operations do not fuse)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")


def d2_rows(p, rows):
    """((dx dx + dy dy) + dz dz) from the given rows to every row: (len(rows), n)."""
    d = p[rows, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_mean(p, k, chunk=256):
    """m_i = (sum_j sqrt(s_j)) / k_eff over the k_eff = min(k, n - 1) smallest d2 to the OTHER rows, summed in ascending order; n = 1 -> 0."""
    p = np.asarray(p, np.float64)
    n = len(p)
    ke = min(int(k), n - 1)
    m = np.zeros(n)
    if ke <= 0:
        return m
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        d = d2_rows(p, rows)
        d[np.arange(len(rows)), rows] = np.inf               # only the row itself is excluded: coincident rows count, at distance 0
        s = np.sort(np.partition(d, ke - 1, axis=1)[:, :ke], axis=1)
        acc = np.zeros(len(rows))
        for j in range(ke):
            acc = acc + np.sqrt(s[:, j])
        m[rows] = acc / ke
    return m


def stat_keep(m, ratio):
    """-> keep, mu, s, the smallest relative distance of an m_i from the threshold."""
    m = np.asarray(m, np.float64)
    n = len(m)
    mu = m.sum() / n
    s = np.sqrt(((m - mu) ** 2).sum() / (n - 1)) if n >= 2 else 0.0
    thr = mu + ratio * s
    margin = float(np.abs(m - thr).min() / thr) if thr > 0 else np.inf
    return m <= thr, mu, s, margin


def radius_count(p, r, chunk=256):
    p = np.asarray(p, np.float64)
    n, r2 = len(p), float(r) * float(r)
    c = np.zeros(n, np.int32)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        c[rows] = (d2_rows(p, rows) <= r2).sum(1) - 1        # the row itself is at d2 = 0 <= r2
    return c


def compact(clouds, keeps):
    """-> points, index (the original row inside its cloud), offsets of the kept rows, in row order."""
    pts = [np.asarray(p)[np.asarray(k, bool)] for p, k in zip(clouds, keeps)]
    idx = [np.flatnonzero(np.asarray(k, bool)).astype(np.int32) for k in keeps]
    off = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int32)
    return np.concatenate(pts), np.concatenate(idx), off


def voxel_cells(p, voxel):
    p = np.asarray(p, np.float64)
    return np.floor((p - p.min(0)) / float(voxel)).astype(np.int64)


def voxel_grid(p, voxel):
    """-> cell (C,3), centroid (C,3) = (sum of the cell's rows in ascending row order) / count, count (C), lowest row (C); cells in ascending
    lexicographic (ix, iy, iz) order."""
    p = np.asarray(p, np.float64)
    cell = voxel_cells(p, voxel)
    order = np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))             # stable: rows of one cell stay in ascending order
    sc = cell[order]
    heads = np.flatnonzero(np.concatenate([[True], (sc[1:] != sc[:-1]).any(1)]))
    ends = np.concatenate([heads[1:], [len(p)]])
    cent, count, lowest = np.zeros((len(heads), 3)), np.zeros(len(heads), np.int32), np.zeros(len(heads), np.int32)
    for c, (a, e) in enumerate(zip(heads, ends)):
        rows = order[a:e]
        acc = p[rows[0]].copy()
        for r in rows[1:]:
            acc = acc + p[r]
        cent[c], count[c], lowest[c] = acc / (e - a), e - a, rows[0]
    return sc[heads], cent, count, lowest


def body_vertices():
    return np.load(GOLDEN)["vertices_q"].astype(np.int64) / 1e8


def stray_fixture(n_stray=140, seed=19):
    """The fixed fixture: the 6 890 body vertices and n_stray points further than 0.05 m from every vertex, drawn as c + 1.2 e uniform(-1, 1, 3)
    (c, e: the bounding-box centre and half-extent), then one permutation of all rows.  -> points (7030,3), is_stray (7030) bool."""
    v = body_vertices()
    c, e = (v.min(0) + v.max(0)) / 2.0, (v.max(0) - v.min(0)) / 2.0
    rng = np.random.default_rng(seed)
    stray = []
    while len(stray) < n_stray:
        q = c + 1.2 * e * rng.uniform(-1.0, 1.0, 3)
        if np.sqrt(((v - q) ** 2).sum(1)).min() > 0.05:
            stray.append(q)
    p = np.concatenate([v, np.array(stray)])
    is_stray = np.arange(len(p)) >= len(v)
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), is_stray[perm]
