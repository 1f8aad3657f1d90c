"""The definitions of DESIGN section 24 restated with numpy, brute force, for one cloud (n,3) float64 at a time -- the checker of
etch_amd.cloud.normals, never the product.  Arithmetic is float64 with one rounding per operation (numpy's element-wise operations do not
fuse); every sum is accumulated in an explicit loop, in the order the definition names."""
import numpy as np

from _cloud_oracle import d2_rows

FLAG_FEW, FLAG_AMBIGUOUS = 1, 2
GAP_EPS = 1e-9
JACOBI_SWEEPS = 10
U = 2.0 ** -53


def neighbours(p, k, chunk=512):
    """-> (n, ke) int64: for every row the ke = min(k, n - 1) least (d2, row) pairs among the OTHER rows, in ascending (d2, row) order."""
    p = np.asarray(p, np.float64)
    n = len(p)
    ke = max(min(int(k), n - 1), 0)
    out = np.zeros((n, ke), np.int64)
    if ke == 0:
        return out
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        d = d2_rows(p, rows)
        d[np.arange(len(rows)), rows] = np.inf
        thr = np.partition(d, ke - 1, axis=1)[:, ke - 1]
        for r in range(len(rows)):
            cand = np.flatnonzero(d[r] <= thr[r])                     # every row tied with the ke-th is a candidate
            out[rows[r]] = cand[np.lexsort((cand, d[r, cand]))][:ke]  # by d2, then by row
    return out


def neighbours_fast(p, k, extra=16):
    """neighbours() through a cKDTree for clouds too large for the brute scan: the k + extra nearest candidates, measured with the definition's
    d2 and ordered by (d2, row).  Exact as long as the last candidate lies strictly beyond the k-th, which is asserted."""
    from scipy.spatial import cKDTree
    p = np.asarray(p, np.float64)
    n = len(p)
    ke = max(min(int(k), n - 1), 0)
    kc = min(ke + extra + 1, n)
    cand = cKDTree(p).query(p, k=kc)[1].reshape(n, kc)
    d = p[cand] - p[:, None, :]
    d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d[cand == np.arange(n)[:, None]] = np.inf
    order = np.lexsort((cand, d), axis=1)
    cand, d = np.take_along_axis(cand, order, 1), np.take_along_axis(d, order, 1)
    assert kc == n or (d[:, kc - 2] > d[:, ke - 1]).all(), "a tie reaches the end of the candidates: raise extra"
    return cand[:, :ke].astype(np.int64)


def covariance(p, nbr):
    """cov (n,6) = xx, xy, xz, yy, yz, zz from the neighbour lists: e = q - p in list order, s and S summed sequentially from 0, w = ke + 1,
    mu = s / w, C_ab = S_ab / w - mu_a mu_b."""
    p = np.asarray(p, np.float64)
    n, ke = nbr.shape
    s = np.zeros((n, 3))
    S = np.zeros((n, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(ke):
        e = p[nbr[:, j]] - p
        s = s + e
        for c, (a, b) in enumerate(pairs):
            S[:, c] = S[:, c] + e[:, a] * e[:, b]
    w = float(ke + 1)
    mu = s / w
    cov = np.zeros((n, 6))
    for c, (a, b) in enumerate(pairs):
        cov[:, c] = S[:, c] / w - mu[:, a] * mu[:, b]
    return cov


def _rotate(a, v, P, Q):
    """The Jacobi rotation of cloud_normal_solve.h on stacks a, v (n,3,3), in place; a row whose a[P][Q] is 0 is left alone."""
    apq = a[:, P, Q].copy()
    on = apq != 0.0
    safe = np.where(on, apq, 1.0)
    with np.errstate(all="ignore"):
        theta = (a[:, Q, Q] - a[:, P, P]) / (2.0 * safe)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
    K = 3 - P - Q
    app, aqq = a[:, P, P] - t * apq, a[:, Q, Q] + t * apq
    akp, akq = a[:, K, P].copy(), a[:, K, Q].copy()
    nkp, nkq = c * akp - s * akq, s * akp + c * akq
    a[:, P, P] = np.where(on, app, a[:, P, P])
    a[:, Q, Q] = np.where(on, aqq, a[:, Q, Q])
    a[:, P, Q] = a[:, Q, P] = 0.0                                      # already 0 where the rotation is skipped
    a[:, K, P] = a[:, P, K] = np.where(on, nkp, akp)
    a[:, K, Q] = a[:, Q, K] = np.where(on, nkq, akq)
    for k in range(3):
        vp, vq = v[:, k, P].copy(), v[:, k, Q].copy()
        v[:, k, P] = np.where(on, c * vp - s * vq, vp)
        v[:, k, Q] = np.where(on, s * vp + c * vq, vq)


def solve(cov, ke, points=None, viewpoint=None):
    """cov (n,6) -> lam (n,3) ascending, normal (n,3), variation (n), flag (n) int32 by cyclic Jacobi (pairs (0,1), (0,2), (1,2), at most
    JACOBI_SWEEPS sweeps) and the flag and sign rules of the definition."""
    cov = np.asarray(cov, np.float64)
    n = len(cov)
    a = np.zeros((n, 3, 3))
    for c, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        a[:, i, j] = a[:, j, i] = cov[:, c]
    v = np.tile(np.eye(3), (n, 1, 1))
    for _ in range(JACOBI_SWEEPS):
        if not (a[:, 0, 1] != 0).any() and not (a[:, 0, 2] != 0).any() and not (a[:, 1, 2] != 0).any():
            break
        _rotate(a, v, 0, 1), _rotate(a, v, 0, 2), _rotate(a, v, 1, 2)        # a row that is diagonal already skips all three
    e = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    low = np.zeros(n, np.int64)                                            # the first minimum: a tie to the lowest column, a NaN never wins
    with np.errstate(all="ignore"):
        low[e[:, 1] < e[:, 0]] = 1
        low[e[:, 2] < e[np.arange(n), low]] = 2
    rest = np.array([[1, 2], [0, 2], [0, 1]])[low]
    ra, rb = e[np.arange(n), rest[:, 0]], e[np.arange(n), rest[:, 1]]
    l0, l1, l2 = e[np.arange(n), low], np.where(ra < rb, ra, rb), np.where(ra < rb, rb, ra)
    tr = (l0 + l1) + l2
    with np.errstate(all="ignore"):
        variation = np.where(tr > 0.0, l0 / np.where(tr > 0.0, tr, 1.0), 0.0)
        flag = np.where(l1 - l0 > GAP_EPS * l2, 0, FLAG_AMBIGUOUS).astype(np.int32)
    if ke < 2:
        flag |= FLAG_FEW
    x, y, z = (v[np.arange(n), r, low] for r in range(3))
    length = np.sqrt((x * x + y * y) + z * z)
    flag[~((length > 0.0) & np.isfinite(length))] |= FLAG_AMBIGUOUS
    ok = flag == 0
    nrm = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        nrm[ok] = np.stack([x / length, y / length, z / length], 1)[ok]
    ax = np.abs(nrm)
    lead = np.where((ax[:, 0] >= ax[:, 1]) & (ax[:, 0] >= ax[:, 2]), nrm[:, 0], np.where(ax[:, 1] >= ax[:, 2], nrm[:, 1], nrm[:, 2]))
    nrm[lead < 0.0] = -nrm[lead < 0.0]
    if viewpoint is not None:
        w = np.asarray(viewpoint, np.float64)[None, :] - np.asarray(points, np.float64)
        s = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2]
        nrm[s < 0.0] = -nrm[s < 0.0]
    nrm[~ok] = 0.0
    return np.stack([l0, l1, l2], 1), nrm, variation, flag


def normals(p, k, viewpoint=None, nbr=None):
    """-> normal (n,3), variation (n), flag (n), cov (n,6), neighbour lists (n, ke) of one cloud."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if nbr is None:
        nbr = neighbours(p, k)
    else:
        nbr = nbr[:, :max(min(int(k), len(p) - 1), 0)]                      # a prefix of a longer list is the shorter list
    cov = covariance(p, nbr)
    _, nrm, variation, flag = solve(cov, nbr.shape[1], p, viewpoint)
    return nrm, variation, flag, cov, nbr


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
def lattice(nx, ny, nz, scale=2.0 ** -4):
    """An nx x ny x nz integer lattice times a power of two, row = (ix ny + iy) nz + iz: every d2 and every moment is exact, ties everywhere."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(g.astype(np.float64) * scale)


def collinear(n=9):
    return np.ascontiguousarray(np.arange(n, dtype=np.float64)[:, None] * np.array([0.25, 0.25, 0.0])[None, :] + np.array([1.0, -2.0, 0.5]))


def sphere(n, seed=5):
    """n points on the unit sphere, a Fibonacci spiral turned by a fixed random rotation (near-uniform spacing h ~ sqrt(4 pi / n))."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = np.pi * (1.0 + 5.0 ** 0.5) * i
    r = np.sqrt(1.0 - z * z)
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    p = p @ q.T
    return np.ascontiguousarray(p / np.sqrt((p * p).sum(1))[:, None])


def eigh_reference(cov):
    """numpy's eigh on the same covariances: lam (n,3) ascending and the eigenvector of the smallest (n,3) -- the second method."""
    cov = np.asarray(cov, np.float64)
    a = np.zeros((len(cov), 3, 3))
    for c, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        a[:, i, j] = a[:, j, i] = cov[:, c]
    lam, vec = np.linalg.eigh(a)
    return lam, vec[:, :, 0], a
