"""The contract of DESIGN section 23 restated with numpy for one pair of clouds at a time -- the checker of etch_amd.cloud's registration, never
the product.  Arithmetic is float64 with one rounding per operation (numpy's element-wise operations do not fuse); the rigid step is an SVD
Kabsch, a second method beside the product's quaternion."""
import math

import numpy as np

import _cloud_oracle as CO

DEGENERATE = 8
RANK_EPS = 1e-9


def rotation(axis, degrees):
    """Rodrigues' matrix of a turn by `degrees` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    th = math.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def start_pose(degrees, shift):
    """The start poses of the issue's experiment: a turn about (0.3, 1, 0.2) and the shift (s, -s/2, s/3)."""
    return rotation([0.3, 1.0, 0.2], degrees), np.array([shift, -shift / 2.0, shift / 3.0])


def angle_between(Ra, Rb):
    """The angle of Ra Rb^T in degrees, from the skew part (exact for small angles) and the trace."""
    D = Ra @ Rb.T
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.degrees(math.atan2(s, 0.5 * (np.trace(D) - 1.0)))


def apply(R, t, p):
    """x = R p + t, per component ((R_r0 px + R_r1 py) + R_r2 pz) + t_r."""
    p = np.asarray(p, np.float64)
    return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)


def d2_cross(x, q):
    d = x[:, None, :] - q[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(p, q, gate, R=None, t=None, chunk=256, tree=None):
    """-> pair (n) int32, d2 (n): the row of q with the least d2 <= gate * gate from x = R p + t, a tie to the lowest row; -1 and inf without one.
    With tree (a cKDTree of q) only its 8 nearest candidates are measured -- the loop's shortcut, never used where bits are compared."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    x = p if R is None else apply(np.asarray(R, np.float64), np.asarray(t, np.float64), p)
    g2 = float(gate) * float(gate)
    pair, best = np.full(len(x), -1, np.int32), np.full(len(x), np.inf)
    if len(q) == 0 or len(x) == 0:
        return pair, best
    if tree is not None:
        k = min(8, len(q))
        cand = tree.query(x, k=k)[1].reshape(len(x), k)
        cand.sort(axis=1)                                       # ascending rows: argmin then takes the lowest row of a tie
        d = x[:, None, :] - q[cand]
        d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = d.argmin(1)
        best = d[np.arange(len(x)), j]
        pair = cand[np.arange(len(x)), j].astype(np.int32)
    else:
        for a in range(0, len(x), chunk):
            d = d2_cross(x[a:a + chunk], q)
            j = d.argmin(1)                                     # the first minimum: the lowest row
            best[a:a + chunk], pair[a:a + chunk] = d[np.arange(len(j)), j], j
    out = best > g2
    pair[out], best[out] = -1, np.inf
    return pair, best


def center_of(q):
    q = np.asarray(q, np.float64)
    return 0.5 * (q.min(0) + q.max(0)) if len(q) else np.zeros(3)


def moment_terms(p, q, pair, R, t):
    """The 16 columns of terms the moment sums add, one row per matched pair: x' (3), q' (3), x' q'^T (9), d2."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    c = center_of(q)
    rows = np.flatnonzero(np.asarray(pair) >= 0)
    x = apply(R, t, p[rows])
    qq = q[np.asarray(pair)[rows]]
    xc, qc = x - c, qq - c
    d = x - qq
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.concatenate([xc, qc, (xc[:, :, None] * qc[:, None, :]).reshape(len(rows), 9), d2[:, None]], 1), c


def moments(terms, exact=True):
    """-> sums (16) (math.fsum: the correctly rounded sum) and the sums of the absolute terms (16)."""
    if exact:
        return np.array([math.fsum(terms[:, k]) for k in range(16)]), np.abs(terms).sum(0)
    return terms.sum(0), np.abs(terms).sum(0)


def kabsch(m, sums, c):
    """-> dR, dt, ok, the singular values of the centred cross-covariance and its sign: dR = V diag(1, 1, det) U^T of C = U S V^T."""
    if m < 3:
        return np.eye(3), np.zeros(3), False, np.zeros(3), 1.0
    C = sums[6:15].reshape(3, 3) - np.outer(sums[0:3], sums[3:6]) / m
    U, S, Vt = np.linalg.svd(C)
    e = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    l1 = S[0] + S[1] + e * S[2]
    if not (l1 > 0.0 and 2.0 * (S[1] + e * S[2]) > RANK_EPS * l1):
        return np.eye(3), np.zeros(3), False, S, e
    dR = Vt.T @ np.diag([1.0, 1.0, e]) @ U.T
    mx, mq = sums[0:3] / m + c, sums[3:6] / m + c
    return dR, mq - dR @ mx, True, S, e


def step(p, q, pair, R, t, exact=True):
    """One rigid step from given pairs.  -> a dict: dR, dt, m, sums, abs_sums, ok, R, t (composed; unchanged when not ok), S, angle (radians), shift."""
    terms, c = moment_terms(p, q, pair, R, t)
    m = len(terms)
    sums, abs_sums = moments(terms, exact)
    dR, dt, ok, S, e = kabsch(m, sums, c)
    out = dict(dR=dR, dt=dt, m=m, sums=sums, abs_sums=abs_sums, ok=ok, R=R, t=t, S=S, sign=e, angle=0.0, shift=0.0,
               rms=math.sqrt(sums[15] / m) if m else math.inf)
    if ok:
        out["R"], out["t"] = dR @ R, dR @ t + dt
        out["angle"] = math.radians(angle_between(dR, np.eye(3)))
        out["shift"] = float(np.sqrt((((sums[3:6] - sums[0:3]) / m) ** 2).sum()))
    return out


def gates(gate, gate_min, decay, iters):
    return [max(float(gate_min), float(gate) * float(decay) ** k) for k in range(int(iters))]


def align(p, q, gate=0.2, gate_min=0.02, decay=0.9, iters=40, tol_angle=1e-9, tol_shift=1e-9, R=None, t=None):
    """The loop.  -> a dict: R, t, pair, d2, matched, rms, steps, status."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    try:
        from scipy.spatial import cKDTree
        tree = cKDTree(q) if len(q) else None
    except ImportError:
        tree = None
    out = dict(R=R, t=t, pair=np.full(len(p), -1, np.int32), d2=np.full(len(p), np.inf), matched=0, rms=math.inf, steps=0, status=0)
    for g in gates(gate, gate_min, decay, iters):
        pair, d2 = nearest(p, q, g, R, t, tree=tree)
        s = step(p, q, pair, R, t, exact=False)
        out.update(pair=pair, d2=d2, matched=s["m"], rms=s["rms"], steps=out["steps"] + 1)
        if not s["ok"]:
            out["status"] |= DEGENERATE
            break
        R, t = s["R"], s["t"]
        out.update(R=R, t=t)
        if s["angle"] < tol_angle and s["shift"] < tol_shift:
            break
    return out


def exact_copy_case():
    """Target: the 6 890 body vertices; source: every other vertex.  -> source (3445,3), target (6890,3)."""
    v = CO.body_vertices()
    return np.ascontiguousarray(v[::2]), v


def partial_case():
    """Target: the vertices with z > -0.02; source: those with x > -0.05.  -> source, target."""
    v = CO.body_vertices()
    return np.ascontiguousarray(v[v[:, 0] > -0.05]), np.ascontiguousarray(v[v[:, 2] > -0.02])


def displaced(p, degrees, shift):
    """-> the source moved away by the start pose's inverse (so that R0, t0 = the start pose is the truth), R0, t0."""
    R0, t0 = start_pose(degrees, shift)
    return np.ascontiguousarray((np.asarray(p) - t0) @ R0), R0, t0              # rows R0^T (p - t0)


def three_views():
    """Three synthetic views of the body: front, left and right half-spaces that overlap.  -> [view0, view1, view2], each (n,3)."""
    v = CO.body_vertices()
    return [np.ascontiguousarray(v[v[:, 2] > -0.03]), np.ascontiguousarray(v[v[:, 0] > -0.06]), np.ascontiguousarray(v[v[:, 0] < 0.06])]


VIEW_POSES = ((0.0, 0.0), (8.0, 0.04), (-6.0, -0.03))          # degrees, metres: view 0 fixes the frame
# the partial-overlap settings: with the default smallest gate of 2 cm the rows a view shares with no other pull the pose off by up to 1 mm
VIEW_SETTINGS = dict(gate=0.2, gate_min=0.01, decay=0.85, iters=60)


def occupied(p, voxel):
    """The number of occupied cells of a voxel grid whose origin is the cloud's bounding-box minimum."""
    return len(np.unique(CO.voxel_cells(p, voxel), axis=0))
