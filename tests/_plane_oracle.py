"""The point-to-plane step and loop of DESIGN section 24 restated with numpy for one pair of clouds at a time -- the checker of
etch_amd.cloud.align(metric="plane"), never the product.  Arithmetic is float64 with one rounding per operation; the 6 x 6 system is solved by
numpy's LU `solve`, a second method beside the product's LDL^T."""
import math
import os

import numpy as np

import _align_oracle as AO
import _cloud_oracle as CO
import _normals_oracle as NO

DEGENERATE = AO.DEGENERATE
PLANE_EPS = 1e-9
TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def plane_terms(p, q, nq, pair, R, t):
    """The 32 columns of terms the sums add, one row per matched row (pair >= 0 and a non-zero target normal): J J^T upper triangle (21), J r (6),
    r^2, d2, x' (3).  -> terms (m,32), the centre c, rho = |c - box minimum|."""
    p, q, nq = (np.asarray(a, np.float64).reshape(-1, 3) for a in (p, q, nq))
    pair = np.asarray(pair)
    c = AO.center_of(q)
    o = q.min(0) if len(q) else np.zeros(3)
    e = c - o
    rho = float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))
    rows = np.flatnonzero(pair >= 0)
    rows = rows[(nq[pair[rows]] != 0.0).any(1)]
    x = AO.apply(R, t, p[rows])
    qq, n = q[pair[rows]], nq[pair[rows]]
    xc, d = x - c, x - qq
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    a = np.stack([xc[:, 1] * n[:, 2] - xc[:, 2] * n[:, 1], xc[:, 2] * n[:, 0] - xc[:, 0] * n[:, 2], xc[:, 0] * n[:, 1] - xc[:, 1] * n[:, 0]], 1)
    J = np.concatenate([a, n], 1)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    cols = [J[:, i] * J[:, j] for i, j in TRI] + [J[:, i] * r for i in range(6)] + [r * r, d2, xc[:, 0], xc[:, 1], xc[:, 2]]
    return np.stack(cols, 1) if len(rows) else np.zeros((0, 32)), c, rho


def plane_sums(terms, exact=True):
    if exact:
        return np.array([math.fsum(terms[:, k]) for k in range(32)]), np.abs(terms).sum(0)
    return terms.sum(0), np.abs(terms).sum(0)


def scaled_system(m, sums, rho):
    """Abar (6,6), gbar (6) and the scaling D."""
    A = np.zeros((6, 6))
    for e, (i, j) in enumerate(TRI):
        A[i, j] = A[j, i] = sums[e]
    D = np.array([1.0 / rho] * 3 + [1.0] * 3)
    return (A / m) * D[:, None] * D[None, :], (sums[21:27] / m) * D, D


def pivots(Abar):
    """The pivots of LDL^T in the order 0 .. 5 without pivoting; None from the first one that fails the test on."""
    top = Abar.diagonal().max()
    L, d = np.eye(6), np.zeros(6)
    for j in range(6):
        dj = Abar[j, j] - sum(L[j, k] * L[j, k] * d[k] for k in range(j))
        if not (dj > PLANE_EPS * top and dj > 0.0):
            return None
        d[j] = dj
        for i in range(j + 1, 6):
            L[i, j] = (Abar[i, j] - sum(L[i, k] * L[j, k] * d[k] for k in range(j))) / dj
    return d


def quat_rotation(w):
    th = float(np.sqrt((w * w).sum()))
    if th == 0.0:
        return np.eye(3)
    return AO.rotation(w / th, math.degrees(th))


def solve(m, sums, c, rho):
    """-> dR, dt, ok, y (6), angle, shift, the condition number of the scaled matrix."""
    bad = (np.eye(3), np.zeros(3), False, np.zeros(6), 0.0, 0.0, np.inf)
    if m < 6 or not (rho > 0.0 and math.isfinite(rho)):
        return bad
    with np.errstate(all="ignore"):
        Abar, gbar, D = scaled_system(m, sums, rho)
        if not np.isfinite(Abar).all() or pivots(Abar) is None:
            return bad
        z = np.linalg.solve(Abar, -gbar)
    y = z * D
    dR = quat_rotation(y[:3])
    dt = c - dR @ c + y[3:]
    mx = sums[29:32] / m
    return dR, dt, True, y, float(np.sqrt((y[:3] ** 2).sum())), float(np.sqrt((((dR - np.eye(3)) @ mx + y[3:]) ** 2).sum())), float(np.linalg.cond(Abar))


def step(p, q, nq, pair, R, t, exact=True):
    """One point-to-plane step from given pairs.  -> a dict like _align_oracle.step's, with y and cond."""
    terms, c, rho = plane_terms(p, q, nq, pair, R, t)
    m = len(terms)
    sums, abs_sums = plane_sums(terms, exact)
    dR, dt, ok, y, angle, shift, cond = solve(m, sums, c, rho)
    out = dict(dR=dR, dt=dt, m=m, sums=sums, abs_sums=abs_sums, ok=ok, R=R, t=t, y=y, angle=angle, shift=shift, cond=cond, rho=rho,
               rms=math.sqrt(sums[28] / m) if m else math.inf)
    if ok:
        out["R"], out["t"] = dR @ R, dR @ t + dt
    return out


def align(p, q, nq, gate=0.2, gate_min=0.02, decay=0.9, iters=40, tol_angle=1e-9, tol_shift=1e-9, R=None, t=None, metric="plane", history=None):
    """The loop of either metric (metric="point": _align_oracle's step).  history: a list that receives (R, t) after every step."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    try:
        from scipy.spatial import cKDTree
        tree = cKDTree(q) if len(q) else None
    except ImportError:
        tree = None
    out = dict(R=R, t=t, pair=np.full(len(p), -1, np.int32), d2=np.full(len(p), np.inf), matched=0, rms=math.inf, steps=0, status=0, cond=1.0)
    for g in AO.gates(gate, gate_min, decay, iters):
        pair, d2 = AO.nearest(p, q, g, R, t, tree=tree)
        s = step(p, q, nq, pair, R, t, exact=False) if metric == "plane" else AO.step(p, q, pair, R, t, exact=False)
        out.update(pair=pair, d2=d2, matched=s["m"], rms=s["rms"], steps=out["steps"] + 1)
        if not s["ok"]:
            out["status"] |= DEGENERATE
            break
        R, t = s["R"], s["t"]
        out.update(R=R, t=t, cond=max(out["cond"], s.get("cond", 1.0)))
        if history is not None:
            history.append((R, t))
        if s["angle"] < tol_angle and s["shift"] < tol_shift:
            break
    return out


# ---- the sampled-body fixture ------------------------------------------------------------------------------------------------------------------------
def body_mesh():
    z = np.load(CO.GOLDEN)
    return z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)


def sample_surface(v, f, n, seed):
    """n area-weighted samples of the mesh: the triangle by its area, the point uniform inside it."""
    rng = np.random.default_rng(seed)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(1))
    tri = rng.choice(len(f), size=n, p=area / area.sum())
    u, w = rng.uniform(size=n), rng.uniform(size=n)
    flip = u + w > 1.0
    u[flip], w[flip] = 1.0 - u[flip], 1.0 - w[flip]
    return np.ascontiguousarray(a[tri] + u[:, None] * (b[tri] - a[tri]) + w[:, None] * (c[tri] - a[tri]))


SAMPLED_SEEDS = (101, 202)
SAMPLED_ROWS = (4000, 12000)


def sampled_case():
    """Two different samplings of the body's surface.  -> source (4000,3), target (12000,3)."""
    v, f = body_mesh()
    return sample_surface(v, f, SAMPLED_ROWS[0], SAMPLED_SEEDS[0]), sample_surface(v, f, SAMPLED_ROWS[1], SAMPLED_SEEDS[1])


def row_error(p, R, t, R0, t0):
    """The largest distance of a source row from where the truth puts it."""
    d = AO.apply(R, t, p) - AO.apply(R0, t0, p)
    return float(np.sqrt((d * d).sum(1)).max())
