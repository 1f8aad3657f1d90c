"""The definitions of DESIGN section 26 restated with numpy -- the checker of csrc/cloud_winding.hip and csrc/cloud_winding_solve.h, never the
product.  The area and the pack are float64 with one rounding per operation; the pair term runs in the dtype of its inputs: float32 inputs are the
kernel's own arithmetic (+, -, x, /, sqrt and a comparison, all correctly rounded by numpy as by the device, so the comparison is by bits), float64
inputs are the truth.  Sums that have an order are accumulated in that order.  The containment term against a cloud and the refinement with it are
tests/_containment_oracle.py's with the row target.  The fixtures of the tests are built here too."""
import functools

import numpy as np
import torch

import _chamfer_oracle as CH
import _cloud_oracle as CO
import _containment_oracle as CT
import _global_oracle as GO
import _surface_oracle as SO
from oracle import stage2 as S2

CHUNK = 1024                      # rows one thread adds in fp32 before the fp64 sum over the chunks
PI = 3.14159265358979323846
INV_4PI = 0.07957747154594767     # the double nearest to 1 / (4 pi)


# --------------------------------------------------------------------------------------------- area and pack
def kth_d2(p, k, chunk=256):
    """d2k (n) float64: the ke-th least d2 among the other rows, ke = min(k, n - 1); zeros for n = 1."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n = len(p)
    ke = min(int(k), n - 1)
    out = np.zeros(n)
    if ke <= 0:
        return out
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        d = CO.d2_rows(p, rows)
        d[np.arange(len(rows)), rows] = np.inf
        out[rows] = np.partition(d, ke - 1, axis=1)[:, ke - 1]
    return out


def areas(p, k, flag=None, d2k=None):
    """a (n) float64 = (pi d2k) / ke; 0 for n = 1, a flagged row and a row that is not finite."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n = len(p)
    ke = min(int(k), n - 1)
    if ke <= 0:
        return np.zeros(n)
    d2k = kth_d2(p, k) if d2k is None else np.asarray(d2k, np.float64)
    with np.errstate(all="ignore"):
        a = (PI * d2k) / float(ke)
    bad = ~np.isfinite(p).all(1)
    if flag is not None:
        bad |= np.asarray(flag) != 0
    return np.where(bad, 0.0, a)


def pack(p, normal, a, center=None):
    """-> pos (n,3), moment (n,3), cap (n) float32: fp32(p - c), fp32(a n), fp32(a / pi), each computed in float64 and rounded once."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    c = np.zeros(3) if center is None else np.asarray(center, np.float64)
    with np.errstate(all="ignore"):
        return ((p - c[None, :]).astype(np.float32), (a[:, None] * np.asarray(normal, np.float64)).astype(np.float32), (a / PI).astype(np.float32))


# --------------------------------------------------------------------------------------------- the sweep
def pair_terms(q, pos, moment, cap):
    """-> term (Q,R), d2 (Q,R) in the inputs' dtype: r = pos - q, d2 = (rx rx + ry ry) + rz rz, s = d2 where d2 > cap else cap,
    term = ((rx mx + ry my) + rz mz) / (s sqrt(s)); exactly 0 for a row with cap == 0."""
    dt = q.dtype
    assert pos.dtype == dt and moment.dtype == dt and cap.dtype == dt
    with np.errstate(all="ignore"):
        r = pos[None, :, :] - q[:, None, :]
        d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        s = np.where(d2 > cap[None, :], d2, cap[None, :])
        num = (r[..., 0] * moment[None, :, 0] + r[..., 1] * moment[None, :, 1]) + r[..., 2] * moment[None, :, 2]
        term = np.where(cap[None, :] == 0, dt.type(0), num / (s * np.sqrt(s)))
    assert term.dtype == dt and d2.dtype == dt
    return term, d2


def winding(pos, moment, cap, queries, block=256):
    """One cloud.  -> w (Q) in the inputs' dtype, nearest (Q) int32, nearest_d2 (Q): per 1024-row chunk a sequential sum from 0 in the dtype, the
    chunks in ascending order in float64, times 1 / (4 pi), one rounding.  nearest = the least (d2, row) among the rows with d2 < +inf (NaN and +inf
    never win), -1 and d2 0 where there is none."""
    dt = queries.dtype
    Q, R = len(queries), len(pos)
    w = np.zeros(Q, dt)
    nearest = np.full(Q, -1, np.int32)
    nd2 = np.zeros(Q, dt)
    for r0 in range(0, Q, block):
        q = queries[r0:r0 + block]
        s = np.zeros(len(q), np.float64)
        best = np.full(len(q), np.inf, dt)
        brow = np.full(len(q), -1, np.int64)
        for c0 in range(0, R, CHUNK):
            term, d2 = pair_terms(q, pos[c0:c0 + CHUNK], moment[c0:c0 + CHUNK], cap[c0:c0 + CHUNK])
            with np.errstate(all="ignore"):
                seq = np.cumsum(np.concatenate([np.zeros((len(q), 1), dt), term], 1), axis=1, dtype=dt)[:, -1]       # 0 + t0 + t1 + ..., in order
            s = s + seq.astype(np.float64)
            d = np.where(np.isnan(d2), dt.type(np.inf), d2)
            j = d.argmin(1)                                                                                         # the first minimum: the lowest row
            dj = d[np.arange(len(q)), j]
            better = dj < best                                                                                      # strict: an earlier chunk keeps a tie
            best, brow = np.where(better, dj, best), np.where(better, j + c0, brow)
        w[r0:r0 + block] = (s * INV_4PI).astype(dt)
        nearest[r0:r0 + block] = brow
        nd2[r0:r0 + block] = np.where(brow >= 0, best, dt.type(0))
    return w, nearest, nd2


def winding_batch(clouds, queries, lengths=None):
    """clouds: a list of (pos, moment, cap); queries (B,Q,3) -> w (B,Q), nearest (B,Q) int32, nearest_d2 (B,Q); padding gets 0, -1, 0."""
    B, Q = queries.shape[:2]
    w, nearest, nd2 = np.zeros((B, Q), queries.dtype), np.full((B, Q), -1, np.int32), np.zeros((B, Q), queries.dtype)
    for b, (pos, moment, cap) in enumerate(clouds):
        n = Q if lengths is None else int(lengths[b])
        dt = queries.dtype
        w[b, :n], nearest[b, :n], nd2[b, :n] = winding(pos.astype(dt), moment.astype(dt), cap.astype(dt), queries[b, :n])
    return w, nearest, nd2


def surface(p, normal, k=8, flag=None, center=None):
    """The oriented cloud of one cloud's rows: (pos, moment, cap) float32."""
    return pack(p, normal, areas(p, k, flag), center)


# --------------------------------------------------------------------------------------------- the containment term, the row target
def outside_and_target(pos, w, nearest):
    """w (V), nearest (V) -> o (V) bool, c (V,3) float64 = pos[nearest].  A NaN w and nearest -1 are not outside."""
    with np.errstate(invalid="ignore"):
        o = (np.abs(w) < 0.5) & (nearest >= 0)
    return o, np.asarray(pos, np.float64)[np.where(nearest >= 0, nearest, 0)] * (nearest >= 0)[:, None]


def metrics(cloud, body_verts):
    """containment_metrics for one oriented cloud (pos, moment, cap) and body_verts (V,3) in fp64 -> (outside_share, protrusion_rms_mm, max_mm)."""
    v = np.asarray(body_verts, np.float64)
    w, near, d2 = winding(*(a.astype(np.float64) for a in cloud), v)
    o = (np.abs(w) < 0.5) & (near >= 0)
    if not o.any():
        return 0.0, 0.0, 0.0
    return float(o.mean()), float(np.sqrt(d2[o].mean()) * 1e3), float(np.sqrt(d2[o].max()) * 1e3)


def fit_surface_contain_cloud(bm, pts, lengths, params0, iters, clouds, lr=2e-2, w_contain=1e2, contain_every=10, weights=None, markers=None, prior=None,
                              w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05, dtype=torch.float64):
    """tests/_containment_oracle.py fit_surface_contain with clouds[b] = (pos, moment, cap) in place of the scan meshes: at iterations 0, K, 2K, ...
    winding() of the current vertices IN `dtype` gives o_v and the row each outside vertex is pulled to; held in between.
    -> (trace (B, iters, 5), final params (B,P))."""
    nj, nb = bm.num_joints, bm.num_betas
    npd = np.float64 if dtype == torch.float64 else np.float32
    tb = S2.TorchBody(bm, dtype)
    faces = torch.from_numpy(np.asarray(bm.faces, np.int64))
    B = len(params0)
    P = torch.as_tensor(np.asarray(pts)).to(dtype)
    W = None if weights is None else torch.as_tensor(np.asarray(weights)).to(dtype)
    p = torch.nn.Parameter(torch.as_tensor(np.asarray(params0)).to(dtype).clone())
    pr = None if prior is None else tuple(torch.as_tensor(np.asarray(a)).to(dtype) for a in prior)
    mk = None
    if markers is not None:
        mk = (torch.as_tensor(np.asarray(markers[0], np.int64)), torch.as_tensor(np.asarray(markers[1])).to(dtype), torch.as_tensor(np.asarray(markers[2]) > 0))
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    ws = tuple(torch.tensor(x, dtype=dtype) for x in (w_dense, w_marker, w_beta, w_prior))
    wc = torch.tensor(w_contain, dtype=dtype)
    held = [None] * B
    trace = []
    for i in range(iters):
        for g in opt.param_groups:
            g["lr"] = CH.lr_at(i, iters, lr)
        verts, _ = CH.forward(tb, p, nj, nb)
        per = []
        for b in range(B):
            n = P.shape[1] if lengths is None else int(lengths[b])
            four = SO.scan_loss(verts[b], faces, P[b, :n], None if W is None else W[b, :n], trunc, None if mk is None else (mk[0], mk[1][b], mk[2][b]),
                                ws, p[b, 3 * nj:3 * nj + nb], p[b, 3:72], pr)
            if i % contain_every == 0:
                pos, moment, cap = (a.astype(npd) for a in clouds[b])
                w, near, _ = winding(pos, moment, cap, verts[b].detach().numpy().astype(npd))
                held[b] = outside_and_target(pos, w, near)
            per.append(torch.cat([four, (wc * CT.contain_sum(verts[b], *held[b]) / verts.shape[1])[None]]))
        per = torch.stack(per)
        trace.append(per.detach().clone())
        opt.zero_grad()
        per.sum().backward()
        p.grad[:, -1] = 0
        opt.step()
    return torch.stack(trace, 1).numpy(), p.detach().numpy()


# --------------------------------------------------------------------------------------------- fixtures
def fibonacci_sphere(n=2000, R=0.5):
    """n rows on the sphere of radius R about 0 by the Fibonacci spiral -> points (n,3), outward unit normals (n,3)."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = np.pi * (1.0 + 5.0 ** 0.5) * i
    r = np.sqrt(1.0 - z * z)
    nrm = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    nrm = nrm / np.sqrt((nrm * nrm).sum(1))[:, None]
    return np.ascontiguousarray(R * nrm), np.ascontiguousarray(nrm)


def sphere_queries(R, lo, hi, n, seed):
    """n queries with radius uniform in [lo R, hi R], direction uniform."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.sqrt((d * d).sum(1))[:, None]
    return d * (R * rng.uniform(lo, hi, n))[:, None]


BODY_AZIMUTHS = (0.0, 120.0, 240.0)
BODY_ROWS = 6721                                         # the de-duplicated union of the three views of the fixture body


def body_mesh():
    z = np.load(CO.GOLDEN)
    return CO.body_vertices(), z["faces"].astype(np.int64)


def orient(p, normal, sensor):
    """Flip where ((n_x w_x + n_y w_y) + n_z w_z) < 0 with w = sensor - p (sensor (3,) or per row (n,3)); float64."""
    w = np.broadcast_to(np.asarray(sensor, np.float64), p.shape) - p
    s = (normal[:, 0] * w[:, 0] + normal[:, 1] * w[:, 1]) + normal[:, 2] * w[:, 2]
    out = normal.copy()
    out[s < 0.0] = -out[s < 0.0]
    return out


@functools.lru_cache(maxsize=None)
def body_views(azimuths=BODY_AZIMUTHS, normal_k=16):
    """The fixture body as the cameras at `azimuths` see it (_global_oracle.view), de-duplicated: a vertex several views saw is kept once, with
    the first view that saw it.  Normals: tests/_normals_oracle.py's on the union, oriented towards that view's camera.
    -> points (n,3), normals (n,3), flags (n), sensors (n,3) per row, view id (n)."""
    import _normals_oracle as NO
    pts, cams, ids = [], [], []
    for k, az in enumerate(azimuths):
        p, cam = GO.view(az)
        pts.append(p), cams.append(np.broadcast_to(cam, p.shape)), ids.append(np.full(len(p), k))
    p, cam, vid = np.concatenate(pts), np.concatenate(cams), np.concatenate(ids)
    _, first = np.unique(p, axis=0, return_index=True)
    first = np.sort(first)
    p, cam, vid = np.ascontiguousarray(p[first]), np.ascontiguousarray(cam[first]), vid[first]
    nrm, _, flag, _, _ = NO.normals(p, normal_k, nbr=NO.neighbours_fast(p, normal_k) if len(p) > 4000 else None)
    return p, orient(p, nrm, cam), flag, cam, vid


def body_queries(n=600, push=0.01, seed=3):
    """n body vertices pushed +push (outside) and -push (inside) along the mesh's outward vertex normal -> outside (n,3), inside (n,3)."""
    v, f = body_mesh()
    vn = CT.vertex_normals(v, f)
    rows = np.random.default_rng(seed).choice(len(v), n, replace=False)
    return v[rows] + push * vn[rows], v[rows] - push * vn[rows]


# --------------------------------------------------------------------------------------------- scans that are samples of a mesh
def sample_mesh(v, f, n, seed):
    """n rows on the mesh (v, f): faces drawn by area, a uniform point on each, the face's unit normal (the faces' own orientation).
    -> points (n,3), normals (n,3) float64."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    rng = np.random.default_rng(seed)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    area = 0.5 * np.sqrt((fn * fn).sum(1))
    k = rng.choice(len(f), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(size=n)), rng.uniform(size=n)
    w = np.stack([1.0 - r1, r1 * (1.0 - r2), r1 * r2], 1)
    return (w[:, :, None] * v[f[k]]).sum(1), fn[k] / (2.0 * area[k])[:, None]


def sampled_scan(v, f, n, seed, k=8):
    """The oriented cloud (pos, moment, cap) float32 of n rows sampled on the mesh, with the points and the normals it was made from."""
    p, nrm = sample_mesh(v, f, n, seed)
    return surface(p, nrm, k), p, nrm


WHY_ROWS = 6000                   # rows per sampled scan of the scene: the oracle alone shows both metrics fall there (profiles/cloud_winding_pins.txt)


@functools.lru_cache(maxsize=None)
def why_clouds(rows=WHY_ROWS):
    """tests/_containment_oracle.py why_scene with each pushed scan replaced by a surface sample of it: -> bm, truth, pts, lengths, clouds."""
    bm, truth, pts, lengths, scans = CT.why_scene()
    return bm, truth, pts, lengths, [sampled_scan(v, f, rows, 40 + b)[0] for b, (v, f) in enumerate(scans)]


@functools.lru_cache(maxsize=None)
def trajectory_clouds(rows=3000):
    """tests/_containment_oracle.py trajectory_problem with each scan replaced by a sample of `rows` rows (three chunks): -> its tuple, the last
    entry the clouds."""
    prob = CT.trajectory_problem()
    return prob[:-1] + ([sampled_scan(v, f, rows, 50 + b)[0] for b, (v, f) in enumerate(prob[-1])],)
