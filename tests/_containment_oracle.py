"""CPU restatement of the containment kernels (csrc/containment.hip, etch_amd/containment.py) -- TEST INFRASTRUCTURE ONLY.

(1) The winding number in numpy, in the dtype of its inputs, with the operation order of the kernel (van Oosterom-Strackee): float64 inputs
are the truth, float32 inputs the entitled error (numpy's arctan2 is not the device's atan2f, so the comparison is by the rule of
tests/_pt_fp64.py, not bitwise).  (2) The ragged closest point: tests/_surface_oracle.py's, per scan.  (3) The containment term and the
refinement with it as a fifth term in torch, written from the contract.  Imports _surface_oracle and changes nothing in it.  The test
meshes (icosphere, holed, reversed) and the scene of the issue are built here too, so the host test can assert their conditions."""
import functools

import numpy as np
import torch

import _chamfer_oracle as CO
import _surface_oracle as SO
from oracle import stage2 as S2

CHUNK = 1024                      # PM_CHUNK of csrc/surface_common.h: the faces one thread adds in fp32 before the fp64 sum over the chunks


# --------------------------------------------------------------------------------------------- winding number
def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def half_angles(q, a, b, c):
    """Omega / 2 of triangles (a, b, c) (F,3) seen from q (Q,3) -> (Q,F), every operation one rounding in the inputs' dtype:
        A = a - q, B = b - q, C = c - q;  la = sqrt(dot(A, A)), lb, lc;  n = B x C;  det = dot(A, n)
        den = (((la*lb)*lc + dot(A, B)*lc) + dot(B, C)*la) + dot(C, A)*lb;   Omega / 2 = atan2(det, den) + ((la + lb) + lc) * 0
    (the last term: 0, or NaN where a corner or the query is not finite)"""
    dt = q.dtype
    assert a.dtype == dt and b.dtype == dt and c.dtype == dt
    with np.errstate(all="ignore"):
        A, B, C = a[None] - q[:, None], b[None] - q[:, None], c[None] - q[:, None]
        la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
        n = np.stack([B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1], B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2],
                      B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]], -1)
        det = _dot(A, n)
        den = (((la * lb) * lc + _dot(A, B) * lc) + _dot(B, C) * la) + _dot(C, A) * lb
        out = np.arctan2(det, den) + ((la + lb) + lc) * dt.type(0)
    assert out.dtype == dt
    return out


def winding_number(verts, faces, queries, block=256):
    """verts (V,3), queries (Q,3) of one dtype, faces (F,3) -> w (Q) in that dtype: per 1024-face chunk a sequential sum in the dtype
    (np.cumsum adds in order), the chunks in ascending order in float64, times 1 / (2 pi), one rounding.  A face with an index outside
    [0, V) contributes 0 (it is staged as the triangle (0, 0, 0), whose term is +-0)."""
    dt = queries.dtype
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(verts))).all(1)
    tri = np.where(ok[:, None, None], verts[np.clip(f, 0, len(verts) - 1)], dt.type(0)).astype(dt)
    out = np.zeros(len(queries), dt)
    for r0 in range(0, len(queries), block):
        q = queries[r0:r0 + block]
        s = np.zeros(len(q), np.float64)
        for c0 in range(0, len(f), CHUNK):
            t = tri[c0:c0 + CHUNK]
            s = s + np.cumsum(half_angles(q, t[:, 0], t[:, 1], t[:, 2]), axis=1, dtype=dt)[:, -1].astype(np.float64)
        out[r0:r0 + block] = (s * 0.15915494309189533577).astype(dt)
    return out


def winding_batch(meshes, queries, lengths=None):
    """meshes: a list of (verts, faces); queries (B,Q,3) -> w (B,Q); padding gets 0."""
    B, Q = queries.shape[:2]
    out = np.zeros((B, Q), queries.dtype)
    for b, (v, f) in enumerate(meshes):
        n = Q if lengths is None else int(lengths[b])
        out[b, :n] = winding_number(v.astype(queries.dtype), f, queries[b, :n])
    return out


def closest_ragged(meshes, points, lengths=None):
    """etch_ragged_mesh_closest's contract: tests/_surface_oracle.py's closest point, scan by scan -> face (B,N), bary (B,N,3), d2 (B,N)."""
    B, N = points.shape[:2]
    face = np.full((B, N), -1, np.int32)
    bary = np.zeros((B, N, 3), points.dtype)
    d2 = np.zeros((B, N), points.dtype)
    for b, (v, f) in enumerate(meshes):
        n = N if lengths is None else int(lengths[b])
        fv = np.asarray(f, np.int64)
        bad = ~((fv >= 0) & (fv < len(v))).all(1)
        vv = np.concatenate([v.astype(points.dtype), np.full((1, 3), np.nan, points.dtype)])        # a face with a bad index: NaN, never wins
        fv = np.where(bad[:, None], len(v), fv)
        face[b, :n], bary[b, :n], d2[b, :n], _ = SO.closest_point_on_mesh(points[b, :n], vv, fv)
    return face, bary, d2


# --------------------------------------------------------------------------------------------- the containment term, in torch
def outside_and_target(scan_v, scan_f, w, face, bary):
    """One scan: w (V) numpy, face (V), bary (V,3) -> o (V) bool, c (V,3) float64 = sum_k bary_k s_k.  NaN w and face -1 are not outside."""
    with np.errstate(invalid="ignore"):
        o = (np.abs(w) < 0.5) & (face >= 0)
    tri = scan_v.astype(np.float64)[np.asarray(scan_f, np.int64)[np.where(face >= 0, face, 0)]]
    c = (bary.astype(np.float64)[:, :, None] * tri).sum(1)
    return o, c


def contain_sum(verts, o, c):
    """sum_v o_v |v - c_v|^2 for torch verts (V,3), o (V) bool and c (V,3) numpy, both held fixed."""
    ot = torch.from_numpy(o)
    if not bool(ot.any()):
        return torch.zeros((), dtype=verts.dtype)
    return ((verts[ot] - torch.from_numpy(c).to(verts.dtype)[ot]) ** 2).sum()


def fit_surface_contain(bm, pts, lengths, params0, iters, scans, lr=2e-2, w_contain=1e2, contain_every=10, weights=None, markers=None, prior=None,
                        w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05, dtype=torch.float64):
    """tests/_surface_oracle.py fit_surface with the fifth term  w_contain (sum_v o_v |v - c_v|^2) / V:  at iterations 0, K, 2K, ... the
    winding numbers and the closest points of the current vertices on scans[b] = (verts, faces) are recomputed IN `dtype`, and o_v, c_v
    are held in between.  -> (trace (B, iters, 5), final params (B,P))."""
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
            g["lr"] = CO.lr_at(i, iters, lr)
        verts, _ = CO.forward(tb, p, nj, nb)
        per = []
        for b in range(B):
            n = P.shape[1] if lengths is None else int(lengths[b])
            four = SO.scan_loss(verts[b], faces, P[b, :n], None if W is None else W[b, :n], trunc, None if mk is None else (mk[0], mk[1][b], mk[2][b]),
                                ws, p[b, 3 * nj:3 * nj + nb], p[b, 3:72], pr)
            if i % contain_every == 0:
                sv, sf = scans[b]
                vb = verts[b].detach().numpy().astype(npd)
                w = winding_number(sv.astype(npd), sf, vb)
                f, bary, _ = closest_ragged([(sv, sf)], vb[None])
                held[b] = outside_and_target(sv.astype(npd), sf, w, f[0], bary[0])
            per.append(torch.cat([four, (wc * contain_sum(verts[b], *held[b]) / verts.shape[1])[None]]))
        per = torch.stack(per)
        trace.append(per.detach().clone())
        opt.zero_grad()
        per.sum().backward()
        p.grad[:, -1] = 0
        opt.step()
    return torch.stack(trace, 1).numpy(), p.detach().numpy()


def metrics(scan, body_verts):
    """containment_metrics for one scan (verts, faces) and body_verts (V,3) in fp64 -> (outside_share, protrusion_rms_mm, protrusion_max_mm)."""
    sv, sf = scan
    v = np.asarray(body_verts, np.float64)
    w = winding_number(sv.astype(np.float64), sf, v)
    f, _, d2 = closest_ragged([(sv.astype(np.float64), sf)], v[None])
    o = (np.abs(w) < 0.5) & (f[0] >= 0)
    if not o.any():
        return 0.0, 0.0, 0.0
    return float(o.mean()), float(np.sqrt(d2[0][o].mean()) * 1e3), float(np.sqrt(d2[0][o].max()) * 1e3)


# --------------------------------------------------------------------------------------------- test meshes
@functools.lru_cache(maxsize=None)
def icosphere(subdiv):
    """The unit icosphere after `subdiv` subdivisions (20 * 4^subdiv faces, outward-oriented, vertices on the unit sphere) -> (verts f64, faces i32)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.stack(v), np.asarray(f, np.int32)


SCALE = np.array([0.15, 0.45, 0.10])
CAP_Y = 0.35


def ellipsoid(subdiv=3):
    v, f = icosphere(subdiv)
    return v * SCALE, f


def holed(subdiv=3):
    """The ellipsoid without the faces whose centroid lies in the cap y > 0.35 -> (verts, faces kept, faces removed)."""
    v, f = ellipsoid(subdiv)
    cap = v[f][:, :, 1].mean(1) > CAP_Y
    return v, f[~cap], f[cap]


def spherical_excess(v, f):
    """Girard: the solid angle of each spherical triangle with corners v[f] on the unit sphere = the sum of its corner angles - pi."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]

    def corner(p, q, r):                      # the angle at p between the great circles to q and r
        tq = q - (p * q).sum(1, keepdims=True) * p
        tr = r - (p * r).sum(1, keepdims=True) * p
        cosang = (tq * tr).sum(1) / (np.linalg.norm(tq, axis=1) * np.linalg.norm(tr, axis=1))
        return np.arccos(np.clip(cosang, -1, 1))

    return corner(a, b, c) + corner(b, c, a) + corner(c, a, b) - np.pi


def vertex_normals(v, f):
    """Area-weighted vertex normals, pointing away from the centroid of the vertices (numpy, fp64)."""
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return n if (n * (v - v.mean(0))).sum() > 0 else -n


def surface_queries(v, f, n, seed, offsets=(1e-4, 1e-3, 5e-3), box=0):
    """n queries at each of +-offsets (metres) along the face normal from random surface points of (v, f), plus `box` uniform ones in the
    bounding box grown by a fifth -> (Q,3) float64."""
    rng = np.random.default_rng(seed)
    out = []
    for d in offsets:
        for s in (1.0, -1.0):
            k = rng.integers(0, len(f), n)
            w = rng.dirichlet(np.ones(3), n)
            tri = v[f[k]]
            nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            out.append((w[:, :, None] * tri).sum(1) + s * d * nrm)
    if box:
        lo, hi = v.min(0), v.max(0)
        out.append(rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (box, 3)))
    return np.concatenate(out)


# --------------------------------------------------------------------------------------------- the scene of the issue
@functools.lru_cache(maxsize=None)
def body():
    from etch_amd.utils.body_model import SyntheticSurfaceSMPL
    bm = SyntheticSurfaceSMPL(7, rings=20, segs=24)
    assert bm.num_verts == 482 and bm.faces.shape == (960, 3)
    return bm


def verts64(bm, p):
    return CO.forward(S2.TorchBody(bm, torch.float64), torch.from_numpy(np.asarray(p)).double(), 24, 10)[0].numpy()


def smooth_params(B, seed):
    """Pose 0.05 rad, betas 0: the smooth body of test_fit_surface_20_iterations_vs_fp64."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal((B, 72)) * 0.05, np.zeros((B, 10)), rng.standard_normal((B, 3)) * 0.1, np.ones((B, 1))], 1).astype(np.float32)


def pushed_scan(bm, v, push=0.008):
    """The "scan" of a body: its vertices pushed `push` metres outward along their normals (fp32, what the device sees), the body's faces."""
    f = np.asarray(bm.faces, np.int32)
    return (v + push * vertex_normals(v, f)).astype(np.float32), f


@functools.lru_cache(maxsize=None)
def why_scene():
    """B = 2 (seeds 7 and 8; lengths 300 and 241): the true body (pose 0.05 rad, betas 0), a scan 8 mm outside it, 300 inner points on the
    true surface whose front half (normal z > 0) is biased 2 cm outward, 1 mm of noise; the fit starts from the truth.
    -> bm, truth (B,P), pts (B,300,3) f32, lengths, scans [(verts f32, faces)]"""
    bm = body()
    f = np.asarray(bm.faces, np.int64)
    truth = np.concatenate([smooth_params(1, 7), smooth_params(1, 8)])
    vt = verts64(bm, truth)
    pts, scans = [], []
    for b, seed in enumerate((17, 18)):
        rng = np.random.default_rng(seed)
        k = rng.integers(0, len(f), 300)
        w = rng.dirichlet(np.ones(3), 300)
        vn = vertex_normals(vt[b], f)
        nrm = (w[:, :, None] * vn[f[k]]).sum(1)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        x = (w[:, :, None] * vt[b][f[k]]).sum(1) + np.where(nrm[:, 2:3] > 0, 0.02, 0.0) * nrm + 0.001 * rng.standard_normal((300, 3))
        pts.append(x)
        scans.append(pushed_scan(bm, vt[b]))
    return bm, truth, np.stack(pts).astype(np.float32), [300, 241], scans


WHY_ITERS, WHY_EVERY = 40, 10


# --------------------------------------------------------------------------------------------- the inputs of the GPU tests
BAND = 0.05                       # the inside flag is compared where | |w64| - 0.5 | >= BAND


def _queries_for(v, f, n, box, seed, Q):
    q = surface_queries(v, f, n, seed, box=box)
    out = np.zeros((Q, 3), np.float32)
    out[:len(q)] = q
    return out, len(q)


@functools.lru_cache(maxsize=None)
def winding_case(name):
    """-> meshes [(verts f32, faces i32)], queries (B,600,3) f32, lengths.  Q = 600 (two 512-query blocks) and 70, ragged.
    "closed": the 1280-face ellipsoid (two 1024-face chunks) and the 320-face one.
    "odd":    the holed ellipsoid (1140 faces), the 320-face one with every face reversed, and the 320-face one with two more faces: one
              with a vertex index out of range and one of zero area (a repeated vertex)."""
    v3, f3 = ellipsoid(3)
    v2, f2 = ellipsoid(2)
    if name == "closed":
        meshes = [(v3, f3), (v2, f2)]
    else:
        hv, hf, _ = holed(3)
        soiled = np.concatenate([f2, [[0, 1, len(v2)], [5, 5, 9]]]).astype(np.int32)
        meshes = [(hv, hf), (v2, f2[:, ::-1].copy()), (v2, soiled)]
    qs, lengths = [], []
    for b, (v, f) in enumerate(meshes):
        good = f[((f >= 0) & (f < len(v))).all(1)]
        q, n = _queries_for(v, good, 80 if b == 0 else 10, 120 if b == 0 else 10, 100 + b + (10 if name == "odd" else 0), 600)
        qs.append(q)
        lengths.append(n)
    return [(v.astype(np.float32), f.astype(np.int32)) for v, f in meshes], np.stack(qs), np.array(lengths, np.int32)


def winding_refs(name):
    """The oracle on winding_case(name)'s fp32 inputs: (w64 (B,Q) from the same values in float64, w32 (B,Q) its own fp32 run)."""
    meshes, q, lengths = winding_case(name)
    w64 = winding_batch([(v.astype(np.float64), f) for v, f in meshes], q.astype(np.float64), lengths)
    return w64, winding_batch(meshes, q, lengths)


@functools.lru_cache(maxsize=None)
def trajectory_problem():
    """The smooth body of test_fit_surface_20_iterations_vs_fp64 (pose 0.05 rad, betas 0; lr 5e-3) under a scan 8 mm outside the TRUE body,
    started 0.03 rad / 0.05 off, so that part of the body starts outside: B = 2, 300 points with 3 mm noise, lengths (300, 241), weights,
    markers with an invalid part and a prior that the gradient can see.  -> bm, pts, lengths, p0, w, (vids, mk, valid), prior, scans"""
    bm = body()
    B, n = 2, 300
    truth = smooth_params(B, 61)
    vt = verts64(bm, truth)
    rng = np.random.default_rng(62)
    f = np.asarray(bm.faces, np.int64)
    pts = []
    for v in vt:
        k = rng.integers(0, len(f), n)
        wb = rng.dirichlet(np.ones(3), n)
        pts.append((wb[:, :, None] * v[f[k]]).sum(1) + 0.003 * rng.standard_normal((n, 3)))
    pts = np.stack(pts).astype(np.float32)
    p0 = truth.copy()
    p0[:, :72] += 0.03 * rng.standard_normal((B, 72)).astype(np.float32)
    p0[:, 72:82] += 0.05 * rng.standard_normal((B, 10)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, (B, n)).astype(np.float32)
    vids = rng.choice(bm.num_verts, 30, replace=False)
    mk = (vt[:, vids] + 0.002 * rng.standard_normal((B, 30, 3))).astype(np.float32)
    valid = rng.random((B, 30)) < 0.7
    mk[~valid] = 0.0
    prior = CO.random_prior(64, prec_scale=1e6, skew=0.2)
    return bm, pts, [n, 241], p0, w, (vids, mk, valid), prior, [pushed_scan(bm, v) for v in vt]
