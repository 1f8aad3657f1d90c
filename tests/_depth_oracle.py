"""fp64 numpy restatement of csrc/depth_render.hip for the single-view tests -- TEST INFRASTRUCTURE ONLY.

Each function repeats the kernels' operation order term by term (numpy never fuses a multiply and an add, and its +, -, * and / are the IEEE
operations), so depth, face, barycentrics, the packed cloud and the picked points must agree bit for bit.  Every (face, pixel) candidate is
evaluated at once and the winner of a pixel is the first in (z, face) order, which is the kernels' integer-min rule."""
import numpy as np

from _sampler_oracle import bbox_center, uniforms

DBL_MAX = np.finfo(np.float64).max


def camera_row(fx, fy, cx, cy, R=None, t=None):
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64)
    return np.concatenate([[fx, fy, cx, cy], R.reshape(9), t.reshape(3)]).astype(np.float64)


def look_at_row(eye, target, fx, fy, cx, cy, up=(0.0, 1.0, 0.0)):
    """The camera of the issue's self-check, built independently of etch_amd.depth.Camera.look_at."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return camera_row(fx, fy, cx, cy, R, -R @ eye)


def _edge(pu, pv, qu, qv, xu, xv):
    return (qu - pu) * (xv - pv) - (qv - pv) * (xu - pu)


def project(verts, cam):
    """-> u, v, z (V) of every vertex under camera row `cam`, and `finite` (V)."""
    fx, fy, cx, cy = cam[:4]
    R, t = cam[4:13].reshape(3, 3), cam[13:16]
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    with np.errstate(all="ignore"):
        pc = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)]
        u = fx * (pc[0] / pc[2]) + cx
        v = fy * (pc[1] / pc[2]) + cy
    finite = np.isfinite(verts).all(1) & np.isfinite(pc[0]) & np.isfinite(pc[1]) & np.isfinite(pc[2])
    return u, v, pc[2], finite


def render(verts, faces, cam, H, W, near=0.05):
    """-> depth (H,W) (+inf), face (H,W) int32 (-1), bary (H,W,3), dropped, status (bit 1: a corner or projection not finite), large (faces
    whose candidate box holds more than 256 pixels)."""
    verts, faces, cam = np.asarray(verts, np.float64), np.asarray(faces, np.int64), np.asarray(cam, np.float64)
    u, v, z, fin = project(verts, cam)
    U, V, Z = u[faces], v[faces], z[faces]                       # (F,3)
    finite = fin[faces].all(1)
    with np.errstate(invalid="ignore"):
        behind = finite & (Z < near).any(1)
    live = finite & ~behind
    proj_ok = np.isfinite(U).all(1) & np.isfinite(V).all(1)
    status = 1 if (~finite).any() or (live & ~proj_ok).any() else 0
    live &= proj_ok
    with np.errstate(all="ignore"):
        area = _edge(U[:, 0], V[:, 0], U[:, 1], V[:, 1], U[:, 2], V[:, 2])
    live &= (area != 0.0) & np.isfinite(area)
    depth = np.full(H * W, np.inf)
    face = np.full(H * W, -1, np.int32)
    bary = np.zeros((H * W, 3))
    idx = np.flatnonzero(live)
    large = 0
    if len(idx):
        U, V, Z, area = U[idx], V[idx], Z[idx], area[idx]
        ulo, uhi, vlo, vhi = U.min(1), U.max(1), V.min(1), V.max(1)
        c0, c1, r0, r1 = np.floor(ulo) - 1.0, np.ceil(uhi), np.floor(vlo) - 1.0, np.ceil(vhi)
        on = ~((c1 < 0.0) | (r1 < 0.0) | (c0 > W - 1) | (r0 > H - 1))
        c0 = np.maximum(c0, 0.0).astype(np.int64)
        c1 = np.minimum(c1, W - 1.0).astype(np.int64)
        r0 = np.maximum(r0, 0.0).astype(np.int64)
        r1 = np.minimum(r1, H - 1.0).astype(np.int64)
        bw = np.where(on, c1 - c0 + 1, 0)
        n = np.where(on, bw * (r1 - r0 + 1), 0)
        large = int((n > 256).sum())
        start = np.cumsum(n) - n
        k = np.repeat(np.arange(len(idx)), n)                    # the candidate's face (row of idx)
        j = np.arange(int(n.sum())) - start[k]
        r, c = r0[k] + j // np.maximum(bw[k], 1), c0[k] + j % np.maximum(bw[k], 1)
        pu, pv = c + 0.5, r + 0.5
        with np.errstate(all="ignore"):
            wA = _edge(U[k, 1], V[k, 1], U[k, 2], V[k, 2], pu, pv)
            wB = _edge(U[k, 2], V[k, 2], U[k, 0], V[k, 0], pu, pv)
            wC = _edge(U[k, 0], V[k, 0], U[k, 1], V[k, 1], pu, pv)
            inbox = (pu >= ulo[k]) & (pu <= uhi[k]) & (pv >= vlo[k]) & (pv <= vhi[k])
            cover = inbox & (((wA >= 0.0) & (wB >= 0.0) & (wC >= 0.0)) | ((wA <= 0.0) & (wB <= 0.0) & (wC <= 0.0)))
            q = np.stack([(wA / area[k]) / Z[k, 0], (wB / area[k]) / Z[k, 1], (wC / area[k]) / Z[k, 2]], 1)
            zz = 1.0 / ((q[:, 0] + q[:, 1]) + q[:, 2])
            cover &= (zz > 0.0) & (zz <= DBL_MAX)
        k, r, c, q, zz = k[cover], r[cover], c[cover], q[cover], zz[cover]
        pix = r * W + c
        order = np.lexsort((idx[k], zz, pix))                    # by pixel, then z, then face
        first = order[np.concatenate([[True], pix[order][1:] != pix[order][:-1]])] if len(order) else order
        depth[pix[first]] = zz[first]
        face[pix[first]] = idx[k[first]]
        bary[pix[first]] = q[first] * zz[first][:, None]
    return depth.reshape(H, W), face.reshape(H, W), bary.reshape(H, W, 3), int(behind.sum()), status, large


def pixel_rays(cam, H, W):
    """Eye and the world directions of the pixel-centre rays with camera-frame direction (., ., 1): t along such a ray is the depth z."""
    fx, fy, cx, cy = cam[:4]
    R, t = cam[4:13].reshape(3, 3), cam[13:16]
    r, c = np.divmod(np.arange(H * W), W)
    d = np.stack([(c + 0.5 - cx) / fx, (r + 0.5 - cy) / fy, np.ones(H * W)], 1)
    return np.broadcast_to(-R.T @ t, (H * W, 3)).copy(), d @ R


def unproject(depth, cam, near=0.05, far=np.inf):
    """One view: depth (H,W) -> index (n) int32 row-major, world points (n,3)."""
    fx, fy, cx, cy = cam[:4]
    R, t = cam[4:13].reshape(3, 3), cam[13:16]
    H, W = depth.shape
    z = depth.reshape(-1)
    with np.errstate(invalid="ignore"):
        index = np.flatnonzero((z > near) & (z < far))
    r, c = np.divmod(index, W)
    z = z[index]
    pc = [((c + 0.5) - cx) / fx * z, ((r + 0.5) - cy) / fy * z, z]
    d = [pc[k] - t[k] for k in range(3)]
    world = np.stack([(R[0, k] * d[0] + R[1, k] * d[1]) + R[2, k] * d[2] for k in range(3)], 1)
    return index.astype(np.int32), world


def pick(index, world, N, key, center=None):
    """-> points (N,3) fp64, fp32, pixel (N) int32, rank (N)."""
    n = len(index)
    uf = uniforms(key, N)[0]
    j = np.arange(N, dtype=np.int64)
    a = j * n // N                                               # stratum j = rows [a, a + w): disjoint, the last one ends at n
    w = (j + 1) * n // N - a
    rank = a + np.maximum(np.minimum(w - 1, np.floor(uf * w.astype(np.float64)).astype(np.int64)), 0)
    p = world[rank] if center is None else world[rank] - np.asarray(center, np.float64)
    return p, p.astype(np.float32), index[rank].astype(np.int32), rank


def bbox_mid(points):
    """(min + max) / 2 of a cloud, as etch_bbox_center defines it."""
    return bbox_center(points)
