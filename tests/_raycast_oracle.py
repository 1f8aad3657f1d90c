"""fp64 numpy restatement of csrc/raycast.hip for the info-point tests -- TEST INFRASTRUCTURE ONLY.

Each function repeats the kernel's operation order term by term (numpy never fuses a multiply and an add, and its +, -, *, / and sqrt are
the IEEE operations), so ray hits, closest points and thinning flags must agree bit for bit.  Vertex normals go through arccos, whose last
bit the device library and numpy may round differently: they agree within 1e-15."""
import numpy as np


def _dot(ax, ay, az, bx, by, bz):
    return ((ax * bx) + (ay * by)) + (az * bz)


def ray_first_hit(orig, dirs, verts, faces, excl=None, t_max=None, block=64):
    """-> face (R) int32 (-1 = miss), t (R) (+inf), bary (R,3), loc (R,3): the smallest t, then the lowest face."""
    R = len(orig)
    tri = verts[faces]
    v0 = tri[:, 0]
    e1 = tri[:, 1] - tri[:, 0]
    e2 = tri[:, 2] - tri[:, 0]
    face = np.full(R, -1, np.int32)
    t_out = np.full(R, np.inf)
    bary = np.zeros((R, 3))
    loc = np.zeros((R, 3))
    fidx = np.arange(len(faces))
    with np.errstate(all="ignore"):
        for r0 in range(0, R, block):
            o = orig[r0:r0 + block, None, :]
            d = dirs[r0:r0 + block, None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            px, py, pz = dy * e2[:, 2] - dz * e2[:, 1], dz * e2[:, 0] - dx * e2[:, 2], dx * e2[:, 1] - dy * e2[:, 0]
            det = _dot(e1[:, 0], e1[:, 1], e1[:, 2], px, py, pz)
            inv = 1.0 / det
            sx, sy, sz = o[..., 0] - v0[:, 0], o[..., 1] - v0[:, 1], o[..., 2] - v0[:, 2]
            u = _dot(sx, sy, sz, px, py, pz) * inv
            qx, qy, qz = sy * e1[:, 2] - sz * e1[:, 1], sz * e1[:, 0] - sx * e1[:, 2], sx * e1[:, 1] - sy * e1[:, 0]
            v = _dot(dx, dy, dz, qx, qy, qz) * inv
            t = _dot(e2[:, 0], e2[:, 1], e2[:, 2], qx, qy, qz) * inv
            tm = np.inf if t_max is None else t_max[r0:r0 + block, None]
            hit = (det != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 0.0) & (t < tm)
            if excl is not None:
                hit &= fidx[None, :] != excl[r0:r0 + block, None]
            tt = np.where(hit, t, np.inf)
            best = tt.min(1)
            for k in range(tt.shape[0]):
                if np.isinf(best[k]):
                    continue
                f = int(np.flatnonzero(tt[k] == best[k])[0])
                r = r0 + k
                face[r], t_out[r] = f, t[k, f]
                bary[r] = ((1.0 - u[k, f]) - v[k, f], u[k, f], v[k, f])
                loc[r] = orig[r] + t[k, f] * dirs[r]
    return face, t_out, bary, loc


def closest_on_triangles(p, a, b, c):
    """Ericson 5.1.5 for points p (..., 3) against triangles (..., 3) (broadcast) -> q (..., 3), bary (..., 3), d2 (...), region (...) 0..6
    = A, B, AB, C, AC, BC, interior."""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
        d2 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
        bp = p - b
        d3 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], bp[..., 0], bp[..., 1], bp[..., 2])
        d4 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], bp[..., 0], bp[..., 1], bp[..., 2])
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], cp[..., 0], cp[..., 1], cp[..., 2])
        d6 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], cp[..., 0], cp[..., 1], cp[..., 2])
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)]
        region = np.select(conds, list(range(6)), 6)
        vab = d1 / (d1 - d3)
        wac = d2 / (d2 - d6)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / ((va + vb) + vc)
        vi, wi = vb * denom, vc * denom
        shape = np.broadcast_shapes(p.shape, a.shape)
        q = np.empty(shape)
        bary = np.empty(shape)
        A, B, C = (np.broadcast_to(x, shape) for x in (a, b, c))
        ABv, ACv = np.broadcast_to(ab, shape), np.broadcast_to(ac, shape)
        z = np.zeros(region.shape)
        one = np.ones(region.shape)
        cands_q = [A, B, A + vab[..., None] * ABv, C, A + wac[..., None] * ACv, B + wbc[..., None] * (C - B),
                   (A + ABv * vi[..., None]) + ACv * wi[..., None]]
        cands_b = [np.stack([one, z, z], -1), np.stack([z, one, z], -1), np.stack([1.0 - vab, vab, z], -1), np.stack([z, z, one], -1),
                   np.stack([1.0 - wac, z, wac], -1), np.stack([z, 1.0 - wbc, wbc], -1), np.stack([(1.0 - vi) - wi, vi, wi], -1)]
        for k in range(7):
            m = region == k
            q[m] = cands_q[k][m]
            bary[m] = cands_b[k][m]
        e = p - q
        dd = _dot(e[..., 0], e[..., 1], e[..., 2], e[..., 0], e[..., 1], e[..., 2])
    return q, bary, dd, region


def closest_point_on_mesh(points, verts, faces, block=32):
    """-> face (P) int32, bary (P,3), closest (P,3), d2 (P): the smallest d2, then the lowest face (NaN never wins)."""
    P = len(points)
    tri = verts[faces]
    face = np.full(P, -1, np.int32)
    bary = np.zeros((P, 3))
    q = np.zeros((P, 3))
    d2 = np.full(P, np.inf)
    for r0 in range(0, P, block):
        p = points[r0:r0 + block, None, :]
        qq, bb, dd, _ = closest_on_triangles(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        dd = np.where(np.isnan(dd), np.inf, dd)
        for k in range(dd.shape[0]):
            m = dd[k].min()
            if np.isinf(m):
                continue
            f = int(np.flatnonzero(dd[k] == m)[0])
            face[r0 + k], bary[r0 + k], q[r0 + k], d2[r0 + k] = f, bb[k, f], qq[k, f], dd[k, f]
    return face, bary, q, d2


def _unit(x):
    n = np.sqrt(_dot(x[:, 0], x[:, 1], x[:, 2], x[:, 0], x[:, 1], x[:, 2]))
    with np.errstate(all="ignore"):
        return np.where((n > 0.0)[:, None], x / n[:, None], x)


def vertex_normals(verts, faces):
    """trimesh.geometry.weighted_vertex_normals with trimesh.triangles.angles weights, summed per vertex in ascending (face, corner) order."""
    tri = verts[faces]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    ln = np.sqrt(_dot(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2]))
    with np.errstate(all="ignore"):
        fn = np.where((ln > 0.0)[:, None], n / ln[:, None], 0.0)
    u, v, w = _unit(e1), _unit(e2), _unit(tri[:, 2] - tri[:, 1])
    a0 = np.arccos(np.clip(_dot(u[:, 0], u[:, 1], u[:, 2], v[:, 0], v[:, 1], v[:, 2]), -1.0, 1.0))
    a1 = np.arccos(np.clip(_dot(-u[:, 0], -u[:, 1], -u[:, 2], w[:, 0], w[:, 1], w[:, 2]), -1.0, 1.0))
    a2 = (np.pi - a0) - a1
    ang = np.nan_to_num(np.stack([a0, a1, a2], 1), nan=0.0)
    flat = faces.ravel()
    order = np.argsort(flat, kind="stable")             # by vertex, then ascending 3 f + corner
    contrib = fn[order // 3] * ang.ravel()[order][:, None]
    s = np.zeros((len(verts), 3))
    np.add.at(s, flat[order], contrib)                  # unbuffered, in the order given: s = s + term
    return _unit(s)


def close_pairs(points, r2, block=512):
    """Every pair i < j with ((dx*dx + dy*dy) + dz*dz) <= r2 -> (K,2) int64, rows in (i, j) order."""
    out = []
    C = len(points)
    for i0 in range(0, C, block):
        d = points[i0:i0 + block, None, :] - points[None, :, :]
        dd = _dot(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2])
        ii, jj = np.nonzero(dd <= r2)
        ii = ii + i0
        m = ii < jj
        out.append(np.stack([ii[m], jj[m]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def remove_close(points, r2):
    """trimesh 4.x points.remove_close: -> (degree (C), removed (C) bool)."""
    pairs = close_pairs(points, r2)
    count = np.bincount(pairs.ravel(), minlength=len(points))
    removed = np.zeros(len(points), bool)
    if len(pairs):
        column = count[pairs].argmax(axis=1)           # the endpoint of higher degree; argmax keeps i on a tie
        removed[pairs.ravel()[column + 2 * np.arange(len(column))]] = True
    return count, removed


class Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)


def load_fixture(path):
    """tests/golden/infopoints_4ddress.npz (written by tests/_make_infopoints_fixture.py): a band of the reference's 4D-Dress frame in which
    every info-point ray sees the whole frame's geometry.  -> dict: scan, body (Mesh, vertices = q / 1e8 exactly as the OBJ parses),
    body_inner (the body's faces with all vertices in the band; samples are drawn there), inner_faces (their indices in body.faces), the
    reference records whose body point lies in the band (info_points, info_vectors, records = their row in the reference file), and the
    reference .ply's header and per-record line pairs (bytes)."""
    d = np.load(path)
    scan = Mesh(d["scan_vertices_e8"] / 1e8, d["scan_faces"])
    body = Mesh(d["body_vertices_e8"] / 1e8, d["body_faces"])
    inner = d["body_inner_faces"].astype(np.int64)
    off = d["ply_line_offsets"]
    raw = d["ply_lines"].tobytes()
    return {"scan": scan, "body": body, "body_inner": Mesh(body.vertices, body.faces[inner]), "inner_faces": inner,
            "info_points": d["info_points"], "info_vectors": d["info_vectors"], "records": d["records"], "band": d["band"],
            "ply_header": d["ply_header"].tobytes(), "ply_lines": [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]}
