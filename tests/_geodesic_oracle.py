"""fp64 numpy + scipy.sparse restatement of the geodesic half of the reference's GTDataset.__getitem__ (src/data_utils/GT_dataloader.py:124-145),
as DESIGN.md section 10 defines it: loop subdivision without smoothing (trimesh.remesh.subdivide), a sequential Lawson flip to the intrinsic
Delaunay triangulation, the cotan operators on its edge lengths and the heat method with direct (splu) solves.  Test infrastructure, never the
product; the GPU tests read only what tests/_make_geodesic_fixture.py wrote from it."""
import numpy as np

DELAUNAY_TOL = 1e-12         # an edge is flipped while cot a + cot b < -DELAUNAY_TOL
MOLLIFY_EPS = 1e-6           # intrinsic mollification, relative to the mean edge length


def subdivide(vertices, faces):
    """trimesh.remesh.subdivide on every face: the original vertices keep their indices, one midpoint per unique edge (a < b) is appended in
    order of (b, a), and face i becomes faces 4i..4i+3 = [v0,m01,m20], [m01,v1,m12], [m20,m12,v2], [m01,m12,m20]."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    e = np.sort(np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
    key = (e[:, 1] << 32) | e[:, 0]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    ue = e[first]
    mid = (v[ue[:, 0]] + v[ue[:, 1]]) / 2.0
    m = inv.reshape(-1, 3) + len(v)
    nf = np.column_stack([f[:, 0], m[:, 0], m[:, 2], m[:, 0], f[:, 1], m[:, 1], m[:, 2], m[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]]).reshape(-1, 3)
    return np.concatenate([v, mid]), nf


class EdgeMesh:
    """A closed oriented manifold triangle mesh stored by edges.  Edge e of the input is (a, b), a < b, in order of (b, a); fe[f, k] = the
    edge opposite corner k of face f (between corners k+1 and k+2), ef[e] = its two faces, fs[f, k] = which slot of ef[fe[f, k]] face f holds."""

    def __init__(self, vertices, faces):
        f = np.asarray(faces, np.int64)
        self.nv = len(vertices)
        opp = np.sort(np.stack([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 1).reshape(-1, 2), axis=1)   # edge opposite corner k
        key = (opp[:, 1] << 32) | opp[:, 0]
        uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
        E = len(uk)
        cnt = np.bincount(inv, minlength=E)
        if np.any(cnt > 2):
            raise ValueError("not a manifold mesh: an edge has more than two faces")
        self.ev = opp[first].copy()
        self.fv = f.copy()
        self.fe = inv.reshape(-1, 3).copy()
        order = np.argsort(inv, kind="stable")           # the lower (face, corner) takes slot 0; a boundary edge has ef[e, 1] = -1
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        slot = np.arange(3 * len(f)) - np.repeat(start, cnt)
        self.ef = np.full((E, 2), -1, np.int64)
        self.ef[inv[order], slot] = order // 3
        self.fs = np.empty(3 * len(f), np.int64)
        self.fs[order] = slot
        self.fs = self.fs.reshape(-1, 3)
        v = np.asarray(vertices, np.float64)
        d = v[self.ev[:, 1]] - v[self.ev[:, 0]]
        self.el = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    @property
    def E(self):
        return len(self.ev)

    def face_lengths(self):
        """(F,3): the length of the edge opposite each corner."""
        return self.el[self.fe]


def mollify(el, fe, eps=MOLLIFY_EPS):
    """geometry-central's mollifyIntrinsic as read here: delta = max(0, max over faces and corners of eps*hbar - (l_j + l_k - l_i)), every
    edge length += delta, hbar = the mean edge length."""
    l = el[fe]
    e = eps * el.mean()
    slack = np.concatenate([l[:, 1] + l[:, 2] - l[:, 0], l[:, 2] + l[:, 0] - l[:, 1], l[:, 0] + l[:, 1] - l[:, 2]])
    delta = max(0.0, float(np.max(e - slack)))
    return el + delta, delta


def face_geometry(l):
    """Per face from its lengths (F,3) (l[:, k] opposite corner k): area (Heron, the stable ordering) and the cotangent of each corner."""
    a, b, c = l[:, 0], l[:, 1], l[:, 2]
    s = -np.sort(-l, axis=1)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    area = 0.25 * np.sqrt(np.maximum((x + (y + z)) * (z - (x - y)) * (z + (x - y)) * (x + (y - z)), 0.0))
    cot = np.stack([(b * b + c * c - a * a), (c * c + a * a - b * b), (a * a + b * b - c * c)], 1) / (4.0 * area[:, None])
    return area, cot


def edge_cot_sums(mesh, el=None):
    """cot a + cot b of every edge (the two corners opposite it)."""
    el = mesh.el if el is None else el
    _, cot = face_geometry(el[mesh.fe])
    w = np.zeros(mesh.E)
    np.add.at(w, mesh.fe.ravel(), cot.ravel())
    return w


def _flip_length(lab, lac, lbc, lbd, lcd):
    """|ad| in the 2-D layout of the quad a-b-d-c around the diagonal bc (b at the origin, c on +x, a above, d below)."""
    xa = (lab * lab - lac * lac + lbc * lbc) / (2.0 * lbc)
    ya = np.sqrt(max(lab * lab - xa * xa, 0.0))
    xd = (lbd * lbd - lcd * lcd + lbc * lbc) / (2.0 * lbc)
    yd = np.sqrt(max(lbd * lbd - xd * xd, 0.0))
    dx, dy = xa - xd, ya + yd
    return np.sqrt(dx * dx + dy * dy)


def _cot_sum_edge(mesh, e):
    if mesh.ef[e, 1] < 0:
        return np.inf                                    # a boundary edge is Delaunay
    s = 0.0
    for f in mesh.ef[e]:
        k = int(np.flatnonzero(mesh.fe[f] == e)[0])
        l = mesh.el[mesh.fe[f]]
        a, b, c = l[k], l[(k + 1) % 3], l[(k + 2) % 3]
        sp = 0.5 * (a + b + c)
        area = np.sqrt(max(sp * (sp - a) * (sp - b) * (sp - c), 0.0))
        s += (b * b + c * c - a * a) / (4.0 * area)
    return s


def flip_edge(mesh, e):
    """Flip edge e = bc between f = (a, b, c) and g = (d, c, b) into ad: f -> (a, b, d), g -> (d, c, a)."""
    f, g = mesh.ef[e]
    k = int(np.flatnonzero(mesh.fe[f] == e)[0])
    j = int(np.flatnonzero(mesh.fe[g] == e)[0])
    a, b, c = mesh.fv[f, k], mesh.fv[f, (k + 1) % 3], mesh.fv[f, (k + 2) % 3]
    d = mesh.fv[g, j]
    e_ca, s_ca = mesh.fe[f, (k + 1) % 3], mesh.fs[f, (k + 1) % 3]
    e_ab, s_ab = mesh.fe[f, (k + 2) % 3], mesh.fs[f, (k + 2) % 3]
    e_bd, s_bd = mesh.fe[g, (j + 1) % 3], mesh.fs[g, (j + 1) % 3]
    e_dc, s_dc = mesh.fe[g, (j + 2) % 3], mesh.fs[g, (j + 2) % 3]
    s_ef, s_eg = mesh.fs[f, k], mesh.fs[g, j]
    l = mesh.el
    mesh.el[e] = _flip_length(l[e_ab], l[e_ca], l[e], l[e_bd], l[e_dc])
    mesh.fv[f] = (a, b, d)
    mesh.fe[f] = (e_bd, e, e_ab)
    mesh.fs[f] = (s_bd, s_ef, s_ab)
    mesh.fv[g] = (d, c, a)
    mesh.fe[g] = (e_ca, e, e_dc)
    mesh.fs[g] = (s_ca, s_eg, s_dc)
    mesh.ef[e_bd, s_bd] = f
    mesh.ef[e_ca, s_ca] = g
    mesh.ev[e] = (min(a, d), max(a, d))
    return (e_ab, e_ca, e_bd, e_dc)


def flip_to_delaunay(mesh, tol=DELAUNAY_TOL, max_flips=10_000_000):
    """Sequential Lawson flips from a queue of every edge in index order; returns the number of flips."""
    from collections import deque

    q = deque(range(mesh.E))
    inq = np.ones(mesh.E, bool)
    n = 0
    while q:
        e = q.popleft()
        inq[e] = False
        if _cot_sum_edge(mesh, e) >= -tol:
            continue
        for o in flip_edge(mesh, e):
            if not inq[o]:
                q.append(o)
                inq[o] = True
        n += 1
        if n > max_flips:
            raise RuntimeError("no Delaunay triangulation within the flip budget")
    return n


def build_intrinsic(vertices, faces, laplacian="intrinsic_delaunay"):
    """-> (mesh, mean input edge length, flips).  "intrinsic_delaunay" mollifies and flips; "cotan" keeps the input triangulation."""
    mesh = EdgeMesh(vertices, faces)
    hbar = float(mesh.el.mean())
    flips = 0
    if laplacian == "intrinsic_delaunay":
        mesh.el, _ = mollify(mesh.el, mesh.fe)
        flips = flip_to_delaunay(mesh)
    elif laplacian != "cotan":
        raise ValueError(laplacian)
    return mesh, hbar, flips


def operators(mesh):
    """PSD cotan Laplacian L (L_ij = -(cot a + cot b) / 2) and lumped masses M_i = sum of the incident face areas / 3, as scipy CSR / arrays."""
    import scipy.sparse as sp

    area, cot = face_geometry(mesh.face_lengths())
    w = np.zeros(mesh.E)
    np.add.at(w, mesh.fe.ravel(), cot.ravel())
    w *= 0.5
    i, j = mesh.ev[:, 0], mesh.ev[:, 1]
    n = mesh.nv
    L = sp.coo_matrix((np.concatenate([-w, -w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    L = L + sp.diags(np.asarray(-L.sum(1)).ravel())
    mass = np.zeros(n)
    np.add.at(mass, mesh.fv.ravel(), np.repeat(area / 3.0, 3))
    return L.tocsc(), mass, area, cot


class HeatSolver:
    """pp3d.MeshHeatMethodDistanceSolver(V, F, t_coef) restated with splu: (M + t L) u = e_src, X = -grad u / |grad u| per face (X = 0 where
    grad u = 0), div X, L phi = -div X with the constant removed (phi[src] pinned), phi -= phi[src]."""

    def __init__(self, vertices, faces, t_coef=1.0, laplacian="intrinsic_delaunay"):
        import scipy.sparse as sp
        import scipy.sparse.linalg as sla

        self.mesh, hbar, self.flips = build_intrinsic(vertices, faces, laplacian)
        self.t = t_coef * hbar * hbar
        self.L, self.mass, self.area, self.cot = operators(self.mesh)
        self.heat = sla.splu((sp.diags(self.mass) + self.t * self.L).tocsc())
        self._sla = sla
        self._poisson = {}

    def _grad_inv_norm(self, u):
        m = self.mesh
        l = m.face_lengths()
        ui, uj, uk = u[m.fv[:, 0]], u[m.fv[:, 1]], u[m.fv[:, 2]]
        # layout: corner 0 at the origin, corner 1 on +x at |l2| (the edge opposite corner 2), corner 2 at (x, y), y > 0
        lij = l[:, 2]
        x = (lij * lij + l[:, 1] * l[:, 1] - l[:, 0] * l[:, 0]) / (2.0 * lij)
        y = 2.0 * self.area / lij
        gx = (uj - ui) / lij
        gy = ((uk - ui) - gx * x) / y
        nrm = np.sqrt(gx * gx + gy * gy)
        return np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)

    def divergence(self, u):
        """div X at every vertex = sum over edges ij of K_ij (u_i - u_j), K_ij = sum over its faces of cot(opposite corner) / (2 |grad u_f|)."""
        m = self.mesh
        inv = self._grad_inv_norm(u)
        K = np.zeros(m.E)
        np.add.at(K, m.fe.ravel(), (0.5 * self.cot * inv[:, None]).ravel())
        i, j = m.ev[:, 0], m.ev[:, 1]
        d = K * (u[i] - u[j])
        div = np.zeros(m.nv)
        np.add.at(div, i, d)
        np.add.at(div, j, -d)
        return div

    def distance(self, src):
        b = np.zeros(self.mesh.nv)
        b[src] = 1.0
        u = self.heat.solve(b)
        rhs = -self.divergence(u)
        rhs -= rhs.mean()
        if src not in self._poisson:
            keep = np.ones(self.mesh.nv, bool)
            keep[src] = False
            self._poisson[src] = (keep, self._sla.splu(self.L[keep][:, keep].tocsc()))
        keep, lu = self._poisson[src]
        phi = np.zeros(self.mesh.nv)
        phi[keep] = lu.solve(rhs[keep])
        return phi - phi[src]


def marker_fields(vertices, faces, marker_vids, t_coef=1.0, laplacian="intrinsic_delaunay", keep=()):
    """Subdivide, solve one column per marker -> (min distance (V'), label (V') int64 = first marker on a tie, second-best margin (V'),
    {marker column: distance (V')} for the columns in `keep`, solver)."""
    sv, sf = subdivide(vertices, faces)
    s = HeatSolver(sv, sf, t_coef, laplacian)
    D = np.stack([s.distance(int(m)) for m in marker_vids])
    lab = np.argmin(D, axis=0)
    srt = np.sort(D, axis=0)
    return srt[0], lab, srt[1] - srt[0], {k: D[k] for k in keep}, s


def targets(inner_points, sub_vertices, min_dist, labels):
    """Nearest subdivided vertex of each inner point (fp64 brute force, lowest index on a tie) -> confidences (N,1) = exp(-10 d), labels (N,),
    and the gap between the nearest and second-nearest vertex distances."""
    p = np.asarray(inner_points, np.float64)
    v = np.asarray(sub_vertices, np.float64)
    nn = np.empty(len(p), np.int64)
    gap = np.empty(len(p))
    for s in range(0, len(p), 256):
        d = ((p[s:s + 256, None, :] - v[None]) ** 2).sum(-1)
        nn[s:s + 256] = np.argmin(d, axis=1)
        two = np.sqrt(np.partition(d, 1, axis=1)[:, :2])
        gap[s:s + 256] = two[:, 1] - two[:, 0]
    return np.exp(-10.0 * min_dist[nn]).reshape(-1, 1), labels[nn], gap


def icosphere(level):
    """Unit icosphere: the icosahedron subdivided `level` times, midpoints projected to the sphere."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        v, f = subdivide(v, f)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v, f


def planar_grid(n, h=1.0 / 32, jitter=0.3, seed=0):
    """An n x n grid in the plane z = 0 with spacing h, interior points moved by up to jitter * h / 2 per axis, two triangles per cell
    (diagonal alternating by cell parity)."""
    rng = np.random.default_rng(seed)
    uu, vv = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    inner = (uu > 0) & (uu < n - 1) & (vv > 0) & (vv < n - 1)
    uu = uu + inner * jitter * rng.uniform(-0.5, 0.5, uu.shape)
    vv = vv + inner * jitter * rng.uniform(-0.5, 0.5, vv.shape)
    v = np.stack([uu.ravel() * h, vv.ravel() * h, np.zeros(n * n)], 1)
    idx = np.arange(n * n).reshape(n, n)
    fs = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = idx[i, j], idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]
            fs += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return v, np.asarray(fs, np.int64)


def load_fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}
