"""The definitions of DESIGN section 27 restated with numpy -- the checker of csrc/cloud_mesh.hip and csrc/cloud_mesh_solve.h, never the product.
The lattice is fp64 with one rounding per node coordinate, the field is section 26a's winding number in fp32 (tests/_cloud_winding_oracle.py's
arithmetic, restated leaner here and compared with it by bits in the tests), the extraction is integers plus three fp32 operations per axis.
Everything that has an order is produced in that order, so the comparison with the kernels is by integers and bits."""
import itertools

import numpy as np

import _cloud_winding_oracle as WO

BLOCK = 8                                   # cells per block and axis
NODES = BLOCK + 1                           # nodes per block and axis: the face nodes are shared with the neighbours
BLOCK_NODES = NODES ** 3
MAX_NODES = (1 << 20) - 1                   # nodes per axis
MAX_BLOCKS = 1 << 24                        # blocks per lattice
MAX_COORD = 1 << 27                         # |lo|, |hi| below this: 8 lo fits an int32 with room
STATUS_RANGE, STATUS_EMPTY = 2, 4
BODY_COMPONENTS_2CM = 8                     # components of the level set of the fixture body's three views at voxel 0.02 (profiles/cloud_mesh_pins.txt)

PERMS = tuple(itertools.permutations((0, 1, 2)))          # lexicographic: (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # a tetrahedron's edges as pairs of its vertices, the lower vertex first
FACE_AXIS = (0, 0, 1, 1, 2, 2)                            # face f of a block: -x, +x, -y, +y, -z, +z
FACE_SIDE = (0, 1, 0, 1, 0, 1)


def corner_code(d):
    return 4 * d[0] + 2 * d[1] + d[2]


def corner_offset(code):
    return np.array([(code >> 2) & 1, (code >> 1) & 1, code & 1])


def tet_corners():
    """(6,4): the corner codes of the vertices of every tetrahedron: 000, e_p0, e_p0 + e_p1, 111."""
    out = np.zeros((6, 4), np.int64)
    for t, (p0, p1, _) in enumerate(PERMS):
        v = np.zeros((4, 3), np.int64)
        v[1, p0] = 1
        v[2, p0] = v[2, p1] = 1
        v[3] = 1
        out[t] = [corner_code(x) for x in v]
    return out


TET = tet_corners()


def _case_triangles(t, case):
    """The triangles of tetrahedron t in `case` as lists of three edges (pairs of tetrahedron vertices, lower first), by the rule of section 27."""
    ins = [v for v in range(4) if case >> v & 1]
    out = [v for v in range(4) if not case >> v & 1]
    if len(ins) in (0, 4):
        return []
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) == 1:
        tris = [[edge(ins[0], o) for o in out]]
    elif len(ins) == 3:
        tris = [[edge(i, out[0]) for i in ins]]
    else:
        (a, b), (c, d) = ins, out
        quad = [edge(a, c), edge(a, d), edge(b, d), edge(b, c)]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    corner = np.array([corner_offset(c) for c in TET[t]], np.float64)
    towards = corner[out].mean(0) - corner[ins].mean(0)
    res = []
    for tri in tris:
        p = [0.5 * (corner[a] + corner[b]) for a, b in tri]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert abs(n @ towards) > 1e-9
        res.append(tri if n @ towards > 0 else [tri[0], tri[2], tri[1]])
    return res


def encode_entry(tris):
    """ntri in bits 0..1, then three bits per edge id (index into EDGES), triangle 0's three edges first."""
    e = len(tris)
    for k, tri in enumerate(tris):
        for j, ed in enumerate(tri):
            e |= EDGES.index(ed) << (2 + 3 * (3 * k + j))
    return e


def tet_table():
    """(6,16) int64, generated from the rule: what the header carries as literals."""
    return np.array([[encode_entry(_case_triangles(t, c)) for c in range(16)] for t in range(6)], np.int64)


TABLE = tet_table()


# --------------------------------------------------------------------------------------------- lattice
def node_position(g, h):
    """fp32((double) g h): one fp64 product and one rounding per axis."""
    return (np.asarray(g, np.int64).astype(np.float64) * float(h)).astype(np.float32)


def valid_rows(pos, cap):
    with np.errstate(invalid="ignore"):
        return (cap > 0) & np.isfinite(pos).all(1)


def lattice(pos, cap, h, pad_blocks=2):
    """-> lo (3), hi (3) int64 in blocks, status."""
    ok = valid_rows(pos, cap)
    if not ok.any():
        return np.zeros(3, np.int64), np.zeros(3, np.int64), STATUS_EMPTY
    p = pos[ok].astype(np.float64)
    lo_d = np.floor(p.min(0) / (8.0 * float(h))) - pad_blocks
    hi_d = np.floor(p.max(0) / (8.0 * float(h))) + 1 + pad_blocks
    n = hi_d - lo_d
    if (np.abs(lo_d) >= MAX_COORD).any() or (np.abs(hi_d) >= MAX_COORD).any() or (8 * n + 1 > MAX_NODES).any() or n.prod() > MAX_BLOCKS:
        return np.zeros(3, np.int64), np.zeros(3, np.int64), STATUS_RANGE
    return lo_d.astype(np.int64), hi_d.astype(np.int64), 0


def seeds(pos, cap, h, lo, hi, seed_dilate=0):
    """The dense table (nx,ny,nz) bool of the blocks of round 0."""
    n = hi - lo
    table = np.zeros(tuple(n), bool)
    ok = valid_rows(pos, cap)
    b = np.floor(pos[ok].astype(np.float64) / (8.0 * float(h))).astype(np.int64) - lo[None, :]
    d = int(seed_dilate)
    for off in itertools.product(range(-d, d + 1), repeat=3):
        c = b + np.array(off)[None, :]
        c = c[((c >= 0) & (c < n[None, :])).all(1)]
        table[c[:, 0], c[:, 1], c[:, 2]] = True
    return table


# --------------------------------------------------------------------------------------------- field
def winding32(cloud, q, block=4096):
    """Section 26a's w at fp32 queries, the arithmetic of _cloud_winding_oracle.winding without the nearest row."""
    pos, moment, cap = (np.ascontiguousarray(a, np.float32) for a in cloud)
    q = np.ascontiguousarray(q, np.float32)
    w = np.zeros(len(q), np.float32)
    f0 = np.float32(0)
    for r0 in range(0, len(q), block):
        qq = q[r0:r0 + block]
        s = np.zeros(len(qq), np.float64)
        for c0 in range(0, len(pos), WO.CHUNK):
            P, M, C = pos[c0:c0 + WO.CHUNK], moment[c0:c0 + WO.CHUNK], cap[c0:c0 + WO.CHUNK]
            with np.errstate(all="ignore"):
                rx, ry, rz = (P[None, :, k] - qq[:, None, k] for k in range(3))
                d2 = (rx * rx + ry * ry) + rz * rz
                sm = np.where(d2 > C[None, :], d2, C[None, :])
                term = np.where(C[None, :] == 0, f0, ((rx * M[None, :, 0] + ry * M[None, :, 1]) + rz * M[None, :, 2]) / (sm * np.sqrt(sm)))
                s = s + np.cumsum(term, axis=1, dtype=np.float32)[:, -1].astype(np.float64) if term.shape[1] else s
        w[r0:r0 + block] = (s * WO.INV_4PI).astype(np.float32)
    return w


def field_at(cloud, g, h, level=0.5):
    """s = fabsf(w) - level at the nodes g (...,3) int64, fp32."""
    g = np.asarray(g, np.int64)
    w = winding32(cloud, node_position(g.reshape(-1, 3), h))
    return (np.abs(w) - np.float32(level)).astype(np.float32).reshape(g.shape[:-1])


def block_nodes(lo, block):
    """Global node coordinates (9,9,9,3) of the block with local coordinates `block` of the lattice that starts at lo."""
    base = 8 * (np.asarray(lo, np.int64) + np.asarray(block, np.int64))
    r = np.arange(NODES)
    return np.stack(np.meshgrid(base[0] + r, base[1] + r, base[2] + r, indexing="ij"), -1)


def block_field(cloud, h, lo, block, level=0.5):
    return field_at(cloud, block_nodes(lo, block), h, level)


def inside(s):
    with np.errstate(invalid="ignore"):
        return ~(s < 0)


def face_nodes(s, f):
    """The 81 values of face f of a block's (9,9,9) field."""
    return np.take(s, 8 * FACE_SIDE[f], axis=FACE_AXIS[f])


def face_mixed(s, f):
    i = inside(face_nodes(s, f))
    return bool(i.any() and not i.all())


# --------------------------------------------------------------------------------------------- growth
def grow(table, fields, last, n):
    """One round's face test over the blocks `last` (local coordinates): -> the sorted list of the blocks to activate, the clipped faces."""
    new, clipped = set(), 0
    for b in last:
        for f in range(6):
            if not face_mixed(fields[b], f):
                continue
            nb = list(b)
            nb[FACE_AXIS[f]] += 2 * FACE_SIDE[f] - 1
            nb = tuple(nb)
            if not all(0 <= nb[k] < n[k] for k in range(3)):
                clipped += 1
            elif not table[nb]:
                new.add(nb)
    return sorted(new), clipped


def follow(cloud, h, level=0.5, seed_dilate=0, pad_blocks=2, max_rounds=32, field_fn=None):
    """Seeds and growth of one cloud -> dict(lo, hi, status, blocks (S,3) sorted, fields (S,9,9,9), closed, clipped, rounds)."""
    pos, cap = np.asarray(cloud[0], np.float32), np.asarray(cloud[2], np.float32)
    lo, hi, status = lattice(pos, cap, h, pad_blocks)
    res = dict(lo=lo, hi=hi, status=status, blocks=np.zeros((0, 3), np.int64), fields=np.zeros((0, NODES, NODES, NODES), np.float32), closed=False,
               clipped=0, rounds=0)
    if status:
        return res
    n = hi - lo
    table = seeds(pos, cap, h, lo, hi, seed_dilate)
    field_fn = field_fn or (lambda b: block_field(cloud, h, lo, b, level))
    last = [tuple(b) for b in np.argwhere(table)]
    fields = {b: field_fn(b) for b in last}
    clipped, rounds, closed = 0, 0, True
    while True:
        new, c = grow(table, fields, last, n)
        clipped += c
        if not new:
            break
        if rounds == max_rounds:
            closed = False
            break
        for b in new:
            table[b] = True
            fields[b] = field_fn(b)
        last, rounds = new, rounds + 1
    blocks = sorted(fields)
    res.update(blocks=np.array(blocks, np.int64).reshape(-1, 3), fields=np.stack([fields[b] for b in blocks]) if blocks else res["fields"],
               closed=bool(closed and clipped == 0), clipped=clipped, rounds=rounds)
    return res


# --------------------------------------------------------------------------------------------- extraction
def node_key(i, kind):
    return ((((i[..., 0] << 20) + i[..., 1]) << 20) + i[..., 2]) * 8 + kind


_OFF = np.array([corner_offset(c) for c in range(8)], np.int64)           # (8,3)
_EDGE_LO = np.array([[TET[t][a] for a, _ in EDGES] for t in range(6)])    # (6,6) corner code of the edge's lower end
_EDGE_UP = np.array([[TET[t][b] for _, b in EDGES] for t in range(6)])


def extract_faces(blocks, fields, lo, h, table=None, chunk=128):
    """blocks (S,3) local coordinates sorted by block key, fields (S,9,9,9) fp32, ANY values -> counts (S,512) int32 triangles per cell,
    face keys (F,3) int64 and positions (F,3,3) fp32 in the order block, cell (cz fastest), tetrahedron, triangle."""
    table = TABLE if table is None else table
    blocks, fields = np.asarray(blocks, np.int64).reshape(-1, 3), np.asarray(fields, np.float32)
    lo = np.asarray(lo, np.int64)
    counts, keys, poss = [], [], []
    cell = np.stack(np.meshgrid(*(np.arange(BLOCK),) * 3, indexing="ij"), -1)                # (8,8,8,3)
    for s0 in range(0, len(blocks), chunk):
        B, Fd = blocks[s0:s0 + chunk], fields[s0:s0 + chunk]
        S = len(B)
        ins = inside(Fd)
        corner_in = np.stack([ins[:, o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8] for o in _OFF], -1)        # (S,8,8,8,8)
        case = np.zeros((S, 8, 8, 8, 6), np.int64)
        for t in range(6):
            for v in range(4):
                case[..., t] |= corner_in[..., TET[t][v]].astype(np.int64) << v
        ent = table[np.arange(6)[None, None, None, None, :], case]                                           # (S,8,8,8,6)
        ntri = ent & 3
        counts.append(ntri.sum(-1).reshape(S, 512).astype(np.int32))
        slot = np.arange(2 * 3).reshape(2, 3)
        eid = (ent[..., None, None] >> (2 + 3 * slot)) & 7                                                   # (S,8,8,8,6,2,3)
        mask = (ntri[..., None] > np.arange(2)).reshape(-1)                                                  # (S*512*6*2)
        tt = np.broadcast_to(np.arange(6)[None, None, None, None, :, None, None], eid.shape)
        eid, tt = eid.reshape(-1, 3)[mask], tt.reshape(-1, 3)[mask]
        ca, cb = _EDGE_LO[tt, eid], _EDGE_UP[tt, eid]                                                        # (F,3) corner codes
        sidx = np.broadcast_to(np.arange(S)[:, None, None, None, None, None, None], (S, 8, 8, 8, 6, 2, 3)).reshape(-1, 3)[mask]
        cl = np.broadcast_to(cell[None, :, :, :, None, None, None, :], (S, 8, 8, 8, 6, 2, 3, 3)).reshape(-1, 3, 3)[mask]
        nl = cl + _OFF[ca]                                                                                   # (F,3,3) node, local to the block
        nu = cl + _OFF[cb]
        s_n = Fd[sidx, nl[..., 0], nl[..., 1], nl[..., 2]]
        s_u = Fd[sidx, nu[..., 0], nu[..., 1], nu[..., 2]]
        i = 8 * B[sidx] + nl                                                                                 # local to the lattice
        keys.append(node_key(i, cb - ca))
        g = i + 8 * lo
        xn, xu = node_position(g, h), node_position(g + _OFF[cb - ca], h)
        with np.errstate(all="ignore"):
            t32 = s_n / (s_n - s_u)
            x = xn + t32[..., None] * (xu - xn)
        poss.append(np.where(_OFF[cb - ca] == 0, xn, x).astype(np.float32))
    if not counts:
        return np.zeros((0, 512), np.int32), np.zeros((0, 3), np.int64), np.zeros((0, 3, 3), np.float32)
    return np.concatenate(counts), np.concatenate(keys), np.concatenate(poss)


def weld(keys, pos):
    """Distinct keys ascending -> vertex keys (V), vertices (V,3) fp32, faces (F,3) int32.  Asserts that a key has one position, by bits."""
    uk, inv = np.unique(keys.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    flat = pos.reshape(-1, 3)
    verts = np.zeros((len(uk), 3), np.float32)
    verts[inv] = flat
    a, b = verts[inv].view(np.uint32), flat.view(np.uint32)
    assert ((a == b) | (np.isnan(verts[inv]) & np.isnan(flat))).all(), "a key with two positions"
    return uk, verts, inv.reshape(-1, 3).astype(np.int32)


# --------------------------------------------------------------------------------------------- components and measures
def labels(nv, faces):
    """label_v = the lowest vertex index of v's connected component over the face edges."""
    L = np.arange(nv, dtype=np.int64)
    f = np.asarray(faces, np.int64)
    while True:
        m = L[f].min(1)
        new = L.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], m)
            np.minimum.at(new, L[f[:, k]], m)
        while True:
            j = new[new]
            if (j == new).all():
                break
            new = j
        if (new == L).all():
            return L
        L = new


def keep_largest(verts, faces, lab):
    """-> verts, faces of the component with the most faces (a tie: the lowest label), order preserved; the number of components."""
    if len(faces) == 0:
        return verts[:0], faces[:0], 0
    fl = lab[faces[:, 0]]
    ids, cnt = np.unique(fl, return_counts=True)
    win = ids[np.argmax(cnt)]                                   # argmax returns the first maximum: the lowest label
    kv = lab == win
    remap = np.cumsum(kv) - 1
    return verts[kv], remap[faces[fl == win]].astype(np.int32), len(np.unique(lab))


def edge_counts(faces):
    """-> (every undirected edge is in exactly two faces, every directed edge in exactly one)."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, dc = np.unique(d[:, 0] * (1 << 32) + d[:, 1], return_counts=True)
    u = np.sort(d, 1)
    _, uc = np.unique(u[:, 0] * (1 << 32) + u[:, 1], return_counts=True)
    return bool((uc == 2).all()), bool((dc == 1).all())


def euler(nv, faces):
    f = np.asarray(faces, np.int64)
    u = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return nv - len(np.unique(u[:, 0] * (1 << 32) + u[:, 1])) + len(f)


def volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def reconstruct(cloud, h, level=0.5, keep="largest", seed_dilate=0, pad_blocks=2, max_rounds=32, dense=False):
    """cloud.reconstruct for one cloud (pos, moment, cap) -> dict(verts fp32, faces, keys, closed, clipped, blocks, rounds, components, status).
    dense=True evaluates every block of the lattice instead of following the surface."""
    if dense:
        pos, cap = np.asarray(cloud[0], np.float32), np.asarray(cloud[2], np.float32)
        lo, hi, status = lattice(pos, cap, h, pad_blocks)
        n = hi - lo
        r = [np.arange(8 * lo[k], 8 * hi[k] + 1) for k in range(3)]
        whole = field_at(cloud, np.stack(np.meshgrid(*r, indexing="ij"), -1), h, level)
        blocks = np.argwhere(np.ones(tuple(n), bool))
        fields = np.stack([whole[8 * b[0]:8 * b[0] + 9, 8 * b[1]:8 * b[1] + 9, 8 * b[2]:8 * b[2] + 9] for b in blocks])
        res = dict(lo=lo, hi=hi, status=status, blocks=blocks, fields=fields, closed=True, clipped=0, rounds=0)
    else:
        res = follow(cloud, h, level, seed_dilate, pad_blocks, max_rounds)
    _, keys, pos3 = extract_faces(res["blocks"], res["fields"], res["lo"], h)
    vk, verts, faces = weld(keys, pos3)
    lab = labels(len(verts), faces)
    comps = len(np.unique(lab))
    if keep == "largest" and len(faces):
        kv = lab == keep_winner(lab, faces)
        vk = vk[kv]
        verts, faces, _ = keep_largest(verts, faces, lab)
    res.update(verts=verts, faces=faces, keys=vk, components=comps, nblocks=len(res["blocks"]))
    return res


def keep_winner(lab, faces):
    ids, cnt = np.unique(lab[faces[:, 0]], return_counts=True)
    return ids[np.argmax(cnt)]


def hemisphere(n=500, R=0.5, z_min=-0.1, area_k=8):
    """The open fixture: the rows with z > z_min of the n-row Fibonacci sphere, as an oriented cloud."""
    p, nrm = WO.fibonacci_sphere(n, R)
    k = p[:, 2] > z_min
    return WO.surface(np.ascontiguousarray(p[k]), np.ascontiguousarray(nrm[k]), area_k)


def sphere(n=2000, R=0.5, area_k=8):
    p, nrm = WO.fibonacci_sphere(n, R)
    return WO.surface(p, nrm, area_k)
