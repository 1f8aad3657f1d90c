"""MI355X counterpart of the geodesic half of the reference's GTDataset.__getitem__ (src/data_utils/GT_dataloader.py:124-145): the per-point
part label (which marker is geodesically nearest) and the confidence exp(-10 d), with pp3d.MeshHeatMethodDistanceSolver replaced by
csrc/geodesic.hip (DESIGN.md section 10 states the operators and where they may differ from potpourri3d).

The host only subdivides (numpy; the topology is cached, SMPL's never changes) and builds the edge tables of that topology once; the
intrinsic Delaunay flips, the operators, the 86 heat / Poisson solves per body, the marker min / argmin and the point lookup run on the GPU.
"""
import numpy as np
import torch

from . import ops
from ._lib import EtchHipError

LAPLACIANS = ("intrinsic_delaunay", "cotan")


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


class SubdivisionTopology:
    """trimesh.remesh.subdivide's topology for one face array: the original vertices keep their indices, one midpoint per unique edge (a < b)
    is appended in order of (b, a) (trimesh's bit-packed unique_rows as read here), face i becomes faces 4i..4i+3 =
    [v0,m01,m20], [m01,v1,m12], [m20,m12,v2], [m01,m12,m20]."""

    def __init__(self, faces, num_vertices):
        f = np.asarray(faces, np.int64)
        if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0:
            raise EtchHipError(f"faces must be (F,3), got {f.shape}")
        if f.min() < 0 or f.max() >= num_vertices:
            raise EtchHipError(f"face indices must lie in [0, {num_vertices})")
        e = np.sort(np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
        _, first, inv = np.unique((e[:, 1] << 32) | e[:, 0], return_index=True, return_inverse=True)
        self.num_vertices = int(num_vertices)
        self.edges = e[first]                                    # (M, 2): the midpoint n + k lies on edges[k]
        m = inv.reshape(-1, 3) + num_vertices
        self.faces = np.column_stack([f[:, 0], m[:, 0], m[:, 2], m[:, 0], f[:, 1], m[:, 1], m[:, 2], m[:, 1], f[:, 2], m[:, 0], m[:, 1],
                                      m[:, 2]]).reshape(-1, 3)

    def vertices(self, vertices):
        """(..., V, 3) -> (..., V + M, 3): midpoints (v_a + v_b) / 2, as trimesh's mean over the pair."""
        v = np.asarray(vertices, np.float64)
        mid = (v[..., self.edges[:, 0], :] + v[..., self.edges[:, 1], :]) / 2.0
        return np.concatenate([v, mid], axis=-2)


_SUBDIV_CACHE = {}


def _topology_key(faces, nv):
    f = np.ascontiguousarray(faces, np.int64)
    return (nv, f.shape, hash(f.tobytes()))


def subdivision(faces, num_vertices):
    """The cached SubdivisionTopology of a face array."""
    k = _topology_key(faces, num_vertices)
    if k not in _SUBDIV_CACHE:
        _SUBDIV_CACHE[k] = SubdivisionTopology(faces, num_vertices)
    return _SUBDIV_CACHE[k]


def subdivide(vertices, faces):
    """trimesh.remesh.subdivide(vertices, faces) -> (vertices (V+M,3) fp64, faces (4F,3) int64); the topology is cached per face array."""
    v = np.asarray(vertices, np.float64)
    t = subdivision(faces, v.shape[-2])
    return t.vertices(v), t.faces.copy()


class EdgeTopology:
    """A manifold mesh stored by edges, the layout the flip kernels work on: fv[f, k] corner k, fe[f, k] the edge opposite corner k, fs[f, k]
    the slot of ef[fe[f, k]] that f holds, ef[e] = its two faces (the lower (face, corner) first; -1 on a boundary), ev[e] = (a, b), a < b,
    edges in order of (b, a)."""

    def __init__(self, faces, num_vertices):
        f = np.asarray(faces, np.int64)
        if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0:
            raise EtchHipError(f"faces must be (F,3), got {f.shape}")
        if f.min() < 0 or f.max() >= num_vertices:
            raise EtchHipError(f"face indices must lie in [0, {num_vertices})")
        if np.any((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])):
            raise EtchHipError("degenerate face (a repeated vertex)")
        opp = np.sort(np.stack([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], 1).reshape(-1, 2), axis=1)
        uk, first, inv = np.unique((opp[:, 1] << 32) | opp[:, 0], return_index=True, return_inverse=True)
        E = len(uk)
        cnt = np.bincount(inv, minlength=E)
        if np.any(cnt > 2):
            raise EtchHipError("not a manifold mesh: an edge has more than two faces")
        order = np.argsort(inv, kind="stable")
        slot = np.arange(3 * len(f)) - np.repeat(np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
        ef = np.full((E, 2), -1, np.int64)
        ef[inv[order], slot] = order // 3
        fs = np.empty(3 * len(f), np.int64)
        fs[order] = slot
        self.num_vertices = int(num_vertices)
        self.fv, self.fe, self.fs = f.astype(np.int32), inv.reshape(-1, 3).astype(np.int32), fs.reshape(-1, 3).astype(np.int32)
        self.ef, self.ev = ef.astype(np.int32), opp[first].astype(np.int32)
        self._dev = {}

    @property
    def E(self):
        return len(self.ev)

    def device(self, device):
        d = str(device)
        if d not in self._dev:
            self._dev[d] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (self.fv, self.fe, self.fs, self.ef, self.ev))
        return self._dev[d]


_EDGE_CACHE = {}


def edge_topology(faces, num_vertices):
    k = _topology_key(faces, num_vertices)
    if k not in _EDGE_CACHE:
        _EDGE_CACHE[k] = EdgeTopology(faces, num_vertices)
    return _EDGE_CACHE[k]


def _verts_batch(vertices, device):
    v = torch.as_tensor(vertices, device=device) if not torch.is_tensor(vertices) else vertices.to(device)
    if v.dtype != torch.float64:
        raise EtchHipError(f"vertices must be float64, got {v.dtype}")
    if v.dim() == 2:
        v = v[None]
    if v.dim() != 3 or v.shape[2] != 3:
        raise EtchHipError(f"vertices must be (V,3) or (B,V,3), got {tuple(v.shape)}")
    return v.contiguous()


def heat_geodesic(vertices, faces, sources, t_coef=1.0, laplacian="intrinsic_delaunay", device=None, return_info=False, **solver):
    """pp3d.MeshHeatMethodDistanceSolver(V, F, t_coef, use_robust=(laplacian == "intrinsic_delaunay")).compute_distance(s) for every s in
    `sources`: vertices (B,V,3) | (V,3) fp64, faces (F,3) -> distances (B,S,V) fp64 on the device.  `return_info` adds the solver's dict
    (iterations per column, flips per body)."""
    if laplacian not in LAPLACIANS:
        raise EtchHipError(f"laplacian must be one of {LAPLACIANS}, got {laplacian!r}")
    dev = _device(device)
    v = _verts_batch(vertices, dev)
    topo = edge_topology(faces, v.shape[1])
    src = torch.as_tensor(np.asarray(sources, np.int64).reshape(-1)).to(torch.int32).to(dev).contiguous()
    if src.numel() == 0:
        raise EtchHipError("sources must not be empty")
    r = ops.geodesic_heat(v, topo.device(dev), src, t_coef=t_coef, intrinsic_delaunay=laplacian == "intrinsic_delaunay", want_min=False, **solver)
    return (r["dist"], r) if return_info else r["dist"]


def marker_fields(body_vertices, body_faces, markerset, t_coef=1.0, laplacian="intrinsic_delaunay", device=None, keep_distances=False, **solver):
    """GT_dataloader.py:129-139 for a batch of bodies: subdivide, one heat-method column per marker (markerset values in order) ->
    dict with min_dist (B,V') fp64 and label (B,V') int64 (the first marker on a tie) per subdivided vertex, vertices (B,V',3) fp64 (the
    subdivided bodies, on the device), iters (B,S,2), flips (B,) and, with keep_distances, dist (B,S,V')."""
    if laplacian not in LAPLACIANS:
        raise EtchHipError(f"laplacian must be one of {LAPLACIANS}, got {laplacian!r}")
    dev = _device(device)
    bv = np.asarray(body_vertices.cpu() if torch.is_tensor(body_vertices) else body_vertices, np.float64)
    if bv.ndim == 2:
        bv = bv[None]
    sub = subdivision(body_faces, bv.shape[1])
    sv = torch.from_numpy(np.ascontiguousarray(sub.vertices(bv))).to(dev)
    topo = edge_topology(sub.faces, sv.shape[1])
    vids = list(markerset.values()) if isinstance(markerset, dict) else list(markerset)
    src = torch.as_tensor(np.asarray(vids, np.int64)).to(torch.int32).to(dev).contiguous()
    r = ops.geodesic_heat(sv, topo.device(dev), src, t_coef=t_coef, intrinsic_delaunay=laplacian == "intrinsic_delaunay", want_min=True, **solver)
    out = {"min_dist": r["dmin"], "label": r["label"].long(), "vertices": sv, "iters": r["iters"], "flips": r["flips"]}
    if keep_distances:
        out["dist"] = r["dist"]
    return out


def convert_geodesic_distances_to_confidence(geodesic_distances):
    """GT_dataloader.py:56-59: exp(-10 d) (numpy or torch)."""
    sharpness_factor = 10.0
    if torch.is_tensor(geodesic_distances):
        return torch.exp(-sharpness_factor * geodesic_distances)
    return np.exp(-sharpness_factor * geodesic_distances)


def geodesic_targets(sample_points, vectors, min_dist, label, sub_vertices, device=None):
    """GT_dataloader.py:141-148 for one body: inner = sample - vector; its nearest subdivided vertex (ops.nn_bidir: exact fp32 distances, the
    lowest index on a tie) gives labels (N,) int64 and confidences (N,1) = exp(-10 min_dist) -> numpy (confidences fp64, labels int64).
    min_dist (V') / label (V') / sub_vertices (V',3) as one body's slice of marker_fields."""
    dev = _device(device)
    inner = torch.as_tensor(np.asarray(sample_points, np.float64) - np.asarray(vectors, np.float64), device=dev)
    sv = torch.as_tensor(sub_vertices, device=dev).to(torch.float64)
    idx, _, _, _ = ops.nn_bidir(inner.float()[None].contiguous(), sv.float()[None].contiguous())
    j = idx[0].long()
    d = torch.as_tensor(min_dist, device=dev)[j]
    lab = torch.as_tensor(label, device=dev)[j].long()
    return convert_geodesic_distances_to_confidence(d).reshape(-1, 1).cpu().numpy(), lab.cpu().numpy()
