"""SMPL+D registration: the SMPL topology deformed onto the scan by per-vertex offsets D in the rest pose, and re-posing of the registered
body and of the scan bound to it.  verts(D) = base + R D with the skinning frames of the fitted parameters; D minimises

    w_s2m mean_i d(x_i, verts) + w_m2s mean_v m_v d(verts_v, scan) + lambda_s mean_(u,v) |D_u - D_v|^2 + lambda_m mean_v |D_v|^2

by Adam, the whole schedule one queue of HIP kernels (csrc/register.hip on top of chamfer_fit.hip's neighbour pass).  Re-posing a scan point
is the arithmetic of the reference's animate.py:172-206 with the skinning weights of the registered surface at the point's closest point;
animate.py's weight transfer (distance / normal thresholds, inpainting, clean_mesh_numpy) is not built: the registered surface lies on the
scan, so every scan vertex has a close point that carries weights."""
import numpy as np
import torch

from .. import ops
from .chamfer_refine import _bm_tables, _lengths_of


def mesh_edges(faces, num_verts):
    """The unique undirected edges u < v of the rows of faces (F,3) (a face listed twice or in both orientations counts once, u = v is
    dropped) as neighbour lists: -> nbr_ptr (V+1) int32, nbr_idx (2 |E|) int32 with the neighbours of v at nbr_idx[nbr_ptr[v]:nbr_ptr[v+1]]
    in ascending order, and |E|.  A vertex in no face has no neighbour.  Host numpy."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(num_verts)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError(f"face indices must lie in [0, {V})")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.sort(e[e[:, 0] != e[:, 1]], axis=1)
    e = np.unique(e, axis=0).reshape(-1, 2)
    both = np.concatenate([e, e[:, ::-1]])
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(both[:, 0], minlength=V), out=ptr[1:])
    return ptr.astype(np.int32), np.ascontiguousarray(both[:, 1], np.int32), len(e)


def _edges_of(body_model, device):
    """mesh_edges of the body's faces, built once per BodyModel; the device copies once per device (cached like _etch_device).
    -> nbr_ptr, nbr_idx on the device, |E|."""
    cache = body_model.__dict__.setdefault("_etch_edges", {})
    if "host" not in cache:
        cache["host"] = mesh_edges(body_model.faces, body_model.num_verts)
    key = str(device)
    if key not in cache:
        ptr, idx, n = cache["host"]
        cache[key] = (torch.from_numpy(ptr).to(device), torch.from_numpy(idx).to(device), n)
    return cache[key]


def _faces_of(body_model, device):
    """The body's faces (F,3) int32 on the device, copied once per device."""
    cache = body_model.__dict__.setdefault("_etch_faces", {})
    key = str(device)
    if key not in cache:
        cache[key] = torch.from_numpy(np.ascontiguousarray(body_model.faces, np.int32)).to(device)
    return cache[key]


def smooth_schedule(l0, l1, iters):
    """The smoothness weight of every iteration, stiff first and loose last: l0 (l1 / l0)^(i / (iters - 1)) in fp64 (iters = 1: l0)."""
    l0, l1, iters = float(l0), float(l1), int(iters)
    if iters < 1:
        raise ValueError("iterations must be >= 1")
    if not (np.isfinite(l0) and np.isfinite(l1) and l0 >= 0.0 and l1 >= 0.0) or ((l0 == 0.0) != (l1 == 0.0)):
        raise ValueError("smooth_w must be two finite weights, both > 0 or both 0")
    if iters == 1 or l0 == 0.0:
        return np.full(iters, l0, np.float64)
    return l0 * (l1 / l0) ** (np.arange(iters, dtype=np.float64) / (iters - 1))


def pack_params(params, nj, nb, device, B=None):
    """fit_cham's `init` dict {pose, beta, trans, scale} or the packed tensor -> (B, 3 nj + nb + 4) fp32 on the device."""
    P = 3 * nj + nb + 4
    if isinstance(params, dict):
        n = B if B is not None else int(torch.as_tensor(params["pose"]).reshape(-1, 3 * nj).shape[0])
        f = lambda k, w: torch.as_tensor(params[k]).to(device=device, dtype=torch.float32).reshape(n, w)
        p = torch.cat([f("pose", 3 * nj), f("beta", nb), f("trans", 3), f("scale", 1)], 1)
    else:
        p = torch.as_tensor(params).to(device=device, dtype=torch.float32)
        if p.dim() == 1:
            p = p[None]
    if p.dim() != 2 or p.shape[1] != P or (B is not None and p.shape[0] != B):
        raise ValueError(f"params must be ({'B' if B is None else B}, {P}) = pose | beta | trans | scale for this body model, got {tuple(p.shape)}")
    return p.contiguous()


def register_smpld(body_model, scan, params, scan_lengths=None, iterations=300, lr=1e-3, w_s2m=1.0, w_m2s=1.0, smooth_w=(10.0, 0.1), mag_w=0.0,
                   trunc=0.05, offsets=None, want_trace=False):
    """Register SMPL+D onto scan (B,N,3) (scan_lengths (B,) for ragged scans) from the fitted params (fit_cham's `init` dict, as
    chamfer_refine.init_from_fit gives it, or the packed (B, 3 nj + nb + 4) tensor).  smooth_w = (first, last) smoothness weight, a geometric
    schedule; trunc (metres, None = off) drops the body -> scan term of vertices further than that from the scan (holes); offsets = a start
    other than zero.  -> {offsets (B,V,3) in the rest pose, verts (B,V,3), energy (B,4) = the four terms at the result, params (B,P) packed[,
    trace (B,iterations,4)]}, tensors on the GPU.  The defaults were chosen on a CPU prototype on the synthetic body, not on real scans."""
    dev = torch.device("cuda", torch.cuda.current_device()) if not torch.is_tensor(scan) or not scan.is_cuda else scan.device
    scan = torch.as_tensor(scan).to(device=dev, dtype=torch.float32).contiguous()
    if scan.dim() == 2:
        scan = scan[None]
    if scan.dim() != 3 or scan.shape[2] != 3:
        raise ValueError(f"scan must be (B,N,3), got {tuple(scan.shape)}")
    B, N = scan.shape[0], scan.shape[1]
    lam = smooth_schedule(smooth_w[0], smooth_w[1], iterations)
    db = _bm_tables(body_model, dev)
    p = pack_params(params, db.nj, db.nb, dev, B)
    sl = _lengths_of(scan_lengths, B, N, dev)
    if N == 0 or (sl is not None and bool((sl == 0).any())):
        raise ValueError("register_smpld needs at least one scan point per scan")
    if offsets is None:
        D = torch.zeros((B, db.V, 3), dtype=torch.float32, device=dev)
    else:
        D = torch.as_tensor(offsets).to(device=dev, dtype=torch.float32).reshape(B, db.V, 3).clone().contiguous()
    ptr, idx, n_edges = _edges_of(body_model, dev)
    base, R, _ = ops.smpl_skin_frames(db.lbs_consts, p, nj=db.nj, nb=db.nb)
    verts, energy, trace = ops.smpld_register(base, R, D, scan, ptr, idx, n_edges, lam, scan_lengths=sl, w_s2m=w_s2m, w_m2s=w_m2s, lambda_m=mag_w,
                                              trunc=trunc, lr=lr, want_trace=want_trace)
    out = dict(offsets=D, verts=verts, energy=energy, params=p)
    if want_trace:
        out["trace"] = trace
    return out


def repose(body_model, params_new, offsets):
    """The registered body at other parameters: verts (B,V,3) = base(params_new) + R(params_new) offsets, by the registration's own kernels."""
    if not torch.is_tensor(offsets) or not offsets.is_cuda:
        raise ValueError("offsets must be the GPU tensor register_smpld returned")
    db = _bm_tables(body_model, offsets.device)
    D = offsets.to(torch.float32).reshape(-1, db.V, 3).contiguous()
    p = pack_params(params_new, db.nj, db.nb, offsets.device, D.shape[0])
    base, R, _ = ops.smpl_skin_frames(db.lbs_consts, p, nj=db.nj, nb=db.nb)
    return ops.smpld_apply(base, R, D)


def bind_scan(reg_verts, faces, points):
    """Bind points (P,3) to the registered surface reg_verts (V,3): -> face (P) int32, bary (P,3) fp64 of each point's closest point
    (ops.closest_point_on_mesh: fp64, the lowest face among equal distances)."""
    dev = reg_verts.device
    v = reg_verts.to(torch.float64).reshape(-1, 3).contiguous()
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device=dev, dtype=torch.int32).contiguous()
    pts = torch.as_tensor(points).to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    face, bary, _, _ = ops.closest_point_on_mesh(pts, v, f)
    return face, bary


def carry_scan(body_model, params, params_new, face, bary, points):
    """Carry bound points from the pose of params to the pose of params_new (one scan: packed (P,) / (1,P) tensors or fit_cham-style dicts):
    animate.py:172-206 with w~ = the barycentric mix of the skinning weights at the bound face.  -> (P,3) fp64 on the GPU."""
    dev = face.device
    db = _bm_tables(body_model, dev)
    p0, p1 = pack_params(params, db.nj, db.nb, dev, 1), pack_params(params_new, db.nj, db.nb, dev, 1)
    _, _, A = ops.smpl_skin_frames(db.lbs_consts, torch.cat([p0, p1]), nj=db.nj, nb=db.nb)
    faces = _faces_of(body_model, dev)
    if face.numel() and (int(face.min()) < 0 or int(face.max()) >= faces.shape[0]):
        raise ValueError(f"face must index the body's {faces.shape[0]} faces")
    pts = torch.as_tensor(points).to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    k = 3 * db.nj + db.nb
    return ops.skin_carry(pts, face.contiguous(), bary.to(torch.float64).contiguous(), faces, db.lbs_consts[3], A[0].contiguous(), A[1].contiguous(),
                          p0[0, k:].contiguous(), p1[0, k:].contiguous())


def _edge_lengths_and_areas(v, f):
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e0, e1, e2 = (v1 - v0).norm(dim=1), (v2 - v1).norm(dim=1), (v0 - v2).norm(dim=1)
    s = (e0 + e1 + e2) / 2                                               # Heron's formula
    return torch.stack([e0, e1, e2], 1), torch.sqrt(torch.clamp(s * (s - e0) * (s - e1) * (s - e2), min=0))


def filter_faces(verts_raw, verts_new, faces):
    """animate.py:30-53: the faces of a carried mesh that kept their shape -- every edge between 0.3 and 2.0 times its raw length and the
    area between 0.1 and 4.0 times its raw area (ratios against raw + 1e-8, strict comparisons).  -> (F,) bool, on the tensors' device."""
    f = torch.as_tensor(faces, device=verts_raw.device).long()
    raw_e, raw_a = _edge_lengths_and_areas(verts_raw, f)
    new_e, new_a = _edge_lengths_and_areas(verts_new.to(verts_raw.dtype), f)
    er, ar = new_e / (raw_e + 1e-8), new_a / (raw_a + 1e-8)
    return ((er > 0.3) & (er < 2.0)).all(1) & (ar > 0.1) & (ar < 4.0)
