"""Containment: is the fitted body inside the scan it is supposed to be under?

The inside/outside test is the generalised winding number (Jacobson et al. 2013): the sum over the scan's faces of the signed solid angle
each subtends at the query, over 4 pi.  It is 1 inside a closed surface, 0 outside, and degrades smoothly at the holes, non-manifold edges
and self-intersections real scans have, where ray parity does not.  A point counts as INSIDE where |w| >= 0.5: the absolute value makes a
scan whose faces are wound inward (w = -1 inside) read the same as one wound outward.  A single-view scan is half a shell (w ~ 0.5 behind
it everywhere): it has no inside, and the commands refuse the combination.

Every function takes the scans as a list of Mesh (vertices, faces; packed and sent to the device here) or as the tuple pack_scans returns,
already on the device, and the queries in the frame of the scans' vertices.

A scan that is a CLOUD comes as the cloud.OrientedCloud that cloud.surface builds -- positions, oriented normals and areas --
wherever a mesh is accepted.  Its winding number is the dipole sum of Barill et al. (2018) over the rows, the same |w| >= 0.5 convention
holds, and "the surface" is the nearest ROW: a distance to it overestimates the distance to the sampled surface by up to the sampling
distance, and a body pulled to it ends within one sampling distance of the surface."""
import numpy as np
import torch

from . import ops
from .mesh_io import pack_meshes


def pack_scans(meshes, device="cuda", center=None):
    """A list of Mesh -> (verts (sum V,3) fp32, faces (sum F,3) int32, vert_offsets (B+1), face_offsets (B+1) int32, max_faces) on the device,
    what the ops of csrc/containment.hip take.  center (B,3): subtracted from each scan's vertices in fp64 before the rounding to fp32."""
    v, f, vo, fo = pack_meshes(meshes)
    if center is not None:
        c = np.asarray(center, np.float64).reshape(len(meshes), 3)
        v = v - np.repeat(c, np.diff(vo), axis=0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    return t(v, torch.float32), t(f, torch.int32), t(vo, torch.int32), t(fo, torch.int32), int(np.diff(fo).max())


def _scans(meshes, device):
    if isinstance(meshes, tuple) and len(meshes) == 5 and torch.is_tensor(meshes[0]):
        return meshes
    return pack_scans(list(meshes), device)


def _is_cloud(scans):
    return all(hasattr(scans, a) for a in ("pos", "moment", "cap", "offsets", "max_rows"))


def _points(queries, device=None):
    q = torch.as_tensor(queries)
    q = q.to(device=device if device is not None else (q.device if q.is_cuda else "cuda"), dtype=torch.float32).contiguous()
    if q.dim() == 2:
        q = q[None]
    if q.dim() != 3 or q.shape[2] != 3:
        raise ValueError(f"queries must be (B,Q,3), got {tuple(q.shape)}")
    return q


def winding_number(meshes, queries, lengths=None):
    """w (B,Q) fp32 of scan b at queries (B,Q,3); lengths (B,) for ragged query sets (padding gets 0).  meshes: meshes, or an OrientedCloud."""
    q = _points(queries, meshes.pos.device if _is_cloud(meshes) else None)
    if _is_cloud(meshes):
        return ops.cloud_winding_number(meshes, q, lengths, want_nearest=False)[0]
    return ops.mesh_winding_number(_scans(meshes, q.device), q, lengths)


def signed_distance(meshes, queries, lengths=None):
    """sign(|w| - 0.5) sqrt(d2): the distance to the scan's surface, NEGATIVE outside the scan (positive inside: how deep under the garment),
    (B,Q) fp32; padding gets 0.  d2 is the exact closest point's (ops.ragged_mesh_closest); a NaN w counts as inside.  With an OrientedCloud
    d2 is the nearest row's, from the same pass as w: the distance then overestimates by up to the sampling distance."""
    q = _points(queries, meshes.pos.device if _is_cloud(meshes) else None)
    if _is_cloud(meshes):
        w, _, d2 = ops.cloud_winding_number(meshes, q, lengths)
        return torch.where(w.abs() < 0.5, -d2.sqrt(), d2.sqrt())
    scans = _scans(meshes, q.device)
    w = ops.mesh_winding_number(scans, q, lengths)
    _, _, d2 = ops.ragged_mesh_closest(scans, q, lengths)
    return torch.where(w.abs() < 0.5, -d2.sqrt(), d2.sqrt())


def containment_metrics(meshes, body_verts):
    """Per scan: how much of the body (B,V,3, in the scans' frame) lies outside its scan -> a list of dicts {outside_share: the share of the
    vertices with |w| < 0.5, protrusion_rms_mm, protrusion_max_mm: the distance to the scan's surface over those vertices (0 with none)}.
    With an OrientedCloud the distance is to the nearest row (an overestimate by up to the sampling distance)."""
    v = _points(body_verts, meshes.pos.device if _is_cloud(meshes) else None)
    if _is_cloud(meshes):
        w, face, d2 = ops.cloud_winding_number(meshes, v)
    else:
        scans = _scans(meshes, v.device)
        w = ops.mesh_winding_number(scans, v)
        face, _, d2 = ops.ragged_mesh_closest(scans, v)
    out = (w.abs() < 0.5) & (face >= 0)
    n = out.sum(1).double()
    d2o = torch.where(out, d2.double(), torch.zeros((), dtype=torch.float64, device=v.device))
    rms = torch.where(n > 0, (d2o.sum(1) / n.clamp(min=1)).sqrt(), torch.zeros_like(n)) * 1e3
    mx = d2o.max(1).values.sqrt() * 1e3
    share = n / v.shape[1]
    return [dict(outside_share=float(s), protrusion_rms_mm=float(r), protrusion_max_mm=float(m)) for s, r, m in zip(share.cpu(), rms.cpu(), mx.cpu())]
