"""Dense surface refinement: fit the body SURFACE to all of stage 1's predicted inner points.

The reference planned this term (src/models/fit_SMPL.py:84 `use_point_mesh_distance = False`, :106 its weight 1e2;
src/utils/customized_losses.py:29 `my_point_mesh_face_distance`) and never switched it on.  Here the point -> face half is exact: the closest
point of the mesh to every inner point by Ericson's region test (csrc/surface_fit.hip), the SQUARED distance (smooth at 0: a point lying on
the mesh has a zero gradient), no epsilons.  `point_mesh_face_distance` is that distance as an autograd Function; `fit_surface` is the Adam
refinement of pose, betas and translation on it, the whole schedule one queue of HIP kernels.  The face -> point half of the reference
function is not built: the fit does not use it."""
import numpy as np
import torch

from .. import ops
from .chamfer_refine import _bm_tables, _lengths_of, _prior_tensors, init_from_fit  # noqa: F401  (init_from_fit: the init of fit_surface too)


def _faces_tensor(faces, device):
    if torch.is_tensor(faces):
        return faces.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(device)


class _PointMesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, points, faces, lengths, weights, trunc, point_reduction, batch_reduction):
        B = verts.shape[0]
        face, bary, d2 = ops.point_mesh_closest(points, verts, faces, lengths)
        terms, _, _ = ops.point_mesh_energy_grad(points, verts, faces, face, bary, d2, weights, trunc, lengths, want_verts=False)
        S1, S0 = terms[:, 0], terms[:, 1]
        per = torch.where(S0 > 0, S1 / S0.clamp(min=1e-300), torch.zeros_like(S1)) if point_reduction == "mean" else S1
        out = per.sum() if batch_reduction == "sum" else per.sum() / B if batch_reduction == "mean" else per
        ctx.save_for_backward(verts, points, faces, face, bary, d2, lengths, weights)
        ctx.trunc, ctx.point_reduction, ctx.batch_reduction = trunc, point_reduction, batch_reduction
        return out.to(torch.float32)

    @staticmethod
    def backward(ctx, go):
        verts, points, faces, face, bary, d2, lengths, weights = ctx.saved_tensors
        B = verts.shape[0]
        gb = go.expand(B) if ctx.batch_reduction is None else go.expand(B) / (B if ctx.batch_reduction == "mean" else 1)
        _, g, gp = ops.point_mesh_energy_grad(points, verts, faces, face, bary, d2, weights, ctx.trunc, lengths, coef=gb.to(torch.float32).contiguous(),
                                              normalize=ctx.point_reduction == "mean", want_verts=ctx.needs_input_grad[0],
                                              want_points=ctx.needs_input_grad[1])
        return g, gp, None, None, None, None, None, None


def point_mesh_face_distance(verts, faces, points, lengths=None, weights=None, trunc=None, point_reduction="mean", batch_reduction="mean"):
    """The point -> face half of the reference's point-mesh distance, squared and exact: per scan sum_i w_i m_i d2_i / sum_i w_i m_i
    ("mean") or sum_i w_i m_i d2_i ("sum"), d2_i = the squared distance of points[b, i] to the closest point of the mesh (verts[b], faces),
    m_i = [d2_i <= trunc^2] (trunc None: no mask), w_i = weights (B,N) >= 0 or 1.  verts (B,V,3), points (B,N,3) fp32 on the GPU, faces
    (F,3) shared by the batch, lengths (B,) for ragged point sets; batch_reduction "mean" | "sum" | None.  Gradients flow to verts and
    points, with the correspondences held fixed (the true gradient, by the envelope argument)."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be "mean" or "sum"')
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be "mean", "sum" or None')
    if verts.dim() != 3 or points.dim() != 3 or verts.shape[2] != 3 or points.shape[2] != 3 or verts.shape[0] != points.shape[0]:
        raise ValueError("verts and points must be (B,V,3) and (B,N,3)")
    verts, points = verts.contiguous(), points.contiguous()
    nl = _lengths_of(lengths, points.shape[0], points.shape[1], points.device)
    if weights is not None:
        weights = torch.as_tensor(weights).to(device=points.device, dtype=torch.float32).contiguous()
    return _PointMesh.apply(verts, points, _faces_tensor(faces, verts.device), nl, weights, -1.0 if trunc is None else float(trunc), point_reduction,
                            batch_reduction)


def fit_surface(body_model, inner_points, init, markers=None, valid=None, marker_vids=None, weights=None, lengths=None, prior=None, iterations=200,
                lr=2e-2, w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05, optimize_scale=False, want_trace=False, scan=None,
                w_contain=1e2, contain_every=10):
    """Refine a fitted body so that its surface passes through the inner points.  inner_points (B,N,3) (GPU tensor or array; lengths (B,) for
    ragged scans, weights (B,N) >= 0 optional), init = fit_cham's dict {pose (B,3J), beta (B,NB), trans (B,3), scale (B,1)}
    (chamfer_refine.init_from_fit), markers (B,M,3) with valid (B,M) and marker_vids (M,): the aggregated markers of stage 2, optional;
    prior as fit_cham's.  Per scan, Adam (fit_cham's schedule) on
        w_dense sum_i w_i m_i d2_i / sum_i w_i m_i + w_marker mean_valid (v_vid(m) - t_m)^2 + w_beta mean(beta^2) + w_prior prior(pose[3:]),
    d2_i the squared distance to the body surface, m_i = [d2_i <= trunc^2] (trunc None or < 0: no mask); correspondences are recomputed at every
    iteration.  scale keeps its initial value unless optimize_scale.  Every scan follows the trajectory it would follow alone.
    Returns (vertices (B,V,3) numpy, params) with params of fit_cham's shape: {loss, loss_per_scan, pose, beta, trans, scale, joints, verts},
    tensors on the GPU; with want_trace also params["loss_trace"] (B, iterations, 4): the dense, marker, beta and prior terms.
    scan: the scans the bodies lie under, in the frame of the inner points -- a list of B Mesh or containment.pack_scans' tuple.
    The loss gains w_contain (sum_v o_v |v - c_v|^2) / V over the body's vertices, o_v = the vertex is outside its scan (|winding number| <
    0.5), c_v its closest point on the scan, both recomputed every contain_every iterations and held in between.  w_contain = 1e2 is w_dense's
    value (both terms are mean squared metres): a default, not a tuned optimum.  scan may also be a cloud.OrientedCloud: c_v is then
    the nearest ROW of the cloud, so the pull ends within one sampling distance of the surface.  params gains "outside_share" (B,) float64, the share of the
    final vertices outside, and the trace a fifth column.  scan=None is the refinement without the term, through the entry point it always used."""
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    if scan is not None and contain_every < 1:
        raise ValueError("contain_every must be >= 1")
    dev = torch.device("cuda", torch.cuda.current_device()) if not torch.is_tensor(inner_points) or not inner_points.is_cuda else inner_points.device
    pts = torch.as_tensor(inner_points).to(device=dev, dtype=torch.float32).contiguous()
    if pts.dim() == 2:
        pts = pts[None]
    B, N = pts.shape[0], pts.shape[1]
    if N == 0:
        raise ValueError("fit_surface needs inner points")
    db = _bm_tables(body_model, dev)
    nj, nb = db.nj, db.nb
    f = lambda k, n: torch.as_tensor(init[k]).to(device=dev, dtype=torch.float32).reshape(B, n)
    params = torch.cat([f("pose", 3 * nj), f("beta", nb), f("trans", 3), f("scale", 1)], 1).contiguous()
    nl = _lengths_of(lengths, B, N, dev)
    mk = None
    if markers is not None:
        if valid is None or marker_vids is None:
            raise ValueError("markers need their valid mask and marker_vids")
        mk = (np.asarray(marker_vids, np.int64).reshape(-1), markers, torch.as_tensor(valid).to(dev).to(torch.float32))
    if weights is not None:
        weights = torch.as_tensor(weights).to(device=dev, dtype=torch.float32).contiguous()
    faces = body_model.__dict__.setdefault("_etch_faces", {})
    if str(dev) not in faces:
        faces[str(dev)] = _faces_tensor(body_model.faces, dev)
    pr = _prior_tensors(prior, nj, dev)
    kw = dict(w_dense=w_dense, w_marker=w_marker, w_beta=w_beta, w_prior=w_prior, trunc=-1.0 if trunc is None else trunc, optimize_scale=optimize_scale,
              nj=nj, nb=nb, n_extra=db.n_extra, want_trace=want_trace)
    if scan is None:
        verts, joints, loss, tr = ops.smpl_surface_refine(db.lbs_consts, faces[str(dev)], pts, params, nl, weights, mk, pr, iterations, lr, **kw)
    else:
        from ..containment import _is_cloud, _scans, containment_metrics
        if _is_cloud(scan):                                 # a cloud.OrientedCloud: the row target, one pass per refresh
            scans = scan
            verts, joints, loss, tr = ops.smpl_surface_refine_contain_cloud(db.lbs_consts, faces[str(dev)], pts, params, scans, nl, weights, mk, pr,
                                                                            iterations, lr, w_contain=w_contain, contain_every=contain_every, **kw)
        else:
            scans = _scans(scan, dev)
            verts, joints, loss, tr = ops.smpl_surface_refine_contain(db.lbs_consts, faces[str(dev)], pts, params, scans, nl, weights, mk, pr, iterations, lr,
                                                                      w_contain=w_contain, contain_every=contain_every, **kw)
    out = dict(loss=loss.sum(), loss_per_scan=loss, pose=params[:, :3 * nj], beta=params[:, 3 * nj:3 * nj + nb],
               trans=params[:, 3 * nj + nb:3 * nj + nb + 3], scale=params[:, 3 * nj + nb + 3:], joints=joints, verts=verts)
    if want_trace:
        out["loss_trace"] = tr
    if scan is not None:
        out["outside_share"] = torch.tensor([m["outside_share"] for m in containment_metrics(scans, verts)], dtype=torch.float64)
    return verts.cpu().numpy(), out
