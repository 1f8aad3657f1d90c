"""MI355X counterpart of scripts/experiment_scripts/chamfer_refine.py: `fit_cham` refines a fitted SMPL body so that its surface lies on
the scan, by Adam on pose, betas, translation and a global scale against the chamfer distance between all mesh vertices and the scan.
The script needs pytorch3d's knn_points and autograd through smplx; here the whole schedule is one queue of HIP kernels
(csrc/chamfer_fit.hip: the two-way nearest-neighbour pass, the full-mesh LBS vector-Jacobian product, Adam).

Divergences from the script, all deliberate: it refines a batch (every scan follows exactly the trajectory it would follow alone and
the returned loss is the sum of the per-scan losses); the GMM pose prior is optional (prior=None drops the term); `scale` is optimised,
as the script's OptimizationSMPL declares it."""
import numpy as np
import torch

from .. import ops
from ..utils.body_model import BodyModel
from .fit_SMPL import _device_body


def _bm_tables(body_model, device):
    if not isinstance(body_model, BodyModel):
        raise TypeError("body_model must be an etch_amd.utils.body_model.BodyModel")
    par = np.asarray(body_model.parents)
    if not all(0 <= par[j] < j for j in range(1, len(par))):
        raise ValueError("the refinement needs a kinematic tree whose parents precede their children")
    return _device_body(body_model, (), device)


def _lengths_of(lengths, B, n, device):
    if lengths is None:
        return None
    t = torch.as_tensor(lengths, device=device).to(torch.int32)
    if t.shape != (B,) or bool((t < 0).any()) or bool((t > n).any()):
        raise ValueError(f"lengths must be ({B},) in [0, {n}]")
    return t


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, xl, yl, single, point_reduction, batch_reduction):
        B, N, V = x.shape[0], x.shape[1], y.shape[1]
        ixy, dxy, iyx, dyx = ops.nn_bidir(x, y, xl, yl)
        nx = xl.to(torch.float32) if xl is not None else torch.full((B,), float(N), device=x.device)
        ny = yl.to(torch.float32) if yl is not None else torch.full((B,), float(V), device=x.device)
        # per-point weight of every distance term in the per-scan value (padding distances are 0)
        wx = 1.0 / nx.clamp(min=1) if point_reduction == "mean" else torch.ones_like(nx)
        wy = 1.0 / ny.clamp(min=1) if point_reduction == "mean" else torch.ones_like(ny)
        cx = dxy.sum(1) * wx
        cy = dyx.sum(1) * wy
        per = cx if single else cx + cy
        out = per.sum() if batch_reduction == "sum" else per.sum() / B if batch_reduction == "mean" else per
        ctx.save_for_backward(x, y, ixy, iyx, wx, wy, xl, yl)
        ctx.single, ctx.batch_reduction = single, batch_reduction
        return out

    @staticmethod
    def backward(ctx, go):
        x, y, ixy, iyx, wx, wy, xl, yl = ctx.saved_tensors
        B = x.shape[0]
        gb = go.expand(B) if ctx.batch_reduction is None else go.expand(B) / (B if ctx.batch_reduction == "mean" else 1)
        gb = gb.to(torch.float32)
        gx, gy = ops.chamfer_grad(x, y, ixy, iyx, (gb * wx).contiguous(), None if ctx.single else (gb * wy).contiguous(), xl, yl,
                                  want_x=ctx.needs_input_grad[0], want_y=ctx.needs_input_grad[1])
        return gx, gy, None, None, None, None, None


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, single_directional=False, point_reduction="mean", batch_reduction="mean"):
    """pytorch3d.loss.chamfer_distance for the subset the refinement uses: L2, no normals, no weights.  x (B,N,3), y (B,M,3) fp32 on the
    GPU; point_reduction "mean" | "sum", batch_reduction "mean" | "sum" | None.  Returns (loss, None) like pytorch3d.  Exact brute-force
    neighbours (ties -> the lowest index); the backward runs on the GPU too."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be "mean" or "sum"')
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be "mean", "sum" or None')
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[0] != y.shape[0]:
        raise ValueError("x and y must be (B,N,3) and (B,M,3)")
    x, y = x.contiguous(), y.contiguous()
    xl = _lengths_of(x_lengths, x.shape[0], x.shape[1], x.device)
    yl = _lengths_of(y_lengths, y.shape[0], y.shape[1], y.device)
    return _Chamfer.apply(x, y, xl, yl, bool(single_directional), point_reduction, batch_reduction), None


_BIDIR = {"both": 0, "partial": 1, "clutter": -1}


def _prior_tensors(prior, nj, device):
    if prior is None:
        return None
    if nj != 24:
        raise ValueError("the GMM pose prior is defined for the 69-dim SMPL body pose only")
    if isinstance(prior, (tuple, list)):
        prior = dict(zip(("means", "precisions", "nll_weights"), prior))
    get = (lambda k: prior[k]) if isinstance(prior, dict) else (lambda k: getattr(prior, k))
    t = lambda a: torch.as_tensor(a).to(device=device, dtype=torch.float32).contiguous()
    means, prec, w = t(get("means")), t(get("precisions")), t(get("nll_weights")).reshape(-1)
    G = w.shape[0]
    if means.shape != (G, 69) or prec.shape != (G, 69, 69) or not 1 <= G <= 16:
        raise ValueError("prior: means (G,69), precisions (G,69,69), nll_weights (G,) with 1 <= G <= 16")
    return means, prec, w


def init_from_fit(dev_fit):
    """The `init` dict of fit_cham from fit_smpl_device's result: pose = global orient | body pose, beta, trans = the LM translation,
    scale = 1 -- so the refinement's first mesh is exactly the LM mesh."""
    x = dev_fit["x"]
    nj, nb = dev_fit.get("nj", 24), dev_fit.get("nb", 10)
    npose = 3 * (nj - 1)
    return dict(pose=torch.cat([x[:, npose + nb:npose + nb + 3], x[:, :npose]], 1), beta=x[:, npose:npose + nb], trans=x[:, npose + nb + 3:npose + nb + 6],
                scale=torch.ones((x.shape[0], 1), dtype=x.dtype, device=x.device))


def fit_cham(body_model, vertices_scan, init, prior=None, bidir=0, iterations=500, lr=2e-2, scan_lengths=None, want_trace=False):
    """chamfer_refine.py:fit_cham, batched.  vertices_scan (B,N,3) (GPU tensor or array; scan_lengths (B,) for ragged scans), init =
    {pose (B,3J), beta (B,NB), trans (B,3), scale (B,1)}, prior = None, an object / dict with the MaxMixturePrior buffers (means,
    precisions, nll_weights) or that triple, bidir 0 (both directions), 1 ("Partial": scan -> body) or -1 ("Clutter": body -> scan), or the names
    "both" / "partial" / "clutter".  Returns (vertices (B,V,3) numpy of the final parameters, params) with params = {loss (the summed
    loss of the last forward), loss_per_scan, beta, pose, trans, scale, joints (B,J',3) without trans and scale}, tensors on the GPU;
    with want_trace also params["loss_trace"] (B, iterations)."""
    bidir = _BIDIR.get(bidir, bidir)
    if bidir not in (0, 1, -1):
        raise ValueError("bidir must be 0, 1, -1 (or both / partial / clutter)")
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    dev = torch.device("cuda", torch.cuda.current_device()) if not torch.is_tensor(vertices_scan) or not vertices_scan.is_cuda else vertices_scan.device
    scan = torch.as_tensor(vertices_scan).to(device=dev, dtype=torch.float32).contiguous()
    if scan.dim() == 2:
        scan = scan[None]
    B, N = scan.shape[0], scan.shape[1]
    db = _bm_tables(body_model, dev)
    nj, nb = db.nj, db.nb
    f = lambda k, n: torch.as_tensor(init[k]).to(device=dev, dtype=torch.float32).reshape(B, n)
    params = torch.cat([f("pose", 3 * nj), f("beta", nb), f("trans", 3), f("scale", 1)], 1).contiguous()
    sl = _lengths_of(scan_lengths, B, N, dev)
    if N == 0 or (sl is not None and bool((sl == 0).any())):
        # an empty scan has S = 0: d sqrt(S)/dS = inf and every gradient NaN (as autograd through sqrt at 0)
        raise ValueError("fit_cham needs at least one scan point per scan")
    pr = _prior_tensors(prior, nj, dev)
    verts, joints, loss, tr = ops.smpl_chamfer_refine(db.lbs_consts, scan, params, db.V, sl, pr, bidir, iterations, lr, nj=nj, nb=nb,
                                                      n_extra=db.n_extra, want_trace=want_trace)
    out = dict(loss=loss.sum(), loss_per_scan=loss, pose=params[:, :3 * nj], beta=params[:, 3 * nj:3 * nj + nb],
               trans=params[:, 3 * nj + nb:3 * nj + nb + 3], scale=params[:, 3 * nj + nb + 3:], joints=joints, verts=verts)
    if want_trace:
        out["loss_trace"] = tr
    return verts.cpu().numpy(), out
