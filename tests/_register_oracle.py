"""CPU restatement of the SMPL+D registration and of re-posing for the register tests -- TEST INFRASTRUCTURE ONLY.

Written from the contract, in any torch dtype (fp64 = the truth, fp32 = the entitled error), on oracle.stage2.TorchBody and
oracle.stage2.rodrigues.  params (B, 3 nj + nb + 4) = pose (global orient first) | beta | trans | scale.  With r_v the rest vertex after
shape and pose blend shapes and A_j the joint transforms (rest joint removed, no trans, no scale):

    base_v = (sum_j W_vj A_j [r_v; 1] + trans) scale,   R_v = scale sum_j W_vj A_j^R,   verts_v(D) = base_v + R_v D_v

    E_b = w_s2m / n_b sum_i d(x_i, y_a(i)) + w_m2s / V sum_v m_v d(y_v, x_c(v)) + lam_s / |E| sum_(u,v) |D_u - D_v|^2 + lam_m / V sum_v |D_v|^2

with y = verts(D), a / c the nearest neighbours (ties -> the lowest index), m_v = [d(y_v, x_c(v)) <= trunc^2] or 1; neighbours and masks are
constants of the differentiation, which autograd does.  torch.optim.Adam(betas (0.9, 0.999), eps 1e-8) at a constant lr."""
import numpy as np
import torch

from oracle import stage2 as S2


def split(params, nj, nb):
    return params[:, :3 * nj], params[:, 3 * nj:3 * nj + nb], params[:, 3 * nj + nb:3 * nj + nb + 3], params[:, 3 * nj + nb + 3:]


def frames(tb, params, nj, nb):
    """-> base (B,V,3), R (B,V,3,3), A (B,J,3,4); the symbols of oracle.stage2.lbs."""
    pose, beta, trans, scale = split(params, nj, nb)
    B, J, dt = params.shape[0], tb.J, params.dtype
    v_s = tb.v_t[None] + torch.einsum("bl,mkl->bmk", beta, tb.S)
    Jl = torch.einsum("bik,ji->bjk", v_s, tb.Jreg)
    R = S2.rodrigues(pose.reshape(-1, 3)).view(B, J, 3, 3)
    pf = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, -1)
    v_p = v_s + (pf @ tb.P).view(B, -1, 3)
    par = torch.tensor(tb.parents[1:])
    rel = torch.cat([Jl[:, :1], Jl[:, 1:] - Jl[:, par]], 1)
    T = torch.cat([torch.cat([R, rel[..., None]], -1), torch.tensor([0, 0, 0, 1.0], dtype=dt).expand(B, J, 1, 4)], -2)
    chain = [T[:, 0]]
    for i in range(1, J):
        chain.append(chain[tb.parents[i]] @ T[:, i])
    G = torch.stack(chain, 1)
    Jh = torch.cat([Jl, torch.zeros(B, J, 1, dtype=dt)], -1)[..., None]
    A = (G - torch.nn.functional.pad(G @ Jh, (3, 0)))[:, :, :3, :]
    Tm = torch.einsum("vj,bjrc->bvrc", tb.W, A)
    base = (torch.einsum("bvrc,bvc->bvr", Tm[..., :3], v_p) + Tm[..., 3] + trans[:, None]) * scale[:, :, None]
    return base, scale[:, :, None, None] * Tm[..., :3], A


def apply(base, R, D):
    return base + torch.einsum("bvrc,bvc->bvr", R, D)


def repose(tb, params_new, D, nj, nb):
    base, R, _ = frames(tb, params_new, nj, nb)
    return apply(base, R, D)


def edges(faces):
    """The unique undirected pairs u < v of the face rows, (|E|,2) int64, sorted."""
    s = set()
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            if u != v:
                s.add((min(u, v), max(u, v)))
    return torch.tensor(sorted(s), dtype=torch.long).reshape(-1, 2)


def two_nearest(a, b):
    """For each row of a: index of the nearest row of b (ties -> the lowest index), and the two smallest squared distances."""
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    i = d.argmin(1)
    k = min(2, d.shape[1])
    return i, torch.topk(d, k, dim=1, largest=False).values


def energy(base, R, D, scans, lengths, E, w_s2m, w_m2s, lam_s, lam_m, trunc=None, assign=None, gaps=None):
    """-> terms (B,4), differentiable in D.  assign = (idx_xy (B,N), idx_yx (B,V)) fixes the neighbours (the mask is still formed here).
    gaps: a list that receives, per call, the smallest relative gap (second - nearest) / second over every query of both directions."""
    y = apply(base, R, D)
    V = y.shape[1]
    out = []
    for b in range(y.shape[0]):
        n = int(lengths[b])
        x = scans[b, :n]
        if assign is None:
            with torch.no_grad():
                a, da = two_nearest(x, y[b])
                c, dc = two_nearest(y[b], x)
                if gaps is not None:
                    g = [((t[:, 1] - t[:, 0]) / t[:, 1]).min().item() for t in (da, dc) if t.shape[1] == 2]
                    gaps.append(min(g) if g else 1.0)
        else:
            a, c = assign[0][b, :n].long(), assign[1][b].long()
        d1 = ((x - y[b][a]) ** 2).sum(-1)
        d2 = ((y[b] - x[c]) ** 2).sum(-1)
        m = torch.ones_like(d2) if trunc is None else (d2.detach() <= trunc ** 2).to(d2.dtype)
        ne = max(len(E), 1)
        out.append(torch.stack([w_s2m / n * d1.sum(), w_m2s / V * (m * d2).sum(), lam_s / ne * ((D[b][E[:, 0]] - D[b][E[:, 1]]) ** 2).sum(),
                                lam_m / V * (D[b] ** 2).sum()]))
    return torch.stack(out)


def body_to_scan_distances(base, R, D, scans, lengths, idx_yx):
    """d(y_v, x_c(v)) (B,V) with the given neighbours: what the mask compares with trunc^2."""
    y = apply(base, R, D)
    return torch.stack([((y[b] - scans[b, :int(lengths[b])][idx_yx[b].long()]) ** 2).sum(-1) for b in range(y.shape[0])])


def schedule(l0, l1, iters):
    return [l0] if iters == 1 else [l0 * (l1 / l0) ** (i / (iters - 1)) for i in range(iters)]


def register(bm, params, scans, lengths, iters, lr=1e-3, w_s2m=1.0, w_m2s=1.0, smooth_w=(10.0, 0.1), mag_w=0.0, trunc=None, dtype=torch.float64,
             smooth=True, gaps=None):
    """-> (trace (B,iters,4) = the terms at the iterate before every step, final D (B,V,3)); numpy in, numpy out.  smooth=False removes the
    smoothness term from the objective (its trace column is 0)."""
    nj, nb = bm.num_joints, bm.num_betas
    tb = S2.TorchBody(bm, dtype)
    E = edges(bm.faces)
    with torch.no_grad():
        base, R, _ = frames(tb, torch.as_tensor(np.asarray(params)).to(dtype), nj, nb)
    scans = torch.as_tensor(np.asarray(scans)).to(dtype)
    D = torch.nn.Parameter(torch.zeros_like(base))
    opt = torch.optim.Adam([D], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    lam = schedule(smooth_w[0], smooth_w[1], iters)
    trace = []
    for i in range(iters):
        t = energy(base, R, D, scans, lengths, E, w_s2m, w_m2s, lam[i] if smooth else 0.0, mag_w, trunc, gaps=gaps)
        trace.append(t.detach().clone())
        opt.zero_grad()
        t.sum().backward()
        opt.step()
    return torch.stack(trace, 1).numpy(), D.detach().numpy()


def carry(tb, params, params_new, face, bary, faces, points, nj, nb):
    """animate.py:172-206 with w~ = sum_k bary_k W[faces[face, k]]: (T' T^-1 (x / scale - trans) + trans') scale'; |det T^R| < 1e-10 -> T = I."""
    dt = points.dtype
    _, _, A0 = frames(tb, params, nj, nb)
    _, _, A1 = frames(tb, params_new, nj, nb)
    w = (bary[:, :, None] * tb.W[faces[face.long()].long()]).sum(1)
    return carry_with(w, A0[0], A1[0], params[0, 3 * nj + nb:], params_new[0, 3 * nj + nb:], points)


def carry_with(w, A0, A1, ts0, ts1, points):
    dt = points.dtype
    bottom = torch.tensor([0, 0, 0, 1.0], dtype=dt)
    full = lambda A: torch.cat([torch.einsum("pj,jrc->prc", w, A), bottom.expand(w.shape[0], 1, 4)], 1)
    T, U = full(A0), full(A1)
    bad = torch.det(T[:, :3, :3]).abs() < 1e-10
    T[bad] = torch.eye(4, dtype=dt)
    x = torch.cat([points / ts0[3] - ts0[:3], torch.ones(points.shape[0], 1, dtype=dt)], 1)
    rest = torch.linalg.solve(T, x[..., None])
    return ((U @ rest)[:, :3, 0] + ts1[:3]) * ts1[3]
