"""CPU restatement of fit_cham (scripts/experiment_scripts/chamfer_refine.py) for the chamfer tests -- TEST INFRASTRUCTURE ONLY.

Written from the contract, in any torch dtype (fp64 = the truth, fp32 = the entitled error): verts = (LBS(pose, beta) + trans) * scale
with oracle.stage2.lbs, S1 = sum over the scan of the squared distance to the nearest vertex, S2 = sum over the vertices of the squared
distance to the nearest scan point, data = sqrt(S1) + sqrt(S2) / sqrt(S1) / sqrt(S2) for bidir 0 / 1 / -1, loss = data + 1e-8 prior(pose[3:])
+ 0.2 mean(beta^2), prior = min_g 0.5 d^T P_g d - log w_g, torch.optim.Adam(betas (0.9, 0.999), eps 1e-8), step i at lr for i = 0 and
lr (N - i + 1) / N after.  Autograd does every derivative."""
import numpy as np
import torch

from oracle import stage2 as S2


def lr_at(i, iters, lr):
    return lr if i == 0 else lr * (iters - i + 1) / iters


def prior_nll(pose69, means, prec, w):
    """merged_log_likelihood: pose69 (B,69) -> (B,)."""
    d = pose69[:, None, :] - means[None]
    q = torch.einsum("gij,bgj->bgi", prec, d)
    ll = 0.5 * (q * d).sum(-1) - torch.log(w)[None]
    return ll.min(1).values


def nn_sq(a, b):
    """For each row of a (n,3): squared distance to the nearest row of b (m,3) and its index (ties -> lowest index)."""
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    v, i = d.min(1)
    return v, i


def scan_loss(verts, scan, bidir, assign=None):
    """Per-scan data term of one scan: verts (V,3), scan (n,3).  assign = (idx scan->verts, idx verts->scan) fixes the neighbours."""
    if assign is None:
        with torch.no_grad():
            _, i1 = nn_sq(scan, verts)
            _, i2 = nn_sq(verts, scan)
    else:
        i1, i2 = assign
    S1 = ((scan - verts[i1]) ** 2).sum()
    S2 = ((verts - scan[i2]) ** 2).sum()
    d1, d2 = torch.sqrt(S1), torch.sqrt(S2)
    return d1 + d2 if bidir == 0 else d1 if bidir == 1 else d2


def forward(tb, params, nj, nb):
    pose, beta = params[:, :3 * nj], params[:, 3 * nj:3 * nj + nb]
    trans, scale = params[:, 3 * nj + nb:3 * nj + nb + 3], params[:, 3 * nj + nb + 3:]
    v, j = S2.lbs(tb, beta, pose, torch.zeros_like(trans))
    return (v + trans[:, None]) * scale[:, :, None], j


def total_loss(tb, params, scans, lengths, bidir, prior, nj, nb):
    verts, _ = forward(tb, params, nj, nb)
    beta = params[:, 3 * nj:3 * nj + nb]
    per = []
    for b in range(params.shape[0]):
        l = scan_loss(verts[b], scans[b, :lengths[b]], bidir)
        if prior is not None:
            l = l + 1e-8 * prior_nll(params[b:b + 1, 3:72], *prior)[0]
        per.append(l + 0.2 * (beta[b] ** 2).mean())
    return torch.stack(per)


def fit_cham(bm, scans, lengths, params0, bidir, iters, lr=2e-2, prior=None, dtype=torch.float64):
    """-> (loss trace (B, iters) of every forward, final params (B,P)); numpy in, numpy out."""
    nj, nb = bm.num_joints, bm.num_betas
    tb = S2.TorchBody(bm, dtype)
    scans = torch.as_tensor(np.asarray(scans)).to(dtype)
    p = torch.nn.Parameter(torch.as_tensor(np.asarray(params0)).to(dtype).clone())
    pr = None if prior is None else tuple(torch.as_tensor(np.asarray(a)).to(dtype) for a in prior)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    trace = []
    for i in range(iters):
        for g in opt.param_groups:
            g["lr"] = lr_at(i, iters, lr)
        per = total_loss(tb, p, scans, lengths, bidir, pr, nj, nb)
        trace.append(per.detach().clone())
        opt.zero_grad()
        per.sum().backward()
        opt.step()
    return torch.stack(trace, 1).numpy(), p.detach().numpy()


def lbs_vjp(bm, params, g, dtype=torch.float64):
    """dL/dparams of L = sum(g * verts) by autograd through oracle.stage2.lbs."""
    tb = S2.TorchBody(bm, dtype)
    p = torch.as_tensor(np.asarray(params)).to(dtype).requires_grad_(True)
    v, _ = forward(tb, p, bm.num_joints, bm.num_betas)
    (v * torch.as_tensor(np.asarray(g)).to(dtype)).sum().backward()
    return p.grad.numpy()


def random_prior(seed, G=8, D=69, prec_scale=1.0, skew=0.0):
    """A seeded random SPD prior: means (G,D), precisions (G,D,D) (times prec_scale), nll_weights (G) fp32.  The refinement weighs the
    prior by 1e-8: prec_scale ~1e7 makes that term O(1) in the loss and the gradient, so a test of it can see it.  skew adds a
    skew-symmetric part (the value is unchanged; the gradient is 0.5 (P + P^T) d, which a kernel using P d alone would miss)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((G, D, D)) * 0.3
    K = rng.standard_normal((G, D, D)) * skew
    prec = (np.einsum("gij,gkj->gik", A, A) + np.eye(D)[None] + K - np.transpose(K, (0, 2, 1))) * prec_scale
    w = rng.uniform(0.5, 2.0, G)
    return rng.standard_normal((G, D)).astype(np.float32) * 0.1, prec.astype(np.float32), (w / w.sum()).astype(np.float32)
