"""Pose priors of the marker fits: the module surface of the reference's src/utils/prior.py (create_prior, MaxMixturePrior, SMPLifyAnglePrior,
L2Prior), with the max-mixture evaluation on the fit kernels' own device function and a bridge to the fits (`as_fit_prior`).

    MaxMixturePrior    min_k [0.5 (pose - mu_k)^T P_k (pose - mu_k) - log c_k] per row (use_merged=True: ops.pose_prior_eval, HIP) or the
                       log-likelihood form (use_merged=False: plain torch on the device; not available inside the fit kernels).
                       In the LM fit:   ops.smpl_lm_fit(..., pose_prior=prior.as_fit_prior(w_gmm, w_ang))
                       in the Adam fit: fit_SMPL_Adam.fit_smpl(..., pose_prior=prior, pose_prior_w=1e-7)
    SMPLifyAnglePrior  exp(s_t pose[a_t])^2 on the elbows and knees; in the LM fit the w_ang of as_fit_prior.
    L2Prior            sum(pose^2).  In the LM fit that is the existing diagonal prior: prior=(mean 0, weight 2 w on the pose DoFs) of
                       ops.smpl_lm_fit adds 0.5 * 2 w * sum(pose^2) = w * L2Prior(pose).

The mixture file is the SMPLify one: `gmm_{num_gaussians:02d}.pkl`, a pickled dict {means (G, D), covars (G, D, D), weights (G)} (read with
encoding="latin1"), or an .npz with those keys.  A pickled sklearn mixture object is refused: sklearn is not a dependency; convert it once with
`np.savez(path, means=g.means_, covars=g.covars_, weights=g.weights_)`."""
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

DEFAULT_DTYPE = torch.float32

ANGLE_PRIOR_IDXS = (55, 58, 12, 15)          # left elbow, right elbow, left knee, right knee: one axis-angle component each, in the 72-vector
ANGLE_PRIOR_SIGNS = (1.0, -1.0, -1.0, -1.0)  # the direction in which the joint must NOT bend


def create_prior(prior_type, **kwargs):
    """'gmm' -> MaxMixturePrior, 'l2' -> L2Prior, 'angle' -> SMPLifyAnglePrior, 'none' / None -> a function that returns 0.0."""
    if prior_type == "gmm":
        return MaxMixturePrior(**kwargs)
    if prior_type == "l2":
        return L2Prior(**kwargs)
    if prior_type == "angle":
        return SMPLifyAnglePrior(**kwargs)
    if prior_type == "none" or prior_type is None:
        return lambda *a, **k: 0.0
    raise ValueError(f"Prior {prior_type} is not implemented")


class SMPLifyAnglePrior(nn.Module):
    """exp(sign * angle)^2 for the four elbow / knee components: large when the joint bends the wrong way.  forward(pose (B, 72 or 69),
    with_global_pose) -> (B, 4); without the global orientation in `pose` the indices move down by 3."""

    def __init__(self, dtype=DEFAULT_DTYPE, **kwargs):
        super().__init__()
        self.register_buffer("angle_prior_idxs", torch.tensor(ANGLE_PRIOR_IDXS, dtype=torch.long))
        self.register_buffer("angle_prior_signs", torch.tensor(ANGLE_PRIOR_SIGNS, dtype=dtype))

    def forward(self, pose, with_global_pose=False):
        idx = self.angle_prior_idxs if with_global_pose else self.angle_prior_idxs - 3
        return torch.exp(pose[:, idx] * self.angle_prior_signs).pow(2)


class L2Prior(nn.Module):
    def __init__(self, dtype=DEFAULT_DTYPE, reduction="sum", **kwargs):
        super().__init__()

    def forward(self, module_input, *args):
        return module_input.pow(2).sum()


def load_mixture(path, num_gaussians=8):
    """{means, covars, weights} as numpy arrays from a folder (gmm_{num_gaussians:02d}.pkl inside it), a .pkl or an .npz."""
    if os.path.isdir(path):
        path = os.path.join(path, "gmm_{:02d}.pkl".format(num_gaussians))
    if not os.path.exists(path):
        raise FileNotFoundError(f'The mixture prior "{path}" does not exist')
    if path.endswith(".npz"):
        with np.load(path) as z:
            missing = [k for k in ("means", "covars", "weights") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: missing arrays {missing}")
            return {k: np.asarray(z[k]) for k in ("means", "covars", "weights")}
    with open(path, "rb") as f:
        try:
            gmm = pickle.load(f, encoding="latin1")
        except (ImportError, AttributeError) as e:       # a pickled object of a library that is not installed
            raise TypeError(f"{path} holds a pickled object ({e}), not a dict {{means, covars, weights}}: sklearn is not a dependency of etch_amd; "
                            "convert it once with np.savez(path, means=g.means_, covars=g.covars_, weights=g.weights_)") from e
    if not isinstance(gmm, dict):
        raise TypeError(f"{path} holds a {type(gmm).__module__}.{type(gmm).__name__}, not a dict {{means, covars, weights}}: pickled sklearn mixture "
                        "objects are not read (sklearn is not a dependency of etch_amd); convert it once with "
                        "np.savez(path, means=g.means_, covars=g.covars_, weights=g.weights_)")
    missing = [k for k in ("means", "covars", "weights") if k not in gmm]
    if missing:
        raise ValueError(f"{path}: missing entries {missing}")
    return {k: np.asarray(gmm[k]) for k in ("means", "covars", "weights")}


class MaxMixturePrior(nn.Module):
    """The SMPLify max-mixture pose prior.  prior_folder: the folder that holds gmm_{num_gaussians:02d}.pkl, or the path of a .pkl / .npz itself.
    Buffers as in the reference: means (G, D), covs, precisions (G, D, D), nll_weights (1, G), weights (1, G), pi_term, cov_dets (G).
    nll_weights = weights / ((2 pi)^(69/2) sqrt(det cov_k) / min_j sqrt(det cov_j)); the 69 is the reference's literal also for D != 69 (it shifts
    every component's constant alike, so no selection depends on it)."""

    def __init__(self, prior_folder="prior", num_gaussians=6, dtype=DEFAULT_DTYPE, epsilon=1e-16, use_merged=True, **kwargs):
        super().__init__()
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"Unknown float type {dtype}")
        npd = np.float32 if dtype == torch.float32 else np.float64
        self.num_gaussians, self.epsilon, self.use_merged = num_gaussians, epsilon, use_merged
        gmm = load_mixture(prior_folder, num_gaussians)
        means, covs = gmm["means"].astype(npd), gmm["covars"].astype(npd)
        if means.ndim != 2 or covs.shape != (means.shape[0],) + 2 * (means.shape[1],) or gmm["weights"].reshape(-1).shape[0] != means.shape[0]:
            raise ValueError(f"mixture shapes: means {means.shape}, covars {covs.shape}, weights {gmm['weights'].shape}")
        weights = gmm["weights"].reshape(-1)
        self.register_buffer("means", torch.tensor(means, dtype=dtype))
        self.register_buffer("covs", torch.tensor(covs, dtype=dtype))
        self.register_buffer("precisions", torch.tensor(np.stack([np.linalg.inv(c) for c in covs]).astype(npd), dtype=dtype))
        root_dets = np.array([np.sqrt(np.linalg.det(c)) for c in gmm["covars"]])
        nll = np.asarray(weights / ((2 * np.pi) ** (69 / 2.0) * (root_dets / root_dets.min())))
        self.register_buffer("nll_weights", torch.tensor(nll, dtype=dtype).unsqueeze(0))
        self.register_buffer("weights", torch.tensor(weights, dtype=dtype).unsqueeze(0))
        self.register_buffer("pi_term", torch.log(torch.tensor(2 * np.pi, dtype=dtype)))
        self.register_buffer("cov_dets", torch.tensor([np.log(np.linalg.det(c.astype(npd)) + epsilon) for c in covs], dtype=dtype))
        self.random_var_dim = self.means.shape[1]
        self._fit_tables = None

    def get_mean(self):
        """The mixture's mean pose (1, D)."""
        return torch.matmul(self.weights, self.means)

    def fit_tables(self):
        """The device tables of the kernels as an ops.PosePrior with zero weights, built once per device (its constructor does the value
        checks): what forward() evaluates and what the Adam fit weighs with its own pose_prior_w."""
        from .. import ops
        key = self.means.device
        if self._fit_tables is None or self._fit_tables[0] != key:
            self._fit_tables = (key, ops.PosePrior(self.means, self.precisions, self.nll_weights.reshape(-1), 0.0, device=key))
        return self._fit_tables[1]

    def as_fit_prior(self, w_gmm, w_ang=0.0):
        """The ops.PosePrior of this mixture for ops.smpl_lm_fit / fit_smpl(..., pose_prior=): weight w_gmm on the max-mixture term and, with
        w_ang > 0, SMPLifyAnglePrior's four terms (indices without the global orientation) at weight w_ang.  Lives on the buffers' device."""
        from .. import ops
        ang = w_ang > 0
        return ops.PosePrior(self.means, self.precisions, self.nll_weights.reshape(-1), w_gmm,
                             angle_idx=[i - 3 for i in ANGLE_PRIOR_IDXS] if ang else None, angle_sign=list(ANGLE_PRIOR_SIGNS) if ang else None,
                             w_ang=w_ang, device=self.means.device)

    def merged_log_likelihood(self, pose, betas):
        """min_k [0.5 d_k^T P_k d_k - log nll_weights_k] per row, on the fit kernels' device function (fp64 inside, the module's dtype out).
        No autograd: the fits take the gradient from the same kernel."""
        from .. import ops
        val, _, _ = ops.pose_prior_eval(pose.detach().to(torch.float32).contiguous(), self.fit_tables())
        return val.to(self.means.dtype)

    def log_likelihood(self, pose, betas, *args, **kwargs):
        """The negative log-likelihood form: per component d^T P_k d + 0.5 (log(det cov_k + epsilon) + D log 2 pi), the smallest of them plus
        -log nll_weights of that component.  Plain torch (differentiable) on the buffers' device."""
        d = pose.unsqueeze(1) - self.means                                           # (B, G, D)
        quad = torch.einsum("bgi,gij,bgj->bg", d, self.precisions, d)
        cov_term = torch.log(torch.linalg.det(self.covs) + self.epsilon)
        ll = quad + 0.5 * (cov_term + self.random_var_dim * self.pi_term)
        best = torch.argmin(ll, dim=1)
        return -torch.log(self.nll_weights[0, best]) + ll.gather(1, best[:, None])[:, 0]

    def forward(self, pose, betas):
        return self.merged_log_likelihood(pose, betas) if self.use_merged else self.log_likelihood(pose, betas)


# ---------------------------------------------------------------------------------------------------------------- command-line bridge
# The only weight the reference gives is 1e-7 on the scale of its Adam fitter's mean-squared loss (fit_SMPL_Adam.py:99).  The LM objective is
# 0.5 * sum r^2 over 3 M coordinates, i.e. 3 M / 2 times that loss: 1e-7 * 3 * 86 / 2 = 1.3e-5 for the 86-marker set.  Nobody has measured
# either value on real captures.
DEFAULT_LM_POSE_PRIOR_W = 1.3e-5


def add_pose_prior_flags(parser):
    """--pose_prior / --pose_prior_gaussians / --pose_prior_w / --angle_prior_w of inference_demo, eval and track.  Absent unless given (the
    namespace of a run without them is what it always was): read them with pose_prior_options.  Without --pose_prior the fit is what it was."""
    import argparse
    parser.add_argument("--pose_prior", type=str, default=argparse.SUPPRESS,
                        help="max-mixture pose prior of the marker fit (DESIGN 14): a folder holding gmm_XX.pkl, or a .pkl / .npz with "
                             "{means, covars, weights}; absent (default): no pose prior")
    parser.add_argument("--pose_prior_gaussians", type=int, default=argparse.SUPPRESS, help="XX of gmm_XX.pkl when --pose_prior is a folder (default 8)")
    parser.add_argument("--pose_prior_w", type=float, default=argparse.SUPPRESS,
                        help=f"weight of the mixture term in the LM objective 0.5 sum r^2 (default {DEFAULT_LM_POSE_PRIOR_W}: the reference's 1e-7 on "
                             "its mean-squared loss times 3 M / 2 for 86 markers; not measured on real captures)")
    parser.add_argument("--angle_prior_w", type=float, default=argparse.SUPPRESS,
                        help="weight of the elbow / knee terms exp(2 s x) (SMPLifyAnglePrior); default 0: none; needs --pose_prior; "
                             "not measured on real captures")
    return parser


def pose_prior_options(args):
    """The four flags with their defaults: dict(path, gaussians, w_gmm, w_ang); path '' = off."""
    return dict(path=getattr(args, "pose_prior", ""), gaussians=getattr(args, "pose_prior_gaussians", 8),
                w_gmm=getattr(args, "pose_prior_w", DEFAULT_LM_POSE_PRIOR_W), w_ang=getattr(args, "angle_prior_w", 0.0))


def pose_prior_from_args(args, device):
    """-> the ops.PosePrior the flags ask for, or None without --pose_prior."""
    o = pose_prior_options(args)
    if not o["path"]:
        return None
    mix = MaxMixturePrior(prior_folder=o["path"], num_gaussians=o["gaussians"]).to(device)
    return mix.as_fit_prior(o["w_gmm"], o["w_ang"])
