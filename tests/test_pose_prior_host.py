"""Host side of the pose priors (etch_amd/utils/prior.py): loading a mixture, the buffers against an fp64 restatement of the
reference's constructor, the small priors, create_prior, and the command-line flags.  No GPU."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

import _pose_prior_oracle as P
from etch_amd.utils import prior as PR

REFERENCE_PRIOR = "/root/reference/src/utils/prior.py"


@pytest.fixture(scope="module")
def gmm():
    return P.mixture(4, 69, seed=5)


def _write_pkl(gmm, folder):
    with open(os.path.join(folder, "gmm_04.pkl"), "wb") as f:
        pickle.dump(gmm, f)
    return str(folder)


def _check_buffers(m, gmm, np_dtype, asked=4):
    b = P.buffers_fp64(gmm, np_dtype)
    for name in ("means", "covs", "precisions", "nll_weights", "weights", "cov_dets", "pi_term"):
        got = getattr(m, name).numpy()
        assert got.dtype == np_dtype and got.shape == np.asarray(b[name]).shape, name
        if name in ("pi_term", "cov_dets"):        # a logarithm taken by torch here, by numpy in fp64 there: one rounding apart
            assert np.allclose(got, b[name], rtol=4 * np.finfo(np_dtype).eps, atol=0), name
        else:
            assert np.array_equal(got, b[name]), name
    assert m.random_var_dim == 69 and m.num_gaussians == asked and m.means.shape[0] == 4
    want = (gmm["weights"].astype(np_dtype)[None] @ gmm["means"].astype(np_dtype))
    assert m.get_mean().shape == (1, 69) and np.allclose(m.get_mean().numpy(), want, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("dtype,np_dtype", [(torch.float32, np.float32), (torch.float64, np.float64)])
def test_mixture_from_a_dict_pickle(gmm, tmp_path, dtype, np_dtype):
    m = PR.MaxMixturePrior(prior_folder=_write_pkl(gmm, tmp_path), num_gaussians=4, dtype=dtype)
    _check_buffers(m, gmm, np_dtype)
    # the precisions are what they claim to be, and the weights of the bracket are positive
    eye = np.einsum("gij,gjk->gik", m.precisions.double().numpy(), gmm["covars"])
    assert np.abs(eye - np.eye(69)).max() < (1e-3 if dtype == torch.float32 else 1e-9)
    assert bool((m.nll_weights > 0).all())


def test_mixture_from_an_npz_and_from_a_pkl_path(gmm, tmp_path):
    np.savez(tmp_path / "mix.npz", **gmm)
    _check_buffers(PR.MaxMixturePrior(prior_folder=str(tmp_path / "mix.npz"), num_gaussians=8), gmm, np.float32, asked=8)
    _write_pkl(gmm, tmp_path)
    _check_buffers(PR.MaxMixturePrior(prior_folder=str(tmp_path / "gmm_04.pkl"), num_gaussians=8), gmm, np.float32, asked=8)


class _NotADict:
    """Stands in for a pickled sklearn mixture object."""
    means_ = covars_ = weights_ = None


def test_pickled_object_and_missing_file_are_clear_errors(gmm, tmp_path):
    with open(tmp_path / "gmm_08.pkl", "wb") as f:
        pickle.dump(_NotADict(), f)
    with pytest.raises(TypeError, match="sklearn is not a dependency"):
        PR.MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=8)
    with pytest.raises(FileNotFoundError, match="gmm_06.pkl"):
        PR.MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=6)
    with pytest.raises(FileNotFoundError):
        PR.MaxMixturePrior(prior_folder=str(tmp_path / "nowhere"))
    np.savez(tmp_path / "half.npz", means=gmm["means"])
    with pytest.raises(ValueError, match="covars"):
        PR.MaxMixturePrior(prior_folder=str(tmp_path / "half.npz"))


def test_small_priors_and_log_likelihood(gmm, tmp_path):
    g = torch.Generator().manual_seed(1)
    pose = torch.randn(3, 69, generator=g, dtype=torch.float64) * 0.3
    ang = PR.SMPLifyAnglePrior(dtype=torch.float64)
    want = np.exp(2.0 * pose.numpy()[:, [52, 55, 9, 12]] * np.array([1.0, -1.0, -1.0, -1.0]))
    assert np.allclose(ang(pose).numpy(), want, rtol=1e-12)
    full = torch.cat([torch.zeros(3, 3, dtype=torch.float64), pose], 1)
    assert torch.equal(ang(full, with_global_pose=True), ang(pose))
    assert float(PR.L2Prior()(pose)) == pytest.approx(float((pose.numpy() ** 2).sum()), rel=1e-12)
    # use_merged=False: min_k [d^T P_k d + 0.5 (log(det cov_k + eps) + D log 2 pi)] - log nll_weights of that k, in fp64 numpy
    m = PR.MaxMixturePrior(prior_folder=_write_pkl(gmm, tmp_path), num_gaussians=4, dtype=torch.float64, use_merged=False)
    b = P.buffers_fp64(gmm, np.float64)
    d = pose.numpy()[:, None] - b["means"][None]
    ll = np.einsum("bgi,gij,bgj->bg", d, b["precisions"], d) + 0.5 * (b["cov_dets"] + 69 * np.log(2 * np.pi))[None]
    k = ll.argmin(1)
    want = ll[np.arange(3), k] - np.log(b["nll_weights"][0, k])
    assert np.allclose(m(pose, None).numpy(), want, rtol=1e-10)


def test_create_prior_branches(gmm, tmp_path):
    assert isinstance(PR.create_prior("gmm", prior_folder=_write_pkl(gmm, tmp_path), num_gaussians=4), PR.MaxMixturePrior)
    assert isinstance(PR.create_prior("l2"), PR.L2Prior)
    assert isinstance(PR.create_prior("angle", dtype=torch.float64), PR.SMPLifyAnglePrior)
    assert PR.create_prior("none")(torch.zeros(1, 69), None) == 0.0 and PR.create_prior(None)() == 0.0
    with pytest.raises(ValueError, match="not implemented"):
        PR.create_prior("vposer")


def test_command_lines_parse_the_flags_and_default_to_off():
    from etch_amd import eval as E
    from etch_amd import inference_demo as D
    from etch_amd import track as T
    flags = ["--pose_prior", "priors/", "--pose_prior_gaussians", "6", "--pose_prior_w", "2e-4", "--angle_prior_w", "0.5"]
    for parse, base in ((D.parse_args, ["--scan_path", "a.obj"]), (T.parse_args, ["--scan_paths", "a.obj", "b.obj"]),
                        (lambda argv: E.build_parser().parse_args(argv), [])):
        off = parse(base)                      # absent unless given: the namespace of a run without the flags is what it was
        assert not any(hasattr(off, k) for k in ("pose_prior", "pose_prior_gaussians", "pose_prior_w", "angle_prior_w"))
        o = PR.pose_prior_options(off)
        assert o["path"] == "" and o["gaussians"] == 8 and o["w_ang"] == 0.0 and o["w_gmm"] == pytest.approx(1e-7 * 3 * 86 / 2, rel=0.02)
        assert PR.pose_prior_from_args(off, "cpu") is None
        on = parse(base + flags)
        assert (on.pose_prior, on.pose_prior_gaussians, on.pose_prior_w, on.angle_prior_w) == ("priors/", 6, 2e-4, 0.5)
        assert PR.pose_prior_options(on) == dict(path="priors/", gaussians=6, w_gmm=2e-4, w_ang=0.5)


def test_against_the_reference_module(gmm, tmp_path):
    if not os.path.exists(REFERENCE_PRIOR):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("_reference_prior", REFERENCE_PRIOR)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    folder = _write_pkl(gmm, tmp_path)
    for dtype in (torch.float32, torch.float64):
        ours = PR.MaxMixturePrior(prior_folder=folder, num_gaussians=4, dtype=dtype)
        theirs = ref.MaxMixturePrior(prior_folder=folder, num_gaussians=4, dtype=dtype)
        for name in ("means", "covs", "precisions", "nll_weights", "weights", "pi_term", "cov_dets"):
            a, b = getattr(ours, name), getattr(theirs, name)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
        assert torch.equal(ours.get_mean(), theirs.get_mean())
    pose = torch.randn(3, 69, generator=torch.Generator().manual_seed(2)) * 0.3
    assert torch.equal(PR.SMPLifyAnglePrior()(pose), ref.SMPLifyAnglePrior()(pose))
    full = torch.cat([torch.zeros(3, 3), pose], 1)
    assert torch.equal(PR.SMPLifyAnglePrior()(full, with_global_pose=True), ref.SMPLifyAnglePrior()(full, with_global_pose=True))
    assert torch.equal(PR.L2Prior()(pose), ref.L2Prior()(pose))
