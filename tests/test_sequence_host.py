"""Host-side parts of the sequence tracker (no GPU): nearest_rotvec, the bookkeeping between the launches, and the argument checks of
ops.smpl_lm_fit / fit_sequence / the track command, all of which raise before anything is launched."""
import math
import types

import numpy as np
import pytest
import torch


def _rot(v):
    """Rotation matrix of a rotation vector (Rodrigues, fp64)."""
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def test_nearest_rotvec_picks_the_equivalent_vector_next_to_the_reference():
    from etch_amd.sequence import nearest_rotvec
    axis = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
    # the same rotation just below and just above pi: as vectors they are ~2 pi apart
    theta, ref = axis * (math.pi - 0.05), -axis * (math.pi - 0.05)
    got = nearest_rotvec(theta, ref)
    assert torch.allclose(got, -axis * (math.pi + 0.05), atol=1e-12)
    assert np.abs(_rot(got.numpy()) - _rot(theta.numpy())).max() < 1e-12            # still the same rotation
    assert float((got - ref).norm()) < 0.11 < float((theta - ref).norm())
    # k = +1: a reference beyond pi on the same side
    got = nearest_rotvec(-axis * 3.0, axis * 3.2)
    assert torch.allclose(got, axis * (2 * math.pi - 3.0), atol=1e-12)
    # already nearest: returned unchanged, bit for bit; zero stays zero
    near = torch.tensor([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0]])
    assert torch.equal(nearest_rotvec(near, near + 0.05), near)


def test_nearest_rotvec_batched_against_enumeration():
    from _fit_prior_oracle import nearest_rotvec_ref
    from etch_amd.sequence import nearest_rotvec
    g = torch.Generator().manual_seed(3)
    theta = torch.randn(4, 23, 3, generator=g) * 2.0
    ref = torch.randn(4, 23, 3, generator=g) * 2.0
    got = nearest_rotvec(theta, ref)
    assert got.shape == theta.shape and got.dtype == torch.float32
    assert np.abs(got.numpy() - nearest_rotvec_ref(theta.numpy(), ref.numpy())).max() < 1e-5
    assert (((got - ref).norm(dim=-1)) <= (theta - ref).norm(dim=-1) + 1e-6).all()
    moved = (got != theta).any(-1)
    assert moved.any() and not moved.all()
    # broadcasting of the reference
    assert torch.equal(nearest_rotvec(theta[0], ref[0, :1]), nearest_rotvec(theta[0], ref[0, :1].expand(23, 3)))


def test_dead_frames_shape_mean_and_sweep_prior():
    from etch_amd import sequence as S
    nj, nb, T = 24, 10, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, 85, generator=g) * 0.1
    off = torch.randn(T, 3, generator=g)
    filled = S.fill_dead_frames(x, [True, False, False, True, False], off, nj, nb)
    assert torch.equal(filled[[0, 3]], x[[0, 3]])
    assert torch.allclose(filled[1, :82], (x[0, :82] + x[3, :82]) / 2, atol=1e-6) and torch.equal(filled[1, :82], filled[2, :82])
    assert torch.allclose(filled[1, 82:] + off[1], (x[0, 82:] + off[0] + x[3, 82:] + off[3]) / 2, atol=1e-6)       # translation: world frame
    assert torch.allclose(filled[4, :82], x[3, :82]) and torch.allclose(filled[4, 82:] + off[4], x[3, 82:] + off[3], atol=1e-6)
    valid = torch.zeros(T, 86)
    valid[0, :10], valid[3, :30] = 1, 1
    assert torch.allclose(S.shape_mean(x, valid, nj, nb), (10 * x[0, 69:79] + 30 * x[3, 69:79]) / 40, atol=1e-6)
    bmean = torch.arange(10.0)
    mean, w = S.sweep_prior(x, torch.tensor([0, 2, 4]), off, bmean, (0.5, 2.0, 3.0), 7.0, nj, nb)
    assert mean.shape == w.shape == (3, 85) and mean.is_contiguous() and w.is_contiguous()
    assert torch.equal(w[0], torch.cat([torch.full((69,), 0.5), torch.full((10,), 7.0), torch.full((3,), 2.0), torch.full((3,), 3.0)]))
    assert torch.equal(w[1, :69], torch.full((69,), 1.0)) and torch.equal(w[1, 82:], torch.full((3,), 6.0)) and torch.equal(w[1, 69:79], w[0, 69:79])
    assert torch.allclose(mean[1, :69], (x[1, :69] + x[3, :69]) / 2, atol=1e-6) and torch.equal(mean[:, 69:79], bmean.expand(3, 10))
    assert torch.allclose(mean[0, 82:] + off[0], x[1, 82:] + off[1], atol=1e-6)
    assert torch.allclose(mean[2, 82:] + off[4], x[3, 82:] + off[3], atol=1e-6)


def test_lm_fit_argument_errors_need_no_gpu(monkeypatch):
    from etch_amd import _lib, ops
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    B, M, dof = 2, 86, 85
    mk, vf = torch.zeros(B, M, 3), torch.ones(B, M)
    z, w = torch.zeros(B, dof), torch.ones(B, dof)
    neg = w.clone()
    neg[1, 80] = -0.5
    inf = w.clone()
    inf[0, 3] = float("inf")
    fit = lambda **kw: ops.smpl_lm_fit([], mk, vf, 1, 0.5, 0.01, 1, 0.2, 1e-3, **kw)
    for kw, msg in ((dict(prior=(z, neg)), "finite and >= 0"), (dict(prior=(z, inf)), "finite and >= 0"), (dict(prior=(z, None)), "without a weight"),
                    (dict(prior=(None, w)), "without a weight"), (dict(prior=z), "without a weight"), (dict(prior=(z, torch.ones(B, dof + 1))), "shape"),
                    (dict(prior=(torch.zeros(B + 1, dof), w)), "shape"), (dict(x_init=torch.zeros(dof)), "shape"),
                    (dict(x_init=z.double()), "float32"), (dict(x_init=torch.zeros(B, 2 * dof)[:, ::2]), "contiguous"),
                    (dict(x_init=[[0.0] * dof] * B), "tensor"), (dict(x_init=torch.full((B, dof), float("nan"))), "finite")):
        with pytest.raises(_lib.EtchHipError, match=msg):
            fit(**kw)
    # check=False skips the value check only (the synchronising part), never the shape checks
    with pytest.raises(_lib.EtchHipError, match="shape"):
        fit(prior=(z, w[:1]), check=False)


def test_fit_sequence_and_track_argument_errors():
    from etch_amd import constants as K
    from etch_amd import track
    from etch_amd.sequence import fit_sequence
    args = types.SimpleNamespace(markerset=K.default_markerset())
    mk, vd = torch.zeros(3, 86, 3), torch.ones(3, 86, dtype=torch.bool)
    for kw in (dict(temporal_w=(1.0, -1.0, 1.0)), dict(temporal_w=(1.0, 1.0)), dict(shape_w=float("nan")), dict(sweeps=-1), dict(refit_steps=-2),
               dict(offsets=torch.zeros(2, 3))):
        with pytest.raises(ValueError):
            fit_sequence(args, mk, vd, "neutral", **kw)
    with pytest.raises(ValueError):
        fit_sequence(args, mk, vd[:2], "neutral")
    with pytest.raises(ValueError):
        fit_sequence(args, mk[:, :80], vd[:, :80], "neutral")
    for argv in ([], ["--scan_paths", "a/f.obj", "b/f.obj"], ["--scan_paths", "a.obj", "--batch_size", "0"],
                 ["--scan_paths", "a.obj", "--chamfer_refine", "both"]):
        with pytest.raises(SystemExit):
            track.parse_args(argv)
    a = track.parse_args(["--scan_paths", "x/a.obj", "y/b.obj", "--temporal_w_pose", "0.25", "--sweeps", "3"])
    assert a.scan_names == ["a", "b"] and a.temporal_w_pose == 0.25 and a.sweeps == 3 and a.num_point == 5000 and a.gender == "neutral"
