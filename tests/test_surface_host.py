"""CPU checks of the dense surface refinement: the fp32 restatement of the region test against the exact answer and the reference's own
values, the stand-in body with a real surface, the restated loss against hand-computed values, the library's new symbols, and the
--surface_refine flags of inference_demo and eval."""
import numpy as np
import pytest
import torch

import _surface_oracle as O


def test_restatement_is_dtype_preserving_and_meets_the_reference_rule():
    """The rule of the GPU test, held by the numpy restatement: sqrt(d2) in fp32 within 2 e_32 + 1e-6 of the reference's fp64 values."""
    z = np.load(O.GOLDEN)
    verts, faces, pts = z["verts"], z["faces"], z["points"]
    f32, b32, d32, reg = O.closest_batch(pts, None, verts, faces)
    f64, b64, d64, _ = O.closest_batch(pts.astype(np.float64), None, verts.astype(np.float64), faces)
    assert d32.dtype == np.float32 and b32.dtype == np.float32 and d64.dtype == np.float64
    assert set(np.unique(reg).tolist()) == set(range(7))
    e32 = float(np.abs(z["ref32"].astype(np.float64) - z["ref64"]).max())
    err = float(np.abs(np.sqrt(d32.astype(np.float64)) - z["ref64"]).max())
    exact = float(np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)).max())
    print(f"reference e_32 {e32:.3e}; restatement fp32 vs reference fp64 {err:.3e}, vs exact {exact:.3e}")
    assert err <= 2 * e32 + 1e-6
    assert float(np.abs(z["ref64"] - np.sqrt(d64)).max()) < 1e-7           # at unit scale the reference's epsilons do no harm
    # the exact tie of the duplicated face goes to the lower face; the zero-area faces never beat the face they lie on
    assert (f32 == 3).any() and not (f32 == 69).any() and not np.isin(f32, (67, 68)).any()
    # barycentric weights sum to 1 and reproduce d2
    assert np.abs(b64.sum(-1) - 1).max() < 1e-12
    q = (b64[..., None] * verts.astype(np.float64)[np.arange(3)[:, None, None], faces.astype(np.int64)[f64]]).sum(2)
    assert np.abs(((pts - q) ** 2).sum(-1) - d64).max() < 1e-12


def test_restatement_agrees_with_the_raycast_oracle_in_fp64():
    import _raycast_oracle as R
    rng = np.random.default_rng(5)
    verts = rng.uniform(-1, 1, (30, 3))
    faces = rng.integers(0, 30, (50, 3)).astype(np.int32)
    pts = rng.uniform(-1.2, 1.2, (90, 3))
    f, b, d2, _ = O.closest_point_on_mesh(pts, verts, faces)
    rf, rb, _, rd = R.closest_point_on_mesh(pts, verts, faces)
    assert np.array_equal(f, rf) and np.array_equal(b, rb) and np.array_equal(d2, rd)


def test_synthetic_surface_body_is_a_closed_manifold():
    from etch_amd.utils.body_model import SyntheticSMPL, SyntheticSurfaceSMPL, uv_ellipsoid
    for rings, segs in ((20, 24), (82, 84), (1, 3)):
        v, f = uv_ellipsoid(rings, segs)
        assert v.shape == (rings * segs + 2, 3) and f.shape == (2 * rings * segs, 3)
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        _, cnt = np.unique(e, axis=0, return_counts=True)
        assert (cnt == 2).all()                                             # every edge lies in exactly two faces
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("ij,ij->i", n, v[f].mean(1)) > 0).all()           # wound outwards
        assert np.abs((v / np.array([0.15, 0.45, 0.10]) ** 1) ** 2 @ np.ones(3) - 1).max() < 1e-12
    bm = SyntheticSurfaceSMPL(7)
    assert bm.num_verts == 6890 and bm.faces.shape == (13776, 3) and bm.num_joints == 24 and bm.num_betas == 10
    assert int(bm.extra_vids.max()) < bm.num_verts and int(SyntheticSurfaceSMPL(7, 20, 24).extra_vids.max()) < 482
    assert (np.count_nonzero(bm.lbs_weights, axis=1) <= 4).all() and np.abs(bm.lbs_weights.sum(1) - 1).max() < 1e-6
    old = SyntheticSMPL(7)                                                    # the existing stand-in is what it was: a strip over random vertices
    assert old.faces.shape == (2 * 6890 - 4, 3) and old.faces[0].tolist() == [0, 1, 2]


def test_restated_loss_terms():
    """One triangle, three points: S1 / S0 with weights and the mask, and its gradient, by hand."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64, requires_grad=True)
    faces = torch.tensor([[0, 1, 2]])
    pts = torch.tensor([[0.25, 0.25, 0.1], [0.25, 0.25, -0.2], [2.0, 0.0, 0.0]], dtype=torch.float64)
    f, b, d2, reg = O.closest_point_on_mesh(pts.numpy(), verts.detach().numpy(), faces.numpy())
    assert reg.tolist() == [6, 6, 1] and np.allclose(d2, [0.01, 0.04, 1.0])
    w = torch.tensor([1.0, 2.0, 5.0], dtype=torch.float64)
    S1, S0 = O.dense_terms(verts, faces, pts, torch.from_numpy(f).long(), torch.from_numpy(b), w, 0.5)
    assert abs(float(S1) - (0.01 + 2 * 0.04)) < 1e-15 and float(S0) == 3.0                       # the third point is beyond trunc
    (S1 / S0).backward()
    # d/dv_k = 2 w_i (c_i - p_i) bary_ik / S0: only z components, bary (0.5, 0.25, 0.25)
    gz = (2 * 1.0 * (-0.1) + 2 * 2.0 * 0.2) / 3.0
    assert np.allclose(verts.grad.numpy()[:, 2], gz * np.array([0.5, 0.25, 0.25])) and np.abs(verts.grad.numpy()[:, :2]).max() == 0
    S1, S0 = O.dense_terms(verts, faces, pts, torch.from_numpy(f).long(), torch.from_numpy(b), None, None)
    assert abs(float(S1) - 1.05) < 1e-15 and float(S0) == 3.0


def test_new_symbols_are_declared():
    from etch_amd import _lib
    protos = _lib.prototypes()
    for n in ("etch_point_mesh_closest", "etch_point_mesh_closest_workspace", "etch_point_mesh_energy_grad", "etch_point_mesh_energy_grad_workspace",
              "etch_smpl_surface_refine", "etch_smpl_surface_refine_workspace"):
        assert n in protos, n
    assert [p for _, p in protos["etch_point_mesh_closest"][1]][-4:] == ["face", "bary", "d2", "stream"]
    assert protos["etch_smpl_surface_refine"][1][-1][1] == "stream" and len(protos["etch_smpl_surface_refine"][1]) == 36
    from etch_amd import build as B
    assert "-ffp-contract=off" in B.EXTRA["surface_fit.hip"] and "surface_fit.hip" in B.sources()


def test_cli_flags_and_the_both_refinements_error():
    from etch_amd import eval as E
    from etch_amd import inference_demo as D

    a = D.parse_args(["--scan_path", "x.obj"])
    assert not any(k.startswith("surface") for k in vars(a)) and D.surface_refine_settings(a) is None      # the namespace is what it was
    a = D.parse_args(["--scan_path", "x.obj", "--surface_refine"])
    assert D.surface_refine_settings(a) == dict(iterations=200, trunc=0.05, w_dense=1e2)
    a = D.parse_args(["--scan_path", "x.obj", "--surface_refine", "--surface_iters", "5", "--surface_trunc", "-1", "--surface_w", "30"])
    assert D.surface_refine_settings(a) == dict(iterations=5, trunc=-1.0, w_dense=30.0)
    for bad in (["--surface_refine", "--chamfer_refine", "both"], ["--surface_iters", "5"], ["--surface_refine", "--surface_iters", "0"]):
        with pytest.raises(SystemExit):
            D.parse_args(["--scan_path", "x.obj"] + bad)
    p = E.build_parser()
    a = p.parse_args([])
    assert not any(k.startswith("surface") for k in vars(a))
    a = p.parse_args(["--surface_refine", "--surface_iters", "7"])
    assert D.surface_refine_settings(a, p) == dict(iterations=7, trunc=0.05, w_dense=1e2)
    # --synthetic_body: the stand-in with a surface only together with --surface_refine
    import types
    for flag, faces in ((False, 2 * 6890 - 4), (True, 13776)):
        ns = types.SimpleNamespace(synthetic_body=True, body_model="", **({"surface_refine": True} if flag else {}))
        D.resolve_body_model(ns)
        assert ns.body_model.faces.shape == (faces, 3)
