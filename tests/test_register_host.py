"""Host-side pieces of the SMPL+D registration and of etch_amd.animate (no GPU): the edge / neighbour-list builder, the smoothness
schedule, pose-file parsing and the face filter."""
import numpy as np
import pytest
import torch


def test_mesh_edges_duplicates_orientations_degenerate_and_isolated():
    from etch_amd.models.register import mesh_edges

    faces = np.array([[0, 1, 2], [2, 1, 0],          # the same face in both orientations
                      [0, 1, 2],                      # and listed twice
                      [2, 3, 3],                      # a degenerate face: the pair (3, 3) is dropped, (2, 3) stays
                      [5, 2, 4]])                     # vertex 6 is in no face
    ptr, idx, n = mesh_edges(faces, 7)
    want = {0: [1, 2], 1: [0, 2], 2: [0, 1, 3, 4, 5], 3: [2], 4: [2, 5], 5: [2, 4], 6: []}
    assert n == 7 and ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr.shape == (8,) and idx.shape == (14,)
    for v, nb in want.items():
        assert idx[ptr[v]:ptr[v + 1]].tolist() == nb, v
    ptr0, idx0, n0 = mesh_edges(np.zeros((0, 3), np.int64), 3)
    assert n0 == 0 and ptr0.tolist() == [0, 0, 0, 0] and idx0.shape == (0,)
    with pytest.raises(ValueError):
        mesh_edges(np.array([[0, 1, 7]]), 7)


def test_mesh_edges_of_the_synthetic_body_and_its_cache():
    from etch_amd.models.register import _edges_of, _faces_of, mesh_edges
    from etch_amd.utils.body_model import SyntheticSMPL

    import _register_oracle as O
    bm = SyntheticSMPL(7, V=50)                      # every face listed both ways
    ptr, idx, n = mesh_edges(bm.faces, bm.num_verts)
    E = O.edges(bm.faces).numpy()
    assert n == len(E)
    got = sorted((u, int(v)) for u in range(50) for v in idx[ptr[u]:ptr[u + 1]] if u < v)
    assert got == [tuple(e) for e in E.tolist()]
    for v in range(50):
        nb = idx[ptr[v]:ptr[v + 1]]
        assert (np.diff(nb) > 0).all()               # ascending, no repeats
    # the cached copies: the lists above, built once per body model and copied once per device; the faces likewise
    cpu = torch.device("cpu")
    first = _edges_of(bm, cpu)
    assert first[0].dtype == torch.int32 and first[0].tolist() == ptr.tolist() and first[1].tolist() == idx.tolist() and first[2] == n
    again = _edges_of(bm, cpu)
    assert all(a is b for a, b in zip(first, again)) and set(bm._etch_edges) == {"host", "cpu"}
    assert _edges_of(SyntheticSMPL(7, V=50), cpu)[0] is not first[0]          # per body model, not per class
    f = _faces_of(bm, cpu)
    assert f is _faces_of(bm, cpu) and f.dtype == torch.int32 and np.array_equal(f.numpy(), bm.faces)


def test_smooth_schedule():
    from etch_amd.models.register import smooth_schedule

    s = smooth_schedule(10.0, 0.1, 5)
    assert s.dtype == np.float64 and np.allclose(s, [10.0, 10 ** 0.5, 1.0, 10 ** -0.5, 0.1], rtol=1e-14, atol=0)
    assert s[0] == 10.0 and abs(s[-1] - 0.1) <= 1e-16
    assert smooth_schedule(3.0, 0.5, 1).tolist() == [3.0]
    assert smooth_schedule(2.0, 2.0, 4).tolist() == [2.0] * 4
    assert smooth_schedule(0.0, 0.0, 3).tolist() == [0.0] * 3
    for bad in ((1.0, 0.0, 3), (0.0, 1.0, 3), (-1.0, 1.0, 3), (1.0, 1.0, 0), (float("nan"), 1.0, 3)):
        with pytest.raises(ValueError):
            smooth_schedule(*bad)


def test_pose_file_both_shapes_and_defaults(tmp_path):
    from etch_amd.animate import new_params, read_pose_file

    rng = np.random.default_rng(1)
    bp = rng.standard_normal((3, 69)).astype(np.float32)
    np.savez(tmp_path / "a.npz", body_pose=bp)
    a = read_pose_file(tmp_path / "a.npz")
    assert a["body_pose"].shape == (3, 69) and np.array_equal(a["body_pose"], bp) and a["global_orient"] is None and a["transl"] is None
    go, tr = rng.standard_normal((3, 3)).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    torch.save({"body_pose": torch.from_numpy(bp.reshape(3, 23, 3)), "global_orient": torch.from_numpy(go), "transl": torch.from_numpy(tr)}, tmp_path / "b.pt")
    b = read_pose_file(tmp_path / "b.pt")
    assert np.array_equal(b["body_pose"], bp) and np.array_equal(b["global_orient"], go) and np.array_equal(b["transl"], np.tile(tr, (3, 1)))
    np.savez(tmp_path / "one.npz", body_pose=bp[0])
    assert read_pose_file(tmp_path / "one.npz")["body_pose"].shape == (1, 69)
    # the fit's parameters with the poses put in: whatever the file leaves out keeps the fit's value
    fit = torch.arange(86, dtype=torch.float32)[None]
    pa, pb = new_params(fit, a, 24, 10), new_params(fit, b, 24, 10)
    assert pa.shape == (3, 86) and torch.equal(pa[:, 3:72], torch.from_numpy(bp))
    assert torch.equal(pa[:, :3], fit[:, :3].expand(3, -1)) and torch.equal(pa[:, 72:], fit[:, 72:].expand(3, -1))
    assert torch.equal(pb[:, :3], torch.from_numpy(go)) and torch.equal(pb[:, 82:85], torch.from_numpy(np.tile(tr, (3, 1))))
    assert torch.equal(pb[:, 72:82], fit[:, 72:82].expand(3, -1)) and torch.equal(pb[:, 85:], fit[:, 85:].expand(3, -1))
    np.savez(tmp_path / "bad.npz", body_pose=bp[:, :60])
    np.savez(tmp_path / "none.npz", pose=bp)
    np.savez(tmp_path / "go.npz", body_pose=bp, global_orient=go[:2])
    for f in ("bad.npz", "none.npz", "go.npz"):
        with pytest.raises(ValueError):
            read_pose_file(tmp_path / f)


def _np_lengths_and_areas(vertices, faces):
    """animate.py:16-27, restated."""
    v0, v1, v2 = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    e0, e1, e2 = np.linalg.norm(v1 - v0, axis=1), np.linalg.norm(v2 - v1, axis=1), np.linalg.norm(v0 - v2, axis=1)
    s = (e0 + e1 + e2) / 2
    return np.stack([e0, e1, e2], axis=1), np.sqrt(np.clip(s * (s - e0) * (s - e1) * (s - e2), 0, None))


def _np_filter(raw_v, new_v, faces):
    """animate.py:30-53, restated."""
    raw_e, raw_a = _np_lengths_and_areas(raw_v, faces)
    new_e, new_a = _np_lengths_and_areas(new_v, faces)
    er, ar = new_e / (raw_e + 1e-8), new_a / (raw_a + 1e-8)
    return np.all((er > 0.3) & (er < 2.0), axis=1) & (ar > 0.1) & (ar < 4.0)


def test_filter_faces_thresholds():
    from etch_amd.models.register import filter_faces

    # one right triangle per case, legs 1: scaled uniformly (edge and area thresholds), stretched along one leg, and collapsed
    raw = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    cases = {"same": (raw, True), "x1.9": (raw * 1.9, True), "x2.1": (raw * 2.1, False), "x0.35": (raw * 0.35, True), "x0.29": (raw * 0.29, False),
             "x0.31": (raw * 0.31, False),                                   # every edge inside (0.31), the area outside (0.0961 < 0.1)
             "thin": (raw * np.array([1.0, 0.09, 1.0]), False),              # a leg at 0.09 of its length: edge and area both out
             "flat": (np.zeros((3, 3)), False)}
    for name, (new, keep) in cases.items():
        got = filter_faces(torch.from_numpy(raw), torch.from_numpy(np.ascontiguousarray(new, np.float64)), np.array([[0, 1, 2]]))
        assert bool(got[0]) == keep == bool(_np_filter(raw, np.asarray(new, np.float64), np.array([[0, 1, 2]]))[0]), name
    # a random mesh, against the restatement, face by face
    rng = np.random.default_rng(2)
    v = rng.standard_normal((200, 3))
    f = rng.integers(0, 200, (500, 3))
    w = v + rng.standard_normal((200, 3)) * 0.4
    got = filter_faces(torch.from_numpy(v), torch.from_numpy(w), f).numpy()
    ref = _np_filter(v, w, f)
    assert got.dtype == bool and np.array_equal(got, ref) and 0 < ref.sum() < len(f)
