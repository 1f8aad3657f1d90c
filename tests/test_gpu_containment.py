"""GPU checks of the containment kernels (csrc/containment.hip): the winding number against the fp64 restatement by the entitled-error rule,
the ragged closest point bit for bit, the containment term and its gradient against fp64 autograd, the refinement with the fifth term
against the fp64 restatement of its schedule (tests/_containment_oracle.py), the scene of DESIGN 18 and the two commands' flags.
tests/test_containment_host.py asserts, without a GPU, the conditions these inputs must meet."""
import functools

import numpy as np
import pytest
import torch

import _containment_oracle as C
import _surface_oracle as SO
from tests._pt_fp64 import check

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pack(meshes):
    """[(verts f32, faces i32)] -> the packed batch on the device, as containment.pack_scans lays it out (without its face-index check: the
    kernels must stand a face that points outside its scan)."""
    vo = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int32)
    return (_dev(np.concatenate([v for v, _ in meshes]).astype(np.float32)), _dev(np.concatenate([f for _, f in meshes]).astype(np.int32)), _dev(vo), _dev(fo),
            int(max(len(f) for _, f in meshes)))


def _winding(meshes, q, lengths=None):
    from etch_amd import ops
    return ops.mesh_winding_number(_pack(meshes), _dev(q), None if lengths is None else _dev(lengths)).cpu().numpy()


# --------------------------------------------------------------------------------------------- winding number
@pytest.mark.parametrize("name", ["closed", "odd"])
def test_winding_number_vs_fp64(name):
    """Per scan e_gpu <= 2 e_32 + 1e-6 against the oracle's fp64 (e_32: the oracle's own fp32 run, the rule of tests/_pt_fp64.py); the inside
    flag |w| >= 0.5 equals the fp64 flag wherever | |w64| - 0.5 | >= 0.05; padding gets 0; batch against alone and run against run bitwise.
    closed: 1280 faces (two chunks) and 320, Q = 600 (two blocks) and 70; odd: a holed mesh, a reversed one, one with a face whose index is
    out of range and a zero-area face."""
    meshes, q, lengths = C.winding_case(name)
    w64, w32 = C.winding_refs(name)
    w = _winding(meshes, q, lengths)
    assert w.dtype == np.float32 and w.shape == w64.shape
    for b in range(len(meshes)):
        n = lengths[b]
        e_gpu = np.abs(w[b, :n].astype(np.float64) - w64[b, :n]).max()
        e_32 = np.abs(w32[b, :n].astype(np.float64) - w64[b, :n]).max()
        print(f"PIN winding number {name}[{b}]: e_gpu {e_gpu:.3e}, e_32 {e_32:.3e}")
        assert e_gpu <= 2 * e_32 + 1e-6, (name, b, e_gpu, e_32)
        far = np.abs(np.abs(w64[b, :n]) - 0.5) >= C.BAND
        assert np.array_equal(np.abs(w[b, :n][far]) >= 0.5, np.abs(w64[b, :n][far]) >= 0.5)
        assert (w[b, n:] == 0).all()
        one = _winding(meshes[b:b + 1], q[b:b + 1, :n].copy())                                     # scan b alone: bitwise
        assert np.array_equal(one[0].view(np.uint32), w[b, :n].view(np.uint32))
    assert np.array_equal(_winding(meshes, q, lengths).view(np.uint32), w.view(np.uint32))         # two runs: bitwise
    garbage = q.copy()                                                                             # what lies past the lengths changes nothing
    garbage[1, lengths[1]:] = np.nan
    assert np.array_equal(_winding(meshes, garbage, lengths).view(np.uint32), w.view(np.uint32))


def test_winding_number_non_finite_vertex_is_nan():
    meshes, q, lengths = C.winding_case("closed")
    v = meshes[1][0].copy()
    v[7, 1] = np.inf
    w = _winding([meshes[0], (v, meshes[1][1])], q, lengths)
    assert np.isnan(w[1, :lengths[1]]).all() and np.isfinite(w[0]).all() and (w[1, lengths[1]:] == 0).all()


# --------------------------------------------------------------------------------------------- ragged closest point
def test_ragged_closest_is_bitwise_the_fp32_restatement():
    """The two closed meshes and their ragged queries, scan by scan against tests/_surface_oracle.py closest_batch: face, bary and d2 bit for bit."""
    from etch_amd import ops
    meshes, q, lengths = C.winding_case("closed")
    face, bary, d2 = (t.cpu().numpy() for t in ops.ragged_mesh_closest(_pack(meshes), _dev(q), _dev(lengths)))
    for b, (v, f) in enumerate(meshes):
        rf, rb, rd, _ = SO.closest_batch(q[b:b + 1], lengths[b:b + 1], v[None], f)
        assert np.array_equal(face[b], rf[0]) and np.array_equal(bary[b].view(np.uint32), rb[0].view(np.uint32))
        assert np.array_equal(d2[b].view(np.uint32), rd[0].view(np.uint32))
        assert (face[b, :lengths[b]] >= 0).all() and (face[b, lengths[b]:] == -1).all()
    assert face[0].max() >= 1024                                                                   # the second chunk wins somewhere


def test_ragged_closest_equals_the_shared_face_kernel_and_stands_bad_faces():
    from etch_amd import ops
    meshes, q, lengths = C.winding_case("closed")
    v, f = meshes[1]
    vs = np.stack([v, v * np.float32(1.1)])
    qq = q[:, :300].copy()
    nl = np.array([300, 70], np.int32)
    a = ops.ragged_mesh_closest(_pack([(vs[0], f), (vs[1], f)]), _dev(qq), _dev(nl))
    s = ops.point_mesh_closest(_dev(qq), _dev(vs), _dev(f), _dev(nl))
    assert all(torch.equal(x, y) for x, y in zip(a, s))
    bad = np.concatenate([[[0, 1, len(v)]], f, [[5, 5, 9]]]).astype(np.int32)                      # a bad face first: the others move up by one
    c = ops.ragged_mesh_closest(_pack([(vs[0], bad), (vs[1], f)]), _dev(qq), _dev(nl))
    assert torch.equal(c[0][0, :300], a[0][0, :300] + 1) and torch.equal(c[2], a[2]) and torch.equal(c[0][1], a[0][1])


# --------------------------------------------------------------------------------------------- the term and its gradient
@functools.lru_cache(maxsize=None)
def _energy_problem():
    from etch_amd import ops
    bm, _, _, p0, _, _, _, scans = C.trajectory_problem()
    body = C.verts64(bm, p0).astype(np.float32)
    mesh = _pack(scans)
    bv = _dev(body)
    w = ops.mesh_winding_number(mesh, bv)
    face, bary, d2 = ops.ragged_mesh_closest(mesh, bv)
    return scans, mesh, body, bv, w, face, bary, d2


def test_energy_and_gradient_vs_fp64():
    """terms to 1e-12 relative from the kernel's own flags and d2; g under check() of tests/_pt_fp64.py against fp64 autograd of
    coef_b w_contain (sum_v o_v |v - c_v|^2) / V with the kernel's flags and correspondences; vertices that are inside keep g's bits."""
    from etch_amd import ops
    scans, mesh, body, bv, w, face, bary, d2 = _energy_problem()
    B, V = body.shape[:2]
    coef = np.array([0.7, 1.9], np.float32)
    wn, fc, bc, dd = (t.cpu().numpy() for t in (w, face, bary, d2))
    wn2 = wn.copy()
    wn2[0, 5] = np.nan                                                                             # a NaN w is not outside
    fc2 = fc.copy()
    out_idx = np.flatnonzero(np.abs(wn[1]) < 0.5)
    fc2[1, out_idx[0]] = -1                                                                        # a vertex without a face is not outside
    o = (np.abs(np.nan_to_num(wn2, nan=1.0)) < 0.5) & (fc2 >= 0)
    assert 0.1 < o.mean() < 0.9
    terms, g = ops.containment_energy_grad(bv, mesh, _dev(wn2), _dev(fc2), bary, d2, coef=_dev(coef), w_contain=1e2)
    terms, g = terms.cpu().numpy(), g.cpu().numpy()
    want = np.stack([(o * dd.astype(np.float64)).sum(1), o.sum(1).astype(np.float64)], 1)
    rel = np.abs(terms - want) / np.abs(want)
    print("PIN containment terms: max relative error", rel.max())
    assert terms.dtype == np.float64 and (rel <= 1e-12).all(), (terms, want)

    def ref(dt):
        v = torch.from_numpy(body).to(dt).requires_grad_(True)
        tot = 0
        for b in range(B):
            sv, sf = scans[b]
            tri = torch.from_numpy(sv).to(dt)[torch.from_numpy(sf.astype(np.int64))[torch.from_numpy(np.maximum(fc2[b], 0)).long()]]
            c = (torch.from_numpy(bc[b]).to(dt)[:, :, None] * tri).sum(1)
            ob = torch.from_numpy(o[b])
            tot = tot + float(coef[b]) * 1e2 * ((v[b][ob] - c[ob]) ** 2).sum() / V
        tot.backward()
        return v.grad.numpy()

    check("containment dL/dverts", g, ref(torch.float64), ref(torch.float32))
    assert (g[~o] == 0).all() and (np.abs(g[o]).sum(-1) > 0).all()
    # the term is ADDED: the inside vertices of a g handed in keep their bits, the outside ones move by the term
    g0 = np.random.default_rng(5).standard_normal(body.shape).astype(np.float32)
    _, g1 = ops.containment_energy_grad(bv, mesh, _dev(wn2), _dev(fc2), bary, d2, coef=_dev(coef), w_contain=1e2, g=_dev(g0))
    g1 = g1.cpu().numpy()
    assert np.array_equal(g1[~o].view(np.uint32), g0[~o].view(np.uint32))
    assert np.abs((g1[o].astype(np.float64) - g0[o]) - g[o]).max() <= 2e-7 * max(np.abs(g0).max(), np.abs(g).max())
    _, gz = ops.containment_energy_grad(bv, mesh, _dev(wn2), _dev(fc2), bary, d2, w_contain=0.0, g=_dev(g0))      # zero weight: every bit stays
    assert np.array_equal(gz.cpu().numpy().view(np.uint32), g0.view(np.uint32))


# --------------------------------------------------------------------------------------------- the refinement
def _init(p):
    return dict(pose=p[:, :72], beta=p[:, 72:82], trans=p[:, 82:85], scale=p[:, 85:])


def _packed(prm):
    return torch.cat([prm["pose"], prm["beta"], prm["trans"], prm["scale"]], 1).cpu().numpy()


def _fit(iters, lr=5e-3, **kw):
    from etch_amd.models.surface_refine import fit_surface
    bm, pts, lengths, p0, w, (vids, mk, valid), prior, scans = C.trajectory_problem()
    return fit_surface(bm, _dev(pts), _init(p0), weights=w, lengths=lengths, iterations=iters, lr=lr, want_trace=True, markers=mk, valid=valid,
                       marker_vids=vids, prior=prior, **kw)


def test_zero_weight_is_bitwise_the_old_entry_point():
    """etch_smpl_surface_refine_contain with w_contain = 0 (every kernel of the term still runs, at contain_every = 2): the parameters, the
    vertices and the first four trace columns are bitwise those of etch_smpl_surface_refine; the fifth column is 0."""
    scans = C.trajectory_problem()[-1]
    v0, prm0 = _fit(6)
    v1, prm1 = _fit(6, scan=_pack(scans), w_contain=0.0, contain_every=2)
    assert prm0["loss_trace"].shape == (2, 6, 4) and prm1["loss_trace"].shape == (2, 6, 5)
    assert np.array_equal(_packed(prm0).view(np.uint32), _packed(prm1).view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
    assert torch.equal(prm0["loss_trace"], prm1["loss_trace"][:, :, :4]) and bool((prm1["loss_trace"][:, :, 4] == 0).all())
    assert "outside_share" in prm1 and "outside_share" not in prm0 and bool((prm1["outside_share"] > 0).all())


@pytest.mark.parametrize("iters,every", [(12, 1), (7, 3)])
def test_fit_surface_contain_vs_fp64(iters, every):
    """Every column of loss_trace (B, iters, 5) and the final parameters against the oracle's fp64 run under the rule of
    test_fit_surface_20_iterations_vs_fp64: err <= max(2 ent, 1e-4), ent = the oracle's own fp32 run, each relative to the largest magnitude
    of its own column; on its smooth body (zero betas, pose 0.05 rad) at its quarter step, for the reasons its docstring gives -- they hold
    for a body vertex's closest location on the scan as they do for a point's on the body.  contain_every = 3 over 7 iterations puts the
    refreshes at 0, 3 and 6 and holds o_v and c_v in between.
    A flip of o_v between two runs is benign: |w| crosses 0.5 AT the scan's surface, where d2_v = 0, so the vertex that one run counts and
    the other does not contributes ~0 to the term and to its gradient (the term is zero and flat there by construction)."""
    bm, pts, lengths, p0, w, (vids, mk, valid), prior, scans = C.trajectory_problem()
    _, prm = _fit(iters, scan=_pack(scans), w_contain=1e2, contain_every=every)
    tr, pg = prm["loss_trace"].cpu().numpy(), _packed(prm)
    assert tr.shape == (2, iters, 5)
    okw = dict(lr=5e-3, w_contain=1e2, contain_every=every, weights=w, markers=(vids, mk, valid), prior=prior)
    t64, p64 = C.fit_surface_contain(bm, pts, lengths, p0, iters, scans, dtype=torch.float64, **okw)
    t32, p32 = C.fit_surface_contain(bm, pts, lengths, p0, iters, scans, dtype=torch.float32, **okw)
    for name, got, r64, r32 in [(f"trace[{q}]", tr[:, :, q], t64[:, :, q], t32[:, :, q]) for q in range(5)] + [("params", pg, p64, p32)]:
        s = np.abs(r64).max()
        err, ent = np.abs(got - r64).max() / s, np.abs(r32 - r64).max() / s
        print(f"PIN fit_surface_contain {name} iters={iters} every={every}: err {err:.3e}, ent {ent:.3e}")
        assert err <= max(2 * ent, 1e-4), (name, err, ent)
    assert (tr > 0).all() or (tr[:, :, 3] != 0).all() and (tr[:, :, [0, 1, 2, 4]] > 0).all()     # every term is at work
    # the comparison can see the term: the fp64 run without it ends elsewhere
    if every == 3:                                                                                 # (once: the shorter schedule)
        _, p64n = SO.fit_surface(bm, pts, lengths, p0, iters, 5e-3, weights=w, markers=(vids, mk, valid), prior=prior, dtype=torch.float64)
        assert np.abs(p64 - p64n).max() / np.abs(p64n).max() > 20 * 1e-4
    again = _fit(iters, scan=_pack(scans), w_contain=1e2, contain_every=every)[1]                  # two runs: bitwise
    assert torch.equal(again["loss_trace"], prm["loss_trace"]) and np.array_equal(_packed(again), pg)


def test_containment_keeps_the_body_inside_the_scan():
    """The scene of DESIGN 18, B = 2 (another seed and a ragged length for the second scan): a scan 8 mm outside the true body, inner
    points whose front half is biased 2 cm outward, 40 iterations from the truth.  With containment (w_contain 1e2, refreshed every 10)
    outside_share and protrusion_rms_mm are strictly smaller than the dense-only run's on both scans.  No ratio is fixed: the figures are
    the PIN lines (profiles/containment_pins.txt, beside the oracle's fp64 ratios for the same schedule)."""
    from etch_amd.containment import containment_metrics, signed_distance, winding_number
    from etch_amd.models.fit_SMPL import Mesh
    from etch_amd.models.surface_refine import fit_surface
    bm, truth, pts, lengths, scans = C.why_scene()
    meshes = [Mesh(v.astype(np.float64), f.astype(np.int64)) for v, f in scans]
    run = lambda **kw: fit_surface(bm, _dev(pts), _init(truth), lengths=lengths, iterations=C.WHY_ITERS, **kw)
    vd, _ = run()
    vc, prm = run(scan=meshes, w_contain=1e2, contain_every=C.WHY_EVERY)
    md, mc = containment_metrics(meshes, vd), containment_metrics(_pack(scans), vc)
    for b in range(2):
        print(f"PIN why scene scan {b}: dense-only {md[b]}, contained {mc[b]}; ratios share {mc[b]['outside_share'] / md[b]['outside_share']:.3f} "
              f"rms {mc[b]['protrusion_rms_mm'] / md[b]['protrusion_rms_mm']:.3f}")
        assert md[b]["outside_share"] >= 0.25
        assert mc[b]["outside_share"] < md[b]["outside_share"] and mc[b]["protrusion_rms_mm"] < md[b]["protrusion_rms_mm"]
        assert mc[b]["protrusion_max_mm"] >= mc[b]["protrusion_rms_mm"] > 0
    assert np.allclose(prm["outside_share"].numpy(), [m["outside_share"] for m in mc])
    # signed_distance: negative exactly where the winding number says outside, |.| = the distance to the scan
    sd = signed_distance(meshes, vc).cpu().numpy()
    wn = winding_number(meshes, vc).cpu().numpy()
    assert np.array_equal(sd < 0, (np.abs(wn) < 0.5) & (sd != 0)) and abs(np.abs(sd[sd < 0]).max() * 1e3 - max(m["protrusion_max_mm"] for m in mc)) < 1e-3
    inside = containment_metrics(meshes, np.stack([v * 0.5 + v.mean(0) * 0.5 for v, _ in scans]).astype(np.float32))     # shrunk scans: all inside
    assert all(m == dict(outside_share=0.0, protrusion_rms_mm=0.0, protrusion_max_mm=0.0) for m in inside)


def test_argument_checks():
    from etch_amd import _lib, ops
    from etch_amd.models.surface_refine import fit_surface
    meshes, q, lengths = C.winding_case("closed")
    mesh = _pack(meshes)
    with pytest.raises(_lib.EtchHipError):
        ops.mesh_winding_number(mesh, _dev(q[:1]))                                                 # one scan of queries, two meshes
    with pytest.raises(_lib.EtchHipError):
        ops.mesh_winding_number(mesh[:4] + (10 ** 6,), _dev(q))                                    # max_faces beyond the batch
    with pytest.raises(_lib.EtchHipError):
        ops.ragged_mesh_closest((mesh[0].double(),) + mesh[1:], _dev(q))
    with pytest.raises(_lib.EtchHipError):
        ops.containment_energy_grad(_dev(q), mesh, _dev(q[:, :, 0]), _dev(q[:, :, 0]).int(), _dev(q), _dev(q[:, :10, 0]))
    bm, truth, pts, lengths, scans = C.why_scene()
    with pytest.raises(ValueError):
        fit_surface(bm, _dev(pts), _init(truth), scan=_pack(scans), contain_every=0)
    with pytest.raises(_lib.EtchHipError):
        fit_surface(bm, _dev(pts), _init(truth), scan=_pack(scans[:1]), iterations=1)               # one scan mesh for two bodies


# --------------------------------------------------------------------------------------------- the commands
def _write_obj(path, v, f):
    path.write_text("".join("v %.8f %.8f %.8f\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))


def _checkpoint(tmp_path):
    import types

    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import load_seeded
    a = types.SimpleNamespace(output_folder=str(tmp_path / "ckpt_model"), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device(DEV),
                              markerset=K.default_markerset(), scale_magnitude=10, body_model=None)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({k: v.cpu() for k, v in load_seeded(GT_network_equiv(option=a), 1).state_dict().items()}, ckpt)
    return ckpt


@pytest.mark.parametrize("ingest", ["host", "device"])
def test_cli_surface_contain(tmp_path, capsys, ingest):
    """inference_demo --synthetic_body --surface_refine --surface_contain on a small closed OBJ, under both --ingest modes: the three metrics
    are printed before and after, the outputs are written."""
    from etch_amd import inference_demo as D
    v, f = C.ellipsoid(2)
    obj = tmp_path / "scan.obj"
    _write_obj(obj, v * 2.0 + np.array([0.3, 1.0, -0.2]), f)
    out = tmp_path / "out"
    D.main(["--scan_path", str(obj), "--synthetic_body", "--output_folder", str(out), "--num_point", "1024", "--markerset_path", "missing.json",
            "--model_path", str(_checkpoint(tmp_path)), "--surface_refine", "--surface_iters", "4", "--surface_contain", "--contain_every", "2",
            "--ingest", ingest])
    text = capsys.readouterr().out
    lines = [l for l in text.split("\n") if l.startswith("containment ")]
    assert len(lines) == 2 and "before" in lines[0] and "after" in lines[1]
    for l in lines:
        vals = l.split(": ")[1].split()
        assert vals[0::2] == ["outside_share", "protrusion_rms_mm", "protrusion_max_mm"] and all(np.isfinite(float(x)) for x in vals[1::2])
        assert 0.0 <= float(vals[1]) <= 1.0
    z = np.load(out / "scan_output_smpl_info.npz")
    assert np.isfinite(z["betas"]).all() and (out / "scan_pred_smpl.obj").exists()
    with pytest.raises(SystemExit):
        D.main(["--scan_path", str(obj), "--synthetic_body", "--surface_contain"])


def test_eval_surface_contain_writes_containment_txt(tmp_path):
    """eval --surface_contain on a two-scan dataset in the reference's layout: the three metrics (and their _before) in every record and a
    line per sample in containment.txt beside v2v_score.txt, whose format does not change."""
    import json

    from etch_amd import constants as K
    from etch_amd import eval as E
    v, f = C.ellipsoid(2)
    for i, s in (("a01", 2.0), ("b02", 1.8)):
        (tmp_path / "scan" / i).mkdir(parents=True)
        (tmp_path / "smpl" / i).mkdir(parents=True)
        _write_obj(tmp_path / "scan" / i / f"{i}.obj", v * s, f)
        rng = np.random.default_rng(3)
        _write_obj(tmp_path / "smpl" / i / f"mesh_smpl_{i}.obj", rng.standard_normal((6890, 3)) * 0.3, np.array([[0, 1, 2]]))
        np.savez(tmp_path / "smpl" / i / f"info_{i}.npz", gender=np.array(1))
        (tmp_path / "info").mkdir(exist_ok=True)
        np.savez(tmp_path / "info" / f"{i}.npz", x=np.zeros(1))
    ms = tmp_path / "markers.json"
    ms.write_text(json.dumps(K.default_markerset()))
    argv = ["--scan_dir", str(tmp_path / "scan"), "--smpl_dir", str(tmp_path / "smpl"), "--infopoints_dir", str(tmp_path / "info"), "--activated_ids_path", "",
            "--markerset_path", str(ms), "--model_path", str(_checkpoint(tmp_path)), "--synthetic_body", "--output_root", str(tmp_path / "exp"), "--i", "t",
            "--num_point", "1024", "--batch_size", "2", "--surface_refine", "--surface_iters", "3", "--surface_contain", "--contain_every", "2"]
    recs, _ = E.main(argv)
    keys = ("outside_share", "protrusion_rms_mm", "protrusion_max_mm")
    assert len(recs) == 2 and all(k in r and k + "_before" in r and np.isfinite(r[k]) for r in recs for k in keys)
    out = tmp_path / "exp" / "eval_outputs_t"
    lines = (out / "containment.txt").read_text().strip().split("\n")
    assert [l.split(":")[0] for l in lines] == ["a01", "b02"] and all("outside_share" in l and "protrusion_max_mm" in l for l in lines)
    score = (out / "v2v_score.txt").read_text().split("\n")
    assert score[0].startswith("a01: ") and score[2] == "==========" and score[3].startswith("average v2v: ")
    with pytest.raises(SystemExit):
        E.main(argv + ["--view_azimuth", "20"])
    with pytest.raises(SystemExit):
        E.main(argv + ["--ingest", "host"])
