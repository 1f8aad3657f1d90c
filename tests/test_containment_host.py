"""CPU checks of the containment work (no GPU): the oracle of tests/_containment_oracle.py against analytic values in fp64, the conditions the
GPU tests' inputs must meet (tests/test_gpu_containment.py relies on them), the C ABI's declarations, and the commands' argument errors."""
import numpy as np
import pytest
import torch

import _containment_oracle as C
import _surface_oracle as SO


# --------------------------------------------------------------------------------------------- the oracle against analytic values
def _inside_outside_queries(rng, n):
    """Points well inside and well outside the ellipsoid x^2/a^2 + y^2/b^2 + z^2/c^2 = 1 (its icosphere is inscribed: 0.9 and 1.1 leave room)."""
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rng.uniform(0.0, 0.9, n // 2), rng.uniform(1.1, 3.0, n - n // 2)])
    return d * r[:, None] * C.SCALE, r < 1


def test_oracle_winding_number_is_an_integer_on_a_closed_mesh():
    """The 1280-face icosphere scaled to (0.15, 0.45, 0.10): 1 inside, 0 outside, within 1e-12; with reversed faces -1 inside."""
    v, f = C.ellipsoid(3)
    assert f.shape == (1280, 3)
    q, inside = _inside_outside_queries(np.random.default_rng(1), 200)
    w = C.winding_number(v, f, q)
    err = np.abs(w - inside).max()
    print("PIN oracle winding number, closed ellipsoid: max |w - {0, 1}|", err)
    assert err <= 1e-12
    wr = C.winding_number(v, f[:, ::-1].copy(), q)
    assert np.abs(wr + inside).max() <= 1e-12


def test_oracle_winding_number_of_the_holed_sphere_is_girards():
    """The icosphere without the cap (1140 faces left), at the centre of the UNSCALED sphere: every planar face subtends the solid angle of
    its spherical triangle there, so w = 1 - (sum of the removed triangles' spherical excess) / (4 pi) -- Girard's theorem, a formula that
    shares nothing with van Oosterom-Strackee."""
    _, kept, removed = C.holed(3)
    u, _ = C.icosphere(3)
    assert len(kept) == 1140 and len(removed) == 140
    w = C.winding_number(u, kept, np.zeros((1, 3)))[0]
    want = 1.0 - C.spherical_excess(u, removed).sum() / (4 * np.pi)
    print("PIN oracle winding number, holed sphere at the centre:", w, "Girard:", want)
    assert 0.85 < want < 0.95 and abs(w - want) <= 1e-12


def test_oracle_degenerate_faces_contribute_nothing():
    v, f = C.ellipsoid(2)
    q, _ = _inside_outside_queries(np.random.default_rng(2), 40)
    more = np.concatenate([f, [[0, 1, len(v)], [-1, 2, 3]]]).astype(np.int32)                        # an index out of range: exactly nothing
    assert np.array_equal(C.winding_number(v, f, q), C.winding_number(v, more, q))
    flat = np.concatenate([f, [[5, 5, 9]]]).astype(np.int32)                                         # zero area: A . (A x C) is 0 up to rounding
    assert np.abs(C.winding_number(v, f, q) - C.winding_number(v, flat, q)).max() <= 1e-15
    nanv = v.copy()
    nanv[7, 1] = np.inf
    assert np.isnan(C.winding_number(nanv, f, q)).all()


# --------------------------------------------------------------------------------------------- conditions of the GPU tests' inputs
@pytest.mark.parametrize("name", ["closed", "odd"])
def test_winding_inputs_meet_their_conditions(name):
    """B, the chunk and block counts, no query on the surface, at most 2 % of the queries inside the band where the inside flag is not
    compared, and the entitled error e_32 the rule is built on."""
    meshes, q, lengths = C.winding_case(name)
    w64, w32 = C.winding_refs(name)
    F = [len(f) for _, f in meshes]
    assert q.shape == (len(meshes), 600, 3) and q.dtype == np.float32 and lengths.tolist() == [600] + [70] * (len(meshes) - 1)
    assert (F == [1280, 320]) if name == "closed" else (F == [1140, 320, 322])
    assert F[0] > C.CHUNK and lengths[0] > 512                                       # two chunks, two blocks
    for b, (v, f) in enumerate(meshes):
        n = lengths[b]
        _, _, d2 = C.closest_ragged([(v.astype(np.float64), f)], q[b:b + 1, :n].astype(np.float64))
        assert np.sqrt(d2.min()) > 5e-5                                              # no query lies on the surface (the nearest are 0.1 mm off)
        band = np.abs(np.abs(w64[b, :n]) - 0.5) < C.BAND
        e32 = np.abs(w32[b, :n].astype(np.float64) - w64[b, :n]).max()
        print(f"PIN winding inputs {name}[{b}]: e_32 {e32:.3e}, in the band {band.mean():.4f}, w in [{w64[b, :n].min():.4f}, {w64[b, :n].max():.4f}]")
        assert band.mean() <= 0.02 and 0 < e32 < 1e-4
        assert (np.abs(w64[b, :n]) >= 0.5).any() and (np.abs(w64[b, :n]) < 0.5).any()      # both sides are asked for
    if name == "odd":
        assert w64[0].min() < -0.01 or w64[0].max() < 0.999                          # the hole is felt
        assert w64[1].min() < -0.99                                                  # the reversed mesh reads -1 inside
        bad = meshes[2][1]
        assert (bad >= len(meshes[2][0])).any() and (bad[:, 0] == bad[:, 1]).any()


def test_trajectory_inputs_start_partly_outside():
    bm, pts, lengths, p0, w, (vids, mk, valid), prior, scans = C.trajectory_problem()
    v0 = C.verts64(bm, p0)
    for b in range(2):
        share, rms, mx = C.metrics(scans[b], v0[b])
        print(f"PIN trajectory start, scan {b}: outside_share {share:.3f}, rms {rms:.2f} mm, max {mx:.2f} mm")
        assert 0.1 < share < 0.9
    assert valid.any(1).all() and not valid.all()


@pytest.fixture(scope="module")
def why_runs():
    """The scene of the issue in the oracle's fp64: the dense-only fit and the fit with containment, same start, same schedule."""
    bm, truth, pts, lengths, scans = C.why_scene()
    _, pd = SO.fit_surface(bm, pts, lengths, truth, C.WHY_ITERS, dtype=torch.float64)
    _, pc = C.fit_surface_contain(bm, pts, lengths, truth, C.WHY_ITERS, scans, contain_every=C.WHY_EVERY)
    vt, vd, vc = (C.verts64(bm, p) for p in (truth, pd, pc))
    return [[C.metrics(scans[b], v[b]) for b in range(2)] for v in (vt, vd, vc)]


def test_why_scene_precondition(why_runs):
    """The dense-only fit pokes through: the final outside_share is at least 0.25 on both scans (the true body: below 0.01).  The ratios with
    containment are the oracle's fp64 lines of profiles/containment_pins.txt."""
    mt, md, mc = why_runs
    for b in range(2):
        print(f"PIN why scene oracle fp64 scan {b}: truth {mt[b]}, dense-only {md[b]}, contained {mc[b]}; "
              f"ratios share {mc[b][0] / md[b][0]:.3f} rms {mc[b][1] / md[b][1]:.3f}")
        assert mt[b][0] < 0.01 and md[b][0] >= 0.25
        assert mc[b][0] < md[b][0] and mc[b][1] < md[b][1]


# --------------------------------------------------------------------------------------------- the C ABI and the commands
def test_abi_declares_the_entry_points():
    from etch_amd import _lib
    from etch_amd.build import EXTRA
    names = _lib.declared_symbols()
    for n in ("etch_mesh_winding_number", "etch_ragged_mesh_closest", "etch_containment_energy_grad", "etch_smpl_surface_refine_contain"):
        assert n in names and n + "_workspace" in names
    assert EXTRA["containment.hip"] == ["-ffp-contract=off"]


def test_pack_scans_is_pack_meshes_in_fp32():
    from etch_amd.containment import pack_scans
    from etch_amd.models.fit_SMPL import Mesh
    v3, f3 = C.ellipsoid(2)
    v2, f2 = C.ellipsoid(1)
    v, f, vo, fo, mf = pack_scans([Mesh(v3, f3.astype(np.int64)), Mesh(v2, f2.astype(np.int64))], device="cpu", center=[[0.1, 0, 0], [0, 0, 0]])
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and vo.tolist() == [0, len(v3), len(v3) + len(v2)] and fo.tolist() == [0, 320, 400]
    assert mf == 320 and np.array_equal(v[:len(v3)].numpy(), (v3 - [0.1, 0, 0]).astype(np.float32)) and int(f[320:].max()) == len(v2) - 1


def _exits(fn, argv):
    with pytest.raises(SystemExit):
        fn(argv)


def test_inference_demo_flag_errors():
    from etch_amd import inference_demo as D
    base = ["--scan_path", "scan.obj"]
    _exits(D.parse_args, base + ["--surface_contain"])                                               # needs --surface_refine
    _exits(D.parse_args, base + ["--surface_refine", "--contain_w", "10"])                           # a setting without the flag
    _exits(D.parse_args, base + ["--surface_refine", "--contain_every", "5"])
    _exits(D.parse_args, base + ["--surface_refine", "--surface_contain", "--contain_every", "0"])
    _exits(D.parse_args, base + ["--surface_refine", "--surface_contain", "--contain_w", "-1"])
    a = D.parse_args(base + ["--surface_refine", "--surface_contain"])
    assert D.surface_contain_settings(a) == dict(w_contain=1e2, contain_every=10)
    a = D.parse_args(base + ["--surface_refine", "--surface_contain", "--contain_w", "30", "--contain_every", "4", "--ingest", "device"])
    assert D.surface_contain_settings(a) == dict(w_contain=30.0, contain_every=4)
    assert D.surface_contain_settings(D.parse_args(base + ["--surface_refine"])) is None
    assert D.surface_refine_settings(a) == dict(iterations=200, trunc=0.05, w_dense=1e2)             # the refinement's own settings are what they were


def test_eval_flag_errors():
    from etch_amd import eval as E
    _exits(E.main, ["--surface_contain"])                                                            # needs --surface_refine
    _exits(E.main, ["--surface_refine", "--surface_contain", "--ingest", "host"])                    # host-ingest items carry no mesh
    _exits(E.main, ["--surface_refine", "--surface_contain", "--view_azimuth", "30"])                # a single view has no inside
    _exits(E.main, ["--surface_refine", "--contain_every", "3"])
    p = E.build_parser()
    a = p.parse_args(["--surface_refine", "--surface_contain", "--contain_every", "3"])
    assert E.contain_from_args(p, a, None) == dict(w_contain=1e2, contain_every=3)
    assert E.contain_from_args(p, p.parse_args(["--surface_refine"]), None) is None
