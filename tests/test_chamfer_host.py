"""CPU checks of the chamfer refinement: the restated schedule, loss and prior against hand-computed values, the library's new
symbols, and the demo's --chamfer_refine flag."""
import math

import numpy as np
import torch

import _chamfer_oracle as O


def test_lr_schedule_by_hand():
    # the script sets lr * (N - i) / N AFTER step i: steps 0 and 1 both run at lr
    assert [O.lr_at(i, 4, 0.02) for i in range(4)] == [0.02, 0.02, 0.02 * 3 / 4, 0.02 * 2 / 4]


def test_prior_by_hand():
    means = torch.zeros(2, 69, dtype=torch.float64)
    means[1, 0] = 1.0
    prec = torch.stack([torch.eye(69), 2 * torch.eye(69)]).double()
    w = torch.tensor([0.5, 0.25], dtype=torch.float64)
    pose = torch.zeros(1, 69, dtype=torch.float64)
    pose[0, 0] = 1.0
    # g0: 0.5 * 1 * 1 - log 0.5 = 0.5 + 0.693 = 1.193;  g1: 0 - log 0.25 = 1.386  -> min = g0
    assert abs(float(O.prior_nll(pose, means, prec, w)[0]) - (0.5 + math.log(2))) < 1e-12


def test_scan_loss_by_hand():
    verts = torch.tensor([[0.0, 0, 0], [1.0, 0, 0]], dtype=torch.float64)
    scan = torch.tensor([[0.0, 0.5, 0], [2.0, 0, 0]], dtype=torch.float64)
    # scan -> body: 0.25 + 1 = 1.25;  body -> scan: 0.25 + min(1 + 0.25, 1) = 1.25
    s1 = math.sqrt(1.25)
    assert abs(float(O.scan_loss(verts, scan, 1)) - s1) < 1e-12
    assert abs(float(O.scan_loss(verts, scan, -1)) - math.sqrt(1.25)) < 1e-12
    assert abs(float(O.scan_loss(verts, scan, 0)) - 2 * s1) < 1e-12


def test_total_loss_regulariser_by_hand():
    from etch_amd.utils.body_model import SyntheticSMPL
    from oracle import stage2 as S2

    bm = SyntheticSMPL(7, V=64)
    tb = S2.TorchBody(bm, torch.float64)
    p = torch.zeros(1, 72 + 10 + 4, dtype=torch.float64)
    p[0, -1] = 1.0
    p[0, 72:82] = 1.0                                  # mean(beta^2) = 1 -> + 0.2
    verts, _ = O.forward(tb, p, 24, 10)
    scan = verts.detach().clone()
    l = O.total_loss(tb, p, scan, [64], 0, None, 24, 10)
    assert abs(float(l[0]) - 0.2) < 1e-12            # the scan IS the mesh: the data term is 0


def test_library_exports_refine_symbols():
    from etch_amd import _lib
    from etch_amd import build as B

    B.build()
    names = _lib.declared_symbols()
    for n in ("etch_nn_bidir", "etch_chamfer_grad", "etch_smpl_lbs_vjp", "etch_smpl_chamfer_refine", "etch_smpl_chamfer_refine_workspace"):
        assert n in names and hasattr(_lib.lib(), n), n
    assert not any(n.endswith("_launcher") for n in names)


def test_cli_parses_chamfer_refine_and_default_is_unchanged():
    from etch_amd import inference_demo as D

    a = D.parse_args(["--scan_path", "x.obj"])
    assert a.chamfer_refine == "none" and a.refine_iters == 500
    before = {"scan_path": "x.obj", "gender": "neutral", "model_path": "", "markerset_path": "datafolder/useful_data_4d-dress/superset_smpl.json",
              "output_folder": "output", "num_point": 5000, "scale_magnitude": 10, "EPN_input_radius": 0.4, "EPN_layer_num": 2, "body_model": "",
              "synthetic_body": False, "seed": 0}
    got = {k: v for k, v in vars(a).items() if k not in ("chamfer_refine", "refine_iters")}
    assert got == before
    for mode in ("both", "partial", "clutter"):
        b = D.parse_args(["--scan_path", "x.obj", "--chamfer_refine", mode, "--refine_iters", "20"])
        assert b.chamfer_refine == mode and b.refine_iters == 20
    import pytest

    with pytest.raises(SystemExit):
        D.parse_args(["--scan_path", "x.obj", "--chamfer_refine", "sideways"])


def test_random_prior_is_spd():
    m, p, w = O.random_prior(3)
    assert m.shape == (8, 69) and p.shape == (8, 69, 69) and np.all(np.linalg.eigvalsh(p.astype(np.float64)) > 0.5) and abs(w.sum() - 1) < 1e-6
