"""Known-answer tests against the released / user-supplied assets (the only routes by which the unpinned parts can be pinned).  Without
them each test runs on the stand-in this repository holds:

  ETCH_CKPT=<released checkpoint .pth>        strict load of the 1 924 state-dict entries + `direction` parity on the bundled scan where so3_mean is
                                              well conditioned (with a TRAINED network it is), vs the CPU oracle
                                              (default: seeded weights saved in the checkpoint's format; the direction check needs trained weights)
  ETCH_SELFCHECK_DUMP=<dump.npz>              the CUDA-box dump of INTEGRATION.md section 7 through etch_amd.selfcheck
                                              (default: tests/golden/selfcheck_dump.npz, the index sections with the oracle's answers)
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_released_checkpoint_loads_strictly_and_direction_matches_the_oracle(tmp_path):
    import types

    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.weights import seeded_state_dict
    from oracle import stage1 as S1
    args = types.SimpleNamespace(output_folder=str(tmp_path), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"), markerset=K.default_markerset())
    model = GT_network_equiv(option=args)
    ckpt = os.environ.get("ETCH_CKPT")
    trained = bool(ckpt)
    if not trained:
        # default: seeded weights saved the way the released checkpoint is (a DataParallel state dict under "state_dict")
        ckpt = str(tmp_path / "seeded.pth")
        torch.save({"state_dict": {"module." + k: v for k, v in seeded_state_dict(model, 1).items()}}, ckpt)
    sd = torch.load(ckpt, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    sd = {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)                      # 1 924 entries, names and shapes of the reference's module tree
    model = model.cuda().eval()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "scan_4ddress_5k.npz"))
    pts = torch.from_numpy(g["points"][:, :2048].copy())
    with torch.no_grad():
        res, _ = model(pts.cuda(), ["confidence", "direction", "magnitude"], "standard_vector")
    ref = S1.forward({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, pts, S1.build_layer_table(), num_markers=len(args.markerset))
    for k in ("part_labels", "confidences", "magnitude"):
        e = float((res[k].cpu() - ref[k]).abs().max() / ref[k].abs().max())
        assert e < 1e-4, (k, e)
    if trained:       # so3_mean is well conditioned with a TRAINED network; seeded weights are held to the conditioning rule of tests/_parity.py elsewhere
        d = (res["direction"].cpu() - ref["direction"]).norm(dim=-1)
        print("trained checkpoint: direction deviation median", float(d.median()), "99.9 %", float(d.flatten().kthvalue(int(0.999 * d.numel())).values), "max", float(d.max()))
        assert float(d.flatten().kthvalue(int(0.999 * d.numel())).values) < 1e-4


def test_cuda_box_dump_through_selfcheck():
    # default: the four index sections with the oracle's answers (oracle/gen_selfcheck_fixture.py) in place of a CUDA box's
    dump = os.environ.get("ETCH_SELFCHECK_DUMP") or os.path.join(os.path.dirname(__file__), "golden", "selfcheck_dump.npz")
    from etch_amd import selfcheck
    rep = selfcheck.check(dict(np.load(dump, allow_pickle=False)), os.environ.get("ETCH_SMPL_PKL"))
    print(rep)
    assert rep and all(v.get("match") is not False for v in rep.values()), rep
