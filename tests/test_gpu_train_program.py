"""python -m etch_amd.train end to end on a two-id dataset on disk (built as test_gpu_geodesic.test_gtdataset_end_to_end builds its own, from the
geodesic fixture's body, num_point = 512): the reference's files, reproducibility, --resume, the fused step against --reference_step, --pred_items,
the NaN guard and --aug."""
import json
import math
import os
import pickle
import types

import numpy as np
import pytest
import torch

import _geodesic_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geodesic_4ddress.npz")
NUM_POINT = 512
LR = 1e-4
WEIGHTS = ["--direction_w", "2.5", "--magnitude_w", "30", "--part_label_w", "1", "--confidence_w", "50"]


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.writelines(f"v {x:.8f} {y:.8f} {z:.8f}\n" for x, y, z in v)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The dataset on disk and the flags that point the program at it."""
    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.inference_demo import Mesh, load_obj
    from etch_amd.infopoints import generate_infopoints, save_data

    root = tmp_path_factory.mktemp("train_data")
    z = O.load_fixture(GOLDEN)
    verts, faces = z["vertices_q"].astype(np.int64) / 1e8, z["faces"].astype(np.int64)
    ids = ["a_0001", "b_0002"]
    body = Mesh(verts, faces)
    n = ops.vertex_normals(torch.as_tensor(verts, device=DEV), torch.as_tensor(faces, device=DEV).to(torch.int32)).cpu().numpy()
    os.makedirs(root / "ip")
    for k, i in enumerate(ids):
        off = np.random.default_rng(k).uniform(0.01, 0.03, (len(verts), 1))
        for d in ("scan", "smpl"):
            os.makedirs(root / d / i)
        _write_obj(root / "scan" / i / f"{i}.obj", verts + off * n, faces)
        _write_obj(root / "smpl" / i / f"mesh_smpl_{i}.obj", verts, faces)
        np.savez(root / "smpl" / i / f"info_{i}.npz", gender=np.array(k))
        ip, iv, _ = generate_infopoints(load_obj(str(root / "scan" / i / f"{i}.obj")), body, num_samples=3000, seed=k, device=DEV)
        save_data(ip, iv, str(root / "ip" / f"{i}.npz"))
    with open(root / "ids.pkl", "wb") as fh:
        pickle.dump(ids, fh)
    with open(root / "markers.json", "w") as fh:
        json.dump(K.default_markerset(), fh)
    flags = ["--activated_ids_path", str(root / "ids.pkl"), "--markerset_path", str(root / "markers.json"), "--infopoints_dir", str(root / "ip"),
             "--scan_dir", str(root / "scan"), "--smpl_dir", str(root / "smpl"), "--num_point", str(NUM_POINT), "--batch_size", "2", "--seed", "3",
             "--vis_loss", "false"] + WEIGHTS
    return types.SimpleNamespace(root=root, flags=flags)


def _folder(root):
    return os.path.join(str(root), f"EPN_layer_2_radius_0.4_num_point_{NUM_POINT}")


@pytest.fixture(scope="module")
def run_a(data):
    from etch_amd import train
    out = data.root / "run_a"
    last = train.main(data.flags + ["--epochs", "2", "--output_root", str(out), "--vis_loss", "true"])
    return types.SimpleNamespace(folder=_folder(out), last=last)


@pytest.fixture(scope="module")
def setup(data):
    """A model, the parsed arguments and one batch of the dataset, for the tests that drive train() themselves."""
    from etch_amd import train
    from etch_amd.datasets import GTDataset
    args = train.build_parser().parse_args(data.flags + ["--output_root", str(data.root / "direct")])
    args.pred_items = args.pred_items.split(",")
    args.device = torch.device("cuda:0")
    args.output_folder = str(data.root / "direct")
    with open(args.markerset_path) as fh:
        args.markerset = json.load(fh)
    ds = GTDataset(args, device=args.device, verbose=False)
    items = [ds[0], ds[1]]
    batch = {k: torch.stack([it[k] for it in items]) for k in ("hitpts", "vectors", "confidences", "labels")}
    return types.SimpleNamespace(args=args, batch=batch)


def _fresh(setup, **over):
    """(args copy, model, optimizer) from the same seeded start."""
    from etch_amd import train
    args = types.SimpleNamespace(**vars(setup.args))
    for k, v in over.items():
        setattr(args, k, v)
    train.default_stuff(args.seed)
    model = train.make_model(args)
    return args, model, train.make_optimizer(args, model)


def _load(path):
    return torch.load(path, map_location="cpu")


def test_files_checkpoint_and_epoch_dict(run_a, setup):
    from etch_amd import train
    f = run_a.folder
    for name in ("training_args.json", "model_epochs_00000000.pth", "model_epochs_00000001.pth", "train_state_00000000.pth", "train_state_00000001.pth",
                 os.path.join("log_all", "train", "losses.json")):
        assert os.path.isfile(os.path.join(f, name)), name
    try:
        import matplotlib  # noqa: F401
        assert os.path.isfile(os.path.join(f, "log_all", "train", "direction_loss.png"))
    except ImportError:
        pass
    keys = {"direction_loss", "magnitude_loss", "confidence_loss", "part_label_loss"}
    assert set(run_a.last) == keys and all(math.isfinite(v) for v in run_a.last.values())
    with open(os.path.join(f, "log_all", "train", "losses.json")) as fh:
        log = json.load(fh)
    assert set(log) == keys and all(len(v) == 2 for v in log.values())
    with open(os.path.join(f, "training_args.json")) as fh:
        assert json.load(fh)["num_point"] == NUM_POINT
    sd = _load(os.path.join(f, "model_epochs_00000001.pth"))
    model = train.make_model(setup.args)
    assert list(sd.keys()) == list(model.state_dict().keys())
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        res, _ = model(setup.batch["hitpts"][:1].to(DEV), ["confidence", "direction", "magnitude"], "standard_vector")
    assert all(torch.isfinite(v).all() for v in res.values())


def _same_checkpoint(run_a, folder, epoch):
    want = _load(os.path.join(run_a.folder, f"model_epochs_{epoch:08d}.pth"))
    got = _load(os.path.join(folder, f"model_epochs_{epoch:08d}.pth"))
    bad = [k for k in want if not torch.equal(want[k], got[k])]
    assert not bad, (epoch, folder, bad[:5], len(bad))


def test_second_run_with_the_same_seed_is_bit_identical(run_a, data):
    from etch_amd import train
    out = data.root / "run_b"
    train.main(data.flags + ["--epochs", "2", "--output_root", str(out)])
    for epoch in (0, 1):
        _same_checkpoint(run_a, _folder(out), epoch)


def test_resume_after_epoch_0_reproduces_epoch_1(run_a, data):
    from etch_amd import train
    out = data.root / "run_c"
    train.main(data.flags + ["--epochs", "2", "--output_root", str(out), "--resume", os.path.join(run_a.folder, "train_state_00000000.pth")])
    _same_checkpoint(run_a, _folder(out), 1)
    assert not os.path.exists(os.path.join(_folder(out), "model_epochs_00000000.pth"))


def _reference_losses(results, sel, vectors, confidences, labels):
    """train.py:81-101 with the weights of WEIGHTS and scale_magnitude 10."""
    F = torch.nn.functional
    vectors_k = torch.gather(vectors, 1, sel)
    labels_k = torch.gather(labels, 1, sel[:, :, 0])
    confidences_k = torch.gather(confidences, 1, sel[:, :, 0].unsqueeze(-1))
    return {"direction_loss": (1 - F.cosine_similarity(vectors_k, results["direction"], dim=-1)).mean() * 2.5,
            "magnitude_loss": F.mse_loss(torch.norm(vectors_k, dim=-1, keepdim=True) * 10, results["magnitude"]) * 30.0,
            "confidence_loss": F.mse_loss(results["confidences"], confidences_k) * 50.0,
            "part_label_loss": F.cross_entropy(results["part_labels"].permute(0, 2, 1).contiguous(), labels_k) * 1.0}


def test_fused_step_against_reference_step(setup):
    from etch_amd import train
    seen = {}
    params = {}
    for mode in ("fused", "reference"):
        args, model, opt = _fresh(setup, reference_step=mode == "reference", on_step=lambda s, mode=mode: seen.__setitem__(mode, s))
        start = {k: v.detach().clone() for k, v in model.named_parameters()}
        train.train(args, model, opt, [setup.batch])
        params[mode] = {k: v.detach().clone() for k, v in model.named_parameters()}
        if mode == "fused":
            assert any(not torch.equal(start[k], params[mode][k]) for k in start)
    s = seen["fused"]
    with torch.no_grad():
        want = _reference_losses({k: v.double() for k, v in s["results"].items()}, s["selected_indexs"], s["vectors"].double(), s["confidences"].double(),
                                 s["labels"])
    for k, v in want.items():
        e = abs(s["losses"][k] - float(v)) / abs(float(v))
        print(k, s["losses"][k], float(v), e)
        assert e <= 1e-4, (k, e)
    # test_gpu_train.py's argument: an element whose gradient changes sign between the two paths moves by 2 lr
    worst = max(float((params["fused"][k] - params["reference"][k]).abs().max()) for k in params["fused"])
    print("max |fused - reference| after one step:", worst, "bound", 2 * LR * (1 + 1e-3))
    assert worst <= 2 * LR * (1 + 1e-3)


def test_pred_items_subset_leaves_the_confidence_head_alone(setup):
    from etch_amd import train
    args, model, opt = _fresh(setup, pred_items=["direction", "magnitude"])
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    losses = train.train(args, model, opt, [setup.batch])
    assert set(losses) == {"direction_loss", "magnitude_loss"}
    named = dict(model.named_parameters())
    conf = [k for k in named if k.startswith("confidence_encoder.")]
    assert conf and all(torch.equal(named[k], start[k]) for k in conf)
    assert all(named[k] not in opt.state or "exp_avg" not in opt.state[named[k]] for k in conf)
    moved = [k for k in named if not k.startswith("confidence_encoder.") and not torch.equal(named[k], start[k])]
    assert moved and all("exp_avg" in opt.state[named[k]] for k in moved)


def test_nan_in_the_target_vectors_skips_the_step(setup):
    from etch_amd import train
    args, model, opt = _fresh(setup)
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    batch = dict(setup.batch)
    batch["vectors"] = batch["vectors"].clone()
    batch["vectors"][1, 17, 2] = float("nan")
    train.train(args, model, opt, [batch])
    assert all(torch.equal(v, start[k]) for k, v in model.named_parameters())
    rep = opt.report()
    assert rep["skipped_steps"] == 1 and rep["tensors_zeroed"] == 0


def test_aug_rotates_points_and_vectors_about_y(setup):
    from etch_amd import train
    seen = []
    args, model, opt = _fresh(setup, aug=True, aug_generator=torch.Generator().manual_seed(7), on_step=seen.append)
    train.train(args, model, opt, [setup.batch])
    theta = train.aug_angles(torch.Generator().manual_seed(7), 2).numpy()
    for b in range(2):
        c, s = math.cos(theta[b]), math.sin(theta[b])
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        for k in ("hitpts", "vectors"):
            want = setup.batch[k][b].numpy().astype(np.float64) @ R.T
            got = seen[0][k][b].cpu().numpy()
            assert np.abs(got - want).max() <= 1e-6, (k, b, np.abs(got - want).max())
    assert abs(theta[0] - theta[1]) > 1e-3          # an angle per item
