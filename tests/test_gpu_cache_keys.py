"""Cache keys are honest: a write through a raw pointer bumps the tensor's `_version` (_lib.wrote), the FPS results computed ahead live in the
forward's pointops.knn_scope and nowhere else, and the shared per-shape constants (etch_amd/_shared.py) are rebuilt once a caller has written into them."""
import numpy as np
import pytest
import torch

from etch_amd.utils.weights import load_seeded

pytestmark = pytest.mark.gpu
ITEMS = ["confidence", "direction", "magnitude"]


# ---------------------------------------------------------------------------------------------- 1. writes through raw pointers bump the version
def test_guarded_adam_step_bumps_the_versions_it_wrote():
    from etch_amd.optim import GuardedAdam
    from etch_amd.vgtk_so3conv import _Derived
    torch.manual_seed(0)
    lin, idle = torch.nn.Linear(4, 4).cuda(), torch.nn.Linear(4, 4).cuda()          # `idle` never receives a gradient: it may or may not bump
    opt = GuardedAdam(list(lin.parameters()) + list(idle.parameters()), lr=1e-2)
    d, built = _Derived(), []
    builder = lambda: built.append(1) or lin.weight.detach().clone()
    d.get((lin.weight,), builder), d.get((lin.weight,), builder)
    assert len(built) == 1
    before = {p: (p._version, p.detach().clone()) for p in lin.parameters()}
    lin(torch.randn(3, 4, device="cuda")).sum().backward()
    opt.step()
    for p, (v, old) in before.items():
        assert p._version > v and not torch.equal(p, old)
    for st in (opt.state[p] for p in lin.parameters()):
        assert st["exp_avg"]._version > 0 and st["exp_avg_sq"]._version > 0 and st["step"]._version > 0
    assert torch.equal(d.get((lin.weight,), builder), lin.weight) and len(built) == 2          # the derived constant follows the step
    assert all(p.grad is None for p in idle.parameters())


def test_train_mode_batch_norm_bumps_the_running_statistics():
    """... and still computes torch.nn.functional.batch_norm's (the comparison of test_gpu_r06's many-calls test, one call)."""
    from etch_amd import autograd_pt as P
    m, m2 = torch.nn.BatchNorm1d(8).cuda().train(), torch.nn.BatchNorm1d(8).cuda().train()
    x = torch.from_numpy((np.random.default_rng(5).standard_normal((64, 8)) * 2 + 1).astype(np.float32)).cuda()
    before = [t._version for t in (m.running_mean, m.running_var, m.num_batches_tracked)]
    y, y2 = P.batch_norm(x, m, relu=True), torch.relu(m2(x))
    for t, v in zip((m.running_mean, m.running_var, m.num_batches_tracked), before):
        assert t._version > v
    assert float((y - y2).detach().abs().max()) <= 2e-6 * float(y2.detach().abs().max())
    for got, want in ((m.running_mean, m2.running_mean), (m.running_var, m2.running_var)):
        assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())
    assert int(m.num_batches_tracked) == int(m2.num_batches_tracked) == 1


@pytest.mark.parametrize("step", [True, False])
def test_eval_forward_after_training_uses_the_trained_weights(tmp_path, monkeypatch, step):
    """eval() forward, one train() forward (+ backward + GuardedAdam.step() if `step`; without it only BatchNorm's running statistics move), eval()
    forward again: bitwise the eval() forward of a model built afresh that loads the trained state dict.  All three heads."""
    import types
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.optim import GuardedAdam
    from tests.test_gpu_train import _losses, _setup
    model, pts, vec, conf, labels = _setup(tmp_path, 2, 512)
    c = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()
    x = torch.from_numpy(pts).cuda()
    opt = GuardedAdam(model.parameters(), lr=1e-3)
    model.eval()
    with torch.no_grad():
        first = {k: v.clone() for k, v in model(x, ITEMS, "standard_vector")[0].items()}
    model.train()
    monkeypatch.setattr(GT_network_equiv, "_warned_switch", True)           # (its once-per-process warning is another test's subject; restored afterwards)
    res, _ = model(x, ITEMS, "standard_vector")
    if step:
        _losses(res, c(vec), c(conf), torch.from_numpy(labels).cuda(), None, ("direction", "magnitude", "confidence"))[0].backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        again = model(x, ITEMS, "standard_vector")[0]
    args = types.SimpleNamespace(output_folder=str(tmp_path), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"), markerset=K.default_markerset())
    fresh = GT_network_equiv(option=args).cuda()
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh(x, ITEMS, "standard_vector")[0]
    assert set(want) == {"part_labels", "confidences", "magnitude", "direction"}
    for k in want:
        assert torch.equal(again[k], want[k]), k
    assert any(not torch.equal(first[k], want[k]) for k in want)          # (the training really changed what the model computes)


def test_in_place_fits_bump_the_tensor_they_update():
    from etch_amd import ops
    from etch_amd.models.chamfer_refine import _bm_tables
    from etch_amd.models.register import _edges_of
    from etch_amd.utils.body_model import SyntheticSMPL
    from tests.test_gpu_chamfer import _random_params, _scan_of
    bm = SyntheticSMPL(7, V=1200)
    db = _bm_tables(bm, torch.device("cuda"))
    truth = _random_params(bm, 2, 21)
    scan = torch.from_numpy(_scan_of(bm, truth, 300, 22)).cuda()
    params = torch.from_numpy(truth).cuda().contiguous()
    params[:, :72] += 0.05
    v0, p0 = params._version, params.clone()
    ops.smpl_chamfer_refine(db.lbs_consts, scan, params, db.V, iters=1, nj=db.nj, nb=db.nb, n_extra=db.n_extra)
    assert params._version > v0 and not torch.equal(params, p0)
    base, R, _ = ops.smpl_skin_frames(db.lbs_consts, params, nj=db.nj, nb=db.nb)
    D = torch.zeros((2, db.V, 3), dtype=torch.float32, device="cuda")
    ptr, idx, n_edges = _edges_of(bm, torch.device("cuda"))
    v0 = D._version
    ops.smpld_register(base, R, D, scan, ptr, idx, n_edges, [1.0])
    assert D._version > v0 and bool((D != 0).any())


# ---------------------------------------------------------------------------------------------- 2. the FPS hand-over dies with the forward
def test_a_forward_that_raises_leaves_no_sampling_result_behind(tmp_path, monkeypatch):
    from etch_amd import ops
    from etch_amd.models import pointops
    from tests.test_gpu_pipeline import make, scan
    args, model = make(tmp_path)
    assert model.fps_pair
    pts = torch.from_numpy(np.stack([scan(500 + b, 2048) for b in range(2)])).cuda()
    other = torch.from_numpy(np.stack([scan(700 + b, 2048) for b in range(2)])).cuda()
    encode, raised = model.encode, []

    def raise_once(f):
        if raised:
            return encode(f)
        raised.append(True)
        raise RuntimeError("encoder failed")
    monkeypatch.setattr(model, "encode", raise_once)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="encoder failed"):
            model(pts, ITEMS, "standard_vector")           # the paired FPS has run and seeded its results by then
        torch.cuda.synchronize()
        assert pointops._knn_cache is None and not [n for n in vars(ops) if "FPS_READY" in n]
        pts.copy_(other)
        got = model(pts, ["direction"], "standard_vector")[0]["direction"]
        want = make(tmp_path)[1](pts, ["direction"], "standard_vector")[0]["direction"]
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- 3. shared constants survive a caller's edit
def test_edited_occupancy_ones_take_the_ordinary_kernels():
    from etch_amd import ops
    from etch_amd._shared import constant_value
    from etch_amd.models.so3conv import SeparableSO3ConvBlock, preprocess_input
    from etch_amd.vgtk_so3conv import SphericalPointCloud
    from tests.test_gpu_r06 import _inter_setup
    g, xyz, new_xyz, ball, conv, _ = _inter_setup(1, 32, 64, 2, 400, 200, seed=9)
    rk, W, Wp, bias = conv._derived()
    pts = xyz.permute(0, 2, 1).contiguous()
    cloud = preprocess_input(pts, 60, add_center=False)
    t = cloud.feats_cl
    assert constant_value(t) == 1.0
    t.mul_(2)
    assert constant_value(t) is None
    twos = torch.full_like(t, 2.0)
    a, (ma, ra) = ops.inter_so3conv(xyz, new_xyz, ball, t, rk, W, Wp, bias, conv.sigma, want_stats=True)
    c, (mc, rc) = ops.inter_so3conv(xyz, new_xyz, ball, twos, rk, W, Wp, bias, conv.sigma, want_stats=True)
    assert torch.equal(a, c) and torch.equal(ma, mc) and torch.equal(ra, rc)
    block = load_seeded(SeparableSO3ConvBlock(dict(dim_in=1, dim_out=32, kernel_size=1, stride=1, radius=0.25, sigma=0.03, n_neighbor=64, multiplier=2,
                                                   lazy_sample=True, dropout_rate=0.0, activation="leaky_relu", pooling=None, kanchor=60)), 3).cuda().eval()
    with torch.no_grad():
        ya = block(cloud, None, None)[3].feats_cl
        yb = block(SphericalPointCloud(cloud.xyz, None, None, feats_cl=twos), None, None)[3].feats_cl
    assert torch.equal(ya, yb)
    fresh = preprocess_input(pts, 60, add_center=False).feats_cl
    assert fresh is not t and bool((fresh == 1).all()) and constant_value(fresh) == 1.0


def test_edited_identity_samples_and_offsets_are_rebuilt():
    from etch_amd.models import pointops
    from etch_amd.vgtk_so3conv import furthest_sample_index
    pc = torch.randn(2, 3, 64, device="cuda")
    idx = furthest_sample_index(pc, 64, True)
    assert furthest_sample_index(pc, 64, True) is idx
    idx.zero_()
    again = furthest_sample_index(pc, 64, True)
    assert torch.equal(again, torch.arange(64, dtype=torch.int32, device="cuda").expand(2, 64))
    o = pointops.offsets_tensor([64, 128], pc.device)
    assert pointops.offsets_tensor([64, 128], pc.device) is o
    o.add_(1)
    o2 = pointops.offsets_tensor([64, 128], pc.device)
    assert o2.tolist() == [64, 128] and pointops.host_offsets(o2) == [64, 128] and pointops.host_offsets(o) == [65, 129]
