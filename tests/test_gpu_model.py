"""GPU parity of the Point-Transformer modules and of the whole GT_network_equiv forward
against golden vectors emitted by the reference's own Python."""
import json
import types

import numpy as np
import pytest
import torch

from etch_amd.utils.weights import load_seeded, seeded_tensor

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def test_point_transformer_modules_vs_reference_golden(golden):
    from etch_amd.models import pointtransformer_seg as P
    g = golden("module_pt.npz")
    seeds = json.loads(str(g["seeds"]))
    d = lambda k: torch.from_numpy(g[k]).cuda()
    p, x, o = d("p"), d("x"), d("o")
    c = 32
    mk = lambda name, m: load_seeded(m, seeds[name]).cuda().eval()
    layer = mk("layer", P.PointTransformerLayer(c, c, 8, 8))
    assert rel_err(layer([p, x, o]).cpu().numpy(), g["layer_out"]) < RTOL
    block = mk("block", P.PointTransformerBlock(c, c, 8, 16))
    assert rel_err(block([p, x, o])[1].cpu().numpy(), g["block_out"]) < RTOL
    down = mk("down", P.TransitionDown(c, 48, 4, 16))
    p2, x2, o2 = down([p, x, o])
    assert np.array_equal(p2.cpu().numpy(), g["down_p"]) and np.array_equal(o2.cpu().numpy(), g["down_o"])
    assert rel_err(x2.cpu().numpy(), g["down_x"]) < RTOL
    down1 = mk("down1", P.TransitionDown(c, 48, 1, 8))
    assert rel_err(down1([p, x, o])[1].cpu().numpy(), g["down1_x"]) < RTOL
    up = mk("up", P.TransitionUp(48, c))
    assert rel_err(up([p, x, o], [d("down_p"), d("down_x"), d("down_o")]).cpu().numpy(), g["up_out"]) < RTOL
    uph = mk("uph", P.TransitionUp(c, None))
    assert rel_err(uph([p, x, o]).cpu().numpy(), g["uph_out"]) < RTOL


@pytest.mark.parametrize("c,co,n", [(128, 128, 4001), (64, 128, 1000), (256, 512, 403)])
def test_transition_down_split_linear_matches_grouped_rows(c, co, n):
    """TransitionDown with the Linear split into per-source-point GEMM + gather-max kernel vs the literal grouped-rows form
    (queryandgroup -> Linear -> BN -> ReLU -> MaxPool, pointtransformer_seg.py:55-63), which the reference golden pins at c = 32."""
    from etch_amd.models import pointtransformer_seg as P
    from etch_amd.models import pointops
    down = load_seeded(P.TransitionDown(c, co, 4, 16), 5).cuda().eval()
    g = torch.Generator().manual_seed(c + n)
    pnt = (torch.randn(n, 3, generator=g) * 0.3).cuda()
    x = torch.randn(n, c, generator=g).cuda()
    o = pointops.offsets_tensor([n // 3, n], "cuda")
    outs = []
    for split in (True, False):
        down.split_linear = split
        with torch.no_grad():
            p2, x2, o2 = down([pnt, x, o])
        outs.append((p2.cpu().numpy(), x2.cpu().numpy(), o2.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][2], outs[1][2])
    assert rel_err(outs[0][1], outs[1][1]) < 5e-6


def build_model(tmp_path, seed):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    opt = types.SimpleNamespace(output_folder=str(tmp_path), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"),
                                markerset=K.default_markerset())
    return load_seeded(GT_network_equiv(option=opt), seed).cuda().eval()


def test_state_dict_matches_reference_manifest(tmp_path, golden):
    import os
    man = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "state_dict_manifest.json")))
    m = build_model(tmp_path, 0)
    sd = m.state_dict()
    assert [k for k, _, _ in man] == list(sd.keys())                       # same names, same order
    for k, shape, dt in man:
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == "torch." + dt, k
    ref_table = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "epn_model_setting.json")))
    assert json.load(open(os.path.join(str(tmp_path), "EPN_model_setting_json"))) == ref_table   # constructor side effect (:30)


def test_whole_model_vs_reference_golden(tmp_path, golden):
    g = golden("model_n1024.npz")
    m = build_model(tmp_path, int(g["seed"]))
    pts = torch.from_numpy(g["points"]).cuda()
    with torch.no_grad():
        res, sel = m(pts, ["confidence", "direction", "magnitude"], "standard_vector")
    assert sel.shape == (2, 1024, 3) and sel.dtype == torch.int64 and np.array_equal(sel[:, :4].cpu().numpy(), g["selected_indexs"])
    for k, shape in (("part_labels", (2, 1024, 86)), ("confidences", (2, 1024, 1)), ("magnitude", (2, 1024, 1)), ("direction", (2, 1024, 3))):
        assert tuple(res[k].shape) == shape and res[k].dtype == torch.float32
    for k in ("part_labels", "confidences", "magnitude"):
        assert rel_err(res[k].cpu().numpy(), g[k]) < RTOL, k
    assert (res["part_labels"].argmax(-1).cpu().numpy() == g["part_labels"].argmax(-1)).mean() > 0.999
    assert rel_err(m.last_anc_w.cpu().numpy(), g["anc_w"]) < RTOL
    # direction = polar projection of Ce = sum_a w_a R_a.  With random weights Ce is nearly singular, so the
    # admissible deviation is the conditioning of the projection times the (already asserted) deviation of anc_w:
    #   |dR| <~ 2 |dCe|_F / gap,  dCe = sum_a (w_gpu - w_ref)_a R_a,  gap = min_{i<j} (s_i + s_j), s = (sv0, sv1, det * sv2)
    from oracle import stage1 as S
    c = golden("constants.npz")
    aw = torch.from_numpy(g["anc_w"]).view(-1, 60)
    Rref, Ce, sv = S.so3_mean(torch.from_numpy(c["anchors"]), aw)
    det = torch.det(Ce).sign()
    s = torch.stack([sv[:, 0], sv[:, 1], det * sv[:, 2]], 1).double()
    gap = torch.stack([s[:, 0] + s[:, 1], s[:, 0] + s[:, 2], s[:, 1] + s[:, 2]], 1).min(1).values.clamp_min(1e-12).numpy()
    dw = m.last_anc_w.cpu().numpy().reshape(-1, 60).astype(np.float64) - g["anc_w"].reshape(-1, 60)
    dCe = np.linalg.norm(np.einsum("ta,aij->tij", dw, c["anchors"].astype(np.float64)).reshape(-1, 9), axis=1)
    bound = 4.0 * dCe / gap + 1e-5
    err = np.abs(res["direction"].cpu().numpy() - g["direction"]).reshape(-1, 3).max(1)
    tight = bound < 0.05
    assert tight.mean() > 0.3
    assert (err[tight] <= bound[tight]).all()
    # and the projection kernel itself, fed with the reference's own anc_w, reproduces the reference direction
    from etch_amd import ops
    d2, _, _ = ops.so3_mean_dir(aw.cuda(), torch.from_numpy(c["anchors"]).cuda())
    err2 = np.abs(d2.cpu().numpy() - g["direction"].reshape(-1, 3)).max(1)
    assert (err2 <= 1e-5 / np.minimum(gap, 1.0) + 1e-5).all()   # fp32 rounding of the reference own Ce / SVD over the conditioning


def test_pt_layer_fused_and_split_variants_agree(golden):
    """etch_pt_attention (one VALU kernel) and the matrix-core split (prep + etch_linear x2 + aggregate) are the same function."""
    from etch_amd.models import pointtransformer_seg as P
    g = golden("module_pt.npz")
    seeds = json.loads(str(g["seeds"]))
    d = lambda k: torch.from_numpy(g[k]).cuda()
    layer = load_seeded(P.PointTransformerLayer(32, 32, 8, 8), seeds["layer"]).cuda().eval()
    layer.attention_impl = "valu"
    a = layer([d("p"), d("x"), d("o")]).cpu().numpy()
    layer.attention_impl = "split"
    b = layer([d("p"), d("x"), d("o")]).cpu().numpy()
    assert rel_err(a, g["layer_out"]) < RTOL and rel_err(b, g["layer_out"]) < RTOL


@pytest.mark.parametrize("c,ns,n", [(64, 8, 1003), (128, 8, 517), (64, 16, 300), (128, 16, 1001), (256, 16, 333), (512, 16, 97)])
def test_pt_attention_mfma_kernel_matches_split_and_valu(c, ns, n):
    """etch_pt_attention_mfma (the whole attention core on the matrix cores in one kernel) against the two older variants, which the
    reference golden pins at c = 32: every instantiated (c, nsample), point counts that leave partial waves / workgroups, two
    segments, with and without the fused output BatchNorm + ReLU."""
    from etch_amd.models import pointtransformer_seg as P
    from etch_amd.models import pointops
    from etch_amd import ops
    layer = load_seeded(P.PointTransformerLayer(c, c, 8, ns), 11).cuda().eval()
    g = torch.Generator().manual_seed(c + ns + n)
    pnt = (torch.randn(n, 3, generator=g) * 0.3).cuda()
    x = torch.randn(n, c, generator=g).cuda()
    o = pointops.offsets_tensor([n // 2, n], "cuda")
    bn = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda() * 0.1
    assert (c, ns) in ops.PT_MFMA_SHAPES
    for out_bn in (None, bn):
        outs = {}
        for impl in ("mfma", "split", "valu"):
            layer.attention_impl = impl
            with torch.no_grad():
                outs[impl] = layer([pnt, x, o], out_bn=out_bn).cpu().numpy()
        assert outs["mfma"].shape == (n, c) and np.isfinite(outs["mfma"]).all()
        assert rel_err(outs["mfma"], outs["split"]) < 5e-6 and rel_err(outs["mfma"], outs["valu"]) < 5e-6


def test_fused_block_vs_reference_golden_falls_back_for_unbuilt_widths(golden):
    """c = 32 (the reference golden's block) is not a width of the nets: run_blocks must take the blocks' own forward and still match."""
    from etch_amd.models import pointtransformer_seg as P
    g = golden("module_pt.npz")
    seeds = json.loads(str(g["seeds"]))
    d = lambda k: torch.from_numpy(g[k]).cuda()
    block = load_seeded(P.PointTransformerBlock(32, 32, 8, 16), seeds["block"]).cuda().eval()
    with torch.no_grad():
        out = P.run_blocks([block], [d("p"), d("x"), d("o")])[1]
    assert rel_err(out.cpu().numpy(), g["block_out"]) < RTOL


def test_whole_model_on_the_fp32_mfma_kernels_vs_reference_golden(tmp_path, golden, monkeypatch):
    """The switches of the split-operand kernels (ETCH_INTER_SPLIT / ETCH_INTRA_SPLIT / ETCH_LRD_SPLIT = 0, here through the module flags they set):
    the model built and run on the fp32-MFMA kernels meets the same fixture of the reference's Python, and the two arithmetic paths agree with
    each other far inside the parity tolerance (they are the same fp32 sums in different orders)."""
    from etch_amd import ops
    g = golden("model_n1024.npz")
    pts = torch.from_numpy(g["points"]).cuda()
    items = ["confidence", "direction", "magnitude"]
    with torch.no_grad():
        split, _ = build_model(tmp_path, int(g["seed"]))(pts, items, "standard_vector")
    for flag in ("INTER_SPLIT", "INTRA_SPLIT", "LRD_SPLIT"):
        monkeypatch.setattr(ops, flag, False)
    m = build_model(tmp_path, int(g["seed"]))             # a fresh model: the weight operands are cached per parameter version
    with torch.no_grad():
        f32, _ = m(pts, items, "standard_vector")
    for k in ("part_labels", "confidences", "magnitude"):
        assert rel_err(f32[k].cpu().numpy(), g[k]) < RTOL, k
        assert rel_err(f32[k].cpu().numpy(), split[k].cpu().numpy()) < 2e-5, k
    assert rel_err(m.last_anc_w.cpu().numpy(), g["anc_w"]) < RTOL
