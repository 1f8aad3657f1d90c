"""The encoder chain's statistics and anchor mean from the producing kernels: etch_linear_stats (the skip conv with the InstanceNorm statistics of its
output from the GEMM's epilogue, strided rows included), etch_instnorm_act_add_mean (the final pass that also writes the mean over the anchors) and the
finalisation of the statistics' partial sums spread over the chip (etch_instnorm_from_partials_n)."""
import types

import numpy as np
import pytest
import torch

from etch_amd.utils.weights import load_seeded

pytestmark = pytest.mark.gpu


def _ulps(a, ref):
    """|a - ref| in units of ref's fp32 spacing (ref = m 2^e with m in [0.5, 1): spacing 2^(e - 24))."""
    ref64 = ref.double()
    e = torch.frexp(ref64)[1]
    return float(((a.double() - ref64).abs() / torch.ldexp(torch.ones_like(ref64), e - 24)).max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _skip_inputs(b, rows_in, K, O, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b * rows_in, K, generator=g) * 1.3 + 0.4).cuda()       # |mean| comparable to sigma
    w = (torch.randn(O, K, generator=g) * 0.3).cuda()
    bias = (torch.randn(O, generator=g) * 0.3).cuda()
    return g, x, w, bias


def _two_blocks_plus_37():
    from etch_amd import _lib
    # two full workgroups of the partition plus a ragged third one (the partition of `rows` rows: etch_linear_stats_rows_per_part(rows))
    rows = 2 * 256 + 37
    per = _lib.lib().etch_linear_stats_rows_per_part(rows, 0)
    assert rows == 2 * per + 37 and _lib.lib().etch_linear_stats_parts(rows, 0) == 3, per
    return rows


@pytest.mark.parametrize("b,rows,K,O", [(3, 1980, 32, 32), (2, 777, 64, 64), (1, 60, 32, 32), (2, None, 32, 32)])
def test_skip_conv_with_statistics(b, rows, K, O):
    """Y bitwise etch_linear's; mean / rstd within 2 ulp of etch_instnorm_stats(Y) (both are fp64 sums of the same fp32 values rounded once: only the
    order differs); run-to-run identical; a sample's result does not depend on its batch neighbours."""
    from etch_amd import ops
    if rows is None:
        rows = _two_blocks_plus_37()
    _, x, w, bias = _skip_inputs(b, rows, K, O, rows + K)
    y, m, r = ops.linear_stats(x, w, bias, b, rows)
    y0 = ops.linear(x, w, bias=bias)
    assert torch.equal(_bits(y), _bits(y0))
    m0, r0 = ops.instnorm_stats(y.view(b, rows, O))
    um, ur = _ulps(m, m0), _ulps(r, r0)
    print(f"linear_stats ({b}, {rows}, {K}, {O}): mean {um:.2f} ulp, rstd {ur:.2f} ulp")
    assert um <= 2.0 and ur <= 2.0, (um, ur)
    y2, m2, r2 = ops.linear_stats(x, w, bias, b, rows)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(m2), _bits(m)) and torch.equal(_bits(r2), _bits(r))
    if b == 3:
        ya, ma, ra = ops.linear_stats(x[rows:2 * rows].contiguous(), w, bias, 1, rows)
        assert torch.equal(_bits(ya), _bits(y[rows:2 * rows])) and torch.equal(_bits(ma[0]), _bits(m[1])) and torch.equal(_bits(ra[0]), _bits(r[1]))


def test_skip_conv_with_statistics_strided_rows():
    """The row map of etch_linear (the stride-2 block: 20 of 40 points per sample, 60 rows each, 32 -> 64 channels; 1200 rows = 18 full tiles and a ragged
    one per sample): against the fp64 product, no worse than twice the present etch_linear(row_idx) result + 2e-6 of the scale -- and in fact its bits,
    which the pipeline's outputs need; statistics as above."""
    from etch_amd import ops
    b, p_in, p_out, grp, K, O = 2, 40, 20, 60, 32, 64
    g, x, w, bias = _skip_inputs(b, p_in * grp, K, O, 77)
    idx = torch.stack([torch.randperm(p_in, generator=g)[:p_out] for _ in range(b)]).to(torch.int32).cuda()
    rows = p_out * grp
    y, m, r = ops.linear_stats(x, w, bias, b, rows, row_idx=idx, grp=grp, p_in=p_in, p_out=p_out)
    y_old = ops.linear(x, w, bias=bias, row_idx=idx, grp=grp, p_in=p_in, p_out=p_out, rows=b * rows)
    xs = torch.gather(x.view(b, p_in, grp, K), 1, idx.long().view(b, p_out, 1, 1).expand(-1, -1, grp, K)).reshape(b * rows, K)
    ref = xs.double() @ w.double().t() + bias.double()
    sc = float(ref.abs().max())
    e_new, e_old = float((y.double() - ref).abs().max()), float((y_old.double() - ref).abs().max())
    print(f"strided skip conv: error {e_new / sc:.3e} of the scale (etch_linear with row_idx: {e_old / sc:.3e})")
    assert e_new <= 2.0 * e_old + 2e-6 * sc, (e_new / sc, e_old / sc)
    assert torch.equal(_bits(y), _bits(y_old))
    y2, m2, r2 = ops.linear_stats(x, w, bias, b, rows, row_idx=idx, grp=grp, p_in=p_in, p_out=p_out)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(m2), _bits(m)) and torch.equal(_bits(r2), _bits(r))
    m0, r0 = ops.instnorm_stats(y.view(b, rows, O))
    um, ur = _ulps(m, m0), _ulps(r, r0)
    print(f"strided skip conv: mean {um:.2f} ulp, rstd {ur:.2f} ulp")
    assert um <= 2.0 and ur <= 2.0, (um, ur)


def test_blocks_with_and_without_the_fused_statistics():
    """SeparableSO3ConvBlock 32 -> 32 (stride 1) and 32 -> 64 (stride 2) on 2 scans of 256 points, ETCH_SKIP_STATS_FUSED on / off: the same output to
    2e-6 of its scale, and no etch_instnorm_stats call with the switch on."""
    from etch_amd import _lib
    from etch_amd import vgtk_so3conv as sptk
    from etch_amd.models.so3conv import SeparableSO3ConvBlock
    from etch_amd.models.so3net import build_params
    bb = build_params(mlps=((32, 32), (64, 64)), strides=(2, 2))["backbone"]
    g = torch.Generator().manual_seed(11)
    xyz = (torch.randn(2, 256, 3, generator=g) * torch.tensor([0.14, 0.31, 0.085])).permute(0, 2, 1).contiguous().cuda()
    feats = (torch.randn(2, 256, 60, 32, generator=g) * 1.3 + 0.4).cuda()
    old = SeparableSO3ConvBlock.skip_stats_fused
    lib = _lib.lib()
    try:
        for params in (bb[0][1]["args"], bb[1][0]["args"]):
            assert (params["dim_in"], params["stride"]) in ((32, 1), (32, 2))
            blk = load_seeded(SeparableSO3ConvBlock(params), 4).cuda().eval()
            outs, calls = {}, {}
            for flag in (True, False):
                SeparableSO3ConvBlock.skip_stats_fused = flag
                seen = []

                def prof(name, args, fn, seen=seen):
                    seen.append(name)
                    return fn(*args)

                lib.profiler = prof
                try:
                    with torch.no_grad():
                        outs[flag] = blk(sptk.SphericalPointCloud(xyz, None, None, feats_cl=feats), None, None)[3].feats_cl
                    torch.cuda.synchronize()
                finally:
                    lib.profiler = None
                calls[flag] = seen
            assert "etch_linear_stats" in calls[True] and "etch_instnorm_stats" not in calls[True], calls[True]
            assert "etch_instnorm_stats" in calls[False] and "etch_linear_stats" not in calls[False], calls[False]
            sc = float(outs[False].abs().max())
            err = float((outs[True] - outs[False]).abs().max())
            print(f"block {params['dim_in']} -> {params['dim_out']} stride {params['stride']}: {err / sc:.3e} of the scale")
            assert err <= 2e-6 * sc, err / sc
    finally:
        SeparableSO3ConvBlock.skip_stats_fused = old


@pytest.mark.parametrize("b,p,C", [(2, 7, 64), (1, 1, 64), (3, 130, 32), (1, 9, 128)])
@pytest.mark.parametrize("second", [False, True])
def test_final_pass_with_the_anchor_mean(b, p, C, second):
    """etch_instnorm_act_add_mean: `out` bitwise etch_instnorm_act_add's, the means bitwise etch_token_mean(out)."""
    from etch_amd import ops
    g = torch.Generator().manual_seed(b * 1000 + p + C)
    x1 = (torch.randn(b, p, 60, C, generator=g) * 1.3 + 0.4).cuda()
    m1, r1 = ops.instnorm_stats(x1)
    x2 = m2 = r2 = None
    if second:
        x2 = (torch.randn(b, p, 60, C, generator=g) * 0.7 - 0.2).cuda()
        m2, r2 = ops.instnorm_stats(x2)
    out, mean = ops.instnorm_act_add_mean(x1, m1, r1, x2, m2, r2)
    out0 = ops.instnorm_act_add(x1, m1, r1, x2, m2, r2)
    assert torch.equal(_bits(out), _bits(out0))
    mean0 = ops.token_mean(out0.view(b * p, 60, C))
    assert mean.shape == mean0.shape and torch.equal(_bits(mean), _bits(mean0))


@pytest.mark.parametrize("nparts", [1, 7, 625])
@pytest.mark.parametrize("C", [32, 64])
def test_finalisation_across_the_chip_is_bitwise_the_one_workgroup_form(nparts, C):
    from etch_amd import ops
    b, count = 3, 120
    g = torch.Generator().manual_seed(nparts + C)
    s = torch.randn(b, nparts, 1, C, generator=g, dtype=torch.float64) * 40.0 + 30.0
    q = s * s / count + torch.rand(b, nparts, 1, C, generator=g, dtype=torch.float64) * 200.0      # sum of squares >= sum^2 / count
    part = torch.cat([s, q], 2).contiguous().cuda()
    total = nparts * count - 13 if nparts > 1 else count                   # a ragged last part: the true count is passed, not parts x count
    mw, rw = ops.instnorm_from_partials(part, total, wide=True)
    m1, r1 = ops.instnorm_from_partials(part, total, wide=False)
    assert torch.equal(_bits(mw), _bits(m1)) and torch.equal(_bits(rw), _bits(r1))
    ref_m = part[:, :, 0].sum(1) / total
    ref_r = 1.0 / torch.sqrt((part[:, :, 1].sum(1) / total - ref_m * ref_m).clamp_min(0.0) + 1e-5)
    assert _ulps(mw, ref_m.float()) <= 1.0 and _ulps(rw, ref_r.float()) <= 1.0


def _model(tmp_path):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.body_model import SyntheticSMPL
    args = types.SimpleNamespace(output_folder=str(tmp_path), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"),
                                 markerset=K.default_markerset(), scale_magnitude=10, body_model=SyntheticSMPL(7))
    return args, load_seeded(GT_network_equiv(option=args), 1).cuda().eval()


def _scan(seed, n):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array([0.14, 0.31, 0.085])).astype(np.float32)


def test_model_with_and_without_the_producers_statistics_and_anchor_mean(tmp_path):
    """GT_network_equiv (EPN_layer_num 2) on 2 x 1500 points with ETCH_SKIP_STATS_FUSED and ETCH_ANCHOR_MEAN_FUSED on / off: the tolerances of
    test_model_with_and_without_the_folded_skip_branch; the anchor mean alone changes no bit."""
    from etch_amd import _lib
    from etch_amd.models.so3conv import SeparableSO3ConvBlock as Blk
    args, model = _model(tmp_path)
    pts = torch.from_numpy(np.stack([_scan(5 + k, 1500) for k in range(2)])).cuda()
    items = ["confidence", "direction", "magnitude"]
    old = Blk.skip_stats_fused, Blk.anchor_mean_fused
    lib = _lib.lib()
    res, calls = {}, {}
    try:
        for flags in ((True, True), (False, False), (False, True)):
            Blk.skip_stats_fused, Blk.anchor_mean_fused = flags
            seen = []

            def prof(name, a, fn, seen=seen):
                seen.append(name)
                return fn(*a)

            lib.profiler = prof
            try:
                with torch.no_grad():
                    res[flags] = model(pts, items, "standard_vector")[0]
                torch.cuda.synchronize()
            finally:
                lib.profiler = None
            calls[flags] = seen
    finally:
        Blk.skip_stats_fused, Blk.anchor_mean_fused = old
    # (etch_instnorm_stats itself stays in the model at this size: the 375-point level is odd, so its intra conv takes the separate statistics pass)
    on, off = calls[(True, True)], calls[(False, False)]
    assert "etch_token_mean" not in on and "etch_instnorm_act_add_mean" in on and on.count("etch_linear_stats") == 3, sorted(set(on))
    assert "etch_token_mean" in off and "etch_linear_stats" not in off and off.count("etch_instnorm_stats") == on.count("etch_instnorm_stats") + 3, sorted(set(off))
    for k in ("magnitude", "confidences", "part_labels", "direction"):
        assert torch.equal(res[(False, True)][k], res[(False, False)][k]), k
    for k in ("magnitude", "confidences", "part_labels"):
        a, b_ = res[(True, True)][k], res[(False, False)][k]
        err = float((a - b_).abs().max())
        print(f"{k}: {err / float(b_.abs().max()):.3e} of the scale")
        assert err <= 2e-5 * float(b_.abs().max()) + 1e-6, k


def test_pipeline_and_graph_replay_on_the_new_path(tmp_path):
    """HotPathPipeline and GraphedHotPath (default fit schedule) on 2 x 1500 points with the new path: bit-identical to predict_smpl_batch; the capture
    succeeds, i.e. nothing on the path allocates outside the graph's pool or synchronises with the host."""
    from etch_amd.graph import GraphedHotPath
    from etch_amd.inference_demo import predict_smpl_batch
    from etch_amd.models.so3conv import SeparableSO3ConvBlock as Blk
    from etch_amd.pipeline import HotPathPipeline
    assert Blk.skip_stats_fused and Blk.anchor_mean_fused
    args, model = _model(tmp_path)
    B, N = 2, 1500
    mk = lambda k: torch.from_numpy(np.stack([_scan(400 + 10 * k + b, N) for b in range(B)])).cuda()
    same = lambda a, b: np.array_equal(np.asarray(a.cpu() if torch.is_tensor(a) else a), np.asarray(b.cpu() if torch.is_tensor(b) else b), equal_nan=True)
    ref = [predict_smpl_batch(args, model, mk(k), "neutral") for k in range(2)]
    got = list(HotPathPipeline(args, model, "neutral", max_in_flight=2).run(mk(k) for k in range(2)))
    for (m0, mk0, v0, i0), (m1, mk1, v1, i1) in zip(ref, got):
        assert same(mk0, mk1) and same(v0, v1)
        for a, b in zip(i0, i1):
            assert same(a, b)
        assert same(m0[0].vertices, m1[0].vertices)
    g = GraphedHotPath(args, model, B, N)
    meshes, markers, valid, info = g(mk(0))
    meshes0, markers0, valid0, info0 = predict_smpl_batch(args, model, mk(0))
    assert torch.equal(valid, valid0) and torch.equal(markers[valid], markers0[valid0])
    for a, b in zip(info, info0):
        assert np.array_equal(a, b, equal_nan=True)
    for m, m0 in zip(meshes, meshes0):
        assert np.array_equal(m.vertices, m0.vertices, equal_nan=True)
