"""The fit paths evaluate the direction head at the markers' points only (etch_marker_select -> etch_mhsa_interp_layer_list -> dirtail -> so3_mean_dir
-> etch_markers_from_selected).  Every comparison here is against the dense chain (direction of all points -> etch_inner_points -> etch_get_markers)
on bit patterns, NaNs equal to NaNs: the list form changes no bit of the markers, the fit or the meshes."""
import types

import numpy as np
import pytest
import torch

from etch_amd.utils.weights import load_seeded

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """Equal bit patterns, any NaN equal to any NaN (tensors or arrays, any dtype)."""
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a))
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    ints = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool(((a.contiguous().view(ints) == b.contiguous().view(ints)) | (torch.isnan(a) & torch.isnan(b))).all())


def scan(seed, n):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array([0.14, 0.31, 0.085])).astype(np.float32)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    from etch_amd import constants as K
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.body_model import SyntheticSMPL
    args = types.SimpleNamespace(output_folder=str(tmp_path_factory.mktemp("model")), EPN_input_radius=0.4, EPN_layer_num=2, device=torch.device("cuda"),
                                 markerset=K.default_markerset(), scale_magnitude=10, body_model=SyntheticSMPL(7))
    return args, load_seeded(GT_network_equiv(option=args), 1).cuda().eval()


def top3_rule(labels, conf, M):
    """The selection in plain torch: per (scan, label) the points carrying the label, ordered by confidence descending (any NaN greatest, -0 == +0),
    equal confidences by index ascending; the first three as global rows b K + i, -1 beyond.  -> sel (B,M,3), cnt (B,M)."""
    labels, conf = labels.cpu(), conf.cpu().reshape(labels.shape).double()
    B, K = labels.shape
    key = torch.where(torch.isnan(conf), torch.full_like(conf, float("inf")), conf + 0.0)       # (-0.0 + 0.0 = +0.0)
    sel = torch.full((B, M, 3), -1, dtype=torch.int32)
    cnt = torch.zeros((B, M), dtype=torch.int32)
    for b in range(B):
        for m in range(M):
            ids = torch.nonzero(labels[b] == m).view(-1)
            order = torch.sort(key[b, ids], descending=True, stable=True).indices[:3]
            cnt[b, m] = len(order)
            sel[b, m, :len(order)] = (b * K + ids[order]).int()
    return sel, cnt


def test_selection_and_markers_from_selected_points():
    """B = 3, K = 300, M = 7: labels with 0, 1, 2, exactly 3 and many points, equal confidences inside a label, a NaN confidence, -0.0 against +0.0,
    a label whose three confidences underflow under conf^20 (NaN marker).  sel / cnt against the top-3 rule restated in torch; the markers built
    from the selected points' directions alone against get_markers of the dense inner points."""
    from etch_amd import ops
    B, K, M = 3, 300, 7
    g = torch.Generator().manual_seed(11)
    labels = torch.full((B, K), 50, dtype=torch.int64)              # 50: no marker's label
    conf = torch.rand(B, K, generator=g) * 0.5 + 0.5
    # scan 0: label 0 none, 1 one point, 2 two, 3 exactly three, 4 many, 5 three confidences of 1e-3, 6 many with equal confidences
    labels[0, 7] = 1
    labels[0, [20, 3]] = 2
    labels[0, [100, 41, 299]] = 3
    labels[0, 120:200] = 4
    labels[0, [210, 64, 250]] = 5
    conf[0, [210, 64, 250]] = 1e-3
    labels[0, 260:290] = 6
    conf[0, 260:290] = 0.75
    # scan 1: random labels; a NaN confidence in label 1; label 2 = {-0.0, +0.0, negative ones}: the two zeros tie, the lower index first
    labels[1] = torch.randint(0, M, (K,), generator=g)
    conf[1, int(torch.nonzero(labels[1] == 1)[2])] = float("nan")
    l2 = torch.nonzero(labels[1] == 2).view(-1)
    conf[1, l2] = -conf[1, l2]
    conf[1, l2[5]], conf[1, l2[1]] = 0.0, -0.0
    # scan 2: every point carries label 4 with one confidence
    labels[2] = 4
    conf[2] = 0.7
    pts = torch.from_numpy(np.stack([scan(20 + b, K) for b in range(B)]))
    direction = torch.nn.functional.normalize(torch.randn(B, K, 3, generator=g), dim=-1)
    magnitude = torch.rand(B, K, 1, generator=g) * 0.3
    labels, conf, pts, direction, magnitude = labels.cuda(), conf.view(B, K, 1).cuda(), pts.cuda(), direction.cuda(), magnitude.cuda()

    sel, cnt = ops.marker_select(labels, conf, M)
    want_sel, want_cnt = top3_rule(labels, conf, M)
    assert torch.equal(cnt.cpu(), want_cnt) and torch.equal(sel.cpu(), want_sel)
    assert want_cnt[0].tolist() == [0, 1, 2, 3, 3, 3, 3] and want_sel[0, 6].tolist() == [260, 261, 262] and want_sel[2, 4].tolist() == [600, 601, 602]
    assert want_sel[1, 2, :2].tolist() == [K + int(l2[1]), K + int(l2[5])]

    ref = ops.get_markers(ops.inner_points(pts, direction, magnitude, 10.0), labels, conf, M)
    compact = direction.view(-1, 3)[sel.view(-1).clamp(min=0).long()].contiguous()
    compact[sel.view(-1) < 0] = float("nan")                        # an empty slot's direction is never read
    got = ops.markers_from_selected(sel, cnt, pts, conf, magnitude, 10.0, compact)
    for a, b in zip(got, ref):
        assert same_bits(a, b)
    assert bool(torch.isnan(ref[0][0, 5]).all()) and bool(ref[2][0, 5])          # the underflowing label: valid, NaN
    assert bool(torch.isnan(ref[0][1, 1]).all())                                  # the NaN confidence is selected first
    assert ref[2].sum(1).tolist() == [6, 7, 1]


@pytest.mark.parametrize("B,P", [(2, 6), (1, 1), (1, 13)])
def test_list_layer_equals_the_dense_layer_at_the_listed_points(B, P):
    """etch_mhsa_interp_layer_list on N = 70 points per scan, S = 20 coarse points: every non-empty slot's 60 x 64 tile equals that point's tile of
    etch_mhsa_interp_layer, and after mhsa_layer_dirtail and so3_mean_dir its direction equals the dense one.  The list carries a duplicate point,
    empty slots and three consecutive slots of one label; 1 slot and 13 slots: counts that are no multiple of the 8 XCD shares."""
    from etch_amd import constants as K
    from etch_amd import ops
    N, S = 70, 20
    g = torch.Generator().manual_seed(7)
    F = torch.randn(2, S, 60, 64, generator=g)[:B].contiguous().cuda()
    idx = torch.randint(0, S, (2, N, 3), generator=g, dtype=torch.int32)[:B].contiguous().cuda()
    w = torch.rand(2, N, 3, generator=g)[:B] + 0.05
    w = (w / w.sum(-1, keepdim=True)).contiguous().cuda()
    W = [(torch.randn(64, 64, generator=g) * 0.125).cuda() for _ in range(7)]
    bc = (torch.randn(64, generator=g) * 0.1).cuda()
    Wf = (torch.randn(128, 64, generator=g) * 0.125).cuda()
    Wfq = ops.dirtail_weight_split(Wf)
    tab = ops.dirtail_constants((torch.randn(128, generator=g) * 0.1).cuda(), (torch.randn(128, generator=g) * 0.1).cuda(),
                                torch.randn(1, generator=g).cuda(), Wfq.wsc)
    anchors = torch.from_numpy(K.get_anchors().astype(np.float32)).cuda().contiguous()
    if (B, P) == (2, 6):
        sel = torch.tensor([[5, 5, -1, 69, 0, -1], [N + 3, N + 17, N + 44, -1, -1, N + 69]], dtype=torch.int32)
    elif P == 1:
        sel = torch.tensor([[33]], dtype=torch.int32)
    else:
        sel = torch.randint(0, N, (1, P), generator=g, dtype=torch.int32)
        sel[0, [2, 12]] = -1
    sel = sel.cuda()

    def tail(x):
        anc = ops.mhsa_layer_dirtail(x, W[4], W[5], W[6], Wfq, tab)
        return ops.so3_mean_dir(anc, anchors)[0]

    dense = ops.mhsa_interp_layer(F, idx, w, W[0], W[1], W[2], W[3], bc)
    dense_dir = tail(dense)
    got = ops.mhsa_interp_layer_list(F, sel, idx, w, W[0], W[1], W[2], W[3], bc)
    got_dir = tail(got)
    assert got.shape == (B * P * 60, 64) and got_dir.shape == (B * P, 3)
    rows = sel.view(-1).cpu().tolist()
    assert any(r >= 0 for r in rows)
    for k, r in enumerate(rows):
        if r >= 0:
            assert same_bits(got[60 * k:60 * k + 60], dense[60 * r:60 * r + 60]), (k, r)
            assert same_bits(got_dir[k], dense_dir[r]), (k, r)
    assert bool(torch.isfinite(got).all())                          # empty slots computed on real data too


def test_composition_with_spread_out_labels(seeded):
    """The seeded model's real encoder output and magnitude on 2 x 1024 points with test-made labels (uniform over the 86 markers) and confidences
    (uniform in (0.5, 1)): nearly all 516 slots are filled (the network's own labels fill ~2 per scan).  Markers and valid of the list form
    (fit_SMPL.markers_from_stage1) against the dense chain: full direction -> inner_points -> get_markers."""
    from etch_amd import ops
    from etch_amd.models.fit_SMPL import markers_from_stage1
    args, model = seeded
    B, N, M = 2, 1024, len(args.markerset)
    pts = torch.from_numpy(np.stack([scan(600 + b, N) for b in range(B)])).cuda()
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, M, (B, N), generator=g).cuda()
    conf = (torch.rand(B, N, 1, generator=g) * 0.5 + 0.5).cuda()
    with torch.no_grad():
        full, _ = model(pts, ["confidence", "direction", "magnitude"], "standard_vector")
        results, ctx = model.forward_for_fit(pts)
        assert ctx is not None and "direction" not in results and same_bits(results["magnitude"], full["magnitude"])
        made = dict(results, confidences=conf, part_labels=torch.nn.functional.one_hot(labels, M).float().contiguous())
        got = markers_from_stage1(args, model, ctx, pts, made)
        _, cnt = ops.marker_select(labels, conf, M)
        ref = ops.get_markers(ops.inner_points(pts, full["direction"], full["magnitude"], float(args.scale_magnitude)), labels, conf, M)
    assert int(cnt.sum()) > 500
    for a, b in zip(got, ref):
        assert same_bits(a, b)
    assert bool(torch.isfinite(ref[0]).all())


def test_fit_paths_with_the_direction_head_at_the_marker_points(seeded, monkeypatch):
    """predict_smpl_batch on 2 x 1500 points with ETCH_SPARSE_DIRECTION on and off: markers, valid, x, verts and err_trace identical; HotPathPipeline
    and GraphedHotPath equal it; a call that asks for the inner points still gets all of them (and the same fit)."""
    from etch_amd import ops
    from etch_amd.graph import GraphedHotPath
    from etch_amd.inference_demo import predict_smpl_batch
    from etch_amd.pipeline import HotPathPipeline
    args, model = seeded
    B, N = 2, 1500
    mk = lambda k: torch.from_numpy(np.stack([scan(400 + 10 * k + b, N) for b in range(B)])).cuda()
    calls = []
    real = ops.mhsa_interp_layer_list
    monkeypatch.setattr(ops, "mhsa_interp_layer_list", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    monkeypatch.setenv("ETCH_SPARSE_DIRECTION", "0")
    dense = [predict_smpl_batch(args, model, mk(k), "neutral", return_trace=True) for k in range(2)]
    assert not calls
    monkeypatch.setenv("ETCH_SPARSE_DIRECTION", "1")
    ref = [predict_smpl_batch(args, model, mk(k), "neutral", return_trace=True) for k in range(2)]
    assert len(calls) == 2
    for (m0, mk0, v0, i0, aux0), (m1, mk1, v1, i1, aux1) in zip(dense, ref):
        assert same_bits(mk0, mk1) and same_bits(v0, v1)
        for key in ("x", "verts", "err_trace", "markers", "valid"):
            assert same_bits(aux0[key], aux1[key]), key
        for a, b in zip(i0, i1):
            assert same_bits(a, b)
        assert all(same_bits(a.vertices, b.vertices) for a, b in zip(m0, m1))

    got = list(HotPathPipeline(args, model, "neutral", max_in_flight=2).run(mk(k) for k in range(2)))
    assert len(calls) == 4
    for (m0, mk0, v0, i0, _), (m1, mk1, v1, i1) in zip(ref, got):
        assert same_bits(mk0, mk1) and same_bits(v0, v1)
        for a, b in zip(i0, i1):
            assert same_bits(a, b)
        assert same_bits(m0[0].vertices, m1[0].vertices)
    meshes, markers, valid, info = GraphedHotPath(args, model, B, N)(mk(0))
    assert len(calls) > 4
    assert same_bits(valid, ref[0][2]) and same_bits(markers[valid], ref[0][1][ref[0][2]])
    for a, b in zip(info, ref[0][3]):
        assert same_bits(a, b)
    for m, m0 in zip(meshes, ref[0][0]):
        assert same_bits(m.vertices, m0.vertices)

    n = len(calls)
    out = {}
    m2, mk2, v2, i2 = predict_smpl_batch(args, model, mk(0), "neutral", inner_out=out)
    assert len(calls) == n                                          # all inner points wanted: the dense head
    with torch.no_grad():
        full, _ = model(mk(0), ["confidence", "direction", "magnitude"], "standard_vector")
    assert out["inner"].shape == (B, N, 3)
    assert same_bits(out["inner"], ops.inner_points(mk(0), full["direction"], full["magnitude"], float(args.scale_magnitude)))
    assert same_bits(mk2, ref[0][1]) and same_bits(v2, ref[0][2]) and same_bits(m2[0].vertices, ref[0][0][0].vertices)
