"""The inference Point-Transformer kernels, the glue kernels and etch_linear's remaining branches against fp64 references, at the
nets' own widths (tests/_pt_fp64.py: per-channel relL2 / relmax, e_gpu <= 2 e_32 + 1e-6 with e_32 the reference's own fp32 run).
Before floats are compared every test asserts that the GPU's kNN / FPS indices are the C oracle's, so a float mismatch cannot be
an index mismatch in disguise.  Every case prints one `PIN` line; profiles/pt_fp64_pins.txt is the record of a run."""
import numpy as np
import pytest
import torch

from etch_amd.utils.weights import load_seeded, seeded_tensor
from oracle import ops as O
from tests import _pt_fp64 as Y

pytestmark = pytest.mark.gpu
SEED = 11


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def offsets(o):
    from etch_amd.models import pointops
    return pointops.offsets_tensor([int(v) for v in o], "cuda")


def window(a, ld, col0=0, fill=0.0):
    """`a` (rows, c) as a column window [col0, col0 + c) of a wider device matrix (rows, ld): same values, row stride ld."""
    a = np.ascontiguousarray(a)
    wide = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device="cuda")
    wide[:, col0:col0 + a.shape[1]] = dev(a)
    return wide[:, col0:col0 + a.shape[1]]


def assert_knn_is_the_oracles(ns, p, q, o, qo, want_dist=False):
    """GPU kNN indices == oracle.O.knnquery's (p, q numpy fp32; o, qo numpy int32)."""
    from etch_amd.models import pointops
    pd = dev(p)
    qd = pd if q is p else dev(q)
    gi, gd = pointops.knnquery(ns, pd, qd, offsets(o), offsets(qo))
    oi, od2 = O.knnquery(ns, p, q, o, qo)
    assert np.array_equal(host(gi), oi), f"kNN indices differ from the oracle's in {(host(gi) != oi).any(1).sum()} of {len(oi)} queries"
    if want_dist:
        np.testing.assert_allclose(host(gd), np.sqrt(od2), rtol=1e-6, atol=0)
    return oi, np.sqrt(od2)


def assert_fps_is_the_oracles(p, o, n_o):
    from etch_amd.models import pointops
    gi = host(pointops.furthestsampling(dev(p), offsets(o), offsets(n_o)))
    oi = O.furthestsampling(p, o, n_o)
    assert np.array_equal(gi, oi), f"FPS indices differ from the oracle's at {(gi != oi).sum()} of {len(oi)} places"
    return oi


_CACHE = {}


def cached(key, make):
    """One reference at a time: consecutive cases of a parametrised test share it, and it is never modified."""
    if _CACHE.get("key") != key:
        _CACHE.clear()
        _CACHE.update(key=key, value=make())
    return _CACHE["value"]


# ================================================================================================ 2. attention core
PT_SHAPES = [(64, 8), (128, 8), (64, 16), (128, 16), (256, 16), (512, 16)]
RAGGED_N = {(64, 8): 1003, (128, 8): 517, (64, 16): 301, (128, 16): 1001, (256, 16): 333, (512, 16): 397}
GRID_ALL_IMPLS = {(64, 8), (128, 16)}         # split's first GEMM there: R = n ns >= 8192, K = c, O = c / 8 <= 16 -> gemm_wres_kernel
ATTN_CASES = [(c, ns, size, impl) for c, ns in PT_SHAPES for size in ("ragged", "grid") for impl in ("mfma", "split", "valu")
              if size == "ragged" or impl == "mfma" or (c, ns) in GRID_ALL_IMPLS]


def attention_points(c, ns, size):
    """ragged: [5, n1, n2] with n odd (a half-filled wave at ns = 8, a partly filled last workgroup) and a segment shorter than nsample.
    grid: 8 CUs (64 / ns) + 137 points: every workgroup of the largest persistent grid (CUs x min(8, occupancy) workgroups of 64 / ns
    points) takes a second trip through pt_attention_mfma_kernel's tile loop, and the last trip is ragged."""
    if size == "ragged":
        n = RAGGED_N[(c, ns)]
        assert n % 2 == 1 and n % (64 // ns) != 0
    else:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = 8 * cus * (64 // ns) + 137
        assert n > 8 * cus * 64 // ns and n % 2 == 1 and n % (64 // ns) != 0
    return n, [5, (n - 5) // 2, n - 5 - (n - 5) // 2]


def attention_reference(c, ns, size):
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1
    n, segs = attention_points(c, ns, size)

    def make():
        p, x, o = Y.cloud(segs, c, 1000 * c + ns + n)
        mod = P.PointTransformerLayer(c, c, 8, ns)
        y64, y32 = Y.both(lambda cast: S1.pt_layer(Y.state(mod, SEED, cast), "", cast(p), cast(x), torch.from_numpy(o), ns))
        g = np.random.default_rng(c + ns)
        bn = (g.uniform(0.5, 1.5, c).astype(np.float32), (0.1 * g.standard_normal(c)).astype(np.float32))
        return p, x, o, y64, y32, bn

    return cached(("attn", c, ns, n), make)


@pytest.mark.parametrize("c,ns,size,impl", ATTN_CASES)
def test_pt_attention_vs_fp64(c, ns, size, impl):
    """PointTransformerLayer in eval() -- q|k|v GEMM, kNN, the attention core `impl` (mfma: etch_pt_attention_mfma; split: etch_pt_attn_prep,
    two etch_linear, etch_pt_attn_aggregate; valu: etch_pt_attention) -- against oracle pt_layer in fp64, without and with the fused output
    BatchNorm + ReLU (reference: relu(y scale + shift) with the same constants)."""
    from etch_amd import ops
    from etch_amd.models import pointtransformer_seg as P
    assert (c, ns) in ops.PT_MFMA_SHAPES
    p, x, o, y64, y32, bn = attention_reference(c, ns, size)
    assert_knn_is_the_oracles(ns, p, p, o, o)
    layer = load_seeded(P.PointTransformerLayer(c, c, 8, ns), SEED).cuda().eval()
    layer.attention_impl = impl
    pd, xd, od = dev(p), dev(x), offsets(o)
    with torch.no_grad():
        plain = host(layer([pd, xd, od]))
        fused = host(layer([pd, xd, od], out_bn=(dev(bn[0]), dev(bn[1]))))
    Y.check(f"attention c={c} ns={ns} n={len(p)} {impl}", plain, y64, y32)
    Y.check(f"attention c={c} ns={ns} n={len(p)} {impl} +bn+relu", fused, Y.bn_relu(y64, *bn), Y.bn_relu(y32, *bn))


# ================================================================================================ 3. modules at the nets' widths
@pytest.mark.parametrize("c,ns,n", [(64, 8, 1003), (128, 16, 1001), (256, 16, 333), (512, 16, 97)])
def test_pt_block_vs_fp64(c, ns, n):
    """PointTransformerBlock, the default four-kernel form (linear1 + bn1 + ReLU, attention with the fused bn2 + ReLU tail,
    linear3 + bn3 + residual + ReLU through res_mode = 1) against oracle pt_block."""
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1
    segs = [5, (n - 5) // 2, n - 5 - (n - 5) // 2]
    p, x, o = Y.cloud(segs, c, 7 * c + n)
    mod = P.PointTransformerBlock(c, c, 8, ns)
    y64, y32 = Y.both(lambda cast: S1.pt_block(Y.state(mod, SEED, cast), "", cast(p), cast(x), torch.from_numpy(o), ns))
    assert_knn_is_the_oracles(ns, p, p, o, o)
    block = load_seeded(mod, SEED).cuda().eval()
    with torch.no_grad():
        got = host(block([dev(p), dev(x), offsets(o)])[1])
    Y.check(f"block c={c} ns={ns} n={n}", got, y64, y32)


DOWN_SEGS = [401, 230, 23]                     # 23 points -> 5 coarse points, fewer than nsample


def down_reference(ci, co):
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1

    def make():
        p, x, o = Y.cloud(DOWN_SEGS, ci, 3 * ci + co)
        mod = P.TransitionDown(ci, co, 4, 16)
        (p64, y64, no64), (_, y32, _) = Y.both(lambda cast: S1.pt_down(Y.state(mod, SEED, cast), "", cast(p), cast(x), torch.from_numpy(o), 4, 16))
        return p, x, o, p64, y64, y32, no64

    return cached(("down", ci, co), make)


@pytest.mark.parametrize("split", [True, False], ids=["split_linear", "grouped_rows"])
@pytest.mark.parametrize("ci,co", [(64, 128), (128, 128), (128, 256), (256, 256), (256, 512)])
def test_transition_down_stride4_vs_fp64(ci, co, split):
    """TransitionDown(stride 4, nsample 16) at every width pair of the nets, in both forms (per-source-point GEMM + etch_pt_down_gather_max;
    etch_pt_group rows -> GEMM -> etch_rows_maxpool) against oracle pt_down: FPS index, coarse points and offsets exactly, features by the rule."""
    from etch_amd.models import pointtransformer_seg as P
    p, x, o, p64, y64, y32, no64 = down_reference(ci, co)
    assert [int(v) for v in no64] == [100, 157, 162]
    fps = assert_fps_is_the_oracles(p, o, no64)
    assert_knn_is_the_oracles(16, p, p[fps], o, no64)
    down = load_seeded(P.TransitionDown(ci, co, 4, 16), SEED).cuda().eval()
    down.split_linear = split
    with torch.no_grad():
        p2, x2, o2 = down([dev(p), dev(x), offsets(o)])
    assert np.array_equal(host(o2), no64) and o2.dtype == torch.int32
    assert np.array_equal(host(p2).astype(np.float64), p64) and np.array_equal(host(p2), p[fps])
    Y.check(f"down stride=4 {ci}->{co} {'split_linear' if split else 'grouped_rows'}", host(x2), y64, y32)


@pytest.mark.parametrize("co", [64, 128])
def test_transition_down_stride1_vs_fp64(co):
    """enc1's TransitionDown(67 -> co, stride 1): the 67 input columns [p | x] zero-padded to 68 as _unet does (the weight is padded to match
    inside the module), against oracle pt_down on the 67 real columns."""
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1
    p, x, o = Y.cloud([5, 500, 498], 67, 67 + co)
    mod = P.TransitionDown(67, co, 1, 8)
    (_, y64, _), (_, y32, _) = Y.both(lambda cast: S1.pt_down(Y.state(mod, SEED, cast), "", cast(p), cast(x), torch.from_numpy(o), 1, 8))
    down = load_seeded(mod, SEED).cuda().eval()
    xd = torch.cat((dev(x), torch.zeros((len(x), 1), device="cuda")), 1)
    with torch.no_grad():
        p2, x2, o2 = down([dev(p), xd, offsets(o)])
    assert np.array_equal(host(p2), p) and np.array_equal(host(o2), o)
    Y.check(f"down stride=1 67->{co}", host(x2), y64, y32)


def test_transition_up_head_vs_fp64():
    """TransitionUp(512, None) on 32 segments of unequal length, one of 1 point: etch_seg_mean, the 512 -> 512 linear on the means,
    etch_concat_bcast and the 1024 -> 512 linear + BN + ReLU, against oracle pt_up."""
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1
    lens = np.random.default_rng(5).integers(2, 40, 32)
    lens[7] = 1
    p, x, o = Y.cloud(lens.tolist(), 512, 512)
    mod = P.TransitionUp(512, None)
    y64, y32 = Y.both(lambda cast: S1.pt_up(Y.state(mod, SEED, cast), "", [cast(p), cast(x), torch.from_numpy(o)]))
    up = load_seeded(mod, SEED).cuda().eval()
    with torch.no_grad():
        got = host(up([dev(p), dev(x), offsets(o)]))
    Y.check(f"up head 512 segments=32 n={len(p)}", got, y64, y32)


@pytest.mark.parametrize("ci,co", [(512, 256), (256, 256), (256, 128), (128, 128), (128, 64)])
def test_transition_up_vs_fp64(ci, co):
    """TransitionUp(ci, co) with two inputs against oracle pt_up.  The coarse points are the FPS of the fine ones, so a quarter of the queries
    have a 3-NN distance of exactly 0 (weight 1 / (0 + 1e-8)); the last segment's coarse level holds 2 points, so its third neighbour is the
    padded slot (the segment's first row at distance sqrt(1e10))."""
    from etch_amd.models import pointtransformer_seg as P
    from oracle import stage1 as S1
    p1, x1, o1 = Y.cloud([301, 203, 9], co, 5 * ci + co)
    o2 = np.array([75, 125, 127], np.int32)
    fps = assert_fps_is_the_oracles(p1, o1, o2)
    p2 = p1[fps]
    x2 = torch.randn(len(p2), ci, generator=torch.Generator().manual_seed(ci + co)).numpy()
    idx, dist = assert_knn_is_the_oracles(3, p2, p1, o2, o1, want_dist=True)
    assert (dist[:, 0] == 0).sum() == len(p2) and (dist[-9:, 2] == np.float32(1e5)).all() and (idx[-9:, 2] == 125).all()
    mod = P.TransitionUp(ci, co)
    y64, y32 = Y.both(lambda cast: S1.pt_up(Y.state(mod, SEED, cast), "", [cast(p1), cast(x1), torch.from_numpy(o1)],
                                            [cast(p2), cast(x2), torch.from_numpy(o2)]))
    up = load_seeded(mod, SEED).cuda().eval()
    with torch.no_grad():
        got = host(up([dev(p1), dev(x1), offsets(o1)], [dev(p2), dev(x2), offsets(o2)]))
    Y.check(f"up {ci}->{co}", got, y64, y32)


def _seed_heads(net, prefixes):
    sd = net.state_dict()
    for k, v in sd.items():
        if k.startswith(prefixes) and not k.endswith("num_batches_tracked"):
            sd[k] = seeded_tensor(k, v.shape, v.dtype, SEED)
    net.load_state_dict(sd)
    return {k: v.clone() for k, v in sd.items() if k.startswith(prefixes)}


@pytest.fixture(scope="module")
def confidence_net():
    from etch_amd.models import pointtransformer_seg as P
    net = P.get_pointtransformer_confidence(c=67, k=86)
    heads = _seed_heads(net, ("cls.", "confi."))
    return net.cuda().eval(), heads


@pytest.fixture(scope="module")
def magnitude_net():
    from etch_amd.models import pointtransformer_seg as P
    net = P.get_pointtransformer_magnitude(c=67, k=1)
    heads = _seed_heads(net, ("final_layer.",))
    return net.cuda().eval(), heads


def _run_head(net, feats):
    """The net's own forward with the U-Net replaced by the given feature matrix: everything after `_unet` is the production code."""
    r = feats.shape[0]
    net._unet = lambda pxo: feats
    try:
        with torch.no_grad():
            return net([torch.zeros((r, 3), device="cuda"), None, offsets([r])])
    finally:
        del net._unet


@pytest.mark.parametrize("R", [700, 8192 + 37])
def test_confidence_head_vs_fp64(confidence_net, R):
    """cls.0 + BN + ReLU, cls.3, etch_linear_relu_dot with the model's permuted weight operand and etch_softmax_dot (k = 86) on a random (R, 128)
    feature matrix against the fp64 restatement of pt_confidence after the U-Net."""
    net, heads = confidence_net
    x1 = np.random.default_rng(R).standard_normal((R, 128)).astype(np.float32)
    (lg64, cf64), (lg32, cf32) = Y.both(lambda cast: Y.confidence_head({k: cast(v) for k, v in heads.items()}, "", cast(x1), 86))
    logits, conf = _run_head(net, dev(x1))
    assert logits.shape == (1, R, 86) and conf.shape == (1, R, 1)
    Y.check(f"confidence head R={R} logits", host(logits)[0], lg64, lg32)
    Y.check(f"confidence head R={R} confidence", host(conf)[0], cf64, cf32)


@pytest.mark.parametrize("R", [700, 8192 + 37])
def test_magnitude_head_vs_fp64(magnitude_net, R):
    """final_layer (Linear 64 -> 64 + BN + ReLU, Linear 64 -> 1) on a random (R, 64) feature matrix; at R = 8 229 the last layer
    (R >= 8192, K = 64, O = 1) runs gemm_wres_kernel."""
    net, heads = magnitude_net
    x1 = np.random.default_rng(R + 1).standard_normal((R, 64)).astype(np.float32)
    m64, m32 = Y.both(lambda cast: Y.magnitude_head({k: cast(v) for k, v in heads.items()}, "", cast(x1)))
    got = _run_head(net, dev(x1))
    assert got.shape == (1, R, 1)
    Y.check(f"magnitude head R={R}", host(got)[0], m64, m32)


# ================================================================================================ 4. glue kernels on their own
def _index_problem(n, m, ns, seed):
    g = np.random.default_rng(seed)
    p = (g.standard_normal((n, 3)) * 0.3).astype(np.float32)
    new_p = (g.standard_normal((m, 3)) * 0.3).astype(np.float32)
    idx = g.integers(0, n, (m, ns)).astype(np.int32)
    idx[0, :] = n - 1                                                              # the last source row is read
    return g, p, new_p, idx


@pytest.mark.parametrize("c", [64, 35])
@pytest.mark.parametrize("pad_to", [1, 4])
def test_pt_group_exact(c, pad_to):
    """etch_pt_group: x is a column window of a wider matrix (ldx > c); the padding columns come back zero."""
    from etch_amd import ops
    n, m, ns = 211, 53, 16
    g, p, new_p, idx = _index_problem(n, m, ns, c + pad_to)
    x = g.standard_normal((n, c)).astype(np.float32)
    got = ops.pt_group(dev(p), dev(new_p), window(x, c + 9, 5, fill=7.0), dev(idx), pad_to=pad_to)
    ld = -(-(3 + c) // pad_to) * pad_to
    assert got.shape == (m * ns, ld)
    Y.check_exact(f"pt_group c={c} pad_to={pad_to}", host(got), Y.group_rows(p, new_p, x, idx, ld))


@pytest.mark.parametrize("c", [3, 64, 512])
@pytest.mark.parametrize("ns", [8, 16])
def test_rows_maxpool_and_gather_rows_exact(ns, c):
    """etch_gather_rows with ldx > c, and etch_rows_maxpool over the gathered (m ns, c) rows (its ABI takes contiguous rows only)."""
    from etch_amd import ops
    n, m = 301, 77
    g, _, _, idx = _index_problem(n, m, ns, 10 * c + ns)
    x = g.standard_normal((n, c)).astype(np.float32)
    rows = ops.gather_rows(window(x, c + 7, 3, fill=9.0), dev(idx.reshape(-1)))
    Y.check_exact(f"gather_rows c={c} rows={m * ns}", host(rows), x[idx.reshape(-1)])
    Y.check_exact(f"rows_maxpool c={c} ns={ns}", host(ops.rows_maxpool(rows, ns)), Y.rows_maxpool(x[idx.reshape(-1)], ns))


@pytest.mark.parametrize("co", [128, 512])
def test_pt_down_gather_max_vs_fp64(co):
    """etch_pt_down_gather_max with ux a column window (ldu > co); the first output rows see only candidates far below zero, so they are 0
    after the ReLU."""
    from etch_amd import ops
    n, m, ns = 407, 101, 16
    g, p, new_p, idx = _index_problem(n, m, ns, co)
    ux = g.standard_normal((n, co)).astype(np.float32)
    ux[:20] = -9.0 - np.abs(ux[:20])
    idx[1:6] = g.integers(0, 20, (5, ns))
    wp = (g.standard_normal((co, 3)) * 0.5).astype(np.float32)
    scale, shift = g.uniform(0.5, 1.5, co).astype(np.float32), (0.1 * g.standard_normal(co)).astype(np.float32)
    got = ops.pt_down_gather_max(window(ux, co + 8, 4, fill=50.0), dev(p), dev(new_p), dev(idx), dev(wp), dev(scale), dev(shift))
    ref64, ref32 = (Y.down_gather_max(ux, p, new_p, idx, wp, scale, shift, t) for t in (np.float64, np.float32))
    assert (ref64[1:6] == 0).all() and (host(got)[1:6] == 0).all()
    Y.check(f"pt_down_gather_max co={co}", host(got), ref64, ref32)


@pytest.mark.parametrize("c", [64, 3])
def test_pt_interp_add_vs_fp64(c):
    """etch_pt_interp_add against fp64 with the fp32 distances the kernel received: generic rows, rows with an exact-zero distance, and rows
    between two coincident coarse points (two zero distances: weights 1/2, 1/2)."""
    from etch_amd import ops
    n, m = 333, 90
    g = np.random.default_rng(c)
    a, f = g.standard_normal((n, c)).astype(np.float32), g.standard_normal((m, c)).astype(np.float32)
    idx = g.integers(0, m, (n, 3)).astype(np.int32)
    idx[0] = m - 1
    dist = np.sort(g.uniform(0.01, 0.5, (n, 3)).astype(np.float32), axis=1)
    dist[10:90, 0] = 0.0
    dist[90:120, :2] = 0.0
    got = ops.pt_interp_add(dev(a), dev(f), dev(idx), dev(dist))
    ref64, ref32 = (Y.interp_add(a, f, idx, dist, t) for t in (np.float64, np.float32))
    np.testing.assert_allclose(ref64[90:120], a[90:120] + 0.5 * (f[idx[90:120, 0]].astype(np.float64) + f[idx[90:120, 1]]), rtol=0, atol=1e-5)
    Y.check(f"pt_interp_add c={c}", host(got), ref64, ref32)


def _segment_lengths(nseg):
    if nseg == 1:
        return [3000]
    if nseg == 2:
        return [1, 3000]
    lens = np.random.default_rng(nseg).integers(1, 200, nseg)
    lens[3], lens[17], lens[31] = 1, 3000, 1
    return lens.tolist()


@pytest.mark.parametrize("c", [4, 512])
@pytest.mark.parametrize("nseg", [1, 2, 32])
def test_seg_mean_and_concat_bcast(nseg, c):
    """etch_seg_mean by the rule, etch_concat_bcast exactly, on segments of 1 to 3 000 rows.  The rows are what TransitionUp's head branch
    sees: the output of a PointTransformerBlock, i.e. values after a ReLU (relu(randn))."""
    from etch_amd import ops
    lens = _segment_lengths(nseg)
    o = np.cumsum(lens).astype(np.int32)
    g = np.random.default_rng(100 * nseg + c)
    x = np.maximum(g.standard_normal((int(o[-1]), c)), 0).astype(np.float32)
    xd, od = dev(x), offsets(o)
    mean = ops.seg_mean(xd, od, nseg)
    Y.check(f"seg_mean segments={nseg} c={c}", host(mean), Y.seg_mean(x, o, torch.float64), Y.seg_mean(x, o, torch.float32))
    gm = g.standard_normal((nseg, c)).astype(np.float32)
    Y.check_exact(f"concat_bcast segments={nseg} c={c}", host(ops.concat_bcast(xd, dev(gm), od, nseg)), Y.concat_bcast(x, gm, o))


@pytest.mark.parametrize("G,J", [(86, 128), (1, 64), (5, 32), (3, 192)])
def test_grouped_dot_vs_fp64(G, J):
    """etch_grouped_dot on its own: h a column window (ldh > G J), the result written through out= into a window (ldo > G) of a buffer whose
    other columns must keep their sentinel, ragged R."""
    from etch_amd import ops
    R = 203
    g = np.random.default_rng(G * J)
    h = g.standard_normal((R, G * J)).astype(np.float32)
    w, b = (g.standard_normal((G, J)) / np.sqrt(J)).astype(np.float32), g.standard_normal(G).astype(np.float32)
    buf = torch.full((R, G + 5), -777.0, device="cuda")
    ops.grouped_dot(window(h, G * J + 12, 8, fill=3.0), dev(w), dev(b), G, J, out=buf[:, 2:2 + G])
    Y.check(f"grouped_dot G={G} J={J}", host(buf[:, 2:2 + G]), Y.grouped_dot(h, w, b, G, J, torch.float64), Y.grouped_dot(h, w, b, G, J, torch.float32))
    assert (buf[:, :2] == -777.0).all() and (buf[:, 2 + G:] == -777.0).all()


@pytest.mark.parametrize("G", [1, 64, 65, 86])
def test_softmax_dot_vs_fp64(G):
    """etch_softmax_dot: rows whose logits carry a common offset of +80 / -80 and a spread of 30 (the maximum subtraction and the range of
    the fast exponential), rows with all logits equal, ordinary rows."""
    from etch_amd import ops
    R = 515
    g = np.random.default_rng(G)
    logits = g.standard_normal((R, G))
    logits[:150] = 80.0 + g.uniform(-15, 15, (150, G))
    logits[150:300] = -80.0 + g.uniform(-15, 15, (150, G))
    logits[300:340] = g.standard_normal((40, 1)) * 5
    logits = logits.astype(np.float32)
    v = g.standard_normal((R, G)).astype(np.float32)
    got = ops.softmax_dot(dev(logits), dev(v))
    Y.check(f"softmax_dot G={G}", host(got), Y.softmax_dot(logits, v, torch.float64), Y.softmax_dot(logits, v, torch.float32))


# ================================================================================================ 5. etch_linear's remaining branches
def _linear_problem(R, K, O, seed, rows_x=None):
    g = np.random.default_rng(seed)
    x = g.standard_normal((R if rows_x is None else rows_x, K)).astype(np.float32)
    w = (g.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32)
    # bias / scale / shift of the size a folded eval-mode BatchNorm has, so that no channel dies in the ReLU
    bias, sh = ((0.3 * g.standard_normal(O)).astype(np.float32) for _ in range(2))
    sc = g.uniform(0.5, 1.5, O).astype(np.float32)
    res = g.standard_normal((R, O)).astype(np.float32)
    return x, w, bias, sc, sh, res


def _linear_forms_gpu(run, bias, sc, sh, res):
    """The four epilogue forms of test_linear_epilogues; run(**kw) -> numpy result of ops.linear with these epilogue arguments."""
    return (run(), run(bias=bias, scale=sc, shift=sh, act="relu"), run(bias=bias, act="relu", res=res, res_mode=1),
            run(act="leaky_relu", res=res, res_mode=2))


FORMS = ("plain", "bias+bn+relu", "bias+res+relu", "leaky+res")


@pytest.mark.parametrize("R,K,O", [(8192, 64, 1), (8191, 64, 1), (8203, 128, 16), (20011, 64, 8), (9001, 128, 1)])
def test_linear_weight_resident_kernel_vs_fp64(R, K, O):
    """gemm_wres_kernel (R >= 8192, O <= 16, K in {64, 128}) and the tiled side of its boundary: first row count on the kernel, the last
    row count off it, a ragged last 16-row tile with a full output tile, several tiles per wave (the prefetch path), K = 128 with O = 1."""
    from etch_amd import ops
    x, w, bias, sc, sh, res = _linear_problem(R, K, O, R + K + O)
    lin64, lin32 = Y.linear_refs(x, w)
    xd, wd = dev(x), dev(w)
    got = _linear_forms_gpu(lambda **kw: host(ops.linear(xd, wd, **kw)), dev(bias), dev(sc), dev(sh), dev(res))
    for name, y, r64, r32 in zip(FORMS, got, Y.linear_forms(lin64, bias, sc, sh, res), Y.linear_forms(lin32, bias, sc, sh, res)):
        Y.check(f"linear R={R} K={K} O={O} {name}", y, r64, r32)


def test_linear_weight_resident_kernel_row_map_vs_fp64():
    """The row map (row_idx / grp) carried by gemm_wres_kernel: R = 2 * 550 * 8 = 8 800 >= 8192, K = 64, O = 8; reference = the gather written out."""
    from etch_amd import ops
    b, p_in, p_out, grp, K, O = 2, 600, 550, 8, 64, 8
    R = b * p_out * grp
    x, w, bias, sc, sh, res = _linear_problem(R, K, O, 4, rows_x=b * p_in * grp)
    sidx = np.stack([np.random.default_rng(i).permutation(p_in)[:p_out] for i in range(b)]).astype(np.int32)
    xg = np.concatenate([x.reshape(b, p_in, grp, K)[i, sidx[i]] for i in range(b)]).reshape(R, K)
    lin64, lin32 = Y.linear_refs(xg, w)
    xd, wd, sd = dev(x), dev(w), dev(sidx)
    run = lambda **kw: host(ops.linear(xd, wd, row_idx=sd, grp=grp, p_in=p_in, p_out=p_out, rows=R, **kw))
    got = _linear_forms_gpu(run, dev(bias), dev(sc), dev(sh), dev(res))
    for name, y, r64, r32 in zip(FORMS, got, Y.linear_forms(lin64, bias, sc, sh, res), Y.linear_forms(lin32, bias, sc, sh, res)):
        Y.check(f"linear row map R={R} K={K} O={O} {name}", y, r64, r32)


def _misaligned(a):
    """A contiguous device copy of `a` that starts one float past a 16-byte boundary."""
    flat = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[1:1 + a.size].view(a.shape)
    t.copy_(dev(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


SENTINEL = -12345.678


@pytest.mark.parametrize("variant", ["x_window", "misaligned", "res_window", "out_window", "all_windows"])
@pytest.mark.parametrize("R,K,O", [(777, 64, 64), (500, 128, 384), (300, 128, 86)])
def test_linear_strided_and_misaligned_operands_vs_fp64(R, K, O, variant):
    """etch_linear with operands that are not the contiguous, 16-byte aligned matrices of test_linear_epilogues, on two weight-stationary split
    shapes and a tiled one: X as the column window [K, 2K) of an (R, 3K) matrix (ldx != K); X and W one float past a 16-byte boundary (the
    non-vector load path with K % 4 == 0); res as a window (ldr != O); out= as a column window of a wider buffer (ldy > O) pre-filled with a
    sentinel, every element of which outside the window must be bit-identical afterwards; and all windows at once."""
    from etch_amd import ops
    x, w, bias, sc, sh, res = _linear_problem(R, K, O, R + K + O)
    lin64, lin32 = Y.linear_refs(x, w)
    every = variant == "all_windows"
    xd = window(x, 3 * K, K, fill=11.0) if every or variant == "x_window" else _misaligned(x) if variant == "misaligned" else dev(x)
    wd = _misaligned(w) if variant == "misaligned" else dev(w)
    resd = window(res, O + 12, 8, fill=13.0) if every or variant == "res_window" else dev(res)
    c0, ldy = 4, O + 12

    def run(**kw):
        if not (every or variant == "out_window"):
            return host(ops.linear(xd, wd, **kw))
        buf = torch.full((R + 2, ldy), SENTINEL, dtype=torch.float32, device="cuda")
        out = buf[1:R + 1, c0:c0 + O]
        assert ops.linear(xd, wd, out=out, **kw) is out
        y = host(out).copy()
        out.fill_(SENTINEL)
        assert torch.equal(buf.view(torch.int32), torch.full_like(buf, SENTINEL).view(torch.int32)), "a store landed outside the out= window"
        return y

    got = _linear_forms_gpu(run, dev(bias), dev(sc), dev(sh), resd)
    for name, y, r64, r32 in zip(FORMS, got, Y.linear_forms(lin64, bias, sc, sh, res), Y.linear_forms(lin32, bias, sc, sh, res)):
        Y.check(f"linear R={R} K={K} O={O} {variant} {name}", y, r64, r32)
