"""Every autograd Function of etch_amd/autograd.py that the encoder and the direction head use, against fp64 autograd through the oracle's
form, at every width EPN_layer_num 1 .. 4 builds, under the per-channel entitled-error rule (tests/_bwd_fp64.py, tests/_pt_fp64.py):
max_ch e_gpu <= 2 max_ch e_32 + 1e-6 with e_32 the oracle's own fp32 autograd; etch_gemm_tn_fused / etch_colsum_fused under the derived
bound of an exact fp64 accumulation.  Every case prints `PIN` lines; profiles/backward_fp64_pins.txt is the record of a run."""
import contextlib

import numpy as np
import pytest
import torch

from tests import _bwd_fp64 as B

pytestmark = pytest.mark.gpu

_CACHE = {}


def cached(key, make):
    """One reference at a time: consecutive cases of a parametrised test share it, and it is never modified."""
    if _CACHE.get("key") != key:
        _CACHE.clear()
        _CACHE.update(key=key, value=make())
    return _CACHE["value"]


def dev(a, grad=False):
    a = np.asarray(a)
    if a.size == 0:                                         # (torch.from_numpy gives an empty array strides of 0; torch's own empty tensors have the usual ones)
        return torch.empty(a.shape, dtype=torch.float32, device="cuda")
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.requires_grad_() if grad else t


@contextlib.contextmanager
def recorded_calls():
    """The (name, args) of every call into the native library that etch_amd.autograd makes inside the block."""
    from etch_amd import _lib
    calls, real = [], _lib.call

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)
    _lib.call = spy
    try:
        yield calls
    finally:
        _lib.call = real


# ================================================================================================ inter conv
PAIRS = B.encoder_channel_pairs()
SETTINGS = {"slots-one-chunk": (True, False), "slots-chunks": (True, True), "fallback-one-chunk": (False, False), "fallback-chunks": (False, True)}


def test_channel_pairs_are_the_encoders():
    assert [p[:2] for p in PAIRS] == [(1, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256)]
    assert all(nn <= 64 for _, _, nn, _, _ in PAIRS)                    # every conv is one etch_inter_dfeat_slots can take


def inter_gpu(pr, slot, chunk):
    """One forward + backward of A.inter_so3conv on the problem `pr` with A.SLOT_DFEAT = slot in chunks of `chunk` target points (None: one
    chunk) -> (y, dfeats or None, dW, dbias) as numpy arrays, the library calls made."""
    from etch_amd import autograd as A
    conv = pr["conv"].cuda()
    rk = conv._derived()[0]
    old = A.SLOT_DFEAT, A.CHUNK_BYTES
    A.SLOT_DFEAT, A.CHUNK_BYTES = slot, (1.2e9 if chunk is None else 1.0)
    try:
        f = dev(B.channels_last(pr["feats"]), grad=pr["cin"] > 1)
        W, bias = dev(pr["W"], True), dev(pr["bias"], True)
        with recorded_calls() as calls:
            y = A.inter_so3conv(f, W, bias, pr["xyz"].cuda(), pr["new_xyz"].cuda(), pr["ball"].cuda(), rk, pr["sigma"], chunk=1024 if chunk is None else chunk)
            (y * dev(B.channels_last(pr["G"]))).sum().backward()
        return (B.host(y), None if f.grad is None else B.host(f.grad), B.host(W.grad), B.host(bias.grad)), calls
    finally:
        A.SLOT_DFEAT, A.CHUNK_BYTES = old


def inter_reference(pair, **kw):
    def make():
        pr = B.inter_problem(*pair, **kw)
        r64, r32, pr["G"] = B.inter_oracle(pr)
        return pr, r64, r32
    return cached(("inter", pair, tuple(sorted(kw.items()))), make)


def check_inter(tag, got, r64, r32):
    y, df, dW, db = got
    B.check(f"{tag} y", y, B.channels_last(r64.y), B.channels_last(r32.y))
    if df is not None:
        B.check(f"{tag} dfeats", df, B.channels_last(r64.grads["feats"]), B.channels_last(r32.grads["feats"]))
    else:
        assert "feats" not in r64.grads
    B.check_weight(f"{tag} dW", dW, r64.grads["W"], r32.grads["W"])
    B.check_bias(f"{tag} dbias", db, r64.grads["bias"], r32.grads["bias"])


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_inter_conv_vs_fp64(pair, setting):
    """A.inter_so3conv (forward: the fused conv; backward: etch_inter_x1_rows, etch_gemm_tn_fused with accumulation over the chunks,
    etch_colsum_fused and one of the two feature-gradient kernels) against fp64 autograd through the oracle's un-fused form, on two scans of
    96 points whose ball lists are padded with repeats of their neighbours.  Launch branches by case:
      slots-*      etch_inter_dfeat_slots (inter_dfeat_slots_kernel) + the ordered segment sum; fallback-*: etch_inter_dfeat (inter_dfeat_kernel);
      *-one-chunk  every target point in one pass; *-chunks: at least 3 chunks of target points with a ragged last one, the weight and
                   feature gradients accumulated over them, at least one source point reached from two chunks;
      128-128, 128-256, 256-256   both kernels run a second .. fourth window of 64 input channels (cbase > 0);
      1-32         the first conv: occupancy features, no feature gradient.
    Every setting is held to fp64 on its own, and a second run gives the same bits."""
    slot, chunked = SETTINGS[setting]
    pr, r64, r32 = inter_reference(pair)
    cin, cout, nn = pair[:3]
    ball, p2 = pr["ball"].numpy(), pr["ball"].shape[1]
    assert any(len(np.unique(row)) < nn for row in ball.reshape(-1, nn)), "no ball list repeats an index"
    chunk = p2 * 5 // 12 if chunked else None
    got, calls = inter_gpu(pr, slot, chunk)
    ranges = [(a[4], a[5]) for name, a in calls if name == "etch_inter_x1_rows"]
    if chunked:
        assert len(ranges) >= 3 and ranges[-1][1] < ranges[0][1] and sum(pc for _, pc in ranges) == p2, ranges
        sources = [set(ball[:, s:s + pc].reshape(-1).tolist()) for s, pc in ranges]
        assert sources[0] & sources[1], "no source point is reached from two chunks"
    else:
        assert ranges == [(0, p2)], ranges
    names = {name for name, _ in calls}
    if cin > 1:
        assert ("etch_inter_dfeat_slots" in names) == slot and ("etch_inter_dfeat" in names) == (not slot), names
    check_inter(f"inter {cin}->{cout} nn={nn} {setting}", got, r64, r32)
    again, _ = inter_gpu(pr, slot, chunk)
    assert same_bits(got, again)


@pytest.mark.parametrize("slot", [True, False], ids=["slots", "fallback"])
def test_inter_conv_single_target_point_vs_fp64(slot):
    """b = 1, p2 = 1 at 128 -> 128 (two channel windows): one workgroup per launch of etch_inter_x1_rows / etch_inter_dfeat_slots, every
    source point outside the one ball gets an exactly zero gradient from either feature-gradient kernel."""
    pair = (128, 128, 32, 1, True)
    pr, r64, r32 = inter_reference(pair, b=1, p2=1)
    assert pr["ball"].shape == (1, 1, 32)
    got, _ = inter_gpu(pr, slot, None)
    check_inter(f"inter 128->128 nn=32 b=1 p2=1 {'slots' if slot else 'fallback'}", got, r64, r32)
    outside = np.setdiff1d(np.arange(pr["n"]), pr["ball"].numpy().reshape(-1))
    assert len(outside) and not got[1][0, outside].any()


# ================================================================================================ intra conv
@pytest.mark.parametrize("C,p", [(32, 37), (64, 37), (128, 1), (128, 37), (256, 1), (256, 37)])
def test_intra_conv_vs_fp64(C, p):
    """A.intra_so3conv at the widths of encoder depths 3 and 4, one point and 37 (forward and data gradient: the fused intra kernel with its
    sum over K = 12 C closed after every tap, the latter with the inverse anchor tables; weight gradient: etch_intra_rows + etch_gemm_tn_fused
    with N = 12 C = 1536 / 3072 columns; bias: etch_colsum_fused), and at the widths of depths 1 and 2 (two points per workgroup, one chain)."""
    import etch_amd.vgtk_so3conv as V
    from etch_amd import autograd as A
    from etch_amd.utils.weights import load_seeded
    conv = load_seeded(V.IntraSO3Conv(C, C), 7).eval()
    x = np.random.default_rng(C + p).standard_normal((2, C, p, 60)).astype(np.float32)
    W, bias = conv.basic_conv.W.detach().numpy().copy(), conv.basic_conv.bias.detach().numpy().copy()
    r64, r32, G = B.intra_oracle(x, W, bias, conv.intra_idx)
    xg, Wg, bg = dev(B.channels_last(x), True), dev(W, True), dev(bias, True)
    y = A.intra_so3conv(xg, Wg, bg, conv.intra_idx.cuda())
    (y * dev(B.channels_last(G))).sum().backward()
    tag = f"intra C={C} p={p}"
    B.check(f"{tag} y", B.host(y), B.channels_last(r64.y), B.channels_last(r32.y))
    B.check(f"{tag} dx", B.host(xg.grad), B.channels_last(r64.grads["x"]), B.channels_last(r32.grads["x"]))
    B.check_weight(f"{tag} dW", B.host(Wg.grad), r64.grads["W"], r32.grads["W"])
    B.check_bias(f"{tag} dbias", B.host(bg.grad), r64.grads["bias"], r32.grads["bias"])


# ================================================================================================ InstanceNorm + LeakyReLU
KINK_MARGIN = 1e-3


def instnorm_input(b, C, p, big_mean):
    """x (b, C, p, 60) of spread 1.7; big_mean: every second channel carries a mean 300 times its spread.  LeakyReLU has no derivative at 0:
    elements whose normalised value lies within 2e-3 of it are moved 4e-3 spreads further out, so that every precision takes the same slope
    (asserted on the result: |normalised value| > 1e-3 everywhere; fp32 statistics of a mean-300 channel move it by ~2e-5)."""
    x = np.random.default_rng(1000 * C + p + big_mean).standard_normal((b, C, p, 60)) * 1.7 + 0.3
    if big_mean:
        x[:, ::2] += 300 * 1.7
    x = x.astype(np.float32)
    stats = lambda a: (a.astype(np.float64).mean((2, 3), keepdims=True), a.astype(np.float64).std((2, 3), keepdims=True))
    mu, sd = stats(x)
    xh = (x - mu) / sd
    x = np.where(np.abs(xh) < 2e-3, x + np.where(xh < 0, -4e-3, 4e-3) * sd, x).astype(np.float32)
    mu, sd = stats(x)
    assert np.abs((x - mu) / sd).min() > KINK_MARGIN
    return x


@pytest.mark.parametrize("C,p,big_mean", [(16, 41, False), (64, 41, False), (128, 41, False), (256, 41, False), (32, 1, False), (256, 1, False), (128, 41, True)])
def test_instancenorm_leaky_relu_vs_fp64(C, p, big_mean):
    """A.instnorm_leaky_relu: instnorm_bwd_partial_kernel with rpp = 256 / C = 16, 4, 2 and 1 rows per pass (8: the p = 1 case); p = 1: 60 rows, fewer than INB_CHUNKS = 64, so four chunks are empty; big_mean: half the channels with
    mean / spread = 300, where statistics or a normalisation formed carelessly in fp32 lose five digits."""
    from etch_amd import autograd as A
    x = instnorm_input(2, C, p, big_mean)
    r64, r32, G = B.instnorm_oracle(x)
    xg = dev(B.channels_last(x), True)
    y = A.instnorm_leaky_relu(xg)
    (y * dev(B.channels_last(G))).sum().backward()
    tag = f"instnorm C={C} p={p}{' mean/spread=300' if big_mean else ''}"
    B.check(f"{tag} y", B.host(y), B.channels_last(r64.y), B.channels_last(r32.y))
    B.check(f"{tag} dx", B.host(xg.grad), B.channels_last(r64.grads["x"]), B.channels_last(r32.grads["x"]))


# ================================================================================================ attention
MHSA_NAMES = ["x", "wq", "wk", "wv", "wc", "bc"]


def mhsa_gpu(inputs, G, mode):
    from etch_amd import autograd as A
    ts = [dev(a, True) for a in inputs]
    y = A.mhsa_heads(*ts) if mode == "heads" else A.mhsa_layer(*ts, residual=mode == "residual")
    (y * dev(G)).sum().backward()
    return [B.host(y)] + [B.host(t.grad) for t in ts]


def check_mhsa(tag, got, r64, r32, names):
    B.check(f"{tag} y", got[0], r64.y, r32.y)
    for name, g in zip(names, got[1:]):
        if name == "x":
            B.check(f"{tag} dx", g, r64.grads[name], r32.grads[name])
        elif name == "bc":
            B.check_bias(f"{tag} dbc", g, r64.grads[name], r32.grads[name])
        else:
            B.check_weight(f"{tag} d{name}", g, r64.grads[name], r32.grads[name])


def run_mhsa_case(E, T, mode, q_scale=1.0):
    inputs = B.mhsa_inputs(T, E, 100 * E + T, q_scale)
    if mode == "heads":
        inputs = inputs[:4]
        r64, r32, G = B.mhsa_oracle(*inputs, g_seed=E + T)
    else:
        r64, r32, G = B.mhsa_oracle(*inputs, residual=mode == "residual", g_seed=E + T)
    if q_scale != 1.0:
        pmax = B.max_softmax_probability(inputs[0], inputs[1], inputs[2])
        assert (pmax > 0.99).mean() > 0.5, "most softmax rows were to be saturated"
    got = mhsa_gpu(inputs, G, mode)
    check_mhsa(f"mhsa {mode} E={E} T={T}{' saturated' if q_scale != 1.0 else ''}", got, r64, r32, MHSA_NAMES[:len(inputs)])
    again = mhsa_gpu(inputs, G, mode)
    assert same_bits(got, again)


@pytest.mark.parametrize("mode", ["residual", "plain"])
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_mhsa_layer_vs_fp64(E, T, mode):
    """A.mhsa_layer at the token widths of encoder depths 1, 3 and 4 (and 64, the fused forward kernel, under the same rule): _mhsa_forward's un-fused chain (etch_linear -> etch_mhsa_attention_dim
    -> etch_linear with / without the residual epilogue), mhsa_attention_backward_kernel<4 | 16 | 32> (head width 32: 123 KB of dynamic LDS;
    lanes 60 - 63 shadow token 59 and must store nothing), etch_gemm_tn_fused for the four weight gradients; bitwise repeatable."""
    run_mhsa_case(E, T, mode)


@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_mhsa_heads_vs_fp64(E, T):
    """A.mhsa_heads (the concatenated head outputs, no head_combine): E = 64 takes the fused kernel in mode 2 and
    mhsa_attention_backward_kernel<8>, the other widths the un-fused chain and head widths 4 / 16 / 32."""
    run_mhsa_case(E, T, "heads")


@pytest.mark.parametrize("E", [32, 128, 256])
def test_mhsa_layer_saturated_softmax_vs_fp64(E):
    """Queries scaled by 32: more than half of the softmax rows put over 0.99 on one key (asserted on the fp64 run), so dS = P (dP - D) is a
    difference of nearly equal numbers; the entitlement is still the oracle's own fp32 run on the same inputs."""
    run_mhsa_case(E, 37, "residual", q_scale=32.0)


# ================================================================================================ gemm_tn / colsum: exact accumulation
def _gemm_case(tag, a, bm, rng):
    from etch_amd import autograd as A
    M, N = a.shape[1], bm.shape[1]
    c0 = rng.standard_normal((M, N)).astype(np.float32)
    ah, bh = B.host(a), B.host(bm)
    for accumulate in (0, 1):
        out = A.gemm_tn(a, bm, out=dev(c0), accumulate=bool(accumulate))
        B.check_exact_accumulation(f"gemm_tn {tag} accumulate={accumulate}", B.host(out), ah, bh, c0 if accumulate else None)
        if a.shape[0] == 0:
            assert np.array_equal(B.host(out), c0 if accumulate else np.zeros_like(c0))


def _operands(R, M, N, rng):
    return dev(rng.standard_normal((R, M)).astype(np.float32)), dev(rng.standard_normal((R, N)).astype(np.float32))


def test_gemm_tn_and_colsum_exact_accumulation():
    """etch_gemm_tn_fused and etch_colsum_fused under the derived bound of tests/_bwd_fp64.py check_exact_accumulation, accumulate 0 and 1:
      VEC = false (four predicated 4-byte loads per piece) by width -- (R, M, N) = (777, 35, 64), (300, 3, 3), (1000, 259, 32), (50, 64, 67):
        the Point-Transformer input widths and 3-wide layers --, by stride (lda = M + 1) and by a base 4 bytes off alignment;
      the two-launch fallbacks inside etch_gemm_tn_fused: (20000, 32, 32) -> 79 row ranges > 64, (300, 256, 1088) -> 68 tiles > 64 counters;
      row edges at M = N = 64 (VEC = true, one fused launch): R = 0 (all zeros, or the old C), 1, 31, 32, 33, 257;
      colsum: C = 1, 3, 35 (W = 1), 256 (W = 4), a strided view, R = 0, 1, 5000.
    Afterwards the reduction counters are all zero."""
    from etch_amd import _lib, autograd as A
    rng = np.random.default_rng(17)
    for R, M, N in ((777, 35, 64), (300, 3, 3), (1000, 259, 32), (50, 64, 67)):
        _gemm_case(f"R={R} M={M} N={N} VEC=false by width", *_operands(R, M, N, rng), rng)
    R, M, N = 257, 64, 64
    wide = dev(rng.standard_normal((R, M + 1)).astype(np.float32))
    a, bm = _operands(R, M, N, rng)
    assert wide[:, :M].stride(0) == M + 1
    _gemm_case("R=257 M=64 N=64 VEC=false by lda=M+1", wide[:, :M], bm, rng)
    flat = dev(rng.standard_normal((R * M + 1,)).astype(np.float32))
    off = flat[1:].view(R, M)
    assert off.data_ptr() % 16 == 4 and a.data_ptr() % 16 == 0
    _gemm_case("R=257 M=64 N=64 VEC=false by a 4-byte base offset", off, bm, rng)
    for (R, M, N), why in (((20000, 32, 32), "splits=79"), ((300, 256, 1088), "tiles=68")):
        if why == "splits=79":
            assert (_lib.call("etch_gemm_tn_workspace_floats", R, M, N) - 2) // (2 * M * N) == 79
        else:
            assert -(-M // 64) * -(-N // 64) == 68
        _gemm_case(f"R={R} M={M} N={N} two launches {why}", *_operands(R, M, N, rng), rng)
    for R in (0, 1, 31, 32, 33, 257):
        _gemm_case(f"R={R} M=64 N=64 row edge", *_operands(R, 64, 64, rng), rng)

    def colsum_case(tag, x):
        got = B.host(A.colsum(x))
        xh = B.host(x)
        B.check_exact_accumulation(f"colsum {tag}", got.reshape(-1, 1), xh, np.ones((xh.shape[0], 1), np.float32))
    for C in (1, 3, 35, 256):
        colsum_case(f"R=777 C={C}", dev((rng.standard_normal((777, C)) * 3 + 0.7).astype(np.float32)))
    colsum_case("R=777 C=64 of ldx=70", dev(rng.standard_normal((777, 70)).astype(np.float32))[:, 3:67])
    for R in (0, 1, 5000):
        colsum_case(f"R={R} C=64", dev((rng.standard_normal((R, 64)) * 3 + 0.7).astype(np.float32)))
    torch.cuda.synchronize()
    assert int(A.reduce_counters(torch.device("cuda", torch.cuda.current_device())).abs().sum()) == 0


# ================================================================================================ segment sums
def test_segment_sum_rows_is_the_fp32_sum_in_row_order():
    """A.segment_sum_rows: 1 000 rows of 64 columns into 50 segments -- segment 7 holds half the rows, segments 0, 20 and 49 none.  Against
    the fp64 sum under the rule, and bit for bit the fp32 sum taken in increasing row order (the order its docstring promises: it is what
    makes the inter conv's feature gradient reproducible)."""
    from etch_amd import autograd as A
    rng = np.random.default_rng(23)
    src = rng.standard_normal((1000, 64)).astype(np.float32)
    index = rng.choice(np.setdiff1d(np.arange(50), [0, 7, 20, 49]), 1000)
    index[rng.permutation(1000)[:500]] = 7
    got = B.host(A.segment_sum_rows(dev(src), dev(index.astype(np.int64)), 50))
    ref64, ref32 = np.zeros((50, 64), np.float64), np.zeros((50, 64), np.float32)
    for e in range(1000):
        ref64[index[e]] += src[e]
        ref32[index[e]] += src[e]
    assert ref32.dtype == np.float32 and (index == 7).sum() >= 500 and not ref64[[0, 20, 49]].any()
    B.check("segment_sum_rows 1000x64 -> 50", got, ref64, ref32)
    assert np.array_equal(got, ref32)


# ================================================================================================ A.linear
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("K", [1, 3, 259])
def test_linear_function_vs_fp64(K, act):
    """A.linear (etch_linear forward; backward: etch_linear for dx, etch_gemm_tn_fused for dW -- VEC = false at K = 3 and 259 --, the K = 1
    branch dW = colsum(dy * x), etch_colsum_fused for the bias).  act = "relu": small-integer x, W and bias, so every pre-activation is exact in
    every precision and many are exactly 0, where the mask (y > 0) must pass no gradient, as torch's relu does."""
    import torch.nn.functional as F
    from etch_amd import autograd as A
    R, O = 777, 64
    rng = np.random.default_rng(K + (act is not None))
    if act == "relu":
        x, bias = rng.integers(-2, 3, (R, K)).astype(np.float32), rng.integers(-1, 2, (O,)).astype(np.float32)
        W = (rng.integers(1, 3, (O, K)) * rng.choice([-1, 1], (O, K))).astype(np.float32)        # 2 |w| > |bias|: no output channel is dead at K = 1
        assert ((x.astype(np.float64) @ W.T.astype(np.float64) + bias) == 0).mean() > 0.005
    else:
        x, W, bias = (rng.standard_normal(s).astype(np.float32) for s in ((R, K), (O, K), (O,)))
    fn = (lambda x, W, bias: F.relu(F.linear(x, W, bias))) if act == "relu" else (lambda x, W, bias: F.linear(x, W, bias))
    r64, r32, G = B.oracle_autograd(fn, dict(x=x, W=W, bias=bias), g_seed=K)
    xg, Wg, bg = dev(x, True), dev(W, True), dev(bias, True)
    y = A.linear(xg, Wg, bg, act=act)
    (y * dev(G)).sum().backward()
    tag = f"linear K={K} act={act}"
    B.check(f"{tag} y", B.host(y), r64.y, r32.y)
    B.check(f"{tag} dx", B.host(xg.grad), r64.grads["x"], r32.grads["x"])
    B.check_weight(f"{tag} dW", B.host(Wg.grad), r64.grads["W"], r32.grads["W"])
    B.check_bias(f"{tag} dbias", B.host(bg.grad), r64.grads["bias"], r32.grads["bias"])
