"""The fp64 yardstick of tests/test_gpu_backward_fp64.py and tests/test_backward_pins_host.py: the oracle's forms under autograd in fp64
and in fp32, the tensor layouts the per-channel rule of tests/_pt_fp64.py is applied in, and the derived bound of the kernels that sum
exact products in fp64.  TEST INFRASTRUCTURE ONLY (no GPU needed to import or run).

Reference = one function of oracle/stage1.py run under torch.autograd with torch's default dtype set to float64, from seeded fp32 values
widened exactly; the SAME function from the SAME values in fp32 on the CPU is the reference's own rounding error e_32.  Rule
(tests/_pt_fp64.py `check`, FACTOR = 2, SLACK = 1e-6), per channel and for both statistics:  max_ch e_gpu <= 2 max_ch e_32 + 1e-6.
Layouts (a column of the 2-d view is a channel):
    outputs, feature / data gradients   channels-last (..., C): `channels_last` brings the oracle's (b, C, p, a) tensors there
    weight gradients (O, K)             twice: per output channel (the transposed matrix) and per input column (`check_weight`)
    bias gradients                      one column
No element is left out; `check` asserts that fewer than 1 channel in 16 sits on the 1e-3 scale floor.
"""
import numpy as np
import torch

from oracle import stage1 as S1
from tests._pt_fp64 import FACTOR, SLACK, channel_errors, check, in_dtype  # noqa: F401  (re-exported: the rule lives in one place)


# --------------------------------------------------------------------------------------------- one oracle function under autograd
class Run:
    """One autograd run: y (numpy), grads {name: numpy} of sum(y * G) with respect to the differentiable inputs."""

    def __init__(self, y, grads):
        self.y, self.grads = y, grads


def oracle_autograd(fn, diff, const=None, G=None, g_seed=0):
    """fn(**tensors) -> y, an oracle/stage1.py form.  diff: {name: fp32 values} the gradients are taken for; const: {name: values} passed
    along (floating point ones in the run's dtype, integers as they are); G: the upstream gradient in fp32 (default: standard normal from
    `g_seed`, of y's shape).  -> (Run in fp64 as float64 arrays, Run in fp32 as float32 arrays, G as a float32 array): both runs start
    from the same fp32 values and the same G, so their difference is the fp32 rounding of the oracle's own arithmetic."""
    const = const or {}
    box = {"G": None if G is None else np.asarray(G, np.float32)}

    def run(cast):
        t = {k: cast(v).clone().requires_grad_() for k, v in diff.items()}
        c = {k: cast(v) for k, v in const.items()}
        with torch.enable_grad():
            y = fn(**t, **c)
            if box["G"] is None:
                box["G"] = torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(g_seed), dtype=torch.float32).numpy()
            (y * cast(box["G"])).sum().backward()
        return y.detach(), {k: v.grad.detach() for k, v in t.items()}

    out = []
    for dtype, npd in ((torch.float64, np.float64), (torch.float32, np.float32)):
        y, grads = in_dtype(dtype, run)
        assert y.dtype == dtype and all(g.dtype == dtype for g in grads.values())
        out.append(Run(y.numpy().astype(npd), {k: g.numpy().astype(npd) for k, g in grads.items()}))
    return out[0], out[1], box["G"]


def channels_last(a):
    """(b, C, ...) -> (b, ..., C)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), 1, -1))


def host(t):
    return t.detach().cpu().numpy()


def check_weight(tag, got, ref64, ref32):
    """A weight gradient (O, K) under the rule per output channel (rows) and per input column."""
    got, ref64, ref32 = (np.asarray(a).reshape(np.asarray(ref64).shape[0], -1) for a in (got, ref64, ref32))
    check(tag + " per output channel", got.T, ref64.T, ref32.T)
    if got.shape[1] > 1:
        check(tag + " per input column", got, ref64, ref32)


def check_bias(tag, got, ref64, ref32):
    check(tag, np.asarray(got).reshape(-1), np.asarray(ref64).reshape(-1), np.asarray(ref32).reshape(-1))


# --------------------------------------------------------------------------------------------- the oracle forms the tests differentiate
def encoder_channel_pairs():
    """(cin, cout, nn, stride, lazy_sample) of every inter conv that EPN_layer_num 1 .. 4 builds, from layer_geometry (the deepest encoder
    contains the shallower ones' convs)."""
    from etch_amd.models.so3net import layer_geometry
    pairs = []
    for depth in (1, 2, 3, 4):
        for block in layer_geometry([[32, 32], [64, 64], [128, 128], [256, 256]][:depth], [2, 2, 2, 2][:depth], 0.4):
            for g in block:
                pair = (g["dim_in"], g["dim_out"], g["n_neighbor"], g["stride"], bool(g["lazy_sample"]))
                if pair not in pairs:
                    pairs.append(pair)
    return pairs


def inter_problem(cin, cout, nn, stride, lazy, b=2, n=96, radius=0.2, sigma=0.02, p2=None, seed=30):
    """Geometry and seeded values of one inter conv on `b` scans of `n` points: the oracle's grouping (ball query with pads that repeat a
    neighbour), optionally only the first p2 target points (a target's output depends on its own ball only)."""
    import etch_amd.vgtk_so3conv as V
    from etch_amd.utils.weights import load_seeded
    from tests.test_gpu_backward import scan
    xyz =torch.from_numpy(np.stack([scan(seed + i, n).T.copy() for i in range(b)]))
    conv = load_seeded(V.InterSO3Conv(cin, cout, 1, stride, radius, sigma, nn, lazy_sample=lazy), 4).eval()
    g, ball, _, new_xyz = S1.inter_grouping(xyz, stride, radius, nn, lazy)
    if p2 is not None:
        g, ball, new_xyz = g[:, :, :p2].contiguous(), ball[:, :p2].contiguous(), new_xyz[:, :, :p2].contiguous()
    rng = np.random.default_rng(cin + cout)
    feats = np.ones((b, 1, n, 60), np.float32) if cin == 1 else rng.standard_normal((b, cin, n, 60)).astype(np.float32)
    return dict(cin=cin, cout=cout, nn=nn, b=b, n=n, sigma=sigma, xyz=xyz, new_xyz=new_xyz, ball=ball, g=g, conv=conv, feats=feats,
                W=conv.basic_conv.W.detach().numpy().copy(), bias=conv.basic_conv.bias.detach().numpy().copy(),
                anchors=conv.anchors.numpy().copy(), kernels=conv.kernels.numpy().copy())


def inter_oracle(pr, ball=None):
    """fp64 / fp32 autograd through inter_weights -> inter_feat_grouping -> basic_so3conv (functional.py:286-324, :61-67, modules.py:33-39)
    for the problem `pr`; the all-ones occupancy features of cin = 1 receive no gradient.  `ball`: another index list (shadow index n = no
    contribution) in place of the problem's."""
    sigma, ball = pr["sigma"], pr["ball"] if ball is None else ball

    def fn(W, bias, g, anchors, kernels, feats):
        w = S1.inter_weights(g, anchors, kernels, sigma)
        pad = torch.zeros(feats.shape[0], feats.shape[1], 1, feats.shape[3])
        return S1.basic_so3conv(W, bias, S1.inter_feat_grouping(ball, w, torch.cat((feats, pad), 2)))

    diff = dict(W=pr["W"], bias=pr["bias"])
    const = dict(g=pr["g"], anchors=pr["anchors"], kernels=pr["kernels"])
    (diff if pr["cin"] > 1 else const)["feats"] = pr["feats"]
    return oracle_autograd(fn, diff, const, g_seed=pr["cin"] + 7 * pr["cout"])


def intra_oracle(x, W, bias, intra_idx):
    """fp64 / fp32 autograd through the intra gather (functional.py:343-344) -> basic_so3conv; x (b, C, p, 60)."""
    ii = torch.as_tensor(intra_idx).long().view(-1)

    def fn(x, W, bias):
        b, C, p, na = x.shape
        gf = x.index_select(3, ii).view(b, C, p, na, -1).permute(0, 1, 4, 2, 3).contiguous()
        return S1.basic_so3conv(W, bias, gf)

    return oracle_autograd(fn, dict(x=x, W=W, bias=bias), g_seed=x.shape[1] + x.shape[2])


def instnorm_oracle(x):
    """fp64 / fp32 autograd through leaky_relu(InstanceNorm2d(x), 0.01) (so3conv.py:36-44); x (b, C, p, 60)."""
    return oracle_autograd(lambda x: S1._inorm_lrelu(x), dict(x=x), g_seed=x.shape[1] + x.shape[2])


MHSA_KEYS = ("query_transform.weight", "key_transform.weight", "value_transform.weight", "head_combine.weight", "head_combine.bias")


def mhsa_inputs(T, E, seed, q_scale=1.0):
    """x (T, 60, E), wq, wk, wv, wc (E, E), bc (E): logits of spread ~2.5 whatever E (the seeded model's are smaller); q_scale > 1 sharpens
    the softmax."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 60, E, generator=g)
    W = [torch.randn(E, E, generator=g) * (1.6 / E ** 0.5) for _ in range(4)]
    W[0] = W[0] * q_scale
    bc = torch.randn(E, generator=g) * 0.1
    return [x.numpy()] + [w.numpy() for w in W] + [bc.numpy()]


def mhsa_oracle(x, wq, wk, wv, wc=None, bc=None, residual=False, g_seed=0):
    """fp64 / fp32 autograd through oracle mhsa_layer (direction_backbones.py:132-194) (+ x: the residual of :216-221).  wc = None: the
    concatenated head outputs -- the same function with the identity as head_combine and a zero bias (products with 1 and sums with 0 are
    exact), neither of them differentiated."""
    heads_only = wc is None
    E = x.shape[-1]

    def fn(x, wq, wk, wv, wc, bc):
        y = S1.mhsa_layer(dict(zip(("l." + k for k in MHSA_KEYS), (wq, wk, wv, wc, bc))), "l.", x)
        return y + x if residual else y

    diff = dict(x=x, wq=wq, wk=wk, wv=wv)
    if heads_only:
        return oracle_autograd(fn, diff, dict(wc=np.eye(E, dtype=np.float32), bc=np.zeros(E, np.float32)), g_seed=g_seed)
    return oracle_autograd(fn, dict(diff, wc=wc, bc=bc), g_seed=g_seed)


def max_softmax_probability(x, wq, wk, heads=8):
    """Per (head, token, query) the largest attention probability, in fp64."""
    x, wq, wk = (torch.from_numpy(np.asarray(a)).double() for a in (x, wq, wk))
    T, L, E = x.shape
    hs = E // heads
    split = lambda o: o.view(T, L, heads, hs).permute(2, 0, 1, 3)
    q, k = split(x @ wq.t()), split(x @ wk.t())
    return torch.softmax(q @ k.transpose(-1, -2) / hs ** 0.5, -1).amax(-1).numpy()


# --------------------------------------------------------------------------------------------- exact products, fp64 sum, one rounding
def check_exact_accumulation(tag, got, a, b, c_old=None):
    """got (M, N) fp32 = A^T B (+ c_old) from a kernel that widens its fp32 operands exactly, forms exact products (48 < 53 bits), keeps an
    fp64 running sum and rounds once to fp32.  Derived, not measured, per element:
        |got - ref64| <= 2^-24 |ref64| + (T + 2) 2^-53 sum_t |a_t| |b_t|,   T = R terms (+ 1: the old C when accumulating)
    (2^-24: the one rounding to nearest fp32; T - 1 roundings of the running sum, each within 2^-53 of a partial sum that the sum of the
    magnitudes bounds, whatever the order -- row ranges summed one after the other included; the rest covers the fp64 reference's own sum)."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    got = np.asarray(got)
    assert got.dtype == np.float32
    ref, mag, terms = a64.T @ b64, np.abs(a64).T @ np.abs(b64), a64.shape[0]
    if c_old is not None:
        c64 = np.asarray(c_old, np.float64).reshape(ref.shape)
        ref, mag, terms = ref + c64, mag + np.abs(c64), terms + 1
    err = np.abs(got.astype(np.float64).reshape(ref.shape) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + (terms + 2) * 2.0 ** -53 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"PIN {tag}: exact accumulation, max |err| / bound {worst:.3f}; max |err| {float(err.max()) if err.size else 0.0:.2e}")
    assert np.isfinite(got).all() and (err <= bound).all(), f"{tag}: {int((err > bound).sum())} of {err.size} elements over the derived bound"
