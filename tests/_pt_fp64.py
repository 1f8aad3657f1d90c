"""The fp64 yardstick of tests/test_gpu_pt_fp64.py: per-channel error statistics, the entitled-error rule and the fp64 restatements
of the inference ops the oracle does not have as separate functions.  TEST INFRASTRUCTURE ONLY (no GPU needed to import or run).

Reference = the plain torch form of oracle/stage1.py (pt_layer / pt_block / pt_down / pt_up, cited there against the reference's
source lines) run under torch.set_default_dtype(float64) with the seeded weights cast to fp64; the SAME function run in fp32 on
the CPU is the reference's own rounding error.  Statistics, per output channel (column) -- never the global maximum:

    relL2_ch  = |got[:,ch] - ref64[:,ch]|_2 / max(|ref64[:,ch]|_2, 1e-3 max_ch |ref64[:,ch]|_2)
    relmax_ch = max_i |got - ref64|[i,ch]   / max(max_i |ref64[i,ch]|, 1e-3 max_ch max_i |ref64[i,ch]|)

The 1e-3 floor guards against dead ReLU channels; it is not a tolerance, and `check` asserts that fewer than 1 channel in 16 sits
on it.  Rule (tests/_parity.py check_stage1_vs_fixture, test_gpu_train.py entitled error): with e_gpu the GPU result against fp64
and e_32 the reference's fp32 run against fp64,  max_ch e_gpu <= 2 max_ch e_32 + 1e-6  for both statistics (the factor 2 is "a
different summation order").  No row, channel or element is left out of a comparison.
"""
import numpy as np
import torch
import torch.nn.functional as F

from etch_amd.utils.weights import seeded_state_dict
from oracle import stage1 as S1

FLOOR = 1e-3
FACTOR, SLACK = 2.0, 1e-6


def _columns(a):
    a = np.asarray(a, np.float64)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, 1)


def channel_errors(got, ref64):
    """-> (max_ch relL2_ch, max_ch relmax_ch, channels on the scale floor, channels)."""
    g, r = _columns(got), _columns(ref64)
    assert g.shape == r.shape, (g.shape, r.shape)
    assert np.isfinite(g).all() and np.isfinite(r).all()
    amax, l2 = np.abs(r).max(0), np.linalg.norm(r, axis=0)
    assert amax.max() > 0
    floor_max, floor_l2 = FLOOR * amax.max(), FLOOR * l2.max()
    d = g - r
    rel_l2 = np.linalg.norm(d, axis=0) / np.maximum(l2, floor_l2)
    rel_max = np.abs(d).max(0) / np.maximum(amax, floor_max)
    on_floor = int(((amax < floor_max) | (l2 < floor_l2)).sum())
    return float(rel_l2.max()), float(rel_max.max()), on_floor, r.shape[1]


def check(tag, got, ref64, ref32):
    """Print (e_gpu, e_32) of both statistics and assert the rule.  got: the GPU result; ref64 / ref32: the reference in fp64 / fp32."""
    gl2, gmax, on_floor, c = channel_errors(got, ref64)
    rl2, rmax, _, _ = channel_errors(ref32, ref64)
    print(f"PIN {tag}: relL2 gpu {gl2:.2e} / fp32 {rl2:.2e}; relmax gpu {gmax:.2e} / fp32 {rmax:.2e}; floor {on_floor}/{c}")
    assert 16 * on_floor < c, f"{tag}: {on_floor} of {c} channels on the scale floor: the per-channel statistic would be vacuous"
    assert gl2 <= FACTOR * rl2 + SLACK, f"{tag}: per-channel relL2 {gl2:.3e} > 2 x {rl2:.3e} + 1e-6"
    assert gmax <= FACTOR * rmax + SLACK, f"{tag}: per-channel relmax {gmax:.3e} > 2 x {rmax:.3e} + 1e-6"


def check_exact(tag, got, want):
    """Copy / gather / max kernels: bit-for-bit the fp32 restatement."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    same = np.array_equal(got, want)
    print(f"PIN {tag}: exact {'equal' if same else 'DIFFERENT'}")
    assert same, tag


def in_dtype(dtype, fn):
    """fn(cast) under torch's default dtype `dtype`; cast(a) -> CPU tensor (floating point: `dtype`; integers unchanged)."""
    def cast(a):
        t = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(dtype) if t.is_floating_point() else t

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            return fn(cast)
    finally:
        torch.set_default_dtype(old)


def _np(out, dtype):
    if isinstance(out, (tuple, list)):
        return tuple(_np(t, dtype) for t in out)
    return out.numpy().astype(dtype) if out.is_floating_point() else out.numpy()


def both(fn):
    """(fn in fp64 as float64 arrays, fn in fp32 as float32 arrays); tuples are mapped element-wise, integer results stay as they are."""
    return _np(in_dtype(torch.float64, fn), np.float64), _np(in_dtype(torch.float32, fn), np.float32)


def state(module, seed, cast):
    """seeded_state_dict(module, seed) in the dtype of `cast`."""
    return {k: cast(v) for k, v in seeded_state_dict(module, seed).items()}


def cloud(segments, c, seed, scale=0.3):
    """Coordinates without exact ties (randn * 0.3, fp32), features randn, cumulative int32 offsets."""
    g = torch.Generator().manual_seed(seed)
    n = int(sum(segments))
    p = (torch.randn(n, 3, generator=g) * scale).numpy()
    x = torch.randn(n, c, generator=g).numpy()
    return p, x, np.cumsum(segments).astype(np.int32)


def bn_relu(y, scale, shift):
    """relu(y * scale + shift) in y's own precision (numpy): the folded eval-mode BatchNorm + ReLU of pointtransformer_seg.py:115."""
    return np.maximum(y * scale.astype(y.dtype) + shift.astype(y.dtype), 0)


# --------------------------------------------------------------------------------------------- the heads after the U-Net
def confidence_head(sd, pre, x1, k, chunk=1024):
    """oracle/stage1.py pt_confidence after pt_unet (pointtransformer_seg.py:163-195, the part after the U-Net): x1 (R, 128) -> logits (R, k), confidence (R, 1).
    Rows are independent; they are taken `chunk` at a time only to bound the (128 k, R) hidden layer of `confi`."""
    logits, conf = [], []
    for s in range(0, x1.shape[0], chunk):
        xt = x1[s:s + chunk].t().unsqueeze(0).contiguous()                                       # (1, 128, r)
        h = F.relu(S1._bn(sd, pre + "cls.1.", F.conv1d(xt, sd[pre + "cls.0.weight"], sd[pre + "cls.0.bias"])))
        lg = F.conv1d(h, sd[pre + "cls.3.weight"], sd[pre + "cls.3.bias"])
        sm = F.softmax(lg, dim=1)
        c = F.relu(F.conv1d(xt, sd[pre + "confi.0.weight"], sd[pre + "confi.0.bias"]))
        c = F.conv1d(c, sd[pre + "confi.2.weight"], sd[pre + "confi.2.bias"], groups=k)
        logits.append(lg[0].t())
        conf.append((c.view(1, 1, k, -1) * sm.unsqueeze(1)).sum(dim=2)[0].t())
    return torch.cat(logits).contiguous(), torch.cat(conf).contiguous()


def magnitude_head(sd, pre, x1):
    """oracle/stage1.py pt_magnitude after pt_unet (pointtransformer_seg.py:237-260, the part after the U-Net): x1 (R, 64) -> (R, 1)."""
    h = F.relu(S1._bn(sd, pre + "final_layer.1.", F.linear(x1, sd[pre + "final_layer.0.weight"], sd[pre + "final_layer.0.bias"])))
    return F.linear(h, sd[pre + "final_layer.3.weight"], sd[pre + "final_layer.3.bias"])


# --------------------------------------------------------------------------------------------- glue kernels (numpy, in the dtype given)
def group_rows(p, new_p, x, idx, ld):
    """pointops.py:90-98 queryandgroup(use_xyz=True): rows [(i, j)] = [p[idx] - new_p[i] | x[idx] | 0 ...] (fp32 in, fp32 out: exact)."""
    m, ns = idx.shape
    out = np.zeros((m * ns, ld), p.dtype)
    flat = idx.reshape(-1)
    out[:, :3] = p[flat] - np.repeat(new_p, ns, axis=0)
    out[:, 3:3 + x.shape[1]] = x[flat]
    return out


def rows_maxpool(x, ns):
    """pointtransformer_seg.py:63 MaxPool1d(nsample) over consecutive row groups."""
    return x.reshape(-1, ns, x.shape[1]).max(1)


def down_gather_max(ux, p, new_p, idx, wp, scale, shift, dtype):
    """pointtransformer_seg.py:61-63 with the Linear split as W [p_j - p_i | x_j] = Wp (p_j - p_i) + Wx x_j (ux = x Wx^T):
    out[i] = max_j relu(bn(ux[idx[i, j]] + Wp (p[idx[i, j]] - new_p[i])))."""
    t = lambda a: a.astype(dtype)
    rel = t(p)[idx] - t(new_p)[:, None, :]                                                     # (m, ns, 3)
    y = t(ux)[idx] + rel @ t(wp).T
    return np.maximum(y * t(scale) + t(shift), 0).max(1)


def interp_add(a, f, idx, dist, dtype):
    """pointops.py:164-178 + pointtransformer_seg.py:97: a + sum_k f[idx_k] w_k, w = (1 / (dist + 1e-8)) / sum, with the (fp32) distances given."""
    t = lambda v: v.astype(dtype)
    r = dtype(1.0) / (t(dist) + dtype(1e-8))
    w = r / r.sum(1, keepdims=True)
    return t(a) + (t(f)[idx] * w[:, :, None]).sum(1)


def seg_mean(x, offset, dtype):
    """pointtransformer_seg.py:86-88 as oracle/stage1.py pt_up writes it: per-segment x.sum(0, True) / count (torch, in `dtype`)."""
    o = [0] + [int(v) for v in offset]
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return torch.cat([xt[o[i]:o[i + 1]].sum(0, True) / (o[i + 1] - o[i]) for i in range(len(o) - 1)]).numpy()


def concat_bcast(x, g, offset):
    """pointtransformer_seg.py:89-91: [x | g[segment of the row]]."""
    o = [0] + [int(v) for v in offset]
    return np.concatenate([x, np.repeat(g, np.diff(o), axis=0)], 1)


def grouped_dot(h, w, bias, G, J, dtype):
    """pointtransformer_seg.py:145 Conv1d(G J, G, 1, groups=G): out[r, g] = h[r, g J:(g + 1) J] . w[g] + b[g]."""
    hh = torch.from_numpy(np.ascontiguousarray(h)).to(dtype).view(h.shape[0], G, J)
    return ((hh * torch.from_numpy(w).to(dtype).view(1, G, J)).sum(-1) + torch.from_numpy(bias).to(dtype)).numpy()


def softmax_dot(logits, v, dtype):
    """pointtransformer_seg.py:183-189: sum_g softmax(logits)_g v_g per row."""
    sm = F.softmax(torch.from_numpy(logits).to(dtype), dim=1)
    return (sm * torch.from_numpy(v).to(dtype)).sum(1).numpy()


def linear_forms(lin, bias, scale, shift, res):
    """The four epilogue forms of tests/test_gpu_encoder.py test_linear_epilogues on lin = x W^T, in lin's own precision (numpy)."""
    t = lambda a: a.astype(lin.dtype)
    slope = lin.dtype.type(0.01)
    return (lin,
            np.maximum((lin + t(bias)) * t(scale) + t(shift), 0),
            np.maximum(lin + t(bias) + t(res), 0),
            np.where(lin > 0, lin, slope * lin) + t(res))


def linear_refs(x, w):
    """x W^T in fp64 (numpy) and, as the reference's fp32 run, torch.nn.functional.linear on the CPU in fp32."""
    lin64 = x.astype(np.float64) @ w.astype(np.float64).T
    lin32 = F.linear(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(w))).numpy()
    return lin64, lin32
