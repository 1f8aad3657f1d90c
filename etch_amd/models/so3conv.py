"""MI355X counterpart of /root/reference/src/models/so3conv.py (same classes, same state-dict keys)."""
import os

import torch
import torch.nn as nn

from .. import ops
from .._shared import Shared, constant_value
from .. import vgtk_so3conv as sptk


def input_xyz(x):
    """(b, n, 3) -> (b, 3, n) contiguous; one tensor per input inside a pointops.knn_scope (the index prefetch and the
    encoder must see the same object: memo keys are tensor addresses)."""
    from . import pointops
    return pointops._memo(("epn_xyz", x.data_ptr(), tuple(x.shape)), (x,), lambda: x.permute(0, 2, 1).contiguous())


_ones_cache = Shared(limit=8)


def _occupancy_ones(b, n, na, device):
    """The all-ones occupancy features (functional.py:70-89) are a constant of the input shape: one shared tensor per shape instead of a 38 MB fill
    per forward (0.9 ms at 32 x 5 000 points).  Registered as filled with 1.0: while constant_value() says so, consumers use the value instead of the
    tensor (ops.inter_so3conv, SeparableSO3ConvBlock's one-channel skip branch); a caller's edit ends that and the next call here builds a fresh one."""
    def make():
        t = torch.ones((b, n, na, 1), dtype=torch.float32, device=device)
        torch.cuda.current_stream(device).synchronize() if device.type == "cuda" else None     # first use only: visible to every stream from here on
        return t
    return _ones_cache.get((b, n, na, device.type, device.index), make, fill=1.0)


def preprocess_input(x, na, add_center=True):
    """so3conv.py:7-16 for xyz-only input and add_center=False (the only mode ETCH uses, so3net.py:27):
    occupancy features = ones [b, 1, n, na] (functional.py:70-89)."""
    assert x.shape[2] == 3 and not add_center
    b, n, _ = x.shape
    xyz = input_xyz(x)
    feats_cl = _occupancy_ones(b, n, na, x.device)
    return sptk.SphericalPointCloud(xyz, None, None, feats_cl=feats_cl)


def _norm_act(x_cl):
    m, r = ops.instnorm_stats(x_cl)
    return ops.instnorm_act_add(x_cl, m, r)


class IntraSO3ConvBlock(nn.Module):
    """so3conv.py:19-44."""

    def __init__(self, dim_in, dim_out, norm=None, activation="relu", dropout_rate=0):
        super().__init__()
        assert activation == "leaky_relu" and dropout_rate == 0
        self.conv = sptk.IntraSO3Conv(dim_in, dim_out)
        self.norm = nn.InstanceNorm2d(dim_out, affine=False)

    def forward(self, x):
        y = self.conv(x)
        return sptk.SphericalPointCloud(y.xyz, None, y.anchors, feats_cl=_norm_act(y.feats_cl))


class InterSO3ConvBlock(nn.Module):
    """so3conv.py:47-104."""

    def __init__(self, dim_in, dim_out, kernel_size, stride, radius, sigma, n_neighbor, multiplier, kanchor=60, lazy_sample=None,
                 norm=None, activation="relu", pooling="none", dropout_rate=0):
        super().__init__()
        assert activation == "leaky_relu" and dropout_rate == 0
        if lazy_sample is None:
            lazy_sample = True
        pooling_method = None if pooling in ("none", None) else pooling
        self.conv = sptk.InterSO3Conv(dim_in, dim_out, kernel_size, stride, radius, sigma, n_neighbor, kanchor=kanchor,
                                      lazy_sample=lazy_sample, pooling=pooling_method)
        self.norm = nn.InstanceNorm2d(dim_out, affine=False)

    def forward(self, x, inter_idx=None, inter_w=None):
        inter_idx, inter_w, sample_idx, y = self.conv(x, inter_idx, inter_w)
        m, r = getattr(y, "in_stats", None) or ops.instnorm_stats(y.feats_cl)
        return inter_idx, inter_w, sample_idx, sptk.SphericalPointCloud(y.xyz, None, y.anchors, feats_cl=ops.instnorm_act_add(y.feats_cl, m, r))


class SeparableSO3ConvBlock(nn.Module):
    """so3conv.py:145-183: inter conv -> IN -> lrelu -> intra conv -> IN -> lrelu, + skip (1x1 conv, IN, lrelu).

    Fused schedule: the inter output is normalised on load inside the intra kernel; the two final
    normalisations + activation + residual add are one elementwise kernel."""

    def __init__(self, params):
        super().__init__()
        dim_in, dim_out = params["dim_in"], params["dim_out"]
        self.use_intra = params["kanchor"] > 1
        assert self.use_intra
        self.inter_conv = InterSO3ConvBlock(**params)
        self.intra_conv = IntraSO3ConvBlock(dim_out, dim_out, dropout_rate=params["dropout_rate"], activation=params["activation"])
        self.stride = params["stride"]
        self.skip_conv = nn.Conv2d(dim_in, dim_out, 1)
        self.norm = nn.InstanceNorm2d(dim_out, affine=False)
        self.emit_planes = False

    # ETCH_SKIP_STREAM=1 (A/B switch): the skip branch (a bandwidth-bound 1x1 conv + its statistics pass, independent of the inter / intra convs until
    # the final add) on a side stream next to the latency-bound inter conv.  The side stream waits for an event recorded on the current stream before
    # the inter conv is enqueued and the current stream waits for the branch before the final pass, so every buffer either stream frees is reused in
    # stream order behind those waits (no record_stream needed).
    skip_on_side_stream = os.environ.get("ETCH_SKIP_STREAM", "0") == "1"
    _side = None

    fold_k1_skip = os.environ.get("ETCH_SKIP_K1_FOLD", "1") != "0"     # one input channel: the skip conv + its InstanceNorm as a slope / offset of the final pass

    skip_stats_fused = os.environ.get("ETCH_SKIP_STATS_FUSED", "1") != "0"   # the skip conv returns its InstanceNorm statistics (0: conv, then the statistics pass)
    anchor_mean_fused = os.environ.get("ETCH_ANCHOR_MEAN_FUSED", "1") != "0"  # emit_anchor_mean blocks: the final pass also writes the anchor mean (0: etch_token_mean later)
    emit_anchor_mean = False      # set by EquivBackbone on the block whose output feeds the heads

    def _skip_branch(self, fin, sample_idx, p2):
        b, p1, na, cin = fin.shape
        w = self.skip_conv.weight.detach().view(self.skip_conv.out_channels, cin)
        bias = self.skip_conv.bias.detach()
        if cin == 1 and self.fold_k1_skip and fin.is_cuda and self.emit_planes in (False, None, "f16"):
            # s = w_c f + bias_c is affine in the ONE input value of a row: its InstanceNorm statistics follow from mean / variance of f over the scan's
            # (sampled) rows -- mean_c = w_c mean(f) + bias_c, var_c = w_c^2 var(f) -- and the normalised branch is f slope_c + offset_c.  The (rows, C)
            # conv output, its statistics pass and its read by the final pass (0.31 + 0.18 ms, 0.6 GB at 32 x 5 000 points) are never made.
            if constant_value(fin) is not None:
                # constant features (the occupancy ones of so3conv.py:7-16): s is constant per channel, its InstanceNorm is 0 -- the branch adds nothing
                return ("zero",)
            f = fin.reshape(b, p1, na)
            if self.stride > 1:
                f = torch.gather(f, 1, sample_idx.long().unsqueeze(-1).expand(-1, -1, na))
            f = f.reshape(b, p2 * na)
            var, mean = torch.var_mean(f.double(), dim=1, unbiased=False, keepdim=True)           # fp64, like the statistics kernels' sums
            w64, b64 = w.double().view(1, -1), bias.double().view(1, -1)
            rstd = torch.rsqrt(w64 * w64 * var + 1e-5)
            slope = (w64 * rstd).float()
            offset = ((b64 - (w64 * mean + b64)) * rstd).float()
            return ("k1", f, slope, offset)
        if self.skip_stats_fused and fin.is_cuda and ops.linear_stats_supported(fin, w, self.stride > 1):
            # the conv's epilogue holds every value it writes: the statistics come with the product (no pass that reads s back); the product itself keeps
            # the bits of ops.linear (the strided block stays on the fp32 MFMA tile kernel)
            if self.stride > 1:
                s, m3, r3 = ops.linear_stats(fin.view(-1, cin), w, bias, b, p2 * na, row_idx=sample_idx.contiguous(), grp=na, p_in=p1, p_out=p2)
            else:
                s, m3, r3 = ops.linear_stats(fin.view(-1, cin), w, bias, b, p2 * na)
            return s.view(b, p2, na, -1), m3, r3
        if self.stride > 1:
            s = ops.linear(fin.view(-1, cin), w, bias=bias, row_idx=sample_idx.contiguous(), grp=na, p_in=p1, p_out=p2, rows=b * p2 * na)
        else:
            s = ops.linear(fin.view(-1, cin), w, bias=bias)
        s = s.view(b, p2, na, -1)
        m3, r3 = ops.instnorm_stats(s)
        return s, m3, r3

    def forward(self, x, inter_idx, inter_w):
        conv = self.inter_conv.conv
        fin = x.feats_cl
        branch = None
        if self.skip_on_side_stream and fin.is_cuda and not torch.is_grad_enabled():
            # one side stream PER main stream (with stage1_streams = 2 a single shared side stream would order the two main streams' skip
            # branches against each other's buffers, and "no record_stream needed" would no longer hold across them)
            main = torch.cuda.current_stream()
            if SeparableSO3ConvBlock._side is None:
                SeparableSO3ConvBlock._side = {}
            side = SeparableSO3ConvBlock._side.get(main.cuda_stream)
            if side is None:
                from ..utils.cu_streams import make_stream
                side = SeparableSO3ConvBlock._side[main.cuda_stream] = make_stream("side")
            _, sidx0, nx = conv.group(x.xyz)                # memoised: the conv below finds the same tensors
            ev0 = torch.cuda.Event()
            ev0.record(main)
            side.wait_event(ev0)
            with torch.cuda.stream(side):
                branch = self._skip_branch(fin, sidx0, nx.shape[-1])
                ev1 = torch.cuda.Event()
                ev1.record(side)
        inter_idx, _, sample_idx, y = conv(x, inter_idx, inter_w)
        m1, r1 = getattr(y, "in_stats", None) or ops.instnorm_stats(y.feats_cl)     # from the conv's epilogue
        z = self.intra_conv.conv(y, m1, r1, want_stats=True)     # IN + lrelu of the inter output applied on load; statistics of z in the epilogue
        m2, r2 = z.in_stats
        # skip branch: 1x1 conv on (optionally sub-sampled) input rows
        b, p1, na, cin = fin.shape
        p2 = y.feats_cl.shape[1]
        if branch is None:
            branch = self._skip_branch(fin, sample_idx, p2)
        else:
            torch.cuda.current_stream().wait_event(ev1)
        if isinstance(branch[0], str):                      # ("k1", f, slope, offset): the folded one-channel branch; ("zero",): constant features
            amean = None
            if branch[0] == "zero" and self._wants_anchor_mean(z.feats_cl):
                res, amean = ops.instnorm_act_add_mean(z.feats_cl, m2, r2)
            elif branch[0] == "zero":
                res = ops.instnorm_act_add(z.feats_cl, m2, r2, want_planes=self.emit_planes)
            else:
                _, f, slope, offset = branch
                res = ops.instnorm_act_add_k1(z.feats_cl, m2, r2, f, slope, offset, want_planes=self.emit_planes)
            out, planes = res if self.emit_planes else (res, None)
            cloud = sptk.SphericalPointCloud(y.xyz, None, z.anchors, feats_cl=out)
            if planes is not None:
                cloud.feats_planes = planes
            if amean is not None:
                cloud.anchor_mean = amean
            return inter_idx, None, sample_idx, cloud
        s, m3, r3 = branch
        # emit_planes (set by EquivBackbone when the NEXT conv gathers planes: "f16", their format -- InterSO3Conv.wants_planes): the output is also written split, once, by this pass
        planes, amean = None, None
        if self.emit_planes:
            out, planes = ops.instnorm_act_add(z.feats_cl, m2, r2, s, m3, r3, want_planes=self.emit_planes)
        elif self._wants_anchor_mean(z.feats_cl):
            out, amean = ops.instnorm_act_add_mean(z.feats_cl, m2, r2, s, m3, r3)
        else:
            out = ops.instnorm_act_add(z.feats_cl, m2, r2, s, m3, r3)
        # x.anchors after the intra conv = the INTRA conv's anchors buffer (vgtk modules.py:153; so3conv.py:182 passes it on)
        cloud = sptk.SphericalPointCloud(y.xyz, None, z.anchors, feats_cl=out)
        if planes is not None:
            cloud.feats_planes = planes
        if amean is not None:
            cloud.anchor_mean = amean         # (b * p, C): the mean over the anchors of feats_cl, read by GT_network_equiv._forward
        return inter_idx, None, sample_idx, cloud

    def _wants_anchor_mean(self, x):
        return (self.emit_anchor_mean and self.anchor_mean_fused and x.is_cuda and not self.emit_planes
                and x.shape[2] == 60 and x.shape[-1] in ops.ANCHOR_MEAN_WIDTHS)


class BasicSO3ConvBlock(nn.Module):
    """so3conv.py:107-142."""

    def __init__(self, params):
        super().__init__()
        self.blocks = nn.ModuleList()
        self.layer_types = []
        for param in params:
            if param["type"] == "intra_block":
                conv = IntraSO3ConvBlock(**param["args"])
            elif param["type"] == "inter_block":
                conv = InterSO3ConvBlock(**param["args"])
            elif param["type"] == "separable_block":
                conv = SeparableSO3ConvBlock(param["args"])
            else:
                raise ValueError(f'No such type of SO3Conv {param["type"]}')
            self.layer_types.append(param["type"])
            self.blocks.append(conv)
        self.params = params

    def forward(self, x):
        inter_idx, inter_w = None, None
        sample_idx_list = []
        for conv, param in zip(self.blocks, self.params):
            if param["type"] in ("inter", "inter_block", "separable_block"):
                inter_idx, inter_w, sample_idx, x = conv(x, inter_idx, inter_w)
                # the reference keeps (inter_idx, inter_w) for the next stride-1 conv but never hits that
                # path in the ETCH configuration; indices are recomputed per conv exactly as it does there
                inter_idx, inter_w = None, None
            elif param["type"] == "intra_block":
                x = conv(x)
                sample_idx = None
            else:
                raise ValueError(f'No such type of SO3Conv {param["type"]}')
            sample_idx_list.append(sample_idx)
        return x, sample_idx_list


def so3_mean(Rs, weights=None):
    """so3conv.py:186-225: chordal-L2 mean of the rotations Rs (B,N,3,3) with optional weights (B,N) -> (B,3,3).  One thread per
    row: fp64 accumulation of Ce = sum_n w_n R_n, one-sided Jacobi SVD, det(U V^T) fix (csrc/heads.hip).  An expanded view of one
    shared rotation set (the way the model calls it, models_pointcloud.py:118-119) is read once instead of B times."""
    from .. import _lib
    B, N = Rs.shape[0], Rs.shape[1]
    shared = Rs.stride(0) == 0
    rs = (Rs[0] if shared else Rs).contiguous().float()
    w = None if weights is None else weights.contiguous().float()
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=Rs.device)
    _lib.call("etch_so3_mean", B, N, rs, 0 if shared else N * 9, w, R)
    return R
