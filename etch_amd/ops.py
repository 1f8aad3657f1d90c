"""Torch-tensor front-end of the C ABI (include/etch_hip.h).

PyTorch is plumbing only: it owns device memory and the current HIP stream.  Every function here
hands raw device pointers to libetch_hip.so; there is no eager/CPU fallback -- a CPU tensor or a
missing library raises.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._shared import Shared, constant_value


# For direct callers of the typed functions (`_lib.lib().etch_x(...)` in tests and profiles/scripts); the package itself goes through _lib.call.
_stream = _lib.stream


def _ptr(t):
    return t.data_ptr()


def _need(t, dtype, name):
    if not t.is_cuda:
        raise _lib.EtchHipError(f"{name} must be a CUDA(HIP) tensor: etch_amd has no CPU path")
    if t.dtype != dtype:
        raise _lib.EtchHipError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.EtchHipError(f"{name} must be contiguous")  # grouping_cuda.cpp:66-68 CHECK_INPUT
    return t


# ------------------------------------------------------------------ epn_grouping / epn_gathering
def ball_query(new_xyz, xyz, radius, nsample):
    """epn_grouping.ball_query (grouping_cuda.cpp:71-86): (b,3,m),(b,3,n) -> idx (b,m,nsample) int32."""
    _need(new_xyz, torch.float32, "new_xyz"), _need(xyz, torch.float32, "xyz")
    b, _, m = new_xyz.shape
    n = xyz.shape[2]
    idx = torch.empty((b, m, nsample), dtype=torch.int32, device=xyz.device)
    _lib.call("etch_ball_query", b, n, m, float(radius), int(nsample), new_xyz, xyz, idx)
    return idx


FPS_SPLIT_FORCE = None      # tests: an int G forces the split kernels (2..8) or disables them (0 / 1); None = fps_split_default


def fps_split_default(nseg, n_max, device=None):
    """Workgroups per scan for the FPS kernels.  Measured (profiles/r04_fps_split.txt): the per-round exchange between the workgroups of a
    split scan costs 0.75 us (one scan) to 1.2 us (32 - 64 scans in flight) on top of a fixed 0.8 us per round, against 1.1 us for the WHOLE
    one-workgroup round at 5 000 points and 2.3 us at 20 000 -- the split is slower at every size the path runs (2.7 us at 20 000 points with
    G = 4), so the default is one workgroup per scan.  The split kernels stay available (bit-identical picks): split=G, FPS_SPLIT_FORCE or
    ETCH_FPS_SPLIT=G; they need nseg * G co-resident workgroups (one per compute unit)."""
    if FPS_SPLIT_FORCE is not None:
        return int(FPS_SPLIT_FORCE) if int(FPS_SPLIT_FORCE) >= 2 else 1
    env = os.environ.get("ETCH_FPS_SPLIT")
    if env is not None and int(env) >= 2:
        cus = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device()).multi_processor_count
        g = min(8, int(env))
        while g >= 2 and (nseg * g > cus or n_max > 8192 * g):
            g = g // 2 if nseg * g > cus else 0
        return g if g >= 2 else 1
    return 1


def _fps_split_ws(nseg, G, device):
    ws = torch.empty((_lib.call("etch_fps_split_workspace_bytes", nseg, G),), dtype=torch.uint8, device=device)
    return ws


def fps_split_failed(idx):
    """True if the split FPS launch that produced `idx` gave up (a workgroup of a scan never arrived); synchronises the current stream."""
    ws = getattr(idx, "_etch_split_ws", None)
    if ws is None:
        return False
    out = ctypes.c_int(0)
    _lib.call("etch_fps_split_failed", ws, ctypes.byref(out))
    return bool(out.value)


def _fps_split_checked(idx, split):
    """A split launch that the DISPATCH chose (split=None: ETCH_FPS_SPLIT / FPS_SPLIT_FORCE -- the model path, whose callers gather with the result at
    once) is verified here: a scan that gave up carries INT_MIN indices, which must not reach a gather.  Costs a stream synchronisation
    on this opt-in path only; an explicit split=G leaves the check to the caller (fps_split_failed), as the failure-path test does."""
    if split is None and fps_split_failed(idx):
        raise _lib.EtchHipError("split FPS gave up (a workgroup of a scan never arrived): rerun with ETCH_FPS_SPLIT unset (one workgroup per scan)")
    return idx


def fps_pair(xyz_b3n, m, xyz_packed, offset, new_offset, new_offset_host):
    """The encoder's FPS (furthest_point_sampling(xyz_b3n, m)) and the Point-Transformer nets' first FPS level (furthestsampling(xyz_packed, offset,
    new_offset)) over the same b scans of n points each in ONE launch of 2 b workgroups (etch_fps_pair): both are one workgroup per scan and depend on the
    coordinates only.  -> (idx_a (b,m) int32, idx_b (sum m') int32), bit-identical to the separate calls."""
    _need(xyz_b3n, torch.float32, "xyz_b3n"), _need(xyz_packed, torch.float32, "xyz_packed")
    _need(offset, torch.int32, "offset"), _need(new_offset, torch.int32, "new_offset")
    b, _, n = xyz_b3n.shape
    assert xyz_packed.shape == (b * n, 3)
    idx_a = torch.zeros((b, m), dtype=torch.int32, device=xyz_b3n.device)
    idx_b = torch.zeros((int(new_offset_host[-1]),), dtype=torch.int32, device=xyz_b3n.device)
    _lib.call("etch_fps_pair", b, n, int(m), xyz_b3n, idx_a, xyz_packed, offset, new_offset, idx_b)
    return idx_a, idx_b


def furthest_point_sampling(xyz, m, split=None):
    """epn_grouping.furthest_point_sampling (grouping_cuda.cpp:158-173): (b,3,n) -> (b,m) int32.  split = workgroups per scan (None: auto)."""
    _need(xyz, torch.float32, "xyz")
    b, _, n = xyz.shape
    idx = torch.zeros((b, m), dtype=torch.int32, device=xyz.device)
    G = fps_split_default(b, n, xyz.device) if split is None else int(split)
    if G >= 2:
        ws = _fps_split_ws(b, G, xyz.device)
        _lib.call("etch_furthest_point_sampling_split", b, n, int(m), xyz, idx, G, ws)
        idx._etch_split_ws = ws
        return _fps_split_checked(idx, split)
    _lib.call("etch_furthest_point_sampling", b, n, int(m), xyz, idx)
    return idx


def gather_points_forward(points, idx):
    """epn_gathering.gather_points_forward (gathering_cuda.cpp:29-46): (b,c,n),(b,m) -> (b,c,m)."""
    _need(points, torch.float32, "points"), _need(idx, torch.int32, "idx")
    b, c, n = points.shape
    m = idx.shape[1]
    out = torch.empty((b, c, m), dtype=torch.float32, device=points.device)
    _lib.call("etch_gather_points", b, c, n, m, points, idx, out)
    return out


def gather_points_backward(grad_out, idx, npoint):
    """epn_gathering.gather_points_backward (gathering_cuda.cpp:45-60): (b,c,m),(b,m),n -> (b,c,n)."""
    _need(grad_out, torch.float32, "grad_out"), _need(idx, torch.int32, "idx")
    b, c, m = grad_out.shape
    out = torch.empty((b, c, int(npoint)), dtype=torch.float32, device=grad_out.device)
    _lib.call("etch_gather_points_backward", b, c, int(npoint), m, grad_out, idx, out)
    return out


# ------------------------------------------------------------------ pointops_cuda
def _seg_max(offset_host):
    prev, mx = 0, 0
    for v in offset_host:
        mx = max(mx, int(v) - prev)
        prev = int(v)
    return mx


# kNN on a per-segment cell grid: the same idx / dist bit for bit.  KNN_GRID = False is the A/B partner and the tests' reference.
KNN_GRID = os.environ.get("ETCH_KNN_GRID", "1") != "0"
KNN_GRID_MIN_POINTS = 512        # smaller segments keep the full scan (a handful of 64-point chunks per query: nothing to save)
KNN_GRID_MAX_POINTS = 16384      # as the library's KNNG_MAX_POINTS / KNNG_MAX_CELLS
KNN_GRID_HEADER = 16


class KnnGrid:
    """The cell grid of one packed point tensor (ops.knn_grid_build): pts (n,4), cell_start (nseg, stride), header (nseg, 16)."""
    __slots__ = ("pts", "cell_start", "header", "stride")

    def __init__(self, pts, cell_start, header, stride):
        self.pts, self.cell_start, self.header, self.stride = pts, cell_start, header, stride

    def tensors(self):
        return [self.pts, self.cell_start, self.header]


def knn_grid_eligible_sizes(offset_host):
    """True if any segment has a size the grid takes (eligibility is a function of a segment's own size, never of the batch)."""
    prev = 0
    for v in offset_host:
        if KNN_GRID_MIN_POINTS <= int(v) - prev <= KNN_GRID_MAX_POINTS and int(v) - prev >= 17:
            return True
        prev = int(v)
    return False


def knn_grid_build(xyz, offset, min_points=None):
    """Cell grid of packed xyz (n,3) + offset for knnquery(grid=...): one launch, no host read."""
    _need(xyz, torch.float32, "xyz"), _need(offset, torch.int32, "offset")
    n, nseg = xyz.shape[0], offset.numel()
    stride = min(KNN_GRID_MAX_POINTS, 4 * max(int(n), 16)) + 1
    pts = torch.empty((n, 4), dtype=torch.float32, device=xyz.device)
    cell_start = torch.empty((nseg, stride), dtype=torch.int32, device=xyz.device)
    header = torch.empty((nseg, KNN_GRID_HEADER), dtype=torch.int32, device=xyz.device)
    _lib.call("etch_knn_grid_build", int(nseg), int(KNN_GRID_MIN_POINTS if min_points is None else min_points), xyz, offset, pts, cell_start, stride, header)
    return KnnGrid(pts, cell_start, header, stride)


def knnquery(nsample, xyz, new_xyz, offset, new_offset, new_offset_host=None, sqrt=True, wave_kernel=True, grid=None, offset_host=None, counters=None):
    """pointops.knnquery (pointops.py:32-45): -> idx (m,nsample) int32, dist (m,nsample) = sqrt(d2).

    `new_offset_host` (list of ints) avoids a device->host sync for the grid size; if omitted it is
    read back from `new_offset` (one sync, like the reference's own .item() calls).
    With KNN_GRID on, the wave kernel and nsample <= 16 the query runs on the cell grid of (xyz, offset): `grid` (knn_grid_build) if the caller
    has one, else built here; `offset_host`, when given, lets a call whose segments are all too small or too large skip the grid.  `counters`
    (5) int32 receives the number of queries per outcome (etch_knnquery_grid) and sends the call to the grid kernel whatever nsample is."""
    if new_xyz is None:
        new_xyz = xyz
    _need(xyz, torch.float32, "xyz"), _need(new_xyz, torch.float32, "new_xyz")
    _need(offset, torch.int32, "offset"), _need(new_offset, torch.int32, "new_offset")
    if new_offset_host is None:
        new_offset_host = new_offset.tolist()
    m = new_xyz.shape[0]
    idx = torch.empty((m, nsample), dtype=torch.int32, device=xyz.device)
    dist = torch.empty((m, nsample), dtype=torch.float32, device=xyz.device)
    use_grid = KNN_GRID and wave_kernel and m > 0 and xyz.shape[0] > 0 and offset.numel() == len(new_offset_host) and (
        counters is not None or grid is not None or (nsample <= 16 and (offset_host is None or knn_grid_eligible_sizes(offset_host))))
    if use_grid:
        if counters is not None:
            _need(counters, torch.int32, "counters")
            assert counters.numel() >= 5
        if grid is None:
            grid = knn_grid_build(xyz, offset)
        _lib.call("etch_knnquery_grid", len(new_offset_host), int(m), int(nsample), xyz, new_xyz, offset, new_offset, grid.pts, grid.cell_start,
                  int(grid.stride), grid.header, idx, dist, 1 if sqrt else 0, counters)
        return idx, dist
    _lib.call("etch_knnquery", len(new_offset_host), _seg_max(new_offset_host), int(m) if wave_kernel else 0, int(nsample), xyz, new_xyz, offset, new_offset,
              idx, dist, 1 if sqrt else 0)
    return idx, dist


def furthestsampling(xyz, offset, new_offset, offset_host=None, new_offset_host=None, split=None):
    """pointops.furthestsampling (pointops.py:10-28): packed (n,3) + offsets -> idx (m) int32."""
    _need(xyz, torch.float32, "xyz"), _need(offset, torch.int32, "offset"), _need(new_offset, torch.int32, "new_offset")
    if offset_host is None:
        offset_host = offset.tolist()
    if new_offset_host is None:
        new_offset_host = new_offset.tolist()
    idx = torch.zeros((int(new_offset_host[-1]),), dtype=torch.int32, device=xyz.device)
    nseg, n_max = len(offset_host), _seg_max(offset_host)
    G = fps_split_default(nseg, n_max, xyz.device) if split is None else int(split)
    if G >= 2:
        ws = _fps_split_ws(nseg, G, xyz.device)
        _lib.call("etch_furthestsampling_split", nseg, n_max, xyz, offset, new_offset, idx, G, ws)
        idx._etch_split_ws = ws
        return _fps_split_checked(idx, split)
    _lib.call("etch_furthestsampling", nseg, n_max, xyz, offset, new_offset, idx)
    return idx


# ------------------------------------------------------------------ dense layers
ACT = {None: 0, "none": 0, "relu": 1, "leaky_relu": 2}


def linear(x, weight, bias=None, scale=None, shift=None, act=None, res=None, res_mode=0, row_idx=None, grp=1, p_in=0, p_out=1,
           rows=None, out=None):
    """Y = epi(X[rowmap] @ W^T) via etch_linear.  x [*, K] (last dim contiguous), weight [O, K]."""
    _need(weight, torch.float32, "weight")
    if x.dtype != torch.float32 or not x.is_cuda:
        raise _lib.EtchHipError("x must be a float32 CUDA(HIP) tensor")
    K = x.shape[-1]
    assert x.stride(-1) == 1 and weight.shape[1] == K, (x.shape, weight.shape)
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    ldx = x2.stride(0) if x2.shape[0] > 1 else K
    R = x2.shape[0] if rows is None else rows
    O = weight.shape[0]
    if out is None:
        out = torch.empty((R, O), dtype=torch.float32, device=x.device)
    else:
        _lib.wrote(out)         # (the caller's tensor; announced ahead of the launch, which is asynchronous anyway)
    ldr = res.stride(0) if res is not None and res.dim() == 2 and res.shape[0] > 1 else O
    _lib.call("etch_linear", int(R), int(K), int(O), x2, ldx, row_idx, int(grp), int(p_in), int(p_out), weight, weight.stride(0), bias, scale, shift, ACT[act],
              res, ldr, int(res_mode), out, out.stride(0))
    return out


LINEAR_STATS_SHAPES = ((32, 32), (64, 64), (32, 64))      # (K, O) of the encoder's skip convs: the shapes etch_linear_stats is built for


def linear_stats_supported(x, weight, strided=False):
    shape = (x.shape[-1], weight.shape[0])
    return (shape == (32, 64) if strided else shape in LINEAR_STATS_SHAPES) and x.is_contiguous() and weight.is_contiguous()


def linear_stats(x, weight, bias, b, rows, row_idx=None, grp=1, p_in=0, p_out=1):
    """The skip conv with its InstanceNorm statistics from the GEMM's epilogue (etch_linear_stats): Y = X[rowmap] W^T + bias for b samples of `rows` rows
    each -> Y (b * rows, O), mean (b, O), rstd (b, O).  x (b * rows_in, K) contiguous; row_idx (b, p_out) int32 with grp / p_in / p_out as in linear()
    (rows = p_out * grp).  (K, O) in LINEAR_STATS_SHAPES; with row_idx (32, 64) only.  Y is bitwise linear()'s with the same arguments."""
    _need(x, torch.float32, "x"), _need(weight, torch.float32, "weight")
    K, O = x.shape[-1], weight.shape[0]
    assert weight.shape[1] == K
    if row_idx is not None:
        _need(row_idx, torch.int32, "row_idx")
        assert row_idx.numel() == b * p_out and rows == p_out * grp
    parts = _lib.call("etch_linear_stats_parts", int(rows), 0 if row_idx is None else 1)
    out = torch.empty((b * rows, O), dtype=torch.float32, device=x.device)
    part = torch.empty((b, parts, 2, O), dtype=torch.float64, device=x.device)
    mean = torch.empty((b, O), dtype=torch.float32, device=x.device)
    rstd = torch.empty((b, O), dtype=torch.float32, device=x.device)
    _lib.call("etch_linear_stats", int(b), int(rows), int(K), int(O), x, K, row_idx, int(grp), int(p_in), int(p_out), weight, K, bias, out, O, part, mean, rstd)
    return out, mean, rstd


def permute_weight_frag(w2):
    """[O, K] (O % 16 == 0, K % 16 == 0) -> MFMA fragment order Wp[t][mt][lane][s] = W2[16mt + lane%16][16t + 4(lane//16) + s]."""
    O, K = w2.shape
    assert O % 16 == 0 and K % 16 == 0
    return w2.reshape(O // 16, 16, K // 16, 4, 4).permute(2, 0, 3, 1, 4).contiguous().reshape(-1)


def permute_weight_frag32(w2):
    """[O, K] (O % 32 == 0, K % 8 == 0) -> 32x32x2 MFMA fragment order Wp[t][mt][lane][s] = W2[32mt + lane%32][8t + 4(lane//32) + s]."""
    O, K = w2.shape
    assert O % 32 == 0 and K % 8 == 0
    return w2.reshape(O // 32, 32, K // 8, 2, 4).permute(2, 0, 3, 1, 4).contiguous().reshape(-1)


def inter_weight_frag(W, cin, ks=24):
    """Fragment-ordered weight of the fused inter conv: the columns of W [cout, cin*ks] are first brought into the kernel's
    contraction order (csrc/so3conv.hip: channels are processed in passes of CCH = min(cin, 64); within a pass a lane gathers
    VEC = CCH/16 consecutive channels per load, so column r of c-tile mi is channel VEC*r + mi and sits at position 16*mi + r of its
    half; halves h of the X1 tile hold the tiles [h*MTH, (h+1)*MTH)), then permuted into MFMA fragment order."""
    return permute_weight_frag(W[:, _inter_contraction_cols(cin, ks, W.device)].contiguous())


_CONTRACTION_COLS = Shared()


def _inter_contraction_cols(cin, ks, device):
    """Column permutation of W [cout, cin*ks] into the contraction order of inter_so3conv_kernel (see inter_weight_frag); one upload per (shape, device)."""
    return _CONTRACTION_COLS.get((cin, ks, str(device)), lambda: _inter_contraction_cols_build(cin, ks, device))


def _inter_contraction_cols_build(cin, ks, device):
    cch = min(cin, 64)
    vec = cch // 16
    halves = 2 if cch >= 32 else 1
    mth = vec // halves
    one = [vec * (cc % 16) + h * mth + cc // 16 for h in range(halves) for cc in range(cch // halves)]
    order = [p * cch + c for p in range(cin // cch) for c in one]
    assert sorted(order) == list(range(cin))
    return torch.tensor([c * ks + k for c in order for k in range(ks)], dtype=torch.long, device=device)


def split3_bf16(x):
    """fp32 tensor -> (3, *x.shape) int16: the bf16 bit patterns of the exact split x = hi + mid + lo (8 + 8 + 8 mantissa bits, by truncation;
    csrc/so3conv.hip split3_pack4 is the device-side twin)."""
    x = x.contiguous()
    hi = x.view(torch.int32) & -65536
    r = x - hi.view(torch.float32)
    mid = r.view(torch.int32) & -65536
    lo = (r - mid.view(torch.float32)).view(torch.int32)
    return torch.stack([(t >> 16).to(torch.int16) for t in (hi, mid, lo)])


def inter_weight_split(W, cin, ks=24):
    """Weight of etch_inter_so3conv_split: columns in the kernel's contraction order (the one of inter_weight_frag), split into three bf16 planes, in
    v_mfma_f32_16x16x32_bf16 A-fragment order: [chunk of 32 kappas][o tile][plane][lane = 16 * (k / 8) + o % 16][8]."""
    cout = W.shape[0]
    assert cin % 16 == 0 and cout % 16 == 0 and W.shape[1] == cin * ks and ks == 24
    planes = split3_bf16(W[:, _inter_contraction_cols(cin, ks, W.device)])     # [3][cout][K]
    K = cin * ks
    q = planes.reshape(3, cout // 16, 16, K // 32, 4, 8)                 # [pl][mt][ol][tg][kg][e]
    return q.permute(3, 1, 0, 4, 2, 5).contiguous().reshape(-1)          # [tg][mt][pl][kg][ol][e]


def intra_weight_split(w2):
    """W2 [C, 12 C] (tap-major K: W2[o, tap * C + ch]) -> the register-resident fragments of the weight-stationary intra conv
    (csrc/so3conv_ws.hip): [mt][kq][K step][plane][lane = 32 * (k / 8) + o % 32][8] with k = 3 kq C + 16 ks + 8 (lane / 32) + e."""
    C, K = w2.shape
    assert K == 12 * C and C in (32, 64)
    nks = 3 * C // 16
    planes = split3_bf16(w2)                                             # [3][C][K]
    q = planes.reshape(3, C // 32, 32, 4, nks, 2, 8)                     # [pl][mt][i][kq][ks][kg][e]
    return q.permute(1, 3, 4, 0, 5, 2, 6).contiguous().reshape(-1)       # [mt][kq][ks][pl][kg][i][e]


def _pow2_exp(m, cap=120):
    """m >= 0 (any shape) -> k (float32, integer valued) with m 2^k in [8, 16) -- the host mirror of the device's etch_scale_exp (csrc/split_bf16.h): zero,
    subnormal (below FLT_MIN) and non-finite maxima give k = 0, and k is capped at 120 so that 2^k AND 2^-k stay normal floats (an
    uncapped 4 - frexp(m) reaches 128 .. 130 for m <= 2^-124, exp2 of which is inf)."""
    ok = (m >= 1.1754943508222875e-38) & torch.isfinite(m)
    x = torch.frexp(torch.where(ok, m, torch.ones_like(m)))[1]           # m = f 2^x, f in [0.5, 1)  ->  m 2^(4 - x) in [8, 16)
    return torch.where(ok, (4 - x).clamp(max=cap), torch.zeros_like(x)).to(torch.float32)


def _row_pow2(w, cap=120):
    """w [rows, K] -> (w with every row times the power of two that puts its maximum into [8, 16), the inverse powers float32 [rows]); exact.  The fp16
    planes of an operand carry 23 bits only near that range: scaling per ROW keeps rows far below the matrix maximum at full precision (a trained
    weight matrix's rows may differ by orders of magnitude).  Rows whose maximum is zero / subnormal / non-finite keep the factor 1 (_pow2_exp)."""
    wd = w.detach()
    e = _pow2_exp(wd.abs().amax(1), cap)
    return wd * torch.exp2(e)[:, None], torch.exp2(-e).contiguous()


def intra_weight_split_f16(w2):
    """W2 [C, 12 C] -> the fragments of etch_intra_so3conv_f16: intra_weight_split's order with TWO fp16 planes (h = fp16(w), l = fp16(w - h)) of W2 with every
    row (output channel) times its own power of two (_row_pow2; exact); the inverse powers ride on the tensor as `.wsc` (the kernel's epilogue applies them)."""
    C, K = w2.shape
    assert K == 12 * C and C in (32, 64)
    nks = 3 * C // 16
    ws, wsc = _row_pow2(w2)
    hi = ws.to(torch.float16)
    planes = torch.stack([hi, (ws - hi.float()).to(torch.float16)])      # [2][C][K]
    q = planes.reshape(2, C // 32, 32, 4, nks, 2, 8)                     # [pl][mt][i][kq][ks][kg][e]
    out = q.permute(1, 3, 4, 0, 5, 2, 6).contiguous().reshape(-1).view(torch.int16)       # [mt][kq][ks][pl][kg][i][e]
    out.wsc = wsc
    return out


INTER_SPLIT = os.environ.get("ETCH_INTER_SPLIT", "1") != "0"      # step 2 of the inter conv on the bf16 matrix cores (split fp32 operands); 0: fp32 MFMA
INTER_X = os.environ.get("ETCH_INTER_X", "1") != "0"             # both contractions of the inter conv on the matrix cores, gathered rows as planes (csrc/so3conv_y.hip); 0: the round-3 kernels
INTER_KQ = os.environ.get("ETCH_INTER_KQ", "1") != "0"          # kernel weights formed on the matrix cores (csrc/so3conv_y.hip); 0: the round-3 kernels (fp32 MFMA step 1,
                                                                 # exact three-plane step 2)


def split2_planes_f16(x_cl):
    """x (..., C) fp32 -> (..., 2, C) float16: h = fp16(x), l = fp16(x - h), both to nearest, the layout etch_inter_so3conv_planes_kq gathers (the
    encoder's own producer, instnorm_act_add(want_planes="f16"), writes it directly)."""
    _need(x_cl, torch.float32, "x")
    C = x_cl.shape[-1]
    planes = torch.empty(tuple(x_cl.shape[:-1]) + (2, C), dtype=torch.float16, device=x_cl.device)
    _lib.call("etch_split2_planes_f16", x_cl.numel() // C, int(C), x_cl, planes)
    return planes


def split2_planes_f16_scaled(x_cl):
    """x (b, ..., C) fp32 of ANY scale -> ((b, ..., 2, C) float16 planes of x[s] * 2^k(s), fsc (b,) float32 = 2^-k(s)): every scan is brought to a maximum
    magnitude in [8, 16) before the split (exact), fsc is the factor etch_inter_so3conv_planes_kq's epilogue multiplies that scan's outputs with."""
    _need(x_cl, torch.float32, "x")
    b, C = x_cl.shape[0], x_cl.shape[-1]
    planes = torch.empty(tuple(x_cl.shape[:-1]) + (2, C), dtype=torch.float16, device=x_cl.device)
    mx = torch.zeros((b,), dtype=torch.int32, device=x_cl.device)
    fsc = torch.empty((b,), dtype=torch.float32, device=x_cl.device)
    _lib.call("etch_split2_planes_f16_scaled", int(b), x_cl.numel() // (b * C), int(C), x_cl, mx, planes, fsc)
    return planes, fsc


def inter_weight_split32_f16(W, cin, ks=24):
    """Weight of etch_inter_so3conv_planes_kq: the columns of W [cout, cin*24] in the kernel's PHYSICAL contraction order -- per channel half h
    (CH = cin / 2 channels), kernel point k, 16-byte block pb, element i: channel h*CH + 4*(pb ^ sw(k)) + i with the X1 tile's store swizzle
    sw(k) = (k >> 1) & 3 (CH = 16) / k & 7 (CH = 32) --, every row (output channel) times its own power of two (_row_pow2: exact; `.wsc` = the inverse
    powers, applied by the kernel's epilogue), as two fp16 planes h = fp16(w), l = fp16(w - h), in A-fragment order
    [K step of 16][o tile of 32][plane][lane = 32 * (kappa / 8 % 2) + o % 32][8]."""
    cout = W.shape[0]
    assert ks == 24 and cin in (32, 64) and cout % 32 == 0 and W.shape[1] == cin * ks
    ch = cin // 2
    cols = [(h * ch + 4 * (pb ^ (((k >> 1) & 3) if ch == 16 else (k & 7))) + i) * ks + k
            for h in range(2) for k in range(ks) for pb in range(ch // 4) for i in range(4)]
    assert sorted(cols) == list(range(cin * ks))
    ws, wsc = _row_pow2(W[:, torch.tensor(cols, dtype=torch.long, device=W.device)])
    hi = ws.to(torch.float16)
    planes = torch.stack([hi, (ws - hi.float()).to(torch.float16)])                       # [2][cout][K]
    K = cin * ks
    q = planes.reshape(2, cout // 32, 32, K // 16, 2, 8)                 # [pl][mt][o][s][kg][e]
    out = q.permute(3, 1, 0, 4, 2, 5).contiguous().reshape(-1)           # [s][mt][pl][kg][o][e]
    out.wsc = wsc
    return out


def inter_kpoint_operand(rk, sigma):
    """rk (60,24,3) fp32 rotated kernel points -> (60,2,64,8) int16: the kernel-point factor of the weights' pre-activation as matrix-core B
    fragments (etch_inter_so3conv_planes_kq)."""
    _need(rk, torch.float32, "rk")
    assert tuple(rk.shape) == (60, 24, 3)
    kq = torch.empty((60, 2, 64, 8), dtype=torch.int16, device=rk.device)
    _lib.call("etch_inter_kpoint_operand", float(sigma), rk, kq)
    return kq


def inter_planes_supported(cin, cout, nn):
    """Shapes etch_inter_so3conv_planes_kq covers (the three convs of the released encoder depth)."""
    return INTER_X and (cin, cout) in ((32, 32), (32, 64), (64, 64)) and nn in (32, 64)      # = etch_inter_so3conv_planes_supported


def split3_planes(x_cl):
    """x (..., C) fp32 -> (..., 3, C) int16: the bf16 bit patterns of the exact split x = hi + mid + lo (the layout instnorm_act_add(want_planes=True)
    writes)."""
    _need(x_cl, torch.float32, "x")
    C = x_cl.shape[-1]
    planes = torch.empty(tuple(x_cl.shape[:-1]) + (3, C), dtype=torch.int16, device=x_cl.device)
    _lib.call("etch_split3_planes", x_cl.numel() // C, int(C), x_cl, planes)
    return planes


# ------------------------------------------------------------------ EPN encoder
def spatial_order(xyz):
    """xyz (b,3,n) -> (b,n) int32 Morton order of each scan (scheduling hint for inter_so3conv / prop_interp: a permutation of
    0..n-1 per scan; 30-bit codes up to 16 384 points, 15-bit codes in 32 768-point slices above)."""
    _need(xyz, torch.float32, "xyz")
    b, _, n = xyz.shape
    order = torch.empty((b, n), dtype=torch.int32, device=xyz.device)
    _lib.call("etch_spatial_order", b, n, xyz, order)
    return order


def inter_so3conv(xyz, new_xyz, ball_idx, feats_cl, rk, W, Wp, bias, sigma, order=None, want_stats=False, Wq=None, feats_planes=None, kq=None, Wqh=None):
    """feats_cl (b,p1,60,cin) channels-last -> (b,p2,60,cout) pre-norm.  order (b,p2) int32: processing order of the output points.
    want_stats: also return the InstanceNorm (mean, rstd) of the output, accumulated in the conv's epilogue.  Three paths, the first that applies:
    kq (inter_kpoint_operand) + Wqh (inter_weight_split32_f16), a shape of inter_planes_supported: etch_inter_so3conv_planes_kq (weights' pre-activation
    on the matrix cores, two fp16 planes per operand); feats_planes (b,p1,60,2,cin) float16 = split2_planes_f16 (made here when absent or in the bf16
    format).  ETCH_INTER_KQ=0 / ETCH_INTER_X=0 switch it off.
    Wq (inter_weight_split), cin a multiple of 16: etch_inter_so3conv_split, the round-3 kernel with step 2 on the bf16 matrix cores (ETCH_INTER_SPLIT=0: off).
    Otherwise etch_inter_so3conv_ordered, the fp32 kernel (W, Wp = inter_weight_frag)."""
    b, p1, na, cin = feats_cl.shape
    p2, nn = ball_idx.shape[1], ball_idx.shape[2]
    cout = W.shape[0]
    for t, n in ((xyz, "xyz"), (new_xyz, "new_xyz"), (feats_cl, "feats"), (rk, "rk"), (W, "W"), (bias, "bias")):
        _need(t, torch.float32, n)
    _need(ball_idx, torch.int32, "ball_idx")
    if order is not None:
        _need(order, torch.int32, "order")
        assert tuple(order.shape) == (b, p2)
    out = torch.empty((b, p2, 60, cout), dtype=torch.float32, device=xyz.device)
    fused = want_stats and 256 % cout == 0 and (cin >= 16 or (cin == 1 and cout <= 64 and nn * 60 >= 1026))      # the c1 kernel's own precondition (so3conv.hip)
    part = torch.empty((b, p2, 2, cout), dtype=torch.float64, device=xyz.device) if fused else None
    if kq is not None and Wqh is not None and INTER_KQ and inter_planes_supported(cin, cout, nn):
        _need(Wqh, torch.float16, "Wqh"), _need(kq, torch.int16, "kq")
        fsc = None
        if feats_planes is None or feats_planes.dtype != torch.float16:
            # the caller's own features, of unknown scale (the operator API has no domain restriction): planes of every scan times its own power of two,
            # undone by the kernel's epilogue (fsc).  Planes that arrive with the features are the producer's (instnorm_act_add: unit scale by construction)
            feats_planes, fsc = split2_planes_f16_scaled(feats_cl)
        _need(feats_planes, torch.float16, "feats_planes")
        assert tuple(feats_planes.shape) == (b, p1, na, 2, cin) and kq.numel() == 60 * 2 * 64 * 8 and Wqh.numel() == 2 * cout * cin * 24
        _lib.call("etch_inter_so3conv_planes_kq", b, cin, cout, p1, p2, nn, float(sigma), xyz, new_xyz, ball_idx, feats_planes, kq, Wqh, Wqh.wsc, fsc, bias,
                  out, order, part)
    elif Wq is not None and INTER_SPLIT and cin % 16 == 0:
        _need(Wq, torch.int16, "Wq")
        _lib.call("etch_inter_so3conv_split", b, cin, cout, p1, p2, nn, float(sigma), xyz, new_xyz, ball_idx, feats_cl, rk, Wq, bias, out, order, part)
    else:
        # all-ones features (the encoder's occupancy tensor, registered by models/so3conv.py and not written to since): the one-channel kernel takes NULL
        # and skips the feature gather
        unit = cin == 1 and constant_value(feats_cl) == 1.0 and cout <= 64 and nn * 60 >= 1026
        _lib.call("etch_inter_so3conv_ordered", b, cin, cout, p1, p2, nn, float(sigma), xyz, new_xyz, ball_idx, None if unit else feats_cl, rk, W, Wp, bias, out,
                  order, part)
    if not want_stats:
        return out
    if not fused:
        return out, instnorm_stats(out)
    mean = torch.empty((b, cout), dtype=torch.float32, device=xyz.device)
    rstd = torch.empty((b, cout), dtype=torch.float32, device=xyz.device)
    _lib.call("etch_instnorm_from_partials", b, p2, cout, 60, part, mean, rstd)
    return out, (mean, rstd)


INTRA_MFMA32 = os.environ.get("ETCH_INTRA_MFMA32", "1") != "0"     # widths 32 / 64: the 32x32x2 MFMA form (ETCH_INTRA_MFMA32=0: the 16x16x4 kernel)
INTRA_SPLIT = os.environ.get("ETCH_INTRA_SPLIT", "1") != "0"       # widths 32 / 64: weight-stationary on the bf16 matrix cores, split fp32 operands
INTRA_F16 = os.environ.get("ETCH_INTRA_SPLIT", "1") != "bf16"     # ... as two fp16 planes and three cross terms (round 5); "bf16": the three-plane bf16 form


def intra_so3conv(x_cl, intra_idx32, Wp, bias, cout, mean=None, rstd=None, want_stats=False, Wp32=None, Wq=None, Wqh=None):
    """want_stats: also return the InstanceNorm (mean, rstd) of the output, accumulated in the conv's epilogue (even point counts;
    otherwise by the separate statistics pass)."""
    b, p, na, c = x_cl.shape
    _need(x_cl, torch.float32, "x"), _need(intra_idx32, torch.int32, "intra_idx"), _need(Wp, torch.float32, "Wp")
    out = torch.empty((b, p, 60, cout), dtype=torch.float32, device=x_cl.device)
    fused = want_stats and p % 2 == 0 and c <= 64        # wider tiles (encoder depths 3 / 4) take the separate statistics pass
    part = torch.empty((b * (p // 2), 2, cout), dtype=torch.float64, device=x_cl.device) if fused else None
    # the two-plane fp16 form splits the NORMALISED tile (unit scale by construction); without statistics the rows are the caller's own, of unknown scale
    # (> 65 504 -> inf, far below 1 -> the planes' absolute floor): those calls take the exact forms below
    if Wqh is not None and mean is not None and rstd is not None and INTRA_SPLIT and INTRA_F16 and c == cout and c in (32, 64) and (part is None or p % 2 == 0):
        _need(Wqh, torch.int16, "Wqh")
        _lib.call("etch_intra_so3conv_f16", b, c, cout, p, x_cl, mean, rstd, intra_idx32, Wqh, Wqh.wsc, bias, out, part)
    elif Wq is not None and INTRA_SPLIT and c == cout and c in (32, 64) and (part is None or p % 2 == 0):
        _need(Wq, torch.int16, "Wq")
        _lib.call("etch_intra_so3conv_split", b, c, cout, p, x_cl, mean, rstd, intra_idx32, Wq, bias, out, part)
    elif Wp32 is not None and INTRA_MFMA32 and c == cout and c in (32, 64):
        _lib.call("etch_intra_so3conv32", b, c, cout, p, x_cl, mean, rstd, intra_idx32, Wp32, bias, out, part)
    else:
        _lib.call("etch_intra_so3conv_stats", b, c, cout, p, x_cl, mean, rstd, intra_idx32, Wp, bias, out, part)
    if not want_stats:
        return out
    if not fused:
        return out, instnorm_stats(out)
    m = torch.empty((b, cout), dtype=torch.float32, device=x_cl.device)
    r = torch.empty((b, cout), dtype=torch.float32, device=x_cl.device)
    _lib.call("etch_instnorm_from_partials", b, p // 2, cout, 120, part, m, r)
    return out, (m, r)


def instnorm_stats(x_cl):
    """x (b, ..., C) -> mean (b,C), rstd (b,C) over all middle dims."""
    _need(x_cl, torch.float32, "x")
    b, C = x_cl.shape[0], x_cl.shape[-1]
    rows = x_cl.numel() // (b * C)
    ws = torch.empty((_lib.call("etch_instnorm_stats_workspace_bytes", b, C) // 8,), dtype=torch.float64, device=x_cl.device)
    mean = torch.empty((b, C), dtype=torch.float32, device=x_cl.device)
    rstd = torch.empty((b, C), dtype=torch.float32, device=x_cl.device)
    _lib.call("etch_instnorm_stats", b, rows, C, x_cl, ws, mean, rstd)
    return mean, rstd


def instnorm_from_partials(part, total, wide=True):
    """part (b, nparts, 2, C) fp64 sums / sums of squares over `total` values per (sample, channel) -> mean (b, C), rstd (b, C).  wide: one workgroup per
    channel quad and sample; False: the one-workgroup form (the same bits)."""
    _need(part, torch.float64, "part")
    b, nparts, two, C = part.shape
    assert two == 2
    mean = torch.empty((b, C), dtype=torch.float32, device=part.device)
    rstd = torch.empty((b, C), dtype=torch.float32, device=part.device)
    _lib.call("etch_instnorm_from_partials_n", b, nparts, C, int(total), part, mean, rstd, 1 if wide else 0)
    return mean, rstd


ANCHOR_MEAN_WIDTHS = (32, 64, 128, 256)


def instnorm_act_add_mean(x1, m1, r1, x2=None, m2=None, r2=None):
    """instnorm_act_add for x1 (b, p, 60, C) that also returns the mean of the result over each point's 60 anchor rows, (b * p, C): bitwise
    token_mean(out.view(b * p, 60, C)), from the pass that wrote out.  C in ANCHOR_MEAN_WIDTHS."""
    _need(x1, torch.float32, "x1")
    b, p, na, C = x1.shape
    assert na == 60 and C in ANCHOR_MEAN_WIDTHS
    if x2 is not None:
        _need(x2, torch.float32, "x2")
    out = torch.empty_like(x1)
    mean = torch.empty((b * p, C), dtype=torch.float32, device=x1.device)
    _lib.call("etch_instnorm_act_add_mean", b, p, C, x1, m1, r1, x2, m2, r2, out, mean)
    return out, mean


def instnorm_act_add_k1(x1, m1, r1, f, slope, offset, want_planes=False):
    """out = lrelu((x1 - m1) r1) + lrelu(f slope + offset): the second branch a one-channel 1x1 conv + InstanceNorm folded into per-(scan, channel)
    slope / offset (etch_instnorm_act_add_k1_planes_f16).  x1 (b, ..., C), f (b, rows) one value per row of x1, slope / offset (b, C).
    want_planes: False or "f16"."""
    _need(x1, torch.float32, "x1"), _need(f, torch.float32, "f"), _need(slope, torch.float32, "slope"), _need(offset, torch.float32, "offset")
    b, C = x1.shape[0], x1.shape[-1]
    rows = x1.numel() // (b * C)
    assert f.numel() == b * rows and tuple(slope.shape) == (b, C) and tuple(offset.shape) == (b, C) and want_planes in (False, None, "f16")
    out = torch.empty_like(x1)
    planes = torch.empty(tuple(x1.shape[:-1]) + (2, C), dtype=torch.float16, device=x1.device) if want_planes else None
    _lib.call("etch_instnorm_act_add_k1_planes_f16", b, rows, C, x1, m1, r1, f.contiguous(), slope.contiguous(), offset.contiguous(), out, planes)
    return (out, planes) if want_planes else out


def instnorm_act_add(x1, m1, r1, x2=None, m2=None, r2=None, want_planes=False):
    """want_planes: also return the result split for the next conv's gathers -- True / "bf16": three bf16 planes (..., 3, C) int16
    (etch_inter_so3conv_planes); "f16": two fp16 planes (..., 2, C) float16 (etch_inter_so3conv_planes_kq)."""
    _need(x1, torch.float32, "x1")
    b, C = x1.shape[0], x1.shape[-1]
    rows = x1.numel() // (b * C)
    out = torch.empty_like(x1)
    f16 = want_planes == "f16"
    planes = None
    if want_planes:
        planes = torch.empty(tuple(x1.shape[:-1]) + ((2, C) if f16 else (3, C)), dtype=torch.float16 if f16 else torch.int16, device=x1.device)
    _lib.call("etch_instnorm_act_add_planes_f16" if f16 else "etch_instnorm_act_add_planes", b, rows, C, x1, m1, r1, x2, m2, r2, out, planes)
    return (out, planes) if want_planes else out


# ------------------------------------------------------------------ propagation + direction head
def prop3nn(xyz1_bn3, xyz2_b3s):
    _need(xyz1_bn3, torch.float32, "xyz1"), _need(xyz2_b3s, torch.float32, "xyz2")
    B, N, _ = xyz1_bn3.shape
    S = xyz2_b3s.shape[2]
    idx = torch.empty((B, N, 3), dtype=torch.int32, device=xyz1_bn3.device)
    w = torch.empty((B, N, 3), dtype=torch.float32, device=xyz1_bn3.device)
    _lib.call("etch_prop3nn", B, N, S, xyz1_bn3, xyz2_b3s, idx, w)
    return idx, w


def prop_interp(feats_cl, idx, w, order=None):
    """feats_cl (B,S,A,C) -> out (B,N,A,C), inv (B,N,C).  order (B,N) int32: processing order of the fine points (scheduling only)."""
    _need(feats_cl, torch.float32, "feats"), _need(idx, torch.int32, "idx"), _need(w, torch.float32, "w")
    if order is not None:
        _need(order, torch.int32, "order")
    B, S, A, C = feats_cl.shape
    N = idx.shape[1]
    out = torch.empty((B, N, A, C), dtype=torch.float32, device=feats_cl.device)
    inv = torch.empty((B, N, C), dtype=torch.float32, device=feats_cl.device)
    _lib.call("etch_prop_interp_ordered", B, N, S, A, C, feats_cl, idx, w, out, inv, order)
    return out, inv


def mhsa_attention(qkv, T, qoff, koff, voff, embedding_dim=64):
    """qkv [T*60, ld] -> [T*60, embedding_dim]: 8-head attention over each point's 60 tokens (heads of embedding_dim / 8)."""
    _need(qkv, torch.float32, "qkv")
    E = int(embedding_dim)
    out = torch.empty((T * 60, E), dtype=torch.float32, device=qkv.device)
    _lib.call("etch_mhsa_attention_dim", T, E, qkv, qkv.stride(0), qoff, koff, voff, out, E)
    return out


def mhsa_layer(x, wq, wk, wv, wc=None, bc=None, mode=0):
    """x [T*60, 64] tokens -> [T*60, 64]: one fused MultiHeadAttention layer (mode 0 residual, 1 plain, 2 heads only)."""
    for t, n in ((x, "x"), (wq, "wq"), (wk, "wk"), (wv, "wv")) + (((wc, "wc"), (bc, "bc")) if mode != 2 else ()):
        _need(t, torch.float32, n)
    assert x.shape[-1] == 64 and x.numel() % (60 * 64) == 0 and wq.shape == (64, 64)
    T = x.numel() // (60 * 64)
    out = torch.empty((T * 60, 64), dtype=torch.float32, device=x.device)
    _lib.call("etch_mhsa_layer", T, x, wq, wk, wv, wc, bc, int(mode), out)
    return out


def dirtail_weight_split(Wf):
    """Wf (128, 64) fp32 (direction_predictor.net[0] o head_combine) -> the two fp16 planes of Wf, every row (hidden unit) times its own power of two 2^kw
    (_row_pow2), as A fragments of v_mfma_f32_32x32x16_f16: [wave w = hidden tile of 32][K step ks][plane][lane = 32 * (k / 8 % 2) + h % 32][8] with
    k = 16 ks + 8 (lane / 32) + e (etch_mhsa_layer_dirtail).  `.wsc` = 2^-kw: the caller folds it into the tail's constants -- relu(2^-kw a + b) v =
    relu(a + 2^kw b) (2^-kw v) -- so the kernel needs no per-unit factor (dirtail_constants)."""
    assert tuple(Wf.shape) == (128, 64)
    ws, wsc = _row_pow2(Wf.float(), cap=60)         # the power is folded into the bias (bf 2^kw, dirtail_constants): capped so that fold cannot overflow
    hi = ws.to(torch.float16)
    planes = torch.stack([hi, (ws - hi.float()).to(torch.float16)])        # [2][128][64]
    q = planes.reshape(2, 4, 32, 4, 2, 8)                                  # [pl][w][h][ks][kg][e]
    out = q.permute(1, 3, 0, 4, 2, 5).contiguous().reshape(-1)             # [w][ks][pl][kg][h][e]
    out.wsc = wsc
    return out


def dirtail_constants(bf, v, c, wsc):
    """[bf (128) | v (128) | c] of etch_mhsa_layer_dirtail with the hidden units' powers of two folded in (exact): bf / wsc, v * wsc."""
    return torch.cat([bf / wsc, v * wsc, c.view(1)]).contiguous()


def mhsa_layer_dirtail(x, wq, wk, wv, Wfq, tab):
    """x [T*60, 64] tokens -> anc_w [T, 60]: the last MultiHeadAttention layer's heads + the folded direction tail in one kernel."""
    for t, n in ((x, "x"), (wq, "wq"), (wk, "wk"), (wv, "wv"), (tab, "tab")):
        _need(t, torch.float32, n)
    _need(Wfq, torch.float16, "Wfq")
    assert x.shape[-1] == 64 and x.numel() % (60 * 64) == 0 and wq.shape == (64, 64) and Wfq.numel() == 2 * 128 * 64 and tab.numel() == 257
    T = x.numel() // (60 * 64)
    out = torch.empty((T, 60), dtype=torch.float32, device=x.device)
    _lib.call("etch_mhsa_layer_dirtail", T, x, wq, wk, wv, Wfq, tab, out)
    return out


def mhsa_interp_layer(feats_cl, idx, w, wq, wk, wv, wc, bc, order=None):
    """First (residual) MHSA layer on the 3-NN interpolated tokens, which are formed inside the kernel: feats_cl (B,S,60,64) coarse
    tokens, idx / w (B,N,3) from prop3nn -> (B*N*60, 64).  order (B,N) int32: processing order of the fine points (scheduling only)."""
    for t, n in ((feats_cl, "feats"), (w, "w"), (wq, "wq"), (wk, "wk"), (wv, "wv"), (wc, "wc")):
        _need(t, torch.float32, n)
    _need(idx, torch.int32, "idx")
    if order is not None:
        _need(order, torch.int32, "order")
    if bc is not None:
        _need(bc, torch.float32, "bc")
    B, S, A, C = feats_cl.shape
    assert (A, C) == (60, 64) and idx.shape[0] == B and idx.shape == w.shape
    N = idx.shape[1]
    out = torch.empty((B * N * 60, 64), dtype=torch.float32, device=feats_cl.device)
    sched = torch.empty((B * N, 8), dtype=torch.int32, device=feats_cl.device)      # workspace: per-slot records of the processing order
    _lib.call("etch_mhsa_interp_layer", B, N, S, feats_cl, idx, w, order, wq, wk, wv, wc, bc, out, sched)
    return out


def mhsa_interp_layer_list(feats_cl, sel, idx, w, wq, wk, wv, wc, bc):
    """mhsa_interp_layer at a list of points: sel (B, P) int32 global point rows b*N + n (or -1: an empty slot, whose output is to be ignored)
    -> (B*P*60, 64), slot k at rows 60 k ...; bitwise the rows of those points in mhsa_interp_layer's output."""
    for t, n in ((feats_cl, "feats"), (w, "w"), (wq, "wq"), (wk, "wk"), (wv, "wv"), (wc, "wc")):
        _need(t, torch.float32, n)
    _need(idx, torch.int32, "idx"), _need(sel, torch.int32, "sel")
    if bc is not None:
        _need(bc, torch.float32, "bc")
    B, S, A, C = feats_cl.shape
    assert (A, C) == (60, 64) and idx.shape[0] == B and idx.shape == w.shape and sel.dim() == 2 and sel.shape[0] == B
    N, P = idx.shape[1], sel.shape[1]
    out = torch.empty((B * P * 60, 64), dtype=torch.float32, device=feats_cl.device)
    sched = torch.empty((B * P, 8), dtype=torch.int32, device=feats_cl.device)      # workspace: one record per slot
    _lib.call("etch_mhsa_interp_layer_list", B, P, N, S, feats_cl, sel, idx, w, wq, wk, wv, wc, bc, out, sched)
    return out


def token_mean(x):
    """x (T, A, C) -> mean over the A tokens (T, C)."""
    _need(x, torch.float32, "x")
    T, A, C = x.shape
    out = torch.empty((T, C), dtype=torch.float32, device=x.device)
    _lib.call("etch_token_mean", T, A, C, x, out)
    return out


def rowdot(x, w, bias):
    _need(x, torch.float32, "x"), _need(w, torch.float32, "w")
    R, K = x.shape
    y = torch.empty((R,), dtype=torch.float32, device=x.device)
    _lib.call("etch_rowdot", R, K, x, x.stride(0), w, float(bias), y)
    return y


def so3_mean_dir(w, anchors, want_R=False, want_sv=False):
    _need(w, torch.float32, "w"), _need(anchors, torch.float32, "anchors")
    T, A = w.shape
    d = torch.empty((T, 3), dtype=torch.float32, device=w.device)
    R = torch.empty((T, 3, 3), dtype=torch.float32, device=w.device) if want_R else None
    sv = torch.empty((T, 3), dtype=torch.float32, device=w.device) if want_sv else None
    _lib.call("etch_so3_mean_dir", T, A, w, anchors, d, R, sv)
    return d, R, sv


# ------------------------------------------------------------------ Point-Transformer pieces
def pt_attention(p, qkv, c, idx, params, ns):
    """qkv [n,3c] (q|k|v) ; params: list of 16 tensors-or-None -> out [n,c]."""
    n = p.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=p.device)
    arr = (ctypes.c_void_p * 16)(*[(0 if t is None else t.data_ptr()) for t in params])
    base = qkv.data_ptr()
    _lib.call("etch_pt_attention", n, c, ns, p, base, base + 4 * c, base + 8 * c, qkv.stride(0), idx, arr, out, c)
    return out


PT_MFMA_SHAPES = {(64, 8), (128, 8), (64, 16), (128, 16), (256, 16), (512, 16)}     # (c, nsample) instantiated in pt.hip


def pt_attention_mfma(p, qkv, c, idx, params, ns, w2):
    """Same result as pt_attention: gather, linear_w MLP (matrix cores), neighbour softmax and aggregation in one kernel."""
    n = p.shape[0]
    _need(w2, torch.float32, "w2")
    out = torch.empty((n, c), dtype=torch.float32, device=p.device)
    arr = (ctypes.c_void_p * 16)(*[(0 if t is None else t.data_ptr()) for t in params])
    base = qkv.data_ptr()
    _lib.call("etch_pt_attention_mfma", n, c, ns, p, base, base + 4 * c, base + 8 * c, qkv.stride(0), idx, arr, w2, out, c)
    return out


def pt_attention_split(p, qkv, c, idx, params, ns, w2, b2, s3, t3, w5, b5):
    """Same result as pt_attention with the two Linear layers of linear_w on the matrix cores (etch_linear)."""
    n = p.shape[0]
    arr = (ctypes.c_void_p * 16)(*[(0 if t is None else t.data_ptr()) for t in params])
    base = qkv.data_ptr()
    ldq = qkv.stride(0)
    w_in = torch.empty((n * ns, c), dtype=torch.float32, device=p.device)
    _lib.call("etch_pt_attn_prep", n, c, ns, p, base, base + 4 * c, ldq, idx, arr, w_in)
    hid = linear(w_in, w2, bias=b2, scale=s3, shift=t3, act="relu")
    logits = linear(hid, w5, bias=b5)
    out = torch.empty((n, c), dtype=torch.float32, device=p.device)
    _lib.call("etch_pt_attn_aggregate", n, c, ns, p, base + 8 * c, ldq, idx, logits, arr, out, c)
    return out


def pt_group(p, new_p, x, idx, pad_to=1):
    """-> (m*ns, ld) with ld = 3 + c rounded up to a multiple of `pad_to` (padding columns are zero)."""
    m, ns = idx.shape
    c = x.shape[1]
    ld = -(-(3 + c) // pad_to) * pad_to
    out = torch.empty((m * ns, ld), dtype=torch.float32, device=p.device)
    _lib.call("etch_pt_group", m, ns, c, p, new_p, x, x.stride(0), idx, out, ld)
    return out


def pt_down_gather_max(ux, p, new_p, idx, wp, scale, shift):
    """out[i] = max_j relu(bn(ux[idx[i,j]] + wp @ (p[idx[i,j]] - new_p[i]))): TransitionDown without the grouped rows."""
    m, ns = idx.shape
    co = ux.shape[1]
    out = torch.empty((m, co), dtype=torch.float32, device=ux.device)
    _lib.call("etch_pt_down_gather_max", m, ns, co, ux, ux.stride(0), p, new_p, idx, wp, scale, shift, out)
    return out


def gather_rows(x, idx):
    m, c = idx.shape[0], x.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=x.device)
    _lib.call("etch_gather_rows", m, c, x, x.stride(0), idx, out)
    return out


def rows_maxpool(x, ns):
    m, c = x.shape[0] // ns, x.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=x.device)
    _lib.call("etch_rows_maxpool", m, ns, c, x, out)
    return out


def pt_interp_add(a, f, idx, dist):
    n, c = a.shape
    out = torch.empty_like(a)
    _lib.call("etch_pt_interp_add", n, c, a, f, idx, dist, out)
    return out


def seg_mean(x, offset, nseg):
    c = x.shape[1]
    out = torch.empty((nseg, c), dtype=torch.float32, device=x.device)
    _lib.call("etch_seg_mean", nseg, c, x, offset, out)
    return out


def concat_bcast(x, g, offset, nseg):
    n, c = x.shape
    out = torch.empty((n, 2 * c), dtype=torch.float32, device=x.device)
    _lib.call("etch_concat_bcast", n, c, nseg, x, g, offset, out)
    return out


def grouped_dot(h, w, bias, G, J, out=None):
    R = h.shape[0]
    if out is None:
        out = torch.empty((R, G), dtype=torch.float32, device=h.device)
    else:
        _lib.wrote(out)
    _lib.call("etch_grouped_dot", R, G, J, h, h.stride(0), w, bias, out, out.stride(0))
    return out


LRD_SPLIT = os.environ.get("ETCH_LRD_SPLIT", "1") != "0"       # linear_relu_dot on the bf16 matrix cores (split fp32 operands); 0: fp32 MFMA
LRD_F16 = os.environ.get("ETCH_LRD_SPLIT", "1") != "bf16"      # ... as two fp16 planes per operand where the weight-stationary kernel applies; "bf16": three bf16 planes


def lrd_weight_split(w, J=128):
    """[G*J, K] -> int16 [G][K/32][J/16 strips][plane hi / mid / lo][lane = 16 * (k / 8) + column][8]: the exactly split weight of
    etch_linear_relu_dot_split in v_mfma_f32_16x16x32_bf16 B-fragment order."""
    GJ, K = w.shape
    assert GJ % J == 0 and J % 16 == 0 and K % 32 == 0
    planes = split3_bf16(w)                                                   # [3][GJ][K]
    q = planes.reshape(3, GJ // J, J // 16, 16, K // 32, 4, 8)               # [pl][g][strip][col][t][kg][e]
    return q.permute(1, 4, 2, 0, 5, 3, 6).contiguous().reshape(-1)           # [g][t][strip][pl][kg][col][e]


def lrd_weight_split_f16(w, J=128):
    """[G*J, K] -> float16 [G][K/32][J/16 strips][plane h / l][lane = 16 * (k / 8) + column][8]: two fp16 planes of W with every ROW (hidden unit) times
    the power of two that puts its maximum into [8, 16) (exact; the kernel's epilogue takes it out again), in v_mfma_f32_16x16x32_f16 fragment order; the
    rows' inverse powers ride on the tensor as `.wsc` (float32 [G*J], etch_linear_relu_dot_f16)."""
    GJ, K = w.shape
    assert GJ % J == 0 and J % 16 == 0 and K % 32 == 0
    ws, wsc = _row_pow2(w)
    hi = ws.to(torch.float16)
    planes = torch.stack([hi, (ws - hi.float()).to(torch.float16)])          # [2][GJ][K]
    q = planes.reshape(2, GJ // J, J // 16, 16, K // 32, 4, 8)               # [pl][g][strip][col][t][kg][e]
    out = q.permute(1, 4, 2, 0, 5, 3, 6).contiguous().reshape(-1)            # [g][t][strip][pl][kg][col][e]
    out.wsc = wsc
    return out


def permute_weight_frag_grouped(w, J=128):
    """[G*J, K] -> the weight operand of linear_relu_dot: two fp16 planes (lrd_weight_split_f16; round 5) where the weight-stationary kernel covers the
    shape, else the three bf16 planes (lrd_weight_split; int16), else the fp32 fragment order [G][K/16][J/16][64][4] of etch_linear_relu_dot."""
    GJ, K = w.shape
    if LRD_SPLIT and LRD_F16 and J == 128 and K in (32, 64, 128) and (GJ // J == 1 or GJ // J >= 8):
        return lrd_weight_split_f16(w.contiguous(), J)
    if LRD_SPLIT and J == 128 and K in (32, 64, 128, 256):
        return lrd_weight_split(w.contiguous(), J)
    return torch.cat([permute_weight_frag(w[g * J:(g + 1) * J].contiguous()) for g in range(GJ // J)])


def linear_relu_dot(x, w, b1, w2, b2, G, wp=None, out=None):
    """out[r,g] = b2[g] + sum_j relu(x[r] . w[g*J+j] + b1[g*J+j]) * w2[g*J+j]   (J = 128), hidden kept on chip."""
    for t, n in ((w, "w"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        _need(t, torch.float32, n)
    if x.dtype != torch.float32 or not x.is_cuda:
        raise _lib.EtchHipError("x must be a float32 CUDA(HIP) tensor")
    R, K = x.shape
    J = w.shape[0] // G
    assert x.stride(1) == 1 and w.shape == (G * J, K) and b1.numel() == G * J and w2.numel() == G * J and b2.numel() == G
    if out is None:
        out = torch.empty((R, G), dtype=torch.float32, device=x.device)
    else:
        _lib.wrote(out)
    if wp is not None and wp.dtype == torch.float16 and (b1.data_ptr() | w2.data_ptr()) % 16 == 0:
        _lib.call("etch_linear_relu_dot_f16", R, int(K), int(G), int(J), x, x.stride(0) if R > 1 else K, wp, wp.wsc, b1, w2, b2, out,
                  out.stride(0) if R > 1 else G)
        return out
    if wp is not None and wp.dtype == torch.float16:
        wp = None                                  # (a bias / w2 view off the 16-byte grid: the fp32 kernel below)
    if wp is not None and wp.dtype == torch.int16:
        _lib.call("etch_linear_relu_dot_split", R, int(K), int(G), int(J), x, x.stride(0) if R > 1 else K, wp, b1, w2, b2, out, out.stride(0) if R > 1 else G)
        return out
    _lib.call("etch_linear_relu_dot", R, int(K), int(G), int(J), x, x.stride(0) if R > 1 else K, w, w.stride(0), wp, b1, w2, b2, out,
              out.stride(0) if R > 1 else G)
    return out


def softmax_dot(logits, v):
    R, G = logits.shape
    out = torch.empty((R,), dtype=torch.float32, device=logits.device)
    _lib.call("etch_softmax_dot", R, G, logits, v, out)
    return out


# ------------------------------------------------------------------ stage 2
def argmax_rows(logits):
    """(..., G) float32 -> (...) int64, first maximum (torch.max semantics: -0 == +0, any NaN greatest, the first NaN wins)."""
    _need(logits, torch.float32, "logits")
    G = logits.shape[-1]
    R = logits.numel() // G
    out = torch.empty(logits.shape[:-1], dtype=torch.int64, device=logits.device)
    _lib.call("etch_argmax_rows", R, G, logits, out)
    return out


def get_markers(points, labels, conf, num_markers):
    _need(points, torch.float32, "points"), _need(labels, torch.int64, "labels"), _need(conf, torch.float32, "conf")
    B, K = labels.shape
    markers = torch.empty((B, num_markers, 3), dtype=torch.float32, device=points.device)
    valid_f = torch.empty((B, num_markers), dtype=torch.float32, device=points.device)
    valid_b = torch.empty((B, num_markers), dtype=torch.bool, device=points.device)
    _lib.call("etch_get_markers", B, K, num_markers, points, labels, conf, markers, valid_f, valid_b)
    return markers, valid_f, valid_b


def marker_select(labels, conf, num_markers):
    """The selection half of get_markers: labels (B,K) int64, conf (B,K,1) -> sel (B,M,3) int32 = global point rows b*K + i of each label's
    top-3 confidences in rank order (-1 beyond cnt), cnt (B,M) int32 = min(points carrying the label, 3)."""
    _need(labels, torch.int64, "labels"), _need(conf, torch.float32, "conf")
    B, K = labels.shape
    assert conf.numel() == B * K
    sel = torch.empty((B, num_markers, 3), dtype=torch.int32, device=labels.device)
    cnt = torch.empty((B, num_markers), dtype=torch.int32, device=labels.device)
    _lib.call("etch_marker_select", B, K, num_markers, labels, conf, sel, cnt)
    return sel, cnt


def markers_from_selected(sel, cnt, points, conf, magnitude, scale, direction):
    """The other half: direction (B*M*3, 3) = the direction at every slot of sel -> (markers (B,M,3), valid_f, valid_b), bitwise
    get_markers(inner_points(points, dense direction, magnitude, scale), labels, conf, M)."""
    _need(sel, torch.int32, "sel"), _need(cnt, torch.int32, "cnt")
    for t, n in ((points, "points"), (conf, "conf"), (magnitude, "magnitude"), (direction, "direction")):
        _need(t, torch.float32, n)
    B, M, _ = sel.shape
    K = points.shape[1]
    assert points.shape == (B, K, 3) and conf.numel() == B * K and magnitude.numel() == B * K and direction.numel() == B * M * 9 and cnt.shape == (B, M)
    markers = torch.empty((B, M, 3), dtype=torch.float32, device=points.device)
    valid_f = torch.empty((B, M), dtype=torch.float32, device=points.device)
    valid_b = torch.empty((B, M), dtype=torch.bool, device=points.device)
    _lib.call("etch_markers_from_selected", B, K, M, sel, cnt, points, conf, magnitude, float(scale), direction, markers, valid_f, valid_b)
    return markers, valid_f, valid_b


LM_SPLIT_MAX_BATCH = 8     # scans per launch up to which a scan's linearisation is split over several workgroups (latency regime)
LM_SPLIT_WGS = 3           # SMPL: 3 marker chunks of 32 -> 3 workgroups (measured: 6.4 -> 5.2 ms per 30+50 fit; 4+ only add exchange cost)
LM_SPLIT_WGS_BY_JOINTS = {55: 4}      # SMPL-X-sized: 10 chunks of 9 markers; 58 -> 45.6 ms per 75+125 fit at B = 8 (G = 5: 42.5 ms at B = 1)


def lm_split_default(B, nj):
    return LM_SPLIT_WGS_BY_JOINTS.get(int(nj), LM_SPLIT_WGS) if B <= LM_SPLIT_MAX_BATCH else 1


def _lm_dof_arg(t, name, B, dof, like):
    """Host-side checks of an optional (B, DOF) input of the LM fit: no launch happens before they pass."""
    if not isinstance(t, torch.Tensor):
        raise _lib.EtchHipError(f"{name} must be a tensor of shape ({B}, {dof})")
    if tuple(t.shape) != (B, dof):
        raise _lib.EtchHipError(f"{name} must have shape ({B}, {dof}), got {tuple(t.shape)}")
    if t.dtype != torch.float32 or t.device != like.device or not t.is_contiguous():
        raise _lib.EtchHipError(f"{name} must be a contiguous float32 tensor on {like.device}")
    return t


POSE_PRIOR_MAX_G, POSE_PRIOR_MAX_ANG, POSE_PRIOR_MAX_D = 16, 8, 162


class PosePrior:
    """Device tables of the fits' pose prior, built ONCE: a max-mixture GMM min_k [0.5 d_k^T P_k d_k - log c_k] on x[:D] with weight
    w_gmm (means (G, D), precisions (G, D, D), nll_weights (G) = MaxMixturePrior's buffers; all three None: no GMM) and joint-angle terms
    w_ang sum_t exp(2 s_t x[a_t]) (angle_idx into the body pose WITHOUT the global orientation, angle_sign; both None: none).
    The constructor does every value check, on host copies of the tables (the only place this object synchronises): finite tables, nll_weights > 0, weights >= 0, every
    symmetrised precision positive definite (an indefinite one can make the damped normal matrix indefinite, and the kernel's Cholesky then yields
    NaN silently).  The precisions are stored symmetrised, 0.5 (P + P^T) formed in fp64 and rounded to fp32.  Calls that take the object only
    check shapes and the device, and never synchronise."""
    __slots__ = ("means", "precisions", "nll_weights", "angle_idx", "angle_sign", "G", "D", "n_ang", "w_gmm", "w_ang", "max_angle_idx", "device",
                 "_tables", "_frozen")

    def __init__(self, means=None, precisions=None, nll_weights=None, w_gmm=0.0, angle_idx=None, angle_sign=None, w_ang=0.0, device="cuda"):
        err = _lib.EtchHipError
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        w_gmm, w_ang = float(w_gmm), float(w_ang)
        if not (math.isfinite(w_gmm) and math.isfinite(w_ang) and w_gmm >= 0.0 and w_ang >= 0.0):
            raise err("PosePrior: w_gmm and w_ang must be finite and >= 0")
        gmm = [means, precisions, nll_weights]
        if any(t is None for t in gmm) and not all(t is None for t in gmm):
            raise err("PosePrior: means, precisions and nll_weights come together")
        if (angle_idx is None) != (angle_sign is None):
            raise err("PosePrior: angle_idx and angle_sign come together")
        if means is None and angle_idx is None:
            raise err("PosePrior: neither a mixture nor angle terms")
        host64 = lambda t: torch.as_tensor(t).detach().to("cpu", torch.float64)
        G = D = 0
        m32 = p32 = c32 = None
        if means is not None:
            m, P, c = host64(means), host64(precisions), host64(nll_weights).reshape(-1)
            if m.dim() != 2 or P.dim() != 3:
                raise err(f"PosePrior: means must be (G, D) and precisions (G, D, D), got {tuple(m.shape)} and {tuple(P.shape)}")
            G, D = m.shape
            if not 1 <= G <= POSE_PRIOR_MAX_G or not 1 <= D <= POSE_PRIOR_MAX_D:
                raise err(f"PosePrior: 1 <= G <= {POSE_PRIOR_MAX_G} and 1 <= D <= {POSE_PRIOR_MAX_D}, got G = {G}, D = {D}")
            if tuple(P.shape) != (G, D, D) or c.numel() != G:
                raise err(f"PosePrior: precisions must be ({G}, {D}, {D}) and nll_weights ({G}), got {tuple(P.shape)} and {tuple(c.shape)}")
            if not (torch.isfinite(m).all() and torch.isfinite(P).all() and torch.isfinite(c).all()):
                raise err("PosePrior: means, precisions and nll_weights must be finite")
            if not (c > 0).all():
                raise err("PosePrior: nll_weights must be > 0")
            p32 = (0.5 * (P + P.transpose(1, 2))).to(torch.float32)
            if not (torch.linalg.cholesky_ex(p32.double()).info == 0).all():
                raise err("PosePrior: every (symmetrised) precision matrix must be positive definite")
            m32, c32 = m.to(torch.float32), c.to(torch.float32)
            if not (c32 > 0).all():
                raise err("PosePrior: nll_weights underflow in float32")
        n_ang, amax, ai, asg = 0, -1, None, None
        if angle_idx is not None:
            ai64 = torch.as_tensor(angle_idx).detach().to("cpu")
            if ai64.dtype.is_floating_point or ai64.dtype == torch.bool:
                raise err("PosePrior: angle_idx must be integers")
            ai64, asg64 = ai64.reshape(-1).long(), host64(angle_sign).reshape(-1)
            n_ang = ai64.numel()
            if not 1 <= n_ang <= POSE_PRIOR_MAX_ANG or asg64.numel() != n_ang:
                raise err(f"PosePrior: 1 <= n_ang <= {POSE_PRIOR_MAX_ANG} indices with as many signs, got {n_ang} and {asg64.numel()}")
            if int(ai64.min()) < 0 or not torch.isfinite(asg64).all():
                raise err("PosePrior: angle indices must be >= 0 and the signs finite")
            amax = int(ai64.max())
            ai, asg = ai64.to(torch.int32), asg64.to(torch.float32)
        put = lambda t: None if t is None else t.contiguous().to(dev)
        object.__setattr__(self, "_frozen", False)
        self.means, self.precisions, self.nll_weights, self.angle_idx, self.angle_sign = put(m32), put(p32), put(c32), put(ai), put(asg)
        self.G, self.D, self.n_ang, self.w_gmm, self.w_ang, self.max_angle_idx, self.device = int(G), int(D), int(n_ang), w_gmm, w_ang, amax, dev
        self._tables = (ctypes.c_void_p * 5)(*[None if t is None else t.data_ptr()
                                               for t in (self.means, self.precisions, self.nll_weights, self.angle_idx, self.angle_sign)])
        self._frozen = True

    def __setattr__(self, name, value):
        if getattr(self, "_frozen", False):
            raise AttributeError("PosePrior is immutable: build a new one")
        object.__setattr__(self, name, value)


def _pose_prior_arg(pp, like, npose, what, need_gmm=False):
    """Per-call checks of a PosePrior: type, device, sizes against the model.  Host-side only."""
    if not isinstance(pp, PosePrior):
        raise _lib.EtchHipError(f"{what}: pose_prior must be an ops.PosePrior")
    if pp.device != like.device:
        raise _lib.EtchHipError(f"{what}: pose_prior lives on {pp.device}, the fit on {like.device}")
    if need_gmm and pp.G == 0:
        raise _lib.EtchHipError(f"{what}: pose_prior has no mixture")
    if pp.D > npose:
        raise _lib.EtchHipError(f"{what}: the prior's dimension {pp.D} exceeds the model's {npose} pose variables")
    if pp.max_angle_idx >= npose:
        raise _lib.EtchHipError(f"{what}: angle index {pp.max_angle_idx} is outside the model's {npose} pose variables")
    return pp


def pose_prior_eval(pose, pose_prior):
    """The max-mixture bracket as the fit kernels evaluate it: pose (B, D) fp32 -> value (B) fp64 = min_k [0.5 d_k^T P_k d_k - log c_k],
    component (B) int32 (ties: the lowest index), gradient P_k* d_k* (B, D) fp64."""
    _need(pose, torch.float32, "pose")
    _pose_prior_arg(pose_prior, pose, POSE_PRIOR_MAX_D, "pose_prior_eval", need_gmm=True)
    if pose.dim() != 2 or pose.shape[1] != pose_prior.D:
        raise _lib.EtchHipError(f"pose must be (B, {pose_prior.D}), got {tuple(pose.shape)}")
    B = pose.shape[0]
    val = torch.empty((B,), dtype=torch.float64, device=pose.device)
    comp = torch.empty((B,), dtype=torch.int32, device=pose.device)
    grad = torch.empty((B, pose_prior.D), dtype=torch.float64, device=pose.device)
    _lib.call("etch_pose_prior_eval", B, pose_prior._tables, pose_prior.G, pose_prior.D, pose, val, comp, grad)
    return val, comp, grad


def smpl_lm_fit(consts, markers, valid_f, it0, step0, damp0, it1, step1, damp1, want_trace=False, phase_ticks=None, nj=24, nb=10, split=None,
                x_init=None, prior=None, check=True, pose_prior=None):
    """x (B, 3 nj + nb + 3) = pose | betas | orient | transl.  (nj, nb) = (24, 10) SMPL or (55, 20) SMPL-X-sized.
    split = workgroups per scan (None: lm_split_default -- 3 / 4 when B <= LM_SPLIT_MAX_BATCH, else one persistent workgroup per scan).
    x_init (B, DOF): the starting point instead of 0 (stage 0 still evaluates with betas[2:] = 0 and hands them to stage 1 unchanged).
    prior = (mean, weight), both (B, DOF), weight >= 0: adds 0.5 sum_i w_i (x_i - mean_i)^2 over each stage's active variables to the
    objective; the trace then holds the full objective.  check=True (the default) rejects negative or non-finite weights and non-finite
    means / x_init: ONE device-to-host read that synchronises the stream -- pass check=False on a pipelined path that guarantees them itself.
    pose_prior: an ops.PosePrior (max-mixture GMM on the pose and / or joint-angle terms), added like the diagonal prior; its values
    were checked when it was built, so this adds no synchronisation.
    With x_init, prior and pose_prior all None this is the call it always was (etch_smpl_lm_fit_split)."""
    B, M = valid_f.shape
    dof = 3 * nj + nb + 3
    if pose_prior is not None:
        _pose_prior_arg(pose_prior, markers, 3 * (nj - 1), "smpl_lm_fit")
    if prior is not None:
        if not isinstance(prior, (tuple, list)) or len(prior) != 2 or prior[0] is None or prior[1] is None:
            raise _lib.EtchHipError("prior must be (mean, weight): a mean without a weight (or the reverse) is not a prior")
        _lm_dof_arg(prior[0], "prior mean", B, dof, markers), _lm_dof_arg(prior[1], "prior weight", B, dof, markers)
    if x_init is not None:
        _lm_dof_arg(x_init, "x_init", B, dof, markers)
    if check and (prior is not None or x_init is not None):
        bad = torch.zeros((), dtype=torch.bool, device=markers.device)
        if prior is not None:
            bad = bad | ~torch.isfinite(prior[0]).all() | ~(torch.isfinite(prior[1]) & (prior[1] >= 0)).all()
        if x_init is not None:
            bad = bad | ~torch.isfinite(x_init).all()
        if bool(bad):           # synchronises
            raise _lib.EtchHipError("smpl_lm_fit: prior weights must be finite and >= 0, prior means and x_init finite")
    arr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in consts])
    x = torch.empty((B, dof), dtype=torch.float32, device=markers.device)
    x0 = torch.empty((B, dof), dtype=torch.float32, device=markers.device)
    tr = torch.zeros((B, it0 + it1 + 2), dtype=torch.float32, device=markers.device) if want_trace else None
    G = int(split) if split is not None else lm_split_default(B, nj)
    if G > 1 and B * G > torch.cuda.get_device_properties(markers.device).multi_processor_count:
        G = 1           # the workgroups of a scan wait for each other: on a small part / CU partition one persistent workgroup per scan (same results up to summation order)
    ws = None
    if G > 1:
        nbytes = _lib.call("etch_smpl_lm_split_workspace_bytes", B, int(nj), int(nb), G)
        ws = torch.empty((nbytes // 8 + 1,), dtype=torch.float64, device=markers.device)
    if pose_prior is not None:
        mean, weight = prior if prior is not None else (None, None)
        pp = pose_prior
        _lib.call("etch_smpl_lm_fit_pose_prior", B, M, int(nj), int(nb), arr, markers, valid_f, int(it0), float(step0), float(damp0), int(it1), float(step1),
                  float(damp1), x, x0, tr, phase_ticks, G, ws, x_init, mean, weight, pp._tables, pp.G, pp.D, pp.n_ang, float(pp.w_gmm), float(pp.w_ang))
    elif x_init is None and prior is None:
        _lib.call("etch_smpl_lm_fit_split", B, M, int(nj), int(nb), arr, markers, valid_f, int(it0), float(step0), float(damp0), int(it1), float(step1),
                  float(damp1), x, x0, tr, phase_ticks, G, ws)
    else:
        mean, weight = prior if prior is not None else (None, None)
        _lib.call("etch_smpl_lm_fit_prior", B, M, int(nj), int(nb), arr, markers, valid_f, int(it0), float(step0), float(damp0), int(it1), float(step1),
                  float(damp1), x, x0, tr, phase_ticks, G, ws, x_init, mean, weight)
    x._etch_split_ws = ws       # the split fit's workspace carries the per-scan give-up flags (smpl_lm_split_failed); None for one workgroup per scan
    return x, x0, tr


def smpl_lm_split_failed(x):
    """Number of scans of a split LM fit that were abandoned because a partner workgroup never arrived (their rows of `x` are NaN).  `x` = the
    first tensor smpl_lm_fit returned.  Synchronises the current stream."""
    ws = getattr(x, "_etch_split_ws", None)
    if ws is None:
        return 0
    n = ctypes.c_int(0)
    _lib.call("etch_smpl_lm_split_failed", int(x.shape[0]), ws, ctypes.byref(n))
    return int(n.value)


def smpl_adam_fit(consts, markers, valid_f, it0, it1, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, want_trace=False, nj=24, nb=10,
                  pose_prior=None, pose_prior_w=1e-7, mean_shape_w=0.0):
    """First-order fitter (fit_SMPL_Adam.py): -> x (B,DOF), x_last (parameters of the last forward pass), loss trace (B, it0+it1) or None.
    pose_prior (an ops.PosePrior with a mixture; its own weights are not used here) adds pose_prior_w * sum_b min_k [.] to the loss and
    mean_shape_w adds mean_shape_w * mean(active betas^2): the reference's use_pose_prior / use_mean_shape (1e-7, 1e-2).  There are no angle terms."""
    B, M = valid_f.shape
    dof = 3 * nj + nb + 3
    pose_prior_w, mean_shape_w = float(pose_prior_w), float(mean_shape_w)
    if pose_prior is not None:
        _pose_prior_arg(pose_prior, markers, 3 * (nj - 1), "smpl_adam_fit", need_gmm=True)
    if not (math.isfinite(pose_prior_w) and math.isfinite(mean_shape_w) and pose_prior_w >= 0.0 and mean_shape_w >= 0.0):
        raise _lib.EtchHipError("smpl_adam_fit: pose_prior_w and mean_shape_w must be finite and >= 0")
    arr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in consts])
    x = torch.empty((B, dof), dtype=torch.float32, device=markers.device)
    xl = torch.empty((B, dof), dtype=torch.float32, device=markers.device)
    tr = torch.zeros((B, it0 + it1), dtype=torch.float32, device=markers.device) if want_trace else None
    if pose_prior is not None or mean_shape_w != 0.0:
        pp = pose_prior
        _lib.call("etch_smpl_adam_fit_prior", B, M, int(nj), int(nb), arr, markers, valid_f, int(it0), int(it1), float(lr), float(beta1), float(beta2),
                  float(eps), x, xl, tr, pp._tables if pp is not None else None, pp.G if pp is not None else 0, pp.D if pp is not None else 0,
                  float(pose_prior_w), float(mean_shape_w))
        return x, xl, tr
    _lib.call("etch_smpl_adam_fit", B, M, int(nj), int(nb), arr, markers, valid_f, int(it0), int(it1), float(lr), float(beta1), float(beta2), float(eps), x, xl,
              tr)
    return x, xl, tr


def marker_status(markers, valid_f):
    """(B,) int32: bit 0 = a valid marker is non-finite (the fit of that scan is NaN, as in the reference), bit 1 = no valid marker."""
    B, M = valid_f.shape
    st = torch.empty((B,), dtype=torch.int32, device=markers.device)
    _lib.call("etch_marker_status", B, M, markers, valid_f, st)
    return st


def smpl_lm_linearize(consts, x, markers, valid_f, nb_active, nj=24, nb=10, want_normal=False):
    """Diagnostics: residual (B,3M), analytic Jacobian (B,3M,DOF) and optionally the matrix-core normal equations (B,DOF+1,DOF+1) fp64."""
    B, M = valid_f.shape
    dof = 3 * nj + nb + 3
    assert x.shape == (B, dof)
    arr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in consts])
    r = torch.empty((B, 3 * M), dtype=torch.float32, device=x.device)
    J = torch.empty((B, 3 * M, dof), dtype=torch.float32, device=x.device)
    N = torch.empty((B, dof + 1, dof + 1), dtype=torch.float64, device=x.device) if want_normal else None
    _lib.call("etch_smpl_lm_linearize", B, M, int(nj), int(nb), int(nb_active), arr, x, markers, valid_f, r, J, N)
    return (r, J, N) if want_normal else (r, J)


def rodrigues(theta):
    """theta (n,3) fp32 -> R (n,3,3) fp64, dR (n,3,3,3) with dR[n,q] = dR/dtheta_q."""
    _need(theta, torch.float32, "theta")
    n = theta.shape[0]
    R = torch.empty((n, 3, 3), dtype=torch.float64, device=theta.device)
    dR = torch.empty((n, 3, 3, 3), dtype=torch.float32, device=theta.device)
    _lib.call("etch_rodrigues", n, theta, R, dR)
    return R, dR


def smpl_lbs(consts, x, V, n_extra, nj=24, nb=10):
    B = x.shape[0]
    assert x.shape[1] == 3 * nj + nb + 3
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    verts = torch.empty((B, V, 3), dtype=torch.float32, device=x.device)
    joints = torch.empty((B, nj + n_extra, 3), dtype=torch.float32, device=x.device)
    _lib.call("etch_smpl_lbs", B, V, int(nj), int(nb), n_extra, arr, x, verts, joints)
    return verts, joints


def inner_points(points, direction, magnitude, scale):
    _need(points, torch.float32, "points"), _need(direction, torch.float32, "direction"), _need(magnitude, torch.float32, "magnitude")
    out = torch.empty_like(points)
    n = points.numel() // 3
    _lib.call("etch_inner_points", n, points, direction, magnitude, float(scale), out)
    return out


# ------------------------------------------------------------------ chamfer refinement (csrc/chamfer_fit.hip)
def _lengths(len_t, B, n, device, name):
    if len_t is None:
        return None
    t = torch.as_tensor(len_t, device=device).to(torch.int32).contiguous()
    if t.shape != (B,):
        raise _lib.EtchHipError(f"{name} must have shape ({B},), got {tuple(t.shape)}")
    return t


def nn_bidir(x, y, x_lengths=None, y_lengths=None):
    """Exact nearest neighbours both ways: x (B,N,3), y (B,V,3) fp32 -> idx_xy (B,N) int32, d_xy (B,N), idx_yx (B,V) int32, d_yx (B,V).
    d = the bit-defined fp32 ((dx*dx)+(dy*dy))+(dz*dz) of the returned pair; exact ties -> the lowest index; padding -> index -1, distance 0."""
    _need(x, torch.float32, "x"), _need(y, torch.float32, "y")
    if x.dim() != 3 or y.dim() != 3 or y.shape[0] != x.shape[0] or x.shape[2] != 3 or y.shape[2] != 3:
        raise _lib.EtchHipError(f"x and y must be (B,N,3) and (B,V,3), got {tuple(x.shape)} and {tuple(y.shape)}")
    B, N, _ = x.shape
    V = y.shape[1]
    xl, yl = _lengths(x_lengths, B, N, x.device, "x_lengths"), _lengths(y_lengths, B, V, x.device, "y_lengths")
    ws = torch.empty((max(B * (N + V), 1),), dtype=torch.int64, device=x.device)
    ixy = torch.empty((B, N), dtype=torch.int32, device=x.device)
    dxy = torch.empty((B, N), dtype=torch.float32, device=x.device)
    iyx = torch.empty((B, V), dtype=torch.int32, device=x.device)
    dyx = torch.empty((B, V), dtype=torch.float32, device=x.device)
    _lib.call("etch_nn_bidir", B, N, V, x, y, xl, yl, ws, ixy, dxy, iyx, dyx)
    return ixy, dxy, iyx, dyx


def chamfer_grad(x, y, idx_xy, idx_yx, w_xy=None, w_yx=None, x_lengths=None, y_lengths=None, want_x=True, want_y=True):
    """Gradient of sum_b [w_xy[b] sum_i d_xy + w_yx[b] sum_j d_yx] (neighbours held fixed) -> (gx (B,N,3) or None, gy (B,V,3) or None)."""
    _need(x, torch.float32, "x"), _need(y, torch.float32, "y")
    if x.dim() != 3 or y.dim() != 3 or y.shape[0] != x.shape[0] or x.shape[2] != 3 or y.shape[2] != 3:
        raise _lib.EtchHipError("chamfer_grad: x (B,N,3), y (B,V,3), idx_xy (B,N), idx_yx (B,V)")
    B, N, _ = x.shape
    V = y.shape[1]
    if tuple(idx_xy.shape) != (B, N) or tuple(idx_yx.shape) != (B, V):
        raise _lib.EtchHipError("chamfer_grad: x (B,N,3), y (B,V,3), idx_xy (B,N), idx_yx (B,V)")
    for w, n in ((w_xy, "w_xy"), (w_yx, "w_yx")):
        if w is not None and tuple(w.shape) != (B,):
            raise _lib.EtchHipError(f"{n} must be ({B},)")
    xl, yl = _lengths(x_lengths, B, N, x.device, "x_lengths"), _lengths(y_lengths, B, V, x.device, "y_lengths")
    w_xy = None if w_xy is None else _need(w_xy.to(torch.float32).contiguous(), torch.float32, "w_xy")
    w_yx = None if w_yx is None else _need(w_yx.to(torch.float32).contiguous(), torch.float32, "w_yx")
    ws = torch.empty((max(3 * B * (N + V), 1),), dtype=torch.int64, device=x.device)
    gx = torch.empty_like(x) if want_x else None
    gy = torch.empty_like(y) if want_y else None
    _lib.call("etch_chamfer_grad", B, N, V, x, y, xl, yl, _need(idx_xy, torch.int32, "idx_xy"), _need(idx_yx, torch.int32, "idx_yx"), w_xy, w_yx, ws, gx, gy)
    return gx, gy


def _check_body(consts, nj, nb, n_extra):
    """The 8 LBS tables (v_template, shapedirs, posedirs, weights, J0, Jd, parents, extra_vids) must match (nj, nb, n_extra)."""
    if len(consts) != 8 or tuple(consts[1].shape[1:]) != (3, nb) or tuple(consts[4].shape) != (nj, 3) or consts[7].numel() != n_extra:
        raise _lib.EtchHipError(f"body tables do not match nj={nj}, nb={nb}, n_extra={n_extra}")


def _refine_workspace(B, N, V, nj, nb, n_extra, device):
    n = ctypes.c_longlong(0)
    _lib.call("etch_smpl_chamfer_refine_workspace", B, N, V, int(nj), int(nb), int(n_extra), ctypes.byref(n))
    return torch.empty((max(int(n.value), 8),), dtype=torch.uint8, device=device)


def smpl_lbs_vjp(consts, params, g, nj=24, nb=10, n_extra=21):
    """params (B, 3 nj + nb + 4) = pose (global orient first) | beta | trans | scale; g (B,V,3) = dL/dverts of
    verts = (LBS(pose, beta) + trans) * scale  ->  dL/dparams (B, 3 nj + nb + 4)."""
    _need(params, torch.float32, "params"), _need(g, torch.float32, "g")
    _check_body(consts, nj, nb, n_extra)
    if g.dim() != 3 or g.shape[2] != 3 or g.shape[1] != consts[0].shape[0] or tuple(params.shape) != (g.shape[0], 3 * nj + nb + 4):
        raise _lib.EtchHipError(f"params must be (B, {3 * nj + nb + 4}) and g (B, {consts[0].shape[0]}, 3)")
    B, V = g.shape[0], g.shape[1]
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    ws = _refine_workspace(B, 0, V, nj, nb, n_extra, g.device)
    grad = torch.empty_like(params)
    _lib.call("etch_smpl_lbs_vjp", B, V, int(nj), int(nb), int(n_extra), arr, params, g, ws, grad)
    return grad


def smpl_chamfer_refine(consts, scan, params, V, scan_lengths=None, prior=None, bidir=0, iters=500, lr=2e-2, beta1=0.9, beta2=0.999, eps=1e-8,
                        nj=24, nb=10, n_extra=21, want_trace=False):
    """fit_cham on the device: params (B, 3 nj + nb + 4) is updated IN PLACE.  prior = None or (means (G,69), precisions (G,69,69),
    nll_weights (G)) fp32 device tensors.  -> verts (B,V,3), joints (B, nj + n_extra, 3) (without trans / scale), loss of the last forward (B,),
    loss trace (B, iters) or None."""
    _need(scan, torch.float32, "scan"), _need(params, torch.float32, "params")
    _check_body(consts, nj, nb, n_extra)
    if scan.dim() != 3 or scan.shape[2] != 3 or tuple(params.shape) != (scan.shape[0], 3 * nj + nb + 4) or int(V) != consts[0].shape[0]:
        raise _lib.EtchHipError(f"scan must be (B,N,3), params (B, {3 * nj + nb + 4}), V = the model's {consts[0].shape[0]} vertices")
    B, N, _ = scan.shape
    sl = _lengths(scan_lengths, B, N, scan.device, "scan_lengths")
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    G, parr = 0, None
    if prior is not None:
        means, prec, w = (_need(t, torch.float32, n) for t, n in zip(prior, ("means", "precisions", "nll_weights")))
        G = int(w.shape[0])
        if tuple(w.shape) != (G,) or tuple(means.shape) != (G, 69) or tuple(prec.shape) != (G, 69, 69):
            raise _lib.EtchHipError("prior: means (G,69), precisions (G,69,69), nll_weights (G,)")
        parr = (ctypes.c_void_p * 3)(means.data_ptr(), prec.data_ptr(), w.data_ptr())
    ws = _refine_workspace(B, N, V, nj, nb, n_extra, scan.device)
    verts = torch.empty((B, V, 3), dtype=torch.float32, device=scan.device)
    joints = torch.empty((B, nj + n_extra, 3), dtype=torch.float32, device=scan.device)
    loss = torch.empty((B,), dtype=torch.float32, device=scan.device)
    tr = torch.empty((B, iters), dtype=torch.float32, device=scan.device) if want_trace else None
    _lib.call("etch_smpl_chamfer_refine", B, N, int(V), int(nj), int(nb), int(n_extra), arr, scan, sl, parr, G, int(bidir), int(iters), float(lr), float(beta1),
              float(beta2), float(eps), params, verts, joints, tr, loss, ws)
    _lib.wrote(params)
    return verts, joints, loss, tr


# ------------------------------------------------------------------ dense surface refinement (csrc/surface_fit.hip)
def _byte_workspace(name, device, *dims):
    n = ctypes.c_longlong(0)
    _lib.call(name, *dims, ctypes.byref(n))
    return torch.empty((max(int(n.value), 8),), dtype=torch.uint8, device=device)


def _mesh_args(points, verts, faces, what):
    _need(points, torch.float32, "points"), _need(verts, torch.float32, "verts"), _need(faces, torch.int32, "faces")
    if points.dim() != 3 or verts.dim() != 3 or points.shape[2] != 3 or verts.shape[2] != 3 or verts.shape[0] != points.shape[0] or faces.dim() != 2 \
            or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"{what}: points (B,N,3), verts (B,V,3), faces (F,3), got {tuple(points.shape)}, {tuple(verts.shape)}, {tuple(faces.shape)}")
    return points.shape[0], points.shape[1], verts.shape[1], faces.shape[0]


def point_mesh_closest(points, verts, faces, lengths=None):
    """Exact closest point of mesh b (verts (B,V,3) fp32, faces (F,3) int32 shared by the batch) to points (B,N,3) fp32 (lengths (B,) for
    ragged point sets) -> face (B,N) int32, bary (B,N,3), d2 (B,N): Ericson's region test in fp32, every pair; the smallest d2 wins, equal
    d2 -> the lowest face, NaN never wins; padding -> face -1, bary 0, d2 0."""
    B, N, V, F = _mesh_args(points, verts, faces, "point_mesh_closest")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    ws = _byte_workspace("etch_point_mesh_closest_workspace", points.device, B, N)
    face = torch.empty((B, N), dtype=torch.int32, device=points.device)
    bary = torch.empty((B, N, 3), dtype=torch.float32, device=points.device)
    d2 = torch.empty((B, N), dtype=torch.float32, device=points.device)
    _lib.call("etch_point_mesh_closest", B, N, V, F, points, nl, verts, faces, ws, face, bary, d2)
    return face, bary, d2


def _marker_args(markers, B, V, device):
    """markers = None or (vids (M,) int, positions (B,M,3), valid (B,M)) -> (M, vids int32, positions fp32, valid fp32) device tensors."""
    if markers is None:
        return 0, None, None, None
    vids, pos, valid = markers
    vids = torch.as_tensor(vids).to(device=device, dtype=torch.int32).contiguous()
    M = int(vids.numel())
    pos = _need(torch.as_tensor(pos).to(device=device, dtype=torch.float32).contiguous(), torch.float32, "markers")
    valid = torch.as_tensor(valid).to(device=device, dtype=torch.float32).contiguous()
    if vids.dim() != 1 or tuple(pos.shape) != (B, M, 3) or tuple(valid.shape) != (B, M):
        raise _lib.EtchHipError(f"markers: vids (M,), positions ({B},M,3), valid ({B},M)")
    if M and (int(vids.min()) < 0 or int(vids.max()) >= V):
        raise _lib.EtchHipError(f"marker vertex ids must lie in [0, {V})")
    return M, vids, pos, valid


def point_mesh_energy_grad(points, verts, faces, face, bary, d2, weights=None, trunc=-1.0, lengths=None, coef=None, w_dense=1.0, normalize=True,
                           markers=None, w_marker=1.0, want_verts=True, want_points=False):
    """The dense term on the correspondences of point_mesh_closest (held fixed): terms (B,2) fp64 = {sum w m d2, sum w m} with m = [d2 <=
    trunc^2] (trunc < 0: no mask), g (B,V,3) = d/dverts of coef_b w_dense S1 / S0 (normalize) or coef_b w_dense S1, plus the marker term's
    gradient for markers = (vids, positions, valid); gp (B,N,3) = the dense term's gradient w.r.t. the points.  -> (terms, g or None, gp or None)."""
    B, N, V, F = _mesh_args(points, verts, faces, "point_mesh_energy_grad")
    if tuple(face.shape) != (B, N) or tuple(bary.shape) != (B, N, 3) or tuple(d2.shape) != (B, N):
        raise _lib.EtchHipError(f"point_mesh_energy_grad: face ({B},{N}), bary ({B},{N},3), d2 ({B},{N})")
    _need(face, torch.int32, "face"), _need(bary, torch.float32, "bary"), _need(d2, torch.float32, "d2")
    if weights is not None:
        weights = _need(weights.to(torch.float32).contiguous(), torch.float32, "weights")
        if tuple(weights.shape) != (B, N):
            raise _lib.EtchHipError(f"weights must be ({B},{N})")
    if coef is not None:
        coef = _need(coef.to(torch.float32).contiguous(), torch.float32, "coef")
        if tuple(coef.shape) != (B,):
            raise _lib.EtchHipError(f"coef must be ({B},)")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    M, vids, pos, valid = _marker_args(markers, B, V, points.device)
    ws = _byte_workspace("etch_point_mesh_energy_grad_workspace", points.device, B, V)
    terms = torch.zeros((B, 2), dtype=torch.float64, device=points.device)
    g = torch.empty_like(verts) if want_verts else None
    gp = torch.empty_like(points) if want_points else None
    _lib.call("etch_point_mesh_energy_grad", B, N, V, F, points, nl, verts, faces, face, bary, d2, weights, float(trunc), coef, float(w_dense), int(bool(normalize)),
              M, vids, pos, valid, float(w_marker), ws, terms, g, gp)
    return terms, g, gp


def smpl_surface_refine(consts, faces, points, params, lengths=None, weights=None, markers=None, prior=None, iters=200, lr=2e-2, beta1=0.9, beta2=0.999,
                        eps=1e-8, w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05, optimize_scale=False, nj=24, nb=10, n_extra=21,
                        want_trace=False):
    """The dense surface refinement on the device: params (B, 3 nj + nb + 4) is updated IN PLACE.  faces (F,3) int32; points (B,N,3) (lengths,
    weights (B,N) optional); markers = None or (vids (M,), positions (B,M,3), valid (B,M)); prior as smpl_chamfer_refine.  -> verts (B,V,3),
    joints (B, nj + n_extra, 3) (without trans / scale), loss of the last forward (B,), loss trace (B, iters, 4) or None."""
    _need(points, torch.float32, "points"), _need(params, torch.float32, "params"), _need(faces, torch.int32, "faces")
    _check_body(consts, nj, nb, n_extra)
    V = int(consts[0].shape[0])
    if points.dim() != 3 or points.shape[2] != 3 or tuple(params.shape) != (points.shape[0], 3 * nj + nb + 4) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"points must be (B,N,3), params (B, {3 * nj + nb + 4}), faces (F,3)")
    B, N, _ = points.shape
    F = int(faces.shape[0])
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise _lib.EtchHipError(f"face vertex ids must lie in [0, {V})")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    if weights is not None:
        weights = _need(weights.to(torch.float32).contiguous(), torch.float32, "weights")
        if tuple(weights.shape) != (B, N):
            raise _lib.EtchHipError(f"weights must be ({B},{N})")
    M, vids, pos, valid = _marker_args(markers, B, V, points.device)
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    G, parr = 0, None
    if prior is not None:
        means, prec, w = (_need(t, torch.float32, n) for t, n in zip(prior, ("means", "precisions", "nll_weights")))
        G = int(w.shape[0])
        if tuple(w.shape) != (G,) or tuple(means.shape) != (G, 69) or tuple(prec.shape) != (G, 69, 69):
            raise _lib.EtchHipError("prior: means (G,69), precisions (G,69,69), nll_weights (G,)")
        parr = (ctypes.c_void_p * 3)(means.data_ptr(), prec.data_ptr(), w.data_ptr())
    ws = _byte_workspace("etch_smpl_surface_refine_workspace", points.device, B, N, V, int(nj), int(nb), int(n_extra))
    verts = torch.empty((B, V, 3), dtype=torch.float32, device=points.device)
    joints = torch.empty((B, nj + n_extra, 3), dtype=torch.float32, device=points.device)
    loss = torch.empty((B,), dtype=torch.float32, device=points.device)
    tr = torch.empty((B, iters, 4), dtype=torch.float32, device=points.device) if want_trace else None
    _lib.call("etch_smpl_surface_refine", B, N, V, F, int(nj), int(nb), int(n_extra), arr, faces, points, nl, weights, M, vids, pos, valid, parr, G, int(iters),
              float(lr), float(beta1), float(beta2), float(eps), float(w_dense), float(w_marker), float(w_beta), float(w_prior), float(trunc),
              int(bool(optimize_scale)), params, verts, joints, tr, loss, ws)
    _lib.wrote(params)
    return verts, joints, loss, tr


# ------------------------------------------------------------------ containment (csrc/containment.hip)
def _ragged_mesh_args(mesh, B, what):
    """mesh = (verts (sum V,3) fp32, faces (sum F,3) int32, vert_offsets (B+1) int32, face_offsets (B+1) int32, max_faces): the packed batch of
    mesh_io.pack_meshes on the device (containment.pack_scans) -> the four tensors and max_faces, shapes and dtypes checked.  The offsets stay
    on the device: max_faces is the caller's (a host integer known when the batch was packed)."""
    if len(mesh) != 5:
        raise _lib.EtchHipError(f"{what}: the scan meshes are (verts, faces, vert_offsets, face_offsets, max_faces)")
    verts, faces, voff, foff, max_faces = mesh
    _need(verts, torch.float32, "scan verts"), _need(faces, torch.int32, "scan faces"), _need(voff, torch.int32, "vert_offsets")
    _need(foff, torch.int32, "face_offsets")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or tuple(voff.shape) != (B + 1,) or tuple(foff.shape) != (B + 1,):
        raise _lib.EtchHipError(f"{what}: scan verts (sum V,3), faces (sum F,3), vert_offsets and face_offsets ({B + 1},), got {tuple(verts.shape)}, "
                                f"{tuple(faces.shape)}, {tuple(voff.shape)}, {tuple(foff.shape)}")
    if int(max_faces) < 0 or int(max_faces) > faces.shape[0]:
        raise _lib.EtchHipError(f"{what}: max_faces must lie in [0, {faces.shape[0]}], got {max_faces}")
    return verts, faces, voff, foff, int(max_faces)


def _queries(points, what):
    _need(points, torch.float32, what)
    if points.dim() != 3 or points.shape[2] != 3:
        raise _lib.EtchHipError(f"{what} must be (B,Q,3), got {tuple(points.shape)}")
    return points.shape[0], points.shape[1]


def mesh_winding_number(mesh, queries, lengths=None):
    """Generalised winding number of scan b (mesh: the packed batch, see _ragged_mesh_args) at queries (B,Q,3) fp32 (lengths (B,) for ragged
    query sets; padding gets 0) -> w (B,Q) fp32: 1 inside a closed outward-oriented surface, 0 outside, -1 inside a reversed one.  Every
    (query, face) pair, van Oosterom-Strackee in fp32, fixed-order sums: bitwise reproducible, scan b alone = scan b in a batch."""
    B, Q = _queries(queries, "queries")
    verts, faces, voff, foff, mf = _ragged_mesh_args(mesh, B, "mesh_winding_number")
    ql = _lengths(lengths, B, Q, queries.device, "lengths")
    ws = _byte_workspace("etch_mesh_winding_number_workspace", queries.device, B, Q, mf)
    w = torch.empty((B, Q), dtype=torch.float32, device=queries.device)
    _lib.call("etch_mesh_winding_number", B, Q, mf, verts, faces, voff, foff, queries, ql, ws, w)
    return w


def ragged_mesh_closest(mesh, points, lengths=None):
    """point_mesh_closest for the packed batch of scan meshes (per-scan faces) -> face (B,N) int32 local to the scan, bary (B,N,3), d2 (B,N);
    the same region test, tie rule (lowest face), NaN rule and padding rule (face -1, bary 0, d2 0)."""
    B, N = _queries(points, "points")
    verts, faces, voff, foff, mf = _ragged_mesh_args(mesh, B, "ragged_mesh_closest")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    ws = _byte_workspace("etch_ragged_mesh_closest_workspace", points.device, B, N)
    face = torch.empty((B, N), dtype=torch.int32, device=points.device)
    bary = torch.empty((B, N, 3), dtype=torch.float32, device=points.device)
    d2 = torch.empty((B, N), dtype=torch.float32, device=points.device)
    _lib.call("etch_ragged_mesh_closest", B, N, mf, verts, faces, voff, foff, points, nl, ws, face, bary, d2)
    return face, bary, d2


def containment_energy_grad(body_verts, mesh, w, face, bary, d2, coef=None, w_contain=1.0, g=None):
    """The containment term of body_verts (B,V,3) against the scans: o_v = [|w_v| < 0.5] (NaN and face -1 are not outside), c_v the closest
    point of (face, bary) -> terms (B,2) fp64 = {sum_v o_v d2_v, sum_v o_v} and g (B,V,3) (given: updated IN PLACE; None: zeros first) with
    coef_b w_contain (2 / V) o_v (v - c_v) added.  -> (terms, g)."""
    B, V = _queries(body_verts, "body_verts")
    verts, faces, voff, foff, _ = _ragged_mesh_args(mesh, B, "containment_energy_grad")
    if tuple(w.shape) != (B, V) or tuple(face.shape) != (B, V) or tuple(bary.shape) != (B, V, 3) or tuple(d2.shape) != (B, V):
        raise _lib.EtchHipError(f"containment_energy_grad: w ({B},{V}), face ({B},{V}), bary ({B},{V},3), d2 ({B},{V})")
    _need(w, torch.float32, "w"), _need(face, torch.int32, "face"), _need(bary, torch.float32, "bary"), _need(d2, torch.float32, "d2")
    if coef is not None:
        coef = _need(coef.to(torch.float32).contiguous(), torch.float32, "coef")
        if tuple(coef.shape) != (B,):
            raise _lib.EtchHipError(f"coef must be ({B},)")
    if g is None:
        g = torch.zeros_like(body_verts)
    elif tuple(g.shape) != (B, V, 3):
        raise _lib.EtchHipError(f"g must be ({B},{V},3)")
    _need(g, torch.float32, "g")
    ws = _byte_workspace("etch_containment_energy_grad_workspace", body_verts.device, B, V)
    terms = torch.zeros((B, 2), dtype=torch.float64, device=body_verts.device)
    _lib.call("etch_containment_energy_grad", B, V, body_verts, verts, faces, voff, foff, w, face, bary, d2, coef, float(w_contain), ws, terms, g)
    _lib.wrote(g)
    return terms, g


def smpl_surface_refine_contain(consts, faces, points, params, scan, lengths=None, weights=None, markers=None, prior=None, iters=200, lr=2e-2, beta1=0.9,
                                beta2=0.999, eps=1e-8, w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05, optimize_scale=False,
                                w_contain=1e2, contain_every=10, nj=24, nb=10, n_extra=21, want_trace=False):
    """smpl_surface_refine with the containment term against scan = the packed batch of scan meshes in the body's frame (_ragged_mesh_args):
    + w_contain (sum_v o_v |v - c_v|^2) / V, o_v and c_v recomputed at iterations 0, K, 2K, ... (K = contain_every) and held in between.
    params is updated IN PLACE.  -> verts, joints, loss of the last forward (B,), loss trace (B, iters, 5) or None."""
    _need(points, torch.float32, "points"), _need(params, torch.float32, "params"), _need(faces, torch.int32, "faces")
    _check_body(consts, nj, nb, n_extra)
    V = int(consts[0].shape[0])
    if points.dim() != 3 or points.shape[2] != 3 or tuple(params.shape) != (points.shape[0], 3 * nj + nb + 4) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"points must be (B,N,3), params (B, {3 * nj + nb + 4}), faces (F,3)")
    B, N, _ = points.shape
    F = int(faces.shape[0])
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise _lib.EtchHipError(f"face vertex ids must lie in [0, {V})")
    if int(contain_every) < 1:
        raise _lib.EtchHipError("contain_every must be at least 1")
    sv, sf, svo, sfo, mf = _ragged_mesh_args(scan, B, "smpl_surface_refine_contain")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    if weights is not None:
        weights = _need(weights.to(torch.float32).contiguous(), torch.float32, "weights")
        if tuple(weights.shape) != (B, N):
            raise _lib.EtchHipError(f"weights must be ({B},{N})")
    M, vids, pos, valid = _marker_args(markers, B, V, points.device)
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    G, parr = 0, None
    if prior is not None:
        means, prec, w = (_need(t, torch.float32, n) for t, n in zip(prior, ("means", "precisions", "nll_weights")))
        G = int(w.shape[0])
        if tuple(w.shape) != (G,) or tuple(means.shape) != (G, 69) or tuple(prec.shape) != (G, 69, 69):
            raise _lib.EtchHipError("prior: means (G,69), precisions (G,69,69), nll_weights (G,)")
        parr = (ctypes.c_void_p * 3)(means.data_ptr(), prec.data_ptr(), w.data_ptr())
    ws = _byte_workspace("etch_smpl_surface_refine_contain_workspace", points.device, B, N, V, int(nj), int(nb), int(n_extra), mf)
    verts = torch.empty((B, V, 3), dtype=torch.float32, device=points.device)
    joints = torch.empty((B, nj + n_extra, 3), dtype=torch.float32, device=points.device)
    loss = torch.empty((B,), dtype=torch.float32, device=points.device)
    tr = torch.empty((B, iters, 5), dtype=torch.float32, device=points.device) if want_trace else None
    _lib.call("etch_smpl_surface_refine_contain", B, N, V, F, int(nj), int(nb), int(n_extra), arr, faces, points, nl, weights, M, vids, pos, valid, parr, G,
              int(iters), float(lr), float(beta1), float(beta2), float(eps), float(w_dense), float(w_marker), float(w_beta), float(w_prior), float(trunc),
              int(bool(optimize_scale)), mf, sv, sf, svo, sfo, float(w_contain), int(contain_every), params, verts, joints, tr, loss, ws)
    _lib.wrote(params)
    return verts, joints, loss, tr


# ------------------------------------------------------------------ SMPL+D registration and re-posing (csrc/register.hip)
def smpl_skin_frames(consts, params, nj=24, nb=10):
    """params (B, 3 nj + nb + 4) = pose (global orient first) | beta | trans | scale -> base (B,V,3), R (B,V,9), A (B,nj,12) with
    verts(D) = base + R D.  consts: the LBS tables of _DeviceBody.lbs_consts."""
    _need(params, torch.float32, "params")
    _check_body(consts, nj, nb, consts[7].numel() if len(consts) == 8 else -1)
    if params.dim() != 2 or params.shape[1] != 3 * nj + nb + 4:
        raise _lib.EtchHipError(f"params must be (B, {3 * nj + nb + 4}), got {tuple(params.shape)}")
    B, V = params.shape[0], consts[0].shape[0]
    arr = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in consts[:7]])
    base = torch.empty((B, V, 3), dtype=torch.float32, device=params.device)
    R = torch.empty((B, V, 9), dtype=torch.float32, device=params.device)
    A = torch.empty((B, nj, 12), dtype=torch.float32, device=params.device)
    _lib.call("etch_smpl_skin_frames", B, V, int(nj), int(nb), arr, params, base, R, A)
    return base, R, A


def _check_frames(base, R, D, what):
    _need(base, torch.float32, "base"), _need(R, torch.float32, "R")
    if base.dim() != 3 or base.shape[2] != 3 or base.shape[1] == 0 or tuple(R.shape) != (base.shape[0], base.shape[1], 9):
        raise _lib.EtchHipError(f"{what}: base (B,V,3) and R (B,V,9), got {tuple(base.shape)} and {tuple(R.shape)}")
    if D is not None:
        _need(D, torch.float32, "D")
        if D.shape != base.shape:
            raise _lib.EtchHipError(f"{what}: D must be {tuple(base.shape)} like base, got {tuple(D.shape)}")
    return base.shape[0], base.shape[1]


def smpld_apply(base, R, D):
    """verts (B,V,3) = base + R D."""
    B, V = _check_frames(base, R, D, "smpld_apply")
    verts = torch.empty_like(base)
    _lib.call("etch_smpld_apply", B, V, base, R, D, verts)
    return verts


def _check_registration(base, R, D, scan, scan_lengths, nbr_ptr, nbr_idx, n_edges, weights, trunc, what):
    B, V = _check_frames(base, R, D, what)
    _need(scan, torch.float32, "scan")
    if scan.dim() != 3 or scan.shape[0] != B or scan.shape[2] != 3 or scan.shape[1] == 0:
        raise _lib.EtchHipError(f"{what}: scan must be ({B},N,3) with N >= 1, got {tuple(scan.shape)}")
    N = scan.shape[1]
    sl = _lengths(scan_lengths, B, N, scan.device, "scan_lengths")
    _need(nbr_ptr, torch.int32, "nbr_ptr"), _need(nbr_idx, torch.int32, "nbr_idx")
    if tuple(nbr_ptr.shape) != (V + 1,) or tuple(nbr_idx.shape) != (2 * int(n_edges),) or n_edges < 0:
        raise _lib.EtchHipError(f"{what}: nbr_ptr must be ({V + 1},) and nbr_idx (2 n_edges,) = ({2 * int(n_edges)},), got {tuple(nbr_ptr.shape)} and "
                                f"{tuple(nbr_idx.shape)}")
    if not all(math.isfinite(float(w)) and float(w) >= 0.0 for w in weights):
        raise _lib.EtchHipError(f"{what}: the weights must be finite and >= 0")
    if trunc is not None and not (math.isfinite(float(trunc)) and float(trunc) >= 0.0):
        raise _lib.EtchHipError(f"{what}: trunc must be None or finite and >= 0")
    n = ctypes.c_longlong(0)
    _lib.call("etch_smpld_register_workspace", B, N, V, ctypes.byref(n))
    ws = torch.empty((max(int(n.value), 8),), dtype=torch.uint8, device=scan.device)
    return B, N, V, sl, ws, -1.0 if trunc is None else float(trunc)


def smpld_energy_grad(base, R, D, scan, nbr_ptr, nbr_idx, n_edges, scan_lengths=None, w_s2m=1.0, w_m2s=1.0, lambda_s=1.0, lambda_m=0.0, trunc=None):
    """One evaluation of the registration energy at the offsets D (B,V,3): -> terms (B,4) = scan -> body, body -> scan, smoothness,
    magnitude; grad (B,V,3) = d energy / dD with neighbours and masks held fixed; verts (B,V,3) = base + R D; idx_xy (B,N), idx_yx (B,V) int32,
    the neighbours of nn_bidir(scan, verts).  nbr_ptr (V+1) / nbr_idx (2 n_edges) int32: the neighbour lists of the mesh edges."""
    B, N, V, sl, ws, tr = _check_registration(base, R, D, scan, scan_lengths, nbr_ptr, nbr_idx, n_edges, (w_s2m, w_m2s, lambda_s, lambda_m), trunc,
                                              "smpld_energy_grad")
    dev = scan.device
    terms = torch.empty((B, 4), dtype=torch.float32, device=dev)
    grad, verts = torch.empty_like(base), torch.empty_like(base)
    ixy = torch.empty((B, N), dtype=torch.int32, device=dev)
    iyx = torch.empty((B, V), dtype=torch.int32, device=dev)
    _lib.call("etch_smpld_energy_grad", B, N, V, base, R, D, scan, sl, nbr_ptr, nbr_idx, int(n_edges), float(w_s2m), float(w_m2s), float(lambda_s),
              float(lambda_m), tr, ws, terms, grad, verts, ixy, iyx)
    return terms, grad, verts, ixy, iyx


def smpld_register(base, R, D, scan, nbr_ptr, nbr_idx, n_edges, lambda_s, scan_lengths=None, w_s2m=1.0, w_m2s=1.0, lambda_m=0.0, trunc=None, lr=1e-3,
                   want_trace=False):
    """len(lambda_s) Adam steps on D (B,V,3), updated IN PLACE; step i uses the smoothness weight lambda_s[i].  -> verts (B,V,3) and energy
    (B,4) of the final D, trace (B,iters,4) = the four terms at the iterate before each step, or None."""
    lam = [float(l) for l in lambda_s]
    if len(lam) < 1:
        raise _lib.EtchHipError("smpld_register: lambda_s must hold one smoothness weight per iteration, at least one")
    if not (math.isfinite(float(lr)) and float(lr) > 0.0):
        raise _lib.EtchHipError("smpld_register: lr must be finite and > 0")
    B, N, V, sl, ws, tr = _check_registration(base, R, D, scan, scan_lengths, nbr_ptr, nbr_idx, n_edges, [w_s2m, w_m2s, lambda_m] + lam, trunc,
                                              "smpld_register")
    iters = len(lam)
    dev = scan.device
    verts = torch.empty_like(base)
    energy = torch.empty((B, 4), dtype=torch.float32, device=dev)
    trace = torch.empty((B, iters, 4), dtype=torch.float32, device=dev) if want_trace else None
    _lib.call("etch_smpld_register", B, N, V, base, R, scan, sl, nbr_ptr, nbr_idx, int(n_edges), iters, (ctypes.c_float * iters)(*lam), float(lambda_m),
              float(w_s2m), float(w_m2s), tr, float(lr), D, verts, energy, trace, ws)
    _lib.wrote(D)
    return verts, energy, trace


def skin_carry(points, face, bary, faces, W, A, A_new, trans_scale, trans_scale_new):
    """Carry points (P,3) fp64 bound to a skinned surface (face (P) int32 into faces (F,3) int32, bary (P,3) fp64) from the pose of A (nj,12)
    to the pose of A_new: (T' T^-1 (x / scale - trans) + trans') scale' with T = sum_j w~_j A_j, w~ = the barycentric mix of W (V,nj);
    trans_scale / trans_scale_new: (4,) fp32 = trans | scale.  |det T^R| < 1e-10 -> T = identity.  -> (P,3) fp64."""
    _need(points, torch.float64, "points"), _need(bary, torch.float64, "bary"), _need(face, torch.int32, "face"), _need(faces, torch.int32, "faces")
    _need(W, torch.float32, "W"), _need(A, torch.float32, "A"), _need(A_new, torch.float32, "A_new")
    _need(trans_scale, torch.float32, "trans_scale"), _need(trans_scale_new, torch.float32, "trans_scale_new")
    P = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or tuple(bary.shape) != (P, 3) or tuple(face.shape) != (P,):
        raise _lib.EtchHipError(f"skin_carry: points (P,3), face (P,), bary (P,3), got {tuple(points.shape)}, {tuple(face.shape)}, {tuple(bary.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0 or W.dim() != 2:
        raise _lib.EtchHipError(f"skin_carry: faces (F,3) with F >= 1 and W (V,nj), got {tuple(faces.shape)} and {tuple(W.shape)}")
    V, nj = W.shape
    if not 1 <= nj <= 55 or tuple(A.shape) != (nj, 12) or tuple(A_new.shape) != (nj, 12):
        raise _lib.EtchHipError(f"skin_carry: A and A_new must be ({nj},12) for W {tuple(W.shape)} (nj <= 55), got {tuple(A.shape)} and {tuple(A_new.shape)}")
    if tuple(trans_scale.shape) != (4,) or tuple(trans_scale_new.shape) != (4,):
        raise _lib.EtchHipError("skin_carry: trans_scale and trans_scale_new must be (4,) = trans | scale")
    out = torch.empty_like(points)
    _lib.call("etch_skin_carry", P, faces.shape[0], V, nj, points, face, bary, faces, W, A, A_new, trans_scale, trans_scale_new, out)
    return out


# ------------------------------------------------------------------ tightness supervision (csrc/raycast.hip)
def _check_mesh(verts, faces):
    """verts (V,3) fp64, faces (F,3) int32 on the device with every index in [0, V): the kernels read vertices through the face indices."""
    _need(verts, torch.float64, "verts"), _need(faces, torch.int32, "faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"mesh must be verts (V,3) and faces (F,3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.numel():
        lo, hi = (int(v) for v in torch.aminmax(faces))
        if lo < 0 or hi >= verts.shape[0]:
            raise _lib.EtchHipError(f"face indices must lie in [0, {verts.shape[0]}), got [{lo}, {hi}]")
    return verts.shape[0], faces.shape[0]


def _mesh_workspace(query, n, F, device):
    b = ctypes.c_longlong(0)
    _lib.call(query, int(n), int(F), ctypes.byref(b))
    return torch.empty((max(int(b.value), 8),), dtype=torch.uint8, device=device)


def ray_first_hit(origins, dirs, verts, faces, excl_face=None, t_max=None):
    """First hit of rays (R,3) fp64 on a mesh (Moller-Trumbore in fp64, csrc/raycast.hip) -> face (R) int32 (-1 = miss), t (R) fp64 (+inf on a
    miss), bary (R,3) = (1 - u - v, u, v), loc (R,3) = o + t d.  excl_face (R) int32: a face each ray skips (-1 = none); t_max (R) fp64: a hit
    needs t < t_max.  The smallest t wins, equal t -> the lowest face."""
    _need(origins, torch.float64, "origins"), _need(dirs, torch.float64, "dirs")
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise _lib.EtchHipError(f"origins and dirs must both be (R,3), got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    R = origins.shape[0]
    _, F = _check_mesh(verts, faces)
    if excl_face is not None and (_need(excl_face, torch.int32, "excl_face").shape != (R,)):
        raise _lib.EtchHipError(f"excl_face must be ({R},)")
    if t_max is not None and (_need(t_max, torch.float64, "t_max").shape != (R,)):
        raise _lib.EtchHipError(f"t_max must be ({R},)")
    dev = origins.device
    ws = _mesh_workspace("etch_ray_first_hit_workspace", R, F, dev)
    face = torch.empty((R,), dtype=torch.int32, device=dev)
    t = torch.empty((R,), dtype=torch.float64, device=dev)
    bary = torch.empty((R, 3), dtype=torch.float64, device=dev)
    loc = torch.empty((R, 3), dtype=torch.float64, device=dev)
    _lib.call("etch_ray_first_hit", R, F, origins, dirs, verts, faces, excl_face, t_max, ws, face, t, bary, loc)
    return face, t, bary, loc


def closest_point_on_mesh(points, verts, faces):
    """Closest point on a mesh of points (P,3) fp64 (Ericson 5.1.5 in fp64, csrc/raycast.hip) -> face (P) int32, bary (P,3), closest (P,3),
    d2 (P) fp64.  The smallest d2 wins, equal d2 -> the lowest face."""
    _need(points, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.EtchHipError(f"points must be (P,3), got {tuple(points.shape)}")
    P = points.shape[0]
    _, F = _check_mesh(verts, faces)
    dev = points.device
    ws = _mesh_workspace("etch_closest_point_on_mesh_workspace", P, F, dev)
    face = torch.empty((P,), dtype=torch.int32, device=dev)
    bary = torch.empty((P, 3), dtype=torch.float64, device=dev)
    closest = torch.empty((P, 3), dtype=torch.float64, device=dev)
    d2 = torch.empty((P,), dtype=torch.float64, device=dev)
    _lib.call("etch_closest_point_on_mesh", P, F, points, verts, faces, ws, face, bary, closest, d2)
    return face, bary, closest, d2


def vertex_face_csr(faces_np, num_vertices):
    """Vertex -> (face, corner) incidence in ascending face order: ptr (V+1), idx (3F) with entries 3 f + corner (host numpy, int32)."""
    import numpy as np

    flat = np.asarray(faces_np, np.int64).ravel()
    idx = np.argsort(flat, kind="stable").astype(np.int32)
    ptr = np.zeros(num_vertices + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=num_vertices), out=ptr[1:])
    return ptr.astype(np.int32), idx


def vertex_normals(verts, faces):
    """trimesh's weighted_vertex_normals (corner-angle weights), summed per vertex in ascending face order -> (V,3) fp64."""
    V, F = _check_mesh(verts, faces)
    ptr, idx = vertex_face_csr(faces.cpu().numpy(), V)
    ptr_d = torch.from_numpy(ptr).to(verts.device)
    idx_d = torch.from_numpy(idx).to(verts.device)
    ws = torch.empty((max(6 * F, 1),), dtype=torch.float64, device=verts.device)
    out = torch.empty((V, 3), dtype=torch.float64, device=verts.device)
    _lib.call("etch_vertex_normals", V, F, verts, faces, ptr_d, idx_d, ws, out)
    return out


def remove_close(points, radius):
    """trimesh 4.x points.remove_close flags: points (C,3) fp64 -> degree (C) int32, removed (C) bool (squared distance <= radius^2 in fp64)."""
    _need(points, torch.float64, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.EtchHipError(f"points must be (C,3), got {tuple(points.shape)}")
    C = points.shape[0]
    r = float(radius)
    deg = torch.empty((C,), dtype=torch.int32, device=points.device)
    rem = torch.empty((C,), dtype=torch.int32, device=points.device)
    _lib.call("etch_remove_close", C, points, r * r, deg, rem)
    return deg, rem.bool()


# ------------------------------------------------------------------ geodesic labels and confidences (csrc/geodesic.hip)
def geodesic_heat(verts, topo, sources, t_coef=1.0, intrinsic_delaunay=True, want_dist=True, want_min=True, want_mesh=False, mollify_eps=1e-6,
                  delaunay_tol=1e-12, max_rounds=4096, heat_tol=1e-9, heat_omega=None, heat_cap=50000, cg_rtol=1e-10, cg_cap=50000):
    """Heat-method distances: verts (B,V,3) fp64 on the device, topo = the shared edge topology (fv, fe, fs (F,3), ef, ev (E,2) int32
    device tensors, etch_amd.geodesic.EdgeTopology.device()), sources (S,) int32 -> dict with dist (B,S,V) fp64, dmin (B,V) fp64, label (B,V)
    int32, iters (B,S,2) int32 (heat sweeps, CG iterations), flips (B,) and, with want_mesh, ev (B,E,2), el (B,E), ecot (B,E,2), area (B,F).
    heat_omega (None: 1 on the intrinsic Delaunay mesh, 0.7 on the cotan one) damps the heat sweeps.
    Raises EtchHipError on bad input before any launch, and when a column reaches an iteration cap."""
    _need(verts, torch.float64, "verts")
    if heat_omega is None:
        heat_omega = 1.0 if intrinsic_delaunay else 0.7
    fv, fe, fs, ef, ev = topo
    for t, n in zip(topo, ("fv", "fe", "fs", "ef", "ev")):
        _need(t, torch.int32, n)
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise _lib.EtchHipError(f"verts must be (B,V,3), got {tuple(verts.shape)}")
    B, V, _ = verts.shape
    F, E = fv.shape[0], ef.shape[0]
    if fv.shape != (F, 3) or fe.shape != (F, 3) or fs.shape != (F, 3) or ef.shape != (E, 2) or ev.shape != (E, 2) or B < 1 or F < 1:
        raise _lib.EtchHipError("topology must be fv, fe, fs (F,3) and ef, ev (E,2) with B, F >= 1")
    if int(fv.min()) < 0 or int(fv.max()) >= V or int(ev.min()) < 0 or int(ev.max()) >= V:
        raise _lib.EtchHipError(f"vertex indices must lie in [0, {V})")
    if int(fe.min()) < 0 or int(fe.max()) >= E or int(ef.max()) >= F or int(ef[:, 0].min()) < 0 or int(ef.min()) < -1:
        raise _lib.EtchHipError("edge / face indices out of range")
    sources = _need(sources, torch.int32, "sources")
    S = int(sources.numel())
    if sources.dim() != 1 or S < 1:
        raise _lib.EtchHipError("sources must be a non-empty (S,) int32 tensor")
    if int(sources.min()) < 0 or int(sources.max()) >= V:
        raise _lib.EtchHipError(f"source indices must lie in [0, {V})")
    dev = verts.device
    nb = ctypes.c_longlong(0)
    _lib.call("etch_geodesic_workspace", B, V, F, E, S, ctypes.byref(nb))
    ws = torch.empty((max(int(nb.value), 8),), dtype=torch.uint8, device=dev)
    dist = torch.empty((B, S, V), dtype=torch.float64, device=dev)
    dmin = torch.empty((B, V), dtype=torch.float64, device=dev) if want_min else None
    label = torch.empty((B, V), dtype=torch.int32, device=dev) if want_min else None
    iters = torch.empty((B, S, 2), dtype=torch.int32, device=dev)
    flips = (ctypes.c_int * B)()
    mesh = {}
    if want_mesh:
        mesh = {"ev": torch.empty((B, E, 2), dtype=torch.int32, device=dev), "el": torch.empty((B, E), dtype=torch.float64, device=dev),
                "ecot": torch.empty((B, E, 2), dtype=torch.float64, device=dev), "area": torch.empty((B, F), dtype=torch.float64, device=dev)}
    _lib.call("etch_geodesic_heat", B, V, F, E, S, verts, fv, fe, fs, ef, ev, sources, t_coef, int(bool(intrinsic_delaunay)), mollify_eps, delaunay_tol,
              int(max_rounds), heat_tol, heat_omega, int(heat_cap), cg_rtol, int(cg_cap), ws, dist, dmin, label, iters, flips, mesh.get("ev"), mesh.get("el"),
              mesh.get("ecot"), mesh.get("area"))
    it = iters.cpu()
    if bool((it < 0).any()):
        bad = torch.nonzero((it < 0).any(2))[:4].tolist()
        raise _lib.EtchHipError(f"etch_geodesic_heat: (body, source) {bad} reached an iteration cap (heat {heat_cap}, CG {cg_cap})")
    out = {"dist": dist if want_dist else None, "dmin": dmin, "label": label, "iters": it, "flips": list(flips)}
    out.update(mesh)
    return out


# ------------------------------------------------------------------ the training step (csrc/train_step.hip)
TRAIN_STATUS_NAN, TRAIN_STATUS_BAD_LABEL = 1, 2       # include/etch_hip.h: ETCH_TRAIN_STATUS_*
_TRAIN_LOSS_WS = {}


def train_losses(direction, magnitude, confidences, part_labels, t_vectors, t_confidences, t_labels, index, weights, scale_magnitude, counter, status=None):
    """etch_train_losses: the four losses of train.py:81-101 and the gradient of their sum, one launch.  Heads (B,K,3) / (B,K,1) / (B,K,1) / (B,K,M) or
    None; targets (B,N,3), (B,N,1), (B,N) int64; index (B,K) int64; weights = (direction_w, magnitude_w, confidence_w, part_label_w); counter: one zero
    int32 (left zero).  Returns (losses (5) = the four weighted losses and their sum, status (>= 1 int32, [0] = the ETCH_TRAIN_STATUS_* bits), gradients
    in the heads' order, None for an absent head)."""
    heads = [direction, magnitude, confidences, part_labels]
    first = next((h for h in heads if h is not None), None)
    if first is None:
        raise _lib.EtchHipError("train_losses: at least one head output is needed")
    B, K = first.shape[0], first.shape[1]
    for h, last, name in zip(heads, (3, 1, 1, None), ("direction", "magnitude", "confidences", "part_labels")):
        if h is not None:
            _need(h, torch.float32, name)
            if h.dim() != 3 or h.shape[:2] != (B, K) or (last is not None and h.shape[2] != last):
                raise _lib.EtchHipError(f"{name} must be (B,K,{last or 'M'}) with B, K = {B}, {K}; got {tuple(h.shape)}")
    if B * K < 1:
        raise _lib.EtchHipError("train_losses: empty batch")
    _need(index, torch.int64, "index")
    if index.shape != (B, K):
        raise _lib.EtchHipError(f"index must be ({B},{K}), got {tuple(index.shape)}")
    N = None
    for t, dtype, tail, name, used in ((t_vectors, torch.float32, (3,), "vectors", direction is not None or magnitude is not None),
                                       (t_confidences, torch.float32, (1,), "confidences", confidences is not None),
                                       (t_labels, torch.int64, (), "labels", part_labels is not None)):
        if not used:
            continue
        if t is None:
            raise _lib.EtchHipError(f"train_losses: the target `{name}` is needed")
        _need(t, dtype, name)
        if t.dim() != 2 + len(tail) or t.shape[0] != B or tuple(t.shape[2:]) != tail or (N is not None and t.shape[1] != N):
            raise _lib.EtchHipError(f"target {name} must be (B,N{',' if tail else ''}{','.join(map(str, tail))}), got {tuple(t.shape)}")
        N = t.shape[1]
    if N < 1:
        raise _lib.EtchHipError("train_losses: empty targets")
    M = part_labels.shape[2] if part_labels is not None else 0
    dev = first.device
    key = (dev.index, _lib.stream())
    ws = _TRAIN_LOSS_WS.get(key)
    if ws is None:
        ws = _TRAIN_LOSS_WS[key] = torch.empty((_lib.call("etch_train_losses_workspace_doubles"),), dtype=torch.float64, device=dev)
    losses = torch.empty((5,), dtype=torch.float32, device=dev)
    if status is None:
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    grads = [torch.empty_like(h) if h is not None else None for h in heads]
    w = [float(x) for x in weights]
    used_t = [t_vectors if (direction is not None or magnitude is not None) else None, t_confidences if confidences is not None else None,
              t_labels if part_labels is not None else None]
    _lib.call("etch_train_losses", int(B), int(K), int(N), int(M), *heads, *used_t, index, w[0], w[1], w[2], w[3],
              float(scale_magnitude), ws, counter, losses, status, *grads)
    _lib.wrote(status)
    return losses, status, grads


def guarded_adam_chunk():
    return _lib.call("etch_guarded_adam_chunk")


def guarded_adam_step(T, C, chunk_tensor, first_chunk, numel, pmv, grads, status, steps, chunkflags, lr, betas, eps, counters):
    """etch_guarded_adam_step over tables built by etch_amd.optim.GuardedAdam (all device tensors; status may be None)."""
    _lib.call("etch_guarded_adam_step", int(T), int(C), chunk_tensor, first_chunk, numel, pmv, grads, status, steps, chunkflags, lr, betas[0], betas[1], eps,
              counters)


def grad_tail_floats():
    return _lib.call("etch_grad_tail_floats")


def grad_pack(T, C, chunk_tensor, first_chunk, numel, grads, offsets, flat, scale, mode, losses=None, status=None, tail_offset=-1, *, layout):
    """etch_grad_pack: one contribution's gradients (grads (T) int64 addresses, 0 = none) times `scale` into the fp32 buffer `flat` at offsets (T) int64
    elements, over GuardedAdam's chunk table.  mode 0 writes, mode 1 adds (product and sum rounded separately).  tail_offset >= 0: losses (5) * scale
    and the two bits of status as 0/1 go into the grad_tail_floats() floats there.  layout = (offsets, numel) as HOST integer arrays, the copies of
    the two device tables: every slot is checked against the buffer here, on the host, before the launch."""
    _need(flat, torch.float32, "flat"), _need(offsets, torch.int64, "offsets"), _need(grads, torch.int64, "grads"), _need(numel, torch.int64, "numel")
    if mode not in (0, 1):
        raise _lib.EtchHipError(f"grad_pack: mode must be 0 (write) or 1 (add), got {mode}")
    if flat.data_ptr() % 16:
        raise _lib.EtchHipError("grad_pack: the flat buffer must be 16-byte aligned")
    off_h, numel_h = (np.asarray(a, np.int64).reshape(-1) for a in layout)
    if not (off_h.size == numel_h.size == int(T) == offsets.numel() == numel.numel() == grads.numel()):
        raise _lib.EtchHipError(f"grad_pack: the tables and the layout must hold T = {T} entries each")
    if (off_h < 0).any() or (off_h % 4).any() or (numel_h < 0).any():
        raise _lib.EtchHipError("grad_pack: offsets must be non-negative multiples of 4 elements")
    if int((off_h + numel_h).max()) > (tail_offset if tail_offset >= 0 else flat.numel()):
        raise _lib.EtchHipError("grad_pack: a slot reaches beyond the flat buffer (or into its tail)")
    if tail_offset >= 0:
        if tail_offset + grad_tail_floats() > flat.numel():
            raise _lib.EtchHipError("grad_pack: the tail does not fit the flat buffer")
        if losses is not None:
            _need(losses, torch.float32, "losses")
            if losses.numel() < 5:
                raise _lib.EtchHipError("grad_pack: losses must hold 5 values")
        if status is not None:
            _need(status, torch.int32, "status")
    _lib.call("etch_grad_pack", int(T), int(C), chunk_tensor, first_chunk, numel, grads, offsets, flat, float(scale), int(mode), losses, status,
              int(tail_offset))
    _lib.wrote(flat)


def grad_unpack_tail(tail, losses=None, status=None):
    """etch_grad_unpack_tail: the (reduced) tail of a flat gradient buffer -> (losses (5) fp32, status (1) int32 with the ETCH_TRAIN_STATUS_* bits any
    contribution set); `losses` / `status` are written in place when given."""
    _need(tail, torch.float32, "tail")
    if tail.numel() < grad_tail_floats():
        raise _lib.EtchHipError(f"grad_unpack_tail: the tail holds {grad_tail_floats()} floats")
    if losses is None:
        losses = torch.empty((5,), dtype=torch.float32, device=tail.device)
    if status is None:
        status = torch.zeros((1,), dtype=torch.int32, device=tail.device)
    _need(losses, torch.float32, "losses"), _need(status, torch.int32, "status")
    _lib.call("etch_grad_unpack_tail", tail, losses, status)
    _lib.wrote(losses, status)
    return losses, status


# ------------------------------------------------------------------ scan ingestion (csrc/mesh_sample.hip)
def bbox_center(verts, vert_offsets):
    """(min + max) / 2 per scan: verts (sum V,3) fp64 concatenated, vert_offsets (B+1) int32 -> (B,3) fp64."""
    _need(verts, torch.float64, "verts"), _need(vert_offsets, torch.int32, "vert_offsets")
    B = vert_offsets.numel() - 1
    center = torch.empty((B, 3), dtype=torch.float64, device=verts.device)
    _lib.call("etch_bbox_center", int(B), verts, vert_offsets, center)
    return center


def sample_surface(verts, faces, vert_offsets, face_offsets, keys, num_points, total_faces, max_faces, center=None, want_fp64=False):
    """etch_sample_surface on a packed ragged batch: verts (sum V,3) fp64, faces (sum F,3) int32 local to their scan and ALREADY VALIDATED,
    vert_offsets / face_offsets (B+1) int32, keys (B) int64 holding the uint64 bits, center (B,3) fp64 or None; total_faces and max_faces are
    the host's copies of face_offsets[B] and the largest face count.  -> points (B,N,3) fp32, points64 (B,N,3) fp64 or None, face (B,N) int32,
    status (B) int32 (ETCH_SAMPLE_STATUS_* bits, still on the device)."""
    _need(verts, torch.float64, "verts"), _need(faces, torch.int32, "faces"), _need(keys, torch.int64, "keys")
    _need(vert_offsets, torch.int32, "vert_offsets"), _need(face_offsets, torch.int32, "face_offsets")
    B, N, dev = keys.numel(), int(num_points), verts.device
    if vert_offsets.numel() != B + 1 or face_offsets.numel() != B + 1 or faces.shape != (total_faces, 3) or N < 0:
        raise _lib.EtchHipError("sample_surface: offsets must be (B+1), faces (total_faces,3) and num_points >= 0")
    if center is not None and _need(center, torch.float64, "center").shape != (B, 3):
        raise _lib.EtchHipError(f"center must be ({B},3)")
    ws = _mesh_workspace("etch_sample_surface_workspace", B, total_faces, dev)
    p32 = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    p64 = torch.empty((B, N, 3), dtype=torch.float64, device=dev) if want_fp64 else None
    face = torch.empty((B, N), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("etch_sample_surface", int(B), N, int(total_faces), int(max_faces), verts, faces, vert_offsets, face_offsets, keys, center, ws, p32, p64, face,
              status)
    return p32, p64, face, status


# ------------------------------------------------------------------ single-view scans (csrc/depth_render.hip)
def _check_cameras(cams, what):
    _need(cams, torch.float64, "cams")
    if cams.dim() != 2 or cams.shape[1] != 16:
        raise _lib.EtchHipError(f"{what}: cams must be (NV,16) = fx, fy, cx, cy, R (9), t (3), got {tuple(cams.shape)}")
    return cams.shape[0]


def depth_large_threshold():
    """Candidate pixels above which etch_render_depth hands a face to its large-face launch."""
    return int(_lib.call("etch_depth_large_threshold"))


def render_depth(verts, faces, vert_offsets, face_offsets, view_mesh, cams, height, width, max_faces, near=0.05, want_bary=False):
    """etch_render_depth on a packed ragged batch (mesh_io.pack_meshes): verts (sum V,3) fp64, faces (sum F,3) int32 local to their mesh and
    ALREADY VALIDATED, vert_offsets / face_offsets (B+1) int32, view_mesh (NV) int32 with every entry in [0, B), cams (NV,16) fp64; max_faces
    is the host's copy of the largest face count.  -> depth (NV,H,W) fp64 (+inf = nothing hit), face (NV,H,W) int32 (-1), bary (NV,H,W,3) or
    None, dropped (NV) int32, status (NV) int32 (ETCH_DEPTH_STATUS_* bits), large (NV) int32 -- all still on the device."""
    _need(verts, torch.float64, "verts"), _need(faces, torch.int32, "faces"), _need(view_mesh, torch.int32, "view_mesh")
    _need(vert_offsets, torch.int32, "vert_offsets"), _need(face_offsets, torch.int32, "face_offsets")
    NV = _check_cameras(cams, "render_depth")
    B, H, W, dev = vert_offsets.numel() - 1, int(height), int(width), verts.device
    if B < 1 or face_offsets.numel() != B + 1 or verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError("render_depth: offsets must be (B+1) with B >= 1, verts (.,3) and faces (.,3)")
    if view_mesh.shape != (NV,) or H < 1 or W < 1 or int(max_faces) < 0 or int(max_faces) > faces.shape[0]:
        raise _lib.EtchHipError(f"render_depth: view_mesh must be ({NV},), the image at least 1 x 1 and 0 <= max_faces <= {faces.shape[0]}")
    if not (float(near) > 0.0 and math.isfinite(float(near))):
        raise _lib.EtchHipError(f"render_depth: near must be positive and finite, got {near}")
    if NV * H * W >= 2 ** 31 - 256:
        raise _lib.EtchHipError("render_depth: NV * H * W must stay below 2^31: render the views in parts")
    b = ctypes.c_longlong(0)
    _lib.call("etch_render_depth_workspace", int(NV), int(max_faces), ctypes.byref(b))
    ws = torch.empty((max(int(b.value), 8),), dtype=torch.uint8, device=dev)
    depth = torch.empty((NV, H, W), dtype=torch.float64, device=dev)
    face = torch.empty((NV, H, W), dtype=torch.int32, device=dev)
    bary = torch.empty((NV, H, W, 3), dtype=torch.float64, device=dev) if want_bary else None
    dropped = torch.empty((NV,), dtype=torch.int32, device=dev)
    status = torch.empty((NV,), dtype=torch.int32, device=dev)
    large = torch.empty((NV,), dtype=torch.int32, device=dev)
    if NV:
        _lib.call("etch_render_depth", int(B), int(NV), H, W, int(max_faces), verts, faces, vert_offsets, face_offsets, view_mesh, cams, float(near), ws,
                  depth, face, bary, dropped, status, large)
    return depth, face, bary, dropped, status, large


def depth_compact(depth, cams, near=0.05, far=math.inf):
    """etch_depth_compact: depth (NV,H,W) fp64 (rendered or a caller's), cams (NV,16) fp64; a pixel is valid where near < z < far.  -> count (NV)
    int32, offsets (NV+1) int32, index (NV*H*W) int32 and points (NV*H*W,3) fp64 whose first offsets[NV] rows are the valid pixels of all
    views in row-major order (the rest is not written) -- all still on the device."""
    _need(depth, torch.float64, "depth")
    NV = _check_cameras(cams, "depth_compact")
    if depth.dim() != 3 or depth.shape[0] != NV:
        raise _lib.EtchHipError(f"depth_compact: depth must be ({NV},H,W), got {tuple(depth.shape)}")
    if not (float(near) >= 0.0 and float(far) > float(near)):
        raise _lib.EtchHipError(f"depth_compact: needs 0 <= near < far, got {near} and {far}")
    _, H, W = depth.shape
    if NV * H * W >= 2 ** 31 - 256:
        raise _lib.EtchHipError("depth_compact: NV * H * W must stay below 2^31: compact the views in parts")
    dev = depth.device
    b = ctypes.c_longlong(0)
    _lib.call("etch_depth_compact_workspace", int(NV), int(H), int(W), ctypes.byref(b))
    ws = torch.empty((max(int(b.value), 8),), dtype=torch.uint8, device=dev)
    count = torch.empty((NV,), dtype=torch.int32, device=dev)
    offsets = torch.empty((NV + 1,), dtype=torch.int32, device=dev)
    index = torch.empty((NV * H * W,), dtype=torch.int32, device=dev)
    points = torch.empty((NV * H * W, 3), dtype=torch.float64, device=dev)
    _lib.call("etch_depth_compact", int(NV), int(H), int(W), depth, cams, float(near), float(far), ws, count, offsets, index, points)
    return count, offsets, index, points


def depth_pick(offsets, index, points, keys, num_points, center=None):
    """etch_depth_pick: offsets (NV+1) int32, index (>= offsets[NV]) int32 and points (same rows,3) fp64 of a packed cloud, keys (NV) int64 holding
    the uint64 bits, center (NV,3) fp64 subtracted from the picked points or None.  -> points (NV,N,3) fp64, their fp32 rounding, pixel (NV,N) int32, status (NV) int32 (ETCH_DEPTH_STATUS_EMPTY where a view
    has no valid pixel; its rows are zeros) -- all still on the device."""
    _need(offsets, torch.int32, "offsets"), _need(index, torch.int32, "index"), _need(points, torch.float64, "points"), _need(keys, torch.int64, "keys")
    NV, N, dev = keys.numel(), int(num_points), points.device
    if offsets.shape != (NV + 1,) or points.dim() != 2 or points.shape[1] != 3 or index.shape != (points.shape[0],) or N < 0:
        raise _lib.EtchHipError(f"depth_pick: offsets must be ({NV + 1},), points (M,3), index (M,) and num_points >= 0")
    if center is not None and _need(center, torch.float64, "center").shape != (NV, 3):
        raise _lib.EtchHipError(f"center must be ({NV},3)")
    p64 = torch.zeros((NV, N, 3), dtype=torch.float64, device=dev)
    p32 = torch.zeros((NV, N, 3), dtype=torch.float32, device=dev)
    pixel = torch.zeros((NV, N), dtype=torch.int32, device=dev)
    status = torch.empty((NV,), dtype=torch.int32, device=dev)
    if NV:
        _lib.call("etch_depth_pick", int(NV), N, offsets, index, points, keys, center, p64, p32, pixel, status)
    return p64, p32, pixel, status


# ------------------------------------------------------------------ raw point clouds (csrc/cloud_filter.hip)
CLOUD_MAX_K = 32


def _cloud_args(points, offsets, what):
    _need(points, torch.float64, "points"), _need(offsets, torch.int32, "offsets")
    if points.dim() != 2 or points.shape[1] != 3 or offsets.dim() != 1 or offsets.numel() < 2:
        raise _lib.EtchHipError(f"{what}: points must be (M,3) and offsets (B+1) with B >= 1, got {tuple(points.shape)} and {tuple(offsets.shape)}")
    if points.shape[0] >= 2 ** 31 // 3:
        raise _lib.EtchHipError(f"{what}: the batch is too large for 32-bit offsets: filter it in parts")
    return offsets.numel() - 1, points.shape[0]


def cloud_cell_grid(points, offsets, mode, k=1, cell=0.0, sort=True):
    """etch_cloud_cell_keys and the stable sort of the rows by (cloud, cell key): mode 0 = kNN (cell 0 = the rule of the header), 1 = radius
    (cell = r), 2 = voxel.  -> grid (B,4) fp64, status (B) int32, and with sort: sorted_points (M,3), sorted_keys (M) int64, order (M) int32
    (None without: a brute-force query needs the status alone)."""
    B, M = _cloud_args(points, offsets, "cloud_cell_grid")
    dev = points.device
    grid = torch.empty((B, 4), dtype=torch.float64, device=dev)
    keys = torch.empty((M,), dtype=torch.int64, device=dev)
    cloud = torch.empty((M,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_cell_keys", int(B), int(M), int(mode), int(k), float(cell), points, offsets, grid, keys, cloud, status)
    if not sort:
        return grid, status, None, None, None
    skeys, order = torch.sort(keys, stable=True)
    if B > 1:                                                   # a second stable sort, by cloud: every cloud's rows are one segment again
        _, second = torch.sort(cloud[order], stable=True)
        order, skeys = order[second], skeys[second]
    return grid, status, points[order].contiguous(), skeys.contiguous(), order.to(torch.int32).contiguous()


def cloud_knn_mean(points, offsets, k, cell=None, brute=False):
    """Mean distance of every row to its min(k, n - 1) nearest other rows of its cloud (0 for a cloud of one row), exact for any cell size.
    -> mean (M) fp64 (zeros for a cloud with a status bit), status (B) int32, both still on the device."""
    B, M = _cloud_args(points, offsets, "cloud_knn_mean")
    if not 1 <= int(k) <= CLOUD_MAX_K:
        raise _lib.EtchHipError(f"cloud_knn_mean: k must lie in 1 .. {CLOUD_MAX_K}, got {k}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise _lib.EtchHipError(f"cloud_knn_mean: cell must be positive and finite, got {cell}")
    grid, status, sp, sk, order = cloud_cell_grid(points, offsets, 0, k, 0.0 if cell is None else float(cell), sort=not brute)
    mean = torch.zeros((M,), dtype=torch.float64, device=points.device)
    _lib.call("etch_cloud_knn_mean", int(B), int(M), int(k), int(bool(brute)), points if brute else sp, sk, order, offsets, grid, status, mean)
    return mean, status


def cloud_normals(points, offsets, k, viewpoint=None, cell=None, brute=False, return_cov=False, grid=None):
    """etch_cloud_normals: the normal of every row from its min(k, n - 1) nearest other rows of its cloud, 3 <= k <= 32, on the
    cell grid of cloud_knn_mean (the same rule for the cell size; `cell` overrides it and changes no bit).  viewpoint (B,3) fp64 or None.
    grid: what cloud_cell_grid(points, offsets, 0, k, ..) returned for these points, to share one grid between calls (None: built here).
    -> normal (M,3) fp64, variation (M) fp64, flag (M) int32 (zeros for a cloud with a status bit), status (B) int32, and with return_cov the
    covariance (M,6) fp64, all still on the device."""
    B, M = _cloud_args(points, offsets, "cloud_normals")
    if not 3 <= int(k) <= CLOUD_MAX_K:
        raise _lib.EtchHipError(f"cloud_normals: k must lie in 3 .. {CLOUD_MAX_K}, got {k}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise _lib.EtchHipError(f"cloud_normals: cell must be positive and finite, got {cell}")
    if viewpoint is not None:
        _need(viewpoint, torch.float64, "viewpoint")
        if tuple(viewpoint.shape) != (B, 3):
            raise _lib.EtchHipError(f"cloud_normals: viewpoint must be ({B},3), got {tuple(viewpoint.shape)}")
    dev = points.device
    grid, status, sp, sk, order = cloud_cell_grid(points, offsets, 0, k, 0.0 if cell is None else float(cell), sort=not brute) if grid is None else grid
    normal = torch.zeros((M, 3), dtype=torch.float64, device=dev)
    variation = torch.zeros((M,), dtype=torch.float64, device=dev)
    flag = torch.zeros((M,), dtype=torch.int32, device=dev)
    cov = torch.zeros((M, 6), dtype=torch.float64, device=dev) if return_cov else None
    _lib.call("etch_cloud_normals", int(B), int(M), int(k), int(bool(brute)), points if brute else sp, sk, order, offsets, grid, status, viewpoint,
              normal, variation, flag, cov)
    return (normal, variation, flag, status, cov) if return_cov else (normal, variation, flag, status)


def cloud_radius_count(points, offsets, radius, brute=False):
    """The number of other rows of its cloud within `radius` of every row (d2 <= radius * radius).  -> count (M) int32, status (B) int32."""
    B, M = _cloud_args(points, offsets, "cloud_radius_count")
    if not (float(radius) > 0.0 and math.isfinite(float(radius))):
        raise _lib.EtchHipError(f"cloud_radius_count: radius must be positive and finite, got {radius}")
    _, status, sp, sk, order = cloud_cell_grid(points, offsets, 1, 1, float(radius), sort=not brute)
    count = torch.zeros((M,), dtype=torch.int32, device=points.device)
    _lib.call("etch_cloud_radius_count", int(B), int(M), float(radius), int(bool(brute)), points if brute else sp, sk, order, offsets, status, count)
    return count, status


def cloud_stat_keep(mean, offsets, ratio, status):
    """keep_i = m_i <= mu + ratio s per cloud.  -> keep (M) int32, stats (B,2) fp64 = mu, s; ETCH_CLOUD_STATUS_EMPTY is ORed into status."""
    _need(mean, torch.float64, "mean"), _need(offsets, torch.int32, "offsets"), _need(status, torch.int32, "status")
    B = offsets.numel() - 1
    if B < 1 or status.shape != (B,) or mean.dim() != 1 or not math.isfinite(float(ratio)):
        raise _lib.EtchHipError("cloud_stat_keep: mean must be (M,), status (B,) and ratio finite")
    keep = torch.zeros((mean.numel(),), dtype=torch.int32, device=mean.device)
    stats = torch.zeros((B, 2), dtype=torch.float64, device=mean.device)
    _lib.call("etch_cloud_stat_keep", int(B), float(ratio), mean, offsets, status, stats, keep)
    return keep, stats


def cloud_compact(points, index, offsets, keep):
    """The rows with keep != 0, in row order.  -> kept (B) int32, new offsets (B+1) int32, new index (M) int32 and new points (M,3) fp64 whose
    first new_offsets[B] rows are written."""
    B, M = _cloud_args(points, offsets, "cloud_compact")
    _need(index, torch.int32, "index"), _need(keep, torch.int32, "keep")
    if index.shape != (M,) or keep.shape != (M,):
        raise _lib.EtchHipError(f"cloud_compact: index and keep must be ({M},)")
    dev = points.device
    kept = torch.empty((B,), dtype=torch.int32, device=dev)
    new_offsets = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    new_index = torch.empty((M,), dtype=torch.int32, device=dev)
    new_points = torch.empty((M, 3), dtype=torch.float64, device=dev)
    _lib.call("etch_cloud_compact", int(B), keep, offsets, points, index, _byte_workspace("etch_cloud_scan_workspace", dev, int(B)), kept, new_offsets,
              new_index, new_points)
    return kept, new_offsets, new_index, new_points


def cloud_voxel_grid(points, offsets, voxel):
    """One row per occupied cell of size `voxel` (origin: the cloud's bounding-box minimum), in ascending (ix, iy, iz) order.  -> offsets (B+1)
    int32, centroid (M,3) fp64, count (M) int32, lowest (M) int32 = the cell's lowest row, local to its cloud, cell (M,3) int32, whose first
    offsets[B] rows are written, and status (B) int32."""
    B, M = _cloud_args(points, offsets, "cloud_voxel_grid")
    if not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise _lib.EtchHipError(f"cloud_voxel_grid: voxel must be positive and finite, got {voxel}")
    _, status, sp, sk, order = cloud_cell_grid(points, offsets, 2, 1, float(voxel))
    dev = points.device
    cells = torch.empty((B,), dtype=torch.int32, device=dev)
    out_offsets = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    centroid = torch.empty((M, 3), dtype=torch.float64, device=dev)
    count = torch.zeros((M,), dtype=torch.int32, device=dev)
    lowest = torch.zeros((M,), dtype=torch.int32, device=dev)
    key = torch.zeros((M,), dtype=torch.int64, device=dev)
    _lib.call("etch_cloud_voxel_grid", int(B), sp, sk, order, offsets, status, _byte_workspace("etch_cloud_scan_workspace", dev, int(B)), cells, out_offsets,
              centroid, count, lowest, key)
    cell = torch.stack([key >> 42, (key >> 21) & (2 ** 21 - 1), key & (2 ** 21 - 1)], 1).to(torch.int32)
    return out_offsets, centroid, count, lowest, cell, status


# ------------------------------------------------------------------ isolating the subject (csrc/cloud_isolate.hip)
CLOUD_MAX_HYPOTHESES = 65536


def _plane_args(planes, B, what):
    _need(planes, torch.float64, "planes")
    if planes.dim() != 3 or planes.shape[0] != B or planes.shape[2] != 4 or not 1 <= planes.shape[1] <= CLOUD_MAX_HYPOTHESES:
        raise _lib.EtchHipError(f"{what}: planes must be ({B},H,4) with 1 <= H <= {CLOUD_MAX_HYPOTHESES}, got {tuple(planes.shape)}")
    return planes.shape[1]


def _check_tau(tau, what):
    if not (float(tau) > 0.0 and math.isfinite(float(tau))):
        raise _lib.EtchHipError(f"{what}: tau must be positive and finite, got {tau}")
    return float(tau)


def cloud_plane_hypotheses(points, offsets, keys, hypotheses, up=None, cos_tilt=0.0):
    """etch_cloud_plane_hypotheses: keys (B) int64 holding the uint64 bits, up a UNIT vector of three floats or None.  -> planes (B,H,4) fp64,
    valid (B,H) int32, both still on the device."""
    B, _ = _cloud_args(points, offsets, "cloud_plane_hypotheses")
    _need(keys, torch.int64, "keys")
    H = int(hypotheses)
    if keys.shape != (B,) or not 1 <= H <= CLOUD_MAX_HYPOTHESES:
        raise _lib.EtchHipError(f"cloud_plane_hypotheses: keys must be ({B},) and 1 <= hypotheses <= {CLOUD_MAX_HYPOTHESES}")
    u = (0.0, 0.0, 0.0) if up is None else tuple(float(x) for x in up)
    if len(u) != 3 or not all(math.isfinite(x) for x in u) or not 0.0 <= float(cos_tilt) <= 1.0:
        raise _lib.EtchHipError("cloud_plane_hypotheses: up must be three finite numbers and cos_tilt lie in [0, 1]")
    planes = torch.empty((B, H, 4), dtype=torch.float64, device=points.device)
    valid = torch.empty((B, H), dtype=torch.int32, device=points.device)
    _lib.call("etch_cloud_plane_hypotheses", int(B), H, points, offsets, keys, int(up is not None), u[0], u[1], u[2], float(cos_tilt), planes, valid)
    return planes, valid


def cloud_plane_score(points, offsets, planes, tau, valid=None):
    """etch_cloud_plane_score for ANY planes (B,H,4): -> counts (B,H,3) int32 = inliers, above, below; valid (B,H) int32 or None."""
    B, M = _cloud_args(points, offsets, "cloud_plane_score")
    H, tau = _plane_args(planes, B, "cloud_plane_score"), _check_tau(tau, "cloud_plane_score")
    if valid is not None and _need(valid, torch.int32, "valid").shape != (B, H):
        raise _lib.EtchHipError(f"cloud_plane_score: valid must be ({B},{H})")
    counts = torch.empty((B, H, 3), dtype=torch.int32, device=points.device)
    _lib.call("etch_cloud_plane_score", int(B), int(M), int(H), tau, points, offsets, planes, valid, counts)
    return counts


def cloud_plane_select(planes, valid, counts, min_inliers=3, has_up=False):
    """etch_cloud_plane_select: -> plane (B,4) fp64, counts (B,3) int32, found (B) int32."""
    _need(valid, torch.int32, "valid"), _need(counts, torch.int32, "counts")
    B = planes.shape[0] if planes.dim() == 3 else 0
    H = _plane_args(planes, B, "cloud_plane_select")
    if B < 1 or valid.shape != (B, H) or counts.shape != (B, H, 3):
        raise _lib.EtchHipError(f"cloud_plane_select: valid must be ({B},{H}) and counts ({B},{H},3) with B >= 1")
    plane = torch.empty((B, 4), dtype=torch.float64, device=planes.device)
    best = torch.empty((B, 3), dtype=torch.int32, device=planes.device)
    found = torch.empty((B,), dtype=torch.int32, device=planes.device)
    _lib.call("etch_cloud_plane_select", int(B), int(H), int(bool(has_up)), int(min_inliers), planes, valid, counts, plane, best, found)
    return plane, best, found


def _one_plane_args(points, offsets, plane, found, what):
    B, M = _cloud_args(points, offsets, what)
    _need(plane, torch.float64, "plane"), _need(found, torch.int32, "found")
    if plane.shape != (B, 4) or found.shape != (B,):
        raise _lib.EtchHipError(f"{what}: plane must be ({B},4) and found ({B},)")
    return B, M


def cloud_plane_refit(points, offsets, plane, counts, found, tau):
    """etch_cloud_plane_refit: one least-squares step on the inliers of every found plane.  -> new plane (B,4), new counts (B,3); the arguments
    are left unchanged."""
    B, _ = _one_plane_args(points, offsets, plane, found, "cloud_plane_refit")
    if _need(counts, torch.int32, "counts").shape != (B, 3):
        raise _lib.EtchHipError(f"cloud_plane_refit: counts must be ({B},3)")
    plane, counts = plane.clone(), counts.clone()
    _lib.call("etch_cloud_plane_refit", int(B), _check_tau(tau, "cloud_plane_refit"), points, offsets, found, plane, counts)
    return plane, counts


def cloud_plane_keep(points, offsets, plane, found, tau):
    """keep (M) int32 = the rows more than tau above a found plane (every row of a cloud without one)."""
    B, M = _one_plane_args(points, offsets, plane, found, "cloud_plane_keep")
    keep = torch.zeros((M,), dtype=torch.int32, device=points.device)
    _lib.call("etch_cloud_plane_keep", int(B), int(M), _check_tau(tau, "cloud_plane_keep"), points, offsets, plane, found, keep)
    return keep


def cloud_components(points, offsets, radius, brute=False):
    """Connected components of the radius graph (d2 <= radius * radius) per cloud.  -> label (M) int32 = the lowest row of the row's component,
    local to its cloud, size (M) int32 = the component's rows, status (B) int32."""
    B, M = _cloud_args(points, offsets, "cloud_components")
    if not (float(radius) > 0.0 and math.isfinite(float(radius))):
        raise _lib.EtchHipError(f"cloud_components: radius must be positive and finite, got {radius}")
    _, status, sp, sk, order = cloud_cell_grid(points, offsets, 1, 1, float(radius), sort=not brute)
    dev = points.device
    parent = torch.empty((M,), dtype=torch.int32, device=dev)
    label = torch.zeros((M,), dtype=torch.int32, device=dev)
    size = torch.zeros((M,), dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_components", int(B), int(M), float(radius), int(bool(brute)), points if brute else sp, sk, order, offsets, status, parent, label, size)
    return label, size, status


def cloud_component_keep(label, size, offsets, largest=True, min_points=1):
    """keep (M) int32 = size >= min_points and (not largest or label == the largest component's, a tie to the lowest label); winner (B) int32."""
    _need(label, torch.int32, "label"), _need(size, torch.int32, "size"), _need(offsets, torch.int32, "offsets")
    B = offsets.numel() - 1
    if B < 1 or label.dim() != 1 or size.shape != label.shape or int(min_points) < 1:
        raise _lib.EtchHipError("cloud_component_keep: label and size must be (M,), offsets (B+1) with B >= 1 and min_points >= 1")
    keep = torch.zeros(label.shape, dtype=torch.int32, device=label.device)
    winner = torch.empty((B,), dtype=torch.int32, device=label.device)
    _lib.call("etch_cloud_component_keep", int(B), int(bool(largest)), int(min_points), label, size, offsets, winner, keep)
    return keep, winner


# ------------------------------------------------------------------ registering views (csrc/cloud_align.hip)
ALIGN_STATUS_DEGENERATE = 8


def _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, what):
    B, Ms = _cloud_args(src_points, src_offsets, what)
    Bt, Mt = _cloud_args(tgt_points, tgt_offsets, what)
    if Bt != B:
        raise _lib.EtchHipError(f"{what}: {B} source clouds but {Bt} target clouds")
    return B, Ms, Mt


def _align_transform(R, t, B, dev, what):
    """R (B,3,3), t (B,3) fp64 on the device, the identity where None; always fresh tensors the library may write."""
    R = torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1) if R is None else _need(R, torch.float64, "R").reshape(-1, 3, 3).clone().contiguous()
    t = torch.zeros((B, 3), dtype=torch.float64, device=dev) if t is None else _need(t, torch.float64, "t").reshape(-1, 3).clone().contiguous()
    if R.shape != (B, 3, 3) or t.shape != (B, 3):
        raise _lib.EtchHipError(f"{what}: R must be ({B},3,3) and t ({B},3), got {tuple(R.shape)} and {tuple(t.shape)}")
    return R, t


def _some(t):
    """A tensor the library can take the address of: an empty one has none, and no row of it is ever read."""
    return t if t is None or t.numel() else t.new_zeros((1,) + tuple(t.shape[1:]))


def _check_gate(gate, cell, what):
    if not (float(gate) > 0.0 and math.isfinite(float(gate))):
        raise _lib.EtchHipError(f"{what}: gate must be positive and finite, got {gate}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise _lib.EtchHipError(f"{what}: cell must be positive and finite, got {cell}")
    return float(gate), 0.0 if cell is None else float(cell)


def cloud_align_grid(points, offsets, gate, cell=None, sort=True):
    """The TARGET's cell grid for etch_cloud_nearest (the header states the cell rule; cell= overrides it) and the stable sort of its rows by
    (cloud, key).  -> grid (B,4), center (B,3) fp64, status (B) int32, and with sort: sorted_points (M,3), sorted_keys (M) int64, order (M) int32."""
    B, M = _cloud_args(points, offsets, "cloud_align_grid")
    gate, cell = _check_gate(gate, cell, "cloud_align_grid")
    dev = points.device
    grid = torch.empty((B, 4), dtype=torch.float64, device=dev)
    center = torch.empty((B, 3), dtype=torch.float64, device=dev)
    keys = torch.empty((M,), dtype=torch.int64, device=dev)
    cloud = torch.empty((M,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_align_grid", int(B), int(M), gate, cell, _some(points), offsets, grid, center, _some(keys), _some(cloud), status)
    if not sort:
        return grid, center, status, None, None, None
    skeys, order = torch.sort(keys, stable=True)
    if B > 1:
        _, second = torch.sort(cloud[order], stable=True)
        order, skeys = order[second], skeys[second]
    return grid, center, status, points[order].contiguous(), skeys.contiguous(), order.to(torch.int32).contiguous()


def _query_order(src_points, src_offsets, gate, cell):
    """The source rows in the order of their own cells: neighbours share a wave, and a rigid motion keeps them neighbours."""
    return cloud_align_grid(src_points, src_offsets, gate, cell if cell else None)[5]


def cloud_nearest(src_points, src_offsets, tgt_points, tgt_offsets, gate, R=None, t=None, cell=None, brute=False):
    """etch_cloud_nearest: the nearest row of target cloud b within `gate` of every moved row R_b p + t_b of source cloud b.  -> pair (Ms) int32
    (the row local to its cloud, -1 without one), d2 (Ms) fp64 (+inf without one), status (B) int32, all still on the device."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_nearest")
    gate, cell = _check_gate(gate, cell, "cloud_nearest")
    dev = src_points.device
    R, t = _align_transform(R, t, B, dev, "cloud_nearest")
    grid, _, status, sp, sk, order = cloud_align_grid(tgt_points, tgt_offsets, gate, cell if cell else None, sort=not brute)
    qorder = None if brute else _query_order(src_points, src_offsets, gate, cell)
    pair = torch.full((Ms,), -1, dtype=torch.int32, device=dev)
    d2 = torch.full((Ms,), math.inf, dtype=torch.float64, device=dev)
    g = torch.tensor([gate], dtype=torch.float64, device=dev)
    _lib.call("etch_cloud_nearest", int(B), int(Ms), int(bool(brute)), _some(src_points), src_offsets, qorder, _some(tgt_points if brute else sp), _some(sk), _some(order),
              tgt_offsets, grid, R, t, g, None, status, _some(pair), _some(d2))
    return pair, d2, status


def _align_state(B, Ms, dev):
    z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=dev)                                    # noqa: E731
    return dict(sums=z(B, 16), matched=z(B, dtype=torch.int32), rms=z(B), dR=z(B, 3, 3), dt=z(B, 3), done=z(B, dtype=torch.int32),
                steps=z(B, dtype=torch.int32))


def cloud_align_step(src_points, src_offsets, tgt_points, tgt_offsets, pair, d2=None, R=None, t=None):
    """etch_cloud_align_step: one rigid step from the given pairs (pair (Ms) int32: the matched row of the target cloud, local to it, or -1).
    -> dR (B,3,3), dt (B,3), m (B) int32, sums (B,16), then status (B) int32 and the composed R (B,3,3), t (B,3) -- unchanged where the status
    holds ALIGN_STATUS_DEGENERATE."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_align_step")
    _need(pair, torch.int32, "pair")
    if pair.shape != (Ms,) or (d2 is not None and _need(d2, torch.float64, "d2").shape != (Ms,)):
        raise _lib.EtchHipError(f"cloud_align_step: pair and d2 must be ({Ms},)")
    dev = src_points.device
    R, t = _align_transform(R, t, B, dev, "cloud_align_step")
    _, center, status, _, _, _ = cloud_align_grid(tgt_points, tgt_offsets, 1.0, sort=False)
    s = _align_state(B, Ms, dev)
    _lib.call("etch_cloud_align_step", int(B), _some(src_points), src_offsets, _some(tgt_points), tgt_offsets, _some(pair), d2, center, 0.0, 0.0, R, t, s["sums"], s["matched"],
              s["rms"], s["dR"], s["dt"], status, s["done"], s["steps"])
    return s["dR"], s["dt"], s["matched"], s["sums"], status, R, t


def _align_normals(tgt_normals, Mt, what):
    _need(tgt_normals, torch.float64, "tgt_normals")
    if tuple(tgt_normals.shape) != (Mt, 3):
        raise _lib.EtchHipError(f"{what}: tgt_normals must be ({Mt},3), got {tuple(tgt_normals.shape)}")
    return tgt_normals


def cloud_align_step_plane(src_points, src_offsets, tgt_points, tgt_offsets, tgt_normals, pair, d2=None, R=None, t=None):
    """etch_cloud_align_step_plane: one point-to-plane step from the given pairs and the target's normals (Mt,3).
    -> dR (B,3,3), dt (B,3), m (B) int32, sums (B,32), y (B,6) = omega, tau, then status (B) int32 and the composed R (B,3,3), t (B,3) -- unchanged
    where the status holds ALIGN_STATUS_DEGENERATE."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_align_step_plane")
    _need(pair, torch.int32, "pair")
    if pair.shape != (Ms,) or (d2 is not None and _need(d2, torch.float64, "d2").shape != (Ms,)):
        raise _lib.EtchHipError(f"cloud_align_step_plane: pair and d2 must be ({Ms},)")
    _align_normals(tgt_normals, Mt, "cloud_align_step_plane")
    dev = src_points.device
    R, t = _align_transform(R, t, B, dev, "cloud_align_step_plane")
    grid, center, status, _, _, _ = cloud_align_grid(tgt_points, tgt_offsets, 1.0, sort=False)
    s = _align_state(B, Ms, dev)
    sums = torch.zeros((B, 32), dtype=torch.float64, device=dev)
    y = torch.zeros((B, 6), dtype=torch.float64, device=dev)
    _lib.call("etch_cloud_align_step_plane", int(B), _some(src_points), src_offsets, _some(tgt_points), _some(tgt_normals), tgt_offsets, _some(pair), d2, grid,
              center, 0.0, 0.0, R, t, sums, s["matched"], s["rms"], s["dR"], s["dt"], y, status, s["done"], s["steps"])
    return s["dR"], s["dt"], s["matched"], sums, y, status, R, t


def cloud_align(src_points, src_offsets, tgt_points, tgt_offsets, gates, tol_angle, tol_shift, R=None, t=None, cell=None, brute=False, tgt_normals=None):
    """etch_cloud_align: len(gates) steps of nearest + rigid step, the target's grid built once, no host synchronisation.  gates: the gate of every
    step, host floats.  tgt_normals (Mt,3) fp64: the point-to-plane step of etch_cloud_align_plane instead of Horn's (None: the point metric).
    -> a dict of device tensors: R (B,3,3), t (B,3), matched (B) int32, rms (B), steps (B) int32, status (B) int32, pair (Ms)
    int32 and d2 (Ms) of the last matching, done (B) int32."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_align")
    if tgt_normals is not None:
        _align_normals(tgt_normals, Mt, "cloud_align")
    gates = [float(g) for g in gates]
    if not gates or not all(g > 0.0 and math.isfinite(g) for g in gates):
        raise _lib.EtchHipError("cloud_align: gates must be a non-empty list of positive finite numbers")
    if not (float(tol_angle) >= 0.0 and float(tol_shift) >= 0.0):
        raise _lib.EtchHipError("cloud_align: the tolerances must not be negative")
    _, cell = _check_gate(gates[0], cell, "cloud_align")
    dev = src_points.device
    R, t = _align_transform(R, t, B, dev, "cloud_align")
    grid, center, status, sp, sk, order = cloud_align_grid(tgt_points, tgt_offsets, max(gates), cell if cell else None, sort=not brute)
    qorder = None if brute else _query_order(src_points, src_offsets, max(gates), cell)
    s = _align_state(B, Ms, dev)
    pair = torch.full((Ms,), -1, dtype=torch.int32, device=dev)
    d2 = torch.full((Ms,), math.inf, dtype=torch.float64, device=dev)
    g = torch.tensor(gates, dtype=torch.float64, device=dev)
    if tgt_normals is not None:
        sums = torch.zeros((B, 32), dtype=torch.float64, device=dev)
        _lib.call("etch_cloud_align_plane", int(B), int(Ms), len(gates), int(bool(brute)), _some(src_points), src_offsets, qorder, _some(sp), _some(sk), _some(order),
                  _some(tgt_points), _some(tgt_normals), tgt_offsets, grid, center, g, float(tol_angle), float(tol_shift), R, t, sums, s["matched"], s["rms"], s["dR"],
                  s["dt"], status, s["done"], s["steps"], _some(pair), _some(d2))
        return dict(R=R, t=t, matched=s["matched"], rms=s["rms"], steps=s["steps"], status=status, pair=pair, d2=d2, done=s["done"])
    _lib.call("etch_cloud_align", int(B), int(Ms), len(gates), int(bool(brute)), _some(src_points), src_offsets, qorder, _some(sp), _some(sk), _some(order), _some(tgt_points),
              tgt_offsets, grid, center, g, float(tol_angle), float(tol_shift), R, t, s["sums"], s["matched"], s["rms"], s["dR"], s["dt"], status, s["done"],
              s["steps"], _some(pair), _some(d2))
    return dict(R=R, t=t, matched=s["matched"], rms=s["rms"], steps=s["steps"], status=status, pair=pair, d2=d2, done=s["done"])


def cloud_transform(points, offsets, R, t):
    """out (M,3) = R_b p + t_b for every row of cloud b (zeros behind the last cloud)."""
    B, M = _cloud_args(points, offsets, "cloud_transform")
    R, t = _align_transform(R, t, B, points.device, "cloud_transform")
    out = torch.zeros((M, 3), dtype=torch.float64, device=points.device)
    _lib.call("etch_cloud_transform", int(B), int(M), _some(points), offsets, R, t, _some(out))
    return out


# ------------------------------------------------------------------ global registration (csrc/cloud_global.hip)
GLOBAL_FEATURES = 33
GLOBAL_MAX_HYPOTHESES = 262144


def cloud_fpfh(points, offsets, normal, normal_flag, k, cell=None, brute=False, grid=None):
    """etch_cloud_fpfh: the FPFH descriptor of every row from its min(k, n - 1) nearest other rows, 3 <= k <= 32, on the cell grid of cloud_normals
    (`cell` overrides the cell size and changes no bit; brute=True scans every cloud whole).  normal (M,3) fp64: unit normals oriented consistently,
    normal_flag (M) int32, both by row.  -> feature (M,33) fp64, has_feature (M) int32, spfh (M,33) int32, count (M) int32, neighbours (M,k) int32
    (rows local to the cloud, -1 behind the last), status (B) int32, all still on the device.  grid: what cloud_cell_grid(points, offsets, 0, k, ..)
    returned for these points (None: built here); cloud_normals takes the same, so that normals and descriptors share one grid and one sort."""
    B, M = _cloud_args(points, offsets, "cloud_fpfh")
    if not 3 <= int(k) <= CLOUD_MAX_K:
        raise _lib.EtchHipError(f"cloud_fpfh: k must lie in 3 .. {CLOUD_MAX_K}, got {k}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise _lib.EtchHipError(f"cloud_fpfh: cell must be positive and finite, got {cell}")
    _need(normal, torch.float64, "normal"), _need(normal_flag, torch.int32, "normal_flag")
    if tuple(normal.shape) != (M, 3) or tuple(normal_flag.shape) != (M,):
        raise _lib.EtchHipError(f"cloud_fpfh: normal must be ({M},3) and normal_flag ({M},), got {tuple(normal.shape)} and {tuple(normal_flag.shape)}")
    dev = points.device
    grid, status, sp, sk, order = cloud_cell_grid(points, offsets, 0, k, 0.0 if cell is None else float(cell), sort=not brute) if grid is None else grid
    feature = torch.zeros((M, GLOBAL_FEATURES), dtype=torch.float64, device=dev)
    has = torch.zeros((M,), dtype=torch.int32, device=dev)
    spfh = torch.zeros((M, GLOBAL_FEATURES), dtype=torch.int32, device=dev)
    count = torch.zeros((M,), dtype=torch.int32, device=dev)
    nbr = torch.full((M, int(k)), -1, dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_fpfh", int(B), int(M), int(k), int(bool(brute)), _some(points if brute else sp), sk, order, _some(points), offsets, grid, status,
              _some(normal), _some(normal_flag), _some(spfh), _some(count), _some(nbr), _some(feature), _some(has))
    return feature, has, spfh, count, nbr, status


def _feature_args(feature, has, offsets, what):
    _need(feature, torch.float64, "feature"), _need(has, torch.int32, "has_feature"), _need(offsets, torch.int32, "offsets")
    if feature.dim() != 2 or feature.shape[1] != GLOBAL_FEATURES or tuple(has.shape) != (feature.shape[0],) or offsets.dim() != 1 or offsets.numel() < 2:
        raise _lib.EtchHipError(f"{what}: feature must be (M,{GLOBAL_FEATURES}), has_feature (M,) and offsets (B+1), got {tuple(feature.shape)}, "
                                f"{tuple(has.shape)} and {tuple(offsets.shape)}")
    return offsets.numel() - 1, feature.shape[0]


def cloud_feature_match(src_feature, src_has, src_offsets, tgt_feature, tgt_has, tgt_offsets):
    """etch_cloud_feature_match: for every source row with a feature the row of target cloud b with a feature and the least (D, row).
    -> match (Ms) int32 (local to the cloud, -1 without one), dist (Ms) fp64 (+inf without one), on the device."""
    B, Ms = _feature_args(src_feature, src_has, src_offsets, "cloud_feature_match")
    Bt, _ = _feature_args(tgt_feature, tgt_has, tgt_offsets, "cloud_feature_match")
    if Bt != B:
        raise _lib.EtchHipError(f"cloud_feature_match: {B} source clouds but {Bt} target clouds")
    match = torch.full((Ms,), -1, dtype=torch.int32, device=src_feature.device)
    dist = torch.full((Ms,), math.inf, dtype=torch.float64, device=src_feature.device)
    _lib.call("etch_cloud_feature_match", int(B), int(Ms), _some(src_feature), _some(src_has), src_offsets, _some(tgt_feature), _some(tgt_has), tgt_offsets,
              _some(match), _some(dist))
    return match, dist


def cloud_correspondences(src_points, src_offsets, tgt_points, tgt_offsets, match):
    """The matched source rows of every pair in ascending row order, compacted on the device (etch_cloud_compact on match >= 0).  -> corr_src (Ms,3)
    fp64, corr_tgt (Ms,3) fp64, corr_row (Ms) int32 = the matched target row, corr_offsets (B+1) int32, corr_index (Ms) int32 = the source row (both
    rows local to their cloud); only the first corr_offsets[B] rows mean anything."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_correspondences")
    _need(match, torch.int32, "match")
    if tuple(match.shape) != (Ms,):
        raise _lib.EtchHipError(f"cloud_correspondences: match must be ({Ms},)")
    dev = src_points.device
    if Ms == 0 or Mt == 0:
        z = torch.zeros((Ms, 3), dtype=torch.float64, device=dev)
        return z, z.clone(), torch.zeros((Ms,), dtype=torch.int32, device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev), torch.zeros((Ms,), dtype=torch.int32, device=dev)
    rows = torch.arange(Ms, dtype=torch.int32, device=dev)
    _, coff, packed, corr_src = cloud_compact(src_points, rows, src_offsets, (match >= 0).to(torch.int32))
    g = packed.long().clamp_(0, Ms - 1)                              # behind corr_offsets[B] the compaction wrote nothing: any row in range does
    cloud = torch.bucketize(g, src_offsets[1:].long().contiguous(), right=True).clamp_(max=B - 1)
    corr_row = match[g]
    corr_tgt = tgt_points[(tgt_offsets.long()[cloud] + corr_row.long()).clamp_(0, Mt - 1)].contiguous()
    return corr_src, corr_tgt, corr_row.contiguous(), coff, (g - src_offsets.long()[cloud]).to(torch.int32)


def _corr_args(corr_src, corr_tgt, corr_offsets, what):
    _need(corr_src, torch.float64, "corr_src"), _need(corr_tgt, torch.float64, "corr_tgt"), _need(corr_offsets, torch.int32, "corr_offsets")
    if corr_src.dim() != 2 or corr_src.shape[1] != 3 or corr_tgt.shape != corr_src.shape or corr_offsets.dim() != 1 or corr_offsets.numel() < 2:
        raise _lib.EtchHipError(f"{what}: corr_src and corr_tgt must be (N,3) and corr_offsets (B+1), got {tuple(corr_src.shape)}, {tuple(corr_tgt.shape)} and "
                                f"{tuple(corr_offsets.shape)}")
    return corr_offsets.numel() - 1, corr_src.shape[0]


def _transform_args(transforms, B, what):
    _need(transforms, torch.float64, "transforms")
    if transforms.dim() != 3 or transforms.shape[0] != B or transforms.shape[2] != 12 or not 1 <= transforms.shape[1] <= GLOBAL_MAX_HYPOTHESES:
        raise _lib.EtchHipError(f"{what}: transforms must be ({B},H,12) with 1 <= H <= {GLOBAL_MAX_HYPOTHESES}, got {tuple(transforms.shape)}")
    return transforms.shape[1]


def cloud_global_hypotheses(corr_src, corr_tgt, corr_row, corr_offsets, keys, hypotheses, edge_similarity=0.9, min_edge=0.05):
    """etch_cloud_global_hypotheses: keys (B) int64 holding the uint64 bits.  -> transforms (B,H,12) fp64 = R row-major and t, valid (B,H) int32,
    triples (B,H,3) int32 = the three correspondences drawn, all still on the device."""
    B, N = _corr_args(corr_src, corr_tgt, corr_offsets, "cloud_global_hypotheses")
    _need(corr_row, torch.int32, "corr_row"), _need(keys, torch.int64, "keys")
    H = int(hypotheses)
    if tuple(corr_row.shape) != (N,) or tuple(keys.shape) != (B,) or not 1 <= H <= GLOBAL_MAX_HYPOTHESES:
        raise _lib.EtchHipError(f"cloud_global_hypotheses: corr_row must be ({N},), keys ({B},) and 1 <= hypotheses <= {GLOBAL_MAX_HYPOTHESES}")
    if not 0.0 < float(edge_similarity) <= 1.0 or not (float(min_edge) >= 0.0 and math.isfinite(float(min_edge))):
        raise _lib.EtchHipError("cloud_global_hypotheses: edge_similarity must lie in (0, 1] and min_edge be finite and not negative")
    dev = corr_src.device
    transforms = torch.empty((B, H, 12), dtype=torch.float64, device=dev)
    valid = torch.empty((B, H), dtype=torch.int32, device=dev)
    triples = torch.empty((B, H, 3), dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_global_hypotheses", int(B), H, _some(corr_src), _some(corr_tgt), _some(corr_row), corr_offsets, keys, float(edge_similarity),
              float(min_edge), transforms, valid, triples)
    return transforms, valid, triples


def cloud_global_score(corr_src, corr_tgt, corr_offsets, transforms, tau, valid=None):
    """etch_cloud_global_score for ANY transforms (B,H,12): -> inliers (B,H) int32; valid (B,H) int32 or None."""
    B, N = _corr_args(corr_src, corr_tgt, corr_offsets, "cloud_global_score")
    H, tau = _transform_args(transforms, B, "cloud_global_score"), _check_tau(tau, "cloud_global_score")
    if valid is not None and tuple(_need(valid, torch.int32, "valid").shape) != (B, H):
        raise _lib.EtchHipError(f"cloud_global_score: valid must be ({B},{H})")
    inliers = torch.empty((B, H), dtype=torch.int32, device=corr_src.device)
    _lib.call("etch_cloud_global_score", int(B), int(N), int(H), tau, _some(corr_src), _some(corr_tgt), corr_offsets, transforms, valid, inliers)
    return inliers


def cloud_global_select(transforms, valid, inliers, min_inliers=6):
    """etch_cloud_global_select: -> R (B,3,3), t (B,3) fp64, best (B) int32 = the winner's inliers, best_h (B) int32, found (B) int32."""
    _need(valid, torch.int32, "valid"), _need(inliers, torch.int32, "inliers")
    B = transforms.shape[0] if transforms.dim() == 3 else 0
    H = _transform_args(transforms, B, "cloud_global_select")
    if B < 1 or tuple(valid.shape) != (B, H) or tuple(inliers.shape) != (B, H):
        raise _lib.EtchHipError(f"cloud_global_select: valid and inliers must be ({B},{H}) with B >= 1")
    dev = transforms.device
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    best, best_h, found = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    _lib.call("etch_cloud_global_select", int(B), int(H), int(min_inliers), transforms, valid, inliers, R, t, best, best_h, found)
    return R, t, best, best_h, found


def cloud_global_inliers(src_points, src_offsets, tgt_points, tgt_offsets, match, R, t, tau):
    """etch_cloud_global_inliers: pair (Ms) int32 = match where the moved source row lies within tau of its matched target row, else -1."""
    B, Ms, Mt = _align_pairs(src_points, src_offsets, tgt_points, tgt_offsets, "cloud_global_inliers")
    _need(match, torch.int32, "match")
    if tuple(match.shape) != (Ms,):
        raise _lib.EtchHipError(f"cloud_global_inliers: match must be ({Ms},)")
    R, t = _align_transform(R, t, B, src_points.device, "cloud_global_inliers")
    pair = torch.full((Ms,), -1, dtype=torch.int32, device=src_points.device)
    _lib.call("etch_cloud_global_inliers", int(B), int(Ms), _check_tau(tau, "cloud_global_inliers"), _some(src_points), src_offsets, _some(tgt_points), tgt_offsets,
              _some(match), R, t, _some(pair))
    return pair


# ------------------------------------------------------------------ point winding numbers (csrc/cloud_winding.hip)
def cloud_knn_kth(points, offsets, k, cell=None, brute=False, grid=None):
    """etch_cloud_knn_kth: d2 of every row to its min(k, n - 1)-th nearest other row of its cloud (0 for a cloud of one row), 3 <= k <= 32, on the
    cell grid of cloud_knn_mean; `cell` and brute change no bit.  grid: what cloud_cell_grid(points, offsets, 0, k, ..) returned, to share one.
    -> d2k (M) fp64 by original row (zeros for a cloud with a status bit), status (B) int32, both still on the device."""
    B, M = _cloud_args(points, offsets, "cloud_knn_kth")
    if not 3 <= int(k) <= CLOUD_MAX_K:
        raise _lib.EtchHipError(f"cloud_knn_kth: k must lie in 3 .. {CLOUD_MAX_K}, got {k}")
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise _lib.EtchHipError(f"cloud_knn_kth: cell must be positive and finite, got {cell}")
    grid, status, sp, sk, order = cloud_cell_grid(points, offsets, 0, k, 0.0 if cell is None else float(cell), sort=not brute) if grid is None else grid
    d2k = torch.zeros((M,), dtype=torch.float64, device=points.device)
    _lib.call("etch_cloud_knn_kth", int(B), int(M), int(k), int(bool(brute)), points if brute else sp, sk, order, offsets, grid, status, d2k)
    return d2k, status


def cloud_surface_pack(points, offsets, normal, flag, d2k, k, center=None):
    """etch_cloud_surface_pack: points (M,3), normal (M,3) oriented unit normals, d2k (M) fp64 and flag (M) int32 by original row, k the k of d2k,
    center (B,3) fp64 or None -> pos (M,3), moment (M,3), cap (M) fp32: the rows cloud_winding_number reads (zeros behind the last cloud)."""
    B, M = _cloud_args(points, offsets, "cloud_surface_pack")
    if not 3 <= int(k) <= CLOUD_MAX_K:
        raise _lib.EtchHipError(f"cloud_surface_pack: k must lie in 3 .. {CLOUD_MAX_K}, got {k}")
    _need(normal, torch.float64, "normal"), _need(flag, torch.int32, "flag"), _need(d2k, torch.float64, "d2k")
    if tuple(normal.shape) != (M, 3) or tuple(flag.shape) != (M,) or tuple(d2k.shape) != (M,):
        raise _lib.EtchHipError(f"cloud_surface_pack: normal ({M},3), flag ({M},), d2k ({M},), got {tuple(normal.shape)}, {tuple(flag.shape)}, {tuple(d2k.shape)}")
    if center is not None:
        _need(center, torch.float64, "center")
        if tuple(center.shape) != (B, 3):
            raise _lib.EtchHipError(f"cloud_surface_pack: center must be ({B},3), got {tuple(center.shape)}")
    dev = points.device
    pos = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    moment = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    cap = torch.zeros((M,), dtype=torch.float32, device=dev)
    _lib.call("etch_cloud_surface_pack", int(B), int(M), int(k), points, normal, flag, d2k, offsets, center, pos, moment, cap)
    return pos, moment, cap


def _oriented_cloud_args(cloud, B, what):
    """cloud = (pos (M,3), moment (M,3), cap (M) fp32, offsets (B+1) int32, max_rows), or an object with these attributes (cloud.OrientedCloud):
    the packed batch of cloud_surface_pack -> the four tensors and max_rows, shapes and dtypes checked.  The offsets stay on the device: max_rows
    is the caller's (a host integer known when the batch was packed)."""
    if isinstance(cloud, (tuple, list)):
        if len(cloud) != 5:
            raise _lib.EtchHipError(f"{what}: the oriented cloud is (pos, moment, cap, offsets, max_rows)")
        pos, moment, cap, offsets, max_rows = cloud
    else:
        pos, moment, cap, offsets, max_rows = cloud.pos, cloud.moment, cloud.cap, cloud.offsets, cloud.max_rows
    _need(pos, torch.float32, "pos"), _need(moment, torch.float32, "moment"), _need(cap, torch.float32, "cap"), _need(offsets, torch.int32, "offsets")
    M = pos.shape[0]
    if pos.dim() != 2 or pos.shape[1] != 3 or tuple(moment.shape) != (M, 3) or tuple(cap.shape) != (M,) or tuple(offsets.shape) != (B + 1,):
        raise _lib.EtchHipError(f"{what}: pos (M,3), moment (M,3), cap (M,), offsets ({B + 1},), got {tuple(pos.shape)}, {tuple(moment.shape)}, "
                                f"{tuple(cap.shape)}, {tuple(offsets.shape)}")
    if int(max_rows) < 0 or int(max_rows) > M:
        raise _lib.EtchHipError(f"{what}: max_rows must lie in [0, {M}], got {max_rows}")
    return pos, moment, cap, offsets, int(max_rows)


def cloud_winding_number(cloud, queries, lengths=None, want_nearest=True):
    """etch_cloud_winding_number: the winding number of the oriented cloud b (_oriented_cloud_args) at queries (B,Q,3) fp32 (lengths (B,) for ragged
    query sets) and, from the same pass, the nearest row.  -> w (B,Q) fp32, nearest (B,Q) int32 local to the cloud (-1: none), nearest_d2 (B,Q)
    fp32 (the last two None without want_nearest).  Padding gets 0, -1, 0.  Bitwise reproducible; cloud b alone = cloud b in a batch."""
    B, Q = _queries(queries, "queries")
    pos, moment, cap, offsets, mr = _oriented_cloud_args(cloud, B, "cloud_winding_number")
    ql = _lengths(lengths, B, Q, queries.device, "lengths")
    ws = _byte_workspace("etch_cloud_winding_number_workspace", queries.device, B, Q, mr)
    dev = queries.device
    w = torch.empty((B, Q), dtype=torch.float32, device=dev)
    nearest = torch.empty((B, Q), dtype=torch.int32, device=dev) if want_nearest else None
    d2 = torch.empty((B, Q), dtype=torch.float32, device=dev) if want_nearest else None
    _lib.call("etch_cloud_winding_number", B, Q, mr, pos, moment, cap, offsets, queries, ql, ws, w, nearest, d2)
    return w, nearest, d2


def cloud_containment_energy_grad(body_verts, cloud, w, nearest, nearest_d2, coef=None, w_contain=1.0, g=None):
    """containment_energy_grad against an oriented cloud: o_v = [|w_v| < 0.5] with a nearest row, c_v = that row's position (a sample of the
    surface) -> terms (B,2) fp64 = {sum_v o_v nearest_d2_v, sum_v o_v} and g (B,V,3) (given: updated IN PLACE; None: zeros first) with
    coef_b w_contain (2 / V) o_v (v - c_v) added.  -> (terms, g)."""
    B, V = _queries(body_verts, "body_verts")
    pos, _, _, offsets, _ = _oriented_cloud_args(cloud, B, "cloud_containment_energy_grad")
    if tuple(w.shape) != (B, V) or tuple(nearest.shape) != (B, V) or tuple(nearest_d2.shape) != (B, V):
        raise _lib.EtchHipError(f"cloud_containment_energy_grad: w, nearest and nearest_d2 must be ({B},{V})")
    _need(w, torch.float32, "w"), _need(nearest, torch.int32, "nearest"), _need(nearest_d2, torch.float32, "nearest_d2")
    if coef is not None:
        coef = _need(coef.to(torch.float32).contiguous(), torch.float32, "coef")
        if tuple(coef.shape) != (B,):
            raise _lib.EtchHipError(f"coef must be ({B},)")
    if g is None:
        g = torch.zeros_like(body_verts)
    elif tuple(g.shape) != (B, V, 3):
        raise _lib.EtchHipError(f"g must be ({B},{V},3)")
    _need(g, torch.float32, "g")
    ws = _byte_workspace("etch_cloud_containment_energy_grad_workspace", body_verts.device, B, V)
    terms = torch.zeros((B, 2), dtype=torch.float64, device=body_verts.device)
    _lib.call("etch_cloud_containment_energy_grad", B, V, body_verts, pos, offsets, w, nearest, nearest_d2, coef, float(w_contain), ws, terms, g)
    _lib.wrote(g)
    return terms, g


def smpl_surface_refine_contain_cloud(consts, faces, points, params, scan, lengths=None, weights=None, markers=None, prior=None, iters=200, lr=2e-2,
                                      beta1=0.9, beta2=0.999, eps=1e-8, w_dense=1e2, w_marker=1.0, w_beta=1e-2, w_prior=1e-7, trunc=0.05,
                                      optimize_scale=False, w_contain=1e2, contain_every=10, nj=24, nb=10, n_extra=21, want_trace=False):
    """smpl_surface_refine_contain with scan = an oriented cloud in the body's frame (_oriented_cloud_args): at iterations 0, K, 2K, ... one pass
    of cloud_winding_number over the current vertices gives o_v and the row c_v each outside vertex is pulled to; held in between.
    params is updated IN PLACE.  -> verts, joints, loss of the last forward (B,), loss trace (B, iters, 5) or None."""
    _need(points, torch.float32, "points"), _need(params, torch.float32, "params"), _need(faces, torch.int32, "faces")
    _check_body(consts, nj, nb, n_extra)
    V = int(consts[0].shape[0])
    if points.dim() != 3 or points.shape[2] != 3 or tuple(params.shape) != (points.shape[0], 3 * nj + nb + 4) or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"points must be (B,N,3), params (B, {3 * nj + nb + 4}), faces (F,3)")
    B, N, _ = points.shape
    F = int(faces.shape[0])
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise _lib.EtchHipError(f"face vertex ids must lie in [0, {V})")
    if int(contain_every) < 1:
        raise _lib.EtchHipError("contain_every must be at least 1")
    pos, moment, cap, offsets, mr = _oriented_cloud_args(scan, B, "smpl_surface_refine_contain_cloud")
    nl = _lengths(lengths, B, N, points.device, "lengths")
    if weights is not None:
        weights = _need(weights.to(torch.float32).contiguous(), torch.float32, "weights")
        if tuple(weights.shape) != (B, N):
            raise _lib.EtchHipError(f"weights must be ({B},{N})")
    M, vids, mpos, valid = _marker_args(markers, B, V, points.device)
    arr = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in consts])
    G, parr = 0, None
    if prior is not None:
        means, prec, w = (_need(t, torch.float32, n) for t, n in zip(prior, ("means", "precisions", "nll_weights")))
        G = int(w.shape[0])
        if tuple(w.shape) != (G,) or tuple(means.shape) != (G, 69) or tuple(prec.shape) != (G, 69, 69):
            raise _lib.EtchHipError("prior: means (G,69), precisions (G,69,69), nll_weights (G,)")
        parr = (ctypes.c_void_p * 3)(means.data_ptr(), prec.data_ptr(), w.data_ptr())
    ws = _byte_workspace("etch_smpl_surface_refine_contain_cloud_workspace", points.device, B, N, V, int(nj), int(nb), int(n_extra), mr)
    verts = torch.empty((B, V, 3), dtype=torch.float32, device=points.device)
    joints = torch.empty((B, nj + n_extra, 3), dtype=torch.float32, device=points.device)
    loss = torch.empty((B,), dtype=torch.float32, device=points.device)
    tr = torch.empty((B, iters, 5), dtype=torch.float32, device=points.device) if want_trace else None
    _lib.call("etch_smpl_surface_refine_contain_cloud", B, N, V, F, int(nj), int(nb), int(n_extra), arr, faces, points, nl, weights, M, vids, mpos, valid, parr,
              G, int(iters), float(lr), float(beta1), float(beta2), float(eps), float(w_dense), float(w_marker), float(w_beta), float(w_prior), float(trunc),
              int(bool(optimize_scale)), mr, pos, moment, cap, offsets, float(w_contain), int(contain_every), params, verts, joints, tr, loss, ws)
    _lib.wrote(params)
    return verts, joints, loss, tr


# ------------------------------------------------------------------ a mesh from the winding field (csrc/cloud_mesh.hip)
MESH_BLOCK_NODES = 729
MESH_BLOCK_CELLS = 512
MESH_TABLE_INACTIVE, MESH_TABLE_MARK = -1, -2


def _mesh_cloud(cloud, what):
    B = int(cloud[3].numel() if isinstance(cloud, (tuple, list)) else cloud.offsets.numel()) - 1
    return (B,) + _oriented_cloud_args(cloud, B, what)


def _mesh_voxel(voxel, what):
    if not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise _lib.EtchHipError(f"{what}: voxel must be positive and finite, got {voxel}")
    return float(voxel)


def _mesh_slots(lattice, slots, B, what):
    _need(lattice, torch.int32, "lattice"), _need(slots, torch.int32, "slots")
    if tuple(lattice.shape) != (B, 6) or slots.dim() != 2 or slots.shape[1] != 2:
        raise _lib.EtchHipError(f"{what}: lattice must be ({B},6) and slots (S,2), got {tuple(lattice.shape)} and {tuple(slots.shape)}")
    return int(slots.shape[0])


def cloud_mesh_lattice(cloud, voxel, pad_blocks=2):
    """etch_cloud_mesh_lattice: the block lattice of every oriented cloud -> lattice (B,6) int32 = lo, hi in blocks, status (B) int32
    (CLOUD_STATUS_EMPTY, CLOUD_STATUS_RANGE), both still on the device."""
    B, pos, _, cap, offsets, mr = _mesh_cloud(cloud, "cloud_mesh_lattice")
    lattice = torch.zeros((B, 6), dtype=torch.int32, device=offsets.device)
    status = torch.zeros((B,), dtype=torch.int32, device=offsets.device)
    _lib.call("etch_cloud_mesh_lattice", B, mr, pos, cap, offsets, _mesh_voxel(voxel, "cloud_mesh_lattice"), int(pad_blocks), lattice, status)
    return lattice, status


def cloud_mesh_seed(cloud, voxel, seed_dilate, lattice, status, table_offsets, table):
    """etch_cloud_mesh_seed: marks (MESH_TABLE_MARK) the blocks of round 0 in table (int32, cloud b's blocks from table_offsets[b] on, (B+1) int64 on
    the device), IN PLACE."""
    B, pos, _, cap, offsets, mr = _mesh_cloud(cloud, "cloud_mesh_seed")
    _need(lattice, torch.int32, "lattice"), _need(status, torch.int32, "status"), _need(table_offsets, torch.int64, "table_offsets"), _need(table, torch.int32, "table")
    if tuple(lattice.shape) != (B, 6) or tuple(status.shape) != (B,) or tuple(table_offsets.shape) != (B + 1,) or table.dim() != 1:
        raise _lib.EtchHipError(f"cloud_mesh_seed: lattice ({B},6), status ({B},), table_offsets ({B + 1},), table (T,)")
    _lib.call("etch_cloud_mesh_seed", B, mr, pos, cap, offsets, _mesh_voxel(voxel, "cloud_mesh_seed"), int(seed_dilate), lattice, status, table_offsets, table)
    _lib.wrote(table)
    return table


def cloud_mesh_field(cloud, voxel, level, lattice, slots):
    """etch_cloud_mesh_field: s = |w| - level at the 729 nodes of the blocks slots (S,2) int32 = (cloud, index in the cloud's table) -> (S,729) fp32;
    w is cloud_winding_number's at the node's fp32 position, to the bit."""
    B, pos, moment, cap, offsets, mr = _mesh_cloud(cloud, "cloud_mesh_field")
    S = _mesh_slots(lattice, slots, B, "cloud_mesh_field")
    field = torch.zeros((S, MESH_BLOCK_NODES), dtype=torch.float32, device=offsets.device)
    _lib.call("etch_cloud_mesh_field", B, S, mr, pos, moment, cap, offsets, _mesh_voxel(voxel, "cloud_mesh_field"), float(level), lattice, slots, field)
    return field


def cloud_mesh_grow(lattice, table_offsets, slots, field, table):
    """etch_cloud_mesh_grow: the face test of the blocks `slots` with their `field` (S,729); marks neighbours in table IN PLACE.
    -> flags (S,6) int32: 1 = mixed towards a block without a slot, 2 = mixed and out of the lattice."""
    B = int(lattice.shape[0])
    S = _mesh_slots(lattice, slots, B, "cloud_mesh_grow")
    _need(field, torch.float32, "field"), _need(table_offsets, torch.int64, "table_offsets"), _need(table, torch.int32, "table")
    if tuple(field.shape) != (S, MESH_BLOCK_NODES) or tuple(table_offsets.shape) != (B + 1,):
        raise _lib.EtchHipError(f"cloud_mesh_grow: field must be ({S},{MESH_BLOCK_NODES}) and table_offsets ({B + 1},)")
    flags = torch.zeros((S, 6), dtype=torch.int32, device=field.device)
    _lib.call("etch_cloud_mesh_grow", B, S, lattice, table_offsets, slots, field, table, flags)
    _lib.wrote(table)
    return flags


def cloud_mesh_extract(lattice, voxel, slots, field):
    """etch_cloud_mesh_extract, both launches: the counts, their prefix sum (torch.cumsum, one read of the total), the faces.  slots sorted by
    (cloud, block) give the faces in DESIGN section 27's order.  -> counts (S,512) int32, face_keys (F,3) int64, face_pos (F,3,3) fp32."""
    B = int(lattice.shape[0])
    S = _mesh_slots(lattice, slots, B, "cloud_mesh_extract")
    _need(field, torch.float32, "field")
    if tuple(field.shape) != (S, MESH_BLOCK_NODES):
        raise _lib.EtchHipError(f"cloud_mesh_extract: field must be ({S},{MESH_BLOCK_NODES}), got {tuple(field.shape)}")
    h, dev = _mesh_voxel(voxel, "cloud_mesh_extract"), field.device
    counts = torch.zeros((S, MESH_BLOCK_CELLS), dtype=torch.int32, device=dev)
    _lib.call("etch_cloud_mesh_extract", B, S, 0, lattice, h, slots, field, counts, None, None, None)
    inclusive = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    F = int(inclusive[-1]) if S else 0
    keys = torch.zeros((F, 3), dtype=torch.int64, device=dev)
    fpos = torch.zeros((F, 3, 3), dtype=torch.float32, device=dev)
    if F:
        cell_offsets = (inclusive - counts.reshape(-1)).contiguous()
        _lib.call("etch_cloud_mesh_extract", B, S, F, lattice, h, slots, field, None, cell_offsets, keys, fpos)
    return counts, keys, fpos


def cloud_mesh_weld(face_keys, face_pos):
    """Integer welding of ONE cloud's faces: the distinct keys in ascending order (torch.unique) are the vertices.  -> vertex keys (V) int64,
    verts (V,3) fp32, faces (F,3) int32.  A key has the same position bits wherever it was produced, so any of its copies serves."""
    keys, inverse = torch.unique(face_keys.reshape(-1), sorted=True, return_inverse=True)
    verts = torch.zeros((keys.numel(), 3), dtype=torch.float32, device=face_keys.device)
    verts[inverse] = face_pos.reshape(-1, 3)
    return keys, verts, inverse.reshape(-1, 3).to(torch.int32).contiguous()


def mesh_components(V, faces, passes=4):
    """etch_mesh_components until no label changes (one int32 read per `passes` rounds) -> labels (V) int32: the lowest vertex of each component."""
    _need(faces, torch.int32, "faces")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.EtchHipError(f"mesh_components: faces must be (F,3), got {tuple(faces.shape)}")
    labels = torch.zeros((int(V),), dtype=torch.int32, device=faces.device)
    changed = torch.zeros((1,), dtype=torch.int32, device=faces.device)
    init = 1
    while True:
        _lib.call("etch_mesh_components", int(V), int(faces.shape[0]), faces, init, int(passes), labels, changed)
        init = 0
        if not int(changed[0]):
            return labels


def mesh_keep_component(verts, faces, labels, label):
    """etch_mesh_keep_component: the vertices and faces of the component `label`, order kept, re-indexed (the prefix sums are torch.cumsum)."""
    _need(verts, torch.float32, "verts"), _need(faces, torch.int32, "faces"), _need(labels, torch.int32, "labels")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if tuple(verts.shape) != (V, 3) or tuple(faces.shape) != (F, 3) or tuple(labels.shape) != (V,):
        raise _lib.EtchHipError("mesh_keep_component: verts (V,3), faces (F,3), labels (V,)")
    kv = labels == int(label)
    vp = torch.cumsum(kv, 0, dtype=torch.int64)
    fp = torch.cumsum(kv[faces[:, 0].long()], 0, dtype=torch.int64) if F else torch.zeros((0,), dtype=torch.int64, device=verts.device)
    nv, nf = (int(vp[-1]) if V else 0), (int(fp[-1]) if F else 0)
    out_v = torch.zeros((nv, 3), dtype=torch.float32, device=verts.device)
    out_f = torch.zeros((nf, 3), dtype=torch.int32, device=verts.device)
    _lib.call("etch_mesh_keep_component", V, F, verts, faces, labels, int(label), vp, fp, nv, nf, out_v, out_f)
    return out_v, out_f
