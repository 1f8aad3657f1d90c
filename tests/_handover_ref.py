"""Plain numpy references, inputs and checkers of the kernels that hand data from one stage to the next: etch_prop3nn, etch_prop_interp[_ordered]
(csrc/heads.hip), etch_argmax_rows, etch_inner_points, etch_get_markers, etch_marker_status (csrc/smpl_fit.hip).

Every checker is `check_x(got, inputs)`: it raises AssertionError on a miss and returns the observed maximum in the unit of its bound.  The same
function judges GPU output (tests/test_gpu_handover.py) and host-made wrong answers (tests/test_handover_host.py).  The inputs are built here, once, so
both files see the same arrays.  Every bound is derived where it is used; U = 2^-24 bounds the relative error of one correctly rounded fp32 operation.

The order of confidences and logits, this project's definition (torch.max / torch.topk wherever those define one): any NaN is greater than every
number, +0 and -0 are equal, equal values go to the lower index."""
import functools
import itertools

import numpy as np

U = 2.0 ** -24
SIGMA = np.array([0.14, 0.31, 0.085])       # the scans' own shape
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]      # what 0/0 gives on the host
POS_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
F32, F64 = np.float32, np.float64


def same_bits(a, b):
    """fp32 arrays equal bit for bit, except that any NaN equals any NaN (the payload a NaN carries through an operation is the hardware's own)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ================================================================================================ 3-NN
P3_SHAPES = [(3, 255), (3, 257), (4, 1), (4, 257), (1023, 255), (1023, 257), (1024, 1), (1024, 256), (1024, 257), (1025, 255), (1025, 257),
             (2049, 1), (2049, 256), (2049, 257)]          # (S, N): every S meets an N below 256 and one above it


@functools.lru_cache(maxsize=None)
def p3_lattice(S, N):
    """xyz1 (2,N,3), xyz2 (2,3,S): integer multiples of 1/8 in [-2, 2], so every product and sum of d = ((-2 dot) + |x|^2) + |y|^2 is exact in fp32.
    Coarse: S//3 repeats 0; 1024 repeats 5 where it is not the last one (an exact tie between the first and the second LDS tile); the last one,
    (2,2,2), is no other's place.  Fine: 0 sits on the last coarse point (d = 0, a unique nearest neighbour in the last tile), 1 on coarse 5."""
    xyz1, xyz2 = np.empty((2, N, 3), F32), np.empty((2, 3, S), F32)
    for b in range(2):
        rng = np.random.default_rng(1000 * S + 10 * N + b)
        c = rng.integers(-16, 17, (S, 3))
        c[(c == 16).all(1)] = 15
        c[S // 3] = c[0]
        if S - 1 > 1024:
            c[1024] = c[5]
        c[S - 1] = 16
        f = rng.integers(-16, 17, (N, 3))
        f[0] = c[S - 1]
        if N > 1:
            f[1] = c[5 % S]
        xyz1[b], xyz2[b] = f / 8.0, c.T / 8.0
    return {"xyz1": xyz1, "xyz2": xyz2}


@functools.lru_cache(maxsize=None)
def p3_gauss(S, N):
    """Gaussian clouds of the scans' shape, different per scan; fine point 0 lies 1 mm off the last coarse point and, where there is a second LDS
    tile, the last fine point 1 mm off its first entry, coarse 1024."""
    rng = np.random.default_rng(77 * S + N)
    xyz1, xyz2 = (rng.standard_normal((2, N, 3)) * SIGMA).astype(F32), (rng.standard_normal((2, S, 3)) * SIGMA).astype(F32)
    xyz1[:, 0] = xyz2[:, S - 1] + F32(1e-3)
    if S > 1024:
        xyz1[:, N - 1] = xyz2[:, 1024] - F32(1e-3)
    return {"xyz1": xyz1, "xyz2": np.ascontiguousarray(xyz2.transpose(0, 2, 1))}


def p3_sqdist(inputs):
    """(B,N,S) fp64 squared distances in the kernel's own expansion (exact on the lattice; elsewhere fp64's error is 2^-29 of the fp32 one)."""
    x, y = inputs["xyz1"].astype(F64), inputs["xyz2"].astype(F64).transpose(0, 2, 1)
    return ((-2.0 * np.einsum("bnc,bsc->bns", x, y)) + (x * x).sum(-1)[:, :, None]) + (y * y).sum(-1)[:, None, :]


def p3_weights(d3):
    """fp64 w_k = r_k / ((r_0 + r_1) + r_2), r_k = 1 / (d_k + 1e-8) with the kernel's constant, the fp32 number next to 1e-8."""
    r = 1.0 / (d3 + F64(F32(1e-8)))
    return r / ((r[..., 0] + r[..., 1]) + r[..., 2])[..., None]


def p3_lattice_ref(inputs, d=None):
    d = p3_sqdist(inputs) if d is None else d
    idx = np.argsort(d, axis=-1, kind="stable")[..., :3]
    return idx.astype(np.int32), p3_weights(np.take_along_axis(d, idx, -1))


def check_p3_lattice(got, inputs):
    """idx equal to the stable ascending order's first three; weights within 6 U relative of their fp64 values: two roundings in r, two more in the
    norm, one division, at most U each.  Returns max relative weight error / U."""
    idx, w = got
    ridx, rw = p3_lattice_ref(inputs)
    assert idx.dtype == np.int32 and idx.shape == ridx.shape
    bad = (idx != ridx).any(-1)
    assert not bad.any(), f"3-NN indices differ at {int(bad.sum())} fine points, first (scan, point) {tuple(int(v) for v in np.argwhere(bad)[0])}: " \
                          f"{idx[bad][0]} for {ridx[bad][0]}"
    rel = float((np.abs(w.astype(F64) - rw) / rw).max())
    assert rel <= 6 * U, f"3-NN weight relative error {rel / U:.2f} U > 6 U"
    return rel / U


def check_p3_gauss(got, inputs):
    """Against fp64 squared distances D: indices distinct and in range; D[idx_r] <= sort(D)[r] + tol with tol = 8 U (|x|^2 + max |y|^2) per fine
    point (three products and two sums in dot, doubled, plus two more sums); weights finite and summing to 1 within 3 U (two roundings in the norm
    and one per division, weighted by w) where all three D > tol.  Returns (max excess / tol, max |sum - 1| / U)."""
    idx, w = got
    x, y = inputs["xyz1"].astype(F64), inputs["xyz2"].astype(F64).transpose(0, 2, 1)
    S = y.shape[1]
    D = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    assert idx.dtype == np.int32 and idx.shape == D.shape[:2] + (3,)
    assert ((idx >= 0) & (idx < S)).all(), "3-NN index out of range"
    assert (idx[..., 0] != idx[..., 1]).all() and (idx[..., 0] != idx[..., 2]).all() and (idx[..., 1] != idx[..., 2]).all(), "3-NN indices repeat"
    tol = 8 * U * ((x * x).sum(-1) + (y * y).sum(-1).max(1)[:, None])
    dg = np.take_along_axis(D, idx.astype(np.int64), -1)
    excess = float(((dg - np.sort(D, -1)[..., :3]) / tol[..., None]).max())
    assert excess <= 1.0, f"3-NN picked a neighbour {excess:.2f} tol farther than the rank's nearest"
    clear = (dg > tol[..., None]).all(-1)
    assert clear.any()
    assert np.isfinite(w[clear]).all(), "3-NN weight not finite"
    dev = float(np.abs(w[clear].astype(F64).sum(-1) - 1.0).max())
    assert dev <= 3 * U, f"3-NN weights sum to 1 +- {dev / U:.2f} U > 3 U"
    return max(excess, 0.0), dev / U


# ================================================================================================ interpolation
PI_S, PI_NS, PI_CS, PI_AS = 5, (1, 9, 16), (32, 64, 128, 256), (1, 7, 60)
PI_ORDERS = ("none", "identity", "permutation")


@functools.lru_cache(maxsize=None)
def pi_inputs(C, A, N):
    """feats (2,S,A,C); idx / weight (2 N + 1, 3) and order (2 N + 8,): one guard row and eight guard slots (pointing at the guard row) past the
    end, which no launch may touch.  Row 0 of each scan hits coarse rows 0 and S - 1 and repeats one, row 1 repeats a neighbour."""
    S = PI_S
    rng = np.random.default_rng(100 * C + 10 * A + N)
    idx = np.zeros((2 * N + 1, 3), np.int32)
    w = np.full((2 * N + 1, 3), 1 / 3, F32)
    idx[:2 * N] = rng.integers(0, S, (2 * N, 3))
    r = rng.random((2 * N, 3)) + 0.01
    w[:2 * N] = (r / r.sum(-1, keepdims=True)).astype(F32)
    for b in range(2):
        idx[b * N] = (0, S - 1, S - 1)
        if N > 1:
            idx[b * N + 1] = (2, 2, 4)
    orders = {"none": None}
    for name in ("identity", "permutation"):
        o = np.full(2 * N + 8, N, np.int32)
        for b in range(2):
            o[b * N:(b + 1) * N] = np.arange(N) if name == "identity" else rng.permutation(N)
        orders[name] = o
    return {"B": 2, "N": N, "S": S, "A": A, "C": C, "feats": rng.standard_normal((2, S, A, C)).astype(F32), "idx": idx, "weight": w, "orders": orders}


def pi_ref(inputs):
    """numpy fp32, every operation rounded on its own: (f0 w0 + f1 w1) + f2 w2."""
    B, N, A, C = inputs["B"], inputs["N"], inputs["A"], inputs["C"]
    idx, w = inputs["idx"][:B * N].reshape(B, N, 3), inputs["weight"][:B * N].reshape(B, N, 3, 1, 1)
    f = np.stack([inputs["feats"][b][idx[b]] for b in range(B)])                 # (B,N,3,A,C)
    out = (f[:, :, 0] * w[:, :, 0] + f[:, :, 1] * w[:, :, 1]) + f[:, :, 2] * w[:, :, 2]
    assert out.dtype == F32
    return out.reshape(B * N, A, C)


def check_interp(got, inputs):
    """got = out (B N + 1, A, C), inv (B N + 1, C), both prefilled with NaN.  out bit-equal to pi_ref; inv within (A + 1) U mean_a |out| of the
    fp64 anchor mean of the kernel's own out (A - 1 sums, the rounding of 1/A, one product); the guard rows still NaN.  Returns max inv err / bound."""
    out, inv = got
    rows, A = inputs["B"] * inputs["N"], inputs["A"]
    assert not np.isnan(out[:rows]).any() and not np.isnan(inv[:rows]).any(), "interp left a row unwritten"
    assert same_bits(out[:rows], pi_ref(inputs)), "interp out differs from (f0 w0 + f1 w1) + f2 w2 in fp32"
    assert np.isnan(out[rows:]).all() and np.isnan(inv[rows:]).all(), "interp wrote past the last fine point"
    o64 = out[:rows].astype(F64)
    err = np.abs(inv[:rows].astype(F64) - o64.mean(1))
    bound = (A + 1) * U * np.abs(o64).mean(1)
    worst = float((err / bound).max())
    assert worst <= 1.0, f"interp anchor mean off by {worst:.2f} of (A + 1) U mean|out|"
    return worst


# ================================================================================================ arg-max
AM_GS, AM_RS = (1, 5, 63, 64, 65, 86, 129, 200), (1, 3, 4, 5, 1031)
AM_BIG = (2097200, 2)        # past 65535 * 8 workgroups of 4 rows: the row-stride loop
AM_PLANTS = 9


def _plant(row, kind, rng):
    """One edge per row; the row's other values are finite and below 50."""
    G = len(row)
    if kind == 0 and G > 64:                    # tie within one lane's passes
        g = int(rng.integers(0, G - 64))
        row[g] = row[g + 64] = 100.0
    elif kind == 1 and G > 1:                   # tie across lanes
        a, b = sorted(rng.choice(min(G, 64), 2, replace=False))
        row[a] = row[b] = 100.0
    elif kind == 2:                             # maximum in the last column
        row[G - 1] = 100.0
    elif kind == 3:
        row[:] = -np.inf
    elif kind in (4, 5) and G > 1:              # -0 and +0, the only non-negative values
        g = int(rng.integers(0, G - 1))
        row[:] = -1.0 - np.abs(row)
        row[g], row[g + 1] = (-0.0, 0.0) if kind == 4 else (0.0, -0.0)
    elif kind in (6, 7) and G > 1:              # +inf first, then a NaN of either sign
        g = int(rng.integers(0, G - 1))
        row[g], row[g + 1] = np.inf, (POS_NAN if kind == 6 else NEG_NAN)
    elif kind == 8 and G > 2:                   # two NaNs, the negative one first, and +inf
        row[G - 1], row[G - 2], row[0] = POS_NAN, NEG_NAN, np.inf


@functools.lru_cache(maxsize=None)
def am_input(R, G):
    rng = np.random.default_rng(31 * R + G)
    if (R, G) == AM_BIG:
        return np.array([-1.0, -0.0, 0.0, 1.0, -np.inf, np.inf, NEG_NAN, POS_NAN], F32)[rng.integers(0, 8, (R, G))]
    x = (rng.integers(-40, 41, (R, G)) / 4.0).astype(F32)          # quarter steps: ties everywhere
    for r in range(R):
        _plant(x[r], (r + G) % AM_PLANTS, rng)
    return x


def am_edge_rows():
    n, p, i = NEG_NAN, POS_NAN, np.inf
    return np.array([[-0.0, 0.0], [0.0, -0.0], [n, i], [i, n], [p, i], [i, p], [n, p], [p, n], [-i, -i], [-i, n], [1.0, 1.0], [-0.0, -1.0]], F32)


def am_inputs():
    yield "edges", am_edge_rows()
    for G in AM_GS:
        for R in AM_RS:
            yield f"R={R} G={G}", am_input(R, G)
    yield "R=%d G=%d" % AM_BIG, am_input(*AM_BIG)


def argmax_ref(x):
    """First maximum, +-0 equal, any NaN greatest (the first NaN wins)."""
    nan = np.isnan(x)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, x).argmax(-1)).astype(np.int64)


def check_argmax(got, inputs):
    ref = argmax_ref(inputs)
    assert got.dtype == np.int64 and got.shape == ref.shape
    bad = got != ref
    assert not bad.any(), f"argmax differs in {int(bad.sum())} rows, first row {np.argwhere(bad)[0]}: {inputs[bad][0][:8]} -> {got[bad][0]} for {ref[bad][0]}"
    return 0


# ================================================================================================ inner points
IP_SHAPES = ((1, 1), (1, 85), (1, 86), (2, 500))      # 3 n = 255 and 258 straddle one workgroup's 256 elements
IP_SCALE = 10.0


@functools.lru_cache(maxsize=None)
def ip_inputs(B, N):
    rng = np.random.default_rng(5 * N + B)
    pts = (rng.standard_normal((B, N, 3)) * SIGMA).astype(F32)
    d = rng.standard_normal((B, N, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    mag = (rng.random((B, N, 1)) * 0.8).astype(F32)
    pts[0, 0, 0] = np.inf
    d[B - 1, N - 1, 2] = np.nan
    return {"pts": pts, "dir": d, "mag": mag, "scale": IP_SCALE}


def inner_ref(inputs):
    with np.errstate(invalid="ignore"):
        out = inputs["pts"] - (inputs["dir"] * inputs["mag"]) / F32(inputs["scale"])
    assert out.dtype == F32
    return out


def check_inner(got, inputs):
    """Bit-equal to numpy fp32 pts - (dir mag) / scale; the inf and the NaN stay in their own element."""
    ref = inner_ref(inputs)
    assert same_bits(got, ref), f"inner points differ in {int((got != ref).sum() - np.isnan(ref).sum())} finite elements"
    B, N = got.shape[:2]
    assert np.array_equal(np.argwhere(~np.isfinite(got)), np.array([[0, 0, 0], [B - 1, N - 1, 2]])), "a non-finite input spread beyond its own element"
    return 0


# ================================================================================================ markers
MK_SHAPES = tuple(itertools.product((3, 86), (1, 63, 64, 65, 200, 1000)))
MK_IGNORED = (-1, None, 300)          # None stands for M


def rank_order(cand, c):
    """The candidates in the order of the definition: NaN greatest, +-0 equal, ties to the lower index."""
    nan = np.isnan(c)
    return cand[np.lexsort((cand, -np.where(nan, 0.0, c).astype(F64), ~nan))]


def select_top3(labels, conf, m):
    cand = np.flatnonzero(labels == m)
    return rank_order(cand, conf[cand])[:3]


def markers_ref(inputs, select=select_top3):
    """sel[b][m] (indices, best first), centres (B,M,3) fp64 = sum p w / sum w with w = c^20 as the fp32 number it is (it underflows to 0 below
    c = 0.0127; 0/0 and 0 inf are NaN as in the kernel), valid (B,M)."""
    pts, labels, conf, M = inputs["pts"], inputs["labels"], inputs["conf"][..., 0], inputs["M"]
    B = labels.shape[0]
    sel = [[select(labels[b], conf[b], m) for m in range(M)] for b in range(B)]
    centres, valid = np.zeros((B, M, 3)), np.zeros((B, M), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            for m in range(M):
                s = sel[b][m]
                if len(s):
                    w = (conf[b, s].astype(F64) ** 20).astype(F32).astype(F64)
                    centres[b, m] = (pts[b, s].astype(F64) * w[:, None]).sum(0) / w.sum()
                    valid[b, m] = True
    return sel, centres, valid


def markers_from(inputs, select):
    """What a kernel that selected by `select` would have returned: (markers fp32, valid_f, valid_b)."""
    _, c, v = markers_ref(inputs, select)
    return c.astype(F32), v.astype(F32), v.copy()


def _mk_tol(inputs, sel):
    """32 U max |p_selected| per (scan, label): three fused products and sums, one division, powf at a few ulp on each weight."""
    B, M = inputs["labels"].shape[0], inputs["M"]
    tol = np.zeros((B, M))
    for b in range(B):
        for m in range(M):
            p = np.abs(inputs["pts"][b, sel[b][m]].astype(F64))
            p = p[np.isfinite(p)]
            tol[b, m] = 32 * U * (p.max() if p.size else 0.0)
    return tol


def check_markers(got, inputs):
    """valid as the reference's and valid_f == valid_b; invalid markers exactly zero; NaN components where the reference has them and nowhere
    else; the others within 32 U max |p_selected| of the fp64 centre.  Returns max error / bound."""
    markers, valid_f, valid_b = got
    if "_ref" not in inputs:
        inputs["_ref"] = markers_ref(inputs)
    sel, ref, valid = inputs["_ref"]
    assert valid_b.dtype == bool and np.array_equal(valid_b, valid), "valid differs from the reference's"
    assert valid_f.dtype == F32 and np.array_equal(valid_f, valid.astype(F32)), "valid_f differs from valid_b"
    assert (markers[~valid].view(np.uint32) == 0).all(), "an invalid marker is not exactly zero"
    nan = np.isnan(ref)
    bad = np.isnan(markers) != nan
    assert not bad.any(), f"NaN components differ at (scan, label, axis) {[tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]]}: got {markers[bad][:4]}"
    err = np.where(nan, 0.0, np.abs(markers.astype(F64) - np.where(nan, 0.0, ref)))
    tol = _mk_tol(inputs, sel)[..., None]
    ratio = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
    worst = float(ratio.max())
    assert (err[np.broadcast_to(tol == 0, err.shape)] == 0).all() and worst <= 1.0, \
        f"marker centre off by {worst:.1f} of 32 U max|p| at (scan, label, axis) {tuple(int(v) for v in np.argwhere(ratio == ratio.max())[0])}"
    return worst


def _conf(rng, n):
    return (0.9 + 0.1 * rng.random(n)).astype(F32)          # c^20 in [0.12, 1): every selected point carries at least 4 % of the weight


@functools.lru_cache(maxsize=None)
def mk_random(M, K):
    """Labels over -1 .. M + 1 (-1, M and 300 are nobody's), confidences on eight levels so that ties straddle rank 3 in most labels."""
    rng = np.random.default_rng(1000 * M + K)
    labels = rng.integers(-1, M + 2, (2, K)).astype(np.int64)
    labels[labels == M + 1] = 300
    conf = (0.9 + rng.integers(0, 8, (2, K, 1)) / 80.0).astype(F32)
    conf[labels[..., None] >= M] = 0.999
    if K == 1:
        labels[0, 0] = 0
    return {"M": M, "pts": (rng.standard_normal((2, K, 3)) * SIGMA).astype(F32), "labels": labels, "conf": conf}


MK_SCENES = ("no point", "one point", "two points", "three points", "four points", "one lane ascending", "one lane descending", "one lane mixed",
             "five lanes", "four equal", "negative", "-0 before +0", "+0 before -0", "positive NaN", "negative NaN", "underflow")


@functools.lru_cache(maxsize=None)
def mk_scenes():
    """M = 86, K = 1000, two scans.  Scene j of MK_SCENES has label j in scan 0 and 85 - j in scan 1; the labels in between are background, about
    13 points each.  The signed-zero scenes show which zero was taken through a point at x = inf: its weight is 0 and 0 inf is NaN."""
    M, K = 86, 1000
    rng = np.random.default_rng(86)
    pts = (rng.standard_normal((2, K, 3)) * SIGMA).astype(F32)
    labels = np.empty((2, K), np.int64)
    conf = np.empty((2, K), F32)
    lane7 = 7 + 64 * np.arange(15)
    for b in range(2):
        lab = (lambda j: j) if b == 0 else (lambda j: 85 - j)
        n_sc = len(MK_SCENES)
        labels[b] = [lab(j) for j in rng.integers(n_sc, M - n_sc, K)]
        conf[b] = _conf(rng, K)
        ign = rng.choice(np.setdiff1d(np.arange(K), lane7), 30, replace=False)
        labels[b, ign] = np.resize([-1, M, 300], 30)
        conf[b, ign] = 0.9999
        free = list(rng.permutation(np.setdiff1d(np.arange(K), np.concatenate([lane7, ign, np.arange(10, 271, 65)]))))
        take = lambda n: np.sort([free.pop() for _ in range(n)])

        def put(j, where, c):
            labels[b, where], conf[b, where] = lab(j), np.asarray(c, F32)

        for j, n in ((1, 1), (2, 2), (3, 3), (4, 4)):
            put(j, take(n), _conf(rng, n))
        put(5, lane7[0:5], [.90, .92, .94, .96, .98])
        put(6, lane7[5:10], [.98, .96, .94, .92, .90])
        put(7, lane7[10:15], [.94, .98, .90, .96, .92])
        put(8, np.arange(10, 271, 65), [.94, .98, .90, .96, .92])          # lanes 10, 11, 12, 13, 14
        put(9, take(5), [.93, .93, .97, .93, .93])
        put(10, take(4), [-.99, -.90, -.96, -.93])
        z = take(4)
        put(11, z, [.95, -0.0, 0.0, .92])
        pts[b, z[1], 0] = np.inf
        z = take(4)
        put(12, z, [.95, 0.0, -0.0, .92])
        pts[b, z[2], 0] = np.inf
        put(13, take(5), [.95, .91, .99, POS_NAN, .93])
        put(14, take(5), [.95, .91, .99, NEG_NAN, .93])
        put(15, take(4), [1e-3, 1e-3, 1e-3, 1e-3])
        assert not (labels[b] == lab(0)).any()
    return {"M": M, "pts": pts, "labels": labels, "conf": conf[..., None]}


def mk_inputs():
    yield "scenes M=86 K=1000", mk_scenes()
    for M, K in MK_SHAPES:
        yield f"random M={M} K={K}", mk_random(M, K)


def swap_margin(inputs):
    """The smallest change of a centre, in units of its bound, over every exchange of one selected point for one left-out point of the same label
    (labels whose centre is NaN aside): above 1 it is the selected SET that check_markers pins, not only the centre."""
    sel, ref, _ = markers_ref(inputs)
    tol = _mk_tol(inputs, sel)
    pts, conf = inputs["pts"].astype(F64), inputs["conf"][..., 0].astype(F64)
    worst = np.inf
    for b in range(len(sel)):
        for m in range(inputs["M"]):
            s = sel[b][m]
            rest = np.setdiff1d(np.flatnonzero(inputs["labels"][b] == m), s)
            if np.isnan(ref[b, m]).any() or not len(rest):
                continue
            for k in range(len(s)):
                keep = np.delete(s, k)
                wk, wr = conf[b, keep] ** 20, conf[b, rest] ** 20
                with np.errstate(invalid="ignore"):                 # a left-out point at x = inf with weight 0
                    c = ((pts[b, keep] * wk[:, None]).sum(0) + pts[b, rest] * wr[:, None]) / (wk.sum() + wr)[:, None]
                d = np.abs(c - ref[b, m]).max(-1)
                d = d[~np.isnan(d)]                  # an exchange that turns the centre into NaN is seen as such
                if d.size:
                    worst = min(worst, float(d.min() / tol[b, m]))
    return worst


# ================================================================================================ marker status
MS_MS = (1, 64, 65, 86)


@functools.lru_cache(maxsize=None)
def ms_inputs(M, bad):
    """Three scans, three outcomes: 0 (its only non-finite marker is not valid), 1 (a valid marker holds `bad`, at m >= 64 where M allows: the lane
    loop's second pass), 2 (no valid marker, non-finite ones among them)."""
    bad = {"inf": np.inf, "-inf": -np.inf, "nan": np.nan}[bad]
    rng = np.random.default_rng(M)
    markers = rng.standard_normal((3, M, 3)).astype(F32)
    valid = np.ones((3, M), F32)
    if M > 1:
        markers[0, M // 2, 1] = bad
        valid[0, M // 2] = 0
        valid[1, 0] = 0
    markers[1, M - 1, 2] = bad
    valid[2] = 0
    markers[2, 0, 0] = bad
    return {"markers": markers, "valid_f": valid}


def status_ref(inputs):
    v = inputs["valid_f"] != 0
    bad = (v & ~np.isfinite(inputs["markers"]).all(-1)).any(-1)
    return (bad.astype(np.int32) | np.where(v.any(-1), 0, 2)).astype(np.int32)


def check_status(got, inputs):
    ref = status_ref(inputs)
    assert got.dtype == np.int32 and np.array_equal(got, ref), f"marker status {got} for {ref}"
    return 0


# ================================================================================================ the chain
@functools.lru_cache(maxsize=None)
def chain_inputs():
    """Logits (2,130,86) on quarter steps (ties), with a -0 / +0 pair and a NaN of either sign as row maxima; labels 3 and 50 favoured so that
    they get more than three points; scan 1 has one marker that is 0/0."""
    rng = np.random.default_rng(130)
    logits = (rng.integers(-20, 21, (2, 130, 86)) / 4.0).astype(F32)
    logits[:, ::5, 3] = 8.0
    logits[:, 1::7, 50] = 8.0
    logits[0, 2] = -1.0 - np.abs(logits[0, 2])
    logits[0, 2, 40], logits[0, 2, 41] = -0.0, 0.0
    logits[1, 4, 9], logits[1, 4, 10] = np.inf, NEG_NAN
    logits[1, 6, 9], logits[1, 6, 12] = np.inf, POS_NAN
    logits[1, :, 77] = -10.0
    logits[1, 8, 77] = 9.0                      # the only point of label 77, and its confidence underflows: a NaN marker, status 1
    conf = _conf(rng, (2, 130, 1))
    conf[1, 8] = 1e-3
    d = rng.standard_normal((2, 130, 3))
    return {"logits": logits, "conf": conf, "pts": (rng.standard_normal((2, 130, 3)) * SIGMA).astype(F32),
            "dir": (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32), "mag": (rng.random((2, 130, 1)) * 0.8).astype(F32), "scale": IP_SCALE}


def chain_stage_inputs(inputs, labels, inner):
    return {"M": 86, "pts": inner, "labels": labels, "conf": inputs["conf"]}
