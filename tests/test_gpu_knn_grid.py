"""kNN on the per-segment cell grid: idx and dist bit for bit the full scan's (ops.KNN_GRID = False) and the oracle's."""
import numpy as np
import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu


def scan(seed, n, sigma=(0.14, 0.31, 0.085)):
    """test_gpu_index_ops.scan's recipe."""
    return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array(sigma)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


GRID, NOT_ELIGIBLE, LARGE_K, SHELLS, TIES = range(5)          # the counter's slots


def bits(t):
    return t.cpu().numpy().view(np.int32)


def check(k, p, q, o, qo, sqrt=True, oracle=True, min_points=None):
    """Grid path against the full scan (and the oracle): -> the counter (5) of the grid run.  min_points: a grid built with that size threshold
    instead of the product's (segments smaller than ops.KNN_GRID_MIN_POINTS on the grid)."""
    from etch_amd import ops
    assert ops.KNN_GRID
    P, Q, Od, QOd = dev(p), dev(q), dev(np.asarray(o, np.int32)), dev(np.asarray(qo, np.int32))
    grid = None if min_points is None else ops.knn_grid_build(P, Od, min_points=min_points)
    counters = torch.zeros(5, dtype=torch.int32, device="cuda")
    gi, gd = ops.knnquery(k, P, Q, Od, QOd, sqrt=sqrt, counters=counters, grid=grid)
    gi2, gd2 = ops.knnquery(k, P, Q, Od, QOd, sqrt=sqrt, grid=grid)          # the product's own dispatch (no counter)
    ops.KNN_GRID = False
    try:
        fi, fd = ops.knnquery(k, P, Q, Od, QOd, sqrt=sqrt)
    finally:
        ops.KNN_GRID = True
    assert np.array_equal(bits(gi), bits(fi)) and np.array_equal(bits(gd), bits(fd))
    assert np.array_equal(bits(gi2), bits(fi)) and np.array_equal(bits(gd2), bits(fd))
    if oracle:
        ri, rd2 = O.knnquery(k, p, q, np.asarray(o, np.int32), np.asarray(qo, np.int32))
        assert np.array_equal(gi.cpu().numpy(), ri)
        assert np.array_equal(gd.cpu().numpy(), np.sqrt(rd2) if sqrt else rd2)
    c = counters.cpu().numpy()
    assert c.sum() == len(q)
    return c


def scans(seed, segs, sigma=(0.14, 0.31, 0.085)):
    return np.concatenate([scan(seed + i, n, sigma) for i, n in enumerate(segs)]), np.cumsum(segs).astype(np.int32)


@pytest.mark.parametrize("k,segs,qsegs", [(8, [1250, 600], None), (16, [1250, 1250], [312, 312]), (3, [312, 300], [1250, 1200]), (1, [700, 520], None),
                                          (3, [1250, 600], [2000, 100]), (8, [5000], None)])
def test_gaussian_scans(k, segs, qsegs):
    from etch_amd import ops
    p, o = scans(3000, segs)
    q, qo = (p, o) if qsegs is None else scans(4000, qsegs)
    c = check(k, p, q, o, qo)
    small = sum(m for n, m in zip(segs, qsegs or segs) if n < ops.KNN_GRID_MIN_POINTS)
    assert c[NOT_ELIGIBLE] == small and c[LARGE_K] == 0
    assert c[GRID] >= 0.98 * (len(q) - small)


def test_mixed_segments_below_k_eligible_and_below_the_threshold():
    p, o = scans(3010, [5, 700, 40])
    c = check(16, p, p, o, o)
    assert c[NOT_ELIGIBLE] == 45 and c[GRID] >= 0.98 * 700


def test_ties_on_a_lattice_with_duplicates():
    rng = np.random.default_rng(5)
    p = (rng.integers(-2, 3, (400, 3)).astype(np.float32)) * 0.5
    o = np.array([150, 400], np.int32)
    for k in (3, 8, 16):
        assert check(k, p, p, o, o, sqrt=False)[NOT_ELIGIBLE] == 400          # 150 and 250 points: below the product's threshold
        c = check(k, p, p, o, o, sqrt=False, min_points=17)                   # both segments on the grid
        assert c[NOT_ELIGIBLE] == 0 and c[TIES] > 0


def test_far_outliers_pass_the_last_shell():
    p = np.concatenate([scan(3002, 500, (0.01, 0.01, 0.01)), scan(3003, 8, (0.01, 0.01, 0.01)) + np.float32(50)]).astype(np.float32)
    o = np.array([508], np.int32)
    c = check(16, p, p, o, o, min_points=17)                                  # (508 points: below the product's threshold)
    assert c[NOT_ELIGIBLE] == 0 and c[SHELLS] >= 8                            # an outlier's 9th .. 16th neighbours lie a dozen cells away
    assert check(8, p, p, o, o, min_points=17)[NOT_ELIGIBLE] == 0
    p = np.concatenate([scan(3004, 600, (0.01, 0.01, 0.01)), p[500:]])        # the same through the product's dispatch
    c = check(16, p, p, np.array([608], np.int32), np.array([608], np.int32))
    assert c[NOT_ELIGIBLE] == 0 and c[SHELLS] >= 8


def test_queries_outside_the_supports_box():
    p, o = scans(3020, [1250, 600])
    q, qo = scans(4020, [400, 300], (0.5, 1.0, 0.4))
    for k in (3, 16):
        check(k, p, q, o, qo)
    far = (q * np.float32(1e4)).astype(np.float32)                            # thousands of cells outside: clamped into the grid
    c = check(8, p, far, o, qo)
    assert c[GRID] + c[SHELLS] + c[TIES] == 700


def test_points_on_cell_walls():
    from etch_amd import ops
    p = scan(3001, 600)
    o = np.array([600], np.int32)
    hdr = ops.knn_grid_build(dev(p), dev(o)).header.cpu().numpy()[0]
    lo, h, dims = hdr[:3].view(np.float32), hdr[3:4].view(np.float32)[0], hdr[5:8]
    assert hdr[8] == 1 and np.array_equal(lo, p.min(0)) and h > 0 and 1 < dims.prod() == hdr[9] <= 2400
    rng = np.random.default_rng(7)
    walls = p[rng.choice(600, 300)].copy()
    for i, row in enumerate(walls):
        a = i % 3
        v = np.float32(lo[a] + np.float32(rng.integers(1, dims[a]) * h))
        row[a] = (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf)))[(i // 3) % 3]
    p2 = np.concatenate([p.min(0)[None], p.max(0)[None], walls, p[:298]]).astype(np.float32)      # the same box and count: the same cells
    hdr2 = ops.knn_grid_build(dev(p2), dev(o)).header.cpu().numpy()[0]
    assert np.array_equal(hdr2[:10], hdr[:10])
    for k in (3, 8, 16):
        c = check(k, p2, p2, o, o)
        assert c[NOT_ELIGIBLE] == 0 and c[GRID] > 300


def test_grid_layout_is_a_counting_sort_of_the_points():
    from etch_amd import ops
    p, o = scans(3030, [700, 40, 1250])
    g = ops.knn_grid_build(dev(p), dev(o))
    pts, cs, hdr = g.pts.cpu().numpy(), g.cell_start.cpu().numpy(), g.header.cpu().numpy()
    assert [int(h[8]) for h in hdr] == [1, 0, 1]
    for s, a, b in [(0, 0, 700), (2, 740, 1990)]:
        cells = int(hdr[s][9])
        start = cs[s][:cells + 1]
        assert start[0] == 0 and start[-1] == b - a and (np.diff(start) >= 0).all()
        gi = pts[a:b, 3].view(np.int32)
        assert np.array_equal(np.sort(gi), np.arange(a, b))
        assert np.array_equal(pts[a:b, :3].view(np.int32), p[gi].view(np.int32))
        lo, inv_h, dims = hdr[s][:3].view(np.float32), hdr[s][4:5].view(np.float32)[0], hdr[s][5:8]
        u = np.floor(((pts[a:b, :3] - lo).astype(np.float32) * inv_h).astype(np.float32))
        c = np.clip(u, 0, dims - 1).astype(np.int64)
        lin = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
        assert (np.diff(lin) >= 0).all() and np.array_equal(np.searchsorted(lin, np.arange(cells + 1)), start)


def test_degenerate_supports():
    one = np.tile(np.float32([0.3, -0.2, 0.1]), (600, 1))
    o = np.array([600], np.int32)
    c = check(8, one, one, o, o)
    assert c[NOT_ELIGIBLE] == 600                                             # no extent
    line = np.zeros((600, 3), np.float32)
    line[:, 1] = np.random.default_rng(3).standard_normal(600).astype(np.float32)
    c = check(8, line, line, o, o)
    assert c[NOT_ELIGIBLE] == 0
    q = scan(4040, 300)
    check(3, line, q, o, np.array([300], np.int32))
    bad = scan(3040, 600)
    bad[17, 1], bad[400, 2] = np.nan, np.inf
    c = check(8, bad, q, o, np.array([300], np.int32), oracle=False)
    assert c[NOT_ELIGIBLE] == 300                                             # a box that is not finite
    good = scan(3041, 600)
    qn = q.copy()
    qn[5, 0], qn[9, 2], qn[11, 1] = np.nan, np.inf, -np.inf
    c = check(8, good, qn, o, np.array([300], np.int32), oracle=False)
    assert c[NOT_ELIGIBLE] == 0 and c[SHELLS] >= 3


def test_fallback_share_is_small():
    p, o = scans(3000, [1250, 1250])
    c = check(16, p, p, o, o)
    print("counter", c.tolist())
    assert c[NOT_ELIGIBLE] == 0 and c[LARGE_K] == 0
    assert c[SHELLS] + c[TIES] <= 0.02 * 2500


def test_nsample_17_takes_the_full_scan():
    p, o = scans(3000, [700, 520])
    c = check(17, p, p, o, o)
    assert c[LARGE_K] == 1220 and c.sum() == 1220


def same(a, b, where="result"):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype.is_floating_point else a,
                                                                          b.view(torch.uint8) if b.dtype.is_floating_point else b), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif hasattr(a, "vertices") and hasattr(a, "faces"):
        same(np.asarray(a.vertices), np.asarray(b.vertices), where + ".vertices")
        same(np.asarray(a.faces), np.asarray(b.faces), where + ".faces")
    else:
        assert a == b, where


def test_end_to_end_is_bitwise_the_same():
    import types

    from etch_amd import constants as K
    from etch_amd import ops
    from etch_amd.inference_demo import predict_smpl_batch
    from etch_amd.models.models_pointcloud import GT_network_equiv
    from etch_amd.utils.body_model import SyntheticSMPL
    from etch_amd.utils.weights import load_seeded
    device = torch.device("cuda:0")
    args = types.SimpleNamespace(output_folder="/tmp/etch_knn_grid", EPN_input_radius=0.4, EPN_layer_num=2, device=device,
                                 markerset=K.default_markerset(), scale_magnitude=10, body_model=SyntheticSMPL(7))
    model = load_seeded(GT_network_equiv(option=args), 1).to(device).eval()
    pts = torch.from_numpy(np.stack([scan(1000, 1024), scan(1001, 1024)])).to(device)
    out = []
    for on in (True, False):
        ops.KNN_GRID = on
        try:
            with torch.no_grad():
                out.append(predict_smpl_batch(args, model, pts, "neutral", steps_stage0=4, steps_stage1=4, return_trace=True))
        finally:
            ops.KNN_GRID = True
        torch.cuda.synchronize()
    same(out[0], out[1])
