"""The any-order rule of the grid kNN, emulated in numpy against the oracle's sequential heap scan: the sorted k-list fed
with a superset of the true neighbours in a random order equals the reference's output for every query that raises none of the three tie flags."""
import numpy as np
import pytest

from oracle import ops as O

BIG = np.float32(1e10)


def sqdist(q, p):
    """etch_sqdist: every operation rounded to fp32, (dx*dx + dy*dy) + dz*dz."""
    d = (q[None, :] - p).astype(np.float32)
    s = (d * d).astype(np.float32)
    return ((s[:, 0] + s[:, 1]).astype(np.float32) + s[:, 2]).astype(np.float32)


def anyorder_list(k, d2, order, start):
    """-> (idx list, d2 list, flagged).  d2[j] is the distance of support point start + j; `order` the visiting order (positions j)."""
    bd, bi = [BIG] * k, [start] * k
    top, flagged = BIG, False
    for j in order:
        cd = d2[j]
        if not cd <= top:
            continue
        if cd < top:
            if k > 1 and bd[k - 2] == top and bi[k - 1] != bi[k - 2]:
                flagged = True                              # eviction while two different points tie for the maximum
            pos = sum(1 for v in bd if v <= cd)
            bd.insert(pos, cd), bi.insert(pos, start + j)
            bd.pop(), bi.pop()
            top = bd[-1]
        else:
            flagged = True                                  # turned away with cd == top
    for a in range(1, k):
        if bd[a] == bd[a - 1] and bi[a] != bi[a - 1]:
            flagged = True                                  # tied results: the heap sort's order is not the sorted one
    return bi, bd, flagged


def datasets():
    rng = np.random.default_rng(11)
    lattice = rng.integers(-2, 3, (90, 3)).astype(np.float32) * np.float32(0.5)
    gauss = (rng.standard_normal((80, 3)) * np.array([0.14, 0.31, 0.085])).astype(np.float32)
    dup = np.concatenate([gauss[:30], gauss[:30], gauss[30:50]])
    short = (rng.standard_normal((5, 3)) * 0.2).astype(np.float32)
    return {"lattice": lattice, "gauss": gauss, "duplicates": dup, "short": short}


@pytest.mark.parametrize("name", ["lattice", "gauss", "duplicates", "short"])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_unflagged_queries_equal_the_reference(name, k):
    p = datasets()[name]
    n = len(p)
    o = np.array([n], np.int32)
    ri, rd2 = O.knnquery(k, p, p, o, o)
    rng = np.random.default_rng(100 + k)
    unflagged = 0
    for q in range(n):
        d2 = sqdist(p[q], p)
        for trial in range(2):
            if trial == 0 or n <= k:
                order = rng.permutation(n)                                  # everything, in a random order
            else:                                                           # a random superset of the true neighbours
                extra = rng.choice(n, rng.integers(0, n), replace=False)
                order = rng.permutation(np.union1d(ri[q], extra))
            bi, bd, flagged = anyorder_list(k, d2, order, 0)
            if not flagged:
                unflagged += 1
                assert bi == list(ri[q]), (name, k, q, trial)
                assert np.array_equal(np.array(bd, np.float32).view(np.int32), rd2[q].view(np.int32)), (name, k, q, trial)
    if name == "gauss":
        assert unflagged == 2 * n                           # no ties in generic data: the rule must not flag what it can answer


# ---- the stop rule: cells, shells and the bound as the kernel computes them, in fp32 -------------------------------------------------------
F = np.float32
DELTA, MARGIN, RMAX = F(2.0 ** -8), F(1 - 2.0 ** -10), 7


def grid_of(p):
    """knn_grid_build_kernel's cell size for one eligible segment: -> origin, h, inv_h, dims."""
    lo, hi = p.min(0), p.max(0)
    ext = (hi - lo).astype(F)
    emax = ext.max()
    cap = min(16384, 4 * len(p))
    thin = F(emax * F(1 / 1024))
    e = np.maximum(ext, thin)
    h = F(F(F(np.cbrt(e[0])) * F(np.cbrt(e[1]))) * F(np.cbrt(e[2])) / F(np.cbrt(F(cap))))
    h = max(h, F(emax * F(1 / 1023)))
    for _ in range(64):
        inv_h = F(1) / h
        dims = np.floor((ext * inv_h).astype(F)).astype(np.int64) + 1
        if dims.max() <= 1024 and dims.prod() <= cap:
            return lo, h, inv_h, dims
        h = F(h * F(1.0625))
    raise AssertionError("no cell size")


def cells_of(x, lo, inv_h, dims):
    u = ((x - lo).astype(F) * inv_h).astype(F)
    return np.clip(np.floor(u), 0, (dims - 1).astype(F)).astype(np.int64)


def stop_shell(k, p, q):
    """Per query: the shell after which the kernel stops (0: not within RMAX), and whether the points visited by then hold the k nearest."""
    lo, h, inv_h, dims = grid_of(p)
    cheb = np.abs(cells_of(q, lo, inv_h, dims)[:, None, :] - cells_of(p, lo, inv_h, dims)[None, :, :]).max(2)
    d2 = np.stack([sqdist(x, p) for x in q])
    kth_all = np.partition(d2, k - 1, axis=1)[:, k - 1]
    shell = np.zeros(len(q), np.int64)
    exact = np.ones(len(q), bool)
    for rho in range(1, RMAX + 1):
        seen = np.where(cheb <= rho, d2, F(np.inf))
        top = np.partition(seen, k - 1, axis=1)[:, k - 1]
        rb = F(F(F(rho) - DELTA) * h)
        stop = (shell == 0) & (top < F(F(rb * rb) * MARGIN))
        shell[stop] = rho
        # exact: no unvisited point is as near as the k-th visited one (strictly farther: not even a tie)
        unseen_min = np.where(cheb > rho, d2, F(np.inf)).min(1)
        exact[stop] = (unseen_min[stop] > top[stop]) & (top[stop] == kth_all[stop])
    return shell, exact


def gauss_scan(seed, n, sigma=(0.14, 0.31, 0.085)):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array(sigma)).astype(np.float32)


@pytest.mark.parametrize("k,n,m,qsigma", [(16, 1250, 1250, None), (8, 700, 700, None), (3, 600, 900, (0.3, 0.6, 0.2)), (1, 520, 300, None)])
def test_stop_rule_never_misses_a_neighbour(k, n, m, qsigma):
    p = gauss_scan(3000, n)
    q = p if qsigma is None and m == n else gauss_scan(4000, m, qsigma or (0.14, 0.31, 0.085))
    shell, exact = stop_shell(k, p, q)
    assert exact.all()
    share = float((shell == 0).mean())
    print(f"k={k} n={n} m={m}: shells {np.bincount(shell, minlength=RMAX + 1).tolist()}, not finished within {RMAX} shells {share:.4%}")
    if qsigma is None:
        assert share <= 0.02


def test_stop_rule_on_cell_walls_and_outliers():
    p = gauss_scan(3001, 600)
    lo, h, inv_h, dims = grid_of(p)
    rng = np.random.default_rng(7)
    walls = p[rng.choice(600, 300)].copy()
    for i, row in enumerate(walls):
        a = i % 3
        v = F(lo[a] + F(rng.integers(1, dims[a]) * h))
        row[a] = (np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf)))[(i // 3) % 3]
    p2 = np.concatenate([p.min(0)[None], p.max(0)[None], walls, p[:298]]).astype(F)     # the same box and count: the same cells
    lo2, h2, _, dims2 = grid_of(p2)
    assert np.array_equal(lo2, lo) and h2 == h and np.array_equal(dims2, dims)
    for k in (3, 16):
        assert stop_shell(k, p2, p2)[1].all()
    far = np.concatenate([gauss_scan(3002, 500, (0.01, 0.01, 0.01)), gauss_scan(3003, 8, (0.01, 0.01, 0.01)) + F(50)]).astype(F)
    shell, exact = stop_shell(16, far, far)
    assert exact.all() and (shell[500:] == 0).all()          # an outlier's 9th .. 16th neighbours lie ~50 units (a dozen cells) away: past RMAX shells
