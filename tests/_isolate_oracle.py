"""The definitions of DESIGN section 22 restated with numpy for one cloud (n,3) float64 at a time -- the checker of etch_amd.cloud's plane and
cluster functions, never the product.  Arithmetic is float64 with one rounding per operation (numpy's element-wise operations do not fuse, and
its +, -, *, / and sqrt are the IEEE operations), so planes, counts, masks, labels and sizes must agree bit for bit."""
import numpy as np

import _cloud_oracle as CO
from _sampler_oracle import philox4x32_10


def hypothesis_rows(key, H, n):
    """Rows i0, i1, i2 of hypotheses 0 .. H-1 of a cloud with n rows under the uint64 key: Philox counter (h, 1, 0, 0), i = (r n) >> 32.  (H,3) int64."""
    ctr = np.zeros((H, 4), np.uint32)
    ctr[:, 0] = np.arange(H, dtype=np.uint32)
    ctr[:, 1] = 1
    r = philox4x32_10(ctr, (int(key) & 0xFFFFFFFF, int(key) >> 32))[:, :3].astype(np.uint64)
    return ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def hypotheses(p, key, H, up=None, cos_tilt=0.0):
    """-> planes (H,4), valid (H) int32.  up: a unit vector or None."""
    p = np.asarray(p, np.float64)
    n = len(p)
    planes, valid = np.zeros((H, 4)), np.zeros(H, np.int32)
    if n < 3:
        return planes, valid
    rows = hypothesis_rows(key, H, n)
    p0, p1, p2 = p[rows[:, 0]], p[rows[:, 1]], p[rows[:, 2]]
    u, v = p1 - p0, p2 - p0
    m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    len2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    ok = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2]) & (len2 > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = m / np.sqrt(len2)[:, None]
        d = -dot3(nrm, p0)
        if up is not None:
            c = dot3(nrm, np.asarray(up, np.float64)[None, :])
            ok &= ~(np.abs(c) < cos_tilt)
            flip = c < 0.0
            nrm, d = np.where(flip[:, None], -nrm, nrm), np.where(flip, -d, d)
    planes[ok, :3], planes[ok, 3], valid[ok] = nrm[ok], d[ok], 1
    return planes, valid


def signed(p, plane):
    """s_i = ((nx x + ny y) + nz z) + d."""
    p, plane = np.asarray(p, np.float64), np.asarray(plane, np.float64)
    return ((plane[0] * p[:, 0] + plane[1] * p[:, 1]) + plane[2] * p[:, 2]) + plane[3]


def score(p, planes, tau, valid=None):
    """-> counts (H,3) int32 = inliers, above, below."""
    planes = np.asarray(planes, np.float64)
    out = np.zeros((len(planes), 3), np.int32)
    for h, pl in enumerate(planes):
        if valid is not None and not valid[h]:
            continue
        s = signed(p, pl)
        out[h] = ((np.abs(s) <= tau).sum(), (s > tau).sum(), (s < -tau).sum())
    return out


def select(planes, valid, counts, min_inliers=3, has_up=False):
    """-> plane (4), counts (3) int32, found."""
    ok = np.flatnonzero(np.asarray(valid) != 0)
    if len(ok) == 0:
        return np.zeros(4), np.zeros(3, np.int32), False
    h = ok[np.argmax(counts[ok, 0])]                              # argmax returns the first of equal counts: the lowest h
    if counts[h, 0] < min_inliers:
        return np.zeros(4), np.zeros(3, np.int32), False
    plane, c = np.array(planes[h], np.float64), np.array(counts[h], np.int32)
    if not has_up and c[2] > c[1]:
        plane, c = -plane, c[[0, 2, 1]]
    return plane, c, True


def ransac(p, key, H, tau, up=None, cos_tilt=0.0, min_inliers=3):
    """Hypotheses, score, select: the plane before the refit."""
    planes, valid = hypotheses(p, key, H, up, cos_tilt)
    return select(planes, valid, score(p, planes, tau, valid), min_inliers, up is not None)


def inlier_covariance(p, plane, tau):
    """-> m, centroid (3), covariance sums (3,3) of p - c over the inliers of `plane`, summed by numpy (the order is not the kernel's)."""
    q = np.asarray(p, np.float64)[np.abs(signed(p, plane)) <= tau]
    c = q.sum(0) / len(q)
    e = q - c
    return len(q), c, e.T @ e


def refit_eigh(p, plane, tau):
    """One least-squares step with numpy.linalg.eigh: NOT bit-defined, the reference of the refit's bound.  -> plane (4), the eigenvalues (3)
    ascending, the inlier count."""
    m, c, cov = inlier_covariance(p, plane, tau)
    w, V = np.linalg.eigh(cov)
    n = V[:, 0] if V[:, 0] @ np.asarray(plane)[:3] >= 0.0 else -V[:, 0]
    return np.array([n[0], n[1], n[2], -float(dot3(n, c))]), w, m


def keep_above(p, plane, found, tau):
    return signed(p, plane) > tau if found else np.ones(len(p), bool)


def components(p, r, chunk=256):
    """-> label (n) int32 = the lowest row of the row's connected component under d2 <= r r, size (n) int32 = the component's rows.  Union-find
    with the lower root as the parent, rows in ascending order."""
    p = np.asarray(p, np.float64)
    n, r2 = len(p), float(r) * float(r)
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        near = CO.d2_rows(p, rows) <= r2
        for k, i in enumerate(rows):
            for j in np.flatnonzero(near[k, :i]):
                x, y = find(i), find(j)
                if x != y:
                    parent[max(x, y)] = min(x, y)
    label = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    size = np.bincount(label, minlength=max(n, 1))[label].astype(np.int32) if n else np.zeros(0, np.int32)
    return label, size


def component_keep(label, size, largest=True, min_points=1):
    """-> keep (n) bool, the winner's label (-1 for an empty cloud)."""
    if len(label) == 0:
        return np.zeros(0, bool), -1
    roots = np.flatnonzero(label == np.arange(len(label)))
    winner = int(roots[np.argmax(size[roots])])                    # the first of equal sizes: the lowest label
    keep = size >= min_points
    return (keep & (label == winner) if largest else keep), winner


# ---------------------------------------------------------------------------------------------------------------- the end-to-end fixture
UP = (0.0, 1.0, 0.0)                                               # the body of the golden file stands along +y
LIFT = 0.003                                                       # the height of the body's lowest vertex in the fixture


def isolate_fixture(seed=23):
    """The body standing on a floor, clutter beside it and stray points: the 6 890 body vertices lifted so that the lowest one is 3 mm above
    y = 0 (on top of the floor's noise), a floor disc of radius 1.5 m (4 000 samples, y = +-3 mm noise) under the body's centre, a box of 400
    clutter points standing on the floor 1 m from the body, and the 140 stray points of _cloud_oracle.stray_fixture, then one permutation.
    -> points (11430,3), kind (11430) int8: 0 body, 1 floor, 2 clutter, 3 stray."""
    both, is_stray = CO.stray_fixture()
    v = CO.body_vertices()
    lift = np.array([0.0, LIFT - v[:, 1].min(), 0.0])
    body, stray = v + lift, both[is_stray] + lift
    rng = np.random.default_rng(seed)
    cx, cz = (body[:, 0].min() + body[:, 0].max()) / 2.0, (body[:, 2].min() + body[:, 2].max()) / 2.0
    rad, ang = 1.5 * np.sqrt(rng.uniform(0.0, 1.0, 4000)), rng.uniform(0.0, 2.0 * np.pi, 4000)
    floor = np.stack([cx + rad * np.cos(ang), rng.uniform(-0.003, 0.003, 4000), cz + rad * np.sin(ang)], 1)
    clutter = np.stack([cx + 1.0 + rng.uniform(-0.15, 0.15, 400), rng.uniform(0.0, 0.5, 400), cz + rng.uniform(-0.15, 0.15, 400)], 1)
    p = np.concatenate([body, floor, clutter, stray])
    kind = np.repeat(np.arange(4, dtype=np.int8), [len(body), len(floor), len(clutter), len(stray)])
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), kind[perm]


def isolate_pipeline(p, key, stat=(8, 1.0), tau=0.02, H=256, max_tilt=10.0, r=0.05):
    """What prepare(stat=, floor=, cluster=) keeps of one cloud, stage by stage, with the RANSAC plane NOT refitted (the refit is not
    bit-defined; the tests hand the device's refitted plane to `after_plane`).  -> keep over the given rows, rows per stage, plane, found."""
    k1 = CO.stat_keep(CO.knn_mean(p, stat[0]), stat[1])[0]
    s1 = p[k1]
    plane, _, found = ransac(s1, key, H, tau, UP, np.cos(np.radians(max_tilt)))
    return (k1, s1, plane, found)


def after_plane(p, k1, s1, plane, found, tau=0.02, r=0.05):
    """The floor and cluster stages on the rows the statistical filter left, for the given plane.  -> keep over the rows of p, rows per stage."""
    k3 = keep_above(s1, plane, found, tau)
    s3 = s1[k3]
    label, size = components(s3, r)
    k4, _ = component_keep(label, size, True, 1)
    keep = k1.copy()
    sub = k3.copy()
    sub[np.flatnonzero(k3)] = k4
    keep[np.flatnonzero(k1)] = sub
    return keep, [int(k1.sum()), int(k3.sum()), int(k4.sum())]
