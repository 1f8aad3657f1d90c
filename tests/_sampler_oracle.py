"""fp64 numpy restatement of csrc/mesh_sample.hip for the ingestion tests -- TEST INFRASTRUCTURE ONLY.

Each function repeats the kernels' operation order term by term (numpy never fuses a multiply and an add, and its +, -, *, / and sqrt are the
IEEE operations), so centres, cumulative areas, drawn faces and points must agree bit for bit."""
import numpy as np

TILE = 64
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Random123's Philox4x32-10: counter (n,4) uint32, key (2,) -> (n,4) uint32."""
    c = [np.asarray(counter, np.uint32)[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def uniforms(key, n):
    """-> u_f, u1, u2 (n) float64 of samples 0..n-1 under the scan key `key` (uint64): all exact in fp64."""
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    r = philox4x32_10(ctr, (int(key) & 0xFFFFFFFF, int(key) >> 32)).astype(np.uint64)
    uf = ((r[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (r[:, 1] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return uf, (r[:, 2].astype(np.float64) + 0.5) * 2.0 ** -32, (r[:, 3].astype(np.float64) + 0.5) * 2.0 ** -32


def bbox_center(verts):
    """(min + max) / 2 with the kernel's order-free rule for zeros: of equal zeros the minimum is -0, the maximum +0."""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    for k in range(3):
        z = v[:, k][v[:, k] == 0.0]
        if lo[k] == 0.0:
            lo[k] = -0.0 if np.signbit(z).any() else 0.0
        if hi[k] == 0.0:
            hi[k] = 0.0 if (~np.signbit(z)).any() else -0.0
    return (lo + hi) / 2.0


def corners(verts, faces, center=None):
    v = np.asarray(verts, np.float64)
    if center is not None:
        v = v - np.asarray(center, np.float64)
    tri = v[np.asarray(faces)]
    return tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]


def face_areas(e1, e2):
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def cumulative_areas(area):
    """Tiles of 64 faces: c[j] = the sequential inclusive sum in the tile, S_t = the sequential sum of the totals in front, cum = S_t + c[j]."""
    F = len(area)
    nt = (F + TILE - 1) // TILE
    pad = np.zeros(nt * TILE)
    pad[:F] = area
    pad = pad.reshape(nt, TILE)
    c = np.empty_like(pad)
    c[:, 0] = pad[:, 0]
    for j in range(1, TILE):                       # every tile at once, each still summed in order
        c[:, j] = c[:, j - 1] + pad[:, j]
    last = np.minimum(F - np.arange(nt) * TILE, TILE) - 1
    totals = c[np.arange(nt), last]
    S = np.empty(nt)
    run = 0.0
    for t in range(nt):
        S[t] = run
        run = run + totals[t]
    return (S[:, None] + c).reshape(-1)[:F]


def sample_surface(verts, faces, key, n, center=None):
    """-> points (n,3) float64, points (n,3) float32, face (n) int32, cum (F)."""
    v0, e1, e2 = corners(verts, faces, center)
    cum = cumulative_areas(face_areas(e1, e2))
    uf, u1, u2 = uniforms(key, n)
    face = np.minimum(np.searchsorted(cum, uf * cum[-1], side="right"), len(cum) - 1)
    flip = u1 + u2 > 1.0
    u1 = np.where(flip, 1.0 - u1, u1)
    u2 = np.where(flip, 1.0 - u2, u2)
    p = (v0[face] + u1[:, None] * e1[face]) + u2[:, None] * e2[face]
    with np.errstate(over="ignore"):
        return p, p.astype(np.float32), face.astype(np.int32), cum
