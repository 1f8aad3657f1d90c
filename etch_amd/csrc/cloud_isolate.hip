// Raw point clouds, isolating the subject: a floor plane by RANSAC with one least-squares refit, and Euclidean clusters as
// the connected components of the radius graph.  fp64, one rounding per operation: this file is built with -ffp-contract=off.
//
// Everything that is compared is an integer or a bit-defined double: a hypothesis is a pure function of (cloud key, h) through Philox4x32-10
// with counter (h, 1, 0, 0) -- the pick of depth_render.hip uses (j, 0, 0, 0) under the same key --, a score is three integer counts added up
// with integer atomics (any order gives the same sum), and a cluster label is the lowest row of its component.  No float atomics anywhere.
//
// Components: union-find over the rows of a cloud, parent[] indexed by packed row.  The one invariant is parent[i] <= i: a root is hooked
// only under a smaller root, and path halving replaces a parent by an ancestor, which is smaller still.  So a find walks strictly decreasing
// rows and ends after at most n steps, and the root of a finished component is its lowest row.  Hooking is one atomicCAS on a root; a CAS that
// fails has seen another thread's successful hook of that root, of which a cloud has at most n - 1.  There is no lock and no wait on another
// workgroup; every loop carries the bound its comment derives.
#include "common.h"
#include "etch_hip.h"
#include "cloud_grid.h"
#include <cmath>

#define ISO_THREADS 256
#define ISO_GROUP 1024                      // the one-workgroup-per-cloud kernels
#define ISO_TILE 1024                       // points of a cloud staged in LDS at a time: 3 x 8 KiB
#define ISO_TILES_PER_GROUP 4               // tiles one workgroup of the score kernel walks
#define ISO_PLANES_PER_THREAD 2             // every LDS broadcast read serves two planes
#define ISO_JACOBI_SWEEPS 16
#define ISO_MAX_H 65536

namespace {

__device__ __forceinline__ void iso_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ double iso_dot(double ax, double ay, double az, double bx, double by, double bz) { return ((ax * bx + ay * by) + az * bz); }

// s = ((nx x + ny y) + nz z) + d
__device__ __forceinline__ double iso_signed(double nx, double ny, double nz, double d, double x, double y, double z) {
    return iso_dot(nx, ny, nz, x, y, z) + d;
}

// ---- hypotheses: one thread per (cloud, h) ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_THREADS) void iso_hypotheses_kernel(int H, const double* __restrict__ P, const int* __restrict__ offsets,
                                                                     const unsigned long long* __restrict__ keys, int has_up, double ux, double uy,
                                                                     double uz, double cos_tilt, double* __restrict__ planes, int* __restrict__ valid) {
    const int b = blockIdx.y, h = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (h >= H) return;
    const int lo = offsets[b], n = offsets[b + 1] - lo;
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    int ok = 0;
    if (n >= 3) {
        const unsigned long long key = keys[b];
        unsigned r[4];
        iso_philox4x32_10((unsigned)h, 1u, 0u, 0u, (unsigned)key, (unsigned)(key >> 32), r);
        const int i0 = (int)(((unsigned long long)r[0] * (unsigned long long)n) >> 32);          // < n: r < 2^32
        const int i1 = (int)(((unsigned long long)r[1] * (unsigned long long)n) >> 32);
        const int i2 = (int)(((unsigned long long)r[2] * (unsigned long long)n) >> 32);
        const double* p0 = P + 3 * (size_t)(lo + i0);
        const double* p1 = P + 3 * (size_t)(lo + i1);
        const double* p2 = P + 3 * (size_t)(lo + i2);
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;
        const double len2 = (mx * mx + my * my) + mz * mz;
        ok = i0 != i1 && i0 != i2 && i1 != i2 && len2 > 0.0;
        if (ok) {
            const double len = sqrt(len2);
            double nx = mx / len, ny = my / len, nz = mz / len;
            double d = -iso_dot(nx, ny, nz, p0[0], p0[1], p0[2]);
            if (has_up) {
                const double c = iso_dot(nx, ny, nz, ux, uy, uz);
                if (fabs(c) < cos_tilt) ok = 0;
                if (c < 0.0) nx = -nx, ny = -ny, nz = -nz, d = -d;
            }
            if (ok) out[0] = nx, out[1] = ny, out[2] = nz, out[3] = d;
        }
    }
    const size_t o = (size_t)b * H + h;
#pragma unroll
    for (int a = 0; a < 4; ++a) planes[4 * o + a] = out[a];
    valid[o] = ok;
}

// ---- score: the hot kernel, H n plane evaluations per cloud ----------------------------------------------------------------------------------
// A workgroup owns ISO_THREADS * ISO_PLANES_PER_THREAD VALID planes of its cloud -- those of rank [512 y, 512 y + 512) among the valid ones, y =
// blockIdx.y -- and ISO_TILES_PER_GROUP tiles of the cloud's rows (blockIdx.x).  It finds its planes itself by a count and a scan over the
// cloud's H flags (H <= 65 536 integers against 2e6 evaluations), so an invalid plane costs no evaluation: under a tilt limit most planes are
// invalid.  The grid is sized by M and H; a workgroup whose rows lie behind its cloud's end, or whose ranks lie behind the last valid plane,
// leaves at once.  A tile's coordinates sit in LDS as three arrays; in the walk every lane reads the same address (a broadcast), and a
// thread's planes and counts stay in registers.
__global__ __launch_bounds__(ISO_THREADS) void iso_score_kernel(int H, double tau, const double* __restrict__ P, const int* __restrict__ offsets,
                                                                const double* __restrict__ planes, const int* __restrict__ valid,
                                                                int* __restrict__ counts) {
    __shared__ double sx[ISO_TILE], sy[ISO_TILE], sz[ISO_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1];
    const long long first = (long long)lo + (long long)blockIdx.x * (ISO_TILE * ISO_TILES_PER_GROUP);
    if (first >= hi) return;                                       // uniform over the workgroup: no barrier is skipped by a part of it
    const int end = first + ISO_TILE * ISO_TILES_PER_GROUP < hi ? (int)(first + ISO_TILE * ISO_TILES_PER_GROUP) : hi;
    constexpr int OWN = ISO_THREADS * ISO_PLANES_PER_THREAD;
    __shared__ int s_slot[OWN], s_scan[ISO_THREADS], s_all;
    const int base = blockIdx.y * OWN;                              // the first rank this workgroup owns
    int mine;                                                       // the planes it owns: 0 .. OWN
    if (valid) {
        const int* v = valid + (size_t)b * H;
        const int chunk = (H + ISO_THREADS - 1) / ISO_THREADS;      // thread tid looks at the flags [tid chunk, tid chunk + chunk)
        const int a = tid * chunk < H ? tid * chunk : H, e = a + chunk < H ? a + chunk : H;
        int c = 0;
        for (int h = a; h < e; ++h) c += v[h] != 0 ? 1 : 0;
        s_scan[tid] = c;
        __syncthreads();
        if (tid == 0) {                                             // exclusive sums of 256 counts
            int run = 0;
            for (int i = 0; i < ISO_THREADS; ++i) {
                const int t = s_scan[i];
                s_scan[i] = run;
                run += t;
            }
        }
        __syncthreads();
        int rank = s_scan[tid];
        for (int h = a; h < e; ++h)
            if (v[h] != 0) {
                if (rank >= base && rank < base + OWN) s_slot[rank - base] = h;
                ++rank;
            }
        if (tid == ISO_THREADS - 1) s_all = rank;                   // the last thread ends at the number of valid planes
        __syncthreads();
        const int all = s_all;
        mine = all - base < 0 ? 0 : (all - base < OWN ? all - base : OWN);
    } else {
        mine = H - base < OWN ? H - base : OWN;                     // every plane counts: rank = h
    }
    if (mine <= 0) return;                                          // uniform over the workgroup
    double nx[ISO_PLANES_PER_THREAD], ny[ISO_PLANES_PER_THREAD], nz[ISO_PLANES_PER_THREAD], d[ISO_PLANES_PER_THREAD];
    int in[ISO_PLANES_PER_THREAD], ab[ISO_PLANES_PER_THREAD], be[ISO_PLANES_PER_THREAD], slot[ISO_PLANES_PER_THREAD];
#pragma unroll
    for (int q = 0; q < ISO_PLANES_PER_THREAD; ++q) {
        const int k = q * ISO_THREADS + tid;
        slot[q] = k < mine ? (valid ? s_slot[k] : base + k) : -1;
        const double* pl = planes + 4 * ((size_t)b * H + (slot[q] >= 0 ? slot[q] : 0));
        nx[q] = pl[0], ny[q] = pl[1], nz[q] = pl[2], d[q] = pl[3];
        in[q] = ab[q] = be[q] = 0;
    }
    const bool walk = __ballot(slot[0] >= 0) != 0;                  // the owned planes fill the slots from k = 0: a wave without one in q = 0 has none
    const double ntau = -tau;
    for (int t0 = (int)first; t0 < end; t0 += ISO_TILE) {
        const int m = end - t0 < ISO_TILE ? end - t0 : ISO_TILE;
        __syncthreads();
        for (int i = tid; i < m; i += ISO_THREADS) {
            const double* p = P + 3 * (size_t)(t0 + i);
            sx[i] = p[0], sy[i] = p[1], sz[i] = p[2];
        }
        __syncthreads();
        for (int i = 0; walk && i < m; ++i) {
            const double x = sx[i], y = sy[i], z = sz[i];
#pragma unroll
            for (int q = 0; q < ISO_PLANES_PER_THREAD; ++q) {
                const double s = iso_signed(nx[q], ny[q], nz[q], d[q], x, y, z);
                in[q] += fabs(s) <= tau ? 1 : 0;
                ab[q] += s > tau ? 1 : 0;
                be[q] += s < ntau ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < ISO_PLANES_PER_THREAD; ++q) {
        if (slot[q] < 0) continue;
        int* c = counts + 3 * ((size_t)b * H + slot[q]);
        if (in[q]) atomicAdd(c, in[q]);
        if (ab[q]) atomicAdd(c + 1, ab[q]);
        if (be[q]) atomicAdd(c + 2, be[q]);
    }
}

// ---- select: one workgroup per cloud -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_GROUP) void iso_select_kernel(int H, int has_up, int min_inliers, const double* __restrict__ planes,
                                                               const int* __restrict__ valid, const int* __restrict__ counts,
                                                               double* __restrict__ plane, int* __restrict__ best_counts, int* __restrict__ found) {
    __shared__ int s_in[ISO_GROUP], s_h[ISO_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    int bi = -1, bh = H;                                            // most inliers, then the lowest h; bh == H: no valid hypothesis seen
    for (int h = tid; h < H; h += ISO_GROUP) {                      // ascending h: a later equal count never replaces an earlier one
        if (!valid[(size_t)b * H + h]) continue;
        const int c = counts[3 * ((size_t)b * H + h)];
        if (c > bi) bi = c, bh = h;
    }
    s_in[tid] = bi, s_h[tid] = bh;
    __syncthreads();
    for (int w = ISO_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const int oi = s_in[tid + w], oh = s_h[tid + w];
            if (oi > s_in[tid] || (oi == s_in[tid] && oh < s_h[tid])) s_in[tid] = oi, s_h[tid] = oh;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    int c[3] = {0, 0, 0}, ok = 0;
    if (s_h[0] < H && s_in[0] >= min_inliers) {
        const size_t o = (size_t)b * H + s_h[0];
        ok = 1;
        c[0] = counts[3 * o], c[1] = counts[3 * o + 1], c[2] = counts[3 * o + 2];
        out[0] = planes[4 * o], out[1] = planes[4 * o + 1], out[2] = planes[4 * o + 2], out[3] = planes[4 * o + 3];
        if (!has_up && c[2] > c[1]) {                               // the bulk of the cloud on the positive side
            out[0] = -out[0], out[1] = -out[1], out[2] = -out[2], out[3] = -out[3];
            const int t = c[1];
            c[1] = c[2], c[2] = t;
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) plane[4 * b + a] = out[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) best_counts[3 * b + a] = c[a];
    found[b] = ok;
}

// ---- refit: one workgroup per cloud, sums in an order n alone fixes ----------------------------------------------------------------------------
__device__ __forceinline__ double iso_block_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int w = ISO_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
    return s[0];
}

__device__ __forceinline__ int iso_block_sum_int(int v, int* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int w = ISO_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
    return s[0];
}

// one Jacobi rotation that zeroes a[P][Q] of the symmetric 3 x 3 matrix a (R is the third index) and accumulates it into the columns of v
template <int P, int Q, int R>
__device__ __forceinline__ void iso_jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

__global__ __launch_bounds__(ISO_GROUP) void iso_refit_kernel(double tau, const double* __restrict__ P, const int* __restrict__ offsets,
                                                              const int* __restrict__ found, double* __restrict__ plane, int* __restrict__ counts) {
    __shared__ double s[ISO_GROUP];
    __shared__ int si[ISO_GROUP];
    __shared__ double s_plane[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!found[b]) return;                                          // uniform over the workgroup
    const int lo = offsets[b], hi = offsets[b + 1];
    const double nx = plane[4 * b], ny = plane[4 * b + 1], nz = plane[4 * b + 2], d = plane[4 * b + 3];
    int m = 0;
    double px = 0.0, py = 0.0, pz = 0.0;
    for (int i = lo + tid; i < hi; i += ISO_GROUP) {
        const double x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], z = P[3 * (size_t)i + 2];
        if (fabs(iso_signed(nx, ny, nz, d, x, y, z)) <= tau) ++m, px += x, py += y, pz += z;
    }
    m = iso_block_sum_int(m, si);
    if (m < 3) return;                                              // fewer than three inliers span no plane: the RANSAC plane stays (uniform)
    const double cx = iso_block_sum(px, s) / (double)m, cy = iso_block_sum(py, s) / (double)m, cz = iso_block_sum(pz, s) / (double)m;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int i = lo + tid; i < hi; i += ISO_GROUP) {
        const double x = P[3 * (size_t)i], y = P[3 * (size_t)i + 1], z = P[3 * (size_t)i + 2];
        if (fabs(iso_signed(nx, ny, nz, d, x, y, z)) <= tau) {
            const double ex = x - cx, ey = y - cy, ez = z - cz;
            xx += ex * ex, xy += ex * ey, xz += ex * ez, yy += ey * ey, yz += ey * ez, zz += ez * ez;
        }
    }
    xx = iso_block_sum(xx, s), xy = iso_block_sum(xy, s), xz = iso_block_sum(xz, s);
    yy = iso_block_sum(yy, s), yz = iso_block_sum(yz, s), zz = iso_block_sum(zz, s);
    if (tid == 0) {
        double a[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
        double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        for (int sweep = 0; sweep < ISO_JACOBI_SWEEPS; ++sweep) {   // cyclic Jacobi; converges quadratically, a 3 x 3 matrix is diagonal after 5 - 7 sweeps
            if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
            iso_jacobi_rotate<0, 1, 2>(a, v);
            iso_jacobi_rotate<0, 2, 1>(a, v);
            iso_jacobi_rotate<1, 2, 0>(a, v);
        }
        const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
        const bool k1 = e1 < e0 && e1 <= e2, k2 = e2 < e0 && e2 < e1;                    // the smallest eigenvalue, a tie to the lowest column
        double wx = k2 ? v[0][2] : (k1 ? v[0][1] : v[0][0]), wy = k2 ? v[1][2] : (k1 ? v[1][1] : v[1][0]), wz = k2 ? v[2][2] : (k1 ? v[2][1] : v[2][0]);
        const double len = sqrt((wx * wx + wy * wy) + wz * wz);
        wx = wx / len, wy = wy / len, wz = wz / len;
        if (iso_dot(wx, wy, wz, nx, ny, nz) < 0.0) wx = -wx, wy = -wy, wz = -wz;          // the side the RANSAC normal points to
        const double wd = -iso_dot(wx, wy, wz, cx, cy, cz);
        const bool good = isfinite(wx) && isfinite(wy) && isfinite(wz) && isfinite(wd);
        s_plane[0] = good ? wx : nx, s_plane[1] = good ? wy : ny, s_plane[2] = good ? wz : nz, s_plane[3] = good ? wd : d;
    }
    __syncthreads();
    const double rx = s_plane[0], ry = s_plane[1], rz = s_plane[2], rd = s_plane[3], ntau = -tau;
    int in = 0, ab = 0, be = 0;
    for (int i = lo + tid; i < hi; i += ISO_GROUP) {
        const double sg = iso_signed(rx, ry, rz, rd, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]);
        in += fabs(sg) <= tau ? 1 : 0, ab += sg > tau ? 1 : 0, be += sg < ntau ? 1 : 0;
    }
    in = iso_block_sum_int(in, si), ab = iso_block_sum_int(ab, si), be = iso_block_sum_int(be, si);
    if (tid == 0) {
        plane[4 * b] = rx, plane[4 * b + 1] = ry, plane[4 * b + 2] = rz, plane[4 * b + 3] = rd;
        counts[3 * b] = in, counts[3 * b + 1] = ab, counts[3 * b + 2] = be;
    }
}

// ---- removal: keep what lies more than tau above a found plane ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_THREADS) void iso_plane_keep_kernel(int B, int M, double tau, const double* __restrict__ P, const int* __restrict__ offsets,
                                                                     const double* __restrict__ plane, const int* __restrict__ found,
                                                                     int* __restrict__ keep) {
    const int t = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (t >= M) return;
    if (t >= offsets[B]) {
        keep[t] = 0;
        return;
    }
    const int b = cloud_of_row(offsets, B, t);
    int k = 1;
    if (found[b])
        k = iso_signed(plane[4 * b], plane[4 * b + 1], plane[4 * b + 2], plane[4 * b + 3], P[3 * (size_t)t], P[3 * (size_t)t + 1], P[3 * (size_t)t + 2]) > tau
                ? 1 : 0;
    keep[t] = k;
}

// ---- components ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int iso_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void iso_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of row i's tree, halving the path on the way
__device__ __forceinline__ int iso_find(int* parent, int i, int n) {
    // parent[x] <= x holds at all times, so every pass either stops (parent[i] == i) or moves to a strictly smaller row of the same cloud: at
    // most n passes.  The store replaces a non-root's parent by that parent's parent, an ancestor that is smaller still.
    for (int step = 0; step < n; ++step) {
        const int p = iso_load(parent + i);
        if (p == i) return i;
        const int g = iso_load(parent + p);
        if (g != p) iso_store(parent + i, g);
        i = g;
    }
    return i;
}

// joins the trees of rows a and b; returns a row both hang under from then on (their root at that moment)
__device__ __forceinline__ int iso_union(int* parent, int a, int b, int n) {
    // A pass ends with the two rows in one tree, with a successful hook, or with a failed CAS.  A CAS on root a fails only after another thread
    // has hooked a under a smaller root; a cloud of n rows sees at most n - 1 successful hooks in all, so at most n passes.
    for (int pass = 0; pass < n; ++pass) {
        a = iso_find(parent, a, n), b = iso_find(parent, b, n);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicCAS(parent + a, a, b);                // the larger root under the smaller: parent[a] = b < a
        if (old == a) return b;
        a = old;                                                    // what the winner wrote: an ancestor of a, continue from there
    }
    return a;
}

__global__ __launch_bounds__(ISO_THREADS) void iso_init_kernel(int M, int* __restrict__ parent, int* __restrict__ size) {
    const int t = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (t < M) parent[t] = t, size[t] = 0;
}

// h >= r, so the 27 cells around a row hold every neighbour; an edge is hooked once, from its higher row
__global__ __launch_bounds__(ISO_THREADS) void iso_link_kernel(int B, int M, double r2, int brute, const double* __restrict__ P,
                                                               const long long* __restrict__ keys, const int* __restrict__ order,
                                                               const int* __restrict__ offsets, const int* __restrict__ status, int* parent) {
    const int t = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    if (brute) {
        int mine = t;                                               // an ancestor of this row: the next find starts there, not at the row
        for (int j = lo; j < t; ++j)
            if (cloud_d2(px, py, pz, P + 3 * (size_t)j) <= r2) mine = iso_union(parent, mine, j, n);
        return;
    }
    const int row = order[t];
    int mine = row;
    auto visit = [&](int j) {
        const int other = order[j];
        if (other < row && cloud_d2(px, py, pz, P + 3 * (size_t)j) <= r2) mine = iso_union(parent, mine, other, n);
    };
    const long long key = keys[t];
    const int ix = (int)(key >> (2 * CLOUD_BITS)), iy = (int)((key >> CLOUD_BITS) & CLOUD_CMAX), iz = (int)(key & CLOUD_CMAX);
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) cloud_scan_column(keys, lo, hi, ix + dx, iy + dy, iz - 1, iz + 1, visit);
}

// the forest is final (a kernel boundary lies behind the last hook): label = the root, local to the cloud; size[root] counts its rows
__global__ __launch_bounds__(ISO_THREADS) void iso_flatten_kernel(int B, int M, const int* __restrict__ offsets, const int* __restrict__ status,
                                                                  int* parent, int* __restrict__ label, int* size) {
    const int t = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], n = offsets[b + 1] - lo;
    const int root = iso_find(parent, t, n);
    label[t] = root - lo;
    atomicAdd(size + root, 1);
}

// every row takes its root's count; roots are only read here, the other rows only written
__global__ __launch_bounds__(ISO_THREADS) void iso_spread_kernel(int B, int M, const int* __restrict__ offsets, const int* __restrict__ status,
                                                                 const int* __restrict__ label, int* size) {
    const int t = blockIdx.x * ISO_THREADS + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int root = offsets[b] + label[t];
    if (root != t) size[t] = iso_load(size + root);
}

// ---- the clusters to keep: one workgroup per cloud -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_GROUP) void iso_component_keep_kernel(int largest, int min_points, const int* __restrict__ label,
                                                                       const int* __restrict__ size, const int* __restrict__ offsets,
                                                                       int* __restrict__ winner, int* __restrict__ keep) {
    __shared__ int s_size[ISO_GROUP], s_label[ISO_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1];
    int bs = 0, bl = 0x7fffffff;                                    // most rows, then the lowest label
    for (int i = lo + tid; i < hi; i += ISO_GROUP)                  // ascending rows: a later equal size never replaces an earlier one
        if (label[i] == i - lo && size[i] > bs) bs = size[i], bl = i - lo;
    s_size[tid] = bs, s_label[tid] = bl;
    __syncthreads();
    for (int w = ISO_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const int os = s_size[tid + w], ol = s_label[tid + w];
            if (os > s_size[tid] || (os == s_size[tid] && ol < s_label[tid])) s_size[tid] = os, s_label[tid] = ol;
        }
        __syncthreads();
    }
    const int win = s_size[0] > 0 ? s_label[0] : -1;
    if (tid == 0) winner[b] = win;
    for (int i = lo + tid; i < hi; i += ISO_GROUP) keep[i] = size[i] >= min_points && (!largest || label[i] == win) ? 1 : 0;
}

}  // namespace

extern "C" {

int etch_cloud_plane_hypotheses(int B, int H, const double* points, const int* offsets, const unsigned long long* keys, int has_up, double up_x,
                                double up_y, double up_z, double cos_tilt, double* planes, int* valid, void* stream) {
    if (B < 1 || H < 1 || H > ISO_MAX_H || !points || !offsets || !keys || !planes || !valid) return ETCH_EINVAL;
    if (has_up && !(std::isfinite(up_x) && std::isfinite(up_y) && std::isfinite(up_z) && cos_tilt >= 0.0 && cos_tilt <= 1.0)) return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // clouds ride on gridDim.y
    hipLaunchKernelGGL(iso_hypotheses_kernel, dim3((H + ISO_THREADS - 1) / ISO_THREADS, B), dim3(ISO_THREADS), 0, (hipStream_t)stream, H, points, offsets,
                       keys, has_up, up_x, up_y, up_z, cos_tilt, planes, valid);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_plane_score(int B, int M, int H, double tau, const double* points, const int* offsets, const double* planes, const int* valid,
                           int* counts, void* stream) {
    if (B < 1 || M < 0 || H < 1 || H > ISO_MAX_H || !(tau > 0.0 && std::isfinite(tau)) || !points || !offsets || !planes || !counts) return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // clouds ride on gridDim.z
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * H * 3 * sizeof(int), st) != hipSuccess) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    const int per = ISO_TILE * ISO_TILES_PER_GROUP, planes_per = ISO_THREADS * ISO_PLANES_PER_THREAD;
    hipLaunchKernelGGL(iso_score_kernel, dim3((M + per - 1) / per, (H + planes_per - 1) / planes_per, B), dim3(ISO_THREADS), 0, st, H, tau, points, offsets,
                       planes, valid, counts);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_plane_select(int B, int H, int has_up, int min_inliers, const double* planes, const int* valid, const int* counts, double* plane,
                            int* best_counts, int* found, void* stream) {
    if (B < 1 || H < 1 || H > ISO_MAX_H || !planes || !valid || !counts || !plane || !best_counts || !found) return ETCH_EINVAL;
    hipLaunchKernelGGL(iso_select_kernel, dim3(B), dim3(ISO_GROUP), 0, (hipStream_t)stream, H, has_up, min_inliers, planes, valid, counts, plane, best_counts,
                       found);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_plane_refit(int B, double tau, const double* points, const int* offsets, const int* found, double* plane, int* counts, void* stream) {
    if (B < 1 || !(tau > 0.0 && std::isfinite(tau)) || !points || !offsets || !found || !plane || !counts) return ETCH_EINVAL;
    hipLaunchKernelGGL(iso_refit_kernel, dim3(B), dim3(ISO_GROUP), 0, (hipStream_t)stream, tau, points, offsets, found, plane, counts);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_plane_keep(int B, int M, double tau, const double* points, const int* offsets, const double* plane, const int* found, int* keep,
                          void* stream) {
    if (B < 1 || M < 0 || !(tau > 0.0 && std::isfinite(tau)) || !points || !offsets || !plane || !found || !keep) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipLaunchKernelGGL(iso_plane_keep_kernel, dim3((M + ISO_THREADS - 1) / ISO_THREADS), dim3(ISO_THREADS), 0, (hipStream_t)stream, B, M, tau, points, offsets,
                       plane, found, keep);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_components(int B, int M, double radius, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                          const int* offsets, const int* status, int* parent, int* label, int* size, void* stream) {
    if (B < 1 || M < 0 || !(radius > 0.0 && std::isfinite(radius)) || !sorted_points || !offsets || !status || !parent || !label || !size)
        return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((M + ISO_THREADS - 1) / ISO_THREADS), block(ISO_THREADS);
    hipLaunchKernelGGL(iso_init_kernel, grid, block, 0, st, M, parent, size);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(iso_link_kernel, grid, block, 0, st, B, M, radius * radius, brute, sorted_points, sorted_keys, order, offsets, status, parent);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(iso_flatten_kernel, grid, block, 0, st, B, M, offsets, status, parent, label, size);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(iso_spread_kernel, grid, block, 0, st, B, M, offsets, status, label, size);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_component_keep(int B, int largest, int min_points, const int* label, const int* size, const int* offsets, int* winner, int* keep,
                              void* stream) {
    if (B < 1 || min_points < 1 || !label || !size || !offsets || !winner || !keep) return ETCH_EINVAL;
    hipLaunchKernelGGL(iso_component_keep_kernel, dim3(B), dim3(ISO_GROUP), 0, (hipStream_t)stream, largest, min_points, label, size, offsets, winner, keep);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
