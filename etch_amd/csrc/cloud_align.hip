// Rigid registration of raw clouds: the nearest target row of every moved source row within a gate, on the target's cell
// grid; the moments of the matched pairs; Horn's closed-form rigid step; and the loop of both, which never returns to the host.  fp64, one
// rounding per operation: this file is built with -ffp-contract=off.
//
// Nearest: one thread per source row.  The query x = R p + t finds its cell in the TARGET cloud's grid (it may lie outside the grid: the columns
// that do not exist are skipped) and examines rings rho = 0, 1, .. of cells around it.  After ring rho every unexamined row differs from x by
// more than lim = rho h (1 - 2^-20) in some coordinate (cloud_filter.hip explains the factor), so the query stops once its best d2 <= lim^2 --
// or once lim^2 > g^2: a source row without a partner inside the gate is the common case in a partial overlap, and it never scans the cloud.
// The default cell is at least gate / (ALIGN_MAX_RINGS - 1), so ring ALIGN_MAX_RINGS always passes the first gate.  A query that is not done after
// ALIGN_MAX_RINGS rings (a cell far below the gate, given by the caller), or whose cell does not fit an int,
// starts again and scans its whole cloud; brute != 0 makes every query do that and reads neither keys nor order.  The result is the least
// (d2, row) among the rows with d2 <= g^2, so no form and no cell size can change it.
//
// Step: one workgroup per pair of clouds.  Every thread sums the rows lo + tid, lo + tid + 1024, .. in that order, a fixed tree adds the 1024
// partials: an order n alone fixes, no float atomics.  Thread 0 solves (cloud_align_solve.h) and composes.
#include "common.h"
#include "etch_hip.h"
#include "cloud_grid.h"
#include "cloud_align_solve.h"
#include <cmath>

#define ALIGN_MAX_RINGS ETCH_ALIGN_MAX_RINGS
#define ALIGN_QUERY_THREADS 256
#define ALIGN_GROUP 1024
#define ALIGN_CELL_ROWS 32.0                 // the cell size aims at this many rows per occupied cell

static_assert(ALIGN_RANK_EPS == ETCH_ALIGN_RANK_EPS, "the rank threshold of the header");

namespace {

// ---- bounding box, centre, status, cell size: one workgroup per target cloud --------------------------------------------------------------------
__global__ __launch_bounds__(ALIGN_GROUP) void align_bounds_kernel(double gate, double cell, const double* __restrict__ points,
                                                                   const int* __restrict__ offsets, double* __restrict__ grid,
                                                                   double* __restrict__ center, int* __restrict__ status) {
    __shared__ double s_min[3][ALIGN_GROUP], s_max[3][ALIGN_GROUP];
    __shared__ int s_bad[ALIGN_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = lo + tid; i < hi; i += ALIGN_GROUP) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = points[3 * (size_t)i + a];
            if (!isfinite(v)) bad = 1;
            mn[a] = fmin(mn[a], v);
            mx[a] = fmax(mx[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) s_min[a][tid] = mn[a], s_max[a][tid] = mx[a];
    s_bad[tid] = bad;
    __syncthreads();
    for (int w = ALIGN_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s_min[a][tid] = fmin(s_min[a][tid], s_min[a][tid + w]);
                s_max[a][tid] = fmax(s_max[a][tid], s_max[a][tid + w]);
            }
            s_bad[tid] |= s_bad[tid + w];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int st = 0;
    double h = 1.0, o[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    if (s_bad[0]) {
        st = ETCH_CLOUD_STATUS_NONFINITE;
    } else if (n > 0) {
        const double ex = s_max[0][0] - s_min[0][0], ey = s_max[1][0] - s_min[1][0], ez = s_max[2][0] - s_min[2][0];
        const double L = fmax(ex, fmax(ey, ez));
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = s_min[a][0], c[a] = 0.5 * (s_min[a][0] + s_max[a][0]);
        // gate / (ALIGN_MAX_RINGS - 1), not gate / ALIGN_MAX_RINGS: ring ALIGN_MAX_RINGS must reach lim = 8 h (1 - 2^-20) > gate STRICTLY, or a row without
        // a partner inside the first gate would leave the ring walk unfinished and scan its whole cloud
        if (cell > 0.0) h = cell;
        else h = fmax(fmax(sqrt(ALIGN_CELL_ROWS * (ex * ey + ey * ez + ez * ex) / (double)n), L * ALIGN_CELL_ROWS / (double)n), gate / (double)(ALIGN_MAX_RINGS - 1));
        h = fmax(h, L * 0x1p-20);                                           // at most 2^20 + 1 cells on an axis
        if (!(h > 0.0) || !isfinite(h)) h = 1.0;
    }
    grid[4 * b + 0] = o[0], grid[4 * b + 1] = o[1], grid[4 * b + 2] = o[2], grid[4 * b + 3] = h;
    center[3 * b + 0] = c[0], center[3 * b + 1] = c[1], center[3 * b + 2] = c[2];
    status[b] = st;
}

__global__ __launch_bounds__(256) void align_keys_kernel(int B, int M, const double* __restrict__ points, const int* __restrict__ offsets,
                                                         const double* __restrict__ grid, const int* __restrict__ status,
                                                         long long* __restrict__ keys, int* __restrict__ cloud) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M) return;
    if (t >= offsets[B]) {                     // no cloud's row: sorted behind all
        cloud[t] = B;
        keys[t] = 0x7fffffffffffffffll;
        return;
    }
    const int b = cloud_of_row(offsets, B, t);
    cloud[t] = b;
    long long key = 0;
    if (!(status[b] & ETCH_CLOUD_STATUS_NONFINITE)) {
        const double h = grid[4 * b + 3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double c = floor((points[3 * (size_t)t + a] - grid[4 * b + a]) / h);
            if (c > (double)CLOUD_CMAX) c = (double)CLOUD_CMAX;
            if (!(c >= 0.0)) c = 0.0;
            key = (key << CLOUD_BITS) | (long long)c;
        }
    }
    keys[t] = key;
}

// ---- the cross-query ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ALIGN_QUERY_THREADS) void align_nearest_kernel(int B, int Ms, int brute, const double* __restrict__ S,
                                                                            const int* __restrict__ soff, const int* __restrict__ qorder,
                                                                            const double* __restrict__ T, const long long* __restrict__ keys,
                                                                            const int* __restrict__ order, const int* __restrict__ toff,
                                                                            const double* __restrict__ grid, const double* __restrict__ Rm,
                                                                            const double* __restrict__ tv, const double* __restrict__ gate,
                                                                            const int* __restrict__ done, int* __restrict__ status,
                                                                            int* __restrict__ pair, double* __restrict__ d2out) {
    const int i = blockIdx.x * ALIGN_QUERY_THREADS + threadIdx.x;
    const int total = soff[B];
    if (i >= Ms || i >= total) return;
    const int row = qorder ? qorder[i] : i;
    if (row < 0 || row >= total) return;
    const int b = cloud_of_row(soff, B, row);
    if (done && done[b]) return;
    const double px = S[3 * (size_t)row], py = S[3 * (size_t)row + 1], pz = S[3 * (size_t)row + 2];
    const bool finite = isfinite(px) && isfinite(py) && isfinite(pz);
    // status[b] is read plainly while other threads may OR the bit in: which rows of such a pair get -1 / +inf depends on the timing, and that is
    // harmless only because a pair with the bit set makes the call raise -- nothing of it is a result
    if (!finite) atomicOr(&status[b], ETCH_CLOUD_STATUS_NONFINITE);
    if (!finite || (status[b] & ETCH_CLOUD_STATUS_NONFINITE)) {
        pair[row] = -1;
        d2out[row] = INFINITY;
        return;
    }
    double x, y, z;
    align_apply(Rm + 9 * b, tv + 3 * b, px, py, pz, x, y, z);
    const double g = gate[0], g2 = g * g;
    const int lo = toff[b], hi = toff[b + 1];
    double best = INFINITY;
    int brow = -1;
    auto visit = [&](int j) {
        const double d = cloud_d2(x, y, z, T + 3 * (size_t)j);
        if (d <= g2 && d <= best) {
            const int r = (brute ? j : order[j]) - lo;
            if (d < best || r < brow) best = d, brow = r;
        }
    };
    bool finished = false;
    if (!brute && hi > lo) {
        const double h = grid[4 * b + 3];
        const double cx = floor((x - grid[4 * b]) / h), cy = floor((y - grid[4 * b + 1]) / h), cz = floor((z - grid[4 * b + 2]) / h);
        if (fabs(cx) < 0x1p30 && fabs(cy) < 0x1p30 && fabs(cz) < 0x1p30) {      // false for NaN too
            const int ix = (int)cx, iy = (int)cy, iz = (int)cz;
            for (int rho = 0; rho <= ALIGN_MAX_RINGS && !finished; ++rho) {
                cloud_scan_ring(keys, lo, hi, ix, iy, iz, rho, visit);
                const double lim = ((double)rho * h) * (1.0 - 0x1p-20);
                const double lim2 = lim * lim;
                finished = best <= lim2 || lim2 > g2;
            }
            if (!finished) best = INFINITY, brow = -1;
        }
    }
    if (!finished)
        for (int j = lo; j < hi; ++j) visit(j);
    pair[row] = brow;
    d2out[row] = best;
}

// ---- moments, solve, compose: one workgroup per pair ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double align_block_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int w = ALIGN_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(ALIGN_GROUP) void align_step_kernel(const double* __restrict__ S, const int* __restrict__ soff, const double* __restrict__ T,
                                                                 const int* __restrict__ toff, const int* __restrict__ pair,
                                                                 const double* __restrict__ d2, const double* __restrict__ center, double tol_angle,
                                                                 double tol_shift, double* __restrict__ Rm, double* __restrict__ tv,
                                                                 double* __restrict__ sums, int* __restrict__ matched, double* __restrict__ rms,
                                                                 double* __restrict__ dR_out, double* __restrict__ dt_out, int* __restrict__ status,
                                                                 int* __restrict__ done, int* __restrict__ steps) {
    __shared__ double s[ALIGN_GROUP];
    __shared__ int si[ALIGN_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (done[b]) return;                                                    // uniform over the workgroup
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) {
        if (tid == 0) done[b] = 1;
        return;
    }
    const int lo = soff[b], hi = soff[b + 1], tlo = toff[b], tn = toff[b + 1] - tlo;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rm[9 * b + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tv[3 * b + k];
    const double c0 = center[3 * b], c1 = center[3 * b + 1], c2 = center[3 * b + 2];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    int m = 0;
    for (int i = lo + tid; i < hi; i += ALIGN_GROUP) {
        const int j = pair[i];
        if (j < 0 || j >= tn) continue;
        double x, y, z;
        align_apply(R, t, S[3 * (size_t)i], S[3 * (size_t)i + 1], S[3 * (size_t)i + 2], x, y, z);
        const double* q = T + 3 * (size_t)(tlo + j);
        const double xc[3] = {x - c0, y - c1, z - c2}, qc[3] = {q[0] - c0, q[1] - c1, q[2] - c2};
        ++m;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[a] += xc[a];
            acc[3 + a] += qc[a];
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[6 + 3 * a + e] += xc[a] * qc[e];
        }
        acc[15] += d2 ? d2[i] : cloud_d2(x, y, z, q);
    }
    __syncthreads();
    si[tid] = m;
    __syncthreads();
    for (int w = ALIGN_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) si[tid] += si[tid + w];
        __syncthreads();
    }
    m = si[0];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = align_block_sum(acc[k], s);
    if (tid != 0) return;
    double dR[9], dt[3], angle, shift;
    const double c[3] = {c0, c1, c2};
    const bool good = align_solve(m, acc, c, dR, dt, angle, shift);
    if (good) {
        align_compose(dR, dt, R, t);
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[9 * b + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[3 * b + k] = t[k];
        if (angle < tol_angle && shift < tol_shift) done[b] = 1;
    } else {
        status[b] |= ETCH_ALIGN_STATUS_DEGENERATE;                          // the transform stays for the rest of the call
        done[b] = 1;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) sums[16 * b + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) dR_out[9 * b + k] = dR[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) dt_out[3 * b + k] = dt[k];
    matched[b] = m;
    rms[b] = m > 0 ? sqrt(acc[15] / (double)m) : INFINITY;
    steps[b] = steps[b] + 1;
}

// ---- the point-to-plane step: 32 sums, the 6 x 6 solve, compose ------------------------------------------------------------------
#define ALIGN_PLANE_SUMS 32
#define ALIGN_PLANE_LANES 4                  // values that share one pass of the tree through LDS (4 x 8 KiB)

static_assert(ALIGN_PLANE_EPS == ETCH_ALIGN_PLANE_EPS, "the pivot threshold of the header");

// ALIGN_PLANE_LANES block sums in one pass: every value walks the tree of align_block_sum (s[tid] + s[tid + w], w = 512 .. 1) in a row of its own,
// so each sum has the bits a pass of its own would give, for a quarter of the barriers
__device__ __forceinline__ void align_block_sum_lanes(double* v, double (*s)[ALIGN_GROUP]) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < ALIGN_PLANE_LANES; ++a) s[a][tid] = v[a];
    __syncthreads();
    for (int w = ALIGN_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int a = 0; a < ALIGN_PLANE_LANES; ++a) s[a][tid] = s[a][tid] + s[a][tid + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < ALIGN_PLANE_LANES; ++a) v[a] = s[a][0];
}

__global__ __launch_bounds__(ALIGN_GROUP) void align_step_plane_kernel(const double* __restrict__ S, const int* __restrict__ soff, const double* __restrict__ T,
                                                                       const double* __restrict__ N, const int* __restrict__ toff,
                                                                       const int* __restrict__ pair, const double* __restrict__ d2,
                                                                       const double* __restrict__ grid, const double* __restrict__ center,
                                                                       double tol_angle, double tol_shift, double* __restrict__ Rm, double* __restrict__ tv,
                                                                       double* __restrict__ sums, int* __restrict__ matched, double* __restrict__ rms,
                                                                       double* __restrict__ dR_out, double* __restrict__ dt_out, double* __restrict__ y_out,
                                                                       int* __restrict__ status, int* __restrict__ done, int* __restrict__ steps) {
    __shared__ double s[ALIGN_PLANE_LANES][ALIGN_GROUP];
    __shared__ int si[ALIGN_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (done[b]) return;                                                    // uniform over the workgroup
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) {
        if (tid == 0) done[b] = 1;
        return;
    }
    const int lo = soff[b], hi = soff[b + 1], tlo = toff[b], tn = toff[b + 1] - tlo;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rm[9 * b + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tv[3 * b + k];
    const double c0 = center[3 * b], c1 = center[3 * b + 1], c2 = center[3 * b + 2];
    double acc[ALIGN_PLANE_SUMS];
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_SUMS; ++k) acc[k] = 0.0;
    int m = 0;
    for (int i = lo + tid; i < hi; i += ALIGN_GROUP) {
        const int j = pair[i];
        if (j < 0 || j >= tn) continue;
        const double* nr = N + 3 * (size_t)(tlo + j);
        const double n0 = nr[0], n1 = nr[1], n2 = nr[2];
        if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) continue;                  // a target row without a normal matches nothing
        double x, y, z;
        align_apply(R, t, S[3 * (size_t)i], S[3 * (size_t)i + 1], S[3 * (size_t)i + 2], x, y, z);
        const double* q = T + 3 * (size_t)(tlo + j);
        const double xc0 = x - c0, xc1 = y - c1, xc2 = z - c2;
        const double r = ((x - q[0]) * n0 + (y - q[1]) * n1) + (z - q[2]) * n2;
        const double J[6] = {xc1 * n2 - xc2 * n1, xc2 * n0 - xc0 * n2, xc0 * n1 - xc1 * n0, n0, n1, n2};
        ++m;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) acc[e++] += J[a] * J[c];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
        acc[27] += r * r;
        acc[28] += d2 ? d2[i] : cloud_d2(x, y, z, q);
        acc[29] += xc0, acc[30] += xc1, acc[31] += xc2;
    }
    __syncthreads();
    si[tid] = m;
    __syncthreads();
    for (int w = ALIGN_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) si[tid] += si[tid + w];
        __syncthreads();
    }
    m = si[0];
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_SUMS; k += ALIGN_PLANE_LANES) align_block_sum_lanes(acc + k, s);
    if (tid != 0) return;
    double* const total = s[0];                                             // the 32 sums parked in LDS: the solve's 6 x 6 factor needs the registers
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_SUMS; ++k) total[k] = acc[k];
    double dR[9], dt[3], yv[6], angle, shift;
    const double c[3] = {c0, c1, c2};
    const double e0 = c0 - grid[4 * b], e1 = c1 - grid[4 * b + 1], e2 = c2 - grid[4 * b + 2];
    const double rho = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    const bool good = align_plane_solve(m, total, c, rho, dR, dt, angle, shift, yv);
    if (good) {
        align_compose(dR, dt, R, t);
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[9 * b + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[3 * b + k] = t[k];
        if (angle < tol_angle && shift < tol_shift) done[b] = 1;
    } else {
        status[b] |= ETCH_ALIGN_STATUS_DEGENERATE;                          // the transform stays for the rest of the call
        done[b] = 1;
    }
#pragma unroll
    for (int k = 0; k < ALIGN_PLANE_SUMS; ++k) sums[ALIGN_PLANE_SUMS * b + k] = total[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) dR_out[9 * b + k] = dR[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) dt_out[3 * b + k] = dt[k];
    if (y_out) {
#pragma unroll
        for (int k = 0; k < 6; ++k) y_out[6 * b + k] = yv[k];
    }
    matched[b] = m;
    rms[b] = m > 0 ? sqrt(total[28] / (double)m) : INFINITY;
    steps[b] = steps[b] + 1;
}

__global__ __launch_bounds__(256) void align_transform_kernel(int B, int M, const double* __restrict__ P, const int* __restrict__ offsets,
                                                              const double* __restrict__ Rm, const double* __restrict__ tv, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M || i >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, i);
    double x, y, z;
    align_apply(Rm + 9 * b, tv + 3 * b, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], x, y, z);
    out[3 * (size_t)i] = x, out[3 * (size_t)i + 1] = y, out[3 * (size_t)i + 2] = z;
}

int launch_nearest(int B, int Ms, int brute, const double* src, const int* soff, const int* qorder, const double* tgt, const long long* keys,
                   const int* order, const int* toff, const double* grid, const double* R, const double* t, const double* gate, const int* done,
                   int* status, int* pair, double* d2, hipStream_t st) {
    hipLaunchKernelGGL(align_nearest_kernel, dim3((Ms + ALIGN_QUERY_THREADS - 1) / ALIGN_QUERY_THREADS), dim3(ALIGN_QUERY_THREADS), 0, st, B, Ms, brute,
                       src, soff, qorder, tgt, keys, order, toff, grid, R, t, gate, done, status, pair, d2);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int launch_step(int B, const double* src, const int* soff, const double* tgt, const int* toff, const int* pair, const double* d2, const double* center,
                double tol_angle, double tol_shift, double* R, double* t, double* sums, int* matched, double* rms, double* dR, double* dt, int* status,
                int* done, int* steps, hipStream_t st) {
    hipLaunchKernelGGL(align_step_kernel, dim3(B), dim3(ALIGN_GROUP), 0, st, src, soff, tgt, toff, pair, d2, center, tol_angle, tol_shift, R, t, sums, matched,
                       rms, dR, dt, status, done, steps);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int launch_step_plane(int B, const double* src, const int* soff, const double* tgt, const double* normals, const int* toff, const int* pair, const double* d2,
                      const double* grid, const double* center, double tol_angle, double tol_shift, double* R, double* t, double* sums, int* matched,
                      double* rms, double* dR, double* dt, double* y, int* status, int* done, int* steps, hipStream_t st) {
    hipLaunchKernelGGL(align_step_plane_kernel, dim3(B), dim3(ALIGN_GROUP), 0, st, src, soff, tgt, normals, toff, pair, d2, grid, center, tol_angle, tol_shift,
                       R, t, sums, matched, rms, dR, dt, y, status, done, steps);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // namespace

extern "C" {

int etch_cloud_align_grid(int B, int M, double gate, double cell, const double* points, const int* offsets, double* grid, double* center,
                          long long* keys, int* cloud, int* status, void* stream) {
    if (B < 1 || M < 0 || !points || !offsets || !grid || !center || !keys || !cloud || !status) return ETCH_EINVAL;
    if (!(gate > 0.0 && std::isfinite(gate)) || !(cell >= 0.0) || !std::isfinite(cell)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(align_bounds_kernel, dim3(B), dim3(ALIGN_GROUP), 0, st, gate, cell, points, offsets, grid, center, status);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (M > 0) {
        hipLaunchKernelGGL(align_keys_kernel, dim3((M + 255) / 256), dim3(256), 0, st, B, M, points, offsets, grid, status, keys, cloud);
        ETCH_RETURN_IF_LAUNCH_FAILED();
    }
    return ETCH_OK;
}

int etch_cloud_nearest(int B, int Ms, int brute, const double* src_points, const int* src_offsets, const int* query_order, const double* tgt_points,
                       const long long* tgt_keys, const int* tgt_order, const int* tgt_offsets, const double* grid, const double* R, const double* t,
                       const double* gate, const int* done, int* status, int* pair, double* d2, void* stream) {
    if (B < 1 || Ms < 0 || !src_points || !src_offsets || !tgt_points || !tgt_offsets || !R || !t || !gate || !status || !pair || !d2) return ETCH_EINVAL;
    if (!brute && (!tgt_keys || !tgt_order || !grid)) return ETCH_EINVAL;
    if (Ms == 0) return ETCH_OK;
    return launch_nearest(B, Ms, brute, src_points, src_offsets, query_order, tgt_points, tgt_keys, tgt_order, tgt_offsets, grid, R, t, gate, done, status,
                          pair, d2, (hipStream_t)stream);
}

int etch_cloud_align_step(int B, const double* src_points, const int* src_offsets, const double* tgt_points, const int* tgt_offsets, const int* pair,
                          const double* d2, const double* center, double tol_angle, double tol_shift, double* R, double* t, double* sums, int* matched,
                          double* rms, double* dR, double* dt, int* status, int* done, int* steps, void* stream) {
    if (B < 1 || !src_points || !src_offsets || !tgt_points || !tgt_offsets || !pair || !center || !R || !t || !sums || !matched || !rms || !dR || !dt ||
        !status || !done || !steps)
        return ETCH_EINVAL;
    if (!(tol_angle >= 0.0) || !(tol_shift >= 0.0)) return ETCH_EINVAL;
    return launch_step(B, src_points, src_offsets, tgt_points, tgt_offsets, pair, d2, center, tol_angle, tol_shift, R, t, sums, matched, rms, dR, dt, status,
                       done, steps, (hipStream_t)stream);
}

int etch_cloud_align(int B, int Ms, int iters, int brute, const double* src_points, const int* src_offsets, const int* query_order,
                     const double* tgt_sorted, const long long* tgt_keys, const int* tgt_order, const double* tgt_points, const int* tgt_offsets,
                     const double* grid, const double* center, const double* gates, double tol_angle, double tol_shift, double* R, double* t,
                     double* sums, int* matched, double* rms, double* dR, double* dt, int* status, int* done, int* steps, int* pair, double* d2,
                     void* stream) {
    if (B < 1 || Ms < 0 || iters < 1 || !src_points || !src_offsets || !tgt_points || !tgt_offsets || !center || !gates || !R || !t || !sums || !matched ||
        !rms || !dR || !dt || !status || !done || !steps || !pair || !d2)
        return ETCH_EINVAL;
    if (!brute && (!tgt_sorted || !tgt_keys || !tgt_order || !grid)) return ETCH_EINVAL;
    if (!(tol_angle >= 0.0) || !(tol_shift >= 0.0)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < iters; ++k) {                                       // two launches a step; the done flags live on the device
        if (Ms > 0) {
            const int e = launch_nearest(B, Ms, brute, src_points, src_offsets, query_order, brute ? tgt_points : tgt_sorted, tgt_keys, tgt_order, tgt_offsets,
                                         grid, R, t, gates + k, done, status, pair, d2, st);
            if (e != ETCH_OK) return e;
        }
        const int e = launch_step(B, src_points, src_offsets, tgt_points, tgt_offsets, pair, d2, center, tol_angle, tol_shift, R, t, sums, matched, rms, dR, dt,
                                  status, done, steps, st);
        if (e != ETCH_OK) return e;
    }
    return ETCH_OK;
}

int etch_cloud_align_step_plane(int B, const double* src_points, const int* src_offsets, const double* tgt_points, const double* tgt_normals,
                                const int* tgt_offsets, const int* pair, const double* d2, const double* grid, const double* center, double tol_angle,
                                double tol_shift, double* R, double* t, double* sums, int* matched, double* rms, double* dR, double* dt, double* y,
                                int* status, int* done, int* steps, void* stream) {
    if (B < 1 || !src_points || !src_offsets || !tgt_points || !tgt_normals || !tgt_offsets || !pair || !grid || !center || !R || !t || !sums || !matched ||
        !rms || !dR || !dt || !status || !done || !steps)
        return ETCH_EINVAL;
    if (!(tol_angle >= 0.0) || !(tol_shift >= 0.0)) return ETCH_EINVAL;
    return launch_step_plane(B, src_points, src_offsets, tgt_points, tgt_normals, tgt_offsets, pair, d2, grid, center, tol_angle, tol_shift, R, t, sums, matched,
                             rms, dR, dt, y, status, done, steps, (hipStream_t)stream);
}

int etch_cloud_align_plane(int B, int Ms, int iters, int brute, const double* src_points, const int* src_offsets, const int* query_order,
                           const double* tgt_sorted, const long long* tgt_keys, const int* tgt_order, const double* tgt_points, const double* tgt_normals,
                           const int* tgt_offsets, const double* grid, const double* center, const double* gates, double tol_angle, double tol_shift,
                           double* R, double* t, double* sums, int* matched, double* rms, double* dR, double* dt, int* status, int* done, int* steps,
                           int* pair, double* d2, void* stream) {
    if (B < 1 || Ms < 0 || iters < 1 || !src_points || !src_offsets || !tgt_points || !tgt_normals || !tgt_offsets || !grid || !center || !gates || !R || !t ||
        !sums || !matched || !rms || !dR || !dt || !status || !done || !steps || !pair || !d2)
        return ETCH_EINVAL;
    if (!brute && (!tgt_sorted || !tgt_keys || !tgt_order)) return ETCH_EINVAL;
    if (!(tol_angle >= 0.0) || !(tol_shift >= 0.0)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < iters; ++k) {                                       // two launches a step; the done flags live on the device
        if (Ms > 0) {
            const int e = launch_nearest(B, Ms, brute, src_points, src_offsets, query_order, brute ? tgt_points : tgt_sorted, tgt_keys, tgt_order, tgt_offsets,
                                         grid, R, t, gates + k, done, status, pair, d2, st);
            if (e != ETCH_OK) return e;
        }
        const int e = launch_step_plane(B, src_points, src_offsets, tgt_points, tgt_normals, tgt_offsets, pair, d2, grid, center, tol_angle, tol_shift, R, t, sums,
                                        matched, rms, dR, dt, nullptr, status, done, steps, st);
        if (e != ETCH_OK) return e;
    }
    return ETCH_OK;
}

int etch_cloud_transform(int B, int M, const double* points, const int* offsets, const double* R, const double* t, double* out, void* stream) {
    if (B < 1 || M < 0 || !points || !offsets || !R || !t || !out) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipLaunchKernelGGL(align_transform_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, M, points, offsets, R, t, out);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
