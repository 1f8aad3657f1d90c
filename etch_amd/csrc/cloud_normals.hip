// Surface normals of raw clouds: for every row the covariance of its min(k, n - 1) nearest other rows of its cloud, the
// eigenvector of the smallest eigenvalue, the surface variation and the flags.  fp64, one rounding per operation: this file is built with
// -ffp-contract=off.
//
// The search is cloud_knn_kernel's (cloud_filter.hip): one thread per query, queries in sorted-cell order, rings rho = 0, 1, .. CLOUD_MAX_RINGS
// of cells, the stop rule kth <= (rho h (1 - 2^-20))^2, the whole-cloud scan for a query that is not done by then, and brute != 0 as the second
// implementation.  What differs is the list: it holds (d2, sorted index) and keeps the ke LEAST (d2, row) pairs, row = the original row, so a
// tie in d2 goes to the lower row whatever order the cells are walked in -- the tie break reads order[], as align_nearest_kernel's does.  After
// ring rho every unexamined row has d2 > lim^2 >= kth strictly, so no unexamined row can tie with a kept one.
//
// LDS: d2 as best[slot][thread] (8-byte stride between lanes) and behind it index[slot][thread] (4-byte stride): 12 k T bytes.  Either array
// puts the 32 lanes of a half wave on 32 different banks whatever slots they touch.  T = 256 threads up to k = 21 (63 KiB); above, T = 128
// (48 KiB at k = 32), which stays under the 64 KiB a workgroup gets without asking and lets three workgroups share a CU's 160 KiB.  Measured
// at 8 x 300 000 rows: 128 threads beat 256 at every k above 21 -- 18.7 against 19.8 ms at k = 22, 40.5 against 63.6 ms at k = 32.
//
// After the search the thread gathers its ke neighbours in list order, forms the moments in that order (so the covariance is defined to the
// bit) and runs the Jacobi of cloud_normal_solve.h in registers.
#include "common.h"
#include "etch_hip.h"
#include "cloud_grid.h"
#include "cloud_normal_solve.h"
#include <cmath>

#define CLOUD_MAX_RINGS ETCH_CLOUD_MAX_RINGS
#define NORMAL_WIDE_THREADS 256
#define NORMAL_NARROW_THREADS 128
#ifndef NORMAL_WIDE_MAX_K
#define NORMAL_WIDE_MAX_K 21                 // 21 * 256 * 12 B = 63 KiB; a measurement build may raise it (the launch then asks for the larger LDS)
#endif

static_assert(NORMAL_GAP_EPS == ETCH_NORMAL_GAP_EPS, "the gap threshold of the header");
static_assert(NORMAL_FLAG_FEW == ETCH_NORMAL_FLAG_FEW && NORMAL_FLAG_AMBIGUOUS == ETCH_NORMAL_FLAG_AMBIGUOUS, "the flags of the header");
static_assert((size_t)NORMAL_WIDE_MAX_K * NORMAL_WIDE_THREADS * 12 <= 160 * 1024 && (size_t)ETCH_CLOUD_MAX_K * NORMAL_NARROW_THREADS * 12 <= 65536,
              "the list of the narrow form fits 64 KiB, that of the wide form a CU");

namespace {

template <int THREADS>
__global__ __launch_bounds__(THREADS) void cloud_normals_kernel(int B, int M, int k, int brute, const double* __restrict__ P,
                                                                const long long* __restrict__ keys, const int* __restrict__ order,
                                                                const int* __restrict__ offsets, const double* __restrict__ grid,
                                                                const int* __restrict__ status, const double* __restrict__ viewpoint,
                                                                double* __restrict__ normal, double* __restrict__ variation, int* __restrict__ flag,
                                                                double* __restrict__ cov_out) {
    extern __shared__ double best[];                  // [k][THREADS] d2, then [k][THREADS] int sorted index
    int* const index = (int*)(best + (size_t)k * THREADS);
    const int tid = threadIdx.x;
    const int t = blockIdx.x * THREADS + tid;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const int row = brute ? t : order[t];
    const int ke = k < hi - lo - 1 ? k : hi - lo - 1;
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    double kth = INFINITY;
    int kidx = -1;
    for (int j = 0; j < ke; ++j) best[j * THREADS + tid] = INFINITY, index[j * THREADS + tid] = -1;
    // the original row of sorted row j; an empty slot sorts behind every row
    auto rowof = [&](int j) { return j < 0 ? 0x7fffffff : (brute ? j : order[j]); };
    auto visit = [&](int j) {
        if (j == t) return;
        const double d = cloud_d2(px, py, pz, P + 3 * (size_t)j);
        if (!(d <= kth)) return;
        if (d == kth && !(rowof(j) < rowof(kidx))) return;
        int s = ke - 1;
        while (s > 0) {
            const double up = best[(s - 1) * THREADS + tid];
            if (up < d) break;
            const int ui = index[(s - 1) * THREADS + tid];
            if (up == d && rowof(ui) < rowof(j)) break;
            best[s * THREADS + tid] = up;
            index[s * THREADS + tid] = ui;
            --s;
        }
        best[s * THREADS + tid] = d;
        index[s * THREADS + tid] = j;
        kth = best[(ke - 1) * THREADS + tid];
        kidx = index[(ke - 1) * THREADS + tid];
    };
    bool done = ke <= 0;
    if (!brute && !done) {
        const long long key = keys[t];
        const int ix = (int)(key >> (2 * CLOUD_BITS)), iy = (int)((key >> CLOUD_BITS) & CLOUD_CMAX), iz = (int)(key & CLOUD_CMAX);
        const double h = grid[4 * b + 3];
        for (int rho = 0; rho <= CLOUD_MAX_RINGS && !done; ++rho) {
            cloud_scan_ring(keys, lo, hi, ix, iy, iz, rho, visit);
            const double lim = ((double)rho * h) * (1.0 - 0x1p-20);
            done = kth <= lim * lim;
        }
        if (!done) {
            for (int j = 0; j < ke; ++j) best[j * THREADS + tid] = INFINITY, index[j * THREADS + tid] = -1;
            kth = INFINITY, kidx = -1;
        }
    }
    if (!done)
        for (int j = lo; j < hi; ++j) visit(j);
    double sum[3] = {0.0, 0.0, 0.0}, sq[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int u = 0; u < ke; ++u) {
        const int j = index[u * THREADS + tid];
        if (j < lo || j >= hi) continue;                                    // never: the scan above fills all ke slots from [lo, hi)
        const double* q = P + 3 * (size_t)j;
        const double e0 = q[0] - px, e1 = q[1] - py, e2 = q[2] - pz;
        sum[0] += e0, sum[1] += e1, sum[2] += e2;
        sq[0] += e0 * e0, sq[1] += e0 * e1, sq[2] += e0 * e2;
        sq[3] += e1 * e1, sq[4] += e1 * e2, sq[5] += e2 * e2;
    }
    double cov[6], lambda[3], n[3], var;
    normal_covariance(ke > 0 ? ke : 0, sum, sq, cov);
    const int fl = normal_solve(ke, cov, lambda, n, var);
    if (viewpoint) normal_face(viewpoint + 3 * b, px, py, pz, n);
    normal[3 * (size_t)row] = n[0], normal[3 * (size_t)row + 1] = n[1], normal[3 * (size_t)row + 2] = n[2];
    variation[row] = var;
    flag[row] = fl;
    if (cov_out) {
#pragma unroll
        for (int a = 0; a < 6; ++a) cov_out[6 * (size_t)row + a] = cov[a];
    }
}

}  // namespace

extern "C" {

int etch_cloud_normals(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets,
                       const double* grid, const int* status, const double* viewpoint, double* normal, double* variation, int* flag, double* cov,
                       void* stream) {
    if (B < 1 || M < 0 || k < 3 || k > ETCH_CLOUD_MAX_K || !sorted_points || !offsets || !status || !normal || !variation || !flag) return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order || !grid)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    if (k <= NORMAL_WIDE_MAX_K) {
        const size_t lds = (size_t)k * NORMAL_WIDE_THREADS * 12;
#if NORMAL_WIDE_MAX_K > 21
        if (hipFuncSetAttribute((const void*)cloud_normals_kernel<NORMAL_WIDE_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return ETCH_EUNSUPPORTED;
#endif
        hipLaunchKernelGGL(cloud_normals_kernel<NORMAL_WIDE_THREADS>, dim3((M + NORMAL_WIDE_THREADS - 1) / NORMAL_WIDE_THREADS),
                           dim3(NORMAL_WIDE_THREADS), lds, st, B, M, k, brute, sorted_points, sorted_keys, order, offsets, grid, status, viewpoint, normal,
                           variation, flag, cov);
    } else {
        const size_t lds = (size_t)k * NORMAL_NARROW_THREADS * 12;
        hipLaunchKernelGGL(cloud_normals_kernel<NORMAL_NARROW_THREADS>, dim3((M + NORMAL_NARROW_THREADS - 1) / NORMAL_NARROW_THREADS),
                           dim3(NORMAL_NARROW_THREADS), lds, st, B, M, k, brute, sorted_points, sorted_keys, order, offsets, grid, status, viewpoint,
                           normal, variation, flag, cov);
    }
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
