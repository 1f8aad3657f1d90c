// Raw point clouds: exact grid kNN mean distance, radius neighbour counts, the statistical keep mask, stable compaction
// and the voxel grid.  fp64, one rounding per operation: this file is built with -ffp-contract=off.
//
// The grid is an accelerator, never an approximation, and it costs O(M) memory: etch_cloud_cell_keys gives every row the 63-bit key of its
// cell (21 bits per axis, origin = the cloud's bounding-box minimum), the caller sorts the rows by (cloud, key) with a stable sort -- so a
// cloud's rows stay one segment, and the rows of one cell one run in ascending row order -- and a query finds a column of cells (fixed ix, iy,
// a range of iz = a range of consecutive keys) with two binary searches over its cloud's segment of the sorted keys.
//
// kNN: one thread per query, queries in sorted-cell order (the lanes of a wave read the same neighbour cells).  The k best squared distances
// of a thread live in LDS as best[slot][thread] (k x 256 doubles per workgroup, 8-byte stride between lanes: no bank conflict whatever slot a
// lane touches), sorted ascending by insertion; the k-th is mirrored in a register.  Rings rho = 0, 1, .. CLOUD_MAX_RINGS of cells around the
// query's cell are examined shell by shell; after ring rho every unexamined point differs by more than rho h in some coordinate, so the query
// stops once its k-th d2 <= (rho h (1 - 2^-20))^2 -- the factor covers the rounding of floor((p - o) / h), which may put a point that lies
// within a few ulp of a cell wall on either side of it.  A query that is not done after CLOUD_MAX_RINGS rings (a far outlier) starts again
// and scans its whole cloud; brute != 0 makes every query do that and reads neither keys nor order.
#include "common.h"
#include "etch_hip.h"
#include "cloud_grid.h"                     // cloud_d2, cloud_of_row, cloud_lower_bound, cloud_scan_column: shared with cloud_isolate.hip
#include <cmath>

#define CLOUD_MAX_RINGS ETCH_CLOUD_MAX_RINGS
#define CLOUD_QUERY_THREADS 256
#define CLOUD_SCAN_THREADS 1024
#define CLOUD_SCAN_GROUPS 32                 // workgroups that share one cloud's rows in the compaction and the voxel grid

namespace {

// ---- bounding box, status, cell size: one workgroup per cloud ------------------------------------------------------------------------------
__global__ __launch_bounds__(CLOUD_SCAN_THREADS) void cloud_bounds_kernel(int mode, int k, double cell, const double* __restrict__ points,
                                                                          const int* __restrict__ offsets, double* __restrict__ grid,
                                                                          int* __restrict__ status) {
    __shared__ double s_min[3][CLOUD_SCAN_THREADS], s_max[3][CLOUD_SCAN_THREADS];
    __shared__ int s_bad[CLOUD_SCAN_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = lo + tid; i < hi; i += CLOUD_SCAN_THREADS) {
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
    for (int w = CLOUD_SCAN_THREADS / 2; w >= 1; w >>= 1) {
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
    double h = 1.0, o[3] = {0.0, 0.0, 0.0};
    if (s_bad[0]) {
        st = ETCH_CLOUD_STATUS_NONFINITE;
    } else if (n == 0) {
        st = mode == 2 ? ETCH_CLOUD_STATUS_EMPTY : 0;
    } else {
        const double ex = s_max[0][0] - s_min[0][0], ey = s_max[1][0] - s_min[1][0], ez = s_max[2][0] - s_min[2][0];
        const double L = fmax(ex, fmax(ey, ez));
        o[0] = s_min[0][0], o[1] = s_min[1][0], o[2] = s_min[2][0];
        if (mode == 2) {
            h = cell;
        } else {
            if (mode == 1) h = cell * (1.0 + 0x1p-20);                      // a little above r: a pair at d2 <= r r never sits two cells apart
            else if (cell > 0.0) h = cell;
            else h = fmax(sqrt((double)k * (ex * ey + ey * ez + ez * ex) / (double)n), L * (double)k / (double)n);
            h = fmax(h, L * 0x1p-20);                                       // at most 2^20 + 1 cells on an axis
            if (!(h > 0.0) || !isfinite(h)) h = 1.0;                        // every point coincides
        }
    }
    grid[4 * b + 0] = o[0], grid[4 * b + 1] = o[1], grid[4 * b + 2] = o[2], grid[4 * b + 3] = h;
    status[b] = st;
}

__global__ __launch_bounds__(256) void cloud_keys_kernel(int B, int M, int mode, const double* __restrict__ points, const int* __restrict__ offsets,
                                                         const double* __restrict__ grid, long long* __restrict__ keys, int* __restrict__ cloud,
                                                         int* __restrict__ status) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M) return;
    if (t >= offsets[B]) {                     // room an earlier compaction left behind the last cloud: no cloud's row, sorted behind all
        cloud[t] = B;
        keys[t] = 0x7fffffffffffffffll;
        return;
    }
    const int b = cloud_of_row(offsets, B, t);
    cloud[t] = b;
    long long key = 0;
    if (!(status[b] & ETCH_CLOUD_STATUS_NONFINITE)) {
        const double h = grid[4 * b + 3];
        bool range = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double c = floor((points[3 * (size_t)t + a] - grid[4 * b + a]) / h);
            if (c > (double)CLOUD_CMAX) range = true, c = (double)CLOUD_CMAX;
            if (!(c >= 0.0)) c = 0.0;
            key = (key << CLOUD_BITS) | (long long)c;
        }
        if (range && mode == 2) atomicOr(&status[b], ETCH_CLOUD_STATUS_RANGE);
    }
    keys[t] = key;
}

// ---- kNN mean distance ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CLOUD_QUERY_THREADS) void cloud_knn_kernel(int B, int M, int k, int brute, const double* __restrict__ P,
                                                                        const long long* __restrict__ keys, const int* __restrict__ order,
                                                                        const int* __restrict__ offsets, const double* __restrict__ grid,
                                                                        const int* __restrict__ status, double* __restrict__ mean) {
    extern __shared__ double best[];                  // [k][CLOUD_QUERY_THREADS]
    const int tid = threadIdx.x;
    const int t = blockIdx.x * CLOUD_QUERY_THREADS + tid;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const int row = brute ? t : order[t];
    const int ke = k < hi - lo - 1 ? k : hi - lo - 1;
    if (ke <= 0) {
        mean[row] = 0.0;
        return;
    }
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    double kth = INFINITY;
    for (int j = 0; j < ke; ++j) best[j * CLOUD_QUERY_THREADS + tid] = INFINITY;
    auto visit = [&](int j) {
        if (j == t) return;
        const double d = cloud_d2(px, py, pz, P + 3 * (size_t)j);
        if (d < kth) {
            int s = ke - 1;
            while (s > 0) {
                const double up = best[(s - 1) * CLOUD_QUERY_THREADS + tid];
                if (!(up > d)) break;
                best[s * CLOUD_QUERY_THREADS + tid] = up;
                --s;
            }
            best[s * CLOUD_QUERY_THREADS + tid] = d;
            kth = best[(ke - 1) * CLOUD_QUERY_THREADS + tid];
        }
    };
    bool done = false;
    if (!brute) {
        const long long key = keys[t];
        const int ix = (int)(key >> (2 * CLOUD_BITS)), iy = (int)((key >> CLOUD_BITS) & CLOUD_CMAX), iz = (int)(key & CLOUD_CMAX);
        const double h = grid[4 * b + 3];
        for (int rho = 0; rho <= CLOUD_MAX_RINGS && !done; ++rho) {
            cloud_scan_ring(keys, lo, hi, ix, iy, iz, rho, visit);
            const double lim = ((double)rho * h) * (1.0 - 0x1p-20);
            done = kth <= lim * lim;
        }
        if (!done) {
            for (int j = 0; j < ke; ++j) best[j * CLOUD_QUERY_THREADS + tid] = INFINITY;
            kth = INFINITY;
        }
    }
    if (!done)
        for (int j = lo; j < hi; ++j) visit(j);
    double s = 0.0;
    for (int j = 0; j < ke; ++j) s += sqrt(best[j * CLOUD_QUERY_THREADS + tid]);
    mean[row] = s / (double)ke;
}

// ---- radius neighbour counts: h >= r, so the 27 cells around a query hold every neighbour ------------------------------------------------------
__global__ __launch_bounds__(CLOUD_QUERY_THREADS) void cloud_radius_kernel(int B, int M, double r2, int brute, const double* __restrict__ P,
                                                                           const long long* __restrict__ keys, const int* __restrict__ order,
                                                                           const int* __restrict__ offsets, const int* __restrict__ status,
                                                                           int* __restrict__ count) {
    const int t = blockIdx.x * CLOUD_QUERY_THREADS + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    int c = 0;
    auto visit = [&](int j) {
        if (j != t && cloud_d2(px, py, pz, P + 3 * (size_t)j) <= r2) ++c;
    };
    if (brute) {
        for (int j = lo; j < hi; ++j) visit(j);
        count[t] = c;
        return;
    }
    const long long key = keys[t];
    const int ix = (int)(key >> (2 * CLOUD_BITS)), iy = (int)((key >> CLOUD_BITS) & CLOUD_CMAX), iz = (int)(key & CLOUD_CMAX);
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) cloud_scan_column(keys, lo, hi, ix + dx, iy + dy, iz - 1, iz + 1, visit);
    count[order[t]] = c;
}

// ---- statistical keep mask: one workgroup per cloud, sums in an order n alone fixes ---------------------------------------------------------
__device__ __forceinline__ double cloud_block_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int w = CLOUD_SCAN_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(CLOUD_SCAN_THREADS) void cloud_stat_kernel(double ratio, const double* __restrict__ mean, const int* __restrict__ offsets,
                                                                        int* __restrict__ status, double* __restrict__ stats, int* __restrict__ keep) {
    __shared__ double s[CLOUD_SCAN_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    if (n == 0) {
        if (tid == 0) status[b] |= ETCH_CLOUD_STATUS_EMPTY, stats[2 * b] = 0.0, stats[2 * b + 1] = 0.0;
        return;
    }
    double part = 0.0;
    for (int i = lo + tid; i < hi; i += CLOUD_SCAN_THREADS) part += mean[i];
    const double mu = cloud_block_sum(part, s) / (double)n;
    part = 0.0;
    for (int i = lo + tid; i < hi; i += CLOUD_SCAN_THREADS) {
        const double d = mean[i] - mu;
        part += d * d;
    }
    const double ss = cloud_block_sum(part, s);
    const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : 0.0;
    const double thr = mu + ratio * sd;
    for (int i = lo + tid; i < hi; i += CLOUD_SCAN_THREADS) keep[i] = mean[i] <= thr ? 1 : 0;
    if (tid == 0) stats[2 * b] = mu, stats[2 * b + 1] = sd;
}

// ---- stable compaction of flagged rows: CLOUD_SCAN_GROUPS workgroups per cloud, each owns one part of its rows, thread i the i-th chunk of it ------
// PHASE 0 counts a workgroup's flagged rows into part[]; PHASE 1 (a second launch) places them behind those of every workgroup before it.
struct KeepFlag {
    const int* keep;
    __device__ bool operator()(int j, int lo) const { return keep[j] != 0; }
};
struct HeadFlag {                                 // the first sorted row of every occupied cell
    const long long* keys;
    __device__ bool operator()(int j, int lo) const { return j == lo || keys[j] != keys[j - 1]; }
};

template <int PHASE, class Flag, class Write>
__device__ __forceinline__ void cloud_compact_body(int B, const int* __restrict__ offsets, bool skip, int* __restrict__ part, int* __restrict__ total,
                                                   int* __restrict__ new_offsets, Flag flag, Write write) {
    __shared__ int s_count[CLOUD_SCAN_THREADS], s_sum[CLOUD_SCAN_THREADS];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
    const int len = (n + CLOUD_SCAN_GROUPS - 1) / CLOUD_SCAN_GROUPS;                  // rows of this workgroup: the g-th part of the cloud
    const long long s64 = (long long)lo + (long long)g * len;
    const int seg_lo = s64 < hi ? (int)s64 : hi, seg_hi = s64 + len < hi ? (int)(s64 + len) : hi;
    const int chunk = (seg_hi - seg_lo + CLOUD_SCAN_THREADS - 1) / CLOUD_SCAN_THREADS;
    const long long a64 = (long long)seg_lo + (long long)tid * chunk;
    const int a = a64 < seg_hi ? (int)a64 : seg_hi;
    const int e = a64 + chunk < seg_hi ? (int)(a64 + chunk) : seg_hi;
    int c = 0;
    if (!skip)
        for (int j = a; j < e; ++j) c += flag(j, lo) ? 1 : 0;
    s_count[tid] = c;
    const int me = b * CLOUD_SCAN_GROUPS + g;
    if (PHASE == 1) {                                 // the flagged rows of every workgroup before this one (integers: any order gives the same sum)
        int before = 0;
        for (int i = tid; i < me; i += CLOUD_SCAN_THREADS) before += part[i];
        s_sum[tid] = before;
    }
    __syncthreads();
    if (PHASE == 1)
        for (int w = CLOUD_SCAN_THREADS / 2; w >= 1; w >>= 1) {
            if (tid < w) s_sum[tid] += s_sum[tid + w];
            __syncthreads();
        }
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < CLOUD_SCAN_THREADS; ++i) {
            const int v = s_count[i];
            s_count[i] = run;
            run += v;
        }
        if (PHASE == 0) {
            part[me] = run;
        } else if (me == 0) {
            int acc = 0;
            for (int i = 0; i < B; ++i) {
                int sum = 0;
                for (int j = 0; j < CLOUD_SCAN_GROUPS; ++j) sum += part[i * CLOUD_SCAN_GROUPS + j];
                new_offsets[i] = acc, total[i] = sum, acc += sum;
            }
            new_offsets[B] = acc;
        }
    }
    if (PHASE == 0) return;
    __syncthreads();
    if (skip) return;
    int slot = s_sum[0] + s_count[tid];
    for (int j = a; j < e; ++j)
        if (flag(j, lo)) write(j, slot++, lo, hi);
}

template <int PHASE>
__global__ __launch_bounds__(CLOUD_SCAN_THREADS) void cloud_compact_kernel(int B, const int* __restrict__ keep, const int* __restrict__ offsets,
                                                                           const double* __restrict__ points, const int* __restrict__ index,
                                                                           int* __restrict__ part, int* __restrict__ total,
                                                                           int* __restrict__ new_offsets, int* __restrict__ new_index,
                                                                           double* __restrict__ new_points) {
    cloud_compact_body<PHASE>(B, offsets, false, part, total, new_offsets, KeepFlag{keep}, [&](int j, int slot, int lo, int hi) {
        new_index[slot] = index[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) new_points[3 * (size_t)slot + a] = points[3 * (size_t)j + a];
    });
}

template <int PHASE>
__global__ __launch_bounds__(CLOUD_SCAN_THREADS) void cloud_voxel_kernel(int B, const double* __restrict__ P, const long long* __restrict__ keys,
                                                                         const int* __restrict__ order, const int* __restrict__ offsets,
                                                                         const int* __restrict__ status, int* __restrict__ part,
                                                                         int* __restrict__ total, int* __restrict__ out_offsets, double* __restrict__ centroid,
                                                                         int* __restrict__ count, int* __restrict__ lowest,
                                                                         long long* __restrict__ cell_key) {
    cloud_compact_body<PHASE>(B, offsets, status[blockIdx.y] != 0, part, total, out_offsets, HeadFlag{keys}, [&](int j, int slot, int lo, int hi) {
        const long long key = keys[j];
        double sx = P[3 * (size_t)j], sy = P[3 * (size_t)j + 1], sz = P[3 * (size_t)j + 2];
        int e = j + 1;
        for (; e < hi && keys[e] == key; ++e) sx += P[3 * (size_t)e], sy += P[3 * (size_t)e + 1], sz += P[3 * (size_t)e + 2];
        const double c = (double)(e - j);
        centroid[3 * (size_t)slot] = sx / c, centroid[3 * (size_t)slot + 1] = sy / c, centroid[3 * (size_t)slot + 2] = sz / c;
        count[slot] = e - j;
        lowest[slot] = order[j] - lo;             // the sort is stable: a cell's first sorted row is its lowest row
        cell_key[slot] = key;
    });
}

}  // namespace

extern "C" {

int etch_cloud_cell_keys(int B, int M, int mode, int k, double cell, const double* points, const int* offsets, double* grid, long long* keys,
                         int* cloud, int* status, void* stream) {
    if (B < 1 || M < 0 || mode < 0 || mode > 2 || !points || !offsets || !grid || !keys || !cloud || !status) return ETCH_EINVAL;
    if (mode == 0 && (k < 1 || k > ETCH_CLOUD_MAX_K || !(cell >= 0.0) || !std::isfinite(cell))) return ETCH_EINVAL;
    if (mode != 0 && !(cell > 0.0 && std::isfinite(cell))) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cloud_bounds_kernel, dim3(B), dim3(CLOUD_SCAN_THREADS), 0, st, mode, k, cell, points, offsets, grid, status);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (M > 0) {
        hipLaunchKernelGGL(cloud_keys_kernel, dim3((M + 255) / 256), dim3(256), 0, st, B, M, mode, points, offsets, grid, keys, cloud, status);
        ETCH_RETURN_IF_LAUNCH_FAILED();
    }
    return ETCH_OK;
}

int etch_cloud_knn_mean(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                        const int* offsets, const double* grid, const int* status, double* mean, void* stream) {
    if (B < 1 || M < 0 || k < 1 || k > ETCH_CLOUD_MAX_K || !sorted_points || !offsets || !status || !mean) return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order || !grid)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    const size_t lds = (size_t)k * CLOUD_QUERY_THREADS * sizeof(double);          // at most 64 KiB
    hipLaunchKernelGGL(cloud_knn_kernel, dim3((M + CLOUD_QUERY_THREADS - 1) / CLOUD_QUERY_THREADS), dim3(CLOUD_QUERY_THREADS), lds, (hipStream_t)stream,
                       B, M, k, brute, sorted_points, sorted_keys, order, offsets, grid, status, mean);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_radius_count(int B, int M, double radius, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                            const int* offsets, const int* status, int* count, void* stream) {
    if (B < 1 || M < 0 || !(radius > 0.0 && std::isfinite(radius)) || !sorted_points || !offsets || !status || !count) return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipLaunchKernelGGL(cloud_radius_kernel, dim3((M + CLOUD_QUERY_THREADS - 1) / CLOUD_QUERY_THREADS), dim3(CLOUD_QUERY_THREADS), 0, (hipStream_t)stream,
                       B, M, radius * radius, brute, sorted_points, sorted_keys, order, offsets, status, count);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_stat_keep(int B, double ratio, const double* mean, const int* offsets, int* status, double* stats, int* keep, void* stream) {
    if (B < 1 || !std::isfinite(ratio) || !mean || !offsets || !status || !stats || !keep) return ETCH_EINVAL;
    hipLaunchKernelGGL(cloud_stat_kernel, dim3(B), dim3(CLOUD_SCAN_THREADS), 0, (hipStream_t)stream, ratio, mean, offsets, status, stats, keep);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_scan_workspace(int B, long long* bytes) {
    if (B < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)B * CLOUD_SCAN_GROUPS * (long long)sizeof(int);
    return ETCH_OK;
}

int etch_cloud_compact(int B, const int* keep, const int* offsets, const double* points, const int* index, void* workspace, int* kept,
                       int* new_offsets, int* new_index, double* new_points, void* stream) {
    if (B < 1 || !keep || !offsets || !points || !index || !workspace || !kept || !new_offsets || !new_index || !new_points) return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // clouds ride on gridDim.y
    hipStream_t st = (hipStream_t)stream;
    int* part = (int*)workspace;
    const dim3 grid(CLOUD_SCAN_GROUPS, B);
    hipLaunchKernelGGL(cloud_compact_kernel<0>, grid, dim3(CLOUD_SCAN_THREADS), 0, st, B, keep, offsets, points, index, part, kept, new_offsets, new_index,
                       new_points);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(cloud_compact_kernel<1>, grid, dim3(CLOUD_SCAN_THREADS), 0, st, B, keep, offsets, points, index, part, kept, new_offsets, new_index,
                       new_points);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_voxel_grid(int B, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets, const int* status,
                          void* workspace, int* cells, int* out_offsets, double* centroid, int* count, int* lowest, long long* cell_key,
                          void* stream) {
    if (B < 1 || !sorted_points || !sorted_keys || !order || !offsets || !status || !workspace || !cells || !out_offsets || !centroid || !count ||
        !lowest || !cell_key)
        return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    int* part = (int*)workspace;
    const dim3 grid(CLOUD_SCAN_GROUPS, B);
    hipLaunchKernelGGL(cloud_voxel_kernel<0>, grid, dim3(CLOUD_SCAN_THREADS), 0, st, B, sorted_points, sorted_keys, order, offsets, status, part, cells,
                       out_offsets, centroid, count, lowest, cell_key);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(cloud_voxel_kernel<1>, grid, dim3(CLOUD_SCAN_THREADS), 0, st, B, sorted_points, sorted_keys, order, offsets, status, part, cells,
                       out_offsets, centroid, count, lowest, cell_key);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
