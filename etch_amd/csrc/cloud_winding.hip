// Inside and outside of an oriented point cloud on gfx950: the winding number of Barill et al. (2018), the dipole sum over
// rows that carry a position, an oriented normal and an area, and with it the containment term of DESIGN 18 against a cloud instead of a mesh.
//
//   etch_cloud_knn_kth                        d2 to the ke-th nearest other row of its cloud, on the cell grid: what the area of a row is made of
//   etch_cloud_surface_pack                   (points, normals, flags, d2k) fp64 -> pos, moment, cap fp32: the rows the sweep reads
//   etch_cloud_winding_number                 w, the nearest row and its d2 of every query against every row, one pass
//   etch_cloud_containment_energy_grad        sum_v o_v d2_v, sum_v o_v and the gradient of the containment term, the target a row
//   etch_smpl_surface_refine_contain_cloud    etch_smpl_surface_refine_contain's schedule against a cloud
//
// The scalar arithmetic is cloud_winding_solve.h's.  Determinism: no atomics at all.  A thread of the sweep adds its chunk's terms in ascending row
// order in fp32 and keeps the least (d2, row) of the chunk; it writes one partial and one key per (query, chunk); the final kernel adds the chunks in
// ascending order in fp64 and merges the keys.  The TU is built with -ffp-contract=off: every expression is evaluated as written, one rounding per
// operation, and the pair term has only +, -, x, /, sqrt and a comparison, all correctly rounded in fp32: tests/_cloud_winding_oracle.py restates
// it with numpy and the results are compared by bits.
//
// The grid search is cloud_normals.hip's (section 24), the three ct_* kernels are containment.hip's (section 18), restated here: the files that
// hold the originals keep their program text.
#include "common.h"
#include "etch_hip.h"
#include "surface_common.h"
#include "cloud_grid.h"
#include "cloud_winding_solve.h"
#include <cmath>

#define CLOUD_MAX_RINGS ETCH_CLOUD_MAX_RINGS
#define KTH_THREADS 256                           // k x 256 doubles of LDS: 64 KiB at k = 32
#define WIND_SLOTS 2                              // float4 per staged row: (pos, cap), (moment, 0)

static_assert(PM_BLOCK == PM_TILE, "one thread stages one row of a tile");
static_assert((size_t)ETCH_CLOUD_MAX_K * KTH_THREADS * sizeof(double) <= 65536, "the lists of a workgroup fit 64 KiB");

namespace {

// ---------------------------------------------------------------------------------------------- d2 to the ke-th neighbour
// The ke-th least d2 among the other rows of the cloud.  The neighbourhood of section 24 is the ke least (d2, row) PAIRS; whichever rows a tie in
// d2 goes to, the ke-th VALUE is the same, so the list holds d2 alone (cloud_filter.hip's form of the search): best[slot][thread] in LDS, sorted
// ascending by insertion, rings rho = 0 .. CLOUD_MAX_RINGS with the stop rule kth <= (rho h (1 - 2^-20))^2, then the whole-cloud scan.
__global__ __launch_bounds__(KTH_THREADS) void cloud_kth_kernel(int B, int M, int k, int brute, const double* __restrict__ P,
                                                                const long long* __restrict__ keys, const int* __restrict__ order,
                                                                const int* __restrict__ offsets, const double* __restrict__ grid,
                                                                const int* __restrict__ status, double* __restrict__ d2k) {
    extern __shared__ double best[];                  // [k][KTH_THREADS]
    const int tid = threadIdx.x;
    const int t = blockIdx.x * KTH_THREADS + tid;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const int row = brute ? t : order[t];
    const int ke = k < hi - lo - 1 ? k : hi - lo - 1;
    if (ke <= 0) {
        d2k[row] = 0.0;
        return;
    }
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    double kth = INFINITY;
    for (int j = 0; j < ke; ++j) best[j * KTH_THREADS + tid] = INFINITY;
    auto visit = [&](int j) {
        if (j == t) return;
        const double d = cloud_d2(px, py, pz, P + 3 * (size_t)j);
        if (d < kth) {
            int s = ke - 1;
            while (s > 0) {
                const double up = best[(s - 1) * KTH_THREADS + tid];
                if (!(up > d)) break;
                best[s * KTH_THREADS + tid] = up;
                --s;
            }
            best[s * KTH_THREADS + tid] = d;
            kth = best[(ke - 1) * KTH_THREADS + tid];
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
            for (int j = 0; j < ke; ++j) best[j * KTH_THREADS + tid] = INFINITY;
            kth = INFINITY;
        }
    }
    if (!done)
        for (int j = lo; j < hi; ++j) visit(j);
    d2k[row] = kth;
}

// ---------------------------------------------------------------------------------------------- pack
__global__ __launch_bounds__(256) void cloud_pack_kernel(int B, int M, int k, const double* __restrict__ points, const double* __restrict__ normal,
                                                         const int* __restrict__ flag, const double* __restrict__ d2k, const int* __restrict__ offsets,
                                                         const double* __restrict__ center, float* __restrict__ pos, float* __restrict__ moment,
                                                         float* __restrict__ cap) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    const int n = offsets[b + 1] - offsets[b];
    const int ke = k < n - 1 ? k : n - 1;
    const double p[3] = {points[3 * (size_t)t], points[3 * (size_t)t + 1], points[3 * (size_t)t + 2]};
    const double nr[3] = {normal[3 * (size_t)t], normal[3 * (size_t)t + 1], normal[3 * (size_t)t + 2]};
    const double c[3] = {center ? center[3 * b] : 0.0, center ? center[3 * b + 1] : 0.0, center ? center[3 * b + 2] : 0.0};
    const double a = wind_area(d2k[t], ke, flag[t], p[0], p[1], p[2]);
    float q[3], m[3], cp;
    wind_pack(p, c, nr, a, q, m, cp);
#pragma unroll
    for (int u = 0; u < 3; ++u) pos[3 * (size_t)t + u] = q[u], moment[3 * (size_t)t + u] = m[u];
    cap[t] = cp;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the sweep
// wn_tile_kernel's shape (containment.hip): one workgroup per (cloud, 512 queries, 1024-row chunk), 256 threads, two queries per thread in
// registers, 256-row tiles of the seven floats per row in LDS, padded to two float4 and read as wave-uniform 128-bit broadcasts.  Blocks past a
// cloud's rows or q_len return at once: the grid is sized by the maxima and nothing is read on the host.  Ascending rows with a strict < keep the
// lowest row of a tie in d2; a NaN d2 fails the <, and so does +inf against the start value.
struct WindCloud {
    const float *pos, *moment, *cap;
    const int* offsets;
    __device__ __forceinline__ int n(int b) const { return max(offsets[b + 1] - offsets[b], 0); }
};

static inline int wind_chunks(int max_rows) { return (max_rows + PM_CHUNK - 1) / PM_CHUNK; }

static __global__ void __launch_bounds__(PM_BLOCK) cw_tile_kernel(int Q, WindCloud cloud, const float* __restrict__ qs, const int* __restrict__ qlen,
                                                                  float* __restrict__ partial, u64* __restrict__ keys) {
    __shared__ float4 tile[WIND_SLOTS][PM_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int n = clamp_len(qlen, b, Q);
    const int r0 = blockIdx.y * PM_ROWS;
    if (r0 >= n) return;                              // uniform: padding is never read
    const int R = cloud.n(b);
    const int f0 = blockIdx.x * PM_CHUNK, f1 = min(R, f0 + PM_CHUNK);
    if (f0 >= R) return;                              // uniform: the final kernel reads the chunks below ceil(R_b / 1024) only
    const size_t base_row = (size_t)cloud.offsets[b];
    const float* Qb = qs + (size_t)b * Q * 3;
    float p[PM_R][3], acc[PM_R], bd[PM_R];
    int bi[PM_R];
    bool ok[PM_R];
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        ok[r] = i < n;
        for (int c = 0; c < 3; ++c) p[r][c] = ok[r] ? Qb[(size_t)i * 3 + c] : 0.f;
        acc[r] = 0.f, bd[r] = INFINITY, bi[r] = -1;
    }
    for (int t0 = f0; t0 < f1; t0 += PM_TILE) {
        const int tn = min(PM_TILE, f1 - t0);
        __syncthreads();
        if (tid < tn) {
            const size_t j = base_row + (size_t)(t0 + tid);
            tile[0][tid] = make_float4(cloud.pos[3 * j], cloud.pos[3 * j + 1], cloud.pos[3 * j + 2], cloud.cap[j]);
            tile[1][tid] = make_float4(cloud.moment[3 * j], cloud.moment[3 * j + 1], cloud.moment[3 * j + 2], 0.f);
        }
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float4 a = tile[0][k], m = tile[1][k];
            const int row = t0 + k;
#pragma unroll
            for (int r = 0; r < PM_R; ++r) {
                const float rx = a.x - p[r][0], ry = a.y - p[r][1], rz = a.z - p[r][2];
                const float d2 = wind_d2(rx, ry, rz);
                acc[r] += wind_term(rx, ry, rz, d2, m.x, m.y, m.z, a.w);
                if (d2 < bd[r]) bd[r] = d2, bi[r] = row;     // from +inf: a d2 that is NaN or +inf (a row that is not finite) never wins
            }
        }
    }
    const size_t base = ((size_t)b * gridDim.x + blockIdx.x) * Q;
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        if (ok[r]) partial[base + i] = acc[r], keys[base + i] = wind_key(bd[r], bi[r]);
    }
}

// w = (sum over the cloud's chunks, ascending, fp64) / (4 pi), rounded once to fp32; the least key of the chunks.  Padding queries: 0, -1, 0.
static __global__ void __launch_bounds__(256) cw_final_kernel(int B, int Q, int chunks, WindCloud cloud, const int* __restrict__ qlen,
                                                              const float* __restrict__ partial, const u64* __restrict__ keys, float* __restrict__ w,
                                                              int* __restrict__ nearest, float* __restrict__ nearest_d2) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * Q) return;
    const int b = (int)(t / Q), i = (int)(t % Q);
    double s = 0.0;
    u64 key = WIND_NO_KEY;
    if (i < clamp_len(qlen, b, Q)) {
        const int nc = min(chunks, (cloud.n(b) + PM_CHUNK - 1) / PM_CHUNK);
        for (int c = 0; c < nc; ++c) {
            s += (double)partial[((size_t)b * chunks + c) * Q + i];
            key = wind_merge(key, keys[((size_t)b * chunks + c) * Q + i]);
        }
    }
    w[t] = (float)(s * WIND_INV_4PI);
    int row;
    float d2;
    wind_unkey(key, row, d2);
    if (nearest) nearest[t] = row;
    if (nearest_d2) nearest_d2[t] = d2;
}

static int cw_run(int B, int Q, int max_rows, WindCloud cloud, const float* queries, const int* q_len, float* partial, u64* keys, float* w, int* nearest,
                  float* nearest_d2, hipStream_t st) {
    const int chunks = wind_chunks(max_rows);
    if (chunks > 0)
        hipLaunchKernelGGL(cw_tile_kernel, dim3(chunks, (Q + PM_ROWS - 1) / PM_ROWS, B), dim3(PM_BLOCK), 0, st, Q, cloud, queries, q_len, partial, keys);
    hipLaunchKernelGGL(cw_final_kernel, dim3(nblk((long)B * Q)), dim3(256), 0, st, B, Q, chunks, cloud, q_len, partial, keys, w, nearest, nearest_d2);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// ---------------------------------------------------------------------------------------------- the containment term
// containment.hip's three ct_* kernels with the row target: o_v = [ |w_v| < 0.5 ] (a NaN w fails the <) and the vertex has a nearest row in
// [0, n_b); c_v = pos[nearest_v] as fp64.  The target is a SAMPLE of the surface, not a point on it.
static __global__ void __launch_bounds__(256) cw_target_kernel(int B, int V, WindCloud cloud, const float* __restrict__ w, const int* __restrict__ nearest,
                                                               int* __restrict__ outside, double* __restrict__ target) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * V) return;
    const int b = (int)(t / V);
    const int r = nearest[t];
    int o = 0;
    double c[3] = {0.0, 0.0, 0.0};
    if (fabsf(w[t]) < 0.5f && r >= 0 && r < cloud.n(b)) {
        const float* pr = cloud.pos + ((size_t)cloud.offsets[b] + (size_t)r) * 3;
        o = 1;
        for (int k = 0; k < 3; ++k) c[k] = (double)pr[k];
    }
    outside[t] = o;
    for (int k = 0; k < 3; ++k) target[t * 3 + k] = c[k];
}

// One workgroup per cloud, fp64, fixed order (strided per thread, then a tree): terms[b] = {sum_v o_v d2_v, sum_v o_v}; d2 = the fp32 values
// handed in, or (d2 NULL) |v - c_v|^2 of the current vertices and the held targets in fp64.
static __global__ void __launch_bounds__(256) cw_terms_kernel(int V, const float* __restrict__ verts, const int* __restrict__ outside,
                                                              const double* __restrict__ target, const float* __restrict__ d2, double* __restrict__ terms) {
    __shared__ double sm[2][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double a[2] = {0.0, 0.0};
    for (int v = tid; v < V; v += 256) {
        const long t = (long)b * V + v;
        if (!outside[t]) continue;
        double d = 0.0;
        if (d2) d = (double)d2[t];
        else
            for (int k = 0; k < 3; ++k) {
                const double e = (double)verts[t * 3 + k] - target[t * 3 + k];
                d += e * e;
            }
        a[0] += d; a[1] += 1.0;
    }
    sm[0][tid] = a[0]; sm[1][tid] = a[1];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { sm[0][tid] += sm[0][tid + s]; sm[1][tid] += sm[1][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { terms[b * 2] = sm[0][0]; terms[b * 2 + 1] = sm[1][0]; }
}

// g_v += coef_b w_contain (2 / V) o_v (v - c_v): one term per vertex, computed in fp64 and added with one rounding; an inside vertex is not touched
static __global__ void __launch_bounds__(256) cw_apply_kernel(int B, int V, const float* __restrict__ verts, const int* __restrict__ outside,
                                                              const double* __restrict__ target, const float* __restrict__ coef, float w_contain,
                                                              float* __restrict__ g) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * V || !outside[t]) return;
    const int b = (int)(t / V);
    const double s = (coef ? (double)coef[b] : 1.0) * (double)w_contain * (2.0 / V);
    if (s == 0.0) return;                             // a zero weight leaves g's bits alone (-0 + 0 would be +0)
    for (int k = 0; k < 3; ++k) g[t * 3 + k] = (float)((double)g[t * 3 + k] + s * ((double)verts[t * 3 + k] - target[t * 3 + k]));
}

// ---------------------------------------------------------------------------------------------- host side
struct CwWork {
    float *wn, *partial, *d2;
    int *nearest, *outside;
    u64* keys;
    double *target, *terms;
    size_t bytes;
};

static CwWork cw_layout(char* base, size_t off, int B, int V, int max_rows) {
    CwWork w;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += al(n); return p; };
    w.wn = (float*)take((size_t)B * V * 4);
    w.partial = (float*)take((size_t)B * wind_chunks(max_rows) * V * 4);
    w.keys = (u64*)take((size_t)B * wind_chunks(max_rows) * V * 8);
    w.d2 = (float*)take((size_t)B * V * 4);
    w.nearest = (int*)take((size_t)B * V * 4);
    w.outside = (int*)take((size_t)B * V * 4);
    w.target = (double*)take((size_t)B * V * 24);
    w.terms = (double*)take((size_t)B * 16);
    w.bytes = off;
    return w;
}

static bool cw_cloud_ok(int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets) {
    return max_rows >= 0 && offsets && (max_rows == 0 || (pos && moment && cap));
}

extern "C" {

int etch_cloud_knn_kth(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets,
                       const double* grid, const int* status, double* d2k, void* stream) {
    if (B < 1 || M < 0 || k < 3 || k > ETCH_CLOUD_MAX_K || !sorted_points || !offsets || !status || !d2k) return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order || !grid)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    const size_t lds = (size_t)k * KTH_THREADS * sizeof(double);
    hipLaunchKernelGGL(cloud_kth_kernel, dim3((M + KTH_THREADS - 1) / KTH_THREADS), dim3(KTH_THREADS), lds, (hipStream_t)stream, B, M, k, brute,
                       sorted_points, sorted_keys, order, offsets, grid, status, d2k);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_surface_pack(int B, int M, int k, const double* points, const double* normal, const int* flag, const double* d2k, const int* offsets,
                            const double* center, float* pos, float* moment, float* cap, void* stream) {
    if (B < 1 || M < 0 || k < 3 || k > ETCH_CLOUD_MAX_K || !offsets) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    if (!points || !normal || !flag || !d2k || !pos || !moment || !cap) return ETCH_EINVAL;
    hipLaunchKernelGGL(cloud_pack_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, M, k, points, normal, flag, d2k, offsets, center,
                       pos, moment, cap);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_winding_number_workspace(int B, int Q, int max_rows, long long* bytes) {
    if (B < 0 || Q < 0 || max_rows < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)(al((size_t)B * wind_chunks(max_rows) * Q * 4) + al((size_t)B * wind_chunks(max_rows) * Q * 8));
    return ETCH_OK;
}

int etch_cloud_winding_number(int B, int Q, int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, const float* queries,
                              const int* q_len, void* workspace, float* w, int* nearest, float* nearest_d2, void* stream) {
    if (B < 0 || Q < 0) return ETCH_EINVAL;
    if (B == 0 || Q == 0) return ETCH_OK;
    if (!cw_cloud_ok(max_rows, pos, moment, cap, offsets) || !queries || !w || (max_rows > 0 && !workspace)) return ETCH_EINVAL;
    float* partial = (float*)workspace;
    u64* keys = (u64*)((char*)workspace + al((size_t)B * wind_chunks(max_rows) * Q * 4));
    return cw_run(B, Q, max_rows, WindCloud{pos, moment, cap, offsets}, queries, q_len, partial, keys, w, nearest, nearest_d2, (hipStream_t)stream);
}

int etch_cloud_containment_energy_grad_workspace(int B, int V, long long* bytes) {
    if (B < 0 || V < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)(al((size_t)B * V * 4) + al((size_t)B * V * 24));
    return ETCH_OK;
}

int etch_cloud_containment_energy_grad(int B, int V, const float* body_verts, const float* pos, const int* offsets, const float* w, const int* nearest,
                                       const float* nearest_d2, const float* coef, float w_contain, void* workspace, double* terms, float* g,
                                       void* stream) {
    if (B < 0 || V < 0 || !terms) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    if (!offsets || !workspace || (V > 0 && (!body_verts || !pos || !w || !nearest || !nearest_d2))) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* outside = (int*)workspace;
    double* target = (double*)((char*)workspace + al((size_t)B * V * 4));
    const WindCloud cloud{pos, nullptr, nullptr, offsets};
    if (V > 0) hipLaunchKernelGGL(cw_target_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, cloud, w, nearest, outside, target);
    hipLaunchKernelGGL(cw_terms_kernel, dim3(B), dim3(256), 0, st, V, body_verts, outside, target, nearest_d2, terms);
    if (g && V > 0) hipLaunchKernelGGL(cw_apply_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, body_verts, outside, target, coef, w_contain, g);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_smpl_surface_refine_contain_cloud_workspace(int B, int N, int V, int nj, int nb, int n_extra, int max_rows, long long* bytes) {
    if (B < 0 || N < 0 || V < 0 || max_rows < 0 || !bytes) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    *bytes = (long long)cw_layout(nullptr, sf_layout(nullptr, B, N, V, nj, nb, n_extra).bytes, B, V, max_rows).bytes;
    return ETCH_OK;
}

int etch_smpl_surface_refine_contain_cloud(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces,
                                           const float* points, const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers,
                                           const float* marker_valid, const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2,
                                           float eps, float w_dense, float w_marker, float w_beta, float w_prior, float trunc, int optimize_scale,
                                           int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, float w_contain,
                                           int contain_every, float* params, float* verts, float* joints, float* loss_trace, float* loss_last,
                                           void* workspace, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || F <= 0 || M < 0 || iters < 1 || n_gauss < 0 || n_gauss > SF_MAXG || contain_every < 1) return ETCH_EINVAL;
    if (M > 0 && (!marker_vids || !markers || !marker_valid)) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (n_gauss > 0 && (nj != 24 || !prior)) return ETCH_EUNSUPPORTED;      // the GMM prior is over the 69-dim SMPL body pose only
    if (B == 0) return ETCH_OK;
    if (!workspace || !params || !verts || !joints || !loss_last) return ETCH_EINVAL;
    if (!cw_cloud_ok(max_rows, pos, moment, cap, offsets)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const SfWork w = sf_layout((char*)workspace, B, N, V, nj, nb, n_extra);
    const CwWork c = cw_layout((char*)workspace, w.bytes, B, V, max_rows);
    const WindCloud cloud{pos, moment, cap, offsets};
    const int P = 3 * nj + nb + 4;
    const float* means = n_gauss ? (const float*)prior[0] : nullptr;
    const float* prec = n_gauss ? (const float*)prior[1] : nullptr;
    const float* nllw = n_gauss ? (const float*)prior[2] : nullptr;
    const PmMarkers mk{M, marker_vids, markers, marker_valid, w_marker};
    hipLaunchKernelGGL(f32_zero_kernel, dim3(nblk((long)B * P)), dim3(256), 0, st, (long)B * P, w.m);      // Adam moments start at zero
    hipLaunchKernelGGL(f32_zero_kernel, dim3(nblk((long)B * P)), dim3(256), 0, st, (long)B * P, w.v);
    double bp1 = 1.0, bp2 = 1.0;
    for (int it = 0; it < iters; ++it) {
        int e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, w.verts, nullptr, 0, st);
        if (!e) e = pm_closest(B, N, V, F, points, n_len, w.verts, faces, w.keys, w.face, w.bary, w.d2, st);
        if (!e) e = pm_energy_grad(B, N, V, F, points, n_len, w.verts, faces, w.face, w.bary, w.d2, weights, trunc, nullptr, w_dense, 1, mk, w.acc, w.macc, w.terms,
                                   w.mterms, w.gy, nullptr, st);
        if (e) return e;
        if (it % contain_every == 0) {                 // refresh: one pass gives which vertices are outside and the row each is pulled to
            e = cw_run(B, V, max_rows, cloud, w.verts, nullptr, c.partial, c.keys, c.wn, c.nearest, c.d2, st);
            if (e) return e;
            hipLaunchKernelGGL(cw_target_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, cloud, c.wn, c.nearest, c.outside, c.target);
        }
        // in between o_v and c_v are held: the term stays a fixed quadratic between two refreshes
        hipLaunchKernelGGL(cw_terms_kernel, dim3(B), dim3(256), 0, st, V, w.verts, c.outside, c.target, (const float*)nullptr, c.terms);
        hipLaunchKernelGGL(cw_apply_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, w.verts, c.outside, c.target, (const float*)nullptr, w_contain, w.gy);
        hipLaunchKernelGGL(sf_loss_kernel, dim3(B), dim3(256), 0, st, nj, nb, w.terms, w.mterms, params, means, prec, nllw, n_gauss, w_dense, w_marker, w_beta,
                           w_prior, w.grad, loss_trace, iters, it, loss_last, c.terms, w_contain, V);
        ETCH_RETURN_IF_LAUNCH_FAILED();
        e = rf_vjp(w, B, V, nj, nb, consts, params, w.gy, w.grad, st);
        if (e) return e;
        if (!optimize_scale) hipLaunchKernelGGL(sf_freeze_scale_kernel, dim3(nblk(B)), dim3(256), 0, st, B, P, w.grad);
        e = rf_adam_step(it, iters, lr, beta1, beta2, eps, bp1, bp2, (long)B * P, params, w.grad, w.m, w.v, st);
        if (e) return e;
    }
    int e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, verts, nullptr, 0, st);
    if (!e) e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, nullptr, joints, 1, st);   // joints without trans and scale, as fit_cham
    return e;
}

}  // extern "C"
