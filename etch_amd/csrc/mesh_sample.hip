// Area-weighted surface sampling of a ragged batch of meshes, and the bounding-box centre of each (inference_demo.py:19-39).  Everything is
// fp64 with one rounding per operation (-ffp-contract=off, build.py), in an order tests/_sampler_oracle.py restates in numpy, so the result is
// defined bit for bit:
//   corners   (v - c) when a centre is given
//   area      e1 = v1 - v0, e2 = v2 - v0, (cx, cy, cz) = e1 x e2, area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz)
//   cum       tiles of 64 faces in face order: c[j] = the sequential inclusive sum inside the tile, S_t = the sequential sum of the totals of the
//             tiles in front, cum[f] = S_t + c[j]
//   random    Philox4x32-10, key = (low, high) half of the scan's key, counter (i, 0, 0, 0) -> r0..r3;
//             u_f = ((r0 >> 5) * 2^26 + (r1 >> 6)) * 2^-53, u1 = (r2 + 0.5) * 2^-32, u2 = (r3 + 0.5) * 2^-32
//   face      the first f with cum[f] > u_f * cum[last], else the last face
//   point     u1 + u2 > 1 -> both 1 - u; p = (v0 + u1*e1) + u2*e2; the fp32 output is its round-to-nearest
// Three launches per call (tile sums, per-scan prefix, samples).  No floating-point atomics; each status word has one writer.
#include "common.h"
#include "etch_hip.h"

#define MS_BLOCK 256
#define MS_TILE 64                       // faces per tile = one wave
#define MS_TILES_PER_BLOCK (MS_BLOCK / MS_TILE)
#define MS_CHUNK 1024                    // tile totals the prefix kernel holds in LDS at a time

// Slot of scan b's first tile total: floor(face_offset / 64) + b >= the tiles in front, and consecutive scans' ranges do not overlap
// (the next base is at least floor(F_b / 64) + 1 >= ceil(F_b / 64) further).  The workspace has floor(total / 64) + B slots.
__device__ __forceinline__ int ms_tile_base(int face_offset, int b) { return face_offset / MS_TILE + b; }

__device__ __forceinline__ int ms_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

struct MsTri {
    double v0[3], e1[3], e2[3];
};

// Corners of face f (global row) of a scan with nv > 0 vertices starting at vertex row v0row, minus the centre.
__device__ __forceinline__ MsTri ms_triangle(const double* __restrict__ verts, const int* __restrict__ faces, int f, int v0row, int nv, const double* c) {
    MsTri t;
    const int i0 = ms_clamp(faces[(size_t)f * 3], nv), i1 = ms_clamp(faces[(size_t)f * 3 + 1], nv), i2 = ms_clamp(faces[(size_t)f * 3 + 2], nv);
    for (int k = 0; k < 3; ++k) {
        double a = verts[(size_t)(v0row + i0) * 3 + k], b = verts[(size_t)(v0row + i1) * 3 + k], d = verts[(size_t)(v0row + i2) * 3 + k];
        if (c) {
            a = a - c[k];
            b = b - c[k];
            d = d - c[k];
        }
        t.v0[k] = a;
        t.e1[k] = b - a;
        t.e2[k] = d - a;
    }
    return t;
}

// One wave per tile, one lane per face: lane j folds areas 0..j of its tile in order, which is the sequential inclusive sum c[j].
__global__ void __launch_bounds__(MS_BLOCK) ms_tile_kernel(const double* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ vert_offsets,
                                                         const int* __restrict__ face_offsets, const double* __restrict__ center, double* __restrict__ cum,
                                                         double* __restrict__ tile_total) {
    __shared__ double s_area[MS_TILES_PER_BLOCK][MS_TILE];
    const int b = blockIdx.y;
    const int f0 = face_offsets[b], F = face_offsets[b + 1] - f0;
    const int v0row = vert_offsets[b], nv = vert_offsets[b + 1] - v0row;
    const int w = threadIdx.x / MS_TILE, lane = threadIdx.x % MS_TILE;
    const int t = blockIdx.x * MS_TILES_PER_BLOCK + w;
    const int j0 = t * MS_TILE;                                  // the tile's first face in its scan; t * 64 <= max_faces + 255
    const bool live = j0 + lane < F && nv > 0;
    double area = 0.0;
    if (live) {
        const MsTri q = ms_triangle(verts, faces, f0 + j0 + lane, v0row, nv, center ? center + (size_t)b * 3 : nullptr);
        const double cx = q.e1[1] * q.e2[2] - q.e1[2] * q.e2[1];
        const double cy = q.e1[2] * q.e2[0] - q.e1[0] * q.e2[2];
        const double cz = q.e1[0] * q.e2[1] - q.e1[1] * q.e2[0];
        area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    }
    s_area[w][lane] = area;
    __syncthreads();
    if (j0 + lane < F) {
        double c = s_area[w][0];
        for (int j = 1; j <= lane; ++j) c = c + s_area[w][j];
        cum[f0 + j0 + lane] = c;
        if (lane == MS_TILE - 1 || j0 + lane == F - 1) tile_total[ms_tile_base(f0, b) + t] = c;
    }
}

// One workgroup per scan: exclusive prefix of the tile totals (thread 0, in tile order), cum[f] = S_t + c[j], and the status word.
__global__ void __launch_bounds__(MS_BLOCK) ms_prefix_kernel(const double* __restrict__ verts, const int* __restrict__ vert_offsets,
                                                           const int* __restrict__ face_offsets, double* __restrict__ cum,
                                                           const double* __restrict__ tile_total, int* __restrict__ status) {
    __shared__ double s_pre[MS_CHUNK];
    __shared__ double s_run;
    const int b = blockIdx.x;
    const int f0 = face_offsets[b], F = face_offsets[b + 1] - f0;
    const int v0row = vert_offsets[b], nv = vert_offsets[b + 1] - v0row;
    const int nt = (F + MS_TILE - 1) / MS_TILE;
    const double* tt = tile_total + ms_tile_base(f0, b);
    int bad = 0;
    for (size_t i = threadIdx.x; i < (size_t)(nv > 0 ? nv : 0) * 3; i += MS_BLOCK) {
        const double x = verts[(size_t)v0row * 3 + i];
        bad |= !(fabs(x) <= 1.7976931348623157e308);
    }
    if (threadIdx.x == 0) s_run = 0.0;
    const int any_bad = __syncthreads_or(bad);
    for (int c0 = 0; c0 < nt; c0 += MS_CHUNK) {
        const int n = min(MS_CHUNK, nt - c0);
        for (int i = threadIdx.x; i < n; i += MS_BLOCK) s_pre[i] = tt[c0 + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            double run = s_run;
            for (int i = 0; i < n; ++i) {
                const double x = s_pre[i];
                s_pre[i] = run;
                run = run + x;
            }
            s_run = run;
        }
        __syncthreads();
        const int fa = c0 * MS_TILE, fb = min(F, (c0 + n) * MS_TILE);
        for (int f = fa + threadIdx.x; f < fb; f += MS_BLOCK) cum[f0 + f] = s_pre[f / MS_TILE - c0] + cum[f0 + f];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = s_run;
        const bool ok = F > 0 && nv > 0 && total > 0.0 && total <= 1.7976931348623157e308;
        status[b] = (ok ? 0 : ETCH_SAMPLE_STATUS_AREA) | (any_bad ? ETCH_SAMPLE_STATUS_VERTEX : 0);
    }
}

__device__ __forceinline__ void ms_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
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

__global__ void __launch_bounds__(MS_BLOCK) ms_sample_kernel(int N, const double* __restrict__ verts, const int* __restrict__ faces,
                                                           const int* __restrict__ vert_offsets, const int* __restrict__ face_offsets,
                                                           const unsigned long long* __restrict__ keys, const double* __restrict__ center,
                                                           const double* __restrict__ cum, const int* __restrict__ status,
                                                           float* __restrict__ points32, double* __restrict__ points64, int* __restrict__ face) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= N || status[b] != 0) return;                       // a flagged scan (no face, no area, not finite) gets no samples
    const int f0 = face_offsets[b], F = face_offsets[b + 1] - f0;
    const int v0row = vert_offsets[b], nv = vert_offsets[b + 1] - v0row;
    const unsigned long long key = keys[b];
    unsigned r[4];
    ms_philox4x32_10((unsigned)i, 0u, 0u, 0u, (unsigned)key, (unsigned)(key >> 32), r);
    const double uf = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * 1.1102230246251565e-16;      // 2^26, 2^-53
    double u1 = ((double)r[2] + 0.5) * 2.3283064365386963e-10;                                             // 2^-32
    double u2 = ((double)r[3] + 0.5) * 2.3283064365386963e-10;
    const double* cs = cum + f0;
    const double target = uf * cs[F - 1];
    int lo = 0, hi = F;                                          // the first f in [0, F) with cs[f] > target
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cs[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    const int f = lo < F ? lo : F - 1;
    const MsTri q = ms_triangle(verts, faces, f0 + f, v0row, nv, center ? center + (size_t)b * 3 : nullptr);
    if (u1 + u2 > 1.0) {
        u1 = 1.0 - u1;
        u2 = 1.0 - u2;
    }
    const size_t o = ((size_t)b * N + i) * 3;
    for (int k = 0; k < 3; ++k) {
        const double p = (q.v0[k] + u1 * q.e1[k]) + u2 * q.e2[k];
        points32[o + k] = (float)p;
        if (points64) points64[o + k] = p;
    }
    face[(size_t)b * N + i] = f;
}

// min / max that do not depend on the order: of equal zeros the minimum is -0, the maximum +0.  A NaN never wins (the prefix kernel flags it).
__device__ __forceinline__ double ms_min(double a, double b) { return (b < a || (b == a && signbit(b))) ? b : a; }
__device__ __forceinline__ double ms_max(double a, double b) { return (b > a || (b == a && !signbit(b))) ? b : a; }

__global__ void __launch_bounds__(MS_BLOCK) ms_bbox_kernel(const double* __restrict__ verts, const int* __restrict__ vert_offsets, double* __restrict__ center) {
    __shared__ double s_lo[3][MS_BLOCK], s_hi[3][MS_BLOCK];
    const int b = blockIdx.x;
    const int v0row = vert_offsets[b], nv = vert_offsets[b + 1] - v0row;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int i = threadIdx.x; i < nv; i += MS_BLOCK)
        for (int k = 0; k < 3; ++k) {
            const double x = verts[(size_t)(v0row + i) * 3 + k];
            lo[k] = ms_min(lo[k], x);
            hi[k] = ms_max(hi[k], x);
        }
    for (int k = 0; k < 3; ++k) {
        s_lo[k][threadIdx.x] = lo[k];
        s_hi[k][threadIdx.x] = hi[k];
    }
    __syncthreads();
    for (int s = MS_BLOCK / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; ++k) {
                s_lo[k][threadIdx.x] = ms_min(s_lo[k][threadIdx.x], s_lo[k][threadIdx.x + s]);
                s_hi[k][threadIdx.x] = ms_max(s_hi[k][threadIdx.x], s_hi[k][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) center[(size_t)b * 3 + threadIdx.x] = (s_lo[threadIdx.x][0] + s_hi[threadIdx.x][0]) / 2.0;
}

extern "C" {

int etch_bbox_center(int B, const double* verts, const int* vert_offsets, double* center, void* stream) {
    if (B < 0 || (B > 0 && (!verts || !vert_offsets || !center))) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    hipLaunchKernelGGL(ms_bbox_kernel, dim3(B), dim3(MS_BLOCK), 0, (hipStream_t)stream, verts, vert_offsets, center);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_sample_surface_workspace(int B, int total_faces, long long* bytes) {
    if (B < 0 || total_faces < 0 || !bytes) return ETCH_EINVAL;
    *bytes = ((long long)total_faces + total_faces / MS_TILE + B) * (long long)sizeof(double);
    return ETCH_OK;
}

int etch_sample_surface(int B, int N, int total_faces, int max_faces, const double* verts, const int* faces, const int* vert_offsets,
                        const int* face_offsets, const unsigned long long* keys, const double* center, void* workspace, float* points32,
                        double* points64, int* face, int* status, void* stream) {
    if (B < 0 || N < 0 || total_faces < 0 || max_faces < 0 || max_faces > total_faces || total_faces > 0x7FFFFFFF - 2 * MS_BLOCK) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // scans ride on gridDim.y
    if (!verts || !faces || !vert_offsets || !face_offsets || !keys || !workspace || !status || (N > 0 && (!points32 || !face))) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* cum = (double*)workspace;                           // (total_faces), then the tile totals (total_faces / 64 + B)
    double* tile_total = cum + total_faces;
    const int tiles = (max_faces + MS_TILE - 1) / MS_TILE;
    if (tiles > 0)
        hipLaunchKernelGGL(ms_tile_kernel, dim3((tiles + MS_TILES_PER_BLOCK - 1) / MS_TILES_PER_BLOCK, B), dim3(MS_BLOCK), 0, st, verts, faces, vert_offsets,
                           face_offsets, center, cum, tile_total);
    hipLaunchKernelGGL(ms_prefix_kernel, dim3(B), dim3(MS_BLOCK), 0, st, verts, vert_offsets, face_offsets, cum, tile_total, status);
    if (N > 0)
        hipLaunchKernelGGL(ms_sample_kernel, dim3((N + MS_BLOCK - 1) / MS_BLOCK, B), dim3(MS_BLOCK), 0, st, N, verts, faces, vert_offsets, face_offsets, keys,
                           center, cum, status, points32, points64, face);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
