// Single-view scans: a depth rasteriser for a ragged batch of meshes, the back-projection of depth maps into a packed point
// cloud, and a stratified pick of N points per view.  All geometry is fp64 with one rounding per operation (-ffp-contract=off, build.py), in an
// order tests/_depth_oracle.py restates in numpy, so every output is defined bit for bit:
//   camera    16 doubles per view: fx, fy, cx, cy, R (3x3 row-major), t (3); x right, y down, z forward
//   to camera p_c[k] = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k]
//   project   u = fx*(x_c/z_c) + cx, v = fy*(y_c/z_c) + cy; pixel (r, c) has its centre P = (c + 0.5, r + 0.5)
//   face      any corner with z_c < near: dropped whole (counted); a corner or a projection that is not finite: the view's status bit
//   edge      edge(P, Q, X) = (Q.u - P.u)*(X.v - P.v) - (Q.v - P.v)*(X.u - P.u); area = edge(A, B, C), area == 0: skipped
//   covered   P inside the closed box [min u, max u] x [min v, max v] of the corners (exact comparisons), and wA = edge(B, C, P), wB = edge(C, A, P),
//             wC = edge(A, B, P) all >= 0 or all <= 0.  In exact arithmetic the edge test implies the box test; stating it makes the candidate range
//             below a superset of the covered pixels under rounding too, so the result does not depend on that range.
//   depth     qA = (wA/area)/z_A, qB, qC alike; s = (qA + qB) + qC; z = 1/s; a fragment needs 0 < z < inf
//   bary      (qA*z, qB*z, qC*z) of the winning face (perspective-corrected), 0 on a miss
//   winner    the smallest z, on equal z the lowest face index (local to its mesh)
//   unproject valid: near < z < far (so finite); p_c = (((c + 0.5) - cx)/fx*z, ((r + 0.5) - cy)/fy*z, z); d = p_c - t;
//             world[k] = (R[0][k]*d0 + R[1][k]*d1) + R[2][k]*d2; valid pixels keep their row-major order
//   pick      stratum j = the cloud rows [a_j, b_j) with a_j = floor(j*n/N), b_j = floor((j + 1)*n/N) in 64-bit integers (b_{N-1} = n); with
//             w = b_j - a_j and u_j = mesh_sample.hip's u_f of sample j under the view's key, rank = a_j + min(w - 1, floor(u_j*w)), and
//             rank = a_j for an empty stratum (n < N).  Strata are disjoint, so with n >= N no row is picked twice.  The point is the
//             cloud's row `rank` (minus the view's centre when one is given), the fp32 output its round-to-nearest
// Rendering: z is folded into the depth output itself with a 64-bit integer atomic min (positive doubles order as their bit patterns), then every
// candidate whose recomputed z equals the stored minimum folds its face index with a 32-bit atomic min, then a resolve pass writes the misses and
// the barycentrics.  Integer min does not depend on the order of arrival and no floating-point value is ever summed atomically, so the outputs are
// reproducible.  Faces whose candidate box holds more than DR_LARGE pixels are listed by the first pass and spread over workgroups in a launch
// of their own (both passes), so a ground plane or a close-up does not serialise one thread.
#include "common.h"
#include "etch_hip.h"

#define DR_BLOCK 256
#define DR_LARGE 256                     // candidate pixels above which a face goes to the large-face launch
#define DR_SPLIT 8                       // workgroups that share one large face
#define DR_LARGE_BLOCKS 256              // workgroups per view of the large-face launch
#define DR_INF_BITS 0x7FF0000000000000ull
#define DR_NO_FACE 0x7FFFFFFF
#define DR_DBL_MAX 1.7976931348623157e308

struct DrCam {
    double fx, fy, cx, cy, R[9], t[3];
};

__device__ __forceinline__ DrCam dr_camera(const double* __restrict__ cams, int v) {
    DrCam c;
    const double* p = cams + (size_t)v * 16;
    c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3];
    for (int i = 0; i < 9; ++i) c.R[i] = p[4 + i];
    for (int i = 0; i < 3; ++i) c.t[i] = p[13 + i];
    return c;
}

__device__ __forceinline__ bool dr_finite(double x) { return fabs(x) <= DR_DBL_MAX; }
__device__ __forceinline__ int dr_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

struct DrFace {
    double u[3], v[3], z[3], area, ulo, uhi, vlo, vhi;
    int c0, c1, r0, r1;                  // the candidate pixel range (inclusive), clamped into the image
    int state;                           // 0 = to rasterise, 1 = nothing to do, 2 = dropped at the near plane, 3 = not finite
};

__device__ __forceinline__ double dr_edge(double pu, double pv, double qu, double qv, double xu, double xv) {
    return (qu - pu) * (xv - pv) - (qv - pv) * (xu - pu);
}

// Face f (local) of a mesh with nv > 0 vertices from row v0row, as view `cam` sees it.
__device__ __forceinline__ DrFace dr_setup(const double* __restrict__ verts, const int* __restrict__ faces, int frow, int v0row, int nv, const DrCam& cam,
                                           double near, int H, int W) {
    DrFace f;
    f.state = 1;
    f.c0 = f.r0 = 0;
    f.c1 = f.r1 = -1;
    f.area = 0.0;
    bool finite = true, behind = false;
    for (int k = 0; k < 3; ++k) {
        const size_t row = (size_t)(v0row + dr_clamp(faces[(size_t)frow * 3 + k], nv)) * 3;
        const double x = verts[row], y = verts[row + 1], z = verts[row + 2];
        finite = finite && dr_finite(x) && dr_finite(y) && dr_finite(z);
        const double xc = ((cam.R[0] * x + cam.R[1] * y) + cam.R[2] * z) + cam.t[0];
        const double yc = ((cam.R[3] * x + cam.R[4] * y) + cam.R[5] * z) + cam.t[1];
        const double zc = ((cam.R[6] * x + cam.R[7] * y) + cam.R[8] * z) + cam.t[2];
        finite = finite && dr_finite(xc) && dr_finite(yc) && dr_finite(zc);
        behind = behind || zc < near;
        f.z[k] = zc;
        f.u[k] = cam.fx * (xc / zc) + cam.cx;
        f.v[k] = cam.fy * (yc / zc) + cam.cy;
    }
    if (!finite) {
        f.state = 3;
        return f;
    }
    if (behind) {
        f.state = 2;
        return f;
    }
    if (!(dr_finite(f.u[0]) && dr_finite(f.u[1]) && dr_finite(f.u[2]) && dr_finite(f.v[0]) && dr_finite(f.v[1]) && dr_finite(f.v[2]))) {
        f.state = 3;
        return f;
    }
    f.area = dr_edge(f.u[0], f.v[0], f.u[1], f.v[1], f.u[2], f.v[2]);
    if (f.area == 0.0 || !dr_finite(f.area)) return f;
    f.ulo = fmin(f.u[0], fmin(f.u[1], f.u[2]));
    f.uhi = fmax(f.u[0], fmax(f.u[1], f.u[2]));
    f.vlo = fmin(f.v[0], fmin(f.v[1], f.v[2]));
    f.vhi = fmax(f.v[0], fmax(f.v[1], f.v[2]));
    // floor(lo) - 1 + 0.5 < lo and ceil(hi) + 0.5 > hi: every pixel centre inside the closed box lies in the range, whatever the rounding
    const double c0 = floor(f.ulo) - 1.0, c1 = ceil(f.uhi), r0 = floor(f.vlo) - 1.0, r1 = ceil(f.vhi);
    if (c1 < 0.0 || r1 < 0.0 || c0 > (double)(W - 1) || r0 > (double)(H - 1)) return f;
    f.c0 = (int)fmax(c0, 0.0);
    f.c1 = (int)fmin(c1, (double)(W - 1));
    f.r0 = (int)fmax(r0, 0.0);
    f.r1 = (int)fmin(r1, (double)(H - 1));
    f.state = 0;
    return f;
}

__device__ __forceinline__ long long dr_box(const DrFace& f) { return (long long)(f.c1 - f.c0 + 1) * (long long)(f.r1 - f.r0 + 1); }

// The fragment of face f at pixel (r, c): false where the pixel is not covered or z is not a positive finite number.
__device__ __forceinline__ bool dr_fragment(const DrFace& f, int r, int c, double& z, double q[3]) {
    const double pu = (double)c + 0.5, pv = (double)r + 0.5;
    if (!(pu >= f.ulo && pu <= f.uhi && pv >= f.vlo && pv <= f.vhi)) return false;
    const double wA = dr_edge(f.u[1], f.v[1], f.u[2], f.v[2], pu, pv);
    const double wB = dr_edge(f.u[2], f.v[2], f.u[0], f.v[0], pu, pv);
    const double wC = dr_edge(f.u[0], f.v[0], f.u[1], f.v[1], pu, pv);
    if (!((wA >= 0.0 && wB >= 0.0 && wC >= 0.0) || (wA <= 0.0 && wB <= 0.0 && wC <= 0.0))) return false;
    q[0] = (wA / f.area) / f.z[0];
    q[1] = (wB / f.area) / f.z[1];
    q[2] = (wC / f.area) / f.z[2];
    const double s = (q[0] + q[1]) + q[2];
    z = 1.0 / s;
    return z > 0.0 && z <= DR_DBL_MAX;
}

// PASS 1: z into the depth word.  PASS 2: the face index where z equals the final depth word.
template <int PASS>
__device__ __forceinline__ void dr_fold(const DrFace& f, int face, int r, int c, int W, unsigned long long* __restrict__ zword, int* __restrict__ fword) {
    double z, q[3];
    if (!dr_fragment(f, r, c, z, q)) return;
    const size_t p = (size_t)r * W + c;
    const unsigned long long zb = (unsigned long long)__double_as_longlong(z);
    if (PASS == 1) {
        if (zb < zword[p]) atomicMin(&zword[p], zb);             // the word only falls: a stale read skips nothing that could win
    } else {
        if (zb == zword[p] && face < fword[p]) atomicMin(&fword[p], face);
    }
}

struct DrView {
    int f0, F, v0row, nv;
    bool ok;
};

__device__ __forceinline__ DrView dr_view(int B, const int* __restrict__ vert_offsets, const int* __restrict__ face_offsets, const int* __restrict__ view_mesh,
                                          int v) {
    DrView d;
    const int m = view_mesh[v];
    d.ok = m >= 0 && m < B;
    d.f0 = d.F = d.v0row = d.nv = 0;
    if (d.ok) {
        d.f0 = face_offsets[m];
        d.F = face_offsets[m + 1] - d.f0;
        d.v0row = vert_offsets[m];
        d.nv = vert_offsets[m + 1] - d.v0row;
        d.ok = d.nv > 0;
    }
    return d;
}

__global__ void __launch_bounds__(DR_BLOCK) dr_init_kernel(size_t pixels, int NV, unsigned long long* __restrict__ zword, int* __restrict__ fword,
                                                         int* __restrict__ dropped, int* __restrict__ status, int* __restrict__ n_large) {
    const size_t i = (size_t)blockIdx.x * DR_BLOCK + threadIdx.x;
    if (i < pixels) {
        zword[i] = DR_INF_BITS;
        fword[i] = DR_NO_FACE;
    }
    if (i < (size_t)NV) {
        dropped[i] = 0;
        status[i] = 0;
        n_large[i] = 0;
    }
}

// One thread per face and view.  Large faces are listed (pass 1) and left to dr_large_kernel.
template <int PASS>
__global__ void __launch_bounds__(DR_BLOCK) dr_small_kernel(int B, int H, int W, int max_faces, const double* __restrict__ verts, const int* __restrict__ faces,
                                                          const int* __restrict__ vert_offsets, const int* __restrict__ face_offsets,
                                                          const int* __restrict__ view_mesh, const double* __restrict__ cams, double near,
                                                          unsigned long long* __restrict__ zword, int* __restrict__ fword, int* __restrict__ dropped,
                                                          int* __restrict__ status, int* __restrict__ n_large, int* __restrict__ large_list) {
    const int v = blockIdx.y;
    const int face = blockIdx.x * DR_BLOCK + threadIdx.x;
    const DrView d = dr_view(B, vert_offsets, face_offsets, view_mesh, v);
    if (!d.ok) {
        if (PASS == 1 && face == 0) atomicOr(&status[v], ETCH_DEPTH_STATUS_MESH);
        return;
    }
    if (face >= d.F) return;
    const DrCam cam = dr_camera(cams, v);
    const DrFace f = dr_setup(verts, faces, d.f0 + face, d.v0row, d.nv, cam, near, H, W);
    if (PASS == 1 && f.state == 2) atomicAdd(&dropped[v], 1);
    if (PASS == 1 && f.state == 3) atomicOr(&status[v], ETCH_DEPTH_STATUS_VERTEX);
    if (f.state != 0) return;
    if (dr_box(f) > DR_LARGE) {
        if (PASS == 1) {
            const int slot = atomicAdd(&n_large[v], 1);          // slot < F <= max_faces; the list's order does not reach the result
            large_list[(size_t)v * max_faces + slot] = face;
        }
        return;
    }
    const size_t base = (size_t)v * H * W;
    for (int r = f.r0; r <= f.r1; ++r)
        for (int c = f.c0; c <= f.c1; ++c) dr_fold<PASS>(f, face, r, c, W, zword + base, fword + base);
}

// DR_SPLIT workgroups per listed face, one candidate pixel per thread and step.
template <int PASS>
__global__ void __launch_bounds__(DR_BLOCK) dr_large_kernel(int B, int H, int W, int max_faces, const double* __restrict__ verts, const int* __restrict__ faces,
                                                          const int* __restrict__ vert_offsets, const int* __restrict__ face_offsets,
                                                          const int* __restrict__ view_mesh, const double* __restrict__ cams, double near,
                                                          unsigned long long* __restrict__ zword, int* __restrict__ fword, const int* __restrict__ n_large,
                                                          const int* __restrict__ large_list) {
    const int v = blockIdx.y;
    const DrView d = dr_view(B, vert_offsets, face_offsets, view_mesh, v);
    if (!d.ok) return;
    const int count = min(n_large[v], min(d.F, max_faces));
    const long long items = (long long)count * DR_SPLIT;
    const DrCam cam = dr_camera(cams, v);
    const size_t base = (size_t)v * H * W;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int face = large_list[(size_t)v * max_faces + (size_t)(it / DR_SPLIT)];
        const int part = (int)(it % DR_SPLIT);
        if (face < 0 || face >= d.F) continue;
        const DrFace f = dr_setup(verts, faces, d.f0 + face, d.v0row, d.nv, cam, near, H, W);
        if (f.state != 0) continue;
        const int bw = f.c1 - f.c0 + 1;
        const long long n = dr_box(f);
        for (long long p = (long long)part * DR_BLOCK + threadIdx.x; p < n; p += (long long)DR_SPLIT * DR_BLOCK)
            dr_fold<PASS>(f, face, f.r0 + (int)(p / bw), f.c0 + (int)(p % bw), W, zword + base, fword + base);
    }
}

__global__ void __launch_bounds__(DR_BLOCK) dr_resolve_kernel(int B, int H, int W, const double* __restrict__ verts, const int* __restrict__ faces,
                                                            const int* __restrict__ vert_offsets, const int* __restrict__ face_offsets,
                                                            const int* __restrict__ view_mesh, const double* __restrict__ cams, double near,
                                                            int* __restrict__ fword, double* __restrict__ bary, const int* __restrict__ large_count,
                                                            int* __restrict__ n_large) {
    const int v = blockIdx.y;
    const int p = blockIdx.x * DR_BLOCK + threadIdx.x;
    if (p == 0 && n_large) n_large[v] = large_count[v];
    if (p >= H * W) return;
    const size_t o = (size_t)v * H * W + p;
    const int face = fword[o];
    double b[3] = {0.0, 0.0, 0.0};
    const DrView d = dr_view(B, vert_offsets, face_offsets, view_mesh, v);
    if (face == DR_NO_FACE || !d.ok || face < 0 || face >= d.F) {
        fword[o] = -1;
    } else if (bary) {
        const DrCam cam = dr_camera(cams, v);
        const DrFace f = dr_setup(verts, faces, d.f0 + face, d.v0row, d.nv, cam, near, H, W);
        double z, q[3];
        if (f.state == 0 && dr_fragment(f, p / W, p % W, z, q))
            for (int k = 0; k < 3; ++k) b[k] = q[k] * z;
    }
    if (bary)
        for (int k = 0; k < 3; ++k) bary[o * 3 + k] = b[k];
}

// ---- back-projection: count per 256-pixel tile, one exclusive scan over every tile of every view, then the ordered write ----------------------

__device__ __forceinline__ bool dc_valid(double z, double near, double far) { return z > near && z < far; }

__global__ void __launch_bounds__(DR_BLOCK) dc_count_kernel(int HW, int tiles, const double* __restrict__ depth, double near, double far, int* __restrict__ tile_count) {
    const int v = blockIdx.y;
    const int p = blockIdx.x * DR_BLOCK + threadIdx.x;
    const int ok = p < HW && dc_valid(depth[(size_t)v * HW + p], near, far);
    const int n = __syncthreads_count(ok);
    if (threadIdx.x == 0) tile_count[(size_t)v * tiles + blockIdx.x] = n;
}

// One workgroup: tile_count (NV * tiles) -> its exclusive prefix in place, count (NV), offsets (NV + 1).  Integer sums: no order to define.
__global__ void __launch_bounds__(DR_BLOCK) dc_scan_kernel(int NV, int tiles, int* __restrict__ tile_count, int* __restrict__ count, int* __restrict__ offsets) {
    __shared__ int s_part[DR_BLOCK];
    const long long total = (long long)NV * tiles;
    const long long per = (total + DR_BLOCK - 1) / DR_BLOCK;
    const long long a = min(total, per * threadIdx.x), b = min(total, a + per);
    int sum = 0;
    for (long long i = a; i < b; ++i) sum += tile_count[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < DR_BLOCK; ++i) {
            const int x = s_part[i];
            s_part[i] = run;
            run += x;
        }
        offsets[NV] = run;
    }
    __syncthreads();
    int run = s_part[threadIdx.x];
    for (long long i = a; i < b; ++i) {
        const int x = tile_count[i];
        tile_count[i] = run;
        if (i % tiles == 0) offsets[i / tiles] = run;
        run += x;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < NV; v += DR_BLOCK) count[v] = offsets[v + 1] - offsets[v];
}

__global__ void __launch_bounds__(DR_BLOCK) dc_write_kernel(int HW, int W, int tiles, const double* __restrict__ depth, const double* __restrict__ cams, double near,
                                                          double far, const int* __restrict__ tile_count, int* __restrict__ index, double* __restrict__ points) {
    __shared__ int s_wave[DR_BLOCK / ETCH_WAVE];
    const int v = blockIdx.y;
    const int p = blockIdx.x * DR_BLOCK + threadIdx.x;
    const double z = p < HW ? depth[(size_t)v * HW + p] : 0.0;
    const bool ok = p < HW && dc_valid(z, near, far);
    const unsigned long long mask = __ballot(ok);
    const int lane = threadIdx.x % ETCH_WAVE, w = threadIdx.x / ETCH_WAVE;
    if (lane == 0) s_wave[w] = __popcll(mask);
    __syncthreads();
    if (!ok) return;
    int rank = tile_count[(size_t)v * tiles + blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) rank += s_wave[i];
    const DrCam cam = dr_camera(cams, v);
    const int r = p / W, c = p % W;
    const double pc[3] = {(((double)c + 0.5) - cam.cx) / cam.fx * z, (((double)r + 0.5) - cam.cy) / cam.fy * z, z};
    const double d0 = pc[0] - cam.t[0], d1 = pc[1] - cam.t[1], d2 = pc[2] - cam.t[2];
    index[rank] = p;
    for (int k = 0; k < 3; ++k) points[(size_t)rank * 3 + k] = (cam.R[k] * d0 + cam.R[3 + k] * d1) + cam.R[6 + k] * d2;
}

// ---- the stratified pick ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void dp_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
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

__global__ void __launch_bounds__(DR_BLOCK) dp_pick_kernel(int N, const int* __restrict__ offsets, const int* __restrict__ index, const double* __restrict__ points,
                                                         const unsigned long long* __restrict__ keys, const double* __restrict__ center, double* __restrict__ out64,
                                                         float* __restrict__ out32,
                                                         int* __restrict__ pixel, int* __restrict__ status) {
    const int v = blockIdx.y;
    const int j = blockIdx.x * DR_BLOCK + threadIdx.x;
    const int o0 = offsets[v], n = offsets[v + 1] - o0;
    if (j == 0) status[v] = n > 0 ? 0 : ETCH_DEPTH_STATUS_EMPTY;
    if (j >= N || n <= 0) return;                                 // an empty view gets no points and never divides
    const unsigned long long key = keys[v];
    unsigned r[4];
    dp_philox4x32_10((unsigned)j, 0u, 0u, 0u, (unsigned)key, (unsigned)(key >> 32), r);
    const double u = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * 1.1102230246251565e-16;      // 2^26, 2^-53
    const long long a = (long long)j * n / N, w = (long long)(j + 1) * n / N - a;      // a <= (N - 1) n / N < n, a + w <= n
    const long long x = w > 0 ? (long long)floor(u * (double)w) : 0;
    const int rank = (int)(a + (x < w - 1 ? x : (w > 0 ? w - 1 : 0)));
    const size_t o = (size_t)v * N + j;
    pixel[o] = index[o0 + rank];
    for (int k = 0; k < 3; ++k) {
        double p = points[(size_t)(o0 + rank) * 3 + k];
        if (center) p = p - center[(size_t)v * 3 + k];
        out64[o * 3 + k] = p;
        out32[o * 3 + k] = (float)p;
    }
}

extern "C" {

int etch_render_depth_workspace(int NV, int max_faces, long long* bytes) {
    if (NV < 0 || max_faces < 0 || !bytes) return ETCH_EINVAL;
    *bytes = ((long long)NV * max_faces + NV) * (long long)sizeof(int);       // the large-face lists, then their lengths
    return ETCH_OK;
}

int etch_render_depth(int B, int NV, int H, int W, int max_faces, const double* verts, const int* faces, const int* vert_offsets, const int* face_offsets,
                      const int* view_mesh, const double* cams, double near, void* workspace, double* depth, int* face, double* bary, int* dropped,
                      int* status, int* n_large, void* stream) {
    if (B < 0 || NV < 0 || H < 0 || W < 0 || max_faces < 0 || !(near > 0.0) || !(near <= DR_DBL_MAX)) return ETCH_EINVAL;
    if (NV == 0) return ETCH_OK;
    if (NV > 65535 || (long long)NV * H * W > 0x7FFFFFFFll - DR_BLOCK || max_faces > 0x7FFFFFFF - DR_BLOCK) return ETCH_EUNSUPPORTED;      // views ride on gridDim.y
    if (B == 0 || !verts || !faces || !vert_offsets || !face_offsets || !view_mesh || !cams || !workspace || !dropped || !status) return ETCH_EINVAL;
    if ((long long)H * W > 0 && (!depth || !face)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* large_list = (int*)workspace;
    int* large_count = large_list + (size_t)NV * max_faces;
    unsigned long long* zword = (unsigned long long*)depth;      // the depth output is the z word: +inf is the largest pattern a fragment can hold
    const size_t pixels = (size_t)NV * H * W;
    const size_t init = pixels > (size_t)NV ? pixels : (size_t)NV;
    hipLaunchKernelGGL(dr_init_kernel, dim3((unsigned)((init + DR_BLOCK - 1) / DR_BLOCK)), dim3(DR_BLOCK), 0, st, pixels, NV, zword, face, dropped, status, large_count);
    const dim3 gs((max_faces + DR_BLOCK - 1) / DR_BLOCK, NV), gl(DR_LARGE_BLOCKS, NV);
    if (max_faces > 0 && pixels > 0) {
        hipLaunchKernelGGL(dr_small_kernel<1>, gs, dim3(DR_BLOCK), 0, st, B, H, W, max_faces, verts, faces, vert_offsets, face_offsets, view_mesh, cams, near, zword,
                           face, dropped, status, large_count, large_list);
        hipLaunchKernelGGL(dr_large_kernel<1>, gl, dim3(DR_BLOCK), 0, st, B, H, W, max_faces, verts, faces, vert_offsets, face_offsets, view_mesh, cams, near, zword,
                           face, large_count, large_list);
        hipLaunchKernelGGL(dr_small_kernel<2>, gs, dim3(DR_BLOCK), 0, st, B, H, W, max_faces, verts, faces, vert_offsets, face_offsets, view_mesh, cams, near, zword,
                           face, dropped, status, large_count, large_list);
        hipLaunchKernelGGL(dr_large_kernel<2>, gl, dim3(DR_BLOCK), 0, st, B, H, W, max_faces, verts, faces, vert_offsets, face_offsets, view_mesh, cams, near, zword,
                           face, large_count, large_list);
    }
    if (pixels > 0)
        hipLaunchKernelGGL(dr_resolve_kernel, dim3((H * W + DR_BLOCK - 1) / DR_BLOCK, NV), dim3(DR_BLOCK), 0, st, B, H, W, verts, faces, vert_offsets, face_offsets,
                           view_mesh, cams, near, face, bary, large_count, n_large);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_depth_large_threshold(void) { return DR_LARGE; }

int etch_depth_compact_workspace(int NV, int H, int W, long long* bytes) {
    if (NV < 0 || H < 0 || W < 0 || !bytes || (long long)NV * H * W > 0x7FFFFFFFll - DR_BLOCK) return ETCH_EINVAL;
    const long long tiles = ((long long)H * W + DR_BLOCK - 1) / DR_BLOCK;
    *bytes = (long long)NV * tiles * (long long)sizeof(int);
    return ETCH_OK;
}

int etch_depth_compact(int NV, int H, int W, const double* depth, const double* cams, double near, double far, void* workspace, int* count, int* offsets,
                       int* index, double* points, void* stream) {
    if (NV < 0 || H < 0 || W < 0 || !(near >= 0.0) || !(far > near)) return ETCH_EINVAL;
    if (NV > 65535 || (long long)NV * H * W > 0x7FFFFFFFll - DR_BLOCK) return ETCH_EUNSUPPORTED;
    if (!offsets || (NV > 0 && (!count || !cams || !workspace))) return ETCH_EINVAL;
    const int HW = H * W;
    if (NV > 0 && HW > 0 && (!depth || !index || !points)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (HW + DR_BLOCK - 1) / DR_BLOCK;
    int* tile_count = (int*)workspace;
    if (NV > 0 && tiles > 0) hipLaunchKernelGGL(dc_count_kernel, dim3(tiles, NV), dim3(DR_BLOCK), 0, st, HW, tiles, depth, near, far, tile_count);
    if (tiles > 0 || NV == 0) {
        hipLaunchKernelGGL(dc_scan_kernel, dim3(1), dim3(DR_BLOCK), 0, st, NV, tiles > 0 ? tiles : 1, tile_count, count, offsets);
    } else {
        const hipError_t e = hipMemsetAsync(offsets, 0, (size_t)(NV + 1) * sizeof(int), st);
        if (e != hipSuccess) return (int)e;
        const hipError_t e2 = hipMemsetAsync(count, 0, (size_t)NV * sizeof(int), st);
        if (e2 != hipSuccess) return (int)e2;
    }
    if (NV > 0 && tiles > 0)
        hipLaunchKernelGGL(dc_write_kernel, dim3(tiles, NV), dim3(DR_BLOCK), 0, st, HW, W, tiles, depth, cams, near, far, tile_count, index, points);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_depth_pick(int NV, int N, const int* offsets, const int* index, const double* points, const unsigned long long* keys, const double* center, double* out64,
                    float* out32, int* pixel, int* status, void* stream) {
    if (NV < 0 || N < 0) return ETCH_EINVAL;
    if (NV == 0) return ETCH_OK;
    if (NV > 65535) return ETCH_EUNSUPPORTED;
    if (!offsets || !index || !points || !keys || !status || (N > 0 && (!out64 || !out32 || !pixel))) return ETCH_EINVAL;
    const int blocks = N > 0 ? (N + DR_BLOCK - 1) / DR_BLOCK : 1;
    hipLaunchKernelGGL(dp_pick_kernel, dim3(blocks, NV), dim3(DR_BLOCK), 0, (hipStream_t)stream, N, offsets, index, points, keys, center, out64, out32, pixel,
                       status);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
