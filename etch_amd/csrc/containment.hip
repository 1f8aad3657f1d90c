// Containment on gfx950: keep the fitted body inside the scan it is supposed to be under.
//
//   etch_mesh_winding_number          generalised winding number of a ragged batch of scan meshes at batched, ragged query sets, fp32
//   etch_ragged_mesh_closest          etch_point_mesh_closest's contract for that ragged batch (per-scan faces)
//   etch_containment_energy_grad      sum_v o_v d2_v, sum_v o_v and the gradient of the containment term w.r.t. the body's vertices
//   etch_smpl_surface_refine_contain  etch_smpl_surface_refine's schedule with the containment term as a fifth term of the loss
//
// Determinism: no floating-point atomics.  A thread of the winding kernel adds its chunk's terms in ascending face order and writes one
// partial per (query, chunk); the final kernel adds the chunks in ascending order in fp64.  The containment gradient is one term per vertex
// (a plain read-modify-write); its sums are fp64 in a fixed order.  The closest points go through surface_common.h's kernels and keys.
// The TU is built with -ffp-contract=off: every expression below is evaluated as written, one rounding per operation.
#include "etch_hip.h"
#include "surface_common.h"

// ---------------------------------------------------------------------------------------------- winding number
// van Oosterom & Strackee (1983): the signed solid angle Omega of triangle (a, b, c) seen from q, with A = a - q, B = b - q, C = c - q:
//   la = sqrt((A.x*A.x + A.y*A.y) + A.z*A.z), lb, lc alike;          dot(X, Y) = (X.x*Y.x + X.y*Y.y) + X.z*Y.z
//   n  = B x C = (B.y*C.z - B.z*C.y, B.z*C.x - B.x*C.z, B.x*C.y - B.y*C.x);   det = dot(A, n)
//   den = (((la*lb)*lc + dot(A, B)*lc) + dot(B, C)*la) + dot(C, A)*lb
//   Omega / 2 = atan2f(det, den) + ((la + lb) + lc) * 0     (the last term is 0, or NaN where a corner or the query is not finite: an
//                                                            infinite corner alone can leave atan2f finite)
// w(q) = sum_faces Omega / (4 pi): 1 inside a closed outward-oriented surface, 0 outside, -1 inside a reversed one, smooth across holes.
// tests/_containment_oracle.py restates the order (its atan2 is numpy's, so the comparison is by the entitled-error rule, not bitwise).
//
// Tiling as pm_tile_kernel: one workgroup per (scan, 512 queries, 1024-face chunk), two queries per thread in registers, 256-face tiles of
// nine floats per face in LDS read as wave-uniform broadcasts.  Blocks past a scan's q_len or face count return at once (the grid is sized by
// the maxima: no host read).  A face with a vertex index outside [0, V_b) is staged as the triangle (0, 0, 0): B x C is then exactly 0, det
// is +-0, den = 4 |q|^3 >= 0 and atan2f(+-0, den) = +-0, which changes no sum.  A non-finite vertex or query gives NaN.
__device__ __forceinline__ float wn_half_angle(const float* q, const float* a, const float* b, const float* c) {
    const float A[3] = {a[0] - q[0], a[1] - q[1], a[2] - q[2]};
    const float B[3] = {b[0] - q[0], b[1] - q[1], b[2] - q[2]};
    const float C[3] = {c[0] - q[0], c[1] - q[1], c[2] - q[2]};
    const float la = sqrtf(rc_dot_t(A[0], A[1], A[2], A[0], A[1], A[2]));
    const float lb = sqrtf(rc_dot_t(B[0], B[1], B[2], B[0], B[1], B[2]));
    const float lc = sqrtf(rc_dot_t(C[0], C[1], C[2], C[0], C[1], C[2]));
    const float n[3] = {B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]};
    const float det = rc_dot_t(A[0], A[1], A[2], n[0], n[1], n[2]);
    const float ab = rc_dot_t(A[0], A[1], A[2], B[0], B[1], B[2]);
    const float bc = rc_dot_t(B[0], B[1], B[2], C[0], C[1], C[2]);
    const float ca = rc_dot_t(C[0], C[1], C[2], A[0], A[1], A[2]);
    const float den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
    return atan2f(det, den) + ((la + lb) + lc) * 0.f;
}

static inline int wn_chunks(int max_faces) { return (max_faces + PM_CHUNK - 1) / PM_CHUNK; }

// partial (B, chunks, Q): the fp32 sum of Omega / 2 over the faces of one chunk, ascending
static __global__ void __launch_bounds__(PM_BLOCK) wn_tile_kernel(int Q, PmRaggedMesh mesh, const float* __restrict__ qs, const int* __restrict__ qlen,
                                                                  float* __restrict__ partial) {
    __shared__ float tri[9][PM_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int n = clamp_len(qlen, b, Q);
    const int r0 = blockIdx.y * PM_ROWS;
    if (r0 >= n) return;                              // uniform: padding is never read
    const int V = mesh.nv(b), F = mesh.nf(b);
    const int f0 = blockIdx.x * PM_CHUNK, f1 = min(F, f0 + PM_CHUNK);
    if (f0 >= F) return;                              // uniform: the final kernel reads the chunks below ceil(F_b / 1024) only
    const float* Qb = qs + (size_t)b * Q * 3;
    const float* Vb = mesh.vb(b);
    const int* Fb = mesh.fb(b);
    float p[PM_R][3], acc[PM_R];
    bool ok[PM_R];
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        ok[r] = i < n;
        for (int c = 0; c < 3; ++c) p[r][c] = ok[r] ? Qb[(size_t)i * 3 + c] : 0.f;
        acc[r] = 0.f;
    }
    for (int t0 = f0; t0 < f1; t0 += PM_TILE) {
        const int tn = min(PM_TILE, f1 - t0);
        __syncthreads();
        if (tid < tn) {
            const int* fv = Fb + (size_t)(t0 + tid) * 3;
            const int v0 = fv[0], v1 = fv[1], v2 = fv[2];
            const bool in = v0 >= 0 && v0 < V && v1 >= 0 && v1 < V && v2 >= 0 && v2 < V;
            const int vi[3] = {v0, v1, v2};
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) tri[3 * k + c][tid] = in ? Vb[(size_t)vi[k] * 3 + c] : 0.f;
        }
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float a[3] = {tri[0][k], tri[1][k], tri[2][k]}, bb[3] = {tri[3][k], tri[4][k], tri[5][k]}, c[3] = {tri[6][k], tri[7][k], tri[8][k]};
#pragma unroll
            for (int r = 0; r < PM_R; ++r) acc[r] += wn_half_angle(p[r], a, bb, c);
        }
    }
    const size_t base = ((size_t)b * gridDim.x + blockIdx.x) * Q;
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        if (ok[r]) partial[base + i] = acc[r];
    }
}

// w = (sum over the scan's chunks, ascending, fp64) / (2 pi), rounded once to fp32; padding queries get 0
static __global__ void __launch_bounds__(256) wn_final_kernel(int B, int Q, int chunks, PmRaggedMesh mesh, const int* __restrict__ qlen,
                                                              const float* __restrict__ partial, float* __restrict__ w) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * Q) return;
    const int b = (int)(t / Q), i = (int)(t % Q);
    double s = 0.0;
    if (i < clamp_len(qlen, b, Q)) {
        const int nc = min(chunks, (mesh.nf(b) + PM_CHUNK - 1) / PM_CHUNK);
        for (int c = 0; c < nc; ++c) s += (double)partial[((size_t)b * chunks + c) * Q + i];
    }
    w[t] = (float)(s * 0.15915494309189533577);       // 1 / (2 pi)
}

static int wn_run(int B, int Q, int max_faces, PmRaggedMesh mesh, const float* queries, const int* q_len, float* partial, float* w, hipStream_t st) {
    const int chunks = wn_chunks(max_faces);
    if (chunks > 0)
        hipLaunchKernelGGL(wn_tile_kernel, dim3(chunks, (Q + PM_ROWS - 1) / PM_ROWS, B), dim3(PM_BLOCK), 0, st, Q, mesh, queries, q_len, partial);
    hipLaunchKernelGGL(wn_final_kernel, dim3(nblk((long)B * Q)), dim3(256), 0, st, B, Q, chunks, mesh, q_len, partial, w);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// ---------------------------------------------------------------------------------------------- the containment term
// o_v = [ |w_v| < 0.5 ] (a NaN w fails the <) and the vertex has a usable correspondence (face in [0, F_b), its three indices in [0, V_b));
// c_v = sum_k bary_k s_k in fp64, s the scan's vertices.  Writes the flag and the target point.
static __global__ void __launch_bounds__(256) ct_target_kernel(int B, int V, PmRaggedMesh mesh, const float* __restrict__ w, const int* __restrict__ face,
                                                               const float* __restrict__ bary, int* __restrict__ outside, double* __restrict__ target) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * V) return;
    const int b = (int)(t / V);
    const int f = face[t], Vs = mesh.nv(b);
    int o = 0;
    double c[3] = {0.0, 0.0, 0.0};
    if (fabsf(w[t]) < 0.5f && f >= 0 && f < mesh.nf(b)) {
        const int* fv = mesh.fb(b) + (size_t)f * 3;
        if (fv[0] >= 0 && fv[0] < Vs && fv[1] >= 0 && fv[1] < Vs && fv[2] >= 0 && fv[2] < Vs) {
            const float* Sb = mesh.vb(b);
            o = 1;
            for (int k = 0; k < 3; ++k)
                c[k] = ((double)bary[t * 3] * (double)Sb[(size_t)fv[0] * 3 + k] + (double)bary[t * 3 + 1] * (double)Sb[(size_t)fv[1] * 3 + k])
                       + (double)bary[t * 3 + 2] * (double)Sb[(size_t)fv[2] * 3 + k];
        }
    }
    outside[t] = o;
    for (int k = 0; k < 3; ++k) target[t * 3 + k] = c[k];
}

// One workgroup per scan, fp64, fixed order (strided per thread, then a tree): terms[b] = {sum_v o_v d2_v, sum_v o_v}; d2 = the fp32 values
// handed in, or (d2 NULL) |v - c_v|^2 of the current vertices and the held targets in fp64.
static __global__ void __launch_bounds__(256) ct_terms_kernel(int V, const float* __restrict__ verts, const int* __restrict__ outside,
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
static __global__ void __launch_bounds__(256) ct_apply_kernel(int B, int V, const float* __restrict__ verts, const int* __restrict__ outside,
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
struct CtWork {
    float *wn, *partial, *bary, *d2;
    int *face, *outside;
    u64* keys;
    double *target, *terms;
    size_t bytes;
};

static CtWork ct_layout(char* base, size_t off, int B, int V, int max_faces) {
    CtWork w;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += al(n); return p; };
    w.wn = (float*)take((size_t)B * V * 4);
    w.partial = (float*)take((size_t)B * wn_chunks(max_faces) * V * 4);
    w.bary = (float*)take((size_t)B * V * 12);
    w.d2 = (float*)take((size_t)B * V * 4);
    w.face = (int*)take((size_t)B * V * 4);
    w.outside = (int*)take((size_t)B * V * 4);
    w.keys = (u64*)take((size_t)B * V * 8);
    w.target = (double*)take((size_t)B * V * 24);
    w.terms = (double*)take((size_t)B * 16);
    w.bytes = off;
    return w;
}

static bool ct_mesh_ok(int max_faces, const float* verts, const int* faces, const int* voff, const int* foff) {
    return max_faces >= 0 && voff && foff && (max_faces == 0 || (verts && faces));
}

extern "C" {

int etch_mesh_winding_number_workspace(int B, int Q, int max_faces, long long* bytes) {
    if (B < 0 || Q < 0 || max_faces < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)B * wn_chunks(max_faces) * Q * 4;
    return ETCH_OK;
}

int etch_mesh_winding_number(int B, int Q, int max_faces, const float* verts, const int* faces, const int* vert_offsets, const int* face_offsets,
                             const float* queries, const int* q_len, void* workspace, float* w, void* stream) {
    if (B < 0 || Q < 0) return ETCH_EINVAL;
    if (B == 0 || Q == 0) return ETCH_OK;
    if (!ct_mesh_ok(max_faces, verts, faces, vert_offsets, face_offsets) || !queries || !w || (max_faces > 0 && !workspace)) return ETCH_EINVAL;
    return wn_run(B, Q, max_faces, PmRaggedMesh{verts, faces, vert_offsets, face_offsets}, queries, q_len, (float*)workspace, w, (hipStream_t)stream);
}

int etch_ragged_mesh_closest_workspace(int B, int N, long long* bytes) {
    if (B < 0 || N < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)B * N * 8;
    return ETCH_OK;
}

int etch_ragged_mesh_closest(int B, int N, int max_faces, const float* verts, const int* faces, const int* vert_offsets, const int* face_offsets,
                             const float* points, const int* n_len, void* workspace, int* face, float* bary, float* d2, void* stream) {
    if (B < 0 || N < 0) return ETCH_EINVAL;
    if (B == 0 || N == 0) return ETCH_OK;
    if (!ct_mesh_ok(max_faces, verts, faces, vert_offsets, face_offsets) || !workspace || !points || !face || !bary || !d2) return ETCH_EINVAL;
    return pm_closest_mesh(B, N, max_faces, PmRaggedMesh{verts, faces, vert_offsets, face_offsets}, points, n_len, (u64*)workspace, face, bary, d2,
                           (hipStream_t)stream);
}

int etch_containment_energy_grad_workspace(int B, int V, long long* bytes) {
    if (B < 0 || V < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)(al((size_t)B * V * 4) + al((size_t)B * V * 24));
    return ETCH_OK;
}

int etch_containment_energy_grad(int B, int V, const float* body_verts, const float* verts, const int* faces, const int* vert_offsets,
                                 const int* face_offsets, const float* w, const int* face, const float* bary, const float* d2, const float* coef,
                                 float w_contain, void* workspace, double* terms, float* g, void* stream) {
    if (B < 0 || V < 0 || !terms) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    if (!vert_offsets || !face_offsets || !workspace || (V > 0 && (!body_verts || !verts || !faces || !w || !face || !bary || !d2))) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* outside = (int*)workspace;
    double* target = (double*)((char*)workspace + al((size_t)B * V * 4));
    const PmRaggedMesh mesh{verts, faces, vert_offsets, face_offsets};
    if (V > 0) hipLaunchKernelGGL(ct_target_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, mesh, w, face, bary, outside, target);
    hipLaunchKernelGGL(ct_terms_kernel, dim3(B), dim3(256), 0, st, V, body_verts, outside, target, d2, terms);
    if (g && V > 0) hipLaunchKernelGGL(ct_apply_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, body_verts, outside, target, coef, w_contain, g);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_smpl_surface_refine_contain_workspace(int B, int N, int V, int nj, int nb, int n_extra, int max_faces, long long* bytes) {
    if (B < 0 || N < 0 || V < 0 || max_faces < 0 || !bytes) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    *bytes = (long long)ct_layout(nullptr, sf_layout(nullptr, B, N, V, nj, nb, n_extra).bytes, B, V, max_faces).bytes;
    return ETCH_OK;
}

int etch_smpl_surface_refine_contain(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces, const float* points,
                                     const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers, const float* marker_valid,
                                     const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2, float eps, float w_dense,
                                     float w_marker, float w_beta, float w_prior, float trunc, int optimize_scale, int max_scan_faces, const float* scan_verts,
                                     const int* scan_faces, const int* scan_vert_offsets, const int* scan_face_offsets, float w_contain, int contain_every,
                                     float* params, float* verts, float* joints, float* loss_trace, float* loss_last, void* workspace, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || F <= 0 || M < 0 || iters < 1 || n_gauss < 0 || n_gauss > SF_MAXG || contain_every < 1) return ETCH_EINVAL;
    if (M > 0 && (!marker_vids || !markers || !marker_valid)) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (n_gauss > 0 && (nj != 24 || !prior)) return ETCH_EUNSUPPORTED;      // the GMM prior is over the 69-dim SMPL body pose only
    if (B == 0) return ETCH_OK;
    if (!workspace || !params || !verts || !joints || !loss_last) return ETCH_EINVAL;
    if (!ct_mesh_ok(max_scan_faces, scan_verts, scan_faces, scan_vert_offsets, scan_face_offsets)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const SfWork w = sf_layout((char*)workspace, B, N, V, nj, nb, n_extra);
    const CtWork c = ct_layout((char*)workspace, w.bytes, B, V, max_scan_faces);
    const PmRaggedMesh scan{scan_verts, scan_faces, scan_vert_offsets, scan_face_offsets};
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
        if (it % contain_every == 0) {                 // refresh: which vertices are outside, and the scan point each is pulled to
            e = wn_run(B, V, max_scan_faces, scan, w.verts, nullptr, c.partial, c.wn, st);
            if (!e) e = pm_closest_mesh(B, V, max_scan_faces, scan, w.verts, nullptr, c.keys, c.face, c.bary, c.d2, st);
            if (e) return e;
            hipLaunchKernelGGL(ct_target_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, scan, c.wn, c.face, c.bary, c.outside, c.target);
        }
        // in between o_v and c_v are held (the target POINT, not the face): the term stays a fixed quadratic between two refreshes
        hipLaunchKernelGGL(ct_terms_kernel, dim3(B), dim3(256), 0, st, V, w.verts, c.outside, c.target, (const float*)nullptr, c.terms);
        hipLaunchKernelGGL(ct_apply_kernel, dim3(nblk((long)B * V)), dim3(256), 0, st, B, V, w.verts, c.outside, c.target, (const float*)nullptr, w_contain, w.gy);
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
