// Kernels and host helpers of the dense surface refinement, shared by surface_fit.hip (its C ABI) and containment.hip (the same
// refinement with the containment term).  Every kernel is `static`: each TU that includes this header gets its own copy, built
// with that TU's flags (both use -ffp-contract=off).
//
// Determinism: every reduction has a fixed order; the only atomics are 64-bit INTEGER ones -- atomicMin on (d2 bits, face) keys, whose
// result is the same in any order, and atomicAdd of fixed-point terms (2^-40 m), which is exact and so order-free too.
// The region test is closest_tri.h's, bit-defined in fp32 (tests/_surface_oracle.py restates it).
#pragma once
#include "etch_hip.h"
#include "refine_common.h"
#include "closest_tri.h"

// ---------------------------------------------------------------------------------------------- closest point on the mesh
// One workgroup per (scan, 512-point block, 1024-face chunk).  A thread keeps PM_R = 2 points in registers (points r0 + 256 r + tid); each
// 256-face tile is gathered through `faces` into LDS as nine floats per face (a, b, c) and read back as wave-uniform broadcasts.  Every
// (point, face) pair runs the full region test; ascending faces with a strict < keep the lowest face of a tie inside the chunk, and the
// chunks merge through one atomicMin per point on key = (fp32 bits of d2) << 32 | face: d2 >= 0, so the integer order is (d2, face).
// A NaN d2 fails the <, so it never wins; a face with a vertex index outside [0, V) is staged as NaN and never wins either.
#define PM_BLOCK 256
#define PM_R 2
#define PM_ROWS (PM_BLOCK * PM_R)
#define PM_TILE 256
#define PM_CHUNK 1024

// How a kernel reaches the mesh of scan b.  PmSharedMesh: verts (B,V,3), one face list for the batch (etch_point_mesh_closest).
// PmRaggedMesh: the packed batch of mesh_io.pack_meshes -- verts (sum V,3), faces (sum F,3) local to their scan, vert_offsets / face_offsets
// (B+1) read on the device, so a launch is sized by the largest face count and needs no host read (containment.hip).
struct PmSharedMesh {
    int V, F;
    const float* verts;
    const int* faces;
    __device__ __forceinline__ int nv(int) const { return V; }
    __device__ __forceinline__ int nf(int) const { return F; }
    __device__ __forceinline__ const float* vb(int b) const { return verts + (size_t)b * V * 3; }
    __device__ __forceinline__ const int* fb(int) const { return faces; }
};
struct PmRaggedMesh {
    const float* verts;
    const int* faces;
    const int *voff, *foff;
    __device__ __forceinline__ int nv(int b) const { return max(voff[b + 1] - voff[b], 0); }
    __device__ __forceinline__ int nf(int b) const { return max(foff[b + 1] - foff[b], 0); }
    __device__ __forceinline__ const float* vb(int b) const { return verts + (size_t)voff[b] * 3; }
    __device__ __forceinline__ const int* fb(int b) const { return faces + (size_t)foff[b] * 3; }
};

template <typename Mesh>
static __global__ void __launch_bounds__(PM_BLOCK) pm_tile_kernel(int N, Mesh mesh, const float* __restrict__ pts, const int* __restrict__ nlen,
                                                                  u64* __restrict__ key) {
    __shared__ float tri[9][PM_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int n = clamp_len(nlen, b, N);
    const int r0 = blockIdx.y * PM_ROWS;
    if (r0 >= n) return;                              // uniform: padding is never read
    const int V = mesh.nv(b), F = mesh.nf(b);
    const int f0 = blockIdx.x * PM_CHUNK, f1 = min(F, f0 + PM_CHUNK);
    if (f0 >= F) return;                              // uniform: a ragged batch's grid is sized by its largest mesh
    const float INF = __int_as_float(0x7f800000), QNAN = __int_as_float(0x7fc00000);
    const float* Pb = pts + (size_t)b * N * 3;
    const float* Vb = mesh.vb(b);
    const int* Fb = mesh.fb(b);
    float p[PM_R][3], best[PM_R];
    int bf[PM_R];
    bool ok[PM_R];
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        ok[r] = i < n;
        for (int c = 0; c < 3; ++c) p[r][c] = ok[r] ? Pb[(size_t)i * 3 + c] : 0.f;
        best[r] = INF;
        bf[r] = -1;
    }
    for (int t0 = f0; t0 < f1; t0 += PM_TILE) {
        const int tn = min(PM_TILE, f1 - t0);
        __syncthreads();
        if (tid < tn) {
            const int* fv = Fb + (size_t)(t0 + tid) * 3;
            for (int k = 0; k < 3; ++k) {
                const int vi = fv[k];
                const bool in = vi >= 0 && vi < V;
                for (int c = 0; c < 3; ++c) tri[3 * k + c][tid] = in ? Vb[(size_t)vi * 3 + c] : QNAN;
            }
        }
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float a[3] = {tri[0][k], tri[1][k], tri[2][k]}, bb[3] = {tri[3][k], tri[4][k], tri[5][k]}, c[3] = {tri[6][k], tri[7][k], tri[8][k]};
#pragma unroll
            for (int r = 0; r < PM_R; ++r) {
                const float d = rc_closest_t<float>(p[r], a, bb, c).d2;
                if (ok[r] && d < best[r]) { best[r] = d; bf[r] = t0 + k; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PM_R; ++r) {
        const int i = r0 + r * PM_BLOCK + tid;
        if (ok[r] && bf[r] >= 0) atomicMin(key + (size_t)b * N + i, ((u64)__float_as_uint(best[r]) << 32) | (unsigned)bf[r]);
    }
}

// keys -> face (int32, -1 for padding and for a point no face could be chosen for), the barycentric weights and d2 of the chosen face,
// recomputed by the same function from the same inputs: the same bits
template <typename Mesh>
static __global__ void __launch_bounds__(256) pm_final_kernel(int B, int N, Mesh mesh, const float* __restrict__ pts, const int* __restrict__ nlen,
                                                              const u64* __restrict__ key, int* __restrict__ face, float* __restrict__ bary,
                                                              float* __restrict__ d2) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * N) return;
    const int b = (int)(t / N), i = (int)(t % N);
    int of = -1;
    float ob[3] = {0.f, 0.f, 0.f}, od = 0.f;
    const u64 k = key[t];
    if (i < clamp_len(nlen, b, N) && k != ~0ull && (unsigned)k < (unsigned)mesh.nf(b)) {
        const int f = (int)(unsigned)k;
        const int* fv = mesh.fb(b) + (size_t)f * 3;
        const float* Vb = mesh.vb(b);
        const float* p = pts + (size_t)t * 3;
        const RcClosestT<float> o = rc_closest_t<float>(p, Vb + (size_t)fv[0] * 3, Vb + (size_t)fv[1] * 3, Vb + (size_t)fv[2] * 3);
        of = f; od = o.d2;
        for (int c = 0; c < 3; ++c) ob[c] = o.b[c];
    }
    face[t] = of; d2[t] = od;
    for (int c = 0; c < 3; ++c) bary[t * 3 + c] = ob[c];
}

// ---------------------------------------------------------------------------------------------- energy and gradient
// m_i = [d2_i <= trunc2] on the fp32 value (no mask: use_mask 0); a point without a face (padding) counts for nothing.
__device__ __forceinline__ float pm_weight(const int* face, const float* d2, const float* weights, long t, float trunc2, int use_mask) {
    if (face[t] < 0 || (use_mask && !(d2[t] <= trunc2))) return 0.f;
    return weights ? weights[t] : 1.f;
}

// a correspondence handed in by a caller is used only if it names a face of the mesh whose three vertices exist
__device__ __forceinline__ bool pm_face_ok(const int* faces, int f, int F, int V) {
    if (f < 0 || f >= F) return false;
    const int* fv = faces + (size_t)f * 3;
    return fv[0] >= 0 && fv[0] < V && fv[1] >= 0 && fv[1] < V && fv[2] >= 0 && fv[2] < V;
}

// One workgroup per scan, fp64, fixed order (strided per thread, then a tree): terms[b] = {sum w m d2, sum w m};
// mterms[b] = {sum over the valid markers of |v_vid - t|^2, number of valid markers}.
static __global__ void __launch_bounds__(256) pm_terms_kernel(int N, int V, int M, const int* __restrict__ nlen, const int* __restrict__ face, const float* __restrict__ d2,
                                                       const float* __restrict__ weights, float trunc2, int use_mask, const float* __restrict__ verts,
                                                       const int* __restrict__ mvids, const float* __restrict__ markers, const float* __restrict__ mvalid,
                                                       double* __restrict__ terms, double* __restrict__ mterms) {
    __shared__ double sm[4][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_len(nlen, b, N);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const long t = (long)b * N + i;
        const double w = (double)pm_weight(face, d2, weights, t, trunc2, use_mask);
        if (w > 0.0) { a[0] += w * (double)d2[t]; a[1] += w; }
    }
    for (int m = tid; m < M; m += 256) {
        const int vid = mvids[m];
        if (!(mvalid[(size_t)b * M + m] > 0.f) || vid < 0 || vid >= V) continue;
        for (int c = 0; c < 3; ++c) {
            const double d = (double)verts[((size_t)b * V + vid) * 3 + c] - (double)markers[((size_t)b * M + m) * 3 + c];
            a[2] += d * d;
        }
        a[3] += 1.0;
    }
    for (int q = 0; q < 4; ++q) sm[q][tid] = a[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < 4; ++q) sm[q][tid] += sm[q][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        terms[b * 2] = sm[0][0]; terms[b * 2 + 1] = sm[1][0];
        mterms[b * 2] = sm[2][0]; mterms[b * 2 + 1] = sm[3][0];
    }
}

// Per point: q = sum_k bary_k v_k in fp64; the three vertices receive w m bary_k (q - p) as 2^-40 fixed-point integers (exact sum, any order).
// Per valid marker (threads past the points): its vertex receives (v_vid - t) in the marker accumulator.
static __global__ void __launch_bounds__(256) pm_scatter_kernel(int B, int N, int V, int F, int M, const float* __restrict__ pts, const int* __restrict__ nlen,
                                                         const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ face,
                                                         const float* __restrict__ bary, const float* __restrict__ d2, const float* __restrict__ weights,
                                                         float trunc2, int use_mask, const int* __restrict__ mvids, const float* __restrict__ markers,
                                                         const float* __restrict__ mvalid, unsigned long long* __restrict__ acc,
                                                         unsigned long long* __restrict__ macc) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long np = (long)B * N;
    if (t >= np + (long)B * M) return;
    if (t >= np) {
        const long u = t - np;
        const int b = (int)(u / M), vid = mvids[u % M];
        if (!(mvalid[u] > 0.f) || vid < 0 || vid >= V) return;
        for (int c = 0; c < 3; ++c) {
            const double d = (double)verts[((size_t)b * V + vid) * 3 + c] - (double)markers[u * 3 + c];
            atomicAdd(macc + ((size_t)b * V + vid) * 3 + c, (unsigned long long)__double2ll_rn(d * CHAM_FIX));
        }
        return;
    }
    const int b = (int)(t / N), i = (int)(t % N);
    if (i >= clamp_len(nlen, b, N)) return;
    const float w = pm_weight(face, d2, weights, t, trunc2, use_mask);
    if (!(w > 0.f) || !pm_face_ok(faces, face[t], F, V)) return;
    const int* fv = faces + (size_t)face[t] * 3;
    const float* Vb = verts + (size_t)b * V * 3;
    double diff[3];
    for (int c = 0; c < 3; ++c)
        diff[c] = (((double)bary[t * 3] * (double)Vb[(size_t)fv[0] * 3 + c] + (double)bary[t * 3 + 1] * (double)Vb[(size_t)fv[1] * 3 + c])
                   + (double)bary[t * 3 + 2] * (double)Vb[(size_t)fv[2] * 3 + c]) - (double)pts[t * 3 + c];
    for (int k = 0; k < 3; ++k) {
        const double wb = (double)w * (double)bary[t * 3 + k];
        if (wb == 0.0) continue;
        unsigned long long* a = acc + ((size_t)b * V + fv[k]) * 3;
        for (int c = 0; c < 3; ++c) atomicAdd(a + c, (unsigned long long)__double2ll_rn(wb * diff[c] * CHAM_FIX));
    }
}

// g_v = coef_b w_dense (2 / S0) acc_v + w_marker (2 / (3 n_valid)) macc_v; S0 = sum w m (normalize) or 1; a term whose denominator is 0 is 0.
static __global__ void __launch_bounds__(256) pm_gather_kernel(int B, int V, const double* __restrict__ terms, const double* __restrict__ mterms,
                                                        const float* __restrict__ coef, float w_dense, int normalize, float w_marker, int M,
                                                        const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ macc,
                                                        float* __restrict__ g) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * V * 3) return;
    const int b = (int)(t / (3L * V));
    const double S0 = terms[b * 2 + 1];
    double o = 0.0;
    if (S0 > 0.0) o = (coef ? (double)coef[b] : 1.0) * (double)w_dense * (2.0 / (normalize ? S0 : 1.0)) * ((double)(long long)acc[t] / CHAM_FIX);
    if (M > 0 && mterms[b * 2 + 1] > 0.0) o += (double)w_marker * (2.0 / (3.0 * mterms[b * 2 + 1])) * ((double)(long long)macc[t] / CHAM_FIX);
    g[t] = (float)o;
}

// the same dense term's gradient w.r.t. the points: coef_b w_dense (2 / S0) w m (p - q); padding rows get 0
static __global__ void __launch_bounds__(256) pm_point_grad_kernel(int B, int N, int V, int F, const float* __restrict__ pts, const int* __restrict__ nlen,
                                                            const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ face,
                                                            const float* __restrict__ bary, const float* __restrict__ d2, const float* __restrict__ weights,
                                                            float trunc2, int use_mask, const double* __restrict__ terms, const float* __restrict__ coef,
                                                            float w_dense, int normalize, float* __restrict__ gp) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * N) return;
    const int b = (int)(t / N), i = (int)(t % N);
    float o[3] = {0.f, 0.f, 0.f};
    const double S0 = terms[b * 2 + 1];
    const float w = i < clamp_len(nlen, b, N) ? pm_weight(face, d2, weights, t, trunc2, use_mask) : 0.f;
    if (w > 0.f && S0 > 0.0 && pm_face_ok(faces, face[t], F, V)) {
        const int* fv = faces + (size_t)face[t] * 3;
        const float* Vb = verts + (size_t)b * V * 3;
        const double s = (coef ? (double)coef[b] : 1.0) * (double)w_dense * (2.0 / (normalize ? S0 : 1.0)) * (double)w;
        for (int c = 0; c < 3; ++c) {
            const double q = ((double)bary[t * 3] * (double)Vb[(size_t)fv[0] * 3 + c] + (double)bary[t * 3 + 1] * (double)Vb[(size_t)fv[1] * 3 + c])
                             + (double)bary[t * 3 + 2] * (double)Vb[(size_t)fv[2] * 3 + c];
            o[c] = (float)(s * ((double)pts[t * 3 + c] - q));
        }
    }
    for (int c = 0; c < 3; ++c) gp[t * 3 + c] = o[c];
}

// ---------------------------------------------------------------------------------------------- refinement: loss
// One workgroup per scan: the four weighted terms of the loss from the reduced sums, the parameters and the optional max-mixture prior
// (min_g 0.5 d^T P_g d - log w_g over pose[3:], first minimum, as fit_cham's); resets grad to the regulariser's and the prior's gradient.
#define SF_PRIOR_D 69
#define SF_MAXG 16
static __global__ void __launch_bounds__(256) sf_loss_kernel(int NJ, int NB, const double* __restrict__ terms, const double* __restrict__ mterms,
                                                      const float* __restrict__ params, const float* __restrict__ means, const float* __restrict__ prec,
                                                      const float* __restrict__ nllw, int G, float w_dense, float w_marker, float w_beta, float w_prior,
                                                      float* __restrict__ grad, float* __restrict__ trace, int iters, int it, float* __restrict__ loss_last,
                                                      const double* __restrict__ cterms, float w_contain, int V) {
    const int b = blockIdx.x, tid = threadIdx.x, P = 3 * NJ + NB + 4;
    __shared__ double Pd[SF_MAXG][SF_PRIOR_D], PTd[SF_MAXG][SF_PRIOR_D], dd[SF_MAXG][SF_PRIOR_D];
    __shared__ int gbest;
    const float* pb = params + (size_t)b * P;
    for (int t = tid; t < G * SF_PRIOR_D; t += 256) dd[t / SF_PRIOR_D][t % SF_PRIOR_D] = (double)pb[3 + t % SF_PRIOR_D] - (double)means[t];
    __syncthreads();
    for (int t = tid; t < G * SF_PRIOR_D; t += 256) {
        const int g = t / SF_PRIOR_D, r = t % SF_PRIOR_D;
        const float* Pg = prec + (size_t)g * SF_PRIOR_D * SF_PRIOR_D;
        double a = 0.0, c = 0.0;
        for (int k = 0; k < SF_PRIOR_D; ++k) { a += (double)Pg[r * SF_PRIOR_D + k] * dd[g][k]; c += (double)Pg[k * SF_PRIOR_D + r] * dd[g][k]; }
        Pd[g][r] = a; PTd[g][r] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int gb = -1;
        double qb = 0.0;
        for (int g = 0; g < G; ++g) {
            double q = 0.0;
            for (int r = 0; r < SF_PRIOR_D; ++r) q += dd[g][r] * Pd[g][r];
            q = 0.5 * q - log((double)nllw[g]);
            if (gb < 0 || q < qb) { gb = g; qb = q; }
        }
        gbest = gb;
        double reg = 0.0;
        for (int l = 0; l < NB; ++l) reg += (double)pb[3 * NJ + l] * (double)pb[3 * NJ + l];
        const double S1 = terms[b * 2], S0 = terms[b * 2 + 1], SM = mterms[b * 2], nv = mterms[b * 2 + 1];
        const double t4[4] = {S0 > 0.0 ? (double)w_dense * (S1 / S0) : 0.0, nv > 0.0 ? (double)w_marker * (SM / (3.0 * nv)) : 0.0,
                              (double)w_beta * (reg / NB), G > 0 ? (double)w_prior * qb : 0.0};
        // cterms (containment.hip): a fifth term w_contain (sum_v o_v d2_v) / V and a fifth trace column; NULL: the four terms alone
        const int ncol = cterms ? 5 : 4;
        if (trace)
            for (int q = 0; q < 4; ++q) trace[((size_t)b * iters + it) * ncol + q] = (float)t4[q];
        double total = ((t4[0] + t4[1]) + t4[2]) + t4[3];
        if (cterms) {
            const double t5 = (double)w_contain * (cterms[b * 2] / V);
            if (trace) trace[((size_t)b * iters + it) * 5 + 4] = (float)t5;
            total += t5;
        }
        loss_last[b] = (float)total;
    }
    __syncthreads();
    float* gr = grad + (size_t)b * P;
    for (int k = tid; k < P; k += 256) {
        double g = 0.0;
        if (k >= 3 * NJ && k < 3 * NJ + NB) g = 2.0 * (double)w_beta * (double)pb[k] / NB;
        if (G > 0 && k >= 3 && k < 3 + SF_PRIOR_D) g = (double)w_prior * 0.5 * (Pd[gbest][k - 3] + PTd[gbest][k - 3]);
        gr[k] = (float)g;
    }
}

// scale stays at its initial value: a zero gradient keeps Adam's moments at zero and its update at exactly 0
static __global__ void __launch_bounds__(256) sf_freeze_scale_kernel(int B, int P, float* __restrict__ grad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) grad[(size_t)b * P + P - 1] = 0.f;
}

// ---------------------------------------------------------------------------------------------- host side
struct SfWork : RfCore {
    float *verts, *gy, *grad, *m, *v, *bary, *d2;
    int* face;
    u64* keys;
    unsigned long long *acc, *macc;
    double *terms, *mterms;
    size_t bytes;
};

static SfWork sf_layout(char* base, int B, int N, int V, int nj, int nb, int n_extra) {
    SfWork w;
    size_t off = 0;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += al(n); return p; };
    const int DOF = 3 * nj + nb + 3, P = DOF + 1, K = 12 * nj + nb + 9 * (nj - 1) + 4;
    w.x = (float*)take((size_t)B * DOF * 4);
    w.u = (float*)take((size_t)B * V * 12);
    w.jtmp = (float*)take((size_t)B * (nj + n_extra) * 12);
    w.h = (float*)take((size_t)B * V * 12);
    w.vp = (float*)take((size_t)B * V * 12);
    w.dvp = (float*)take((size_t)B * V * 12);
    w.gu = (float*)take((size_t)B * V * 4);
    w.red = (double*)take((size_t)B * K * 8);
    w.verts = (float*)take((size_t)B * V * 12);
    w.gy = (float*)take((size_t)B * V * 12);
    w.grad = (float*)take((size_t)B * P * 4);
    w.m = (float*)take((size_t)B * P * 4);
    w.v = (float*)take((size_t)B * P * 4);
    w.bary = (float*)take((size_t)B * N * 12);
    w.d2 = (float*)take((size_t)B * N * 4);
    w.face = (int*)take((size_t)B * N * 4);
    w.keys = (u64*)take((size_t)B * N * 8);
    w.acc = (unsigned long long*)take((size_t)B * V * 24);
    w.macc = (unsigned long long*)take((size_t)B * V * 24);
    w.terms = (double*)take((size_t)B * 16);
    w.mterms = (double*)take((size_t)B * 16);
    w.bytes = off;
    return w;
}

// maxF: the largest face count of the batch (PmSharedMesh: its F), which sizes the grid
template <typename Mesh>
static int pm_closest_mesh(int B, int N, int maxF, Mesh mesh, const float* points, const int* n_len, u64* keys, int* face, float* bary, float* d2,
                           hipStream_t st) {
    const long nk = (long)B * N;
    hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(nk), 4096)), dim3(256), 0, st, nk, keys, ~0ull);
    if (maxF > 0)
        hipLaunchKernelGGL(pm_tile_kernel<Mesh>, dim3((maxF + PM_CHUNK - 1) / PM_CHUNK, (N + PM_ROWS - 1) / PM_ROWS, B), dim3(PM_BLOCK), 0, st, N, mesh, points,
                           n_len, keys);
    hipLaunchKernelGGL(pm_final_kernel<Mesh>, dim3(nblk(nk)), dim3(256), 0, st, B, N, mesh, points, n_len, keys, face, bary, d2);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

static int pm_closest(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, u64* keys, int* face,
                      float* bary, float* d2, hipStream_t st) {
    return pm_closest_mesh(B, N, V > 0 ? F : 0, PmSharedMesh{V, F, verts, faces}, points, n_len, keys, face, bary, d2, st);
}

struct PmMarkers {
    int M;
    const int* vids;
    const float* pos;
    const float* valid;
    float w;
};

static int pm_energy_grad(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, const int* face, const float* bary,
                          const float* d2, const float* weights, float trunc, const float* coef, float w_dense, int normalize, PmMarkers mk,
                          unsigned long long* acc, unsigned long long* macc, double* terms, double* mterms, float* g, float* gp, hipStream_t st) {
    const int use_mask = trunc >= 0.f;
    const float trunc2 = trunc * trunc;
    hipLaunchKernelGGL(pm_terms_kernel, dim3(B), dim3(256), 0, st, N, V, mk.M, n_len, face, d2, weights, trunc2, use_mask, verts, mk.vids, mk.pos, mk.valid,
                       terms, mterms);
    if (g) {
        const long na = 3L * B * V;
        hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(na), 4096)), dim3(256), 0, st, na, (u64*)acc, 0ull);
        if (mk.M > 0) hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(na), 4096)), dim3(256), 0, st, na, (u64*)macc, 0ull);
        const long nt = (long)B * N + (long)B * mk.M;
        if (nt > 0)
            hipLaunchKernelGGL(pm_scatter_kernel, dim3(nblk(nt)), dim3(256), 0, st, B, N, V, F, mk.M, points, n_len, verts, faces, face, bary, d2, weights, trunc2,
                               use_mask, mk.vids, mk.pos, mk.valid, acc, macc);
        hipLaunchKernelGGL(pm_gather_kernel, dim3(nblk(3L * B * V)), dim3(256), 0, st, B, V, terms, mterms, coef, w_dense, normalize, mk.w, mk.M, acc, macc, g);
    }
    if (gp && N > 0)
        hipLaunchKernelGGL(pm_point_grad_kernel, dim3(nblk((long)B * N)), dim3(256), 0, st, B, N, V, F, points, n_len, verts, faces, face, bary, d2, weights, trunc2,
                           use_mask, terms, coef, w_dense, normalize, gp);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}
