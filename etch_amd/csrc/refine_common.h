// Kernels shared by the Adam refinements of a fitted body (chamfer_fit.hip: against the scan's vertices; surface_fit.hip: the body surface
// against the predicted inner points): the parameter packing, the full-mesh LBS vector-Jacobian product, the Adam update and the small fills.
// Every kernel is `static`: each TU that includes this header gets its own copy, built with that TU's flags (both use -ffp-contract=off).
//
// Parameters of a refinement, per scan: p = pose[3 nj] (global orient first) | beta[nb] | trans[3] | scale[1];
// verts = (LBS(pose, beta) + trans) * scale, LBS = smpl_lbs_kernel (smpl_fit.hip) on x = pose[3:] | beta | pose[:3] | trans.
#pragma once
#include "common.h"
#include "etch_hip.h"
#include "smpl_common.h"
#include <algorithm>

typedef unsigned long long u64;

#define CHAM_FIX 1099511627776.0      // 2^40: the fixed-point unit of the order-free scatters (2^-40 m, exact while |sum| < 2^23 m)

__device__ __forceinline__ int clamp_len(const int* len, int b, int n) { return len ? min(max(len[b], 0), n) : n; }

static __global__ void __launch_bounds__(256) u64_fill_kernel(long n, u64* __restrict__ p, u64 val) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = val;
}

static __global__ void __launch_bounds__(256) f32_zero_kernel(long n, float* __restrict__ p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// ---------------------------------------------------------------------------------------------- LBS vector-Jacobian product
#define RF_MAXJ 55
#define RF_MAXB 20
struct RfConsts {
    const float* v_template; const float* shapedirs; const float* posedirs; const float* weights;
    const float* J0; const float* Jd; const int* parents; const int* extra_vids;
};

static __global__ void __launch_bounds__(256) rf_pack_kernel(int B, int nj, int nb, const float* __restrict__ p, float* __restrict__ x, int zero_trans) {
    const int P = 3 * nj + nb + 4, DOF = 3 * nj + nb + 3, NPOSE = 3 * (nj - 1);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * DOF) return;
    const int b = t / DOF, k = t % DOF;
    const float* pb = p + (size_t)b * P;
    float v;
    if (k < NPOSE) v = pb[3 + k];
    else if (k < NPOSE + nb) v = pb[3 * nj + (k - NPOSE)];
    else if (k < NPOSE + nb + 3) v = pb[k - NPOSE - nb];
    else v = zero_trans ? 0.f : pb[3 * nj + nb + (k - NPOSE - nb - 3)];
    x[t] = v;
}

static __global__ void __launch_bounds__(256) rf_scale_kernel(int B, int V, int P, const float* __restrict__ p, const float* __restrict__ u, float* __restrict__ verts) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * V * 3) return;
    verts[t] = u[t] * p[(t / (3L * V)) * P + P - 1];
}

// per vertex: h = scale g, the posed rest vertex vp, dL/dvp = T_v^T h (T_v = sum_j w_vj Rw_j) and g . u (the scale gradient's summand)
static __global__ void __launch_bounds__(256) rf_vertex_kernel(RfConsts C, int NJ, int NB, int V, const float* __restrict__ x, const float* __restrict__ params,
                                                               const float* __restrict__ g, const float* __restrict__ u, float* __restrict__ h_out,
                                                               float* __restrict__ vp_out, float* __restrict__ dvp_out, float* __restrict__ gu_out) {
    __shared__ double R[RF_MAXJ * 9], Rw[RF_MAXJ * 9], tw[RF_MAXJ * 3], Jj[RF_MAXJ * 3], xs[3 * RF_MAXJ + RF_MAXB + 3];
    __shared__ float Rf[RF_MAXJ][9], pf[9 * (RF_MAXJ - 1)];
    __shared__ int parents[RF_MAXJ];
    const int NPOSE = 3 * (NJ - 1), NPF = 9 * (NJ - 1), DOF = NPOSE + NB + 6, P = 3 * NJ + NB + 4;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < DOF) xs[tid] = (double)x[(size_t)b * DOF + tid];
    if (tid < NJ) parents[tid] = C.parents[tid];
    __syncthreads();
    smpl_block_chain(NJ, NB, C.J0, C.Jd, parents, xs, R, Jj, Rw, tw);
    for (int e = tid; e < NPF; e += 256) { const int k = 1 + e / 9, q = e % 9; pf[e] = (float)(R[k * 9 + q] - ((q % 4 == 0) ? 1.0 : 0.0)); }
    __syncthreads();
    if (tid < NJ)
        for (int e = 0; e < 9; ++e) Rf[tid][e] = (float)Rw[tid * 9 + e];
    __syncthreads();
    const int v = blockIdx.x * 256 + tid;
    if (v >= V) return;
    float vp[3];
    for (int c = 0; c < 3; ++c) {
        float acc = C.v_template[v * 3 + c];
        for (int l = 0; l < NB; ++l) acc += C.shapedirs[((size_t)v * 3 + c) * NB + l] * (float)xs[NPOSE + l];
        vp[c] = acc;
    }
    for (int e = 0; e < NPF; ++e) {
        const float* Pp = C.posedirs + (size_t)e * V * 3 + v * 3;
        vp[0] += pf[e] * Pp[0]; vp[1] += pf[e] * Pp[1]; vp[2] += pf[e] * Pp[2];
    }
    float T[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < NJ; ++j) {
        const float w = C.weights[(size_t)v * NJ + j];
        if (w != 0.f)
            for (int i = 0; i < 9; ++i) T[i] += w * Rf[j][i];
    }
    const size_t o = ((size_t)b * V + v) * 3;
    const float s = params[(size_t)b * P + P - 1];
    const float h[3] = {s * g[o], s * g[o + 1], s * g[o + 2]};
    for (int c = 0; c < 3; ++c) {
        h_out[o + c] = h[c];
        vp_out[o + c] = vp[c];
        dvp_out[o + c] = T[c] * h[0] + T[3 + c] * h[1] + T[6 + c] * h[2];
    }
    gu_out[(size_t)b * V + v] = g[o] * u[o] + g[o + 1] * u[o + 1] + g[o + 2] * u[o + 2];
}

// per-scan reductions over the V vertices, one workgroup per (item, scan), fp64, fixed order (strided per thread, then a tree):
//   [0, 12 NJ)        dL/dA_j (a, c) = sum_v w_vj h_va [vp_v, 1]_c        (A_j = [Rw_j | tw_j - Rw_j J_j])
//   + NB              dL/dbeta_l (blend shapes) = sum_v S_v[:, l] . dvp_v
//   + 9 (NJ - 1)      dL/dpf_e = sum_v posedirs[e, v, :] . dvp_v
//   + 3, + 1          dL/dtrans = sum_v h_v,  dL/dscale = sum_v g_v . u_v
static __global__ void __launch_bounds__(256) rf_reduce_kernel(RfConsts C, int NJ, int NB, int V, const float* __restrict__ h, const float* __restrict__ vp,
                                                               const float* __restrict__ dvp, const float* __restrict__ gu, double* __restrict__ red) {
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int NPF = 9 * (NJ - 1), K = 12 * NJ + NB + NPF + 4;
    const float* hb = h + (size_t)b * V * 3;
    const float* vb = vp + (size_t)b * V * 3;
    const float* db = dvp + (size_t)b * V * 3;
    double acc = 0.0;
    if (k < 12 * NJ) {
        const int j = k / 12, a = (k % 12) / 4, c = k % 4;
        for (int v = tid; v < V; v += 256) {
            const float w = C.weights[(size_t)v * NJ + j];
            if (w != 0.f) acc += (double)w * (double)hb[v * 3 + a] * (c < 3 ? (double)vb[v * 3 + c] : 1.0);
        }
    } else if (k < 12 * NJ + NB) {
        const int l = k - 12 * NJ;
        for (int v = tid; v < V; v += 256)
            for (int c = 0; c < 3; ++c) acc += (double)C.shapedirs[((size_t)v * 3 + c) * NB + l] * (double)db[v * 3 + c];
    } else if (k < 12 * NJ + NB + NPF) {
        const float* Pe = C.posedirs + (size_t)(k - 12 * NJ - NB) * V * 3;
        for (int v = tid; v < 3 * V; v += 256) acc += (double)Pe[v] * (double)db[v];
    } else if (k < K - 1) {
        const int a = k - (K - 4);
        for (int v = tid; v < V; v += 256) acc += (double)hb[v * 3 + a];
    } else {
        for (int v = tid; v < V; v += 256) acc += (double)gu[(size_t)b * V + v];
    }
    __shared__ double sm[256];
    sm[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sm[tid] += sm[tid + s];
        __syncthreads();
    }
    if (tid == 0) red[(size_t)b * K + k] = sm[0];
}

// per scan: the reduced sums -> dL/d(pose, beta, trans, scale), backward through A_j, fk_chain and rodrigues_d in fp64; ADDED to grad.
// Needs parents[j] < j (true of the SMPL and SMPL-X trees; the host checks).
static __global__ void __launch_bounds__(64) rf_chain_kernel(RfConsts C, int NJ, int NB, const float* __restrict__ x, const double* __restrict__ red,
                                                             float* __restrict__ grad) {
    __shared__ double R[RF_MAXJ * 9], Rw[RF_MAXJ * 9], tw[RF_MAXJ * 3], Jj[RF_MAXJ * 3], xs[3 * RF_MAXJ + RF_MAXB + 3];
    __shared__ double dRw[RF_MAXJ * 9], dtw[RF_MAXJ * 3], dJ[RF_MAXJ * 3], dR[RF_MAXJ * 9];
    __shared__ float dRd[RF_MAXJ][3][9];
    __shared__ int parents[RF_MAXJ];
    const int NPOSE = 3 * (NJ - 1), NPF = 9 * (NJ - 1), DOF = NPOSE + NB + 6, P = 3 * NJ + NB + 4, K = 12 * NJ + NB + NPF + 4;
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* rb = red + (size_t)b * K;
    for (int t = tid; t < DOF; t += 64) xs[t] = (double)x[(size_t)b * DOF + t];
    for (int t = tid; t < NJ; t += 64) parents[t] = C.parents[t];
    __syncthreads();
    for (int j = tid; j < NJ; j += 64) {
        double th[3];
        joint_theta(xs, j, NPOSE, NB, th);
        rodrigues_d(th, R + j * 9, dRd[j], true);
        for (int c = 0; c < 3; ++c) {
            double v = C.J0[j * 3 + c];
            for (int l = 0; l < NB; ++l) v += (double)C.Jd[(j * 3 + c) * NB + l] * xs[NPOSE + l];
            Jj[j * 3 + c] = v;
        }
    }
    __syncthreads();
    if (tid == 0) {
        fk_chain(NJ, parents, R, Jj, Rw, tw);
        for (int j = 0; j < NJ; ++j) {                 // A_j = [Rw_j | t'_j], t'_j = tw_j - Rw_j J_j
            const double* dA = rb + 12 * j;
            for (int a = 0; a < 3; ++a) {
                const double dt = dA[a * 4 + 3];
                for (int c = 0; c < 3; ++c) dRw[j * 9 + a * 3 + c] = dA[a * 4 + c] - dt * Jj[j * 3 + c];
                dtw[j * 3 + a] = dt;
            }
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int a = 0; a < 3; ++a) s += Rw[j * 9 + a * 3 + c] * dA[a * 4 + 3];
                dJ[j * 3 + c] = -s;
            }
        }
        for (int j = NJ - 1; j >= 1; --j) {            // Rw_j = Rw_p R_j,  tw_j = Rw_p (J_j - J_p) + tw_p
            const int p = parents[j];
            const double* Rp = Rw + p * 9;
            const double* Rj = R + j * 9;
            const double* G = dRw + j * 9;
            const double d[3] = {Jj[j * 3] - Jj[p * 3], Jj[j * 3 + 1] - Jj[p * 3 + 1], Jj[j * 3 + 2] - Jj[p * 3 + 2]};
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0, r = 0.0;
                    for (int m = 0; m < 3; ++m) { s += G[a * 3 + m] * Rj[c * 3 + m]; r += Rp[m * 3 + a] * G[m * 3 + c]; }
                    dRw[p * 9 + a * 3 + c] += s + dtw[j * 3 + a] * d[c];
                    dR[j * 9 + a * 3 + c] = r;
                }
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int a = 0; a < 3; ++a) s += Rp[a * 3 + c] * dtw[j * 3 + a];
                dJ[j * 3 + c] += s;
                dJ[p * 3 + c] -= s;
            }
            for (int a = 0; a < 3; ++a) dtw[p * 3 + a] += dtw[j * 3 + a];
        }
        for (int e = 0; e < 9; ++e) dR[e] = dRw[e];
        for (int c = 0; c < 3; ++c) dJ[c] += dtw[c];
        for (int e = 0; e < NPF; ++e) dR[9 + e] += rb[12 * NJ + NB + e];      // pf = vec(R_k - I), k >= 1
    }
    __syncthreads();
    float* gb = grad + (size_t)b * P;
    for (int t = tid; t < 3 * NJ; t += 64) {          // pose: the refinement's order (joint j at 3 j, global orient first)
        const int j = t / 3, q = t % 3;
        double s = 0.0;
        for (int e = 0; e < 9; ++e) s += dR[j * 9 + e] * (double)dRd[j][q][e];
        gb[t] += (float)s;
    }
    for (int l = tid; l < NB; l += 64) {
        double s = rb[12 * NJ + l];
        for (int jc = 0; jc < 3 * NJ; ++jc) s += dJ[jc] * (double)C.Jd[jc * NB + l];
        gb[3 * NJ + l] += (float)s;
    }
    if (tid < 4) gb[3 * NJ + NB + tid] += (float)rb[K - 4 + tid];
}

// torch.optim.Adam (single-tensor form, no weight decay): m = m + (1 - b1)(g - m), v = b2 v + (1 - b2) g^2, p -= step_size m / (sqrt(v) / bc2s + eps)
static __global__ void __launch_bounds__(256) rf_adam_kernel(long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                             float b1c, float b2, float b2c, float step_size, float bc2s, float eps) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float gt = g[t];
    const float mt = m[t] + b1c * (gt - m[t]);
    const float vt = v[t] * b2 + b2c * (gt * gt);
    m[t] = mt; v[t] = vt;
    const float denom = sqrtf(vt) / bc2s + eps;
    p[t] = p[t] + (-step_size) * (mt / denom);
}

// ---------------------------------------------------------------------------------------------- host side
static inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }
static inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

// the buffers of the forward and of the vector-Jacobian product; a refinement's workspace struct derives from it
struct RfCore {
    float *x, *u, *jtmp, *h, *vp, *dvp, *gu;
    double* red;
};

static inline RfConsts rf_consts(const void* const* c) {
    return RfConsts{(const float*)c[0], (const float*)c[1], (const float*)c[2], (const float*)c[3], (const float*)c[4], (const float*)c[5],
                    (const int*)c[6], (const int*)c[7]};
}

static inline bool rf_supported(int nj, int nb) { return (nj == 24 && nb == 10) || (nj == 55 && nb == 20); }

extern "C" int etch_smpl_lbs(int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* x, float* verts, float* joints, void* stream);

static inline int rf_vjp(const RfCore& w, int B, int V, int nj, int nb, const void* const* consts, const float* params, const float* g, float* grad,
                         hipStream_t st) {
    const RfConsts C = rf_consts(consts);
    const int K = 12 * nj + nb + 9 * (nj - 1) + 4;
    hipLaunchKernelGGL(rf_vertex_kernel, dim3((V + 255) / 256, B), dim3(256), 0, st, C, nj, nb, V, w.x, params, g, w.u, w.h, w.vp, w.dvp, w.gu);
    hipLaunchKernelGGL(rf_reduce_kernel, dim3(K, B), dim3(256), 0, st, C, nj, nb, V, w.h, w.vp, w.dvp, w.gu, w.red);
    hipLaunchKernelGGL(rf_chain_kernel, dim3(B), dim3(64), 0, st, C, nj, nb, w.x, w.red, grad);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

static inline int rf_forward(const RfCore& w, int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* params, float* verts,
                             float* joints, int zero_trans, hipStream_t st) {
    const int DOF = 3 * nj + nb + 3;
    hipLaunchKernelGGL(rf_pack_kernel, dim3(nblk((long)B * DOF)), dim3(256), 0, st, B, nj, nb, params, w.x, zero_trans);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    int e = etch_smpl_lbs(B, V, nj, nb, n_extra, consts, w.x, w.u, joints ? joints : w.jtmp, st);
    if (e) return e;
    if (verts) hipLaunchKernelGGL(rf_scale_kernel, dim3(nblk((long)B * V * 3)), dim3(256), 0, st, B, V, DOF + 1, params, w.u, verts);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// step i of a refinement's Adam schedule: the script sets the learning rate AFTER each step, so step 0 and step 1 both run at lr, step
// i >= 1 at lr (N - i + 1) / N.  bp1 / bp2 carry beta^i.
static inline int rf_adam_step(int it, int iters, float lr, float beta1, float beta2, float eps, double& bp1, double& bp2, long n, float* params,
                               const float* grad, float* m, float* v, hipStream_t st) {
    const double lr_i = it == 0 ? (double)lr : (double)lr * (double)(iters - it + 1) / (double)iters;
    bp1 *= (double)beta1; bp2 *= (double)beta2;
    const double bc1 = 1.0 - bp1, bc2 = 1.0 - bp2;
    hipLaunchKernelGGL(rf_adam_kernel, dim3(nblk(n)), dim3(256), 0, st, n, params, grad, m, v, (float)(1.0 - beta1), beta2, (float)(1.0 - beta2),
                       (float)(lr_i / bc1), (float)sqrt(bc2), eps);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}
