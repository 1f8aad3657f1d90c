// SMPL+D registration of a fitted body onto its scan, and re-posing with it, on gfx950:
//
//   etch_smpl_skin_frames    params -> per-vertex skinning frames: verts(D) = base + R D, and the joint transforms A
//   etch_smpld_energy_grad   one evaluation of the registration energy (4 terms) and its gradient w.r.t. the offsets D
//   etch_smpld_register      the whole Adam schedule on D, queued on one stream
//   etch_skin_carry          carry points bound to the registered surface from one pose to another
//
// The neighbour pass and the scan -> body scatter are chamfer_fit.hip's (etch_nn_bidir, etch_chamfer_grad), called as they are.
// Determinism as there: no floating-point atomics, every sum in a fixed order, nothing depends on the batch a scan is in.
// The TU is built with -ffp-contract=off, so apply_vertex gives the same bits from the stand-alone apply and from the fused update.
#include "common.h"
#include "etch_hip.h"
#include "smpl_common.h"
#include <algorithm>

#define SK_MAXJ 55
#define SK_MAXB 20
#define RG_T 256

struct SkinConsts {
    const float* v_template; const float* shapedirs; const float* posedirs; const float* weights;
    const float* J0; const float* Jd; const int* parents;
};

// ---------------------------------------------------------------------------------------------- skinning frames
// smpl_lbs_kernel's forward (smpl_fit.hip) on params = pose (global orient first) | beta | trans | scale, stopped one step early:
// T_v = sum_j w_vj A_j is kept, base_v = (T_v [r_v; 1] + trans) scale and R_v = scale T_v^R are written instead of the vertex.
// The frames are computed once per registration and every later distance is a small difference of vertices built on them, so the
// per-vertex sums run in fp64 and round to fp32 once (the sequential fp32 sums of smpl_lbs_kernel cost about 5 ulp of the vertex).
__global__ void __launch_bounds__(RG_T) skin_frames_kernel(SkinConsts C, int NJ, int NB, int V, const float* __restrict__ params, float* __restrict__ base,
                                                           float* __restrict__ Rout, float* __restrict__ Aout) {
    __shared__ double R[SK_MAXJ * 9], Rw[SK_MAXJ * 9], tw[SK_MAXJ * 3], Jj[SK_MAXJ * 3], xs[3 * SK_MAXJ + SK_MAXB + 3];
    __shared__ double A[SK_MAXJ][12], pf[9 * (SK_MAXJ - 1)];
    __shared__ int parents[SK_MAXJ];
    const int NPOSE = 3 * (NJ - 1), NPF = 9 * (NJ - 1), P = 3 * NJ + NB + 4;
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* pb = params + (size_t)b * P;
    // the LM variable order joint_theta reads: body pose | betas | global orient (trans and scale are applied below)
    if (tid < NPOSE + NB + 3) xs[tid] = (double)(tid < NPOSE ? pb[3 + tid] : tid < NPOSE + NB ? pb[3 * NJ + (tid - NPOSE)] : pb[tid - NPOSE - NB]);
    if (tid < NJ) parents[tid] = C.parents[tid];
    __syncthreads();
    smpl_block_chain(NJ, NB, C.J0, C.Jd, parents, xs, R, Jj, Rw, tw);
    for (int e = tid; e < NPF; e += RG_T) { const int k = 1 + e / 9, q = e % 9; pf[e] = R[k * 9 + q] - ((q % 4 == 0) ? 1.0 : 0.0); }
    __syncthreads();
    if (tid < NJ) {                            // A_j = [Rw_j | tw_j - Rw_j J_j]
        for (int a = 0; a < 3; ++a) {
            double t = tw[tid * 3 + a];
            for (int c = 0; c < 3; ++c) { A[tid][a * 4 + c] = Rw[tid * 9 + a * 3 + c]; t -= Rw[tid * 9 + a * 3 + c] * Jj[tid * 3 + c]; }
            A[tid][a * 4 + 3] = t;
        }
        if (blockIdx.x == 0)
            for (int i = 0; i < 12; ++i) Aout[((size_t)b * NJ + tid) * 12 + i] = (float)A[tid][i];
    }
    __syncthreads();
    const int v = blockIdx.x * RG_T + tid;
    if (v >= V) return;
    double vp[3];
    for (int c = 0; c < 3; ++c) {
        double acc = C.v_template[v * 3 + c];
        for (int l = 0; l < NB; ++l) acc += (double)C.shapedirs[((size_t)v * 3 + c) * NB + l] * xs[NPOSE + l];
        vp[c] = acc;
    }
    for (int e = 0; e < NPF; ++e) {
        const float* Pp = C.posedirs + (size_t)e * V * 3 + v * 3;
        vp[0] += pf[e] * (double)Pp[0]; vp[1] += pf[e] * (double)Pp[1]; vp[2] += pf[e] * (double)Pp[2];
    }
    double T[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < NJ; ++j) {
        const float w = C.weights[(size_t)v * NJ + j];
        if (w != 0.f)
            for (int i = 0; i < 12; ++i) T[i] += (double)w * A[j][i];
    }
    const double s = (double)pb[P - 1];
    const size_t o = (size_t)b * V + v;
    for (int a = 0; a < 3; ++a) {
        base[o * 3 + a] = (float)((T[a * 4] * vp[0] + T[a * 4 + 1] * vp[1] + T[a * 4 + 2] * vp[2] + T[a * 4 + 3] + (double)pb[3 * NJ + NB + a]) * s);
        for (int c = 0; c < 3; ++c) Rout[o * 9 + a * 3 + c] = (float)(s * T[a * 4 + c]);
    }
}

// ---------------------------------------------------------------------------------------------- apply, energy, gradient, update
// A workgroup owns RG_T consecutive vertices of one scan.  Their frames are one contiguous run of 9 RG_T floats: the workgroup copies it
// to LDS with unit-stride loads and a thread reads its own 9 from there (stride 9 words: odd, no bank conflict).
__device__ __forceinline__ void load_frames(float* lds, const float* __restrict__ R, size_t first, int count) {
    const float* src = R + first * 9;
    for (int e = threadIdx.x; e < count * 9; e += RG_T) lds[e] = src[e];
    __syncthreads();
}

__device__ __forceinline__ void apply_vertex(const float* __restrict__ base3, const float* Rv, const float d[3], float* __restrict__ out3) {
    for (int a = 0; a < 3; ++a) out3[a] = base3[a] + ((Rv[a * 3] * d[0] + Rv[a * 3 + 1] * d[1]) + Rv[a * 3 + 2] * d[2]);
}

__global__ void __launch_bounds__(RG_T) smpld_apply_kernel(int V, const float* __restrict__ base, const float* __restrict__ R, const float* __restrict__ D,
                                                           float* __restrict__ verts) {
    __shared__ float Rs[RG_T * 9];
    const int b = blockIdx.y, v0 = blockIdx.x * RG_T, v = v0 + threadIdx.x;
    load_frames(Rs, R, (size_t)b * V + v0, min(RG_T, V - v0));
    if (v >= V) return;
    const size_t o = ((size_t)b * V + v) * 3;
    const float d[3] = {D[o], D[o + 1], D[o + 2]};
    apply_vertex(base + o, Rs + threadIdx.x * 9, d, verts + o);
}

__device__ __forceinline__ int scan_len_of(const int* len, int b, int n) { return len ? min(max(len[b], 0), n) : n; }

// One workgroup per scan: the four terms from fixed-order fp64 sums (strided per thread, then a tree), and the per-point weight
// w_s2m / n_b that the scan -> body scatter applies.  trunc2 < 0: no mask.  The kernel is bound by the latency of its dependent loads
// (CSR pointer -> neighbour index -> neighbour offset) with one workgroup per scan on the device, hence the 1024 threads.
// nbr_idx holds 2 n_edges entries: here and in smpld_grad_kernel a list is cut to that range and a neighbour outside [0, V) is skipped, so
// no contents of the two arrays can make a read leave them.
#define TERMS_T 1024
__global__ void __launch_bounds__(TERMS_T) smpld_terms_kernel(int N, int V, const int* __restrict__ slen, const float* __restrict__ d_xy,
                                                           const float* __restrict__ d_yx, const int* __restrict__ idx_yx, const float* __restrict__ D,
                                                           const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx, int n_edges, float w_s2m,
                                                           float w_m2s, float lambda_s, float lambda_m, float trunc2, float* __restrict__ w_xy,
                                                           float* __restrict__ terms, float* __restrict__ trace, int iters, int it) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = scan_len_of(slen, b, N);
    __shared__ double sm[4][TERMS_T];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = tid; i < n; i += TERMS_T) a0 += (double)d_xy[(size_t)b * N + i];
    const float* Db = D + (size_t)b * V * 3;
    for (int v = tid; v < V; v += TERMS_T) {
        const float d = d_yx[(size_t)b * V + v];
        if (idx_yx[(size_t)b * V + v] >= 0 && (trunc2 < 0.f || d <= trunc2)) a1 += (double)d;
        const double x = Db[v * 3], y = Db[v * 3 + 1], z = Db[v * 3 + 2];
        a3 += x * x + y * y + z * z;
        for (int e = max(nbr_ptr[v], 0), e1 = min(nbr_ptr[v + 1], 2 * n_edges); e < e1; ++e) {          // every edge once, from its lower end
            const int u = nbr_idx[e];
            if (u > v && u < V) {
                const double dx = x - (double)Db[u * 3], dy = y - (double)Db[u * 3 + 1], dz = z - (double)Db[u * 3 + 2];
                a2 += dx * dx + dy * dy + dz * dz;
            }
        }
    }
    sm[0][tid] = a0; sm[1][tid] = a1; sm[2][tid] = a2; sm[3][tid] = a3;
    __syncthreads();
    for (int s = TERMS_T / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; ++k) sm[k][tid] += sm[k][tid + s];
        __syncthreads();
    }
    if (tid < 4) {
        double scale = (double)lambda_m / V;
        if (tid == 0) scale = n > 0 ? (double)w_s2m / n : 0.0;
        if (tid == 1) scale = (double)w_m2s / V;
        if (tid == 2) scale = n_edges > 0 ? (double)lambda_s / n_edges : 0.0;
        const float t = (float)(scale * sm[tid][0]);
        terms[b * 4 + tid] = t;
        if (trace) trace[((size_t)b * iters + it) * 4 + tid] = t;
        if (tid == 0) w_xy[b] = (float)scale;
    }
}

// dE/dD of one vertex, every neighbour and mask held fixed.  g_s2m = the scan -> body half that etch_chamfer_grad scattered and gathered
// (-2 w_s2m / n_b times the sum of x_i - y_v over the scan points that chose v).  The CSR gather of the neighbours' D is the one irregular read.
__global__ void __launch_bounds__(RG_T) smpld_grad_kernel(int N, int V, const float* __restrict__ R, const float* __restrict__ D, const float* __restrict__ verts,
                                                          const float* __restrict__ scan, const int* __restrict__ idx_yx, const float* __restrict__ d_yx,
                                                          const float* __restrict__ g_s2m, const int* __restrict__ nbr_ptr, const int* __restrict__ nbr_idx,
                                                          int n_edges, float w_m2s, float lambda_s, float lambda_m, float trunc2, float* __restrict__ grad) {
    __shared__ float Rs[RG_T * 9];
    const int b = blockIdx.y, v0 = blockIdx.x * RG_T, v = v0 + threadIdx.x;
    load_frames(Rs, R, (size_t)b * V + v0, min(RG_T, V - v0));
    if (v >= V) return;
    const size_t bv = (size_t)b * V + v, o = bv * 3;
    float g[3] = {g_s2m[o], g_s2m[o + 1], g_s2m[o + 2]};
    const int c = idx_yx[bv];
    if (c >= 0 && c < N && (trunc2 < 0.f || d_yx[bv] <= trunc2)) {
        const float* x = scan + ((size_t)b * N + c) * 3;
        const float w2 = 2.f * (w_m2s / (float)V);
        for (int a = 0; a < 3; ++a) g[a] += w2 * (verts[o + a] - x[a]);
    }
    const float* Db = D + (size_t)b * V * 3;
    const float d[3] = {Db[v * 3], Db[v * 3 + 1], Db[v * 3 + 2]};
    float s[3] = {0.f, 0.f, 0.f};
    for (int e = max(nbr_ptr[v], 0), e1 = min(nbr_ptr[v + 1], 2 * n_edges); e < e1; ++e) {
        const int u = nbr_idx[e];
        if (u >= 0 && u < V)
            for (int a = 0; a < 3; ++a) s[a] += d[a] - Db[u * 3 + a];
    }
    const float* Rv = Rs + threadIdx.x * 9;
    const float cs = n_edges > 0 ? 2.f * (lambda_s / (float)n_edges) : 0.f, cm = 2.f * (lambda_m / (float)V);
    for (int a = 0; a < 3; ++a) grad[o + a] = ((Rv[a] * g[0] + Rv[3 + a] * g[1]) + Rv[6 + a] * g[2]) + cs * s[a] + cm * d[a];
}

// torch.optim.Adam (single-tensor form, no weight decay), the formula of rf_adam_kernel (chamfer_fit.hip), on the three offsets of a vertex,
// then verts = base + R D of the updated offsets.
__global__ void __launch_bounds__(RG_T) smpld_adam_apply_kernel(int V, const float* __restrict__ base, const float* __restrict__ R, float* __restrict__ D,
                                                                const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ vv, float b1c, float b2,
                                                                float b2c, float step_size, float bc2s, float eps, float* __restrict__ verts) {
    __shared__ float Rs[RG_T * 9];
    const int b = blockIdx.y, v0 = blockIdx.x * RG_T, v = v0 + threadIdx.x;
    load_frames(Rs, R, (size_t)b * V + v0, min(RG_T, V - v0));
    if (v >= V) return;
    const size_t o = ((size_t)b * V + v) * 3;
    float d[3];
    for (int a = 0; a < 3; ++a) {
        const size_t t = o + a;
        const float gt = grad[t];
        const float mt = m[t] + b1c * (gt - m[t]);
        const float vt = vv[t] * b2 + b2c * (gt * gt);
        m[t] = mt; vv[t] = vt;
        const float denom = sqrtf(vt) / bc2s + eps;
        d[a] = D[t] + (-step_size) * (mt / denom);
        D[t] = d[a];
    }
    apply_vertex(base + o, Rs + threadIdx.x * 9, d, verts + o);
}

// ---------------------------------------------------------------------------------------------- carrying bound points
// One thread per point, fp64.  w~ = sum_k bary_k W[f_k]; T = sum_j w~_j A_j, T' = sum_j w~_j A'_j (3 x 4);
// x' = (T' T^-1 (x / scale - trans) + trans') scale'.  |det T^R| < 1e-10: T is the identity (animate.py:181-184).
// A point whose face or vertex index is out of range comes back as NaN; nothing is read out of bounds.
__global__ void __launch_bounds__(RG_T) skin_carry_kernel(int P, int F, int V, int NJ, const double* __restrict__ pts, const int* __restrict__ face,
                                                          const double* __restrict__ bary, const int* __restrict__ faces, const float* __restrict__ W,
                                                          const float* __restrict__ A0, const float* __restrict__ A1, const float* __restrict__ ts0,
                                                          const float* __restrict__ ts1, double* __restrict__ out) {
    __shared__ float As[2][SK_MAXJ * 12];
    for (int e = threadIdx.x; e < NJ * 12; e += RG_T) { As[0][e] = A0[e]; As[1][e] = A1[e]; }
    __syncthreads();
    const int p = blockIdx.x * RG_T + threadIdx.x;
    if (p >= P) return;
    const int f = face[p];
    int vid[3] = {-1, -1, -1};
    if (f >= 0 && f < F)
        for (int k = 0; k < 3; ++k) vid[k] = faces[(size_t)f * 3 + k];
    double* o = out + (size_t)p * 3;
    if (vid[0] < 0 || vid[0] >= V || vid[1] < 0 || vid[1] >= V || vid[2] < 0 || vid[2] >= V) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        o[0] = nan; o[1] = nan; o[2] = nan;
        return;
    }
    const double bw[3] = {bary[(size_t)p * 3], bary[(size_t)p * 3 + 1], bary[(size_t)p * 3 + 2]};
    double T[12], U[12];
    for (int i = 0; i < 12; ++i) { T[i] = 0.0; U[i] = 0.0; }
    for (int j = 0; j < NJ; ++j) {
        const double w = bw[0] * (double)W[(size_t)vid[0] * NJ + j] + bw[1] * (double)W[(size_t)vid[1] * NJ + j] + bw[2] * (double)W[(size_t)vid[2] * NJ + j];
        if (w != 0.0)
            for (int i = 0; i < 12; ++i) { T[i] += w * (double)As[0][j * 12 + i]; U[i] += w * (double)As[1][j * 12 + i]; }
    }
    // cofactors of T^R (rows a, columns c at T[a * 4 + c])
    const double c00 = T[5] * T[10] - T[6] * T[9], c01 = T[6] * T[8] - T[4] * T[10], c02 = T[4] * T[9] - T[5] * T[8];
    const double det = T[0] * c00 + T[1] * c01 + T[2] * c02;
    const double s0 = (double)ts0[3], s1 = (double)ts1[3];
    const double q[3] = {pts[(size_t)p * 3] / s0 - (double)ts0[0], pts[(size_t)p * 3 + 1] / s0 - (double)ts0[1], pts[(size_t)p * 3 + 2] / s0 - (double)ts0[2]};
    double r[3];
    if (fabs(det) < 1e-10) {
        r[0] = q[0]; r[1] = q[1]; r[2] = q[2];
    } else {
        const double y[3] = {q[0] - T[3], q[1] - T[7], q[2] - T[11]};
        const double c10 = T[2] * T[9] - T[1] * T[10], c11 = T[0] * T[10] - T[2] * T[8], c12 = T[1] * T[8] - T[0] * T[9];
        const double c20 = T[1] * T[6] - T[2] * T[5], c21 = T[2] * T[4] - T[0] * T[6], c22 = T[0] * T[5] - T[1] * T[4];
        r[0] = (c00 * y[0] + c10 * y[1] + c20 * y[2]) / det;          // inverse = adjugate / det = transposed cofactors / det
        r[1] = (c01 * y[0] + c11 * y[1] + c21 * y[2]) / det;
        r[2] = (c02 * y[0] + c12 * y[1] + c22 * y[2]) / det;
    }
    for (int a = 0; a < 3; ++a) o[a] = (U[a * 4] * r[0] + U[a * 4 + 1] * r[1] + U[a * 4 + 2] * r[2] + U[a * 4 + 3] + (double)ts1[a]) * s1;
}

// ---------------------------------------------------------------------------------------------- host side
static inline unsigned nblk(long n) { return (unsigned)((n + RG_T - 1) / RG_T); }
static inline size_t al(size_t n) { return (n + 255) & ~(size_t)255; }
static bool sk_supported(int nj, int nb) { return (nj == 24 && nb == 10) || (nj == 55 && nb == 20); }

struct RgWork {
    void *keys, *acc;
    float *d_xy, *d_yx, *g_s2m, *grad, *m, *v, *w_xy;
    int *idx_xy, *idx_yx;
    size_t bytes;
};

static RgWork rg_layout(char* base, int B, int N, int V) {
    RgWork w;
    size_t off = 0;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += al(n); return p; };
    w.keys = take((size_t)B * (N + V) * 8);               // etch_nn_bidir's
    w.acc = take((size_t)B * (N + V) * 24);               // etch_chamfer_grad's
    w.d_xy = (float*)take((size_t)B * N * 4);
    w.d_yx = (float*)take((size_t)B * V * 4);
    w.g_s2m = (float*)take((size_t)B * V * 12);
    w.grad = (float*)take((size_t)B * V * 12);
    w.m = (float*)take((size_t)B * V * 12);
    w.v = (float*)take((size_t)B * V * 12);
    w.w_xy = (float*)take((size_t)B * 4);
    w.idx_xy = (int*)take((size_t)B * N * 4);
    w.idx_yx = (int*)take((size_t)B * V * 4);
    w.bytes = off;
    return w;
}

struct RgProblem {
    int B, N, V, n_edges;
    const float *base, *R, *scan;
    const int *scan_len, *nbr_ptr, *nbr_idx;
    float w_s2m, w_m2s, lambda_m, trunc2;
};

// verts must hold base + R D.  Queues: neighbours, the four terms, the scan -> body scatter, the per-vertex gradient.
static int rg_evaluate(const RgProblem& q, const RgWork& w, const float* D, const float* verts, float lambda_s, int* idx_xy, int* idx_yx, float* terms,
                       float* trace, int iters, int it, float* grad, hipStream_t st) {
    int e = etch_nn_bidir(q.B, q.N, q.V, q.scan, verts, q.scan_len, nullptr, w.keys, idx_xy, w.d_xy, idx_yx, w.d_yx, st);
    if (e) return e;
    hipLaunchKernelGGL(smpld_terms_kernel, dim3(q.B), dim3(TERMS_T), 0, st, q.N, q.V, q.scan_len, w.d_xy, w.d_yx, idx_yx, D, q.nbr_ptr, q.nbr_idx, q.n_edges, q.w_s2m,
                       q.w_m2s, lambda_s, q.lambda_m, q.trunc2, w.w_xy, terms, trace, iters, it);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (!grad) return ETCH_OK;
    e = etch_chamfer_grad(q.B, q.N, q.V, q.scan, verts, q.scan_len, nullptr, idx_xy, idx_yx, w.w_xy, nullptr, w.acc, nullptr, w.g_s2m, st);
    if (e) return e;
    hipLaunchKernelGGL(smpld_grad_kernel, dim3((q.V + RG_T - 1) / RG_T, q.B), dim3(RG_T), 0, st, q.N, q.V, q.R, D, verts, q.scan, idx_yx, w.d_yx, w.g_s2m, q.nbr_ptr,
                       q.nbr_idx, q.n_edges, q.w_m2s, lambda_s, q.lambda_m, q.trunc2, grad);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

static inline float rg_trunc2(float trunc) { return trunc < 0.f ? -1.f : (float)((double)trunc * (double)trunc); }

extern "C" {

int etch_smpl_skin_frames(int B, int V, int nj, int nb, const void* const* consts, const float* params, float* base, float* R, float* A, void* stream) {
    if (B < 0 || V <= 0) return ETCH_EINVAL;
    if (!sk_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (B == 0) return ETCH_OK;
    const SkinConsts C{(const float*)consts[0], (const float*)consts[1], (const float*)consts[2], (const float*)consts[3], (const float*)consts[4],
                       (const float*)consts[5], (const int*)consts[6]};
    hipLaunchKernelGGL(skin_frames_kernel, dim3((V + RG_T - 1) / RG_T, B), dim3(RG_T), 0, (hipStream_t)stream, C, nj, nb, V, params, base, R, A);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_smpld_apply(int B, int V, const float* base, const float* R, const float* D, float* verts, void* stream) {
    if (B < 0 || V <= 0) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    hipLaunchKernelGGL(smpld_apply_kernel, dim3((V + RG_T - 1) / RG_T, B), dim3(RG_T), 0, (hipStream_t)stream, V, base, R, D, verts);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_smpld_register_workspace(int B, int N, int V, long long* bytes) {
    if (B < 0 || N < 0 || V < 0) return ETCH_EINVAL;
    *bytes = (long long)rg_layout(nullptr, B, N, V).bytes;
    return ETCH_OK;
}

int etch_smpld_energy_grad(int B, int N, int V, const float* base, const float* R, const float* D, const float* scan, const int* scan_len, const int* nbr_ptr,
                           const int* nbr_idx, int n_edges, float w_s2m, float w_m2s, float lambda_s, float lambda_m, float trunc, void* workspace, float* terms,
                           float* grad, float* verts, int* idx_xy, int* idx_yx, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || n_edges < 0) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const RgWork w = rg_layout((char*)workspace, B, N, V);
    const RgProblem q{B, N, V, n_edges, base, R, scan, scan_len, nbr_ptr, nbr_idx, w_s2m, w_m2s, lambda_m, rg_trunc2(trunc)};
    int e = etch_smpld_apply(B, V, base, R, D, verts, st);
    if (e) return e;
    return rg_evaluate(q, w, D, verts, lambda_s, idx_xy, idx_yx, terms, nullptr, 0, 0, grad, st);
}

int etch_smpld_register(int B, int N, int V, const float* base, const float* R, const float* scan, const int* scan_len, const int* nbr_ptr, const int* nbr_idx,
                        int n_edges, int iters, const float* lambda_s, float lambda_m, float w_s2m, float w_m2s, float trunc, float lr, float* D, float* verts,
                        float* energy, float* trace, void* workspace, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || n_edges < 0 || iters < 1 || !lambda_s) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const RgWork w = rg_layout((char*)workspace, B, N, V);
    const RgProblem q{B, N, V, n_edges, base, R, scan, scan_len, nbr_ptr, nbr_idx, w_s2m, w_m2s, lambda_m, rg_trunc2(trunc)};
    const long n3 = 3L * B * V;
    const double beta1 = 0.9, beta2 = 0.999;
    if (hipMemsetAsync(w.m, 0, (size_t)n3 * 4, st) != hipSuccess || hipMemsetAsync(w.v, 0, (size_t)n3 * 4, st) != hipSuccess)      // Adam moments start at zero
        return (int)hipGetLastError();
    int e = etch_smpld_apply(B, V, base, R, D, verts, st);
    if (e) return e;
    double bp1 = 1.0, bp2 = 1.0;
    for (int it = 0; it < iters; ++it) {
        // the whole gradient of step `it` is taken at the iterate before it: D is read-only until the update kernel
        e = rg_evaluate(q, w, D, verts, lambda_s[it], w.idx_xy, w.idx_yx, energy, trace, iters, it, w.grad, st);
        if (e) return e;
        bp1 *= beta1; bp2 *= beta2;
        const double bc1 = 1.0 - bp1, bc2 = 1.0 - bp2;
        hipLaunchKernelGGL(smpld_adam_apply_kernel, dim3((V + RG_T - 1) / RG_T, B), dim3(RG_T), 0, st, V, base, R, D, w.grad, w.m, w.v, (float)(1.0 - beta1),
                           (float)beta2, (float)(1.0 - beta2), (float)((double)lr / bc1), (float)sqrt(bc2), 1e-8f, verts);
        ETCH_RETURN_IF_LAUNCH_FAILED();
    }
    // the returned energy: one more forward at the final offsets, with the last smoothness weight
    return rg_evaluate(q, w, D, verts, lambda_s[iters - 1], w.idx_xy, w.idx_yx, energy, nullptr, 0, 0, nullptr, st);
}

int etch_skin_carry(int P, int F, int V, int nj, const double* points, const int* face, const double* bary, const int* faces, const float* W, const float* A,
                    const float* A_new, const float* trans_scale, const float* trans_scale_new, double* out, void* stream) {
    if (P < 0 || F <= 0 || V <= 0 || nj < 1 || nj > SK_MAXJ) return ETCH_EINVAL;
    if (P == 0) return ETCH_OK;
    hipLaunchKernelGGL(skin_carry_kernel, dim3(nblk(P)), dim3(RG_T), 0, (hipStream_t)stream, P, F, V, nj, points, face, bary, faces, W, A, A_new, trans_scale,
                       trans_scale_new, out);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
