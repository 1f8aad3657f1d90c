// Chamfer refinement of a fitted SMPL body against its scan on gfx950 (the inference-time step after the marker fit):
//
//   etch_nn_bidir            exact brute-force nearest neighbours between two batched clouds, BOTH directions in one pass
//   etch_chamfer_grad        the gradient of sum_i w_x d(x_i, NN_y(x_i)) + sum_j w_y d(y_j, NN_x(y_j)) w.r.t. both clouds
//   etch_smpl_lbs_vjp        reverse mode of verts = (LBS(pose, beta) + trans) * scale over the FULL mesh
//   etch_smpl_chamfer_refine the whole Adam schedule (forward, neighbours, loss, VJP, update) queued on one stream
//
// Determinism: every reduction has a fixed order; the only atomics are 64-bit INTEGER ones -- atomicMin on (distance bits, index) keys,
// whose result is the same in any order, and atomicAdd of fixed-point differences (2^-40 m), which is exact and so order-free too.
// The TU is built with -ffp-contract=off: distances are etch_sqdist's bit-defined ((dx*dx)+(dy*dy))+(dz*dz).
#include "etch_hip.h"
#include "refine_common.h"

// ---------------------------------------------------------------------------------------------- nearest neighbours
// One wave per (scan, 1024-row block, 256-column block).  A lane keeps NN_R = 16 rows in registers (rows r0 + 64 r + lane), the block's
// columns sit in LDS and are read as wave-uniform broadcasts.  Per column: the 16 distances update the rows' running minima (registers)
// and the lane's own column minimum; a 6-step butterfly gives the wave's column minimum, which lane (c mod 64) keeps until 64 columns
// are done and then merges into the global key with one atomicMin per lane.  Rows are merged the same way after the last column.
// Key = (fp32 bits of the distance) << 32 | index: distances are >= 0, so the integer order is (distance, index) -- the minimum is
// the smallest distance and, among exact ties, the LOWEST index.
#define NN_R 16
#define NN_ROWS (64 * NN_R)
#define NN_COLS 256

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(64) nn_tile_kernel(int N, int V, const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ xlen,
                                                     const int* __restrict__ ylen, u64* __restrict__ xkey, u64* __restrict__ ykey) {
    const int b = blockIdx.z, lane = threadIdx.x;
    const int nx = clamp_len(xlen, b, N), ny = clamp_len(ylen, b, V);
    const int r0 = blockIdx.y * NN_ROWS, c0 = blockIdx.x * NN_COLS;
    if (r0 >= nx || c0 >= ny) return;                 // uniform: padding is never read
    const int cn = min(NN_COLS, ny - c0);
    __shared__ float4 ys[NN_COLS];
    const float* Yb = Y + ((size_t)b * V + c0) * 3;
    for (int c = lane; c < cn; c += 64) ys[c] = make_float4(Yb[c * 3], Yb[c * 3 + 1], Yb[c * 3 + 2], 0.f);
    __syncthreads();
    const float INF = __int_as_float(0x7f800000);
    float px[NN_R], py[NN_R], pz[NN_R], best[NN_R];
    int bi[NN_R];
    const float* Xb = X + (size_t)b * N * 3;
#pragma unroll
    for (int r = 0; r < NN_R; ++r) {
        const int i = r0 + r * 64 + lane;
        const bool ok = i < nx;                       // rows past the length sit at infinity: every distance is +inf, never below a real one
        px[r] = ok ? Xb[(size_t)i * 3] : INF;
        py[r] = ok ? Xb[(size_t)i * 3 + 1] : INF;
        pz[r] = ok ? Xb[(size_t)i * 3 + 2] : INF;
        best[r] = INF;
        bi[r] = -1;
    }
    for (int cb = 0; cb < cn; cb += 64) {
        const int ce = min(64, cn - cb);
        u64 mine = ~0ull;
        for (int cc = 0; cc < ce; ++cc) {
            const float4 q = ys[cb + cc];
            const int col = c0 + cb + cc;
            float cm = INF;
            int ci = -1;
#pragma unroll
            for (int r = 0; r < NN_R; ++r) {          // ascending r = ascending row index: strict < keeps the lowest index of a tie
                const float d = etch_sqdist(px[r], py[r], pz[r], q.x, q.y, q.z);
                if (d < best[r]) { best[r] = d; bi[r] = col; }
                if (d < cm) { cm = d; ci = r; }
            }
            u64 key = ((u64)__float_as_uint(cm) << 32) | (unsigned)(ci < 0 ? -1 : r0 + ci * 64 + lane);
            key = wave_min_u64(key);
            if (lane == cc) mine = key;
        }
        if (lane < ce) atomicMin(ykey + (size_t)b * V + c0 + cb + lane, mine);
    }
#pragma unroll
    for (int r = 0; r < NN_R; ++r) {
        const int i = r0 + r * 64 + lane;
        if (i < nx && bi[r] >= 0) atomicMin(xkey + (size_t)b * N + i, ((u64)__float_as_uint(best[r]) << 32) | (unsigned)bi[r]);
    }
}

// keys -> index (int32, -1 for padding) and the exact fp32 distance of the chosen pair, recomputed from the two points
__global__ void __launch_bounds__(256) nn_final_kernel(int B, int N, int V, const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ xlen,
                                                       const int* __restrict__ ylen, const u64* __restrict__ xkey, const u64* __restrict__ ykey,
                                                       int* __restrict__ idx_xy, float* __restrict__ d_xy, int* __restrict__ idx_yx, float* __restrict__ d_yx) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nxt = (long)B * N;
    if (t >= nxt + (long)B * V) return;
    const bool xs = t < nxt;
    const long u = xs ? t : t - nxt;
    const int M = xs ? N : V, Mo = xs ? V : N;
    const int b = (int)(u / M), i = (int)(u % M);
    const int nself = clamp_len(xs ? xlen : ylen, b, M), nother = clamp_len(xs ? ylen : xlen, b, Mo);
    const unsigned j = (unsigned)(xs ? xkey[u] : ykey[u]);
    int oi = -1;
    float od = 0.f;
    if (i < nself && j < (unsigned)nother) {
        const float* p = (xs ? X : Y) + u * 3;
        const float* q = (xs ? Y : X) + ((size_t)b * Mo + j) * 3;
        oi = (int)j;
        od = etch_sqdist(p[0], p[1], p[2], q[0], q[1], q[2]);
    }
    if (xs) { idx_xy[u] = oi; d_xy[u] = od; }
    else { idx_yx[u] = oi; d_yx[u] = od; }
}

// ---------------------------------------------------------------------------------------------- chamfer gradient
// d/dx_i of w_x(b) d(x_i, y_nn(i)) is 2 w_x (x_i - y_nn(i)) (the point's own term); the neighbour receives the negative.  The scatter
// half accumulates the differences (x_i - y_j) per target in 64-bit fixed point (2^-40 m, exact while |sum| < 2^23 m), so the sum does
// not depend on the order the atomics land in.

__global__ void __launch_bounds__(256) cham_scatter_kernel(int B, int N, int V, const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ xlen,
                                                           const int* __restrict__ ylen, const int* __restrict__ idx_xy, const int* __restrict__ idx_yx,
                                                           int use_xy, int use_yx, unsigned long long* __restrict__ acc_x, unsigned long long* __restrict__ acc_y) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nxt = (long)B * N;
    if (t >= nxt + (long)B * V) return;
    const bool xs = t < nxt;
    if (xs ? !use_xy : !use_yx) return;
    const long u = xs ? t : t - nxt;
    const int M = xs ? N : V, Mo = xs ? V : N;
    const int b = (int)(u / M), i = (int)(u % M);
    if (i >= clamp_len(xs ? xlen : ylen, b, M)) return;
    const int j = xs ? idx_xy[u] : idx_yx[u];
    if (j < 0) return;
    const float* p = (xs ? X : Y) + u * 3;
    const float* q = (xs ? Y : X) + ((size_t)b * Mo + j) * 3;
    unsigned long long* a = (xs ? acc_y : acc_x) + ((size_t)b * Mo + j) * 3;
    for (int c = 0; c < 3; ++c) atomicAdd(a + c, (unsigned long long)__double2ll_rn((double)(p[c] - q[c]) * CHAM_FIX));
}

__global__ void __launch_bounds__(256) cham_gather_kernel(int B, int N, int V, const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ xlen,
                                                          const int* __restrict__ ylen, const int* __restrict__ idx_xy, const int* __restrict__ idx_yx,
                                                          const float* __restrict__ w_xy, const float* __restrict__ w_yx, const unsigned long long* __restrict__ acc_x,
                                                          const unsigned long long* __restrict__ acc_y, float* __restrict__ gx, float* __restrict__ gy) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nxt = (long)B * N;
    if (t >= nxt + (long)B * V) return;
    const bool xs = t < nxt;
    float* g = xs ? gx : gy;
    if (!g) return;
    const long u = xs ? t : t - nxt;
    const int M = xs ? N : V, Mo = xs ? V : N;
    const int b = (int)(u / M), i = (int)(u % M);
    float o[3] = {0.f, 0.f, 0.f};
    if (i < clamp_len(xs ? xlen : ylen, b, M)) {
        const float* wown = xs ? w_xy : w_yx;          // this point's own distance term
        const float* woth = xs ? w_yx : w_xy;          // the other cloud's terms that chose this point
        const int j = xs ? idx_xy[u] : idx_yx[u];
        const float* p = (xs ? X : Y) + u * 3;
        if (wown && j >= 0) {
            const float* q = (xs ? Y : X) + ((size_t)b * Mo + j) * 3;
            const float w2 = 2.f * wown[b];
            for (int c = 0; c < 3; ++c) o[c] = w2 * (p[c] - q[c]);
        }
        if (woth) {
            const unsigned long long* a = (xs ? acc_x : acc_y) + u * 3;
            const double w2 = 2.0 * (double)woth[b];
            for (int c = 0; c < 3; ++c) o[c] = (float)((double)o[c] - w2 * ((double)(long long)a[c] / CHAM_FIX));
        }
    }
    g[u * 3] = o[0]; g[u * 3 + 1] = o[1]; g[u * 3 + 2] = o[2];
}

// ---------------------------------------------------------------------------------------------- refinement: loss and update
// One workgroup per scan.  S1 = sum over the scan's points of their distance to the mesh, S2 = sum over the vertices; data term
// sqrt(S1) + sqrt(S2) (bidir 0), sqrt(S1) (1) or sqrt(S2) (-1); + 1e-8 prior(pose[3:]) + 0.2 mean(beta^2).  S = 0 (a scan lying exactly on
// the mesh) gives a weight of +inf and NaN gradients, as autograd through sqrt at 0 does; fit_cham rejects empty scans.  Writes the per-point
// weights of the distance terms (d sqrt(S) / dS = 0.5 / sqrt(S)) and resets grad to the regulariser's and the prior's gradient.
#define RF_PRIOR_D 69
#define RF_MAXG 16
__global__ void __launch_bounds__(256) rf_loss_kernel(int N, int V, int NJ, int NB, const int* __restrict__ slen, const float* __restrict__ d_xy,
                                                      const float* __restrict__ d_yx, const float* __restrict__ params, const float* __restrict__ means,
                                                      const float* __restrict__ prec, const float* __restrict__ nllw, int G, int bidir,
                                                      float* __restrict__ w_xy, float* __restrict__ w_yx, float* __restrict__ grad,
                                                      float* __restrict__ trace, int iters, int it, float* __restrict__ loss_last) {
    const int b = blockIdx.x, tid = threadIdx.x, P = 3 * NJ + NB + 4;
    const int n = clamp_len(slen, b, N);
    __shared__ double s1[256], s2[256];
    __shared__ double Pd[RF_MAXG][RF_PRIOR_D], PTd[RF_MAXG][RF_PRIOR_D], dd[RF_MAXG][RF_PRIOR_D];
    __shared__ int gbest;
    double a1 = 0.0, a2 = 0.0;
    for (int i = tid; i < n; i += 256) a1 += (double)d_xy[(size_t)b * N + i];
    for (int v = tid; v < V; v += 256) a2 += (double)d_yx[(size_t)b * V + v];
    s1[tid] = a1; s2[tid] = a2;
    const float* pb = params + (size_t)b * P;
    for (int t = tid; t < G * RF_PRIOR_D; t += 256) dd[t / RF_PRIOR_D][t % RF_PRIOR_D] = (double)pb[3 + t % RF_PRIOR_D] - (double)means[t];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { s1[tid] += s1[tid + s]; s2[tid] += s2[tid + s]; }
        __syncthreads();
    }
    for (int t = tid; t < G * RF_PRIOR_D; t += 256) {
        const int g = t / RF_PRIOR_D, r = t % RF_PRIOR_D;
        const float* Pg = prec + (size_t)g * RF_PRIOR_D * RF_PRIOR_D;
        double a = 0.0, c = 0.0;
        for (int k = 0; k < RF_PRIOR_D; ++k) { a += (double)Pg[r * RF_PRIOR_D + k] * dd[g][k]; c += (double)Pg[k * RF_PRIOR_D + r] * dd[g][k]; }
        Pd[g][r] = a; PTd[g][r] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int gb = -1;
        double qb = 0.0;
        for (int g = 0; g < G; ++g) {                  // merged_log_likelihood: min_g 0.5 d^T P_g d - log w_g (first minimum)
            double q = 0.0;
            for (int r = 0; r < RF_PRIOR_D; ++r) q += dd[g][r] * Pd[g][r];
            q = 0.5 * q - log((double)nllw[g]);
            if (gb < 0 || q < qb) { gb = g; qb = q; }
        }
        gbest = gb;
        const double S1 = s1[0], S2 = s2[0];
        const double d1 = sqrt(S1), d2 = sqrt(S2);
        double data = bidir == 1 ? d1 : bidir == -1 ? d2 : d1 + d2;
        double reg = 0.0;
        for (int l = 0; l < NB; ++l) reg += (double)pb[3 * NJ + l] * (double)pb[3 * NJ + l];
        const double loss = data + (G > 0 ? 1e-8 * qb : 0.0) + 0.2 * (reg / NB);
        if (trace) trace[(size_t)b * iters + it] = (float)loss;
        loss_last[b] = (float)loss;
        if (w_xy) w_xy[b] = (float)(0.5 / d1);
        if (w_yx) w_yx[b] = (float)(0.5 / d2);
    }
    __syncthreads();
    float* gr = grad + (size_t)b * P;
    for (int k = tid; k < P; k += 256) {
        double g = 0.0;
        if (k >= 3 * NJ && k < 3 * NJ + NB) g = 0.4 * (double)pb[k] / NB;
        if (G > 0 && k >= 3 && k < 3 + RF_PRIOR_D) g = 1e-8 * 0.5 * (Pd[gbest][k - 3] + PTd[gbest][k - 3]);
        gr[k] = (float)g;
    }
}

// ---------------------------------------------------------------------------------------------- host side

struct RfWork : RfCore {
    float *verts, *gy, *grad, *m, *v, *w_xy, *w_yx, *d_xy, *d_yx;
    int *idx_xy, *idx_yx;
    u64* keys;
    unsigned long long* acc;
    size_t bytes;
};

static RfWork rf_layout(char* base, int B, int N, int V, int nj, int nb, int n_extra) {
    RfWork w;
    size_t off = 0;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += al(n); return p; };
    const int DOF = 3 * nj + nb + 3, P = DOF + 1, K = 12 * nj + nb + 9 * (nj - 1) + 4;
    w.x = (float*)take((size_t)B * DOF * 4);
    w.u = (float*)take((size_t)B * V * 12);
    w.verts = (float*)take((size_t)B * V * 12);
    w.jtmp = (float*)take((size_t)B * (nj + n_extra) * 12);
    w.gy = (float*)take((size_t)B * V * 12);
    w.h = (float*)take((size_t)B * V * 12);
    w.vp = (float*)take((size_t)B * V * 12);
    w.dvp = (float*)take((size_t)B * V * 12);
    w.gu = (float*)take((size_t)B * V * 4);
    w.grad = (float*)take((size_t)B * P * 4);
    w.m = (float*)take((size_t)B * P * 4);
    w.v = (float*)take((size_t)B * P * 4);
    w.w_xy = (float*)take((size_t)B * 4);
    w.w_yx = (float*)take((size_t)B * 4);
    w.d_xy = (float*)take((size_t)B * N * 4);
    w.d_yx = (float*)take((size_t)B * V * 4);
    w.idx_xy = (int*)take((size_t)B * N * 4);
    w.idx_yx = (int*)take((size_t)B * V * 4);
    w.keys = (u64*)take((size_t)B * (N + V) * 8);
    w.acc = (unsigned long long*)take((size_t)B * (N + V) * 24);
    w.red = (double*)take((size_t)B * K * 8);
    w.bytes = off;
    return w;
}

extern "C" {
int etch_smpl_lbs(int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* x, float* verts, float* joints, void* stream);

int etch_nn_bidir(int B, int N, int V, const float* X, const float* Y, const int* x_len, const int* y_len, void* workspace, int* idx_xy, float* d_xy,
                  int* idx_yx, float* d_yx, void* stream) {
    if (B < 0 || N < 0 || V < 0) return ETCH_EINVAL;
    if (B == 0 || (long)N + V == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    u64* xkey = (u64*)workspace;
    u64* ykey = xkey + (size_t)B * N;
    const long nk = (long)B * (N + V);
    hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(nk), 4096)), dim3(256), 0, st, nk, xkey, ~0ull);
    if (N > 0 && V > 0)
        hipLaunchKernelGGL(nn_tile_kernel, dim3((V + NN_COLS - 1) / NN_COLS, (N + NN_ROWS - 1) / NN_ROWS, B), dim3(64), 0, st, N, V, X, Y, x_len, y_len, xkey, ykey);
    hipLaunchKernelGGL(nn_final_kernel, dim3(nblk(nk)), dim3(256), 0, st, B, N, V, X, Y, x_len, y_len, xkey, ykey, idx_xy, d_xy, idx_yx, d_yx);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_chamfer_grad(int B, int N, int V, const float* X, const float* Y, const int* x_len, const int* y_len, const int* idx_xy, const int* idx_yx,
                      const float* w_xy, const float* w_yx, void* workspace, float* gx, float* gy, void* stream) {
    if (B < 0 || N < 0 || V < 0) return ETCH_EINVAL;
    if (B == 0 || (long)N + V == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* acc_x = (unsigned long long*)workspace;
    unsigned long long* acc_y = acc_x + (size_t)B * N * 3;
    const long nk = (long)B * (N + V);
    const long nax = 3L * B * N, nay = 3L * B * V;
    if (gx && nax) hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(nax), 4096)), dim3(256), 0, st, nax, (u64*)acc_x, 0ull);
    if (gy && nay) hipLaunchKernelGGL(u64_fill_kernel, dim3(std::min<long>(nblk(nay), 4096)), dim3(256), 0, st, nay, (u64*)acc_y, 0ull);
    // an x point's term scatters into the y side (needed only for gy), a y point's into the x side (only for gx)
    hipLaunchKernelGGL(cham_scatter_kernel, dim3(nblk(nk)), dim3(256), 0, st, B, N, V, X, Y, x_len, y_len, idx_xy, idx_yx, w_xy != nullptr && gy != nullptr,
                       w_yx != nullptr && gx != nullptr,
                       acc_x, acc_y);
    hipLaunchKernelGGL(cham_gather_kernel, dim3(nblk(nk)), dim3(256), 0, st, B, N, V, X, Y, x_len, y_len, idx_xy, idx_yx, w_xy, w_yx, acc_x, acc_y, gx, gy);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_smpl_chamfer_refine_workspace(int B, int N, int V, int nj, int nb, int n_extra, long long* bytes) {
    if (B < 0 || N < 0 || V < 0 || !rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    *bytes = (long long)rf_layout(nullptr, B, N, V, nj, nb, n_extra).bytes;
    return ETCH_OK;
}

int etch_smpl_lbs_vjp(int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* params, const float* g, void* workspace, float* grad,
                      void* stream) {
    if (B < 0 || V <= 0) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (B == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const RfWork w = rf_layout((char*)workspace, B, 0, V, nj, nb, n_extra);
    int e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, nullptr, nullptr, 0, st);
    if (e) return e;
    const long P = 3 * nj + nb + 4;
    hipLaunchKernelGGL(f32_zero_kernel, dim3(nblk(B * P)), dim3(256), 0, st, B * P, grad);
    return rf_vjp(w, B, V, nj, nb, consts, params, g, grad, st);
}

int etch_smpl_chamfer_refine(int B, int N, int V, int nj, int nb, int n_extra, const void* const* consts, const float* scan, const int* scan_len,
                             const void* const* prior, int n_gauss, int bidir, int iters, float lr, float beta1, float beta2, float eps, float* params,
                             float* verts, float* joints, float* loss_trace, float* loss_last, void* workspace, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || iters < 1 || bidir < -1 || bidir > 1 || n_gauss < 0 || n_gauss > RF_MAXG) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (n_gauss > 0 && (nj != 24 || !prior)) return ETCH_EUNSUPPORTED;      // the GMM prior is over the 69-dim SMPL body pose only
    if (B == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const RfWork w = rf_layout((char*)workspace, B, N, V, nj, nb, n_extra);
    const long P = 3 * nj + nb + 4;
    const float* means = n_gauss ? (const float*)prior[0] : nullptr;
    const float* prec = n_gauss ? (const float*)prior[1] : nullptr;
    const float* nllw = n_gauss ? (const float*)prior[2] : nullptr;
    hipLaunchKernelGGL(f32_zero_kernel, dim3(nblk(B * P)), dim3(256), 0, st, B * P, w.m);      // Adam moments start at zero
    hipLaunchKernelGGL(f32_zero_kernel, dim3(nblk(B * P)), dim3(256), 0, st, B * P, w.v);
    float* wx = bidir != -1 ? w.w_xy : nullptr;
    float* wy = bidir != 1 ? w.w_yx : nullptr;
    double bp1 = 1.0, bp2 = 1.0;
    for (int it = 0; it < iters; ++it) {
        int e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, w.verts, nullptr, 0, st);
        if (!e) e = etch_nn_bidir(B, N, V, scan, w.verts, scan_len, nullptr, w.keys, w.idx_xy, w.d_xy, w.idx_yx, w.d_yx, st);
        if (e) return e;
        hipLaunchKernelGGL(rf_loss_kernel, dim3(B), dim3(256), 0, st, N, V, nj, nb, scan_len, w.d_xy, w.d_yx, params, means, prec, nllw, n_gauss, bidir,
                           wx, wy, w.grad, loss_trace, iters, it, loss_last);
        ETCH_RETURN_IF_LAUNCH_FAILED();
        e = etch_chamfer_grad(B, N, V, scan, w.verts, scan_len, nullptr, w.idx_xy, w.idx_yx, wx, wy, w.acc, nullptr, w.gy, st);
        if (!e) e = rf_vjp(w, B, V, nj, nb, consts, params, w.gy, w.grad, st);
        if (e) return e;
        e = rf_adam_step(it, iters, lr, beta1, beta2, eps, bp1, bp2, (long)B * P, params, w.grad, w.m, w.v, st);
        if (e) return e;
    }
    int e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, verts, nullptr, 0, st);
    if (!e) e = rf_forward(w, B, V, nj, nb, n_extra, consts, params, nullptr, joints, 1, st);   // joints without trans and scale, as the script
    return e;
}

}  // extern "C"
