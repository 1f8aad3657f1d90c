// Dense surface refinement on gfx950: fit the body SURFACE (not its vertices) to all predicted inner points.
//
//   etch_point_mesh_closest      exact closest point of a batch of meshes (shared faces) to batched, ragged point sets, fp32
//   etch_point_mesh_energy_grad  sum_i w_i m_i d2_i, sum_i w_i m_i and the gradient of the dense (+ marker) term w.r.t. the vertices
//   etch_smpl_surface_refine     the whole Adam schedule (forward, closest points, loss, gradient, LBS VJP, update) queued on one stream
//
// The kernels are in surface_common.h (containment.hip builds the same refinement with one more term); this file is their C ABI.
// The TU is built with -ffp-contract=off: the region test is closest_tri.h's, bit-defined in fp32 (tests/_surface_oracle.py restates it).
#include "etch_hip.h"
#include "surface_common.h"

extern "C" {

int etch_point_mesh_closest_workspace(int B, int N, long long* bytes) {
    if (B < 0 || N < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)B * N * 8;
    return ETCH_OK;
}

int etch_point_mesh_closest(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, void* workspace, int* face,
                            float* bary, float* d2, void* stream) {
    if (B < 0 || N < 0 || V < 0 || F < 0) return ETCH_EINVAL;
    if (B == 0 || N == 0) return ETCH_OK;
    if (!workspace || !points || !face || !bary || !d2 || (F > 0 && (!verts || !faces))) return ETCH_EINVAL;
    return pm_closest(B, N, V, F, points, n_len, verts, faces, (u64*)workspace, face, bary, d2, (hipStream_t)stream);
}

int etch_point_mesh_energy_grad_workspace(int B, int V, long long* bytes) {
    if (B < 0 || V < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)(2 * al((size_t)B * V * 24) + al((size_t)B * 16));
    return ETCH_OK;
}

int etch_point_mesh_energy_grad(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, const int* face,
                                const float* bary, const float* d2, const float* weights, float trunc, const float* coef, float w_dense, int normalize, int M,
                                const int* marker_vids, const float* markers, const float* marker_valid, float w_marker, void* workspace, double* terms,
                                float* g, float* gp, void* stream) {
    if (B < 0 || N < 0 || V < 0 || F < 0 || M < 0 || !terms) return ETCH_EINVAL;
    if (M > 0 && (!marker_vids || !markers || !marker_valid)) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    if (!workspace) return ETCH_EINVAL;
    char* base = (char*)workspace;
    unsigned long long* acc = (unsigned long long*)base;
    unsigned long long* macc = (unsigned long long*)(base + al((size_t)B * V * 24));
    double* mterms = (double*)(base + 2 * al((size_t)B * V * 24));
    return pm_energy_grad(B, N, V, F, points, n_len, verts, faces, face, bary, d2, weights, trunc, coef, w_dense, normalize,
                          PmMarkers{M, marker_vids, markers, marker_valid, w_marker}, acc, macc, terms, mterms, V > 0 ? g : nullptr, gp, (hipStream_t)stream);
}

int etch_smpl_surface_refine_workspace(int B, int N, int V, int nj, int nb, int n_extra, long long* bytes) {
    if (B < 0 || N < 0 || V < 0 || !bytes) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    *bytes = (long long)sf_layout(nullptr, B, N, V, nj, nb, n_extra).bytes;
    return ETCH_OK;
}

int etch_smpl_surface_refine(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces, const float* points,
                             const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers, const float* marker_valid,
                             const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2, float eps, float w_dense, float w_marker,
                             float w_beta, float w_prior, float trunc, int optimize_scale, float* params, float* verts, float* joints, float* loss_trace,
                             float* loss_last, void* workspace, void* stream) {
    if (B < 0 || N <= 0 || V <= 0 || F <= 0 || M < 0 || iters < 1 || n_gauss < 0 || n_gauss > SF_MAXG) return ETCH_EINVAL;
    if (M > 0 && (!marker_vids || !markers || !marker_valid)) return ETCH_EINVAL;
    if (!rf_supported(nj, nb)) return ETCH_EUNSUPPORTED;
    if (n_gauss > 0 && (nj != 24 || !prior)) return ETCH_EUNSUPPORTED;      // the GMM prior is over the 69-dim SMPL body pose only
    if (B == 0) return ETCH_OK;
    if (!workspace || !params || !verts || !joints || !loss_last) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const SfWork w = sf_layout((char*)workspace, B, N, V, nj, nb, n_extra);
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
        hipLaunchKernelGGL(sf_loss_kernel, dim3(B), dim3(256), 0, st, nj, nb, w.terms, w.mterms, params, means, prec, nllw, n_gauss, w_dense, w_marker, w_beta,
                           w_prior, w.grad, loss_trace, iters, it, loss_last, nullptr, 0.f, V);
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
