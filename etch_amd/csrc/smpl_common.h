// Body-model kinematics shared by the LM / LBS kernels (smpl_fit.hip), the chamfer refinement (chamfer_fit.hip) and the skinning frames
// of the registration (register.hip):
// batch_rodrigues with its derivative, the joint-angle lookup of the LM variable vector and forward kinematics, in fp64.
#pragma once
#include <hip/hip_runtime.h>

__device__ inline void rodrigues_d(const double th[3], double R[9], float dR[3][9], bool want_d) {
    // R = I + sin(a) K(n) + (1 - cos a) K(n)^2,  a = |theta + 1e-8|, n = theta / a
    const double e = 1e-8;
    const double a = sqrt((th[0] + e) * (th[0] + e) + (th[1] + e) * (th[1] + e) + (th[2] + e) * (th[2] + e));
    const double n[3] = {th[0] / a, th[1] / a, th[2] / a};
    const double s = sin(a), c = cos(a);
    double K[9] = {0, -n[2], n[1], n[2], 0, -n[0], -n[1], n[0], 0};
    double K2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2[i * 3 + j] = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * K[i] + (1.0 - c) * K2[i];
    if (!want_d) return;
    for (int q = 0; q < 3; ++q) {
        const double da = (th[q] + e) / a;
        double dn[3];
        for (int i = 0; i < 3; ++i) dn[i] = ((i == q ? 1.0 : 0.0) * a - th[i] * da) / (a * a);
        const double dK[9] = {0, -dn[2], dn[1], dn[2], 0, -dn[0], -dn[1], dn[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double dKK = 0, KdK = 0;
                for (int m = 0; m < 3; ++m) { dKK += dK[i * 3 + m] * K[m * 3 + j]; KdK += K[i * 3 + m] * dK[m * 3 + j]; }
                dR[q][i * 3 + j] = (float)(c * da * K[i * 3 + j] + s * dK[i * 3 + j] + s * da * K2[i * 3 + j] + (1.0 - c) * (dKK + KdK));
            }
    }
}

// x layout: pose[3(nj-1)] | betas[nb] | orient[3] | transl[3]
__device__ inline void joint_theta(const double* x, int j, int npose, int nb, double th[3]) {
    const double* p = j == 0 ? x + npose + nb : x + 3 * (j - 1);
    th[0] = p[0]; th[1] = p[1]; th[2] = p[2];
}

// Forward kinematics by one thread: Rw_j = Rw_p R_j, tw_j = Rw_p (J_j - J_p) + tw_p
__device__ inline void fk_chain(int nj, const int* parents, const double* R, const double* Jj, double* Rw, double* tw) {
    for (int i = 0; i < 9; ++i) Rw[i] = R[i];
    for (int i = 0; i < 3; ++i) tw[i] = Jj[i];
    for (int j = 1; j < nj; ++j) {
        const int p = parents[j];
        const double* Rp = Rw + p * 9;
        const double* Rj = R + j * 9;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Rw[j * 9 + a * 3 + b] = Rp[a * 3] * Rj[b] + Rp[a * 3 + 1] * Rj[3 + b] + Rp[a * 3 + 2] * Rj[6 + b];
        const double d[3] = {Jj[j * 3] - Jj[p * 3], Jj[j * 3 + 1] - Jj[p * 3 + 1], Jj[j * 3 + 2] - Jj[p * 3 + 2]};
        for (int a = 0; a < 3; ++a) tw[j * 3 + a] = Rp[a * 3] * d[0] + Rp[a * 3 + 1] * d[1] + Rp[a * 3 + 2] * d[2] + tw[p * 3 + a];
    }
}

// The pose set-up of a full-mesh kernel, by one workgroup (>= nj threads, every thread calls it): xs (the variable vector, already in LDS
// and synchronised) -> joint rotations R, shaped rest joints Jj, the world chain (Rw, tw).  All arrays are LDS.  R and Jj are synchronised
// on return; Rw and tw are thread 0's until the caller's next __syncthreads().
__device__ inline void smpl_block_chain(int nj, int nb, const float* J0, const float* Jd, const int* parents, const double* xs, double* R, double* Jj,
                                        double* Rw, double* tw) {
    const int tid = threadIdx.x, npose = 3 * (nj - 1);
    if (tid < nj) {
        double th[3];
        joint_theta(xs, tid, npose, nb, th);
        float dummy[3][9];
        rodrigues_d(th, R + tid * 9, dummy, false);
        for (int c = 0; c < 3; ++c) {
            double v = J0[tid * 3 + c];
            for (int l = 0; l < nb; ++l) v += (double)Jd[(tid * 3 + c) * nb + l] * xs[npose + l];
            Jj[tid * 3 + c] = v;
        }
    }
    __syncthreads();
    if (tid == 0) fk_chain(nj, parents, R, Jj, Rw, tw);
}
