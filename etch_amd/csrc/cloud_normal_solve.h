// The per-row solve of cloud_normals.hip in plain C++, for the device and for a host build alike: the covariance from the
// moment sums, its eigen-decomposition by cyclic Jacobi on the symmetric 3 x 3 matrix, the flags and the sign of the normal.  fp64, one rounding
// per operation (the including file is built with -ffp-contract=off); every array index is a compile-time constant, so nothing spills.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define NORMAL_HD __host__ __device__ __forceinline__
#else
#define NORMAL_HD inline
#endif

#define NORMAL_JACOBI_SWEEPS 10              // a symmetric 3 x 3 matrix is diagonal to rounding after 4 - 6 cyclic sweeps
#define NORMAL_GAP_EPS 1e-9                  // = ETCH_NORMAL_GAP_EPS of the header
#define NORMAL_FLAG_FEW 1                    // = ETCH_NORMAL_FLAG_FEW
#define NORMAL_FLAG_AMBIGUOUS 2              // = ETCH_NORMAL_FLAG_AMBIGUOUS

// one Jacobi rotation that zeroes a[P][Q] of the symmetric 3 x 3 matrix a and accumulates it into the columns of v
template <int P, int Q>
NORMAL_HD void normal_jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    constexpr int K = 3 - P - Q;
    const double akp = a[K][P], akq = a[K][Q];
    a[K][P] = a[P][K] = c * akp - s * akq;
    a[K][Q] = a[Q][K] = s * akp + c * akq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// sum[3] = s = sum e, sq[6] = S_xx, S_xy, S_xz, S_yy, S_yz, S_zz over the ke neighbours, e = q - p -> cov[6] in the same order:
// w = ke + 1 (the row itself counts with e = 0), mu = s / w, C_ab = S_ab / w - mu_a mu_b
NORMAL_HD void normal_covariance(int ke, const double* sum, const double* sq, double* cov) {
    const double w = (double)(ke + 1);
    const double m0 = sum[0] / w, m1 = sum[1] / w, m2 = sum[2] / w;
    cov[0] = sq[0] / w - m0 * m0, cov[1] = sq[1] / w - m0 * m1, cov[2] = sq[2] / w - m0 * m2;
    cov[3] = sq[3] / w - m1 * m1, cov[4] = sq[4] / w - m1 * m2, cov[5] = sq[5] / w - m2 * m2;
}

// cov[6] (xx, xy, xz, yy, yz, zz) -> lambda[3] ascending, n = the normalised eigenvector of lambda[0] with its largest component positive (a tie
// of magnitudes to the lowest axis), variation = lambda0 / ((lambda0 + lambda1) + lambda2) (0 where that trace is not positive).  Returns the
// flags: FEW where ke < 2, AMBIGUOUS where lambda1 - lambda0 > NORMAL_GAP_EPS lambda2 does not hold (collinear, coincident and isotropic
// neighbourhoods, and a NaN); a flagged row gets n = 0.
NORMAL_HD int normal_solve(int ke, const double* cov, double* lambda, double* n, double& variation) {
    double a[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < NORMAL_JACOBI_SWEEPS; ++sweep) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
        normal_jacobi_rotate<0, 1>(a, v);
        normal_jacobi_rotate<0, 2>(a, v);
        normal_jacobi_rotate<1, 2>(a, v);
    }
    const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
    int low = 0;                                                     // the smallest eigenvalue, a tie to the lowest column
    double l0 = e0;
    if (e1 < l0) l0 = e1, low = 1;
    if (e2 < l0) l0 = e2, low = 2;
    const double ra = low == 0 ? e1 : e0, rb = low == 2 ? e1 : e2;   // the other two
    const double l1 = ra < rb ? ra : rb, l2 = ra < rb ? rb : ra;
    lambda[0] = l0, lambda[1] = l1, lambda[2] = l2;
    const double tr = (l0 + l1) + l2;
    variation = tr > 0.0 ? l0 / tr : 0.0;
    int flag = ke < 2 ? NORMAL_FLAG_FEW : 0;
    if (!(l1 - l0 > NORMAL_GAP_EPS * l2)) flag |= NORMAL_FLAG_AMBIGUOUS;
    double x = low == 0 ? v[0][0] : low == 1 ? v[0][1] : v[0][2];
    double y = low == 0 ? v[1][0] : low == 1 ? v[1][1] : v[1][2];
    double z = low == 0 ? v[2][0] : low == 1 ? v[2][1] : v[2][2];
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0) || !std::isfinite(len)) flag |= NORMAL_FLAG_AMBIGUOUS;
    if (flag) {
        n[0] = n[1] = n[2] = 0.0;
        return flag;
    }
    x = x / len, y = y / len, z = z / len;
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    if (lead < 0.0) x = -x, y = -y, z = -z;
    n[0] = x, n[1] = y, n[2] = z;
    return flag;
}

// n.(view - p) >= 0: flips n where s = ((n_x w_x + n_y w_y) + n_z w_z) < 0, w = view - p; an exact 0 keeps the sign normal_solve gave
NORMAL_HD void normal_face(const double* view, double px, double py, double pz, double* n) {
    const double wx = view[0] - px, wy = view[1] - py, wz = view[2] - pz;
    const double s = (n[0] * wx + n[1] * wy) + n[2] * wz;
    if (s < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}
