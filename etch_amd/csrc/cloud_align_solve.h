// The rigid step of cloud_align.hip in plain C++, for the device and for a host build alike: the transform, Horn's
// quaternion from the 16 moment sums by cyclic Jacobi on the symmetric 4 x 4 matrix, the rank test and the composition.  fp64, one rounding
// per operation (the including file is built with -ffp-contract=off); every array index is a compile-time constant, so nothing spills.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define ALIGN_HD __host__ __device__ __forceinline__
#else
#define ALIGN_HD inline
#endif

#define ALIGN_JACOBI_SWEEPS 12               // a symmetric 4 x 4 matrix is diagonal to rounding after 6 - 8 cyclic sweeps
#define ALIGN_RANK_EPS 1e-9                  // = ETCH_ALIGN_RANK_EPS of the header

// x = R p + t, per component ((R_r0 px + R_r1 py) + R_r2 pz) + t_r
ALIGN_HD void align_apply(const double* R, const double* t, double px, double py, double pz, double& x, double& y, double& z) {
    x = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0];
    y = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1];
    z = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2];
}

// one Jacobi rotation that zeroes a[P][Q] of the symmetric 4 x 4 matrix a and accumulates it into the columns of v
template <int P, int Q>
ALIGN_HD void align_jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = a[k][P], akq = a[k][Q];
            a[k][P] = a[P][k] = c * akp - s * akq;
            a[k][Q] = a[Q][k] = s * akp + c * akq;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// sums[16] = sum x' (3), sum q' (3), sum x' q'^T (9, row = the component of x'), sum d2, over the m matched pairs, x' = x - c, q' = q - c.
// -> dR (9), dt (3) minimising sum |dR x + dt - q|^2, angle = the turn of dR in radians, shift = |mean q - mean x|.  Returns false, and dR = I,
// dt = 0, where the step is degenerate: m < 3, or the two largest eigenvalues of Horn's matrix closer than ALIGN_RANK_EPS of the largest.
ALIGN_HD bool align_solve(int m, const double* sums, const double* c, double* dR, double* dt, double& angle, double& shift) {
    dR[0] = dR[4] = dR[8] = 1.0;
    dR[1] = dR[2] = dR[3] = dR[5] = dR[6] = dR[7] = 0.0;
    dt[0] = dt[1] = dt[2] = 0.0;
    angle = 0.0, shift = 0.0;
    if (m < 3) return false;
    const double dm = (double)m;
    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) S[a][b] = sums[6 + 3 * a + b] - sums[a] * sums[3 + b] / dm;
    double n[4][4] = {{(S[0][0] + S[1][1]) + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                      {S[1][2] - S[2][1], (S[0][0] - S[1][1]) - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                      {S[2][0] - S[0][2], S[0][1] + S[1][0], (S[1][1] - S[0][0]) - S[2][2], S[1][2] + S[2][1]},
                      {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], (S[2][2] - S[0][0]) - S[1][1]}};
    double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < ALIGN_JACOBI_SWEEPS; ++sweep) {
        if (n[0][1] == 0.0 && n[0][2] == 0.0 && n[0][3] == 0.0 && n[1][2] == 0.0 && n[1][3] == 0.0 && n[2][3] == 0.0) break;
        align_jacobi_rotate<0, 1>(n, v);
        align_jacobi_rotate<0, 2>(n, v);
        align_jacobi_rotate<0, 3>(n, v);
        align_jacobi_rotate<1, 2>(n, v);
        align_jacobi_rotate<1, 3>(n, v);
        align_jacobi_rotate<2, 3>(n, v);
    }
    const double e0 = n[0][0], e1 = n[1][1], e2 = n[2][2], e3 = n[3][3];
    int top = 0;                                                     // the largest eigenvalue, a tie to the lowest column
    double l1 = e0;
    if (e1 > l1) l1 = e1, top = 1;
    if (e2 > l1) l1 = e2, top = 2;
    if (e3 > l1) l1 = e3, top = 3;
    double l2 = -INFINITY;
    if (top != 0) l2 = fmax(l2, e0);
    if (top != 1) l2 = fmax(l2, e1);
    if (top != 2) l2 = fmax(l2, e2);
    if (top != 3) l2 = fmax(l2, e3);
    if (!(l1 > 0.0) || !std::isfinite(l1) || !(l1 - l2 > ALIGN_RANK_EPS * l1)) return false;
    double qw = top == 0 ? v[0][0] : top == 1 ? v[0][1] : top == 2 ? v[0][2] : v[0][3];
    double qx = top == 0 ? v[1][0] : top == 1 ? v[1][1] : top == 2 ? v[1][2] : v[1][3];
    double qy = top == 0 ? v[2][0] : top == 1 ? v[2][1] : top == 2 ? v[2][2] : v[2][3];
    double qz = top == 0 ? v[3][0] : top == 1 ? v[3][1] : top == 2 ? v[3][2] : v[3][3];
    const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    if (qw < 0.0) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
    qw = qw / len, qx = qx / len, qy = qy / len, qz = qz / len;
    // a unit quaternion's matrix in the 1 - 2 (..) form: det = +1 and orthogonal to rounding, exact at the identity
    dR[0] = 1.0 - 2.0 * (qy * qy + qz * qz), dR[1] = 2.0 * (qx * qy - qw * qz), dR[2] = 2.0 * (qx * qz + qw * qy);
    dR[3] = 2.0 * (qx * qy + qw * qz), dR[4] = 1.0 - 2.0 * (qx * qx + qz * qz), dR[5] = 2.0 * (qy * qz - qw * qx);
    dR[6] = 2.0 * (qx * qz - qw * qy), dR[7] = 2.0 * (qy * qz + qw * qx), dR[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    const double mx[3] = {sums[0] / dm + c[0], sums[1] / dm + c[1], sums[2] / dm + c[2]};
    const double mq[3] = {sums[3] / dm + c[0], sums[4] / dm + c[1], sums[5] / dm + c[2]};
#pragma unroll
    for (int r = 0; r < 3; ++r) dt[r] = mq[r] - ((dR[3 * r] * mx[0] + dR[3 * r + 1] * mx[1]) + dR[3 * r + 2] * mx[2]);
    const double ux = (sums[3] - sums[0]) / dm, uy = (sums[4] - sums[1]) / dm, uz = (sums[5] - sums[2]) / dm;
    shift = sqrt((ux * ux + uy * uy) + uz * uz);
    angle = 2.0 * atan2(sqrt((qx * qx + qy * qy) + qz * qz), qw);
    return true;
}

// R <- dR R, t <- dR t + dt
ALIGN_HD void align_compose(const double* dR, const double* dt, double* R, double* t) {
    double Rn[9], tn[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) Rn[3 * r + k] = (dR[3 * r] * R[k] + dR[3 * r + 1] * R[3 + k]) + dR[3 * r + 2] * R[6 + k];
        tn[r] = ((dR[3 * r] * t[0] + dR[3 * r + 1] * t[1]) + dR[3 * r + 2] * t[2]) + dt[r];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

// ---- the point-to-plane step -------------------------------------------------------------------------------------------------
#define ALIGN_PLANE_EPS 1e-9                 // = ETCH_ALIGN_PLANE_EPS of the header
#define ALIGN_PLANE_SERIES 1e-4              // below this angle the half-angle sine and cosine come from their series

// the index of entry (i, j), i <= j, of a symmetric 6 x 6 matrix stored as its upper triangle, row-major
ALIGN_HD constexpr int align_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// sums[32] = the 21 upper-triangle entries of A = sum J J^T (row-major), g = sum J r (6), sum r^2, sum d2, sum x' (3) over the m matched rows,
// J = (x' x n, n), r = (x - q).n, x' = x - c.  Minimises sum (r + J.y)^2 over y = (omega, tau): A y = -g, solved as Abar z = -gbar with
// Abar = D A D / m, gbar = D g / m, y = D z, D = diag(1/rho, 1/rho, 1/rho, 1, 1, 1) and rho the half-diagonal of the target's box: the rotation
// columns then carry lengths relative to the cloud, like the translation columns, and nothing is scaled by diag(A) -- that scaling divides by zero
// on an exactly planar target and hides a plane's, a cylinder's or a sphere's free motions behind pivots of 0.99.  LDL^T in the fixed order
// 0 .. 5, no pivoting.  -> dR (9) from the quaternion (cos th/2, sin(th/2) omega / th), th = |omega|, normalised and written in the 1 - 2 (..)
// form, so dR is a rotation to rounding whatever the data; dt = c - dR c + tau; angle = th; shift = |(dR - I) mean x' + tau|, the movement of the
// matched rows' centroid; y (6) = omega, tau.  Returns false, and dR = I, dt = 0, y = 0, where the step is degenerate: m < 6, rho not positive
// and finite, or a pivot d_i that fails d_i > ALIGN_PLANE_EPS max_j Abar_jj (a zero or NaN pivot fails and is never divided by).  The criterion
// guards exact singularity only -- an exact plane with exact normals, collinear data, no normal at all; a merely near-symmetric target (a noisy
// plane, a cylinder) is not flagged and slides, as a planar patch does under Horn's rule above.
ALIGN_HD bool align_plane_solve(int m, const double* sums, const double* c, double rho, double* dR, double* dt, double& angle, double& shift, double* y) {
    dR[0] = dR[4] = dR[8] = 1.0;
    dR[1] = dR[2] = dR[3] = dR[5] = dR[6] = dR[7] = 0.0;
    dt[0] = dt[1] = dt[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = 0.0;
    angle = 0.0, shift = 0.0;
    if (m < 6 || !(rho > 0.0) || !std::isfinite(rho)) return false;
    const double dm = (double)m, inv = 1.0 / rho;
    double L[6][6], d[6], z[6];                                      // L: the scaled matrix on and above the diagonal, the factor below it
    double top = -INFINITY;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = sums[align_tri(i, j)] / dm;
            if (i < 3) v = v * inv;
            if (j < 3) v = v * inv;
            L[i][j] = v;
        }
        z[i] = -(i < 3 ? (sums[21 + i] / dm) * inv : sums[21 + i] / dm);
        if (L[i][i] > top) top = L[i][i];
    }
    const double floor_ = ALIGN_PLANE_EPS * top;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
        if (!(dj > floor_) || !(dj > 0.0)) return false;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v / dj;
        }
    }
#pragma unroll
    for (int i = 1; i < 6; ++i)                                      // L w = -gbar
#pragma unroll
        for (int k = 0; k < i; ++k) z[i] = z[i] - L[i][k] * z[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) z[i] = z[i] / d[i];
#pragma unroll
    for (int i = 4; i >= 0; --i)                                     // L^T z = w
#pragma unroll
        for (int k = i + 1; k < 6; ++k) z[i] = z[i] - L[k][i] * z[k];
    const double wx = z[0] * inv, wy = z[1] * inv, wz = z[2] * inv, tx = z[3], ty = z[4], tz = z[5];
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    if (!std::isfinite(th) || !std::isfinite(tx) || !std::isfinite(ty) || !std::isfinite(tz)) return false;
    double qw, kf;                                                   // q = (qw, kf omega)
    if (th < ALIGN_PLANE_SERIES) qw = 1.0 - (th * th) / 8.0, kf = 0.5 - (th * th) / 48.0;
    else qw = cos(0.5 * th), kf = sin(0.5 * th) / th;
    double qx = kf * wx, qy = kf * wy, qz = kf * wz;
    const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / len, qx = qx / len, qy = qy / len, qz = qz / len;
    dR[0] = 1.0 - 2.0 * (qy * qy + qz * qz), dR[1] = 2.0 * (qx * qy - qw * qz), dR[2] = 2.0 * (qx * qz + qw * qy);
    dR[3] = 2.0 * (qx * qy + qw * qz), dR[4] = 1.0 - 2.0 * (qx * qx + qz * qz), dR[5] = 2.0 * (qy * qz - qw * qx);
    dR[6] = 2.0 * (qx * qz - qw * qy), dR[7] = 2.0 * (qy * qz + qw * qx), dR[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    const double tau[3] = {tx, ty, tz};
    const double mx[3] = {sums[29] / dm, sums[30] / dm, sums[31] / dm};
    double sh[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        dt[r] = (c[r] - ((dR[3 * r] * c[0] + dR[3 * r + 1] * c[1]) + dR[3 * r + 2] * c[2])) + tau[r];
        sh[r] = (((dR[3 * r] * mx[0] + dR[3 * r + 1] * mx[1]) + dR[3 * r + 2] * mx[2]) - mx[r]) + tau[r];
    }
    shift = sqrt((sh[0] * sh[0] + sh[1] * sh[1]) + sh[2] * sh[2]);
    angle = th;
    y[0] = wx, y[1] = wy, y[2] = wz, y[3] = tx, y[4] = ty, y[5] = tz;
    return true;
}
