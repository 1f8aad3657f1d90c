// The per-pair and per-triple arithmetic of cloud_global.hip in plain C++, for the device and for a host build alike: the
// Philox block that draws a hypothesis, the pair feature of the descriptors and its bins, the validity test of a triple of correspondences and
// the triple's moments, which go to align_solve of cloud_align_solve.h.  fp64, one rounding per operation (the including file is built with
// -ffp-contract=off); every array index is a compile-time constant, so nothing spills.
#pragma once
#include <cmath>

#include "cloud_align_solve.h"

#define GLOBAL_HD ALIGN_HD
#define GLOBAL_BINS 11                       // = ETCH_GLOBAL_BINS of the header
#define GLOBAL_FEATURES 33                   // three blocks of GLOBAL_BINS: theta, alpha, phi
#define GLOBAL_PI 3.14159265358979323846     // the double nearest to pi

// Philox4x32-10, the text of cloud_isolate.hip's: counter (c0, c1, c2, c3), key (k0, k1) -> r[4]
GLOBAL_HD void global_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
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

// the three correspondences of hypothesis h under the pair's key: counter (h, 2, 0, 0) -- (j, 0, 0, 0) is the pick of depth_render.hip and
// (h, 1, 0, 0) the plane of cloud_isolate.hip --, i_a = (r_a n) >> 32 < n
GLOBAL_HD void global_hypothesis_rows(unsigned long long key, int h, int n, int& i0, int& i1, int& i2) {
    unsigned r[4];
    global_philox4x32_10((unsigned)h, 2u, 0u, 0u, (unsigned)key, (unsigned)(key >> 32), r);
    i0 = (int)(((unsigned long long)r[0] * (unsigned long long)n) >> 32);
    i1 = (int)(((unsigned long long)r[1] * (unsigned long long)n) >> 32);
    i2 = (int)(((unsigned long long)r[2] * (unsigned long long)n) >> 32);
}

GLOBAL_HD double global_dot(double ax, double ay, double az, double bx, double by, double bz) { return ((ax * bx + ay * by) + az * bz); }

// ((dx dx + dy dy) + dz dz), d = a - b
GLOBAL_HD double global_d2(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return ((dx * dx + dy * dy) + dz * dz);
}

// floor(x) clamped into 0 .. GLOBAL_BINS - 1; a NaN goes to bin 0
GLOBAL_HD int global_bin(double x) {
    double b = floor(x);
    if (!(b >= 0.0)) b = 0.0;
    if (b > (double)(GLOBAL_BINS - 1)) b = (double)(GLOBAL_BINS - 1);
    return (int)b;
}

// The pair feature of rows i and j (points p, unit normals n, d2 = ((dx dx + dy dy) + dz dz) > 0 as the search measured it).  d = (pj - pi) / sqrt(d2)
// per component; ai = ni.d, aj = nj.d (each ((x + y) + z)); the source is i where |ai| >= |aj|, else j with d negated; u = the source's normal,
// nt = the other's; c = d x u (each component a difference of two rounded products), cl2 = (c0 c0 + c1 c1) + c2 c2 -- the pair is not counted,
// and false returned, unless cl2 > 0 --, v = c / sqrt(cl2), w = u x v; f[0] = theta = atan2(w.nt, u.nt), f[1] = alpha = v.nt, f[2] = phi = u.d.
// bin[0] = floor((11 (theta + pi)) / (2 pi)), bin[1] = floor((11 (alpha + 1)) / 2), bin[2] = floor((11 (phi + 1)) / 2), each clamped to 0 .. 10.
GLOBAL_HD bool global_pair_feature(const double* pi, const double* ni, const double* pj, const double* nj, double d2, double* f, int* bin) {
    const double len = sqrt(d2);
    double d0 = (pj[0] - pi[0]) / len, d1 = (pj[1] - pi[1]) / len, dd2 = (pj[2] - pi[2]) / len;
    const double ai = global_dot(ni[0], ni[1], ni[2], d0, d1, dd2), aj = global_dot(nj[0], nj[1], nj[2], d0, d1, dd2);
    const bool first = fabs(ai) >= fabs(aj);
    const double u0 = first ? ni[0] : nj[0], u1 = first ? ni[1] : nj[1], u2 = first ? ni[2] : nj[2];
    const double t0 = first ? nj[0] : ni[0], t1 = first ? nj[1] : ni[1], t2 = first ? nj[2] : ni[2];
    if (!first) d0 = -d0, d1 = -d1, dd2 = -dd2;
    const double c0 = d1 * u2 - dd2 * u1, c1 = dd2 * u0 - d0 * u2, c2 = d0 * u1 - d1 * u0;
    const double cl2 = (c0 * c0 + c1 * c1) + c2 * c2;
    f[0] = f[1] = f[2] = 0.0;
    bin[0] = bin[1] = bin[2] = 0;
    if (!(cl2 > 0.0)) return false;
    const double cl = sqrt(cl2);
    const double v0 = c0 / cl, v1 = c1 / cl, v2 = c2 / cl;
    const double w0 = u1 * v2 - u2 * v1, w1 = u2 * v0 - u0 * v2, w2 = u0 * v1 - u1 * v0;
    f[0] = atan2(global_dot(w0, w1, w2, t0, t1, t2), global_dot(u0, u1, u2, t0, t1, t2));
    f[1] = global_dot(v0, v1, v2, t0, t1, t2);
    f[2] = global_dot(u0, u1, u2, d0, d1, dd2);
    bin[0] = global_bin((11.0 * (f[0] + GLOBAL_PI)) / (2.0 * GLOBAL_PI));
    bin[1] = global_bin((11.0 * (f[1] + 1.0)) / 2.0);
    bin[2] = global_bin((11.0 * (f[2] + 1.0)) / 2.0);
    return true;
}

// one edge of a triple: the squared lengths on either side are similar (e2 = edge_similarity^2) and the source's is at least min2 = min_edge^2
GLOBAL_HD bool global_edge_valid(double ls2, double lt2, double e2, double min2) { return ls2 >= e2 * lt2 && lt2 >= e2 * ls2 && ls2 >= min2; }

// the three edges (0,1), (1,2), (2,0) of the source points a0, a1, a2 and the target points b0, b1, b2
GLOBAL_HD bool global_triple_valid(const double* a0, const double* a1, const double* a2, const double* b0, const double* b1, const double* b2, double e2,
                                   double min2) {
    return global_edge_valid(global_d2(a0, a1), global_d2(b0, b1), e2, min2) && global_edge_valid(global_d2(a1, a2), global_d2(b1, b2), e2, min2) &&
           global_edge_valid(global_d2(a2, a0), global_d2(b2, b0), e2, min2);
}

// sums[16] in the layout of align_solve, over the pairs (a0, b0), (a1, b1), (a2, b2) in that order, about c = the centre of the target triple's
// bounding box (0.5 (min + max) per component): x' = a - c, q' = b - c, sum x' (3), sum q' (3), sum x' q'^T (9), sum d2 with d2 = global_d2(a, b)
GLOBAL_HD void global_triple_moments(const double* a0, const double* a1, const double* a2, const double* b0, const double* b1, const double* b2, double* c,
                                     double* sums) {
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = 0.5 * (fmin(fmin(b0[r], b1[r]), b2[r]) + fmax(fmax(b0[r], b1[r]), b2[r]));
#pragma unroll
    for (int k = 0; k < 16; ++k) sums[k] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double* x = a == 0 ? a0 : a == 1 ? a1 : a2;
        const double* q = a == 0 ? b0 : a == 1 ? b1 : b2;
        const double xc[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]}, qc[3] = {q[0] - c[0], q[1] - c[1], q[2] - c[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            sums[r] += xc[r];
            sums[3 + r] += qc[r];
#pragma unroll
            for (int e = 0; e < 3; ++e) sums[6 + 3 * r + e] += xc[r] * qc[e];
        }
        sums[15] += global_d2(x, q);
    }
}

// (R, t) of the triple by align_solve; false, and R = I, t = 0, where align_solve calls the three pairs degenerate (collinear points)
GLOBAL_HD bool global_triple_solve(const double* a0, const double* a1, const double* a2, const double* b0, const double* b1, const double* b2, double* R,
                                   double* t) {
    double c[3], sums[16], angle, shift;
    global_triple_moments(a0, a1, a2, b0, b1, b2, c, sums);
    return align_solve(3, sums, c, R, t, angle, shift);
}
