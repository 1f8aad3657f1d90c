// Closest point of a triangle to a point, shared by the fp64 mesh geometry (raycast.hip) and the fp32 dense surface fit (surface_fit.hip).
// Both TUs are built with -ffp-contract=off: every expression is evaluated exactly as written, one rounding per operation, in T.
//
// Ericson 5.1.5 ClosestPtPointTriangle, operation order (dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z; vector ops componentwise):
//   ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
//   region A   d1 <= 0 && d2 <= 0                                   -> a                    bary (1, 0, 0)
//   bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
//   region B   d3 >= 0 && d4 <= d3                                  -> b                    bary (0, 1, 0)
//   vc = d1*d4 - d3*d2
//   edge AB    vc <= 0 && d1 >= 0 && d3 <= 0    v = d1 / (d1 - d3)  -> a + v*ab             bary (1 - v, v, 0)
//   cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
//   region C   d6 >= 0 && d5 <= d6                                  -> c                    bary (0, 0, 1)
//   vb = d5*d2 - d1*d6
//   edge AC    vb <= 0 && d2 >= 0 && d6 <= 0    w = d2 / (d2 - d6)  -> a + w*ac             bary (1 - w, 0, w)
//   va = d3*d6 - d5*d4
//   edge BC    va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0
//              w = (d4 - d3) / ((d4 - d3) + (d5 - d6))              -> b + w*(c - b)        bary (0, 1 - w, w)
//   interior   denom = 1 / ((va + vb) + vc), v = vb*denom, w = vc*denom
//                                                                   -> (a + ab*v) + ac*w    bary ((1 - v) - w, v, w)
//   d2 = dot(p - q, p - q).  A degenerate triangle can give NaN: never below a running minimum, so never chosen.
#pragma once
#include <hip/hip_runtime.h>

template <typename T>
struct RcClosestT {
    T q[3], b[3], d2;
};

template <typename T>
__device__ __forceinline__ T rc_dot_t(T ax, T ay, T az, T bx, T by, T bz) {
    return ((ax * bx) + (ay * by)) + (az * bz);
}

template <typename T>
__device__ __forceinline__ RcClosestT<T> rc_closest_t(const T* p, const T* a, const T* b, const T* c) {
    RcClosestT<T> o;
    const T zero = (T)0, one = (T)1;
    const T ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const T ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const T ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const T d1 = rc_dot_t(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]), d2 = rc_dot_t(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    const T bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const T d3 = rc_dot_t(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]), d4 = rc_dot_t(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    const T vc = d1 * d4 - d3 * d2;
    const T cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const T d5 = rc_dot_t(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]), d6 = rc_dot_t(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    const T vb = d5 * d2 - d1 * d6;
    const T va = d3 * d6 - d5 * d4;
    if (d1 <= zero && d2 <= zero) {
        for (int i = 0; i < 3; ++i) o.q[i] = a[i];
        o.b[0] = one; o.b[1] = zero; o.b[2] = zero;
    } else if (d3 >= zero && d4 <= d3) {
        for (int i = 0; i < 3; ++i) o.q[i] = b[i];
        o.b[0] = zero; o.b[1] = one; o.b[2] = zero;
    } else if (vc <= zero && d1 >= zero && d3 <= zero) {
        const T v = d1 / (d1 - d3);
        for (int i = 0; i < 3; ++i) o.q[i] = a[i] + v * ab[i];
        o.b[0] = one - v; o.b[1] = v; o.b[2] = zero;
    } else if (d6 >= zero && d5 <= d6) {
        for (int i = 0; i < 3; ++i) o.q[i] = c[i];
        o.b[0] = zero; o.b[1] = zero; o.b[2] = one;
    } else if (vb <= zero && d2 >= zero && d6 <= zero) {
        const T w = d2 / (d2 - d6);
        for (int i = 0; i < 3; ++i) o.q[i] = a[i] + w * ac[i];
        o.b[0] = one - w; o.b[1] = zero; o.b[2] = w;
    } else if (va <= zero && (d4 - d3) >= zero && (d5 - d6) >= zero) {
        const T w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int i = 0; i < 3; ++i) o.q[i] = b[i] + w * (c[i] - b[i]);
        o.b[0] = zero; o.b[1] = one - w; o.b[2] = w;
    } else {
        const T denom = one / ((va + vb) + vc);
        const T v = vb * denom, w = vc * denom;
        for (int i = 0; i < 3; ++i) o.q[i] = (a[i] + ab[i] * v) + ac[i] * w;
        o.b[0] = (one - v) - w; o.b[1] = v; o.b[2] = w;
    }
    const T e[3] = {p[0] - o.q[0], p[1] - o.q[1], p[2] - o.q[2]};
    o.d2 = rc_dot_t(e[0], e[1], e[2], e[0], e[1], e[2]);
    return o;
}
