// The cell grid of the raw-cloud kernels (DESIGN sections 19, 22 and 23), shared by cloud_filter.hip, cloud_isolate.hip and cloud_align.hip: the
// squared distance, the cloud of a packed row, and the walk over one column or one ring of cells of a cloud's sorted keys.  All three files are
// built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#define CLOUD_BITS 21
#define CLOUD_CMAX ((1 << CLOUD_BITS) - 1)

namespace {

__device__ __forceinline__ double cloud_d2(double px, double py, double pz, const double* __restrict__ q) {
    const double dx = px - q[0], dy = py - q[1], dz = pz - q[2];
    return ((dx * dx + dy * dy) + dz * dz);
}

// the cloud that owns packed row t: the last b with offsets[b] <= t (empty clouds repeat an offset)
__device__ __forceinline__ int cloud_of_row(const int* __restrict__ offsets, int B, int t) {
    int lo = 0, hi = B;                       // answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// first j in [lo, hi) with keys[j] >= v, hi if none
__device__ __forceinline__ int cloud_lower_bound(const long long* __restrict__ keys, int lo, int hi, long long v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// f(j) for every sorted row j of the segment [lo, hi) whose cell is (x, y, z0 .. z1)
template <class F>
__device__ __forceinline__ void cloud_scan_column(const long long* __restrict__ keys, int lo, int hi, int x, int y, int z0, int z1, F&& f) {
    if (x < 0 || y < 0 || x > CLOUD_CMAX || y > CLOUD_CMAX) return;
    z0 = z0 < 0 ? 0 : z0;
    z1 = z1 > CLOUD_CMAX ? CLOUD_CMAX : z1;
    if (z0 > z1) return;
    const long long base = ((long long)x << (2 * CLOUD_BITS)) | ((long long)y << CLOUD_BITS);
    const int a = cloud_lower_bound(keys, lo, hi, base | (long long)z0);
    const int e = cloud_lower_bound(keys, a, hi, (base | (long long)z1) + 1);
    for (int j = a; j < e; ++j) f(j);
}

// the shell of Chebyshev ring rho around the cell (ix, iy, iz): the rim columns whole, the inner columns' two caps
template <class F>
__device__ __forceinline__ void cloud_scan_ring(const long long* __restrict__ keys, int lo, int hi, int ix, int iy, int iz, int rho, F&& f) {
    for (int dx = -rho; dx <= rho; ++dx)
        for (int dy = -rho; dy <= rho; ++dy) {
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            if ((ax > ay ? ax : ay) == rho) {
                cloud_scan_column(keys, lo, hi, ix + dx, iy + dy, iz - rho, iz + rho, f);
            } else {
                cloud_scan_column(keys, lo, hi, ix + dx, iy + dy, iz - rho, iz - rho, f);
                cloud_scan_column(keys, lo, hi, ix + dx, iy + dy, iz + rho, iz + rho, f);
            }
        }
}

}  // namespace
