// The per-row and per-pair arithmetic of cloud_winding.hip in plain C++, for the device and for a host build alike: the area
// of a row, the packed row, the pair term of the dipole sum (Barill et al. 2018) and the key that orders (d2, row).  The area and the pack are
// fp64, the pair term fp32, one rounding per operation (the including file is built with -ffp-contract=off).  tests/_cloud_winding_oracle.py
// restates every function with numpy.
#pragma once
#include <cmath>
#include <cstring>

#ifdef __HIPCC__
#define WIND_HD __host__ __device__ __forceinline__
#else
#define WIND_HD inline
#endif

#define WIND_PI 3.14159265358979323846          // the double nearest to pi
#define WIND_INV_4PI 0.07957747154594767        // the double nearest to 1 / (4 pi)
#define WIND_NO_KEY 0xffffffffffffffffull       // no row: behind every key

// a_i = (pi d2k) / ke: the disc to the ke-th neighbour holds ke rows, so one row stands for a ke-th of it.  0 for a cloud of one row (ke = 0), a
// row whose normal is flagged and a row that is not finite.
WIND_HD double wind_area(double d2k, int ke, int flag, double px, double py, double pz) {
    if (ke <= 0 || flag != 0 || !std::isfinite(px) || !std::isfinite(py) || !std::isfinite(pz)) return 0.0;
    return (WIND_PI * d2k) / (double)ke;
}

// pos = fp32(p - c), moment = fp32(a n), cap = fp32(a / pi): differences, products and the quotient in fp64, one rounding each to fp32
WIND_HD void wind_pack(const double p[3], const double c[3], const double n[3], double a, float pos[3], float moment[3], float& cap) {
    pos[0] = (float)(p[0] - c[0]), pos[1] = (float)(p[1] - c[1]), pos[2] = (float)(p[2] - c[2]);
    moment[0] = (float)(a * n[0]), moment[1] = (float)(a * n[1]), moment[2] = (float)(a * n[2]);
    cap = (float)(a / WIND_PI);
}

WIND_HD float wind_d2(float rx, float ry, float rz) { return (rx * rx + ry * ry) + rz * rz; }

// r = pos_i - q, d2 = wind_d2(r), s = max(d2, cap) -- cap where d2 is NaN --, term = (r . m) / (s sqrt(s)).  Inside the row's own disc
// (d2 < cap = the disc's radius squared) the kernel of the dipole stops growing.  A row with cap == 0 contributes exactly 0, whatever else it holds.
WIND_HD float wind_term(float rx, float ry, float rz, float d2, float mx, float my, float mz, float cap) {
    if (cap == 0.f) return 0.f;
    const float s = d2 > cap ? d2 : cap;
    return ((rx * mx + ry * my) + rz * mz) / (s * sqrtf(s));
}

// (d2, row) as one integer that orders like the pair: the bits of a non-negative fp32 ascend with its value.  A NaN d2 has no key.
WIND_HD unsigned long long wind_key(float d2, int row) {
    if (!(d2 >= 0.f) || row < 0) return WIND_NO_KEY;
    unsigned u;
    std::memcpy(&u, &d2, 4);
    return ((unsigned long long)u << 32) | (unsigned)row;
}

WIND_HD unsigned long long wind_merge(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

// the row and its d2 of a merged key; -1 and 0 where no row had a key (an empty cloud, or every d2 NaN)
WIND_HD void wind_unkey(unsigned long long key, int& row, float& d2) {
    if (key == WIND_NO_KEY) {
        row = -1, d2 = 0.f;
        return;
    }
    const unsigned u = (unsigned)(key >> 32);
    row = (int)(unsigned)key;
    std::memcpy(&d2, &u, 4);
}
