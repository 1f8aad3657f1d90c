// csrc/cloud_global_solve.h built by the host compiler alone, for tests/test_global_host.py (address and undefined-behaviour sanitizers).
// argv[1]: a text file, one problem per line.  `P pi[3] ni[3] pj[3] nj[3]`: the pair feature, prints `P counted theta alpha phi bin[3]`.
// `T a0[3] a1[3] a2[3] b0[3] b1[3] b2[3] e min_edge`: a triple, prints `T valid solved R[9] t[3] c[3] sums[16]`.  `H key h n`: the draw of a
// hypothesis, prints `H i0 i1 i2`.  17 significant digits; `done` at the end.
#include <cstdio>
#include <cstring>

#include "cloud_global_solve.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 3;
    char tag[8];
    while (std::fscanf(fh, "%7s", tag) == 1) {
        if (std::strcmp(tag, "P") == 0) {
            double v[12], f[3];
            int bin[3];
            for (int a = 0; a < 12; ++a)
                if (std::fscanf(fh, "%lf", &v[a]) != 1) return 4;
            const double d2 = global_d2(v, v + 6);
            const bool counted = d2 > 0.0 && global_pair_feature(v, v + 3, v + 6, v + 9, d2, f, bin);
            if (!counted) f[0] = f[1] = f[2] = 0.0, bin[0] = bin[1] = bin[2] = 0;
            std::printf("P %d %.17g %.17g %.17g %d %d %d\n", counted ? 1 : 0, f[0], f[1], f[2], bin[0], bin[1], bin[2]);
        } else if (std::strcmp(tag, "T") == 0) {
            double v[18], e = 0.0, min_edge = 0.0, R[9], t[3], c[3], sums[16];
            for (int a = 0; a < 18; ++a)
                if (std::fscanf(fh, "%lf", &v[a]) != 1) return 4;
            if (std::fscanf(fh, "%lf %lf", &e, &min_edge) != 2) return 4;
            const bool valid = global_triple_valid(v, v + 3, v + 6, v + 9, v + 12, v + 15, e * e, min_edge * min_edge);
            global_triple_moments(v, v + 3, v + 6, v + 9, v + 12, v + 15, c, sums);
            const bool solved = global_triple_solve(v, v + 3, v + 6, v + 9, v + 12, v + 15, R, t);
            std::printf("T %d %d", valid ? 1 : 0, solved ? 1 : 0);
            for (int a = 0; a < 9; ++a) std::printf(" %.17g", R[a]);
            for (int a = 0; a < 3; ++a) std::printf(" %.17g", t[a]);
            for (int a = 0; a < 3; ++a) std::printf(" %.17g", c[a]);
            for (int a = 0; a < 16; ++a) std::printf(" %.17g", sums[a]);
            std::printf("\n");
        } else if (std::strcmp(tag, "H") == 0) {
            unsigned long long key = 0;
            int h = 0, n = 0, i0 = 0, i1 = 0, i2 = 0;
            if (std::fscanf(fh, "%llu %d %d", &key, &h, &n) != 3) return 4;
            global_hypothesis_rows(key, h, n, i0, i1, i2);
            std::printf("H %d %d %d\n", i0, i1, i2);
        } else {
            return 5;
        }
    }
    std::fclose(fh);
    std::printf("done\n");
    return 0;
}
