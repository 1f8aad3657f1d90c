// csrc/cloud_normal_solve.h and csrc/cloud_align_solve.h built by the host compiler alone, for tests/test_normals_host.py (address and
// undefined-behaviour sanitizers).  argv[1]: a text file, one problem per line.  `J ke c_xx c_xy c_xz c_yy c_yz c_zz`: the 3 x 3 Jacobi, prints
// `J flag lambda0 lambda1 lambda2 nx ny nz variation`.  `S m rho c0 c1 c2 sums[32]`: the 6 x 6 point-to-plane solve, prints
// `S ok y[6] dR[9] dt[3] angle shift`.  17 significant digits; `done` at the end.
#include <cstdio>
#include <cstring>

#include "cloud_align_solve.h"
#include "cloud_normal_solve.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 3;
    char tag[8];
    while (std::fscanf(fh, "%7s", tag) == 1) {
        if (std::strcmp(tag, "J") == 0) {
            int ke = 0;
            double cov[6], lambda[3], n[3], variation = 0.0;
            if (std::fscanf(fh, "%d", &ke) != 1) return 4;
            for (int a = 0; a < 6; ++a)
                if (std::fscanf(fh, "%lf", &cov[a]) != 1) return 4;
            const int flag = normal_solve(ke, cov, lambda, n, variation);
            std::printf("J %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", flag, lambda[0], lambda[1], lambda[2], n[0], n[1], n[2], variation);
        } else if (std::strcmp(tag, "S") == 0) {
            int m = 0;
            double rho = 0.0, c[3], sums[32], dR[9], dt[3], y[6], angle = 0.0, shift = 0.0;
            if (std::fscanf(fh, "%d %lf %lf %lf %lf", &m, &rho, &c[0], &c[1], &c[2]) != 5) return 4;
            for (int a = 0; a < 32; ++a)
                if (std::fscanf(fh, "%lf", &sums[a]) != 1) return 4;
            const bool ok = align_plane_solve(m, sums, c, rho, dR, dt, angle, shift, y);
            std::printf("S %d", ok ? 1 : 0);
            for (int a = 0; a < 6; ++a) std::printf(" %.17g", y[a]);
            for (int a = 0; a < 9; ++a) std::printf(" %.17g", dR[a]);
            for (int a = 0; a < 3; ++a) std::printf(" %.17g", dt[a]);
            std::printf(" %.17g %.17g\n", angle, shift);
        } else {
            return 5;
        }
    }
    std::fclose(fh);
    std::printf("done\n");
    return 0;
}
