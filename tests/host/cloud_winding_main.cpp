// Drives etch_amd/csrc/cloud_winding_solve.h on the host (tests/test_cloud_winding_host.py builds it with the address and undefined-behaviour
// sanitizers): one case per input line, one output line per case, "done" at the end.
//   A d2k ke flag px py pz                 -> the area
//   P px py pz cx cy cz nx ny nz a         -> pos[3] moment[3] cap
//   T qx qy qz px py pz mx my mz cap       -> d2 term                      (every value an fp32)
//   K d2 row                               -> key row d2                   (the key, and what wind_unkey makes of it)
//   M a b                                  -> the merged key
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "cloud_winding_solve.h"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 3;
    std::vector<char> buf(1 << 16);
    while (std::fgets(buf.data(), (int)buf.size(), fh)) {
        std::istringstream in(buf.data());
        std::string kind, tok;
        in >> kind;
        std::vector<std::string> v;
        while (in >> tok) v.push_back(tok);
        auto d = [&](size_t i) { return std::strtod(v.at(i).c_str(), nullptr); };
        auto f = [&](size_t i) { return (float)std::strtod(v.at(i).c_str(), nullptr); };
        if (kind == "A") {
            std::printf("A %.17g\n", wind_area(d(0), (int)d(1), (int)d(2), d(3), d(4), d(5)));
        } else if (kind == "P") {
            const double p[3] = {d(0), d(1), d(2)}, c[3] = {d(3), d(4), d(5)}, n[3] = {d(6), d(7), d(8)};
            float pos[3], mom[3], cap;
            wind_pack(p, c, n, d(9), pos, mom, cap);
            std::printf("P %u %u %u %u %u %u %u\n", bits(pos[0]), bits(pos[1]), bits(pos[2]), bits(mom[0]), bits(mom[1]), bits(mom[2]), bits(cap));
        } else if (kind == "T") {
            const float rx = f(3) - f(0), ry = f(4) - f(1), rz = f(5) - f(2);
            const float d2 = wind_d2(rx, ry, rz);
            std::printf("T %u %u\n", bits(d2), bits(wind_term(rx, ry, rz, d2, f(6), f(7), f(8), f(9))));
        } else if (kind == "K") {
            const unsigned long long key = wind_key(f(0), (int)d(1));
            int row;
            float d2;
            wind_unkey(key, row, d2);
            std::printf("K %" PRIu64 " %d %u\n", (uint64_t)key, row, bits(d2));
        } else if (kind == "M") {
            std::printf("M %" PRIu64 "\n", (uint64_t)wind_merge(std::strtoull(v.at(0).c_str(), nullptr, 10), std::strtoull(v.at(1).c_str(), nullptr, 10)));
        } else {
            return 4;
        }
    }
    std::fclose(fh);
    std::printf("done\n");
    return 0;
}
