// Drives etch_amd/csrc/cloud_mesh_solve.h on the host (tests/test_cloud_mesh_host.py builds it with the address and undefined-behaviour
// sanitizers): one case per input line, one output line per case, "done" at the end.
//   E t case                               -> the table entry, its triangle count and its six edge ids
//   C t v                                  -> the corner code of vertex v of tetrahedron t
//   G e                                    -> the two vertices of edge e
//   Q t corners                            -> the case of tetrahedron t for the cell's inside bits
//   N g h                                  -> the bits of the node's position
//   L mnx mny mnz mxx mxy mxz h pad        -> ok lo[3] hi[3]
//   K ix iy iz kind                        -> the key
//   X s_n s_up x_n x_up moves              -> inside(s_n) inside(s_up), the bits of t and of the crossing      (fp32 values given as bits)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "cloud_mesh_solve.h"

static unsigned bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

static float from_bits(unsigned u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
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
        auto n = [&](size_t i) { return (int)std::strtol(v.at(i).c_str(), nullptr, 10); };
        auto fb = [&](size_t i) { return from_bits((unsigned)std::strtoul(v.at(i).c_str(), nullptr, 10)); };
        if (kind == "E") {
            const unsigned e = mesh_tet_entry(n(0), n(1));
            std::printf("E %u %d", e, mesh_entry_triangles(e));
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 3; ++j) std::printf(" %d", mesh_entry_edge(e, k, j));
            std::printf("\n");
        } else if (kind == "C") {
            std::printf("C %d\n", mesh_tet_corner(n(0), n(1)));
        } else if (kind == "G") {
            std::printf("G %d %d\n", mesh_edge_lo(n(0)), mesh_edge_up(n(0)));
        } else if (kind == "Q") {
            std::printf("Q %d\n", mesh_tet_case(n(0), (unsigned)n(1)));
        } else if (kind == "N") {
            std::printf("N %u\n", bits(mesh_node(n(0), d(1))));
        } else if (kind == "L") {
            const double mn[3] = {d(0), d(1), d(2)}, mx[3] = {d(3), d(4), d(5)};
            int lo[3], hi[3];
            const bool ok = mesh_lattice(mn, mx, d(6), n(7), lo, hi);
            std::printf("L %d %d %d %d %d %d %d\n", (int)ok, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
        } else if (kind == "K") {
            std::printf("K %" PRId64 "\n", (int64_t)mesh_key(n(0), n(1), n(2), n(3)));
        } else if (kind == "X") {
            const float t = mesh_cross_t(fb(0), fb(1));
            std::printf("X %d %d %u %u\n", (int)mesh_inside(fb(0)), (int)mesh_inside(fb(1)), bits(t), bits(mesh_cross(fb(2), fb(3), t, n(4))));
        } else {
            return 4;
        }
    }
    std::fclose(fh);
    std::printf("done\n");
    return 0;
}
