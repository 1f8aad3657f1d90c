// The definitions of cloud_mesh.hip in plain C++, for the device and for a host build alike: the lattice a cloud's blocks
// live on, a node's position, the marching-tetrahedra table of the Freudenthal split, the key of a crossing and its position.  The lattice is
// fp64 with one rounding per node coordinate; a crossing is three fp32 operations per axis, one rounding each (the including file is built with
// -ffp-contract=off).  tests/_cloud_mesh_oracle.py GENERATES the table from its rule and restates every function with numpy.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define MESH_HD __host__ __device__ __forceinline__
#else
#define MESH_HD inline
#endif

#define MESH_BLOCK 8                             // cells per block and axis
#define MESH_NODES 9                             // nodes per block and axis: the face nodes are shared with the neighbours
#define MESH_BLOCK_NODES 729
#define MESH_BLOCK_CELLS 512
#define MESH_MAX_NODES ((1 << 20) - 1)           // nodes per axis of a lattice
#define MESH_MAX_BLOCKS (1 << 24)                // blocks of a lattice
#define MESH_MAX_COORD 134217728.0               // 2^27: |lo| and |hi| stay below it, so 8 lo fits an int32 with room

// a node's position on one axis: fp32((double) g h)
MESH_HD float mesh_node(int g, double h) { return (float)((double)g * h); }

// the block that holds the coordinate x: floor(x / (8 h)) in fp64
MESH_HD double mesh_block_of(double x, double h) { return std::floor(x / (8.0 * h)); }

// lo = floor(min / (8h)) - pad, hi = floor(max / (8h)) + 1 + pad per axis, from the extremes of the rows that count.  false: out of range.
MESH_HD bool mesh_lattice(const double mn[3], const double mx[3], double h, int pad, int lo[3], int hi[3]) {
    double blocks = 1.0;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const double l = mesh_block_of(mn[k], h) - (double)pad, u = mesh_block_of(mx[k], h) + 1.0 + (double)pad;
        const double n = u - l;
        if (!(std::fabs(l) < MESH_MAX_COORD) || !(std::fabs(u) < MESH_MAX_COORD) || 8.0 * n + 1.0 > (double)MESH_MAX_NODES) ok = false;
        blocks *= n;
        lo[k] = ok ? (int)l : 0, hi[k] = ok ? (int)u : 0;
    }
    if (!ok || blocks > (double)MESH_MAX_BLOCKS) {
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = 0;
        return false;
    }
    return true;
}

// inside iff !(s < 0): a NaN counts as inside (section 18's convention), and so do 0 and -0
MESH_HD bool mesh_inside(float s) { return !(s < 0.f); }

// the corner code 4 dx + 2 dy + dz of vertex v of tetrahedron t: 000, e_p0, e_p0 + e_p1, 111 with (p0, p1, p2) the t-th permutation of the axes in
// lexicographic order
MESH_HD int mesh_tet_corner(int t, int v) {
    constexpr unsigned char C[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
    return C[t][v];
}

// a tetrahedron's edge e as its two vertices, the lower first: (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)
MESH_HD int mesh_edge_lo(int e) { return e < 3 ? 0 : (e < 5 ? 1 : 2); }
MESH_HD int mesh_edge_up(int e) { return e < 3 ? e + 1 : (e < 5 ? e - 1 : 3); }

// The case table: bit v of the case is set when vertex v is inside.  An entry holds the number of triangles in bits 0..1 and then three bits per
// edge, the three edges of triangle 0 first.  The triangles point from the inside vertices to the outside ones.
MESH_HD unsigned mesh_tet_entry(int t, int c) {
    constexpr unsigned T[6][16] = {
        {0x00000u, 0x00221u, 0x00381u, 0x70c46u, 0x00565u, 0xac2a2u, 0x34582u, 0x00589u, 0x004a9u, 0x94522u, 0xa83a2u, 0x003a5u, 0x50c66u, 0x00461u, 0x00141u, 0x00000u},
        {0x00000u, 0x00141u, 0x00461u, 0x8ca86u, 0x003a5u, 0x74542u, 0xa44a2u, 0x004a9u, 0x00589u, 0xb01a2u, 0x54562u, 0x00565u, 0x88b86u, 0x00381u, 0x00221u, 0x00000u},
        {0x00000u, 0x00141u, 0x00461u, 0x8ca86u, 0x003a5u, 0x74542u, 0xa44a2u, 0x004a9u, 0x00589u, 0xb01a2u, 0x54562u, 0x00565u, 0x88b86u, 0x00381u, 0x00221u, 0x00000u},
        {0x00000u, 0x00221u, 0x00381u, 0x70c46u, 0x00565u, 0xac2a2u, 0x34582u, 0x00589u, 0x004a9u, 0x94522u, 0xa83a2u, 0x003a5u, 0x50c66u, 0x00461u, 0x00141u, 0x00000u},
        {0x00000u, 0x00221u, 0x00381u, 0x70c46u, 0x00565u, 0xac2a2u, 0x34582u, 0x00589u, 0x004a9u, 0x94522u, 0xa83a2u, 0x003a5u, 0x50c66u, 0x00461u, 0x00141u, 0x00000u},
        {0x00000u, 0x00141u, 0x00461u, 0x8ca86u, 0x003a5u, 0x74542u, 0xa44a2u, 0x004a9u, 0x00589u, 0xb01a2u, 0x54562u, 0x00565u, 0x88b86u, 0x00381u, 0x00221u, 0x00000u}};
    return T[t][c];
}
MESH_HD int mesh_entry_triangles(unsigned e) { return (int)(e & 3u); }
MESH_HD int mesh_entry_edge(unsigned e, int tri, int j) { return (int)((e >> (2 + 3 * (3 * tri + j))) & 7u); }

// the case of tetrahedron t of a cell whose corners' inside bits are `corners` (bit = corner code)
MESH_HD int mesh_tet_case(int t, unsigned corners) {
    int c = 0;
    for (int v = 0; v < 4; ++v) c |= (int)((corners >> mesh_tet_corner(t, v)) & 1u) << v;
    return c;
}

// the 63-bit key of the crossing on the edge that starts at the node i (local to the lattice, every coordinate in [0, 2^20)) and has the kind 1..7
MESH_HD long long mesh_key(int ix, int iy, int iz, int kind) {
    return (((((long long)ix << 20) + (long long)iy) << 20) + (long long)iz) * 8 + (long long)kind;
}

// the crossing on one axis: t = s_n / (s_n - s_up), x = x_n + t (x_up - x_n), from the lower end whichever end is inside; an axis the edge does not
// move along keeps x_n
MESH_HD float mesh_cross_t(float s_n, float s_up) { return s_n / (s_n - s_up); }
MESH_HD float mesh_cross(float x_n, float x_up, float t, int moves) { return moves ? x_n + t * (x_up - x_n) : x_n; }
