// A watertight mesh from the winding field of an oriented cloud on gfx950: the level set |w| = level of section 26's winding
// number, extracted by marching tetrahedra on a lattice of 8 x 8 x 8-cell blocks that follows the surface.
//
//   etch_cloud_mesh_lattice       the lattice [lo, hi) of every cloud, in blocks, and its status
//   etch_cloud_mesh_seed          marks the blocks that hold a row (dilated) in the dense block table
//   etch_cloud_mesh_field         s = |w| - level at the 729 nodes of every listed block: the hot path, cw_tile_kernel's sweep with generated queries
//   etch_cloud_mesh_grow          the face test of the blocks of the last round: marks the neighbours the level set runs into
//   etch_cloud_mesh_extract       triangles per cell, then every triangle as three 63-bit crossing keys and their positions
//   etch_mesh_components          label_v = the lowest vertex of v's component, by hooking and pointer jumping
//   etch_mesh_keep_component      vertices and faces of one component, compacted in order
//
// The scalar arithmetic is cloud_mesh_solve.h's and, for the pair term, cloud_winding_solve.h's.  Determinism: the field has no atomics and its
// sums have section 26a's order, so a node has the same bits in every block that holds it; the table marks are stores of one value; the labels
// use atomicMin on integers, whose fixed point does not depend on the order.  Every count and every order comes from the block table's layout and
// from prefix sums the caller makes between the launches.  The TU is built with -ffp-contract=off.
//
// The staging of the rows is cw_tile_kernel's (cloud_winding.hip), restated here: the file that holds the original keeps its program text.
#include "common.h"
#include "etch_hip.h"
#include "cloud_winding_solve.h"
#include "cloud_mesh_solve.h"
#include <cmath>

#define CM_THREADS 256
#define CM_TILE 256                               // rows staged at a time
#define CM_CHUNK 1024                             // rows added in fp32 before the fp64 sum over the chunks: section 26a's
#define CM_R 3                                    // nodes per thread: 3 x 256 >= 729
#define CM_MARK (-2)                              // block table: marked for the next round; -1 inactive; >= 0 the block's slot

static_assert(CM_R * CM_THREADS >= MESH_BLOCK_NODES, "a workgroup holds a block's nodes");
static_assert(CM_TILE == CM_THREADS, "one thread stages one row of a tile");

namespace {

struct MeshCloud {
    const float *pos, *moment, *cap;
    const int* offsets;
    __device__ __forceinline__ int n(int b) const { return max(offsets[b + 1] - offsets[b], 0); }
};

__device__ __forceinline__ bool cm_row_counts(const float* p, float cap) {
    return cap > 0.f && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
}

// the block with the flat index `flat` of a lattice of (ny, nz) blocks on its last two axes
__device__ __forceinline__ void cm_unflatten(int flat, int ny, int nz, int c[3]) {
    c[2] = flat % nz, c[1] = (flat / nz) % ny, c[0] = flat / (nz * ny);
}

// ---------------------------------------------------------------------------------------------- lattice
// One workgroup per cloud: the extremes of the rows that count in fp64 (strided per thread, then a tree; min and max do not depend on the order).
__global__ __launch_bounds__(CM_THREADS) void cm_lattice_kernel(MeshCloud cloud, double h, int pad, int* __restrict__ lattice, int* __restrict__ status) {
    __shared__ double sm[6][CM_THREADS];
    __shared__ int any[CM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = cloud.n(b);
    const size_t base = (size_t)cloud.offsets[b];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int seen = 0;
    for (int j = tid; j < R; j += CM_THREADS) {
        const float* p = cloud.pos + 3 * (base + j);
        if (!cm_row_counts(p, cloud.cap[base + j])) continue;
        seen = 1;
        for (int k = 0; k < 3; ++k) mn[k] = fmin(mn[k], (double)p[k]), mx[k] = fmax(mx[k], (double)p[k]);
    }
    for (int k = 0; k < 3; ++k) sm[k][tid] = mn[k], sm[3 + k][tid] = mx[k];
    any[tid] = seen;
    __syncthreads();
    for (int s = CM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < 3; ++k) sm[k][tid] = fmin(sm[k][tid], sm[k][tid + s]), sm[3 + k][tid] = fmax(sm[3 + k][tid], sm[3 + k][tid + s]);
            any[tid] |= any[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, st = 0;
        if (!any[0]) st = ETCH_CLOUD_STATUS_EMPTY;
        else {
            const double a[3] = {sm[0][0], sm[1][0], sm[2][0]}, c[3] = {sm[3][0], sm[4][0], sm[5][0]};
            if (!mesh_lattice(a, c, h, pad, lo, hi)) st = ETCH_CLOUD_STATUS_RANGE;
        }
        for (int k = 0; k < 3; ++k) lattice[6 * b + k] = lo[k], lattice[6 * b + 3 + k] = hi[k];
        status[b] = st;
    }
}

// One thread per row: the row's block and its (2 d + 1)^3 neighbourhood, clipped to the lattice, get the mark.  A store of one value.
__global__ __launch_bounds__(CM_THREADS) void cm_seed_kernel(MeshCloud cloud, double h, int dilate, const int* __restrict__ lattice,
                                                             const int* __restrict__ status, const long long* __restrict__ table_offsets,
                                                             int* __restrict__ table) {
    const int b = blockIdx.y, j = blockIdx.x * CM_THREADS + threadIdx.x;
    if (j >= cloud.n(b) || status[b] != 0) return;
    const size_t row = (size_t)cloud.offsets[b] + j;
    const float* p = cloud.pos + 3 * row;
    if (!cm_row_counts(p, cloud.cap[row])) return;
    const int* L = lattice + 6 * b;
    int c[3], n[3];
    for (int k = 0; k < 3; ++k) c[k] = (int)mesh_block_of((double)p[k], h) - L[k], n[k] = L[3 + k] - L[k];
    const long long cells = table_offsets[b + 1] - table_offsets[b];
    for (int dx = -dilate; dx <= dilate; ++dx)
        for (int dy = -dilate; dy <= dilate; ++dy)
            for (int dz = -dilate; dz <= dilate; ++dz) {
                const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                if (x < 0 || y < 0 || z < 0 || x >= n[0] || y >= n[1] || z >= n[2]) continue;
                const long long flat = ((long long)x * n[1] + y) * n[2] + z;
                if (flat < cells) table[table_offsets[b] + flat] = CM_MARK;
            }
}

// ---------------------------------------------------------------------------------------------- the field
// One workgroup per listed block, 256 threads, three nodes per thread in registers (node r 256 + tid; its offsets in the block are
// (node / 81, node / 9 % 9, node % 9)), generated from the block's coordinates: nothing is loaded per query.  The workgroup walks all rows of its
// cloud: 256-row tiles of the seven floats per row in LDS, padded to two float4 and read as wave-uniform 128-bit broadcasts; a chunk of 1024 rows
// is added in fp32 from 0 in ascending order, the chunks in ascending order in fp64 in registers.  That is section 26a's w to the bit, so no
// workspace and no second kernel are needed.  s = fabsf(w) - level.
__global__ __launch_bounds__(CM_THREADS) void cm_field_kernel(int B, MeshCloud cloud, double h, float level, const int* __restrict__ lattice,
                                                              const int* __restrict__ slots, float* __restrict__ field) {
    __shared__ float4 tile[2][CM_TILE];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = slots[2 * s], flat = slots[2 * s + 1];
    if (b < 0 || b >= B) return;                      // uniform
    const int* L = lattice + 6 * b;
    const int ny = L[4] - L[1], nz = L[5] - L[2], nx = L[3] - L[0];
    if (flat < 0 || nx <= 0 || ny <= 0 || nz <= 0 || flat >= nx * ny * nz) return;      // uniform
    int c[3];
    cm_unflatten(flat, ny, nz, c);
    float p[CM_R][3], acc[CM_R];
    double sum[CM_R];
#pragma unroll
    for (int r = 0; r < CM_R; ++r) {
        const int node = min(r * CM_THREADS + tid, MESH_BLOCK_NODES - 1);      // the threads past the block's nodes repeat the last one and store nothing
        const int o[3] = {node / 81, (node / 9) % 9, node % 9};
        for (int k = 0; k < 3; ++k) p[r][k] = mesh_node(8 * (L[k] + c[k]) + o[k], h);
        sum[r] = 0.0;
    }
    const int R = cloud.n(b);
    const size_t base_row = (size_t)cloud.offsets[b];
    for (int f0 = 0; f0 < R; f0 += CM_CHUNK) {
        const int f1 = min(R, f0 + CM_CHUNK);
#pragma unroll
        for (int r = 0; r < CM_R; ++r) acc[r] = 0.f;
        for (int t0 = f0; t0 < f1; t0 += CM_TILE) {
            const int tn = min(CM_TILE, f1 - t0);
            __syncthreads();
            if (tid < tn) {
                const size_t j = base_row + (size_t)(t0 + tid);
                tile[0][tid] = make_float4(cloud.pos[3 * j], cloud.pos[3 * j + 1], cloud.pos[3 * j + 2], cloud.cap[j]);
                tile[1][tid] = make_float4(cloud.moment[3 * j], cloud.moment[3 * j + 1], cloud.moment[3 * j + 2], 0.f);
            }
            __syncthreads();
            for (int k = 0; k < tn; ++k) {
                const float4 a = tile[0][k], m = tile[1][k];
#pragma unroll
                for (int r = 0; r < CM_R; ++r) {
                    const float rx = a.x - p[r][0], ry = a.y - p[r][1], rz = a.z - p[r][2];
                    acc[r] += wind_term(rx, ry, rz, wind_d2(rx, ry, rz), m.x, m.y, m.z, a.w);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CM_R; ++r) sum[r] += (double)acc[r];
    }
#pragma unroll
    for (int r = 0; r < CM_R; ++r) {
        const int node = r * CM_THREADS + tid;
        if (node < MESH_BLOCK_NODES) field[(size_t)s * MESH_BLOCK_NODES + node] = fabsf((float)(sum[r] * WIND_INV_4PI)) - level;
    }
}

// ---------------------------------------------------------------------------------------------- growth
// One wave per block of the last round.  Face f (-x, +x, -y, +y, -z, +z): its 81 nodes are mixed when neither all inside nor all outside.  A mixed
// face marks the neighbour behind it in the table where that is inactive (flag 1), or points out of the lattice (flag 2: clipped).
__global__ __launch_bounds__(64) void cm_grow_kernel(int B, const int* __restrict__ lattice, const long long* __restrict__ table_offsets,
                                                     const int* __restrict__ slots, const float* __restrict__ field, int* __restrict__ table,
                                                     int* __restrict__ flags) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = slots[2 * s], flat = slots[2 * s + 1];
    const int* L = lattice + 6 * (b < 0 || b >= B ? 0 : b);
    const int n[3] = {L[3] - L[0], L[4] - L[1], L[5] - L[2]};
    if (b < 0 || b >= B || flat < 0 || n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || flat >= n[0] * n[1] * n[2]) {      // uniform: no such block
        if (tid < 6) flags[6 * s + tid] = 0;
        return;
    }
    int c[3];
    cm_unflatten(flat, n[1], n[2], c);
    const float* fld = field + (size_t)s * MESH_BLOCK_NODES;
    for (int f = 0; f < 6; ++f) {
        const int axis = f >> 1, fixed = (f & 1) * MESH_BLOCK;
        int in = 0, out = 0;
        for (int i = tid; i < 81; i += 64) {
            const int u = i / 9, v = i % 9;
            const int node = axis == 0 ? fixed * 81 + u * 9 + v : (axis == 1 ? u * 81 + fixed * 9 + v : u * 81 + v * 9 + fixed);
            if (mesh_inside(fld[node])) in = 1;
            else out = 1;
        }
        const bool mixed = __any(in) && __any(out);
        if (tid != 0) continue;
        int flag = 0;
        if (mixed) {
            int nb[3] = {c[0], c[1], c[2]};
            nb[axis] += (f & 1) ? 1 : -1;
            if (nb[axis] < 0 || nb[axis] >= n[axis]) flag = 2;
            else {
                const long long at = table_offsets[b] + ((long long)nb[0] * n[1] + nb[1]) * n[2] + nb[2];
                if (table[at] < 0) table[at] = CM_MARK, flag = 1;
            }
        }
        flags[6 * s + f] = flag;
    }
}

// ---------------------------------------------------------------------------------------------- extraction
// One workgroup per block, one thread per cell (cz fastest), the block's 729 values in LDS.  offsets == NULL: counts alone.  Otherwise the cell
// writes its triangles at offsets[cell] (the exclusive prefix sum of the counts): tetrahedron 0..5, triangle 0..1, three crossings each.
__global__ __launch_bounds__(MESH_BLOCK_CELLS) void cm_extract_kernel(int B, long long F, const int* __restrict__ lattice, double h,
                                                                      const int* __restrict__ slots, const float* __restrict__ field,
                                                                      int* __restrict__ counts, const long long* __restrict__ offsets,
                                                                      long long* __restrict__ face_keys, float* __restrict__ face_pos) {
    __shared__ float fld[MESH_BLOCK_NODES];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = slots[2 * s], flat = slots[2 * s + 1];
    if (b < 0 || b >= B) return;
    const int* L = lattice + 6 * b;
    const int n[3] = {L[3] - L[0], L[4] - L[1], L[5] - L[2]};
    if (flat < 0 || n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || flat >= n[0] * n[1] * n[2]) return;
    int c[3];
    cm_unflatten(flat, n[1], n[2], c);
    for (int i = tid; i < MESH_BLOCK_NODES; i += MESH_BLOCK_CELLS) fld[i] = field[(size_t)s * MESH_BLOCK_NODES + i];
    __syncthreads();
    const int cell[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
    unsigned corners = 0;
    for (int k = 0; k < 8; ++k) {
        const int node = (cell[0] + ((k >> 2) & 1)) * 81 + (cell[1] + ((k >> 1) & 1)) * 9 + cell[2] + (k & 1);
        corners |= (unsigned)mesh_inside(fld[node]) << k;
    }
    unsigned entry[6];
    int count = 0;
    for (int t = 0; t < 6; ++t) {
        entry[t] = mesh_tet_entry(t, mesh_tet_case(t, corners));
        count += mesh_entry_triangles(entry[t]);
    }
    if (counts) counts[(size_t)s * MESH_BLOCK_CELLS + tid] = count;
    if (!offsets || count == 0) return;
    long long at = offsets[(size_t)s * MESH_BLOCK_CELLS + tid];
    if (at < 0 || at + count > F) return;             // a prefix that does not belong to these counts writes nothing
    for (int t = 0; t < 6; ++t)
        for (int k = 0; k < mesh_entry_triangles(entry[t]); ++k, ++at)
            for (int j = 0; j < 3; ++j) {
                const int e = mesh_entry_edge(entry[t], k, j);
                const int ca = mesh_tet_corner(t, mesh_edge_lo(e)), kind = mesh_tet_corner(t, mesh_edge_up(e)) - ca;
                const int nl[3] = {cell[0] + ((ca >> 2) & 1), cell[1] + ((ca >> 1) & 1), cell[2] + (ca & 1)};
                const int d[3] = {(kind >> 2) & 1, (kind >> 1) & 1, kind & 1};
                const float s_n = fld[nl[0] * 81 + nl[1] * 9 + nl[2]], s_up = fld[(nl[0] + d[0]) * 81 + (nl[1] + d[1]) * 9 + nl[2] + d[2]];
                const float tt = mesh_cross_t(s_n, s_up);
                int i[3];
                for (int a = 0; a < 3; ++a) {
                    i[a] = 8 * c[a] + nl[a];
                    const int g = 8 * L[a] + i[a];
                    face_pos[((size_t)at * 3 + j) * 3 + a] = mesh_cross(mesh_node(g, h), mesh_node(g + d[a], h), tt, d[a]);
                }
                face_keys[(size_t)at * 3 + j] = mesh_key(i[0], i[1], i[2], kind);
            }
}

// ---------------------------------------------------------------------------------------------- components
__global__ __launch_bounds__(256) void cc_init_kernel(int V, int* __restrict__ labels) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) labels[v] = v;
}

__global__ void cc_zero_kernel(int* __restrict__ word) {
    if (threadIdx.x == 0) *word = 0;
}

// Hooking: every vertex of a face, and the vertex its label names, take the least label of the face.  Labels only fall, and a label always names a
// vertex of the same component, so the fixed point -- every vertex carries its component's lowest index -- does not depend on the order.
__global__ __launch_bounds__(256) void cc_hook_kernel(int V, int F, const int* __restrict__ faces, int* __restrict__ labels, int* __restrict__ changed) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int v[3], l[3];
    for (int k = 0; k < 3; ++k) {
        v[k] = faces[3 * (size_t)f + k];
        if (v[k] < 0 || v[k] >= V) return;
    }
    for (int k = 0; k < 3; ++k) l[k] = labels[v[k]];
    const int m = min(l[0], min(l[1], l[2]));
    bool ch = false;
    for (int k = 0; k < 3; ++k) {
        if (l[k] < 0 || l[k] >= V) continue;
        if (atomicMin(labels + v[k], m) > m) ch = true;
        if (atomicMin(labels + l[k], m) > m) ch = true;
    }
    if (ch) *changed = 1;
}

// Pointer jumping: every vertex takes the label at the end of its chain.  Chains descend strictly, so the walk ends.
__global__ __launch_bounds__(256) void cc_jump_kernel(int V, int* __restrict__ labels) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int l = labels[v];
    while (l >= 0 && l < V) {
        const int up = labels[l];
        if (up >= l) break;
        l = up;
    }
    labels[v] = l;
}

__global__ __launch_bounds__(256) void cc_keep_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces,
                                                      const int* __restrict__ labels, int label, const long long* __restrict__ vert_prefix,
                                                      const long long* __restrict__ face_prefix, long long Vk, long long Fk, float* __restrict__ out_verts,
                                                      int* __restrict__ out_faces) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < V && labels[t] == label) {
        const long long at = vert_prefix[t] - 1;
        if (at >= 0 && at < Vk)
            for (int k = 0; k < 3; ++k) out_verts[3 * at + k] = verts[3 * (size_t)t + k];
    }
    if (t < F) {
        const int a = faces[3 * (size_t)t];
        if (a >= 0 && a < V && labels[a] == label) {
            const long long at = face_prefix[t] - 1;
            if (at >= 0 && at < Fk)
                for (int k = 0; k < 3; ++k) {
                    const int v = faces[3 * (size_t)t + k];
                    out_faces[3 * at + k] = v >= 0 && v < V ? (int)(vert_prefix[v] - 1) : -1;
                }
        }
    }
}

bool cm_cloud_ok(int B, int max_rows, const float* pos, const float* cap, const int* offsets) {
    return B >= 0 && max_rows >= 0 && offsets && (max_rows == 0 || (pos && cap));
}

}  // namespace

extern "C" {

int etch_cloud_mesh_lattice(int B, int max_rows, const float* pos, const float* cap, const int* offsets, double voxel, int pad_blocks, int* lattice,
                            int* status, void* stream) {
    if (!cm_cloud_ok(B, max_rows, pos, cap, offsets) || !(voxel > 0.0) || !std::isfinite(voxel) || pad_blocks < 0 || pad_blocks > 64) return ETCH_EINVAL;
    if (B == 0) return ETCH_OK;
    if (!lattice || !status) return ETCH_EINVAL;
    hipLaunchKernelGGL(cm_lattice_kernel, dim3(B), dim3(CM_THREADS), 0, (hipStream_t)stream, MeshCloud{pos, nullptr, cap, offsets}, voxel, pad_blocks, lattice,
                       status);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_mesh_seed(int B, int max_rows, const float* pos, const float* cap, const int* offsets, double voxel, int seed_dilate, const int* lattice,
                         const int* status, const long long* table_offsets, int* table, void* stream) {
    if (!cm_cloud_ok(B, max_rows, pos, cap, offsets) || !(voxel > 0.0) || !std::isfinite(voxel) || seed_dilate < 0 || seed_dilate > 2) return ETCH_EINVAL;
    if (B == 0 || max_rows == 0) return ETCH_OK;
    if (!lattice || !status || !table_offsets || !table) return ETCH_EINVAL;
    hipLaunchKernelGGL(cm_seed_kernel, dim3((max_rows + CM_THREADS - 1) / CM_THREADS, B), dim3(CM_THREADS), 0, (hipStream_t)stream,
                       MeshCloud{pos, nullptr, cap, offsets}, voxel, seed_dilate, lattice, status, table_offsets, table);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_mesh_field(int B, int S, int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, double voxel, float level,
                          const int* lattice, const int* slots, float* field, void* stream) {
    if (!cm_cloud_ok(B, max_rows, pos, cap, offsets) || S < 0 || !(voxel > 0.0) || !std::isfinite(voxel) || (max_rows > 0 && !moment)) return ETCH_EINVAL;
    if (S == 0) return ETCH_OK;
    if (!lattice || !slots || !field) return ETCH_EINVAL;
    hipLaunchKernelGGL(cm_field_kernel, dim3(S), dim3(CM_THREADS), 0, (hipStream_t)stream, B, MeshCloud{pos, moment, cap, offsets}, voxel, level, lattice, slots,
                       field);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_mesh_grow(int B, int S, const int* lattice, const long long* table_offsets, const int* slots, const float* field, int* table, int* flags,
                         void* stream) {
    if (B < 0 || S < 0) return ETCH_EINVAL;
    if (S == 0) return ETCH_OK;
    if (!lattice || !table_offsets || !slots || !field || !table || !flags) return ETCH_EINVAL;
    hipLaunchKernelGGL(cm_grow_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, B, lattice, table_offsets, slots, field, table, flags);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_mesh_extract(int B, int S, long long F, const int* lattice, double voxel, const int* slots, const float* field, int* counts,
                            const long long* cell_offsets, long long* face_keys, float* face_pos, void* stream) {
    if (B < 0 || S < 0 || F < 0 || !(voxel > 0.0) || !std::isfinite(voxel)) return ETCH_EINVAL;
    if (S == 0) return ETCH_OK;
    if (!lattice || !slots || !field || (!counts && !cell_offsets) || (cell_offsets && F > 0 && (!face_keys || !face_pos))) return ETCH_EINVAL;
    hipLaunchKernelGGL(cm_extract_kernel, dim3(S), dim3(MESH_BLOCK_CELLS), 0, (hipStream_t)stream, B, F, lattice, voxel, slots, field, counts,
                       F > 0 ? cell_offsets : nullptr, face_keys, face_pos);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_mesh_components(int V, int F, const int* faces, int init, int passes, int* labels, int* changed, void* stream) {
    if (V < 0 || F < 0 || passes < 0 || !changed) return ETCH_EINVAL;
    if ((V > 0 && !labels) || (F > 0 && !faces)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const unsigned vb = (unsigned)((V + 255) / 256), fb = (unsigned)((F + 255) / 256);
    hipLaunchKernelGGL(cc_zero_kernel, dim3(1), dim3(64), 0, st, changed);
    if (init && V > 0) hipLaunchKernelGGL(cc_init_kernel, dim3(vb), dim3(256), 0, st, V, labels);
    for (int p = 0; p < passes && V > 0 && F > 0; ++p) {
        hipLaunchKernelGGL(cc_hook_kernel, dim3(fb), dim3(256), 0, st, V, F, faces, labels, changed);
        hipLaunchKernelGGL(cc_jump_kernel, dim3(vb), dim3(256), 0, st, V, labels);
    }
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_mesh_keep_component(int V, int F, const float* verts, const int* faces, const int* labels, int label, const long long* vert_prefix,
                             const long long* face_prefix, long long kept_verts, long long kept_faces, float* out_verts, int* out_faces, void* stream) {
    if (V < 0 || F < 0 || kept_verts < 0 || kept_faces < 0 || kept_verts > V || kept_faces > F) return ETCH_EINVAL;
    if (V == 0) return ETCH_OK;
    if (!verts || !labels || !vert_prefix || (F > 0 && (!faces || !face_prefix)) || (kept_verts > 0 && !out_verts) || (kept_faces > 0 && !out_faces))
        return ETCH_EINVAL;
    const int n = V > F ? V : F;
    hipLaunchKernelGGL(cc_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, F, verts, faces, labels, label, vert_prefix,
                       face_prefix, kept_verts, kept_faces, out_verts, out_faces);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
