// Brute-force mesh geometry in fp64 on gfx950: the tightness supervision of the training data (scripts/generate_infopoints.py and the
// vector half of GTDataset.__getitem__, src/data_utils/GT_dataloader.py:95-122).
//
//   etch_ray_first_hit          first hit of R rays against a triangle mesh (Moller-Trumbore)
//   etch_closest_point_on_mesh  closest point of P points on a triangle mesh (Ericson, Real-Time Collision Detection 5.1.5)
//   etch_vertex_normals         trimesh's angle-weighted vertex normals, summed in a fixed per-vertex order
//   etch_remove_close           trimesh 4.x points.remove_close, the thinning step of sample_surface_even
//
// Every result is bit-defined.  The TU is built with -ffp-contract=off, so each expression below is evaluated exactly as written, one rounding
// per operation, and tests/_raycast_oracle.py restates it term by term in numpy.  No atomics touch a value: the mesh kernels write one
// candidate per (face chunk, query) and a final kernel reduces the chunks in ascending order, so the result does not depend on the launch shape.
#include "common.h"
#include "etch_hip.h"
#include "closest_tri.h"

#define RC_BLOCK 256                 // queries per workgroup, one per lane
#define RC_TILE 256                  // faces (points) staged in LDS per step
#define RC_CHUNK 2048                // faces per workgroup along grid.y (a result never depends on it)

static inline unsigned rc_nblk(long n) { return (unsigned)((n + RC_BLOCK - 1) / RC_BLOCK); }
static inline int rc_nchunk(int F) { return (F + RC_CHUNK - 1) / RC_CHUNK; }

__device__ __forceinline__ double rc_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// ---------------------------------------------------------------------------------------------- ray / triangle
// Moller-Trumbore, operation order (e1 = v1 - v0, e2 = v2 - v0 componentwise):
//   p   = cross(d, e2)   px = dy*e2z - dz*e2y,  py = dz*e2x - dx*e2z,  pz = dx*e2y - dy*e2x
//   det = (e1x*px + e1y*py) + e1z*pz;           det == 0 (ray parallel to the plane) is a miss
//   inv = 1 / det
//   s   = o - v0;  u = ((sx*px + sy*py) + sz*pz) * inv
//   q   = cross(s, e1)   qx = sy*e1z - sz*e1y,  qy = sz*e1x - sx*e1z,  qz = sx*e1y - sy*e1x
//   v   = ((dx*qx + dy*qy) + dz*qz) * inv
//   t   = ((e2x*qx + e2y*qy) + e2z*qz) * inv
//   hit iff u >= 0, v >= 0, u + v <= 1, t > 0 and t < t_max (a NaN fails every test: a miss)
struct RcHit {
    double t, u, v;
    bool hit;
};

__device__ __forceinline__ RcHit rc_intersect(double ox, double oy, double oz, double dx, double dy, double dz, double v0x, double v0y, double v0z,
                                              double e1x, double e1y, double e1z, double e2x, double e2y, double e2z, double tmax) {
    RcHit h;
    const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const double det = rc_dot(e1x, e1y, e1z, px, py, pz);
    const double inv = 1.0 / det;
    const double sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
    h.u = rc_dot(sx, sy, sz, px, py, pz) * inv;
    const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    h.v = rc_dot(dx, dy, dz, qx, qy, qz) * inv;
    h.t = rc_dot(e2x, e2y, e2z, qx, qy, qz) * inv;
    h.hit = det != 0.0 && h.u >= 0.0 && h.v >= 0.0 && h.u + h.v <= 1.0 && h.t > 0.0 && h.t < tmax;
    return h;
}

// One lane per ray, a workgroup per (256 rays, 2048-face chunk).  Each 256-face tile is staged in LDS as (v0, e1, e2) and read as wave-uniform
// broadcasts.  Ascending faces with a strict < keep the lowest face among equal t.  Output per (chunk, ray): t (+inf = none) and the face.
__global__ void __launch_bounds__(RC_BLOCK) rc_ray_chunk_kernel(int R, int F, const double* __restrict__ orig, const double* __restrict__ dir,
                                                              const double* __restrict__ V, const int* __restrict__ faces, const int* __restrict__ excl,
                                                              const double* __restrict__ tmax, double* __restrict__ ct, int* __restrict__ cf) {
    __shared__ double tri[9][RC_TILE];
    const int r = blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool ok = r < R;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 1, tm = INF;
    int ex = -1;
    if (ok) {
        ox = orig[(size_t)r * 3]; oy = orig[(size_t)r * 3 + 1]; oz = orig[(size_t)r * 3 + 2];
        dx = dir[(size_t)r * 3]; dy = dir[(size_t)r * 3 + 1]; dz = dir[(size_t)r * 3 + 2];
        if (tmax) tm = tmax[r];
        if (excl) ex = excl[r];
    }
    double best = INF;
    int bf = -1;
    const int f0 = blockIdx.y * RC_CHUNK, f1 = min(F, f0 + RC_CHUNK);
    for (int t0 = f0; t0 < f1; t0 += RC_TILE) {
        const int tn = min(RC_TILE, f1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < tn) {
            const int f = t0 + threadIdx.x;
            const int* fv = faces + (size_t)f * 3;
            const double* a = V + (size_t)fv[0] * 3;
            const double* b = V + (size_t)fv[1] * 3;
            const double* c = V + (size_t)fv[2] * 3;
            tri[0][threadIdx.x] = a[0]; tri[1][threadIdx.x] = a[1]; tri[2][threadIdx.x] = a[2];
            tri[3][threadIdx.x] = b[0] - a[0]; tri[4][threadIdx.x] = b[1] - a[1]; tri[5][threadIdx.x] = b[2] - a[2];
            tri[6][threadIdx.x] = c[0] - a[0]; tri[7][threadIdx.x] = c[1] - a[1]; tri[8][threadIdx.x] = c[2] - a[2];
        }
        __syncthreads();
        if (ok) {
            for (int k = 0; k < tn; ++k) {
                const RcHit h = rc_intersect(ox, oy, oz, dx, dy, dz, tri[0][k], tri[1][k], tri[2][k], tri[3][k], tri[4][k], tri[5][k], tri[6][k],
                                             tri[7][k], tri[8][k], tm);
                if (h.hit && h.t < best && t0 + k != ex) { best = h.t; bf = t0 + k; }
            }
        }
    }
    if (ok) {
        ct[(size_t)blockIdx.y * R + r] = best;
        cf[(size_t)blockIdx.y * R + r] = bf;
    }
}

// chunks in ascending order with a strict <: the smallest t, then the lowest face.  The chosen face is intersected again for u, v (the same
// function on the same inputs: the same bits).
__global__ void __launch_bounds__(RC_BLOCK) rc_ray_final_kernel(int R, int nchunk, const double* __restrict__ orig, const double* __restrict__ dir,
                                                              const double* __restrict__ V, const int* __restrict__ faces, const double* __restrict__ ct,
                                                              const int* __restrict__ cf, int* __restrict__ face, double* __restrict__ t,
                                                              double* __restrict__ bary, double* __restrict__ loc) {
    const int r = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (r >= R) return;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double best = INF;
    int bf = -1;
    for (int c = 0; c < nchunk; ++c) {
        const int f = cf[(size_t)c * R + r];
        const double tc = ct[(size_t)c * R + r];
        if (f >= 0 && tc < best) { best = tc; bf = f; }
    }
    face[r] = bf;
    if (bf < 0) {
        t[r] = INF;
        for (int i = 0; i < 3; ++i) { bary[(size_t)r * 3 + i] = 0.0; if (loc) loc[(size_t)r * 3 + i] = 0.0; }
        return;
    }
    const double ox = orig[(size_t)r * 3], oy = orig[(size_t)r * 3 + 1], oz = orig[(size_t)r * 3 + 2];
    const double dx = dir[(size_t)r * 3], dy = dir[(size_t)r * 3 + 1], dz = dir[(size_t)r * 3 + 2];
    const int* fv = faces + (size_t)bf * 3;
    const double* a = V + (size_t)fv[0] * 3;
    const double* b = V + (size_t)fv[1] * 3;
    const double* c = V + (size_t)fv[2] * 3;
    const RcHit h = rc_intersect(ox, oy, oz, dx, dy, dz, a[0], a[1], a[2], b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - a[0], c[1] - a[1],
                                 c[2] - a[2], INF);
    t[r] = h.t;
    bary[(size_t)r * 3] = (1.0 - h.u) - h.v;
    bary[(size_t)r * 3 + 1] = h.u;
    bary[(size_t)r * 3 + 2] = h.v;
    if (loc) {                                       // o + t d
        loc[(size_t)r * 3] = ox + h.t * dx;
        loc[(size_t)r * 3 + 1] = oy + h.t * dy;
        loc[(size_t)r * 3 + 2] = oz + h.t * dz;
    }
}

// ---------------------------------------------------------------------------------------------- point / triangle
// Ericson 5.1.5 ClosestPtPointTriangle: the region test and its operation order are stated in closest_tri.h (shared with the fp32 surface fit);
// this TU uses the fp64 instantiation.
typedef RcClosestT<double> RcClosest;

__device__ __forceinline__ RcClosest rc_closest(const double* p, const double* a, const double* b, const double* c) {
    return rc_closest_t<double>(p, a, b, c);
}

// One lane per point, a workgroup per (256 points, 2048-face chunk); each tile's (a, b, c) in LDS.  Output per (chunk, point): d2, face.
__global__ void __launch_bounds__(RC_BLOCK) rc_closest_chunk_kernel(int P, int F, const double* __restrict__ pts, const double* __restrict__ V,
                                                                  const int* __restrict__ faces, double* __restrict__ cd, int* __restrict__ cf) {
    __shared__ double tri[9][RC_TILE];
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool ok = i < P;
    double p[3] = {0.0, 0.0, 0.0};
    if (ok) for (int c = 0; c < 3; ++c) p[c] = pts[(size_t)i * 3 + c];
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int bf = -1;
    const int f0 = blockIdx.y * RC_CHUNK, f1 = min(F, f0 + RC_CHUNK);
    for (int t0 = f0; t0 < f1; t0 += RC_TILE) {
        const int tn = min(RC_TILE, f1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < tn) {
            const int* fv = faces + (size_t)(t0 + threadIdx.x) * 3;
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) tri[3 * k + c][threadIdx.x] = V[(size_t)fv[k] * 3 + c];
        }
        __syncthreads();
        if (ok) {
            for (int k = 0; k < tn; ++k) {
                const double a[3] = {tri[0][k], tri[1][k], tri[2][k]}, b[3] = {tri[3][k], tri[4][k], tri[5][k]}, c[3] = {tri[6][k], tri[7][k], tri[8][k]};
                const RcClosest o = rc_closest(p, a, b, c);
                if (o.d2 < best) { best = o.d2; bf = t0 + k; }
            }
        }
    }
    if (ok) {
        cd[(size_t)blockIdx.y * P + i] = best;
        cf[(size_t)blockIdx.y * P + i] = bf;
    }
}

__global__ void __launch_bounds__(RC_BLOCK) rc_closest_final_kernel(int P, int nchunk, const double* __restrict__ pts, const double* __restrict__ V,
                                                                  const int* __restrict__ faces, const double* __restrict__ cd, const int* __restrict__ cf,
                                                                  int* __restrict__ face, double* __restrict__ bary, double* __restrict__ q,
                                                                  double* __restrict__ d2) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= P) return;
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int bf = -1;
    for (int c = 0; c < nchunk; ++c) {
        const int f = cf[(size_t)c * P + i];
        const double dc = cd[(size_t)c * P + i];
        if (f >= 0 && dc < best) { best = dc; bf = f; }
    }
    face[i] = bf;
    if (bf < 0) {
        d2[i] = __longlong_as_double(0x7ff0000000000000ll);
        for (int c = 0; c < 3; ++c) { bary[(size_t)i * 3 + c] = 0.0; q[(size_t)i * 3 + c] = 0.0; }
        return;
    }
    const double p[3] = {pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]};
    const int* fv = faces + (size_t)bf * 3;
    const RcClosest o = rc_closest(p, V + (size_t)fv[0] * 3, V + (size_t)fv[1] * 3, V + (size_t)fv[2] * 3);
    for (int c = 0; c < 3; ++c) { bary[(size_t)i * 3 + c] = o.b[c]; q[(size_t)i * 3 + c] = o.q[c]; }
    d2[i] = o.d2;
}

// ---------------------------------------------------------------------------------------------- vertex normals
// Per face: n = cross(v1 - v0, v2 - v0) / |.| (0 for a zero-area face); the corner angles of trimesh.triangles.angles:
// u = unit(v1 - v0), v = unit(v2 - v0), w = unit(v2 - v1) (a zero vector stays 0), a0 = acos(clip(dot(u, v))), a1 = acos(clip(dot(-u, w))),
// a2 = (pi - a0) - a1, NaN -> 0.  |x| = sqrt((x*x + y*y) + z*z), unit(x) = x / |x| componentwise.
__device__ __forceinline__ void rc_unit(double& x, double& y, double& z) {
    const double n = sqrt(rc_dot(x, y, z, x, y, z));
    if (n > 0.0) { x = x / n; y = y / n; z = z / n; }
}

__global__ void __launch_bounds__(RC_BLOCK) rc_face_normal_kernel(int F, const double* __restrict__ V, const int* __restrict__ faces,
                                                                double* __restrict__ fn, double* __restrict__ ang) {
    const int f = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int* fv = faces + (size_t)f * 3;
    const double* a = V + (size_t)fv[0] * 3;
    const double* b = V + (size_t)fv[1] * 3;
    const double* c = V + (size_t)fv[2] * 3;
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = sqrt(rc_dot(nx, ny, nz, nx, ny, nz));
    if (len > 0.0) { nx = nx / len; ny = ny / len; nz = nz / len; }
    else { nx = 0.0; ny = 0.0; nz = 0.0; }
    fn[(size_t)f * 3] = nx; fn[(size_t)f * 3 + 1] = ny; fn[(size_t)f * 3 + 2] = nz;
    double ux = e1x, uy = e1y, uz = e1z, vx = e2x, vy = e2y, vz = e2z;
    double wx = c[0] - b[0], wy = c[1] - b[1], wz = c[2] - b[2];
    rc_unit(ux, uy, uz); rc_unit(vx, vy, vz); rc_unit(wx, wy, wz);
    double a0 = acos(fmin(fmax(rc_dot(ux, uy, uz, vx, vy, vz), -1.0), 1.0));
    double a1 = acos(fmin(fmax(rc_dot(-ux, -uy, -uz, wx, wy, wz), -1.0), 1.0));
    double a2 = (3.141592653589793 - a0) - a1;
    if (a0 != a0) a0 = 0.0;
    if (a1 != a1) a1 = 0.0;
    if (a2 != a2) a2 = 0.0;
    ang[(size_t)f * 3] = a0; ang[(size_t)f * 3 + 1] = a1; ang[(size_t)f * 3 + 2] = a2;
}

// vertex i: s = 0; for each (face f, corner k) of csr_idx[csr_ptr[i] .. csr_ptr[i+1]) in order, s = s + fn[f] * ang[f][k] (componentwise);
// out = unit(s).  csr_idx holds 3 f + k.
__global__ void __launch_bounds__(RC_BLOCK) rc_vertex_normal_kernel(int Vn, const int* __restrict__ csr_ptr, const int* __restrict__ csr_idx,
                                                                  const double* __restrict__ fn, const double* __restrict__ ang, double* __restrict__ out) {
    const int i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= Vn) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int e = csr_ptr[i]; e < csr_ptr[i + 1]; ++e) {
        const int fk = csr_idx[e], f = fk / 3;
        const double w = ang[fk];
        sx = sx + fn[(size_t)f * 3] * w;
        sy = sy + fn[(size_t)f * 3 + 1] * w;
        sz = sz + fn[(size_t)f * 3 + 2] * w;
    }
    rc_unit(sx, sy, sz);
    out[(size_t)i * 3] = sx; out[(size_t)i * 3 + 1] = sy; out[(size_t)i * 3 + 2] = sz;
}

// ---------------------------------------------------------------------------------------------- remove_close
// Close pair (i < j): ((dx*dx + dy*dy) + dz*dz) <= r2 with d = p_i - p_j (the square of a negated difference is the same, so the test is
// symmetric).  deg[k] = number of close pairs containing k.  Pass 2: the pair drops its endpoint of higher degree, i on equal degree; so k is
// removed iff some close j has deg[k] > deg[j], or deg[k] == deg[j] and k < j.  One lane per candidate, the others in 256-point LDS tiles.
template <int PASS>
__global__ void __launch_bounds__(RC_BLOCK) rc_close_kernel(int C, const double* __restrict__ pts, double r2, const int* __restrict__ deg_in,
                                                          int* __restrict__ out) {
    __shared__ double tp[3][RC_TILE];
    __shared__ int td[RC_TILE];
    const int k = blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool ok = k < C;
    double p[3] = {0.0, 0.0, 0.0};
    int mydeg = 0;
    if (ok) {
        for (int c = 0; c < 3; ++c) p[c] = pts[(size_t)k * 3 + c];
        if (PASS == 1) mydeg = deg_in[k];
    }
    int acc = 0;
    for (int t0 = 0; t0 < C; t0 += RC_TILE) {
        const int tn = min(RC_TILE, C - t0);
        __syncthreads();
        if ((int)threadIdx.x < tn) {
            for (int c = 0; c < 3; ++c) tp[c][threadIdx.x] = pts[(size_t)(t0 + threadIdx.x) * 3 + c];
            if (PASS == 1) td[threadIdx.x] = deg_in[t0 + threadIdx.x];
        }
        __syncthreads();
        if (ok) {
            for (int j = 0; j < tn; ++j) {
                const double dx = p[0] - tp[0][j], dy = p[1] - tp[1][j], dz = p[2] - tp[2][j];
                const bool close = rc_dot(dx, dy, dz, dx, dy, dz) <= r2 && t0 + j != k;
                if (PASS == 0) acc += close;
                else acc |= close && (mydeg > td[j] || (mydeg == td[j] && k < t0 + j));
            }
        }
    }
    if (ok) out[k] = acc;
}

extern "C" {

int etch_ray_first_hit_workspace(int R, int F, long long* bytes) {
    if (R < 0 || F < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)rc_nchunk(F) * R * (sizeof(double) + sizeof(int));
    return ETCH_OK;
}

int etch_ray_first_hit(int R, int F, const double* origins, const double* dirs, const double* verts, const int* faces, const int* excl_face,
                       const double* t_max, void* workspace, int* face, double* t, double* bary, double* loc, void* stream) {
    if (R < 0 || F < 0) return ETCH_EINVAL;
    if (R == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nc = rc_nchunk(F);
    double* ct = (double*)workspace;
    int* cf = (int*)(ct + (size_t)nc * R);
    if (nc > 0)
        hipLaunchKernelGGL(rc_ray_chunk_kernel, dim3(rc_nblk(R), nc), dim3(RC_BLOCK), 0, st, R, F, origins, dirs, verts, faces, excl_face, t_max, ct, cf);
    hipLaunchKernelGGL(rc_ray_final_kernel, dim3(rc_nblk(R)), dim3(RC_BLOCK), 0, st, R, nc, origins, dirs, verts, faces, ct, cf, face, t, bary, loc);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_closest_point_on_mesh_workspace(int P, int F, long long* bytes) { return etch_ray_first_hit_workspace(P, F, bytes); }

int etch_closest_point_on_mesh(int P, int F, const double* points, const double* verts, const int* faces, void* workspace, int* face, double* bary,
                               double* closest, double* d2, void* stream) {
    if (P < 0 || F < 0) return ETCH_EINVAL;
    if (P == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nc = rc_nchunk(F);
    double* cd = (double*)workspace;
    int* cf = (int*)(cd + (size_t)nc * P);
    if (nc > 0) hipLaunchKernelGGL(rc_closest_chunk_kernel, dim3(rc_nblk(P), nc), dim3(RC_BLOCK), 0, st, P, F, points, verts, faces, cd, cf);
    hipLaunchKernelGGL(rc_closest_final_kernel, dim3(rc_nblk(P)), dim3(RC_BLOCK), 0, st, P, nc, points, verts, faces, cd, cf, face, bary, closest, d2);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_vertex_normals(int Vn, int F, const double* verts, const int* faces, const int* csr_ptr, const int* csr_idx, void* workspace, double* normals,
                        void* stream) {
    if (Vn < 0 || F < 0) return ETCH_EINVAL;
    if (Vn == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    double* fn = (double*)workspace;
    double* ang = fn + (size_t)F * 3;
    if (F > 0) hipLaunchKernelGGL(rc_face_normal_kernel, dim3(rc_nblk(F)), dim3(RC_BLOCK), 0, st, F, verts, faces, fn, ang);
    hipLaunchKernelGGL(rc_vertex_normal_kernel, dim3(rc_nblk(Vn)), dim3(RC_BLOCK), 0, st, Vn, csr_ptr, csr_idx, fn, ang, normals);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_remove_close(int C, const double* points, double r2, int* degree, int* removed, void* stream) {
    if (C < 0) return ETCH_EINVAL;
    if (C == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rc_close_kernel<0>, dim3(rc_nblk(C)), dim3(RC_BLOCK), 0, st, C, points, r2, nullptr, degree);
    hipLaunchKernelGGL(rc_close_kernel<1>, dim3(rc_nblk(C)), dim3(RC_BLOCK), 0, st, C, points, r2, degree, removed);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
