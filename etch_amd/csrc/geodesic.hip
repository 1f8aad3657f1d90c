// Heat-method geodesic distances in fp64 on gfx950: the label / confidence half of GTDataset.__getitem__
// (src/data_utils/GT_dataloader.py:124-145, pp3d.MeshHeatMethodDistanceSolver with its defaults).  DESIGN.md section 10 is the definition.
//
//   gd_init_kernel          per-body copy of the edge topology, input edge lengths from the positions
//   gd_mollify_kernel       one workgroup per body: mean input edge length (-> t), intrinsic mollification
//   gd_bad / claim / flip   one round of independent intrinsic Delaunay flips, all bodies at once
//   gd_face_geom_kernel     per face: area, corner cotans, 2-D layout
//   gd_edge_geom_kernel     per edge: the cotans of its two opposite corners
//   gd_csr_*                vertex -> edge CSR per body: count, scan, fill, sort each row by edge index, L / M rows
//   gd_solve_kernel         one workgroup per (body, 4 marker columns): heat (Jacobi), normalised gradient, divergence, Poisson (Jacobi-PCG)
//   gd_marker_min_kernel    min / argmin over the columns per vertex
//
// Every value is bit-defined: the TU is built with -ffp-contract=off, every sum runs in a fixed order (rows in CSR order, which is sorted by
// edge index; reductions through wave shuffles and then the waves in order), and no atomic touches a floating-point value (integer atomics
// count degrees and flips only; the CSR fill they order is sorted afterwards).  A body's result does not depend on the other bodies of the
// batch, and a column's result does not depend on the other columns of its workgroup: a column stops on its own criterion and is frozen.
#include <vector>

#include "common.h"
#include "etch_hip.h"

#define GD_BLOCK 256
#define GD_SOLVE_THREADS 1024
#define GD_NC 4                      // marker columns per solve workgroup
#define GD_WAVES (GD_SOLVE_THREADS / ETCH_WAVE)
#define GD_ROUNDS_PER_CHECK 8        // flip rounds queued between two reads of the flip counters

static inline unsigned gd_nblk(long n) { return (unsigned)((n + GD_BLOCK - 1) / GD_BLOCK); }

// ---------------------------------------------------------------------------------------------- triangle helpers
// Area from the three lengths, Kahan's stable Heron (x >= y >= z): 0.25 sqrt((x + (y + z)) (z - (x - y)) (z + (x - y)) (x + (y - z))).
__device__ __forceinline__ double gd_area(double a, double b, double c) {
    double x = a, y = b, z = c, s;
    if (x < y) { s = x; x = y; y = s; }
    if (y < z) { s = y; y = z; z = s; }
    if (x < y) { s = x; x = y; y = s; }
    double p = (x + (y + z)) * (z - (x - y)) * (z + (x - y)) * (x + (y - z));
    return 0.25 * sqrt(p > 0.0 ? p : 0.0);
}

// cotangent of the corner opposite the side of length a: ((b*b + c*c) - a*a) / (4 area)
__device__ __forceinline__ double gd_cot(double a, double b, double c, double area) { return ((b * b + c * c) - a * a) / (4.0 * area); }

// |ad| in the 2-D layout of the quad a-b-d-c around the diagonal bc: b at the origin, c at (lbc, 0), a above, d below.
__device__ __forceinline__ double gd_flip_length(double lab, double lac, double lbc, double lbd, double lcd) {
    const double xa = ((lab * lab - lac * lac) + lbc * lbc) / (2.0 * lbc);
    double ya = lab * lab - xa * xa;
    ya = sqrt(ya > 0.0 ? ya : 0.0);
    const double xd = ((lbd * lbd - lcd * lcd) + lbc * lbc) / (2.0 * lbc);
    double yd = lbd * lbd - xd * xd;
    yd = sqrt(yd > 0.0 ? yd : 0.0);
    const double dx = xa - xd, dy = ya + yd;
    return sqrt(dx * dx + dy * dy);
}

// Per-body mesh by edges: fv[f][k] corner k, fe[f][k] the edge opposite corner k, fs[f][k] the slot of ef[fe[f][k]] that f holds,
// ef[e][0..1] the faces of e (slot 1 = -1 on a boundary edge), ev[e] its endpoints (low, high), el[e] its intrinsic length.
struct GdMesh {
    int *fv, *fe, *fs, *ef, *ev;
    double* el;
};

__device__ __forceinline__ GdMesh gd_mesh(const GdMesh& m, int b, int F, int E) {
    GdMesh r;
    r.fv = m.fv + (size_t)b * 3 * F; r.fe = m.fe + (size_t)b * 3 * F; r.fs = m.fs + (size_t)b * 3 * F;
    r.ef = m.ef + (size_t)b * 2 * E; r.ev = m.ev + (size_t)b * 2 * E; r.el = m.el + (size_t)b * E;
    return r;
}

// cot of the corner of face f opposite its edge e (f holds e)
__device__ __forceinline__ double gd_face_cot_opposite(const GdMesh& m, int f, int e) {
    const int* fe = m.fe + 3 * f;
    const int k = fe[0] == e ? 0 : (fe[1] == e ? 1 : 2);
    const double a = m.el[fe[k]], b = m.el[fe[(k + 1) % 3]], c = m.el[fe[(k + 2) % 3]];
    return gd_cot(a, b, c, gd_area(a, b, c));
}

// ---------------------------------------------------------------------------------------------- setup and flips
__global__ void __launch_bounds__(GD_BLOCK) gd_init_kernel(int B, int F, int E, const double* __restrict__ verts, int V, const int* __restrict__ fv0,
                                                         const int* __restrict__ fe0, const int* __restrict__ fs0, const int* __restrict__ ef0,
                                                         const int* __restrict__ ev0, GdMesh M) {
    const long n = (long)B * (F > E ? F : E);
    for (long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x; g < n; g += (long)gridDim.x * GD_BLOCK) {
        const int b = (int)(g / (F > E ? F : E)), i = (int)(g % (F > E ? F : E));
        GdMesh m = gd_mesh(M, b, F, E);
        if (i < F)
            for (int k = 0; k < 3; ++k) { m.fv[3 * i + k] = fv0[3 * i + k]; m.fe[3 * i + k] = fe0[3 * i + k]; m.fs[3 * i + k] = fs0[3 * i + k]; }
        if (i < E) {
            m.ef[2 * i] = ef0[2 * i]; m.ef[2 * i + 1] = ef0[2 * i + 1];
            const int a = ev0[2 * i], c = ev0[2 * i + 1];
            m.ev[2 * i] = a; m.ev[2 * i + 1] = c;
            const double* p = verts + ((size_t)b * V + a) * 3;
            const double* q = verts + ((size_t)b * V + c) * 3;
            const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
            m.el[i] = sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
}

// Block-wide fixed-order reductions: wave shuffles (a fixed tree), then the waves' partials in ascending order.  Every thread gets the result.
template <int NT>
__device__ __forceinline__ double gd_block_sum(double v, double* lds) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += lds[w];
    return s;
}
template <int NT>
__device__ __forceinline__ double gd_block_max(double v, double* lds) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < NT / 64; ++w) s = fmax(s, lds[w]);
    return s;
}

// hbar = mean input edge length, t = t_coef hbar^2; with mollify: delta = max(0, max over face corners of eps hbar - (l_j + l_k - l_i)),
// every length += delta (geometry-central's mollifyIntrinsic as DESIGN 10a reads it).
__global__ void __launch_bounds__(GD_BLOCK) gd_mollify_kernel(int F, int E, GdMesh M, double t_coef, double eps, int mollify, double* __restrict__ tval) {
    __shared__ double lds[GD_BLOCK / 64];
    const int b = blockIdx.x;
    GdMesh m = gd_mesh(M, b, F, E);
    double s = 0.0;
    for (int i = threadIdx.x; i < E; i += GD_BLOCK) s += m.el[i];
    const double hbar = gd_block_sum<GD_BLOCK>(s, lds) / (double)E;
    if (threadIdx.x == 0) tval[b] = t_coef * (hbar * hbar);
    if (!mollify) return;
    const double e = eps * hbar;
    double d = 0.0;
    for (int f = threadIdx.x; f < F; f += GD_BLOCK) {
        const double l0 = m.el[m.fe[3 * f]], l1 = m.el[m.fe[3 * f + 1]], l2 = m.el[m.fe[3 * f + 2]];
        d = fmax(d, fmax(e - (l1 + l2 - l0), fmax(e - (l2 + l0 - l1), e - (l0 + l1 - l2))));
    }
    const double delta = gd_block_max<GD_BLOCK>(d, lds);
    __syncthreads();
    if (delta > 0.0)
        for (int i = threadIdx.x; i < E; i += GD_BLOCK) m.el[i] += delta;
}

// bad[e] = cot a + cot b < -tol (never on a boundary edge)
__global__ void __launch_bounds__(GD_BLOCK) gd_bad_kernel(int B, int F, int E, GdMesh M, double tol, int* __restrict__ bad) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * E) return;
    const int b = (int)(g / E), e = (int)(g % E);
    GdMesh m = gd_mesh(M, b, F, E);
    const int f0 = m.ef[2 * e], f1 = m.ef[2 * e + 1];
    int r = 0;
    if (f1 >= 0) r = (gd_face_cot_opposite(m, f0, e) + gd_face_cot_opposite(m, f1, e)) < -tol;
    bad[g] = r;
}

// each face claims its lowest-index non-Delaunay edge
__global__ void __launch_bounds__(GD_BLOCK) gd_claim_kernel(int B, int F, int E, GdMesh M, const int* __restrict__ bad, int* __restrict__ claim) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * F) return;
    const int b = (int)(g / F), f = (int)(g % F);
    const int* fe = M.fe + (size_t)b * 3 * F + 3 * f;
    const int* bd = bad + (size_t)b * E;
    int c = -1;
    for (int k = 0; k < 3; ++k)
        if (bd[fe[k]] && (c < 0 || fe[k] < c)) c = fe[k];
    claim[g] = c;
}

// An edge flips when both its faces claimed it.  e = bc between f = (a, b, c) and g = (d, c, b) becomes ad: f -> (a, b, d), g -> (d, c, a).
// The flips of one round own disjoint face pairs; each writes its two faces, its edge, and the one slot of bd (g -> f) and of ca (f -> g)
// that its faces hold, so no two flips write (or one writes what another reads) the same word.
__global__ void __launch_bounds__(GD_BLOCK) gd_flip_kernel(int B, int F, int E, GdMesh M, const int* __restrict__ bad, const int* __restrict__ claim,
                                                         int* __restrict__ flips) {
    const long gi = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (gi >= (long)B * E || !bad[gi]) return;
    const int b = (int)(gi / E), e = (int)(gi % E);
    GdMesh m = gd_mesh(M, b, F, E);
    const int f = m.ef[2 * e], g = m.ef[2 * e + 1];
    const int* cl = claim + (size_t)b * F;
    if (cl[f] != e || cl[g] != e) return;
    int* fvf = m.fv + 3 * f; int* fef = m.fe + 3 * f; int* fsf = m.fs + 3 * f;
    int* fvg = m.fv + 3 * g; int* feg = m.fe + 3 * g; int* fsg = m.fs + 3 * g;
    const int k = fef[0] == e ? 0 : (fef[1] == e ? 1 : 2);
    const int j = feg[0] == e ? 0 : (feg[1] == e ? 1 : 2);
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    const int a = fvf[k], vb = fvf[k1], c = fvg[j1], d = fvg[j];
    const int e_ca = fef[k1], s_ca = fsf[k1], e_ab = fef[k2], s_ab = fsf[k2];
    const int e_bd = feg[j1], s_bd = fsg[j1], e_dc = feg[j2], s_dc = fsg[j2];
    const int s_ef = fsf[k], s_eg = fsg[j];
    m.el[e] = gd_flip_length(m.el[e_ab], m.el[e_ca], m.el[e], m.el[e_bd], m.el[e_dc]);
    fvf[0] = a; fvf[1] = vb; fvf[2] = d;
    fef[0] = e_bd; fef[1] = e; fef[2] = e_ab;
    fsf[0] = s_bd; fsf[1] = s_ef; fsf[2] = s_ab;
    fvg[0] = d; fvg[1] = c; fvg[2] = a;
    feg[0] = e_ca; feg[1] = e; feg[2] = e_dc;
    fsg[0] = s_ca; fsg[1] = s_eg; fsg[2] = s_dc;
    m.ef[2 * e_bd + s_bd] = f;
    m.ef[2 * e_ca + s_ca] = g;
    m.ev[2 * e] = a < d ? a : d;
    m.ev[2 * e + 1] = a < d ? d : a;
    atomicAdd(flips + b, 1);
}

// ---------------------------------------------------------------------------------------------- operators
// per face: area, cot of each corner, layout (corner 0 at the origin, corner 1 at (l2, 0), corner 2 at (x, y), y = 2 area / l2 > 0)
__global__ void __launch_bounds__(GD_BLOCK) gd_face_geom_kernel(int B, int F, int E, GdMesh M, double* __restrict__ farea, double* __restrict__ fcot,
                                                              double* __restrict__ flay) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * F) return;
    const int b = (int)(g / F), f = (int)(g % F);
    GdMesh m = gd_mesh(M, b, F, E);
    const double l0 = m.el[m.fe[3 * f]], l1 = m.el[m.fe[3 * f + 1]], l2 = m.el[m.fe[3 * f + 2]];
    const double A = gd_area(l0, l1, l2);
    farea[g] = A;
    fcot[3 * g] = gd_cot(l0, l1, l2, A);
    fcot[3 * g + 1] = gd_cot(l1, l2, l0, A);
    fcot[3 * g + 2] = gd_cot(l2, l0, l1, A);
    flay[3 * g] = l2;
    flay[3 * g + 1] = ((l2 * l2 + l1 * l1) - l0 * l0) / (2.0 * l2);
    flay[3 * g + 2] = (2.0 * A) / l2;
}

// per edge: the cot of the corner opposite it in each of its faces (0 for a missing face); w = (cot0 + cot1) / 2
__global__ void __launch_bounds__(GD_BLOCK) gd_edge_geom_kernel(int B, int F, int E, GdMesh M, const double* __restrict__ fcot, double* __restrict__ ecot) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * E) return;
    const int b = (int)(g / E), e = (int)(g % E);
    GdMesh m = gd_mesh(M, b, F, E);
    for (int s = 0; s < 2; ++s) {
        const int f = m.ef[2 * e + s];
        double c = 0.0;
        if (f >= 0) {
            const int* fe = m.fe + 3 * f;
            const int k = fe[0] == e ? 0 : (fe[1] == e ? 1 : 2);
            c = fcot[((size_t)b * F + f) * 3 + k];
        }
        ecot[2 * g + s] = c;
    }
}

// vertex degrees (integer atomics: the counts are order-free)
__global__ void __launch_bounds__(GD_BLOCK) gd_csr_count_kernel(int B, int V, int E, const int* __restrict__ ev, int* __restrict__ deg) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * E) return;
    const int b = (int)(g / E);
    atomicAdd(deg + (size_t)b * V + ev[2 * g], 1);
    atomicAdd(deg + (size_t)b * V + ev[2 * g + 1], 1);
}

// exclusive scan of the degrees per body (one workgroup, chunks of GD_BLOCK in order) -> rowptr (V+1); cursor = rowptr
__global__ void __launch_bounds__(GD_BLOCK) gd_csr_scan_kernel(int V, const int* __restrict__ deg, int* __restrict__ rowptr, int* __restrict__ cursor) {
    __shared__ int buf[GD_BLOCK];
    const int b = blockIdx.x;
    const int* d = deg + (size_t)b * V;
    int* rp = rowptr + (size_t)b * (V + 1);
    int* cu = cursor + (size_t)b * V;
    int base = 0;
    for (int c0 = 0; c0 < V; c0 += GD_BLOCK) {
        const int i = c0 + threadIdx.x;
        const int x = i < V ? d[i] : 0;
        buf[threadIdx.x] = x;
        __syncthreads();
        for (int off = 1; off < GD_BLOCK; off <<= 1) {
            const int y = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += y;
            __syncthreads();
        }
        if (i < V) { rp[i] = base + buf[threadIdx.x] - x; cu[i] = base + buf[threadIdx.x] - x; }
        base += buf[GD_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) rp[V] = base;
}

__global__ void __launch_bounds__(GD_BLOCK) gd_csr_fill_kernel(int B, int V, int E, const int* __restrict__ ev, int* __restrict__ cursor,
                                                             int* __restrict__ ent) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * E) return;
    const int b = (int)(g / E), e = (int)(g % E);
    for (int s = 0; s < 2; ++s) {
        const int p = atomicAdd(cursor + (size_t)b * V + ev[2 * g + s], 1);
        ent[(size_t)b * 2 * E + p] = e;
    }
}

// sort each row by edge index, then: col = the other endpoint, w = (cot0 + cot1) / 2, Ldiag = sum of the row's w, mass = sum over the row's
// edges of (area f0 + area f1) / 6 (each incident face is met through its two edges at the vertex), all in row order
__global__ void __launch_bounds__(GD_BLOCK) gd_csr_rows_kernel(int B, int V, int F, int E, const int* __restrict__ ev, const int* __restrict__ ef,
                                                             const double* __restrict__ ecot, const double* __restrict__ farea,
                                                             const int* __restrict__ rowptr, int* __restrict__ ent, int* __restrict__ col,
                                                             double* __restrict__ w, double* __restrict__ ldiag, double* __restrict__ mass) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * V) return;
    const int b = (int)(g / V), i = (int)(g % V);
    const int r0 = rowptr[(size_t)b * (V + 1) + i], r1 = rowptr[(size_t)b * (V + 1) + i + 1];
    int* en = ent + (size_t)b * 2 * E;
    for (int p = r0 + 1; p < r1; ++p) {
        const int x = en[p];
        int q = p - 1;
        while (q >= r0 && en[q] > x) { en[q + 1] = en[q]; --q; }
        en[q + 1] = x;
    }
    double sw = 0.0, sm = 0.0;
    for (int p = r0; p < r1; ++p) {
        const size_t e = (size_t)b * E + en[p];
        const int a = ev[2 * e], c = ev[2 * e + 1];
        col[(size_t)b * 2 * E + p] = a == i ? c : a;
        const double we = 0.5 * (ecot[2 * e] + ecot[2 * e + 1]);
        w[(size_t)b * 2 * E + p] = we;
        sw += we;
        const int f0 = ef[2 * e], f1 = ef[2 * e + 1];
        sm += (farea[(size_t)b * F + f0] + (f1 >= 0 ? farea[(size_t)b * F + f1] : 0.0)) / 6.0;
    }
    ldiag[g] = sw;
    mass[g] = sm;
}

// ---------------------------------------------------------------------------------------------- the solve
struct GdOps {
    const int *rowptr, *col, *ent, *fv, *ef;
    const double *w, *ldiag, *mass, *tval, *flay, *ecot;
};

struct GdSolveArgs {
    int V, F, E, S, heat_cap, cg_cap;
    double heat_tol, heat_omega, cg_rtol;
    const int* src;
    double* vec;          // per workgroup: 4 V-vectors of GD_NC columns + F face values, interleaved [row][GD_NC]
    double* dist;         // (B, S, V)
    int* iters;           // (B, S, 2): heat sweeps, CG iterations (-1 = the cap was hit)
};

// One workgroup per (body, GD_NC marker columns).  Per column c with source s:
//   heat   u <- (e_s + t W u) / (m + t Ldiag) from u = 0 (Jacobi: every term is >= 0 on a Delaunay mesh, so the far field, down to 1e-100 of
//          the peak, keeps its relative accuracy; a Krylov solve stopped on the residual leaves it at 0) until no vertex changes by more
//          than heat_tol of its value; heat_omega != 1 damps the sweep, u <- u + omega (jacobi(u) - u) (the cotan Laplacian's negative
//          weights make the undamped sweep diverge);
//   grad   per face: g = ((u1 - u0) / l2, ((u2 - u0) - gx x) / y), inv = 1 / |g| (0 where g = 0);
//   rhs    b_i = -div X_i = sum over row i of K_e (u_j - u_i), K_e = (cot0 inv_f0 + cot1 inv_f1) / 2; b -= mean(b);
//   poisson L phi = b by Jacobi-PCG from phi = 0 until |r| <= cg_rtol |b|; dist = phi - phi[s].
__global__ void __launch_bounds__(GD_SOLVE_THREADS) gd_solve_kernel(GdOps O, GdSolveArgs A) {
    __shared__ double red[GD_NC][GD_WAVES];
    __shared__ int flag[GD_NC];
    const int V = A.V, F = A.F, E = A.E, S = A.S;
    const int b = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
    const int nblk = gridDim.x;
    const int* rp = O.rowptr + (size_t)b * (V + 1);
    const int* col = O.col + (size_t)b * 2 * E;
    const int* ent = O.ent + (size_t)b * 2 * E;
    const double* w = O.w + (size_t)b * 2 * E;
    const double* ld = O.ldiag + (size_t)b * V;
    const double* ms = O.mass + (size_t)b * V;
    const int* fv = O.fv + (size_t)b * 3 * F;
    const double* fl = O.flay + (size_t)b * 3 * F;
    const int* ef = O.ef + (size_t)b * 2 * E;
    const double* ec = O.ecot + (size_t)b * 2 * E;
    const double t = O.tval[b];
    const size_t vs = (size_t)V * GD_NC;
    double* base = A.vec + ((size_t)b * nblk + q) * (4 * vs + (size_t)F * GD_NC);
    double* U0 = base;
    double* U1 = base + vs;
    double* P = base + 2 * vs;
    double* Q = base + 3 * vs;
    double* INV = base + 4 * vs;
    int src[GD_NC];
    bool active[GD_NC];
    int it_heat[GD_NC], it_cg[GD_NC];
    for (int c = 0; c < GD_NC; ++c) {
        const int m = q * GD_NC + c;
        src[c] = m < S ? A.src[m] : -1;
        active[c] = m < S;
        it_heat[c] = 0;
        it_cg[c] = 0;
    }
    for (int i = tid; i < V; i += GD_SOLVE_THREADS)
        for (int c = 0; c < GD_NC; ++c) U0[(size_t)i * GD_NC + c] = 0.0;
    __syncthreads();

    // ---- heat: Jacobi sweeps, U0 -> U1 -> U0 ...
    double* uc = U0;
    double* un = U1;
    bool any = true;
    int sweep = 0;
    while (any) {
        if (tid < GD_NC) flag[tid] = 0;
        __syncthreads();
        int nc = 0;
        for (int i = tid; i < V; i += GD_SOLVE_THREADS) {
            double s[GD_NC];
            for (int c = 0; c < GD_NC; ++c) s[c] = i == src[c] ? 1.0 : 0.0;
            for (int p = rp[i]; p < rp[i + 1]; ++p) {
                const double wt = t * w[p];
                const double* uj = uc + (size_t)col[p] * GD_NC;
                for (int c = 0; c < GD_NC; ++c) s[c] += wt * uj[c];
            }
            const double dg = ms[i] + t * ld[i];
            for (int c = 0; c < GD_NC; ++c) {
                const double old = uc[(size_t)i * GD_NC + c];
                double v = old;
                if (active[c]) {
                    v = s[c] / dg;
                    if (A.heat_omega != 1.0) v = old + A.heat_omega * (v - old);
                    if (!(fabs(v - old) <= A.heat_tol * fabs(v))) nc |= 1 << c;
                }
                un[(size_t)i * GD_NC + c] = v;
            }
        }
        for (int c = 0; c < GD_NC; ++c)
            if (nc & (1 << c)) atomicOr(&flag[c], 1);
        __syncthreads();
        ++sweep;
        any = false;
        for (int c = 0; c < GD_NC; ++c) {
            if (!active[c]) continue;
            it_heat[c] = sweep;
            if (!flag[c]) active[c] = false;
            else if (sweep >= A.heat_cap) { active[c] = false; it_heat[c] = -1; }
            any |= active[c];
        }
        double* x = uc; uc = un; un = x;
        __syncthreads();
    }
    // uc holds every column's last sweep (a frozen column is copied forward unchanged)

    // ---- normalised gradient per face
    for (int f = tid; f < F; f += GD_SOLVE_THREADS) {
        const double* u0 = uc + (size_t)fv[3 * f] * GD_NC;
        const double* u1 = uc + (size_t)fv[3 * f + 1] * GD_NC;
        const double* u2 = uc + (size_t)fv[3 * f + 2] * GD_NC;
        const double l2 = fl[3 * f], x = fl[3 * f + 1], y = fl[3 * f + 2];
        for (int c = 0; c < GD_NC; ++c) {
            const double gx = (u1[c] - u0[c]) / l2;
            const double gy = ((u2[c] - u0[c]) - gx * x) / y;
            const double n = sqrt(gx * gx + gy * gy);
            INV[(size_t)f * GD_NC + c] = n > 0.0 ? 1.0 / n : 0.0;
        }
    }
    __syncthreads();
    // ---- rhs into un (= r), then the mean removed
    double part[GD_NC];
    for (int c = 0; c < GD_NC; ++c) part[c] = 0.0;
    for (int i = tid; i < V; i += GD_SOLVE_THREADS) {
        double s[GD_NC];
        for (int c = 0; c < GD_NC; ++c) s[c] = 0.0;
        const double* ui = uc + (size_t)i * GD_NC;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            const int e = ent[p];
            const int f0 = ef[2 * e], f1 = ef[2 * e + 1];
            const double* uj = uc + (size_t)col[p] * GD_NC;
            for (int c = 0; c < GD_NC; ++c) {
                double K = ec[2 * e] * INV[(size_t)f0 * GD_NC + c];
                if (f1 >= 0) K = K + ec[2 * e + 1] * INV[(size_t)f1 * GD_NC + c];
                s[c] += (0.5 * K) * (uj[c] - ui[c]);
            }
        }
        for (int c = 0; c < GD_NC; ++c) { un[(size_t)i * GD_NC + c] = s[c]; part[c] += s[c]; }
    }
    double mean[GD_NC];
    for (int c = 0; c < GD_NC; ++c) mean[c] = gd_block_sum<GD_SOLVE_THREADS>(part[c], red[0]) / (double)V;
    __syncthreads();
    // ---- Jacobi-PCG: X = uc (x), R = un (r), P (p), Q (Ap); z = r / Ldiag on the fly
    double* X = uc;
    double* R = un;
    double rz[GD_NC], bb[GD_NC], rr[GD_NC];
    for (int c = 0; c < GD_NC; ++c) { part[c] = 0.0; rr[c] = 0.0; }
    for (int i = tid; i < V; i += GD_SOLVE_THREADS)
        for (int c = 0; c < GD_NC; ++c) {
            const size_t k = (size_t)i * GD_NC + c;
            const double r = R[k] - mean[c];
            R[k] = r;
            X[k] = 0.0;
            const double z = r / ld[i];
            P[k] = z;
            part[c] += r * z;
            rr[c] += r * r;
        }
    for (int c = 0; c < GD_NC; ++c) {
        rz[c] = gd_block_sum<GD_SOLVE_THREADS>(part[c], red[0]);
        __syncthreads();
        bb[c] = gd_block_sum<GD_SOLVE_THREADS>(rr[c], red[0]);
        __syncthreads();
        const int m = q * GD_NC + c;
        active[c] = m < S && bb[c] > 0.0;
    }
    any = false;
    for (int c = 0; c < GD_NC; ++c) any |= active[c];
    int iter = 0;
    while (any) {
        ++iter;
        for (int c = 0; c < GD_NC; ++c) part[c] = 0.0;
        for (int i = tid; i < V; i += GD_SOLVE_THREADS) {
            double s[GD_NC];
            const double* pi = P + (size_t)i * GD_NC;
            for (int c = 0; c < GD_NC; ++c) s[c] = ld[i] * pi[c];
            for (int p = rp[i]; p < rp[i + 1]; ++p) {
                const double wt = w[p];
                const double* pj = P + (size_t)col[p] * GD_NC;
                for (int c = 0; c < GD_NC; ++c) s[c] -= wt * pj[c];
            }
            for (int c = 0; c < GD_NC; ++c) { Q[(size_t)i * GD_NC + c] = s[c]; part[c] += pi[c] * s[c]; }
        }
        double alpha[GD_NC];
        for (int c = 0; c < GD_NC; ++c) { alpha[c] = rz[c] / gd_block_sum<GD_SOLVE_THREADS>(part[c], red[0]); __syncthreads(); }
        for (int c = 0; c < GD_NC; ++c) { part[c] = 0.0; rr[c] = 0.0; }
        for (int i = tid; i < V; i += GD_SOLVE_THREADS)
            for (int c = 0; c < GD_NC; ++c) {
                if (!active[c]) continue;
                const size_t k = (size_t)i * GD_NC + c;
                X[k] += alpha[c] * P[k];
                const double r = R[k] - alpha[c] * Q[k];
                R[k] = r;
                part[c] += r * (r / ld[i]);
                rr[c] += r * r;
            }
        double beta[GD_NC];
        for (int c = 0; c < GD_NC; ++c) {
            const double rzn = gd_block_sum<GD_SOLVE_THREADS>(part[c], red[0]);
            __syncthreads();
            const double rrn = gd_block_sum<GD_SOLVE_THREADS>(rr[c], red[0]);
            __syncthreads();
            beta[c] = rzn / rz[c];
            if (active[c]) {
                rz[c] = rzn;
                it_cg[c] = iter;
                if (rrn <= (A.cg_rtol * A.cg_rtol) * bb[c]) active[c] = false;
                else if (iter >= A.cg_cap) { active[c] = false; it_cg[c] = -1; }
                else continue;
                beta[c] = 0.0;
            }
        }
        any = false;
        for (int c = 0; c < GD_NC; ++c) any |= active[c];
        if (!any) break;
        for (int i = tid; i < V; i += GD_SOLVE_THREADS)
            for (int c = 0; c < GD_NC; ++c) {
                if (!active[c]) continue;
                const size_t k = (size_t)i * GD_NC + c;
                P[k] = R[k] / ld[i] + beta[c] * P[k];
            }
        __syncthreads();
    }
    __syncthreads();
    for (int c = 0; c < GD_NC; ++c) {
        const int m = q * GD_NC + c;
        if (m >= S) continue;
        const double x0 = X[(size_t)src[c] * GD_NC + c];
        double* out = A.dist + ((size_t)b * S + m) * V;
        for (int i = tid; i < V; i += GD_SOLVE_THREADS) out[i] = X[(size_t)i * GD_NC + c] - x0;
        if (tid == 0) {
            A.iters[((size_t)b * S + m) * 2] = it_heat[c];
            A.iters[((size_t)b * S + m) * 2 + 1] = it_cg[c];
        }
    }
}

// min / argmin over the S columns in ascending order with a strict < (the first column wins a tie)
__global__ void __launch_bounds__(GD_BLOCK) gd_marker_min_kernel(int B, int S, int V, const double* __restrict__ dist, double* __restrict__ dmin,
                                                               int* __restrict__ label) {
    const long g = blockIdx.x * (long)GD_BLOCK + threadIdx.x;
    if (g >= (long)B * V) return;
    const int b = (int)(g / V), i = (int)(g % V);
    const double* d = dist + (size_t)b * S * V + i;
    double best = d[0];
    int bl = 0;
    for (int s = 1; s < S; ++s) {
        const double x = d[(size_t)s * V];
        if (x < best) { best = x; bl = s; }
    }
    dmin[g] = best;
    label[g] = bl;
}

// ---------------------------------------------------------------------------------------------- C ABI
namespace {
struct GdLayout {
    size_t fv, fe, fs, ef, ev, el, bad, claim, farea, fcot, flay, ecot, deg, rowptr, cursor, ent, col, w, ldiag, mass, tval, flips_dev, vec, total;
};

size_t gd_align(size_t x) { return (x + 255) & ~(size_t)255; }

GdLayout gd_layout(int B, int V, int F, int E, int S) {
    GdLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += gd_align(bytes); return at; };
    const size_t b = (size_t)B;
    L.fv = take(b * 3 * F * 4); L.fe = take(b * 3 * F * 4); L.fs = take(b * 3 * F * 4);
    L.ef = take(b * 2 * E * 4); L.ev = take(b * 2 * E * 4); L.el = take(b * E * 8);
    L.bad = take(b * E * 4); L.claim = take(b * F * 4);
    L.farea = take(b * F * 8); L.fcot = take(b * 3 * F * 8); L.flay = take(b * 3 * F * 8); L.ecot = take(b * 2 * E * 8);
    L.deg = take(b * V * 4); L.rowptr = take(b * (V + 1) * 4); L.cursor = take(b * V * 4);
    L.ent = take(b * 2 * E * 4); L.col = take(b * 2 * E * 4); L.w = take(b * 2 * E * 8);
    L.ldiag = take(b * V * 8); L.mass = take(b * V * 8); L.tval = take(b * 8);
    L.flips_dev = take((size_t)GD_ROUNDS_PER_CHECK * B * 4);
    const size_t nblk = (size_t)((S + GD_NC - 1) / GD_NC);
    L.vec = take(b * nblk * (4 * (size_t)V * GD_NC + (size_t)F * GD_NC) * 8);
    L.total = o;
    return L;
}
}  // namespace

extern "C" {

int etch_geodesic_workspace(int B, int V, int F, int E, int S, long long* bytes) {
    if (B < 1 || V < 3 || F < 1 || E < 3 || S < 0 || !bytes) return ETCH_EINVAL;
    *bytes = (long long)gd_layout(B, V, F, E, S < 1 ? 1 : S).total;
    return ETCH_OK;
}

int etch_geodesic_heat(int B, int V, int F, int E, int S, const double* verts, const int* fv0, const int* fe0, const int* fs0, const int* ef0,
                       const int* ev0, const int* sources, double t_coef, int intrinsic_delaunay, double mollify_eps, double delaunay_tol,
                       int max_rounds, double heat_tol, double heat_omega, int heat_cap, double cg_rtol, int cg_cap, void* workspace, double* dist, double* dmin,
                       int* label, int* iters, int* flips, int* out_ev, double* out_el, double* out_ecot, double* out_area, void* stream) {
    if (B < 1 || V < 3 || F < 1 || E < 3 || S < 0 || !verts || !fv0 || !fe0 || !fs0 || !ef0 || !ev0 || !workspace || !flips) return ETCH_EINVAL;
    if (S > 0 && (!sources || !dist || !iters)) return ETCH_EINVAL;
    if ((dmin != nullptr) != (label != nullptr)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const GdLayout L = gd_layout(B, V, F, E, S < 1 ? 1 : S);
    char* ws = (char*)workspace;
    GdMesh M;
    M.fv = (int*)(ws + L.fv); M.fe = (int*)(ws + L.fe); M.fs = (int*)(ws + L.fs);
    M.ef = (int*)(ws + L.ef); M.ev = (int*)(ws + L.ev); M.el = (double*)(ws + L.el);
    int* bad = (int*)(ws + L.bad);
    int* claim = (int*)(ws + L.claim);
    double* tval = (double*)(ws + L.tval);
    int* fl_dev = (int*)(ws + L.flips_dev);
    const long nBE = (long)B * E, nBF = (long)B * F, nBV = (long)B * V;
    const long nmax = (long)B * (F > E ? F : E);
    hipLaunchKernelGGL(gd_init_kernel, dim3(gd_nblk(nmax) < 65535u ? gd_nblk(nmax) : 65535u), dim3(GD_BLOCK), 0, st, B, F, E, verts, V, fv0, fe0, fs0,
                       ef0, ev0, M);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(gd_mollify_kernel, dim3(B), dim3(GD_BLOCK), 0, st, F, E, M, t_coef, mollify_eps, intrinsic_delaunay, tval);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    for (int b = 0; b < B; ++b) flips[b] = 0;
    if (intrinsic_delaunay) {
        // rounds of independent flips; the flip counters of GD_ROUNDS_PER_CHECK rounds are read back together, and a round that flips
        // nothing ends the loop (the rounds queued after it flip nothing either: no edge is bad)
        std::vector<int> hbuf((size_t)GD_ROUNDS_PER_CHECK * B);
        int done = 0, rounds = 0;
        while (!done) {
            if (rounds >= max_rounds) return ETCH_EUNSUPPORTED;
            if (hipMemsetAsync(fl_dev, 0, (size_t)GD_ROUNDS_PER_CHECK * B * 4, st) != hipSuccess) return (int)hipGetLastError();
            for (int r = 0; r < GD_ROUNDS_PER_CHECK; ++r) {
                hipLaunchKernelGGL(gd_bad_kernel, dim3(gd_nblk(nBE)), dim3(GD_BLOCK), 0, st, B, F, E, M, delaunay_tol, bad);
                hipLaunchKernelGGL(gd_claim_kernel, dim3(gd_nblk(nBF)), dim3(GD_BLOCK), 0, st, B, F, E, M, (const int*)bad, claim);
                hipLaunchKernelGGL(gd_flip_kernel, dim3(gd_nblk(nBE)), dim3(GD_BLOCK), 0, st, B, F, E, M, (const int*)bad, (const int*)claim,
                                   fl_dev + (size_t)r * B);
                ETCH_RETURN_IF_LAUNCH_FAILED();
            }
            if (hipMemcpyAsync(hbuf.data(), fl_dev, hbuf.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return (int)hipGetLastError();
            if (hipStreamSynchronize(st) != hipSuccess) return (int)hipGetLastError();
            rounds += GD_ROUNDS_PER_CHECK;
            for (int r = 0; r < GD_ROUNDS_PER_CHECK; ++r) {
                int n = 0;
                for (int b = 0; b < B; ++b) { n += hbuf[(size_t)r * B + b]; flips[b] += hbuf[(size_t)r * B + b]; }
                if (n == 0) done = 1;
            }
        }
    }
    double* farea = (double*)(ws + L.farea);
    double* fcot = (double*)(ws + L.fcot);
    double* flay = (double*)(ws + L.flay);
    double* ecot = (double*)(ws + L.ecot);
    int* deg = (int*)(ws + L.deg);
    int* rowptr = (int*)(ws + L.rowptr);
    int* cursor = (int*)(ws + L.cursor);
    int* ent = (int*)(ws + L.ent);
    int* col = (int*)(ws + L.col);
    double* w = (double*)(ws + L.w);
    double* ldiag = (double*)(ws + L.ldiag);
    double* mass = (double*)(ws + L.mass);
    hipLaunchKernelGGL(gd_face_geom_kernel, dim3(gd_nblk(nBF)), dim3(GD_BLOCK), 0, st, B, F, E, M, farea, fcot, flay);
    hipLaunchKernelGGL(gd_edge_geom_kernel, dim3(gd_nblk(nBE)), dim3(GD_BLOCK), 0, st, B, F, E, M, (const double*)fcot, ecot);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (hipMemsetAsync(deg, 0, (size_t)B * V * 4, st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(gd_csr_count_kernel, dim3(gd_nblk(nBE)), dim3(GD_BLOCK), 0, st, B, V, E, (const int*)M.ev, deg);
    hipLaunchKernelGGL(gd_csr_scan_kernel, dim3(B), dim3(GD_BLOCK), 0, st, V, (const int*)deg, rowptr, cursor);
    hipLaunchKernelGGL(gd_csr_fill_kernel, dim3(gd_nblk(nBE)), dim3(GD_BLOCK), 0, st, B, V, E, (const int*)M.ev, cursor, ent);
    hipLaunchKernelGGL(gd_csr_rows_kernel, dim3(gd_nblk(nBV)), dim3(GD_BLOCK), 0, st, B, V, F, E, (const int*)M.ev, (const int*)M.ef,
                       (const double*)ecot, (const double*)farea, (const int*)rowptr, ent, col, w, ldiag, mass);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (out_ev && hipMemcpyAsync(out_ev, M.ev, (size_t)B * 2 * E * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
    if (out_el && hipMemcpyAsync(out_el, M.el, (size_t)B * E * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
    if (out_area && hipMemcpyAsync(out_area, farea, (size_t)B * F * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
    if (out_ecot && hipMemcpyAsync(out_ecot, ecot, (size_t)B * 2 * E * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return (int)hipGetLastError();
    if (S == 0) return ETCH_OK;
    GdOps O;
    O.rowptr = rowptr; O.col = col; O.ent = ent; O.fv = M.fv; O.ef = M.ef;
    O.w = w; O.ldiag = ldiag; O.mass = mass; O.tval = tval; O.flay = flay; O.ecot = ecot;
    GdSolveArgs A;
    A.V = V; A.F = F; A.E = E; A.S = S; A.heat_cap = heat_cap; A.cg_cap = cg_cap; A.heat_tol = heat_tol; A.heat_omega = heat_omega; A.cg_rtol = cg_rtol;
    A.src = sources; A.vec = (double*)(ws + L.vec); A.dist = dist; A.iters = iters;
    hipLaunchKernelGGL(gd_solve_kernel, dim3((S + GD_NC - 1) / GD_NC, B), dim3(GD_SOLVE_THREADS), 0, st, O, A);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    if (dmin) {
        hipLaunchKernelGGL(gd_marker_min_kernel, dim3(gd_nblk(nBV)), dim3(GD_BLOCK), 0, st, B, S, V, (const double*)dist, dmin, label);
        ETCH_RETURN_IF_LAUNCH_FAILED();
    }
    return ETCH_OK;
}

}  // extern "C"
