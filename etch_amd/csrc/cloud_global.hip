// Global registration of raw clouds: FPFH descriptors on the cell grid, nearest-feature correspondences, RANSAC over triples
// of correspondences.  fp64, one rounding per operation: this file is built with -ffp-contract=off.  Everything that is compared is an integer or
// a bit-defined double: counts are integers, a hypothesis is a pure function of (pair key, h) through Philox4x32-10 with counter (h, 2, 0, 0),
// scores are added up with integer atomics, every fp64 sum runs in an order its definition names.  No float atomics anywhere.
//
// Descriptors, pass 1: the search of cloud_normals_kernel (cloud_normals.hip) -- one thread per query in sorted-cell order, rings rho = 0 ..
// CLOUD_MAX_RINGS, the stop rule kth <= (rho h (1 - 2^-20))^2, the whole-cloud scan behind it, brute != 0 as the second implementation, the
// ke least (d2, row) pairs kept in LDS as best[slot][thread] and index[slot][thread] -- and behind the list, in the same LDS block, the row's
// 33 counters as bytes, hist[bin][thread] (a counter never exceeds ke <= 32).  (12 k + 36) T bytes: T = 256 threads up to k = 18 (63 KiB), above
// T = 128 (52.5 KiB at k = 32): under the 64 KiB a workgroup gets without asking, three workgroups to a CU's 160 KiB, as section 24b chose.
// The thread then walks its list in order, counts the pair features (cloud_global_solve.h) and writes list, counters and their number.
// Pass 2: one thread per row, 33 sums in registers over the row's list in its order.
//
// Matching: brute force by design.  A workgroup of 256 source rows keeps each row's 33 features in registers and walks the target's features
// through LDS in tiles of 64 rows; every lane reads the same address (a broadcast), so one LDS read serves 64 source rows.
//
// Scores: the shape of iso_score_kernel (cloud_isolate.hip).  A workgroup owns 512 VALID hypotheses, which it ranks itself by a count and a
// scan over the pair's H flags, so an invalid hypothesis costs nothing; a thread keeps two transforms in registers; the correspondences sit in
// LDS as six arrays and are read as broadcasts; counts go out as integer atomics.
#include "common.h"
#include "etch_hip.h"
#include "cloud_grid.h"
#include "cloud_global_solve.h"
#include <cmath>

#define CLOUD_MAX_RINGS ETCH_CLOUD_MAX_RINGS
#define GLOBAL_WIDE_THREADS 256
#define GLOBAL_NARROW_THREADS 128
#define GLOBAL_WIDE_MAX_K 18                 // (12 * 18 + 36) * 256 B = 63 KiB
#define GLOBAL_HIST_ROWS 36                  // 33 byte counters per thread, rounded up to a multiple of 4
#define GLOBAL_ROW_THREADS 256
#define GLOBAL_MATCH_THREADS 256
#define GLOBAL_MATCH_TILE 64                 // target rows staged at a time: 64 x 33 x 8 B = 16.5 KiB
#define GLOBAL_SCORE_THREADS 256
#define GLOBAL_SCORE_PER_THREAD 2            // every LDS broadcast read serves two hypotheses
#define GLOBAL_SCORE_TILE 512                // correspondences staged at a time: 6 x 4 KiB
#define GLOBAL_SCORE_TILES_PER_GROUP 4
#define GLOBAL_GROUP 1024                    // the one-workgroup-per-pair kernel

static_assert(GLOBAL_BINS == ETCH_GLOBAL_BINS && GLOBAL_FEATURES == ETCH_GLOBAL_FEATURES, "the descriptor's shape of the header");
static_assert(GLOBAL_FEATURES <= GLOBAL_HIST_ROWS && ETCH_CLOUD_MAX_K <= 255, "a byte counter holds a row's pairs");
static_assert((size_t)(12 * GLOBAL_WIDE_MAX_K + GLOBAL_HIST_ROWS) * GLOBAL_WIDE_THREADS <= 65536 &&
                  (size_t)(12 * ETCH_CLOUD_MAX_K + GLOBAL_HIST_ROWS) * GLOBAL_NARROW_THREADS <= 65536,
              "list and counters fit 64 KiB in either form");

namespace {

// ---- descriptors, pass 1: the neighbour list and the pair-feature counts of every row --------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void global_spfh_kernel(int B, int M, int k, int brute, const double* __restrict__ P,
                                                              const long long* __restrict__ keys, const int* __restrict__ order,
                                                              const int* __restrict__ offsets, const double* __restrict__ grid,
                                                              const int* __restrict__ status, const double* __restrict__ normal,
                                                              const int* __restrict__ nflag, int* __restrict__ spfh, int* __restrict__ count,
                                                              int* __restrict__ nbr) {
    extern __shared__ double best[];                  // [k][THREADS] d2, then [k][THREADS] int sorted index, then [36][THREADS] byte counters
    int* const index = (int*)(best + (size_t)k * THREADS);
    unsigned char* const hist = (unsigned char*)(index + (size_t)k * THREADS);
    const int tid = threadIdx.x;
    const int t = blockIdx.x * THREADS + tid;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const int row = brute ? t : order[t];
    const int ke = k < hi - lo - 1 ? k : hi - lo - 1;
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    double kth = INFINITY;
    int kidx = -1;
    for (int j = 0; j < ke; ++j) best[j * THREADS + tid] = INFINITY, index[j * THREADS + tid] = -1;
    // the original row of sorted row j; an empty slot sorts behind every row
    auto rowof = [&](int j) { return j < 0 ? 0x7fffffff : (brute ? j : order[j]); };
    auto visit = [&](int j) {
        if (j == t) return;
        const double d = cloud_d2(px, py, pz, P + 3 * (size_t)j);
        if (!(d <= kth)) return;
        if (d == kth && !(rowof(j) < rowof(kidx))) return;
        int s = ke - 1;
        while (s > 0) {
            const double up = best[(s - 1) * THREADS + tid];
            if (up < d) break;
            const int ui = index[(s - 1) * THREADS + tid];
            if (up == d && rowof(ui) < rowof(j)) break;
            best[s * THREADS + tid] = up;
            index[s * THREADS + tid] = ui;
            --s;
        }
        best[s * THREADS + tid] = d;
        index[s * THREADS + tid] = j;
        kth = best[(ke - 1) * THREADS + tid];
        kidx = index[(ke - 1) * THREADS + tid];
    };
    bool done = ke <= 0;
    if (!brute && !done) {
        const long long key = keys[t];
        const int ix = (int)(key >> (2 * CLOUD_BITS)), iy = (int)((key >> CLOUD_BITS) & CLOUD_CMAX), iz = (int)(key & CLOUD_CMAX);
        const double h = grid[4 * b + 3];
        for (int rho = 0; rho <= CLOUD_MAX_RINGS && !done; ++rho) {
            cloud_scan_ring(keys, lo, hi, ix, iy, iz, rho, visit);
            const double lim = ((double)rho * h) * (1.0 - 0x1p-20);
            done = kth <= lim * lim;
        }
        if (!done) {
            for (int j = 0; j < ke; ++j) best[j * THREADS + tid] = INFINITY, index[j * THREADS + tid] = -1;
            kth = INFINITY, kidx = -1;
        }
    }
    if (!done)
        for (int j = lo; j < hi; ++j) visit(j);
    for (int f = 0; f < GLOBAL_FEATURES; ++f) hist[f * THREADS + tid] = 0;
    const double pi[3] = {px, py, pz};
    const double ni[3] = {normal[3 * (size_t)row], normal[3 * (size_t)row + 1], normal[3 * (size_t)row + 2]};
    const int fi = nflag[row];
    int c = 0;
    for (int u = 0; u < k; ++u) {
        const int j = u < ke ? index[u * THREADS + tid] : -1;
        if (j < lo || j >= hi) {                                            // behind the list; never inside it: the scan fills all ke slots from [lo, hi)
            nbr[(size_t)row * k + u] = -1;
            continue;
        }
        const int rj = brute ? j : order[j];
        nbr[(size_t)row * k + u] = rj - lo;
        const double d2 = best[u * THREADS + tid];
        if (fi != 0 || nflag[rj] != 0 || !(d2 > 0.0)) continue;
        const double pj[3] = {P[3 * (size_t)j], P[3 * (size_t)j + 1], P[3 * (size_t)j + 2]};
        const double nj[3] = {normal[3 * (size_t)rj], normal[3 * (size_t)rj + 1], normal[3 * (size_t)rj + 2]};
        double f[3];
        int bin[3];
        if (!global_pair_feature(pi, ni, pj, nj, d2, f, bin)) continue;
        ++c;
        hist[bin[0] * THREADS + tid] += 1;
        hist[(GLOBAL_BINS + bin[1]) * THREADS + tid] += 1;
        hist[(2 * GLOBAL_BINS + bin[2]) * THREADS + tid] += 1;
    }
    for (int f = 0; f < GLOBAL_FEATURES; ++f) spfh[GLOBAL_FEATURES * (size_t)row + f] = (int)hist[f * THREADS + tid];
    count[row] = c;
}

// ---- descriptors, pass 2: one thread per row, in row order ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GLOBAL_ROW_THREADS) void global_fpfh_kernel(int B, int M, int k, const double* __restrict__ P, const int* __restrict__ offsets,
                                                                         const int* __restrict__ status, const int* __restrict__ nflag,
                                                                         const int* __restrict__ spfh, const int* __restrict__ count,
                                                                         const int* __restrict__ nbr, double* __restrict__ feature,
                                                                         int* __restrict__ has) {
    const int t = blockIdx.x * GLOBAL_ROW_THREADS + threadIdx.x;
    if (t >= M || t >= offsets[B]) return;
    const int b = cloud_of_row(offsets, B, t);
    if (status[b] & ETCH_CLOUD_STATUS_NONFINITE) return;
    const int lo = offsets[b], hi = offsets[b + 1];
    const double px = P[3 * (size_t)t], py = P[3 * (size_t)t + 1], pz = P[3 * (size_t)t + 2];
    double F[GLOBAL_FEATURES];
#pragma unroll
    for (int f = 0; f < GLOBAL_FEATURES; ++f) F[f] = 0.0;
    for (int u = 0; u < k; ++u) {
        const int jl = nbr[(size_t)t * k + u];
        if (jl < 0 || jl >= hi - lo) continue;
        const int j = lo + jl;
        const int cj = count[j];
        const double d2 = cloud_d2(px, py, pz, P + 3 * (size_t)j);
        if (cj <= 0 || !(d2 > 0.0)) continue;
        const double w = 1.0 / d2, dc = (double)cj;
        const int* sj = spfh + GLOBAL_FEATURES * (size_t)j;
#pragma unroll
        for (int f = 0; f < GLOBAL_FEATURES; ++f) F[f] += w * ((100.0 * (double)sj[f]) / dc);
    }
    bool ok = true;
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
        double s = 0.0;
#pragma unroll
        for (int f = 0; f < GLOBAL_BINS; ++f) s += F[GLOBAL_BINS * blk + f];
        const bool pos = s > 0.0;
        ok = ok && pos;
#pragma unroll
        for (int f = 0; f < GLOBAL_BINS; ++f) F[GLOBAL_BINS * blk + f] = pos ? (100.0 * F[GLOBAL_BINS * blk + f]) / s : 0.0;
    }
#pragma unroll
    for (int f = 0; f < GLOBAL_FEATURES; ++f) feature[GLOBAL_FEATURES * (size_t)t + f] = F[f];
    has[t] = nflag[t] == 0 && count[t] > 0 && ok ? 1 : 0;
}

// ---- matching: the target row with the least (D, row) for every source row --------------------------------------------------------------------------
__global__ __launch_bounds__(GLOBAL_MATCH_THREADS) void global_match_kernel(const double* __restrict__ Fs, const int* __restrict__ hs,
                                                                            const int* __restrict__ soff, const double* __restrict__ Ft,
                                                                            const int* __restrict__ ht, const int* __restrict__ toff,
                                                                            int* __restrict__ match, double* __restrict__ dist) {
    __shared__ double tile[GLOBAL_MATCH_TILE * GLOBAL_FEATURES];
    __shared__ int thas[GLOBAL_MATCH_TILE];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int lo = soff[b], hi = soff[b + 1], tlo = toff[b], thi = toff[b + 1];
    const long long first = (long long)lo + (long long)blockIdx.x * GLOBAL_MATCH_THREADS;
    if (first >= hi) return;                                                // uniform over the workgroup: no barrier is skipped by a part of it
    const int i = (int)first + tid;
    const bool inside = i < hi;
    const bool active = inside && hs[i] != 0;
    double a[GLOBAL_FEATURES];
#pragma unroll
    for (int f = 0; f < GLOBAL_FEATURES; ++f) a[f] = active ? Fs[GLOBAL_FEATURES * (size_t)i + f] : 0.0;
    double best = INFINITY;
    int brow = -1;
    for (int t0 = tlo; t0 < thi; t0 += GLOBAL_MATCH_TILE) {
        const int m = thi - t0 < GLOBAL_MATCH_TILE ? thi - t0 : GLOBAL_MATCH_TILE;
        __syncthreads();
        for (int e = tid; e < m * GLOBAL_FEATURES; e += GLOBAL_MATCH_THREADS) tile[e] = Ft[GLOBAL_FEATURES * (size_t)t0 + e];
        if (tid < m) thas[tid] = ht[t0 + tid];
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < m; ++j) {
            if (!thas[j]) continue;
            double D = 0.0;
#pragma unroll
            for (int f = 0; f < GLOBAL_FEATURES; ++f) {
                const double e = a[f] - tile[j * GLOBAL_FEATURES + f];
                D += e * e;
            }
            if (D < best) best = D, brow = t0 + j - tlo;                    // ascending rows: an equal D never replaces a lower row
        }
    }
    if (inside) match[i] = brow, dist[i] = brow >= 0 ? best : INFINITY;
}

// ---- hypotheses: one thread per (pair, h) -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_hypotheses_kernel(int H, const double* __restrict__ A, const double* __restrict__ Q, const int* __restrict__ qrow,
                                                                const int* __restrict__ coff, const unsigned long long* __restrict__ keys, double e2,
                                                                double min2, double* __restrict__ transforms, int* __restrict__ valid,
                                                                int* __restrict__ triples) {
    const int b = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const int lo = coff[b], n = coff[b + 1] - lo;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
    int i0, i1, i2;
    global_hypothesis_rows(keys[b], h, n > 0 ? n : 0, i0, i1, i2);
    bool ok = n >= 3 && i0 != i1 && i0 != i2 && i1 != i2;
    if (ok) {
        const int r0 = qrow[lo + i0], r1 = qrow[lo + i1], r2 = qrow[lo + i2];
        ok = r0 != r1 && r0 != r2 && r1 != r2;
    }
    if (ok) {
        const double* a0 = A + 3 * (size_t)(lo + i0);
        const double* a1 = A + 3 * (size_t)(lo + i1);
        const double* a2 = A + 3 * (size_t)(lo + i2);
        const double* b0 = Q + 3 * (size_t)(lo + i0);
        const double* b1 = Q + 3 * (size_t)(lo + i1);
        const double* b2 = Q + 3 * (size_t)(lo + i2);
        const double sa[3][3] = {{a0[0], a0[1], a0[2]}, {a1[0], a1[1], a1[2]}, {a2[0], a2[1], a2[2]}};
        const double sb[3][3] = {{b0[0], b0[1], b0[2]}, {b1[0], b1[1], b1[2]}, {b2[0], b2[1], b2[2]}};
        ok = global_triple_valid(sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], e2, min2);
        if (ok) ok = global_triple_solve(sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], R, t);
    }
    const size_t o = (size_t)b * H + h;
#pragma unroll
    for (int a = 0; a < 9; ++a) transforms[12 * o + a] = R[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) transforms[12 * o + 9 + a] = t[a];
    valid[o] = ok ? 1 : 0;
    triples[3 * o] = i0, triples[3 * o + 1] = i1, triples[3 * o + 2] = i2;
}

// ---- score: the hot kernel, H n_c transform evaluations per pair -------------------------------------------------------------------------------------
__global__ __launch_bounds__(GLOBAL_SCORE_THREADS) void global_score_kernel(int H, double tau2, const double* __restrict__ A, const double* __restrict__ Q,
                                                                            const int* __restrict__ coff, const double* __restrict__ transforms,
                                                                            const int* __restrict__ valid, int* __restrict__ inliers) {
    __shared__ double sa[3][GLOBAL_SCORE_TILE], sq[3][GLOBAL_SCORE_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int lo = coff[b], hi = coff[b + 1];
    const long long first = (long long)lo + (long long)blockIdx.x * (GLOBAL_SCORE_TILE * GLOBAL_SCORE_TILES_PER_GROUP);
    if (first >= hi) return;                                        // uniform over the workgroup: no barrier is skipped by a part of it
    const int end = first + GLOBAL_SCORE_TILE * GLOBAL_SCORE_TILES_PER_GROUP < hi ? (int)(first + GLOBAL_SCORE_TILE * GLOBAL_SCORE_TILES_PER_GROUP) : hi;
    constexpr int OWN = GLOBAL_SCORE_THREADS * GLOBAL_SCORE_PER_THREAD;
    __shared__ int s_slot[OWN], s_scan[GLOBAL_SCORE_THREADS], s_all;
    const int base = blockIdx.y * OWN;                              // the first rank this workgroup owns
    int mine;                                                       // the hypotheses it owns: 0 .. OWN
    if (valid) {
        const int* v = valid + (size_t)b * H;
        const int chunk = (H + GLOBAL_SCORE_THREADS - 1) / GLOBAL_SCORE_THREADS;      // thread tid looks at the flags [tid chunk, tid chunk + chunk)
        const int a = tid * chunk < H ? tid * chunk : H, e = a + chunk < H ? a + chunk : H;
        int c = 0;
        for (int h = a; h < e; ++h) c += v[h] != 0 ? 1 : 0;
        s_scan[tid] = c;
        __syncthreads();
        if (tid == 0) {                                             // exclusive sums of 256 counts
            int run = 0;
            for (int i = 0; i < GLOBAL_SCORE_THREADS; ++i) {
                const int x = s_scan[i];
                s_scan[i] = run;
                run += x;
            }
        }
        __syncthreads();
        int rank = s_scan[tid];
        for (int h = a; h < e; ++h)
            if (v[h] != 0) {
                if (rank >= base && rank < base + OWN) s_slot[rank - base] = h;
                ++rank;
            }
        if (tid == GLOBAL_SCORE_THREADS - 1) s_all = rank;          // the last thread ends at the number of valid hypotheses
        __syncthreads();
        const int all = s_all;
        mine = all - base < 0 ? 0 : (all - base < OWN ? all - base : OWN);
    } else {
        mine = H - base < OWN ? H - base : OWN;                     // every hypothesis counts: rank = h
    }
    if (mine <= 0) return;                                          // uniform over the workgroup
    double R[GLOBAL_SCORE_PER_THREAD][9], t[GLOBAL_SCORE_PER_THREAD][3];
    int in[GLOBAL_SCORE_PER_THREAD], slot[GLOBAL_SCORE_PER_THREAD];
#pragma unroll
    for (int q = 0; q < GLOBAL_SCORE_PER_THREAD; ++q) {
        const int k = q * GLOBAL_SCORE_THREADS + tid;
        slot[q] = k < mine ? (valid ? s_slot[k] : base + k) : -1;
        const double* tr = transforms + 12 * ((size_t)b * H + (slot[q] >= 0 ? slot[q] : 0));
#pragma unroll
        for (int a = 0; a < 9; ++a) R[q][a] = tr[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) t[q][a] = tr[9 + a];
        in[q] = 0;
    }
    const bool walk = __ballot(slot[0] >= 0) != 0;                  // the owned hypotheses fill the slots from k = 0: a wave without one in q = 0 has none
    for (int t0 = (int)first; t0 < end; t0 += GLOBAL_SCORE_TILE) {
        const int m = end - t0 < GLOBAL_SCORE_TILE ? end - t0 : GLOBAL_SCORE_TILE;
        __syncthreads();
        for (int i = tid; i < m; i += GLOBAL_SCORE_THREADS) {
            const double* p = A + 3 * (size_t)(t0 + i);
            const double* r = Q + 3 * (size_t)(t0 + i);
            sa[0][i] = p[0], sa[1][i] = p[1], sa[2][i] = p[2];
            sq[0][i] = r[0], sq[1][i] = r[1], sq[2][i] = r[2];
        }
        __syncthreads();
        for (int i = 0; walk && i < m; ++i) {
            const double ax = sa[0][i], ay = sa[1][i], az = sa[2][i];
            const double qv[3] = {sq[0][i], sq[1][i], sq[2][i]};
#pragma unroll
            for (int q = 0; q < GLOBAL_SCORE_PER_THREAD; ++q) {
                double x, y, z;
                align_apply(R[q], t[q], ax, ay, az, x, y, z);
                in[q] += cloud_d2(x, y, z, qv) <= tau2 ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < GLOBAL_SCORE_PER_THREAD; ++q)
        if (slot[q] >= 0 && in[q]) atomicAdd(inliers + (size_t)b * H + slot[q], in[q]);
}

// ---- select: one workgroup per pair ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GLOBAL_GROUP) void global_select_kernel(int H, int min_inliers, const double* __restrict__ transforms,
                                                                     const int* __restrict__ valid, const int* __restrict__ inliers,
                                                                     double* __restrict__ Rm, double* __restrict__ tv, int* __restrict__ best,
                                                                     int* __restrict__ best_h, int* __restrict__ found) {
    __shared__ int s_in[GLOBAL_GROUP], s_h[GLOBAL_GROUP];
    const int b = blockIdx.x, tid = threadIdx.x;
    int bi = -1, bh = H;                                            // most inliers, then the lowest h; bh == H: no valid hypothesis seen
    for (int h = tid; h < H; h += GLOBAL_GROUP) {                   // ascending h: a later equal count never replaces an earlier one
        if (!valid[(size_t)b * H + h]) continue;
        const int c = inliers[(size_t)b * H + h];
        if (c > bi) bi = c, bh = h;
    }
    s_in[tid] = bi, s_h[tid] = bh;
    __syncthreads();
    for (int w = GLOBAL_GROUP / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const int oi = s_in[tid + w], oh = s_h[tid + w];
            if (oi > s_in[tid] || (oi == s_in[tid] && oh < s_h[tid])) s_in[tid] = oi, s_h[tid] = oh;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double out[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    int c = 0, hh = -1, ok = 0;
    if (s_h[0] < H && s_in[0] >= min_inliers) {
        const size_t o = (size_t)b * H + s_h[0];
        ok = 1, c = s_in[0], hh = s_h[0];
#pragma unroll
        for (int a = 0; a < 12; ++a) out[a] = transforms[12 * o + a];
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) Rm[9 * b + a] = out[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) tv[3 * b + a] = out[9 + a];
    best[b] = c, best_h[b] = hh, found[b] = ok;
}

// ---- the inliers of one transform per pair, as the pairs of etch_cloud_align_step --------------------------------------------------------------------
__global__ __launch_bounds__(GLOBAL_ROW_THREADS) void global_inliers_kernel(int B, int Ms, double tau2, const double* __restrict__ S,
                                                                            const int* __restrict__ soff, const double* __restrict__ T,
                                                                            const int* __restrict__ toff, const int* __restrict__ match,
                                                                            const double* __restrict__ Rm, const double* __restrict__ tv,
                                                                            int* __restrict__ pair) {
    const int i = blockIdx.x * GLOBAL_ROW_THREADS + threadIdx.x;
    if (i >= Ms || i >= soff[B]) return;
    const int b = cloud_of_row(soff, B, i);
    const int j = match[i], tn = toff[b + 1] - toff[b];
    int out = -1;
    if (j >= 0 && j < tn) {
        double x, y, z;
        align_apply(Rm + 9 * b, tv + 3 * b, S[3 * (size_t)i], S[3 * (size_t)i + 1], S[3 * (size_t)i + 2], x, y, z);
        if (cloud_d2(x, y, z, T + 3 * (size_t)(toff[b] + j)) <= tau2) out = j;
    }
    pair[i] = out;
}

}  // namespace

extern "C" {

int etch_cloud_fpfh(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const double* points,
                    const int* offsets, const double* grid, const int* status, const double* normal, const int* normal_flag, int* spfh, int* count,
                    int* neighbours, double* feature, int* has_feature, void* stream) {
    if (B < 1 || M < 0 || k < 3 || k > ETCH_CLOUD_MAX_K || !sorted_points || !points || !offsets || !status || !normal || !normal_flag || !spfh || !count ||
        !neighbours || !feature || !has_feature)
        return ETCH_EINVAL;
    if (!brute && (!sorted_keys || !order || !grid)) return ETCH_EINVAL;
    if (M == 0) return ETCH_OK;
    hipStream_t st = (hipStream_t)stream;
    if (k <= GLOBAL_WIDE_MAX_K) {
        const size_t lds = (size_t)(12 * k + GLOBAL_HIST_ROWS) * GLOBAL_WIDE_THREADS;
        hipLaunchKernelGGL(global_spfh_kernel<GLOBAL_WIDE_THREADS>, dim3((M + GLOBAL_WIDE_THREADS - 1) / GLOBAL_WIDE_THREADS), dim3(GLOBAL_WIDE_THREADS), lds,
                           st, B, M, k, brute, sorted_points, sorted_keys, order, offsets, grid, status, normal, normal_flag, spfh, count, neighbours);
    } else {
        const size_t lds = (size_t)(12 * k + GLOBAL_HIST_ROWS) * GLOBAL_NARROW_THREADS;
        hipLaunchKernelGGL(global_spfh_kernel<GLOBAL_NARROW_THREADS>, dim3((M + GLOBAL_NARROW_THREADS - 1) / GLOBAL_NARROW_THREADS),
                           dim3(GLOBAL_NARROW_THREADS), lds, st, B, M, k, brute, sorted_points, sorted_keys, order, offsets, grid, status, normal, normal_flag,
                           spfh, count, neighbours);
    }
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(global_fpfh_kernel, dim3((M + GLOBAL_ROW_THREADS - 1) / GLOBAL_ROW_THREADS), dim3(GLOBAL_ROW_THREADS), 0, st, B, M, k, points, offsets,
                       status, normal_flag, spfh, count, neighbours, feature, has_feature);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_feature_match(int B, int Ms, const double* src_feature, const int* src_has, const int* src_offsets, const double* tgt_feature,
                             const int* tgt_has, const int* tgt_offsets, int* match, double* dist, void* stream) {
    if (B < 1 || Ms < 0 || !src_feature || !src_has || !src_offsets || !tgt_feature || !tgt_has || !tgt_offsets || !match || !dist) return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // pairs ride on gridDim.y
    if (Ms == 0) return ETCH_OK;
    hipLaunchKernelGGL(global_match_kernel, dim3((Ms + GLOBAL_MATCH_THREADS - 1) / GLOBAL_MATCH_THREADS, B), dim3(GLOBAL_MATCH_THREADS), 0, (hipStream_t)stream,
                       src_feature, src_has, src_offsets, tgt_feature, tgt_has, tgt_offsets, match, dist);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_global_hypotheses(int B, int H, const double* corr_src, const double* corr_tgt, const int* corr_row, const int* corr_offsets,
                                 const unsigned long long* keys, double edge_similarity, double min_edge, double* transforms, int* valid, int* triples,
                                 void* stream) {
    if (B < 1 || H < 1 || H > ETCH_GLOBAL_MAX_H || !corr_src || !corr_tgt || !corr_row || !corr_offsets || !keys || !transforms || !valid || !triples)
        return ETCH_EINVAL;
    if (!(edge_similarity > 0.0 && edge_similarity <= 1.0) || !(min_edge >= 0.0 && std::isfinite(min_edge))) return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // pairs ride on gridDim.y
    hipLaunchKernelGGL(global_hypotheses_kernel, dim3((H + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, H, corr_src, corr_tgt, corr_row, corr_offsets, keys,
                       edge_similarity * edge_similarity, min_edge * min_edge, transforms, valid, triples);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_global_score(int B, int N, int H, double tau, const double* corr_src, const double* corr_tgt, const int* corr_offsets,
                            const double* transforms, const int* valid, int* inliers, void* stream) {
    if (B < 1 || N < 0 || H < 1 || H > ETCH_GLOBAL_MAX_H || !(tau > 0.0 && std::isfinite(tau)) || !corr_src || !corr_tgt || !corr_offsets || !transforms ||
        !inliers)
        return ETCH_EINVAL;
    if (B > 65535) return ETCH_EUNSUPPORTED;                    // pairs ride on gridDim.z
    hipStream_t st = (hipStream_t)stream;
    const hipError_t cleared = hipMemsetAsync(inliers, 0, (size_t)B * H * sizeof(int), st);
    if (cleared != hipSuccess) return (int)cleared;             // a runtime failure is reported as what it is, not as a bad argument
    if (N == 0) return ETCH_OK;
    const int per = GLOBAL_SCORE_TILE * GLOBAL_SCORE_TILES_PER_GROUP, own = GLOBAL_SCORE_THREADS * GLOBAL_SCORE_PER_THREAD;
    hipLaunchKernelGGL(global_score_kernel, dim3((N + per - 1) / per, (H + own - 1) / own, B), dim3(GLOBAL_SCORE_THREADS), 0, st, H, tau * tau, corr_src,
                       corr_tgt, corr_offsets, transforms, valid, inliers);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_global_select(int B, int H, int min_inliers, const double* transforms, const int* valid, const int* inliers, double* R, double* t, int* best,
                             int* best_h, int* found, void* stream) {
    if (B < 1 || H < 1 || H > ETCH_GLOBAL_MAX_H || !transforms || !valid || !inliers || !R || !t || !best || !best_h || !found) return ETCH_EINVAL;
    hipLaunchKernelGGL(global_select_kernel, dim3(B), dim3(GLOBAL_GROUP), 0, (hipStream_t)stream, H, min_inliers, transforms, valid, inliers, R, t, best, best_h,
                       found);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

int etch_cloud_global_inliers(int B, int Ms, double tau, const double* src_points, const int* src_offsets, const double* tgt_points, const int* tgt_offsets,
                              const int* match, const double* R, const double* t, int* pair, void* stream) {
    if (B < 1 || Ms < 0 || !(tau > 0.0 && std::isfinite(tau)) || !src_points || !src_offsets || !tgt_points || !tgt_offsets || !match || !R || !t || !pair)
        return ETCH_EINVAL;
    if (Ms == 0) return ETCH_OK;
    hipLaunchKernelGGL(global_inliers_kernel, dim3((Ms + GLOBAL_ROW_THREADS - 1) / GLOBAL_ROW_THREADS), dim3(GLOBAL_ROW_THREADS), 0, (hipStream_t)stream, B, Ms,
                       tau * tau, src_points, src_offsets, tgt_points, tgt_offsets, match, R, t, pair);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

}  // extern "C"
