/*
 * etch_hip.h -- C ABI of libetch_hip.so, the MI355X (gfx950) implementation of the ETCH hot path.
 *
 * Every entry point takes plain device pointers + sizes, an explicit HIP stream (hipStream_t passed
 * as void*) and returns an int status: 0 = ok, >0 = hipError_t of the failed launch, -1 = invalid
 * argument, -2 = unsupported size.  The caller owns all memory; kernels are asynchronous on `stream`.
 * No torch types appear in any signature.
 *
 * Each function cites the reference interface it replaces (paths relative to the ETCH repository).
 * INTEGRATION.md shows the binding a reference maintainer would add.
 */
#ifndef ETCH_HIP_H
#define ETCH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- epn_grouping / epn_gathering (external/vgtk/vgtk/cuda) ------------------------------------ */

/* Replaces epn_grouping.ball_query: grouping_cuda.cpp:71-86 -> ball_query_cuda_kernel
 * grouping_cuda_kernel.cu:68-113.  new_xyz (b,3,m) f32, xyz (b,3,n) f32 -> idx (b,m,nsample) i32.
 * First `nsample` support indices (ascending) with d2 < radius^2; rows with cnt < nsample-1 are padded
 * cyclically with their own prefix, the last slot stays 0 when cnt == nsample-1 (reference quirk). */
int etch_ball_query(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz,
                    int* idx, void* stream);

/* Replaces epn_grouping.furthest_point_sampling: grouping_cuda.cpp:158-173 ->
 * furthest_point_sampling_cuda_kernel grouping_cuda_kernel.cu:352-466.  xyz (b,3,n) f32 -> idx (b,m) i32.
 * Start index 0, points with |p|^2 <= 1e-3 never selected, reference tie-breaking reproduced exactly. */
int etch_furthest_point_sampling(int b, int n, int m, const float* xyz, int* idx, void* stream);

/* The same samplers with every scan split over G workgroups (2 <= G <= 8; large scans: one compute unit's distance update bounds the
 * round): bit-identical picks (unique 64-bit keys, grouping_cuda_kernel.cu:352-466 / sampling_cuda_kernel.cu:15-129 tie-breaking).  The
 * G workgroups of a scan exchange one candidate per round through `workspace` (etch_fps_split_workspace_bytes(nseg, G) bytes, zeroed by the
 * call) and must be co-resident: callers keep nseg * G at or below the number of compute units.  A workgroup that waits longer than the
 * spin limit sets the fail word (etch_fps_split_failed, synchronises the stream) and the scan's remaining indices become INT_MIN.
 * etch_fps_split_debug(spin_limit, drop_group): test hook (0 / -1 = defaults). */
int etch_fps_split_workspace_bytes(int nseg, int G);
int etch_furthest_point_sampling_split(int b, int n, int m, const float* xyz, int* idx, int G, void* workspace, void* stream);
int etch_furthestsampling_split(int b, int n_max, const float* xyz, const int* offset, const int* new_offset, int* idx, int G, void* workspace,
                                void* stream);
int etch_fps_split_failed(const void* workspace, int* failed, void* stream);
int etch_fps_split_debug(unsigned spin_limit, int drop_group);
/* A/B switch of the one-workgroup kernels' branch-free slot loop (default 1; 0 = the 64-bit-key loop everywhere): same picks either way. */
int etch_fps_fast(int enable);

/* Replaces epn_gathering.gather_points_forward: gathering_cuda.cpp:29-46 -> gathering_cuda_kernel.cu:43-68.
 * points (b,c,n) f32, idx (b,m) i32 -> out (b,c,m) f32. */
int etch_gather_points(int b, int c, int n, int m, const float* points, const int* idx, float* out, void* stream);

/* Replaces epn_gathering.gather_points_backward: gathering_cuda.cpp:45-60 -> gathering_cuda_kernel.cu:73-98 (the
 * first of the training-side ops): grad_out (b,c,m), idx (b,m) -> grad_points (b,c,n), every element written (no zero-fill needed);
 * contributions of a repeated index are summed in ascending m order (the reference's atomicAdd order is unspecified). */
int etch_gather_points_backward(int b, int c, int n, int m, const float* grad_out, const int* idx, float* grad_points, void* stream);

/* ---- pointops_cuda (external/pointops/src) ------------------------------------------------------ */

/* Replaces knnquery_cuda_launcher: knnquery/knnquery_cuda_kernel.h:10-16, kernel .cu:65-108.
 * xyz (n,3), new_xyz (m,3), offset/new_offset (b) cumulative i32 -> idx (m,nsample) i32, dist (m,nsample) f32.
 * `m_max` = largest number of queries in one segment, `m_total` = total number of queries (grid sizing; known to the
 * host that built the offsets).  m_total > 0 selects the wave-per-query kernel (64-wide distance evaluation, the
 * reference's sequential heap updates preserved); m_total == 0 the thread-per-query kernel.  Results are identical.
 * write_sqrt != 0 stores sqrt(d2) (what pointops.py:43 returns), else d2.  nsample <= 100 (the reference's best_dist[100],
 * knnquery_cuda_kernel.cu:86-87) on the wave-per-query kernel, <= 28 on the thread-per-query form. */
int etch_knnquery(int b, int m_max, int m_total, int nsample, const float* xyz, const float* new_xyz, const int* offset,
                  const int* new_offset, int* idx, float* dist, int write_sqrt, void* stream);

/* Replaces furthestsampling_cuda_launcher: sampling/sampling_cuda_kernel.h:10-16, kernel .cu:15-129.
 * xyz (n,3), offset/new_offset (b) -> idx (new_offset[b-1]) i32 (global indices).  n_max = largest segment.
 * The reference's caller-provided `tmp` scratch is not needed (distances live in registers). */
int etch_furthestsampling(int b, int n_max, const float* xyz, const int* offset, const int* new_offset, int* idx,
                          void* stream);
/* Round 6: the vgtk FPS of a batch (grouping_cuda_kernel.cu:352-466, as etch_furthest_point_sampling) and the pointops FPS of the SAME scans
 * (sampling_cuda_kernel.cu:15-129, as etch_furthestsampling; every segment n points) in one launch of 2 b workgroups -- both chains are one workgroup per
 * scan and depend on the coordinates only; bit-identical picks. */
int etch_fps_pair(int b, int n, int m, const float* xyz_b3n, int* idx_a, const float* xyz_packed, const int* offset, const int* new_offset, int* idx_b,
                  void* stream);

/* etch_knnquery without any host knowledge of the offsets: every query finds its segment on the device by scanning new_offset the way
 * the reference kernel does (knnquery_cuda_kernel.cu:52-62 get_bt_idx, :74-80), the grid is sized from m alone.  Same results as
 * etch_knnquery; this is the form a binding calls when the offsets only exist on the device (no .tolist() / .item() sync). */
int etch_knnquery_dev(int m, int nsample, const float* xyz, const float* new_xyz, const int* offset, const int* new_offset, int* idx,
                      float* dist, int write_sqrt, void* stream);
/* The same with the number of segments given (entries of offset / new_offset: known on the host without a device read): the per-query segment
 * scan is clamped to it.  etch_knnquery_dev keeps the reference launcher's contract (m == new_offset[nseg - 1]). */
int etch_knnquery_dev_bounded(int m, int nsample, int nseg, const float* xyz, const float* new_xyz, const int* offset, const int* new_offset,
                              int* idx, float* dist, int write_sqrt, void* stream);

/* kNN on a per-segment cell grid: etch_knnquery's results bit for bit, from the cells around each query.
 * etch_knn_grid_build: packed xyz (n,3) + offset (nseg) -> pts (n,4) f32 = x, y, z, bits(global index) per point in cell order (z fastest),
 * cell_start (nseg, cell_stride) i32 = first point of every cell relative to the segment, cells + 1 entries used, and header (nseg, 16) words =
 * origin[3], h, 1/h (f32), dims[3], eligible, cells (i32).  One workgroup per segment, at most min(16 384, 4 n, cell_stride - 1) cells
 * (2 <= cell_stride <= 16 385).  A segment is not eligible -- its queries take the full scan -- if it has fewer than max(min_points, 17) or
 * more than 16 384 points, a non-finite coordinate, or no extent. */
int etch_knn_grid_build(int nseg, int min_points, const float* xyz, const int* offset, float* pts, int* cell_start, int cell_stride, int* header,
                        void* stream);
/* etch_knnquery (wave-per-query form) over a grid built from the same xyz and offset.  A query goes to the full scan of etch_knnquery when its
 * segment is not eligible, nsample > 16, it is not finished after 7 shells of cells, or a tied distance makes the any-order result ambiguous.
 * counters (5) i32, may be NULL, are incremented by the number of queries answered from the grid [0] and sent to the full scan for each of
 * these causes [1..4], in that order. */
int etch_knnquery_grid(int b, int m_total, int nsample, const float* xyz, const float* new_xyz, const int* offset, const int* new_offset,
                       const float* pts, const int* cell_start, int cell_stride, const int* header, int* idx, float* dist, int write_sqrt,
                       int* counters, void* stream);

/* ---- the reference's own launcher symbols --------------------------------------------------------------
 * Exactly the names and signatures the reference's host wrappers link against, so knnquery_cuda.cpp / sampling_cuda.cpp (and a
 * pointer-level wrapper of the vgtk kernels) build against libetch_hip.so unchanged.  Like the reference they launch on the NULL
 * stream (`<<<blocks, threads, 0>>>`), return void, and report a failed launch on stderr.  dist2 receives SQUARED distances. */

/* external/pointops/src/knnquery/knnquery_cuda_kernel.h:14 (definition knnquery_cuda_kernel.cu:111-116). */
void knnquery_cuda_launcher(int m, int nsample, const float* xyz, const float* new_xyz, const int* offset, const int* new_offset, int* idx,
                            float* dist2);
/* external/pointops/src/sampling/sampling_cuda_kernel.h:14 (definition sampling_cuda_kernel.cu:131-171).  n = largest segment
 * (pointops.py:20-24); tmp (n_total) is accepted and left untouched (the running minimum distances live in registers). */
void furthestsampling_cuda_launcher(int b, int n, const float* xyz, const int* offset, const int* new_offset, float* tmp, int* idx);
/* Pointer-level forms of the vgtk launches, argument order of the kernels they start:
 * ball_query_cuda_kernel<<<b, opt_n_threads(m)>>>(b,n,m,radius,nsample,new_xyz,xyz,idx)   grouping_cuda_kernel.cu:68-73,476-481
 * furthest_point_sampling_cuda_kernel<<<nb, n_threads>>>(nb,nq,m,source,temp,idx)         grouping_cuda_kernel.cu:352-354,637-642
 * gather_points_forward_kernel / gather_points_backward_kernel                            gathering_cuda_kernel.cu:43-98,103-165 */
void ball_query_cuda_launcher(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int* idx);
void furthest_point_sampling_cuda_launcher(int b, int n, int m, const float* dataset, float* temp, int* idxs);
void gather_points_forward_cuda_launcher(int b, int c, int n, int m, const float* points, const int* idx, float* out);
void gather_points_backward_cuda_launcher(int b, int c, int n, int m, const float* grad_out, const int* idx, float* grad_points);

/* ---- dense per-point layers ----------------------------------------------------------------------- */

/* Y[r,o] = epi(sum_k X[rowmap(r),k] * W[o,k]) on the fp32 matrix cores.  Replaces the un-fused ATen calls
 * torch.nn.Linear / Conv1d(k=1) / Conv2d(1x1) + eval BatchNorm + ReLU used all over the path
 * (src/models/direction_backbones.py:33-35,53-57, src/models/pointtransformer_seg.py:15-22,44-49,66,104-122,144-145,
 * src/models/so3conv.py:166,181).  epi: v = acc + bias[o]; if scale: v = v*scale[o] + shift[o];
 * res_mode 1: v += res[r,o]; act (0 none, 1 relu, 2 leaky 0.01); res_mode 2: v += res[r,o].
 * rowmap: identity when row_idx == NULL; else q = r / grp, src = ((q / p_out) * p_in + row_idx[q]) * grp + r % grp
 * (grp = 1, p_in = 0 gives a plain global row gather).  X, W need not be padded: any K / ld is accepted. */
int etch_linear(int R, int K, int O, const float* X, long ldx, const int* row_idx, int grp, int p_in, int p_out,
                const float* W, long ldw, const float* bias, const float* scale, const float* shift, int act,
                const float* res, long ldr, int res_mode, float* Y, long ldy, void* stream);

/* The encoder's skip conv with the InstanceNorm2d statistics of its output (src/models/so3conv.py:166-168,181) from the GEMM's epilogue:
 *   Y[s][r] = X[rowmap(s, r)] W^T + bias for b samples of `rows` rows each (X and Y contiguous over the samples), mean / rstd (b,O) of Y per
 *   (sample, channel), eps 1e-5 -- what etch_instnorm_stats gives on Y (fp64 sums of the same fp32 values, in another fixed order).
 * rowmap: identity when row_idx == NULL; else rows = p_out * grp and sample s reads source row (s * p_in + row_idx[s * p_out + r / grp]) * grp + r % grp.
 * Y is bitwise etch_linear's: the weight-stationary three-plane kernel without a row map, the fp32 MFMA tile kernel with one (strided = 1 below;
 * (K, O) = (32,64) only).  A sample's rows are divided among etch_linear_stats_parts(rows, strided) workgroups of
 * etch_linear_stats_rows_per_part(rows, strided) rows each (the last one ragged): a function of `rows` alone, so a scan's statistics do not depend
 * on its batch neighbours or on the chip.  partial: workspace of parts * b * 2 * O doubles (16-byte aligned).
 * (K, O) in {(32,32), (64,64), (32,64)}, 16-byte aligned X / W / Y with ld % 4 == 0; otherwise ETCH_EUNSUPPORTED (etch_linear + etch_instnorm_stats). */
int etch_linear_stats(int b, int rows, int K, int O, const float* X, long ldx, const int* row_idx, int grp, int p_in, int p_out,
                      const float* W, long ldw, const float* bias, float* Y, long ldy, double* partial, float* mean, float* rstd, void* stream);
int etch_linear_stats_parts(int rows, int strided);
int etch_linear_stats_rows_per_part(int rows, int strided);

/* ---- EPN encoder (channels-last activations F[b][p][60][c]) -------------------------------------------- */

/* Fused inter-SO(3) convolution.  Replaces inter_so3conv_grouping_anchor + inter_so3conv_feat_grouping
 * (external/vgtk/vgtk/so3conv/functional.py:286-324, 61-67) + BasicSO3Conv (modules.py:33-39): the
 * [b,p2,60,24,nn] kernel-weight tensor is never materialised.
 * xyz (b,3,p1), new_xyz (b,3,p2), ball_idx (b,p2,nn) i32, feats (b,p1,60,cin), rk (60,24,3) = anchors @ kernels^T,
 * W (cout, cin*24) reference layout, Wp = etch fragment order of W (used when cin % 16 == 0), bias (cout)
 * -> out (b,p2,60,cout), pre-normalisation. */
int etch_inter_so3conv(int b, int cin, int cout, int p1, int p2, int nn, float sigma, const float* xyz,
                       const float* new_xyz, const int* ball_idx, const float* feats, const float* rk, const float* W,
                       const float* Wp, const float* bias, float* out, void* stream);

/* The same convolution with an explicit processing order of the output points (a scheduling hint: results are identical).
 * order (b,p2) int32 = a permutation of 0..p2-1 per scan, e.g. from etch_spatial_order; NULL = index order.  Workgroups walk
 * `order`, one contiguous eighth per XCD, so that the workgroups sharing an L2 gather from the same source rows.
 * stat_part (b,p2,2,cout) fp64 or NULL: per output point the sum and the sum of squares of its 60 x cout outputs, i.e. the
 * InstanceNorm2d statistics of so3conv.py:96-99 without a second pass over the output (etch_instnorm_from_partials finishes them);
 * accumulated in fp64 so that a channel whose mean dominates its spread keeps its variance.
 * Round 6: cin == 1 accepts feats == NULL for ALL-ONES features (the encoder's occupancy input, so3conv.py:7-16): the neighbours' feature rows are then
 * neither gathered nor multiplied in. */
int etch_inter_so3conv_ordered(int b, int cin, int cout, int p1, int p2, int nn, float sigma, const float* xyz, const float* new_xyz,
                               const int* ball_idx, const float* feats, const float* rk, const float* W, const float* Wp,
                               const float* bias, float* out, const int* order, double* stat_part, void* stream);

/* The same convolution with its second contraction (W x X1, 1/2 - 2/3 of the flops) on the bf16 matrix cores: every fp32 operand split exactly
 * into three bf16 values (8 + 8 + 8 mantissa bits), the six largest cross products accumulated in fp32 -- the error against fp64 of the fp32
 * MFMA (profiles/r03_bf16x3_split.txt) at 2.3 x its rate.  cin, cout multiples of 16.  Wq: 3 * cout * cin * 24 bf16 =
 * [chunk of 32 kappas][o tile][plane hi / mid / lo][lane][8] in the kernel's contraction order (etch_amd/ops.py inter_weight_split). */
int etch_inter_so3conv_split(int b, int cin, int cout, int p1, int p2, int nn, float sigma, const float* xyz, const float* new_xyz,
                             const int* ball_idx, const float* feats, const float* rk, const void* Wq, const float* bias, float* out,
                             const int* order, double* stat_part, void* stream);

/* 1 if (cin, cout, nn) is a shape the planes kernel (etch_inter_so3conv_planes_kq) is built for. */
int etch_inter_so3conv_planes_supported(int cin, int cout, int nn);

/* Round 5 (etch_amd/csrc/so3conv_y.hip): the inter conv of functional.py:286-324, :61-67 + modules.py:33-39 rebuilt around three measurements of
 * this round (profiles/r05_inter_conv_latency_bound.txt, r05_f16_two_plane_split.txt):
 *   (1) kernel weights off the MATRIX cores: the pre-activation 1 - |g_n - R_a kappa_k|^2 / sigma = [a_n, 1, G_n] . [1, b_k, r_ak] is a rank-5
 *       bilinear form whose six largest exactly-split bf16 cross terms fill one pair of v_mfma_f32_32x32x16_bf16 per (anchor, 32 neighbours);
 *   (2) both contractions on v_mfma_f32_32x32x16_f16 with TWO fp16 planes per operand (x = h + l, h = fp16(x), l = fp16(x - h), both to nearest:
 *       22 significant bits, absolute floor 2^-24; three cross products): for the O(1) operands of this path the error of the fp32 MFMA, with half
 *       the matrix instructions, 4 instead of 6 bytes per gathered element and 40 % of the split work of the three-plane bf16 split;
 *   (3) gathered rows through a register ring (plain loads, several chunks in flight per wave) instead of LDS-direct loads.
 * feats_planes (b, p1, 60, 2, cin) fp16 = etch_split2_planes_f16 / etch_instnorm_act_add_planes_f16 of the fp32 features; kq =
 * etch_inter_kpoint_operand(sigma, rk): [60 anchors][2 K steps][64 lanes][8] bf16 (122 880 bytes), the kernel-point factor in B-fragment order, built
 * once per layer from rk [60][24][3] = anchors @ kernel points (functional.py:296); Wq: 2 * cout * cin * 24 fp16 = the two planes of W, every row (output
 * channel) times the power of two that puts its maximum into [8, 16), in the kernel's physical contraction order,
 * [K step of 16][o tile of 32][plane][lane][8]; wsc (cout floats) = the rows' inverse powers (etch_amd/ops.py inter_weight_split32_f16 and its `.wsc`).
 * fsc: NULL (the planes are those of the features as they stand: InstanceNorm outputs, unit scale by construction) or b floats, scan s's outputs
 * (before the bias) are multiplied by fsc[s] (etch_split2_planes_f16_scaled).  Round 6: persistent workgroups (one grid of 2 x CUs workgroups walks the
 * b * p2 output points, XCD-aware, dynamic beyond the first two points of a workgroup) -- results are bit for bit those of one workgroup per point.
 * Covers every shape of etch_inter_so3conv_planes_supported; order / stat_part as for etch_inter_so3conv.  Same result as the fp32 kernels to
 * ~1e-6 of the output scale (tests/test_gpu_r05.py holds it to the fp32 kernel AND to fp64 under the entitled-error rule). */
int etch_inter_kpoint_operand(float sigma, const float* rk, void* kq, void* stream);
int etch_inter_so3conv_planes_kq(int b, int cin, int cout, int p1, int p2, int nn, float sigma, const float* xyz, const float* new_xyz,
                                 const int* ball_idx, const void* feats_planes, const void* kq, const void* Wq32, const float* wsc, const float* fsc,
                                 const float* bias, float* out, const int* order, double* stat_part, void* stream);

/* x (rows, C) fp32 -> planes (rows, 2, C) fp16: h = fp16(x), l = fp16(x - h), both to nearest (the gather format of etch_inter_so3conv_planes_kq). */
int etch_split2_planes_f16(long rows, int C, const float* x, void* planes, void* stream);
/* Features of unknown scale (callers of the operator API, vgtk so3conv/modules.py:92-128 has no domain restriction): x (b, rows, C) fp32 -> planes
 * (b, rows, 2, C) fp16 of x[s] * 2^k(s), k(s) = the power of two that brings scan s's largest magnitude into [8, 16) (exact), and fsc[s] = 2^-k(s): pass
 * `fsc` to etch_inter_so3conv_planes_kq, whose epilogue multiplies scan s's outputs by it.  mx: b unsigned words of workspace, zeroed by the caller. */
int etch_split2_planes_f16_scaled(int b, long rows, int C, const float* x, void* mx, void* planes, float* fsc, void* stream);

/* x (rows, C) fp32 -> planes (rows, 3, C) bf16: the exact split x = hi + mid + lo (8 + 8 + 8 mantissa bits, by truncation). */
int etch_split3_planes(long rows, int C, const float* x, void* planes, void* stream);

/* mean / rstd (b,C) of InstanceNorm2d(affine=False, eps 1e-5) from per-part partial sums: partial (b,nparts,2,C) fp64, each over `count`
 * values.  Same result as etch_instnorm_stats over the full tensor (fp64 accumulation, fixed order). */
int etch_instnorm_from_partials(int b, int nparts, int C, int count, const double* partial, float* mean, float* rstd, void* stream);
/* The same with the TRUE number of values per (sample, channel) (`total`: the parts need not be equally large).  wide != 0: one workgroup per channel
 * quad and sample instead of one per sample (the same slices and the same order of every sum: the same bits); wide == 0: the one-workgroup form. */
int etch_instnorm_from_partials_n(int b, int nparts, int C, long total, const double* partial, float* mean, float* rstd, int wide, void* stream);

/* Morton (Z-curve) order of each scan's points on its own bounding box, ties by index: xyz (b,3,n) -> order (b,n) int32, a
 * permutation of 0..n-1 per scan.  n <= 16384: 10 bits per axis; larger scans: 5 bits per axis, sorted in independent slices of
 * 32768 points.  No counterpart in the reference: it only schedules etch_inter_so3conv_ordered / etch_prop_interp_ordered. */
int etch_spatial_order(int b, int n, const float* xyz, int* order, void* stream);

/* Fused intra-SO(3) convolution.  Replaces intra_so3conv_grouping (functional.py:331-378) + BasicSO3Conv
 * (modules.py:150-153).  X (b,p,60,c); if mean != NULL the input is first normalised per (b,c) and passed
 * through leaky_relu(0.01) on load (InstanceNorm of the preceding inter block, src/models/so3conv.py:96-99).
 * intra_idx (60,12) i32; Wp = fragment order of W2[o][tap*c + ch] = W[o][ch*12 + tap]; -> Y (b,p,60,cout). */
int etch_intra_so3conv(int b, int c, int cout, int p, const float* X, const float* mean, const float* rstd,
                       const int* intra_idx, const float* Wp, const float* bias, float* Y, void* stream);
/* The same with the InstanceNorm partial sums of Y from the epilogue: stat_part (b * p/2, 2, cout) = per workgroup (2 points) the sum and
 * the sum of squares per output channel; finish with etch_instnorm_from_partials(b, p/2, cout, 120, ...).  p must be even; NULL = plain. */
int etch_intra_so3conv_stats(int b, int c, int cout, int p, const float* X, const float* mean, const float* rstd,
                             const int* intra_idx, const float* Wp, const float* bias, float* Y, double* stat_part, void* stream);
/* The same convolution on the 32x32x2 fp32 MFMA (0.986 of the matrix peak on this chip against 0.85 for 16x16x4, profiles/r03_mfma_issue_rate.txt);
 * c = cout in {32, 64}; Wp32[t][mt][lane][s] = W2[32 mt + lane % 32][8 t + 4 (lane / 32) + s] with W2 as above.  stat_part as above (p even) or NULL. */
int etch_intra_so3conv32(int b, int c, int cout, int p, const float* X, const float* mean, const float* rstd, const int* intra_idx,
                         const float* Wp32, const float* bias, float* Y, double* stat_part, void* stream);

/* The same convolution, weight-stationary on the bf16 matrix cores (csrc/so3conv_ws.hip): fp32 operands split exactly into three bf16 values, six
 * cross products accumulated in fp32 (the fp32 MFMA's error against fp64, profiles/r03_bf16x3_split.txt); W lives in registers for the whole launch,
 * persistent workgroups walk point pairs.  c = cout in {32, 64}; Wq = etch_amd/ops.py intra_weight_split:
 * [mt][kq][K step][plane hi / mid / lo][lane][8 bf16] of W2 above.  stat_part as etch_intra_so3conv_stats (p even) or NULL. */
int etch_intra_so3conv_split(int b, int c, int cout, int p, const float* X, const float* mean, const float* rstd, const int* intra_idx,
                             const void* Wq, const float* bias, float* Y, double* stat_part, void* stream);

/* Round 5: the same kernel on v_mfma_f32_32x32x16_f16 with TWO fp16 planes per operand (h = fp16(x), l = fp16(x - h), both to nearest; three cross
 * products; for this path's unit-scale operands the fp32 MFMA's error against fp64, profiles/r05_f16_two_plane_split.txt).  Wqh = etch_amd/ops.py
 * intra_weight_split_f16: [mt][kq][K step][plane h / l][lane][8 fp16] of W2 with every row (output channel) times its own power of two; wsc (cout
 * floats) = the inverse powers, applied by the kernel's epilogue (exact). */
int etch_intra_so3conv_f16(int b, int c, int cout, int p, const float* X, const float* mean, const float* rstd, const int* intra_idx,
                           const void* Wqh, const float* wsc, const float* bias, float* Y, double* stat_part, void* stream);

/* InstanceNorm2d(affine=False, eps=1e-5) statistics over (p,a) per (b,c) (src/models/so3conv.py:24,85,168).
 * x (b,rows,C) -> mean (b,C), rstd (b,C).  workspace: etch_instnorm_stats_workspace_bytes(b, C) bytes. */
int etch_instnorm_stats(int b, int rows, int C, const float* x, double* workspace, float* mean, float* rstd, void* stream);
int etch_instnorm_stats_workspace_bytes(int b, int C);

/* out = leaky_relu((x1-m1)*r1) [+ leaky_relu((x2-m2)*r2)]: norm + activation + skip add of
 * SeparableSO3ConvBlock.forward (src/models/so3conv.py:178-182).  x2 may be NULL. */
int etch_instnorm_act_add(int b, int rows, int C, const float* x1, const float* m1, const float* r1, const float* x2,
                          const float* m2, const float* r2, float* out, void* stream);
/* The same, additionally writing the result as three bf16 planes (b, rows, 3, C), the format of etch_split3_planes (planes may be NULL). */
/* The same for x1 / x2 / out (b,p,60,C), additionally writing mean (b*p,C) = the mean of out over each point's 60 anchor rows: bitwise what
 * etch_token_mean(b*p, 60, C, out) gives, without re-reading out.  C in {32, 64, 128, 256}; otherwise ETCH_EUNSUPPORTED. */
int etch_instnorm_act_add_mean(int b, int p, int C, const float* x1, const float* m1, const float* r1, const float* x2, const float* m2, const float* r2,
                               float* out, float* mean, void* stream);
int etch_instnorm_act_add_planes(int b, int rows, int C, const float* x1, const float* m1, const float* r1, const float* x2,
                                 const float* m2, const float* r2, float* out, void* planes, void* stream);
/* The same with two fp16 planes (b, rows, 2, C) for etch_inter_so3conv_planes_kq. */
int etch_instnorm_act_add_planes_f16(int b, int rows, int C, const float* x1, const float* m1, const float* r1, const float* x2,
                                     const float* m2, const float* r2, float* out, void* planes, void* stream);
/* Round 6 -- the same with the second branch a ONE-channel 1x1 conv + InstanceNorm folded in (the skip branch of the encoder's first block,
 * so3conv.py:171-183 with dim_in = 1): f [b][rows] holds the branch's input value per row; slope / offset [b][C] = w_c rstd_c and (bias_c - mean_c) rstd_c
 * of its conv output s = w_c f + bias_c (mean_c = w_c mean(f) + bias_c, var_c = w_c^2 var(f): the conv output and its statistics pass are never made):
 *   out = lrelu((x1 - m1) r1) + lrelu(f slope_c + offset_c);  planes (may be NULL): the two fp16 planes of out. */
int etch_instnorm_act_add_k1_planes_f16(int b, int rows, int C, const float* x1, const float* m1, const float* r1, const float* f, const float* slope,
                                        const float* offset, float* out, void* planes, void* stream);

/* ---- feature propagation + direction head --------------------------------------------------------------- */

/* 3-NN of PointFeatPropagation (src/models/pointnet2_utils.py:45-70): xyz1 (B,N,3), xyz2 (B,3,S) ->
 * idx (B,N,3) i32 (ascending distance), weight (B,N,3) = normalised 1/(d2+1e-8) with d2 from the
 * reference's expansion formula -2xy + |x|^2 + |y|^2 in fp32. */
int etch_prop3nn(int B, int N, int S, const float* xyz1, const float* xyz2, int* idx, float* weight, void* stream);

/* Weighted gather (pointnet2_utils.py:71) + anchor mean (models_pointcloud.py:184): feats (B,S,A,C) channels-last
 * -> out (B,N,A,C), inv (B,N,C) = mean over A.  C in {32,64,128}. */
int etch_prop_interp(int B, int N, int S, int A, int C, const float* feats, const int* idx, const float* weight,
                     float* out, float* inv, void* stream);
/* The same with a processing order of the fine points (scheduling hint, results identical): order (B,N) int32 from
 * etch_spatial_order, NULL = index order. */
int etch_prop_interp_ordered(int B, int N, int S, int A, int C, const float* feats, const int* idx, const float* weight,
                             float* out, float* inv, const int* order, void* stream);

/* DotProdAttention of MultiHeadAttention (src/models/direction_backbones.py:102-129,160-194) for 60 tokens,
 * 8 heads x 8 dims: rows [T*60][ld] hold q/k/v at column offsets qoff/koff/voff -> out rows [T*60][ldo] (64 cols). */
int etch_mhsa_attention(long T, const float* qkv, long ld, int qoff, int koff, int voff, float* out, long ldo, void* stream);
/* The same attention core for the other encoder depths (models_pointcloud.py:34-48: embedding_dim 32 / 64 / 128 / 256 -> 8 heads of
 * 4 / 8 / 16 / 32, direction_backbones.py:151; logits / sqrt(head size), :125).  out (T*60, ldo) = concatenated heads. */
int etch_mhsa_attention_dim(long T, int embedding_dim, const float* qkv, long ld, int qoff, int koff, int voff, float* out, long ldo,
                            void* stream);

/* One whole MultiHeadAttention layer (direction_backbones.py:132-194; 64 dims, 8 heads x 8, 60 tokens per point) in a single
 * kernel: q/k/v transforms (no bias, weights (64,64) row-major as in key/query/value_transform.weight) -> per-head softmax
 * attention -> head_combine (Wc (64,64), bc (64)).  X, out: (T*60, 64) contiguous.
 * mode 0: out = X + att Wc^T + bc  (the residual form StackedMHSA.forward :216-221 applies to all but the last layer)
 * mode 1: out = att Wc^T + bc       mode 2: out = att (concatenated heads; Wc/bc unused -- head_combine folded downstream) */
int etch_mhsa_layer(long T, const float* X, const float* Wq, const float* Wk, const float* Wv, const float* Wc, const float* bc,
                    int mode, float* out, void* stream);
/* Round 5: the LAST attention layer of the direction head with the folded tail inside (models_pointcloud.py:115-117): out (T, 60) =
 * v . relu(Wf att + bf) + c per token, the anchor weights that so3_mean consumes -- the (T*60, 64) attention output and the (T*60, 128) hidden layer
 * never reach HBM.  Wfq = the two fp16 planes of Wf with every hidden unit's row times its own power of two, the powers folded into tab (ops.dirtail_weight_split /
 * dirtail_constants) (Wf 128 x 64 = direction_predictor.net[0] o head_combine, folded on the host) as matrix-core A
 * fragments [4 waves][4 K steps][2 planes][64 lanes][8] (etch_amd/ops.py dirtail_weight_split); tab = [bf (128) | v (128) | c] fp32 (257 floats). */
int etch_mhsa_layer_dirtail(long T, const float* X, const float* Wq, const float* Wk, const float* Wv, const void* Wfq, const float* tab,
                            float* out, void* stream);

/* The first MultiHeadAttention layer of the direction head applied to 3-NN INTERPOLATED tokens (PointFeatPropagation,
 * pointnet2_utils.py:45-74, feeding StackedMHSA, direction_backbones.py:216-221) without writing them out: F (B,S,60,64) coarse
 * tokens, idx / weight (B,N,3) from etch_prop3nn, order (B,N) int32 or NULL (scheduling only), weights as etch_mhsa_layer
 * -> out (B*N*60, 64) = X + att Wc^T + bc with X = the interpolated tokens (mode 0 of etch_mhsa_layer on etch_prop_interp's output).
 * sched: workspace of B*N*8 int32 (16-byte aligned).
 * etch_token_mean: X (T,A,C) -> mean over the A tokens (T,C) (the anchor mean of models_pointcloud.py:184 at the coarse points). */
int etch_mhsa_interp_layer(int B, int N, int S, const float* F, const int* idx, const float* weight, const int* order, const float* Wq,
                           const float* Wk, const float* Wv, const float* Wc, const float* bc, float* out, int* sched, void* stream);
int etch_token_mean(long T, int A, int C, const float* X, float* mean, void* stream);
/* etch_mhsa_interp_layer at a LIST of points (the fit paths evaluate the direction head at the marker points only): sel (B,P) int32 = global
 * point rows b*N + n, or -1 for an empty slot (computed on point 0 of the slot's scan; its output is to be ignored) -> out (B*P*60, 64), slot k at
 * rows 60 k ...; bitwise the rows of that point in etch_mhsa_interp_layer's output.  sched: workspace of B*P*8 int32 (16-byte aligned). */
int etch_mhsa_interp_layer_list(int B, int P, int N, int S, const float* F, const int* sel, const int* idx, const float* weight, const float* Wq,
                                const float* Wk, const float* Wv, const float* Wc, const float* bc, float* out, int* sched, void* stream);

/* y[r] = x[r,:K] . w + bias: so3_reg Conv1d(128,1,1) (src/models/models_pointcloud.py:54,117). */
int etch_rowdot(long R, int K, const float* x, long ldx, const float* w, float bias, float* y, void* stream);

/* so3_mean (src/models/so3conv.py:186-225) + R @ [0,0,1] (models_pointcloud.py:120-124): w (T,60), anchors (60,3,3)
 * -> dir (T,3); optional R (T,3,3) and singular values sv (T,3) (NULL to skip). */
int etch_so3_mean_dir(long T, int A, const float* w, const float* anchors, float* dir, float* R, float* sv, void* stream);
/* Backward of etch_so3_mean_dir (autograd through so3conv.py:186-225 + models_pointcloud.py:120-124 in train.py:77-85): ddir (T,3) = dL/d dir
 * -> dw (T,A) = dL/d w.  Derivative of the polar factor through the 3x3 Sylvester equation in V's basis, fp64 per point. */
int etch_so3_mean_dir_backward(long T, int A, const float* w, const float* anchors, const float* ddir, float* dw, void* stream);
/* Backward of the 3-NN propagation (pointnet2_utils.py:45-74; forward etch_prop_interp) and of any weighted row gather:
 * dst (nseg,C)[q] = sum_{k in [seg[q], seg[q+1])} wgt[perm[k]] * src[perm[k] / fan], perm = stable sort of the flattened (rows, fan) index
 * list by target row, seg its offsets (int64): scatter-add in a fixed order.  C % 4 == 0. */
int etch_weighted_segment_sum_rows(long nseg, int C, int fan, const float* src, const float* wgt, const long long* perm, const long long* seg,
                                   float* dst, void* stream);

/* ---- Point-Transformer heads (src/models/pointtransformer_seg.py) ------------------------------------------ */

/* PointTransformerLayer.forward after the q/k/v Linear layers (pointtransformer_seg.py:28-36; grouping as
 * src/models/pointops.py:79-100).  p (n,3); xq/xk/xv rows with leading dimension ldq; idx (n,ns) kNN indices;
 * params = 14 device pointers: linear_p[0] W(3x3), b(3); BN(3) folded scale, shift; linear_p[3] W(c,3), b(c);
 * linear_w[0] BN(c) scale, shift; linear_w[2] W TRANSPOSED (c, c/8), b(c/8); linear_w[3] BN(c/8) scale, shift;
 * linear_w[5] W(c/8,c/8), b(c/8); then an optional output BN(c) scale, shift (+ReLU) = block.bn2 (:117), NULL to skip
 * (16 pointers in total).  -> out (n,c) rows with leading dimension ldo. */
int etch_pt_attention(int n, int c, int ns, const float* p, const float* xq, const float* xk, const float* xv, long ldq,
                      const int* idx, const float* const* params, float* out, long ldo, void* stream);

/* The same layer split around the matrix cores (the schedule the model uses): prep builds the attention-MLP input
 * w_in[(i,j),:] = relu(bn(x_k[idx] - x_q + p_r)) (pointtransformer_seg.py:31-33 up to the first Linear), the two Linear
 * layers of linear_w run through etch_linear over all n*ns rows, aggregate applies softmax over the neighbours and the
 * shared-plane weighted sum (:34-36) [+ block.bn2 + ReLU].  params: the same 16 pointers as etch_pt_attention. */
int etch_pt_attn_prep(int n, int c, int ns, const float* p, const float* xq, const float* xk, long ldq, const int* idx,
                      const float* const* params, float* w_in, void* stream);
int etch_pt_attn_aggregate(int n, int c, int ns, const float* p, const float* xv, long ldq, const int* idx, const float* logits,
                           const float* const* params, float* out, long ldo, void* stream);

/* The same attention core in one matrix-core kernel: the c -> c/8 -> c/8 MLP of linear_w runs as two chained MFMA products on
 * w_in rows built in registers from the gathered k rows; softmax over the neighbours and the aggregation of (v + p_r) follow in
 * the same wave.  W2 = linear_w[2].weight (c/8, c) row-major (params[8] holds its transpose for the other variants).
 * (c, ns) in {(64,8), (128,8), (64,16), (128,16), (256,16), (512,16)}, otherwise ETCH_EUNSUPPORTED (-2). */
int etch_pt_attention_mfma(int n, int c, int ns, const float* p, const float* xq, const float* xk, const float* xv, long ldq,
                           const int* idx, const float* const* params, const float* W2, float* out, long ldo, void* stream);

/* queryandgroup(use_xyz=True) rows for TransitionDown (pointtransformer_seg.py:61, pointops.py:90-98):
 * out[(i*ns+j)] = [p[idx[i,j]] - new_p[i] | x[idx[i,j]] | 0...], row stride ldo >= 3+c (padding columns zeroed). */
int etch_pt_group(int m, int ns, int c, const float* p, const float* new_p, const float* x, long ldx, const int* idx,
                  float* out, long ldo, void* stream);

/* Row gather n_p = p[idx] (pointtransformer_seg.py:60): out[i,:c] = x[idx[i],:c]. */
int etch_gather_rows(int m, int c, const float* x, long ldx, const int* idx, float* out, void* stream);

/* TransitionDown with stride (pointtransformer_seg.py:40-68) without the m*ns grouped rows: ux = x Wx^T per SOURCE point (n, co),
 * Wx = linear.weight[:, 3:]; this kernel adds the coordinate part Wp (p_j - p_i), Wp = linear.weight[:, :3] (co,3), applies the
 * folded BatchNorm + ReLU and max-pools over the ns neighbours:  out[i,o] = max_j relu(bn(ux[idx[i,j],o] + Wp[o].(p[idx[i,j]] - new_p[i]))). */
int etch_pt_down_gather_max(int m, int ns, int co, const float* ux, long ldu, const float* p, const float* new_p, const int* idx,
                            const float* Wp, const float* scale, const float* shift, float* out, void* stream);

/* MaxPool1d(nsample) over consecutive row groups (pointtransformer_seg.py:63): x (m*ns, c) -> out (m, c). */
int etch_rows_maxpool(int m, int ns, int c, const float* x, float* out, void* stream);

/* TransitionUp tail (pointtransformer_seg.py:97, pointops.py:164-178): out = a + sum_k w_k f[idx_k],
 * w = (1/(dist+1e-8))/sum with the NON-squared kNN distances.  a,out (n,c); f (m,c); idx,dist (n,3). */
int etch_pt_interp_add(int n, int c, const float* a, const float* f, const int* idx, const float* dist, float* out, void* stream);

/* TransitionUp head branch (pointtransformer_seg.py:83-93): per-segment mean, and [x | g[segment]] concat. */
int etch_seg_mean(int nseg, int c, const float* x, const int* offset, float* mean, void* stream);
int etch_concat_bcast(int n, int c, int nseg, const float* x, const float* g, const int* offset, float* out, void* stream);

/* confi[2]: Conv1d(G*J, G, 1, groups=G) (pointtransformer_seg.py:145): out[r,g] = h[r, g*J:(g+1)*J] . w[g] + b[g]. */
int etch_grouped_dot(long R, int G, int J, const float* h, long ldh, const float* w, const float* bias, float* out, long ldo,
                     void* stream);

/* Fused Conv1d(K, G*J, 1) -> ReLU -> Conv1d(G*J, G, 1, groups=G) of the confidence head (pointtransformer_seg.py:145,
 * applied at :183-189; G = k markers, J = K = 128) and of the direction-head tail MLP.net[0] -> ReLU -> (net[2] o so3_reg)
 * (models_pointcloud.py:115-117, direction_backbones.py:38-75; G = 1, K = 64, J = 128):
 *   out[r,g] = b2[g] + sum_{j<J} relu(X[r,:] . W[g*J+j,:] + b1[g*J+j]) * w2[g*J+j]
 * The (R x G*J) hidden activations never leave the chip.  X (R,K) row stride ldx; W (G*J,K) row stride ldw; Wp = optional
 * copy of W in MFMA fragment order [G][K/16][8][64][4] (Wp[g][t][s][l][e] = W[g*J+16s+l%16][16t+4(l/16)+e]; NULL -> W is
 * read directly); out (R,G) row stride ldo.  J must be 128, K 64 or 128; ldx % 4 == 0, 16-byte aligned pointers. */
int etch_linear_relu_dot(long R, int K, int G, int J, const float* X, long ldx, const float* W, long ldw, const float* Wp,
                         const float* b1, const float* w2, const float* b2, float* out, long ldo, void* stream);

/* The same chain on the bf16 matrix cores with exactly split fp32 operands (three bf16 values per fp32 value, six cross products accumulated in
 * fp32: the fp32 MFMA's error against fp64, profiles/r03_bf16x3_split.txt).  K in {32, 64, 128, 256}, J = 128.  Wq = etch_amd/ops.py
 * lrd_weight_split: [g][K/32][8 strips][plane hi / mid / lo][lane][8 bf16]. */
int etch_linear_relu_dot_split(long R, int K, int G, int J, const float* X, long ldx, const void* Wq, const float* b1, const float* w2,
                               const float* b2, float* out, long ldo, void* stream);

/* Round 5: the weight-stationary form of the same chain on v_mfma_f32_16x16x32_f16 with TWO fp16 planes per operand (three cross terms; half the matrix
 * instructions).  Neither operand carries a known scale: each row of X is staged times the power of two that puts its maximum into [8, 16), each row of
 * W (hidden unit) likewise on the host; both powers leave in the epilogue's fmaf with the bias (exact).  Wqh = etch_amd/ops.py lrd_weight_split_f16;
 * wsc (G * J floats) = the weight rows' inverse powers.  K in {32, 64, 128}, G = 1 or G >= 8, b1 / w2 / wsc 16-byte aligned; other shapes:
 * ETCH_EUNSUPPORTED (the caller keeps etch_linear_relu_dot_split / etch_linear_relu_dot). */
int etch_linear_relu_dot_f16(long R, int K, int G, int J, const float* X, long ldx, const void* Wqh, const float* wsc, const float* b1, const float* w2,
                             const float* b2, float* out, long ldo, void* stream);

/* confidence = sum_g softmax(logits)_g * v_g (pointtransformer_seg.py:183-189): (R,G),(R,G) -> (R). */
int etch_softmax_dot(long R, int G, const float* logits, const float* v, float* out, void* stream);

/* so3_mean with the reference's own signature (src/models/so3conv.py:186-225): Rs (T,A,3,3) [rs_stride = A*9] or one rotation set
 * shared by all rows [rs_stride = 0], weights w (T,A) or NULL (uniform) -> chordal-L2 mean rotation R (T,3,3). */
int etch_so3_mean(long T, int A, const float* Rs, long rs_stride, const float* w, float* R, void* stream);

/* ---- un-fused operator forms of the reference's functional API (never on the hot path; csrc/functional_ops.hip) ---------- */

/* inter_so3conv_grouping_anchor (external/vgtk/vgtk/so3conv/functional.py:286-324): grouped_xyz (b,3,p,nn), rotated kernel points
 * (na,ks,3) = anchors @ kernels^T -> w (b,p,na,ks,nn) = relu(1 - |g - R_a kappa_k|^2 / sigma). */
int etch_inter_kernel_weights(int b, int p, int nn, int na, int ks, const float* grouped_xyz, const float* rotated_kernels, float sigma,
                              float* w, void* stream);

/* inter_so3conv_feat_grouping (functional.py:61-67): idx (b,p,nn) i32 into the q rows of feats (b,c,q,na) [q includes the shadow
 * row of add_shadow_feature, :101-105], w (b,p,na,ks,nn) -> (b,c,ks,p,na). */
int etch_inter_feat_grouping(int b, int c, int q, int p, int nn, int na, int ks, const int* idx, const float* w, const float* feats,
                             float* out, void* stream);

/* intra_so3conv_grouping (functional.py:331-378): intra_idx (na,nt) i64, feat (b,c,p,na) -> (b,c,nt,p,na). */
int etch_intra_grouping(int b, int c, int p, int na, int nt, const long long* intra_idx, const float* feat, float* out, void* stream);

/* square_distance (src/models/pointnet2_utils.py:4-23): src (B,N,C), dst (B,M,C) -> (B,N,M), expansion formula in the reference's
 * operation order. */
int etch_square_distance(int B, int N, int M, int C, const float* src, const float* dst, float* out, void* stream);

/* index_points (pointnet2_utils.py:26-43): points (B,N,C), idx (B,S) i64 -> (B,S,C). */
int etch_index_points(int B, int N, long S, int C, const float* points, const long long* idx, float* out, void* stream);

/* ---- backward kernels of the encoder's native ops (csrc/backward.hip).  The reference gets these gradients from
 * torch.autograd through the un-fused forms (vgtk/so3conv/functional.py:224-324, :61-67; modules.py:33-39, :131-153; src/models/
 * so3conv.py:24-44; call sites src/train.py:77-101).  All reductions run in a fixed order (no atomics). ---------------------------- */

/* Grouped features of the inter conv, recomputed for output points [p_begin, p_begin + pc): x1 (b, pc, 60, cin*24) with
 * x1[.., a, c*24+k] = sum_n feats[b, idx[b,p,n], a, c] * w[p,a,k,n]  (feats channels-last (b,p1,60,cin); w regenerated from xyz). */
int etch_inter_x1_rows(int b, int cin, int p1, int p2, int p_begin, int pc, int nn, float sigma, const float* xyz, const float* new_xyz,
                       const int* ball_idx, const float* feats, const float* rk, float* x1, void* stream);

/* C (M,N) (+)= A (R,M)^T B (R,N) (dW = dY^T X1: the weight gradients, sums over every row of the batch) on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64: fp32 operands widened exactly, exact products, fp64 accumulation -- these sums cancel to ~1e-7 of their terms for the
 * direction head, profiles/r05_weight_gradient_accumulation.txt): split over R, fp64 partial tiles in `workspace`
 * (etch_gemm_tn_workspace_floats(R, M, N) floats), summed in split order, rounded to fp32 once. */
int etch_gemm_tn_workspace_floats(long R, int M, int N);
int etch_gemm_tn(long R, int M, int N, const float* A, long lda, const float* B, long ldb, float* C, int accumulate, float* workspace,
                 void* stream);
/* etch_gemm_tn in ONE launch: the workgroup of a 64 x 64 tile of C that finishes last sums the tile's partials in split order (bit for bit
 * etch_gemm_tn's result).  counters: 64 unsigned, zero before the first call, left zero (see etch_bn_train_forward); more than 64 tiles or more
 * than 64 row ranges per tile (long-and-narrow products): the two-launch form. */
int etch_gemm_tn_fused(long R, int M, int N, const float* A, long lda, const float* B, long ldb, float* C, int accumulate, float* workspace,
                       unsigned* counters, void* stream);

/* d feats of the inter conv from d x1 of the output points [p_begin, p_begin + pc): dfeats (b,p1,60,cin) (+)= the gather-side sum over
 * the neighbour slots (p,n) with idx[b,p,n] == q, taken in slot order.  cin in {4..64}, multiple of 4. */
int etch_inter_dfeat(int b, int cin, int p1, int p2, int p_begin, int pc, int nn, float sigma, const float* xyz, const float* new_xyz,
                     const int* ball_idx, const float* rk, const float* dx1, float* dfeats, int accumulate, void* stream);
/* The same gradient from the target side (round 6): contrib [b][pc][nn][60][cin] receives, per neighbour slot (p, n) of the chunk, the row
 * sum_k w[p,a,k,n] dX1[(p,a), c*24+k]; d feats[b, q] = the sum of the rows of the slots with ball_idx == q, which the caller takes with
 * etch_segment_sum_rows over a stable sort of the slots by source point (fixed order: reproducible).  Reads every dX1 tile once instead of nn times.
 * nn <= 64; cin as for etch_inter_dfeat.  A slot with ball_idx < 0 gets a zero row. */
int etch_inter_dfeat_slots(int b, int cin, int p1, int p2, int p_begin, int pc, int nn, float sigma, const float* xyz, const float* new_xyz,
                           const int* ball_idx, const float* rk, const float* dx1, float* contrib, void* stream);

/* Gathered operand of the intra conv's weight gradient: x (points,60,C) -> xg (points,60,nt,C) with xg[p,a,t,:] = x[p,intra_idx[a,t],:]
 * (functional.py:331-378 in channels-last rows). */
int etch_intra_rows(long points, int C, int nt, const int* intra_idx, const float* x, float* xg, void* stream);

/* Backward of the vector-attention core of etch_pt_attention (pointtransformer_seg.py:28-36, eval-mode BatchNorm as folded constants, no
 * output BN): arguments as etch_pt_attention (params[0..13]) + dout (n,c) rows with leading dimension lddo.  outs = 10 device pointers,
 * rows indexed by e = i*ns + j:  GV (E,c) gradient of (x_v[idx] + p_r);  GU (E,c) gradient of x_k[idx] - x_q + p_r;  A (E,c), DZ (E,c/8)
 * input / output-gradient rows of linear_w[2];  G (E,c/8), DL (E,c/8) the same for linear_w[5];  H4, DH4, R4 (E,4) hidden, output
 * gradient of linear_p[0] and relative positions (3 used);  dxq (n,c) = -sum_j GU.  The caller closes the sums over rows with
 * etch_gemm_tn / etch_colsum and scatters GV / GU to the source points with etch_segment_sum_rows (etch_amd/autograd.py). */
int etch_pt_attention_backward(int n, int c, int ns, const float* p, const float* xq, const float* xk, const float* xv, long ldq, const int* idx,
                               const float* const* params, const float* dout, long lddo, float* const* outs, void* stream);
/* dst[q,:] = sum of src[perm[k],:] for k in [seg[q], seg[q+1]) in that order (perm = stable sort of an index list by target row, seg its
 * segment offsets, int64): the reproducible form of scatter-add.  C % 4 == 0. */
int etch_segment_sum_rows(long nseg, int C, const float* src, const long long* perm, const long long* seg, float* dst, void* stream);

/* ---- training-side kernels of the Point-Transformer nets (train.py:77-101 through pointtransformer_seg.py in train() mode; etch_amd/autograd_pt.py) */
/* BatchNorm1d batch statistics of the rows of x (R,C; leading dimension ldx): mean[c], biased var[c], summed in fp64 in a fixed order.
 * workspace: 64 * 2 * C doubles. */
int etch_bn_stats(long R, int C, const float* x, long ldx, double* workspace, float* mean, float* var, void* stream);
/* y (R,C) = act((x - mean[c]) * scale[c] + beta[c]) with scale = gamma / sqrt(var + eps); act = ReLU if relu != 0. */
int etch_bn_apply(long R, int C, const float* x, long ldx, const float* mean, const float* scale, const float* beta, int relu, float* y, void* stream);
/* Backward of y = act(gamma * (x - mean) * rstd + beta): dgamma, dbeta and (dx != NULL) dx.  train != 0: mean / rstd are the batch
 * statistics of x (torch.nn.BatchNorm1d in train() mode); train == 0: constants (running statistics).  y is read only when relu != 0.
 * workspace: 64 * 2 * C doubles. */
int etch_bn_backward(long R, int C, const float* x, long ldx, const float* y, const float* dy, const float* mean, const float* rstd, const float* gamma,
                     int relu, int train, double* workspace, float* dx, float* dgamma, float* dbeta, void* stream);
/* Round 6 -- the same reductions in ONE launch each (the workgroup that finishes last sums the partials in their fixed order: results bit for bit those
 * of the two-launch forms above).  counters: ETCH_REDUCE_COUNTERS (64) unsigned, ZERO before the first call and left zero by every call; calls that
 * share `counters` / `workspace` must be ordered on one stream.
 * etch_bn_train_forward = torch.nn.functional.batch_norm(training=True) (+ ReLU) on rows (pointtransformer_seg.py's nn.BatchNorm1d in train() mode,
 * train.py:77-101): batch statistics -> mean, rstd = 1/sqrt(var + eps), scale = gamma rstd (kept for the backward), y = act((x - mean) scale + beta),
 * and -- when running_mean / running_var are given -- running = (1 - momentum) running + momentum {mean, unbiased var} (momentum < 0: the cumulative
 * average over *num_batches + 1 calls); *num_batches += 1 when given.  2 launches.  workspace: 64 * 2 * C doubles; C <= 4096. */
int etch_bn_train_forward(long R, int C, const float* x, long ldx, const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, long long* num_batches, int relu, double* workspace, unsigned* counters,
                          float* mean, float* rstd, float* scale, float* y, void* stream);
/* etch_bn_backward with the column sums and their final reduction in one launch (2 launches with dx). */
int etch_bn_backward_fused(long R, int C, const float* x, long ldx, const float* y, const float* dy, const float* mean, const float* rstd,
                           const float* gamma, int relu, int train, double* workspace, unsigned* counters, float* dx, float* dgamma, float* dbeta,
                           void* stream);
/* Backward of etch_rows_maxpool (nn.MaxPool1d(nsample), pointtransformer_seg.py:66): dy (m*ns,c) = dout at the first maximum of each group. */
int etch_rows_maxpool_backward(long m, int ns, int c, const float* y, const float* dout, float* dy, void* stream);
/* The tail of PointTransformerLayer.forward (pointtransformer_seg.py:34-36): softmax over the ns neighbours of logit (n*ns, cs), then
 * out[i, s*cs + j] = sum_k sm[i,k,j] v[i,k,s*cs + j] for v (n*ns, c); sm (n*ns, cs) is kept for the backward. */
int etch_pt_softmax_agg(long n, int ns, int c, int cs, const float* logit, const float* v, float* sm, float* out, void* stream);
int etch_pt_softmax_agg_backward(long n, int ns, int c, int cs, const float* sm, const float* v, const float* dout, float* dlogit, float* dv, void* stream);

/* Backward of the 8-head dot-product attention over a point's 60 tokens (direction_backbones.py:102-129; autograd through it in
 * train.py:77-101): qkv rows [T*60][ld] with q / k / v at column offsets qoff / koff / voff (the layout of etch_mhsa_attention), dO rows
 * [T*60][ldo] = gradient of the concatenated head outputs -> dqkv rows [T*60][ld] at the same offsets.  Fixed summation order. */
int etch_mhsa_attention_backward(long T, const float* qkv, long ld, int qoff, int koff, int voff, const float* dO, long ldo, float* dqkv,
                                 void* stream);
/* The same for the other encoder depths: embedding_dim in {32, 64, 128, 256} = 8 heads of width 4 / 8 / 16 / 32 (models_pointcloud.py:34-48). */
int etch_mhsa_attention_backward_dim(long T, int embedding_dim, const float* qkv, long ld, int qoff, int koff, int voff, const float* dO, long ldo,
                                     float* dqkv, void* stream);

/* Column sums s[c] = sum_r x[r,c] (bias gradients): fp64, two levels, fixed order.  workspace: 64*C doubles. */
int etch_colsum(long R, int C, const float* x, double* workspace, float* out, void* stream);

/* The same in one coalesced launch (x with leading dimension ldx; counters / ordering as etch_bn_train_forward); C > 4096: the two-launch form
 * (which needs ldx == C). */
int etch_colsum_fused(long R, int C, const float* x, long ldx, double* workspace, unsigned* counters, float* out, void* stream);

/* d/dx of leaky_relu(InstanceNorm2d(x), slope) (so3conv.py:36-44): x, dy (b,rows,C) channels-last, mean / rstd (b,C) of the forward. */
int etch_instnorm_act_backward_workspace_bytes(int b, int C);
int etch_instnorm_act_backward(int b, int rows, int C, const float* x, const float* dy, const float* mean, const float* rstd, float slope,
                               double* workspace, float* dx, void* stream);

/* ---- stage 2: markers + SMPL Levenberg-Marquardt fit ------------------------------------------------------ */

/* torch.max(part_labels, -1) of predict_smpl (src/inference_demo.py:52-53): logits (R,G) -> int64 labels (R).
 * The first maximum; -0 == +0; a NaN of either sign is the greatest value and the first NaN wins. */
int etch_argmax_rows(long R, int G, const float* logits, long long* out, void* stream);

/* pred_inner_points = points - direction * magnitude / scale_magnitude (src/inference_demo.py:58-59): (n,3),(n,3),(n) -> (n,3). */
int etch_inner_points(long n, const float* pts, const float* dir, const float* mag, float scale, float* out, void* stream);

/* get_markers (src/models/fit_SMPL.py:17-62): pts (B,K,3), labels (B,K) i64, conf (B,K,1) -> markers (B,M,3),
 * valid as float (B,M) and/or as bool bytes (B,M) (either may be NULL).  Per (scan,label): top-3 confidences,
 * weights conf^20, weighted centre; empty label -> zeros + invalid.  The confidences are ordered as by torch.topk where that defines an
 * order (a NaN of either sign greatest -- the marker is then NaN and etch_marker_status flags it -- and -0 == +0); equal ones go to the lower index. */
int etch_get_markers(int B, int K, int M, const float* pts, const long long* labels, const float* conf, float* markers,
                     float* valid_f, unsigned char* valid_b, void* stream);
/* get_markers in two halves, for callers that know the inner points only at the selected points:
 * etch_marker_select: labels (B,K) i64, conf (B,K,1) -> sel (B,M,3) i32 = global point rows b*K + i of the label's top-3 confidences in rank
 *   order (confidence descending, then lower index), -1 beyond cnt (B,M) i32 = min(points with the label, 3).
 * etch_markers_from_selected: pts (B,K,3), conf, mag (B,K,1), scale and dir (B*M*3, 3) = the direction of every slot of sel -> markers (B,M,3),
 *   valid (cnt > 0) as float and/or bool bytes: bitwise etch_get_markers of etch_inner_points(pts, dense direction, mag, scale). */
int etch_marker_select(int B, int K, int M, const long long* labels, const float* conf, int* sel, int* cnt, void* stream);
int etch_markers_from_selected(int B, int K, int M, const int* sel, const int* cnt, const float* pts, const float* conf, const float* mag,
                               float scale, const float* dir, float* markers, float* valid_f, unsigned char* valid_b, void* stream);

/* Per-scan status of the aggregated markers (NaN check on the marker weights at the boundary): status (B) i32,
 * bit 0 = a valid marker of the scan is non-finite -- every one of a label's top-3 confidences underflowed in conf**20, so the
 * weighted centre is 0/0 exactly as fit_SMPL.py:52-57 computes it, and the fit of that scan is NaN; bit 1 = no valid marker. */
int etch_marker_status(int B, int M, const float* markers, const float* valid_f, int* status, void* stream);

/* fit_smpl's two Levenberg-Marquardt stages (src/models/fit_SMPL.py:161-249; Theseus LM + smplx LBS upstream).
 * Body model: nj joints, nb shape coefficients -- (24, 10) = SMPL, the reference's model (fit_SMPL.py:100); (55, 20) = an
 * SMPL-X-sized model (BASELINE configs[4]); other sizes return ETCH_EUNSUPPORTED.  P = 9 (nj - 1) pose-feature rows.
 * consts = 7 device pointers {J0 (nj,3) = J_regressor @ v_template, Jd (nj,3,nb) = J_regressor @ shapedirs, parents (nj) i32, and for
 * the M <= 96 marker vertices: v_template rows (M,3), shapedirs rows (M,3,nb), posedirs columns as (M, nj-1, 28): per joint k >= 1 its 9 x 3 block (pose-feature row e, component a at 3 e + a) zero-padded to 28 floats,
 * lbs_weights rows (M,nj)}.
 * markers (B,M,3), valid (B,M) float mask.  Variable vector x (B, 3 nj + nb + 3) = pose | betas | global_orient | transl
 * (fit_SMPL.py:174,225).  Stage 0: it0 iterations, step0, damping damp0, betas[:2] only (:161-200); stage 1: it1, step1, damp1, all
 * betas (:219-249).  x_stage0 / err_trace (B, it0+it1+2) / phase_ticks (B,8) may be NULL. */
int etch_smpl_lm_fit(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, float step0,
                     float damp0, int it1, float step1, float damp1, float* x_out, float* x_stage0, float* err_trace, long long* phase_ticks,
                     void* stream);
/* The same fit with every scan's linearisation split over G workgroups (latency regime: a handful of scans leave most of the chip idle):
 * workgroup g takes the marker chunks g, g + G, ...; the partial tiles of [J | r]^T [J | r] are exchanged through `workspace` once per
 * linearisation and added in a fixed order, all G copies of a scan's state stay bit-identical and solve redundantly.  Results may differ
 * from G = 1 in the last bits of the fp64 normal matrix (a different, still fixed, summation order).  B * G must not exceed the CU count
 * (the workgroups of a scan wait for each other); workspace: etch_smpl_lm_split_workspace_bytes(B, nj, nb, G) bytes, contents arbitrary. */
long etch_smpl_lm_split_workspace_bytes(int B, int nj, int nb, int G);
int etch_smpl_lm_fit_split(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, float step0,
                           float damp0, int it1, float step1, float damp1, float* x_out, float* x_stage0, float* err_trace, long long* phase_ticks,
                           int G, void* workspace, void* stream);
/* The same fit (G workgroups per scan, G = 1: workspace may be NULL) with an optional warm start and an optional diagonal Gaussian prior, each
 * (B, DOF) fp32 in x's layout, NULL = absent.  x_init: the fit starts there instead of at 0; stage 0 evaluates with betas[2:] = 0 as always
 * (they do not move and get no prior) and hands them to stage 1 at their x_init value, so with it0 = 0 x_stage0 = x_init bitwise.
 * prior_mean / prior_weight (w >= 0, the caller's duty): the objective becomes 0.5 |r|^2 + 0.5 sum_i w_i (x_i - mean_i)^2 over the stage's
 * active variables -- added to the normal equations in fp64 after every linearisation, before the damping -- and that sum is what the
 * convergence freeze and err_trace see.  Exactly one of the two non-NULL: ETCH_EINVAL.  All three NULL: etch_smpl_lm_fit_split. */
int etch_smpl_lm_fit_prior(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, float step0,
                           float damp0, int it1, float step1, float damp1, float* x_out, float* x_stage0, float* err_trace, long long* phase_ticks,
                           int G, void* workspace, const float* x_init, const float* prior_mean, const float* prior_weight, void* stream);
/* The same fit under a pose prior on top of whatever etch_smpl_lm_fit_prior takes:
 *     + w_gmm min_k [0.5 d_k^T P_k d_k - log c_k],  d_k = x[:pp_D] - mu_k     (max-mixture GMM, MaxMixturePrior.merged_log_likelihood)
 *     + w_ang sum_t exp(2 s_t x[a_t])                                        (SMPLifyAnglePrior, indices without the global orientation)
 * as Gauss-Newton rows added in fp64 after every linearisation (the component is chosen again each time); err_trace holds the full objective.
 * pp_tables: 5 device pointers {means (pp_G, pp_D), precisions (pp_G, pp_D, pp_D) fp32 SYMMETRIC and positive definite, nll_weights (pp_G) > 0,
 * angle_idx (n_ang) int32 in [0, NPOSE), angle_sign (n_ang) fp32} -- values are the caller's duty.  pp_G = 0 or n_ang = 0 leaves that part (and
 * its tables) out.  ETCH_EINVAL: pp_G == 0 && n_ang == 0, pp_G > 16, n_ang > 8, pp_D outside [1, NPOSE], a NULL table that is needed. */
int etch_smpl_lm_fit_pose_prior(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, float step0,
                                float damp0, int it1, float step1, float damp1, float* x_out, float* x_stage0, float* err_trace, long long* phase_ticks,
                                int G, void* workspace, const float* x_init, const float* prior_mean, const float* prior_weight,
                                const void* const* pp_tables, int pp_G, int pp_D, int n_ang, float w_gmm, float w_ang, void* stream);
/* The max-mixture bracket alone, as the fits evaluate it (the same device function): pose (B, D) fp32 -> value (B) fp64 = min_k [...],
 * component (B) int32 = argmin (ties: lowest index), grad (B, D) fp64 = P_k* d_k*.  tables: {means, precisions, nll_weights}; 1 <= G <= 16,
 * 1 <= D <= 162. */
int etch_pose_prior_eval(int B, const void* const* tables, int G, int D, const float* pose, double* value, int* component, double* grad, void* stream);
/* Failure path of the split fit.  A workgroup that waits longer than its spin limit for its partners (they were not co-resident: another kernel, a CU
 * partition) flags the scan and every workgroup of the scan abandons the fit: the scan's x_out / x_stage0 / err_trace rows are NaN -- never a fit of
 * partial sums -- and the flag stays set in the workspace.  etch_smpl_lm_split_failed counts the flagged scans (synchronises the stream).
 * etch_smpl_lm_debug is the test hook: spin limit in polls (0 = default, ~10 s) and a group index that returns at launch (-1 = none). */
int etch_smpl_lm_split_failed(int B, const void* workspace, int* n_failed, void* stream);
int etch_smpl_lm_debug(unsigned spin_limit, int drop_group);
/* LDS bytes one scan's fit holds for its whole duration (one workgroup per scan); ETCH_EUNSUPPORTED for unknown (nj, nb). */
int etch_smpl_lm_workspace_bytes(int nj, int nb);

/* fit_smpl of the first-order variant (src/models/fit_SMPL_Adam.py:68-225): torch.optim.Adam semantics (bias-corrected, betas / eps as
 * given; the reference uses the defaults 0.9 / 0.999 / 1e-8 and lr 1e-2) on the batch-mean squared marker error over the valid marker
 * coordinates; it0 steps on betas[:2] (:104-160), then it1 steps with a fresh optimizer state on all betas (:166-218).  Same consts /
 * markers / valid / x layout as etch_smpl_lm_fit.  x_last (optional) = the parameters of the last forward pass (before the final
 * step): the reference builds its output meshes from that forward.  loss_trace (B, it0+it1, optional): this scan's share of L. */
int etch_smpl_adam_fit(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, int it1,
                       float lr, float beta1, float beta2, float eps, float* x_out, float* x_last, float* loss_trace, void* stream);

/* etch_smpl_adam_fit with the two optional loss terms of the reference's fitter (fit_SMPL_Adam.py:141-153, 202-214):
 *     + w_pp sum_b min_k [0.5 d^T P_k d - log c_k] on pose[:pp_D]  (pp_tables: {means, precisions, nll_weights}; pp_G = 0: absent)
 *     + w_ms mean(betas_active^2) over the batch (2 coefficients in stage 0, all in stage 1)
 * and loss_trace rows that still sum to the batch loss.  ETCH_EINVAL: neither term (pp_G == 0 && w_ms == 0), pp_G > 16, pp_D outside
 * [1, NPOSE], a NULL table. */
int etch_smpl_adam_fit_prior(int B, int M, int nj, int nb, const void* const* consts, const float* markers, const float* valid, int it0, int it1,
                             float lr, float beta1, float beta2, float eps, float* x_out, float* x_last, float* loss_trace,
                             const void* const* pp_tables, int pp_G, int pp_D, float w_pp, float w_ms, void* stream);

/* Diagnostics of the LM kernel (tests): ONE linearisation at a caller-given x (B,DOF) with nb_active betas -> residual
 * (B,3M) = mask * (target - markers(x)) (fit_SMPL.py:127-131), the analytic Jacobian d resid / d x (B,3M,DOF) the fit uses in place
 * of the reference's autograd Jacobian (AutoDiffCostFunction, fit_SMPL.py:176-183, 227-234), and (optional) the normal equations
 * as the fit accumulates them on the fp64 matrix cores: (B, DOF+1, DOF+1) fp64, lower triangle = J^T J, row DOF = -J^T r. */
int etch_smpl_lm_linearize(int B, int M, int nj, int nb_model, int nb_active, const void* const* consts, const float* x, const float* markers,
                           const float* valid, float* resid, float* jac, double* normal, void* stream);

/* batch_rodrigues as the fit evaluates it (in-tree copy src/data_utils/GT_dataloader_mixed.py:29-64, angle = |theta + 1e-8|):
 * theta (n,3) -> R (n,9) fp64 and dR/dtheta_q (n,3,9). */
int etch_rodrigues(int n, const float* theta, double* R, float* dR, void* stream);

/* Final smpl_model(...) (fit_SMPL.py:258-259, smplx.SMPL.forward upstream): x (B, 3 nj + nb + 3) -> verts (B,V,3), joints
 * (B, nj + n_extra, 3) = regressed joints + n_extra vertex-picked joints.  consts = 8 device pointers {v_template (V,3), shapedirs
 * (V,3,nb), posedirs (9 (nj-1), V*3), lbs_weights (V,nj), J0, Jd, parents, extra_vids (n_extra) i32}.  nj <= 55, nb <= 20. */
int etch_smpl_lbs(int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* x, float* verts, float* joints, void* stream);

/* ---- chamfer refinement of the fit against the scan (scripts/experiment_scripts/chamfer_refine.py:fit_cham) --------------------- */

/* Exact brute-force nearest neighbours between X (B,N,3) and Y (B,V,3), both directions in one pass over the pair tiles.
 * x_len / y_len (B) int32 or NULL: points at or past a scan's length are never chosen and change nothing.  Outputs: idx_xy (B,N) int32 =
 * the Y index nearest to each X point, d_xy (B,N) its squared distance; idx_yx / d_yx (B,V) the same towards X.  The distance is the
 * bit-defined fp32 ((dx*dx)+(dy*dy))+(dz*dz) of the returned pair; among exactly equal distances the LOWEST index wins.  Padding rows
 * get index -1 and distance 0.  workspace: B (N + V) * 8 bytes, contents arbitrary. */
int etch_nn_bidir(int B, int N, int V, const float* X, const float* Y, const int* x_len, const int* y_len, void* workspace, int* idx_xy, float* d_xy,
                  int* idx_yx, float* d_yx, void* stream);
/* Gradient of L = sum_b [w_xy[b] sum_i d_xy(b,i) + w_yx[b] sum_j d_yx(b,j)] with the neighbours of etch_nn_bidir held fixed:
 * gx (B,N,3), gy (B,V,3) (either may be NULL; padding rows get 0).  w_xy / w_yx (B) or NULL (direction absent).  Deterministic: the
 * neighbour-side scatter sums fixed-point differences with integer atomics.  workspace: B (N + V) * 24 bytes, contents arbitrary. */
int etch_chamfer_grad(int B, int N, int V, const float* X, const float* Y, const int* x_len, const int* y_len, const int* idx_xy, const int* idx_yx,
                      const float* w_xy, const float* w_yx, void* workspace, float* gx, float* gy, void* stream);
/* Workspace bytes of etch_smpl_chamfer_refine (N scan points) and of etch_smpl_lbs_vjp (N = 0); (nj, nb) in {(24, 10), (55, 20)}. */
int etch_smpl_chamfer_refine_workspace(int B, int N, int V, int nj, int nb, int n_extra, long long* bytes);
/* Reverse mode of verts = (LBS(pose, beta) + trans) * scale over the full mesh.  params (B, P = 3 nj + nb + 4) = pose[3 nj] (global
 * orient first) | beta[nb] | trans[3] | scale; g (B,V,3) = dL/dverts -> grad (B,P) = dL/dparams.  consts as etch_smpl_lbs. */
int etch_smpl_lbs_vjp(int B, int V, int nj, int nb, int n_extra, const void* const* consts, const float* params, const float* g, void* workspace, float* grad,
                      void* stream);
/* fit_cham: `iters` torch.optim.Adam steps (beta1, beta2, eps; no weight decay) on params (B,P, updated in place) of the per-scan loss
 * data + 1e-8 prior(pose[3:]) + 0.2 mean(beta^2), data = sqrt(S1) + sqrt(S2) (bidir 0), sqrt(S1) (1: scan -> body only) or sqrt(S2)
 * (-1: body -> scan only), S1 = sum over the scan (B,N,3; scan_len or NULL) of the squared distance to the nearest vertex, S2 = sum over
 * the vertices of the squared distance to the nearest scan point.  Step i runs at lr for i = 0 and lr (iters - i + 1) / iters after.
 * prior: NULL (n_gauss 0) or {means (G,69), precisions (G,69,69), nll_weights (G)} of the max-mixture GMM, SMPL (nj 24) only.
 * Outputs: verts (B,V,3) of the final params, joints (B, nj + n_extra, 3) of the final params without trans and scale, loss_last (B) =
 * the loss of the last forward, loss_trace (B, iters) or NULL.  Everything is queued on `stream` without a host wait (capturable). */
int etch_smpl_chamfer_refine(int B, int N, int V, int nj, int nb, int n_extra, const void* const* consts, const float* scan, const int* scan_len,
                             const void* const* prior, int n_gauss, int bidir, int iters, float lr, float beta1, float beta2, float eps, float* params,
                             float* verts, float* joints, float* loss_trace, float* loss_last, void* workspace, void* stream);

/* ---- dense surface refinement: the body surface against all predicted inner points (csrc/surface_fit.hip) ------------- */

/* Workspace bytes of etch_point_mesh_closest. */
int etch_point_mesh_closest_workspace(int B, int N, long long* bytes);
/* Exact closest point of mesh b (verts (B,V,3) fp32, faces (F,3) int32 shared by the batch) to each point of points (B,N,3) fp32; n_len (B)
 * int32 or NULL: points at or past a scan's length are padding.  Ericson's region test in fp32 with the operation order of
 * csrc/closest_tri.h, every (point, face) pair, nothing approximate.  Outputs: face (B,N) int32, bary (B,N,3), d2 (B,N) =
 * ((ex*ex)+(ey*ey))+(ez*ez) of e = p - q.  The smallest d2 wins, equal d2 -> the lowest face, a NaN d2 (degenerate face) never wins and
 * neither does a face with a vertex index outside [0, V).  Padding rows (and a point no face could be chosen for): face -1, bary 0, d2 0. */
int etch_point_mesh_closest(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, void* workspace, int* face,
                            float* bary, float* d2, void* stream);
/* Workspace bytes of etch_point_mesh_energy_grad. */
int etch_point_mesh_energy_grad_workspace(int B, int V, long long* bytes);
/* With the correspondences of etch_point_mesh_closest held fixed, m_i = [d2_i <= trunc^2] on the fp32 value (trunc < 0: no mask) and
 * w_i = weights (B,N) or NULL (1): terms (B,2) fp64 = {S1 = sum_i w_i m_i d2_i, S0 = sum_i w_i m_i}, fixed-order sums; g (B,V,3) or NULL =
 * d/dverts of  coef_b w_dense S1 / S0 (normalize 1; S0 = 0: the term is 0) or coef_b w_dense S1 (normalize 0)
 *            + w_marker mean over the valid markers' coordinates of (v_vid(m) - t_m)^2   (M > 0: marker_vids (M) int32, markers (B,M,3),
 *              marker_valid (B,M) fp32, > 0 = valid; no valid marker: the term is 0),
 * coef (B) or NULL (1); gp (B,N,3) or NULL = the dense term's gradient w.r.t. the points.  The per-vertex sums are 2^-40 fixed-point
 * differences added with 64-bit integer atomics: exact, independent of order; no floating-point atomics. */
int etch_point_mesh_energy_grad(int B, int N, int V, int F, const float* points, const int* n_len, const float* verts, const int* faces, const int* face,
                                const float* bary, const float* d2, const float* weights, float trunc, const float* coef, float w_dense, int normalize, int M,
                                const int* marker_vids, const float* markers, const float* marker_valid, float w_marker, void* workspace, double* terms,
                                float* g, float* gp, void* stream);
/* Workspace bytes of etch_smpl_surface_refine; (nj, nb) in {(24, 10), (55, 20)}. */
int etch_smpl_surface_refine_workspace(int B, int N, int V, int nj, int nb, int n_extra, long long* bytes);
/* `iters` torch.optim.Adam steps (beta1, beta2, eps; fit_cham's schedule: step i at lr for i = 0 and lr (iters - i + 1) / iters after) on
 * params (B, P = 3 nj + nb + 4, updated in place) of the per-scan loss
 *   w_dense S1 / S0 + w_marker mean_valid (v_vid(m) - t_m)^2 + w_beta mean(beta^2) + w_prior min_k [0.5 d^T P_k d - log c_k] (pose[3:]),
 * S1, S0 as in etch_point_mesh_energy_grad for the surface of verts = (LBS(pose, beta) + trans) * scale and points (B,N,3) (n_len, weights
 * or NULL); the correspondences are recomputed at every iteration and held fixed inside the gradient.  optimize_scale 0: scale keeps its
 * initial value.  prior: NULL (n_gauss 0) or {means (G,69), precisions (G,69,69), nll_weights (G)}, SMPL (nj 24) only.  Outputs: verts
 * (B,V,3) and joints (B, nj + n_extra, 3; without trans and scale) of the final params, loss_last (B) = the loss of the last forward,
 * loss_trace (B, iters, 4) = the four weighted terms at the iterate before each step, or NULL.  Everything is queued on `stream` without a
 * host wait (capturable).  consts as etch_smpl_lbs. */
int etch_smpl_surface_refine(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces, const float* points,
                             const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers, const float* marker_valid,
                             const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2, float eps, float w_dense, float w_marker,
                             float w_beta, float w_prior, float trunc, int optimize_scale, float* params, float* verts, float* joints, float* loss_trace,
                             float* loss_last, void* workspace, void* stream);

/* ---- containment: keep the fitted body inside the scan (csrc/containment.hip) ------------------------------------------- */

/* A ragged batch of B scan meshes is given as mesh_io.pack_meshes lays it out: verts (sum V,3) fp32, already in the frame of the queries,
 * faces (sum F,3) int32 local to their scan, vert_offsets and face_offsets (B+1) int32 in device memory, starting at 0 and not decreasing;
 * max_faces >= every scan's face count sizes the launches (a scan's faces past it are not visited).  Nothing is read on the host. */

/* Workspace bytes of etch_mesh_winding_number. */
int etch_mesh_winding_number_workspace(int B, int Q, int max_faces, long long* bytes);
/* Generalised winding number w (B,Q) fp32 of scan b at queries (B,Q,3) fp32; q_len (B) int32 or NULL: queries at or past a scan's length
 * are padding and get 0.  Per (query q, face (a, b, c)), with A = a - q, B = b - q, C = c - q, la, lb, lc their norms, every operation fp32
 * in the order of csrc/containment.hip:  Omega / 2 = atan2f(A . (B x C), la lb lc + (A . B) lc + (B . C) la + (C . A) lb)  (van Oosterom and
 * Strackee).  A thread adds the terms of one 1024-face chunk in ascending face order in fp32; the chunks are added in ascending order in
 * fp64, multiplied by 1 / (2 pi) and rounded once: w = 1 inside a closed outward-oriented surface, 0 outside, -1 inside a reversed one.
 * A face with a vertex index outside [0, V_b) contributes 0; a non-finite vertex or query gives NaN.  No atomics: scan b in a batch is
 * bitwise scan b alone, and two runs are bitwise equal. */
int etch_mesh_winding_number(int B, int Q, int max_faces, const float* verts, const int* faces, const int* vert_offsets, const int* face_offsets,
                             const float* queries, const int* q_len, void* workspace, float* w, void* stream);
/* Workspace bytes of etch_ragged_mesh_closest. */
int etch_ragged_mesh_closest_workspace(int B, int N, long long* bytes);
/* etch_point_mesh_closest for the ragged batch: the exact closest point of scan b's mesh to each point of points (B,N,3) fp32 (n_len (B) or
 * NULL).  The same region test (csrc/closest_tri.h), the same key merge and the same rules: the smallest d2 wins, equal d2 -> the lowest
 * face, a NaN d2 never wins and neither does a face with a vertex index outside [0, V_b).  Outputs: face (B,N) int32 local to the scan, bary
 * (B,N,3), d2 (B,N); padding rows (and a point no face could be chosen for): face -1, bary 0, d2 0. */
int etch_ragged_mesh_closest(int B, int N, int max_faces, const float* verts, const int* faces, const int* vert_offsets, const int* face_offsets,
                             const float* points, const int* n_len, void* workspace, int* face, float* bary, float* d2, void* stream);
/* Workspace bytes of etch_containment_energy_grad. */
int etch_containment_energy_grad_workspace(int B, int V, long long* bytes);
/* The containment term of body_verts (B,V,3) fp32 against the scans, from w (B,V) = the winding numbers of the vertices and (face, bary, d2)
 * (B,V) = their correspondences on the scan (etch_ragged_mesh_closest):  o_v = [ |w_v| < 0.5 ] (a NaN w is not outside; neither is a vertex
 * whose face is -1, out of range, or has a vertex index out of range), c_v = sum_k bary_k s_k the closest point.  Outputs: terms (B,2) fp64 =
 * {sum_v o_v d2_v, sum_v o_v}, fixed order; g (B,V,3) or NULL, to which coef_b w_contain (2 / V) o_v (v - c_v) is ADDED (coef (B) or NULL =
 * 1): the gradient of coef_b w_contain (sum_v o_v d2_v) / V with the correspondences held.  Each vertex receives one term, computed in fp64
 * and added with one rounding: no scatter, no atomics; a vertex that is not outside keeps its bits, and so does every vertex when
 * coef_b w_contain is 0. */
int etch_containment_energy_grad(int B, int V, const float* body_verts, const float* verts, const int* faces, const int* vert_offsets,
                                 const int* face_offsets, const float* w, const int* face, const float* bary, const float* d2, const float* coef,
                                 float w_contain, void* workspace, double* terms, float* g, void* stream);
/* Workspace bytes of etch_smpl_surface_refine_contain. */
int etch_smpl_surface_refine_contain_workspace(int B, int N, int V, int nj, int nb, int n_extra, int max_faces, long long* bytes);
/* etch_smpl_surface_refine with a fifth term of the loss, w_contain (sum_v o_v |v - c_v|^2) / V over the body's V vertices, against the scan
 * meshes (max_scan_faces, scan_verts, scan_faces, scan_vert_offsets, scan_face_offsets: the ragged batch above, in the frame of the body).
 * At iterations 0, K, 2K, ... (K = contain_every >= 1) the winding numbers and the scan correspondences of the current vertices are
 * recomputed, every vertex against every face; in between o_v and c_v -- the target POINT, not the face -- are held, and |v - c_v|^2 is
 * taken in fp64 at the current vertices.  The term is normalised by V, not by the count of outside vertices, so it is zero and flat where a
 * vertex crosses the surface.  loss_trace is (B, iters, 5) or NULL, the fifth column this term.  With w_contain = 0 the parameters and the
 * first four trace columns are bitwise those of etch_smpl_surface_refine.  Everything is queued on `stream` without a host wait. */
int etch_smpl_surface_refine_contain(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces, const float* points,
                                     const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers, const float* marker_valid,
                                     const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2, float eps, float w_dense,
                                     float w_marker, float w_beta, float w_prior, float trunc, int optimize_scale, int max_scan_faces, const float* scan_verts,
                                     const int* scan_faces, const int* scan_vert_offsets, const int* scan_face_offsets, float w_contain, int contain_every,
                                     float* params, float* verts, float* joints, float* loss_trace, float* loss_last, void* workspace, void* stream);

/* ---- SMPL+D registration and re-posing (csrc/register.hip) ------------------------------------------------------------ */

/* Skinning frames of params (B, 3 nj + nb + 4) = pose (global orient first) | beta | trans | scale: with r_v the rest vertex after shape and
 * pose blend shapes and A_j the joint transforms (rest joint removed, no trans, no scale), base (B,V,3) = (sum_j W_vj A_j [r_v; 1] + trans)
 * scale, R (B,V,9) = scale sum_j W_vj A_j^R (row-major 3 x 3), A (B,nj,12) (row-major 3 x 4).  consts: the first 7 tables of etch_smpl_lbs. */
int etch_smpl_skin_frames(int B, int V, int nj, int nb, const void* const* consts, const float* params, float* base, float* R, float* A, void* stream);
/* verts (B,V,3) = base + R D, D (B,V,3) the per-vertex offsets in the rest pose. */
int etch_smpld_apply(int B, int V, const float* base, const float* R, const float* D, float* verts, void* stream);
/* Workspace bytes of etch_smpld_energy_grad and etch_smpld_register. */
int etch_smpld_register_workspace(int B, int N, int V, long long* bytes);
/* One evaluation of the registration energy of every scan b (n_b = scan_len[b] or N points x, y = base + R D, a / c / d the neighbours and
 * distances of etch_nn_bidir(scan, y)):
 *   w_s2m / n_b sum_i d(x_i, y_a(i)) + w_m2s / V sum_v m_v d(y_v, x_c(v)) + lambda_s / n_edges sum_(u,v) |D_u - D_v|^2 + lambda_m / V sum_v |D_v|^2,
 * m_v = 1, or with trunc >= 0, [d(y_v, x_c(v)) <= trunc^2] on the fp32 distance (trunc < 0: no mask).  The edges are given as the
 * neighbour lists nbr_idx[nbr_ptr[v] .. nbr_ptr[v+1]) (nbr_ptr (V+1), every edge in both lists, n_edges of them; shared by the batch).
 * Outputs: terms (B,4) in the order above, grad (B,V,3) = d energy / dD with neighbours and masks held fixed, verts (B,V,3), idx_xy (B,N),
 * idx_yx (B,V).  Sums are fp64 in a fixed order; no floating-point atomics. */
int etch_smpld_energy_grad(int B, int N, int V, const float* base, const float* R, const float* D, const float* scan, const int* scan_len, const int* nbr_ptr,
                           const int* nbr_idx, int n_edges, float w_s2m, float w_m2s, float lambda_s, float lambda_m, float trunc, void* workspace, float* terms,
                           float* grad, float* verts, int* idx_xy, int* idx_yx, void* stream);
/* `iters` torch.optim.Adam steps (betas 0.9 / 0.999, eps 1e-8, constant lr, fp32 moments from zero) on D (B,V,3, updated in place) of the
 * energy above; step i uses lambda_s[i] (a HOST array of iters floats, read during the call) and its gradient is taken entirely at the
 * iterate before it.  Outputs: verts (B,V,3) and energy (B,4) of the final D (evaluated with lambda_s[iters-1]), trace (B,iters,4) = the
 * terms at the iterate before each step, or NULL.  Everything is queued on `stream` without a host wait (capturable). */
int etch_smpld_register(int B, int N, int V, const float* base, const float* R, const float* scan, const int* scan_len, const int* nbr_ptr, const int* nbr_idx,
                        int n_edges, int iters, const float* lambda_s, float lambda_m, float w_s2m, float w_m2s, float trunc, float lr, float* D, float* verts,
                        float* energy, float* trace, void* workspace, void* stream);
/* Carry P points (fp64) bound to a skinned surface (face (P) int32 into faces (F,3), bary (P,3)) from one pose to another: w~ = sum_k
 * bary_k W[faces[f,k]] (W (V,nj)), T = sum_j w~_j A_j, T' = sum_j w~_j A_new_j, out = (T' T^-1 (x / scale - trans) + trans') scale', with
 * trans_scale / trans_scale_new = 4 device floats each (trans | scale).  |det T^R| < 1e-10: T is the identity.  A point whose face or
 * vertex index is out of range comes back as NaN. */
int etch_skin_carry(int P, int F, int V, int nj, const double* points, const int* face, const double* bary, const int* faces, const float* W, const float* A,
                    const float* A_new, const float* trans_scale, const float* trans_scale_new, double* out, void* stream);

/* ---- tightness supervision: info points and vector targets (scripts/generate_infopoints.py, GT_dataloader.py:95-122) ------------- */

/* Workspace bytes of etch_ray_first_hit (R rays) / etch_closest_point_on_mesh (P points) against F faces. */
int etch_ray_first_hit_workspace(int R, int F, long long* bytes);
/* First hit of R rays (origins, dirs (R,3) fp64) on a mesh (verts (V,3) fp64, faces (F,3) int32, every index in [0, V)): Moller-Trumbore in
 * fp64 with the operation order of csrc/raycast.hip; a hit needs det != 0, u >= 0, v >= 0, u + v <= 1, 0 < t < t_max.  excl_face (R) int32
 * or NULL: a face each ray skips (-1 = none); t_max (R) fp64 or NULL (+inf).  Outputs: face (R) int32 (-1 = miss), t (R) (+inf on a miss),
 * bary (R,3) = (1 - u - v, u, v) (0 on a miss), loc (R,3) = o + t d or NULL.  The smallest t wins, equal t -> the lowest face. */
int etch_ray_first_hit(int R, int F, const double* origins, const double* dirs, const double* verts, const int* faces, const int* excl_face,
                       const double* t_max, void* workspace, int* face, double* t, double* bary, double* loc, void* stream);
int etch_closest_point_on_mesh_workspace(int P, int F, long long* bytes);
/* Closest point on the mesh of P points (P,3) fp64: Ericson's region test (Real-Time Collision Detection 5.1.5) with the operation order of
 * csrc/raycast.hip.  Outputs: face (P) int32, bary (P,3), closest (P,3), d2 (P) fp64; the smallest d2 wins, equal d2 -> the lowest face. */
int etch_closest_point_on_mesh(int P, int F, const double* points, const double* verts, const int* faces, void* workspace, int* face, double* bary,
                               double* closest, double* d2, void* stream);
/* trimesh's angle-weighted vertex normals: per vertex the sum of (unit face normal x corner angle) over csr_idx[csr_ptr[i] .. csr_ptr[i+1])
 * (entries 3 f + corner, in the order given), normalised.  csr_ptr (V+1), csr_idx (3F) int32; workspace F * 48 bytes; normals (V,3) fp64. */
int etch_vertex_normals(int V, int F, const double* verts, const int* faces, const int* csr_ptr, const int* csr_idx, void* workspace, double* normals,
                        void* stream);
/* trimesh 4.x points.remove_close on C points (C,3) fp64: a close pair is i < j with squared distance <= r2; degree (C) int32 = close pairs
 * containing each point; removed (C) int32 = 1 where the point is dropped (each pair drops its endpoint of higher degree, i on a tie). */
int etch_remove_close(int C, const double* points, double r2, int* degree, int* removed, void* stream);

/* ---- geodesic labels and confidences (GT_dataloader.py:124-145, pp3d.MeshHeatMethodDistanceSolver) -------------- */

/* Workspace bytes of etch_geodesic_heat for B bodies of V vertices, F faces, E edges and S sources. */
int etch_geodesic_workspace(int B, int V, int F, int E, int S, long long* bytes);
/* Heat-method distances from S source vertices on B bodies (verts (B,V,3) fp64) sharing one manifold topology stored by edges (fv0, fe0, fs0
 * (F,3): corners, the edge opposite each corner, the slot of that edge the face holds; ef0 (E,2): faces, -1 = boundary; ev0 (E,2) endpoints),
 * all int32 and in range.  intrinsic_delaunay != 0: mollify (relative mollify_eps) and flip while cot a + cot b < -delaunay_tol, at most
 * max_rounds rounds (ETCH_EUNSUPPORTED past them; waits on `stream`).  t = t_coef * (mean input edge length)^2.  Heat: Jacobi sweeps (damped
 * by heat_omega when it is not 1) until no vertex changes by more than heat_tol of its value (heat_cap sweeps at most); Poisson: Jacobi-PCG until |r| <= cg_rtol |b| (cg_cap at most).
 * Outputs: dist (B,S,V) fp64 with dist[source] = 0; dmin (B,V) / label (B,V) int32 = min / first argmin over the sources, or both NULL;
 * iters (B,S,2) int32 = heat sweeps, CG iterations (-1 where the cap was hit); flips (B) HOST int32.  Optional (NULL = not written): out_ev
 * (B,E,2) int32 and out_el (B,E) fp64 = the final triangulation's edges and lengths, out_ecot (B,E,2) the cotans opposite each edge,
 * out_area (B,F) face areas.  S = 0 builds the triangulation and operators only. */
int etch_geodesic_heat(int B, int V, int F, int E, int S, const double* verts, const int* fv0, const int* fe0, const int* fs0, const int* ef0,
                       const int* ev0, const int* sources, double t_coef, int intrinsic_delaunay, double mollify_eps, double delaunay_tol,
                       int max_rounds, double heat_tol, double heat_omega, int heat_cap, double cg_rtol, int cg_cap, void* workspace, double* dist, double* dmin,
                       int* label, int* iters, int* flips, int* out_ev, double* out_el, double* out_ecot, double* out_area, void* stream);

/* ---- the training step (train.py:81-125) -------------------------------------------------------------------------- */

/* Bits of the status word etch_train_losses writes and etch_guarded_adam_step reads. */
#define ETCH_TRAIN_STATUS_NAN 1          /* the total loss is NaN: the optimizer step that follows changes nothing */
#define ETCH_TRAIN_STATUS_BAD_LABEL 2    /* a label outside [0, M) or a gather index outside [0, N): that row contributed nothing */
/* The four losses of train.py:81-101 and the gradient of their sum, one launch.  Head outputs direction (B,K,3), magnitude (B,K,1), confidences
 * (B,K,1), part_labels (B,K,M) logits -- any may be NULL (absent: loss 0, no gradient; at least one given); targets t_vectors (B,N,3),
 * t_confidences (B,N,1), t_labels (B,N) int64, read at index (B,K) int64 = selected_indexs[:, :, 0].
 *   losses[0] = direction_w mean(1 - cos(t_vectors_k, direction)), each norm clamped at 1e-8 (F.cosine_similarity)
 *   losses[1] = magnitude_w mean((|t_vectors_k| scale_magnitude - magnitude)^2)       losses[2] = confidence_w mean((confidences - t_confidences_k)^2)
 *   losses[3] = part_label_w mean(logsumexp(row) - row[label])  (row maximum subtracted)    losses[4] = their sum
 * g_* (shapes of the heads): d losses[4] / d head.  fp32 per element, sums in fp64 in a fixed order: bitwise reproducible.  status[0] = the
 * ETCH_TRAIN_STATUS_* bits of this call.  workspace: etch_train_losses_workspace_doubles() doubles; counter: one unsigned, zero before the first
 * call and left zero (as etch_bn_train_forward's). */
int etch_train_losses_workspace_doubles(void);
int etch_train_losses(int B, int K, int N, int M, const float* direction, const float* magnitude, const float* confidences, const float* part_labels,
                      const float* t_vectors, const float* t_confidences, const long long* t_labels, const long long* index, float direction_w,
                      float magnitude_w, float confidence_w, float part_label_w, float scale_magnitude, double* workspace, unsigned* counter,
                      float* losses, int* status, float* g_direction, float* g_magnitude, float* g_confidences, float* g_part_labels, void* stream);

/* torch.optim.Adam (weight_decay 0, no amsgrad) over T fp32 tensors with train.py:111-125's guards, 2 launches whatever T is.  The tensors are cut
 * into C chunks of etch_guarded_adam_chunk() elements (a tensor's last chunk shorter): chunk_tensor (C) = the tensor of each chunk, first_chunk
 * (T+1) = the first chunk of each tensor, numel (T).  pmv (3,T) = device addresses of parameter, exp_avg, exp_avg_sq; grads (T) = address of each
 * gradient, 0 = none (the tensor is skipped: no moment update, no step).  A gradient that holds a NaN, or +inf and -inf, is taken as zero
 * (`param.grad.sum().isnan()`); counters[0] counts such tensors.  steps (T) fp32: the per-tensor step counts, advanced here.  status (may be NULL):
 * with ETCH_TRAIN_STATUS_NAN set nothing is changed and counters[1] advances; ETCH_TRAIN_STATUS_BAD_LABEL is ORed into counters[2].
 * chunkflags: C unsigned of scratch.  16-byte accesses where parameter, gradient and moments are 16-byte aligned, scalar otherwise. */
int etch_guarded_adam_chunk(void);
int etch_guarded_adam_step(int T, int C, const int* chunk_tensor, const int* first_chunk, const long long* numel, const unsigned long long* pmv,
                           const unsigned long long* grads, const int* status, float* steps, unsigned* chunkflags, double lr, double beta1,
                           double beta2, double eps, int* counters, void* stream);

/* Accumulated and data-parallel steps: one contribution's gradients into a flat fp32 buffer, one launch over the chunk table of
 * etch_guarded_adam_step.  Tensor t occupies flat[offsets[t], offsets[t] + numel[t]); offsets are multiples of 4 elements, so 16-byte accesses hold on
 * a 16-byte aligned buffer.  mode 0: flat = g * scale (zeros for a gradient address of 0); mode 1: flat += g * scale (nothing for address 0).  Product
 * and sum are rounded separately (no FMA); non-finite values pass through.  16-byte accesses where source and destination are 16-byte aligned, scalar
 * otherwise.  Nothing between the slots is written.  tail_offset >= 0: the etch_grad_tail_floats() floats there receive (mode 0) or are advanced by
 * (mode 1) losses[0..5) * scale, 1 if status[0] has ETCH_TRAIN_STATUS_NAN, 1 if it has ETCH_TRAIN_STATUS_BAD_LABEL, 0 (losses, status may be NULL:
 * zeros); tail_offset < 0: no tail. */
int etch_grad_tail_floats(void);
int etch_grad_pack(int T, int C, const int* chunk_tensor, const int* first_chunk, const long long* numel, const unsigned long long* grads,
                   const long long* offsets, float* flat, float scale, int mode, const float* losses, const int* status, long long tail_offset,
                   void* stream);
/* The (summed) tail back into what the step reads: losses (5) = tail[0..5); status[0] = ETCH_TRAIN_STATUS_NAN if tail[5] != 0, | ETCH_TRAIN_STATUS_BAD_LABEL
 * if tail[6] != 0. */
int etch_grad_unpack_tail(const float* tail, float* losses, int* status, void* stream);

/* ---- scan ingestion: OBJ reader / writer (host) and the surface sampler (inference_demo.py:19-39, eval.py) ------- */

/* Status codes of the etch_obj_* calls beyond 0 and -1.  The calls are host code on HOST buffers, keep no state and may run concurrently. */
#define ETCH_OBJ_EVERTEX (-3)            /* a "v" line with fewer than three coordinates, or a coordinate that is no number */
#define ETCH_OBJ_EFACE (-4)              /* an "f" token that is no integer, or an integer outside int64 */
#define ETCH_OBJ_EINDEX (-5)             /* a face index outside [1, nv] in the file (0, negative = relative, too large) */
#define ETCH_OBJ_ECOUNT (-6)             /* the buffer does not hold the nv vertices and nf triangles given */
#define ETCH_OBJ_ESPACE (-7)             /* etch_obj_format: cap is too small; *written = the bytes needed */
/* Vertices ("v " lines) and triangles ("f " lines, polygons fanned) in an OBJ text of len bytes.  Content errors are left to etch_obj_parse. */
int etch_obj_count(const char* data, long long len, long long* nv, long long* nf);
/* Fills v (nv,3) fp64 and f (nf,3) int64 (0-based) for the counts etch_obj_count gave: what etch_amd.inference_demo.load_obj returns, with the
 * rules of csrc/obj_io.h, and every index checked against [0, nv).  On an error *err_line = the 1-based line and v, f hold no result. */
int etch_obj_parse(const char* data, long long len, long long nv, long long nf, double* v, long long* f, long long* err_line);
/* The text Mesh.export writes ("v %.8f %.8f %.8f\n", "f %d %d %d\n" 1-based) into out[0, cap); *written = its length, also when cap is too small. */
int etch_obj_format(const double* v, long long nv, const long long* f, long long nf, char* out, long long cap, long long* written);

/* Bits of the per-scan status word of etch_sample_surface. */
#define ETCH_SAMPLE_STATUS_AREA 1        /* the scan's total area is zero or not finite: nothing was sampled */
#define ETCH_SAMPLE_STATUS_VERTEX 2      /* a vertex of the scan is not finite */
/* Bounding-box mid-point (min + max) / 2 per scan (preprocess_scan): verts fp64 (sum of scans, 3) concatenated, vert_offsets (B+1) int32 ->
 * center (B,3) fp64.  Of equal zeros the minimum is -0 and the maximum +0, so the bits do not depend on the order of the reduction. */
int etch_bbox_center(int B, const double* verts, const int* vert_offsets, double* center, void* stream);
/* Workspace bytes of etch_sample_surface for B scans of total_faces faces together. */
int etch_sample_surface_workspace(int B, int total_faces, long long* bytes);
/* N area-weighted surface samples on each of B meshes (trimesh.sample.sample_surface's distribution), bit-defined:
 * verts fp64 and faces (.,3) int32 concatenated, face indices local to their scan; vert_offsets, face_offsets (B+1) int32 with face_offsets[B] =
 * total_faces; max_faces = the largest face count of a scan; keys (B) uint64 = the Philox4x32-10 key of each scan, sample i uses counter (i,0,0,0); center (B,3) fp64
 * subtracted from the corners, or NULL.  Outputs: points32 (B,N,3) fp32, points64 (B,N,3) fp64 or NULL, face (B,N) int32, status (B) int32 =
 * ETCH_SAMPLE_STATUS_* bits (a scan with a bit set gets no samples).  Indices are clamped into their scan; validate them before the call.
 * Preconditions the call cannot check (the offsets are device memory): both offset arrays start at 0 and do not decrease, face_offsets[B] ==
 * total_faces, and max_faces >= every scan's face count -- with a smaller max_faces the faces past it get no cumulative area and no status bit. */
int etch_sample_surface(int B, int N, int total_faces, int max_faces, const double* verts, const int* faces, const int* vert_offsets,
                        const int* face_offsets, const unsigned long long* keys, const double* center, void* workspace, float* points32,
                        double* points64, int* face, int* status, void* stream);

/* ---- single-view scans: depth rasteriser, back-projection, stratified pick (csrc/depth_render.hip) --------------- */

/* Bits of the per-view status words of etch_render_depth and etch_depth_pick. */
#define ETCH_DEPTH_STATUS_VERTEX 1       /* a face of the view has a corner, or a projection of one, that is not finite */
#define ETCH_DEPTH_STATUS_MESH 2         /* view_mesh names no mesh of the batch, or one without vertices: nothing was rendered */
#define ETCH_DEPTH_STATUS_EMPTY 4        /* etch_depth_pick: the view has no valid pixel, nothing was picked */
/* Workspace bytes of etch_render_depth for NV views of meshes with at most max_faces faces. */
int etch_render_depth_workspace(int NV, int max_faces, long long* bytes);
/* Candidate pixels above which a face is rasterised by the large-face launch. */
int etch_depth_large_threshold(void);
/* Depth maps of NV views of a ragged batch of B meshes, packed as etch_sample_surface takes it (verts fp64, faces int32 local to their mesh and
 * clamped into it, vert_offsets / face_offsets (B+1) int32, max_faces >= every face count).  view_mesh (NV) int32 = the mesh each view looks
 * at; cams (NV,16) fp64 = fx, fy, cx, cy, R (3x3 row-major), t (3), world to camera p_c = R x + t with x right, y down, z forward; pixel (r, c)
 * has its centre at (c + 0.5, r + 0.5); near > 0.  Bit-defined, with the operation order of csrc/depth_render.hip: a face with a corner at
 * z_c < near is dropped whole, a pixel is covered where the three edge functions are all >= 0 or all <= 0 (and it lies in the corners' box),
 * z = 1 / sum_k ((w_k / area) / z_k); the smallest z wins, equal z -> the lowest face.  Outputs: depth (NV,H,W) fp64 (+inf = nothing hit),
 * face (NV,H,W) int32 local to the mesh (-1), bary (NV,H,W,3) fp64 perspective-corrected (0 on a miss) or NULL, dropped (NV) int32 = faces
 * dropped at the near plane, status (NV) int32 = ETCH_DEPTH_STATUS_* bits, n_large (NV) int32 = faces that took the large-face launch, or NULL. */
int etch_render_depth(int B, int NV, int H, int W, int max_faces, const double* verts, const int* faces, const int* vert_offsets,
                      const int* face_offsets, const int* view_mesh, const double* cams, double near, void* workspace, double* depth, int* face,
                      double* bary, int* dropped, int* status, int* n_large, void* stream);
/* Workspace bytes of etch_depth_compact. */
int etch_depth_compact_workspace(int NV, int H, int W, long long* bytes);
/* Back-projection of depth maps (NV,H,W) fp64, rendered or a caller's: a pixel is valid where near < z < far (far may be +inf; NaN, inf and 0
 * are background).  Outputs: count (NV) int32, offsets (NV+1) int32, and for the valid pixels of all views, view after view in row-major order,
 * index (their flat pixel r W + c, int32) and points (.,3) fp64 = R^T (p_c - t) with p_c = ((c + 0.5 - cx) / fx z, (r + 0.5 - cy) / fy z, z).
 * index and points need room for offsets[NV] entries (NV H W is always enough). */
int etch_depth_compact(int NV, int H, int W, const double* depth, const double* cams, double near, double far, void* workspace, int* count,
                       int* offsets, int* index, double* points, void* stream);
/* N points per view of the packed cloud, stratified in row-major order: sample j owns the rows [a_j, b_j) of its view, a_j = floor(j n / N),
 * b_j = floor((j + 1) n / N) with n the view's count, and takes rank_j = a_j + min(w - 1, floor(u_j w)), w = b_j - a_j (rank_j = a_j where the
 * stratum is empty, n < N); u_j is the 53-bit Philox uniform etch_sample_surface draws as u_f for sample j under keys[view].  The strata are
 * disjoint: with n >= N no row is picked twice.  center (NV,3) fp64 is subtracted from the picked points, or NULL.  Outputs: out64 (NV,N,3)
 * fp64, out32 its fp32 rounding, pixel (NV,N) int32, status (NV) int32 = ETCH_DEPTH_STATUS_EMPTY where n == 0 (that view's outputs are not
 * written). */
int etch_depth_pick(int NV, int N, const int* offsets, const int* index, const double* points, const unsigned long long* keys, const double* center,
                    double* out64, float* out32, int* pixel, int* status, void* stream);

/* ---- raw point clouds: exact grid kNN outlier filters, compaction, voxel grid (csrc/cloud_filter.hip) --------------- */

/* Bits of the per-cloud status words of the etch_cloud_* calls. */
#define ETCH_CLOUD_STATUS_NONFINITE 1    /* a coordinate of the cloud is not finite: nothing of that cloud is written */
#define ETCH_CLOUD_STATUS_RANGE 2        /* voxel grid: an axis of the cloud has more than 2^21 cells */
#define ETCH_CLOUD_STATUS_EMPTY 4        /* the cloud has no row where a result needs one (voxel origin, mean and deviation) */
#define ETCH_CLOUD_MAX_K 32              /* the largest k of etch_cloud_knn_mean */
#define ETCH_CLOUD_MAX_RINGS 4           /* rings of cells a kNN query examines before it scans its whole cloud instead */
/* A packed batch is points (M,3) fp64 and offsets (B+1) int32 that start at 0, do not decrease and end at or below M (the calls cannot check device
 * memory); M may exceed offsets[B]: the rows behind the last cloud are no cloud's, they are never read and sort behind all.
 * Bounding box, status and cell size per cloud, and the cell key of every row: grid (B,4) fp64 = the cloud's bounding-box minimum
 * and its cell size h, keys (M) int64 = (ix << 42) | (iy << 21) | iz with i = floor((p - origin) / h) clamped into [0, 2^21), cloud (M) int32 =
 * the cloud of each row, status (B) int32 = ETCH_CLOUD_STATUS_* (written, not ORed).  mode 0 (kNN): h = cell where cell > 0, else
 * max(sqrt(k S / n), L k / n) with S = ex ey + ey ez + ez ex and L = the largest of the extents ex, ey, ez; mode 1 (radius): h = cell (1 + 2^-20),
 * cell = r; both raised to L / 2^20 where smaller, and 1 where every point coincides.  mode 2 (voxel): h = cell; a row beyond 2^21 cells sets
 * ETCH_CLOUD_STATUS_RANGE.  The caller then sorts the rows by (cloud, key) with a STABLE sort: order (M) int32 = the sorted rows,
 * sorted_keys = keys[order], sorted_points = points[order]. */
int etch_cloud_cell_keys(int B, int M, int mode, int k, double cell, const double* points, const int* offsets, double* grid, long long* keys,
                         int* cloud, int* status, void* stream);
/* mean (M) fp64, by original row: (sum_j sqrt(s_j)) / k_eff over the k_eff = min(k, n - 1) smallest d2 = ((dx dx + dy dy) + dz dz) from the row to
 * the OTHER rows of its cloud (coincident ones count), summed in ascending order; 0 where n == 1.  Exact for any cell size.  brute != 0: every
 * query scans its whole cloud; sorted_points is then the unsorted points and sorted_keys, order, grid may be NULL.  Rows of a cloud with
 * ETCH_CLOUD_STATUS_NONFINITE are not written.  1 <= k <= ETCH_CLOUD_MAX_K. */
int etch_cloud_knn_mean(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                        const int* offsets, const double* grid, const int* status, double* mean, void* stream);
/* count (M) int32, by original row: the OTHER rows of the cloud with d2 <= radius radius (the product rounded once).  Needs the mode 1 keys of the
 * same radius; brute as above. */
int etch_cloud_radius_count(int B, int M, double radius, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                            const int* offsets, const int* status, int* count, void* stream);
/* Statistical filter per cloud: mu = (sum m_i) / n, s = sqrt(sum (m_i - mu)^2 / (n - 1)) (0 for n < 2), keep_i = m_i <= mu + ratio s.  The sums run in an
 * order n alone fixes (no float atomics).  stats (B,2) fp64 = mu, s; keep (M) int32; n == 0 ORs ETCH_CLOUD_STATUS_EMPTY into status. */
int etch_cloud_stat_keep(int B, double ratio, const double* mean, const int* offsets, int* status, double* stats, int* keep, void* stream);
/* Workspace bytes of etch_cloud_compact and etch_cloud_voxel_grid for B clouds. */
int etch_cloud_scan_workspace(int B, long long* bytes);
/* The rows with keep != 0, in row order: kept (B) int32 = their number per cloud, new_offsets (B+1) int32, new_index = index of the kept rows,
 * new_points their coordinates (room for M rows is always enough).  workspace: etch_cloud_scan_workspace(B) bytes. */
int etch_cloud_compact(int B, const int* keep, const int* offsets, const double* points, const int* index, void* workspace, int* kept,
                       int* new_offsets, int* new_index, double* new_points, void* stream);
/* Voxel grid from the mode 2 keys, sorted: one output row per occupied cell in ascending (ix, iy, iz) order, cloud after cloud.  cells (B) int32,
 * out_offsets (B+1) int32, centroid (.,3) fp64 = (sum of the cell's rows in ascending row order) / count, count, lowest = the cell's lowest row
 * (local to its cloud), cell_key its key (room for M rows is always enough).  A cloud with a status bit set gets no cell.  workspace: etch_cloud_scan_workspace(B)
 * bytes. */
int etch_cloud_voxel_grid(int B, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets, const int* status,
                          void* workspace, int* cells, int* out_offsets, double* centroid, int* count, int* lowest, long long* cell_key, void* stream);

/* ---- raw point clouds: isolating the subject -- RANSAC floor plane, Euclidean clusters (csrc/cloud_isolate.hip) ------- */

/* H plane hypotheses per cloud, 1 <= H <= 65536: planes (B,H,4) fp64 = unit normal and d (a point x lies at s = ((nx x + ny y) + nz z) + d),
 * valid (B,H) int32.  Hypothesis h of a cloud with n rows and key K: Philox4x32-10 with counter (h, 1, 0, 0) and key (low32 K, high32 K) -> r0..r3,
 * rows i_a = (r_a n) >> 32 (a = 0, 1, 2); u = p[i1] - p[i0], v = p[i2] - p[i0], m = u x v (each component a difference of two rounded products),
 * len2 = (mx mx + my my) + mz mz, normal = m / sqrt(len2), d = -((nx p0x + ny p0y) + nz p0z).  Invalid (four zeros, valid 0): two equal rows,
 * !(len2 > 0), n < 3, or with has_up |normal . up| < cos_tilt; with has_up a plane is negated where normal . up < 0.  up must be a unit vector. */
int etch_cloud_plane_hypotheses(int B, int H, const double* points, const int* offsets, const unsigned long long* keys, int has_up, double up_x,
                                double up_y, double up_z, double cos_tilt, double* planes, int* valid, void* stream);
/* counts (B,H,3) int32 = the rows of the cloud with |s| <= tau, with s > tau and with s < -tau, for ANY planes (B,H,4); a plane whose valid flag is 0
 * scores 0, 0, 0 (valid may be NULL: every plane counts).  counts is zeroed by the call and filled with integer atomics. */
int etch_cloud_plane_score(int B, int M, int H, double tau, const double* points, const int* offsets, const double* planes, const int* valid,
                           int* counts, void* stream);
/* The valid plane with the most inliers per cloud, a tie to the lowest h: plane (B,4), best_counts (B,3), found (B) int32.  Without has_up the
 * winner is negated (and above / below swapped) where below > above.  found = 0, and zeros, where no plane is valid or inliers < min_inliers. */
int etch_cloud_plane_select(int B, int H, int has_up, int min_inliers, const double* planes, const int* valid, const int* counts, double* plane,
                            int* best_counts, int* found, void* stream);
/* One least-squares step on the inliers of a found plane, in place: centroid c and the covariance of p - c over the rows with |s| <= tau (sums in
 * an order n alone fixes, no float atomics), normal = the eigenvector of the smallest eigenvalue (cyclic Jacobi) on the side of the given normal,
 * d = -(normal . c); counts are taken again against the new plane.  A plane with fewer than 3 inliers is left as it is. */
int etch_cloud_plane_refit(int B, double tau, const double* points, const int* offsets, const int* found, double* plane, int* counts, void* stream);
/* keep (M) int32 = s > tau for the rows of a cloud with a found plane, 1 for the rows of a cloud without, 0 behind the last cloud. */
int etch_cloud_plane_keep(int B, int M, double tau, const double* points, const int* offsets, const double* plane, const int* found, int* keep,
                          void* stream);
/* Connected components of the graph that links rows i != j of one cloud with d2 <= radius radius: label (M) int32 = the lowest row of the row's
 * component, local to its cloud, size (M) int32 = the component's rows, both by original row.  Needs the mode 1 keys of the same radius, sorted;
 * brute != 0 scans the whole cloud instead: sorted_points is then the unsorted points and sorted_keys, order may be NULL.  parent (M) int32 is
 * workspace.  Rows of a cloud with ETCH_CLOUD_STATUS_NONFINITE are not written. */
int etch_cloud_components(int B, int M, double radius, int brute, const double* sorted_points, const long long* sorted_keys, const int* order,
                          const int* offsets, const int* status, int* parent, int* label, int* size, void* stream);
/* winner (B) int32 = the label of the largest component, a tie to the lowest label (-1 for an empty cloud); keep (M) int32 =
 * size >= min_points and (largest == 0 or label == winner). */
int etch_cloud_component_keep(int B, int largest, int min_points, const int* label, const int* size, const int* offsets, int* winner, int* keep,
                              void* stream);

/* ---- raw point clouds: rigid registration of several views -- gated nearest rows, moments, Horn's step (csrc/cloud_align.hip) */

#define ETCH_ALIGN_STATUS_DEGENERATE 8   /* a step had fewer than 3 matched pairs or a cross-covariance of rank < 2: the transform was kept */
#define ETCH_ALIGN_MAX_RINGS 8           /* rings of cells a nearest query examines before it scans its whole cloud instead */
/* The rank threshold.  With s1 >= s2 >= s3 the singular values of the centred cross-covariance C = sum (x - mean x)(q - mean q)^T and
 * e = sign det C, Horn's 4 x 4 matrix has the two largest eigenvalues l1 = s1 + s2 + e s3 (the trace of C's singular values, signed) and
 * l2 = s1 - s2 - e s3.  A step is degenerate when l1 - l2 = 2 (s2 + e s3) <= ETCH_ALIGN_RANK_EPS l1: the second singular value lies below
 * 5e-10 of that trace, which is where the rotation about the first singular direction stops being determined. */
#define ETCH_ALIGN_RANK_EPS 1e-9
/* A transform is R (B,9) fp64 row-major and t (B,3) per pair of clouds: x = R p + t, per component ((R_r0 px + R_r1 py) + R_r2 pz) + t_r.
 *
 * The TARGET's cell grid: grid (B,4) fp64 = the bounding-box minimum and the cell size h of every target cloud, center (B,3) its bounding-box
 * centre, keys (M) int64 and cloud (M) int32 as etch_cloud_cell_keys writes them, status (B) int32 (written).  h = cell where cell > 0, else
 * max(sqrt(32 (ex ey + ey ez + ez ex) / n), 32 L / n, gate / (ETCH_ALIGN_MAX_RINGS - 1)): 32 rows per occupied cell, and ring
 * ETCH_ALIGN_MAX_RINGS lies strictly beyond the first gate (8 h (1 - 2^-20) >= 8/7 gate (1 - 2^-20) > gate), so a row without a partner ends its
 * ring walk there and never scans its cloud; always h >= 2^-20 L.  The caller sorts the rows by (cloud, key) with a STABLE sort. */
int etch_cloud_align_grid(int B, int M, double gate, double cell, const double* points, const int* offsets, double* grid, double* center,
                          long long* keys, int* cloud, int* status, void* stream);
/* For source row i of pair b: among the rows j of target cloud b with d2 = ((dx dx + dy dy) + dz dz) <= g g (g = gate[0] on the device, the
 * product rounded once; d = R p_i + t - q_j) the one with the least d2, a tie to the lowest row: pair (Ms) int32 = that row local to its cloud,
 * d2 (Ms) fp64; -1 and +inf where there is none.  Exact for any cell size and for queries outside the target's grid.  tgt_points are the target's
 * rows sorted with tgt_keys and tgt_order; brute != 0 scans the whole target cloud for every row: tgt_points is then the unsorted target and
 * tgt_keys, tgt_order, grid may be NULL.  query_order (Ms) int32 or NULL: thread i serves source row query_order[i] (a permutation of the rows
 * that groups neighbours into a wave; it changes no result).  done (B) int32 or NULL: the rows of a pair with done != 0 are not touched.
 * status (B) int32 is read and ORed: a pair with ETCH_CLOUD_STATUS_NONFINITE gets -1 / +inf, and a non-finite source row sets that bit. */
int etch_cloud_nearest(int B, int Ms, int brute, const double* src_points, const int* src_offsets, const int* query_order, const double* tgt_points,
                       const long long* tgt_keys, const int* tgt_order, const int* tgt_offsets, const double* grid, const double* R, const double* t,
                       const double* gate, const int* done, int* status, int* pair, double* d2, void* stream);
/* One rigid step per pair from the matched rows (pair[i] >= 0; tgt_points UNSORTED): with x = R p + t, x' = x - center and q' = q - center,
 * sums (B,16) fp64 = sum x' (3), sum q' (3), sum x' q'^T (9, row = the component of x'), sum d2 (d2 (Ms) as etch_cloud_nearest wrote it; NULL:
 * recomputed), each summed as one strided partial per thread (rows lo + tid, lo + tid + 1024, ..) and a fixed tree over the 1024 partials: an
 * order n alone fixes.  matched (B) int32 = m, rms (B) = sqrt(sum d2 / m) (+inf for m = 0).  dR (B,9), dt (B,3) minimise sum |dR x + dt - q|^2
 * (Horn's quaternion, cyclic Jacobi, det dR = +1); R <- dR R, t <- dR t + dt in place.  A degenerate step (above) ORs
 * ETCH_ALIGN_STATUS_DEGENERATE into status, leaves R, t, writes dR = I, dt = 0 and sets done.  done (B) int32: a pair with done != 0 is
 * skipped whole; it is set when the step turned by less than tol_angle (radians) and moved the matched rows' centroid by less than tol_shift,
 * and for a pair with ETCH_CLOUD_STATUS_NONFINITE.  steps (B) int32 is incremented for every pair that took the step. */
int etch_cloud_align_step(int B, const double* src_points, const int* src_offsets, const double* tgt_points, const int* tgt_offsets, const int* pair,
                          const double* d2, const double* center, double tol_angle, double tol_shift, double* R, double* t, double* sums, int* matched,
                          double* rms, double* dR, double* dt, int* status, int* done, int* steps, void* stream);
/* The loop: iters times etch_cloud_nearest with the gate gates[k] (iters fp64 on the device) and etch_cloud_align_step, 2 iters launches and no
 * host synchronisation; everything a step leaves stays on the device.  tgt_sorted, tgt_keys, tgt_order: the target's grid, built once;
 * tgt_points: the unsorted target.  brute != 0 reads tgt_points alone.  pair and d2 hold the last matching of every pair of clouds. */
int etch_cloud_align(int B, int Ms, int iters, int brute, const double* src_points, const int* src_offsets, const int* query_order,
                     const double* tgt_sorted, const long long* tgt_keys, const int* tgt_order, const double* tgt_points, const int* tgt_offsets,
                     const double* grid, const double* center, const double* gates, double tol_angle, double tol_shift, double* R, double* t,
                     double* sums, int* matched, double* rms, double* dR, double* dt, int* status, int* done, int* steps, int* pair, double* d2,
                     void* stream);
/* out (M,3) = R_b p + t_b for every row of cloud b; the rows behind the last cloud are not written. */
int etch_cloud_transform(int B, int M, const double* points, const int* offsets, const double* R, const double* t, double* out, void* stream);

/* ---- raw point clouds: surface normals on the cell grid (csrc/cloud_normals.hip, csrc/cloud_normal_solve.h) ------------------ */

#define ETCH_NORMAL_FLAG_FEW 1           /* the row has fewer than 2 neighbours (a cloud of 1 or 2 rows) */
#define ETCH_NORMAL_FLAG_AMBIGUOUS 2     /* lambda1 - lambda0 > ETCH_NORMAL_GAP_EPS lambda2 does not hold: collinear, coincident or isotropic neighbours */
#define ETCH_NORMAL_GAP_EPS 1e-9
/* For row i of a cloud with n rows, ke = min(k, n - 1), 3 <= k <= ETCH_CLOUD_MAX_K.  The neighbourhood is the ke least (d2, row) pairs among the
 * OTHER rows of the cloud, d2 = ((dx dx + dy dy) + dz dz), row = the original row: a tie in d2 goes to the lower row.  With e_j = q_j - p_i per
 * component, taken in ascending (d2, row) order, s = sum e_j and S_ab = sum e_a e_b (the product rounded once), each a sequential sum from 0 in
 * that order; w = ke + 1 (the row itself counts with e = 0), mu = s / w, C_ab = S_ab / w - mu_a mu_b.  cov (M,6) fp64 = C_xx, C_xy, C_xz, C_yy,
 * C_yz, C_zz or NULL (not written): the order is fixed, so it is defined to the bit.  Cyclic Jacobi (pairs (0,1), (0,2), (1,2), at most 10 sweeps)
 * gives lambda0 <= lambda1 <= lambda2; normal (M,3) fp64 = the normalised eigenvector of lambda0, variation (M) fp64 = lambda0 / ((lambda0 +
 * lambda1) + lambda2), 0 where that trace is not positive.  flag (M) int32 = ETCH_NORMAL_FLAG_*; a flagged row gets the normal (0, 0, 0).
 * Sign: the component of the largest magnitude is positive, a tie to the lowest axis; with viewpoint (B,3) fp64, one sensor position per cloud
 * (NULL: none), the normal is then flipped where ((n_x w_x + n_y w_y) + n_z w_z) < 0, w = viewpoint - p, so n.(v - p) >= 0 and an exact 0
 * keeps the first rule.  No orientation is propagated between rows.
 * Inputs as etch_cloud_knn_mean takes them: the mode 0 keys, sorted; exact for any cell size; brute != 0: every query scans its whole cloud,
 * sorted_points is then the unsorted points and sorted_keys, order, grid may be NULL.  All outputs are by original row.  Rows of a cloud with
 * ETCH_CLOUD_STATUS_NONFINITE are not written. */
int etch_cloud_normals(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets,
                       const double* grid, const int* status, const double* viewpoint, double* normal, double* variation, int* flag, double* cov,
                       void* stream);

/* ---- raw point clouds: the point-to-plane step of the registration (csrc/cloud_align.hip, csrc/cloud_align_solve.h) ---------- */

/* A pivot d_i of the LDL^T factorisation below must exceed this fraction of the largest diagonal entry of the scaled matrix. */
#define ETCH_ALIGN_PLANE_EPS 1e-9
/* One point-to-plane step per pair from given pairs.  tgt_normals (Mt,3) fp64: one normal per UNSORTED target row, as etch_cloud_normals or a
 * file gives them; the residual ((x - q).n)^2 is blind to the sign of n, so no consistent orientation is needed.  A matched row is a source
 * row i with pair[i] >= 0 whose target row has a non-zero normal.  x = R p + t, c = center, x' = x - c and d2 as etch_cloud_align_step states them;
 * r = ((dx n_x + dy n_y) + dz n_z), d = x - q; a = x' x n, every product rounded once; J = (a, n).  sums (B,32) fp64 = the 21 upper-triangle
 * entries of sum J J^T, row-major (a product rounded once per term), the 6 of sum J r, sum r^2, sum d2, sum x' (3), each summed as
 * etch_cloud_align_step sums: one strided partial per thread (rows lo + tid, lo + tid + 1024, ..) and the fixed tree over the 1024 partials (four sums
 * share a pass through LDS, each in the tree a pass of its own would walk).  matched (B) = m, rms (B) = sqrt(sum d2 / m) (+inf for m = 0).
 * Solve A y = -g, y = (omega, tau): the three rotation rows and columns are scaled by 1 / rho, rho = |center - box minimum| from grid (B,4) (as
 * etch_cloud_align_grid wrote it: always needed, brute or not), everything is divided by m, LDL^T runs in the fixed order 0 .. 5.  The step is
 * degenerate -- ETCH_ALIGN_STATUS_DEGENERATE is ORed into status, R and t stay, dR = I, dt = 0, y = 0, done is set -- where m < 6, rho is not
 * positive, or a pivot fails d_i > ETCH_ALIGN_PLANE_EPS max_j Abar_jj (a zero or NaN pivot fails).  That guards exact singularity only: an exact
 * plane with exact normals, collinear data, no normals; a near-symmetric target is not flagged, it slides.  Update: th = |omega|, dR from the
 * quaternion (cos th/2, sin(th/2) omega / th) (a series below th = 1e-4), normalised, in the 1 - 2 (yy + zz) form; dt = c - dR c + tau;
 * R <- dR R, t <- dR t + dt in place; y (B,6) fp64 = omega, tau (NULL: not written).  done is also set when th < tol_angle and the matched rows'
 * centroid moved by |(dR - I) mean x' + tau| < tol_shift.  status, done and steps as etch_cloud_align_step. */
int etch_cloud_align_step_plane(int B, const double* src_points, const int* src_offsets, const double* tgt_points, const double* tgt_normals,
                                const int* tgt_offsets, const int* pair, const double* d2, const double* grid, const double* center, double tol_angle,
                                double tol_shift, double* R, double* t, double* sums, int* matched, double* rms, double* dR, double* dt, double* y,
                                int* status, int* done, int* steps, void* stream);
/* etch_cloud_align with the point-to-plane step: iters times etch_cloud_nearest (unchanged: the nearest row within the gate, whatever its normal)
 * and etch_cloud_align_step_plane, 2 iters launches and no host synchronisation; sums is (B,32).  brute != 0 reads tgt_points, tgt_normals and
 * grid alone and gives the same bits: the pairs are the same, and the sums depend on the pairs alone. */
int etch_cloud_align_plane(int B, int Ms, int iters, int brute, const double* src_points, const int* src_offsets, const int* query_order,
                           const double* tgt_sorted, const long long* tgt_keys, const int* tgt_order, const double* tgt_points, const double* tgt_normals,
                           const int* tgt_offsets, const double* grid, const double* center, const double* gates, double tol_angle, double tol_shift,
                           double* R, double* t, double* sums, int* matched, double* rms, double* dR, double* dt, int* status, int* done, int* steps,
                           int* pair, double* d2, void* stream);

/* ---- raw point clouds: global registration -- FPFH descriptors, feature matches, RANSAC over triples (csrc/cloud_global.hip,
 * csrc/cloud_global_solve.h) ---------------------------------------------------------------------------------------------- */

#define ETCH_GLOBAL_BINS 11              /* bins per feature */
#define ETCH_GLOBAL_FEATURES 33          /* a descriptor: the blocks theta, alpha, phi of ETCH_GLOBAL_BINS bins each */
#define ETCH_GLOBAL_MAX_H 262144         /* the most hypotheses per pair */
/* Descriptors.  Inputs as etch_cloud_normals takes them (the mode 0 keys, sorted; exact for any cell size; brute != 0: every query scans its whole
 * cloud, sorted_points is then the unsorted points and sorted_keys, order, grid may be NULL), and points (M,3) UNSORTED, normal (M,3) fp64 unit
 * normals ORIENTED consistently (etch_cloud_normals with a viewpoint) and normal_flag (M) int32, both by original row.  3 <= k <= ETCH_CLOUD_MAX_K.
 * The neighbourhood of row i is etch_cloud_normals': the ke = min(k, n - 1) least (d2, row) pairs among the other rows of its cloud.
 * neighbours (M,k) int32 = those rows in ascending (d2, row) order, local to the cloud, -1 behind the ke-th.
 * Pass 1.  A pair (i, j), j in the list of i, is counted when both normal flags are 0, d2 > 0 and, with d = (q_j - p_i) / sqrt(d2) per component,
 * a_i = ((n_ix d_x + n_iy d_y) + n_iz d_z) and a_j likewise: the source s is i where |a_i| >= |a_j|, else j with d negated; u = n_s, t = the other
 * normal; c = d x u (each component a difference of two rounded products); cl2 = (c_x c_x + c_y c_y) + c_z c_z > 0 (else the pair is not counted);
 * v = c / sqrt(cl2); w = u x v; theta = atan2(w.t, u.t), alpha = v.t, phi = u.d, every dot ((x + y) + z).  Bins: floor((11 (theta + pi)) / (2 pi)),
 * floor((11 (alpha + 1)) / 2), floor((11 (phi + 1)) / 2), pi = the nearest double, each clamped to 0 .. 10.  spfh (M,33) int32 = the counts per
 * bin in the order theta, alpha, phi; count (M) int32 = c_i, the pairs counted.  All of it is one rounding per operation except atan2, whose last
 * bit belongs to the math library: a theta within rounding of a bin edge may fall on either side.
 * Pass 2.  F_i[f] = sum_j (1 / d2_ij) ((100 spfh_j[f]) / c_j) over the list of i in its order, sequentially from 0, skipping c_j = 0 and d2 = 0;
 * then per block s = the sequential sum of its 11 entries and F[f] <- (100 F[f]) / s where s > 0, else 0.  feature (M,33) fp64; has_feature (M)
 * int32 = 0 where the row's normal is flagged, c_i = 0 or a block sum is not positive.  Rows of a cloud with ETCH_CLOUD_STATUS_NONFINITE are not
 * written. */
int etch_cloud_fpfh(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const double* points,
                    const int* offsets, const double* grid, const int* status, const double* normal, const int* normal_flag, int* spfh, int* count,
                    int* neighbours, double* feature, int* has_feature, void* stream);
/* For source row i of pair b with src_has != 0: among the rows j of target cloud b with tgt_has != 0 the one with the least (D, row),
 * D = sum_f (a_f - b_f)^2 summed sequentially over f = 0 .. 32 from 0 (the product rounded once): match (Ms) int32 = that row local to its cloud,
 * dist (Ms) fp64 = D; -1 and +inf where the row has no feature or the target none. */
int etch_cloud_feature_match(int B, int Ms, const double* src_feature, const int* src_has, const int* src_offsets, const double* tgt_feature,
                             const int* tgt_has, const int* tgt_offsets, int* match, double* dist, void* stream);
/* The correspondences of pair b are its matched source rows in ascending row order: corr_offsets (B+1) int32, corr_src (N,3) fp64 the source
 * points, corr_tgt (N,3) the matched target points, corr_row (N) int32 the matched target rows.  Hypothesis h of a pair with n_c correspondences and
 * key K, 1 <= H <= ETCH_GLOBAL_MAX_H: Philox4x32-10 with counter (h, 2, 0, 0) and key (low32 K, high32 K) -> r0..r3, i_a = (r_a n_c) >> 32 (a = 0,
 * 1, 2), written to triples (B,H,3) int32.  Invalid (valid 0, the identity written): n_c < 3; two equal i_a; two equal target rows; an edge (0,1),
 * (1,2) or (2,0) that fails ls2 >= e2 lt2 and lt2 >= e2 ls2 and ls2 >= m2, with ls2, lt2 = ((dx dx + dy dy) + dz dz) on the source and the target
 * side, e2 = edge_similarity edge_similarity, m2 = min_edge min_edge; or a degenerate solve.  The solve is etch_cloud_align_step's on the three pairs:
 * c = 0.5 (min + max) of the target triple per component, the 16 sums of x' = a - c, q' = b - c taken in the order a = 0, 1, 2, Horn's quaternion.
 * transforms (B,H,12) fp64 = R row-major, then t. */
int etch_cloud_global_hypotheses(int B, int H, const double* corr_src, const double* corr_tgt, const int* corr_row, const int* corr_offsets,
                                 const unsigned long long* keys, double edge_similarity, double min_edge, double* transforms, int* valid, int* triples,
                                 void* stream);
/* inliers (B,H) int32 = the correspondences c of pair b with ((dx dx + dy dy) + dz dz) <= tau tau (the product rounded once), d = R a_c + t - b_c and
 * the transform applied as etch_cloud_align_grid states it, for ANY transforms (B,H,12); a hypothesis whose valid flag is 0 scores 0 (valid may be
 * NULL: every one counts).  inliers is zeroed by the call and filled with integer atomics. */
int etch_cloud_global_score(int B, int N, int H, double tau, const double* corr_src, const double* corr_tgt, const int* corr_offsets,
                            const double* transforms, const int* valid, int* inliers, void* stream);
/* The valid hypothesis with the most inliers per pair, a tie to the lowest h: R (B,9), t (B,3), best (B) int32 its inliers, best_h (B) int32 = h,
 * found (B) int32.  found = 0, the identity, best = 0 and best_h = -1 where no hypothesis is valid or inliers < min_inliers. */
int etch_cloud_global_select(int B, int H, int min_inliers, const double* transforms, const int* valid, const int* inliers, double* R, double* t, int* best,
                             int* best_h, int* found, void* stream);
/* pair (Ms) int32 = match[i] where match[i] >= 0 and source row i, moved by its pair's R, t, lies within tau of its matched target row (the test of
 * etch_cloud_global_score), else -1: the pairs etch_cloud_align_step refits on. */
int etch_cloud_global_inliers(int B, int Ms, double tau, const double* src_points, const int* src_offsets, const double* tgt_points, const int* tgt_offsets,
                              const int* match, const double* R, const double* t, int* pair, void* stream);

/* ---- raw point clouds: point winding numbers and containment against a cloud (csrc/cloud_winding.hip, csrc/cloud_winding_solve.h; DESIGN
 * section 26) -------------------------------------------------------------------------------------------------------------------------------- */

/* d2k (M) fp64 by original row = the ke-th least d2 among the other rows of the row's cloud, ke = min(k, n - 1), 3 <= k <= ETCH_CLOUD_MAX_K: the d2
 * of the last row of etch_cloud_normals' neighbourhood; 0 for a cloud of one row.  Inputs as etch_cloud_knn_mean takes them (the mode 0 keys, sorted;
 * exact for any cell size; brute != 0: every query scans its whole cloud, sorted_points is then the unsorted points and sorted_keys, order, grid may
 * be NULL), and the same bits in every form.  Rows of a cloud with ETCH_CLOUD_STATUS_NONFINITE are not written. */
int etch_cloud_knn_kth(int B, int M, int k, int brute, const double* sorted_points, const long long* sorted_keys, const int* order, const int* offsets,
                       const double* grid, const int* status, double* d2k, void* stream);
/* The rows the winding sweep reads, from points (M,3), normal (M,3) ORIENTED unit normals, flag (M) int32 and d2k (M) of etch_cloud_knn_kth at the
 * same k, all fp64 by original row; center (B,3) fp64 or NULL = 0.  a_i = (pi d2k_i) / ke in fp64 in that order, 0 where ke = 0, flag_i != 0 or a
 * coordinate of the row is not finite.  pos (M,3) = fp32(p - center), moment (M,3) = fp32(a n), cap (M) = fp32(a / pi): each difference, product and
 * quotient in fp64, rounded once. */
int etch_cloud_surface_pack(int B, int M, int k, const double* points, const double* normal, const int* flag, const double* d2k, const int* offsets,
                            const double* center, float* pos, float* moment, float* cap, void* stream);
/* Workspace bytes of etch_cloud_winding_number. */
int etch_cloud_winding_number_workspace(int B, int Q, int max_rows, long long* bytes);
/* The winding number of the oriented cloud b (rows offsets[b] .. offsets[b + 1] of pos, moment, cap; offsets (B+1) int32 in device memory; max_rows
 * >= every cloud's row count sizes the launch, rows of a cloud past it are not visited) at queries (B,Q,3) fp32; q_len (B) int32 or NULL: queries at
 * or past it are padding and get w 0, nearest -1, nearest_d2 0.  Per (query q, row i), every operation fp32 and rounded once: r = pos_i - q,
 * d2 = (rx rx + ry ry) + rz rz, s = d2 where d2 > cap_i else cap_i, term = ((rx mx + ry my) + rz mz) / (s sqrtf(s)); a row with cap_i == 0 contributes
 * exactly 0.  A thread adds the terms of one 1024-row chunk in ascending row order in fp32 from 0; the chunks are added in ascending order in fp64,
 * multiplied by the double nearest 1 / (4 pi) and rounded once: w (B,Q) = 1 inside a closed surface sampled with outward normals, 0 outside, -1
 * with inward normals.  nearest (B,Q) int32 or NULL = the row, local to its cloud, with the least (d2, row) among the rows with d2 < +inf (a NaN or
 * infinite d2 never wins; -1 where there is none), nearest_d2 (B,Q) fp32 or NULL its d2 (0 with -1), from the same pass.  No atomics: cloud b in a
 * batch is bitwise cloud b alone, and two runs are bitwise equal. */
int etch_cloud_winding_number(int B, int Q, int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, const float* queries,
                              const int* q_len, void* workspace, float* w, int* nearest, float* nearest_d2, void* stream);
/* Workspace bytes of etch_cloud_containment_energy_grad. */
int etch_cloud_containment_energy_grad_workspace(int B, int V, long long* bytes);
/* etch_containment_energy_grad against a cloud: o_v = [ |w_v| < 0.5 ] and nearest_v in [0, n_b) (a NaN w is not outside), c_v = pos[nearest_v] as
 * fp64 -- a SAMPLE of the surface.  terms (B,2) fp64 = {sum_v o_v nearest_d2_v, sum_v o_v}; g (B,V,3) or NULL, to which coef_b w_contain (2 / V)
 * o_v (v - c_v) is ADDED under the rules stated there. */
int etch_cloud_containment_energy_grad(int B, int V, const float* body_verts, const float* pos, const int* offsets, const float* w, const int* nearest,
                                       const float* nearest_d2, const float* coef, float w_contain, void* workspace, double* terms, float* g,
                                       void* stream);
/* Workspace bytes of etch_smpl_surface_refine_contain_cloud. */
int etch_smpl_surface_refine_contain_cloud_workspace(int B, int N, int V, int nj, int nb, int n_extra, int max_rows, long long* bytes);
/* etch_smpl_surface_refine_contain with the scan given as an oriented cloud (max_rows, pos, moment, cap, offsets, in the frame of the body): at a
 * refresh the one pass of etch_cloud_winding_number over the current vertices gives o_v and the row each outside vertex is pulled to; everything
 * else -- the hold-fixed rule, the normalisation by V, the trace (B, iters, 5), the schedule on `stream` without a host wait -- is as stated
 * there.  With w_contain = 0 the parameters and the first four trace columns are bitwise those of etch_smpl_surface_refine. */
int etch_smpl_surface_refine_contain_cloud(int B, int N, int V, int F, int nj, int nb, int n_extra, const void* const* consts, const int* faces,
                                           const float* points, const int* n_len, const float* weights, int M, const int* marker_vids, const float* markers,
                                           const float* marker_valid, const void* const* prior, int n_gauss, int iters, float lr, float beta1, float beta2,
                                           float eps, float w_dense, float w_marker, float w_beta, float w_prior, float trunc, int optimize_scale,
                                           int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, float w_contain,
                                           int contain_every, float* params, float* verts, float* joints, float* loss_trace, float* loss_last,
                                           void* workspace, void* stream);

/* ---- raw point clouds: a watertight mesh from the winding field (csrc/cloud_mesh.hip, csrc/cloud_mesh_solve.h) ------------- */
#define ETCH_MESH_BLOCK_NODES 729        /* 9^3 nodes of a block of 8 x 8 x 8 cells */
#define ETCH_MESH_BLOCK_CELLS 512
#define ETCH_MESH_TABLE_INACTIVE (-1)    /* block table: the block is not evaluated */
#define ETCH_MESH_TABLE_MARK (-2)        /* block table: marked by etch_cloud_mesh_seed or etch_cloud_mesh_grow; the caller gives it a slot >= 0 */

/* The lattice of the oriented cloud b (pos, cap, offsets as etch_cloud_winding_number takes them) for the voxel h = `voxel` > 0: node g of an axis
 * lies at fp32((double) g h), a block covers the nodes 8 B .. 8 B + 8 of every axis.  lattice (B,6) int32 = lo[3], hi[3] in blocks with
 * lo = floor(min / (8 h)) - pad_blocks, hi = floor(max / (8 h)) + 1 + pad_blocks over the rows with cap > 0 and a finite pos, in fp64.  status (B)
 * int32 (written): ETCH_CLOUD_STATUS_EMPTY without such a row, ETCH_CLOUD_STATUS_RANGE where an axis has more than 2^20 - 1 nodes, the lattice more
 * than 2^24 blocks or |lo|, |hi| reach 2^27; lo = hi = 0 then. */
int etch_cloud_mesh_lattice(int B, int max_rows, const float* pos, const float* cap, const int* offsets, double voxel, int pad_blocks, int* lattice,
                            int* status, void* stream);
/* Round 0: the block of every row that counts, dilated by seed_dilate (0 .. 2) blocks in the 26-neighbourhood and clipped to the lattice, gets
 * ETCH_MESH_TABLE_MARK in table.  table: one int32 per block of every cloud, cloud b's at table_offsets[b] (B+1 int64 in device memory), block
 * (x, y, z) local to lo at (x ny + y) nz + z -- the order of the block keys.  A cloud with a status bit is skipped. */
int etch_cloud_mesh_seed(int B, int max_rows, const float* pos, const float* cap, const int* offsets, double voxel, int seed_dilate, const int* lattice,
                         const int* status, const long long* table_offsets, int* table, void* stream);
/* field (S,729) fp32: s = fabsf(w) - level at the nodes of the blocks slots (S,2) int32 = (cloud, the block's index in the cloud's table), node
 * (ox, oy, oz) of a block at (ox 9 + oy) 9 + oz.  w is etch_cloud_winding_number's at the node's fp32 position, to the bit; one workgroup per slot,
 * no workspace, no atomics: a node shared by two blocks has the same bits in both.  A slot that names no block of its lattice is not written. */
int etch_cloud_mesh_field(int B, int S, int max_rows, const float* pos, const float* moment, const float* cap, const int* offsets, double voxel, float level,
                          const int* lattice, const int* slots, float* field, void* stream);
/* The face test of the S blocks of the last round (slots, field as above): face f (-x, +x, -y, +y, -z, +z) is mixed when its 81 nodes are neither
 * all inside nor all outside, inside = !(s < 0).  flags (S,6) int32 = 0, or 1: mixed towards a block that has no slot -- that block now holds
 * ETCH_MESH_TABLE_MARK --, or 2: mixed and pointing out of the lattice (clipped). */
int etch_cloud_mesh_grow(int B, int S, const int* lattice, const long long* table_offsets, const int* slots, const float* field, int* table, int* flags,
                         void* stream);
/* Marching tetrahedra on the Freudenthal split of every cell of the S blocks, for ANY field values.  counts (S,512) int32 or NULL = triangles per
 * cell, cell (cx, cy, cz) at (cx 8 + cy) 8 + cz.  With cell_offsets (S,512) int64 = the exclusive prefix sum of the counts and F their total, cell c
 * writes its triangles (tetrahedron 0..5, triangle 0..1) from face cell_offsets[c] on: face_keys (F,3) int64 = the 63-bit keys of the three
 * crossings, (((ix 2^20 + iy) 2^20 + iz) 8 + kind) with i the edge's lower node local to the lattice and kind = 4 dx + 2 dy + dz the edge's offset;
 * face_pos (F,3,3) fp32 = their positions, per axis t = s_n / (s_n - s_up), x = x_n + t (x_up - x_n) in fp32, one rounding per operation. */
int etch_cloud_mesh_extract(int B, int S, long long F, const int* lattice, double voxel, const int* slots, const float* field, int* counts,
                            const long long* cell_offsets, long long* face_keys, float* face_pos, void* stream);
/* labels (V) int32: `passes` rounds of hooking and pointer jumping over faces (F,3) int32; init != 0 starts from label_v = v.  changed (1) int32 is
 * set to 0 and then to 1 by a round that lowered a label: call again (init = 0) until it stays 0; then label_v = the lowest vertex index of v's
 * connected component. */
int etch_mesh_components(int V, int F, const int* faces, int init, int passes, int* labels, int* changed, void* stream);
/* The vertices with labels == label and the faces whose first vertex has it, compacted with their order kept: vert_prefix (V), face_prefix (F)
 * int64 = the INCLUSIVE prefix sums of those two conditions, kept_verts, kept_faces their totals.  out_verts (kept_verts,3) fp32, out_faces
 * (kept_faces,3) int32 re-indexed. */
int etch_mesh_keep_component(int V, int F, const float* verts, const int* faces, const int* labels, int label, const long long* vert_prefix,
                             const long long* face_prefix, long long kept_verts, long long kept_faces, float* out_verts, int* out_faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ETCH_HIP_H */
