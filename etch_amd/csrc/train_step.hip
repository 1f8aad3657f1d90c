// The training step's own kernels (train.py:81-125): the four losses with their gradients in one launch, and Adam with the reference's NaN guards in
// two launches whatever the number of parameter tensors; the pack of the gradients into one flat buffer for accumulated and data-parallel steps.
// DESIGN section 11.
#include "common.h"
#include "etch_hip.h"

// ---------------------------------------------------------------------------------------------------------------- losses
// One wave per row r = b K + k of the head outputs.  Every lane computes the row's three point terms (uniform loads, no divergence), the wave
// shares the row's M logits.  Sums: fp64, per wave over its rows in row order, per workgroup over its 4 waves, then by the workgroup that arrives
// last over the workgroups: lane l of wave 0 takes workgroups l, l + 64, ... in order and a fixed butterfly joins the lanes -- one order, whichever
// workgroup is last.
#define TL_WAVES 4
#define TL_MAX_BLOCKS 256                 /* measured: 47 us per call at 5 000 rows; a cap of 2 048 (one row per wave) took 118 us -- the arrival fence and counter cost more than the rows */
#define TL_SLOTS 5                        /* direction, magnitude, confidence, part label, rows dropped for a bad label / index */

__device__ __forceinline__ double tl_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(64 * TL_WAVES) train_losses_kernel(
    long R, int K, int N, int M, const float* __restrict__ direction, const float* __restrict__ magnitude, const float* __restrict__ conf,
    const float* __restrict__ logits, const float* __restrict__ t_vec, const float* __restrict__ t_conf, const long long* __restrict__ t_lab,
    const long long* __restrict__ index, float w_dir, float w_mag, float w_conf, float w_part, float scale_mag, double* part, unsigned* counter,
    float* __restrict__ losses, int* __restrict__ status, float* __restrict__ g_dir, float* __restrict__ g_mag, float* __restrict__ g_conf,
    float* __restrict__ g_logits) {
    __shared__ double s_part[TL_WAVES][TL_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves = (long)gridDim.x * TL_WAVES;
    const float inv_r = 1.f / (float)R;
    const float c_dir = w_dir * inv_r, c_mag = 2.f * w_mag * inv_r, c_conf = 2.f * w_conf * inv_r, c_part = w_part * inv_r;
    double acc[TL_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long r = (long)blockIdx.x * TL_WAVES + wave; r < R; r += waves) {
        const long b = r / K;
        const long long n = index[r];
        const bool row_ok = n >= 0 && n < (long long)N;
        const long tr = b * (long)N + (row_ok ? (long)n : 0);
        bool dropped = !row_ok;
        if (direction || magnitude) {
            const float vx = t_vec[tr * 3], vy = t_vec[tr * 3 + 1], vz = t_vec[tr * 3 + 2];
            const float vn = sqrtf(vx * vx + vy * vy + vz * vz);
            if (direction) {
                // F.cosine_similarity: each operand divided by max(its norm, eps) first, then the dot product
                const float dx = direction[r * 3], dy = direction[r * 3 + 1], dz = direction[r * 3 + 2];
                const float dn = sqrtf(dx * dx + dy * dy + dz * dz);
                const float eps = 1e-8f;
                const float iv = 1.f / fmaxf(vn, eps), id = 1.f / fmaxf(dn, eps);
                const float ax = vx * iv, ay = vy * iv, az = vz * iv;
                const float cs = (ax * dx + ay * dy + az * dz) * id;
                // d cos / d d = a / |d| - cos d / |d|^2 ; below the clamp the norm is the constant eps
                const float k2 = dn >= eps ? cs * id * id : 0.f;
                float gx = -c_dir * (ax * id - k2 * dx), gy = -c_dir * (ay * id - k2 * dy), gz = -c_dir * (az * id - k2 * dz);
                if (!row_ok) gx = gy = gz = 0.f;
                else acc[0] += (double)(1.f - cs);
                if (lane == 0) { g_dir[r * 3] = gx; g_dir[r * 3 + 1] = gy; g_dir[r * 3 + 2] = gz; }
            }
            if (magnitude) {
                const float d = vn * scale_mag - magnitude[r];
                if (row_ok) acc[1] += (double)(d * d);
                if (lane == 0) g_mag[r] = row_ok ? -c_mag * d : 0.f;
            }
        }
        if (conf) {
            const float d = conf[r] - t_conf[tr];
            if (row_ok) acc[2] += (double)(d * d);
            if (lane == 0) g_conf[r] = row_ok ? c_conf * d : 0.f;
        }
        if (logits) {
            const long long lab = t_lab[tr];
            const bool ok = row_ok && lab >= 0 && lab < (long long)M;
            dropped = dropped || !ok;
            const float* x = logits + r * (long)M;
            float* gx = g_logits + r * (long)M;
            if (ok) {
                float mx = -INFINITY;
                for (int j = lane; j < M; j += 64) mx = fmaxf(mx, x[j]);
                mx = etch_wave_max_f32(mx);
                float s = 0.f;
                for (int j = lane; j < M; j += 64) s += expf(x[j] - mx);
                s = etch_wave_sum_f32(s);
                acc[3] += (double)(mx + logf(s) - x[lab]);
                const float is = 1.f / s;
                for (int j = lane; j < M; j += 64) gx[j] = c_part * (expf(x[j] - mx) * is - (j == (int)lab ? 1.f : 0.f));
            } else {
                for (int j = lane; j < M; j += 64) gx[j] = 0.f;
            }
        }
        if (dropped) acc[4] += 1.0;
    }
    if (lane == 0)
        for (int k = 0; k < TL_SLOTS; ++k) s_part[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < TL_SLOTS) {
        double s = 0.0;
        for (int w = 0; w < TL_WAVES; ++w) s += s_part[w][threadIdx.x];
        part[(size_t)blockIdx.x * TL_SLOTS + threadIdx.x] = s;
    }
    if (!etch_last_block(counter, gridDim.x)) return;
    if (wave != 0) return;
    double tot[TL_SLOTS];
    for (int k = 0; k < TL_SLOTS; ++k) {
        double s = 0.0;
        for (unsigned i = lane; i < gridDim.x; i += 64) s += part[(size_t)i * TL_SLOTS + k];
        tot[k] = tl_wave_sum_f64(s);
    }
    if (lane == 0) {
        const double w[4] = {(double)w_dir, (double)w_mag, (double)w_conf, (double)w_part};
        const bool present[4] = {direction != nullptr, magnitude != nullptr, conf != nullptr, logits != nullptr};
        double total = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double v = present[k] ? tot[k] / (double)R * w[k] : 0.0;
            losses[k] = (float)v;
            total += v;
        }
        losses[4] = (float)total;
        status[0] = (total != total ? ETCH_TRAIN_STATUS_NAN : 0) | (tot[4] > 0.0 ? ETCH_TRAIN_STATUS_BAD_LABEL : 0);
    }
}

int etch_train_losses_workspace_doubles(void) { return TL_MAX_BLOCKS * TL_SLOTS; }

int etch_train_losses(int B, int K, int N, int M, const float* direction, const float* magnitude, const float* confidences, const float* part_labels,
                      const float* t_vectors, const float* t_confidences, const long long* t_labels, const long long* index, float direction_w,
                      float magnitude_w, float confidence_w, float part_label_w, float scale_magnitude, double* workspace, unsigned* counter,
                      float* losses, int* status, float* g_direction, float* g_magnitude, float* g_confidences, float* g_part_labels, void* stream) {
    if (B <= 0 || K <= 0 || N <= 0 || !index || !workspace || !counter || !losses || !status) return ETCH_EINVAL;
    if (!direction && !magnitude && !confidences && !part_labels) return ETCH_EINVAL;
    if ((direction && !g_direction) || (magnitude && !g_magnitude) || (confidences && !g_confidences) || (part_labels && !g_part_labels)) return ETCH_EINVAL;
    if ((direction || magnitude) && !t_vectors) return ETCH_EINVAL;
    if (confidences && !t_confidences) return ETCH_EINVAL;
    if (part_labels && (!t_labels || M <= 0)) return ETCH_EINVAL;
    const long R = (long)B * K;
    long blocks = (R + TL_WAVES - 1) / TL_WAVES;
    if (blocks > TL_MAX_BLOCKS) blocks = TL_MAX_BLOCKS;
    hipLaunchKernelGGL(train_losses_kernel, dim3((unsigned)blocks), dim3(64 * TL_WAVES), 0, (hipStream_t)stream, R, K, N, M, direction, magnitude,
                       confidences, part_labels, t_vectors, t_confidences, t_labels, index, direction_w, magnitude_w, confidence_w, part_label_w,
                       scale_magnitude, workspace, counter, losses, status, g_direction, g_magnitude, g_confidences, g_part_labels);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- guarded Adam
// The parameter tensors are cut into chunks of ADAM_CHUNK elements (a tensor's last chunk is shorter; a small tensor is one chunk); one workgroup per
// chunk, so one 5 M-element tensor and a thousand 64-element ones spread over the compute units alike.  Pass 1 writes, per chunk, which of {NaN,
// +inf, -inf} its gradient holds (a plain store per chunk: nothing to zero between steps) and advances the step counts; pass 2 ORs the flags of its
// tensor's chunks and updates.  Both read the loss kernel's status word: NaN total -> nothing changes.
#define ADAM_CHUNK 8192
#define ADAM_THREADS 256

int etch_guarded_adam_chunk(void) { return ADAM_CHUNK; }

struct AdamChunk { int t; long start; int len; };
__device__ __forceinline__ AdamChunk adam_chunk(const int* __restrict__ chunk_tensor, const int* __restrict__ first_chunk, const long long* __restrict__ numel) {
    AdamChunk c;
    c.t = chunk_tensor[blockIdx.x];
    c.start = (long)((int)blockIdx.x - first_chunk[c.t]) * ADAM_CHUNK;
    const long left = (long)numel[c.t] - c.start;
    c.len = (int)(left < ADAM_CHUNK ? (left > 0 ? left : 0) : ADAM_CHUNK);
    return c;
}

__device__ __forceinline__ unsigned adam_classify(float g) {
    return g != g ? 1u : (g == INFINITY ? 2u : (g == -INFINITY ? 4u : 0u));
}

__global__ void __launch_bounds__(ADAM_THREADS) guarded_adam_flag_kernel(const int* __restrict__ chunk_tensor, const int* __restrict__ first_chunk,
                                                                          const long long* __restrict__ numel, const unsigned long long* __restrict__ gtab,
                                                                          const int* __restrict__ status, float* steps, unsigned* __restrict__ chunkflags) {
    __shared__ unsigned s_bits;
    const AdamChunk c = adam_chunk(chunk_tensor, first_chunk, numel);
    const float* g = reinterpret_cast<const float*>(gtab[c.t]);
    if (!g) {
        if (threadIdx.x == 0) chunkflags[blockIdx.x] = 0u;
        return;
    }
    const bool skip = status && (status[0] & ETCH_TRAIN_STATUS_NAN);
    if (threadIdx.x == 0) {
        s_bits = 0u;
        if (c.start == 0 && !skip) steps[c.t] += 1.f;
    }
    __syncthreads();
    g += c.start;
    unsigned bits = 0u;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int n4 = c.len >> 2;
        for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
            const float4 q = reinterpret_cast<const float4*>(g)[i];
            bits |= adam_classify(q.x) | adam_classify(q.y) | adam_classify(q.z) | adam_classify(q.w);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += ADAM_THREADS) bits |= adam_classify(g[i]);
    } else {
        for (int i = threadIdx.x; i < c.len; i += ADAM_THREADS) bits |= adam_classify(g[i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off, 64);
    if ((threadIdx.x & 63) == 0 && bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0) chunkflags[blockIdx.x] = s_bits;
}

struct AdamCoef { float w1, b2, w2, step_size, bc2_sqrt, eps; };
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamCoef& k) {
    // torch.optim.Adam's single-tensor step: exp_avg.lerp_(g, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2);
    // p.addcdiv_(exp_avg, sqrt(exp_avg_sq) / sqrt(bias_correction2) + eps, -lr / bias_correction1) -- lerp's two forms included, so that non-finite
    // moments behave as torch's do
    const float diff = g - m;
    m = k.w1 < 0.5f ? m + k.w1 * diff : g - diff * (1.f - k.w1);
    v = v * k.b2 + (k.w2 * g) * g;
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p - k.step_size * (m / denom);
}

__global__ void __launch_bounds__(ADAM_THREADS) guarded_adam_update_kernel(const int* __restrict__ chunk_tensor, const int* __restrict__ first_chunk,
                                                                            const long long* __restrict__ numel, const unsigned long long* __restrict__ pmv,
                                                                            int T, const unsigned long long* __restrict__ gtab, const int* __restrict__ status,
                                                                            const float* __restrict__ steps, const unsigned* __restrict__ chunkflags,
                                                                            double lr, double beta1, double beta2, double eps, int* counters) {
    __shared__ unsigned s_bits;
    __shared__ AdamCoef s_coef;
    const bool skip = status && (status[0] & ETCH_TRAIN_STATUS_NAN);
    if (blockIdx.x == 0 && threadIdx.x == 0 && status) {
        if (skip) atomicAdd(&counters[1], 1);
        if (status[0] & ETCH_TRAIN_STATUS_BAD_LABEL) atomicOr(&counters[2], 1);
    }
    if (skip) return;
    const AdamChunk c = adam_chunk(chunk_tensor, first_chunk, numel);
    const float* g = reinterpret_cast<const float*>(gtab[c.t]);
    if (!g) return;
    float* p = reinterpret_cast<float*>(pmv[c.t]);
    float* m = reinterpret_cast<float*>(pmv[(size_t)T + c.t]);
    float* v = reinterpret_cast<float*>(pmv[(size_t)2 * T + c.t]);
    if (threadIdx.x == 0) {
        s_bits = 0u;
        const double step = (double)steps[c.t];
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
        s_coef = AdamCoef{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps};
    }
    __syncthreads();
    {
        unsigned bits = 0u;
        for (int i = first_chunk[c.t] + (int)threadIdx.x; i < first_chunk[c.t + 1]; i += ADAM_THREADS) bits |= chunkflags[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off, 64);
        if ((threadIdx.x & 63) == 0 && bits) atomicOr(&s_bits, bits);
    }
    __syncthreads();
    // train.py:122 `param.grad.sum().isnan()`: a NaN in the gradient, or infinities of both signs
    const bool zeroed = (s_bits & 1u) || (s_bits & 6u) == 6u;
    if (zeroed && c.start == 0 && threadIdx.x == 0) atomicAdd(&counters[0], 1);
    const AdamCoef k = s_coef;
    p += c.start; g += c.start; m += c.start; v += c.start;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const int n4 = vec ? c.len >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
        float4 pq = reinterpret_cast<float4*>(p)[i], mq = reinterpret_cast<float4*>(m)[i], vq = reinterpret_cast<float4*>(v)[i];
        float4 gq = reinterpret_cast<const float4*>(g)[i];
        if (zeroed) gq = make_float4(0.f, 0.f, 0.f, 0.f);
        adam_element(pq.x, gq.x, mq.x, vq.x, k);
        adam_element(pq.y, gq.y, mq.y, vq.y, k);
        adam_element(pq.z, gq.z, mq.z, vq.z, k);
        adam_element(pq.w, gq.w, mq.w, vq.w, k);
        reinterpret_cast<float4*>(p)[i] = pq;
        reinterpret_cast<float4*>(m)[i] = mq;
        reinterpret_cast<float4*>(v)[i] = vq;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += ADAM_THREADS) {
        float pe = p[i], me = m[i], ve = v[i];
        adam_element(pe, zeroed ? 0.f : g[i], me, ve, k);
        p[i] = pe; m[i] = me; v[i] = ve;
    }
}

int etch_guarded_adam_step(int T, int C, const int* chunk_tensor, const int* first_chunk, const long long* numel, const unsigned long long* pmv,
                           const unsigned long long* grads, const int* status, float* steps, unsigned* chunkflags, double lr, double beta1,
                           double beta2, double eps, int* counters, void* stream) {
    if (T <= 0 || C <= 0 || !chunk_tensor || !first_chunk || !numel || !pmv || !grads || !steps || !chunkflags || !counters) return ETCH_EINVAL;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return ETCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(guarded_adam_flag_kernel, dim3((unsigned)C), dim3(ADAM_THREADS), 0, st, chunk_tensor, first_chunk, numel, grads, status, steps,
                       chunkflags);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(guarded_adam_update_kernel, dim3((unsigned)C), dim3(ADAM_THREADS), 0, st, chunk_tensor, first_chunk, numel, pmv, T, grads, status,
                       steps, chunkflags, lr, beta1, beta2, eps, counters);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- gradient pack
// Accumulated and data-parallel steps: every contribution's gradients go, scaled, into one flat buffer over the Adam chunk table -- one
// workgroup per chunk, tensor t at flat[off[t], off[t] + numel[t]) with off[t] a multiple of 4 elements -- and the step's small words into the
// GRAD_TAIL floats at `tail`: one SUM all-reduce then moves everything.  The product and the sum are rounded separately (no FMA), as torch's
// `flat + g * s` is: contributions combine to the same bits whether they were added here or by the collective.
#define GRAD_TAIL 8                       /* 5 losses, NaN-total count, bad-label count, spare (zero) */

int etch_grad_tail_floats(void) { return GRAD_TAIL; }

__device__ __forceinline__ float grad_pack_value(float g, float s, float prev, bool add) {
#pragma clang fp contract(off)
    const float v = g * s;
    return add ? prev + v : v;
}

__global__ void __launch_bounds__(ADAM_THREADS) grad_pack_kernel(const int* __restrict__ chunk_tensor, const int* __restrict__ first_chunk,
                                                                  const long long* __restrict__ numel, const unsigned long long* __restrict__ gtab,
                                                                  const long long* __restrict__ off, float* flat, float s, int mode,
                                                                  const float* __restrict__ losses, const int* __restrict__ status, long long tail) {
    const bool add = mode != 0;
    if (blockIdx.x == 0 && threadIdx.x < GRAD_TAIL && tail >= 0) {
        const int k = threadIdx.x;
        float v = 0.f;              // a count needs no scale: the unpack asks only whether it is zero
        if (k < 5) v = losses ? losses[k] : 0.f;
        else if (k == 5) v = status && (status[0] & ETCH_TRAIN_STATUS_NAN) ? 1.f : 0.f;
        else if (k == 6) v = status && (status[0] & ETCH_TRAIN_STATUS_BAD_LABEL) ? 1.f : 0.f;
        float* d = flat + tail + k;
        *d = grad_pack_value(v, k < 5 ? s : 1.f, add ? *d : 0.f, add);
    }
    const AdamChunk c = adam_chunk(chunk_tensor, first_chunk, numel);
    const float* g = reinterpret_cast<const float*>(gtab[c.t]);
    float* d = flat + off[c.t] + c.start;
    if (!g) {                       // no gradient in this contribution: zeros for the first, nothing to add afterwards
        if (!add)
            for (int i = threadIdx.x; i < c.len; i += ADAM_THREADS) d[i] = 0.f;
        return;
    }
    g += c.start;
    const bool vec = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
    const int n4 = vec ? c.len >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += ADAM_THREADS) {
        const float4 gq = reinterpret_cast<const float4*>(g)[i];
        float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (add) dq = reinterpret_cast<const float4*>(d)[i];
        dq.x = grad_pack_value(gq.x, s, dq.x, add);
        dq.y = grad_pack_value(gq.y, s, dq.y, add);
        dq.z = grad_pack_value(gq.z, s, dq.z, add);
        dq.w = grad_pack_value(gq.w, s, dq.w, add);
        reinterpret_cast<float4*>(d)[i] = dq;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < c.len; i += ADAM_THREADS) d[i] = grad_pack_value(g[i], s, add ? d[i] : 0.f, add);
}

int etch_grad_pack(int T, int C, const int* chunk_tensor, const int* first_chunk, const long long* numel, const unsigned long long* grads,
                   const long long* offsets, float* flat, float scale, int mode, const float* losses, const int* status, long long tail_offset,
                   void* stream) {
    if (T <= 0 || C <= 0 || !chunk_tensor || !first_chunk || !numel || !grads || !offsets || !flat || (mode != 0 && mode != 1)) return ETCH_EINVAL;
    hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)C), dim3(ADAM_THREADS), 0, (hipStream_t)stream, chunk_tensor, first_chunk, numel, grads, offsets,
                       flat, scale, mode, losses, status, tail_offset);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}

// After the reduction: the tail back into the words the step reads -- the (5) losses, and the status word etch_guarded_adam_step obeys (a bit is set
// if any contribution set it).
__global__ void __launch_bounds__(64) grad_unpack_tail_kernel(const float* __restrict__ tail, float* __restrict__ losses, int* __restrict__ status) {
    const int k = threadIdx.x;
    if (k < 5) losses[k] = tail[k];
    else if (k == 5) status[0] = (tail[5] != 0.f ? ETCH_TRAIN_STATUS_NAN : 0) | (tail[6] != 0.f ? ETCH_TRAIN_STATUS_BAD_LABEL : 0);
}

int etch_grad_unpack_tail(const float* tail, float* losses, int* status, void* stream) {
    if (!tail || !losses || !status) return ETCH_EINVAL;
    hipLaunchKernelGGL(grad_unpack_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tail, losses, status);
    ETCH_RETURN_IF_LAUNCH_FAILED();
    return ETCH_OK;
}
