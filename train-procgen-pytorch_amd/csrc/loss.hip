// The PPO loss (agents/ppo.py:131-169 with cross_batch_entropy, common/misc_util.py:42-51): per-sample terms, forward statistics,
// finalisation and the analytic gradient; and the feature-sparsity metric (common/model.py:207) with its gradient, single-rank and
// multi-rank.  gfx950 only.  Every reduction has a fixed summation order (no float atomics anywhere).
#include "common.h"
#include "device_util.h"
#include "loss_sample.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ PPO loss
// (the per-sample terms, the per-sample gradient and the finalisation of a segment's statistics are in loss_sample.h)
// samples per workgroup of the loss kernels: one wave -- 128 workgroups for an 8192-sample minibatch (the exp / log heavy per-sample
// work ran on 32 CUs with four-wave workgroups: 35 us)
constexpr int LOSS_BLK = 64;
int loss_blocks(int n) { return (n + LOSS_BLK - 1) / LOSS_BLK; }

template <bool LSE>
__global__ __launch_bounds__(LOSS_BLK) void loss_bwd_kernel(LossArgs a) {
    const int s = blockIdx.x * LOSS_BLK + threadIdx.x;
    if (s >= a.n) return;
    SampleTerms t;
    sample_terms<LSE>(a, s, t);
    loss_bwd_sample<LSE>(a, s, t);
}
// one LOSS_BLK-sample block of the loss: sums over the samples s < s_end of this block -> partial row `row` (per value: wave sums,
// then the waves in order, one barrier per block).  BWD: the loss has no
// batch-level term (x_entropy_coef == 0), so the gradient of the sample goes out in the same pass.
template <bool BWD, bool LSE>
__device__ __forceinline__ void loss_fwd_block(const LossArgs& a, int s, int s_end, int row) {
    constexpr int NW = LOSS_BLK / 64;
    __shared__ float sw[NW][8 + MAXA];
    SampleTerms t;
    float pi = 0.f, vm = 0.f, H = 0.f;
    float pa[MAXA];
#pragma unroll
    for (int k = 0; k < MAXA; ++k) pa[k] = 0.f;
    if (s < s_end) {
        sample_terms<LSE>(a, s, t);
        pi = fminf(t.surr1, t.surr2);
        vm = fmaxf(t.vs1, t.vs2);
        H = t.H;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < a.A) pa[k] = t.p[k];
        if (BWD) loss_bwd_sample<LSE>(a, s, t);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float r = wave_sum(pi); if (lane == 0) sw[w][0] = r;
    r = wave_sum(vm);       if (lane == 0) sw[w][1] = r;
    r = wave_sum(H);        if (lane == 0) sw[w][2] = r;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < a.A) { r = wave_sum(pa[k]); if (lane == 0) sw[w][8 + k] = r; }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 3 || (k >= 8 && k < 8 + a.A)) {
        float t = sw[0][k];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) t += sw[w2][k];
        a.partial[(long long)row * (8 + a.A) + k] = t;
    }
}
template <bool LSE>
__global__ __launch_bounds__(LOSS_BLK) void loss_fwd_kernel(LossArgs a) {
    loss_fwd_block<false, LSE>(a, blockIdx.x * LOSS_BLK + threadIdx.x, a.n, blockIdx.x);
}
// segment k owns ceil(len_k / LOSS_BLK) consecutive blocks (no block straddles two minibatches)
__device__ __forceinline__ void seg_of_block(const SegTab& st, int b, int& k, int& first) {
    first = 0;
    for (k = 0; k < st.n_seg - 1; ++k) {
        const int nb = (st.start[k + 1] - st.start[k] + LOSS_BLK - 1) / LOSS_BLK;
        if (b < first + nb) break;
        first += nb;
    }
}
template <bool BWD, bool LSE>
__global__ __launch_bounds__(LOSS_BLK) void loss_fwd_seg_kernel(LossArgs a, SegTab st) {
    int k, first;
    seg_of_block(st, blockIdx.x, k, first);
    loss_fwd_block<BWD, LSE>(a, st.start[k] + (blockIdx.x - first) * LOSS_BLK + threadIdx.x, st.start[k + 1], blockIdx.x);
}
int loss_blocks_seg(const SegTab& st) {
    int nb = 0;
    for (int k = 0; k < st.n_seg; ++k) nb += (st.start[k + 1] - st.start[k] + LOSS_BLK - 1) / LOSS_BLK;
    return nb;
}
void launch_loss_fwd_seg(const LossArgs& a, const SegTab& st, bool with_bwd, hipStream_t stream) {
    const int nb = loss_blocks_seg(st);
    if (nb <= 0) return;
    if (a.value_from_logits) {
        if (with_bwd) hipLaunchKernelGGL((loss_fwd_seg_kernel<true, true>), dim3(nb), dim3(LOSS_BLK), 0, stream, a, st);
        else hipLaunchKernelGGL((loss_fwd_seg_kernel<false, true>), dim3(nb), dim3(LOSS_BLK), 0, stream, a, st);
    } else if (with_bwd) hipLaunchKernelGGL((loss_fwd_seg_kernel<true, false>), dim3(nb), dim3(LOSS_BLK), 0, stream, a, st);
    else hipLaunchKernelGGL((loss_fwd_seg_kernel<false, false>), dim3(nb), dim3(LOSS_BLK), 0, stream, a, st);
}
void launch_loss_fwd(const LossArgs& a, hipStream_t st) {
    if (a.n <= 0) return;
    if (a.value_from_logits) hipLaunchKernelGGL(loss_fwd_kernel<true>, dim3(loss_blocks(a.n)), dim3(LOSS_BLK), 0, st, a);
    else hipLaunchKernelGGL(loss_fwd_kernel<false>, dim3(loss_blocks(a.n)), dim3(LOSS_BLK), 0, st, a);
}

__global__ void loss_finalize_kernel(LossArgs a, int nblk, int phase, const float* fs_ptr, float* log_slot) {
    loss_finalize_body(a, nblk, phase, fs_ptr, log_slot);
}
__global__ void loss_finalize_seg_kernel(LossArgs a, SegTab st, int phase, float* stats_base, const double* fs_parts, int fs_d, float* fs_out,
                                         float* log_base) {
    const int k = blockIdx.x;
    int first = 0;
    for (int j = 0; j < k; ++j) first += (st.start[j + 1] - st.start[j] + LOSS_BLK - 1) / LOSS_BLK;
    a.partial += (long long)first * (8 + a.A);
    a.stats = stats_base + 32 * k;
    if (fs_parts && threadIdx.x == 0) {                 // second half of the feature-sparsity metric: mean over the d columns
        double tot = 0.0;
        for (int j = 0; j < FS_PARTS; ++j) tot += fs_parts[k * FS_PARTS + j];
        fs_out[k] = (float)(tot / fs_d);
    }
    loss_finalize_body(a, (st.start[k + 1] - st.start[k] + LOSS_BLK - 1) / LOSS_BLK, phase, fs_parts ? fs_out + k : nullptr, log_base ? log_base + 8 * k : nullptr);
}
// phase 2 of n_rec records at once (after the cross-rank sum of the statistics ring): record k from stats_base + 32 k, fs_base[k]
__global__ void loss_finalize_records_kernel(LossArgs a, float* stats_base, const float* fs_base, float* log_base) {
    const int k = blockIdx.x;
    a.stats = stats_base + 32 * k;
    loss_finalize_body(a, 0, 2, fs_base ? fs_base + k : nullptr, log_base + 8 * k);
}
void launch_loss_finalize_records(const LossArgs& a, int n_rec, float* stats_base, const float* fs_base, float* log_base, hipStream_t stream) {
    if (n_rec <= 0) return;
    hipLaunchKernelGGL(loss_finalize_records_kernel, dim3(n_rec), dim3(64), 0, stream, a, stats_base, fs_base, log_base);
}
void launch_loss_finalize_seg(const LossArgs& a, const SegTab& st, int phase, float* stats_base, const double* fs_parts, int fs_d, float* fs_out,
                              float* log_base, hipStream_t stream) {
    hipLaunchKernelGGL(loss_finalize_seg_kernel, dim3(st.n_seg), dim3(256), 0, stream, a, st, phase, stats_base, fs_parts, fs_d, fs_out, log_base);
}
void launch_loss_finalize(const LossArgs& a, int nblk, int phase, const float* fs_ptr, float* log_slot, hipStream_t st) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, a, nblk, phase, fs_ptr, log_slot);
}

void launch_loss_bwd(const LossArgs& a, hipStream_t st) {
    if (a.n <= 0) return;
    if (a.value_from_logits) hipLaunchKernelGGL(loss_bwd_kernel<true>, dim3(loss_blocks(a.n)), dim3(LOSS_BLK), 0, st, a);
    else hipLaunchKernelGGL(loss_bwd_kernel<false>, dim3(loss_blocks(a.n)), dim3(LOSS_BLK), 0, st, a);
}

// feature-sparsity metric (common/model.py:207): mean_j max_b tanh(|100*relu(h_bj)|)
// = mean_j tanh(100 * max_b relu(h_bj)) (tanh monotone).  flat_pre is block3's output BEFORE the ReLU.
// FS_GROUPS row groups x d columns of partial maxima; a thread owns 8 consecutive columns (16-byte bf16 / 2 x 16-byte
// fp32 loads), a workgroup walks whole rows.
constexpr int FS_GROUPS = 128;
__global__ __launch_bounds__(256) void colmax_partial_kernel(const void* x, int bf16, int n, int d, float* part) {
    for (int j = threadIdx.x * 8; j < d; j += 256 * 8) {
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = blockIdx.x; b < n; b += FS_GROUPS) {
            const long long o = (long long)b * d + j;
            if (bf16) {
                const uint4 u = *(const uint4*)((const unsigned short*)x + o);
                const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], (k & 1) ? bfw_hi(w[k >> 1]) : bfw_lo(w[k >> 1]));
            } else {
                const f32x4 lo = *(const f32x4*)((const float*)x + o), hi = *(const f32x4*)((const float*)x + o + 4);
                m[0] = fmaxf(m[0], lo.x); m[1] = fmaxf(m[1], lo.y); m[2] = fmaxf(m[2], lo.z); m[3] = fmaxf(m[3], lo.w);
                m[4] = fmaxf(m[4], hi.x); m[5] = fmaxf(m[5], hi.y); m[6] = fmaxf(m[6], hi.z); m[7] = fmaxf(m[7], hi.w);
            }
        }
        float* p = part + (long long)blockIdx.x * d + j;
        *(f32x4*)p = (f32x4){m[0], m[1], m[2], m[3]};
        *(f32x4*)(p + 4) = (f32x4){m[4], m[5], m[6], m[7]};
    }
}
__global__ __launch_bounds__(1024) void fs_finalize_kernel(const float* part, int groups, int d, float* fs_out) {
    __shared__ double sb[16];
    double s = 0.0;
    for (int j = threadIdx.x; j < d; j += 1024) {
        float m = 0.f;
#pragma unroll 16
        for (int g = 0; g < groups; ++g) m = fmaxf(m, part[(long long)g * d + j]);
        s += (double)tanhf(fabsf(m * 100.f));
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double tot = 0.0; for (int k = 0; k < 16; ++k) tot += sb[k]; fs_out[0] = (float)(tot / d); }
}
// segment-aware two-stage version (mi_minibatch_multi and the single-minibatch path of modes 0 / 2): G row groups per segment with
// G x n_seg ~ 512 workgroups (all CUs busy, 4 rows in flight per thread), then FS_PARTS column blocks per segment whose fp64
// partial sums the loss finalisation adds up.
__device__ __forceinline__ void fs_row_max(const void* x, int bf16, long long o, float (&m)[8]) {
    if (bf16) {
        const uint4 u = *(const uint4*)((const unsigned short*)x + o);
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) m[q] = fmaxf(m[q], (q & 1) ? bfw_hi(w[q >> 1]) : bfw_lo(w[q >> 1]));
    } else {
        const f32x4 lo = *(const f32x4*)((const float*)x + o), hi = *(const f32x4*)((const float*)x + o + 4);
        m[0] = fmaxf(m[0], lo.x); m[1] = fmaxf(m[1], lo.y); m[2] = fmaxf(m[2], lo.z); m[3] = fmaxf(m[3], lo.w);
        m[4] = fmaxf(m[4], hi.x); m[5] = fmaxf(m[5], hi.y); m[6] = fmaxf(m[6], hi.z); m[7] = fmaxf(m[7], hi.w);
    }
}
template <bool BF16>
__global__ __launch_bounds__(256) void colmax_partial_seg_kernel(const void* x, SegTab st, int d, int G, float* part) {
    const int k = blockIdx.y, r0 = st.start[k], r1 = st.start[k + 1];
    for (int j = threadIdx.x * 8; j < d; j += 256 * 8) {
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int b = r0 + blockIdx.x;
        // 8 rows in flight (the storage type is a template parameter: no branch between the loads): a workgroup's 32 rows are a chain
        // of load round trips otherwise (14.8 us for 32 MB with 4 in flight)
        for (; b + 7 * G < r1; b += 8 * G) {
            if constexpr (BF16) {
                uint4 u[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) u[q] = *(const uint4*)((const unsigned short*)x + (long long)(b + q * G) * d + j);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const unsigned w[4] = {u[q].x, u[q].y, u[q].z, u[q].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], (e & 1) ? bfw_hi(w[e >> 1]) : bfw_lo(w[e >> 1]));
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) fs_row_max(x, 0, (long long)(b + q * G) * d + j, m);
            }
        }
        for (; b < r1; b += G) fs_row_max(x, BF16 ? 1 : 0, (long long)b * d + j, m);
        float* p = part + ((long long)k * G + blockIdx.x) * d + j;
        *(f32x4*)p = (f32x4){m[0], m[1], m[2], m[3]};
        *(f32x4*)(p + 4) = (f32x4){m[4], m[5], m[6], m[7]};
    }
}
__global__ __launch_bounds__(256) void fs_parts_seg_kernel(const float* part, int G, int d, double* fs_parts) {
    __shared__ double sb[4];
    const int k = blockIdx.y, cols = d / FS_PARTS;
    part += (long long)k * G * d;
    double s = 0.0;
    for (int j = blockIdx.x * cols + threadIdx.x; j < (blockIdx.x + 1) * cols; j += 256) {
        float m = 0.f;
#pragma unroll 16
        for (int g = 0; g < G; ++g) m = fmaxf(m, part[(long long)g * d + j]);
        s += (double)tanhf(fabsf(m * 100.f));
    }
    const double t = block_sum256(s, sb);
    if (threadIdx.x == 0) fs_parts[k * FS_PARTS + blockIdx.x] = t;
}
#ifndef FS_TOTAL_GROUPS
#define FS_TOTAL_GROUPS 256      // row groups over all segments: stage 1 (column maxima) gets faster, stage 2 (max over groups) slower with more
#endif
int fs_groups_per_segment(int n_seg) { int g = FS_TOTAL_GROUPS / (n_seg < 1 ? 1 : n_seg); int p = 32; while (p * 2 <= g) p *= 2; return p; }
void launch_fs_metric_seg(const void* flat_pre, int bf16, const SegTab& st, int d, float* colmax_scratch, double* fs_parts, hipStream_t stream) {
    if (st.n_seg <= 0) return;
    if (d % (8 * FS_PARTS)) { mi_launch_fail("feature-sparsity metric: the feature count must be a multiple of 64"); return; }
    const int G = fs_groups_per_segment(st.n_seg);
    if (bf16) hipLaunchKernelGGL(colmax_partial_seg_kernel<true>, dim3(G, st.n_seg), dim3(256), 0, stream, flat_pre, st, d, G, colmax_scratch);
    else hipLaunchKernelGGL(colmax_partial_seg_kernel<false>, dim3(G, st.n_seg), dim3(256), 0, stream, flat_pre, st, d, G, colmax_scratch);
    hipLaunchKernelGGL(fs_parts_seg_kernel, dim3(FS_PARTS, st.n_seg), dim3(256), 0, stream, (const float*)colmax_scratch, G, d, fs_parts);
}
int fs_metric_groups() { return FS_GROUPS; }                    // row groups launch_fs_metric leaves in its scratch
void launch_fs_metric(const void* flat_pre, int bf16, int n, int d, float* colmax_scratch, float* fs_out, hipStream_t st) {
    if (n <= 0) return;
    if (d % 8) { mi_launch_fail("feature-sparsity metric: the feature count must be a multiple of 8"); return; }      // the flattened IMPALA feature map (2048)
    hipLaunchKernelGGL(colmax_partial_kernel, dim3(FS_GROUPS), dim3(256), 0, st, flat_pre, bf16, n, d, colmax_scratch);
    hipLaunchKernelGGL(fs_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)colmax_scratch, FS_GROUPS, d, fs_out);
}

// Gradient of the feature-sparsity term fs_coef * mean_j max_b tanh(|100 h_bj|) (agents/ppo.py:148-169, common/model.py:207) with
// respect to the pre-fc features: for every column j the term depends on ONE row, the first one (in minibatch order, torch.max's
// choice) that attains the column maximum m_j; d/dh = fs_coef * 100 * (1 - tanh(100 m_j)^2) / d there (h > 0: |.| is the identity; a
// column whose maximum is 0 has gradient 0, abs'(0) = 0).  part: the G x d partial column maxima the metric kernels left behind.
__global__ __launch_bounds__(256) void fs_colmax_final_kernel(const float* part, int G, int d, float* colmax, int* arg) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    float m = 0.f;
    for (int g = 0; g < G; ++g) m = fmaxf(m, part[(long long)g * d + j]);
    colmax[j] = m; arg[j] = 0x7fffffff;
}
__global__ __launch_bounds__(256) void fs_argfirst_kernel(const void* x, int bf16, int n, int d, const float* colmax, int* arg) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const float m = colmax[j];
    if (!(m > 0.f)) return;
    int first = 0x7fffffff;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const long long o = (long long)b * d + j;
        const float v = bf16 ? __uint_as_float(((unsigned)((const unsigned short*)x)[o]) << 16) : ((const float*)x)[o];
        if (v == m && b < first) first = b;
    }
    if (first != 0x7fffffff) atomicMin(arg + j, first);
}
__global__ __launch_bounds__(256) void fs_apply_kernel(void* G, int bf16, int d, const float* colmax, const int* arg, float scale) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const int b = arg[j];
    if (b == 0x7fffffff) return;
    const float t = tanhf(fabsf(colmax[j] * 100.f)), g = scale * (1.f - t * t);
    const long long o = (long long)b * d + j;
    if (bf16) {
        unsigned short* p = (unsigned short*)G + o;
        *p = f2bf(__uint_as_float(((unsigned)*p) << 16) + g);
    } else ((float*)G)[o] += g;
}
// Multi-rank: the column maxima are those of the GLOBAL minibatch.  Every rank packs its own candidate per column
// into one 64-bit key -- (bits of the local maximum) << 32 | (0xffffffff - global position of its first row attaining it) -- so that ONE
// max-all-reduce yields the global maximum (non-negative floats order like their bit patterns) and, among equal maxima, the row that
// comes first in the global minibatch (torch.max's choice in the single-process reference).  Key 0 = no positive value in the column.
__global__ __launch_bounds__(256) void fs_keys_kernel(const float* colmax, const int* arg, const int32_t* gpos, int d, long long* keys, long long* keys_local) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const int b = arg[j];
    long long k = 0;
    if (b != 0x7fffffff && colmax[j] > 0.f)
        k = ((long long)__float_as_uint(colmax[j]) << 32) | (long long)(0xffffffffu - (unsigned)gpos[b]);
    keys[j] = k; keys_local[j] = k;
}
// after the all-reduce: the winner of column j adds the gradient at its row; every rank takes the global maximum for the metric
__global__ __launch_bounds__(256) void fs_apply_keys_kernel(void* G, int bf16, int d, const long long* keys, const long long* keys_local, const int* arg, float scale) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const long long k = keys[j];
    if (k == 0 || k != keys_local[j]) return;
    const float m = __uint_as_float((unsigned)((unsigned long long)k >> 32));
    const float t = tanhf(fabsf(m * 100.f)), g = scale * (1.f - t * t);
    const long long o = (long long)arg[j] * d + j;
    if (bf16) {
        unsigned short* p = (unsigned short*)G + o;
        *p = f2bf(__uint_as_float(((unsigned)*p) << 16) + g);
    } else ((float*)G)[o] += g;
}
__global__ __launch_bounds__(1024) void fs_from_keys_kernel(const long long* keys, int d, float* fs_out) {      // mean_j tanh(|100 m_j|) of the global maxima
    __shared__ double sb[16];
    double s = 0.0;
    for (int j = threadIdx.x; j < d; j += 1024) s += (double)tanhf(fabsf(__uint_as_float((unsigned)((unsigned long long)keys[j] >> 32)) * 100.f));
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double tot = 0.0; for (int k = 0; k < 16; ++k) tot += sb[k]; fs_out[0] = (float)(tot / d); }
}
// part: [G][d] partial column maxima of this rank's rows; gpos: global minibatch position of every local row (ascending)
void launch_fs_keys(const void* x, int bf16, int n, int d, const float* part, int G, const int32_t* gpos, float* colmax, int* arg,
                    long long* keys, long long* keys_local, hipStream_t st) {
    hipLaunchKernelGGL(fs_colmax_final_kernel, dim3((d + 255) / 256), dim3(256), 0, st, part, G, d, colmax, arg);
    if (n > 0) hipLaunchKernelGGL(fs_argfirst_kernel, dim3((d + 255) / 256, n < 64 ? n : 64), dim3(256), 0, st, x, bf16, n, d, (const float*)colmax, arg);
    hipLaunchKernelGGL(fs_keys_kernel, dim3((d + 255) / 256), dim3(256), 0, st, (const float*)colmax, (const int*)arg, gpos, d, keys, keys_local);
}
void launch_fs_apply_keys(void* Gd, int bf16, int d, const long long* keys, const long long* keys_local, const int* arg, float fs_coef, hipStream_t st) {
    hipLaunchKernelGGL(fs_apply_keys_kernel, dim3((d + 255) / 256), dim3(256), 0, st, Gd, bf16, d, keys, keys_local, arg, fs_coef * 100.f / (float)d);
}
void launch_fs_from_keys(const long long* keys, int d, float* fs_out, hipStream_t st) {
    hipLaunchKernelGGL(fs_from_keys_kernel, dim3(1), dim3(1024), 0, st, keys, d, fs_out);
}
// x: block3's output before the ReLU [n][d] (fp32 / bf16); part: [G][d] partial column maxima of relu(x); Gd: d loss / d x [n][d], updated in place
void launch_fs_grad(const void* x, int bf16, int n, int d, const float* part, int G, void* Gd, float fs_coef, float* colmax, int* arg, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(fs_colmax_final_kernel, dim3((d + 255) / 256), dim3(256), 0, st, part, G, d, colmax, arg);
    hipLaunchKernelGGL(fs_argfirst_kernel, dim3((d + 255) / 256, n < 64 ? n : 64), dim3(256), 0, st, x, bf16, n, d, (const float*)colmax, arg);
    hipLaunchKernelGGL(fs_apply_kernel, dim3((d + 255) / 256), dim3(256), 0, st, Gd, bf16, d, (const float*)colmax, (const int*)arg, fs_coef * 100.f / (float)d);
}
