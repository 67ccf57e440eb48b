// The policy / value heads (common/policy.py:74-80) at update size, forward and backward, and the rollout's action sampling
// (agents/ppo.py:77-79): the stand-alone sampler, the log-probability table, the fused heads + sample kernel of a policy step and the
// Philox test hook.  gfx950 only.
#include "common.h"
#include "policy_math.h"
#include <hip/hip_ext.h>
#include <math.h>

// ------------------------------------------------------------------------------------------ heads forward (training-sized batches)
// hout[s][o] = feat[s] . Wh[o] + bh[o] for the (A+1) <= 16 head outputs, H == 256 (policy.py:74-80).  The generic GEMM ran this
// 8192 x 16 x 256 product as 16-wide tiles of a 64-wide kernel plus a split-K pass (19 us); here 16 rows and the head matrix go
// through LDS and thread (row, output) owns one dot product, written with the sums in the order of heads_sample_kernel's H == 256 loop.
// The two kernels' logits of one observation under one set of weights are NOT the same bits, as this comment used to say: how the four
// products of a step are rounded is left to the compiler's contraction, and as built this loop multiplies and adds them unfused while
// heads_sample_kernel's takes one multiply and three fused multiply-adds.  What holds, and what tests/test_gpu_policy_ops.py pins: each is
// within the dot product's bound of the float64 logit, and the two differ by at most 138 * 2^-24 * (sum|feat * W| + |b|) (a step's term differs
// by at most 8 roundings of its products, each of the 64 additions and the bias's by one more in either kernel).  Making them equal means spelling
// the step out with fmaf in both loops; that moves every update-sized logit by a rounding and with it the training results, so it is not
// done in passing.
__global__ __launch_bounds__(256) void heads_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ Wh, const float* __restrict__ bh,
                                                        float* __restrict__ hout, int n, int O) {
    __shared__ __attribute__((aligned(16))) float s_f[16 * 260];
    __shared__ __attribute__((aligned(16))) float s_w[16 * 260];
    const int tid = threadIdx.x, e0 = blockIdx.x * 16, el = tid >> 4, o = tid & 15;
    f32x4 rf[4], rw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = tid + j * 256, r = k >> 6, kk = (k & 63) * 4;
        const int rr = e0 + r < n ? e0 + r : n - 1;
        rf[j] = *(const f32x4*)(feat + (long long)rr * 256 + kk);
        rw[j] = *(const f32x4*)(Wh + (long long)(r < O ? r : O - 1) * 256 + kk);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int k = tid + j * 256; *(f32x4*)(s_f + (k >> 6) * 260 + (k & 63) * 4) = rf[j]; *(f32x4*)(s_w + (k >> 6) * 260 + (k & 63) * 4) = rw[j]; }
    __syncthreads();
    const float* w = s_w + o * 260;
    const float* f = s_f + el * 260;
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < 256; k += 4) {
        const f32x4 fv = *(const f32x4*)(f + k), ww = *(const f32x4*)(w + k);
        acc += fv.x * ww.x + fv.y * ww.y + fv.z * ww.z + fv.w * ww.w;
    }
    if (o < O && e0 + el < n) hout[(long long)(e0 + el) * O + o] = acc + bh[o];
}
void launch_heads_fwd(const float* feat, const float* Wh, const float* bh, float* hout, int n, int O, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(heads_fwd_kernel, dim3((n + 15) / 16), dim3(256), 0, st, feat, Wh, bh, hout, n, O);
}

// ------------------------------------------------------------------------------------------ heads backward in one launch
// The policy / value heads are one 256 x (A+1) linear layer (policy.py:74-80): their data gradient, weight gradient and bias gradient
// used to be two GEMM launches (each too small to fill a matrix-core tile grid), a split-K reduce and a two-stage column sum -- five
// launches of 5-14 us for 67 MFLOP.  One thread per feature column k: for every row of the workgroup's chunk it forms
// dfeat[s][k] = (feat > 0) * sum_o dY[s][o] W[o][k] (an fmaf chain in output order) and accumulates gW[o][k] += dY[s][o] feat[s][k];
// threads k < O also sum dY[s][k] (the bias gradient).  One slab per workgroup, added in fixed order by reduce_slabs_kernel.
// dY rows are read through the constant address space (uniform address -> scalar loads: 16 values per row for the whole workgroup).
// H <= 256, O <= 16.
typedef const __attribute__((address_space(4))) float* hb_const_f32p;
__global__ __launch_bounds__(256) void heads_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ feat, const float* __restrict__ Wh,
                                                        int relu_mask, float* __restrict__ dfeat, float* __restrict__ slab, int n, int H, int O) {
    const int k = threadIdx.x;
    const int chunk = (n + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * chunk, r1 = min(n, r0 + chunk);
    float w[16], gw[16], gb = 0.f;
#pragma unroll
    for (int o = 0; o < 16; ++o) { w[o] = (o < O && k < H) ? Wh[(long long)o * H + k] : 0.f; gw[o] = 0.f; }
    const int kk = k < H ? k : H - 1;
    int s = r0;
    constexpr int RF = 8;                                  // rows in flight (a workgroup's rows are a chain of load round trips otherwise)
    for (; s + RF <= r1; s += RF) {
        float f[RF], d[RF];
#pragma unroll
        for (int q = 0; q < RF; ++q) f[q] = feat[(long long)(s + q) * H + kk];
#pragma unroll
        for (int q = 0; q < RF; ++q) {
            hb_const_f32p dy = (hb_const_f32p)(dY + (long long)(s + q) * O);
            float acc = 0.f;
#pragma unroll
            for (int o = 0; o < 16; ++o) if (o < O) { const float v = dy[o]; acc = fmaf(v, w[o], acc); gw[o] = fmaf(v, f[q], gw[o]); }
            d[q] = (relu_mask && !(f[q] > 0.f)) ? 0.f : acc;
            if (k < O) gb += dY[(long long)(s + q) * O + k];
        }
        if (k < H) {
#pragma unroll
            for (int q = 0; q < RF; ++q) dfeat[(long long)(s + q) * H + k] = d[q];
        }
    }
    for (; s < r1; ++s) {
        const float f = feat[(long long)s * H + kk];
        hb_const_f32p dy = (hb_const_f32p)(dY + (long long)s * O);
        float acc = 0.f;
#pragma unroll
        for (int o = 0; o < 16; ++o) if (o < O) { const float v = dy[o]; acc = fmaf(v, w[o], acc); gw[o] = fmaf(v, f, gw[o]); }
        if (k < H) dfeat[(long long)s * H + k] = (relu_mask && !(f > 0.f)) ? 0.f : acc;
        if (k < O) gb += dY[(long long)s * O + k];
    }
    float* sl = slab + (long long)blockIdx.x * (O * H + O);
    if (k < H) {
#pragma unroll
        for (int o = 0; o < 16; ++o) if (o < O) sl[(long long)o * H + k] = gw[o];
    }
    if (k < O) sl[(long long)O * H + k] = gb;
}
// gW[O][H] += dY^T feat ; gb[O] += colsum(dY) ; dfeat = (dY W) * (feat > 0 if relu_mask).  ws: >= 512 * (O*H + O) floats.
static int heads_bwd_grid(int n) { const int g = (n + 15) / 16; return g > 512 ? 512 : g; }   // 16 rows per workgroup at the training sizes: two steps of 8 rows, two workgroups per CU
// the slab sum of launch_heads_bwd(..., with_reduce = false), on a stream of the caller's choice (nothing but the optimizer needs gW / gb)
void launch_heads_bwd_reduce(const float* ws, float* gW, float* gb, int n, int H, int O, hipStream_t st) {
    if (n <= 0) return;
    launch_reduce_slabs(ws, heads_bwd_grid(n), O * H + O, gW, O * H, gb, O, st);
}
void launch_heads_bwd(const float* dY, const float* feat, const float* Wh, int relu_mask, float* dfeat, float* gW, float* gb, float* ws,
                      int n, int H, int O, hipStream_t st, bool with_reduce, hipEvent_t done_ev) {
    if (n <= 0) return;
    // done_ev: completion of THIS launch as an event (hipExtLaunchKernelGGL: the dispatch packet's own completion signal) -- a separate
    // hipEventRecord behind the kernel is one more packet on the queue and a 7-9 us bubble in front of the next kernel
    if (done_ev) hipExtLaunchKernelGGL(heads_bwd_kernel, dim3(heads_bwd_grid(n)), dim3(256), 0, st, nullptr, done_ev, 0, dY, feat, Wh, relu_mask, dfeat, ws, n, H, O);
    else
    hipLaunchKernelGGL(heads_bwd_kernel, dim3(heads_bwd_grid(n)), dim3(256), 0, st, dY, feat, Wh, relu_mask, dfeat, ws, n, H, O);
    if (with_reduce) launch_heads_bwd_reduce(ws, gW, gb, n, H, O, st);
}

// ------------------------------------------------------------------------------------------ rollout head: sample
// agents/ppo.py:77-79: dist.sample(), dist.log_prob(act).  Inverse-CDF over the A probabilities with a
// uniform from a caller-supplied array (tests) or Philox4x32-10 keyed by (seed, counter + env).
template <bool LSE>
__global__ void sample_kernel(const float* hout, int n, int A, const float* u, unsigned long long seed,
                              unsigned long long ctr, int32_t* act, float* logp, float* value) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float* h = hout + (long long)e * (A + 1);
    float z[MAXA], lp[MAXA], p[MAXA];
    for (int k = 0; k < A; ++k) z[k] = h[k];
    float lse = 0.f, q1[MAXA];
    log_softmax_twice_t<LSE>(z, A, lp, p, lse, q1);
    const float uu = u ? u[e] : philox_uniform(seed, ctr + e);
    float cdf = 0.f;
    int a_sel = 0;
    for (int k = 0; k < A; ++k) { cdf += expf(lp[k]); if (cdf <= uu) a_sel = k + 1; }
    if (a_sel > A - 1) a_sel = A - 1;
    if (act) act[e] = a_sel;
    if (logp) logp[e] = lp[a_sel];
    if (value) value[e] = LSE ? lse : h[A];
}
template <bool LSE>
__global__ void logp_all_kernel(const float* hout, int n, int A, float* lp_out, float* value_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float* h = hout + (long long)e * (A + 1);
    float z[MAXA], lp[MAXA], p[MAXA];
    for (int k = 0; k < A; ++k) z[k] = h[k];
    float lse = 0.f, q1[MAXA];
    log_softmax_twice_t<LSE>(z, A, lp, p, lse, q1);
    if (lp_out) for (int k = 0; k < A; ++k) lp_out[(long long)e * A + k] = lp[k];
    if (value_out) value_out[e] = LSE ? lse : h[A];
}
void launch_logp_all(const float* hout, int n, int A, float* lp_out, float* value_out, hipStream_t st, int value_from_logits) {
    if (n <= 0) return;
    if (value_from_logits) hipLaunchKernelGGL(logp_all_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, st, hout, n, A, lp_out, value_out);
    else hipLaunchKernelGGL(logp_all_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, st, hout, n, A, lp_out, value_out);
}
// test hook: in6[i] = {c0,c1,c2,c3,k0,k1} -> out4[i] = the four output words; u_out[i] = the sampler's uniform for
// (seed = k0 | k1 << 32, counter = c0 | c1 << 32), i.e. exactly what sample_kernel / heads_sample_kernel draw
__global__ void philox_debug_kernel(const uint32_t* in6, int n, uint32_t* out4, float* u_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c[4] = {in6[6 * i], in6[6 * i + 1], in6[6 * i + 2], in6[6 * i + 3]};
    uint32_t k[2] = {in6[6 * i + 4], in6[6 * i + 5]};
    philox4x32_10(c, k);
    for (int j = 0; j < 4; ++j) out4[4 * i + j] = c[j];
    u_out[i] = philox_uniform((unsigned long long)in6[6 * i + 4] | ((unsigned long long)in6[6 * i + 5] << 32),
                              (unsigned long long)in6[6 * i] | ((unsigned long long)in6[6 * i + 1] << 32));
}
void launch_philox_debug(const uint32_t* in6, int n, uint32_t* out4, float* u_out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(philox_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in6, n, out4, u_out);
}
// Rollout head, fused: policy/value heads (common/policy.py:74-80) + log-softmax + sample + log_prob
// (agents/ppo.py:77-79); results also packed [n][3] = {act, logp, value} for ONE read-back.
// 16 envs per workgroup: feature rows AND the (A+1) x H head matrix go through LDS, thread (env, output) owns one dot
// product and then one ACTION of the normalisation: the exp / log terms are computed one per lane, every sum is still
// taken in action order 0..A-1 (each lane re-adds the terms from LDS), so the numbers are those of the sequential
// log_softmax_twice + CDF walk of sample_kernel.
// WIDE (H > 256: IMPALA output_dim up to 512, any MLP latent_size): features and head rows are staged in K chunks of 256 through the
// same LDS rows, each dot product carried across the chunks in the same order of sums as the single-chunk loop (whether the
// four products of a step are fused is the compiler's choice per loop: as built, the H == 256 loop fuses them, the others do not).
// LSE (mi_config.value_from_logits): the value is mx + log(s1) of the first normalisation below -- the same sums in the same order as
// log_softmax_twice_t<true>, so GIVEN THE SAME LOGITS it is the number sample_kernel / logp_all_kernel / the loss compute.  This kernel's
// logits are its own dot products, taken in another order than the GEMM's that feeds those kernels, so across the two paths the values
// agree to a few ulp, not bit for bit (as the logits do with the flag off).  Column A of hout stays fc_value's output.
template <bool WIDE, bool LSE>
__global__ __launch_bounds__(256) void heads_sample_kernel(const float* __restrict__ feat, const float* __restrict__ Wh,
                                                           const float* __restrict__ bh, int n, int H, int A, const float* u,
                                                           unsigned long long seed, unsigned long long ctr, int32_t* act,
                                                           float* logp, float* value, float* pack, float* hout,
                                                           const float* rd, float* rew_dst, float* done_dst,
                                                           unsigned* done_ctr, unsigned* host_flag, unsigned ticket) {
    __shared__ __attribute__((aligned(16))) float s_f[16 * 260];
    __shared__ __attribute__((aligned(16))) float s_w[17 * 260];
    __shared__ float s_z[16 * 17];
    const int tid = threadIdx.x, e0 = blockIdx.x * 16;
    const int el = tid >> 4, o = tid & 15, e = e0 + el;
    float rwd = 0.f, dn = 0.f;
    if (rd && o == 0 && e < n) { rwd = rd[e]; dn = rd[n + e]; }          // (host-visible staging) issued first: latency hidden by the dots
    if constexpr (WIDE) {
        float acc0 = 0.f, acc1 = 0.f;                     // outputs o and (o == 0 only, A + 1 == 17) 16
        for (int c0 = 0; c0 < H; c0 += 256) {
            const int HC = H - c0 < 256 ? H - c0 : 256;
            __syncthreads();                              // (every thread is done with the previous chunk)
            if ((H & 3) == 0) {
                const int H4 = HC >> 2;
                for (int k = tid; k < 16 * H4; k += 256) {
                    const int r = k / H4, kk = (k % H4) * 4;
                    *(f32x4*)(s_f + r * 260 + kk) = (e0 + r < n) ? *(const f32x4*)(feat + (long long)(e0 + r) * H + c0 + kk) : (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                for (int k = tid; k < (A + 1) * H4; k += 256) {
                    const int r = k / H4, kk = (k % H4) * 4;
                    *(f32x4*)(s_w + r * 260 + kk) = *(const f32x4*)(Wh + (long long)r * H + c0 + kk);
                }
            } else {
                for (int k = tid; k < 16 * HC; k += 256) { const int r = k / HC, kk = k % HC; s_f[r * 260 + kk] = (e0 + r < n) ? feat[(long long)(e0 + r) * H + c0 + kk] : 0.f; }
                for (int k = tid; k < (A + 1) * HC; k += 256) { const int r = k / HC, kk = k % HC; s_w[r * 260 + kk] = Wh[(long long)r * H + c0 + kk]; }
            }
            __syncthreads();
            auto dot = [&](int oo, float acc) {
                const float* w = s_w + oo * 260;
                const float* f = s_f + el * 260;
                int k = 0;
                for (; k + 4 <= HC; k += 4) {
                    const f32x4 fv = *(const f32x4*)(f + k), ww = *(const f32x4*)(w + k);
                    acc += fv.x * ww.x + fv.y * ww.y + fv.z * ww.z + fv.w * ww.w;
                }
                for (; k < HC; ++k) acc += f[k] * w[k];
                return acc;
            };
            if (o <= A) acc0 = dot(o, acc0);
            if (o + 16 <= A) acc1 = dot(o + 16, acc1);
        }
        if (o <= A) s_z[el * 17 + o] = acc0 + bh[o];
        if (o + 16 <= A) s_z[el * 17 + o + 16] = acc1 + bh[o + 16];
    } else {
    if (H == 256) {
        // the IMPALA width: all 9 loads of a thread are issued before the first LDS store (the general loop below divides by a
        // run-time H and waits for every load before the next: 9 memory latencies in a row, half of this kernel's time)
        f32x4 rf[4], rw[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = tid + j * 256, r = k >> 6, kk = (k & 63) * 4;
            rf[j] = (e0 + r < n) ? *(const f32x4*)(feat + (long long)(e0 + r) * 256 + kk) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = tid + j * 256, r = k >> 6, kk = (k & 63) * 4;
            rw[j] = (r <= A) ? *(const f32x4*)(Wh + (long long)r * 256 + kk) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int k = tid + j * 256; *(f32x4*)(s_f + (k >> 6) * 260 + (k & 63) * 4) = rf[j]; }
#pragma unroll
        for (int j = 0; j < 5; ++j) { const int k = tid + j * 256; if ((k >> 6) <= A) *(f32x4*)(s_w + (k >> 6) * 260 + (k & 63) * 4) = rw[j]; }
    } else if ((H & 3) == 0) {
        const int H4 = H >> 2;
        for (int k = tid; k < 16 * H4; k += 256) {
            const int r = k / H4, kk = (k % H4) * 4;
            *(f32x4*)(s_f + r * 260 + kk) = (e0 + r < n) ? *(const f32x4*)(feat + (long long)(e0 + r) * H + kk) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        for (int k = tid; k < (A + 1) * H4; k += 256) {
            const int r = k / H4, kk = (k % H4) * 4;
            *(f32x4*)(s_w + r * 260 + kk) = *(const f32x4*)(Wh + (long long)r * H + kk);
        }
    } else {
        for (int k = tid; k < 16 * H; k += 256) { const int r = k / H, kk = k % H; s_f[r * 260 + kk] = (e0 + r < n) ? feat[(long long)(e0 + r) * H + kk] : 0.f; }
        for (int k = tid; k < (A + 1) * H; k += 256) { const int r = k / H, kk = k % H; s_w[r * 260 + kk] = Wh[(long long)r * H + kk]; }
    }
    __syncthreads();
    for (int oo = o; oo <= A; oo += 16) {                 // A+1 <= 17 outputs: output 16 (if any) is taken by o == 0
        const float* w = s_w + oo * 260;
        const float* f = s_f + el * 260;
        float acc = 0.f;
        int k = 0;
        if (H == 256) {                                   // same order of operations, LDS reads of 8 steps in flight
#pragma unroll 8
            for (; k < 256; k += 4) {
                const f32x4 fv = *(const f32x4*)(f + k), ww = *(const f32x4*)(w + k);
                acc += fv.x * ww.x + fv.y * ww.y + fv.z * ww.z + fv.w * ww.w;
            }
        }
        for (; k + 4 <= H; k += 4) {
            const f32x4 fv = *(const f32x4*)(f + k), ww = *(const f32x4*)(w + k);
            acc += fv.x * ww.x + fv.y * ww.y + fv.z * ww.z + fv.w * ww.w;
        }
        for (; k < H; ++k) acc += f[k] * w[k];
        s_z[el * 17 + oo] = acc + bh[oo];
    }
    }
    __syncthreads();
    // The 16 lanes of an env sit in one wave (lane = 16*(el & 3) + o).  A lane publishes its term in the env's 64-byte LDS row and
    // reads the whole row back with four 16-byte reads (same wave: LDS executes a wave's operations in order, no barrier), then adds
    // the A terms in action order from registers.  (A run-time loop of 15 ds_bpermute + add, each waiting for the previous, was ~40 %
    // of this kernel: six such loops.)
    __shared__ __attribute__((aligned(16))) float s_t[16 * 16];
    const bool lane_on = o < A;
    auto row = [&](float term, float (&v)[16]) {
        __builtin_amdgcn_wave_barrier();
        s_t[el * 16 + o] = term;
        __builtin_amdgcn_wave_barrier();
        const f32x4 a0 = *(const f32x4*)(s_t + el * 16), a1 = *(const f32x4*)(s_t + el * 16 + 4);
        const f32x4 a2 = *(const f32x4*)(s_t + el * 16 + 8), a3 = *(const f32x4*)(s_t + el * 16 + 12);
        v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
        v[8] = a2.x; v[9] = a2.y; v[10] = a2.z; v[11] = a2.w; v[12] = a3.x; v[13] = a3.y; v[14] = a3.z; v[15] = a3.w;
    };
    auto group_sum = [&](float term) {                    // sum over the env's A lanes, in action order
        float v[16];
        row(term, v);
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < A) t += v[k];
        return t;
    };
    const float z = lane_on ? s_z[el * 17 + o] : 0.f;
    float mx;
    {
        float v[16];
        row(z, v);
        mx = v[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) if (k < A) mx = fmaxf(mx, v[k]);
    }
    const float s1 = group_sum(lane_on ? expf(z - mx) : 0.f);
    const float lse1 = mx + logf(s1);
    float lp = z - lse1;
    const float s2 = group_sum(lane_on ? expf(lp) : 0.f);
    lp -= logf(s2);                                        // Categorical(logits=log_probs) normalises again (policy.py:86-87)
    const float pr = lane_on ? expf(lp) : 0.f;
    float cdf = 0.f;
    {
        float v[16];
        row(pr, v);
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < A) cdf += (k <= o) ? v[k] : 0.f;      // prefix in action order
    }
    const float uu = (e < n) ? (u ? u[e] : philox_uniform(seed, ctr + e)) : 0.f;
    const float mark = (lane_on && cdf <= uu) ? (float)(o + 1) : 0.f;
    float sel = 0.f;
    {
        float v[16];
        row(mark, v);
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < A) sel = fmaxf(sel, v[k]);
    }
    int a_sel = (int)sel;
    if (a_sel > A - 1) a_sel = A - 1;
    float lp_pick;
    {
        float v[16];
        row(lp, v);
        lp_pick = v[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) lp_pick = (k == a_sel) ? v[k] : lp_pick;
    }
    if (o == 0 && e < n) {
        const float lp_sel = lp_pick, val = LSE ? lse1 : s_z[el * 17 + A];
        if (rd) { rew_dst[e] = rwd; done_dst[e] = dn; }        // previous step's reward / done into the (T,E) arrays
        if (act) act[e] = a_sel;
        if (logp) logp[e] = lp_sel;
        if (value) value[e] = val;
        if (pack) { pack[e * 3] = (float)a_sel; pack[e * 3 + 1] = lp_sel; pack[e * 3 + 2] = val; }
        if (hout) for (int k = 0; k <= A; ++k) hout[(long long)e * (A + 1) + k] = s_z[el * 17 + k];
    }
    if (host_flag) {
        // completion ticket in host-visible memory, written by the LAST workgroup after every workgroup's results are visible system-
        // wide: the host spins on it instead of waiting for the stream (hipStreamSynchronize returns ~5 us later: scratch/synclat.hip)
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned old = atomicAdd(done_ctr, 1u);
            if (old == gridDim.x - 1) {
                *done_ctr = 0;
                __threadfence_system();
                __hip_atomic_store(host_flag, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}
void launch_heads_sample(const float* feat, const float* Wh, const float* bh, int n, int H, int A, const float* u,
                         unsigned long long seed, unsigned long long ctr, int32_t* act, float* logp, float* value, float* pack,
                         float* hout, const float* rd, float* rew_dst, float* done_dst, hipStream_t st,
                         unsigned* done_ctr, unsigned* host_flag, unsigned ticket, int value_from_logits) {
    if (n <= 0) return;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((n + 15) / 16), dim3(256), 0, st, feat, Wh, bh, n, H, A, u, seed, ctr, act, logp, value, pack, hout,
                           rd, rew_dst, done_dst, done_ctr, host_flag, ticket);
    };
    if (value_from_logits) { if (H > 256) go(heads_sample_kernel<true, true>); else go(heads_sample_kernel<false, true>); }
    else if (H > 256) go(heads_sample_kernel<true, false>);
    else go(heads_sample_kernel<false, false>);
}
void launch_sample(const float* hout, int n, int A, const float* u, unsigned long long seed, unsigned long long ctr,
                   int32_t* act, float* logp, float* value, hipStream_t st, int value_from_logits) {
    if (n <= 0) return;
    if (value_from_logits) hipLaunchKernelGGL(sample_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, st, hout, n, A, u, seed, ctr, act, logp, value);
    else hipLaunchKernelGGL(sample_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, st, hout, n, A, u, seed, ctr, act, logp, value);
}
