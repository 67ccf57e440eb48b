// Sparse-autoencoder agent (reference agents/sae.py, common/model.py:1623-1667) on an existing IMPALA context: a sparse autoencoder
// on the 2048 block-3 features of the FROZEN policy (stage 1) and a linear probe that acts from its codes (stage 2).  All SAE / probe
// arithmetic is fp32 (the policy's forward pass runs in the context's precision); nothing here touches the PPO path's buffers
// except the activation buffers a forward pass fills anyway and the context's own value / action rings.
//
// Device layouts.  The engine keeps block 3's output pixel-major ([n][8][8][32], column p*32 + ch) where the reference's Flatten() on
// NCHW gives ch*64 + p: the encoder's 2048 input columns, the decoder's 2048 rows / biases and the feature ring are kept in the
// device order and permuted at the host boundary, exactly as embedder.fc.weight is (engine.hip to_device_layout, K_FCW).
//   SAE vector   {W_e [S][2048], b_e [S], W_d [2048][S], b_d [2048]}
//   probe vector {W [(A+1)][S] = fc_policy rows then the fc_value row, b [A+1]}      (host: fc_policy.weight, .bias, fc_value.weight, .bias)
// The GEMMs are the engine's generic fp32-MFMA kernel (gemm.hip gemm_kernel).  The forward products never split K (GemmArgs.ws null):
// launch_gemm picks its split from the number of output tiles, i.e. from n, and a row's codes must not depend on n or on its
// neighbours; without a split a row is one fixed-order sum over K whatever the batch.  The weight gradients (K = n) may split.
#include "engine_ctx.h"
#include "device_util.h"

namespace {
constexpr int D = 2048;            // encoded_dim = latent_dim * 8 * 8 (common/model.py:175)
constexpr int COLSUM_GROUPS = 256; // row groups of the column mean's first pass
}

struct mi_sae {
    int S = 0; float rho = 0.f;
    int64_t n_sae = 0, n_probe = 0;
    float *p[2] = {}, *g[2] = {}, *m[2] = {}, *v[2] = {};      // [0] SAE, [1] probe: parameters, gradients, Adam moments
    float *ring_h = nullptr, *ring_l = nullptr;                 // features [T+1][E][2048] (device column order), policy logits [T][E][A]
    float *X = nullptr, *enc = nullptr, *rec = nullptr, *dEnc = nullptr, *pout = nullptr, *pdY = nullptr, *step_h = nullptr;
    double *col_part = nullptr, *red_part = nullptr, *sumsq = nullptr;
    float *kl_term = nullptr, *seed = nullptr, *log = nullptr, *gnorm = nullptr;
    int32_t* h_idx = nullptr; hipEvent_t ev_idx = nullptr; bool idx_pending = false;
    float* h_log = nullptr;
    unsigned long long counter = 0;                             // Philox counter of the NEXT mi_sae_step (advances by E per call)
    std::vector<int64_t> map[2];                                // device index of host element i
    // the context holds the state (mi_ctx::sae): mi_sae_create makes it, mi_sae_destroy or mi_destroy (sae_release) lets go of it
    DevPool pool{hip_pool()};                                    // owns every buffer and the event above (declared last: destroyed first)
};

// ------------------------------------------------------------------------------------------ kernels
// hidden = ReLU(block-3 output) (common/model.py:186-196), fp32, device column order
__global__ __launch_bounds__(256) void sae_hidden_kernel(const void* p2, int bf16, float* dst, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float v = bf16 ? __uint_as_float(((unsigned)((const unsigned short*)p2)[e]) << 16) : ((const float*)p2)[e];
    dst[e] = fmaxf(v, 0.f);
}

// X[s] = ring[idx[s]]: one float4 per thread (512 per row)
__global__ __launch_bounds__(256) void sae_gather_kernel(const float4* ring, const int32_t* idx, float4* X, int n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n * (D / 4)) return;
    const int s = (int)(e / (D / 4)), q = (int)(e % (D / 4));
    X[e] = ring[(long long)idx[s] * (D / 4) + q];
}

// recon_loss = mean((rec - x)^2) (agents/sae.py:152): block partial sums in fp64, and the gradient seed dRec = 2 (rec - x) / (n * 2048)
// written over rec
__global__ __launch_bounds__(256) void sae_recon_kernel(float4* rec, const float4* X, long long total4, float scale, double* part) {
    __shared__ double sb[4];
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long long)gridDim.x * 256) {
        float4 r = rec[e];
        const float4 x = X[e];
        r.x -= x.x; r.y -= x.y; r.z -= x.z; r.w -= x.w;
        s += (double)r.x * r.x; s += (double)r.y * r.y; s += (double)r.z * r.z; s += (double)r.w * r.w;
        r.x *= scale; r.y *= scale; r.z *= scale; r.w *= scale;
        rec[e] = r;
    }
    const double t = block_sum256(s, sb);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// rho_hat_j = mean_b enc[b][j] (SparseAutoencoder.kl_divergence, common/model.py:1645-1653), first pass: row group rg = 4 * blockIdx.y +
// (threadIdx.x >> 6) sums rows rg, rg + groups, ... of column j in row order
__global__ __launch_bounds__(256) void sae_colsum_kernel(const float* enc, int n, int S, double* part) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), rg = blockIdx.y * 4 + (threadIdx.x >> 6), groups = gridDim.y * 4;
    if (j >= S) return;
    double s = 0.0;
    for (int b = rg; b < n; b += groups) s += (double)enc[(long long)b * S + j];
    part[(long long)rg * S + j] = s;
}
// second pass: the column's mean, its KL term and the seed of its gradient into dEnc,
//   d/d rho_hat_j [rho log((rho+eps)/(rho_hat_j+eps)) + (1-rho) log((1-rho+eps)/(1-rho_hat_j+eps))] = -rho/(rho_hat_j+eps) + (1-rho)/(1-rho_hat_j+eps),
// times sparse_coef / n (the mean over the batch).  rho_hat_j >= 1 gives the NaN torch gives: nothing is clamped.
__global__ __launch_bounds__(256) void sae_kl_kernel(const double* part, int groups, int n, int S, double rho, double coef, float* kl_term, float* seed) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    double s = 0.0;
    for (int r = 0; r < groups; ++r) s += part[(long long)r * S + j];
    const double rh = s / (double)n, eps = 1e-10;
    kl_term[j] = (float)(rho * log((rho + eps) / (rh + eps)) + (1.0 - rho) * log((1.0 - rho + eps) / (1.0 - rh + eps)));
    seed[j] = (float)(coef * (-rho / (rh + eps) + (1.0 - rho) / (1.0 - rh + eps)) / (double)n);
}
// dEnc[b][j] += seed_j where the unit is active (ReLU's gradient: enc > 0)
__global__ __launch_bounds__(256) void sae_seed_kernel(float* dEnc, const float* enc, const float* seed, long long total, int S) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    if (enc[e] > 0.f) dEnc[e] += seed[(int)(e % S)];
}
// one workgroup: recon = sum(part) / (n * 2048), KL = sum_j kl_term_j, loss = recon + sparse_coef * KL  -> log {recon, KL, loss}
__global__ __launch_bounds__(256) void sae_finish_kernel(const double* part, int nblk, const float* kl_term, int S, double inv_count, float coef, float* log) {
    __shared__ double sb[4];
    double a = 0.0, k = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) a += part[i];
    for (int j = threadIdx.x; j < S; j += 256) k += (double)kl_term[j];
    a = block_sum256(a, sb);
    k = block_sum256(k, sb);
    if (threadIdx.x == 0) {
        const float recon = (float)(a * inv_count), kl = (float)k;
        log[0] = recon; log[1] = kl; log[2] = recon + coef * kl;
    }
}

// optimize_linear_model's losses (agents/sae.py:196-200), one thread per row.  out[b] = {logits z [A], v_hat}.
//   logit_loss = KLDivLoss(batchmean)(log_softmax(z), softmax(l)) = sum_b sum_k p_bk (log p_bk - lhat_bk) / n, l = the stored policy logits;
//   dz_bk = (q_bk sum_k p_bk - p_bk) / n  (log_softmax's backward of -p / n), q = softmax(z).
// Block partials (fp64): {KL sum, sum v_hat, sum v_hat^2, sum v, sum v^2}; the value column's gradient needs the batch mean of v and is
// written by sae_probe_value_kernel.
__global__ __launch_bounds__(256) void sae_probe_loss_kernel(const float* out, const float* ring_l, const float* value, const int32_t* idx, int n, int A,
                                                             float* dY, double* part) {
    __shared__ double sb[4];
    const int b = blockIdx.x * 256 + threadIdx.x;
    double kl = 0.0, vh = 0.0, vv = 0.0;
    if (b < n) {
        const float* z = out + (long long)b * (A + 1);
        const float* l = ring_l + (long long)idx[b] * A;
        float zm = z[0], lm = l[0];
        for (int k = 1; k < A; ++k) { zm = fmaxf(zm, z[k]); lm = fmaxf(lm, l[k]); }
        float zs = 0.f, ls = 0.f;
        for (int k = 0; k < A; ++k) { zs += expf(z[k] - zm); ls += expf(l[k] - lm); }
        const float zl = zm + logf(zs), ll = lm + logf(ls);
        float psum = 0.f;
        for (int k = 0; k < A; ++k) psum += expf(l[k] - ll);
        const float inv_n = 1.f / (float)n;
        for (int k = 0; k < A; ++k) {
            const float lp = l[k] - ll, p = expf(lp), lhat = z[k] - zl;
            if (p > 0.f) kl += (double)(p * (lp - lhat));      // xlogy: a zero target contributes nothing
            dY[(long long)b * (A + 1) + k] = (expf(lhat) * psum - p) * inv_n;
        }
        vh = (double)z[A]; vv = (double)value[idx[b]];
    }
    const double s0 = block_sum256(kl, sb), s1 = block_sum256(vh, sb), s2 = block_sum256(vh * vh, sb), s3 = block_sum256(vv, sb),
                 s4 = block_sum256(vv * vv, sb);
    if (threadIdx.x == 0) { double* q = part + (long long)blockIdx.x * 5; q[0] = s0; q[1] = s1; q[2] = s2; q[3] = s3; q[4] = s4; }
}
// The reference writes value_loss = ((value_hat - value_batch)**2).mean() with value_hat (n,1) and value_batch (n,): the difference
// broadcasts to (n,n), so the loss is the mean over ALL n^2 pairs (i, j) of (v_hat_i - v_j)^2 -- not the per-sample error.  That
// expression is reproduced, in O(n) from the batch sums:  mean(v_hat^2) - 2 mean(v_hat) mean(v) + mean(v^2), gradient 2 (v_hat_i - mean(v)) / n.
// One workgroup: log {value_loss, logit_loss, loss}, stat[0] = mean(v) (fp64: col_part is free in this pass), and fc_value.bias's gradient.
__global__ __launch_bounds__(256) void sae_probe_finish_kernel(const double* part, int nblk, int n, float* log, double* stat, float* gb_value) {
    __shared__ double sb[4];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256)
        for (int q = 0; q < 5; ++q) s[q] += part[(long long)i * 5 + q];
    for (int q = 0; q < 5; ++q) s[q] = block_sum256(s[q], sb);
    if (threadIdx.x == 0) {
        const double inv = 1.0 / (double)n, mvh = s[1] * inv, mv = s[3] * inv;
        const float vloss = (float)(s[2] * inv - 2.0 * mvh * mv + s[4] * inv), lloss = (float)(s[0] * inv);
        log[0] = vloss; log[1] = lloss; log[2] = lloss + vloss;
        stat[0] = mv;
        gb_value[0] += (float)(2.0 * (mvh - mv));      // fc_value.bias: sum_i 2 (v_hat_i - mean(v)) / n, from the fp64 batch sums
    }
}
__global__ __launch_bounds__(256) void sae_probe_value_kernel(const float* out, const double* stat, int n, int A, float* dY) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    dY[(long long)b * (A + 1) + A] = (float)(2.0 * ((double)out[(long long)b * (A + 1) + A] - stat[0]) / (double)n);
}

// clip_grad_norm_ + optim.Adam(eps=1e-5).step() + zero_grad() on one flat vector: optim.hip's adam_kernel with torch's own constants.
// torch computes 1 - beta1 and 1 - beta2 in Python (float64) and hands the kernels the ROUNDED results, 0.1f and 0.001f; adam_kernel
// subtracts in fp32, 1.f - 0.999f = 0.000999987: exp_avg_sq 1.3e-5 and the step 6.5e-6 (relative) away from torch's -- inside the PPO
// tests' absolute bounds, 20 x outside this agent's (8 x torch's own fp32 error, tests/test_gpu_sae.py).  The PPO path's kernel stays
// as it is (its numbers are pinned); w1 / w2 are (float)(1.0 - beta).  sumsq: the 128 partial sums of launch_sumsq_partials.
__global__ __launch_bounds__(256) void sae_adam_kernel(float* p, float* g, float* m, float* v, long long n, const double* sumsq, float max_norm, float w1,
                                                       float beta2, float w2, float eps, float step_size, float bc2_sqrt, float* gnorm_out) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double t = 0.0;
    for (int q = threadIdx.x & 63; q < 128; q += 64) t += sumsq[q];
    t = wave_sum(t);
    const float norm = (float)sqrt(__shfl(t, 0, 64));
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
    if (k == 0 && gnorm_out) gnorm_out[0] = norm;
    if (k >= n) return;
    const float gk = g[k] * coef;
    float mk = m[k], vk = v[k];
    mk = mk + w1 * (gk - mk);                            // exp_avg.lerp_(grad, 1 - beta1)
    vk = vk * beta2 + (w2 * gk) * gk;                    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vk) / bc2_sqrt + eps;
    p[k] = p[k] + (-step_size) * (mk / denom);           // param.addcdiv_(exp_avg, denom, value=-step_size)
    m[k] = mk; v[k] = vk;
    g[k] = 0.f;                                          // optimizer.zero_grad()
}
void launch_sae_adam(float* p, float* g, float* m, float* v, long long n, const double* sumsq, float max_norm, float w1, float beta2, float w2,
                     float eps, float step_size, float bc2_sqrt, float* gnorm_out, hipStream_t st) {
    hipLaunchKernelGGL(sae_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, g, m, v, n, sumsq, max_norm, w1, beta2, w2, eps,
                       step_size, bc2_sqrt, gnorm_out);
}

// ------------------------------------------------------------------------------------------ host helpers
static void sae_gemm(mi_ctx* c, const float* A, long long sam, const float* B, long long sbk, long long sbn, float* C, int M, int N, int K,
                     const float* bias, int relu_out, const float* mask) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K;
    g.sam = sam; g.sak = 1; g.sbk = sbk; g.sbn = sbn; g.ldc = N;
    g.bias = bias; g.relu_out = relu_out; g.mask = mask;
    g.ws = nullptr; g.ws_floats = 0;          // never split K: see the head of this file
    launch_gemm(g, c->stream);
}
static inline float* sae_We(mi_sae* s) { return s->p[0]; }
static inline float* sae_be(mi_sae* s) { return s->p[0] + (size_t)s->S * D; }
static inline float* sae_Wd(mi_sae* s) { return s->p[0] + (size_t)s->S * D + s->S; }
static inline float* sae_bd(mi_sae* s) { return s->p[0] + (size_t)2 * s->S * D + s->S; }
// enc = relu(x W_e^T + b_e), n rows
static void sae_encode(mi_ctx* c, const float* x, float* enc, int n) {
    mi_sae* s = c->sae;
    sae_gemm(c, x, D, sae_We(s), 1, D, enc, n, s->S, D, sae_be(s), 1, nullptr);
}
static void sae_decode(mi_ctx* c, const float* enc, float* rec, int n) {
    mi_sae* s = c->sae;
    sae_gemm(c, enc, s->S, sae_Wd(s), 1, s->S, rec, n, D, s->S, sae_bd(s), 0, nullptr);
}
static void sae_probe_fwd(mi_ctx* c, const float* enc, float* out, int n) {
    mi_sae* s = c->sae;
    sae_gemm(c, enc, s->S, s->p[1], 1, s->S, out, n, c->A + 1, s->S, s->p[1] + (size_t)(c->A + 1) * s->S, 0, nullptr);
}

static void sae_build_maps(mi_ctx* c) {
    mi_sae* s = c->sae;
    const int64_t S = s->S, A = c->A;
    auto dcol = [](int64_t h) { return (h % 64) * 32 + h / 64; };      // host column ch*64 + p -> device column p*32 + ch
    std::vector<int64_t>& a = s->map[0];
    a.resize(s->n_sae);
    int64_t i = 0;
    for (int64_t o = 0; o < S; ++o) for (int64_t h = 0; h < D; ++h) a[i++] = o * D + dcol(h);
    for (int64_t o = 0; o < S; ++o) a[i++] = S * D + o;
    for (int64_t h = 0; h < D; ++h) for (int64_t o = 0; o < S; ++o) a[i++] = S * D + S + dcol(h) * S + o;
    for (int64_t h = 0; h < D; ++h) a[i++] = 2 * S * D + S + dcol(h);
    std::vector<int64_t>& b = s->map[1];
    b.resize(s->n_probe);
    i = 0;
    for (int64_t k = 0; k < A * S; ++k) b[i++] = k;                     // fc_policy.weight
    for (int64_t k = 0; k < A; ++k) b[i++] = (A + 1) * S + k;           // fc_policy.bias
    for (int64_t k = 0; k < S; ++k) b[i++] = A * S + k;                 // fc_value.weight
    b[i++] = (A + 1) * S + A;                                           // fc_value.bias
}
static int sae_upload(mi_ctx* c, int which, float* dbuf, const float* flat, int64_t n) {
    mi_sae* s = c->sae;
    ARG(flat, "null"); ARG(n == (which ? s->n_probe : s->n_sae), "flat vector length != mi_sae_param_count"); JOIN(c);
    std::vector<float> tmp(n);
    const std::vector<int64_t>& mp = s->map[which];
    for (int64_t i = 0; i < n; ++i) tmp[mp[i]] = flat[i];
    HIPC(hipMemcpyAsync(dbuf, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
static int sae_download(mi_ctx* c, int which, const float* dbuf, float* flat, int64_t n) {
    mi_sae* s = c->sae;
    ARG(flat, "null"); ARG(n == (which ? s->n_probe : s->n_sae), "flat vector length != mi_sae_param_count"); JOIN(c);
    std::vector<float> tmp(n);
    HIPC(hipMemcpyAsync(tmp.data(), dbuf, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    const std::vector<int64_t>& mp = s->map[which];
    for (int64_t i = 0; i < n; ++i) flat[i] = tmp[mp[i]];
    return 0;
}
#define SAE_CTX(c, which) ARG(c, "null"); mi_sae* const s = c->sae; ARG(s, "no SAE on this context: call mi_sae_create first"); ARG((which) == 0 || (which) == 1, "which must be 0 (SAE) or 1 (probe)")

// minibatch indices -> c->d_idx through the SAE's pinned buffer (rewritten only after the copy that read it has completed)
static int sae_stage_idx(mi_ctx* c, const int64_t* idx, int n) {
    mi_sae* s = c->sae;
    const int64_t N = (int64_t)c->T * c->E;
    for (int k = 0; k < n; ++k) ARG(idx[k] >= 0 && idx[k] < N, "minibatch index out of range [0, T*E)");
    if (s->idx_pending) { HIPC(hipEventSynchronize(s->ev_idx)); s->idx_pending = false; }
    for (int k = 0; k < n; ++k) s->h_idx[k] = (int32_t)idx[k];
    HIPC(hipMemcpyAsync(c->d_idx, s->h_idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPC(hipEventRecord(s->ev_idx, c->stream)); s->idx_pending = true;
    return 0;
}
static int sae_read_log(mi_ctx* c, float* log_out) {
    mi_sae* s = c->sae;
    HIPC(hipGetLastError()); NETCHK(c);
    if (log_out) {
        HIPC(hipMemcpyAsync(s->h_log, s->log, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        memcpy(log_out, s->h_log, 3 * sizeof(float));
    }
    return 0;
}

void sae_release(mi_ctx* c) {
    if (!c->sae) return;
    hipDeviceSynchronize();      // (not the context's stream alone: the pool lets go of the pinned buffers and the event first)
    delete c->sae;
    c->sae = nullptr;
}

// ------------------------------------------------------------------------------------------ C ABI
int mi_sae_create(mi_ctx* c, int32_t sae_dim, float rho) {
    ARG(c, "null"); JOIN(c);
    ARG(!c->sae, "this context already has an SAE");
    ARG(c->cfg.arch == MI_ARCH_IMPALA, "the SAE agent needs an IMPALA context (encoded_dim / forward_to_pool exist only on ImpalaModel); arch mlp is not supported");
    ARG(!c->gru_on, "the SAE agent is non-recurrent: a context with a GRU set (recurrent policy) is not supported");
    ARG(c->comm_world <= 1 && c->multirank == 0, "the SAE agent is single-GPU: a multi-rank context (world size > 1) is not supported");
    ARG(c->n_groups <= 1, "the SAE agent runs serial rollout steps: a context with env groups (rollout_groups > 1) is not supported");
    ARG(sae_dim >= 64 && sae_dim <= 4096 && sae_dim % 64 == 0, "sae_dim must be a multiple of 64 in [64, 4096]");
    mi_sae* s = c->sae = new mi_sae();
    s->S = sae_dim; s->rho = rho;
    const size_t S = sae_dim, A = c->A, T = c->T, E = c->E, NB = c->NB;
    s->n_sae = (int64_t)(2 * S * D + S + D); s->n_probe = (int64_t)((A + 1) * S + A + 1);
    auto all = [&]() -> int {
        DevPool& m = s->pool;
        for (int w = 0; w < 2; ++w) {
            const size_t n = w ? s->n_probe : s->n_sae;
            HIPC(m.dev(&s->p[w], n)); HIPC(m.dev(&s->g[w], n)); HIPC(m.dev(&s->m[w], n)); HIPC(m.dev(&s->v[w], n));
        }
        HIPC(m.dev(&s->ring_h, (T + 1) * E * D)); HIPC(m.dev(&s->ring_l, T * E * A));
        HIPC(m.dev(&s->X, NB * D)); HIPC(m.dev(&s->rec, NB * D)); HIPC(m.dev(&s->enc, NB * S)); HIPC(m.dev(&s->dEnc, NB * S));
        HIPC(m.dev(&s->pout, NB * (A + 1))); HIPC(m.dev(&s->pdY, NB * (A + 1))); HIPC(m.dev(&s->step_h, E * D));
        HIPC(m.dev(&s->col_part, (size_t)COLSUM_GROUPS * S)); HIPC(m.dev(&s->red_part, (size_t)1024 * 5)); HIPC(m.dev(&s->sumsq, 128));
        HIPC(m.dev(&s->kl_term, S)); HIPC(m.dev(&s->seed, S)); HIPC(m.dev(&s->log, 8)); HIPC(m.dev(&s->gnorm, 2));
        HIPC(m.pinned(&s->h_idx, NB * sizeof(int32_t), hipHostMallocDefault)); HIPC(m.pinned(&s->h_log, 8 * sizeof(float), hipHostMallocDefault));
        HIPC(m.event(&s->ev_idx, hipEventDisableTiming));
        return 0;
    };
    if (int r = all()) { sae_release(c); return r; }
    sae_build_maps(c);
    return 0;
}

int mi_sae_destroy(mi_ctx* c) { ARG(c, "null"); JOIN(c); sae_release(c); return 0; }
int64_t mi_sae_param_count(mi_ctx* c, int32_t which) { mi_sae* s = c ? c->sae : nullptr; return (s && (which == 0 || which == 1)) ? (which ? s->n_probe : s->n_sae) : -1; }
int mi_sae_set_params(mi_ctx* c, int32_t which, const float* flat, int64_t n) { SAE_CTX(c, which); return sae_upload(c, which, s->p[which], flat, n); }
int mi_sae_get_params(mi_ctx* c, int32_t which, float* flat, int64_t n) { SAE_CTX(c, which); return sae_download(c, which, s->p[which], flat, n); }
int mi_sae_get_grads(mi_ctx* c, int32_t which, float* flat, int64_t n) { SAE_CTX(c, which); return sae_download(c, which, s->g[which], flat, n); }
int mi_sae_set_adam_state(mi_ctx* c, int32_t which, const float* m, const float* v, int64_t n) {
    SAE_CTX(c, which);
    if (int r = sae_upload(c, which, s->m[which], m, n)) return r;
    return sae_upload(c, which, s->v[which], v, n);
}
int mi_sae_get_adam_state(mi_ctx* c, int32_t which, float* m, float* v, int64_t n) {
    SAE_CTX(c, which);
    if (int r = sae_download(c, which, s->m[which], m, n)) return r;
    return sae_download(c, which, s->v[which], v, n);
}

int mi_sae_put_ring(mi_ctx* c, int32_t t, const float* hidden, const float* logits) {
    SAE_CTX(c, 0); JOIN(c); ARG(t >= 0 && t <= c->T, "t out of range"); ARG(!logits || t < c->T, "step T stores hidden and value only");
    const size_t E = c->E;
    if (hidden) {
        std::vector<float> tmp(E * D);
        for (size_t e = 0; e < E; ++e)
            for (int h = 0; h < D; ++h) tmp[e * D + (h % 64) * 32 + h / 64] = hidden[e * D + h];
        HIPC(hipMemcpyAsync(s->ring_h + (size_t)t * E * D, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    if (logits) {
        HIPC(hipMemcpyAsync(s->ring_l + (size_t)t * E * c->A, logits, E * c->A * 4, hipMemcpyHostToDevice, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    return 0;
}
int mi_sae_get_hidden(mi_ctx* c, int32_t t, float* out) {
    SAE_CTX(c, 0); JOIN(c); ARG(out, "null"); ARG(t >= -1 && t <= c->T, "t out of range");
    const size_t E = c->E;
    std::vector<float> tmp(E * D);
    HIPC(hipMemcpyAsync(tmp.data(), t < 0 ? s->step_h : s->ring_h + (size_t)t * E * D, tmp.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (size_t e = 0; e < E; ++e)
        for (int h = 0; h < D; ++h) out[e * D + h] = tmp[e * D + (h % 64) * 32 + h / 64];
    return 0;
}
int mi_sae_get_logits(mi_ctx* c, int32_t t, float* out) {
    SAE_CTX(c, 0); JOIN(c); ARG(out, "null"); ARG(t >= -1 && t < c->T, "t out of range");
    HIPC(hipMemcpyAsync(out, t < 0 ? c->d_lp : s->ring_l + (size_t)t * c->E * c->A, (size_t)c->E * c->A * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}

// SAE.get_hidden_and_acts (agents/sae.py:73-86)
int mi_sae_step(mi_ctx* c, int32_t t, const void* obs, size_t bytes, int32_t act_from_probe, int32_t store, uint64_t seed, const float* u,
                int64_t* act_out, float* value_out) {
    SAE_CTX(c, 0); JOIN(c); ARG(obs, "null obs"); ARG(t >= 0 && t <= c->T, "t out of range");
    ARG(bytes == (size_t)c->E * c->obs_bytes_per_env, "obs must be E frames of 64x64x3 uint8");
    const int E = c->E, A = c->A;
    const bool last = (t == c->T), st = store != 0;
    c->staged_valid = false;
    HIPC(hipMemcpyAsync(c->stage_frames, obs, bytes, hipMemcpyHostToDevice, c->stream));
    const float* du = nullptr;
    if (u) { HIPC(hipMemcpyAsync(c->d_u, u, (size_t)E * 4, hipMemcpyHostToDevice, c->stream)); du = c->d_u; }
    InputSrc src{c->stage_frames, nullptr, 0};
    net_forward(c, src, E, {});
    float* hid = st ? s->ring_h + (size_t)t * E * D : s->step_h;
    const long long nh = (long long)E * D;
    hipLaunchKernelGGL(sae_hidden_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, c->stream, (const void*)c->blk[2].P2, c->bf ? 1 : 0, hid, nh);
    if (st) HIPC(hipMemcpyAsync(c->frames + (size_t)t * bytes, c->stage_frames, bytes, hipMemcpyDeviceToDevice, c->stream));      // obs_batch[t]
    launch_logp_all(c->hout, E, A, (st && !last) ? s->ring_l + (size_t)t * E * A : c->d_lp, nullptr, c->stream, c->lse);      // p.logits: always the policy's
    const unsigned long long ctr = s->counter;
    s->counter += (unsigned long long)E;
    int32_t* act_dst = (st && !last) ? c->act + (size_t)t * E : c->s_act;
    float* val_dst = st ? c->value + (size_t)t * E : c->s_val;
    launch_sample(c->hout, E, A, du, seed, ctr, act_from_probe ? nullptr : act_dst, c->s_logp, val_dst, c->stream, c->lse);
    if (act_from_probe) {      // Categorical(logits = linear_model(sae(hidden)[1])[0]).sample(): same uniform, the probe's distribution
        sae_encode(c, hid, s->enc, E);
        sae_probe_fwd(c, s->enc, s->pout, E);
        launch_sample(s->pout, E, A, du, seed, ctr, act_dst, c->s_logp, nullptr, c->stream, 0);
    }
    HIPC(hipGetLastError()); NETCHK(c);
    if (act_out) HIPC(hipMemcpyAsync(c->h_i, act_dst, (size_t)E * 4, hipMemcpyDeviceToHost, c->stream));
    if (value_out) HIPC(hipMemcpyAsync(c->h_f, val_dst, (size_t)E * 4, hipMemcpyDeviceToHost, c->stream));
    if (act_out || value_out || u) HIPC(hipStreamSynchronize(c->stream));
    if (act_out) for (int e = 0; e < E; ++e) act_out[e] = c->h_i[e];
    if (value_out) memcpy(value_out, c->h_f, (size_t)E * 4);
    return 0;
}

static int sae_forward_rows(mi_ctx* c, const int64_t* idx, int n) {
    mi_sae* s = c->sae;
    ARG(idx, "null idx"); ARG(n >= 1 && n <= c->NB, "n must be in [1, max_batch]");
    if (int r = sae_stage_idx(c, idx, n)) return r;
    const long long g4 = (long long)n * (D / 4);
    hipLaunchKernelGGL(sae_gather_kernel, dim3((unsigned)((g4 + 255) / 256)), dim3(256), 0, c->stream, (const float4*)s->ring_h, (const int32_t*)c->d_idx,
                       (float4*)s->X, n);
    sae_encode(c, s->X, s->enc, n);
    return 0;
}

// the body of SAE.optimize_sae's loop (agents/sae.py:151-156) on ring rows idx; gradients accumulate un-scaled (:156-163)
int mi_sae_minibatch(mi_ctx* c, const int64_t* idx, int32_t n, float sparse_coef, float* log_out) {
    SAE_CTX(c, 0); JOIN(c);
    if (int r = sae_forward_rows(c, idx, n)) return r;
    const int S = s->S;
    sae_decode(c, s->enc, s->rec, n);
    const long long tot4 = (long long)n * (D / 4);
    const int nblk = (int)((tot4 + 255) / 256 < 1024 ? (tot4 + 255) / 256 : 1024);
    hipLaunchKernelGGL(sae_recon_kernel, dim3(nblk), dim3(256), 0, c->stream, (float4*)s->rec, (const float4*)s->X, tot4, 2.f / ((float)n * (float)D), s->red_part);
    const int gy = (n + 3) / 4 < COLSUM_GROUPS / 4 ? (n + 3) / 4 : COLSUM_GROUPS / 4;
    hipLaunchKernelGGL(sae_colsum_kernel, dim3(S / 64, gy), dim3(256), 0, c->stream, (const float*)s->enc, n, S, s->col_part);
    hipLaunchKernelGGL(sae_kl_kernel, dim3((S + 255) / 256), dim3(256), 0, c->stream, (const double*)s->col_part, gy * 4, n, S, (double)s->rho, (double)sparse_coef,
                       s->kl_term, s->seed);
    hipLaunchKernelGGL(sae_finish_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)s->red_part, nblk, (const float*)s->kl_term, S, 1.0 / ((double)n * D),
                       sparse_coef, s->log);
    // backward: rec now holds dRec.  dW_d += dRec^T enc, db_d += colsum(dRec); dEnc = (dRec W_d + seed) (enc > 0); dW_e += dEnc^T x, db_e += colsum(dEnc)
    linear_wgrad(c, s->rec, s->enc, 0, s->g[0] + (size_t)S * D + S, s->g[0] + (size_t)2 * S * D + S, n, S, D);
    sae_gemm(c, s->rec, D, sae_Wd(s), S, 1, s->dEnc, n, S, D, nullptr, 0, s->enc);
    const long long te = (long long)n * S;
    hipLaunchKernelGGL(sae_seed_kernel, dim3((unsigned)((te + 255) / 256)), dim3(256), 0, c->stream, s->dEnc, (const float*)s->enc, (const float*)s->seed, te, S);
    linear_wgrad(c, s->dEnc, s->X, 0, s->g[0], s->g[0] + (size_t)S * D, n, D, S);
    return sae_read_log(c, log_out);
}

// the body of SAE.optimize_linear_model's loop (agents/sae.py:193-201): the encoder runs forward only (torch.no_grad) and gets no gradient
int mi_sae_probe_minibatch(mi_ctx* c, const int64_t* idx, int32_t n, float* log_out) {
    SAE_CTX(c, 0); JOIN(c);
    if (int r = sae_forward_rows(c, idx, n)) return r;
    const int S = s->S, A = c->A, nblk = (n + 255) / 256;
    ARG(nblk <= 1024, "n too large for the probe's partial sums");
    sae_probe_fwd(c, s->enc, s->pout, n);
    hipLaunchKernelGGL(sae_probe_loss_kernel, dim3(nblk), dim3(256), 0, c->stream, (const float*)s->pout, (const float*)s->ring_l, (const float*)c->value,
                       (const int32_t*)c->d_idx, n, A, s->pdY, s->red_part);
    hipLaunchKernelGGL(sae_probe_finish_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)s->red_part, nblk, n, s->log, s->col_part,
                       s->g[1] + (size_t)(A + 1) * S + A);
    hipLaunchKernelGGL(sae_probe_value_kernel, dim3(nblk), dim3(256), 0, c->stream, (const float*)s->pout, (const double*)s->col_part, n, A, s->pdY);
    // gW += dY^T enc (all A + 1 rows); gb += colsum(dY) for the A policy columns (the value column's came from the batch sums above)
    GemmArgs g{};
    g.ws = c->gemm_ws; g.ws_floats = c->gemm_ws_floats;
    g.A = s->pdY; g.B = s->enc; g.C = s->g[1]; g.M = A + 1; g.N = S; g.K = n;
    g.sam = 1; g.sak = A + 1; g.sbk = S; g.sbn = 1; g.ldc = S; g.accumulate = 1;
    launch_gemm(g, c->stream);
    launch_colsum_acc(s->pdY, n, A, A + 1, s->g[1] + (size_t)(A + 1) * S, c->col_ws, c->stream);
    return sae_read_log(c, log_out);
}

// clip_grad_norm_(model.parameters(), c) + Adam(eps=1e-5).step() + zero_grad() (agents/sae.py:159-162 / :204-207) on that model's flat vector:
// mi_optimizer_step's partial-sum kernel for the norm, sae_adam_kernel for the step
int mi_sae_optimizer_step(mi_ctx* c, int32_t which, float lr, float max_norm, int32_t step, float* gnorm_out) {
    SAE_CTX(c, which); JOIN(c); ARG(step >= 1, "adam_step is 1-based");
    const AdamScalars a = adam_scalars(lr, step);
    const long long n = which ? s->n_probe : s->n_sae;
    launch_sumsq_partials(s->g[which], n, s->sumsq, c->stream);
    launch_sae_adam(s->p[which], s->g[which], s->m[which], s->v[which], n, s->sumsq, max_norm, a.w1, a.beta2, a.w2, a.eps, a.step_size, a.bc2_sqrt,
                    s->gnorm, c->stream);
    HIPC(hipGetLastError()); NETCHK(c);
    if (gnorm_out) {
        HIPC(hipMemcpyAsync(s->h_log + 4, s->gnorm, 4, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        *gnorm_out = s->h_log[4];
    }
    return 0;
}

// test hook: the forward pass of mi_sae_minibatch on ring rows idx -> enc (n x S) and rec (n x 2048, the reference's column order)
int mi_sae_debug_forward(mi_ctx* c, const int64_t* idx, int32_t n, float* enc_out, float* rec_out) {
    SAE_CTX(c, 0); JOIN(c);
    if (int r = sae_forward_rows(c, idx, n)) return r;
    sae_decode(c, s->enc, s->rec, n);
    HIPC(hipGetLastError()); NETCHK(c);
    std::vector<float> tmp;
    if (enc_out) HIPC(hipMemcpyAsync(enc_out, s->enc, (size_t)n * s->S * 4, hipMemcpyDeviceToHost, c->stream));
    if (rec_out) { tmp.resize((size_t)n * D); HIPC(hipMemcpyAsync(tmp.data(), s->rec, tmp.size() * 4, hipMemcpyDeviceToHost, c->stream)); }
    HIPC(hipStreamSynchronize(c->stream));
    if (rec_out)
        for (size_t b = 0; b < (size_t)n; ++b)
            for (int h = 0; h < D; ++h) rec_out[b * D + h] = tmp[b * D + (h % 64) * 32 + h / 64];
    return 0;
}
