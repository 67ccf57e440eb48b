// One minibatch pass of an MLP context in TWO launches (mi_minibatch_fused in include/mi355ppo.h; opt-in beside mi_minibatch's chain
// of more than twenty launches, the update-side counterpart of env_resident.hip).  gfx950 only.
//
// Launch 1, mlp_fused_pass_kernel: a workgroup owns ONE tile of RES_R = 16 gathered samples (one MFMA M tile) and never talks to another
// workgroup.  It gathers the observation rows by d_idx, runs the MLP and the heads in fp32 on v_mfma_f32_16x16x4_f32 with the activations
// ping-ponging between two LDS buffers and the weights streamed from global memory (res_layer, res_layer.h; bias and ReLU as
// forward_mlp / linear_fwd place them), takes the per-sample loss terms and dY with the loss kernels' own device functions
// (loss_sample.h), and walks back through the heads and the layers: the data gradient of a layer through the ReLU mask of the layer's
// stored input, as backward_mlp / linear_dgrad take it.  On the way it leaves in global memory, for ALL rows, what the weight gradients
// need: every layer's input activation (act[l]), every layer's output gradient (g[l]), the heads' dY, and the per-sample loss terms.
//
// Launch 2, mlp_fused_reduce_kernel: workgroups 0 .. n_seg - 1 turn the loss terms of their segment into the statistics row and the log
// record (the block partials of loss_fwd_block, then loss_finalize_body: same layout, same order).  Every other workgroup owns one
// 16 x 16 tile of one layer's dW (and, for the tiles of input column 0, the matching 16 entries of db): its four waves walk a quarter of
// the n rows each, in row order, the four sums meet in LDS in wave order and go to the flat gradient buffer.  Every gradient element has
// exactly one owner.
//
// This is design (b) of the two that fit the rules: no per-workgroup slabs of the whole gradient vector, no float
// atomics, no grid barrier, no spin wait, no cooperative launch; every loop is bounded by n, the layer count and the layer sizes; the
// result is a function of the inputs alone, whatever the order the workgroups run in.
//
// Summation orders (fp32, no wider accumulation anywhere):
//   a forward dot product (res_layer)   K in chunks of 16; MFMA m of a chunk covers columns kk + 4 q + m (q = 0 .. 3 in order inside the
//                                       instruction); accumulators acc0 (m = 0, 2) and acc1 (m = 1, 3) are fmaf chains of K / 2 terms;
//                                       y = acc0 + acc1 + bias.                                                  d = K / 2 + 2
//   a data gradient (fused_dgrad)       the same form over the layer's outputs o.                                d = out / 2 + 1
//   dW / db of a layer                  the rows in four contiguous ranges of span = ceil(n / 128) * 32 rows, one per wave of the tile's
//                                       workgroup.  A wave: row chunks of 16, chunk j of its range into accumulator set j & 1; MFMA m of
//                                       a chunk covers rows r0 + 4 q + m.  Accumulator [s][m] is an fmaf chain over the range's rows
//                                       = 16 (2 j' + s) + 4 q + m in ascending order, ceil(span / 8) terms at most; the eight are added as
//                                       ((a00 + a01) + (a02 + a03)) + ((a10 + a11) + (a12 + a13)); the four waves' sums as
//                                       ((w0 + w1) + w2) + w3; then grads += that.                        d = ceil(n / 32) + 8
//   a segment's loss statistics         64-sample blocks of the segment (no block straddles two segments) by wave_sum, six shuffle
//                                       steps; then loss_finalize_body: 8 row groups, then the groups in order.
//                                                                                       d = 6 + ceil(blocks / 8) + 8, as the chain's
// Means are sum / n_global (LossArgs.inv_n_global), as in the chain.
#include "engine_ctx.h"
#include "device_util.h"
#include "loss_sample.h"
#include "res_layer.h"

#define FUSED_TERMS_LD 32      // floats per row of the per-sample loss terms: 0 pi, 1 vm, 2 H, 8 .. 8 + A - 1 p[k] (the columns of a block partial)
#define FUSED_RED_THREADS 256

// dX[16][N] = G[16][O] W (* mask > 0): W [O][N] row-major in global memory, G / dX in LDS (row stride RES_LD; G's columns O .. Op - 1 are
// zero, Op = O rounded up to 16).  Column tile n0 .. n0 + 15 of dX belongs to wave (n0 / 16) % waves; N is a multiple of 16.  Lane
// (i = lane & 15, q = lane >> 4) holds A[i][oo + 4 q + m] (one 16-byte read of a gradient row) and B[oo + 4 q + m][n0 + i] (four loads, one
// per weight row, 64 contiguous bytes per 16 lanes) for MFMA m.  Rows of W past O (the heads: A + 1 <= 16) load zeros.  mask: the layer's
// stored input [n][N] (post-ReLU), null for none; gdst: dX of the rows < n goes to global memory as well, [n][N].
__device__ __forceinline__ void fused_dgrad(const float* __restrict__ W, int O, int N, const float* mask, const float* G, float* DX,
                                            float* __restrict__ gdst, int row0, int n, int wave, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const int Op = (O + 15) & ~15;
    for (int n0 = wave * 16; n0 < N; n0 += (RES_THREADS / 64) * 16) {
        const float* wcol = W + n0 + i;
        const float* grow = G + i * RES_LD + 4 * q;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if ((O & 63) == 0) {
            // O in groups of 64: the 16 weights of group g + 1 are in flight while the 16 MFMAs of group g issue (res_layer's scheme; the
            // prefetch behind the last group reads that group again and drops it)
            float wc[16], wn[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wc[u] = wcol[(size_t)(16 * (u >> 2) + 4 * q + (u & 3)) * (size_t)N];
            for (int oo = 0; oo < O; oo += 64) {
                const int on = oo + 64 < O ? oo + 64 : oo;
#pragma unroll
                for (int u = 0; u < 16; ++u) wn[u] = wcol[(size_t)(on + 16 * (u >> 2) + 4 * q + (u & 3)) * (size_t)N];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 a = *(const f32x4*)(grow + oo + 16 * u);
                    acc0 = MFMA16(a.x, wc[4 * u + 0], acc0);
                    acc1 = MFMA16(a.y, wc[4 * u + 1], acc1);
                    acc0 = MFMA16(a.z, wc[4 * u + 2], acc0);
                    acc1 = MFMA16(a.w, wc[4 * u + 3], acc1);
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) wc[u] = wn[u];
            }
        } else {
            for (int oo = 0; oo < Op; oo += 16) {
                const f32x4 a = *(const f32x4*)(grow + oo);
                const int o = oo + 4 * q;
                // (a row past O is clamped to row O - 1 and dropped: the loads stay unconditional, nothing is read past the matrix)
                float w[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float v = wcol[(size_t)(o + m < O ? o + m : O - 1) * (size_t)N];
                    w[m] = (o + m < O) ? v : 0.f;
                }
                acc0 = MFMA16(a.x, w[0], acc0);
                acc1 = MFMA16(a.y, w[1], acc1);
                acc0 = MFMA16(a.z, w[2], acc0);
                acc1 = MFMA16(a.w, w[3], acc1);
            }
        }
        const float y[4] = {acc0.x + acc1.x, acc0.y + acc1.y, acc0.z + acc1.z, acc0.w + acc1.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * q + r;
            float v = y[r];
            if (mask) v = (mask[(size_t)(row < n ? row : n - 1) * (size_t)N + n0 + i] > 0.f) ? v : 0.f;      // (rows >= n: v is zero already)
            DX[(4 * q + r) * RES_LD + n0 + i] = v;
            if (row < n) gdst[(size_t)row * (size_t)N + n0 + i] = v;
        }
    }
}

template <bool LSE>
__global__ __launch_bounds__(RES_THREADS) void mlp_fused_pass_kernel(FusedNet f, LossArgs a, int n) {
    __shared__ __attribute__((aligned(16))) float s_x[2][RES_R * RES_LD];
    __shared__ float s_z[RES_R * RES_ZLD], s_dy[RES_R * RES_ZLD];      // the tile's head rows and their gradient, [16][A + 1]
    __shared__ int s_in[RES_MAX_LAYERS], s_out[RES_MAX_LAYERS], s_vec[RES_MAX_LAYERS];
    __shared__ long long s_w[RES_MAX_LAYERS], s_b[RES_MAX_LAYERS];
    __shared__ float* s_act[RES_MAX_LAYERS + 1];
    __shared__ float* s_g[RES_MAX_LAYERS];
    const ResidentNet& net = f.net;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
#pragma unroll
        for (int l = 0; l < RES_MAX_LAYERS; ++l) {
            s_in[l] = net.in[l]; s_out[l] = net.out[l]; s_vec[l] = net.vec[l]; s_w[l] = net.w_off[l]; s_b[l] = net.b_off[l];
            s_act[l] = f.act[l]; s_g[l] = f.g[l];
        }
        s_act[RES_MAX_LAYERS] = f.act[RES_MAX_LAYERS];
    }
    const int L = net.n_layers, A = a.A, O = A + 1, W = f.obs_dim;
    const int row0 = blockIdx.x * RES_R;
    // rows >= n of the tail tile compute on zeros, their dY is zero, and nothing of them is stored
    if (tid < RES_R * 16) {
        const int r = tid >> 4, j = tid & 15, row = row0 + r;
        const bool on = row < n && j < W;
        const float v = on ? f.obs[(size_t)a.idx[row] * (size_t)W + j] : 0.f;      // K tail zero-padded in LDS
        s_x[0][r * RES_LD + j] = v;
        if (on) f.act[0][(size_t)row * (size_t)W + j] = v;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        float* y = s_x[(l + 1) & 1];
        res_layer(net.params + s_w[l], net.params + s_b[l], s_in[l], s_out[l], s_vec[l] != 0, l + 1 < L, s_x[l & 1], y, RES_LD, wave, lane);
        __syncthreads();
        // the layer's output for the weight gradient of the next layer and its ReLU mask (the next LDS write into y is two barriers away)
        const int N = s_out[l];
        float* dst = s_act[l + 1];
        const int r = tid >> 5;          // 512 threads: 32 per row, 128 contiguous bytes per store instruction and row
        if (row0 + r < n)
            for (int j = tid & 31; j < N; j += 32) dst[(size_t)(row0 + r) * (size_t)N + j] = y[r * RES_LD + j];
    }
    res_layer(net.params + net.wh_off, net.params + net.bh_off, net.H, O, net.heads_vec != 0, false, s_x[L & 1], s_z, O, wave, lane);
    __syncthreads();
    if (tid < RES_R) {
        const int row = row0 + tid;
        if (row < n) {
            LossArgs la = a;                 // the tile's rows as samples 0 .. 15 of head rows and a gradient that live in LDS
            la.hout = s_z; la.idx = a.idx + row0; la.dY = s_dy;
            SampleTerms t;
            sample_terms<LSE>(la, tid, t);
            loss_bwd_sample<LSE>(la, tid, t);
            float* tr = f.terms + (size_t)row * FUSED_TERMS_LD;      // what loss_fwd_block sums
            tr[0] = fminf(t.surr1, t.surr2); tr[1] = fmaxf(t.vs1, t.vs2); tr[2] = t.H;
#pragma unroll
            for (int k = 0; k < MAXA; ++k) if (k < A) tr[8 + k] = t.p[k];
        } else {
            for (int k = 0; k < O; ++k) s_dy[tid * O + k] = 0.f;
        }
    }
    __syncthreads();
    if (tid < RES_R * 16) {
        const int r = tid >> 4, j = tid & 15, row = row0 + r;
        const float v = j < O ? s_dy[r * O + j] : 0.f;
        s_x[0][r * RES_LD + j] = v;
        if (row < n && j < O) f.dYh[(size_t)row * (size_t)O + j] = v;
    }
    __syncthreads();
    // backward: d / d feat through the heads (no mask), then layer by layer through the ReLU mask of the layer's input
    fused_dgrad(net.params + net.wh_off, O, net.H, nullptr, s_x[0], s_x[1], s_g[L - 1], row0, n, wave, lane);
    __syncthreads();
    int cur = 1;
    for (int l = L - 1; l >= 1; --l) {
        fused_dgrad(net.params + s_w[l], s_out[l], s_in[l], s_act[l], s_x[cur], s_x[cur ^ 1], s_g[l - 1], row0, n, wave, lane);
        __syncthreads();
        cur ^= 1;
    }
}

// segment k's statistics row and log record (workgroup k of the reduce launch)
__device__ __forceinline__ void fused_records(const FusedNet& f, LossArgs a, const SegTab& st, int k, float* stats_base, float* log_base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int first = 0;
    for (int j = 0; j < k; ++j) first += (st.start[j + 1] - st.start[j] + 63) / 64;
    const int s0 = st.start[k], s1 = st.start[k + 1], nblk = (s1 - s0 + 63) / 64;
    a.partial += (long long)first * (8 + a.A);
    for (int b = wave; b < nblk; b += FUSED_RED_THREADS / 64) {
        const int s = s0 + b * 64 + lane;
        const float* tr = f.terms + (size_t)(s < s1 ? s : s0) * FUSED_TERMS_LD;
        float* prow = a.partial + (long long)b * (8 + a.A);
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = tr[c], r = wave_sum(s < s1 ? v : 0.f); if (lane == 0) prow[c] = r; }
#pragma unroll
        for (int c = 0; c < MAXA; ++c) if (c < a.A) { const float v = tr[8 + c], r = wave_sum(s < s1 ? v : 0.f); if (lane == 0) prow[8 + c] = r; }
    }
    __syncthreads();
    a.stats = stats_base + 32 * k;
    loss_finalize_body(a, nblk, 3, nullptr, log_base + 8 * k);
}

// one wave's share, rows r_lo .. r_hi - 1, of a 16 x 16 tile of dW[o][k] = sum_rows G[row][o] X[row][k] (BIAS, the tiles of k0 == 0: + db[o] =
// sum_rows G[row][o], the same MFMAs against a B of ones).  Lane (i, q), MFMA m of a 16-row chunk: A = G[r0 + 4 q + m][o0 + i], B = X[r0 + 4 q + m][k0 + i];
// D: dW[o0 + 4 q + r][k0 + i].  Every load is unconditional: a row >= n is clamped to row n - 1, and the A value of a row >= r_hi multiplied by zero; a
// column past the layer (the first layer's obs_dim, the heads' A + 1) is clamped to column 0 and lands in rows / columns of D that are not
// stored.  Two register sets of 32 rows each take turns, one in flight while the other's MFMAs issue.
template <bool BIAS>
__device__ __forceinline__ void fused_wgrad_tile(const float* __restrict__ G, const float* __restrict__ X, int out, int in, int o0, int k0,
                                                 int n, int r_lo, int r_hi, f32x4& w_out, f32x4& b_out, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const float* gp = G + (o0 + i < out ? o0 + i : 0);
    const float* xp = X + (k0 + i < in ? k0 + i : 0);
    f32x4 acc[2][4], accb[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int m = 0; m < 4; ++m) { acc[s][m] = (f32x4){0.f, 0.f, 0.f, 0.f}; accb[s][m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    float a0[2][4], b0[2][4], a1[2][4], b1[2][4];
    auto fetch = [&](int r0, float (&ga)[2][4], float (&xb)[2][4]) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int row = r0 + 16 * s + 4 * q + m;
                const size_t rc = (size_t)(row < n ? row : n - 1);
                ga[s][m] = gp[rc * (size_t)out] * (row < r_hi ? 1.f : 0.f);
                xb[s][m] = xp[rc * (size_t)in];
            }
    };
    auto mma = [&](const float (&ga)[2][4], const float (&xb)[2][4]) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc[s][m] = MFMA16(ga[s][m], xb[s][m], acc[s][m]);
                if (BIAS) accb[s][m] = MFMA16(ga[s][m], 1.0f, accb[s][m]);
            }
    };
    fetch(r_lo, a0, b0);
    for (int r0 = r_lo; r0 < r_hi; r0 += 64) {      // (a set that starts at or past r_hi adds zeros)
        fetch(r0 + 32, a1, b1);
        mma(a0, b0);
        fetch(r0 + 64, a0, b0);
        mma(a1, b1);
    }
    w_out = ((acc[0][0] + acc[0][1]) + (acc[0][2] + acc[0][3])) + ((acc[1][0] + acc[1][1]) + (acc[1][2] + acc[1][3]));
    if (BIAS) b_out = ((accb[0][0] + accb[0][1]) + (accb[0][2] + accb[0][3])) + ((accb[1][0] + accb[1][1]) + (accb[1][2] + accb[1][3]));
}

__global__ __launch_bounds__(FUSED_RED_THREADS) void mlp_fused_reduce_kernel(FusedNet f, LossArgs a, SegTab st, int n, float* grads, float* stats_base,
                                                                             float* log_base) {
    if ((int)blockIdx.x < st.n_seg) { fused_records(f, a, st, (int)blockIdx.x, stats_base, log_base); return; }
    const ResidentNet& net = f.net;
    constexpr int NW = FUSED_RED_THREADS / 64;
    __shared__ f32x4 s_part[2][NW][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int t = (int)blockIdx.x - st.n_seg;      // the workgroup's tile among those of all layers, then the heads
    // wave w sums rows [w span, (w + 1) span), span = n / 4 rounded up to the 32 rows of a register set
    const int span = ((n + NW * 32 - 1) / (NW * 32)) * 32, r_lo = wave * span, r_hi = min(n, r_lo + span);
    const int L = net.n_layers;
    for (int l = 0; l <= L; ++l) {
        const int out = l < L ? net.out[l] : a.A + 1, in = l < L ? net.in[l] : net.H;
        const int to = (out + 15) / 16, tk = (in + 15) / 16;
        if (t < to * tk) {
            const long long w_off = l < L ? net.w_off[l] : net.wh_off, b_off = l < L ? net.b_off[l] : net.bh_off;
            const float* G = l < L ? f.g[l] : f.dYh;
            const int o0 = (t / tk) * 16, k0 = (t % tk) * 16;
            const bool bias = k0 == 0;
            f32x4 w = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (bias) fused_wgrad_tile<true>(G, f.act[l], out, in, o0, k0, n, r_lo, r_hi, w, b, lane);
            else fused_wgrad_tile<false>(G, f.act[l], out, in, o0, k0, n, r_lo, r_hi, w, b, lane);
            s_part[0][wave][lane] = w; s_part[1][wave][lane] = b;
            __syncthreads();
            if (wave == 0) {
                const int i = lane & 15, q = lane >> 4;
                w = ((s_part[0][0][lane] + s_part[0][1][lane]) + s_part[0][2][lane]) + s_part[0][3][lane];
                b = ((s_part[1][0][lane] + s_part[1][1][lane]) + s_part[1][2][lane]) + s_part[1][3][lane];
                const float wv[4] = {w.x, w.y, w.z, w.w}, bv[4] = {b.x, b.y, b.z, b.w};
                float* gW = grads + w_off;
                float* gb = grads + b_off;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = o0 + 4 * q + r;
                    if (o < out && k0 + i < in) gW[(size_t)o * (size_t)in + k0 + i] += wv[r];
                    if (bias && i == 0 && o < out) gb[o] += bv[r];
                }
            }
            return;
        }
        t -= to * tk;
    }
}

int mlp_fused_tiles(const FusedNet& f, int A) {
    int t = 0;
    for (int l = 0; l < f.net.n_layers; ++l) t += ((f.net.out[l] + 15) / 16) * ((f.net.in[l] + 15) / 16);
    return t + ((A + 1 + 15) / 16) * ((f.net.H + 15) / 16);
}
void launch_mlp_fused_pass(const FusedNet& f, const LossArgs& a, int n, hipStream_t st) {
    const dim3 grid((unsigned)((n + RES_R - 1) / RES_R)), block(RES_THREADS);
    if (a.value_from_logits) hipLaunchKernelGGL(mlp_fused_pass_kernel<true>, grid, block, 0, st, f, a, n);
    else hipLaunchKernelGGL(mlp_fused_pass_kernel<false>, grid, block, 0, st, f, a, n);
}
void launch_mlp_fused_reduce(const FusedNet& f, const LossArgs& a, const SegTab& seg, int n, float* grads, float* stats_base, float* log_base,
                             hipStream_t st) {
    hipLaunchKernelGGL(mlp_fused_reduce_kernel, dim3((unsigned)(seg.n_seg + mlp_fused_tiles(f, a.A))), dim3(FUSED_RED_THREADS), 0, st, f, a, seg, n,
                       grads, stats_base, log_base);
}
