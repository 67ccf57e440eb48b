// The GRU cell of a rollout step (GruPolicy, common/model.py:212-225): the piecewise kernels around the GEMM, the value gradient through
// the gates (saliency) and the fused one-launch step of the pipelined rollout.  Training through the GRU over a trajectory is
// gru_seq.hip.  gfx950 only.
#include "common.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ GRU cell (rollout only)
// nn.GRU single step (common/model.py:219-225): gi = W_ih x + b_ih, gh = W_hh (h*mask) + b_hh come from the GEMM;
// r = s(gi_r+gh_r), z = s(gi_z+gh_z), n = tanh(gi_n + r*gh_n), h' = (1-z)*n + z*h.
__global__ void mask_rows_kernel(const float* h, const float* done, float* out, int n, int H) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * H) return;
    out[e] = h[e] * (1.f - done[e / H]);
}
void launch_mask_rows(const float* h, const float* done, float* out, int n, int H, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mask_rows_kernel, dim3((n * H + 255) / 256), dim3(256), 0, st, h, done, out, n, H);
}
__global__ void gru_gates_kernel(const float* gi, const float* gh, const float* hm, float* h_out, float* feat_out, int n, int H) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * H) return;
    const int row = e / H, j = e % H;
    const float* a = gi + (long long)row * 3 * H;
    const float* b = gh + (long long)row * 3 * H;
    const float r = 1.f / (1.f + expf(-(a[j] + b[j])));
    const float z = 1.f / (1.f + expf(-(a[H + j] + b[H + j])));
    const float nn = tanhf(a[2 * H + j] + r * b[2 * H + j]);
    const float hn = (1.f - z) * nn + z * hm[e];
    h_out[e] = hn;
    feat_out[e] = hn;
}
// d value / d (GRU input pre-activations): value = w_v . h' + b_v with h' = (1 - z) n + z h (gates as in gru_gates_kernel), so with
// g = w_v[j]:  dn = g (1 - z), dz = g (h - n);  d pre_n = dn (1 - n^2), d pre_z = dz z (1 - z), d pre_r = d pre_n gh_n r (1 - r).
// dgates[row] = {d pre_r, d pre_z, d pre_n} (3H): the gradient wrt gi = W_ih x + b_ih; dx = dgates W_ih follows as a GEMM.
// ROWSEED (value_from_logits): d value / d h' differs from row to row -- wv is [n][H] (lse_hidden_seed_kernel) instead of fc_value's one weight row.
template <bool ROWSEED>
__global__ void gru_value_bwd_kernel(const float* gi, const float* gh, const float* hm, const float* wv, float* dgates, int n, int H) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * H) return;
    const int row = e / H, j = e % H;
    const float* a = gi + (long long)row * 3 * H;
    const float* b = gh + (long long)row * 3 * H;
    const float r = 1.f / (1.f + expf(-(a[j] + b[j])));
    const float z = 1.f / (1.f + expf(-(a[H + j] + b[H + j])));
    const float nn = tanhf(a[2 * H + j] + r * b[2 * H + j]);
    const float g = ROWSEED ? wv[e] : wv[j];
    const float dpn = g * (1.f - z) * (1.f - nn * nn);
    const float dpz = g * (hm[e] - nn) * z * (1.f - z);
    const float dpr = dpn * b[2 * H + j] * r * (1.f - r);
    float* d = dgates + (long long)row * 3 * H;
    d[j] = dpr; d[H + j] = dpz; d[2 * H + j] = dpn;
}
void launch_gru_value_bwd(const float* gi, const float* gh, const float* hm, const float* wv, float* dgates, int n, int H, hipStream_t st, int row_seed) {
    if (n <= 0) return;
    if (row_seed) hipLaunchKernelGGL(gru_value_bwd_kernel<true>, dim3((n * H + 255) / 256), dim3(256), 0, st, gi, gh, hm, wv, dgates, n, H);
    else hipLaunchKernelGGL(gru_value_bwd_kernel<false>, dim3((n * H + 255) / 256), dim3(256), 0, st, gi, gh, hm, wv, dgates, n, H);
}
void launch_gru_gates(const float* gi, const float* gh, const float* hm, float* h_out, float* feat_out, int n, int H, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gru_gates_kernel, dim3((n * H + 255) / 256), dim3(256), 0, st, gi, gh, hm, h_out, feat_out, n, H);
}
// One GRU step of an env group in ONE launch (the pipelined rollout's cell, rollout.hip group_issue; common/model.py:212-225 for one step):
//   hm = h_in (1 - done[row]);  gi = W_ih x + b_ih;  gh = W_hh hm + b_hh;  r, z, n as gru_gates_kernel;  h' = (1 - z) n + z hm  -> h_out, h_copy
// It replaces mask_rows + two linear_fwd + gru_gates.  Workgroup = 4 waves = hidden units j0 .. j0+3 (one per wave) x 64 rows (one per
// lane); its 24 weight rows (gates r, z, n of W_ih and W_hh for those units) sit in LDS and are read as wave-uniform broadcasts, the
// rows' x / h_in come from L1 / L2 as float4.  Every (row, unit) output is one thread's six k-ordered fp32 FMA chains, so a row's result
// is a fixed function of that row's inputs: it does not depend on n, on the row's offset or on the grid (env groups of any size give
// bit-identical states) and there is no split-K workspace.  h_in must not alias h_out / h_copy / x (other workgroups still read the
// rows' whole h_in / x while one writes its units).  H: multiple of 64, <= 512 (LDS 96 H bytes).
__global__ __launch_bounds__(256) void gru_step_kernel(const float* __restrict__ x, const float* __restrict__ h_in, const float* __restrict__ done,
                                                       const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                       const float* __restrict__ b_hh, float* __restrict__ h_out, float* __restrict__ h_copy, int n, int H) {
    extern __shared__ float4 gru_sw[];                      // [matrix ih, hh][gate r, z, n][unit 0..3][H / 4]
    const int H4 = H >> 2, j0 = blockIdx.x * 4, tid = threadIdx.x;
    for (int i = tid; i < 24 * H4; i += 256) {
        const int q = i / H4, k4 = i - q * H4;
        const int m = q / 12, g = (q >> 2) % 3, u = q & 3;
        gru_sw[i] = reinterpret_cast<const float4*>((m ? w_hh : w_ih) + (size_t)(g * H + j0 + u) * H)[k4];
    }
    __syncthreads();
    const int u = tid >> 6;                                  // this wave's unit
    const int row = blockIdx.y * 64 + (tid & 63);
    if (row >= n) return;
    const int j = j0 + u;
    const float keep = 1.f - done[row];
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * H);
    const float4* hr = reinterpret_cast<const float4*>(h_in + (size_t)row * H);
    const float4 *wir = gru_sw + (0 + u) * H4, *wiz = gru_sw + (4 + u) * H4, *win = gru_sw + (8 + u) * H4;
    const float4 *whr = gru_sw + (12 + u) * H4, *whz = gru_sw + (16 + u) * H4, *whn = gru_sw + (20 + u) * H4;
    float ar = 0.f, az = 0.f, an = 0.f, br = 0.f, bz = 0.f, bn = 0.f;
    // The rows' x / h_in stream through registers in chunks of 32 k, two chunks in flight: a load per k4 step would put one L2 round trip
    // on the chain for every 4 k (24 us per call at 64 rows, H = 256, measured).  H / 32 chunks: even for H a multiple of 64.
    constexpr int C4 = 8;
    float4 xa[C4], ha[C4], xb[C4], hb[C4];
    auto load = [&](float4* xs, float4* hs, int c) {
#pragma unroll
        for (int i = 0; i < C4; ++i) { xs[i] = xr[c * C4 + i]; hs[i] = hr[c * C4 + i]; }
    };
    auto step = [&](const float4* xs, const float4* hs, int c) {
#define GRU_FMA4(acc, p, v) acc = fmaf(p.x, v.x, acc); acc = fmaf(p.y, v.y, acc); acc = fmaf(p.z, v.z, acc); acc = fmaf(p.w, v.w, acc)
#pragma unroll
        for (int i = 0; i < C4; ++i) {
            const int k4 = c * C4 + i;
            const float4 xv = xs[i];
            float4 hv = hs[i];
            hv.x *= keep; hv.y *= keep; hv.z *= keep; hv.w *= keep;
            const float4 a0 = wir[k4], a1 = wiz[k4], a2 = win[k4], c0 = whr[k4], c1 = whz[k4], c2 = whn[k4];
            GRU_FMA4(ar, a0, xv); GRU_FMA4(az, a1, xv); GRU_FMA4(an, a2, xv);
            GRU_FMA4(br, c0, hv); GRU_FMA4(bz, c1, hv); GRU_FMA4(bn, c2, hv);
        }
#undef GRU_FMA4
    };
    const int nc = H4 / C4;
    load(xa, ha, 0);
    for (int c = 0; c < nc; c += 2) {
        load(xb, hb, c + 1);
        step(xa, ha, c);
        if (c + 2 < nc) load(xa, ha, c + 2);
        step(xb, hb, c + 1);
    }
    const float r = 1.f / (1.f + expf(-((ar + b_ih[j]) + (br + b_hh[j]))));
    const float z = 1.f / (1.f + expf(-((az + b_ih[H + j]) + (bz + b_hh[H + j]))));
    const float nn = tanhf((an + b_ih[2 * H + j]) + r * (bn + b_hh[2 * H + j]));
    const size_t e = (size_t)row * H + j;
    const float hn = (1.f - z) * nn + z * (h_in[e] * keep);
    h_out[e] = hn;
    if (h_copy) h_copy[e] = hn;
}
void launch_gru_step(const float* x, const float* h_in, const float* done, const float* w_ih, const float* w_hh, const float* b_ih,
                     const float* b_hh, float* h_out, float* h_copy, int n, int H, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gru_step_kernel, dim3(H / 4, (n + 63) / 64), dim3(256), (size_t)96 * H, st, x, h_in, done, w_ih, w_hh, b_ih, b_hh,
                       h_out, h_copy, n, H);
}
