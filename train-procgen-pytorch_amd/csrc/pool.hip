// The stand-alone max-pool kernels, nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of the IMPALA blocks (common/model.py:158), forward
// and backward, fp32 and bf16 storage.  (The bf16 update path pools inside the fused conv kernels, convpool_bf16.hip; these serve the
// fp32 path and the op-level hooks.)  gfx950 only.
#include "common.h"
#include "device_util.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ max pool 3/2/1
// nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (common/model.py:158), NHWC.  The winner is the
// FIRST maximum in (ky,kx) scan order (strict >), which is where torch's CPU kernel routes the
// gradient; its window-relative position is kept as one byte per output for the backward pass.
template <int HW, int C>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          uint8_t* __restrict__ arg, int n) {
    constexpr int HO = HW / 2, C4 = C / 4;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;          // one thread = 4 channels of one output pixel
    const unsigned tot = (unsigned)n * HO * HO * C4;
    if (e >= tot) return;
    const unsigned c4 = e % C4, ox = (e / C4) % HO, oy = (e / (C4 * HO)) % HO, img = e / (C4 * HO * HO);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned bi[4] = {0, 0, 0, 0};
    bool first = true;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int y = 2 * (int)oy - 1 + ky, x = 2 * (int)ox - 1 + kx;
            if (y < 0 || y >= HW || x < 0 || x >= HW) continue;
            const f32x4 v = *(const f32x4*)(in + (((size_t)img * HW + y) * HW + x) * C + c4 * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (first || v[k] > best[k] || v[k] != v[k]) { best[k] = v[k]; bi[k] = ky * 3 + kx; }
            first = false;
        }
    *(f32x4*)(out + (size_t)e * 4) = best;
    *(uint32_t*)(arg + (size_t)e * 4) = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
}

template <int HW, int C>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dout, const uint8_t* __restrict__ arg,
                                                          float* __restrict__ din, int n) {
    constexpr int HO = HW / 2, C4 = C / 4;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;          // 4 channels of one INPUT pixel
    const unsigned tot = (unsigned)n * HW * HW * C4;
    if (e >= tot) return;
    const unsigned c4 = e % C4, x = (e / C4) % HW, y = (e / (C4 * HW)) % HW, img = e / (C4 * HW * HW);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    // windows oy with 2*oy-1 <= y <= 2*oy+1
    for (unsigned oy = y / 2; oy <= (y + 1) / 2; ++oy) {
        if (oy >= HO) continue;
        for (unsigned ox = x / 2; ox <= (x + 1) / 2; ++ox) {
            if (ox >= HO) continue;
            const size_t o = ((((size_t)img * HO + oy) * HO + ox) * C4 + c4) * 4;
            const unsigned pos = (y - (2 * oy - 1)) * 3 + (x - (2 * ox - 1));
            const uint32_t a = *(const uint32_t*)(arg + o);
            const f32x4 d = *(const f32x4*)(dout + o);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((a >> (8 * k)) & 0xffu) == pos) s[k] += d[k];
        }
    }
    *(f32x4*)(din + (size_t)e * 4) = s;
}

// bf16 storage: 8 channels (16 bytes) per thread; comparisons on the exact bf16 values
template <int HW, int C>
__global__ __launch_bounds__(256) void maxpool_fwd_bf16_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
                                                               uint8_t* __restrict__ arg, int n) {
    constexpr int HO = HW / 2, C8 = C / 8;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    const unsigned tot = (unsigned)n * HO * HO * C8;
    if (e >= tot) return;
    const unsigned c8 = e % C8, ox = (e / C8) % HO, oy = (e / (C8 * HO)) % HO, img = e / (C8 * HO * HO);
    float best[8];
    unsigned bw[4] = {0, 0, 0, 0};       // winning bf16 bits, packed
    unsigned bi[8];
    bool first = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) { best[k] = -INFINITY; bi[k] = 0; }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int y = 2 * (int)oy - 1 + ky, x = 2 * (int)ox - 1 + kx;
            if (y < 0 || y >= HW || x < 0 || x >= HW) continue;
            const uint4 u = *(const uint4*)(in + (((size_t)img * HW + y) * HW + x) * C + c8 * 8);
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = (k & 1) ? bfw_hi(w[k >> 1]) : bfw_lo(w[k >> 1]);
                if (first || v > best[k] || v != v) {
                    best[k] = v; bi[k] = ky * 3 + kx;
                    const unsigned bits = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
                    bw[k >> 1] = (k & 1) ? ((bw[k >> 1] & 0x0000ffffu) | (bits << 16)) : ((bw[k >> 1] & 0xffff0000u) | bits);
                }
            }
            first = false;
        }
    *(uint4*)(out + (size_t)e * 8) = (uint4){bw[0], bw[1], bw[2], bw[3]};
    *(uint2*)(arg + (size_t)e * 8) = (uint2){bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24), bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24)};
}

template <int HW, int C>
__global__ __launch_bounds__(256) void maxpool_bwd_bf16_kernel(const unsigned short* __restrict__ dout, const uint8_t* __restrict__ arg,
                                                               unsigned short* __restrict__ din, int n) {
    constexpr int HO = HW / 2, C8 = C / 8;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    const unsigned tot = (unsigned)n * HW * HW * C8;
    if (e >= tot) return;
    const unsigned c8 = e % C8, x = (e / C8) % HW, y = (e / (C8 * HW)) % HW, img = e / (C8 * HW * HW);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (unsigned oy = y / 2; oy <= (y + 1) / 2; ++oy) {
        if (oy >= HO) continue;
        for (unsigned ox = x / 2; ox <= (x + 1) / 2; ++ox) {
            if (ox >= HO) continue;
            const size_t o = ((((size_t)img * HO + oy) * HO + ox) * C8 + c8) * 8;
            const unsigned pos = (y - (2 * oy - 1)) * 3 + (x - (2 * ox - 1));
            const uint2 a = *(const uint2*)(arg + o);
            const uint4 d = *(const uint4*)(dout + o);
            const unsigned w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned ak = ((k < 4 ? a.x : a.y) >> (8 * (k & 3))) & 0xffu;
                if (ak == pos) s[k] += (k & 1) ? bfw_hi(w[k >> 1]) : bfw_lo(w[k >> 1]);
            }
        }
    }
    uint4 r;
    r.x = f2bf(s[0]) | ((unsigned)f2bf(s[1]) << 16); r.y = f2bf(s[2]) | ((unsigned)f2bf(s[3]) << 16);
    r.z = f2bf(s[4]) | ((unsigned)f2bf(s[5]) << 16); r.w = f2bf(s[6]) | ((unsigned)f2bf(s[7]) << 16);
    *(uint4*)(din + (size_t)e * 8) = r;
}

// host side: one (image size, channel count) dispatch for the four launchers; F<HW, C>::run launches its kernel
template <template <int, int> class F, typename... Args>
static bool pool_dispatch_shape(int hw, int c, Args... args) {
    if (hw == 64 && c == 16) F<64, 16>::run(args...);
    else if (hw == 32 && c == 32) F<32, 32>::run(args...);
    else if (hw == 16 && c == 32) F<16, 32>::run(args...);
    else return false;
    return true;
}
template <int HW, int C> struct PoolFwd { static void run(const float* in, float* out, uint8_t* arg, int n, hipStream_t st) {
    const unsigned tot = (unsigned)n * (HW / 2) * (HW / 2) * (C / 4);
    hipLaunchKernelGGL((maxpool_fwd_kernel<HW, C>), dim3((tot + 255) / 256), dim3(256), 0, st, in, out, arg, n);
} };
template <int HW, int C> struct PoolBwd { static void run(const float* dout, const uint8_t* arg, float* din, int n, hipStream_t st) {
    const unsigned tot = (unsigned)n * HW * HW * (C / 4);
    hipLaunchKernelGGL((maxpool_bwd_kernel<HW, C>), dim3((tot + 255) / 256), dim3(256), 0, st, dout, arg, din, n);
} };
template <int HW, int C> struct PoolFwdBf { static void run(const unsigned short* in, unsigned short* out, uint8_t* arg, int n, hipStream_t st) {
    const unsigned tot = (unsigned)n * (HW / 2) * (HW / 2) * (C / 8);
    hipLaunchKernelGGL((maxpool_fwd_bf16_kernel<HW, C>), dim3((tot + 255) / 256), dim3(256), 0, st, in, out, arg, n);
} };
template <int HW, int C> struct PoolBwdBf { static void run(const unsigned short* dout, const uint8_t* arg, unsigned short* din, int n, hipStream_t st) {
    const unsigned tot = (unsigned)n * HW * HW * (C / 8);
    hipLaunchKernelGGL((maxpool_bwd_bf16_kernel<HW, C>), dim3((tot + 255) / 256), dim3(256), 0, st, dout, arg, din, n);
} };
void launch_maxpool_fwd(const float* in, float* out, uint8_t* arg, int n, int hw, int c, hipStream_t st) {
    if (n > 0 && !pool_dispatch_shape<PoolFwd>(hw, c, in, out, arg, n, st)) mi_launch_fail("max pool: unsupported image size / channel count");
}
void launch_maxpool_bwd(const float* dout, const uint8_t* arg, float* din, int n, int hw, int c, hipStream_t st) {
    if (n > 0 && !pool_dispatch_shape<PoolBwd>(hw, c, dout, arg, din, n, st)) mi_launch_fail("max pool backward: unsupported image size / channel count");
}
void launch_maxpool_fwd_bf16(const void* in, void* out, uint8_t* arg, int n, int hw, int c, hipStream_t st) {
    if (n > 0 && !pool_dispatch_shape<PoolFwdBf>(hw, c, (const unsigned short*)in, (unsigned short*)out, arg, n, st))
        mi_launch_fail("max pool (bf16): unsupported image size / channel count");
}
void launch_maxpool_bwd_bf16(const void* dout, const uint8_t* arg, void* din, int n, int hw, int c, hipStream_t st) {
    if (n > 0 && !pool_dispatch_shape<PoolBwdBf>(hw, c, (const unsigned short*)dout, arg, (unsigned short*)din, n, st))
        mi_launch_fail("max pool backward (bf16): unsupported image size / channel count");
}
