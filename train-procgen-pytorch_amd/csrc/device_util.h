// Device-side helpers shared by the kernels of every file: wave / workgroup sums in a fixed order, the bf16 <-> fp32 conversions, the MFMA shorthands,
// the packed two-value conversion and MaxPool2d(3,2,1) on order-preserving integer keys (the fused conv + pool kernels).  Device code
// only: include it from .hip files; the host-visible declarations are in common.h.  gfx950 (64-lane waves).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;      // ds_read_b64_tr_b16 operand
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}
// sum over a 256-thread block, result valid in thread 0; sbuf >= 4 entries
template <typename T>
__device__ __forceinline__ T block_sum256(T v, T* sbuf) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sbuf[w] = v;
    __syncthreads();
    return sbuf[0] + sbuf[1] + sbuf[2] + sbuf[3];
}

__device__ __forceinline__ unsigned short f2bf(float x) {
    __bf16 h = (__bf16)x;                                   // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
    return __builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
// the low / high bf16 of a dword of two, as fp32 (element k of eight bf16 in a uint4's words w[4]: (k & 1) ? bfw_hi(w[k >> 1]) : bfw_lo(w[k >> 1]))
__device__ __forceinline__ float bfw_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bfw_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// two fp32 -> one dword of two bf16 (lo in bits 0..15), round to nearest even: ONE v_cvt_pk_bf16_f32 (converting the halves
// separately costs two converts + and + shift + or)
typedef float mi_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mi_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned mi_pk_bf16(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((mi_f32x2){lo, hi}, mi_bf16x2));
}

// ---- MaxPool2d(3,2,1) on order-preserving integer keys (the fused conv+pool kernels are VALU-issue bound, and a float
// compare + two selects per (window position, channel) was most of their instruction count).
// key16(v): signed-int16 order == float order of the bf16 value, -0 and +0 share a key.  The conv epilogue stores keys, the
// pooling widens a key to the high half of a dword and puts (8 - window position) in the low bits: ONE v_max3_i32 per
// three positions then yields the maximum AND its first row-major position (ties: larger low bits = earlier position --
// the `v > best` rule of torch's max_pool2d and of the stand-alone kernel in pool.hip).  A positive NaN sorts above +inf
// and so propagates; cells outside the image hold MI_KEY_MIN.
typedef short mi_s16x2 __attribute__((ext_vector_type(2)));
constexpr unsigned MI_KEY_MIN2 = 0x80008000u;                 // two minimal keys
__device__ __forceinline__ unsigned mi_bf16x2_to_keys(unsigned w) {
    const mi_s16x2 v = __builtin_bit_cast(mi_s16x2, w), s = v >> (mi_s16x2){15, 15};          // 0 / -1 per half
    return __builtin_bit_cast(unsigned, (mi_s16x2)((v ^ (s & (mi_s16x2){0x7fff, 0x7fff})) - s));
}
__device__ __forceinline__ unsigned mi_keys_to_bf16x2(unsigned kk) {
    mi_s16x2 k = __builtin_bit_cast(mi_s16x2, kk);
    const mi_s16x2 s = k >> (mi_s16x2){15, 15};
    k = k + s;
    return __builtin_bit_cast(unsigned, (mi_s16x2)(k ^ (s & (mi_s16x2){0x7fff, 0x7fff})));
}
__device__ __forceinline__ int mi_max3i(int a, int b, int c) { return max(max(a, b), c); }
// u[p] = the 8 channel keys (4 dwords) of window position p = ky*3 + kx; val = 8 pooled bf16, arg = 8 position bytes
__device__ __forceinline__ void mi_pool9_keys(const uint4 (&u)[9], uint4& val, uint2& arg) {
    int best[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int k[9];
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const unsigned w = (q >> 1) == 0 ? u[p].x : (q >> 1) == 1 ? u[p].y : (q >> 1) == 2 ? u[p].z : u[p].w;
            k[p] = (int)((q & 1) ? ((w & 0xffff0000u) | (unsigned)(8 - p)) : ((w << 16) | (unsigned)(8 - p)));
        }
        best[q] = mi_max3i(mi_max3i(k[0], k[1], k[2]), mi_max3i(k[3], k[4], k[5]), mi_max3i(k[6], k[7], k[8]));
    }
    unsigned kv[4], lo[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) kv[j] = ((unsigned)best[2 * j] >> 16) | ((unsigned)best[2 * j + 1] & 0xffff0000u);
#pragma unroll
    for (int j = 0; j < 2; ++j)        // low bytes of four keys = 8 - position
        lo[j] = __builtin_amdgcn_perm(__builtin_amdgcn_perm((unsigned)best[4 * j + 3], (unsigned)best[4 * j + 2], 0x0c0c0400u),
                                      __builtin_amdgcn_perm((unsigned)best[4 * j + 1], (unsigned)best[4 * j], 0x0c0c0400u), 0x05040100u);
    val = (uint4){mi_keys_to_bf16x2(kv[0]), mi_keys_to_bf16x2(kv[1]), mi_keys_to_bf16x2(kv[2]), mi_keys_to_bf16x2(kv[3])};
    arg = (uint2){0x08080808u - lo[0], 0x08080808u - lo[1]};
}
// ReLU of two packed bf16 as a signed 16-bit max with 0: one v_pk_max_i16.  Every half with its sign bit set (-0 and negative NaNs included)
// becomes +0, every other half keeps its bits -- the same bits for every input as the shift / mask / multiply form this replaces (4 instructions).
__device__ __forceinline__ unsigned mi_relu_bf16x2(unsigned w) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(mi_s16x2, w), (mi_s16x2){0, 0}));
}
__device__ __forceinline__ float mi_bf16x4_lane(uint2 w, int r) {          // bf16 element r (0..3) of an 8-byte word, widened
    const unsigned u = (r >> 1) ? w.y : w.x;
    return (r & 1) ? bfw_hi(u) : bfw_lo(u);
}
__device__ __forceinline__ uint2 mi_pk_bf16x4(const float (&v)[4]) { return (uint2){mi_pk_bf16(v[0], v[1]), mi_pk_bf16(v[2], v[3])}; }
