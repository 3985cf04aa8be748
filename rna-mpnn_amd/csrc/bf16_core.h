// The bf16 device primitives every translation unit with bf16 or training kernels shares - ONE definition each: vector types, round-to-nearest-even
// conversions and packs, the 32x32x16 bf16 MFMA, the two GELU forms and kSEPS.  Precision-neutral: what is specific to the f16 / fused inference
// kernels stays in bf16_dev.h, GELU's derivatives and the dropout hash of the trainers in train_dev.h (both include this).  Device code only.
#pragma once
#include "rnampnn_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

static constexpr float kSEPS = 1.0e-6f;

__device__ __forceinline__ bf16_t f2bf(float x) { return __builtin_bit_cast(bf16_t, (__bf16)x); }   // RNE, NaN kept
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ unsigned pack2(float a, float b) {        // one v_cvt_pk_bf16_f32: two RNE bf16 in one word, a in the low half
    f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float lo_bf(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_bf(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
// 8 consecutive elements of a row <-> the four words of a 16-byte bf16 chunk
__device__ __forceinline__ u32x4 pack8(const float (&v)[8]) {
    return u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
}
__device__ __forceinline__ void unpack8(const u32x4& u, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = lo_bf(u[i]); v[2 * i + 1] = hi_bf(u[i]); }
}

__device__ __forceinline__ f32x16 mfma32(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// nn.GELU() default (erf form): the f32 paths and the node-level GEMM epilogues
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
// GELU for the bf16 paths: x * Phi(x) with Phi(x) ~ sigmoid(x * (c0 + c1 x^2)), coefficients minimax-fitted to the exact
// erf form (max |x Phi - gelu| 2.7e-4 at |x| ~ 2-3, 15-30x below the bf16 rounding of the result there);
// monotone argument, so no clamp: 7 VALU instructions, 2 of them transcendental.
__device__ __forceinline__ float phi_fast(float x) {
    const float p = fmaf(x * x, -0.10012571f, -2.3087657f);           // -log2(e) * (c0 + c1 x^2), c0 = 1.60031416, c1 = 0.06940179
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * p));          // 1 / (1 + exp(-x (c0 + c1 x^2)))
}
__device__ __forceinline__ float gelu_fast(float x) { return x * phi_fast(x); }
