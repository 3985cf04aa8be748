// Device primitives shared by the translation units with training kernels (kernels_train.hip, rdesign_train.hip, rdesign_train_bf16.hip): on top of
// bf16_core.h (bf16 packs, MFMA, gelu_erf, gelu_fast / phi_fast) the derivatives of both GELU forms, the row count of a TRows, and the dropout
// counter hash.  ONE definition: every kernel of the trainer and oracle/rnampnn_oracle.py: dropout_multiplier must
// agree on the mask bit for bit.  Include from device code only.
#pragma once
#include "kernels_train.h"
#include "bf16_core.h"

__device__ __forceinline__ float gelu_d(float x) {     // d/dx [x Phi(x)] = Phi(x) + x phi(x)
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}
__device__ __forceinline__ int nrows(const TRows& r) { return *r.ntot * r.mul; }
// dropout multiplier of one element: 0 or 1/(1-p) (kernels_train.h: TDrop; restated by the oracle's dropout_multiplier).
__device__ __forceinline__ unsigned drop_key(const TDrop& d, unsigned site) {         // wave-uniform part of the hash input
    const unsigned long long sd = d.seed_dev ? *d.seed_dev : d.seed;
    return site * 0x85EBCA6Bu + (unsigned)sd + (unsigned)(sd >> 32) * 0x27D4EB2Fu;
}
__device__ __forceinline__ unsigned drop_hash(unsigned x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float drop_mul(const TDrop& d, unsigned site, unsigned long long idx) {
    if (d.thresh == 0u) return 1.f;
    const unsigned long long P = idx >> 1;
    const unsigned x = drop_hash((unsigned)P + (unsigned)(P >> 32) * 0xC2B2AE35u + drop_key(d, site));
    return ((idx & 1ull) ? x >> 16 : x & 0xffffu) >= d.thresh ? d.scale : 0.f;
}
// both elements of pair P (element indices 2P, 2P + 1) when P is known to fit 32 bits (every [rows][D] tensor of the trainer: the
// entry points bound rows * D / 2 < 2^32); key = drop_key(d, site)
__device__ __forceinline__ void drop_pair(const TDrop& d, unsigned key, unsigned P, float& m0, float& m1) {
    if (d.thresh == 0u) { m0 = 1.f; m1 = 1.f; return; }
    const unsigned x = drop_hash(P + key);
    m0 = (x & 0xffffu) >= d.thresh ? d.scale : 0.f;
    m1 = (x >> 16) >= d.thresh ? d.scale : 0.f;
}
// the 8 multipliers of elements 8 * P8 .. 8 * P8 + 7  (P8 = element index / 8)
__device__ __forceinline__ void drop8(const TDrop& d, unsigned key, unsigned P8, float (&m)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) drop_pair(d, key, 4u * P8 + q, m[2 * q], m[2 * q + 1]);
}
// The derivative of gelu_fast (bf16_core.h) for the fused prologues / epilogues of the bf16-mixed GEMMs: Phi + x phi with the same sigmoid-form
// Phi (below the bf16 rounding of the operands these values are converted to).  The f32 kernels (parity grade) keep erff.
__device__ __forceinline__ float gelu_d_fast(float x) {
    return fmaf(x * 0.3989422804f, __builtin_amdgcn_exp2f(x * x * -0.72134752f), phi_fast(x));
}
__device__ __forceinline__ void gelu_both_fast(float x, float& g, float& d) {          // (gelu_fast(x), gelu_d_fast(x)) sharing the sigmoid
    const float sg = phi_fast(x);
    g = x * sg;
    d = fmaf(x * 0.3989422804f, __builtin_amdgcn_exp2f(x * x * -0.72134752f), sg);
}
