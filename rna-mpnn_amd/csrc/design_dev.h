// Device pieces shared by the two design kernels, k_design (design.hip) and k_design_tied (design_tied.hip): the uniform of a position and
// the base-pair compatibility sets.  One definition of each, so that one state per group draws from the same uniforms as rnampnn_design.
#pragma once
#include "score_dev.h"

namespace {
__device__ __forceinline__ unsigned ds_u24(unsigned long long seed, int s, int b, int t) {
    unsigned long long h = mix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(s + 1));
    h = mix64(h ^ (0xD6E8FEB86659FD93ull * (unsigned long long)(b + 1)));
    h = mix64(h ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(t + 1)));
    return (unsigned)(h >> 40);
}

// the classes that pair with class a (AUCG = 0..3): A-U, U-A, C-G, G-C, and with wobble G-U, U-G
__device__ __forceinline__ int ds_compat(int a, int wobble) {
    return a == 0 ? 2 : a == 1 ? (wobble ? 9 : 1) : a == 2 ? 8 : (wobble ? 6 : 4);
}
}  // namespace
