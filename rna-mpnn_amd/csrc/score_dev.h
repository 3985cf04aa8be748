// Device pieces shared by the two per-(RNA, pass) kernels on f32 logits, k_score (score.hip) and k_design (design.hip): the extent of an
// RNA in either layout, the NLL of one row and the fixed-order workgroup sums.  One definition of each, so that the likelihood k_design
// writes for its own draws is byte for byte the one k_score returns for them.
#pragma once
#include "api_internal.h"

namespace {
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sc_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The length and the first logits row of RNA b.  Both come from caller data (a mask that need not be the collate's prefix mask, a cu that
// need not be a prefix sum): they are clamped to the tensors' extents, so a malformed input gives meaningless numbers but no out-of-bounds
// access.  The mask row is summed as k_lengths sums it (the forward's own length of the RNA).  Every thread of the workgroup calls it
// (two barriers in the padded layout); s_tmp holds SC_WAVES floats and is free again on return.
__device__ __forceinline__ void sc_extent(const float* mask, const int32_t* cu, long long n_rows, int T, int b, int tid, float* s_tmp,
                                          int& n, long long& row0) {
    if (cu) {
        const long long lo = min(max((long long)cu[b], 0ll), n_rows);
        const long long len = min(max((long long)cu[b + 1] - (long long)cu[b], 0ll), (long long)T);
        n = (int)min(len, n_rows - lo);
        row0 = lo;
        return;
    }
    float s = 0.f;
    for (int t = tid; t < T; t += SC_THREADS) s += mask[(size_t)b * T + t];
    s = sc_wave_sum(s);
    if ((tid & 63) == 0) s_tmp[tid >> 6] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) tot += s_tmp[w];
    __syncthreads();                                           // s_tmp is reused by the reductions below
    n = tot >= 0.f ? (int)fminf(tot + 0.5f, (float)T) : 0;      // (a NaN sum compares false: 0)
    n = min(max(n, 0), T);
    row0 = (long long)b * T;
}

// logsumexp(x) - x[q]: the NLL of class q under one row of logits (any q outside 0..2 reads class 3)
__device__ __forceinline__ float sc_row_nll(const float4 x, int q) {
    const float m = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
    const float se = (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
    const float xl = q == 0 ? x.x : q == 1 ? x.y : q == 2 ? x.z : x.w;
    return (m - xl) + logf(se);
}

// The workgroup's totals of (cnt, nll, loss): wave butterfly, then one LDS hop over the four waves in ascending order.  Valid in thread 0
// only; every thread calls it (one barrier).  s_i holds SC_WAVES ints, s_f 2 x SC_WAVES floats.
__device__ __forceinline__ void sc_block_sums(int& cnt, float& nll, float& loss, int tid, int* s_i, float (*s_f)[SC_WAVES]) {
    cnt = sc_wave_sum(cnt);
    nll = sc_wave_sum(nll);
    loss = sc_wave_sum(loss);
    if ((tid & 63) == 0) { s_i[tid >> 6] = cnt; s_f[0][tid >> 6] = nll; s_f[1][tid >> 6] = loss; }
    __syncthreads();
    if (tid != 0) return;
    cnt = 0; nll = 0.f; loss = 0.f;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { cnt += s_i[w]; nll += s_f[0][w]; loss += s_f[1][w]; }
}
}  // namespace
