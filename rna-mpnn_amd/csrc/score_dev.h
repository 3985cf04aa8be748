// Pieces shared by the per-(RNA, pass) kernels on f32 logits - k_score (score.hip) and the six design kernels k_design, k_design_tied,
// k_design_gc, k_design_count, k_design_distinct and k_design_avoid (through design_dev.h) - and by k_rd_score (rdesign_score.hip): the argument checks
// of rnampnn_score and, through ds_prepare, of the six design entries, the extent of an RNA in either layout, the first-maximum argmax
// and the NLL of one row, and the fixed-order workgroup sums.  One definition of each, so that the likelihood every design kernel writes
// for its own draws is byte for byte the one k_score returns for them.
#pragma once
#include "api_internal.h"

namespace {
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;

struct ScRows {                  // the logits of a batch in either layout: what the three kernels' argument structs start with
    const float4* logits;        // (B*T) or (n_rows) rows of 4
    const float* mask;           // (B,T) prefix mask, or null
    const int32_t* cu;           // (B+1), or null
    int B, T;
    long long n_rows;            // rows the logits tensor holds
};
struct ScDraw { int S; const char* per; float temperature; const float* bias; int bias_per_position; };   // what only a design entry checks

// The argument checks rnampnn_score and the six design entries share, in the order they fire, and the fields of ScRows.
// `draw`: the S / temperature / bias checks of a design entry (null for rnampnn_score).  `own(slot)`: the entry's own checks that fire
// in between - slot 0 after the batch check, slot 1 after the alignment checks; it returns what fail() returned, or RNAMPNN_OK.
template <typename Own>
int sc_check_args(const char* name, const float* logits, int64_t n_rows, const float* mask, const int32_t* cu, int32_t B, int32_t T,
                  const ScDraw* draw, ScRows& a, Own own) {
    if (!logits || B <= 0 || T <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: null logits or empty batch (B = %d, T = %d)", name, (int)B, (int)T);
    if (int rc = own(0)) return rc;
    if (draw && draw->S <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: S = %d sequences per %s", name, draw->S, draw->per);
    if (draw && draw->S + 1 > 65535) return fail(RNAMPNN_ERR_BAD_ARG, "%s: at most 65534 sequences per call", name);
    if ((mask != nullptr) == (cu != nullptr))
        return fail(RNAMPNN_ERR_BAD_ARG, "%s: pass exactly one of mask (padded logits) and cu_seqlens (packed logits)", name);
    if (draw && (!(draw->temperature > 0.f) || !(draw->temperature <= 3.402823466e38f)))
        return fail(RNAMPNN_ERR_BAD_ARG, "%s: the temperature must be positive and finite (got %g)", name, (double)draw->temperature);
    if (((uintptr_t)logits & 15) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: logits must be 16-byte aligned", name);
    if (draw && draw->bias && draw->bias_per_position && ((uintptr_t)draw->bias & 15) != 0)
        return fail(RNAMPNN_ERR_BAD_ARG, "%s: a per-position bias must be 16-byte aligned", name);
    if (int rc = own(1)) return rc;
    if (cu && n_rows < 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: negative row count", name);
    a.logits = reinterpret_cast<const float4*>(logits);
    a.mask = mask; a.cu = cu;
    a.n_rows = mask ? (long long)B * T : (long long)n_rows;
    a.B = B; a.T = T;
    return RNAMPNN_OK;
}

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
__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the first logits row of batch row b: b * T in the padded layout, cu[b] clamped to the rows the tensor holds in the packed one
__device__ __forceinline__ long long sc_row0(const ScRows& a, int b) {
    return a.cu ? min(max((long long)a.cu[b], 0ll), a.n_rows) : (long long)b * a.T;
}

// The length and the first logits row of RNA b.  Both come from caller data (a mask that need not be the collate's prefix mask, a cu that
// need not be a prefix sum): they are clamped to the tensors' extents, so a malformed input gives meaningless numbers but no out-of-bounds
// access.  The mask row is summed as k_lengths sums it (the forward's own length of the RNA).  Every thread of the workgroup calls it
// (two barriers in the padded layout); s_tmp holds SC_WAVES floats and is free again on return.
__device__ __forceinline__ void sc_extent(const ScRows& a, int b, int tid, float* s_tmp, int& n, long long& row0) {
    const int T = a.T;
    if (a.cu) {
        row0 = sc_row0(a, b);
        const long long len = min(max((long long)a.cu[b + 1] - (long long)a.cu[b], 0ll), (long long)T);
        n = (int)min(len, a.n_rows - row0);
        return;
    }
    float s = 0.f;
    for (int t = tid; t < T; t += SC_THREADS) s += a.mask[(size_t)b * T + t];
    s = sc_wave_sum(s);
    if ((tid & 63) == 0) s_tmp[tid >> 6] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) tot += s_tmp[w];
    __syncthreads();                                           // s_tmp is reused by the reductions below
    n = tot >= 0.f ? (int)fminf(tot + 0.5f, (float)T) : 0;      // (a NaN sum compares false: 0)
    n = min(max(n, 0), T);
    row0 = sc_row0(a, b);
}

// argmax of a row, the first maximum wins (torch.argmax, numpy.argmax, rnampnn_argmax_recovery); m <- the maximum
__device__ __forceinline__ int sc_argmax(const float4 x, float& m) {
    int best = 0;
    m = x.x;
    if (x.y > m) { m = x.y; best = 1; }
    if (x.z > m) { m = x.z; best = 2; }
    if (x.w > m) { m = x.w; best = 3; }
    return best;
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
