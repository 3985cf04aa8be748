// rnampnn_design: S constrained sequences per RNA drawn from f32 logits and scored, in ONE launch.  Three constraints meet in the draw of
// a position: `allowed` (a 4-bit set of classes: a fixed nucleotide, an IUPAC code, an omitted letter), `partner` (the two ends of a base
// pair of the target secondary structure are drawn TOGETHER, from the joint distribution over the compatible cells AU UA CG GC [+ GU UG])
// and `bias` (added to the logits, global or per position).  The reference has no sampler; the contract is the one include/rnampnn_hip.h
// documents and tests/_design_ref.py restates in float64.
// The draw rule (weights, selection, the pair's joint cell) is design_dev.h's, instantiated in f32; k_design_tied instantiates the same
// templates in fp64.  One 256-thread workgroup per (RNA, sample) as in score.hip, the same extent (sc_extent), the same walk over the rows,
// the same per-row NLL and the same reduction (score_dev.h), so `seq_nll` is byte for byte what rnampnn_score returns for the draws.  Both
// ends of a pair compute the pair's cell on their own (the partner's row is one more 16-byte load) and each writes its own component: no
// exchange between threads, so a pair may span waves or 256-strides.  No workspace, no runtime fill / copy node, no atomics, no host
// synchronisation; the draw is a pure function of (seed, s, b, t) and the rows it reads.
#include "design_dev.h"

namespace {
using DsPosF = DsPos<float>;

// row t of RNA b.  A mask that admits no class is drawn as free; `empty` tells the caller to count it.
__device__ __forceinline__ DsPosF ds_load(const DesignArgs& a, size_t pad0, long long row0, int t, float4& x, bool& empty) {
    x = a.logits[row0 + t];
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bi = a.bias_per_position ? reinterpret_cast<const float4*>(a.bias)[pad0 + t] : make_float4(a.bias[0], a.bias[1], a.bias[2], a.bias[3]);
    DsPosF p;
    p.z[0] = (x.x + bi.x) / a.temperature; p.z[1] = (x.y + bi.y) / a.temperature;
    p.z[2] = (x.z + bi.z) / a.temperature; p.z[3] = (x.w + bi.w) / a.temperature;
    const int m = a.allowed ? (a.allowed[pad0 + t] & 15) : 15;
    empty = m == 0;
    p.m = empty ? 15 : m;
    return p;
}

__global__ void __launch_bounds__(SC_THREADS) k_design(DesignArgs a) {
    __shared__ int s_i[SC_WAVES];
    __shared__ float s_f[2][SC_WAVES];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    int n;
    long long row0;
    sc_extent(a, b, tid, s_f[0], n, row0);
    const size_t pad0 = (size_t)b * a.T;
    int8_t* seq = a.seqs ? a.seqs + ((size_t)s * a.B + b) * a.T : nullptr;
    int bad = 0;
    float nll = 0.f, unused = 0.f;
    for (int t = tid; t < n; t += SC_THREADS) {
        float4 x, xj;
        bool empty, empty_j;
        const DsPosF p = ds_load(a, pad0, row0, t, x, empty);
        bad += empty ? 1 : 0;
        // paired only when the table is symmetric and stays inside the RNA: every index is checked before it is used
        int j = a.partner ? a.partner[pad0 + t] : -1;
        if (j < 0 || j >= n || j == t || a.partner[pad0 + j] != t) j = -1;
        int q = -1;
        if (j >= 0) {
            const DsPosF pj = ds_load(a, pad0, row0, j, xj, empty_j);
            const bool first = t < j;
            const int cell = ds_draw_pair(first ? p : pj, first ? pj : p, a.wobble, ds_u24(seed, s, b, first ? t : j));
            if (cell >= 0) q = first ? (cell >> 2) : (cell & 3);
            else bad += 1;                                          // each end counts itself: 2 per pair
        }
        if (q < 0) q = ds_draw_single(p, ds_u24(seed, s, b, t));
        if (seq) seq[t] = (int8_t)q;
        if (a.seq_nll) nll += sc_row_nll(x, q);
    }
    if (seq)
        for (int t = n + tid; t < a.T; t += SC_THREADS) seq[t] = (int8_t)-1;
    sc_block_sums(bad, nll, unused, tid, s_i, s_f);
    if (tid != 0) return;
    if (a.seq_nll) a.seq_nll[(size_t)s * a.B + b] = nll;
    if (a.infeasible && s == 0) a.infeasible[b] = bad;
}
}  // namespace

extern "C" int rnampnn_design(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                              float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                              const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs,
                              float* seq_nll, int32_t* infeasible, void* stream) {
    DesignArgs a{};
    const ScDraw draw{S, "RNA", temperature, bias, bias_per_position};
    const int rc = sc_check_args("rnampnn_design", logits, n_rows, mask, cu_seqlens, B, T, &draw, a, [](int) { return RNAMPNN_OK; });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible) return RNAMPNN_OK;    // nothing asked for
    ds_fill(a, seed, seed_dev, allowed, partner, wobble, bias, bias_per_position, temperature, seqs, seq_nll, infeasible);
    const int passes = (seqs || seq_nll) ? S : 1;               // the count of infeasible positions is that of sample 0
    hipLaunchKernelGGL(k_design, dim3(B, passes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
