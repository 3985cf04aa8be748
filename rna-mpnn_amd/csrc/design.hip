// rnampnn_design: S constrained sequences per RNA drawn from f32 logits and scored, in ONE launch.  Three constraints meet in the draw of
// a position: `allowed` (a 4-bit set of classes: a fixed nucleotide, an IUPAC code, an omitted letter), `partner` (the two ends of a base
// pair of the target secondary structure are drawn TOGETHER, from the joint distribution over the compatible cells AU UA CG GC [+ GU UG])
// and `bias` (added to the logits, global or per position).  The reference has no sampler; the contract is the one include/rnampnn_hip.h
// documents and tests/_design_ref.py restates in float64.
// The mask, the row, the validated partner and the draw rule (weights, selection, the pair's joint cell) are design_dev.h's, instantiated
// in f32; the other four design kernels instantiate the same templates in fp64.  The draw is fused into the walk over the rows, so the
// walk is written out here and not taken from ds_write_rows, which serves the kernels that draw into LDS first.  One 256-thread workgroup per (RNA, sample) as in score.hip, the same extent (sc_extent), the same walk over the rows,
// the same per-row NLL and the same reduction (score_dev.h), so `seq_nll` is byte for byte what rnampnn_score returns for the draws.  Both
// ends of a pair compute the pair's cell on their own (the partner's row is one more 16-byte load) and each writes its own component: no
// exchange between threads, so a pair may span waves or 256-strides.  No workspace, no runtime fill / copy node, no atomics, no host
// synchronisation; the draw is a pure function of (seed, s, b, t) and the rows it reads.
#include "design_dev.h"

namespace {
using DsPosF = DsPos<float>;

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
        float4 x;
        bool empty, empty_j;
        const DsPosF p = ds_load<float>(a, pad0, row0, t, x, empty);
        bad += empty ? 1 : 0;
        const int j = ds_partner(a, pad0, n, t);
        int q = -1;
        if (j >= 0) {
            const DsPosF pj = ds_load<float>(a, pad0, row0, j, empty_j);
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
    const int rc = ds_prepare("rnampnn_design", "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner,
                              wobble, bias, bias_per_position, seqs, seq_nll, infeasible, a, [](int) { return RNAMPNN_OK; });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible) return RNAMPNN_OK;    // nothing asked for
    const int passes = (seqs || seq_nll) ? S : 1;               // the count of infeasible positions is that of sample 0
    hipLaunchKernelGGL(k_design, dim3(B, passes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
