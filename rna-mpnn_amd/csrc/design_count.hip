// rnampnn_design_count: constrained design conditioned EXACTLY on a count window, in one launch - the count of the positions whose class
// falls in a per-position COUNTED SET (four bits over AUCG).  With the sets 15 ^ (1 << reference id) the count is the Hamming distance to
// a reference sequence, and the window a mutation budget; with C|G everywhere it is rnampnn_design_gc.  The count is a sum over the
// independent units of rnampnn_design (unpaired positions, base pairs), so the draw is the product tree of count polynomials of
// count_tree_dev.h, instantiated with the sets read from the call and degrees truncated at `count_cap`.
// Truncation is exact.  A coefficient c(k) = LSE over a + r = k of L(a) + R(r) reads child coefficients of index <= k only, so with
// k <= cap nothing above the cap is ever needed, at any level; and the candidate range max(0, k - deg_R) .. min(k, deg_L) of a sum or a
// split is the same with capped and uncapped child degrees (k <= cap gives min(k, min(D, cap)) = min(k, D) and k - min(D, cap) =
// max(k - D, k - cap) with k - cap <= 0).  Every sum therefore runs over the same terms in the same order: the outputs of an RNA whose
// window and target lie within the cap do not depend on the cap, byte for byte.  What the cap buys is LDS - node (l, i) holds
// min(2 * positions, T, cap) + 1 doubles, so a budget of 8 fits 2867 nt where the uncapped tree stops at 1017 - and residency.
// When no count of 0 .. min(n, cap) is reachable the target is k_min, the sum over the leaves of the smallest d with a finite p_t(d),
// formed by a workgroup reduction in phase A; every leaf then draws at its own minimum, which is the exact conditional on "count =
// k_min" because the units are independent.  The contract is the one include/rnampnn_hip.h documents and tests/_design_count_ref.py
// restates; all of the draw is fp64.
#include "count_tree_dev.h"

namespace {
// Three workgroups per CU (168 VGPRs, 7 of them spilled) rather than the 197 VGPRs the compiler takes unasked (two per CU, no spill): the
// kernel is latency-bound, and the two-workgroup form measured 23 .. 29 % slower on every leg (profiles/design_count_kernel_stats.txt).
__global__ void __launch_bounds__(SC_THREADS, 3) k_design_count(CtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char count_lds[];
    ct_design<true>(a, count_lds);
}
}  // namespace

extern "C" int rnampnn_design_count(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                    float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                    const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                    const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap,
                                    int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* count, int32_t* count_miss, void* stream) {
    CtArgs a{};
    const int rc = ds_prepare("rnampnn_design_count", "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed,
                              partner, wobble, bias, bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        return slot == 0 ? ct_count_side("rnampnn_design_count", counted, count_lo, count_hi, count_cap, T, 0, a) : RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible && !count && !count_miss) return RNAMPNN_OK;    // nothing asked for
    size_t lds_tree = 0, lds_sq = 0;
    const size_t lds = ct_lds_bytes(T, a.cap, lds_tree, lds_sq);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED,
                    "rnampnn_design_count: T = %d at count_cap = %d needs %zu bytes of LDS for the count tree, the limit is %zu (T <= %d at that cap)",
                    (int)T, (int)count_cap, lds, DS_LDS_MAX, ct_max_T(count_cap));
    a.count = count; a.miss = count_miss;
    a.lds_tree = (unsigned)lds_tree; a.lds_sq = (unsigned)lds_sq;
    const int passes = (seqs || seq_nll || count) ? S : 1;      // count_miss and the count of infeasible positions are those of sample 0
    return ds_launch<k_design_count>(dim3(B, passes), lds, stream, a);
}
