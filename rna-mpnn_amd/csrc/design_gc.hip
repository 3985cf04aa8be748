// rnampnn_design_gc: constrained design with a G+C content window, drawn EXACTLY, in one launch.  The model is one-shot, so under the
// constraints of rnampnn_design the distribution factorises over independent units - unpaired positions and base pairs - and the G+C
// count is a sum over the units.  Conditioning on "count in [lo, hi]" is therefore a product tree of count polynomials: the tree, its
// three phases and its selections are count_tree_dev.h's, instantiated with the counted set {C, G} at every position and a cap of T, which
// bounds no degree.  The contract is the one include/rnampnn_hip.h documents and tests/_design_gc_ref.py restates; all of the draw is fp64.
#include "count_tree_dev.h"

namespace {
__global__ void __launch_bounds__(SC_THREADS) k_design_gc(CtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
    ct_design<false>(a, gc_lds);
}
}  // namespace

extern "C" int rnampnn_design_gc(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                 float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                 const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                 const int32_t* gc_lo, const int32_t* gc_hi, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                                 int32_t* gc_count, int32_t* gc_miss, void* stream) {
    CtArgs a{};
    const int rc = ds_prepare("rnampnn_design_gc", "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner,
                              wobble, bias, bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0 && (!gc_lo || !gc_hi)) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design_gc: null gc_lo or gc_hi");
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible && !gc_count && !gc_miss) return RNAMPNN_OK;    // nothing asked for
    size_t lds_tree = 0, lds_sq = 0;
    const size_t lds = ct_lds_bytes(T, T, lds_tree, lds_sq);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_gc: T = %d needs %zu bytes of LDS for the count tree, the limit is %zu (T <= %d)",
                    (int)T, lds, DS_LDS_MAX, ct_max_T(T));
    a.counted = nullptr; a.lo = gc_lo; a.hi = gc_hi; a.count = gc_count; a.miss = gc_miss; a.cap = T;
    ct_tree_doubles(T, T, a.base);
    a.lds_tree = (unsigned)lds_tree; a.lds_sq = (unsigned)lds_sq;
    const int passes = (seqs || seq_nll || gc_count) ? S : 1;   // gc_miss and the count of infeasible positions are those of sample 0
    return ds_launch<k_design_gc>(dim3(B, passes), lds, stream, a);
}
