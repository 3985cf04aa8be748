// What rnampnn_design_avoid (design_avoid.hip) and rnampnn_design_avoid_profile (design_profile.hip) share about the chain over
// (position x automaton state), as count_tree_dev.h serves the entries on the count tree: the automaton's constants and arguments, the
// entry's checks of them and the refusal of base pairs (av_prepare), and the bytes of the rows, the table and the masks (av_rows_bytes),
// to which each kernel's byte formula adds its own part.  Each kernel carves its own LDS (the masks sit in different places) and keeps
// its own statements for the automaton half of phase A and for phase B (the backward table l_t(a)): folded into two helpers they
// compiled to the same loop instructions at another code offset, and every avoid variant measured 1.0 .. 1.5 % slower
// (docs/experiments.md, Round 15) - so the two texts stay, and tests/test_design_profile_gpu.py holds the profile to the draw's flags.
// The row loop of phase A alone is design_dev.h's ds_rows_to_lds, within the spread on every avoid variant (Round 18).
#pragma once
#include "design_dev.h"

namespace {
constexpr int AV_MAX_STATES = RNAMPNN_DESIGN_AVOID_MAX_STATES;
static_assert(AV_MAX_STATES == 64, "one lane of a wave per state; `terminal` is one 64-bit word");
constexpr unsigned AV_DEAD = 0xFFu;            // the column of a transition into a terminal state or out of the automaton

struct AvChainArgs : DesignArgs {
    const uint8_t* delta;        // (A,4)
    unsigned long long terminal;
    int A, live;                 // states, live states
};

// the bytes both kernels spend on (T, live states): the fp64 rows, the table and the masks, as include/rnampnn_hip.h gives them
inline size_t av_rows_bytes(long long T, long long live) {
    const size_t t = (size_t)T;
    return (32 + 8 * (size_t)live) * t + 16 * ((t + 15) / 16);
}

// The prologue of both entries: ds_prepare with the automaton's checks in slot 0 and the entry's `own1` in slot 1, the refusal of base
// pairs, then the chain's fields - `terminal` cut to the states the automaton has, `live` counted from it.  (`miss` stays with each
// kernel's own arguments, where the kernels have it today: the argument layout is part of the code they compile to.)
template <typename Own1>
int av_prepare(const char* name, const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
               float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed, const int32_t* partner,
               int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs, float* seq_nll, int32_t* infeasible,
               const uint8_t* delta, int32_t n_states, uint64_t terminal, AvChainArgs& a, Own1 own1) {
    const int rc = ds_prepare(name, "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                              bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0 && !delta) return fail(RNAMPNN_ERR_BAD_ARG, "%s: null delta", name);
        if (slot == 0 && (n_states < 1 || n_states > AV_MAX_STATES))
            return fail(RNAMPNN_ERR_BAD_ARG, "%s: n_states = %d, an automaton has 1 .. %d states", name, (int)n_states, AV_MAX_STATES);
        if (slot == 0 && (terminal & 1ull)) return fail(RNAMPNN_ERR_BAD_ARG, "%s: state 0, the start, is marked terminal", name);
        return slot == 1 ? own1() : RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (partner)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: base pairs (a non-null partner) are not built together with forbidden motifs: a pair couples two "
                    "distant positions, so an exact chain over (position, automaton state) would carry the class of every open pair in its "
                    "state, 4^depth states", name);
    const unsigned long long in_range = n_states == 64 ? ~0ull : ((1ull << n_states) - 1ull);
    a.delta = delta; a.terminal = terminal & in_range; a.A = n_states; a.live = n_states - __builtin_popcountll(terminal & in_range);
    return RNAMPNN_OK;
}
}  // namespace
