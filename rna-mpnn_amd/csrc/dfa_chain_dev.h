// What the entries on the 256-state automaton share - rnampnn_design_dfa (design_dfa.hip), rnampnn_design_dfa_count
// (design_dfa_count.hip), rnampnn_design_nested (design_nested.hip) and the profile rnampnn_design_dfa_profile (design_dfa_profile.hip) -
// as avoid_chain_dev.h serves the two entries on the 64-state chain: the automaton's constants, the pure helpers (dfa_words, dfa_bit, dfa_column), the automaton's arguments as a mixin over the entry's base
// (DfaChainArgs), the host prologue (dfa_prepare) and the device pieces that are the same statements in every kernel: the automaton half
// of phase A (dfa_load_state, dfa_load_delta: dfa and nested), one step of the automaton (dfa_advance), the read of a 2-bit draw (dfa_drawn) and the
// candidates of one step of the forward walk of k_design_dfa and k_design_dfa_count (dfa_walk_step<COUNTED>), and phase B of k_design_dfa
// and k_design_dfa_profile (dfa_rows_init, dfa_backward; Round 18).  All of them are
// __forceinline__ and hold the statements in the order the kernels had them; each fold was held against the compiler's resource report
// and the kernels' times (docs/experiments.md, Round 17): with these the three kernels use the registers of their own texts, and
// k_design_nested compiles to its own text's instructions.
// What stays with each kernel: its LDS carve-up, its own arrays of phase A (`col` as 16-bit columns, `dl` by live column, `of` / `ac`),
// phase B of dfa_count and nested - flat dealing over (column, k), transfer tables with tiles: two other loops than dfa's thread per
// state - the LDS byte formula, the LDS-ceiling message and, in design_nested.hip, NS_MAX_LIVE and the walk of the tree.  And
// the CHUNK EPILOGUE, the loop of ds_write_rows over a chunk's samples with its barrier: as one function it cost every kernel 2 - 4 VGPRs
// and measured k_design_dfa 1.6 % slower at 73 live states and k_design_nested 0.5 - 0.7 % slower (the same round), so the seven lines
// stand in each kernel, as avoid_chain_dev.h keeps the phases of the avoid kernels.  k_design_dfa_count keeps its own phase-A load for
// the same reason: it fills `of` between the stores of `own` and `kd`, and through the two functions its G+C variant measured 1.5 % slower.
#pragma once
#include <cstdio>
#include "design_dev.h"

namespace {
constexpr int DFA_MAX_STATES = RNAMPNN_DESIGN_DFA_MAX_STATES;
static_assert(DFA_MAX_STATES == SC_THREADS, "one thread of the workgroup per state");
constexpr int DFA_CHUNK = SC_THREADS;          // samples that walk together: one lane each
constexpr unsigned DFA_DEAD = 0xFFFFu;         // a 16-bit column (dfa, dfa_count): a transition into a dead state or out of the automaton
constexpr unsigned DFA_DEAD8 = 0xFFu;          // the same mark where a column is a byte (nested: at most 64 live states)
constexpr size_t DFA_LDS_SCRATCH = 96;         // the reduction's DS_SCRATCH bytes, padded (dfa_count keeps its target behind them)
static_assert(DS_SCRATCH <= DFA_LDS_SCRATCH, "the reduction's scratch");

// The automaton's arguments behind the entry's base: DesignArgs (dfa, nested) or CtArgs (dfa_count, whose `miss` is the count side's).
// `More`: what an entry keeps behind `tab` (nested: its goal stacks) - the argument layout is part of what the kernels compile to, so every
// kernel keeps the order of fields it had; an empty More takes no room.
struct DfaNoMore {};
template <class Base, class More = DfaNoMore>
struct DfaChainArgs : Base {
    const uint8_t* delta;        // (A,4), device
    unsigned long long dead[4];  // bit a set = state a is dead; set for every a >= A
    unsigned long long acc[4];   // bit a set = state a is live and accepting
    double* tab;                 // the caller's workspace: the entry's table(s), [b][t][live column]...
    [[no_unique_address]] More more;
    int A, live, S, words;       // states, live states, samples, 32-bit words of one sample's draws
    int32_t* hits;               // (S,B) or null
    int32_t* accepted;           // (S,B) or null
    int32_t* dfa_miss;           // (B) or null
};
static_assert(sizeof(DfaChainArgs<DesignArgs>) == sizeof(DesignArgs) + 8 + 2 * 32 + 8 + 4 * 4 + 3 * 8, "an empty More takes no room");

// the words of one sample's draws: 2 bits per position, an odd count (lanes a word stride apart fall into different banks)
__host__ __device__ inline int dfa_words(int T) { return ((T + 15) / 16) | 1; }

__device__ __forceinline__ bool dfa_bit(const unsigned long long (&set)[4], unsigned a) {
    const unsigned long long w = (a >> 6) == 0 ? set[0] : (a >> 6) == 1 ? set[1] : (a >> 6) == 2 ? set[2] : set[3];
    return (w >> (a & 63u)) & 1ull;
}

// the live states below a: the table column of a live state a
__device__ __forceinline__ int dfa_column(const unsigned long long (&dead)[4], unsigned a) {
    int k = 0;
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
        const unsigned long long below = j < (a >> 6) ? ~0ull : j == (a >> 6) ? ((1ull << (a & 63u)) - 1ull) : 0ull;
        k += __popcll(~dead[j] & below);
    }
    return k;
}

// The prologue of the four entries: ds_prepare with the automaton's four checks and then the entry's `own0` in slot 0 and the workspace
// check in slot 1, the refusal of base pairs where the entry has one, then the automaton's fields.  `kind` is read once: the same loop
// counts `live` for the workspace check and fills dead[] / acc[].  `need(live, what, n)` -> the bytes the workspace must hold, and in
// `what` the entry's words for it up to the number ("the table of partition sums at (...) needs").  NS_MAX_LIVE, the LDS ceiling and
// "nothing asked for" stay with the entry: their words are its own.  -> RNAMPNN_OK or what fail() returned.
template <class Base, class More, typename Own0, typename Need>
int dfa_prepare(const char* name, const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed, const int32_t* partner,
                int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace, size_t workspace_bytes, int32_t* hits,
                int32_t* accepted, int32_t* dfa_miss, bool refuse_pairs, DfaChainArgs<Base, More>& a, Own0 own0, Need need) {
    const int rc = ds_prepare(name, "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                              bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0 && !delta) return fail(RNAMPNN_ERR_BAD_ARG, "%s: null delta", name);
        if (slot == 0 && !kind) return fail(RNAMPNN_ERR_BAD_ARG, "%s: null kind (a HOST array of n_states bytes)", name);
        if (slot == 0 && (n_states < 1 || n_states > DFA_MAX_STATES))
            return fail(RNAMPNN_ERR_BAD_ARG, "%s: n_states = %d, an automaton has 1 .. %d states", name, (int)n_states, DFA_MAX_STATES);
        if (slot == 0 && (kind[0] & 1)) return fail(RNAMPNN_ERR_BAD_ARG, "%s: state 0, the start, is marked dead", name);
        if (slot == 0) return own0();
        a.live = 0;
        for (int w = 0; w < 4; ++w) { a.dead[w] = ~0ull; a.acc[w] = 0; }
        for (int s = 0; s < n_states; ++s) {
            if (kind[s] & 1) continue;
            a.dead[s >> 6] &= ~(1ull << (s & 63));
            if (kind[s] & 2) a.acc[s >> 6] |= 1ull << (s & 63);
            ++a.live;
        }
        char what[160];
        const size_t bytes = need(a.live, what, sizeof what);
        if (!workspace || workspace_bytes < bytes)
            return fail(RNAMPNN_ERR_BAD_ARG, "%s: the workspace is %s (%zu bytes), %s %zu (%s_workspace_bytes)", name,
                        workspace ? "too small" : "null", workspace_bytes, what, bytes, name);
        if (((uintptr_t)workspace & 7) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: the workspace must be 8-byte aligned", name);
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (refuse_pairs && partner)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: base pairs (a non-null partner) are not built together with an automaton: a pair couples two "
                    "distant positions, so an exact chain over (position, automaton state) would carry the class of every open pair in its "
                    "state, 4^depth states", name);
    a.delta = delta; a.A = n_states; a.S = S; a.words = dfa_words(T);
    a.tab = reinterpret_cast<double*>(workspace);
    a.hits = hits; a.accepted = accepted; a.dfa_miss = dfa_miss;
    return RNAMPNN_OK;
}

// Phase A, thread = state: whether state tid is live and accepts and its column (or `dead_mark`); the column goes into own[], the kind
// into kd[] (bit 0 dead, bit 1 accepting).  A barrier follows before dfa_load_delta reads own[].  (Returned, not written through
// references: with out-parameters the kernels compiled to other code than their own statements had.)
struct DfaState { bool live, accepts; unsigned mine; };
template <class Args, typename Col>
__device__ __forceinline__ DfaState dfa_load_state(const Args& a, int A, int tid, unsigned dead_mark, Col* own, unsigned char* kd) {
    const bool live = tid < A && !dfa_bit(a.dead, tid);
    const bool accepts = live && dfa_bit(a.acc, tid);
    const unsigned mine = live ? (unsigned)dfa_column(a.dead, tid) : dead_mark;
    own[tid] = (Col)mine;
    kd[tid] = (unsigned char)((live ? 0 : 1) | (accepts ? 2 : 0));
    return DfaState{live, accepts, mine};
}

// Phase A, thread = state: delta(tid, .) a byte per class into nx[]; each(c, next state, its column or `dead_mark`) lets the kernel pack
// the columns the way its own arrays hold them.
template <class Args, typename Col, typename Each>
__device__ __forceinline__ void dfa_load_delta(const Args& a, int tid, unsigned dead_mark, const Col* own, unsigned* nx, Each each) {
    unsigned raw = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned nxt = tid < a.A ? a.delta[4 * tid + c] : 0xFFu;
        const unsigned k = tid < a.A && nxt < (unsigned)a.A ? own[nxt] : dead_mark;
        raw |= (nxt & 255u) << (8 * c);
        each(c, nxt, k);
    }
    nx[tid] = tid < a.A ? raw : 0u;
}

// Phase B of k_design_dfa and k_design_dfa_profile, thread = state.  Two pieces, because the kernels load delta between them under the
// barrier the rows need anyway.  dfa_rows_init: l_n into row n & 1 of the two LDS rows [2][256] indexed by state, -inf into the other
// (a dead state's entry is never written again); a barrier follows.  dfa_backward: l_t(a) for t = n-1 .. 0 - the row of t + 1 is read
// through cc[c] = delta(a, c) (0 for a class `ok` does not admit), the row of t written, every live l_t(a) stored to the workspace at
// the state's column, one workgroup barrier per step.  -> miss: l_0 of state 0 is -inf (the loop ends on row 0, and n = 0 starts there).
__device__ __forceinline__ void dfa_rows_init(double* row, int n, int tid, bool accepts) {
    row[(n & 1) * DFA_MAX_STATES + tid] = accepts ? 0.0 : -INFINITY;               // l_n
    row[((n + 1) & 1) * DFA_MAX_STATES + tid] = -INFINITY;
}
__device__ __forceinline__ bool dfa_backward(const double* zs, const unsigned char* ms, double* row, double* tab, const unsigned short* own, int n, int AL,
                                             int tid, bool live, const int (&cc)[4], int ok) {
    const int mine = own[tid];
    for (int t = n - 1; t >= 0; --t) {
        if (live) {
            const double* next = row + ((t + 1) & 1) * DFA_MAX_STATES;
            double l[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) l[c] = next[cc[c]];
            const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
            const double v[4] = {z01.x + l[0], z01.y + l[1], z23.x + l[2], z23.y + l[3]};
            const double lt = ds_lse<4>(v, (int)ms[t] & ok);
            row[(t & 1) * DFA_MAX_STATES + tid] = lt;
            tab[(size_t)t * AL + mine] = lt;
        }
        __syncthreads();
    }
    return !(row[0] > -INFINITY);
}

// One step of the automaton by state number: `step` = nx[st], q the class drawn.  A transition out of the automaton or into a dead state
// is a hit; out of the automaton the walk restarts at state 0.
__device__ __forceinline__ void dfa_advance(unsigned step, int q, int A, const unsigned char* kd, int& st, int& hit) {
    const unsigned nxt = (step >> (8 * q)) & 255u;
    const bool out = nxt >= (unsigned)A;
    hit += out || (kd[nxt] & 1) ? 1 : 0;
    st = out ? 0 : (int)nxt;
}

// the class drawn at position t, from the words of one sample's draws
__device__ __forceinline__ int dfa_drawn(const unsigned* words, int t) { return (int)((words[t >> 4] >> (2 * (t & 15))) & 3u); }

// One step of the forward walk of k_design_dfa and k_design_dfa_count: the four candidates l_{t+1}(delta(a, c)[, r - counted]) from the
// table in the workspace (`next`: the row or slab of t + 1; the last step reads one that exists and uses none of it), the weights and the
// selection.  `cl`: the 16-bit columns of delta(a, .); `step` = nx[a]; COUNTED: `r` the remaining count, `cs` the counted set of the
// position, `cap1` the entries of a column; without it nothing counts and a column is one entry.  -> the class, or -1 when no admitted
// candidate is finite (the caller then draws as rnampnn_design does).
template <bool COUNTED>
__device__ __forceinline__ int dfa_walk_step(const DsPos<double>& p, unsigned u, uint2 cl, unsigned step, const unsigned char* kd, const double* next,
                                             bool last, int cap1, int r, int cs) {
    double v[4];
    int adm = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned kc = ((c < 2 ? cl.x : cl.y) >> (16 * (c & 1))) & 0xFFFFu;
        const int kk = COUNTED ? r - ((cs >> c) & 1) : 0;
        const bool in = ((p.m >> c) & 1) && kc != DFA_DEAD && kk >= 0;
        const double far = next[in ? (COUNTED ? (size_t)kc * cap1 + kk : (size_t)kc) : 0];
        const double end = (kd[(step >> (8 * c)) & 255u] & 2) && kk == 0 ? 0.0 : -INFINITY;
        const double l = !in ? -INFINITY : last ? end : far;
        v[c] = p.z[c] + l;
        adm |= (in && l > -INFINITY ? 1 : 0) << c;
    }
    if (!adm) return -1;
    double w[4];
    ds_weights(v, adm, w);
    return ds_select(w, adm, u);
}
}  // namespace
