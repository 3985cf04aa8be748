// rnampnn_design_dfa: constrained design conditioned EXACTLY on the sequence being accepted by a finite automaton, in one launch - motifs
// that MUST occur somewhere (a "seen" flag per required motif multiplies the Aho-Corasick states) together with motifs that must not
// (rnampnn/utils/motifs.py: DesignAutomaton).  The chain over (position x automaton state) is rnampnn_design_avoid's; three things differ.
// An ACCEPTANCE set ends it: l_n(a) = 0 for a live accepting state and -inf for every other.  The automaton has up to 256 states, one
// THREAD of the workgroup per state instead of one lane of a wave.  And the table of partition sums l_t(a) lives in the caller's
// WORKSPACE in global memory, [b][t][live column], so LDS does not grow with T x L and neither T nor the live states are bound by it.
// The contract is the one include/rnampnn_hip.h documents and tests/_design_dfa_ref.py restates; all of the draw is fp64, and with an
// automaton of at most 64 states in which every live state accepts the outputs are rnampnn_design_avoid's byte for byte: the statements
// that form z, the logsumexp, the weights and the selection are design_dev.h's and stand in the same order.
// One 256-thread workgroup per RNA.  (A) every thread: the fp64 rows and the masks of the RNA into LDS; thread a: the kind and the table
// column of state a, then the columns of delta(a, .).  (B) thread = state: l_t for t = n-1 .. 0; l_{t+1} and l_t sit in two LDS rows
// indexed by state (a dead state's entry stays -inf), one workgroup barrier per step, and every live thread stores its l_t(a) to the
// global table.  (C) 256 samples at a time, one lane per sample: the forward walk reads its four candidates l_{t+1}(delta(a, c)) from the
// global table - written by this workgroup, so a barrier orders them, not a grid sync - 2 bits per position into LDS words the lane owns,
// `hits` and `accepted` from the lane's own integers; then per sample the rows and the NLL as k_design writes them (ds_write_rows).
// No atomics, no fill / copy node, no host synchronisation; every table entry that is read was written by the same launch before.
// dfa_chain_dev.h holds what this entry shares with rnampnn_design_dfa_count and rnampnn_design_nested: the automaton's constants, helpers
// and arguments (DfaChainArgs), the host prologue (dfa_prepare), the automaton half of phase A, the candidates and the automaton step of
// the forward walk (dfa_walk_step<false>, dfa_advance) and the read of a draw (dfa_drawn), and phase B, which the profile shares
// (dfa_rows_init, dfa_backward).  The LDS carve-up, the row loop of phase A and `col` / `cc` are this file's.
#include "dfa_chain_dev.h"

namespace {
using DfaArgs = DfaChainArgs<DesignArgs>;      // tab: (B,T,live)

__global__ void __launch_bounds__(SC_THREADS) k_design_dfa(DfaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dfa_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live, W = a.words;
    double* zs = reinterpret_cast<double*>(dfa_lds);                               // [T][4]      z of a position
    double* row = zs + 4 * (size_t)T;                                              // [2][256]    l_{t+1} and l_t by state
    unsigned* draws = reinterpret_cast<unsigned*>(row + 2 * DFA_MAX_STATES);       // [256][W]    a chunk's draws
    unsigned* nx = draws + DFA_CHUNK * W;                                          // [256]       delta(a, .), a byte per class
    uint2* col = reinterpret_cast<uint2*>(nx + DFA_MAX_STATES);                    // [256]       the columns of delta(a, .), 16 bits per class
    unsigned short* own = reinterpret_cast<unsigned short*>(col + DFA_MAX_STATES); // [256]       the column of state a, or DFA_DEAD
    unsigned char* red = reinterpret_cast<unsigned char*>(own + DFA_MAX_STATES);   // the reduction's scratch
    const DsScratch sc = ds_scratch(red);
    unsigned char* kd = red + DFA_LDS_SCRATCH;                                     // [256]       bit 0 dead, bit 1 accepting
    unsigned char* ms = kd + DFA_MAX_STATES;                                       // [T]         the mask of a position
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    double* tab = a.tab + (size_t)b * T * AL;                                      // [T][AL]     l_t of a live state
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    // ---- A: rows, masks and the automaton (the row loop is ds_rows_to_lds' text: through the function this kernel measured 2.8 % slower
    // at 73 live states, docs/experiments.md Round 18)
    int bad = 0;
    for (int t = tid; t < n; t += SC_THREADS) {
        bool empty;
        const DsPos<double> p = ds_load<double>(a, pad0, row0, t, empty);
        bad += empty ? 1 : 0;
        zs[4 * t] = p.z[0]; zs[4 * t + 1] = p.z[1]; zs[4 * t + 2] = p.z[2]; zs[4 * t + 3] = p.z[3];
        ms[t] = (unsigned char)p.m;
    }
    const DfaState me = dfa_load_state(a, A, tid, DFA_DEAD, own, kd);
    const bool live = me.live, accepts = me.accepts;
    dfa_rows_init(row, n, tid, accepts);
    __syncthreads();
    unsigned cl[2] = {0, 0};
    int cc[4], ok = 0;
    dfa_load_delta(a, tid, DFA_DEAD, own, nx, [&](int c, unsigned nxt, unsigned k) {
        cl[c >> 1] |= k << (16 * (c & 1));
        ok |= (k != DFA_DEAD ? 1 : 0) << c;
        cc[c] = k != DFA_DEAD ? (int)nxt : 0;                                      // (the LDS rows are indexed by state)
    });
    col[tid] = make_uint2(cl[0], cl[1]);
    __syncthreads();
    // ---- B: l_t(a), t = n-1 .. 0; thread = state; the row of t + 1 is read, the row of t written, one barrier per step
    const bool miss = dfa_backward(zs, ms, row, tab, own, n, AL, tid, live, cc, ok);
    if (tid == 0 && a.dfa_miss) a.dfa_miss[b] = miss ? 1 : 0;
    // ---- C: the walks of 256 samples, then their rows
    const int S = (a.seqs || a.seq_nll || a.hits || a.accepted) ? a.S : 1;         // `infeasible` is written with sample 0
    for (int s0 = 0; s0 < S; s0 += DFA_CHUNK) {
        const int cn = min(DFA_CHUNK, S - s0);
        if (tid < cn) {
            const int s = s0 + tid;
            unsigned* mine = draws + tid * W;
            unsigned word = 0;
            int st = 0, hit = 0;
            for (int t = 0; t < n; ++t) {
                DsPos<double> p;
                const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
                p.z[0] = z01.x; p.z[1] = z01.y; p.z[2] = z23.x; p.z[3] = z23.y;
                p.m = ms[t];
                const unsigned u = ds_u24(seed, s, b, t);
                const unsigned step = nx[st];
                int q = -1;
                if (!miss) {
                    const bool last = t + 1 == n;
                    q = dfa_walk_step<false>(p, u, col[st], step, kd, tab + (size_t)(last ? t : t + 1) * AL, last, 1, 0, 0);
                }
                if (q < 0) q = ds_draw_single(p, u);                // no admitted sequence is accepted: rnampnn_design's draw
                dfa_advance(step, q, A, kd, st, hit);
                word |= (unsigned)q << (2 * (t & 15));
                if ((t & 15) == 15 || t == n - 1) { mine[t >> 4] = word; word = 0; }
            }
            if (a.hits) a.hits[(size_t)s * a.B + b] = hit;
            if (a.accepted) a.accepted[(size_t)s * a.B + b] = (kd[st] & 3) == 2 ? 1 : 0;
        }
        __syncthreads();
        for (int i = 0; i < cn; ++i) {
            const int s = s0 + i;
            const unsigned* drawn = draws + i * W;
            ds_write_rows(a, s, b, n, row0, tid, s == 0 ? bad : 0, sc, [&](int t) { return dfa_drawn(drawn, t); }, DsNoSum{});
            __syncthreads();                                        // the scratch is written again by the next sample
        }
    }
}

// the bytes of dynamic LDS, from T alone: the formula include/rnampnn_hip.h gives
size_t dfa_lds_bytes(long long T) {
    const size_t t = (size_t)T;
    return 32 * t + 16 * ((t + 15) / 16) + (size_t)DFA_CHUNK * 4 * (size_t)dfa_words((int)T) + 2 * 8 * DFA_MAX_STATES + (4 + 8 + 2 + 1) * DFA_MAX_STATES +
           DFA_LDS_SCRATCH;
}
}  // namespace

extern "C" size_t rnampnn_design_dfa_workspace_bytes(int32_t B, int32_t T, int32_t n_live) {
    if (B <= 0 || T <= 0 || n_live <= 0) return 0;
    return (size_t)8 * (size_t)B * (size_t)T * (size_t)n_live;
}

extern "C" int rnampnn_design_dfa(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                  float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                  const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                  const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace, size_t workspace_bytes,
                                  int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits, int32_t* accepted, int32_t* dfa_miss,
                                  void* stream) {
    const char* name = "rnampnn_design_dfa";
    DfaArgs a{};
    const int rc = dfa_prepare(name, logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                               bias_per_position, seqs, seq_nll, infeasible, delta, kind, n_states, workspace, workspace_bytes, hits, accepted,
                               dfa_miss, true, a, [] { return RNAMPNN_OK; }, [&](int live, char* what, size_t len) {
        std::snprintf(what, len, "the table of partition sums at (B = %d, T = %d, %d live states) needs", (int)B, (int)T, live);
        return rnampnn_design_dfa_workspace_bytes(B, T, live);
    });
    if (rc != RNAMPNN_OK) return rc;
    const size_t lds = dfa_lds_bytes(T);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d needs %zu bytes of LDS for the rows and the draws of 256 samples, the limit is %zu "
                    "(T <= %lld; the table of partition sums is in the workspace and does not count)", name, (int)T, lds, DS_LDS_MAX,
                    ds_max_T([](long long t) { return dfa_lds_bytes(t); }));
    if (!seqs && !seq_nll && !infeasible && !hits && !accepted && !dfa_miss) return RNAMPNN_OK;    // nothing asked for
    return ds_launch<k_design_dfa>(dim3(B), lds, stream, a);
}
