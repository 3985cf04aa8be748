// rnampnn_design_dfa_count: constrained design conditioned EXACTLY on BOTH a finite automaton (motifs that must and must not occur,
// rnampnn_design_dfa) and a count window (a G+C window or a mutation budget, rnampnn_design_count), in one launch.  The count joins the
// automaton's chain as a third index: l_t(a, k) = the log of the total weight of the suffixes from t that start in live state a, stay
// live, end in an accepting state and count exactly k.  Everything about a position, the automaton and its walk is design_dfa.hip's -
// the same functions of dfa_chain_dev.h: the arguments (DfaChainArgs over CtArgs), the prologue (dfa_prepare, with the count side's two
// checks), the walk's candidates (dfa_walk_step<true>: the count is its optional part), dfa_advance and dfa_drawn; phase A's automaton
// load is this file's own text, which fills `of` between the stores of `own` and `kd` (through the header's two functions the G+C
// variant measured 1.5 % slower, docs/experiments.md Round 17) - so with nothing counted the outputs are rnampnn_design_dfa's byte for byte; the counted sets, the window, the
// target and the selection of the total are count_tree_dev.h's (ct_target, ct_select, the salt).  The contract is the one
// include/rnampnn_hip.h documents and tests/_design_dfa_count_ref.py restates; all of the draw is fp64.
// The table l_t(a, k) lives in the caller's WORKSPACE in global memory, [b][t][live column][k], k = 0 .. cap: 8 B T L (cap + 1) bytes.
// One 256-thread workgroup per RNA.  (A) the fp64 rows, the masks, the counted sets and the automaton into LDS, as k_design_dfa.  (B) for
// t = n-1 .. 0 the slab of step t - the items (live column, k), L (K + 1) of them, K = min(cap, n) - is dealt flat over the threads; an
// item is one ds_lse<4> over four entries of the slab of t + 1; entries with k > n - t are -inf without arithmetic (a suffix of n - t
// positions counts no more).  The slab of t + 1 has TWO HOMES, the template parameter SLAB: true - two slabs in LDS, where 16 L (cap + 1)
// bytes fit beside the rest (a budget at every automaton, a G+C window at a small one); false - the workspace itself, written by this
// workgroup one barrier earlier.  Every entry is the same four-term LSE whichever home it is read from, so the homes cannot differ in a
// byte, and LDS bounds neither L x K nor T x L.  Every entry goes to the workspace either way.  (C) thread 0 reads the root l_0(0, .),
// forms window, target, misses and log_z; then 256 samples at a time, one lane each, draw their total and walk forward with (state,
// remaining count), reading the four candidates from the workspace; then per sample the rows and the NLL (ds_write_rows).
// No atomics, no fill / copy node, no host synchronisation; every table entry that is read was written by the same launch before.
#include "count_tree_dev.h"
#include "dfa_chain_dev.h"

#ifndef DFC_SLAB_LDS_MAX
#define DFC_SLAB_LDS_MAX DS_LDS_MAX            // the LDS a call may take with the two slabs in it; 0 builds the workspace home alone (the A/B of profiles/)
#endif

namespace {
static_assert(DS_SCRATCH <= 48, "the layout of the scratch: the reduction's bytes, then at 48 the six ints of the target");

struct DfcArgs : DfaChainArgs<CtArgs> {   // counted, lo, hi, count, miss (= count_miss), cap: the count side as CtArgs names it; tab: (B,T,live,cap+1)
    double* log_z;               // (B) or null
};

template <bool SLAB>
__global__ void __launch_bounds__(SC_THREADS) k_design_dfa_count(DfcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dfc_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live, W = a.words, cap1 = a.cap + 1;
    const size_t slab_doubles = SLAB ? (size_t)AL * cap1 : 0;
    double* zs = reinterpret_cast<double*>(dfc_lds);                               // [T][4]      z of a position
    double* slab = zs + 4 * (size_t)T;                                             // [2][AL][cap1]  l_{t+1} and l_t (SLAB only)
    unsigned* draws = reinterpret_cast<unsigned*>(slab + 2 * slab_doubles);        // [256][W]    a chunk's draws
    unsigned* nx = draws + DFA_CHUNK * W;                                          // [256]       delta(a, .), a byte per class
    uint2* col = reinterpret_cast<uint2*>(nx + DFA_MAX_STATES);                    // [256]       the columns of delta(a, .), 16 bits per class
    unsigned short* own = reinterpret_cast<unsigned short*>(col + DFA_MAX_STATES); // [256]       the column of state a, or DFA_DEAD
    unsigned char* of = reinterpret_cast<unsigned char*>(own + DFA_MAX_STATES);    // [256]       the state of a live column
    unsigned char* red = of + DFA_MAX_STATES;                                      // the reduction's scratch, then the target
    const DsScratch sc = ds_scratch(red);
    int* tg = reinterpret_cast<int*>(red + 48);                                    // lo, hi, K, any, dfa_miss
    unsigned char* kd = red + DFA_LDS_SCRATCH;                                     // [256]       bit 0 dead, bit 1 accepting
    unsigned char* ms = kd + DFA_MAX_STATES;                                       // [T]         the mask of a position
    unsigned char* cn = ms + (((size_t)T + 15) & ~(size_t)15);                     // [T]         its counted set
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const size_t step = (size_t)AL * cap1;                                         // the doubles of one slab
    double* tab = a.tab + (size_t)b * T * step;                                    // [T][AL][cap1]
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    const int K = min(a.cap, n);
    // ---- A: rows, masks, counted sets and the automaton
    int bad = 0;
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad, [&](int t, const DsPos<double>&) { cn[t] = (unsigned char)ct_counted<true>(a, pad0, t); });
    {
        const bool live = tid < A && !dfa_bit(a.dead, tid);
        const bool accepts = live && dfa_bit(a.acc, tid);
        const int mine = live ? dfa_column(a.dead, tid) : (int)DFA_DEAD;
        own[tid] = (unsigned short)mine;
        if (live) of[mine] = (unsigned char)tid;
        kd[tid] = (unsigned char)((live ? 0 : 1) | (accepts ? 2 : 0));
    }
    __syncthreads();
    {
        unsigned raw = 0, cl[2] = {0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned nxt = tid < A ? a.delta[4 * tid + c] : 0xFFu;
            const unsigned k = tid < A && nxt < (unsigned)A ? own[nxt] : DFA_DEAD;
            raw |= (nxt & 255u) << (8 * c);
            cl[c >> 1] |= k << (16 * (c & 1));
        }
        nx[tid] = tid < A ? raw : 0u;
        col[tid] = make_uint2(cl[0], cl[1]);
    }
    __syncthreads();
    // ---- B: l_t(a, k), t = n-1 .. 0; the items (live column, k) dealt flat; the slab of t + 1 is read, that of t written, one barrier per step
    const int items = AL * (K + 1);
    for (int t = n - 1; t >= 0; --t) {
        const bool last = t + 1 == n;
        const double* next = SLAB ? slab + ((t + 1) & 1) * slab_doubles : tab + (size_t)(last ? t : t + 1) * step;    // (the last step reads none of it)
        double* mine = slab + (t & 1) * slab_doubles;
        const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
        const double z[4] = {z01.x, z01.y, z23.x, z23.y};
        const int m = ms[t], cs = cn[t];
        for (int idx = tid; idx < items; idx += SC_THREADS) {
            const int j = idx / (K + 1), k = idx - j * (K + 1);
            double lt = -INFINITY;
            if (k <= n - t) {
                const unsigned st = of[j], nxt = nx[st];
                const uint2 cl = col[st];
                double v[4];
                int adm = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned kc = ((c < 2 ? cl.x : cl.y) >> (16 * (c & 1))) & 0xFFFFu;
                    const int kk = k - ((cs >> c) & 1);
                    const bool in = ((m >> c) & 1) && kc != DFA_DEAD && kk >= 0;
                    const double far = next[in ? (size_t)kc * cap1 + kk : 0];
                    const double end = (kd[(nxt >> (8 * c)) & 255u] & 2) && kk == 0 ? 0.0 : -INFINITY;
                    v[c] = z[c] + (last ? end : far);
                    adm |= (in ? 1 : 0) << c;
                }
                lt = ds_lse<4>(v, adm);
            }
            const size_t at = (size_t)j * cap1 + k;
            if (SLAB) mine[at] = lt;
            tab[(size_t)t * step + at] = lt;
        }
        __syncthreads();
    }
    // ---- C: window, target and log_z by thread 0; then the walks of 256 samples, then their rows
    if (tid == 0) {
        const double* root = tab;                                   // l_0(0, .): state 0 is live, so its column is 0
        CtTarget g;
        bool none;
        double lz;
        if (n > 0) {
            g = ct_target<false>(a, root, nullptr, b, n, n > 1 ? 32 - __clz(n - 1) : 0);
            none = !g.any && !ct_finite(root[g.K]);                 // no count of 0 .. K is reachable: ct_target left K = lo, miss = 0
            lz = none ? -INFINITY : g.any ? ct_lse_terms(g.lo, g.hi, [&](int k) { return root[k]; }) : root[g.K];
        } else {                                                    // the RNA of length 0: feasible iff state 0 accepts
            g.lo = g.hi = g.deg = g.K = g.miss = 0; g.at_min = false;
            g.any = (kd[0] & 2) != 0;
            none = !g.any;
            lz = none ? -INFINITY : 0.0;
        }
        tg[0] = g.lo; tg[1] = g.hi; tg[2] = min(g.K, K); tg[3] = g.any ? 1 : 0; tg[4] = none ? 1 : 0;
        if (a.dfa_miss) a.dfa_miss[b] = none ? 1 : 0;
        if (a.miss) a.miss[b] = none ? 0 : g.miss;
        if (a.log_z) a.log_z[b] = lz;
    }
    __syncthreads();
    const int lo = tg[0], hi = tg[1], target = tg[2];
    const bool any = tg[3] != 0, miss = tg[4] != 0;
    const int S = (a.seqs || a.seq_nll || a.hits || a.accepted || a.count) ? a.S : 1;      // `infeasible` is written with sample 0
    for (int s0 = 0; s0 < S; s0 += DFA_CHUNK) {
        const int cnum = min(DFA_CHUNK, S - s0);
        if (tid < cnum) {
            const int s = s0 + tid;
            unsigned* mine = draws + tid * W;
            unsigned word = 0;
            int st = 0, hit = 0, cnt = 0, r = target;
            if (any && n > 0) r = min(max(ct_select(lo, hi, ds_u24(seed ^ CT_SALT, s, b, 0), [&](int k) { return tab[k]; }), 0), K);
            for (int t = 0; t < n; ++t) {
                DsPos<double> p;
                const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
                p.z[0] = z01.x; p.z[1] = z01.y; p.z[2] = z23.x; p.z[3] = z23.y;
                p.m = ms[t];
                const int cs = cn[t];
                const unsigned u = ds_u24(seed, s, b, t);
                const unsigned nxts = nx[st];
                int q = -1;
                if (!miss) {
                    const bool last = t + 1 == n;
                    q = dfa_walk_step<true>(p, u, col[st], nxts, kd, tab + (size_t)(last ? t : t + 1) * step, last, cap1, r, cs);
                }
                if (q < 0) q = ds_draw_single(p, u);                // no admitted sequence holds both conditions: rnampnn_design's draw
                dfa_advance(nxts, q, A, kd, st, hit);
                cnt += (cs >> q) & 1;
                r = max(r - ((cs >> q) & 1), 0);
                word |= (unsigned)q << (2 * (t & 15));
                if ((t & 15) == 15 || t == n - 1) { mine[t >> 4] = word; word = 0; }
            }
            if (a.hits) a.hits[(size_t)s * a.B + b] = hit;
            if (a.accepted) a.accepted[(size_t)s * a.B + b] = (kd[st] & 3) == 2 ? 1 : 0;
            if (a.count) a.count[(size_t)s * a.B + b] = cnt;
        }
        __syncthreads();
        for (int i = 0; i < cnum; ++i) {
            const int s = s0 + i;
            const unsigned* drawn = draws + i * W;
            ds_write_rows(a, s, b, n, row0, tid, s == 0 ? bad : 0, sc, [&](int t) { return dfa_drawn(drawn, t); }, DsNoSum{});
            __syncthreads();                                        // the scratch is written again by the next sample
        }
    }
}

// the bytes of dynamic LDS without the slabs, from T alone, and the bytes of the two slabs: the formulas include/rnampnn_hip.h gives
size_t dfc_lds_bytes(long long T) {
    const size_t t = (size_t)T;
    return 32 * t + 2 * 16 * ((t + 15) / 16) + (size_t)DFA_CHUNK * 4 * (size_t)dfa_words((int)T) + (4 + 8 + 2 + 1 + 1) * DFA_MAX_STATES + DFA_LDS_SCRATCH;
}
size_t dfc_slab_bytes(int live, int cap) { return (size_t)16 * (size_t)live * ((size_t)cap + 1); }
// the table: 8 B T L (cap + 1) bytes, cap already clamped to 0 .. T
size_t dfc_table_bytes(int B, int T, int live, int cap) { return (size_t)8 * (size_t)B * (size_t)T * (size_t)live * ((size_t)cap + 1); }
}  // namespace

extern "C" size_t rnampnn_design_dfa_count_workspace_bytes(int32_t B, int32_t T, int32_t n_live, int32_t count_cap) {
    if (B <= 0 || T <= 0 || n_live <= 0 || count_cap <= 0) return 0;
    return dfc_table_bytes(B, T, n_live, std::min<int>(count_cap, T));
}

extern "C" int rnampnn_design_dfa_count(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                        float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                        const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                        const uint8_t* delta, const uint8_t* kind, int32_t n_states, const uint8_t* counted,
                                        const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap, void* workspace,
                                        size_t workspace_bytes, int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits,
                                        int32_t* accepted, int32_t* count, int32_t* dfa_miss, int32_t* count_miss, double* log_z, void* stream) {
    const char* name = "rnampnn_design_dfa_count";
    DfcArgs a{};
    const int rc = dfa_prepare(name, logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                               bias_per_position, seqs, seq_nll, infeasible, delta, kind, n_states, workspace, workspace_bytes, hits, accepted,
                               dfa_miss, true, a, [&] { return ct_count_side(name, counted, count_lo, count_hi, count_cap, T, 0, a); }, [&](int live, char* what, size_t len) {
        const int cap = std::min<int>(count_cap, T);
        std::snprintf(what, len, "the table of partition sums at (B = %d, T = %d, %d live states, counts 0 .. %d) needs", (int)B, (int)T, live, cap);
        return dfc_table_bytes(B, T, live, cap);
    });
    if (rc != RNAMPNN_OK) return rc;
    size_t lds = dfc_lds_bytes(T);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d needs %zu bytes of LDS for the rows and the draws of 256 samples, the limit is %zu "
                    "(T <= %lld; the table of partition sums is in the workspace and does not count)", name, (int)T, lds, DS_LDS_MAX,
                    ds_max_T([](long long t) { return dfc_lds_bytes(t); }));
    if (!seqs && !seq_nll && !infeasible && !hits && !accepted && !count && !dfa_miss && !count_miss && !log_z) return RNAMPNN_OK;    // nothing asked for
    a.log_z = log_z;
    a.count = count; a.miss = count_miss;
    const size_t slabs = dfc_slab_bytes(a.live, a.cap);
    if (lds + slabs <= (size_t)DFC_SLAB_LDS_MAX) return ds_launch<k_design_dfa_count<true>>(dim3(B), lds + slabs, stream, a);
    return ds_launch<k_design_dfa_count<false>>(dim3(B), lds, stream, a);
}
