// rnampnn_design_nested: constrained design under BASE PAIRS and an automaton at once - the draws of rnampnn_design on a nested (pseudoknot
// free) structure, conditioned EXACTLY on the sequence being accepted by the automaton of rnampnn_design_dfa, in one launch.  A pair
// couples two distant positions, so the chain over (position x state) of k_design_dfa does not carry it; but a nested structure is a TREE,
// and on a tree the automaton travels as a TRANSFER TABLE per enclosed interval: R_t(a, g) = the log weight of everything from t to the end
// of t's loop that starts in live state a and ends in goal g (a live state inside a pair, "accepted" at the top level).  A stem's interior
// is an L x L table, a loop a (log-domain) product of such tables, and the draw walks the tree top down.  L^2 per position, no dependence
// on the depth.  The contract is the one include/rnampnn_hip.h documents and tests/_design_nested_ref.py restates; all of it is fp64, and
// on an RNA without a valid pair every output is rnampnn_design_dfa's byte for byte: the statements that form z, the logsumexp, the
// weights and the selection are design_dev.h's and stand in the same order.
// One 256-thread workgroup per RNA.  (A) every thread: the fp64 rows and the masks of the RNA into LDS, the automaton by live COLUMN
// (L <= 64), the validated partner of every position (a pair without an admitted compatible cell is dropped and counts 2), whether two
// pairs cross (nest_miss), and which positions lie at the top level.  (B) t = n-1 .. 0, the L x G entries of R_t dealt over the threads
// (G = L inside a pair, 1 at the top level): an unpaired position reads the table of its successor from the workspace; an opener stages
// R^in in an LDS tile, forms P_t in a second tile, stages the successor's table and forms the product.  Every table is written and later
// read by this workgroup alone, so workgroup barriers order the accesses.  (C) 256 samples at a time, one lane per sample, 2 bits per
// position in LDS words the lane owns (they lie over the tiles, which phase B is done with); the goals of the open pairs are a stack of
// bytes per lane in the workspace; then per sample the rows and the NLL as k_design writes them (ds_write_rows).
// No atomics, no fill / copy node, no host synchronisation; every workspace byte that is read was written by the same launch before.
// dfa_chain_dev.h holds what this entry shares with rnampnn_design_dfa and rnampnn_design_dfa_count: the automaton's constants, helpers
// and arguments (DfaChainArgs), the host prologue (dfa_prepare; pairs are not refused here), the automaton half of phase A (columns as
// bytes, DFA_DEAD8), dfa_advance on a miss and dfa_drawn.  NS_MAX_LIVE, `dl` / `ac`, the structure, phase B and the
// walk of the tree are this file's.
#include "dfa_chain_dev.h"

namespace {
constexpr int NS_MAX_LIVE = RNAMPNN_DESIGN_NESTED_MAX_LIVE;
static_assert(NS_MAX_LIVE <= 254, "a live column and the dead mark fit a byte");

struct NestStacks { unsigned char* stack; };   // (B,T/2+1,256): the goals of a lane's open pairs, behind the tables
struct NestArgs : DfaChainArgs<DesignArgs, NestStacks> {   // tab: (B,T,live,live), the tables
    int32_t* nest;               // (B) or null
};

// A table as the recurrence reads it: one in the workspace (rows of G goals), the identity behind the last element of an inner loop, or
// the acceptance vector behind position n-1.
enum { NS_TABLE = 0, NS_IDENTITY = 1, NS_FINAL = 2 };
struct NsTab { const double* p; int kind, G; };
__device__ __forceinline__ double ns_at(const NsTab& t, const unsigned char* ac, int row, int goal) {
    if (t.kind == NS_TABLE) return t.p[row * t.G + goal];
    const bool zero = t.kind == NS_IDENTITY ? row == goal : ac[row] != 0;
    return zero ? 0.0 : -INFINITY;
}

__global__ void __launch_bounds__(SC_THREADS) k_design_nested(NestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ns_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live, W = a.words;
    const size_t area = max((size_t)16 * AL * AL, (size_t)DFA_CHUNK * 4 * W);
    double* zs = reinterpret_cast<double*>(ns_lds);                                // [T][4]      z of a position
    double* tile_a = zs + 4 * (size_t)T;                                           // [L][L]      R^in, then the successor's table (phase B)
    double* tile_b = tile_a + AL * AL;                                             // [L][L]      P_t (phase B)
    unsigned* draws = reinterpret_cast<unsigned*>(tile_a);                         // [256][W]    a chunk's draws (phase C, over the tiles)
    unsigned* nx = reinterpret_cast<unsigned*>(ns_lds + 32 * (size_t)T + area);    // [256]       delta(a, .), a byte per class
    unsigned* dl = nx + DFA_MAX_STATES;                                            // [64]        the columns of delta(column k, .), a byte per class
    unsigned char* red = reinterpret_cast<unsigned char*>(dl + NS_MAX_LIVE);       // the reduction's scratch
    const DsScratch sc = ds_scratch(red);
    short* pr = reinterpret_cast<short*>(red + DFA_LDS_SCRATCH);                   // [T]         the partner of a position, -1 for none
    unsigned char* own = reinterpret_cast<unsigned char*>(pr + T);                 // [256]       the column of state a, or DFA_DEAD8
    unsigned char* kd = own + DFA_MAX_STATES;                                      // [256]       bit 0 dead, bit 1 accepting
    unsigned char* ac = kd + DFA_MAX_STATES;                                       // [64]        column k accepts
    unsigned char* ms = ac + NS_MAX_LIVE;                                          // [T]         the mask of a position
    unsigned char* fl = ms + T;                                                    // [T]         1 = the position lies inside no pair
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    double* tab = a.tab + (size_t)b * T * AL * AL;                                 // [T][L][G]   R_t
    unsigned char* stack = a.more.stack + (size_t)b * (T / 2 + 1) * DFA_CHUNK + tid;    // [T/2+1][256]
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    // ---- A: rows, masks, the automaton and the structure
    int bad = 0;
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad);
    const DfaState me = dfa_load_state(a, A, tid, DFA_DEAD8, own, kd);
    const bool live = me.live;
    const unsigned mine_col = me.mine;
    if (live) ac[mine_col] = me.accepts ? 1 : 0;
    __syncthreads();
    {
        unsigned cols = 0;
        dfa_load_delta(a, tid, DFA_DEAD8, own, nx, [&](int c, unsigned, unsigned k) { cols |= k << (8 * c); });
        if (live) dl[mine_col] = cols;
    }
    for (int t = tid; t < n; t += SC_THREADS) {
        int j = ds_partner(a, pad0, n, t);
        if (j >= 0 && !ds_pair_mask(ms[min(t, j)], ms[max(t, j)], a.wobble)) { bad += 1; j = -1; }   // each end counts itself: 2 per pair
        pr[t] = (short)j;
    }
    __syncthreads();
    int cross = 0;
    for (int t = tid; t < n; t += SC_THREADS) {
        const int j = pr[t];
        for (int k = t + 1; k < j; ++k) {
            const int pk = pr[k];
            cross |= (pk >= 0 && (pk < t || pk > j)) ? 1 : 0;
        }
    }
    const bool nest = __syncthreads_or(cross) != 0;
    if (tid == 0 && !nest) {
        int depth = 0;
        for (int t = 0; t < n; ++t) {
            const int j = pr[t];
            depth -= (j >= 0 && j < t) ? 1 : 0;
            fl[t] = depth == 0 ? 1 : 0;
            depth += j > t ? 1 : 0;
        }
    }
    __syncthreads();
    // the table of the element that starts at x in the loop that `top` describes: behind position n-1, behind a loop's last element, or R_x
    auto table_at = [&](int x, bool top) {
        NsTab r;
        r.G = top ? 1 : AL;
        r.p = tab + (size_t)x * AL * AL;
        const int px = x < n ? (int)pr[x] : -1;
        r.kind = x >= n ? NS_FINAL : (px >= 0 && px < x) ? NS_IDENTITY : NS_TABLE;
        return r;
    };
    // ---- B: R_t, t = n-1 .. 0; the L x G entries of a step dealt over the threads; a barrier after every step
    if (!nest) {
        for (int t = n - 1; t >= 0; --t) {
            const int j = pr[t];
            if (j >= 0 && j < t) continue;                          // a closer holds no table
            const bool top = fl[t] != 0;
            const int G = top ? 1 : AL, m = ms[t];
            double* out = tab + (size_t)t * AL * AL;
            const double z[4] = {zs[4 * t], zs[4 * t + 1], zs[4 * t + 2], zs[4 * t + 3]};
            if (j < 0) {
                const NsTab N = table_at(t + 1, top);
                for (int e = tid; e < AL * G; e += SC_THREADS) {
                    const int r = e / G, g = e - r * G;
                    const unsigned d = dl[r];
                    double v[4];
                    int ok = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const unsigned k = (d >> (8 * c)) & 255u;
                        v[c] = z[c] + ns_at(N, ac, k != DFA_DEAD8 ? (int)k : 0, g);
                        ok |= (k != DFA_DEAD8 ? 1 : 0) << c;
                    }
                    out[e] = ds_lse<4>(v, m & ok);
                }
                __syncthreads();
                continue;
            }
            const int pm = ds_pair_mask(m, ms[j], a.wobble);
            NsTab In = table_at(t + 1, false);                      // (j == t + 1: position t + 1 is this pair's closer, the identity)
            for (int e = tid; e < AL * AL; e += SC_THREADS) {
                const int r = e / AL;
                tile_a[e] = ns_at(In, ac, r, e - r * AL);
            }
            __syncthreads();
            // P_t(a, b): the pair's cells in a-major order, within a cell the states b' before the closer, ascending, that the closer sends to b
            for (int e = tid; e < AL * AL; e += SC_THREADS) {
                const int r = e / AL, goal = e - r * AL;
                const unsigned d = dl[r];
                double mx = -INFINITY, sum = 0.0;
                for (int pass = 0; pass < 2; ++pass) {
                    for (int cell = 0; cell < 16; ++cell) {
                        const unsigned k = (d >> (8 * (cell >> 2))) & 255u;
                        if (!((pm >> cell) & 1) || k == DFA_DEAD8) continue;
                        const double zc = zs[4 * t + (cell >> 2)] + zs[4 * j + (cell & 3)];
                        const double* rin = tile_a + k * AL;
                        for (int b2 = 0; b2 < AL; ++b2) {
                            if (((dl[b2] >> (8 * (cell & 3))) & 255u) != (unsigned)goal || !(rin[b2] > -INFINITY)) continue;
                            const double v = zc + rin[b2];
                            if (pass == 0) mx = fmax(mx, v);
                            else sum += exp(v - mx);
                        }
                    }
                    if (!(mx > -INFINITY)) break;
                }
                tile_b[e] = mx > -INFINITY ? mx + log(sum) : -INFINITY;
            }
            __syncthreads();
            const NsTab N = table_at(j + 1, top);
            for (int e = tid; e < AL * G; e += SC_THREADS) {
                const int r = e / G;
                tile_a[e] = ns_at(N, ac, r, e - r * G);
            }
            __syncthreads();
            for (int e = tid; e < AL * G; e += SC_THREADS) {
                const int r = e / G, g = e - r * G;
                const double* prow = tile_b + r * AL;
                double mx = -INFINITY, sum = 0.0;
                for (int k = 0; k < AL; ++k)
                    if (prow[k] > -INFINITY && tile_a[k * G + g] > -INFINITY) mx = fmax(mx, prow[k] + tile_a[k * G + g]);
                if (mx > -INFINITY)
                    for (int k = 0; k < AL; ++k)
                        if (prow[k] > -INFINITY && tile_a[k * G + g] > -INFINITY) sum += exp(prow[k] + tile_a[k * G + g] - mx);
                out[e] = mx > -INFINITY ? mx + log(sum) : -INFINITY;
            }
            __syncthreads();
        }
    }
    __syncthreads();                                                // the tiles are done with: the draws lie over them
    const bool dmiss = !nest && !((n > 0 ? tab[0] : (ac[0] ? 0.0 : -INFINITY)) > -INFINITY);       // R_0(0, accepted)
    const bool miss = nest || dmiss;
    if (tid == 0 && a.dfa_miss) a.dfa_miss[b] = dmiss ? 1 : 0;
    if (tid == 0 && a.nest) a.nest[b] = nest ? 1 : 0;
    // ---- C: the walks of 256 samples, then their rows
    const int S = (a.seqs || a.seq_nll || a.hits || a.accepted) ? a.S : 1;         // `infeasible` is written with sample 0
    for (int s0 = 0; s0 < S; s0 += DFA_CHUNK) {
        const int cn = min(DFA_CHUNK, S - s0);
        if (tid < cn) {
            const int s = s0 + tid;
            unsigned* mine = draws + tid * W;
            for (int w = 0; w < W; ++w) mine[w] = 0u;
            int st = 0, hit = 0, col = 0, g = 0, sp = 0;            // the state by number (a miss) and by column, the goal, the open pairs
            for (int t = 0; t < n; ++t) {
                const int j = pr[t];
                const bool closer = j >= 0 && j < t;
                DsPos<double> p;
                p.z[0] = zs[4 * t]; p.z[1] = zs[4 * t + 1]; p.z[2] = zs[4 * t + 2]; p.z[3] = zs[4 * t + 3];
                p.m = ms[t];
                const unsigned u = ds_u24(seed, s, b, closer ? j : t);
                int q = -1;
                if (miss) {                                         // rnampnn_design's draw in fp64; the automaton only counts
                    if (j >= 0) {
                        DsPos<double> o;
                        o.z[0] = zs[4 * j]; o.z[1] = zs[4 * j + 1]; o.z[2] = zs[4 * j + 2]; o.z[3] = zs[4 * j + 3];
                        o.m = ms[j];
                        const int cell = closer ? ds_draw_pair(o, p, a.wobble, u) : ds_draw_pair(p, o, a.wobble, u);
                        if (cell >= 0) q = closer ? (cell & 3) : (cell >> 2);
                    }
                    if (q < 0) q = ds_draw_single(p, ds_u24(seed, s, b, t));
                    dfa_advance(nx[st], q, A, kd, st, hit);
                    mine[t >> 4] |= (unsigned)q << (2 * (t & 15));
                    continue;
                }
                if (closer) {                                       // its class came with the opener's
                    q = dfa_drawn(mine, t);
                    const unsigned k = (dl[col] >> (8 * q)) & 255u;
                    col = k != DFA_DEAD8 ? (int)k : 0;
                    sp -= sp > 0 ? 1 : 0;
                    g = stack[(size_t)sp * DFA_CHUNK];
                    continue;
                }
                const bool top = fl[t] != 0;
                const unsigned d = dl[col];
                if (j < 0) {
                    const NsTab N = table_at(t + 1, top);
                    double v[4];
                    int adm = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const unsigned k = (d >> (8 * c)) & 255u;
                        const bool in = ((p.m >> c) & 1) && k != DFA_DEAD8;
                        const double l = in ? ns_at(N, ac, (int)k, g) : -INFINITY;
                        v[c] = p.z[c] + l;
                        adm |= (in && l > -INFINITY ? 1 : 0) << c;
                    }
                    if (adm) {
                        double w[4];
                        ds_weights(v, adm, w);
                        q = ds_select(w, adm, u);
                    }
                    if (q < 0) q = ds_draw_single(p, u);
                    const unsigned k = (d >> (8 * q)) & 255u;
                    col = k != DFA_DEAD8 ? (int)k : 0;
                    mine[t >> 4] |= (unsigned)q << (2 * (t & 15));
                    continue;
                }
                // an opener: one selection over (c, c', b') in the order of P_t, weighted on to the goal through the successor's table
                const int pm = ds_pair_mask(p.m, ms[j], a.wobble);
                const NsTab In = table_at(t + 1, false), N = table_at(j + 1, top);
                double mx = -INFINITY, tot = 0.0, run = 0.0, lim = 0.0;
                int sel = -1;
                bool found = false;
                for (int pass = 0; pass < 3; ++pass) {
                    for (int cell = 0; cell < 16; ++cell) {
                        const unsigned k = (d >> (8 * (cell >> 2))) & 255u;
                        if (!((pm >> cell) & 1) || k == DFA_DEAD8) continue;
                        const double zc = zs[4 * t + (cell >> 2)] + zs[4 * j + (cell & 3)];
                        for (int b2 = 0; b2 < AL; ++b2) {
                            const unsigned k2 = (dl[b2] >> (8 * (cell & 3))) & 255u;
                            if (k2 == DFA_DEAD8) continue;
                            const double rin = ns_at(In, ac, (int)k, b2);
                            if (!(rin > -INFINITY)) continue;
                            const double far = ns_at(N, ac, (int)k2, g);
                            if (!(far > -INFINITY)) continue;
                            const double v = zc + rin + far;
                            if (pass == 0) mx = fmax(mx, v);
                            else if (pass == 1) tot += exp(v - mx);
                            else {
                                run += exp(v - mx);
                                if (!found) { sel = cell * NS_MAX_LIVE + b2; found = run > lim; }   // (it ends on the last admitted one)
                            }
                        }
                    }
                    lim = (double)u * (1.0 / 16777216.0) * tot;
                }
                int cell = sel >= 0 ? sel / NS_MAX_LIVE : -1, b2 = sel >= 0 ? sel % NS_MAX_LIVE : 0;
                if (cell < 0) {                                     // (no admitted cell reaches the goal: not on a feasible RNA)
                    DsPos<double> o;
                    o.z[0] = zs[4 * j]; o.z[1] = zs[4 * j + 1]; o.z[2] = zs[4 * j + 2]; o.z[3] = zs[4 * j + 3];
                    o.m = ms[j];
                    cell = max(ds_draw_pair(p, o, a.wobble, u), 0);
                }
                stack[(size_t)sp * DFA_CHUNK] = (unsigned char)g;
                ++sp;
                g = b2;
                const unsigned k = (d >> (8 * (cell >> 2))) & 255u;
                col = k != DFA_DEAD8 ? (int)k : 0;
                mine[t >> 4] |= (unsigned)(cell >> 2) << (2 * (t & 15));
                mine[j >> 4] |= (unsigned)(cell & 3) << (2 * (j & 15));
            }
            if (a.hits) a.hits[(size_t)s * a.B + b] = hit;
            if (a.accepted) a.accepted[(size_t)s * a.B + b] = miss ? ((kd[st] & 3) == 2 ? 1 : 0) : (ac[col] ? 1 : 0);
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

// the bytes of dynamic LDS, from T and the live states: the formula include/rnampnn_hip.h gives
size_t ns_lds_bytes(long long T, int live) {
    const size_t t = (size_t)T, tiles = (size_t)16 * live * live, draws = (size_t)DFA_CHUNK * 4 * (size_t)dfa_words((int)T);
    return 32 * t + (tiles > draws ? tiles : draws) + 4 * DFA_MAX_STATES + 4 * NS_MAX_LIVE + DFA_LDS_SCRATCH + 2 * t + 2 * DFA_MAX_STATES + NS_MAX_LIVE +
           2 * t;
}

size_t ns_table_bytes(int32_t B, int32_t T, int32_t live) { return (size_t)8 * (size_t)B * (size_t)T * (size_t)live * (size_t)live; }
}  // namespace

extern "C" size_t rnampnn_design_nested_workspace_bytes(int32_t B, int32_t T, int32_t n_live) {
    if (B <= 0 || T <= 0 || n_live <= 0) return 0;
    return ns_table_bytes(B, T, n_live) + (size_t)DFA_CHUNK * (size_t)B * (size_t)(T / 2 + 1);
}

extern "C" int rnampnn_design_nested(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                     float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                     const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                     const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace, size_t workspace_bytes,
                                     int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits, int32_t* accepted, int32_t* dfa_miss,
                                     int32_t* nest_miss, void* stream) {
    const char* name = "rnampnn_design_nested";
    NestArgs a{};
    const int rc = dfa_prepare(name, logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                               bias_per_position, seqs, seq_nll, infeasible, delta, kind, n_states, workspace, workspace_bytes, hits, accepted,
                               dfa_miss, false, a, [] { return RNAMPNN_OK; }, [&](int live, char* what, size_t len) {
        std::snprintf(what, len, "the tables and the goal stacks at (B = %d, T = %d, %d live states) need", (int)B, (int)T, live);
        return rnampnn_design_nested_workspace_bytes(B, T, live);
    });
    if (rc != RNAMPNN_OK) return rc;
    const int live = a.live;
    if (live > NS_MAX_LIVE)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: the automaton has %d live states, the limit is %d (a table per position holds live x live "
                    "entries, and two of them sit in LDS): require or avoid fewer or shorter motifs", name, live, NS_MAX_LIVE);
    const size_t lds = ns_lds_bytes(T, live);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d needs %zu bytes of LDS for the rows, the structure and the draws of 256 samples, the "
                    "limit is %zu (T <= %lld at %d live states; the tables are in the workspace and do not count)", name, (int)T, lds, DS_LDS_MAX,
                    ds_max_T([&](long long t) { return ns_lds_bytes(t, live); }), live);
    if (!seqs && !seq_nll && !infeasible && !hits && !accepted && !dfa_miss && !nest_miss) return RNAMPNN_OK;    // nothing asked for
    a.more.stack = reinterpret_cast<unsigned char*>(workspace) + ns_table_bytes(B, T, live);
    a.nest = nest_miss;
    return ds_launch<k_design_nested>(dim3(B), lds, stream, a);
}
