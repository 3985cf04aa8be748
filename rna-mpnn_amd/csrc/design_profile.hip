// rnampnn_design_count_profile / rnampnn_design_avoid_profile: INFERENCE next to the draws of rnampnn_design_count and
// rnampnn_design_avoid.  Each returns, in one launch and in fp64, the exact distribution its draw entry samples from - per-position marginals
// P(x_t = c), the log partition sum over the set drawn from (log_z), the free log partition sum (log_z_free) and the entropy - together with
// the draw entry's own `infeasible` and `*_miss`.  The contract is the one include/rnampnn_hip.h documents and tests/_design_profile_ref.py
// restates.  One 256-thread workgroup per RNA, no sample axis, no workspace, no atomics, no runtime fill / copy node, no host synchronisation.
//
// k_design_count_profile.  The leaves, the tree, the convolution, the window, the target and the k_min rule are count_tree_dev.h's (ct_leaf,
// ct_inside, ct_lse_terms, ct_target, ct_deg / ct_stride / ct_nodes, ct_min_d); phase B (pf_ct_root), a coefficient of phase C (pf_outside),
// phase D (pf_ct_leaves) and the final writer are profile_dev.h's, which the same profile on trees in global memory (design_long.hip) shares.  (A) ct_inside: the inside tree bottom-up into LDS, k_min and
// the free sum on the way.  (B) wave 0: ct_target - the window, the target and count_miss of the draw; K* and log_z; the root's outside
// O(k) = 0 on K*, -inf elsewhere.
// (C) the OUTSIDE pass top-down into a second tree of the same layout: O_L(a) = LSE_k O(k) + R(k - a), O_R(b) = LSE_k O(k) + L(k - b), dealt
// flat over (child node, coefficient); a node whose right half is empty hands O to its left half.  (D) one level-1 node per thread: the two
// leaves again from the rows, their outsides from the node's, then P = exp(z + O(d) - log_z) per admitted class / cell; the owner of a pair
// writes both ends.  Under the k_min rule (C) is skipped and every leaf is normalised over the cells of its own smallest d.  (E) padding
// rows as zeros, three fixed-order fp64 workgroup sums (free, sum of P z, the k_min log_z), thread 0 writes the scalars.
//   LDS bytes(T, cap) = 16 * doubles(T, cap) + 240: the inside and the outside tree (the outside of a child needs its parent's outside
//   and its SIBLING's inside at once, so neither can be overwritten), doubles(T, cap) as in rnampnn_design_count, and 240 bytes of scratch.
//   160 KiB holds T <= 1457 at cap 8 (163,792 bytes) and T <= 535 at cap >= T (the draw kernel: 2867 and 1017).
//
// k_design_avoid_profile.  The rows, the automaton's tables and the backward table l_t(a) are k_design_avoid's, statement for statement
// (avoid_chain_dev.h says why the two texts stay; the constants, the arguments and the entry's checks are that header's).
// Then wave 0, lane = state, walks FORWARD once: alpha_t(a) lives in the lane's register; per step the lane turns its four cells into
// exp(alpha + z + l_{t+1}(delta) - log_z), a wave butterfly sums them into P_t(c) (lane 0 writes the row and adds P z), and alpha_{t+1}(a') is
// gathered by lane a' over its predecessor cells - a list per state built once (counting sort over the 4 A cells, cell order, four cells to a word) - from the
// candidates alpha + z the lanes parked in LDS: the target takes their maximum, the sources exponentiate their own four candidates
// against it, the target adds - eight exps per lane and step whatever the fan-in of a state.  With avoid_miss = 1 there is no chain: all threads write the per-position softmax (pf_softmax_rows).
//   LDS bytes(T, L) = (32 + 8 L) T + 16 ceil(T / 16) + 3,680: the fp64 rows, the table of L live states, the masks; 2,560 for the
//   candidates and the maxima, 512 for the automaton, 448 for the predecessor lists, 160 for the sums and the reduction's scratch.
//   160 KiB holds T <= 1168 at L = 13 (no run longer than 3) and T <= 293 at L = 64 (the draw kernel: 1064 and 290).
// Non-finite rows can make the outputs of THAT RNA NaN; no index depends on a value, so nothing faults and no other RNA changes.
#include "avoid_chain_dev.h"
#include "profile_dev.h"

namespace {
__global__ void __launch_bounds__(SC_THREADS) k_design_count_profile(PfCtArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfc_lds[];
    double* tree = reinterpret_cast<double*>(pfc_lds);
    double* outs = reinterpret_cast<double*>(pfc_lds + a.lds_tree);                          // the outside tree, the inside tree's layout
    const PfCtScratch ps = pf_ct_scratch(pfc_lds + 2 * (size_t)a.lds_tree);
    const DsScratch sc = ps.sc;
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T, cap = a.cap;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    int bad = 0;
    // ---- A: the inside tree
    double free_sum = ct_inside<true, true>(a, tree, ps.s_leaf, sc.s_i, pad0, row0, n, tid, bad);
    // ---- B: the window, the target, K*, log_z and the root's outside
    if (tid < 64 && n > 0) pf_ct_root(a, Ln ? tree + a.base[Ln] : ps.s_leaf, Ln ? outs + a.base[Ln] : ps.o_leaf, sc.s_i, b, n, Ln, tid, ps.s_flag, ps.s_logz);
    __syncthreads();
    const bool at_min = n > 0 && ps.s_flag[0] != 0;                // the same in every thread
    const int miss = n > 0 ? ps.s_flag[1] : 0;
    const double log_z = n > 0 ? *ps.s_logz : 0.0;
    // ---- C: the outside pass, top down: level l hands its children at level l - 1 their outsides
    for (int l = Ln; l >= 2 && !at_min; --l) {
        const int stride = ct_stride(l, T, cap), cstride = ct_stride(l - 1, T, cap), cnodes = ct_nodes(l - 1, n);
        for (int idx = tid; idx < cnodes * cstride; idx += SC_THREADS) {
            const int j = idx / cstride, c = idx - j * cstride;
            if (c > ct_deg(l - 1, j, n, cap)) continue;
            outs[a.base[l - 1] + idx] = pf_outside(outs + a.base[l], tree + a.base[l - 1], l, j, c, n, cap, stride, cstride, cnodes);
        }
        __syncthreads();
    }
    // ---- D: the leaves of a level-1 node, their outsides and their marginals
    double pz_sum = 0.0, lz_sum = 0.0;
    pf_ct_leaves(a, outs + a.base[1], ps.o_leaf, pad0, row0, n, tid, at_min, log_z, pz_sum, lz_sum);
    // ---- E: padding, sums, scalars
    pf_finish(a.out, a, a.miss, miss, b, n, tid, bad, free_sum, pz_sum, lz_sum, at_min, log_z, sc, ps.s_d);
}

inline size_t pf_ct_lds_bytes(int T, int cap, size_t& tree) {
    tree = ct_tree_doubles(T, cap, nullptr) * sizeof(double);
    return 2 * tree + PF_CT_SCRATCH;
}
// the largest T whose two trees fit at that cap (a cap above T is T: the byte count grows with T)
inline int pf_ct_max_T(int cap) {
    size_t tree;
    return (int)ds_max_T([&](long long T) { return pf_ct_lds_bytes((int)T, std::min(cap, (int)T), tree); });
}

// ---------------------------------------------------------------------------------------------------------------- the avoid profile
constexpr int PF_PRED_WORDS = (4 * AV_MAX_STATES + 3 * AV_MAX_STATES) / 4;         // 256 cells, each of 64 lists padded to a word
constexpr size_t PF_AV_FIXED = 8 * 4 * AV_MAX_STATES + 8 * AV_MAX_STATES + 8 * 3 * SC_WAVES + 64 + 2 * 4 * AV_MAX_STATES + 4 * PF_PRED_WORDS;
static_assert(PF_AV_FIXED == 3680 && DS_SCRATCH <= 64, "the bytes include/rnampnn_hip.h gives");

struct PfAvArgs : AvChainArgs {
    int32_t* miss;               // (B) or null
    PfOut out;
};

__global__ void __launch_bounds__(SC_THREADS) k_design_avoid_profile(PfAvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfa_lds[];
    const int T = a.T, b = blockIdx.x, tid = threadIdx.x, A = a.A, AL = a.live;
    double* zs = reinterpret_cast<double*>(pfa_lds);                                // [T][4]      z of a position
    double* tab = zs + 4 * (size_t)T;                                              // [T][AL]     l_t of a live state
    double* cand = tab + (size_t)AL * T;                                           // [64][4]     alpha_t(a) + z_t(c) of an admitted live cell
    double* tmax = cand + 4 * AV_MAX_STATES;                                       // [64]        the maximum over the cells that lead into a state
    double (*s_d)[SC_WAVES] = reinterpret_cast<double (*)[SC_WAVES]>(tmax + AV_MAX_STATES);
    unsigned char* red = reinterpret_cast<unsigned char*>(s_d + 3);                // the reduction's scratch, 64 bytes
    const DsScratch sc = ds_scratch(red);
    unsigned* nx = reinterpret_cast<unsigned*>(red + 64);                          // [64]        delta(a, .), a byte per class
    unsigned* col = nx + AV_MAX_STATES;                                            // [64]        the table column of delta(a, .), or AV_DEAD
    unsigned* pw = col + AV_MAX_STATES;                                            // [112]       the predecessor cells 4 a + c of every state, cell order,
    unsigned char* pcell = reinterpret_cast<unsigned char*>(pw);                   //             four to a word, a state's list starting on a word
    unsigned char* ms = pcell + 4 * PF_PRED_WORDS;                                 // [T]         the mask of a position
    const unsigned long long term = a.terminal;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    // ---- A: rows, masks, the free sum and the automaton
    int bad = 0;
    double free_sum = 0.0;
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad, [&](int, const DsPos<double>& p) { free_sum += ds_lse<4>(p.z, 15); });
    if (tid < AV_MAX_STATES) {
        unsigned raw = 0, cl = 0;
        for (int c = 0; c < 4; ++c) {
            const unsigned nxt = tid < A ? a.delta[4 * tid + c] : AV_DEAD;
            const bool dead = nxt >= (unsigned)A || ((term >> (nxt & 63u)) & 1ull);
            raw |= (nxt & 255u) << (8 * c);
            cl |= (dead ? AV_DEAD : (unsigned)__popcll(~term & ((1ull << (nxt & 63u)) - 1ull))) << (8 * c);      // live states before it
        }
        nx[tid] = raw; col[tid] = cl;
    }
    __syncthreads();
    // ---- B: l_t(a), t = n-1 .. 0, as k_design_avoid forms it; one wave, lane = state; then the predecessor lists
    const bool live = tid < A && !((term >> (tid & 63)) & 1ull);
    int cc[4] = {0, 0, 0, 0}, ok = 0, mine = 0, pwoff = 0, pcnt = 0;
    if (tid < AV_MAX_STATES) {
        const unsigned cl = col[tid];
        mine = __popcll(~term & ((1ull << tid) - 1ull));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned k = (cl >> (8 * c)) & 255u;
            ok |= (k != AV_DEAD ? 1 : 0) << c;
            cc[c] = k != AV_DEAD ? (int)k : 0;
        }
        for (int t = n - 1; t >= 0; --t) {
            if (live) {
                const double* next = tab + (size_t)(t + 1) * AL;
                double l[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) l[c] = t + 1 < n ? next[cc[c]] : 0.0;
                const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
                const double v[4] = {z01.x + l[0], z01.y + l[1], z23.x + l[2], z23.y + l[3]};
                tab[(size_t)t * AL + mine] = ds_lse<4>(v, (int)ms[t] & ok);
            }
            ds_wave_sync();
        }
        // the cells (a, c) of a live a < A whose delta is the live state `tid`, counted, scanned over the lanes, then listed in cell order
        int cnt = 0;
        for (int cell = 0; cell < 4 * A; ++cell) {
            const int src = cell >> 2;
            const bool src_live = !((term >> src) & 1ull);
            cnt += live && src_live && ((nx[src] >> (8 * (cell & 3))) & 255u) == (unsigned)tid ? 1 : 0;
        }
        const int words = (cnt + 3) >> 2;
        int incl = words;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (tid >= o) incl += v;
        }
        pwoff = incl - words;                                       // <= 112 - words: 256 cells and at most three bytes of padding per list
        pcnt = cnt;
        for (int w = 0; w < words; ++w) pw[pwoff + w] = 0u;
        int at = 4 * pwoff;
        for (int cell = 0; cell < 4 * A; ++cell) {
            const int src = cell >> 2;
            const bool src_live = !((term >> src) & 1ull);
            if (live && src_live && ((nx[src] >> (8 * (cell & 3))) & 255u) == (unsigned)tid) pcell[at++] = (unsigned char)cell;
        }
    }
    __syncthreads();
    const bool miss = n > 0 && !(tab[0] > -INFINITY);               // state 0 is live and has column 0
    const double log_z = n > 0 && !miss ? tab[0] : 0.0;
    double pz_sum = 0.0, lz_sum = 0.0;
    if (miss) {
        // ---- C': no admitted sequence avoids the motifs: the per-position softmax over the admitted classes, as the draw falls back to
        pf_softmax_rows(a.out.marg, zs, ms, pad0, n, tid, pz_sum, lz_sum);
    } else if (tid < AV_MAX_STATES) {
        // ---- C: the forward walk; alpha_t(a) in the register of lane a.  The LSE of a state's incoming cells is split so that no lane
        // runs more than four exps per step whatever the fan-in of its state: the TARGET takes the maximum over its list, the SOURCES
        // turn their own four candidates into exp(candidate - that maximum) in place, the target adds them up in cell order.
        double alpha = tid == 0 ? 0.0 : -INFINITY;
        const unsigned raw = nx[tid];
        const unsigned w0 = pcnt > 0 ? pw[pwoff] : 0u, w1 = pcnt > 4 ? pw[pwoff + 1] : 0u;      // the first eight cells of the list stay in registers
        // over the list, four cells to a word: one read for the word (none for the first two), four independent reads of the candidates
        auto over_list = [&](auto visit) {
            for (int w = 0; 4 * w < pcnt; ++w) {
                const unsigned cells = w == 0 ? w0 : w == 1 ? w1 : pw[pwoff + w];
                double v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = cand[(cells >> (8 * j)) & 255u];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * w + j < pcnt) visit(v[j]);
            }
        };
        for (int t = 0; t < n; ++t) {
            const double2 z01 = *reinterpret_cast<const double2*>(zs + 4 * t), z23 = *reinterpret_cast<const double2*>(zs + 4 * t + 2);
            const double z[4] = {z01.x, z01.y, z23.x, z23.y};
            const int m = live ? ((int)ms[t] & ok) : 0;
            const double* next = tab + (size_t)(t + 1) * AL;
            double p[4], av[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool in = (m >> c) & 1;
                const double l = t + 1 < n ? next[cc[c]] : 0.0;     // (cc is 0 for a dead cell: in bounds, not used)
                av[c] = alpha + z[c];
                p[c] = sc_wave_sum(in ? exp(av[c] + l - log_z) : 0.0);
                cand[4 * tid + c] = in ? av[c] : -INFINITY;
            }
            if (tid == 0) {
                pf_store4(a.out.marg, pad0 + t, p);
#pragma unroll
                for (int c = 0; c < 4; ++c) pz_sum += pf_pz(p[c], z[c]);
            }
            if (t + 1 == n) break;
            ds_wave_sync();
            double mx = -INFINITY, sum = 0.0;
            over_list([&](double v) { mx = fmax(mx, v); });
            tmax[tid] = mx;
            ds_wave_sync();
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double tm = tmax[(raw >> (8 * c)) & 63u];     // (the state this cell leads to; read only for an admitted live cell)
                cand[4 * tid + c] = ((m >> c) & 1) && tm > -INFINITY ? exp(av[c] - tm) : 0.0;
            }
            ds_wave_sync();
            over_list([&](double v) { sum += v; });
            alpha = mx > -INFINITY ? mx + log(sum) : -INFINITY;
            ds_wave_sync();                                         // the candidates are overwritten by the next step
        }
    }
    pf_finish(a.out, a, a.miss, miss ? 1 : 0, b, n, tid, bad, free_sum, pz_sum, lz_sum, miss, log_z, sc, s_d);
}

// the bytes of dynamic LDS, from (T, live states) alone: the formula include/rnampnn_hip.h gives
size_t pf_av_lds_bytes(long long T, long long live) { return av_rows_bytes(T, live) + PF_AV_FIXED; }
}  // namespace

extern "C" int rnampnn_design_count_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                            float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                            int32_t bias_per_position, const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi,
                                            int32_t count_cap, double* marginals, double* log_z, double* log_z_free, double* entropy,
                                            int32_t* infeasible, int32_t* count_miss, void* stream) {
    const char* name = "rnampnn_design_count_profile";
    const PfAsked asked{name, marginals, log_z, log_z_free, entropy, infeasible, count_miss};
    PfCtArgs a{};
    const int rc = ds_prepare(name, "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, 1, 0, nullptr, allowed, partner, wobble, bias,
                              bias_per_position, nullptr, nullptr, infeasible, a, [&](int slot) {
        return slot == 0 ? ct_count_side(name, counted, count_lo, count_hi, count_cap, T, 0, a) : asked.aligned();
    });
    if (rc != RNAMPNN_OK) return rc;
    if (asked.nothing()) return RNAMPNN_OK;
    size_t lds_tree = 0;
    const size_t lds = pf_ct_lds_bytes(T, a.cap, lds_tree);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED,
                    "rnampnn_design_count_profile: T = %d at count_cap = %d needs %zu bytes of LDS for the inside and the outside tree, the limit is "
                    "%zu (T <= %d at that cap)", (int)T, (int)count_cap, lds, DS_LDS_MAX, pf_ct_max_T(count_cap));
    a.count = nullptr; a.miss = count_miss;
    a.lds_tree = (unsigned)lds_tree; a.lds_sq = 0;
    a.out = asked.out();
    return ds_launch<k_design_count_profile>(dim3(B), lds, stream, a);
}

extern "C" int rnampnn_design_avoid_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                            float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                            int32_t bias_per_position, const uint8_t* delta, int32_t n_states, uint64_t terminal,
                                            double* marginals, double* log_z, double* log_z_free, double* entropy, int32_t* infeasible,
                                            int32_t* avoid_miss, void* stream) {
    const PfAsked asked{"rnampnn_design_avoid_profile", marginals, log_z, log_z_free, entropy, infeasible, avoid_miss};
    PfAvArgs a{};
    const int rc = av_prepare(asked.name, logits, n_rows, mask, cu_seqlens, B, T, temperature, 1, 0, nullptr, allowed, partner, wobble, bias,
                              bias_per_position, nullptr, nullptr, infeasible, delta, n_states, terminal, a, [&] { return asked.aligned(); });
    if (rc != RNAMPNN_OK) return rc;
    if (asked.nothing()) return RNAMPNN_OK;
    const size_t lds = pf_av_lds_bytes(T, a.live);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_avoid_profile: T = %d with %d live states needs %zu bytes of LDS for the table of "
                    "partition sums, the limit is %zu (T <= %lld at this automaton)", (int)T, a.live, lds, DS_LDS_MAX,
                    ds_max_T([&](long long t) { return pf_av_lds_bytes(t, a.live); }));
    a.miss = avoid_miss; a.out = asked.out();
    return ds_launch<k_design_avoid_profile>(dim3(B), lds, stream, a);
}
