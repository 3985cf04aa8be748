// rnampnn_design_tied: multi-state design.  A GROUP of consecutive batch rows (its states: conformers of one RNA, or the two backbones of a
// switch) receives ONE sequence per sample, drawn from the product of the states' distributions under the UNION of their base-pair tables.
// The union has degree <= 2 after each position keeps its first two distinct partners, so every component is an isolated position, a path
// or a cycle, and the joint over a component is drawn exactly: forward weights alpha_k along the chain, kept as lambda_k = log alpha_k and
// normalised at every step (at a temperature of 1e-3 exp(z - max) is 0 for every class but one, and the constrained optimum need not use
// that one), the last node from lambda, then backwards each node given its successor; a cycle first draws its head class from the four
// conditioned partition sums.  The contract is the one include/rnampnn_hip.h documents and tests/_design_tied_ref.py restates; all of the
// draw is fp64.
// An isolated position, a 2-node path and every selection along a chain are design_dev.h's rule - the templates k_design instantiates in
// f32 - so one state per group draws what rnampnn_design draws.  One 256-thread workgroup per (group, sample), the extent / NLL /
// reduction of score_dev.h per state row, so seq_nll is byte for byte rnampnn_score's for the written rows.  Three phases separated by barriers: (A) the thread that owns v_0 of a
// component walks it and leaves the classes of its nodes in LDS (`sq`, one byte per position; lambda_k is parked in LDS at 32 bytes per
// position, both indexed by position: nothing is allocated, nothing depends on timing); (B) every thread draws what is still open as an
// isolated position and writes the group's rows; (C) per state the NLL.  Neighbour lists are never stored: a step recomputes them from the
// tables (2 M loads per node looked at).  No atomics, no workspace, no host synchronisation.
#include "design_dev.h"

namespace {
struct TiedArgs : DesignArgs {
    const int32_t* group_cu;     // (G+1)
    const float* weight;         // (B) or null
    unsigned lds_alpha, lds_sq;  // bytes of the two LDS arrays (alpha: 0 without a partner table)
};

struct TdGroup { int b0, M, n; };        // first row, number of states, common length
using TdPos = DsPos<double>;              // z = (sum_m weight_m logit_m + bias) / temperature; m = the AND of the states' masks (never empty)
struct TdKeep { int k0, k1, over; };     // the first two distinct well-formed partners of a position in state order; over: there was a third

__device__ __forceinline__ int td_mask(const TiedArgs& a, const TdGroup& g, int t, bool& empty) {
    int m = 15;
    if (a.allowed)
        for (int i = 0; i < g.M; ++i) m &= a.allowed[(size_t)(g.b0 + i) * a.T + t];
    m &= 15;
    empty = m == 0;
    return empty ? 15 : m;
}

__device__ __forceinline__ TdPos td_load(const TiedArgs& a, const TdGroup& g, int t, bool& empty) {
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
    for (int i = 0; i < g.M; ++i) {
        const float4 x = a.logits[sc_row0(a, g.b0 + i) + t];
        const double w = a.weight ? (double)a.weight[g.b0 + i] : 1.0;
        z0 += w * (double)x.x; z1 += w * (double)x.y; z2 += w * (double)x.z; z3 += w * (double)x.w;
    }
    if (a.bias) {
        const float4 bi = a.bias_per_position ? reinterpret_cast<const float4*>(a.bias)[(size_t)g.b0 * a.T + t]
                                              : make_float4(a.bias[0], a.bias[1], a.bias[2], a.bias[3]);
        z0 += (double)bi.x; z1 += (double)bi.y; z2 += (double)bi.z; z3 += (double)bi.w;
    }
    const double temp = (double)a.temperature;
    TdPos p;
    p.z[0] = z0 / temp; p.z[1] = z1 / temp; p.z[2] = z2 / temp; p.z[3] = z3 / temp;
    p.m = td_mask(a, g, t, empty);
    return p;
}

// every index is checked before it is used: a malformed table never causes an out-of-range access
__device__ __forceinline__ TdKeep td_keep(const TiedArgs& a, const TdGroup& g, int t) {
    TdKeep k{-1, -1, 0};
    for (int i = 0; i < g.M; ++i) {
        const int32_t* p = a.partner + (size_t)(g.b0 + i) * a.T;
        const int j = p[t];
        if (j < 0 || j >= g.n || j == t || p[j] != t) continue;
        if (j == k.k0 || j == k.k1) continue;
        if (k.k0 < 0) k.k0 = j;
        else if (k.k1 < 0) k.k1 = j;
        else k.over = 1;
    }
    return k;
}

__device__ __forceinline__ bool td_keeps(const TiedArgs& a, const TdGroup& g, int j, int t) {    // does j keep t ?
    const TdKeep k = td_keep(a, g, j);
    return k.k0 == t || k.k1 == t;
}

// the live neighbour of cur other than prev (the edge prev - cur is live), or -1
__device__ __forceinline__ int td_next(const TiedArgs& a, const TdGroup& g, int cur, int prev) {
    const TdKeep k = td_keep(a, g, cur);
    const int cand = k.k0 == prev ? k.k1 : k.k1 == prev ? k.k0 : -1;
    return cand >= 0 && td_keeps(a, g, cand, cur) ? cand : -1;
}

// log(exp(x) + exp(y)) and its one-term form; -inf when no term is above -inf (NaN included)
__device__ __forceinline__ double td_lse1(double x) { return x > -INFINITY ? x : -INFINITY; }
__device__ __forceinline__ double td_lse2(double x, double y) {
    const double m = fmax(x, y);
    return m > -INFINITY ? m + log(exp(x - m) + exp(y - m)) : -INFINITY;
}

// lambda = log alpha.  lambda(c) <- z(c) + log sum_{a pairs with c} exp(lambda(a)) for the classes the mask admits (-inf for the others),
// minus its largest component, which is added to lognorm; false when that component is not above -inf (an infeasible chain)
__device__ __forceinline__ bool td_step(const TdPos& p, double (&la)[4], int wobble, double& lognorm) {
    const double t0 = td_lse1(la[1]), t1 = wobble ? td_lse2(la[0], la[3]) : td_lse1(la[0]);
    const double t2 = td_lse1(la[3]), t3 = wobble ? td_lse2(la[1], la[2]) : td_lse1(la[2]);
    const double n0 = (p.m & 1) ? p.z[0] + t0 : -INFINITY, n1 = (p.m & 2) ? p.z[1] + t1 : -INFINITY;
    const double n2 = (p.m & 4) ? p.z[2] + t2 : -INFINITY, n3 = (p.m & 8) ? p.z[3] + t3 : -INFINITY;
    const double mx = fmax(fmax(n0, n1), fmax(n2, n3));
    if (!(mx > -INFINITY)) return false;
    la[0] = n0 - mx; la[1] = n1 - mx; la[2] = n2 - mx; la[3] = n3 - mx;
    lognorm += mx;
    return true;
}

// The component v_0, v_1, ... of L nodes (a path from its smaller end, or a cycle from its smallest node towards the smaller neighbour),
// walked by one thread.  Leaves the drawn classes in sq; an infeasible component leaves sq untouched (-1: every node then draws as an
// isolated position in phase B) and counts its nodes.
__device__ __forceinline__ void td_component(const TiedArgs& a, const TdGroup& g, int s, unsigned long long seed, int v0, int v1, int L,
                                             bool cyc, double* alpha, int8_t* sq, int& bad) {
    bool e;
    const TdPos p0 = td_load(a, g, v0, e);
    if (!cyc && L == 2) {
        const TdPos p1 = td_load(a, g, v1, e);
        const int cell = ds_draw_pair(p0, p1, a.wobble, ds_u24(seed, s, g.b0, v0));
        if (cell >= 0) { sq[v0] = (int8_t)(cell >> 2); sq[v1] = (int8_t)(cell & 3); }
        else bad += 2;
        return;
    }
    double l0[4], la[4];                                           // lambda_0 = log omega_0
    {
        double mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((p0.m >> c) & 1) mx = fmax(mx, p0.z[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) l0[c] = ((p0.m >> c) & 1) ? p0.z[c] - mx : -INFINITY;
    }
    double lz0 = -INFINITY, lz1 = -INFINITY, lz2 = -INFINITY, lz3 = -INFINITY;     // log Z_h of a cycle
    int head = -1, last = v0, before = v0;
    for (int pass = cyc ? 0 : 4; pass <= 4; ++pass) {              // passes 0..3: Z_h of a cycle; pass 4: the stored forward pass
        if (pass == 4 && cyc) {
            const double mx = fmax(fmax(lz0, lz1), fmax(lz2, lz3));
            if (!(mx > -INFINITY)) { bad += L; return; }
            const double w[4] = {exp(lz0 - mx), exp(lz1 - mx), exp(lz2 - mx), exp(lz3 - mx)};
            head = ds_select(w, p0.m, ds_u24(seed, s, g.b0, v0));
        }
        const int hh = pass < 4 ? pass : head;
#pragma unroll
        for (int c = 0; c < 4; ++c) la[c] = (hh < 0 || hh == c) ? l0[c] : -INFINITY;
        if (pass < 4 && !(fmax(fmax(la[0], la[1]), fmax(la[2], la[3])) > -INFINITY)) continue;
        if (pass == 4 && !cyc) {
#pragma unroll
            for (int c = 0; c < 4; ++c) alpha[(size_t)v0 * 4 + c] = la[c];
        }
        double lognorm = 0.0;
        bool ok = true;
        int pv = v0, cur = v1;
        for (int k = 1; k < L; ++k) {                              // L <= n: no table can make this spin
            if (cur < 0) { ok = false; break; }
            const TdPos p = td_load(a, g, cur, e);
            ok = td_step(p, la, a.wobble, lognorm);
            if (!ok) break;
            if (pass == 4) {
#pragma unroll
                for (int c = 0; c < 4; ++c) alpha[(size_t)cur * 4 + c] = la[c];
            }
            if (k + 1 < L) {
                const int nx = td_next(a, g, cur, pv);
                pv = cur; cur = nx;
            }
        }
        if (pass == 4) {
            if (!ok) { bad += L; return; }
            last = cur; before = pv;
        } else {
            const double t = hh == 0 ? td_lse1(la[1]) : hh == 1 ? (a.wobble ? td_lse2(la[0], la[3]) : td_lse1(la[0]))
                           : hh == 2 ? td_lse1(la[3]) : (a.wobble ? td_lse2(la[1], la[2]) : td_lse1(la[2]));
            const double lz = ok ? t + lognorm : -INFINITY;
            lz0 = pass == 0 ? lz : lz0; lz1 = pass == 1 ? lz : lz1; lz2 = pass == 2 ? lz : lz2; lz3 = pass == 3 ? lz : lz3;
        }
    }
    // v_{L-1} from lambda_{L-1} (a cycle: over the classes that pair with the head), then backwards: v_k from lambda_k over the classes
    // that pair with c_{k+1}
    double w[4];                                                   // exp(lambda(c) - max over the eligible classes), 0 for the others
    ds_weights(la, cyc ? ds_compat(head, a.wobble) : 15, w);
    int c_succ = ds_select(w, td_mask(a, g, last, e), ds_u24(seed, s, g.b0, last));
    sq[last] = (int8_t)c_succ;
    const int stop = cyc ? 1 : 0;
    int succ = last, cur = before;
    for (int k = L - 2; k >= stop && cur >= 0; --k) {
#pragma unroll
        for (int c = 0; c < 4; ++c) la[c] = alpha[(size_t)cur * 4 + c];
        ds_weights(la, ds_compat(c_succ, a.wobble), w);
        c_succ = ds_select(w, td_mask(a, g, cur, e), ds_u24(seed, s, g.b0, cur));
        sq[cur] = (int8_t)c_succ;
        if (k > stop) {
            const int nx = td_next(a, g, cur, succ);
            succ = cur; cur = nx;
        }
    }
    if (cyc) sq[v0] = (int8_t)head;
}

__global__ void __launch_bounds__(SC_THREADS) k_design_tied(TiedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char td_lds[];
    double* alpha = reinterpret_cast<double*>(td_lds);                                         // (T,4), with a partner table only
    int8_t* sq = reinterpret_cast<int8_t*>(td_lds + a.lds_alpha);                              // (T)
    const DsScratch sc = ds_scratch(td_lds + a.lds_alpha + a.lds_sq);
    int* const s_i = sc.s_i;
    float (*const s_f)[SC_WAVES] = sc.s_f;
    const int s = blockIdx.y, tid = threadIdx.x;
    TdGroup g;
    g.b0 = min(max((int)a.group_cu[blockIdx.x], 0), a.B);
    g.M = min(max((int)a.group_cu[blockIdx.x + 1], 0), a.B) - g.b0;
    if (g.M <= 0) return;                                          // an empty group writes nothing (uniform over the workgroup)
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    g.n = a.T;
    for (int i = 0; i < g.M; ++i) {
        int n;
        long long row0;
        sc_extent(a, g.b0 + i, tid, s_f[0], n, row0);
        g.n = min(g.n, n);
    }
    int bad = 0;
    // ---- A: the components of the union graph
    if (a.partner) {
        for (int t = tid; t < g.n; t += SC_THREADS) sq[t] = (int8_t)-1;
        __syncthreads();
        for (int t = tid; t < g.n; t += SC_THREADS) {
            const TdKeep kp = td_keep(a, g, t);
            bad += kp.over;
            int l0 = kp.k0 >= 0 && td_keeps(a, g, kp.k0, t) ? kp.k0 : -1;
            int l1 = kp.k1 >= 0 && td_keeps(a, g, kp.k1, t) ? kp.k1 : -1;
            if (l0 < 0) { l0 = l1; l1 = -1; }
            if (l0 < 0) continue;                                  // isolated: phase B
            // is t the v_0 of its component ?  a path's smaller end, a cycle's smallest node
            int v1, L = 2, prev = t, cur;
            bool cyc = false, own = false;
            if (l1 < 0) {
                v1 = cur = l0;
                for (int st = 0; st < g.n; ++st) {
                    const int nx = td_next(a, g, cur, prev);
                    if (nx < 0) { own = t < cur; break; }
                    prev = cur; cur = nx; ++L;
                }
            } else {
                if (l0 < t || l1 < t) continue;
                v1 = cur = min(l0, l1);
                for (int st = 0; st < g.n; ++st) {
                    const int nx = td_next(a, g, cur, prev);
                    if (nx < 0 || nx < t) break;                   // an inner node of a path, or not the smallest of its cycle
                    if (nx == t) { own = cyc = true; break; }
                    prev = cur; cur = nx; ++L;
                }
            }
            if (own && L <= g.n) td_component(a, g, s, seed, t, v1, L, cyc, alpha, sq, bad);
        }
        __syncthreads();
    }
    // ---- B: what is still open draws as an isolated position; the group's rows
    for (int t = tid; t < g.n; t += SC_THREADS) {
        int q = a.partner ? (int)sq[t] : -1;
        bool empty;
        if (q < 0) {
            const TdPos p = td_load(a, g, t, empty);
            q = ds_draw_single(p, ds_u24(seed, s, g.b0, t));
        } else {
            td_mask(a, g, t, empty);
        }
        bad += empty ? 1 : 0;
        sq[t] = (int8_t)q;
        if (a.seqs)
            for (int i = 0; i < g.M; ++i) a.seqs[((size_t)s * a.B + g.b0 + i) * a.T + t] = (int8_t)q;
    }
    if (a.seqs)
        for (int i = 0; i < g.M; ++i)
            for (int t = g.n + tid; t < a.T; t += SC_THREADS) a.seqs[((size_t)s * a.B + g.b0 + i) * a.T + t] = (int8_t)-1;
    // ---- C: per state row the NLL of the written row, as k_score walks and reduces it (a row longer than the group reads class 3 at its
    // -1 entries, as k_score does); the group's count rides on the first reduction
    const int rounds = a.seq_nll ? g.M : 1;
    for (int i = 0; i < rounds; ++i) {
        float nll = 0.f, unused = 0.f;
        int cnt = i == 0 ? bad : 0;
        if (a.seq_nll) {
            int n;
            long long row0;
            sc_extent(a, g.b0 + i, tid, s_f[0], n, row0);
            for (int t = tid; t < n; t += SC_THREADS) nll += sc_row_nll(a.logits[row0 + t], t < g.n ? (int)sq[t] : -1);
        }
        sc_block_sums(cnt, nll, unused, tid, s_i, s_f);
        if (tid == 0) {
            if (a.seq_nll) a.seq_nll[(size_t)s * a.B + g.b0 + i] = nll;
            if (i == 0 && a.infeasible && s == 0)
                for (int r = 0; r < g.M; ++r) a.infeasible[g.b0 + r] = cnt;
        }
        __syncthreads();                                           // s_i / s_f are written again in the next round
    }
}
}  // namespace

extern "C" int rnampnn_design_tied(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                   const int32_t* group_cu, int32_t G, const float* weight, float temperature, int32_t S, uint64_t seed,
                                   const uint64_t* seed_dev, const uint8_t* allowed, const int32_t* partner, int32_t wobble,
                                   const float* bias, int32_t bias_per_position, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                                   void* stream) {
    TiedArgs a{};
    const int rc = ds_prepare("rnampnn_design_tied", "group", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed,
                              partner, wobble, bias, bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0 && (!group_cu || G <= 0))
            return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design_tied: null group_cu or no group (G = %d)", (int)G);
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible) return RNAMPNN_OK;    // nothing asked for
    // LDS by position: 32 bytes of alpha (with a partner table only) + 1 byte of class id, + the reduction's scratch, padded to 64 bytes
    static_assert(DS_SCRATCH <= 64, "the reduction's scratch");
    const size_t lds_alpha = partner ? (size_t)T * 32 : 0, lds_sq = ((size_t)T + 15) & ~(size_t)15, lds = lds_alpha + lds_sq + 64;
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_tied: T = %d needs %zu bytes of LDS, the limit is %zu (T <= %d with a partner table)",
                    (int)T, lds, DS_LDS_MAX, (int)((DS_LDS_MAX - 64 - 15) / 33));
    a.group_cu = group_cu; a.weight = weight;
    a.lds_alpha = (unsigned)lds_alpha; a.lds_sq = (unsigned)lds_sq;
    const int passes = (seqs || seq_nll) ? S : 1;               // the count of infeasible positions is that of sample 0
    return ds_launch<k_design_tied>(dim3(G, passes), lds, stream, a);
}
