// Pieces shared by the profile kernels - k_design_count_profile and k_design_avoid_profile (design_profile.hip), which keep their tables in
// LDS, the count profile on a tree in global memory (design_long.hip) and k_design_dfa_profile (design_dfa_profile.hip) - and by their
// four entries: the outputs as the caller passed them (PfAsked: the alignment check, "nothing asked for", the kernel's PfOut), the miss
// fallback of the two automaton profiles (pf_softmax_rows), the outputs and their final writer (PfOut, pf_finish), the
// fixed-order fp64 workgroup sums, and of the count profile phase B (pf_ct_root: the target, K*, log_z and the root's outside), one
// coefficient of the outside pass (pf_outside) and phase D (pf_ct_leaves: the leaves' outsides and marginals).  One definition of each, so
// the two homes of the tree return the same bytes.
#pragma once
#include "count_tree_dev.h"

namespace {
struct PfOut {
    double* marg;                // (B,T,4) or null
    double* log_z;               // (B) or null
    double* log_z_free;          // (B) or null
    double* entropy;             // (B) or null
};

// The outputs of a profile entry as its caller passed them, and what the four entries do with them on the host: the check of slot 1
// (before the entry's workspace check, where it has one), "nothing asked for", and the kernel's PfOut.
struct PfAsked {
    const char* name;
    double *marginals, *log_z, *log_z_free, *entropy;
    int32_t *infeasible, *miss;
    int aligned() const {
        if (marginals && ((uintptr_t)marginals & 15) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: marginals must be 16-byte aligned", name);
        return RNAMPNN_OK;
    }
    bool nothing() const { return !marginals && !log_z && !log_z_free && !entropy && !infeasible && !miss; }
    PfOut out() const { return PfOut{marginals, log_z, log_z_free, entropy}; }
};

// The workgroup's totals of three doubles: wave butterfly, then one LDS hop over the four waves in ascending order - a fixed order, so two
// calls give the same bytes.  Valid in thread 0 only; every thread calls it (one barrier).  s_d holds 3 x SC_WAVES doubles.
__device__ __forceinline__ void pf_block_sums(double& x, double& y, double& z, int tid, double (*s_d)[SC_WAVES]) {
    x = sc_wave_sum(x); y = sc_wave_sum(y); z = sc_wave_sum(z);
    if ((tid & 63) == 0) { s_d[0][tid >> 6] = x; s_d[1][tid >> 6] = y; s_d[2][tid >> 6] = z; }
    __syncthreads();
    if (tid != 0) return;
    x = 0.0; y = 0.0; z = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { x += s_d[0][w]; y += s_d[1][w]; z += s_d[2][w]; }
}
// P z for the entropy: a class of probability 0 is skipped (its z may be -inf)
__device__ __forceinline__ double pf_pz(double p, double z) { return p != 0.0 ? p * z : 0.0; }
__device__ __forceinline__ void pf_store4(double* marg, size_t row, const double (&p)[4]) {
    if (!marg) return;
    double2* out = reinterpret_cast<double2*>(marg + 4 * row);
    out[0] = make_double2(p[0], p[1]); out[1] = make_double2(p[2], p[3]);
}
// What the two automaton profiles write on a miss (no admitted sequence passes the automaton), every thread: the per-position softmax
// over the admitted classes from the rows and masks in LDS, as the draw falls back to.  pz_sum, lz_sum: this thread's shares of the sum
// of P z and of log_z, which is then the sum of the positions' logsumexps.
__device__ __forceinline__ void pf_softmax_rows(double* marg, const double* zs, const unsigned char* ms, size_t pad0, int n, int tid, double& pz_sum,
                                                double& lz_sum) {
    for (int t = tid; t < n; t += SC_THREADS) {
        const double z[4] = {zs[4 * t], zs[4 * t + 1], zs[4 * t + 2], zs[4 * t + 3]};
        const int m = ms[t];
        const double l = ds_lse<4>(z, m);
        double p[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            p[c] = ((m >> c) & 1) ? exp(z[c] - l) : 0.0;
            pz_sum += pf_pz(p[c], z[c]);
        }
        lz_sum += l;
        pf_store4(marg, pad0 + t, p);
    }
}
// what every thread and the final writer share
__device__ __forceinline__ void pf_finish(const PfOut& o, const DesignArgs& a, int32_t* miss_out, int miss, int b, int n, int tid, int bad, double free_sum,
                                          double pz_sum, double lz_sum, bool lz_from_sum, double log_z, const DsScratch& sc, double (*s_d)[SC_WAVES]) {
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = n + tid; t < a.T; t += SC_THREADS) pf_store4(o.marg, (size_t)b * a.T + t, zero);
    float f0 = 0.f, f1 = 0.f;
    sc_block_sums(bad, f0, f1, tid, sc.s_i, sc.s_f);
    pf_block_sums(free_sum, pz_sum, lz_sum, tid, s_d);
    if (tid != 0) return;
    const double lz = n == 0 ? 0.0 : lz_from_sum ? lz_sum : log_z;
    if (o.log_z) o.log_z[b] = lz;
    if (o.log_z_free) o.log_z_free[b] = n == 0 ? 0.0 : free_sum;
    if (o.entropy) o.entropy[b] = n == 0 ? 0.0 : lz - pz_sum;
    if (a.infeasible) a.infeasible[b] = bad;
    if (miss_out) miss_out[b] = miss;
}

// ---------------------------------------------------------------------------------------------------------------- the count profile
constexpr size_t PF_CT_SCRATCH = 240;          // DS_SCRATCH 48 | at 48 two flags | at 64 the 1-mer's leaf | at 96 its outside | at 120 log_z | at 128 3 x 4 sums
static_assert(DS_SCRATCH == 48 && CT_LDS_SCRATCH == 96, "the layout of the count profile's scratch");

struct PfCtArgs : CtArgs { PfOut out; };

// the count profile's scratch at scr (PF_CT_SCRATCH bytes of LDS, 8-byte aligned)
struct PfCtScratch { DsScratch sc; int* s_flag; double* s_leaf; double* o_leaf; double* s_logz; double (*s_d)[SC_WAVES]; };
__device__ __forceinline__ PfCtScratch pf_ct_scratch(unsigned char* scr) {
    return PfCtScratch{ds_scratch(scr),
                       reinterpret_cast<int*>(scr + 48),                                     // [0]: every leaf at its own minimum; [1]: count_miss
                       reinterpret_cast<double*>(scr + 64),                                  // 3 doubles
                       reinterpret_cast<double*>(scr + 96),                                  // 3 doubles
                       reinterpret_cast<double*>(scr + 120),
                       reinterpret_cast<double (*)[SC_WAVES]>(scr + 128)};
}

// Phase B, every lane of wave 0 (n > 0): ct_target - the window, the target and count_miss of the draw; K* = the finite counts of the
// window, or the target alone; log_z = LSE over K* of the root, by the wave in a fixed order; the root's outside O(k) = 0 on K*, -inf
// elsewhere, into oroot when it is given.  Lane 0 leaves (at_min, miss) in s_flag and log_z in s_logz.  s_i: k_min per wave.
__device__ __forceinline__ void pf_ct_root(const CtArgs& a, const double* root, double* oroot, const int* s_i, int b, int n, int Ln, int lane,
                                           int* s_flag, double* s_logz) {
    const CtTarget g = ct_target<true>(a, root, s_i, b, n, Ln);
    const int deg = g.deg, lo = g.lo, hi = g.hi, K = g.K;
    const bool any = g.any;
    double mx = -INFINITY, sum = 0.0;
    for (int k = lane; k <= deg; k += 64) {
        const bool in = (any ? (k >= lo && k <= hi) : k == K) && ct_finite(root[k]);
        if (in) mx = fmax(mx, root[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    for (int k = lane; k <= deg; k += 64) {
        const bool in = (any ? (k >= lo && k <= hi) : k == K) && ct_finite(root[k]);
        if (in) sum += exp(root[k] - mx);
        if (oroot) oroot[k] = in ? 0.0 : -INFINITY;
    }
    sum = sc_wave_sum(sum);
    if (lane == 0) {
        s_flag[0] = g.at_min ? 1 : 0; s_flag[1] = g.miss;
        *s_logz = mx > -INFINITY ? mx + log(sum) : -INFINITY;
    }
}

// Coefficient c <= deg of the outside of child node (l - 1, j) from `O`, the first double of level l of the outside tree, and `below`, the
// first double of level l - 1 of the INSIDE tree (stride: level l's; cstride, cnodes: level l - 1's): one ct_lse_terms over the parent's
// outside and the sibling's inside in index order; a node whose right half is empty hands its outside to its left half.
__device__ __forceinline__ double pf_outside(const double* O, const double* below, int l, int j, int c, int n, int cap, int stride, int cstride,
                                             int cnodes) {
    const int i = j >> 1, sib = j ^ 1, degP = ct_deg(l, i, n, cap);
    O += (size_t)i * stride;
    if (sib >= cnodes) return c <= degP ? O[c] : -INFINITY;
    const double* Sb = below + (size_t)sib * cstride;
    return ct_lse_terms(c, min(c + ct_deg(l - 1, sib, n, cap), degP), [&](int k) { return O[k] + Sb[k - c]; });
}

// LSE_k over k = k0 .. k1 of O[k] + p(k - k0 .. ) with the sibling LEAF's polynomial (s0, s1, s2): the outside of a leaf below a level-1 node
__device__ __forceinline__ double pf_leaf_outside(const double* O, int deg, int a, double s0, double s1, double s2) {
    double v[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) v[d] = a + d <= deg ? O[a + d] + ct_pick(s0, s1, s2, d) : -INFINITY;
    return ds_lse<3>(v, 7);
}

// The marginals of leaf t from w(d) = the log of what multiplies exp(z) of a cell that counts d; -> its share of the sum of P z.
__device__ __forceinline__ double pf_leaf_out(const PfCtArgs& a, const CtLeaf& lf, size_t pad0, int t, double w0, double w1, double w2) {
    if (lf.kind == 2) return 0.0;                                   // written by the owner of the pair
    double pz = 0.0;
    if (lf.kind == 0) {
        double p[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            p[c] = ((lf.p.m >> c) & 1) ? exp(lf.p.z[c] + ct_pick(w0, w1, w2, (lf.ci >> c) & 1)) : 0.0;
            pz += pf_pz(p[c], lf.p.z[c]);
        }
        pf_store4(a.out.marg, pad0 + t, p);
        return pz;
    }
    double pi[4] = {0.0, 0.0, 0.0, 0.0}, pj[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int d = ((lf.ci >> (c >> 2)) & 1) + ((lf.cj >> (c & 3)) & 1);
        const double pc = ((lf.m16 >> c) & 1) ? exp(lf.p.z[c >> 2] + lf.pj.z[c & 3] + ct_pick(w0, w1, w2, d)) : 0.0;
        pi[c >> 2] += pc; pj[c & 3] += pc;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) pz += pf_pz(pi[c], lf.p.z[c]) + pf_pz(pj[c], lf.pj.z[c]);
    pf_store4(a.out.marg, pad0 + t, pi);
    pf_store4(a.out.marg, pad0 + lf.j, pj);
    return pz;
}

// Phase D, every thread: one level-1 node per thread and turn - the two leaves again from the rows, their outsides from the node's (O1:
// the first double of level 1 of the outside tree; o_leaf: the outside of the only leaf of a 1-mer), then P = exp(z + O(d) - log_z) per
// admitted class / cell; the owner of a pair writes both ends.  Under the k_min rule every leaf is normalised over the cells of its own
// smallest d and lz_sum collects log_z.  pz_sum, lz_sum: this thread's shares.
__device__ __forceinline__ void pf_ct_leaves(const PfCtArgs& a, const double* O1, const double* o_leaf, size_t pad0, long long row0, int n, int tid,
                                             bool at_min, double log_z, double& pz_sum, double& lz_sum) {
    const int T = a.T, cap = a.cap;
    int unused_bad = 0;
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        const bool two = t + 1 < n;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        const CtLeaf ll = ct_leaf<true>(a, pad0, row0, n, t, l0, l1, l2, unused_bad);
        CtLeaf lr = ll;
        if (two) lr = ct_leaf<true>(a, pad0, row0, n, t + 1, r0, r1, r2, unused_bad);
        double wl0, wl1, wl2, wr0 = -INFINITY, wr1 = -INFINITY, wr2 = -INFINITY;
        if (at_min) {
            const int dl = ct_min_d(l0, l1, l2), dr = ct_min_d(r0, r1, r2);
            const double pl = ct_pick(l0, l1, l2, dl), pr = ct_pick(r0, r1, r2, dr);
            lz_sum += pl + (two ? pr : 0.0);
            wl0 = dl == 0 ? -pl : -INFINITY; wl1 = dl == 1 ? -pl : -INFINITY; wl2 = dl == 2 ? -pl : -INFINITY;
            wr0 = dr == 0 ? -pr : -INFINITY; wr1 = dr == 1 ? -pr : -INFINITY; wr2 = dr == 2 ? -pr : -INFINITY;
        } else {
            const double* O = n == 1 ? o_leaf : O1 + (size_t)i * ct_stride(1, T, cap);
            const int deg = n == 1 ? min(1, cap) : ct_deg(1, i, n, cap);
            if (two) {
                wl0 = pf_leaf_outside(O, deg, 0, r0, r1, r2) - log_z; wr0 = pf_leaf_outside(O, deg, 0, l0, l1, l2) - log_z;
                wl1 = pf_leaf_outside(O, deg, 1, r0, r1, r2) - log_z; wr1 = pf_leaf_outside(O, deg, 1, l0, l1, l2) - log_z;
                wl2 = pf_leaf_outside(O, deg, 2, r0, r1, r2) - log_z; wr2 = pf_leaf_outside(O, deg, 2, l0, l1, l2) - log_z;
            } else {                                                // an empty right half: the leaf is the node
                wl0 = O[0] - log_z; wl1 = (1 <= deg ? O[1] : -INFINITY) - log_z; wl2 = (2 <= deg ? O[2] : -INFINITY) - log_z;
            }
        }
        pz_sum += pf_leaf_out(a, ll, pad0, t, wl0, wl1, wl2);
        if (two) pz_sum += pf_leaf_out(a, lr, pad0, t + 1, wr0, wr1, wr2);
    }
}
}  // namespace
