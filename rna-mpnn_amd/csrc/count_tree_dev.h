// The count tree shared by k_design_gc (design_gc.hip), k_design_count (design_count.hip) and, up to the target, k_design_count_profile
// (design_profile.hip): a draw of rnampnn_design conditioned EXACTLY
// on a count that is a sum over the independent units of an RNA - unpaired positions and base pairs - lying in a window.  Position t carries
// a leaf polynomial p_t(d), d = 0..2, in the log domain (a pair's mass sits on its lower index, its upper index carries "1"); node (l, i)
// covers the positions [i 2^l, min((i+1) 2^l, n)) and holds the log-domain convolution of its halves; the root's coefficients over the
// window give the total, and a walk down the tree splits the count of a node between its halves until every leaf knows its own.
// What a position counts is its COUNTED SET, four bits over the classes AUCG: a class in the set counts 1.  The template parameter SETS
// says where the set comes from: false - the constant 12 (C and G) everywhere, rnampnn_design_gc; true - the byte counted[b,t] of the
// call, rnampnn_design_count, which also knows the k_min rule (below).  `cap` bounds every degree: node (l, i) holds the coefficients
// 0 .. min(2 * positions covered, n, cap).  TRUNCATION IS EXACT: c(k) = LSE over a + r = k of L(a) + R(r) reads child coefficients of
// index <= k only, so the coefficients 0..cap of a node are those of the uncapped tree whatever lies above cap; and for k <= cap the
// candidate range max(0, k - deg_R) .. min(k, deg_L) is the same for capped and uncapped child degrees (min(k, min(D, cap)) = min(k, D),
// max(0, k - min(D, cap)) = max(0, k - D) as k - cap <= 0), so every sum runs over the same terms in the same order: the bytes do not
// depend on the cap.  rnampnn_design_gc passes cap = T, which bounds nothing.
// One 256-thread workgroup per (RNA, sample) as in design.hip, the extent / NLL / reduction of score_dev.h; of design_dev.h the mask, the
// fp64 row, the validated partner and the pair cells of a leaf, the logsumexp of its polynomial, the selection rule of its draw, the scratch
// and phase C - nothing about a position under the constraints is defined here.
// Three phases separated by barriers: (A, ct_inside) the tree bottom-up into dynamic LDS - level 1 one node per thread straight from the rows (level 0 is never stored), the levels above dealt flat over (node, coefficient); with SETS the
// smallest reachable count k_min (the sum over the leaves of the smallest d with a finite p_t(d)) is reduced over the workgroup here; (B) the
// window and the target (ct_target), then the walk down, one node per thread and level (one WAVE per node, with a wave-wide scan over the candidates, where a level has at most four
// nodes, and for the total): a node's count is parked in slot 0 of its own coefficients, which nobody reads once its parent has split;
// the last step recomputes the two leaves of a level-1 node, splits and draws them into `sq` (one byte per position, the owner of a pair
// writes both ends); when no count of 0 .. min(n, cap) is reachable (SETS only) the walk is skipped and every leaf draws at its own
// minimum; (C) the rows, the NLL and the counts as k_design writes and reduces them (ds_write_rows, the count as its third sum).
// No workspace, no atomics, no runtime fill / copy node, no host synchronisation; the draw is a pure function of (seed, s, b) and the rows of the RNA.
// The tree has a second home, a caller workspace in global memory (design_long.hip: rnampnn_design_count_long, for RNAs whose tree does not
// fit LDS).  Its kernels build the tree one level per launch and walk it per (RNA, sample) with the per-node counts in LDS; what a leaf, a
// level-1 node (ct_node1), a coefficient (ct_conv, ct_lse_terms), the target, a selection and a leaf's draw ARE is defined here once, so
// the two homes return the same bytes.
#pragma once
#include "design_dev.h"

namespace {
constexpr unsigned long long CT_SALT = RNAMPNN_DESIGN_GC_SALT;
constexpr int CT_MAX_LEVELS = 16;
// the reduction's DS_SCRATCH = 48 bytes (k_min borrows its SC_WAVES ints), at 48 the flag "every leaf at its minimum", at 64 the three
// coefficients of the only leaf of a 1-mer
constexpr size_t CT_LDS_SCRATCH = 96;
static_assert(DS_SCRATCH == 48, "the layout of the count tree's scratch");

struct CtArgs : DesignArgs {
    const uint8_t* counted;      // (B,T); null with SETS = false
    const int32_t* lo;           // (B)
    const int32_t* hi;           // (B)
    int32_t* count;              // (S,B) or null
    int32_t* miss;               // (B) or null
    int cap;                     // 0 .. T
    unsigned base[CT_MAX_LEVELS + 1];    // base[l]: first double of level l (l >= 1)
    unsigned lds_tree, lds_sq;   // bytes of the two LDS arrays
};

using CtPos = DsPos<double>;
// kind: 0 a single position, 1 the lower end of a feasible pair, 2 its upper end; ci, cj: the counted sets of the lower and the upper index
// of a pair (ci: of the position itself when it is single)
struct CtLeaf { CtPos p, pj; int j, kind, m16, ci, cj; };

template <bool SETS>
__device__ __forceinline__ int ct_counted(const CtArgs& a, size_t pad0, int t) { return SETS ? (a.counted[pad0 + t] & 15) : 12; }
// the classes of a position that count d, and the cells (a, b) = 4 a + b of a pair whose ends count d together
__device__ __forceinline__ int ct_classes(int ci, int d) { return d == 0 ? (~ci & 15) : d == 1 ? ci : 0; }
__device__ __forceinline__ int ct_cells(int ci, int cj, int d) {
    int rows = 0, cols = 0;                                         // the cells whose a counts, the cells whose b counts
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        rows |= ((ci >> c) & 1) ? 0xF << (4 * c) : 0;
        cols |= ((cj >> c) & 1) ? 0x1111 << c : 0;
    }
    return (d == 0 ? ~(rows | cols) : d == 1 ? rows ^ cols : d == 2 ? rows & cols : 0) & 0xFFFF;
}
__device__ __forceinline__ double ct_pick(double p0, double p1, double p2, int d) { return d == 0 ? p0 : d == 1 ? p1 : d == 2 ? p2 : -INFINITY; }
__device__ __forceinline__ bool ct_finite(double x) { return fabs(x) < INFINITY; }    // false for NaN
// the smallest d with a finite coefficient, 0 for a leaf with none
__device__ __forceinline__ int ct_min_d(double p0, double p1, double p2) { return ct_finite(p0) ? 0 : ct_finite(p1) ? 1 : ct_finite(p2) ? 2 : 0; }

// Leaf t: what it is and its polynomial (p0, p1, p2).  `bad` counts as k_design counts: an empty mask 1, each end of a pair without an
// admitted compatible cell 1.  Every index is checked before it is used.
template <bool SETS>
__device__ __forceinline__ CtLeaf ct_leaf(const CtArgs& a, size_t pad0, long long row0, int n, int t, double& p0, double& p1, double& p2,
                                          int& bad) {
    CtLeaf lf;
    bool empty, empty_j;
    lf.p = ds_load<double>(a, pad0, row0, t, empty);
    bad += empty ? 1 : 0;
    const int j = ds_partner(a, pad0, n, t);
    lf.j = j; lf.kind = 0; lf.m16 = 0;
    lf.ci = lf.cj = ct_counted<SETS>(a, pad0, t);
    lf.pj = lf.p;
    if (j >= 0) {
        const int mj = ds_mask(a, pad0, j, empty_j);
        const int m = ds_pair_mask(t < j ? lf.p.m : mj, t < j ? mj : lf.p.m, a.wobble);
        if (!m) bad += 1;
        else { lf.kind = t < j ? 1 : 2; lf.m16 = m; }
    }
    if (lf.kind == 2) { p0 = 0.0; p1 = -INFINITY; p2 = -INFINITY; return lf; }
    if (lf.kind == 0) {
        p0 = ds_lse(lf.p.z, lf.p.m & ct_classes(lf.ci, 0)); p1 = ds_lse(lf.p.z, lf.p.m & ct_classes(lf.ci, 1)); p2 = -INFINITY;
        return lf;
    }
    lf.pj = ds_load<double>(a, pad0, row0, j, empty_j);
    lf.cj = ct_counted<SETS>(a, pad0, j);
    double z[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = lf.p.z[c >> 2] + lf.pj.z[c & 3];
    // ds_lse over the cells that count 0, 1 and 2, in ONE pass over the 16 cells: per d the maximum, then the sum of exp(z - that maximum)
    // in cell order - the same operations on the same operands, a third of the exps
    double mx[3] = {-INFINITY, -INFINITY, -INFINITY}, sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int d = ((lf.ci >> (c >> 2)) & 1) + ((lf.cj >> (c & 3)) & 1);
        if ((lf.m16 >> c) & 1) {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (d == e) mx[e] = fmax(mx[e], z[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int d = ((lf.ci >> (c >> 2)) & 1) + ((lf.cj >> (c & 3)) & 1);
        if ((lf.m16 >> c) & 1) {
            const double w = exp(z[c] - (d == 0 ? mx[0] : d == 1 ? mx[1] : mx[2]));
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (d == e) sum[e] += w;
        }
    }
    p0 = mx[0] > -INFINITY ? mx[0] + log(sum[0]) : -INFINITY;
    p1 = mx[1] > -INFINITY ? mx[1] + log(sum[1]) : -INFINITY;
    p2 = mx[2] > -INFINITY ? mx[2] + log(sum[2]) : -INFINITY;
    return lf;
}

// The leaf's draw given its count d, into sq.  A leaf that cannot realise d draws as rnampnn_design would.
__device__ __forceinline__ void ct_leaf_draw(const CtLeaf& lf, int t, int d, unsigned u24, int8_t* sq) {
    if (lf.kind == 2) return;                                       // written by the owner of the pair
    if (lf.kind == 0) {
        CtPos p = lf.p;
        const int md = p.m & ct_classes(lf.ci, d);
        if (md) p.m = md;
        sq[t] = (int8_t)(ds_draw_single(p, u24) & 3);
        return;
    }
    double z[16], w[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = lf.p.z[c >> 2] + lf.pj.z[c & 3];
    const int md = lf.m16 & ct_cells(lf.ci, lf.cj, d), m = md ? md : lf.m16;
    ds_weights(z, m, w);
    const int cell = ds_select(w, m, u24) & 15;
    sq[t] = (int8_t)(cell >> 2);
    sq[lf.j] = (int8_t)(cell & 3);
}

// The family's selection over the candidates i0..i1 with log-weights term(i): weights exp(term - max), the first candidate whose running
// sum exceeds u24 * 2^-24 * total, else the last candidate with a finite log-weight, else the first candidate.
template <typename Term>
__device__ __forceinline__ int ct_select(int i0, int i1, unsigned u24, Term term) {
    double mx = -INFINITY, tot = 0.0;
#pragma unroll 4
    for (int i = i0; i <= i1; ++i) mx = fmax(mx, term(i));
#pragma unroll 4
    for (int i = i0; i <= i1; ++i) tot += exp(term(i) - mx);
    const double u = (double)u24 * (1.0 / 16777216.0) * tot;
    double run = 0.0;
    int last = i0;
    for (int i = i0; i <= i1; ++i) {
        const double x = term(i);
        run += exp(x - mx);
        if (run > u) return i;
        if (ct_finite(x)) last = i;
    }
    return last;
}

// The same selection by ONE WAVE (every lane calls it): the candidates are dealt to the 64 lanes in contiguous chunks, a lane's running sum
// starts at the wave scan of the chunks before it, and the first hit is the smallest over the lanes.  The order of summation differs from
// ct_select's (the contract leaves it free); what is chosen differs only for a uniform within rounding of a cumulative boundary.
template <typename Term>
__device__ __forceinline__ int ct_select_wave(int i0, int i1, unsigned u24, int lane, Term term) {
    const int chunk = (i1 - i0 + 64) >> 6, a = i0 + lane * chunk, b = min(a + chunk - 1, i1);    // a > b: no candidate for this lane
    double mx = -INFINITY, part = 0.0;
    for (int i = a; i <= b; ++i) mx = fmax(mx, term(i));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    for (int i = a; i <= b; ++i) part += exp(term(i) - mx);
    double incl = part;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const double u = (double)u24 * (1.0 / 16777216.0) * __shfl(incl, 63, 64);
    double run = __shfl_up(incl, 1, 64);
    if (lane == 0) run = 0.0;
    int hit = 0x7fffffff, last = -1;
    for (int i = a; i <= b; ++i) {
        const double x = term(i);
        run += exp(x - mx);
        if (hit == 0x7fffffff && run > u) hit = i;
        if (ct_finite(x)) last = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { hit = min(hit, __shfl_xor(hit, o, 64)); last = max(last, __shfl_xor(last, o, 64)); }
    return hit != 0x7fffffff ? hit : last >= 0 ? last : i0;
}

__host__ __device__ __forceinline__ int ct_deg(int l, int i, int n, int cap) { return min(min(2 * (min((i + 1) << l, n) - (i << l)), n), cap); }
__host__ __device__ __forceinline__ int ct_stride(int l, int T, int cap) { return min(min(2 << l, T), cap) + 1; }
__host__ __device__ __forceinline__ int ct_nodes(int l, int n) { return (n + (1 << l) - 1) >> l; }

// LSE over i = i0 .. i1 of term(i), the convolution of the tree: the maximum, then the sum of exp(term - maximum) in index order, -inf
// when no term is above -inf (unrolled by four: the loads and the exps of four terms overlap).
template <typename Term>
__device__ __forceinline__ double ct_lse_terms(int i0, int i1, Term term) {
    double mx = -INFINITY, sum = 0.0;
#pragma unroll 4
    for (int i = i0; i <= i1; ++i) mx = fmax(mx, term(i));
#pragma unroll 4
    for (int i = i0; i <= i1; ++i) sum += exp(term(i) - mx);
    return mx > -INFINITY ? mx + log(sum) : -INFINITY;
}

// The coefficients 0 .. deg of a level-1 node from the polynomials of its two leaves (`two` false: the right leaf is empty and the node is
// its left leaf), into out.  Whoever builds level 1 - ct_inside into LDS, design_long.hip into the workspace - builds it here.
__device__ __forceinline__ void ct_node1(const double (&l)[3], const double (&r)[3], bool two, int deg, double* out) {
#pragma unroll
    for (int k = 0; k <= 4; ++k) {
        double mx = -INFINITY, sum = 0.0;
#pragma unroll
        for (int c = 0; c <= 2; ++c)
            if (c <= k && k - c <= 2) mx = fmax(mx, l[c] + r[k - c]);
#pragma unroll
        for (int c = 0; c <= 2; ++c)
            if (c <= k && k - c <= 2) sum += exp(l[c] + r[k - c] - mx);
        if (k <= deg) out[k] = two ? (mx > -INFINITY ? mx + log(sum) : -INFINITY) : (k <= 2 ? l[k < 2 ? k : 2] : -INFINITY);
    }
}

// Coefficient k <= deg of node (l, i), l >= 2, from `below`, the first double of level l - 1 of the same tree (cstride, cnodes: that
// level's stride and node count): one ct_lse_terms over the halves in index order, or the left half's own when the right half is empty.
__device__ __forceinline__ double ct_conv(const double* below, int l, int i, int k, int n, int cap, int cstride, int cnodes) {
    const double* L = below + (size_t)(2 * i) * cstride;
    const double* R = L + cstride;
    const int degL = ct_deg(l - 1, 2 * i, n, cap);
    if (2 * i + 1 >= cnodes) return k <= degL ? L[k] : -INFINITY;
    const int degR = ct_deg(l - 1, 2 * i + 1, n, cap);
    return ct_lse_terms(max(0, k - degR), min(k, degL), [&](int c) { return L[c] + R[k - c]; });
}

// Phase A of every kernel on the tree: the inside tree of RNA b bottom-up into `tree` - level 1 one node per thread straight from the
// rows, the levels above dealt flat over (node, coefficient) - and on the way `bad` and, SETS only, k_min per wave into s_i (free until
// the sums of the kernel's last phase).  FREE: -> the sum, over the positions this thread loads, of the LSE of z_t over all four classes
// (the count profile's free partition sum); 0 without it.  Every thread calls it; the tree, s_leaf (the only leaf of a 1-mer) and s_i
// are valid on return.
template <bool SETS, bool FREE>
__device__ __forceinline__ double ct_inside(const CtArgs& a, double* tree, double* s_leaf, int* s_i, size_t pad0, long long row0, int n, int tid,
                                            int& bad) {
    const int T = a.T, cap = a.cap;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    int kmin = 0;
    double free_sum = 0.0;
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        const CtLeaf ll = ct_leaf<SETS>(a, pad0, row0, n, t, l0, l1, l2, bad);
        if (FREE) free_sum += ds_lse<4>(ll.p.z, 15);
        if (t + 1 < n) {
            const CtLeaf lr = ct_leaf<SETS>(a, pad0, row0, n, t + 1, r0, r1, r2, bad);
            if (FREE) free_sum += ds_lse<4>(lr.p.z, 15);
        }
        if (SETS) kmin += ct_min_d(l0, l1, l2) + ct_min_d(r0, r1, r2);
        if (n == 1) { s_leaf[0] = l0; s_leaf[1] = l1; s_leaf[2] = l2; break; }
        const double l[3] = {l0, l1, l2}, r[3] = {r0, r1, r2};
        ct_node1(l, r, t + 1 < n, ct_deg(1, i, n, cap), tree + a.base[1] + (size_t)i * ct_stride(1, T, cap));
    }
    if (SETS) {
        kmin = sc_wave_sum(kmin);
        if ((tid & 63) == 0) s_i[tid >> 6] = kmin;
    }
    __syncthreads();
    for (int l = 2; l <= Ln; ++l) {
        const int stride = ct_stride(l, T, cap), cstride = ct_stride(l - 1, T, cap), nodes = ct_nodes(l, n), cnodes = ct_nodes(l - 1, n);
        for (int idx = tid; idx < nodes * stride; idx += SC_THREADS) {
            const int i = idx / stride, k = idx - i * stride;
            if (k > ct_deg(l, i, n, cap)) continue;
            tree[a.base[l] + idx] = ct_conv(tree + a.base[l - 1], l, i, k, n, cap, cstride, cnodes);
        }
        __syncthreads();
    }
    return free_sum;
}

// The window of RNA b clamped to the root's degree, and what the count is conditioned on when the window holds no reachable count: the
// nearest reachable one, or (SETS only) k_min with every leaf at its own minimum.  `root`: the root's coefficients, s_i: k_min per wave
// as ct_inside left it.  any: a count of lo .. hi is reachable - the caller draws K from the window (ct_design) or sums over it (the
// count profile); else K is the target and miss its distance from the window (K = lo, unreachable, under at_min).  Every lane of wave 0
// calls it and gets the same answer: the draw's count_miss and the profile's are one computation.
struct CtTarget { int lo, hi, deg, K, miss; bool any, at_min; };
template <bool SETS>
__device__ __forceinline__ CtTarget ct_target(const CtArgs& a, const double* root, const int* s_i, int b, int n, int Ln) {
    CtTarget g;
    g.deg = Ln ? ct_deg(Ln, 0, n, a.cap) : min(1, a.cap);           // = min(n, cap)
    g.lo = min(max((int)a.lo[b], 0), g.deg);
    g.hi = max(min(max((int)a.hi[b], 0), g.deg), g.lo);
    g.K = g.lo; g.miss = 0;
    g.any = false; g.at_min = false;
    for (int k = g.lo; k <= g.hi; ++k) g.any = g.any || ct_finite(root[k]);
    if (g.any) return g;
    bool found = false;
    for (int d = 1; d <= g.deg && !found; ++d) {                   // the nearest reachable count, the lower one first
        const int kl = g.lo - d, kh = g.hi + d;
        if (kl >= 0 && kl <= g.deg && ct_finite(root[kl])) { g.K = kl; g.miss = d; found = true; }
        else if (kh <= g.deg && ct_finite(root[kh])) { g.K = kh; g.miss = d; found = true; }
    }
    if (SETS && !found) {                                          // nothing in 0 .. min(n, cap): k_min, every leaf at its own minimum
        int km = 0;
#pragma unroll
        for (int w = 0; w < SC_WAVES; ++w) km += s_i[w];
        g.miss = km < g.lo ? g.lo - km : km > g.hi ? km - g.hi : 0;
        g.at_min = true;
    }
    return g;
}

// The body of both kernels; `lds` is the workgroup's dynamic LDS (tree, sq, scratch).
template <bool SETS>
__device__ __forceinline__ void ct_design(const CtArgs& a, unsigned char* lds) {
    double* tree = reinterpret_cast<double*>(lds);
    int8_t* sq = reinterpret_cast<int8_t*>(lds + a.lds_tree);                               // (T)
    const DsScratch sc = ds_scratch(lds + a.lds_tree + a.lds_sq);
    int* const s_i = sc.s_i;
    int* s_min = reinterpret_cast<int*>(lds + a.lds_tree + a.lds_sq + 48);                  // 1: every leaf draws at its own minimum
    double* s_leaf = reinterpret_cast<double*>(lds + a.lds_tree + a.lds_sq + 64);           // 3 doubles
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, T = a.T, cap = a.cap;
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const unsigned long long salted = seed ^ CT_SALT;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;                  // the root is node (Ln, 0)
    int bad = 0;
    // ---- A: the tree, bottom-up
    ct_inside<SETS, false>(a, tree, s_leaf, s_i, pad0, row0, n, tid, bad);
    // ---- B: the total from the root over the window, then the walk down
    if (tid < 64 && n > 0) {                                      // wave 0, every lane with the same window and target
        double* root = Ln ? tree + a.base[Ln] : s_leaf;
        const CtTarget g = ct_target<SETS>(a, root, s_i, b, n, Ln);
        int K = g.K;
        if (g.any) K = ct_select_wave(g.lo, g.hi, ds_u24(salted, s, b, 0), tid, [&](int k) { return root[k]; });
        K = min(K, g.deg);
        if (tid == 0) {
            if (a.miss && s == 0) a.miss[b] = g.miss;
            if (SETS) *s_min = g.at_min ? 1 : 0;
            root[0] = (double)K;
        }
    }
    if (n == 0 && tid == 0 && a.miss && s == 0) a.miss[b] = 0;
    __syncthreads();
    const bool at_min = SETS && n > 0 && *s_min != 0;              // the same in every thread
    for (int l = Ln; l >= 2 && !at_min; --l) {
        const int stride = ct_stride(l, T, cap), cstride = ct_stride(l - 1, T, cap), nodes = ct_nodes(l, n), cnodes = ct_nodes(l - 1, n);
        const bool by_wave = nodes <= SC_WAVES;                    // the top levels: one wave per node, a wave-wide scan over its candidates
        for (int i = by_wave ? (tid >> 6) : tid; i < nodes; i += by_wave ? SC_WAVES : SC_THREADS) {
            const int k = min(max((int)tree[a.base[l] + (size_t)i * stride], 0), ct_deg(l, i, n, cap));
            double* L = tree + a.base[l - 1] + (size_t)(2 * i) * cstride;
            double* R = L + cstride;
            const int degL = ct_deg(l - 1, 2 * i, n, cap);
            int cl = min(k, degL), cr = -1;                        // an empty right half: all of k, no uniform
            if (2 * i + 1 < cnodes) {
                const int degR = ct_deg(l - 1, 2 * i + 1, n, cap), c0 = max(0, k - degR), c1 = min(k, degL);
                const unsigned u24 = ds_u24(salted, s, b, (2 * i + 1) << (l - 1));
                cl = by_wave ? ct_select_wave(c0, c1, u24, tid & 63, [&](int x) { return L[x] + R[k - x]; })
                             : ct_select(c0, c1, u24, [&](int x) { return L[x] + R[k - x]; });
                cr = k - cl;
            }
            if (!by_wave || (tid & 63) == 0) {
                L[0] = (double)cl;
                if (cr >= 0) R[0] = (double)cr;
            }
        }
        __syncthreads();
    }
    int unused_bad = 0;
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        const CtLeaf ll = ct_leaf<SETS>(a, pad0, row0, n, t, l0, l1, l2, unused_bad);
        if (t + 1 >= n) {
            const int k = at_min ? ct_min_d(l0, l1, l2) : n == 1 ? (int)s_leaf[0] : (int)tree[a.base[1] + (size_t)i * ct_stride(1, T, cap)];
            ct_leaf_draw(ll, t, min(max(k, 0), 2), ds_u24(seed, s, b, t), sq);
            break;
        }
        const CtLeaf lr = ct_leaf<SETS>(a, pad0, row0, n, t + 1, r0, r1, r2, unused_bad);
        int c, k;
        if (at_min) {
            c = ct_min_d(l0, l1, l2);
            k = c + ct_min_d(r0, r1, r2);
        } else {
            k = min(max((int)tree[a.base[1] + (size_t)i * ct_stride(1, T, cap)], 0), ct_deg(1, i, n, cap));
            const int c0 = max(0, k - 2), c1 = min(k, 2);
            c = ct_select(c0, c1, ds_u24(salted, s, b, t + 1), [&](int x) { return ct_pick(l0, l1, l2, x) + ct_pick(r0, r1, r2, k - x); });
        }
        ct_leaf_draw(ll, t, c, ds_u24(seed, s, b, t), sq);
        ct_leaf_draw(lr, t + 1, k - c, ds_u24(seed, s, b, t + 1), sq);
    }
    __syncthreads();
    // ---- C: the rows, the NLL and the counts, as k_design walks and reduces them; the count rides as the third sum
    const float cnt = ds_write_rows(a, s, b, n, row0, tid, bad, sc, [&](int t) { return sq[t] & 3; }, [&](int t, int q) {
        return ((ct_counted<SETS>(a, pad0, t) >> q) & 1) ? 1.f : 0.f;  // (whole numbers below 2^24: the float sum is exact)
    });
    if (tid == 0 && a.count) a.count[(size_t)s * a.B + b] = (int)cnt;
}

// doubles of the levels 1..ceil(log2 T): node (l, i) holds min(2 * its extent within T, T, cap) + 1; base[l] (when given) = first double
// of level l
inline size_t ct_tree_doubles(int T, int cap, unsigned* base) {
    size_t total = 0;
    for (int l = 1; l < 31 && (1ll << (l - 1)) < T; ++l) {
        if (base && l <= CT_MAX_LEVELS) base[l] = (unsigned)total;
        const long long size = 1ll << l, nodes = (T + size - 1) / size, tail = T - (nodes - 1) * size, top = std::min<long long>(T, cap);
        total += (size_t)(nodes - 1) * (size_t)(std::min<long long>(2 * size, top) + 1) + (size_t)(std::min<long long>(2 * tail, top) + 1);
    }
    return total;
}
// The count side of an entry that reads the counted sets from the call, in slot 0 of its checks: the two refusals, then the fields -
// the sets, the window, cap = min(count_cap, T) (no node counts more than its positions) and base[] of the tree at that cap, or at
// max(cap, tree_cap_min) where a tree in global memory keeps one entry per node even at cap 0.  An entry without a tree leaves base unread.
inline int ct_count_side(const char* name, const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap, int32_t T,
                         int tree_cap_min, CtArgs& a) {
    if (!counted || !count_lo || !count_hi) return fail(RNAMPNN_ERR_BAD_ARG, "%s: null counted, count_lo or count_hi", name);
    if (count_cap < 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: count_cap = %d is negative", name, (int)count_cap);
    a.counted = counted; a.lo = count_lo; a.hi = count_hi; a.cap = std::min<int>(count_cap, T);
    ct_tree_doubles(T, std::min<int>(std::max<int>(count_cap, tree_cap_min), T), a.base);
    return RNAMPNN_OK;
}
inline size_t ct_lds_bytes(int T, int cap, size_t& tree, size_t& sq) {
    tree = ct_tree_doubles(T, cap, nullptr) * sizeof(double);
    sq = ((size_t)T + 15) & ~(size_t)15;
    return tree + sq + CT_LDS_SCRATCH;
}
// the largest T whose tree fits at that cap (a cap above T is T: the byte count grows with T)
inline int ct_max_T(int cap) {
    size_t tree, sq;
    return (int)ds_max_T([&](long long T) { return ct_lds_bytes((int)T, std::min(cap, (int)T), tree, sq); });
}
}  // namespace
