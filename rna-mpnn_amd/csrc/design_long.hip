// rnampnn_design_count_long / rnampnn_design_count_profile_long: the count tree of count_tree_dev.h in a caller WORKSPACE in global memory,
// for RNAs whose tree does not fit the LDS of one workgroup (a ribosomal RNA under a G+C window).  The leaves, the convolution, the window,
// the target, the selections and the leaf's draw are that header's, so whenever rnampnn_design_count / rnampnn_design_count_profile accept a
// call these entries return its bytes: every coefficient is one ct_lse_terms in index order, whoever computes it.
// The inside tree of RNA b lies at workspace + b * doubles(T, cap) doubles in ct_tree_doubles' layout, [level][node][coefficient]; it is
// built ONCE per RNA and read by all S samples.  Several launches on the one stream, stream order between them:
//   k_ct_long_leaves           level 1 straight from the rows, one node per thread (ct_leaf, ct_node1)
//   k_ct_long_level, l = 2..   level l dealt flat over (node, coefficient), 256 to a workgroup, the RNA in blockIdx.x - the top levels of one long
//                              RNA spread over the device (ct_conv on level l - 1, which the launch before wrote)
//   k_design_count_long        one 256-thread workgroup per (RNA, sample): `bad` and k_min again from the leaves, ct_target on the root read
//                              from the workspace, the walk down with L and R read from the workspace - the counts of the current and the
//                              next level in two LDS int arrays, never in the tree - then the leaves' draws into `sq` and phase C
//                              (ds_write_rows), as ct_design.
//   LDS bytes(T) of the walk = 2 * (4 * ceil(T / 2) rounded up to 16) + T rounded up to 16 + 96: it grows with T, not with the tree.
// The profile: the same level launches, then
//   k_pf_long_root             one workgroup per RNA: k_min from the leaves, then pf_ct_root - the root's outside into the second tree, which
//                              lies at workspace + (B + b) * doubles(T, cap) doubles in the same layout
//   k_pf_long_outside, l = ..2 level l hands its children their outsides, dealt flat over (child node, coefficient) (pf_outside)
//   k_pf_long_leaves           one workgroup per RNA: `bad`, k_min and the free sum from the leaves, pf_ct_root again for (at_min, count_miss,
//                              log_z) - the workspace has no room for them, and wave 0 has them from the root in microseconds - then phases D
//                              and E of k_design_count_profile with O read from the workspace (pf_ct_leaves, pf_finish).  Under the k_min rule
//                              the outside launches still run; what they wrote is not read.
// No atomics, no runtime fill / copy node, no host synchronisation; the workspace's contents before the call do not matter.
#include "profile_dev.h"

namespace {
struct CtLongArgs : CtArgs {
    double* ws;                  // the caller's workspace
    size_t per_rna;              // doubles(T, cap): the doubles of one tree
    unsigned lds_cnt;            // bytes of ONE of the walk's two count arrays
};

__device__ __forceinline__ double* ctl_tree(const CtLongArgs& a, int b) { return a.ws + (size_t)b * a.per_rna; }

// Level 1: node i = blockIdx.y * 256 + tid of RNA blockIdx.x from its two leaves.  A 1-mer has no level 1.
__global__ void __launch_bounds__(SC_THREADS) k_ct_long_leaves(CtLongArgs a) {
    __shared__ float s_tmp[SC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T, cap = a.cap;
    int n;
    long long row0;
    sc_extent(a, b, tid, s_tmp, n, row0);
    const int i = blockIdx.y * SC_THREADS + tid, t = 2 * i;
    if (n < 2 || t >= n) return;
    const size_t pad0 = (size_t)b * T;
    int unused_bad = 0;
    double l[3], r[3] = {0.0, -INFINITY, -INFINITY};
    ct_leaf<true>(a, pad0, row0, n, t, l[0], l[1], l[2], unused_bad);
    const bool two = t + 1 < n;
    if (two) ct_leaf<true>(a, pad0, row0, n, t + 1, r[0], r[1], r[2], unused_bad);
    ct_node1(l, r, two, ct_deg(1, i, n, cap), ctl_tree(a, b) + a.base[1] + (size_t)i * ct_stride(1, T, cap));
}

// Level l >= 2: coefficient idx = blockIdx.y * 256 + tid of the level's flat (node, coefficient) array of RNA blockIdx.x.
__global__ void __launch_bounds__(SC_THREADS) k_ct_long_level(CtLongArgs a, int l) {
    __shared__ float s_tmp[SC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T, cap = a.cap;
    int n;
    long long row0;
    sc_extent(a, b, tid, s_tmp, n, row0);
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    if (l > Ln) return;                                            // this RNA's tree ends below level l
    const int stride = ct_stride(l, T, cap), cstride = ct_stride(l - 1, T, cap), nodes = ct_nodes(l, n), cnodes = ct_nodes(l - 1, n);
    const int idx = blockIdx.y * SC_THREADS + tid;
    if (idx >= nodes * stride) return;
    const int i = idx / stride, k = idx - i * stride;
    if (k > ct_deg(l, i, n, cap)) return;
    double* tree = ctl_tree(a, b);
    tree[a.base[l] + idx] = ct_conv(tree + a.base[l - 1], l, i, k, n, cap, cstride, cnodes);
}

// What is left of phase A once the tree is in the workspace: `bad`, k_min per wave into s_i, the only leaf of a 1-mer into s_leaf and,
// with FREE, -> this thread's share of the free sum, over the leaves in ct_inside's order.  Every thread calls it (one barrier).
template <bool FREE>
__device__ __forceinline__ double ctl_leaf_sums(const CtArgs& a, double* s_leaf, int* s_i, size_t pad0, long long row0, int n, int tid, int& bad) {
    int kmin = 0;
    double free_sum = 0.0;
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        const CtLeaf ll = ct_leaf<true>(a, pad0, row0, n, t, l0, l1, l2, bad);
        if (FREE) free_sum += ds_lse<4>(ll.p.z, 15);
        if (t + 1 < n) {
            const CtLeaf lr = ct_leaf<true>(a, pad0, row0, n, t + 1, r0, r1, r2, bad);
            if (FREE) free_sum += ds_lse<4>(lr.p.z, 15);
        }
        kmin += ct_min_d(l0, l1, l2) + ct_min_d(r0, r1, r2);
        if (n == 1) { s_leaf[0] = l0; s_leaf[1] = l1; s_leaf[2] = l2; }
    }
    kmin = sc_wave_sum(kmin);
    if ((tid & 63) == 0) s_i[tid >> 6] = kmin;
    __syncthreads();
    return free_sum;
}

constexpr int CTL_MAX_T = 1 << CT_MAX_LEVELS;  // the levels the argument block addresses
constexpr size_t CTL_ALIGN = 15;
inline size_t ctl_lds_bytes(long long T, size_t& cnt, size_t& sq) {
    cnt = (4 * (((size_t)T + 1) / 2) + CTL_ALIGN) & ~CTL_ALIGN;
    sq = ((size_t)T + CTL_ALIGN) & ~CTL_ALIGN;
    return 2 * cnt + sq + CT_LDS_SCRATCH;
}

// Three workgroups per CU, as k_design_count and for its reason: the walk is latency-bound.
__global__ void __launch_bounds__(SC_THREADS, 3) k_design_count_long(CtLongArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ctl_lds[];
    int* cur = reinterpret_cast<int*>(ctl_lds);                                             // the counts of the level being split
    int* nxt = reinterpret_cast<int*>(ctl_lds + a.lds_cnt);                                 // the counts of the level below it
    int8_t* sq = reinterpret_cast<int8_t*>(ctl_lds + 2 * (size_t)a.lds_cnt);                // (T)
    unsigned char* scr = ctl_lds + 2 * (size_t)a.lds_cnt + a.lds_sq;
    const DsScratch sc = ds_scratch(scr);
    int* const s_i = sc.s_i;
    int* s_min = reinterpret_cast<int*>(scr + 48);                                          // 1: every leaf draws at its own minimum
    double* s_leaf = reinterpret_cast<double*>(scr + 64);                                   // 3 doubles
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, T = a.T, cap = a.cap;
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const unsigned long long salted = seed ^ CT_SALT;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    const double* tree = ctl_tree(a, b);
    // ---- A: `bad` and k_min from the leaves (the tree is in the workspace already)
    int bad = 0;
    ctl_leaf_sums<false>(a, s_leaf, s_i, pad0, row0, n, tid, bad);
    // ---- B: the total from the root over the window, then the walk down
    if (tid < 64 && n > 0) {
        const double* root = Ln ? tree + a.base[Ln] : s_leaf;
        const CtTarget g = ct_target<true>(a, root, s_i, b, n, Ln);
        int K = g.K;
        if (g.any) K = ct_select_wave(g.lo, g.hi, ds_u24(salted, s, b, 0), tid, [&](int k) { return root[k]; });
        K = min(K, g.deg);
        if (tid == 0) {
            if (a.miss && s == 0) a.miss[b] = g.miss;
            *s_min = g.at_min ? 1 : 0;
            cur[0] = K;
        }
    }
    if (n == 0 && tid == 0 && a.miss && s == 0) a.miss[b] = 0;
    __syncthreads();
    const bool at_min = n > 0 && *s_min != 0;                      // the same in every thread
    for (int l = Ln; l >= 2 && !at_min; --l) {
        const int cstride = ct_stride(l - 1, T, cap), nodes = ct_nodes(l, n), cnodes = ct_nodes(l - 1, n);
        const bool by_wave = nodes <= SC_WAVES;                    // ct_design's rule
        for (int i = by_wave ? (tid >> 6) : tid; i < nodes; i += by_wave ? SC_WAVES : SC_THREADS) {
            const int k = min(max(cur[i], 0), ct_deg(l, i, n, cap));
            const double* L = tree + a.base[l - 1] + (size_t)(2 * i) * cstride;
            const double* R = L + cstride;
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
                nxt[2 * i] = cl;
                if (cr >= 0) nxt[2 * i + 1] = cr;
            }
        }
        __syncthreads();
        int* const swap = cur; cur = nxt; nxt = swap;
    }
    int unused_bad = 0;
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        const CtLeaf ll = ct_leaf<true>(a, pad0, row0, n, t, l0, l1, l2, unused_bad);
        if (t + 1 >= n) {
            const int k = at_min ? ct_min_d(l0, l1, l2) : cur[i];
            ct_leaf_draw(ll, t, min(max(k, 0), 2), ds_u24(seed, s, b, t), sq);
            break;
        }
        const CtLeaf lr = ct_leaf<true>(a, pad0, row0, n, t + 1, r0, r1, r2, unused_bad);
        int c, k;
        if (at_min) {
            c = ct_min_d(l0, l1, l2);
            k = c + ct_min_d(r0, r1, r2);
        } else {
            k = min(max(cur[i], 0), ct_deg(1, i, n, cap));
            const int c0 = max(0, k - 2), c1 = min(k, 2);
            c = ct_select(c0, c1, ds_u24(salted, s, b, t + 1), [&](int x) { return ct_pick(l0, l1, l2, x) + ct_pick(r0, r1, r2, k - x); });
        }
        ct_leaf_draw(ll, t, c, ds_u24(seed, s, b, t), sq);
        ct_leaf_draw(lr, t + 1, k - c, ds_u24(seed, s, b, t + 1), sq);
    }
    __syncthreads();
    // ---- C: the rows, the NLL and the counts, as ct_design
    const float cnt = ds_write_rows(a, s, b, n, row0, tid, bad, sc, [&](int t) { return sq[t] & 3; }, [&](int t, int q) {
        return ((ct_counted<true>(a, pad0, t) >> q) & 1) ? 1.f : 0.f;
    });
    if (tid == 0 && a.count) a.count[(size_t)s * a.B + b] = (int)cnt;
}

// the doubles of one tree as the entries lay it out: count_cap = 0 (nothing may count) is stored at the extents of cap 1, so that the
// workspace functions, which return 0 for an argument <= 0, still size it
inline size_t ctl_doubles(int T, int count_cap) { return ct_tree_doubles(T, std::min<int>(std::max<int>(count_cap, 1), T), nullptr); }

// What both entries check about the workspace (slot 1 of ds_prepare) -> RNAMPNN_OK or what fail() returned.
int ctl_check_workspace(const char* name, const char* what, const void* workspace, size_t workspace_bytes, size_t need, int B, int T, int count_cap) {
    if (!workspace || workspace_bytes < need)
        return fail(RNAMPNN_ERR_BAD_ARG, "%s: the workspace is %s (%zu bytes), %s at (B = %d, T = %d, count_cap = %d) needs %zu (%s_workspace_bytes)",
                    name, workspace ? "too small" : "null", workspace_bytes, what, B, T, count_cap, need, name);
    if (((uintptr_t)workspace & 7) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "%s: the workspace must be 8-byte aligned", name);
    return RNAMPNN_OK;
}

// The inside pass of both entries: level 1, then one launch per level.  (B, blocks): the RNA in x, so B is not bound by the 65,535 of y;
// a level has at most 2.5 T entries, 320 workgroups at the largest T.
int ctl_inside(const CtLongArgs& a, void* stream) {
    const int B = a.B, T = a.T;
    if (T < 2) return RNAMPNN_OK;
    hipLaunchKernelGGL(k_ct_long_leaves, dim3(B, (ct_nodes(1, T) + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    for (int l = 2; (1 << (l - 1)) < T; ++l) {
        const int entries = ct_nodes(l, T) * ct_stride(l, T, a.cap);
        hipLaunchKernelGGL(k_ct_long_level, dim3(B, (entries + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, (hipStream_t)stream, a, l);
        HIP_TRY(hipGetLastError());
    }
    return RNAMPNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the profile
struct PfLongArgs : PfCtArgs {
    double* ws;
    size_t per_rna;
};
__device__ __forceinline__ double* pfl_inside(const PfLongArgs& a, int b) { return a.ws + (size_t)b * a.per_rna; }
__device__ __forceinline__ double* pfl_outside(const PfLongArgs& a, int b) { return a.ws + ((size_t)a.B + b) * a.per_rna; }

__global__ void __launch_bounds__(SC_THREADS) k_pf_long_root(PfLongArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char scr[PF_CT_SCRATCH];
    const PfCtScratch ps = pf_ct_scratch(scr);
    const int b = blockIdx.x, tid = threadIdx.x;
    int n;
    long long row0;
    sc_extent(a, b, tid, ps.sc.s_f[0], n, row0);
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    if (Ln == 0) return;                                           // no tree in the workspace: the leaf kernel holds the 1-mer's outside in LDS
    int unused_bad = 0;
    ctl_leaf_sums<false>(a, ps.s_leaf, ps.sc.s_i, (size_t)b * a.T, row0, n, tid, unused_bad);
    if (tid < 64) pf_ct_root(a, pfl_inside(a, b) + a.base[Ln], pfl_outside(a, b) + a.base[Ln], ps.sc.s_i, b, n, Ln, tid, ps.s_flag, ps.s_logz);
}

// Level l >= 2 hands level l - 1 its outsides: coefficient idx = blockIdx.y * 256 + tid of the flat (child node, coefficient) array.
__global__ void __launch_bounds__(SC_THREADS) k_pf_long_outside(PfLongArgs a, int l) {
    __shared__ float s_tmp[SC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T, cap = a.cap;
    int n;
    long long row0;
    sc_extent(a, b, tid, s_tmp, n, row0);
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    if (l > Ln) return;
    const int stride = ct_stride(l, T, cap), cstride = ct_stride(l - 1, T, cap), cnodes = ct_nodes(l - 1, n);
    const int idx = blockIdx.y * SC_THREADS + tid;
    if (idx >= cnodes * cstride) return;
    const int j = idx / cstride, c = idx - j * cstride;
    if (c > ct_deg(l - 1, j, n, cap)) return;
    double* outs = pfl_outside(a, b);
    outs[a.base[l - 1] + idx] = pf_outside(outs + a.base[l], pfl_inside(a, b) + a.base[l - 1], l, j, c, n, cap, stride, cstride, cnodes);
}

__global__ void __launch_bounds__(SC_THREADS) k_pf_long_leaves(PfLongArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char scr[PF_CT_SCRATCH];
    const PfCtScratch ps = pf_ct_scratch(scr);
    const DsScratch sc = ps.sc;
    const int b = blockIdx.x, tid = threadIdx.x;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * a.T;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;
    int bad = 0;
    double free_sum = ctl_leaf_sums<true>(a, ps.s_leaf, sc.s_i, pad0, row0, n, tid, bad);
    if (tid < 64 && n > 0)
        pf_ct_root(a, Ln ? pfl_inside(a, b) + a.base[Ln] : ps.s_leaf, Ln ? nullptr : ps.o_leaf, sc.s_i, b, n, Ln, tid, ps.s_flag, ps.s_logz);
    __syncthreads();
    const bool at_min = n > 0 && ps.s_flag[0] != 0;                // the same in every thread
    const int miss = n > 0 ? ps.s_flag[1] : 0;
    const double log_z = n > 0 ? *ps.s_logz : 0.0;
    double pz_sum = 0.0, lz_sum = 0.0;
    pf_ct_leaves(a, pfl_outside(a, b) + a.base[1], ps.o_leaf, pad0, row0, n, tid, at_min, log_z, pz_sum, lz_sum);
    pf_finish(a.out, a, a.miss, miss, b, n, tid, bad, free_sum, pz_sum, lz_sum, at_min, log_z, sc, ps.s_d);
}
}  // namespace

extern "C" size_t rnampnn_design_count_long_workspace_bytes(int32_t B, int32_t T, int32_t count_cap) {
    if (B <= 0 || T <= 0 || count_cap <= 0) return 0;
    return (size_t)B * sizeof(double) * ctl_doubles(T, count_cap);
}

extern "C" int rnampnn_design_count_long(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                         float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                         const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                         const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap,
                                         void* workspace, size_t workspace_bytes, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                                         int32_t* count, int32_t* count_miss, void* stream) {
    const char* name = "rnampnn_design_count_long";
    CtLongArgs a{};
    const int rc = ds_prepare(name, "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed, partner, wobble, bias,
                              bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0) return ct_count_side(name, counted, count_lo, count_hi, count_cap, T, 1, a);
        if (slot == 1)
            return ctl_check_workspace(name, "the count tree", workspace, workspace_bytes,
                                       rnampnn_design_count_long_workspace_bytes(B, T, std::max<int>(count_cap, 1)), B, T, count_cap);
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible && !count && !count_miss) return RNAMPNN_OK;    // nothing asked for
    size_t lds_cnt = 0, lds_sq = 0;
    const size_t lds = ctl_lds_bytes(T, lds_cnt, lds_sq);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d needs %zu bytes of LDS for the counts of two levels and the draw, the limit is %zu "
                    "(T <= %lld; the count tree is in the workspace and does not count)", name, (int)T, lds, DS_LDS_MAX,
                    ds_max_T([](long long t) { size_t c, q; return ctl_lds_bytes(t, c, q); }));
    a.count = count; a.miss = count_miss;
    a.ws = reinterpret_cast<double*>(workspace); a.per_rna = ctl_doubles(T, count_cap);
    a.lds_tree = 0; a.lds_sq = (unsigned)lds_sq; a.lds_cnt = (unsigned)lds_cnt;
    if (const int rl = ctl_inside(a, stream)) return rl;
    const int passes = (seqs || seq_nll || count) ? S : 1;      // count_miss and the count of infeasible positions are those of sample 0
    return ds_launch<k_design_count_long>(dim3(B, passes), lds, stream, a);
}

extern "C" size_t rnampnn_design_count_profile_long_workspace_bytes(int32_t B, int32_t T, int32_t count_cap) {
    return 2 * rnampnn_design_count_long_workspace_bytes(B, T, count_cap);
}

extern "C" int rnampnn_design_count_profile_long(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B,
                                                 int32_t T, float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble,
                                                 const float* bias, int32_t bias_per_position, const uint8_t* counted, const int32_t* count_lo,
                                                 const int32_t* count_hi, int32_t count_cap, void* workspace, size_t workspace_bytes,
                                                 double* marginals, double* log_z, double* log_z_free, double* entropy, int32_t* infeasible,
                                                 int32_t* count_miss, void* stream) {
    const char* name = "rnampnn_design_count_profile_long";
    const PfAsked asked{name, marginals, log_z, log_z_free, entropy, infeasible, count_miss};
    PfLongArgs a{};
    const int rc = ds_prepare(name, "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, 1, 0, nullptr, allowed, partner, wobble, bias,
                              bias_per_position, nullptr, nullptr, infeasible, a, [&](int slot) {
        if (slot == 0) return ct_count_side(name, counted, count_lo, count_hi, count_cap, T, 1, a);
        if (const int ra = asked.aligned()) return ra;
        if (slot == 1)
            return ctl_check_workspace(name, "the inside and the outside tree", workspace, workspace_bytes,
                                       rnampnn_design_count_profile_long_workspace_bytes(B, T, std::max<int>(count_cap, 1)), B, T, count_cap);
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (asked.nothing()) return RNAMPNN_OK;
    if (T > CTL_MAX_T)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "%s: T = %d lies above %d, the largest T whose tree the %d levels of the argument block address",
                    name, (int)T, CTL_MAX_T, CT_MAX_LEVELS);
    a.count = nullptr; a.miss = count_miss;
    a.ws = reinterpret_cast<double*>(workspace); a.per_rna = ctl_doubles(T, count_cap);
    a.out = asked.out();
    CtLongArgs in{};
    static_cast<CtArgs&>(in) = a;
    in.ws = a.ws; in.per_rna = a.per_rna;
    if (const int rl = ctl_inside(in, stream)) return rl;
    if (T >= 2) {
        hipLaunchKernelGGL(k_pf_long_root, dim3(B), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        int top = 1;
        while ((1 << top) < T) ++top;                                // the root level of an RNA of T positions
        for (int l = top; l >= 2; --l) {
            const int entries = ct_nodes(l - 1, T) * ct_stride(l - 1, T, a.cap);
            hipLaunchKernelGGL(k_pf_long_outside, dim3(B, (entries + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, (hipStream_t)stream, a, l);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_pf_long_leaves, dim3(B), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
