// rnampnn_design_gc: constrained design with a G+C content window, drawn EXACTLY, in one launch.  The model is one-shot, so under the
// constraints of rnampnn_design the distribution factorises over independent units - unpaired positions and base pairs - and the G+C
// count is a sum over the units.  Conditioning on "count in [lo, hi]" is therefore a product tree of count polynomials: position t carries
// a leaf polynomial p_t(d), d = 0..2, in the log domain (a pair's mass sits on its lower index, its upper index carries "1"); node (l, i)
// covers the positions [i 2^l, min((i+1) 2^l, n)) and holds the log-domain convolution of its halves; the root's coefficients over the
// window give the total, and a walk down the tree splits the count of a node between its halves until every leaf knows its own.  The
// contract is the one include/rnampnn_hip.h documents and tests/_design_gc_ref.py restates; all of the draw is fp64.
// One 256-thread workgroup per (RNA, sample) as in design.hip, the extent / NLL / reduction of score_dev.h, the masks, the pair cells and
// the selection rule of a leaf of design_dev.h.  Three phases separated by barriers: (A) the tree bottom-up into dynamic LDS - level 1 one
// node per thread straight from the rows (level 0 is never stored), the levels above dealt flat over (node, coefficient); (B) the walk
// down, one node per thread and level (one WAVE per node, with a wave-wide scan over the candidates, where a level has at most four
// nodes, and for the total): a node's count is parked in slot 0 of its own coefficients, which nobody reads once its parent has split;
// the last step recomputes the two leaves of a level-1 node, splits and draws them into `sq` (one byte per position, the owner of a pair
// writes both ends); (C) the rows, the NLL and the counts as k_design writes and reduces them.  No workspace, no atomics, no
// runtime fill / copy node, no host synchronisation; the draw is a pure function of (seed, s, b) and the rows of the RNA.
#include "design_dev.h"

namespace {
constexpr unsigned long long GC_SALT = RNAMPNN_DESIGN_GC_SALT;
constexpr int GC_MAX_LEVELS = 16;
constexpr size_t GC_LDS_MAX = 160 * 1024;
constexpr size_t GC_LDS_SCRATCH = 96;    // the reduction's 48 bytes, then (at 64) the three coefficients of the only leaf of a 1-mer

struct GcArgs : DesignArgs {
    const int32_t* gc_lo;        // (B)
    const int32_t* gc_hi;        // (B)
    int32_t* gc_count;           // (S,B) or null
    int32_t* gc_miss;            // (B) or null
    unsigned base[GC_MAX_LEVELS + 1];    // base[l]: first double of level l (l >= 1)
    unsigned lds_tree, lds_sq;   // bytes of the two LDS arrays
};

using GcPos = DsPos<double>;
struct GcLeaf { GcPos p, pj; int j, kind, m16; };    // kind: 0 a single position, 1 the lower end of a feasible pair, 2 its upper end

// cells (a, b) = 4 a + b of a pair by G+C(a) + G+C(b), and the classes of a position by G+C
__device__ __forceinline__ int gc_cells(int d) { return d == 0 ? 0x0033 : d == 1 ? 0x33CC : d == 2 ? 0xCC00 : 0; }
__device__ __forceinline__ int gc_classes(int d) { return d == 0 ? 3 : d == 1 ? 12 : 0; }
__device__ __forceinline__ double gc_pick(double p0, double p1, double p2, int d) { return d == 0 ? p0 : d == 1 ? p1 : d == 2 ? p2 : -INFINITY; }
__device__ __forceinline__ bool gc_finite(double x) { return fabs(x) < INFINITY; }    // false for NaN

__device__ __forceinline__ int gc_mask(const GcArgs& a, size_t pad0, int t, bool& empty) {
    const int m = a.allowed ? (a.allowed[pad0 + t] & 15) : 15;
    empty = m == 0;
    return empty ? 15 : m;
}

__device__ __forceinline__ GcPos gc_load(const GcArgs& a, size_t pad0, long long row0, int t, bool& empty) {
    const float4 x = a.logits[row0 + t];
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bi = a.bias_per_position ? reinterpret_cast<const float4*>(a.bias)[pad0 + t] : make_float4(a.bias[0], a.bias[1], a.bias[2], a.bias[3]);
    const double temp = (double)a.temperature;
    GcPos p;
    p.z[0] = ((double)x.x + (double)bi.x) / temp; p.z[1] = ((double)x.y + (double)bi.y) / temp;
    p.z[2] = ((double)x.z + (double)bi.z) / temp; p.z[3] = ((double)x.w + (double)bi.w) / temp;
    p.m = gc_mask(a, pad0, t, empty);
    return p;
}

// logsumexp of z over the cells m admits: max + log(sum of exp(z - max)) in cell order, -inf when no cell is above -inf
template <int N>
__device__ __forceinline__ double gc_lse(const double (&z)[N], int m) {
    double mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < N; ++c)
        if ((m >> c) & 1) mx = fmax(mx, z[c]);
    if (!(mx > -INFINITY)) return -INFINITY;
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c)
        if ((m >> c) & 1) sum += exp(z[c] - mx);
    return mx + log(sum);
}

// Leaf t: what it is and its polynomial (p0, p1, p2).  `bad` counts as k_design counts: an empty mask 1, each end of a pair without an
// admitted compatible cell 1.  Every index is checked before it is used.
__device__ __forceinline__ GcLeaf gc_leaf(const GcArgs& a, size_t pad0, long long row0, int n, int t, double& p0, double& p1, double& p2,
                                          int& bad) {
    GcLeaf lf;
    bool empty, empty_j;
    lf.p = gc_load(a, pad0, row0, t, empty);
    bad += empty ? 1 : 0;
    int j = a.partner ? a.partner[pad0 + t] : -1;
    if (j < 0 || j >= n || j == t || a.partner[pad0 + j] != t) j = -1;
    lf.j = j; lf.kind = 0; lf.m16 = 0;
    lf.pj = lf.p;
    if (j >= 0) {
        const int mj = gc_mask(a, pad0, j, empty_j);
        const int mlo = t < j ? lf.p.m : mj, mhi = t < j ? mj : lf.p.m;
        int m = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int ca = c >> 2, cb = c & 3;
            const bool ok = ((mlo >> ca) & 1) && ((mhi >> cb) & 1) && ((ds_compat(ca, a.wobble) >> cb) & 1);
            m |= (ok ? 1 : 0) << c;
        }
        if (!m) bad += 1;
        else { lf.kind = t < j ? 1 : 2; lf.m16 = m; }
    }
    if (lf.kind == 2) { p0 = 0.0; p1 = -INFINITY; p2 = -INFINITY; return lf; }
    if (lf.kind == 0) {
        p0 = gc_lse(lf.p.z, lf.p.m & 3); p1 = gc_lse(lf.p.z, lf.p.m & 12); p2 = -INFINITY;
        return lf;
    }
    lf.pj = gc_load(a, pad0, row0, j, empty_j);
    double z[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = lf.p.z[c >> 2] + lf.pj.z[c & 3];
    p0 = gc_lse(z, lf.m16 & 0x0033); p1 = gc_lse(z, lf.m16 & 0x33CC); p2 = gc_lse(z, lf.m16 & 0xCC00);
    return lf;
}

// The leaf's draw given its count d, into sq.  A leaf that cannot realise d draws as rnampnn_design would.
__device__ __forceinline__ void gc_leaf_draw(const GcLeaf& lf, int t, int d, int wobble, unsigned u24, int8_t* sq) {
    if (lf.kind == 2) return;                                       // written by the owner of the pair
    if (lf.kind == 0) {
        GcPos p = lf.p;
        const int md = p.m & gc_classes(d);
        if (md) p.m = md;
        sq[t] = (int8_t)(ds_draw_single(p, u24) & 3);
        return;
    }
    double z[16], w[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = lf.p.z[c >> 2] + lf.pj.z[c & 3];
    const int md = lf.m16 & gc_cells(d), m = md ? md : lf.m16;
    ds_weights(z, m, w);
    const int cell = ds_select(w, m, u24) & 15;
    sq[t] = (int8_t)(cell >> 2);
    sq[lf.j] = (int8_t)(cell & 3);
}

// The family's selection over the candidates i0..i1 with log-weights term(i): weights exp(term - max), the first candidate whose running
// sum exceeds u24 * 2^-24 * total, else the last candidate with a finite log-weight, else the first candidate.
template <typename Term>
__device__ __forceinline__ int gc_select(int i0, int i1, unsigned u24, Term term) {
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
        if (gc_finite(x)) last = i;
    }
    return last;
}

// The same selection by ONE WAVE (every lane calls it): the candidates are dealt to the 64 lanes in contiguous chunks, a lane's running sum
// starts at the wave scan of the chunks before it, and the first hit is the smallest over the lanes.  The order of summation differs from
// gc_select's (the contract leaves it free); what is chosen differs only for a uniform within rounding of a cumulative boundary.
template <typename Term>
__device__ __forceinline__ int gc_select_wave(int i0, int i1, unsigned u24, int lane, Term term) {
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
        if (gc_finite(x)) last = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { hit = min(hit, __shfl_xor(hit, o, 64)); last = max(last, __shfl_xor(last, o, 64)); }
    return hit != 0x7fffffff ? hit : last >= 0 ? last : i0;
}

__device__ __forceinline__ int gc_deg(int l, int i, int n) { return min(2 * (min((i + 1) << l, n) - (i << l)), n); }
__device__ __forceinline__ int gc_stride(int l, int T) { return min(2 << l, T) + 1; }
__device__ __forceinline__ int gc_nodes(int l, int n) { return (n + (1 << l) - 1) >> l; }

__global__ void __launch_bounds__(SC_THREADS) k_design_gc(GcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
    double* tree = reinterpret_cast<double*>(gc_lds);
    int8_t* sq = reinterpret_cast<int8_t*>(gc_lds + a.lds_tree);                               // (T)
    int* s_i = reinterpret_cast<int*>(gc_lds + a.lds_tree + a.lds_sq);                         // SC_WAVES ints
    float (*s_f)[SC_WAVES] = reinterpret_cast<float (*)[SC_WAVES]>(s_i + SC_WAVES);            // 2 x SC_WAVES floats
    double* s_leaf = reinterpret_cast<double*>(gc_lds + a.lds_tree + a.lds_sq + 64);           // 3 doubles
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, T = a.T;
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const unsigned long long salted = seed ^ GC_SALT;
    int n;
    long long row0;
    sc_extent(a, b, tid, s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    const int Ln = n > 1 ? 32 - __clz(n - 1) : 0;                  // the root is node (Ln, 0)
    int bad = 0;
    // ---- A: the tree, bottom-up.  Level 1 from the rows, one node per thread
    for (int i = tid; 2 * i < n; i += SC_THREADS) {
        const int t = 2 * i;
        double l0, l1, l2, r0 = 0.0, r1 = -INFINITY, r2 = -INFINITY;
        gc_leaf(a, pad0, row0, n, t, l0, l1, l2, bad);
        if (t + 1 < n) gc_leaf(a, pad0, row0, n, t + 1, r0, r1, r2, bad);
        if (n == 1) { s_leaf[0] = l0; s_leaf[1] = l1; s_leaf[2] = l2; break; }
        double* out = tree + a.base[1] + (size_t)i * gc_stride(1, T);
        const int deg = gc_deg(1, i, n);
        const double l[3] = {l0, l1, l2}, r[3] = {r0, r1, r2};
#pragma unroll
        for (int k = 0; k <= 4; ++k) {
            double mx = -INFINITY, sum = 0.0;
#pragma unroll
            for (int c = 0; c <= 2; ++c)
                if (c <= k && k - c <= 2) mx = fmax(mx, l[c] + r[k - c]);
#pragma unroll
            for (int c = 0; c <= 2; ++c)
                if (c <= k && k - c <= 2) sum += exp(l[c] + r[k - c] - mx);
            if (k <= deg) out[k] = t + 1 < n ? (mx > -INFINITY ? mx + log(sum) : -INFINITY) : (k <= 2 ? l[k < 2 ? k : 2] : -INFINITY);
        }
    }
    __syncthreads();
    for (int l = 2; l <= Ln; ++l) {
        const int stride = gc_stride(l, T), cstride = gc_stride(l - 1, T), nodes = gc_nodes(l, n), cnodes = gc_nodes(l - 1, n);
        for (int idx = tid; idx < nodes * stride; idx += SC_THREADS) {
            const int i = idx / stride, k = idx - i * stride;
            if (k > gc_deg(l, i, n)) continue;
            const double* L = tree + a.base[l - 1] + (size_t)(2 * i) * cstride;
            const double* R = L + cstride;
            const int degL = gc_deg(l - 1, 2 * i, n);
            double v;
            if (2 * i + 1 < cnodes) {
                const int degR = gc_deg(l - 1, 2 * i + 1, n), c0 = max(0, k - degR), c1 = min(k, degL);
                double mx = -INFINITY, sum = 0.0;
#pragma unroll 4
                for (int c = c0; c <= c1; ++c) mx = fmax(mx, L[c] + R[k - c]);
#pragma unroll 4
                for (int c = c0; c <= c1; ++c) sum += exp(L[c] + R[k - c] - mx);      // (unrolled: the loads and the exps of four terms overlap)
                v = mx > -INFINITY ? mx + log(sum) : -INFINITY;
            } else {
                v = k <= degL ? L[k] : -INFINITY;
            }
            tree[a.base[l] + idx] = v;
        }
        __syncthreads();
    }
    // ---- B: the total from the root over the window, then the walk down
    if (tid < 64 && n > 0) {                                      // wave 0, every lane with the same window and target
        double* root = Ln ? tree + a.base[Ln] : s_leaf;
        const int deg = Ln ? gc_deg(Ln, 0, n) : 1;
        const int lo = min(max((int)a.gc_lo[b], 0), n), hi = max(min(max((int)a.gc_hi[b], 0), n), lo);
        int K = lo, miss = 0;
        bool any = false;
        for (int k = lo; k <= min(hi, deg); ++k) any = any || gc_finite(root[k]);
        if (any) {
            K = gc_select_wave(lo, min(hi, deg), ds_u24(salted, s, b, 0), tid, [&](int k) { return root[k]; });
        } else {
            for (int d = 1; d <= n; ++d) {                             // the nearest reachable count, the lower one first
                const int kl = lo - d, kh = hi + d;
                if (kl >= 0 && kl <= deg && gc_finite(root[kl])) { K = kl; miss = d; break; }
                if (kh <= deg && gc_finite(root[kh])) { K = kh; miss = d; break; }
            }
        }
        K = min(K, deg);
        if (tid == 0) {
            if (a.gc_miss && s == 0) a.gc_miss[b] = miss;
            root[0] = (double)K;
        }
    }
    if (n == 0 && tid == 0 && a.gc_miss && s == 0) a.gc_miss[b] = 0;
    __syncthreads();
    for (int l = Ln; l >= 2; --l) {
        const int stride = gc_stride(l, T), cstride = gc_stride(l - 1, T), nodes = gc_nodes(l, n), cnodes = gc_nodes(l - 1, n);
        const bool by_wave = nodes <= SC_WAVES;                    // the top levels: one wave per node, a wave-wide scan over its candidates
        for (int i = by_wave ? (tid >> 6) : tid; i < nodes; i += by_wave ? SC_WAVES : SC_THREADS) {
            const int k = min(max((int)tree[a.base[l] + (size_t)i * stride], 0), gc_deg(l, i, n));
            double* L = tree + a.base[l - 1] + (size_t)(2 * i) * cstride;
            double* R = L + cstride;
            const int degL = gc_deg(l - 1, 2 * i, n);
            int cl = min(k, degL), cr = -1;                        // an empty right half: all of k, no uniform
            if (2 * i + 1 < cnodes) {
                const int degR = gc_deg(l - 1, 2 * i + 1, n), c0 = max(0, k - degR), c1 = min(k, degL);
                const unsigned u24 = ds_u24(salted, s, b, (2 * i + 1) << (l - 1));
                cl = by_wave ? gc_select_wave(c0, c1, u24, tid & 63, [&](int x) { return L[x] + R[k - x]; })
                             : gc_select(c0, c1, u24, [&](int x) { return L[x] + R[k - x]; });
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
        const GcLeaf ll = gc_leaf(a, pad0, row0, n, t, l0, l1, l2, unused_bad);
        if (t + 1 >= n) {
            const int k = n == 1 ? (int)s_leaf[0] : (int)tree[a.base[1] + (size_t)i * gc_stride(1, T)];
            gc_leaf_draw(ll, t, min(max(k, 0), 2), a.wobble, ds_u24(seed, s, b, t), sq);
            break;
        }
        const GcLeaf lr = gc_leaf(a, pad0, row0, n, t + 1, r0, r1, r2, unused_bad);
        const int k = min(max((int)tree[a.base[1] + (size_t)i * gc_stride(1, T)], 0), gc_deg(1, i, n));
        const int c0 = max(0, k - 2), c1 = min(k, 2);
        const int c = gc_select(c0, c1, ds_u24(salted, s, b, t + 1), [&](int x) { return gc_pick(l0, l1, l2, x) + gc_pick(r0, r1, r2, k - x); });
        gc_leaf_draw(ll, t, c, a.wobble, ds_u24(seed, s, b, t), sq);
        gc_leaf_draw(lr, t + 1, k - c, a.wobble, ds_u24(seed, s, b, t + 1), sq);
    }
    __syncthreads();
    // ---- C: the rows, the NLL and the counts, as k_design walks and reduces them
    int8_t* seq = a.seqs ? a.seqs + ((size_t)s * a.B + b) * T : nullptr;
    float nll = 0.f, gc = 0.f;
    for (int t = tid; t < n; t += SC_THREADS) {
        const int q = sq[t] & 3;
        if (seq) seq[t] = (int8_t)q;
        if (a.seq_nll) nll += sc_row_nll(a.logits[row0 + t], q);
        gc += q >= 2 ? 1.f : 0.f;                                   // (whole numbers below 2^24: the float sum is exact)
    }
    if (seq)
        for (int t = n + tid; t < T; t += SC_THREADS) seq[t] = (int8_t)-1;
    sc_block_sums(bad, nll, gc, tid, s_i, s_f);
    if (tid != 0) return;
    if (a.seq_nll) a.seq_nll[(size_t)s * a.B + b] = nll;
    if (a.gc_count) a.gc_count[(size_t)s * a.B + b] = (int)gc;
    if (a.infeasible && s == 0) a.infeasible[b] = bad;
}

// doubles of the levels 1..ceil(log2 T): node (l, i) holds min(2 * its extent within T, T) + 1; base[l] (when given) = first double of level l
size_t gc_tree_doubles(int T, unsigned* base) {
    size_t total = 0;
    for (int l = 1; l < 31 && (1ll << (l - 1)) < T; ++l) {
        if (base && l <= GC_MAX_LEVELS) base[l] = (unsigned)total;
        const long long size = 1ll << l, nodes = (T + size - 1) / size, tail = T - (nodes - 1) * size;
        total += (size_t)(nodes - 1) * (size_t)(std::min<long long>(2 * size, T) + 1) + (size_t)(std::min<long long>(2 * tail, T) + 1);
    }
    return total;
}
size_t gc_lds_bytes(int T, size_t& tree, size_t& sq) {
    tree = gc_tree_doubles(T, nullptr) * sizeof(double);
    sq = ((size_t)T + 15) & ~(size_t)15;
    return tree + sq + GC_LDS_SCRATCH;
}
int gc_max_T() {
    static const int t_max = [] {
        int T = 1;
        size_t tree, sq;
        while (gc_lds_bytes(T + 1, tree, sq) <= GC_LDS_MAX) ++T;   // (the byte count grows with T)
        return T;
    }();
    return t_max;
}
}  // namespace

extern "C" int rnampnn_design_gc(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                 float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                 const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                                 const int32_t* gc_lo, const int32_t* gc_hi, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                                 int32_t* gc_count, int32_t* gc_miss, void* stream) {
    GcArgs a{};
    const ScDraw draw{S, "RNA", temperature, bias, bias_per_position};
    const int rc = sc_check_args("rnampnn_design_gc", logits, n_rows, mask, cu_seqlens, B, T, &draw, a, [&](int slot) {
        if (slot == 0 && (!gc_lo || !gc_hi)) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design_gc: null gc_lo or gc_hi");
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (!seqs && !seq_nll && !infeasible && !gc_count && !gc_miss) return RNAMPNN_OK;    // nothing asked for
    size_t lds_tree = 0, lds_sq = 0;
    const size_t lds = gc_lds_bytes(T, lds_tree, lds_sq);
    if (lds > GC_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_gc: T = %d needs %zu bytes of LDS for the count tree, the limit is %zu (T <= %d)",
                    (int)T, lds, GC_LDS_MAX, gc_max_T());
    ds_fill(a, seed, seed_dev, allowed, partner, wobble, bias, bias_per_position, temperature, seqs, seq_nll, infeasible);
    a.gc_lo = gc_lo; a.gc_hi = gc_hi; a.gc_count = gc_count; a.gc_miss = gc_miss;
    gc_tree_doubles(T, a.base);
    a.lds_tree = (unsigned)lds_tree; a.lds_sq = (unsigned)lds_sq;
    const int passes = (seqs || seq_nll || gc_count) ? S : 1;   // gc_miss and the count of infeasible positions are those of sample 0
    static DevAttr attr;
    ensure_dyn_lds((const void*)k_design_gc, lds, attr);
    hipLaunchKernelGGL(k_design_gc, dim3(B, passes), dim3(SC_THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
