// Fitting the gradient-boosted-tree read-out on the device: a histogram-method trainer for `multi:softmax` that
// writes its trees in the record layout k_gbdt_predict (gbdt.hip) walks.  PARITY UNPINNED, as the evaluator: what is restated is XGBoost's
// published objective (softmax gradient / hessian), split gain and leaf weight; the cuts, the binning and the sampling are this project's
// own (DESIGN section 9 states them; tests/_gbdt_fit_ref.py restates them in numpy).
//
// Exactness: gradients are quantised onto the grid 2^-20 and every histogram entry is an INTEGER sum (64-bit LDS and global integer
// atomics), so a histogram does not depend on arrival order, on the launch geometry or on the order of the rows inside a node's segment;
// the split search is fp64 with contraction OFF; leaves are fp64 rounded once to f32.  There is no float atomic in this file.
//
// A tree grows as a complete heap in device memory (node n has children 2n+1, 2n+2) with no host round trip: launch extents that depend
// on a row count are taken at their upper bound (n_rows) and the kernels read the real count on the device.  The sampled rows are kept
// GROUPED PER NODE (perm / pnode, segment start and length per heap node; the order inside a segment is arbitrary, which integer sums
// allow), so a histogram workgroup serves one node's segment at a time.  k_compact renumbers the heap breadth-first into the model.
#include "../../include/rnampnn_hip.h"
#include "rnampnn_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int GB_BINS = 256;          // bins per feature (a bin is one byte)
constexpr int GB_CUTS = 255;          // row stride of the cuts matrix
constexpr int GB_FT = 8;              // features per histogram tile: 8 x 257 x (g, h) x 8 B = 32.1 KB of LDS
constexpr int GB_HS = 257;            // padded bin stride of the LDS tile (features fall on different banks for one bin)
constexpr int GB_UNROLL = 4;          // rows a histogram thread loads before it adds (the loop is latency-bound otherwise)
constexpr int GB_LDS_MIN = 128;       // a piece of a node's segment shorter than this adds straight to global memory
constexpr int GB_MAX_DEPTH = 10;      // level D - 1 holds 2^(D-1) <= 512 histogram nodes; k_level_scan / k_compact use one 1024-thread workgroup
constexpr double GB_SCALE = 1048576.0;            // gradients live on the grid 2^-20
constexpr double GB_INV_SCALE = 1.0 / 1048576.0;
constexpr double GB_MIN_GAIN = 1e-6;              // XGBoost's kRtEps

typedef unsigned long long u64;
typedef long long i64;

// u(seed, a, b): splitmix64 finaliser of one counter, 24 bits -> [0, 1).  Rows of round r use a = 2r, features of tree t use a = 2t + 1.
__host__ __device__ inline double gb_hash_u(uint64_t seed, uint64_t a, uint64_t b) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((a << 32) + b + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 40) * (1.0 / 16777216.0);
}

// ------------------------------------------------------------------------------------------------ binning
// bin(x) = number of cuts <= x (binary search in the feature's ascending cuts); a non-finite x raises *flag
__global__ void __launch_bounds__(256) k_bin(const float* __restrict__ X, int n_rows, int ldx, int F, const float* __restrict__ cuts,
                                             const int* __restrict__ ncuts, unsigned char* __restrict__ bins, int* __restrict__ flag) {
    const size_t total = (size_t)n_rows * F;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int row = (int)(e / F), f = (int)(e - (size_t)row * F);
        const float x = X[(size_t)row * ldx + f];
        if (flag && !(fabsf(x) <= 3.402823466e38f)) *flag = 1;
        const float* c = cuts + (size_t)f * GB_CUTS;
        int lo = 0, hi = min(max(ncuts[f], 0), GB_CUTS);            // first index with c[i] > x
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] <= x) lo = mid + 1; else hi = mid;
        }
        bins[e] = (unsigned char)lo;
    }
}
__global__ void __launch_bounds__(256) k_check_labels(const int* __restrict__ y, int n, int C, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && (y[i] < 0 || y[i] >= C)) *flag = 2;
}
__global__ void __launch_bounds__(256) k_fill_f32(float* __restrict__ p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

// ------------------------------------------------------------------------------------------------ gradients
// softmax of the row's margins in fp64 (row maximum subtracted, sum in class order), g = p - [y == c], h = max(2 p (1 - p), 1e-16),
// both rounded to nearest (ties to even) onto the grid 2^-20; g, h are (C, n) so a tree reads one contiguous plane
__global__ void __launch_bounds__(256) k_grad(const float* __restrict__ margin, const int* __restrict__ y, int n, int C,
                                              int* __restrict__ g, int* __restrict__ h) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* m = margin + (size_t)i * C;
    double mx = (double)m[0];
    for (int c = 1; c < C; ++c) mx = fmax(mx, (double)m[c]);
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += exp((double)m[c] - mx);
    const int yi = y[i];
    for (int c = 0; c < C; ++c) {
        const double p = exp((double)m[c] - mx) / s;
        const double gd = p - (c == yi ? 1.0 : 0.0);
        const double hd = fmax(2.0 * p * (1.0 - p), 1e-16);
        g[(size_t)c * n + i] = (int)rint(gd * GB_SCALE);
        h[(size_t)c * n + i] = (int)rint(hd * GB_SCALE);
    }
}

// ------------------------------------------------------------------------------------------------ sampling
__global__ void __launch_bounds__(256) k_row_mask(unsigned char* __restrict__ mask, int n, uint64_t seed, uint64_t round, double subsample) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[i] = (subsample >= 1.0 || gb_hash_u(seed, 2 * round, (uint64_t)i) < subsample) ? 1 : 0;
}

// One atomic per wave and key: the lanes of a wave that hold the same key share one add of their count; returns the slot of an active
// lane (base + its rank among the lanes of its key), -1 for an inactive one.  Every lane of the wave must call it.
__device__ inline int gb_wave_slots(int* __restrict__ counters, int key, bool active) {
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(active);
    int res = -1;
    while (todo) {
        const int leader = __ffsll((i64)todo) - 1;
        const int k = __shfl(key, leader);
        const bool mine = active && key == k;
        const u64 m = __ballot(mine);
        int base = 0;
        if (lane == leader) base = atomicAdd(&counters[k], __popcll(m));
        base = __shfl(base, leader);
        if (mine) res = base + __popcll(m & ((1ull << lane) - 1ull));
        todo &= ~m;
    }
    return res;
}

// rows of the round's sample -> perm0 (any order), all at the root; *n0 counts them (zeroed by the caller)
__global__ void __launch_bounds__(256) k_init_perm(const unsigned char* __restrict__ mask, int n, int* __restrict__ perm0, int* __restrict__ n0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && (!mask || mask[i]);
    const int slot = gb_wave_slots(n0, 0, on);
    if (on) perm0[slot] = i;
}
// the sampled features in ascending order (ties in the split search go to the lowest feature index)
__global__ void __launch_bounds__(64) k_feature_list(const unsigned char* __restrict__ fmask, int F, int* __restrict__ flist, int* __restrict__ nfs) {
    const int lane = threadIdx.x;                                   // one wave, 64 features per step
    int n = 0;
    for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane;
        const bool on = f < F && (!fmask || fmask[f]);
        const u64 m = __ballot(on);
        if (on) flist[n + __popcll(m & ((1ull << lane) - 1ull))] = f;
        n += __popcll(m);
    }
    if (lane == 0) *nfs = n;
}

// ------------------------------------------------------------------------------------------------ one tree: heap state
struct GrowHeap {            // per-tree arrays indexed by heap node (all zeroed at the start of a tree, one launch)
    int* state;              // 0 absent, 1 leaf, 2 split
    int* feat;               // split feature
    int* cutj;               // split cut: bin <= cutj goes left
    float* cond;             // cuts[feat][cutj] of a split, the value of a leaf
    int* seg_start;          // the node's segment of perm
    int* seg_cnt;
    int* cursor;             // running write position of the scatter
    i64* nodeG;              // integer totals handed down by the parent's split (used at the last level, which has no histogram)
    i64* nodeH;
    int* level_n;            // [GB_MAX_DEPTH + 1] rows still grouped at each level
};

__global__ void k_tree_begin(GrowHeap hp, const int* __restrict__ n0) {
    if (blockIdx.x || threadIdx.x) return;
    hp.seg_cnt[0] = *n0;
    hp.level_n[0] = *n0;
}

// ------------------------------------------------------------------------------------------------ histograms (the hot path)
// grid (row chunks of R positions, feature tiles of GB_FT).  A chunk is cut into the pieces that lie in one node's segment; a piece is
// summed in an LDS tile [feature][bin]{g, h} with 64-bit integer LDS atomics and flushed once (non-zero entries only) with 64-bit
// integer global atomics; a piece shorter than GB_LDS_MIN rows (deep levels: most entries would be written once) adds to global memory
// directly.  Thread t serves feature (t & 7) of the tile for rows (t >> 3), (t >> 3) + 32, ...
__global__ void __launch_bounds__(256) k_hist(const unsigned char* __restrict__ bins, int F, const int* __restrict__ g, const int* __restrict__ h,
        const int* __restrict__ perm, const int* __restrict__ pnode, const int* __restrict__ n_cur_ptr, const int* __restrict__ seg_start,
        const int* __restrict__ seg_cnt, const int* __restrict__ flist, const int* __restrict__ nfs_ptr, int level_base, int R,
        u64* __restrict__ hist) {
    __shared__ u64 sh[GB_FT * GB_HS * 2];
    const int t = threadIdx.x, fl = t & (GB_FT - 1), rsub = t >> 3;
    const int nfs = *nfs_ptr, tile0 = blockIdx.y * GB_FT;
    if (tile0 >= nfs) return;
    const int n_cur = *n_cur_ptr;
    const long long p0 = (long long)blockIdx.x * R;
    if (p0 >= n_cur) return;
    const int p1 = (int)min((long long)n_cur, p0 + R);
    const bool fvalid = tile0 + fl < nfs;
    const int f = fvalid ? flist[tile0 + fl] : 0;
    int p = (int)p0;
    while (p < p1) {
        const int node = pnode ? pnode[p] : 0;
        const int end = min(p1, seg_start[node] + seg_cnt[node]);
        if (end <= p) break;                                        // cannot happen with consistent segments; never spin
        u64* hn = hist + (size_t)(node - level_base) * F * (GB_BINS * 2);
        if (end - p >= GB_LDS_MIN) {
            for (int e = t; e < GB_FT * GB_HS * 2; e += 256) sh[e] = 0;
            __syncthreads();
            if (fvalid)
                for (int q = p + rsub; q < end; q += 32 * GB_UNROLL) {      // GB_UNROLL independent load chains in flight per thread
                    int row[GB_UNROLL], b[GB_UNROLL], gv[GB_UNROLL], hv[GB_UNROLL];
#pragma unroll
                    for (int k = 0; k < GB_UNROLL; ++k) row[k] = perm[min(q + 32 * k, end - 1)];
#pragma unroll
                    for (int k = 0; k < GB_UNROLL; ++k) { b[k] = bins[(size_t)row[k] * F + f]; gv[k] = g[row[k]]; hv[k] = h[row[k]]; }
#pragma unroll
                    for (int k = 0; k < GB_UNROLL; ++k)
                        if (q + 32 * k < end) {
                            atomicAdd(&sh[(fl * GB_HS + b[k]) * 2], (u64)(i64)gv[k]);
                            atomicAdd(&sh[(fl * GB_HS + b[k]) * 2 + 1], (u64)(i64)hv[k]);
                        }
                }
            __syncthreads();
            for (int e = t; e < GB_FT * GB_BINS; e += 256) {
                const int efl = e >> 8, b = e & 255, fs = tile0 + efl;
                if (fs < nfs) {
                    const u64 vg = sh[(efl * GB_HS + b) * 2], vh = sh[(efl * GB_HS + b) * 2 + 1];
                    u64* dst = hn + ((size_t)fs * GB_BINS + b) * 2;
                    if (vg) atomicAdd(dst, vg);
                    if (vh) atomicAdd(dst + 1, vh);
                }
            }
            __syncthreads();
        } else if (fvalid) {
            for (int q = p + rsub; q < end; q += 32) {
                const int row = perm[q];
                const int b = bins[(size_t)row * F + f];
                u64* dst = hn + ((size_t)(tile0 + fl) * GB_BINS + b) * 2;
                const int gv = g[row], hv = h[row];
                if (gv) atomicAdd(dst, (u64)(i64)gv);
                if (hv) atomicAdd(dst + 1, (u64)(i64)hv);
            }
        }
        p = end;
    }
}

// ------------------------------------------------------------------------------------------------ split search
struct SplitParams { double lambda, gamma, min_child_weight, learning_rate; };

__device__ inline double gb_gain(i64 GL, i64 HL, i64 G, i64 H, const SplitParams& sp) {
    const double gl = (double)GL * GB_INV_SCALE, hl = (double)HL * GB_INV_SCALE;
    const double gr = (double)(G - GL) * GB_INV_SCALE, hr = (double)(H - HL) * GB_INV_SCALE;
    const double gt = (double)G * GB_INV_SCALE, ht = (double)H * GB_INV_SCALE;
    if (!(hl >= sp.min_child_weight) || !(hr >= sp.min_child_weight)) return -INFINITY;
    const double a = gl * gl / (hl + sp.lambda), b = gr * gr / (hr + sp.lambda), c = gt * gt / (ht + sp.lambda);
    const double gain = 0.5 * ((a + b) - c) - sp.gamma;
    return gain > GB_MIN_GAIN ? gain : -INFINITY;
}
__device__ inline float gb_leaf(i64 G, i64 H, const SplitParams& sp) {
    const double gt = (double)G * GB_INV_SCALE, ht = (double)H * GB_INV_SCALE;
    return (float)(sp.learning_rate * (-gt / (ht + sp.lambda)));
}
__device__ inline bool gb_better(double ga, int ka, double gb, int kb) { return ga > gb || (ga == gb && ka < kb); }

// One 1024-thread workgroup per node of the level; a wave scans one sampled feature at a time (lane = 4 consecutive bins: local prefix,
// wave scan of the lane totals), evaluates the gain of every cut and keeps (largest gain, lowest feature, lowest cut).  The node total is
// the sum of all bins of a feature (every sampled row falls in exactly one bin of each).
__global__ void __launch_bounds__(1024) k_split(const i64* __restrict__ hist, int F, const int* __restrict__ flist, const int* __restrict__ nfs_ptr,
        const float* __restrict__ cuts, const int* __restrict__ ncuts, int level_base, SplitParams sp, GrowHeap hp) {
    __shared__ double s_gain[16];
    __shared__ int s_key[16];
    __shared__ i64 s_gl[16], s_hl[16], s_tot[2];
    const int node = level_base + blockIdx.x;
    if (node > 0 && hp.state[(node - 1) >> 1] != 2) return;        // the parent did not split: the node does not exist
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int nfs = *nfs_ptr;
    double best = -INFINITY;
    int bkey = 0x7fffffff;
    i64 bgl = 0, bhl = 0, G = 0, H = 0;
    for (int fs = wave; fs < nfs; fs += 16) {
        const int f = flist[fs];
        const int nc = min(max(ncuts[f], 0), GB_CUTS);
        const i64* src = hist + ((size_t)blockIdx.x * F + fs) * (GB_BINS * 2) + lane * 8;
        i64 pg[4], ph[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { pg[k] = src[2 * k]; ph[k] = src[2 * k + 1]; }
#pragma unroll
        for (int k = 1; k < 4; ++k) { pg[k] += pg[k - 1]; ph[k] += ph[k - 1]; }
        i64 ig = pg[3], ih = ph[3];                                 // inclusive scan of the lane totals
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const i64 ug = __shfl_up(ig, off), uh = __shfl_up(ih, off);
            if (lane >= off) { ig += ug; ih += uh; }
        }
        G = __shfl(ig, 63); H = __shfl(ih, 63);
        const i64 eg = ig - pg[3], eh = ih - ph[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = lane * 4 + k;
            if (j < nc) {
                const double gain = gb_gain(eg + pg[k], eh + ph[k], G, H, sp);
                const int key = f * GB_BINS + j;
                if (gb_better(gain, key, best, bkey)) { best = gain; bkey = key; bgl = eg + pg[k]; bhl = eh + ph[k]; }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double og = __shfl_xor(best, off);
        const int ok = __shfl_xor(bkey, off);
        const i64 ogl = __shfl_xor(bgl, off), ohl = __shfl_xor(bhl, off);
        if (gb_better(og, ok, best, bkey)) { best = og; bkey = ok; bgl = ogl; bhl = ohl; }
    }
    if (lane == 0) { s_gain[wave] = best; s_key[wave] = bkey; s_gl[wave] = bgl; s_hl[wave] = bhl; }
    if (t == 0) { s_tot[0] = G; s_tot[1] = H; }                     // wave 0 always scans a feature (nfs >= 1)
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 16; ++w)
            if (gb_better(s_gain[w], s_key[w], best, bkey)) { best = s_gain[w]; bkey = s_key[w]; bgl = s_gl[w]; bhl = s_hl[w]; }
        G = s_tot[0]; H = s_tot[1];
        if (best > GB_MIN_GAIN) {
            const int f = bkey / GB_BINS, j = bkey % GB_BINS;
            hp.state[node] = 2; hp.feat[node] = f; hp.cutj[node] = j; hp.cond[node] = cuts[(size_t)f * GB_CUTS + j];
            hp.nodeG[2 * node + 1] = bgl; hp.nodeH[2 * node + 1] = bhl;
            hp.nodeG[2 * node + 2] = G - bgl; hp.nodeH[2 * node + 2] = H - bhl;
        } else {
            hp.state[node] = 1; hp.cond[node] = gb_leaf(G, H, sp);
        }
    }
}
// the nodes of level max_depth are leaves of the totals their parent's split handed down
__global__ void __launch_bounds__(256) k_last_level(int level_base, int n_level, SplitParams sp, GrowHeap hp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_level) return;
    const int node = level_base + i;
    if (hp.state[(node - 1) >> 1] != 2) return;
    hp.state[node] = 1;
    hp.cond[node] = gb_leaf(hp.nodeG[node], hp.nodeH[node], sp);
}

// ------------------------------------------------------------------------------------------------ row partition (level d -> d + 1)
__device__ inline int gb_child(const unsigned char* __restrict__ bins, int F, int row, int node, const GrowHeap& hp) {
    return 2 * node + 1 + (bins[(size_t)row * F + hp.feat[node]] > hp.cutj[node] ? 1 : 0);
}
__global__ void __launch_bounds__(256) k_child_count(const unsigned char* __restrict__ bins, int F, const int* __restrict__ perm,
        const int* __restrict__ pnode, const int* __restrict__ n_cur_ptr, GrowHeap hp) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    bool on = q < *n_cur_ptr;
    int child = 0;
    if (on) {
        const int node = pnode ? pnode[q] : 0;
        on = hp.state[node] == 2;
        if (on) child = gb_child(bins, F, perm[q], node, hp);
    }
    (void)gb_wave_slots(hp.seg_cnt, child, on);
}
// exclusive scan of the child counts of one level (<= 1024 nodes): segment starts, scatter cursors, the level's row count
__global__ void __launch_bounds__(1024) k_level_scan(int child_base, int n_child, int level, GrowHeap hp) {
    __shared__ int s[1024];
    const int t = threadIdx.x;
    const int v = t < n_child ? hp.seg_cnt[child_base + t] : 0;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int u = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    if (t < n_child) { hp.seg_start[child_base + t] = s[t] - v; hp.cursor[child_base + t] = s[t] - v; }
    if (t == 1023) hp.level_n[level] = s[t];
}
__global__ void __launch_bounds__(256) k_scatter(const unsigned char* __restrict__ bins, int F, const int* __restrict__ perm,
        const int* __restrict__ pnode, const int* __restrict__ n_cur_ptr, GrowHeap hp, int* __restrict__ perm_out, int* __restrict__ pnode_out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    bool on = q < *n_cur_ptr;
    int child = 0, row = 0;
    if (on) {
        const int node = pnode ? pnode[q] : 0;
        on = hp.state[node] == 2;
        if (on) { row = perm[q]; child = gb_child(bins, F, row, node, hp); }
    }
    const int slot = gb_wave_slots(hp.cursor, child, on);
    if (on) { perm_out[slot] = row; pnode_out[slot] = child; }
}

// ------------------------------------------------------------------------------------------------ heap -> model records
// Breadth-first numbering = heap order with the absent nodes dropped: the new id of a node is the number of present nodes before it.
// Records go to nodes_out + off[0]; off[1] = off[0] + node count.  One workgroup; heap_n <= 2047.
__global__ void __launch_bounds__(1024) k_compact(int heap_n, GrowHeap hp, const int* __restrict__ off_in, int* __restrict__ off_out,
                                                  int4* __restrict__ nodes_out) {
    __shared__ int s[1024];
    const int t = threadIdx.x;
    const int a = 2 * t, b = 2 * t + 1;
    const int ea = a < heap_n && hp.state[a] != 0, eb = b < heap_n && hp.state[b] != 0;
    s[t] = ea + eb;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int u = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    const int before_a = s[t] - ea - eb, before_b = before_a + ea;
    __syncthreads();
    const int total = s[1023];
    __syncthreads();
    // second pass needs the new id of arbitrary children: publish every node's id through the (now free) cursor array
    if (ea) hp.cursor[a] = before_a;
    if (eb) hp.cursor[b] = before_b;
    __threadfence_block();
    __syncthreads();
    int4* out = nodes_out + off_in[0];
    for (int k = 0; k < 2; ++k) {
        const int n = k ? b : a;
        if (!(k ? eb : ea)) continue;
        int4 rec;
        if (hp.state[n] == 2) { rec.x = hp.cursor[2 * n + 1]; rec.y = hp.cursor[2 * n + 2]; rec.z = hp.feat[n]; }
        else { rec.x = -1; rec.y = -1; rec.z = 0; }
        rec.w = __float_as_int(hp.cond[n]);
        out[k ? before_b : before_a] = rec;
    }
    if (t == 0) off_out[0] = off_in[0] + total;
}

// every row (sampled or not) adds the leaf it falls in to its margin of the tree's class
__global__ void __launch_bounds__(256) k_update(const unsigned char* __restrict__ bins, int n, int F, GrowHeap hp, float* __restrict__ margin, int C, int c) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int node = 0;
    while (hp.state[node] == 2) node = gb_child(bins, F, i, node, hp);
    margin[(size_t)i * C + c] += hp.cond[node];
}

// ------------------------------------------------------------------------------------------------ host side
struct GrowWS {
    void* heap_block = nullptr; size_t heap_bytes = 0;
    GrowHeap hp{};
    int heap_n = 0;
    u64* hist = nullptr; size_t hist_nodes = 0;
    int *perm0 = nullptr, *permA = nullptr, *permB = nullptr, *pnodeA = nullptr, *pnodeB = nullptr;
    int *flist = nullptr, *nfs = nullptr, *n0 = nullptr;     // nfs, n0: two ints of one 16-byte block
    void* small = nullptr;
    void release() {
        for (void* p : {heap_block, (void*)hist, (void*)perm0, (void*)permA, (void*)permB, (void*)pnodeA, (void*)pnodeB, (void*)flist, small})
            if (p) (void)hipFree(p);
        *this = GrowWS();
    }
};

bool grow_ws_alloc(GrowWS& w, int n_rows, int F, int max_depth) {
    const int heap_n = (1 << (max_depth + 1)) - 1;
    w.heap_n = heap_n;
    const size_t hn = ((size_t)heap_n + 3) / 4 * 4;                 // every int array a multiple of 16 bytes
    // state, feat, cutj, cond, seg_start, seg_cnt, cursor (7 x 4 B), nodeG, nodeH (2 x 8 B), level_n (16 ints)
    w.heap_bytes = hn * 4 * 7 + hn * 8 * 2 + 64;
    if (hipMalloc(&w.heap_block, w.heap_bytes) != hipSuccess) return false;
    char* p = (char*)w.heap_block;
    auto take = [&](size_t bytes) { char* q = p; p += bytes; return q; };
    w.hp.nodeG = (i64*)take(hn * 8); w.hp.nodeH = (i64*)take(hn * 8);
    w.hp.state = (int*)take(hn * 4); w.hp.feat = (int*)take(hn * 4); w.hp.cutj = (int*)take(hn * 4); w.hp.cond = (float*)take(hn * 4);
    w.hp.seg_start = (int*)take(hn * 4); w.hp.seg_cnt = (int*)take(hn * 4); w.hp.cursor = (int*)take(hn * 4);
    w.hp.level_n = (int*)take(64);
    w.hist_nodes = (size_t)1 << (max_depth - 1);
    const size_t rows = (size_t)n_rows * sizeof(int);
    bool ok = hipMalloc((void**)&w.hist, w.hist_nodes * F * GB_BINS * 2 * sizeof(u64)) == hipSuccess;
    ok = ok && hipMalloc((void**)&w.perm0, rows) == hipSuccess && hipMalloc((void**)&w.permA, rows) == hipSuccess &&
         hipMalloc((void**)&w.permB, rows) == hipSuccess && hipMalloc((void**)&w.pnodeA, rows) == hipSuccess &&
         hipMalloc((void**)&w.pnodeB, rows) == hipSuccess && hipMalloc((void**)&w.flist, (size_t)F * sizeof(int)) == hipSuccess &&
         hipMalloc(&w.small, 16) == hipSuccess;
    if (ok) { w.nfs = (int*)w.small; w.n0 = w.nfs + 1; }
    return ok;
}

inline unsigned blocks_for(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// rows per histogram chunk: long enough that the flush (one tile per piece) is small against the adds, short enough to fill the chip
int hist_chunk_rows(int n_rows) {
    int r = (n_rows / 64 + 31) / 32 * 32;
    return r < 512 ? 512 : (r > 8192 ? 8192 : r);
}

// perm0 / n0 hold the tree's sampled rows; enqueues the growth of ONE tree, leaves it in w.hp (heap form)
void grow_tree_enqueue(GrowWS& w, const unsigned char* bins, int n_rows, int F, const float* cuts, const int* ncuts, const int* g, const int* h,
                       const unsigned char* feat_mask, int max_depth, const SplitParams& sp, hipStream_t s) {
    launch_zero_bytes(w.heap_block, w.heap_bytes, s);
    hipLaunchKernelGGL(k_feature_list, dim3(1), dim3(64), 0, s, feat_mask, F, w.flist, w.nfs);
    hipLaunchKernelGGL(k_tree_begin, dim3(1), dim3(64), 0, s, w.hp, (const int*)w.n0);
    const int R = hist_chunk_rows(n_rows);
    const dim3 hgrid(blocks_for((size_t)n_rows, (unsigned)R), blocks_for((size_t)F, GB_FT));
    const unsigned rgrid = blocks_for((size_t)n_rows, 256);
    const int* perm = w.perm0;
    const int* pnode = nullptr;                                     // level 0: every sampled row is at the root
    for (int d = 0; d < max_depth; ++d) {
        const int level_base = (1 << d) - 1, n_level = 1 << d;
        launch_zero_bytes(w.hist, (size_t)n_level * F * GB_BINS * 2 * sizeof(u64), s);
        hipLaunchKernelGGL(k_hist, hgrid, dim3(256), 0, s, bins, F, g, h, perm, pnode, (const int*)(w.hp.level_n + d), (const int*)w.hp.seg_start,
                           (const int*)w.hp.seg_cnt, (const int*)w.flist, (const int*)w.nfs, level_base, R, w.hist);
        hipLaunchKernelGGL(k_split, dim3(n_level), dim3(1024), 0, s, (const i64*)w.hist, F, (const int*)w.flist, (const int*)w.nfs, cuts, ncuts,
                           level_base, sp, w.hp);
        if (d + 1 < max_depth) {                                    // the rows of level max_depth are never histogrammed: no grouping
            int* perm_out = (d & 1) ? w.permB : w.permA;
            int* pnode_out = (d & 1) ? w.pnodeB : w.pnodeA;
            hipLaunchKernelGGL(k_child_count, dim3(rgrid), dim3(256), 0, s, bins, F, perm, pnode, (const int*)(w.hp.level_n + d), w.hp);
            hipLaunchKernelGGL(k_level_scan, dim3(1), dim3(1024), 0, s, 2 * level_base + 1, 2 * n_level, d + 1, w.hp);
            hipLaunchKernelGGL(k_scatter, dim3(rgrid), dim3(256), 0, s, bins, F, perm, pnode, (const int*)(w.hp.level_n + d), w.hp, perm_out, pnode_out);
            perm = perm_out; pnode = pnode_out;
        }
    }
    hipLaunchKernelGGL(k_last_level, dim3(blocks_for((size_t)1 << max_depth, 256)), dim3(256), 0, s, (1 << max_depth) - 1, 1 << max_depth, sp, w.hp);
}

int check_params(const rnampnn_gbdt_params* p, bool full) {
    if (!p) return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt: null params");
    if (p->max_depth < 1 || p->max_depth > GB_MAX_DEPTH) return gb_fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_gbdt: max_depth must be 1..10");
    if (!(p->reg_lambda >= 0.0) || !(p->min_child_weight >= 0.0) || !(p->gamma >= 0.0) || !std::isfinite(p->learning_rate))
        return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt: reg_lambda, gamma, min_child_weight must be >= 0 and learning_rate finite");
    if (full) {
        if (p->num_class < 2 || p->num_class > 64 || p->n_estimators < 1) return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_fit: num_class must be 2..64, n_estimators >= 1");
        if (p->max_bin < 2 || p->max_bin > GB_BINS) return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_fit: max_bin must be 2..256");
        if (!(p->subsample > 0.0 && p->subsample <= 1.0) || !(p->colsample_bytree > 0.0 && p->colsample_bytree <= 1.0))
            return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_fit: subsample and colsample_bytree must be in (0, 1]");
    }
    return RNAMPNN_OK;
}

void launch_bin(const float* X, int n_rows, int ldx, int F, const float* cuts, const int* ncuts, unsigned char* bins, int* flag, hipStream_t s) {
    size_t g = ((size_t)n_rows * F + 255) / 256;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(k_bin, dim3((unsigned)g), dim3(256), 0, s, X, n_rows, ldx, F, cuts, ncuts, bins, flag);
}

}  // namespace

extern "C" int rnampnn_gbdt_bin(const float* X, int32_t n_rows, int32_t ldx, int32_t num_feature, const float* cuts, const int32_t* n_cuts,
                                uint8_t* bins, void* stream) {
    if (!X || !cuts || !n_cuts || !bins || n_rows <= 0 || num_feature <= 0 || ldx < num_feature)
        return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_bin: bad argument");
    launch_bin(X, n_rows, ldx, num_feature, cuts, n_cuts, bins, nullptr, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return gb_fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_bin: launch failed");
    return RNAMPNN_OK;
}

extern "C" int rnampnn_gbdt_grow_tree(const rnampnn_gbdt_params* params, const uint8_t* bins, int32_t n_rows, int32_t num_feature, const float* cuts,
                                      const int32_t* n_cuts, const int32_t* g, const int32_t* h, const uint8_t* row_mask, const uint8_t* feat_mask,
                                      int32_t* left_children, int32_t* right_children, int32_t* split_indices, float* split_conditions,
                                      int32_t* n_nodes, void* stream) {
    if (int rc = check_params(params, false)) return rc;
    if (!bins || !cuts || !n_cuts || !g || !h || !left_children || !right_children || !split_indices || !split_conditions || !n_nodes ||
        n_rows <= 0 || num_feature <= 0)
        return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_grow_tree: bad argument");
    hipStream_t s = (hipStream_t)stream;
    GrowWS w;
    const int heap_n = (1 << (params->max_depth + 1)) - 1;
    int4* d_nodes = nullptr;
    int* d_off = nullptr;
    bool ok = grow_ws_alloc(w, n_rows, num_feature, params->max_depth) && hipMalloc((void**)&d_nodes, sizeof(int4) * heap_n) == hipSuccess &&
              hipMalloc((void**)&d_off, 16) == hipSuccess;
    int rc = RNAMPNN_OK;
    if (ok) {
        const SplitParams sp{params->reg_lambda, params->gamma, params->min_child_weight, params->learning_rate};
        launch_zero_bytes(w.small, 16, s);
        launch_zero_bytes(d_off, 16, s);
        hipLaunchKernelGGL(k_init_perm, dim3(blocks_for((size_t)n_rows, 256)), dim3(256), 0, s, row_mask, n_rows, w.perm0, w.n0);
        grow_tree_enqueue(w, bins, n_rows, num_feature, cuts, n_cuts, g, h, feat_mask, params->max_depth, sp, s);
        hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, heap_n, w.hp, (const int*)d_off, d_off + 1, d_nodes);
        std::vector<int4> host((size_t)heap_n);
        int off[2] = {0, 0};
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess &&
             hipMemcpy(off, d_off, sizeof(off), hipMemcpyDeviceToHost) == hipSuccess && off[1] >= 1 && off[1] <= heap_n &&
             hipMemcpy(host.data(), d_nodes, sizeof(int4) * off[1], hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) {
            *n_nodes = off[1];
            for (int i = 0; i < off[1]; ++i) {
                left_children[i] = host[i].x; right_children[i] = host[i].y; split_indices[i] = host[i].z;
                memcpy(&split_conditions[i], &host[i].w, sizeof(float));
            }
        }
    }
    if (!ok) rc = gb_fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_grow_tree: device allocation, launch or copy failed");
    w.release();
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_off) (void)hipFree(d_off);
    return rc;
}

extern "C" int rnampnn_gbdt_fit(const rnampnn_gbdt_params* params, const float* X, int32_t n_rows, int32_t ldx, int32_t num_feature, const int32_t* y,
                                const float* cuts, const int32_t* n_cuts, void* stream, rnampnn_gbdt_handle* out) {
    if (int rc = check_params(params, true)) return rc;
    if (!X || !y || !cuts || !n_cuts || !out || n_rows <= 0 || num_feature <= 0 || ldx < num_feature)
        return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_fit: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int C = params->num_class, F = num_feature, D = params->max_depth, T = params->n_estimators * C;
    const int heap_n = (1 << (D + 1)) - 1;
    const SplitParams sp{params->reg_lambda, params->gamma, params->min_child_weight, params->learning_rate};

    // the feature sample of every tree, on the host (T x F hashes), uploaded once before the first launch
    const int n_sampled = std::max(1, (int)std::floor(params->colsample_bytree * F));
    std::vector<unsigned char> fmask((size_t)T * F, 1);
    if (params->colsample_bytree < 1.0) {
        std::vector<std::pair<double, int>> u((size_t)F);
        for (int t = 0; t < T; ++t) {
            for (int f = 0; f < F; ++f) u[f] = {gb_hash_u(params->seed, 2ull * (uint64_t)t + 1ull, (uint64_t)f), f};
            std::sort(u.begin(), u.end());                          // smallest u first, ties to the lower index
            unsigned char* m = fmask.data() + (size_t)t * F;
            memset(m, 0, (size_t)F);
            for (int k = 0; k < n_sampled; ++k) m[u[k].second] = 1;
        }
    }

    GrowWS w;
    rnampnn_gbdt* model = new rnampnn_gbdt();
    unsigned char *bins = nullptr, *d_fmask = nullptr, *row_mask = nullptr;
    int *gq = nullptr, *hq = nullptr, *flag = nullptr;
    float* margin = nullptr;
    std::vector<int> cls((size_t)T);
    for (int t = 0; t < T; ++t) cls[t] = t % C;                     // round-major, class-minor
    auto fail = [&](int code, const char* msg) {
        w.release();
        for (void* p : {(void*)bins, (void*)d_fmask, (void*)row_mask, (void*)gq, (void*)hq, (void*)flag, (void*)margin})
            if (p) (void)hipFree(p);
        rnampnn_gbdt_destroy(model);
        return gb_fail(code, msg);
    };
    bool ok = grow_ws_alloc(w, n_rows, F, D) && hipMalloc((void**)&bins, (size_t)n_rows * F) == hipSuccess &&
              hipMalloc((void**)&d_fmask, (size_t)T * F) == hipSuccess && hipMalloc((void**)&row_mask, (size_t)n_rows) == hipSuccess &&
              hipMalloc((void**)&gq, sizeof(int) * (size_t)n_rows * C) == hipSuccess && hipMalloc((void**)&hq, sizeof(int) * (size_t)n_rows * C) == hipSuccess &&
              hipMalloc((void**)&flag, 16) == hipSuccess && hipMalloc((void**)&margin, sizeof(float) * (size_t)n_rows * C) == hipSuccess &&
              hipMalloc((void**)&model->d_nodes, sizeof(int4) * (size_t)T * heap_n) == hipSuccess &&
              hipMalloc((void**)&model->d_off, sizeof(int) * ((size_t)T + 4)) == hipSuccess && hipMalloc((void**)&model->d_cls, sizeof(int) * (size_t)T) == hipSuccess;
    if (!ok) return fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_fit: device allocation failed");
    ok = hipMemcpy(d_fmask, fmask.data(), fmask.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(model->d_cls, cls.data(), sizeof(int) * (size_t)T, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) return fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_fit: upload failed");

    // inputs are checked ONCE, before the fit: the only host synchronisation until the model is complete
    const unsigned rgrid = blocks_for((size_t)n_rows, 256);
    launch_zero_bytes(flag, 16, s);
    launch_bin(X, n_rows, ldx, F, cuts, n_cuts, bins, flag, s);
    hipLaunchKernelGGL(k_check_labels, dim3(rgrid), dim3(256), 0, s, y, n_rows, C, flag);
    int hflag = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_fit: binning failed");
    if (hflag) return fail(RNAMPNN_ERR_BAD_ARG, hflag == 1 ? "rnampnn_gbdt_fit: X holds a non-finite value" : "rnampnn_gbdt_fit: a label is outside [0, num_class)");

    const float base = (float)params->base_score;
    hipLaunchKernelGGL(k_fill_f32, dim3(std::min(rgrid * (unsigned)C, 65536u)), dim3(256), 0, s, margin, (size_t)n_rows * C, base);
    launch_zero_bytes(model->d_off, 16, s);                         // d_off[0] = 0; k_compact writes d_off[t + 1]
    for (int r = 0; r < params->n_estimators; ++r) {
        hipLaunchKernelGGL(k_row_mask, dim3(rgrid), dim3(256), 0, s, row_mask, n_rows, (uint64_t)params->seed, (uint64_t)r, params->subsample);
        launch_zero_bytes(w.small, 16, s);
        hipLaunchKernelGGL(k_init_perm, dim3(rgrid), dim3(256), 0, s, (const unsigned char*)row_mask, n_rows, w.perm0, w.n0);
        hipLaunchKernelGGL(k_grad, dim3(rgrid), dim3(256), 0, s, (const float*)margin, y, n_rows, C, gq, hq);
        for (int c = 0; c < C; ++c) {
            const int t = r * C + c;
            grow_tree_enqueue(w, bins, n_rows, F, cuts, n_cuts, gq + (size_t)c * n_rows, hq + (size_t)c * n_rows, d_fmask + (size_t)t * F, D, sp, s);
            hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, heap_n, w.hp, (const int*)(model->d_off + t), model->d_off + t + 1, model->d_nodes);
            hipLaunchKernelGGL(k_update, dim3(rgrid), dim3(256), 0, s, (const unsigned char*)bins, n_rows, F, w.hp, margin, C, c);
        }
    }
    int total = 0;
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess &&
         hipMemcpy(&total, model->d_off + T, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && total >= T;
    if (!ok) return fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_fit: a launch failed");
    model->num_trees = T; model->num_class = C; model->num_feature = F; model->total_nodes = total; model->base_score = base;
    w.release();
    for (void* p : {(void*)bins, (void*)d_fmask, (void*)row_mask, (void*)gq, (void*)hq, (void*)flag, (void*)margin}) (void)hipFree(p);
    *out = model;
    return RNAMPNN_OK;
}

extern "C" int rnampnn_gbdt_export(rnampnn_gbdt_handle g, int32_t* num_trees, int32_t* total_nodes, int32_t* num_class, int32_t* num_feature,
                                   float* base_score, int32_t* tree_offsets, int32_t* tree_class, int32_t* left_children, int32_t* right_children,
                                   int32_t* split_indices, float* split_conditions, uint8_t* default_left) {
    if (!g) return gb_fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_gbdt_export: null handle");
    if (num_trees) *num_trees = g->num_trees;
    if (total_nodes) *total_nodes = g->total_nodes;
    if (num_class) *num_class = g->num_class;
    if (num_feature) *num_feature = g->num_feature;
    if (base_score) *base_score = g->base_score;
    bool ok = true;
    if (tree_offsets) ok = ok && hipMemcpy(tree_offsets, g->d_off, sizeof(int) * ((size_t)g->num_trees + 1), hipMemcpyDeviceToHost) == hipSuccess;
    if (tree_class) ok = ok && hipMemcpy(tree_class, g->d_cls, sizeof(int) * (size_t)g->num_trees, hipMemcpyDeviceToHost) == hipSuccess;
    if (left_children || right_children || split_indices || split_conditions || default_left) {
        std::vector<int4> host((size_t)g->total_nodes);
        ok = ok && hipMemcpy(host.data(), g->d_nodes, sizeof(int4) * (size_t)g->total_nodes, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok)
            for (int i = 0; i < g->total_nodes; ++i) {
                if (left_children) left_children[i] = host[i].x;
                if (right_children) right_children[i] = host[i].y;
                if (split_indices) split_indices[i] = host[i].z & 0x7fffffff;
                if (split_conditions) memcpy(&split_conditions[i], &host[i].w, sizeof(float));
                if (default_left) default_left[i] = host[i].z < 0 ? 1 : 0;
            }
    }
    if (!ok) return gb_fail(RNAMPNN_ERR_HIP, "rnampnn_gbdt_export: copy from the device failed");
    return RNAMPNN_OK;
}
