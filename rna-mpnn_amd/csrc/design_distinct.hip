// rnampnn_design_distinct: S DIFFERENT constrained sequences per RNA in one launch - an exact sample without replacement (noise != 0) or the
// S most probable admitted sequences (noise == 0).  Under the constraints of rnampnn_design the distribution factorises over independent
// units (unpaired positions, feasible base pairs), so a beam of width S over the units with conditioned Gumbel keys (Kool et al. 2019,
// "Stochastic Beams and Where to Find Them") is exact in both readings.  The contract is the one include/rnampnn_hip.h documents and
// tests/_design_distinct_ref.py restates; all of the draw is fp64.
// One 256-thread workgroup per RNA (the samples of an RNA interact), the extent / NLL / reduction of score_dev.h; of design_dev.h the
// mask, the fp64 row, the validated partner and the pair cells of a unit, the logsumexp of its cells, the scratch, phase C per slot and
// the entry's prologue - the pieces the count tree uses, so a unit here is a leaf there.
// (A) the walk over the units, 128 positions at a time: one thread per position forms the unit's cells and their l = z - LSE into LDS, then per unit: one thread per candidate (slot, cell) forms its key, one thread per
// candidate counts the candidates that order before it (its rank; a rank below S is a survivor), one thread per survivor writes the new
// slot state and its back-pointer into the history (12 bits: the parent slot in a byte, the cell's index and a pair flag in half a
// byte).  (B) the walk back: one thread per slot follows its back-pointers and leaves the class of every position in the history's rows,
// all slots in step.  (C) per filled slot the rows, the NLL and the counts as k_design writes and reduces them (ds_write_rows).  No
// workspace, no atomics, no runtime fill / copy node, no host synchronisation.
#include "design_dev.h"

namespace {
constexpr unsigned long long DD_SALT = RNAMPNN_DESIGN_DISTINCT_SALT;
constexpr int DD_MAX_S = RNAMPNN_DESIGN_DISTINCT_MAX_S;
constexpr int DD_CELLS = 6;                    // a position admits at most 4 classes, a pair at most 6 compatible cells
constexpr int DD_CHUNK = 128;                  // positions whose units are formed together
constexpr size_t DD_LDS_SCRATCH = 96;          // the reduction's DS_SCRATCH bytes, padded
static_assert(DS_SCRATCH <= DD_LDS_SCRATCH, "the reduction's scratch");
constexpr unsigned DD_SKIP = 0xFFu;            // history: the first byte of the 4-bit row of a position that is no unit (an upper end)

struct DdArgs : DesignArgs {
    int S, noise;
    float* logp;                 // (S,B) or null
    int32_t* n_distinct;         // (B) or null
};

using DdPos = DsPos<double>;

// the cells m admits, in order, with l = z - LSE -> the unit's word: bits 0..2 the number of cells, bit 3 a pair, bits 4 + 4 k.. cell k
template <int N>
__device__ __forceinline__ unsigned dd_cells(const double (&z)[N], int m, unsigned pair, double* ell) {
    const double lse = ds_lse(z, m);
    unsigned w = pair << 3;
    int k = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        if (!((m >> c) & 1) || k >= DD_CELLS) continue;
        ell[k] = z[c] - lse;
        w |= (unsigned)c << (4 + 4 * k);
        ++k;
    }
    return w | (unsigned)k;
}

// Position t as a unit: 0 for the upper end of a feasible pair, else its word and the l of its cells.  `bad` counts as k_design counts: an
// empty mask 1, each end of a pair without an admitted compatible cell 1.  Every index is checked before it is used.
__device__ __forceinline__ unsigned dd_unit(const DdArgs& a, size_t pad0, long long row0, int n, int t, double* ell, int& bad) {
    bool empty, empty_j;
    const DdPos p = ds_load<double>(a, pad0, row0, t, empty);
    bad += empty ? 1 : 0;
    const int j = ds_partner(a, pad0, n, t);
    if (j >= 0) {
        const int mj = ds_mask(a, pad0, j, empty_j);
        const int m = t < j ? ds_pair_mask(p.m, mj, a.wobble) : ds_pair_mask(mj, p.m, a.wobble);
        if (!m) bad += 1;
        else if (t > j) return 0u;
        else {
            const DdPos pj = ds_load<double>(a, pad0, row0, j, empty_j);
            double z[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) z[c] = p.z[c >> 2] + pj.z[c & 3];
            return dd_cells(z, m, 1u, ell);
        }
    }
    return dd_cells(p.z, p.m, 0u, ell);
}

__device__ __forceinline__ unsigned long long dd_child(unsigned long long h, int t, int cell) {
    return mix64(h ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(16 * (t + 1) + cell)));
}
__device__ __forceinline__ double dd_key(double x) { return x == x ? x : -INFINITY; }    // a NaN key is -inf

// The ranks of the candidates tid, tid + 256, .. (R of them) among the N keys: how many order before each - key descending, then candidate
// index ascending (parent slot, then cell).  A candidate of rank r < keep becomes slot r.
template <int R>
__device__ __forceinline__ void dd_rank(const double* key, int N, int keep, int tid, unsigned short* sel) {
    double kc[R];
    int rk[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = tid + r * SC_THREADS;
        kc[r] = c < N ? key[c] : 0.0;
        rk[r] = 0;
    }
#pragma unroll 8
    for (int m = 0; m < N; ++m) {                                   // (unrolled: one wave per SIMD runs here, so the loads of eight keys overlap)
        const double km = key[m];                                   // (one address for the whole wave: a broadcast)
#pragma unroll
        for (int r = 0; r < R; ++r) rk[r] += (int)(km > kc[r]) | ((int)(km == kc[r]) & (int)(m < tid + r * SC_THREADS));   // (no branch)
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = tid + r * SC_THREADS;
        if (c < N && rk[r] < keep) sel[rk[r]] = (unsigned short)c;
    }
}

__global__ void __launch_bounds__(SC_THREADS) k_design_distinct(DdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dd_lds[];
    const int S = a.S, NS = (S + 1) >> 1, T = a.T, b = blockIdx.x, tid = threadIdx.x;
    double* phi = reinterpret_cast<double*>(dd_lds);                               // [2][S]   phi of a slot
    double* gum = phi + 2 * S;                                                     // [2][S]   G of a slot
    unsigned long long* hsh = reinterpret_cast<unsigned long long*>(gum + 2 * S);  // [2][S]   H of a slot's prefix
    double* gk = reinterpret_cast<double*>(hsh + 2 * S);                           // [6 S]    g of a candidate
    double* key = gk + DD_CELLS * S;                                               // [6 S]    its key
    double* ell = key + DD_CELLS * S;                                              // [128][6] l of the cells of a chunk's units
    unsigned* unit = reinterpret_cast<unsigned*>(ell + DD_CHUNK * DD_CELLS);       // [128]    their words
    unsigned char* red = reinterpret_cast<unsigned char*>(unit + DD_CHUNK);        // the reduction's scratch
    const DsScratch sc = ds_scratch(red);
    unsigned short* sel = reinterpret_cast<unsigned short*>(red + DD_LDS_SCRATCH);  // [S], padded to 8
    unsigned char* hp = reinterpret_cast<unsigned char*>(sel + ((S + 7) & ~7));    // [T][S]   history: the parent slot, then the class
    unsigned char* hn = hp + (size_t)T * S;                                        // [T][NS]  history: the cell's index and the pair flag, 4 bits
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    int n;
    long long row0;
    sc_extent(a, b, tid, sc.s_f[0], n, row0);
    const size_t pad0 = (size_t)b * T;
    if (tid == 0) {
        phi[0] = 0.0; gum[0] = 0.0;
        hsh[0] = mix64(mix64(seed ^ DD_SALT) ^ (0xD6E8FEB86659FD93ull * (unsigned long long)(b + 1)));
    }
    // ---- A: the beam over the units
    int cur = 0, live = 1, bad = 0;
    for (int t0 = 0; t0 < n; t0 += DD_CHUNK) {
        __syncthreads();                                            // the units of the chunk before are done with ell / unit
        if (tid < DD_CHUNK && t0 + tid < n) unit[tid] = dd_unit(a, pad0, row0, n, t0 + tid, ell + tid * DD_CELLS, bad);
        __syncthreads();
        const int tn = min(DD_CHUNK, n - t0);
        for (int dt = 0; dt < tn; ++dt) {
            const unsigned w = unit[dt];
            const int nc = w & 7, t = t0 + dt;
            const unsigned flag = w & 8;                            // a pair's cell
            const double* el = ell + dt * DD_CELLS;
            double* ph = phi + cur * S;
            double* gm = gum + cur * S;
            unsigned long long* hs = hsh + cur * S;
            if (nc == 0) {                                          // no unit: the walk back passes over this row
                if (tid == 0) hn[t * NS] = (unsigned char)DD_SKIP;
                continue;
            }
            if (nc == 1) {                                          // one cell: every slot keeps its place, no selection
                if (tid < live) {
                    const double f = ph[tid] + el[0];
                    ph[tid] = f;
                    if (a.noise) hs[tid] = dd_child(hs[tid], t, (w >> 4) & 15);
                    else gm[tid] = dd_key(f);
                    hp[t * S + tid] = (unsigned char)tid;
                    if (!(tid & 1)) hn[t * NS + (tid >> 1)] = (unsigned char)(flag | (flag << 4));    // cell index 0 in both halves
                }
                __syncthreads();
                continue;
            }
            const int N = live * nc, keep = min(S, N);
            for (int c = tid; c < N; c += SC_THREADS) {             // candidate c = parent slot * nc + cell
                const int p = c / nc, k = c - p * nc;
                const double f = ph[p] + el[k];
                if (!a.noise) { key[c] = dd_key(f); continue; }
                const unsigned long long h = dd_child(hs[p], t, (w >> (4 + 4 * k)) & 15);
                const double u = ((double)(h >> 11) + 0.5) * 0x1p-53;
                gk[c] = f - log(-log(u));
            }
            if (a.noise) {
                __syncthreads();
                for (int c = tid; c < N; c += SC_THREADS) {
                    const int p = c / nc;
                    double Z = -INFINITY;
                    for (int k = 0; k < nc; ++k) Z = fmax(Z, gk[p * nc + k]);
                    const double g = gk[c], G = gm[p];
                    double kap = G;                                 // the child that attains Z keeps G exactly
                    if (!(g == Z)) {
                        const double v = G - g + log1p(-exp(g - Z));
                        kap = G - fmax(0.0, v) - log1p(exp(-fabs(v)));
                    }
                    key[c] = dd_key(kap);
                }
            }
            __syncthreads();
            if (N <= SC_THREADS) dd_rank<1>(key, N, keep, tid, sel);
            else if (N <= 2 * SC_THREADS) dd_rank<2>(key, N, keep, tid, sel);
            else if (N <= 4 * SC_THREADS) dd_rank<4>(key, N, keep, tid, sel);
            else dd_rank<DD_CELLS>(key, N, keep, tid, sel);
            __syncthreads();
            unsigned nib = 0;                                       // the survivor's cell index and flag; the even slot writes its neighbour's too
            if (tid < keep) {
                const int c = sel[tid], p = c / nc, k = c - p * nc;
                const int nx = (cur ^ 1) * S + tid;
                phi[nx] = ph[p] + el[k];
                gum[nx] = key[c];
                if (a.noise) hsh[nx] = dd_child(hs[p], t, (w >> (4 + 4 * k)) & 15);
                hp[t * S + tid] = (unsigned char)p;
                nib = (unsigned)k | flag;
            }
            const unsigned up = __shfl_down(nib, 1, 64);
            if (tid < keep && !(tid & 1)) hn[t * NS + (tid >> 1)] = (unsigned char)(nib | (up << 4));
            __syncthreads();
            cur ^= 1;
            live = keep;
        }
    }
    __syncthreads();
    // ---- B: the walk back, every slot in step: read the row's back-pointer, barrier, leave the class in the slot's own column of hp
    int p = tid;
    for (int t = n - 1; t >= 0; --t) {
        const unsigned n0 = hn[t * NS];                             // (slot 0 is always filled; one address: the branches below are uniform)
        if ((n0 & 15) == DD_SKIP >> 4) continue;
        bool empty;
        int cells = ds_mask(a, pad0, t, empty), j = -1;             // the unit's cells again: integers only
        if (n0 & 8) {
            j = a.partner[pad0 + t];                                // the partner the walk forward validated, checked again before use
            if (j <= t || j >= n) j = -1;
            else cells = ds_pair_mask(cells, ds_mask(a, pad0, j, empty), a.wobble);
        }
        int k = 0, up = 0;
        if (tid < live) {
            up = hp[t * S + p];
            k = (hn[t * NS + (p >> 1)] >> (4 * (p & 1))) & 7;
        }
        __syncthreads();
        if (tid >= live) continue;
        p = up;
        int cell = 0;
        for (int c = 0; c < 16; ++c) {                              // the k-th cell the unit admits
            if (!((cells >> c) & 1)) continue;
            cell = c;
            if (k-- == 0) break;
        }
        if (j >= 0) { hp[t * S + tid] = (unsigned char)(cell >> 2); hp[j * S + tid] = (unsigned char)(cell & 3); }
        else hp[t * S + tid] = (unsigned char)(cell & 3);
    }
    __syncthreads();
    // ---- C: the rows, the NLL and the counts of every slot, as k_design walks and reduces them
    for (int s = 0; s < S; ++s) {
        if (s >= live) {
            if (a.seqs)
                for (int t = tid; t < T; t += SC_THREADS) a.seqs[((size_t)s * a.B + b) * T + t] = (int8_t)-1;
            continue;
        }
        ds_write_rows(a, s, b, n, row0, tid, s == 0 ? bad : 0, sc, [&](int t) { return hp[t * S + s] & 3; }, DsNoSum{});
        __syncthreads();                                            // the scratch is written again by the next slot
    }
    if (tid < S) {
        const size_t o = (size_t)tid * a.B + b;
        if (a.logp) a.logp[o] = tid < live ? (float)phi[cur * S + tid] : -INFINITY;
        if (a.seq_nll && tid >= live) a.seq_nll[o] = INFINITY;
    }
    if (tid == 0 && a.n_distinct) a.n_distinct[b] = live;
}

// the bytes of dynamic LDS, from (S, T) alone: the formula include/rnampnn_hip.h gives
size_t dd_lds_bytes(long long S, long long T) {
    const size_t state = 3 * 2 * 8 * (size_t)S, cand = 2 * DD_CELLS * 8 * (size_t)S, chunk = (size_t)DD_CHUNK * (DD_CELLS * 8 + 4);
    const size_t sel = 16 * (((size_t)S + 7) / 8), hist = 16 * ((((size_t)S + ((size_t)S + 1) / 2) * (size_t)T + 15) / 16);
    return state + cand + chunk + DD_LDS_SCRATCH + sel + hist;
}
long long dd_max_T(long long S) {
    const size_t fixed = dd_lds_bytes(S, 0);
    if (fixed >= DS_LDS_MAX) return 0;
    long long T = (long long)((DS_LDS_MAX - fixed) / (size_t)(S + (S + 1) / 2));
    while (T > 0 && dd_lds_bytes(S, T) > DS_LDS_MAX) --T;           // (the history is rounded up to 16 bytes)
    return T;
}
}  // namespace

extern "C" int rnampnn_design_distinct(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                       float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                                       const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position, int32_t noise,
                                       int8_t* seqs, float* seq_nll, int32_t* infeasible, float* logp, int32_t* n_distinct, void* stream) {
    DdArgs a{};
    const int rc = ds_prepare("rnampnn_design_distinct", "RNA", logits, n_rows, mask, cu_seqlens, B, T, temperature, S, seed, seed_dev, allowed,
                              partner, wobble, bias, bias_per_position, seqs, seq_nll, infeasible, a, [&](int slot) {
        if (slot == 0 && S > DD_MAX_S)
            return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design_distinct: S = %d, at most %d distinct sequences per RNA", (int)S, DD_MAX_S);
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    const size_t lds = dd_lds_bytes(S, T);
    if (lds > DS_LDS_MAX)
        return fail(RNAMPNN_ERR_UNSUPPORTED, "rnampnn_design_distinct: S = %d, T = %d needs %zu bytes of LDS for the beam's history, the limit is %zu "
                    "(T <= %lld at this S)", (int)S, (int)T, lds, DS_LDS_MAX, dd_max_T(S));
    if (!seqs && !seq_nll && !infeasible && !logp && !n_distinct) return RNAMPNN_OK;    // nothing asked for
    a.S = S; a.noise = noise ? 1 : 0; a.logp = logp; a.n_distinct = n_distinct;
    return ds_launch<k_design_distinct>(dim3(B), lds, stream, a);
}
