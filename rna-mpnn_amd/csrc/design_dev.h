// Pieces shared by the nine design kernels - k_design (design.hip, f32), k_design_tied (design_tied.hip), k_design_gc / k_design_count
// (count_tree_dev.h), k_design_distinct (design_distinct.hip), k_design_avoid (design_avoid.hip, avoid_chain_dev.h), k_design_dfa
// (design_dfa.hip: what k_design_avoid uses, with workgroup barriers instead of the fence) and the two profile kernels of
// design_profile.hip, all fp64 - and the kernels of the count tree in global memory (design_long.hip) - and by their entries.  Everything that is about "a position
// under the constraints" has its one definition here: the arguments and the entry prologue (ds_prepare), the mask of a position (ds_mask),
// its row (ds_load<F>), the rows and masks of an RNA into LDS (ds_rows_to_lds), its validated partner (ds_partner), the 16 cells of a pair (ds_pair_mask), the uniform of a position, the DRAW
// RULE as templates over the scalar type - the weights exp(z - max over the admitted), the selection over an admitted set, the joint cell
// of a base pair - the logsumexp over an admitted set (ds_lse), the LDS ceiling, the largest T under it and the reduction's scratch
// (DS_LDS_MAX, ds_max_T, ds_scratch), the fence between lanes of one wave (ds_wave_sync), phase "C" of the kernels that draw into LDS first
// (ds_write_rows) and the tail of an entry that launches with dynamic LDS (ds_launch).  So every entry draws under the same constraints as
// rnampnn_design by construction, and one state per group draws what rnampnn_design draws.  Who uses what: k_design everything up to
// ds_draw_pair (its draw is fused into its row loop, so it keeps that loop, and it asks for no dynamic LDS); k_design_tied the draw rule,
// the prologue, the ceiling, the scratch and the tail (its td_load / td_mask sum and AND over the states of a group: other functions); the
// count tree (both draw kernels and the count profile) and k_design_distinct all of it but the fence; the avoid chain (k_design_avoid and
// the avoid profile) all of it but the partner and the pair (it refuses pairs); the profiles write no rows, so no ds_write_rows.
#pragma once
#include <type_traits>
#include "score_dev.h"

namespace {
struct DesignArgs : ScRows {
    const uint8_t* allowed;      // (B,T) or null
    const int32_t* partner;      // (B,T) or null
    const float* bias;           // 4 floats, (B,T,4), or null
    const unsigned long long* seed_dev;
    unsigned long long seed;
    int wobble, bias_per_position;
    float temperature;
    int8_t* seqs;                // (S,B,T)
    float* seq_nll;              // (S,B)
    int32_t* infeasible;         // (B)
};

constexpr size_t DS_LDS_MAX = 160 * 1024;      // the LDS a workgroup of a design kernel may ask for
constexpr size_t DS_SCRATCH = (SC_WAVES + 2 * SC_WAVES) * 4;     // the bytes sc_block_sums needs: SC_WAVES ints, 2 x SC_WAVES floats

// The prologue of every design entry: the checks of sc_check_args with the entry's `own` checks in its two slots, then the fields of
// DesignArgs past ScRows.  `per`: what S counts sequences per ("RNA", "group").  -> RNAMPNN_OK or what fail() returned.
template <typename Own>
int ds_prepare(const char* name, const char* per, const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B,
               int32_t T, float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed, const int32_t* partner,
               int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs, float* seq_nll, int32_t* infeasible, DesignArgs& a,
               Own own) {
    const ScDraw draw{S, per, temperature, bias, bias_per_position};
    const int rc = sc_check_args(name, logits, n_rows, mask, cu_seqlens, B, T, &draw, a, own);
    if (rc != RNAMPNN_OK) return rc;
    a.allowed = allowed; a.partner = partner; a.bias = bias;
    a.seed_dev = reinterpret_cast<const unsigned long long*>(seed_dev);
    a.seed = (unsigned long long)seed;
    a.wobble = wobble ? 1 : 0; a.bias_per_position = bias_per_position ? 1 : 0;
    a.temperature = temperature;
    a.seqs = seqs; a.seq_nll = seq_nll; a.infeasible = infeasible;
    return RNAMPNN_OK;
}

// the largest T >= 0 whose workgroup fits the ceiling; bytes(T) grows with T.  Only an entry's refusal calls it.
template <typename Bytes>
long long ds_max_T(Bytes bytes) {
    long long T = 0;
    while (bytes(T + 1) <= DS_LDS_MAX) ++T;
    return T;
}

// The tail of an entry whose kernel asks for dynamic LDS: the opt-in above 64 KiB (one DevAttr per kernel), the launch on SC_THREADS
// threads and its error.  "Nothing asked for" and the refusal at the ceiling stay with the entry: their outputs and words are its own.
template <auto Kernel, class Args>
int ds_launch(dim3 grid, size_t lds, void* stream, const Args& a) {
    static DevAttr attr;
    ensure_dyn_lds((const void*)Kernel, lds, attr);
    hipLaunchKernelGGL(Kernel, grid, dim3(SC_THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}

__device__ __forceinline__ void ds_wave_sync() {                   // LDS written by a lane is read by another lane of the SAME wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the reduction's scratch at p (DS_SCRATCH bytes of LDS, 4-byte aligned)
struct DsScratch { int* s_i; float (*s_f)[SC_WAVES]; };
__device__ __forceinline__ DsScratch ds_scratch(unsigned char* p) {
    int* s_i = reinterpret_cast<int*>(p);
    return DsScratch{s_i, reinterpret_cast<float (*)[SC_WAVES]>(s_i + SC_WAVES)};
}

template <typename F> struct DsPos { F z[4]; int m; };   // z = (logit + bias) / temperature; m = the admitted classes (never empty)

// the classes position t admits.  A mask that admits no class is drawn as free; `empty` tells the caller to count it.
__device__ __forceinline__ int ds_mask(const DesignArgs& a, size_t pad0, int t, bool& empty) {
    const int m = a.allowed ? (a.allowed[pad0 + t] & 15) : 15;
    empty = m == 0;
    return empty ? 15 : m;
}

// row t of RNA b in the scalar type F: z = ((F) logit + (F) bias) / (F) temperature; x <- the raw row
template <typename F>
__device__ __forceinline__ DsPos<F> ds_load(const DesignArgs& a, size_t pad0, long long row0, int t, float4& x, bool& empty) {
    x = a.logits[row0 + t];
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bi = a.bias_per_position ? reinterpret_cast<const float4*>(a.bias)[pad0 + t] : make_float4(a.bias[0], a.bias[1], a.bias[2], a.bias[3]);
    const F temp = (F)a.temperature;
    DsPos<F> p;
    p.z[0] = ((F)x.x + (F)bi.x) / temp; p.z[1] = ((F)x.y + (F)bi.y) / temp;
    p.z[2] = ((F)x.z + (F)bi.z) / temp; p.z[3] = ((F)x.w + (F)bi.w) / temp;
    p.m = ds_mask(a, pad0, t, empty);
    return p;
}
template <typename F>
__device__ __forceinline__ DsPos<F> ds_load(const DesignArgs& a, size_t pad0, long long row0, int t, bool& empty) {
    float4 x;                                                      // (dies here)
    return ds_load<F>(a, pad0, row0, t, x, empty);
}

// the partner of position t, or -1: paired only when the table is symmetric and stays inside the RNA: every index is checked before it is used
__device__ __forceinline__ int ds_partner(const DesignArgs& a, size_t pad0, int n, int t) {
    int j = a.partner ? a.partner[pad0 + t] : -1;
    if (j < 0 || j >= n || j == t || a.partner[pad0 + j] != t) j = -1;
    return j;
}

__device__ __forceinline__ unsigned ds_u24(unsigned long long seed, int s, int b, int t) {
    unsigned long long h = mix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(s + 1));
    h = mix64(h ^ (0xD6E8FEB86659FD93ull * (unsigned long long)(b + 1)));
    h = mix64(h ^ (0xBF58476D1CE4E5B9ull * (unsigned long long)(t + 1)));
    return (unsigned)(h >> 40);
}

// the classes that pair with class a (AUCG = 0..3): A-U, U-A, C-G, G-C, and with wobble G-U, U-G
__device__ __forceinline__ int ds_compat(int a, int wobble) {
    return a == 0 ? 2 : a == 1 ? (wobble ? 9 : 1) : a == 2 ? 8 : (wobble ? 6 : 4);
}

// the compatible cells (a, b) = 4 a + b that the masks of a pair's lower and upper end admit
__device__ __forceinline__ int ds_pair_mask(int mlo, int mhi, int wobble) {
    int m = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int ca = c >> 2, cb = c & 3;
        const bool ok = ((mlo >> ca) & 1) && ((mhi >> cb) & 1) && ((ds_compat(ca, wobble) >> cb) & 1);
        m |= (ok ? 1 : 0) << c;
    }
    return m;
}

// w(c) = exp(z(c) - max over the classes m admits), 0 for a class it does not admit
template <typename F, int N>
__device__ __forceinline__ void ds_weights(const F (&z)[N], int m, F (&w)[N]) {
    F mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < N; ++c)
        if ((m >> c) & 1) mx = fmax(mx, z[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) w[c] = ((m >> c) & 1) ? exp(z[c] - mx) : (F)0;
}

// the selection rule over the classes m admits: the first whose running sum of w exceeds u24 * 2^-24 * total, else the last admitted
template <typename F, int N>
__device__ __forceinline__ int ds_select(const F (&w)[N], int m, unsigned u24) {
    F tot = 0;
#pragma unroll
    for (int c = 0; c < N; ++c)
        if ((m >> c) & 1) tot += w[c];
    const F u = (F)u24 * (F)(1.0 / 16777216.0) * tot;
    int q = 0;
    bool found = false;
    F run = 0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        if (!((m >> c) & 1)) continue;
        run += w[c];
        if (!found) { q = c; found = run > u; }                     // (q ends on the last admitted class when nothing is found)
    }
    return q;
}

template <typename F>
__device__ __forceinline__ int ds_draw_single(const DsPos<F>& p, unsigned u24) {
    F w[4];
    ds_weights(p.z, p.m, w);
    return ds_select(w, p.m, u24);
}

// the pair (lo at the smaller index, hi at the larger): the same rule over the 16 cells (a, b) in a-major order, z = z_lo(a) + z_hi(b),
// admitted = compatible and in both masks.  -> the chosen cell as 4 a + b, or -1 when no cell exists
template <typename F>
__device__ __forceinline__ int ds_draw_pair(const DsPos<F>& lo, const DsPos<F>& hi, int wobble, unsigned u24) {
    F z[16], w[16];
    const int m = ds_pair_mask(lo.m, hi.m, wobble);
    if (!m) return -1;
#pragma unroll
    for (int c = 0; c < 16; ++c) z[c] = lo.z[c >> 2] + hi.z[c & 3];
    ds_weights(z, m, w);
    return ds_select(w, m, u24);
}

// logsumexp of z over the cells m admits: max + log(sum of exp(z - max)) in cell order, -inf when no cell is above -inf
template <int N>
__device__ __forceinline__ double ds_lse(const double (&z)[N], int m) {
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

struct DsNoSum {};

// Phase "A" of the kernels that keep the rows of an RNA in LDS (k_design_avoid, k_design_dfa, k_design_dfa_count, k_design_nested and the
// two automaton profiles): the fp64 row of position t into zs[4 t ..], its mask into ms[t], t = tid, tid + 256, ..; `bad` counts the
// positions whose mask admits no class.  `each(t, p)`: what a kernel does with the row in the same turn (the avoid profile's free sum,
// the counted set of k_design_dfa_count); DsNoSum for nothing.  k_design_dfa keeps the loop as its own text: through this function it
// compiled to the same instructions on other scalar registers (295 of 2,848 lines) and measured 2.7 - 3.1 % slower at 73 live states in
// two sessions, +7.40 and +6.96 us where 4.14 and 2.66 were allowed, and within them with the loop back (docs/experiments.md, Round 18).
template <typename Each>
__device__ __forceinline__ void ds_rows_to_lds(const DesignArgs& a, size_t pad0, long long row0, int n, int tid, double* zs, unsigned char* ms, int& bad,
                                               Each each) {
    for (int t = tid; t < n; t += SC_THREADS) {
        bool empty;
        const DsPos<double> p = ds_load<double>(a, pad0, row0, t, empty);
        bad += empty ? 1 : 0;
        zs[4 * t] = p.z[0]; zs[4 * t + 1] = p.z[1]; zs[4 * t + 2] = p.z[2]; zs[4 * t + 3] = p.z[3];
        ms[t] = (unsigned char)p.m;
        if constexpr (!std::is_same<Each, DsNoSum>::value) each(t, p);
    }
}
__device__ __forceinline__ void ds_rows_to_lds(const DesignArgs& a, size_t pad0, long long row0, int n, int tid, double* zs, unsigned char* ms, int& bad) {
    ds_rows_to_lds(a, pad0, row0, n, tid, zs, ms, bad, DsNoSum{});
}

// Phase "C" of a kernel that has drawn into LDS: sample s of RNA b, whose position t holds class cls(t).  Writes the row and its -1
// padding, sums sc_row_nll and `bad` as k_design walks and reduces them (t = tid, tid + 256, ..; sc_block_sums once, one barrier), and
// thread 0 writes seq_nll[s, b] and, for s == 0, infeasible[b].  `extra(t, q)`: a third per-position float to sum; DsNoSum for none.
// -> its total, valid in thread 0.  Every thread calls it.
template <typename Class, typename Extra>
__device__ __forceinline__ float ds_write_rows(const DesignArgs& a, int s, int b, int n, long long row0, int tid, int bad, const DsScratch& sc,
                                               Class cls, Extra extra) {
    int8_t* seq = a.seqs ? a.seqs + ((size_t)s * a.B + b) * a.T : nullptr;
    float nll = 0.f, sum = 0.f;
    for (int t = tid; t < n; t += SC_THREADS) {
        const int q = cls(t);
        if (seq) seq[t] = (int8_t)q;
        if (a.seq_nll) nll += sc_row_nll(a.logits[row0 + t], q);
        if constexpr (!std::is_same<Extra, DsNoSum>::value) sum += extra(t, q);
    }
    if (seq)
        for (int t = n + tid; t < a.T; t += SC_THREADS) seq[t] = (int8_t)-1;
    sc_block_sums(bad, nll, sum, tid, sc.s_i, sc.s_f);
    if (tid == 0) {
        if (a.seq_nll) a.seq_nll[(size_t)s * a.B + b] = nll;
        if (a.infeasible && s == 0) a.infeasible[b] = bad;
    }
    return sum;
}
}  // namespace
