// Pieces shared by the two design kernels, k_design (design.hip, f32) and k_design_tied (design_tied.hip, fp64): their arguments, the
// uniform of a position, the base-pair compatibility sets and the DRAW RULE as templates over the scalar type - the weights
// exp(z - max over the admitted), the selection over an admitted set and the joint cell of a base pair.  One definition of each, so that
// one state per group draws what rnampnn_design draws by construction.
#pragma once
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

// the fields of DesignArgs past ScRows, from an entry's arguments
inline void ds_fill(DesignArgs& a, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed, const int32_t* partner, int32_t wobble,
                    const float* bias, int32_t bias_per_position, float temperature, int8_t* seqs, float* seq_nll, int32_t* infeasible) {
    a.allowed = allowed; a.partner = partner; a.bias = bias;
    a.seed_dev = reinterpret_cast<const unsigned long long*>(seed_dev);
    a.seed = (unsigned long long)seed;
    a.wobble = wobble ? 1 : 0; a.bias_per_position = bias_per_position ? 1 : 0;
    a.temperature = temperature;
    a.seqs = seqs; a.seq_nll = seq_nll; a.infeasible = infeasible;
}

template <typename F> struct DsPos { F z[4]; int m; };   // z = (logit + bias) / temperature; m = the admitted classes (never empty)

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
    int m = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int ca = c >> 2, cb = c & 3;
        const bool ok = ((lo.m >> ca) & 1) && ((hi.m >> cb) & 1) && ((ds_compat(ca, wobble) >> cb) & 1);
        m |= (ok ? 1 : 0) << c;
        z[c] = lo.z[ca] + hi.z[cb];
    }
    if (!m) return -1;
    ds_weights(z, m, w);
    return ds_select(w, m, u24);
}
}  // namespace
