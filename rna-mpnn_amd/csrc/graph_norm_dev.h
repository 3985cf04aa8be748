// Device side of the forward GraphNormalization (functional.py:33-46) shared by kernels_f32.hip and kernels_bf16.hip:
//   mu = sum_valid x / n ;  var = [sum_valid (x - mu)^2 + (T_tot - n) mu^2] / n ;  y = (x - mu) / sqrt(var + 1e-6) * scale + shift
// TWO-PASS statistics (mean, then squared deviations): the one-pass form sum x^2 + (T - 2n) mu^2 cancels once |h| >> sigma.
// The T_tot - n padded rows of the reference do not exist on packed rows; they enter the variance as (0 - mu)^2.
// Here live the ONE row core (a thread's float4 rows of one RNA and their two partial sums) and the ONE place the variance is
// formed; how a block folds the partials (linear order through LDS, shuffle tree, DPP tree) stays with each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "bf16_core.h"             // kSEPS

// sqrt(var + eps) from the folded sum of squared deviations and the mean of one (RNA, channel)
__device__ __forceinline__ float gn_sd(float sq, float mean, int n, int t_tot) {
    const float pad = (float)(t_tot - n), fn = (float)n;
    return sqrtf((sq + pad * mean * mean) / fn + kSEPS);
}
// the same as the affine map y = a x + b
__device__ __forceinline__ void gn_affine(float sq, float mean, int n, int t_tot, float scale, float shift, float& a, float& b) {
    a = scale / gn_sd(sq, mean, n, t_tot);
    b = shift - mean * a;
}

// Rows g, g + NG, g + 2 NG, ... < n of one channel quad (xb: row 0 of the quad; a row is 32 float4).
// NR > 0: the thread's <= NR rows are read ONCE into registers (clamped index, so all NR loads are in flight together) and
// serve both passes and the epilogue; the caller guarantees n <= NG * NR.  NR == 0: every pass re-reads the L2-resident rows.
// Per-thread order: ascending rows, plain adds for the sum, fmaf(d, d, acc) for the squared deviations.
template <int NG, int NR>
struct GnRows {
    const float4* xb;
    int g, n;
    float4 v[NR > 0 ? NR : 1];
    __device__ __forceinline__ GnRows(const float4* xb_, int g_, int n_) : xb(xb_), g(g_), n(n_) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int r = g + NG * i, rc = r < n ? r : n - 1;
            v[i] = xb[(size_t)rc * 32];
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {            // f(row, value) over the thread's valid rows, ascending
        if constexpr (NR > 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
                if (g + NG * i < n) f(g + NG * i, v[i]);
        } else {
            // (four rows in flight: with two the long-RNA instance measured 13.6 against 10.7 us; a row is a float4 already, so no
            //  vectorised second copy of the loop behind a run-time overlap check)
#pragma clang loop unroll_count(4) vectorize(disable)
            for (int r = g; r < n; r += NG) f(r, xb[(size_t)r * 32]);
        }
    }
    __device__ __forceinline__ float4 sum() const {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        each([&](int, const float4& x) { s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w; });
        return s;
    }
    __device__ __forceinline__ float4 sqdev(const float4& mean) const {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        each([&](int, const float4& x) {
            const float dx = x.x - mean.x, dy = x.y - mean.y, dz = x.z - mean.z, dw = x.w - mean.w;
            q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w);
        });
        return q;
    }
};
