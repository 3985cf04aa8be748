// rnampnn_augment_coords: Gaussian coordinate noise on the device - the role of the reference's RNADataset.noise_augmentation
// (rnampnn/utils/data.py:278-295: a stored copy of an RNA with coordinates + N(0, 1e-2)) and of RNAFeatures(augment_eps) in the rdesign
// sibling (rdesign/model/feature.py:157-158: X + eps * randn_like(X) on every training forward) for the padded training batches.
// The noise of a value is a PURE FUNCTION of (stream of its sample, residue index in the SOURCE RNA, atom, axis): a "noisy copy" is a row of
// a small (sigma, key, offset) table and never a stored array; it is the same in every epoch, on every rank and in whatever batch it lands,
// and a slice of a noisy copy (offset = its start) carries exactly that copy's noise.
// The generator is the one rnampnn/utils/synth.py defines (uniform01 / normal01: splitmix64 finaliser, 24-bit uniforms, Box-Muller with
// 1 - u1, cosine branch), restated in f32 with the accurate logf / sqrtf / cospif; rnampnn/utils/augment.py: noise_reference is the checker.
// One thread per value; 2 x B*T*atoms*12 bytes of traffic.  No runtime fill / copy nodes, no atomics, no synchronisation, nothing read
// from the environment: the launch depends on (B, T, atoms) only, sigma / key / offset are read on the device.
#include "api_internal.h"

namespace {
constexpr int AUG_THREADS = 256;
constexpr unsigned long long AUG_GOLDEN = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ unsigned long long aug_mix64(unsigned long long x) {     // splitmix64 finaliser (synth._mix64)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// synth.uniform01(stream, idx): 24 bits -> [0, 1), exact in f32
__device__ __forceinline__ float aug_uniform01(unsigned long long stream, unsigned long long idx) {
    const unsigned long long bits = aug_mix64(aug_mix64((idx + 1ull) * AUG_GOLDEN + stream) ^ (stream * 0xD6E8FEB86659FD93ull));
    return (float)(unsigned)(bits >> 40) * (1.0f / 16777216.0f);
}
// synth.normal01(stream, idx) in f32: 1 - u1 lies in [2^-24, 1] and is exact, 2 * u2 is exact, so cospif sees the same angle as the f64 form
__device__ __forceinline__ float aug_normal01(unsigned long long stream, unsigned long long idx) {
    const float u1 = aug_uniform01(stream, 2ull * idx);
    const float u2 = aug_uniform01(stream, 2ull * idx + 1ull);
    return sqrtf(-2.0f * logf(1.0f - u1)) * cospif(2.0f * u2);
}

// coords / out may be the same buffer (every thread reads and writes its own word only), hence no __restrict__ on them.
// Grid: x over the T * PER_RES values of one batch row, y over the rows (strided beyond 65,535): sigma / key / offset / the stream are
// uniform over a workgroup, and the residue index is a 32-bit division by a constant.
template <int PER_RES>
__global__ void __launch_bounds__(AUG_THREADS) k_augment_coords(const uint32_t* coords, const float* __restrict__ mask, int B, int T,
                                                                const float* __restrict__ sigma, const unsigned long long* __restrict__ key,
                                                                const int32_t* __restrict__ offset, unsigned long long seed_mixed,
                                                                uint32_t* out) {
    const unsigned row_vals = (unsigned)T * PER_RES;
    const unsigned j = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (j >= row_vals) return;
    const unsigned t = j / PER_RES, within = j - t * PER_RES;       // within = a * 3 + x
    for (unsigned b = blockIdx.y; b < (unsigned)B; b += gridDim.y) {
        const size_t i = (size_t)b * row_vals + j;
        const uint32_t word = coords[i];
        const float sg = sigma[b];
        if (sg == 0.0f || mask[(size_t)b * T + t] == 0.0f) {       // a plain row or a padded residue: the input's bits (-0.0 stays -0.0)
            out[i] = word;
            continue;
        }
        const unsigned long long stream = key ? key[b] : aug_mix64(seed_mixed + ((unsigned long long)b + 1ull) * AUG_GOLDEN);
        const long long res = (long long)(offset ? offset[b] : 0) + (long long)t;
        const unsigned long long idx = (unsigned long long)res * PER_RES + within;
        {
#pragma clang fp contract(off)                                     // one rounded product, one rounded add: what noise_reference states
            const float noise = sg * aug_normal01(stream, idx);
            out[i] = __float_as_uint(__uint_as_float(word) + noise);                // a NaN coordinate stays NaN
        }
    }
}
}  // namespace

extern "C" int rnampnn_augment_coords(const float* coords, const float* mask, int32_t B, int32_t T, int32_t atoms, const float* sigma,
                                      const uint64_t* key, const int32_t* offset, uint64_t seed, float* out, void* stream) {
    if (!coords || !mask || !sigma || !out) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_augment_coords: null coords / mask / sigma / out");
    if (B <= 0 || T <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_augment_coords: empty batch (B = %d, T = %d)", (int)B, (int)T);
    if (atoms != 6 && atoms != 7) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_augment_coords: atoms must be 6 or 7, got %d", (int)atoms);
    if ((long long)T * atoms * 3 > 0x7FFFFFFFll) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_augment_coords: T = %d is beyond the 32-bit row index", (int)T);
    const unsigned row_vals = (unsigned)T * (unsigned)atoms * 3u;
    const dim3 grid((row_vals + AUG_THREADS - 1) / AUG_THREADS, (unsigned)(B < 65535 ? B : 65535));
    auto kernel = atoms == 7 ? k_augment_coords<21> : k_augment_coords<18>;
    hipLaunchKernelGGL(kernel, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(coords), mask, (int)B, (int)T,
                       sigma, reinterpret_cast<const unsigned long long*>(key), offset, aug_mix64((unsigned long long)seed),
                       reinterpret_cast<uint32_t*>(out));
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
