// rnampnn_design: S constrained sequences per RNA drawn from f32 logits and scored, in ONE launch.  Three constraints meet in the draw of
// a position: `allowed` (a 4-bit set of classes: a fixed nucleotide, an IUPAC code, an omitted letter), `partner` (the two ends of a base
// pair of the target secondary structure are drawn TOGETHER, from the joint distribution over the compatible cells AU UA CG GC [+ GU UG])
// and `bias` (added to the logits, global or per position).  The reference has no sampler; the contract is the one include/rnampnn_hip.h
// documents and tests/_design_ref.py restates in float64.
// A sibling of score.hip: one 256-thread workgroup per (RNA, sample), the same extent (sc_extent), the same walk over the rows, the same
// per-row NLL and the same reduction (score_dev.h), so `seq_nll` is byte for byte what rnampnn_score returns for the drawn sequences.  Both
// ends of a pair compute the pair's cell on their own (the partner's row is one more 16-byte load) and each writes its own component: no
// exchange between threads, so a pair may span waves or 256-strides.  No workspace, no runtime fill / copy node, no atomics, no host
// synchronisation; the draw is a pure function of (seed, s, b, t) and the rows it reads.
#include "design_dev.h"

namespace {
struct DesignArgs {
    const float4* logits;        // (B*T) or (n_rows) rows of 4
    const float* mask;           // (B,T) prefix mask, or null
    const int32_t* cu;           // (B+1), or null
    const uint8_t* allowed;      // (B,T) or null
    const int32_t* partner;      // (B,T) or null
    const float* bias;           // 4 floats, (B,T,4), or null
    const unsigned long long* seed_dev;
    unsigned long long seed;
    long long n_rows;
    int B, T;
    int wobble, bias_per_position;
    float temperature;
    int8_t* seqs;                // (S,B,T)
    float* seq_nll;              // (S,B)
    int32_t* infeasible;         // (B)
};

struct DsPos { float z[4]; int m; };     // z = (logit + bias) / temperature; m = the admitted classes (never empty)

// row t of RNA b.  A mask that admits no class is drawn as free; `empty` tells the caller to count it.
__device__ __forceinline__ DsPos ds_load(const DesignArgs& a, size_t pad0, long long row0, int t, float4& x, bool& empty) {
    x = a.logits[row0 + t];
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bi = a.bias_per_position ? reinterpret_cast<const float4*>(a.bias)[pad0 + t] : make_float4(a.bias[0], a.bias[1], a.bias[2], a.bias[3]);
    DsPos p;
    p.z[0] = (x.x + bi.x) / a.temperature; p.z[1] = (x.y + bi.y) / a.temperature;
    p.z[2] = (x.z + bi.z) / a.temperature; p.z[3] = (x.w + bi.w) / a.temperature;
    const int m = a.allowed ? (a.allowed[pad0 + t] & 15) : 15;
    empty = m == 0;
    p.m = empty ? 15 : m;
    return p;
}

// the first admitted class whose running sum of exp(z - max) exceeds u24 * 2^-24 * total; the last admitted one if none does
__device__ __forceinline__ int ds_draw_single(const DsPos& p, unsigned u24) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if ((p.m >> c) & 1) mx = fmaxf(mx, p.z[c]);
    float w[4], tot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        w[c] = ((p.m >> c) & 1) ? expf(p.z[c] - mx) : 0.f;
        if ((p.m >> c) & 1) tot += w[c];
    }
    const float u = (float)u24 * (1.0f / 16777216.0f) * tot;
    int q = 0;
    bool found = false;
    float run = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((p.m >> c) & 1)) continue;
        run += w[c];
        if (!found) { q = c; found = run > u; }                 // (q ends on the last admitted class when nothing is found)
    }
    return q;
}

// the pair (lo at the smaller index, hi at the larger): cells (a, b) in a-major order, weight exp(z_lo(a) + z_hi(b) - max) over the compatible
// cells both masks admit.  -> the chosen cell as 4 a + b, or -1 when no cell exists.
__device__ __forceinline__ int ds_draw_pair(const DsPos& lo, const DsPos& hi, int wobble, unsigned u24) {
    float mx = -INFINITY;
    int any = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int ca = c >> 2, cb = c & 3;
        const bool ok = ((lo.m >> ca) & 1) && ((hi.m >> cb) & 1) && ((ds_compat(ca, wobble) >> cb) & 1);
        if (ok) { any = 1; mx = fmaxf(mx, lo.z[ca] + hi.z[cb]); }
    }
    if (!any) return -1;
    float tot = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int ca = c >> 2, cb = c & 3;
        const bool ok = ((lo.m >> ca) & 1) && ((hi.m >> cb) & 1) && ((ds_compat(ca, wobble) >> cb) & 1);
        if (ok) tot += expf((lo.z[ca] + hi.z[cb]) - mx);
    }
    const float u = (float)u24 * (1.0f / 16777216.0f) * tot;
    int q = 0;
    bool found = false;
    float run = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int ca = c >> 2, cb = c & 3;
        const bool ok = ((lo.m >> ca) & 1) && ((hi.m >> cb) & 1) && ((ds_compat(ca, wobble) >> cb) & 1);
        if (!ok) continue;
        run += expf((lo.z[ca] + hi.z[cb]) - mx);
        if (!found) { q = c; found = run > u; }
    }
    return q;
}

__global__ void __launch_bounds__(SC_THREADS) k_design(DesignArgs a) {
    __shared__ int s_i[SC_WAVES];
    __shared__ float s_f[2][SC_WAVES];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    int n;
    long long row0;
    sc_extent(a.mask, a.cu, a.n_rows, a.T, b, tid, s_f[0], n, row0);
    const size_t pad0 = (size_t)b * a.T;
    int8_t* seq = a.seqs ? a.seqs + ((size_t)s * a.B + b) * a.T : nullptr;
    int bad = 0;
    float nll = 0.f, unused = 0.f;
    for (int t = tid; t < n; t += SC_THREADS) {
        float4 x, xj;
        bool empty, empty_j;
        const DsPos p = ds_load(a, pad0, row0, t, x, empty);
        bad += empty ? 1 : 0;
        // paired only when the table is symmetric and stays inside the RNA: every index is checked before it is used
        int j = a.partner ? a.partner[pad0 + t] : -1;
        if (j < 0 || j >= n || j == t || a.partner[pad0 + j] != t) j = -1;
        int q = -1;
        if (j >= 0) {
            const DsPos pj = ds_load(a, pad0, row0, j, xj, empty_j);
            const bool first = t < j;
            const int cell = ds_draw_pair(first ? p : pj, first ? pj : p, a.wobble, ds_u24(seed, s, b, first ? t : j));
            if (cell >= 0) q = first ? (cell >> 2) : (cell & 3);
            else bad += 1;                                          // each end counts itself: 2 per pair
        }
        if (q < 0) q = ds_draw_single(p, ds_u24(seed, s, b, t));
        if (seq) seq[t] = (int8_t)q;
        if (a.seq_nll) nll += sc_row_nll(x, q);
    }
    if (seq)
        for (int t = n + tid; t < a.T; t += SC_THREADS) seq[t] = (int8_t)-1;
    sc_block_sums(bad, nll, unused, tid, s_i, s_f);
    if (tid != 0) return;
    if (a.seq_nll) a.seq_nll[(size_t)s * a.B + b] = nll;
    if (a.infeasible && s == 0) a.infeasible[b] = bad;
}
}  // namespace

extern "C" int rnampnn_design(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                              float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                              const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs,
                              float* seq_nll, int32_t* infeasible, void* stream) {
    if (!logits || B <= 0 || T <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: null logits or empty batch (B = %d, T = %d)", (int)B, (int)T);
    if (S <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: S = %d sequences per RNA", (int)S);
    if (S + 1 > 65535) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: at most 65534 sequences per call");
    if ((mask != nullptr) == (cu_seqlens != nullptr))
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: pass exactly one of mask (padded logits) and cu_seqlens (packed logits)");
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f))
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: the temperature must be positive and finite (got %g)", (double)temperature);
    if (((uintptr_t)logits & 15) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: logits must be 16-byte aligned");
    if (bias && bias_per_position && ((uintptr_t)bias & 15) != 0)
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: a per-position bias must be 16-byte aligned");
    if (cu_seqlens && n_rows < 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_design: negative row count");
    if (!seqs && !seq_nll && !infeasible) return RNAMPNN_OK;    // nothing asked for
    DesignArgs a{};
    a.logits = reinterpret_cast<const float4*>(logits);
    a.mask = mask; a.cu = cu_seqlens; a.allowed = allowed; a.partner = partner; a.bias = bias;
    a.seed_dev = reinterpret_cast<const unsigned long long*>(seed_dev);
    a.seed = (unsigned long long)seed;
    a.n_rows = mask ? (long long)B * T : (long long)n_rows;
    a.B = B; a.T = T; a.wobble = wobble ? 1 : 0; a.bias_per_position = bias_per_position ? 1 : 0;
    a.temperature = temperature;
    a.seqs = seqs; a.seq_nll = seq_nll; a.infeasible = infeasible;
    const int passes = (seqs || seq_nll) ? S : 1;               // the count of infeasible positions is that of sample 0
    hipLaunchKernelGGL(k_design, dim3(B, passes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
