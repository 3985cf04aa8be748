// rdesign_score: the per-RNA metrics of RNAModel.validation_step / test_step (rdesign/model/rdesign.py:106-141 of the reference: argmax of
// the read-out against the labels, recovery per RNA, cross-entropy) on the device, from the PACKED logits rdesign_forward writes - or from
// packed class ids (the tree read-out) - and the padded labels the training step takes.  One 256-thread workgroup per RNA; a thread walks
// its rows in ascending order (one 16-byte load per row), then a wave butterfly and one LDS hop over the four waves: a fixed order, no
// atomics, so two calls give identical bytes.  About 20 bytes per nucleotide: the call is bounded by its three launches, not by bandwidth.
// No runtime fill / copy nodes, no host synchronisation.
#include "rdesign_internal.h"
#include "score_dev.h"

namespace {
constexpr int RDS_THREADS = 256;

// len / cu come from the mask the caller handed in: they are clamped to the tensors' extents (T, n_rows), so a mask that is not the
// collate's prefix mask gives meaningless numbers but no out-of-bounds access.
template <bool FROM_LOGITS>
__global__ void __launch_bounds__(RDS_THREADS) k_rd_score(const float4* __restrict__ logits, const int32_t* __restrict__ pred, int n_rows,
                                                          const int* __restrict__ len, const int* __restrict__ cu,
                                                          const int32_t* __restrict__ labels, int T, int32_t* __restrict__ correct,
                                                          int32_t* __restrict__ valid, float* __restrict__ nll, int32_t* __restrict__ pred_out) {
    __shared__ int s_c[RDS_THREADS / 64];
    __shared__ float s_l[RDS_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int off = min(max(cu[b], 0), n_rows);
    const int n = min(min(max(len[b], 0), T), n_rows - off);
    int c = 0;
    float l = 0.f;
    for (int t = tid; t < n; t += RDS_THREADS) {
        const int p = off + t;
        const int lab = labels[(size_t)b * T + t];
        int best;
        if (FROM_LOGITS) {
            const float4 x = logits[p];
            float m;
            best = sc_argmax(x, m);
            if (nll) {                                         // logsumexp(x) - x[label]
                const float se = expf(x.x - m) + expf(x.y - m) + expf(x.z - m) + expf(x.w - m);
                const float xl = lab == 0 ? x.x : lab == 1 ? x.y : lab == 2 ? x.z : x.w;
                l += (m - xl) + logf(se);
            }
        } else {
            best = pred[p];
        }
        c += best == lab ? 1 : 0;
        if (pred_out) pred_out[p] = best;
    }
    c = sc_wave_sum(c);
    l = sc_wave_sum(l);
    if ((tid & 63) == 0) { s_c[tid >> 6] = c; s_l[tid >> 6] = l; }
    __syncthreads();
    if (tid == 0) {
        int ct = 0;
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < RDS_THREADS / 64; ++w) { ct += s_c[w]; lt += s_l[w]; }
        correct[b] = ct;
        valid[b] = n;
        if (nll) nll[b] = lt;
    }
}

size_t rds_ints(int B) { return ((size_t)2 * B + 1 + 63) / 64 * 64; }     // len [B], cu [B + 1]
}  // namespace

extern "C" size_t rdesign_score_workspace_bytes(int32_t B) {
    return B > 0 ? rds_ints(B) * sizeof(int) : 0;
}

extern "C" int rdesign_score(const float* logits, const int32_t* pred, int32_t n_rows, const float* mask, const int32_t* labels, int32_t B,
                             int32_t T, int32_t* correct, int32_t* valid, float* nll, int32_t* pred_out, void* ws, size_t ws_bytes,
                             void* stream) {
    if ((logits != nullptr) == (pred != nullptr)) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: pass exactly one of logits and pred");
    if (B <= 0 || T <= 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: empty batch (B = %d, T = %d)", (int)B, (int)T);
    if (!mask || !labels || !correct || !valid || !ws || n_rows < 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: null pointer or negative row count");
    if (pred && nll) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: nll needs logits (class ids carry no likelihood)");
    if (logits && ((uintptr_t)logits & 15) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: logits must be 16-byte aligned");
    if (((uintptr_t)ws & 15) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_score: workspace must be 16-byte aligned");
    if (ws_bytes < rdesign_score_workspace_bytes(B)) return rd_fail(RDESIGN_ERR_WORKSPACE, "rdesign_score: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    PackInfo pk{};
    pk.len = (int*)ws; pk.cu = pk.len + B; pk.node_b = nullptr; pk.B = B; pk.T = T; pk.Nmax = n_rows; pk.packed_in = 0;
    launch_lengths(mask, pk, s);
    if (logits)
        hipLaunchKernelGGL(k_rd_score<true>, dim3(B), dim3(RDS_THREADS), 0, s, reinterpret_cast<const float4*>(logits), nullptr, n_rows, pk.len,
                           pk.cu, labels, T, correct, valid, nll, pred_out);
    else
        hipLaunchKernelGGL(k_rd_score<false>, dim3(B), dim3(RDS_THREADS), 0, s, nullptr, pred, n_rows, pk.len, pk.cu, labels, T, correct, valid,
                           nullptr, pred_out);
    RD_TRY(hipGetLastError());
    return RDESIGN_OK;
}
