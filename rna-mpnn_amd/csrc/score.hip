// rnampnn_score: the per-RNA metrics of RNAMPNN.validation_step / test_step (rnampnn.py:209-236 of the reference: argmax of the read-out
// against the labels, recovery per RNA, mix_loss = cross-entropy applied to the softmax PROBABILITIES, rnampnn.py:151-154) and the
// likelihood of given sequences, on the device, from f32 logits in the padded (B,T,4) + prefix-mask layout rnampnn_forward writes or the
// packed (N,4) + cu_seqlens layout rnampnn_forward_packed writes.  A sibling of rdesign_score.hip: one 256-thread workgroup per
// (RNA, pass) - pass 0 scores the labels, pass 1 + s the candidate sequence s - a thread walks its rows in ascending order (one 16-byte
// load per row), then a wave butterfly and one LDS hop over the four waves: a fixed order that depends on the RNA's length only, so the two
// layouts give the same bytes for the same rows and two calls give identical bytes.  ONE launch: the workgroup finds its own length (the
// sum of its mask row, or the difference of two cu entries), so there is no workspace, no runtime fill / copy node, no atomics and no host
// synchronisation.  About 20 bytes per nucleotide and pass: the call is bounded by its launch, not by bandwidth.
#include "score_dev.h"

namespace {
struct ScoreArgs : ScRows {
    const int32_t* labels;       // (B,T) or null
    const int8_t* seqs;          // (S,B,T) or null
    int S;
    int pass0;                   // 1: pass 0 (the label / decode pass) has an output to write
    int32_t* valid;              // (B)
    int8_t* pred;                // (B,T)
    int32_t* correct;            // (B)
    float* label_nll;            // (B)
    float* label_loss;           // (B)
    float* seq_nll;              // (S,B)
    int32_t* seq_match;          // (S,B)
};

__global__ void __launch_bounds__(SC_THREADS) k_score(ScoreArgs a) {
    __shared__ int s_i[SC_WAVES];
    __shared__ float s_f[2][SC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pass = (int)blockIdx.y + (a.pass0 ? 0 : 1);
    int n;
    long long row0;
    sc_extent(a, b, tid, s_f[0], n, row0);
    const size_t lab0 = (size_t)b * a.T;
    int cnt = 0;
    float nll = 0.f, loss = 0.f;
    if (pass == 0) {
        for (int t = tid; t < n; t += SC_THREADS) {
            const float4 x = a.logits[row0 + t];
            float m;
            const int best = sc_argmax(x, m);
            if (a.pred) a.pred[lab0 + t] = (int8_t)best;
            if (a.labels) {
                const int lab = a.labels[lab0 + t];
                cnt += best == lab ? 1 : 0;
                if (a.label_nll || a.label_loss) {
                    const float e0 = expf(x.x - m), e1 = expf(x.y - m), e2 = expf(x.z - m), e3 = expf(x.w - m);
                    const float se = (e0 + e1) + (e2 + e3);
                    const float xl = lab == 0 ? x.x : lab == 1 ? x.y : lab == 2 ? x.z : x.w;
                    nll += (m - xl) + logf(se);                // logsumexp(x) - x[label]
                    const float inv = 1.0f / se;               // mix_loss: -log_softmax(softmax(x))[label]; the probabilities lie in [0, 1]
                    const float p0 = e0 * inv, p1 = e1 * inv, p2 = e2 * inv, p3 = e3 * inv;
                    const float pl = lab == 0 ? p0 : lab == 1 ? p1 : lab == 2 ? p2 : p3;
                    loss += logf((expf(p0) + expf(p1)) + (expf(p2) + expf(p3))) - pl;
                }
            }
        }
        if (a.pred)
            for (int t = n + tid; t < a.T; t += SC_THREADS) a.pred[lab0 + t] = (int8_t)-1;
    } else {
        const int8_t* seq = a.seqs + ((size_t)(pass - 1) * a.B + b) * a.T;
        for (int t = tid; t < n; t += SC_THREADS) {
            const int q = seq[t];
            if (a.seq_nll) nll += sc_row_nll(a.logits[row0 + t], q);
            if (a.seq_match) cnt += q == a.labels[lab0 + t] ? 1 : 0;
        }
    }
    sc_block_sums(cnt, nll, loss, tid, s_i, s_f);
    if (tid != 0) return;
    const int ct = cnt;
    const float nt = nll, lt = loss;
    if (pass == 0) {
        if (a.valid) a.valid[b] = n;
        if (a.correct) a.correct[b] = ct;
        if (a.label_nll) a.label_nll[b] = nt;
        if (a.label_loss) a.label_loss[b] = lt;
    } else {
        const size_t o = (size_t)(pass - 1) * a.B + b;
        if (a.seq_nll) a.seq_nll[o] = nt;
        if (a.seq_match) a.seq_match[o] = ct;
    }
}
}  // namespace

extern "C" int rnampnn_score(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, const int32_t* labels,
                             const int8_t* seqs, int32_t S, int32_t B, int32_t T, int32_t* valid, int8_t* pred, int32_t* correct,
                             float* label_nll, float* label_loss, float* seq_nll, int32_t* seq_match, void* stream) {
    ScoreArgs a{};
    const int rc = sc_check_args("rnampnn_score", logits, n_rows, mask, cu_seqlens, B, T, nullptr, a, [&](int slot) {
        if (slot != 1) return RNAMPNN_OK;
        if (S < 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_score: S = %d candidate sequences", (int)S);
        if ((S > 0) != (seqs != nullptr)) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_score: seqs and S > 0 go together");
        if ((seq_nll || seq_match) && !seqs) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_score: seq_nll / seq_match need seqs");
        if ((correct || seq_match || label_nll || label_loss) && !labels)
            return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_score: correct / seq_match / label_nll / label_loss need labels");
        return RNAMPNN_OK;
    });
    if (rc != RNAMPNN_OK) return rc;
    if (S + 1 > 65535) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_score: at most 65534 sequences per call");
    a.labels = labels; a.seqs = seqs; a.S = S;
    a.pass0 = (valid || pred || correct || label_nll || label_loss) ? 1 : 0;
    a.valid = valid; a.pred = pred; a.correct = correct; a.label_nll = label_nll; a.label_loss = label_loss;
    a.seq_nll = seq_nll; a.seq_match = seq_match;
    const int passes = a.pass0 + ((seq_nll || seq_match) ? S : 0);
    if (passes == 0) return RNAMPNN_OK;                        // nothing asked for
    hipLaunchKernelGGL(k_score, dim3(B, passes), dim3(SC_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
