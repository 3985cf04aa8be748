// Training path of librnampnn_hip.so (the handle and the model structure come from api_internal.h): taped f32 forward and the gradient of every
// parameter.  Reference surface: RNAMPNN.training_step (rnampnn.py:187-207) + Lightning's `loss.backward()`:
//   rnampnn_train_forward  = `self(coords, mask)` in train mode: dropout p after every GELU and on the attention
//                            probabilities (mpnn.py:140,150; feature.py:200; functional.py:69,109,124,184), masks from a
//                            counter hash of (seed, site, element) that the CPU oracle restates bit for bit;
//   rnampnn_train_backward = backward from d loss / d logits (any loss the caller built with autograd);
//   rnampnn_loss_and_grad  = both around the reference loss softmax -> cross_entropy(probs, label) (double softmax,
//                            rnampnn.py:151-154), mean over valid nucleotides.
// The forward is the "taped" variant: it materialises per-edge pre-activations so the backward can walk them with
// generic row kernels (kernels_train.hip); the tape lives in the caller's workspace between the two calls.
// Gradients land in a flat f32 buffer laid out like the weight arena (rnampnn_weight_offset), ready for ONE RCCL
// all-reduce.  Every cross-workgroup sum is an ordered two-stage reduction: gradients are bit-reproducible.
// Layout of this file: workspace and small entry points; the node-level helpers (one dispatch per GEMM: MFMA form when the shape is covered, f32
// kernel otherwise); the edge side TWICE, once per precision (f32, bf16-mixed: edge embedding, per-edge MLPs, layer loops - each readable top to
// bottom without a precision flag); the shared forward / backward skeletons that pick one of the two; the C entry points.
#include "api_internal.h"

// dropout sites (must match oracle/rnampnn_oracle.py: SITE_*)
static inline unsigned site_ee(int i) { return 1u + i; }
static inline unsigned site_emb_ffn(int i) { return 10u + i; }
static inline unsigned site_emb_att(int j) { return 20u + j; }
static inline unsigned site_post_ffn(int i) { return 30u + i; }
static inline unsigned site_post_att(int j) { return 40u + j; }
static inline unsigned site_raw(int i) { return 50u + i; }
static inline unsigned site_ro(int i) { return 60u + i; }
static inline unsigned site_msg(int l, int i) { return 100u + 4u * l + i; }
static inline unsigned site_edge(int l, int i) { return 102u + 4u * l + i; }

struct BertTape { std::vector<float*> qkv, o, t, x, st; std::vector<float*> pre; };      // st: softmax statistics [N][heads][3] per attention layer
struct TW {                        // training workspace
    int *len, *cu, *node_b, *nbr;
    int *rdeg, *rstart, *rfill, *rlist;   // reverse adjacency of the k-NN graph (t_build_reverse)
    float *geom, *raw_p;
    TScratch sc;                          // arena of the backward's ordered reductions (red_begin); the loss partials before it
    // tape
    float *F, *pe1, *pe2;
    std::vector<float*> e, pm1, pm2, pu1, pu2, h, hpre;
    float *x0, *n1;
    BertTape emb, post;
    std::vector<float*> raw_pre, ro_pre;
    float *r1, *re, *hp, *logits_p;
    // scratch
    float *pq, *act, *dA, *dB, *E1, *E2, *dE, *dpq, *dh, *dh2, *dqkv, *stat, *dlogits, *dhp, *dre, *nscr;
    float *invc;                          // 1 / #valid neighbours per residue (bf16-mixed backward)
    size_t total;
};

static size_t carve_train(const rnampnn_ctx* c, int B, int T, char* base, TW* out) {
    size_t off = 0;
    auto takeb = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return base ? base + o : (char*)nullptr; };
    auto takef = [&](size_t floats) { return (float*)takeb(floats * sizeof(float)); };
    const RnaMpnnConfig& g = c->cfg;
    const size_t N = (size_t)B * T, k = g.num_res_neighbours, E = N * k, D = RN_D, F = c->fmax;
    const int L = g.num_res_mpnn_layers;
    TW tmp;
    TW& w = out ? *out : tmp;
    w.len = (int*)takeb(B * sizeof(int)); w.cu = (int*)takeb((B + 1) * sizeof(int)); w.node_b = (int*)takeb(N * sizeof(int));
    w.nbr = (int*)takeb(E * sizeof(int));
    w.rdeg = (int*)takeb((N + 1) * sizeof(int)); w.rstart = (int*)takeb((N + 1) * sizeof(int));
    w.rfill = (int*)takeb((N + 1) * sizeof(int)); w.rlist = (int*)takeb(E * sizeof(int));
    // 256 MB: four producer budgets (RED_VIEW) of the backward's batched reductions, and never less than the largest single extent (a budget, or
    // t_gn_bwd's B * 256 per-RNA partials)
    w.sc.floats = 4 * RED_VIEW;
    if (w.sc.floats < (size_t)B * 256 + 4096) w.sc.floats = (size_t)B * 256 + 4096;
    w.sc.p = takef(w.sc.floats);
    w.geom = takef((N + B) * RN_GEOM); w.raw_p = takef(N * RN_RAWP);
    w.F = takef(E * RN_ERAWP); w.pe1 = takef(E * D); w.pe2 = takef(E * D);
    w.e.assign(L, nullptr); w.pm1.assign(L, nullptr); w.pm2.assign(L, nullptr); w.pu1.assign(L, nullptr); w.pu2.assign(L, nullptr);
    w.h.assign(L + 1, nullptr); w.hpre.assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        w.e[l] = takef(E * D); w.pm1[l] = takef(E * D); w.pm2[l] = takef(E * D);
        if (l + 1 < L) { w.pu1[l] = takef(E * D); w.pu2[l] = takef(E * D); }
        w.hpre[l] = takef(N * D);
    }
    for (int l = 0; l <= L; ++l) w.h[l] = takef((N + 1) * D);
    w.x0 = takef(N * D); w.n1 = takef(N * D);
    auto bert = [&](const Bert& b, BertTape& t) {
        size_t J = b.attn.size();
        t.qkv.assign(J, nullptr); t.o.assign(J, nullptr); t.t.assign(J, nullptr); t.x.assign(J + 1, nullptr); t.st.assign(J, nullptr);
        for (size_t j = 0; j < J; ++j) { t.qkv[j] = takef(N * 3 * D); t.o[j] = takef(N * D); t.t[j] = takef(N * D); t.x[j + 1] = takef(N * D); t.st[j] = takef(N * 16 * 3); }
        t.pre.assign(b.ffn.size() - 1, nullptr);
        for (size_t i = 0; i + 1 < b.ffn.size(); ++i) t.pre[i] = takef(N * b.ffn[i].out);
    };
    bert(c->emb, w.emb);
    bert(c->post, w.post);
    w.emb.x[0] = w.x0;             // inputs of the two RNABert stacks (the backward re-carves: nothing may live only in a forward-time copy)
    w.post.x[0] = w.h[L];
    w.raw_pre.assign(c->raw_ffn.size() - 1, nullptr);
    for (size_t i = 0; i + 1 < c->raw_ffn.size(); ++i) w.raw_pre[i] = takef(N * c->raw_ffn[i].out);
    w.ro_pre.assign(c->readout.size() - 1, nullptr);
    for (size_t i = 0; i + 1 < c->readout.size(); ++i) w.ro_pre[i] = takef(N * c->readout[i].out);
    w.r1 = takef(N * D); w.re = takef(N * D); w.hp = takef(N * D); w.logits_p = takef(N * 4);
    w.pq = takef((N + 1) * 256); w.act = takef(N * F); w.dA = takef(N * F); w.dB = takef(N * F);
    w.E1 = takef(E * D); w.E2 = takef(E * D); w.dE = takef(E * D); w.dpq = takef((N + 1) * 256);
    w.dh = takef(N * D); w.dh2 = takef(N * D); w.dqkv = takef(N * 3 * D); w.stat = takef(N * 16 * 3);
    w.dlogits = takef(N * 4); w.dhp = takef(N * D); w.dre = takef(N * D); w.nscr = takef(N * D);
    w.invc = takef(N + 1);
    w.total = off;
    return off;
}

extern "C" size_t rnampnn_train_workspace_bytes(rnampnn_handle h, int32_t B, int32_t T) {
    if (!h || B <= 0 || T <= 0) return 0;
    return carve_train(h, B, T, nullptr, nullptr);
}
extern "C" int64_t rnampnn_grad_numel(rnampnn_handle h) { return h ? (int64_t)h->raw_floats : 0; }
// Chunks of the flat gradient in the order the backward finishes them (registration order of the parameters is forward order,
// rnampnn.py:94-134, so each chunk is one contiguous range): 0 = [post_fusion .. readout], 1 = ResMPNN layers L/2 .. L-1,
// 2 = everything before (final only at the end of the backward).  begin / end: float offsets, 3 entries each.
extern "C" int rnampnn_grad_chunks(rnampnn_handle h, int64_t* begin, int64_t* end) {
    if (!h || !begin || !end) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_grad_chunks: null argument");
    const int L = h->cfg.num_res_mpnn_layers;
    const int64_t total = (int64_t)h->raw_floats;
    const int64_t tail = (int64_t)h->raw[h->post.attn.empty() ? h->post.ffn[0].w : h->post.attn[0].qkv.w].off;
    const int64_t mid = (int64_t)h->raw[h->mpnn[L / 2].gn_scale].off;
    begin[0] = tail; end[0] = total;
    begin[1] = mid;  end[1] = tail;
    begin[2] = 0;    end[2] = mid;
    return RNAMPNN_OK;
}
// seed_device != null: every later rnampnn_train_forward / rnampnn_loss_and_grad (and the backward of such a tape) reads the dropout seed
// from *seed_device at KERNEL time and ignores its `seed` argument - a captured training step replays with fresh masks.  null: back to
// the argument.  The word must stay unchanged between a forward and its backward.
extern "C" int rnampnn_set_seed_source(rnampnn_handle h, const uint64_t* seed_device) {
    if (!h) return fail(RNAMPNN_ERR_BAD_ARG, "null handle");
    h->seed_dev = reinterpret_cast<const unsigned long long*>(seed_device);
    return RNAMPNN_OK;
}
// ev0 / ev1: hipEvent_t handles (or null) recorded by every later backward on ITS stream when chunk 0 / chunk 1 is final.
extern "C" int rnampnn_set_grad_events(rnampnn_handle h, void* ev0, void* ev1) {
    if (!h) return fail(RNAMPNN_ERR_BAD_ARG, "null handle");
    h->grad_ev[0] = (hipEvent_t)ev0; h->grad_ev[1] = (hipEvent_t)ev1;
    return RNAMPNN_OK;
}
extern "C" int rnampnn_weight_offset(rnampnn_handle h, int32_t i, int64_t* offset) {
    if (!h || i < 0 || i >= (int)h->raw.size() || !offset) return fail(RNAMPNN_ERR_BAD_ARG, "weight index out of range");
    *offset = (int64_t)h->raw[i].off;
    return RNAMPNN_OK;
}

namespace {
struct Tr {                        // one training call
    rnampnn_ctx* c;
    PackInfo pk;
    TW w;
    TCall cx;                      // stream, the backward's reduction queue, the handle's weight-image cache (bf16-mixed)
    float* g;                      // flat gradient buffer (arena layout)
    int k, t_norm;
    TDrop dr;
    bool bad = false;              // a bf16-storage GEMM variant that is not instantiated was requested (reported at the end of the pass)
    bool mixed;                    // bf16-mixed: GEMMs on MFMA with bf16 operands / f32 accumulate (kernels_train.hip, second half)
    bool att_mfma = false;         // the MFMA attention kernels (bf16-mixed unless RNAMPNN_F32_ATTN=1); decided ONCE per forward and kept on the tape
    TRows rn() const { return TRows{pk.cu + pk.B, 1, pk.Nmax}; }
    TRows re() const { return TRows{pk.cu + pk.B, k, pk.Nmax * k}; }
    float* gw(int idx) const { return g + c->raw[idx].off; }
};

// The three GEMM shapes of the path.  f32 mode: plain FMA kernels (parity grade); mixed mode: MFMA, bf16 operands.
// Y = beta Y + X . W + bias            W [K][N] row-major (ldw)
void mm_nn(Tr& t, const TRows& rows, const float* X, int ldx, int K, const float* W, int ldw, const float* bias, int N,
           float* Y, int ldy, int beta) {
    if (t.mixed && tm_gemm_nn(rows, X, ldx, K, W, ldw, bias, N, Y, ldy, beta, nullptr, 0, t.dr, 0u, t.cx)) return;
    t_gemm(rows, X, ldx, K, W, ldw, bias, N, Y, ldy, beta, t.cx.s);
}
// Y = beta Y + X . W^T + bias          W [N][K] row-major (nn.Linear.weight); wt = its K-major copy for the f32 kernel
void mm_nt(Tr& t, const TRows& rows, const float* X, int ldx, int K, const float* W, int ldw, const float* wt, int ldwt,
           const float* bias, int N, float* Y, int ldy, int beta) {
    if (t.mixed && tm_gemm_nt(rows, X, ldx, K, W, ldw, bias, N, Y, ldy, beta, false, t.dr, 0u, t.cx)) return;
    t_gemm(rows, X, ldx, K, wt, ldwt, bias, N, Y, ldy, beta, t.cx.s);
}
// dW += A^T B                          (contraction over the rows; ordered two-stage reduction in both modes)
// dbias (optional) += column sums of A: the bias gradient of the same Linear (fused into the MFMA kernel's staging pass)
void mm_tn(Tr& t, const TRows& rows, const float* A, int lda, int M, const float* B, int ldb, int K, float* dW, int ldw,
           float* dbias = nullptr) {
    if (t.mixed && tm_gemm_tn(rows, A, lda, M, B, ldb, K, dW, ldw, false, t.dr, 0u, dbias, t.cx)) return;
    t_gemm_tn(rows, A, lda, M, B, ldb, K, dW, ldw, t.cx);
    if (dbias) t_colsum(rows, A, lda, M, dbias, t.cx);
}

void lin_fwd(Tr& t, const Lin& l, const float* X, int ldx, float* Y, int ldy) {
    // (X carries in_pad columns; the weight has `in`: when they differ - the 28 raw features - the MFMA form is skipped)
    const bool mm = t.mixed && l.in == l.in_pad;
    if (mm && tm_gemm_nt(t.rn(), X, ldx, l.in, rawp(t.c, l.w), l.in, rawp(t.c, l.b), l.out, Y, ldy, 0, false, t.dr, 0u, t.cx)) return;
    t_gemm(t.rn(), X, ldx, l.in_pad, derp<float>(t.c, l.wt), l.out, rawp(t.c, l.b), l.out, Y, ldy, 0, t.cx.s);
}
// dX (optional) = dY . W ; dW += dY^T X ; db += colsum(dY)
void lin_bwd(Tr& t, const Lin& l, const float* X, int ldx, const float* dY, int lddy, float* dX, int lddx) {
    if (dX) mm_nn(t, t.rn(), dY, lddy, l.out, rawp(t.c, l.w), l.in, nullptr, l.in, dX, lddx, 0);
    mm_tn(t, t.rn(), dY, lddy, l.out, X, ldx, l.in, t.gw(l.w), l.in, t.gw(l.b));
}

// FFN chain forward with pre-activation tape; last layer writes `out`.  Mixed mode: a1 = drop(gelu(pre)) is formed while the next
// Linear loads its operand (no activation tensor, no element-wise launch); the explicit form stays for the f32 path and odd shapes.
static inline bool fusable(const Lin& l, const float* pre, int ld) {
    return l.in == l.in_pad && l.in % 16 == 0 && ld == l.in && ld % 4 == 0 && (((uintptr_t)pre) & 15) == 0;
}
void ffn_fwd(Tr& t, const std::vector<Lin>& L, const float* X, int ldx, std::vector<float*>& pre, float* out, unsigned site0) {
    const float* cur = X;
    int ld = ldx;
    bool cur_is_pre = false;               // `cur` is a taped pre-activation whose GELU + dropout is still to be applied
    for (size_t i = 0; i < L.size(); ++i) {
        bool last = i + 1 == L.size();
        float* dst = last ? out : pre[i];
        if (cur_is_pre) {
            if (t.mixed && fusable(L[i], cur, ld) &&
                tm_gemm_nt(t.rn(), cur, ld, L[i].in, rawp(t.c, L[i].w), L[i].in, rawp(t.c, L[i].b), L[i].out, dst, L[i].out, 0, true, t.dr,
                           site0 + (unsigned)(i - 1), t.cx)) {
                cur = dst; ld = L[i].out; cur_is_pre = true;
                continue;
            }
            t_gelu_fwd(t.rn(), cur, t.w.act, ld, t.dr, site0 + (unsigned)(i - 1), t.cx.s);
            cur = t.w.act;
        }
        lin_fwd(t, L[i], cur, ld, dst, L[i].out);
        cur = dst; ld = L[i].out; cur_is_pre = true;
    }
}
// backward of the chain; dOut [N][L.back().out] is consumed; dX (optional, [N][lddx]) receives the input gradient
void ffn_bwd(Tr& t, const std::vector<Lin>& L, const float* X, int ldx, const std::vector<float*>& pre, const float* dOut,
             float* dX, int lddx, unsigned site0) {
    const float* d = dOut;
    float* bufs[2] = {t.w.dA, t.w.dB};
    for (int i = (int)L.size() - 1; i >= 0; --i) {
        float* din = i == 0 ? dX : bufs[i & 1];
        const unsigned site = site0 + (unsigned)(i - 1);
        // dW += dY^T drop(gelu(pre)), db += colsum(dY): the activation recomputed in the staging pass;  d pre = (dY . W) gelu'(pre) mask
        if (i > 0 && t.mixed && fusable(L[i], pre[i - 1], L[i - 1].out) && L[i].out % 16 == 0 && (((uintptr_t)d) & 15) == 0 &&
            tm_gemm_tn(t.rn(), d, L[i].out, L[i].out, pre[i - 1], L[i].in, L[i].in, t.gw(L[i].w), L[i].in, true, t.dr, site, t.gw(L[i].b), t.cx)) {
            if (tm_gemm_nn(t.rn(), d, L[i].out, L[i].out, rawp(t.c, L[i].w), L[i].in, nullptr, L[i].in, din, L[i].in, 0, pre[i - 1], L[i].in, t.dr, site, t.cx)) {
                d = din;
                continue;
            }
            mm_nn(t, t.rn(), d, L[i].out, L[i].out, rawp(t.c, L[i].w), L[i].in, nullptr, L[i].in, din, L[i].in, 0);
            t_gelu_bwd(t.rn(), din, pre[i - 1], din, L[i - 1].out, t.dr, site, t.cx.s);
            d = din;
            continue;
        }
        const float* in;
        int ldin;
        if (i == 0) { in = X; ldin = ldx; }
        else { t_gelu_fwd(t.rn(), pre[i - 1], t.w.act, L[i - 1].out, t.dr, site, t.cx.s); in = t.w.act; ldin = L[i - 1].out; }
        lin_bwd(t, L[i], in, ldin, d, L[i].out, din, i == 0 ? lddx : L[i].in);
        if (i > 0) { t_gelu_bwd(t.rn(), din, pre[i - 1], din, L[i - 1].out, t.dr, site, t.cx.s); d = din; }
    }
}

// RNAMPNN_F32_ATTN is read when a FORWARD starts (tests flip it inside one process); the backward of that forward takes the value from the tape:
// with tapes outliving a call (leases, several outstanding forwards) an environment flip in between would otherwise recompute S from other
// operands than the taped (m, l) statistics belong to
static inline bool att_mfma_env(bool mixed) { return mixed && !ab_switch("RNAMPNN_F32_ATTN"); }
int bert_fwd(Tr& t, const Bert& b, BertTape& tp, float* x_in, float* out, unsigned site_att0, unsigned site_ffn0) {
    tp.x[0] = x_in;
    for (size_t j = 0; j < b.attn.size(); ++j) {
        const Attn& a = b.attn[j];
        lin_fwd(t, a.qkv, tp.x[j], RN_D, tp.qkv[j], 3 * RN_D);
        // bf16-mixed: the MFMA attention (forward and backward recompute S from the same bf16 operands); RNAMPNN_F32_ATTN=1 keeps the f32 kernels (A/B)
        if (!(t.att_mfma && te_attention_fwd(t.pk, tp.qkv[j], b.heads, tp.o[j], tp.st[j], t.dr, site_att0 + (unsigned)j, t.cx.s) == 0))
            if (t_attention_fwd(t.pk, tp.qkv[j], b.heads, tp.o[j], tp.st[j], t.dr, site_att0 + (unsigned)j, t.cx.s)) return 1;
        lin_fwd(t, a.out, tp.o[j], RN_D, tp.t[j], RN_D);
        t_add(t.rn(), tp.x[j], tp.t[j], RN_D, t.cx.s);                                          // residual (functional.py:165)
        launch_graph_norm_packed(t.pk, tp.t[j], tp.x[j + 1], rawp(t.c, a.gn_scale), rawp(t.c, a.gn_shift),
                                 t.c->cfg.padding_len, t.cx.s);
    }
    ffn_fwd(t, b.ffn, tp.x[b.attn.size()], RN_D, tp.pre, out, site_ffn0);
    return 0;
}
// dOut [N][128] -> dIn [N][128] (written to `dIn`)
int bert_bwd(Tr& t, const Bert& b, BertTape& tp, const float* dOut, float* dIn, unsigned site_att0, unsigned site_ffn0) {
    const size_t J = b.attn.size();
    ffn_bwd(t, b.ffn, tp.x[J], RN_D, tp.pre, dOut, dIn, RN_D, site_ffn0);
    for (int j = (int)J - 1; j >= 0; --j) {
        const Attn& a = b.attn[j];
        // GraphNorm backward: dIn = d x[j+1]  ->  nscr = d t[j]
        t_gn_bwd(t.pk, tp.t[j], dIn, rawp(t.c, a.gn_scale), t.c->cfg.padding_len, t.w.nscr, t.gw(a.gn_scale), t.gw(a.gn_shift), t.cx);
        // out_proj backward: d o = d t . Wout
        lin_bwd(t, a.out, tp.o[j], RN_D, t.w.nscr, RN_D, t.w.dh2, RN_D);
        if (!(t.att_mfma && te_attention_bwd(t.pk, tp.qkv[j], tp.o[j], t.w.dh2, b.heads, t.w.dqkv, tp.st[j], t.dr, site_att0 + (unsigned)j, t.cx.s) == 0))
            if (t_attention_bwd(t.pk, tp.qkv[j], tp.o[j], t.w.dh2, b.heads, t.w.dqkv, tp.st[j], t.dr, site_att0 + (unsigned)j, t.cx.s)) return 1;
        lin_bwd(t, a.qkv, tp.x[j], RN_D, t.w.dqkv, 3 * RN_D, dIn, RN_D);                     // d x[j] (through q,k,v)
        t_add(t.rn(), t.w.nscr, dIn, RN_D, t.cx.s);                                              // + residual path
    }
    return 0;
}

// ================================================================ edge side, f32: every [E][128] tensor of the tape and the scratch is f32; the
// GEMMs are the plain FMA kernels on the K-major weight copies rnampnn_finalize_weights builds (parity grade)
// one per-edge MLP on the tape:  pre1 = e.Wc + P[i] + Q[j] ; pre2 = gelu(pre1).W2^T + b2
void mlp_edge_fwd(Tr& t, const Mlp2& m, const float* h, const float* e, float* pre1, float* pre2, unsigned site0) {
    rnampnn_ctx* c = t.c;
    t_gemm(t.rn(), h, RN_D, RN_D, derp<float>(c, m.pq_t), 256, derp<float>(c, m.pq_b), 256, t.w.pq, 256, 0, t.cx.s);   // [P | Q] = h [Wa | Wb]^T + [b1 | 0]
    t_gemm(t.re(), e, RN_D, RN_D, derp<float>(c, m.wc_t), RN_D, nullptr, RN_D, pre1, RN_D, 0, t.cx.s);
    t_edge_add_pq(t.pk, t.k, t.w.nbr, t.w.pq, pre1, t.cx.s);
    if (m.depth > 1) {
        t_gelu_fwd(t.re(), pre1, t.w.E1, RN_D, t.dr, site0, t.cx.s);
        t_gemm(t.re(), t.w.E1, RN_D, RN_D, derp<float>(c, m.w2_t), RN_D, rawp(c, m.b[1]), RN_D, pre2, RN_D, 0, t.cx.s);
    }
}
// backward of one per-edge MLP.  On entry E2 holds d(pre_last) [E][128] (already multiplied by gelu' of the
// last pre-activation and masked).  Accumulates: parameter grads, dE += d e, dh_acc += d h.
void mlp_edge_bwd(Tr& t, const Mlp2& m, const float* h, const float* e, const float* pre1, float* dE, float* dh_acc, unsigned site0) {
    rnampnn_ctx* c = t.c;
    float* dpre1 = t.w.E2;
    if (m.depth > 1) {
        // E2 = d pre2 ; a1 = gelu(pre1) -> E1
        t_gelu_fwd(t.re(), pre1, t.w.E1, RN_D, t.dr, site0, t.cx.s);
        mm_tn(t, t.re(), t.w.E2, RN_D, RN_D, t.w.E1, RN_D, RN_D, t.gw(m.w[1]), RN_D, t.gw(m.b[1]));  // dW2 += dpre2^T a1, db2
        mm_nn(t, t.re(), t.w.E2, RN_D, RN_D, rawp(c, m.w[1]), RN_D, nullptr, RN_D, t.w.E1, RN_D, 0);  // d a1 = dpre2 . W2
        t_gelu_bwd(t.re(), t.w.E1, pre1, t.w.E1, RN_D, t.dr, site0, t.cx.s);                           // d pre1
        dpre1 = t.w.E1;
    }
    float* gw0 = t.gw(m.w[0]);                     // [128][384] = [Wa | Wb | Wc]
    const float* w0 = rawp(c, m.w[0]);
    mm_tn(t, t.re(), dpre1, RN_D, RN_D, e, RN_D, RN_D, gw0 + 2 * RN_D, 3 * RN_D);                  // dWc += dpre1^T e
    mm_nn(t, t.re(), dpre1, RN_D, RN_D, w0 + 2 * RN_D, 3 * RN_D, nullptr, RN_D, dE, RN_D, 1);      // dE += dpre1 . Wc
    t_edge_pq_bwd(t.pk, t.k, dpre1, t.w.rstart, t.w.rlist, t.w.dpq, t.cx.s);                          // dP (segment sum), dQ (gather over incoming edges)
    mm_tn(t, t.rn(), t.w.dpq, 256, RN_D, h, RN_D, RN_D, gw0, 3 * RN_D, t.gw(m.b[0]));              // dWa += dP^T h, db1 += sum dP
    mm_tn(t, t.rn(), t.w.dpq + RN_D, 256, RN_D, h, RN_D, RN_D, gw0 + RN_D, 3 * RN_D);              // dWb += dQ^T h
    mm_nn(t, t.rn(), t.w.dpq, 256, RN_D, w0, 3 * RN_D, nullptr, RN_D, dh_acc, RN_D, 1);            // dh += dP . Wa
    mm_nn(t, t.rn(), t.w.dpq + RN_D, 256, RN_D, w0 + RN_D, 3 * RN_D, nullptr, RN_D, dh_acc, RN_D, 1);   // dh += dQ . Wb
}
// edge embedding (feature.py:540-571): raw features F [E][96] -> pe1 [-> pe2] -> e[0], absent slots zeroed
void edge_embed_fwd_f32(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int k = t.k;
    t_edge_features(t.pk, k, w.geom, w.nbr, w.F, s);
    const Lin& ee0 = c->edge_embed[0];
    mm_nn(t, t.re(), w.F, RN_ERAWP, RN_ERAWP, derp<float>(c, ee0.wt), RN_D, rawp(c, ee0.b), RN_D, w.pe1, RN_D, 0);   // K-major copy: 90 -> 96 padded
    if (c->cfg.depth_res_edge_feature > 1) {
        const Lin& ee1 = c->edge_embed[1];
        t_gelu_fwd(t.re(), w.pe1, w.E1, RN_D, t.dr, site_ee(0), s);
        mm_nt(t, t.re(), w.E1, RN_D, RN_D, rawp(c, ee1.w), RN_D, derp<float>(c, ee1.wt), RN_D, rawp(c, ee1.b), RN_D, w.pe2, RN_D, 0);
        t_gelu_fwd(t.re(), w.pe2, w.e[0], RN_D, t.dr, site_ee(1), s);
    } else {
        t_gelu_fwd(t.re(), w.pe1, w.e[0], RN_D, t.dr, site_ee(0), s);
    }
    t_edge_zero_invalid(t.pk, k, w.nbr, w.e[0], s);
}
// ResMPNN layers (mpnn.py:283-294)
void layers_fwd_f32(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    for (int l = 0; l < L; ++l) {
        const MpnnLayer& m = c->mpnn[l];
        mlp_edge_fwd(t, m.msg, w.h[l], w.e[l], w.pm1[l], w.pm2[l], site_msg(l, 0));
        t_seg_mean(t.pk, k, w.nbr, m.msg.depth > 1 ? w.pm2[l] : w.pm1[l], w.h[l], w.hpre[l], t.dr, site_msg(l, m.msg.depth - 1), s);
        launch_graph_norm_packed(t.pk, w.hpre[l], w.h[l + 1], rawp(c, m.gn_scale), rawp(c, m.gn_shift), t.t_norm, s);
        if (l + 1 < L) {
            mlp_edge_fwd(t, m.edge, w.h[l + 1], w.e[l], w.pu1[l], w.pu2[l], site_edge(l, 0));
            t_edge_residual(t.pk, k, w.nbr, w.e[l], m.edge.depth > 1 ? w.pu2[l] : w.pu1[l], w.e[l + 1], t.dr, site_edge(l, m.edge.depth - 1), s);
        }
    }
}
// backward of layers l_hi .. l_lo (descending).  On entry dh = d h[l_hi + 1], dE = d e[l_hi + 1]; on return dh = d h[l_lo], dE = d e[l_lo]
void layers_bwd_f32(Tr& t, int l_hi, int l_lo) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    const size_t N = (size_t)t.pk.Nmax;
    for (int l = l_hi; l >= l_lo; --l) {
        const MpnnLayer& m = c->mpnn[l];
        if (l + 1 < L) {     // edge update of layer l: e[l+1] = e[l] + drop(gelu(pre_last)) (valid slots); inputs h[l+1], e[l]
            const float* plast = m.edge.depth > 1 ? w.pu2[l] : w.pu1[l];
            t_edge_res_bwd(t.pk, k, w.nbr, w.dE, plast, w.E2, t.dr, site_edge(l, m.edge.depth - 1), s);   // E2 = d pre_last ; dE stays = identity path into e[l]
            mlp_edge_bwd(t, m.edge, w.h[l + 1], w.e[l], w.pu1[l], w.dE, w.dh, site_edge(l, 0));
        }
        // GraphNorm: dh = d h[l+1] -> dh2 = d hpre[l]
        t_gn_bwd(t.pk, w.hpre[l], w.dh, rawp(c, m.gn_scale), t.t_norm, w.dh2, t.gw(m.gn_scale), t.gw(m.gn_shift), t.cx);
        // hpre = h[l] + agg: d h[l] starts as dh2; messages get d agg = dh2
        const float* plast = m.msg.depth > 1 ? w.pm2[l] : w.pm1[l];
        t_seg_mean_bwd(t.pk, k, w.nbr, w.dh2, plast, w.E2, t.dr, site_msg(l, m.msg.depth - 1), s);        // E2 = d pre_last of the message MLP
        launch_copy_bytes(w.dh, w.dh2, N * RN_D * sizeof(float), s);
        mlp_edge_bwd(t, m.msg, w.h[l], w.e[l], w.pm1[l], w.dE, w.dh, site_msg(l, 0));
    }
}
// ResFeature, edge side: dE = d e[0] (masked output of the embedding MLP)
void edge_embed_bwd_f32(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const Lin& ee0 = c->edge_embed[0];
    t_edge_zero_invalid(t.pk, t.k, w.nbr, w.dE, s);
    if (c->cfg.depth_res_edge_feature > 1) {
        const Lin& ee1 = c->edge_embed[1];
        t_gelu_bwd(t.re(), w.dE, w.pe2, w.E2, RN_D, t.dr, site_ee(1), s);                      // d pe2
        t_gelu_fwd(t.re(), w.pe1, w.E1, RN_D, t.dr, site_ee(0), s);
        mm_tn(t, t.re(), w.E2, RN_D, RN_D, w.E1, RN_D, RN_D, t.gw(ee1.w), RN_D, t.gw(ee1.b));
        mm_nn(t, t.re(), w.E2, RN_D, RN_D, rawp(c, ee1.w), RN_D, nullptr, RN_D, w.E1, RN_D, 0);
        t_gelu_bwd(t.re(), w.E1, w.pe1, w.E1, RN_D, t.dr, site_ee(0), s);                      // d pe1
    } else {
        t_gelu_bwd(t.re(), w.dE, w.pe1, w.E1, RN_D, t.dr, site_ee(0), s);
    }
    mm_tn(t, t.re(), w.E1, RN_D, RN_D, w.F, RN_ERAWP, RN_ERAW, t.gw(ee0.w), RN_ERAW, t.gw(ee0.b));
}

// ================================================================ edge side, bf16-mixed: every [E][128] tensor is bf16 in HBM - the layout of every
// w.F / w.pe / w.e / w.pm / w.pu tensor and of E1, E2, dE in this mode (kernels_train.h, last part); P + Q and the edge update's residual
// ride in the GEMM epilogues, so a forward MLP is two passes: (read e, write pre1) and (read pre1, write pre2 [, read e, write e_out]).
inline tb16* eb(float* p) { return reinterpret_cast<tb16*>(p); }
inline const tb16* eb(const float* p) { return reinterpret_cast<const tb16*>(p); }
// bf16-mixed, depth-2 per-edge MLPs on the fused kernels: the pre2 tapes (pu2, pm2) hold gelu'(pre2) * mask - all the backward needs of them -
// written by the forward where it evaluates the activation anyway (k_emm_fwd2's edge update; k_eseg_mean, in place).
void mlp_edge_fwd_mixed(Tr& t, const Mlp2& m, const float* h, const tb16* e, tb16* pre1, tb16* pre2, unsigned site0,
                        tb16* res_out, unsigned site_res) {
    rnampnn_ctx* c = t.c;
    const float* w0 = rawp(c, m.w[0]);             // [128][384] = [Wa | Wb | Wc]
    // P = h Wa^T + b1 and Q = h Wb^T as bf16 tables [N+1][128] inside the pq buffer (row N of Q stays zero: absent neighbours)
    tb16* Pt = eb(t.w.pq);
    tb16* Qt = Pt + (size_t)(t.pk.Nmax + 1) * RN_D;
    te_gemm_pq(t.rn(), h, w0, rawp(c, m.b[0]), Pt, Qt, t.cx);
    EFuse f{Pt, Qt, t.w.nbr, t.k, t.pk.Nmax, e, res_out, site_res};
    if (m.depth > 1)
        te_mlp2_fwd(t.re(), e, w0 + 2 * RN_D, 3 * RN_D, rawp(c, m.w[1]), RN_D, rawp(c, m.b[1]), pre1, pre2, f, t.dr, site0, t.cx);
    else
        t.bad |= !te_gemm(t.re(), e, true, RN_D, w0 + 2 * RN_D, 3 * RN_D, true, nullptr, pre1, false, nullptr, &f, t.dr, 0u, t.cx);
}
// Accumulates parameter grads, dE (bf16) += d e, dh_acc (f32) += d h.  Depth 1: on entry E2 (bf16) holds d pre1.  Depth 2: `from` is required;
// d pre2 is formed inside the fused kernel from the upstream gradient (EBwd2Src).
// `dpre1_keep` (depth-2 MLPs): d pre1 is left in that buffer and the e-side pass (dWc, dE) is NOT run - the caller runs it for both MLPs of the
// layer at once (mlp_edge_bwd1_pair).
void mlp_edge_bwd_mixed(Tr& t, const Mlp2& m, const float* h, const tb16* e, const tb16* pre1, tb16* dE, float* dh_acc,
                        const EBwd2Src* from = nullptr, const tb16* dy_in = nullptr, tb16* dpre1_keep = nullptr) {
    rnampnn_ctx* c = t.c;
    tb16* dpre1 = eb(t.w.E2);
    if (m.depth > 1) {
        dpre1 = dpre1_keep ? dpre1_keep : eb(t.w.E1);
        te_gemm_bwd2(t.re(), dy_in, pre1, dpre1, rawp(c, m.w[1]), RN_D, t.gw(m.w[1]), RN_D, t.dr, t.gw(m.b[1]), t.cx, *from);
    }
    float* gw0 = t.gw(m.w[0]);
    const float* w0 = rawp(c, m.w[0]);
    if (!dpre1_keep) te_gemm_bwd1(t.re(), dpre1, e, dE, w0 + 2 * RN_D, 3 * RN_D, gw0 + 2 * RN_D, 3 * RN_D, t.cx);   // dWc, dE: one pass over dpre1
    te_edge_pq_bwd(t.pk, t.k, dpre1, t.w.rstart, t.w.rlist, t.w.dpq, t.cx.s);
    tm_gemm_tn_pq(t.rn(), t.w.dpq, h, gw0, t.gw(m.b[0]), t.cx);                 // [dWa ; dWb] += [dP | dQ]^T h, db1 += colsum(dP)
    if (!tm_gemm_nn_pq(t.rn(), t.w.dpq, w0, dh_acc, t.cx.s)) {                            // dh += dP . Wa + dQ . Wb
        mm_nn(t, t.rn(), t.w.dpq, 256, RN_D, w0, 3 * RN_D, nullptr, RN_D, dh_acc, RN_D, 1);
        mm_nn(t, t.rn(), t.w.dpq + RN_D, 256, RN_D, w0 + RN_D, 3 * RN_D, nullptr, RN_D, dh_acc, RN_D, 1);
    }
}
// the e-side backward of the edge-update MLP and the message MLP of one layer (both read e[l], both add into dE): one pass over e and dE
void mlp_edge_bwd1_pair(Tr& t, const Mlp2& me, const Mlp2& mm, const tb16* e, const tb16* dpre1_e, const tb16* dpre1_m, tb16* dE) {
    rnampnn_ctx* c = t.c;
    te_gemm_bwd1x2(t.re(), dpre1_e, dpre1_m, e, dE, rawp(c, me.w[0]) + 2 * RN_D, rawp(c, mm.w[0]) + 2 * RN_D, 3 * RN_D,
                   t.gw(me.w[0]) + 2 * RN_D, t.gw(mm.w[0]) + 2 * RN_D, 3 * RN_D, t.cx);
}
// edge embedding (feature.py:540-571), bf16 chain: raw features [E][128] (90 live columns) -> pe1 -> pe2 -> e[0], the activations fused into the
// GEMM operand loads
void edge_embed_fwd_mixed(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int k = t.k;
    const Lin& ee0 = c->edge_embed[0];
    te_edge_features(t.pk, k, w.geom, w.nbr, eb(w.F), s);
    t.bad |= !te_gemm(t.re(), w.F, true, RN_D, rawp(c, ee0.w), RN_ERAW, true, rawp(c, ee0.b), eb(w.pe1), false, nullptr, nullptr, t.dr, 0u, t.cx, RN_ERAW);
    if (c->cfg.depth_res_edge_feature > 1) {
        const Lin& ee1 = c->edge_embed[1];
        t.bad |= !te_gemm(t.re(), w.pe1, true, RN_D, rawp(c, ee1.w), RN_D, true, rawp(c, ee1.b), eb(w.pe2), true, nullptr, nullptr, t.dr, site_ee(0), t.cx);
        te_edge_act(t.pk, k, w.nbr, eb(w.pe2), eb(w.e[0]), t.dr, site_ee(1), s);
    } else {
        te_edge_act(t.pk, k, w.nbr, eb(w.pe1), eb(w.e[0]), t.dr, site_ee(0), s);
    }
}
// ResMPNN layers (mpnn.py:283-294)
void layers_fwd_mixed(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    for (int l = 0; l < L; ++l) {
        const MpnnLayer& m = c->mpnn[l];
        mlp_edge_fwd_mixed(t, m.msg, w.h[l], eb(w.e[l]), eb(w.pm1[l]), eb(w.pm2[l]), site_msg(l, 0), nullptr, 0u);
        te_seg_mean(t.pk, k, w.nbr, eb(m.msg.depth > 1 ? w.pm2[l] : w.pm1[l]), w.h[l], w.hpre[l], t.dr, site_msg(l, m.msg.depth - 1), s,
                    m.msg.depth > 1 ? eb(w.pm2[l]) : nullptr);
        launch_graph_norm_packed(t.pk, w.hpre[l], w.h[l + 1], rawp(c, m.gn_scale), rawp(c, m.gn_shift), t.t_norm, s);
        if (l + 1 < L)
            mlp_edge_fwd_mixed(t, m.edge, w.h[l + 1], eb(w.e[l]), eb(w.pu1[l]), eb(w.pu2[l]), site_edge(l, 0), eb(w.e[l + 1]),
                               site_edge(l, m.edge.depth - 1));
    }
}
// backward of layers l_hi .. l_lo (descending).  On entry dh = d h[l_hi + 1], dE (bf16) = d e[l_hi + 1]; on return dh = d h[l_lo], dE = d e[l_lo]
void layers_bwd_mixed(Tr& t, int l_hi, int l_lo) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    const size_t N = (size_t)t.pk.Nmax;
    for (int l = l_hi; l >= l_lo; --l) {
        const MpnnLayer& m = c->mpnn[l];
        const bool nopair = ab_switch("RNAMPNN_NO_BWD1_PAIR");
        // both MLPs of the layer read e[l] and add into dE: their e-side passes (dWc, dE) run as ONE kernel after the message MLP's (the two
        // d pre1 tensors live in the two bf16 halves of E1, which is carved for f32)
        const bool pair = l + 1 < L && m.edge.depth > 1 && m.msg.depth > 1 && !nopair;
        tb16* dp1_e = pair ? eb(w.E1) : nullptr;
        tb16* dp1_m = pair ? eb(w.E1) + N * k * RN_D : nullptr;
        if (l + 1 < L) {
            if (m.edge.depth > 1) {     // the residual backward rides in the fused kernel's staging pass
                EBwd2Src from{1, eb(w.pu2[l]), w.nbr, nullptr, nullptr, k};
                mlp_edge_bwd_mixed(t, m.edge, w.h[l + 1], eb(w.e[l]), eb(w.pu1[l]), eb(w.dE), w.dh, &from, eb(w.dE), dp1_e);
            } else {
                te_edge_res_bwd(t.pk, k, w.nbr, eb(w.dE), eb(w.pu1[l]), eb(w.E2), t.dr, site_edge(l, 0), s);
                mlp_edge_bwd_mixed(t, m.edge, w.h[l + 1], eb(w.e[l]), eb(w.pu1[l]), eb(w.dE), w.dh);
            }
        }
        t_gn_bwd(t.pk, w.hpre[l], w.dh, rawp(c, m.gn_scale), t.t_norm, w.dh2, t.gw(m.gn_scale), t.gw(m.gn_shift), t.cx);
        if (m.msg.depth > 1) {          // ... and so does the backward of the message mean (dagg = dh2)
            launch_copy_bytes(w.dh, w.dh2, N * RN_D * sizeof(float), s);
            EBwd2Src from{2, eb(w.pm2[l]), w.nbr, w.dh2, w.invc, k};
            mlp_edge_bwd_mixed(t, m.msg, w.h[l], eb(w.e[l]), eb(w.pm1[l]), eb(w.dE), w.dh, &from, nullptr, dp1_m);
            if (pair) mlp_edge_bwd1_pair(t, m.edge, m.msg, eb(w.e[l]), dp1_e, dp1_m, eb(w.dE));
        } else {
            te_seg_mean_bwd(t.pk, k, w.nbr, w.dh2, eb(w.pm1[l]), eb(w.E2), t.dr, site_msg(l, 0), s);
            launch_copy_bytes(w.dh, w.dh2, N * RN_D * sizeof(float), s);
            mlp_edge_bwd_mixed(t, m.msg, w.h[l], eb(w.e[l]), eb(w.pm1[l]), eb(w.dE), w.dh);
        }
    }
}
// ResFeature, edge side: dE (bf16) = d e[0]
void edge_embed_bwd_mixed(Tr& t) {
    rnampnn_ctx* c = t.c; TW& w = t.w; hipStream_t s = t.cx.s;
    const int k = t.k;
    const Lin& ee0 = c->edge_embed[0];
    tb16* dpe1 = eb(w.E1);
    if (c->cfg.depth_res_edge_feature > 1) {
        const Lin& ee1 = c->edge_embed[1];
        te_edge_res_bwd(t.pk, k, w.nbr, eb(w.dE), eb(w.pe2), eb(w.E2), t.dr, site_ee(1), s);                              // d pe2 (absent edges: 0)
        te_gemm_tn(t.re(), eb(w.E2), eb(w.pe1), t.gw(ee1.w), RN_D, true, t.dr, site_ee(0), t.gw(ee1.b), t.cx);
        t.bad |= !te_gemm(t.re(), w.E2, true, RN_D, rawp(c, ee1.w), RN_D, false, nullptr, dpe1, false, eb(w.pe1), nullptr, t.dr, site_ee(0), t.cx);   // d pe1
    } else {
        te_edge_res_bwd(t.pk, k, w.nbr, eb(w.dE), eb(w.pe1), dpe1, t.dr, site_ee(0), s);
    }
    te_gemm_tn(t.re(), dpe1, eb(w.F), t.gw(ee0.w), RN_ERAW, false, t.dr, 0u, t.gw(ee0.b), t.cx, RN_ERAW);
}
}  // namespace

// shared argument checks + workspace carve of the three training entry points
static int train_begin(Tr& t, rnampnn_handle h, int B, int T, void* ws, size_t ws_bytes, void* stream, bool mixed) {
    if (!h) return fail(RNAMPNN_ERR_BAD_ARG, "null handle");
    if (!h->raw_arena) return fail(RNAMPNN_ERR_WEIGHTS, "no weights have been set");
    // the f32 kernels read the K-major weight copies finalize builds; the mixed kernels read nn.Linear.weight as stored
    // and refresh the three copies they still need themselves (train_forward_impl)
    if (!mixed && !h->finalized) return fail(RNAMPNN_ERR_WEIGHTS, "weights not finalized (call rnampnn_finalize_weights)");
    for (auto& w : h->raw)
        if (!w.set) return fail(RNAMPNN_ERR_WEIGHTS, "weight '%s' has not been set", w.key.c_str());
    if (!ws || B <= 0 || T <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "training call: null workspace or non-positive B/T");
    if (T > h->cfg.padding_len) return fail(RNAMPNN_ERR_T_GT_P, "max_len %d exceeds padding_len %d", T, h->cfg.padding_len);
    // 32-bit element-pair indices of the dropout hash (kernels_train.h) and 32-bit edge-row indexing: rows * D / 2 < 2^32
    if ((long long)B * T * h->cfg.num_res_neighbours >= (1LL << 26) || (long long)B * T >= (1LL << 23))
        return fail(RNAMPNN_ERR_BAD_ARG, "row count out of range for the training path (B*T*k < 2^26); split the batch");
    size_t need = carve_train(h, B, T, nullptr, nullptr);
    if (ws_bytes < need) return fail(RNAMPNN_ERR_WORKSPACE, "training workspace %zu bytes < required %zu", ws_bytes, need);
    if (((uintptr_t)ws & 255) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    t.c = h; t.cx.s = (hipStream_t)stream; t.g = nullptr; t.k = h->cfg.num_res_neighbours; t.mixed = mixed;
    if (mixed && !h->wimg) h->wimg = t_wimg_create(1024);      // (null on allocation failure: the kernels then build their images themselves)
    t.cx.wimg = mixed ? h->wimg : nullptr;
    carve_train(h, B, T, (char*)ws, &t.w);
    t.pk.len = t.w.len; t.pk.cu = t.w.cu; t.pk.node_b = t.w.node_b; t.pk.B = B; t.pk.T = T; t.pk.Nmax = B * T; t.pk.packed_in = 0;
    return RNAMPNN_OK;
}

static int train_forward_impl(Tr& t, const float* coords, const float* mask, float* logits) {
    rnampnn_ctx* c = t.c;
    TW& w = t.w;
    hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    const size_t N = (size_t)t.pk.Nmax;
    launch_zero_bytes(w.pq + N * 256, 256 * sizeof(float), s);
    if (t.mixed) launch_zero_bytes(eb(w.pq) + (2 * N + 1) * RN_D, RN_D * sizeof(tb16), s);      // row N of the bf16 Q table
    for (int l = 0; l <= L; ++l) launch_zero_bytes(w.h[l] + N * RN_D, RN_D * sizeof(float), s);
    if (t.mixed) t_wimg_refresh(c->wimg, s);                    // weight-fragment images of every 128 x 128 block seen so far, from the current weights
    if (t.mixed)       // K-major copies of the two weights whose in-dim (28) the MFMA form does not take
        for (const Lin* l : {&c->raw_project, &c->raw_ffn[0]})
            launch_transpose(rawp(c, l->w), l->in, l->out, l->in, derp<float>(c, l->wt), l->out, s);
    launch_lengths(mask, t.pk, s);
    launch_geom(coords, t.pk, t.t_norm, nullptr, w.raw_p, w.geom, nullptr, s);
    if (launch_knn(coords, t.pk, t.t_norm, k, w.nbr, nullptr, s)) return fail(RNAMPNN_ERR_UNSUPPORTED, "max_len too long for k-NN");
    t_build_reverse(t.pk, k, w.nbr, w.rdeg, w.rstart, w.rfill, w.rlist, reinterpret_cast<int*>(w.E1), s);
    if (t.mixed) te_inv_count(t.pk, k, w.nbr, w.invc, s);
    // edge embedding: the launch sequence of the call's precision
    if (t.mixed) edge_embed_fwd_mixed(t); else edge_embed_fwd_f32(t);
    // node embedding (feature.py:531-538, 591)
    lin_fwd(t, c->raw_project, w.raw_p, RN_RAWP, w.x0, RN_D);
    if (bert_fwd(t, c->emb, w.emb, w.x0, w.n1, site_emb_att(0), site_emb_ffn(0))) return fail(RNAMPNN_ERR_UNSUPPORTED, "head dim unsupported");
    launch_graph_norm_packed(t.pk, w.n1, w.h[0], rawp(c, c->feat_gn_scale), rawp(c, c->feat_gn_shift), t.t_norm, s);
    // ResMPNN layers
    if (t.mixed) layers_fwd_mixed(t); else layers_fwd_f32(t);
    // post fusion, raw embedding, readout (rnampnn.py:179-181)
    if (bert_fwd(t, c->post, w.post, w.h[L], w.hp, site_post_att(0), site_post_ffn(0))) return fail(RNAMPNN_ERR_UNSUPPORTED, "head dim unsupported");
    ffn_fwd(t, c->raw_ffn, w.raw_p, RN_RAWP, w.raw_pre, w.r1, site_raw(0));
    launch_graph_norm_packed(t.pk, w.r1, w.re, rawp(c, c->rawffn_gn_scale), rawp(c, c->rawffn_gn_shift), t.t_norm, s);
    {   // readout on cat(hp, re): first Linear split over the two sources
        const Lin& r0 = c->readout[0];
        bool single = c->readout.size() == 1;
        float* dst = single ? w.logits_p : w.ro_pre[0];
        const float* wt = derp<float>(c, r0.wt);
        const float* wr = rawp(c, r0.w);                    // [out][256] = [h_post part | raw_emb part]
        mm_nt(t, t.rn(), w.hp, RN_D, RN_D, wr, 2 * RN_D, wt, r0.out, rawp(c, r0.b), r0.out, dst, r0.out, 0);
        mm_nt(t, t.rn(), w.re, RN_D, RN_D, wr + RN_D, 2 * RN_D, wt + (size_t)RN_D * r0.out, r0.out, nullptr, r0.out, dst, r0.out, 1);
        const float* cur = dst;
        int ld = r0.out;
        for (size_t i = 1; i < c->readout.size(); ++i) {
            const Lin& l = c->readout[i];
            bool last = i + 1 == c->readout.size();
            t_gelu_fwd(t.rn(), cur, w.act, ld, t.dr, site_ro((int)i - 1), s);
            float* d2 = last ? w.logits_p : w.ro_pre[i];
            lin_fwd(t, l, w.act, ld, d2, l.out);
            cur = d2; ld = l.out;
        }
    }
    if (logits) launch_unpack_nodes(t.pk, w.logits_p, 4, 4, logits, s);
    HIP_TRY(hipGetLastError());
    if (t.bad) return fail(RNAMPNN_ERR_UNSUPPORTED, "bf16-mixed training: a GEMM variant this configuration needs is not built");
    return RNAMPNN_OK;
}

// backward from w.dlogits (packed rows) into t.g; `accumulate` = 0 overwrites the gradient buffer
static int train_backward_impl(Tr& t, int accumulate) {
    rnampnn_ctx* c = t.c;
    TW& w = t.w;
    hipStream_t s = t.cx.s;
    const int L = c->cfg.num_res_mpnn_layers, k = t.k;
    const size_t N = (size_t)t.pk.Nmax;
    if (!accumulate) launch_zero_bytes(t.g, c->raw_floats * sizeof(float), s);
    red_begin(t.cx, w.sc);         // the queue of this backward; it lives in the call's context and dies with it on every return
    {   // readout
        const float* d = w.dlogits;
        float* bufs[2] = {w.dA, w.dB};
        for (int i = (int)c->readout.size() - 1; i >= 1; --i) {
            const Lin& l = c->readout[i];
            t_gelu_fwd(t.rn(), w.ro_pre[i - 1], w.act, l.in, t.dr, site_ro(i - 1), s);
            float* din = bufs[i & 1];
            lin_bwd(t, l, w.act, l.in, d, l.out, din, l.in);
            t_gelu_bwd(t.rn(), din, w.ro_pre[i - 1], din, l.in, t.dr, site_ro(i - 1), s);
            d = din;
        }
        const Lin& r0 = c->readout[0];
        const float* w0 = rawp(c, r0.w);                    // [out][256]
        mm_nn(t, t.rn(), d, r0.out, r0.out, w0, 2 * RN_D, nullptr, RN_D, w.dhp, RN_D, 0);
        mm_nn(t, t.rn(), d, r0.out, r0.out, w0 + RN_D, 2 * RN_D, nullptr, RN_D, w.dre, RN_D, 0);
        mm_tn(t, t.rn(), d, r0.out, r0.out, w.hp, RN_D, RN_D, t.gw(r0.w), 2 * RN_D, t.gw(r0.b));
        mm_tn(t, t.rn(), d, r0.out, r0.out, w.re, RN_D, RN_D, t.gw(r0.w) + RN_D, 2 * RN_D);
    }
    // raw embedding branch
    t_gn_bwd(t.pk, w.r1, w.dre, rawp(c, c->rawffn_gn_scale), t.t_norm, w.nscr, t.gw(c->rawffn_gn_scale), t.gw(c->rawffn_gn_shift), t.cx);
    ffn_bwd(t, c->raw_ffn, w.raw_p, RN_RAWP, w.raw_pre, w.nscr, nullptr, 0, site_raw(0));
    // post fusion -> dh = d h[L]
    if (bert_bwd(t, c->post, w.post, w.dhp, w.dh, site_post_att(0), site_post_ffn(0))) return fail(RNAMPNN_ERR_UNSUPPORTED, "head dim unsupported");
    // gradient chunk 0 (post_fusion, raw_embedding, readout: the tail of the flat buffer) is final
    red_flush(t.cx);
    if (c->grad_ev[0]) HIP_TRY(hipEventRecord(c->grad_ev[0], s));
    // ResMPNN layers, reverse.  dE = d e[l+1] (zero for the last layer: its edge update is dead)
    launch_zero_bytes(w.dE, N * k * RN_D * (t.mixed ? sizeof(tb16) : sizeof(float)), s);
    const auto layers_bwd = t.mixed ? layers_bwd_mixed : layers_bwd_f32;
    layers_bwd(t, L - 1, L / 2);
    // chunk 1 (layers L/2 .. L-1; L == 1: the one layer) is final
    red_flush(t.cx);
    if (c->grad_ev[1]) HIP_TRY(hipEventRecord(c->grad_ev[1], s));
    layers_bwd(t, L / 2 - 1, 0);
    // ResFeature: node side  dh = d h[0]
    t_gn_bwd(t.pk, w.n1, w.dh, rawp(c, c->feat_gn_scale), t.t_norm, w.dh2, t.gw(c->feat_gn_scale), t.gw(c->feat_gn_shift), t.cx);
    if (bert_bwd(t, c->emb, w.emb, w.dh2, w.dh, site_emb_att(0), site_emb_ffn(0))) return fail(RNAMPNN_ERR_UNSUPPORTED, "head dim unsupported");
    lin_bwd(t, c->raw_project, w.raw_p, RN_RAWP, w.dh, RN_D, nullptr, 0);
    // ResFeature: edge side  dE = d e[0]
    if (t.mixed) edge_embed_bwd_mixed(t); else edge_embed_bwd_f32(t);
    t.bad |= !red_end(t.cx);
    HIP_TRY(hipGetLastError());
    if (t.bad) return fail(RNAMPNN_ERR_UNSUPPORTED, "training backward: a GEMM variant this configuration needs is not built, or the reduction "
                           "queue refused a request (red_queue.h: RedQueue)");
    return RNAMPNN_OK;
}

static int check_dropout(float p) {
    if (!(p >= 0.f) || p >= 1.f) return fail(RNAMPNN_ERR_BAD_ARG, "dropout must be in [0, 1), got %g", (double)p);
    return RNAMPNN_OK;
}

// tape bookkeeping: a forward into workspace `ws` invalidates whatever tape lived there before
static void tape_drop_ws(rnampnn_ctx* h, const void* ws) {
    for (size_t i = 0; i < h->tapes.size();)
        if (h->tapes[i].ws == ws) h->tapes.erase(h->tapes.begin() + i); else ++i;
}

extern "C" int rnampnn_train_forward(rnampnn_handle h, const float* coords, const float* mask, int32_t B, int32_t T,
                                     int32_t T_norm, float dropout, uint64_t seed, int32_t flags, float* logits, void* ws,
                                     size_t ws_bytes, void* stream, int64_t* tape_id) {
    if (!coords || !mask || !tape_id) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_train_forward: null input");
    *tape_id = 0;
    int rc = check_dropout(dropout);
    if (rc) return rc;
    Tr t;
    rc = train_begin(t, h, B, T, ws, ws_bytes, stream, (flags & RNAMPNN_TRAIN_BF16_MIXED) != 0);
    if (rc) return rc;
    t.t_norm = T_norm > 0 ? T_norm : T;
    if (t.t_norm < T) return fail(RNAMPNN_ERR_BAD_ARG, "T_norm %d < T %d", t.t_norm, T);
    t.dr = t_drop(dropout, seed, h->seed_dev);
    t.att_mfma = att_mfma_env(t.mixed);
    tape_drop_ws(h, ws);
    rc = train_forward_impl(t, coords, mask, logits);
    if (rc) return rc;
    // a record dies when its workspace is reused (tape_drop_ws) or its backward... never: the cap only bounds a caller that keeps opening NEW
    // workspaces without ever running a backward (a record is 64 bytes; gradient accumulation over thousands of outstanding forwards stays valid)
    if (h->tapes.size() >= 4096) h->tapes.erase(h->tapes.begin());
    h->tapes.push_back(rnampnn_ctx::Tape{++h->tape_counter, B, T, t.t_norm, dropout, seed, ws, t.mixed, h->seed_dev, t.att_mfma});
    *tape_id = h->tape_counter;
    return RNAMPNN_OK;
}

extern "C" int rnampnn_train_backward(rnampnn_handle h, int64_t tape_id, const float* dlogits, int32_t B, int32_t T,
                                      int32_t accumulate, float* grad, void* ws, size_t ws_bytes, void* stream) {
    if (!h || !dlogits || !grad) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_train_backward: null argument");
    const rnampnn_ctx::Tape* tp = nullptr;
    for (auto& x : h->tapes) if (x.id == tape_id) tp = &x;
    if (!tp)
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_train_backward: tape %lld is gone (its workspace was overwritten by a later "
                    "rnampnn_train_forward / rnampnn_loss_and_grad, or it was never recorded)", (long long)tape_id);
    if (tp->B != B || tp->T != T || tp->ws != ws)
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_train_backward: tape %lld was recorded with B=%d T=%d in another workspace",
                    (long long)tape_id, tp->B, tp->T);
    const rnampnn_ctx::Tape tape = *tp;
    Tr t;
    int rc = train_begin(t, h, B, T, ws, ws_bytes, stream, tape.mixed);
    if (rc) return rc;
    t.t_norm = tape.tnorm;
    t.dr = t_drop(tape.p, tape.seed, tape.seed_dev);
    t.att_mfma = tape.att_mfma;
    t.g = grad;
    t_pack_dlogits(t.pk, dlogits, t.w.dlogits, t.cx.s);
    return train_backward_impl(t, accumulate);
}

extern "C" int rnampnn_loss_and_grad(rnampnn_handle h, const float* coords, const float* mask, const int32_t* labels,
                                     int32_t B, int32_t T, int32_t T_norm, float dropout, uint64_t seed, int32_t flags,
                                     float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    if (!coords || !mask || !labels || !loss || !grad)
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_loss_and_grad: null pointer");
    int rc = check_dropout(dropout);
    if (rc) return rc;
    Tr t;
    rc = train_begin(t, h, B, T, ws, ws_bytes, stream, (flags & RNAMPNN_TRAIN_BF16_MIXED) != 0);
    if (rc) return rc;
    t.t_norm = T_norm > 0 ? T_norm : T;
    if (t.t_norm < T) return fail(RNAMPNN_ERR_BAD_ARG, "T_norm %d < T %d", t.t_norm, T);
    t.dr = t_drop(dropout, seed, h->seed_dev);
    t.att_mfma = att_mfma_env(t.mixed);
    t.g = grad;
    tape_drop_ws(h, ws);
    rc = train_forward_impl(t, coords, mask, logits);
    if (rc) return rc;
    t_loss_grad(t.pk, t.w.logits_p, labels, t.w.dlogits, loss, t.w.sc.p, t.cx.s);
    return train_backward_impl(t, 0);
}

// torch.optim.Adam(lr, betas, eps, weight_decay) step (rnampnn.py:156-159: lr 2e-3, weight_decay 2e-4, L2 form: the decay
// enters the gradient) as ONE launch over the flat parameter / gradient buffers instead of 150 per-tensor updates.
extern "C" int rnampnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || numel <= 0 || step < 1)
        return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_adam_step: bad argument");
    t_adam_step(param, grad, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}

// ---- test tap of the 90 raw edge features (feature.py:386-517: 49 cross distances, 25 bond-angle and 16 dihedral-normal dot products) -
// the tensor the inference kernels never materialise; the f32 trainer's own feature kernel writes it, so the reference's golden `edge_raw`
// pins rows A3 / A4 directly instead of through e0.  feats: (B, T, k, 96) f32, columns 90..95 and absent / padded edges zero.
namespace {
struct RawWs { int *len, *cu, *node_b, *nbr; float *raw_p, *geom, *F; };
size_t carve_edge_raw(int B, int T, int k, char* base, RawWs* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return base ? base + o : (char*)nullptr; };
    const size_t N = (size_t)B * T;
    RawWs tmp;
    RawWs& r = w ? *w : tmp;
    r.len = (int*)take(B * sizeof(int)); r.cu = (int*)take((B + 1) * sizeof(int)); r.node_b = (int*)take(N * sizeof(int));
    r.nbr = (int*)take(N * k * sizeof(int));
    r.raw_p = (float*)take(N * RN_RAWP * sizeof(float)); r.geom = (float*)take((N + B) * RN_GEOM * sizeof(float));      // (+ one phantom record per RNA, k_geom)
    r.F = (float*)take(N * k * RN_ERAWP * sizeof(float));
    return off;
}
}  // namespace
extern "C" size_t rnampnn_edge_raw_workspace_bytes(rnampnn_handle h, int32_t B, int32_t T) {
    if (!h || B <= 0 || T <= 0) return 0;
    return carve_edge_raw(B, T, h->cfg.num_res_neighbours, nullptr, nullptr);
}
extern "C" int rnampnn_edge_raw_features(rnampnn_handle h, const float* coords, const float* mask, int32_t B, int32_t T, int64_t* edge_index,
                                         float* feats, void* ws, size_t ws_bytes, void* stream) {
    if (!h || !coords || !mask || !feats || !ws || B <= 0 || T <= 0) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_edge_raw_features: null pointer or non-positive B/T");
    const int k = h->cfg.num_res_neighbours;
    if ((long long)B * T * k >= (1LL << 26)) return fail(RNAMPNN_ERR_BAD_ARG, "rnampnn_edge_raw_features: batch too large");
    if (ws_bytes < carve_edge_raw(B, T, k, nullptr, nullptr)) return fail(RNAMPNN_ERR_WORKSPACE, "rnampnn_edge_raw_features: workspace too small");
    if (((uintptr_t)ws & 255) != 0) return fail(RNAMPNN_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    RawWs w;
    carve_edge_raw(B, T, k, (char*)ws, &w);
    hipStream_t s = (hipStream_t)stream;
    PackInfo pk;
    pk.len = w.len; pk.cu = w.cu; pk.node_b = w.node_b; pk.B = B; pk.T = T; pk.Nmax = B * T; pk.packed_in = 0;
    launch_lengths(mask, pk, s);
    launch_geom(coords, pk, pk.T, nullptr, w.raw_p, w.geom, nullptr, s);
    if (launch_knn(coords, pk, pk.T, k, w.nbr, edge_index, s)) return fail(RNAMPNN_ERR_UNSUPPORTED, "max_len too long for k-NN");
    t_edge_features(pk, k, w.geom, w.nbr, w.F, s);
    HIP_TRY(hipMemsetAsync(feats, 0, (size_t)B * T * k * RN_ERAWP * sizeof(float), s));
    launch_unpack_nodes(pk, w.F, k * RN_ERAWP, k * RN_ERAWP, feats, s);
    HIP_TRY(hipGetLastError());
    return RNAMPNN_OK;
}
