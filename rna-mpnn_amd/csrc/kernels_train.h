// Training-path building blocks (kernels_train.hip): f32, packed rows.
#pragma once
#include "rnampnn_internal.h"
#include "red_queue.h"

struct TRows { const int* ntot; int mul; int maxrows; };   // row count = *ntot * mul (device side), maxrows = host upper bound

// Dropout of the training path (the reference: nn.Dropout(p) after every GELU, mpnn.py:140,150, feature.py:200,
// functional.py:69,124,184, and on the attention probabilities, functional.py:109).  The keep decision of one element is a
// pure function of (seed, site, element index), restated by the CPU oracle, so that the HIP forward / backward and the oracle's
// autograd see THE SAME mask.  One 32-bit counter hash (murmur3 finaliser) serves the PAIR of elements (2P, 2P + 1): the low
// 16 bits decide the even element, the high 16 bits the odd one (keep iff >= thresh = round(p * 65536)): the kernels that own 8
// consecutive channels of a row pay 4 hashes for 8 decisions.  element index = row * D + channel with rows in the packed order
// (node row p, edge row p*k + slot); attention: ((query row * heads + head) << 13) + key.
// seed_dev (optional): the seed is read from DEVICE memory at kernel time instead (a hipGraph that captured a training step then draws
// fresh masks on every replay once the caller has updated *seed_dev - the decode path's rnampnn_sample_dev_seed idea).
struct TDrop { unsigned long long seed; unsigned thresh; float scale; const unsigned long long* seed_dev; };   // scale = 1/(1-p)
static inline TDrop t_drop(float p, unsigned long long seed, const unsigned long long* seed_dev = nullptr) {
    TDrop d;
    d.seed = seed;
    d.seed_dev = seed_dev;
    d.thresh = p > 0.f ? (unsigned)(p * 65536.0f + 0.5f) : 0u;
    d.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    return d;
}

// blocks of a grid-stride element-wise launch over `units` work items, 256 per block: at least one, at most 16384
static inline unsigned ew_grid(size_t units) { const size_t g = (units + 255) / 256; return (unsigned)(g < 16384 ? (g ? g : 1) : 16384); }

void t_gemm(const TRows& rows, const float* X, int ldx, int K, const float* Wt, int ldw, const float* bias, int N,
            float* Y, int ldy, int beta, hipStream_t s);                      // Y = beta*Y + X.Wt + bias   (Wt K-major, row stride ldw)
// One training or inference call as the launchers below see it: its stream, the ordered reductions of its backward and the weight-image cache of
// its handle (null: kernels build their images themselves).  Tr (train.cpp) and RdRun (rdesign_internal.h) each own one; the launchers that
// allocate partials or look up an image take it in place of the stream.
// Ordered reductions (red_queue.h: RedQueue): between red_begin and red_end every producer of partial tiles (t_gemm_tn, t_colsum, tm_gemm_tn[_pq],
// te_gemm_tn, te_gemm_bwd1[x2], te_gemm_bwd2, t_gn_bwd) takes an exact extent of the arena and records its reduction, and the recorded reductions
// run many per launch (RNAMPNN_NO_RED_BATCH=1, read at red_begin: one per launch); a producer called outside the two is refused.  red_flush makes
// everything recorded so far final (before a gradient chunk's event); red_end flushes, closes the queue and returns false when a request or job was
// refused since red_begin (nothing of it was launched).  An arena holds at least one producer's budget of RED_VIEW floats.
struct TScratch { float* p; size_t floats; };
static constexpr size_t RED_VIEW = (size_t)16 << 20;
struct WImageCache;
struct TCall { hipStream_t s = nullptr; RedQueue red; WImageCache* wimg = nullptr; };
static inline void red_begin(TCall& cx, const TScratch& arena) { cx.red.open(arena.p, arena.floats, cx.s, ab_switch("RNAMPNN_NO_RED_BATCH")); }
static inline void red_flush(TCall& cx) { cx.red.flush(); }
static inline bool red_end(TCall& cx) { return cx.red.end(); }
void t_gemm_tn(const TRows& rows, const float* A, int lda, int M, const float* B, int ldb, int K, float* dW, int ldw, TCall& cx);   // dW += A^T B
// bf16-mixed MFMA versions (kernels_train.hip, second half).  _nt / _nn / _tn return false (nothing launched) when the shape is not covered
// (K not a multiple of 16, unaligned rows; _tn with actB: a partial tile larger than its budget): the caller then uses the f32 kernels.
bool tm_gemm_nt(const TRows& rows, const float* X, int ldx, int K, const float* W, int ldw, const float* bias, int N, float* Y,
                int ldy, int beta, bool actA, const TDrop& dr, unsigned site, TCall& cx);
bool tm_gemm_nn(const TRows& rows, const float* X, int ldx, int K, const float* W, int ldw, const float* bias, int N, float* Y,
                int ldy, int beta, const float* epi_pre, int ld_epi, const TDrop& dr, unsigned site, TCall& cx);
// dbias (optional): += column sums of A, computed from the tiles the kernel stages anyway (the bias gradient of the same Linear)
bool tm_gemm_tn(const TRows& rows, const float* A, int lda, int M, const float* B, int ldb, int K, float* dW, int ldw,
                bool actB, const TDrop& dr, unsigned site, float* dbias, TCall& cx);
void t_colsum(const TRows& rows, const float* A, int lda, int M, float* out, TCall& cx);   // out += column sums
void t_gelu_fwd(const TRows& rows, const float* x, float* y, int D, const TDrop& dr, unsigned site, hipStream_t s);   // y = drop(gelu(x))
void t_gelu_bwd(const TRows& rows, const float* dy, const float* pre, float* dx, int D, const TDrop& dr, unsigned site,
                hipStream_t s);                                                                             // dx = dy * mask * gelu'(pre)
void t_add(const TRows& rows, const float* a, float* dst, int D, hipStream_t s);                            // dst += a
void t_edge_features(const PackInfo& pk, int k, const float* geom, const int* nbr, float* F, hipStream_t s);        // [E][96]
void t_edge_add_pq(const PackInfo& pk, int k, const int* nbr, const float* pq, float* pre, hipStream_t s);          // pre += P[i] + Q[j]
void t_edge_zero_invalid(const PackInfo& pk, int k, const int* nbr, float* x, hipStream_t s);
void t_edge_residual(const PackInfo& pk, int k, const int* nbr, const float* e_in, const float* pre2, float* e_out,
                     const TDrop& dr, unsigned site, hipStream_t s);
void t_seg_mean(const PackInfo& pk, int k, const int* nbr, const float* pre2, const float* h, float* out,
                const TDrop& dr, unsigned site, hipStream_t s);
void t_seg_mean_bwd(const PackInfo& pk, int k, const int* nbr, const float* dagg, const float* pre2, float* dpre2,
                    const TDrop& dr, unsigned site, hipStream_t s);
void t_edge_res_bwd(const PackInfo& pk, int k, const int* nbr, const float* de, const float* pre2, float* dpre2,
                    const TDrop& dr, unsigned site, hipStream_t s);
// reverse adjacency (deg/start/fill: [Nmax+1] ints, list: [Nmax*k] ints) and the gather-form backward of P[i] + Q[j]
void t_build_reverse(const PackInfo& pk, int k, const int* nbr, int* deg, int* start, int* fill, int* list, int* tmp, hipStream_t s);   // tmp: [Nmax*k] ints of scratch
void t_edge_pq_bwd(const PackInfo& pk, int k, const float* dpre1, const int* start, const int* list, float* dpq, hipStream_t s);
void t_gn_bwd(const PackInfo& pk, const float* x, const float* dy, const float* scale, int t_tot, float* dx, float* dscale,
              float* dshift, TCall& cx);
// stat [N][heads][3]: the forward writes (row max, normaliser) per (query, head); the backward reads them and adds delta (it is a TAPE: one per attention layer)
int  t_attention_fwd(const PackInfo& pk, const float* qkv, int heads, float* out, float* stat, const TDrop& dr, unsigned site, hipStream_t s);
int  t_attention_bwd(const PackInfo& pk, const float* qkv, const float* O, const float* dO, int heads, float* dqkv, float* stat,
                     const TDrop& dr, unsigned site, hipStream_t s);
// the same on MFMA for the bf16-mixed trainer (head dim 16): returns 1 (nothing launched) when the shape is not covered
int  te_attention_fwd(const PackInfo& pk, const float* qkv, int heads, float* out, float* stat, const TDrop& dr, unsigned site, hipStream_t s);
int  te_attention_bwd(const PackInfo& pk, const float* qkv, const float* O, const float* dO, int heads, float* dqkv, float* stat,
                      const TDrop& dr, unsigned site, hipStream_t s);
// loss = mean_valid CE(softmax(logits), label) and d loss / d logits (packed rows)
void t_pack_dlogits(const PackInfo& pk, const float* dlogits_padded, float* dlogits_p, hipStream_t s);
void t_loss_grad(const PackInfo& pk, const float* logits, const int32_t* labels, float* dlogits, float* loss, float* part,
                 hipStream_t s);                                                                             // part: grid-size floats of scratch
void t_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
                 int step, hipStream_t s);

// ---- bf16-STORAGE edge kernels of the bf16-mixed trainer (kernels_train.hip, last part).  Under the reference's bf16 autocast
// (rnampnn/utils/train.py:109) every nn.Linear output - hence the whole per-edge chain e, pre-activations and their gradients - is a
// bf16 tensor; here all [E][128] tensors of the ResMPNN layers are bf16 row-major in HBM (half the bytes of the f32 tape), f32
// only inside the kernels (MFMA accumulators, GELU, sums).  `tb16` = raw bf16 bits, round-to-nearest-even on store.
typedef unsigned short tb16;
struct EFuse {                       // optional epilogue fusions of te_gemm
    const tb16* P; const tb16* Q;    // v += P[row / k] + Q[nbr[row]]       (bf16 [N+1][128] each; row `zero_row` of Q = zeros)
    const int* nbr; int k; int zero_row;
    const tb16* res_in; tb16* res_out;   // res_out = res_in + (nbr[row] >= 0 ? drop(gelu(v), site2) : 0)     (edge update, mpnn.py:250-262)
    unsigned site2;
};
// Y[R][128] (bf16) = actA(X)[R][128] . W' + bias, [* gelu'(epi_pre) * mask(site)]; W' = W^T (w_rows: W [128][ldw] as
// nn.Linear stores it) or W (W [128][ldw] k-major).  X is bf16 (x_bf16) or f32, row stride ldx.  Returns false (nothing launched) for a
// combination of options that is not instantiated.
bool te_gemm(const TRows& rows, const void* X, bool x_bf16, int ldx, const float* W, int ldw, bool w_rows, const float* bias, tb16* Y,
             bool actA, const tb16* epi_pre, const EFuse* fuse, const TDrop& dr, unsigned site, TCall& cx, int kvalid = 128);   // kvalid: live columns of X (the rest is zero padding)
// dW[128][ldw] += A^T . actB(B), dbias += colsum(A)     (A, B bf16 [R][128])
void te_gemm_tn(const TRows& rows, const tb16* A, const tb16* B, float* dW, int ldw, bool actB, const TDrop& dr,
                unsigned site, float* dbias, TCall& cx, int cols_keep = 128);      // cols_keep: live columns of B
// the node-side GEMMs of a factored first Linear, each pair as one launch: P / Q tables, [dWa ; dWb] (+ db1), dh += dP Wa + dQ Wb
void te_gemm_pq(const TRows& rows, const float* h, const float* w0, const float* b1, tb16* Pt, tb16* Qt, TCall& cx);
void tm_gemm_tn_pq(const TRows& rows, const float* dpq, const float* h, float* gw0, float* db1, TCall& cx);
bool tm_gemm_nn_pq(const TRows& rows, const float* dpq, const float* w0, float* dh, hipStream_t s);
#define TE_DROPPED (-1.0e4f)         // taped in place of a dropped pre-activation: gelu_fast, gelu_d_fast and gelu_both_fast give exactly (-)0 there
// forward of a depth-2 per-edge MLP in one kernel (the hidden activation stays in registers; pre1 / pre2 written once as the tape;
// pre1 = null: not kept).  pre1 is taped with its dropped elements replaced by TE_DROPPED; with f.res_out (edge update) pre2 receives
// gelu'(pre2) * mask(site2) - the tapes te_gemm_bwd2 reads
void te_mlp2_fwd(const TRows& rows, const tb16* X, const float* W1, int ldw1, const float* W2, int ldw2, const float* bias2, tb16* pre1,
                 tb16* pre2, const EFuse& f, const TDrop& dr, unsigned site, TCall& cx);
// fused pair of a first Linear's backward: dW += dY^T X, DE += dY . W   (one pass over dY)
void te_gemm_bwd1(const TRows& rows, const tb16* dY, const tb16* X, tb16* DE, const float* W, int ldw, float* dW, int ldw_out, TCall& cx);
// fused pair of a depth-2 MLP's backward: dW += d pre2^T drop(gelu(PRE)), dbias += colsum(d pre2), DX = (d pre2 . W) gelu'(PRE) mask   (one pass
// over PRE).  d pre2 is formed on the fly while the tile is staged - mode 1: dY = d e_out, d pre2 = valid ? dY gelu'(pre2) mask(site2) : 0 (the
// edge update's residual backward); mode 2: d pre2 = valid ? dagg[row / k] inv_cnt[row / k] gelu'(pre2) mask(site2) : 0 (the message mean's).
// The `pre2` tensor holds gelu'(pre2) * mask(site2) as the forward left it (k_emm_fwd2 / k_eseg_mean, below) and PRE the TE_DROPPED tape of
// k_emm_fwd2: the staging pass multiplies, and evaluates no dropout hash
struct EBwd2Src { int mode; const tb16* pre2; const int* nbr; const float* dagg; const float* inv_cnt; int k; };
void te_gemm_bwd1x2(const TRows& rows, const tb16* dY1, const tb16* dY2, const tb16* X, tb16* DE, const float* W1, const float* W2, int ldw,
                    float* dW1, float* dW2, int ldw_out, TCall& cx);
void te_gemm_bwd2(const TRows& rows, const tb16* dY, const tb16* PRE, tb16* DX, const float* W, int ldw, float* dW, int ldw_out,
                  const TDrop& dr, float* dbias, TCall& cx, const EBwd2Src& from);
void te_inv_count(const PackInfo& pk, int k, const int* nbr, float* inv_cnt, hipStream_t s);   // 1 / max(#valid slots, 1) per residue
// g2_out (optional, may alias pre2): gelu'(pre2) * mask(site) per element - what the message MLP's backward needs of pre2
void te_seg_mean(const PackInfo& pk, int k, const int* nbr, const tb16* pre2, const float* h, float* out, const TDrop& dr, unsigned site, hipStream_t s,
                 tb16* g2_out = nullptr);
void te_seg_mean_bwd(const PackInfo& pk, int k, const int* nbr, const float* dagg, const tb16* pre2, tb16* dpre2, const TDrop& dr, unsigned site, hipStream_t s);
void te_edge_res_bwd(const PackInfo& pk, int k, const int* nbr, const tb16* de, const tb16* pre2, tb16* dpre2, const TDrop& dr, unsigned site, hipStream_t s);
void te_edge_pq_bwd(const PackInfo& pk, int k, const tb16* dpre1, const int* start, const int* list, float* dpq, hipStream_t s);
void te_edge_features(const PackInfo& pk, int k, const float* geom, const int* nbr, tb16* F, hipStream_t s);          // raw edge features, bf16 [E][128] (90 live columns)
void te_edge_act(const PackInfo& pk, int k, const int* nbr, const tb16* pre, tb16* out, const TDrop& dr, unsigned site, hipStream_t s);   // out = valid ? drop(gelu(pre)) : 0

// ---- cache of prebuilt bf16 fragment images of the 128 x 128 weight blocks the weights-resident GEMMs use (kernels_train.hip): a handle owns one
// and hands it to its calls (TCall::wimg); refresh at the start of a training forward (one launch rebuilds every image registered so far).
WImageCache* t_wimg_create(int capacity);
void t_wimg_destroy(WImageCache* c);
void t_wimg_clear(WImageCache* c);           // the weights moved (new arena)
void t_wimg_refresh(WImageCache* c, hipStream_t s);
int t_wimg_pending(const WImageCache* c);     // blocks registered since the last refresh (their kernels still build their own image)
