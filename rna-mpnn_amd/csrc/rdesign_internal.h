// Declarations shared by the translation units of the `rdesign` path: rdesign.hip (handle, features, run set-up, the node-level Linear dispatch,
// inference forward), rdesign_train.hip (everything the two training steps share - checks, workspace, node side, loss, entry points - and the f32
// edge sequence), rdesign_train_bf16.hip (the bf16-mixed edge sequence and its kernels) and rdesign_score.hip (per-RNA metrics).
#pragma once
#include "../../include/rdesign_hip.h"
#include "rnampnn_internal.h"
#include "kernels_train.h"

#include <string>
#include <vector>

#define RD_H 128
#define RD_NODE 101
#define RD_NODEP 104
#define RD_EDGE 115
#define RD_EDGEP 116
#define RD_KMAX 64

int rd_fail(int code, const char* fmt, ...);          // records the text rdesign_last_error returns (thread-local), returns code
#define RD_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return rd_fail(RDESIGN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); } while (0)

struct RdT { std::string key; int64_t numel; size_t off; };
struct RdLin { int in, out, w, b; size_t wt; };          // wt: K-major f32 copy [in_pad][out] (f32 path, and K % 16 != 0 shapes)
struct RdLayer { int n1w, n1b, n2w, n2b; std::vector<RdLin> msg, dense; };
struct rdesign_ctx {
    RDesignConfig cfg;
    std::vector<RdT> raw;
    size_t raw_floats = 0, der_floats = 0;
    float* arena = nullptr;          // caller's flat parameter buffer
    float* der = nullptr;
    bool finalized = false;
    WImageCache* wimg = nullptr;     // prebuilt bf16 fragment images of the 128 x 128 weight blocks (bf16 path; kernels_train.h)
    bool wimg_fresh = false;         // images match the weights (reset by finalize)
    RdLin node_emb, edge_emb;
    int nn_g, nn_b, ne_g, ne_b;
    std::vector<RdLayer> layers;
    std::vector<RdLin> readout;
};
static inline float* rdp(rdesign_ctx* c, int i) { return c->arena + c->raw[i].off; }

struct RdWs {
    int *len, *cu, *node_b, *nbr;
    float *coords_p, *frame, *node_raw, *edge_raw, *hV, *hV2, *hE, *E1, *E2, *pq, *dh, *dA, *dB, *logits;
    size_t total;
};
size_t rd_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdWs* w, bool edges = true);

struct RdRun { rdesign_ctx* c; PackInfo pk; RdWs w; TCall cx; bool mixed; TDrop nodrop; int K; bool bad = false;
    TRows rn() const { return TRows{pk.cu + pk.B, 1, pk.Nmax}; }
    TRows re() const { return TRows{pk.cu + pk.B, K, pk.Nmax * K}; } };
// the run over a carved workspace: the call context (its stream; the bf16 callers hand it the handle's weight-image cache), precision, the
// no-dropout TDrop, K and the PackInfo of B x T padded rows on w's length tables
RdRun rd_run(rdesign_ctx* c, void* stream, bool mixed, const RdWs& w, int B, int T);
// One node-level Linear, one dispatch per GEMM: the MFMA form (tm_gemm_*) when r.mixed and the shape is covered, otherwise the f32 blocks.
// Y = [beta Y] + [drop(gelu(] X[:, 0:Kc] [))] . W[:, k0:k0+Kc]^T [+ b]; f32 form: t_gelu_fwd into `scratch` (may be X itself where X is not a taped
// pre-activation), t_gemm on the K-major copy.  ldx == width of the activation when gelu_in.
void rd_mm(RdRun& r, const TRows& rows, const float* X, int ldx, const RdLin& l, int k0, int Kc, bool use_bias, float* Y, int ldy, int beta,
           bool gelu_in, float* scratch, const TDrop& dr, unsigned site);
// dW += dy^T [drop(gelu(] x [))], db += colsum(dy) into the flat gradient; x = the Linear's input, or the taped pre-activation behind it (act)
void rd_mm_wb(RdRun& r, const TRows& rows, const float* dy, const RdLin& l, const float* x, bool act, float* scratch, const TDrop& dr, unsigned site,
              float* grad);
// dx = [beta dx] + dy . W [* gelu'(pre) * mask]      (pre: the taped pre-activation the Linear's input was the activation of; beta = 0 with it)
void rd_mm_dx(RdRun& r, const TRows& rows, const float* dy, const RdLin& l, float* dx, int beta, const float* pre, float* scratch, const TDrop& dr,
              unsigned site);

// RNAFeatures.forward up to the raw tensors (feature.py:157-233): lengths, packed coordinates and frames, k-NN table, w.node_raw / w.edge_raw;
// zeroes row Nmax of w.hV, w.hV2 and w.pq (the gather target of absent slots).  The caller has checked T against the k-NN kernel's LDS row.
void rd_front(RdRun& r, const float* X, const float* mask, int64_t* edge_index);
size_t rd_knn_lds_bytes(int T);
// row normalisations on 128-wide rows: mode 0 functional.Normalize, mode 1 nn.LayerNorm(x + res)
void rd_rownorm(const int* ntot, int mul, size_t maxrows, const float* x, const float* res, const float* gain, const float* bias, int mode,
                float* y, hipStream_t s, tb16* yb = nullptr);
// packed output: rows [0, *ntot * mul) of src (row stride ld_src floats) -> dst (row stride ld_dst), `width` floats each.  The row count is the device's
// (no host sync), so rows >= N of the caller's tensor are left untouched; maxrows sizes the grid.
void rd_copy_rows(const int* ntot, int mul, size_t maxrows, const float* src, int ld_src, float* dst, int ld_dst, int width, hipStream_t s);

// ---- shared by the two training steps (defined in rdesign_train.hip)
#define RDT_CE_BLOCKS 1024
struct RdtArgs { const float *X, *mask; const int32_t* labels; int32_t B, T; float dropout; uint64_t seed; float *loss, *logits, *grad;
                 void* ws; size_t ws_bytes; void* stream; };
struct RdtLayer { std::vector<float*> dense; float *dh, *h1, *y; };      // pre-activations of the hidden dense Linears, dh, norm1 output, dense output
struct RdtWs {                               // what both steps carve alike; the [E][128] tensors are carved behind it by the step that owns them
    RdWs f;                                  // the forward's buffers: features, k-NN table, P/Q table; its three [E][128] regions serve the edge side
    float* embN;                             // tape: node embedding Linear output (input of Normalize)
    std::vector<float*> hv;                  // tape: h_V entering layer l (hv[L] = the stack's output)
    std::vector<RdtLayer> layers;
    std::vector<float*> rpre;                // tape: hidden read-out pre-activations
    float *logits, *dlogits, *part;
    float *gH, *gX, *bA, *bB, *bC;           // node-sized gradient / scratch buffers ([N][128] and [N][Dm])
    int *rdeg, *rstart, *rfill, *rlist;      // reverse adjacency (t_build_reverse)
    TScratch sc;                             // arena of the ordered reductions
    char* base; size_t off, tape_bytes;      // carve state: every tensor is rounded to 256 bytes on its own; tape = kept between forward and backward
    char* take(size_t bytes, bool tape = false) {
        const size_t o = off, n = (bytes + 255) / 256 * 256;
        off += n;
        if (tape) tape_bytes += n;
        return base ? base + o : nullptr;
    }
    float* tf(size_t floats, bool tape = false) { return (float*)take(floats * sizeof(float), tape); }
};
// One training call.  Dropout addressing (restated by tests/_rdesign_train_ref.py): the TDrop counter hash; site = index of the Dropout module in
// forward order from 1 - layer l, message Linear i: 1 + l (M + D) + i; layer l, hidden dense Linear i: 1 + l (M + D) + M + i; hidden read-out
// Linear j: 1 + L (M + D) + j; element = row * width + channel, row = packed node row p or packed edge row p K + slot.
struct RdtStep {
    RdRun r; RdtWs w; TDrop dr; float* grad; int L, M, D;
    unsigned site_msg(int l, int i) const { return (unsigned)(1 + l * (M + D) + i); }
    unsigned site_dense(int l, int i) const { return site_msg(l, M + i); }
    unsigned site_ro(int j) const { return site_msg(L, j); }
    float* G(int i) const { return grad + r.c->raw[i].off; }          // gradient of raw tensor i in the flat buffer
};
int rdt_dm(const rdesign_ctx* c);                                  // widest node-level activation: max(128, dense width, hidden read-out width)
void rdt_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdtWs& w);
// the argument checks of a step (`need` = its carved byte count, `who` = the entry point named in the message), then the run over the carved w
int rdt_begin(RdtStep& t, rdesign_handle h, const RdtArgs& a, bool mixed, size_t need, const char* who);
// Node side.  A chain of Linears with GELU + Dropout between them (dense FFN, read-out): pre[i] = the taped pre-activation of hidden Linear i,
// site0 + i its Dropout.  Backward: dy = d out; dx = d x, added to what dx holds when `acc`.  Scratch: w.bA / w.bB / w.bC.
void rdt_ffn_fwd(RdtStep& t, const std::vector<RdLin>& lin, const float* x, const std::vector<float*>& pre, float* out, unsigned site0);
void rdt_ffn_bwd(RdtStep& t, const std::vector<RdLin>& lin, const float* x, const std::vector<float*>& pre, const float* dy, float* dx, bool acc,
                 unsigned site0);
void rdt_node_emb_bwd(RdtStep& t);                                 // w.gX = d (node embedding Linear output): the 101-input Linear's dW, db
// between forward and backward: logits copy-out (the N valid rows), loss and w.dlogits, zeroed gradient, red_begin on the
// queue of the step's own context (t.r.cx);  rdt_end: red_end of that queue
void rdt_loss(RdtStep& t, const RdtArgs& a);
int rdt_end(RdtStep& t, const char* who);
// the bf16-mixed step (rdesign_train_bf16.hip); sizes != null: no launch, sizes[0] = workspace bytes, sizes[1] = tape bytes
int rdb_step(rdesign_handle h, const RdtArgs& a, size_t* sizes);
