// Declarations shared by the translation units of the `rdesign` path: rdesign.hip (handle, features, inference forward), rdesign_train.hip
// (taped forward + backward of the f32 training step), rdesign_train_bf16.hip (the bf16-mixed training step) and rdesign_score.hip (per-RNA metrics).
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

struct RdRun { rdesign_ctx* c; PackInfo pk; RdWs w; hipStream_t s; bool mixed; TDrop nodrop; int K; bool bad = false;
    TRows rn() const { return TRows{pk.cu + pk.B, 1, pk.Nmax}; }
    TRows re() const { return TRows{pk.cu + pk.B, K, pk.Nmax * K}; } };

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
int rdt_dm(const rdesign_ctx* c);                                  // widest node-level activation: max(128, dense width, hidden read-out width)
int rdt_check_rows(rdesign_handle h, int32_t B, int32_t T);        // B, T > 0 and the row limits of the dropout hash / 32-bit edge indexing (h non-null)
// loss = mean over the valid residues of the cross-entropy, dlogits = d loss / d logits (packed rows); part: RDT_CE_BLOCKS floats of scratch
void rdt_ce_loss(const PackInfo& pk, const float* logits, const int32_t* labels, float* dlogits, float* part, float* loss, hipStream_t s);
