// Private to the two host translation units of the rnampnn C ABI: api.cpp (handle, weight registry, inference forward) and train.cpp
// (training path).  The model structure as rnampnn_create lays it out, the handle, and the error helper behind rnampnn_last_error.
#pragma once
#include "../../include/rnampnn_hip.h"
#include "rnampnn_internal.h"
#include "kernels_train.h"

#include <string>
#include <vector>

// records the text rnampnn_last_error returns (thread-local) and returns code.  ONE definition, in api.cpp, next to the buffer it fills; hidden:
// the library's dynamic symbol table does not grow by it
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) return fail(RNAMPNN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// splitmix64 finaliser: the counter hash behind the draws of k_sample (kernels_f32.hip) and k_design (design.hip)
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

struct RawT {                 // one state_dict entry in the reference's layout
    std::string key;
    int64_t numel;
    size_t off;               // float offset in the raw arena
    bool set;
};

struct Lin {                  // nn.Linear
    int in, out, in_pad;
    int w, b;                 // RawT indices
    size_t wt;                // derived: K-major f32 [in_pad][out]
    size_t wb;                // derived: bf16 [out][in_pad] (fast path; f16 when h16), or (size_t)-1
    bool gelu;
    bool h16 = false;         // fast path without a fused chain: f16 (not bf16) operands in launch_gemm_bf16 (the raw chain, api.cpp)
};
struct Chain {                // fused FFN chain of the fast path (kernels_bf16.hip: k_ffn_chain)
    bool ok = false;
    int K0 = 0, H = 0, NH = 0, NOUT = 0, n_valid = 0;
    size_t img = 0;           // derived: fragment image of all layers
    size_t last_bias = 0;     // derived: bias of the last Linear padded to NOUT
};
struct Attn { Lin qkv, out; int gn_scale, gn_shift; size_t img_qkv = 0, img_out = 0; };    // img_*: fragment images of the fused per-RNA layer kernel
struct Bert { std::vector<Attn> attn; std::vector<Lin> ffn; int heads; Chain chain; };
struct Mlp2 {                 // message_layers / edge_layers of one ResMPNN
    int depth;
    int w[2], b[2];           // RawT indices
    size_t pq_t, pq_b;        // derived f32: [128][256] K-major (P | Q parts of Linear 0), bias [b1 | 0]
    size_t wc_t, w2_t;        // derived f32: e-part of Linear 0 and Linear 1, K-major
    size_t pq_img;            // derived bf16 [P | Q] fragment image for the fused node-update kernel
    size_t pq_bp;             // derived f32 bias of Linear 0 in the order of that image's P rows
    size_t img;               // derived bf16 fragment image of (Wc, W2) for the fused edge kernel
    size_t b2p;               // derived f32 bias of Linear 1 in the kernel's channel order
};
struct MpnnLayer { int gn_scale, gn_shift; Mlp2 msg, edge; };

struct rnampnn_ctx {
    RnaMpnnConfig cfg;
    std::vector<RawT> raw;
    size_t raw_floats = 0;
    float* raw_arena = nullptr;
    size_t der_bytes = 0;
    char* der_arena = nullptr;
    bool finalized = false;
    // structure
    Lin raw_project;
    Bert emb, post;
    int feat_gn_scale, feat_gn_shift;
    std::vector<Lin> edge_embed;
    size_t edge_embed_img = 0;    // bf16 fragment image for the fast path
    size_t edge_embed_b1p = 0;    // bias of its second Linear in the kernel's channel order
    std::vector<MpnnLayer> mpnn;
    std::vector<Lin> raw_ffn;
    Chain raw_chain;
    int rawffn_gn_scale, rawffn_gn_shift;
    std::vector<Lin> readout;
    Chain readout_chain;
    int fmax = 0;                 // widest node activation
    // optional live timing of the dominant kernel (bench.py roofline leg)
    bool prof = false;
    int prof_stride = 1;          // time every prof_stride-th fused launch (events cost ~6 us of stream idle each)
    long long prof_seen = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    std::vector<unsigned char> ev_kind;   // per event pair: 0 = <edge update, message> launch, 1 = message-only / edge-only launch
    double prof_ms = 0.0, prof_ms_kind[2] = {0.0, 0.0};
    long long prof_n = 0, prof_n_kind[2] = {0, 0};
    // tapes of rnampnn_train_forward calls whose backward may still come (the activations themselves live in the caller's
    // workspaces): one record per workspace, identified by a monotonically increasing id that rnampnn_train_backward must present
    struct Tape { int64_t id; int B, T, tnorm; float p; uint64_t seed; const void* ws; bool mixed; const unsigned long long* seed_dev;
                  bool att_mfma; };     // att_mfma: which attention kernels wrote the (m, l) statistics of this tape - the backward must recompute S with the same ones
    std::vector<Tape> tapes;
    int64_t tape_counter = 0;
    // optional: events the backward records on its stream once a chunk of the flat gradient is final (rnampnn_grad_chunks),
    // so that the caller's all-reduce of that chunk can run on a side stream under the rest of the backward
    hipEvent_t grad_ev[2] = {nullptr, nullptr};
    const unsigned long long* seed_dev = nullptr;   // rnampnn_set_seed_source: the training kernels read the dropout seed from device memory
    WImageCache* wimg = nullptr;   // prebuilt weight-fragment images of the bf16-mixed trainer (kernels_train.h)
    bool raw_external = false;     // raw_arena is the caller's flat parameter buffer (rnampnn_use_weight_arena)
};

static inline float* rawp(rnampnn_ctx* c, int idx) { return c->raw_arena + c->raw[idx].off; }
template <typename T> static inline T* derp(rnampnn_ctx* c, size_t off) { return reinterpret_cast<T*>(c->der_arena + off); }
