// bf16-MIXED TRAINING STEP of the `rdesign` model (C ABI: include/rdesign_hip.h, rdesign_loss_and_grad_ex with RDESIGN_TRAIN_BF16_MIXED): the job of
// rdesign_train.hip - taped forward with the same dropout sites and TDrop addressing, CrossEntropyLoss over the valid residues, the gradient of
// every parameter into ONE flat buffer - on the kernels of the main model's bf16-mixed trainer (kernels_train.h: te_* MFMA edge GEMMs with P / Q,
// GELU and dropout fused in, tm_* MFMA node GEMMs, the weight-image cache).  Every [E][128] tensor is bf16 (`tb16`) in HBM: h_E, the embedding
// Linear's output, the M message pre-activations per layer and their gradients; f32 lives inside the kernels only.  Node-level tensors stay f32.
// The exact-f32 step of rdesign_train.hip is this path's parity reference (tests/test_rdesign_train_bf16_gpu.py checks both against fp64).
//
// TAPE CONVENTION per tensor (layer l, message Linears 0 .. M-1, M = 2 | 3; any other depth is refused):
//   msg[i], i < M-1   pre-activation with its DROPPED elements replaced by TE_DROPPED (gelu = gelu' = exactly 0 there): msg[0] is written that way
//                     by te_mlp2_fwd; msg[1] of M = 3 is written plain by te_mlp2_fwd, read plain (+ hash) by the third Linear's operand load and
//                     then marked in place (k_rdb_mark_dropped) - te_gemm_bwd2 evaluates no hash on its PRE operand.  Kernels that do evaluate
//                     the hash (te_gemm_tn actB, te_gemm epi_pre) read the marked tape as well: the hash drops the same elements.
//   msg[M-1]          plain until the segment sum, which leaves gelu'(pre) * mask in its place (k_rdb_segsum, like te_seg_mean's g2_out): the
//                     form te_gemm_bwd2 mode 2 multiplies d dh / 30 with (the 1 / 30 rides in its per-residue table, a constant here).
//   embE              plain bf16 output of the 115-input Linear (input of Normalize); h_E = Normalize(embE) bf16.
// Backward of one layer: te_gemm_bwd2 mode 2 (last Linear: dW, db, d pre[M-2] in one pass); M = 3: the middle Linear takes its dY as given -
// te_gemm_tn (dW, db) + te_gemm with the gelu' * mask epilogue (d pre[0]); te_gemm_bwd1 (dW_e and d h_E of THIS layer into a zeroed bf16 buffer),
// k_rdb_acc adds that into the f32 accumulator of d h_E and re-zeroes it (the sum over the L layers is never rounded to bf16); te_edge_pq_bwd +
// tm_gemm_tn_pq / tm_gemm_nn_pq for the factored node side.  Dense FFN and read-out: tm_gemm_nt / _nn / _tn with GELU and dropout in the operand
// load; a shape they do not cover (the 4-wide read-out, the 101-input node embedding) takes the f32 block for that GEMM.  An edge kernel that
// refuses (te_gemm returning false) fails the call with RDESIGN_ERR_UNSUPPORTED.
// No float atomics: weight gradients go through the ordered reductions (red_begin .. red_end), the row-normalisation parameter gradients through
// fixed-order per-block partials.  No runtime fill / copy nodes: launch_zero_bytes / launch_copy_bytes.  No host synchronisation.
// PARITY: the p = 0 loss and gradients are pinned to the reference's own float64 autograd (tests/golden/rdesign_*.npz); the dropout masks are not
// (torch's RNG cannot be matched): with dropout the checker is the restatement tests/_rdesign_train_ref.py, itself pinned at p = 0.
#include "rdesign_internal.h"
#include "train_dev.h"

typedef __attribute__((ext_vector_type(2))) float rbf2;
typedef __attribute__((ext_vector_type(4))) float rbf4;
typedef __attribute__((ext_vector_type(4))) unsigned rbu4;
typedef __attribute__((ext_vector_type(2))) __bf16 rbb2;
__device__ __forceinline__ unsigned rb_pack2(float a, float b) {          // two round-to-nearest-even bf16 in one word (even channel low)
    rbf2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, rbb2));
}
__device__ __forceinline__ float rb_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float rb_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// ------------------------------------------------------------------------------------------ raw edge features as a bf16 GEMM operand
// F[e][0:128] (bf16) = edge_raw[e][0:115] | zeros: the operand te_gemm (kvalid 115) and te_gemm_tn (cols_keep 115) read.  One thread = 8 channels.
__global__ void __launch_bounds__(256) k_rdb_eraw16(const int* __restrict__ ntot_p, int K, const float* __restrict__ raw, tb16* __restrict__ F) {
    const size_t n = (size_t)*ntot_p * K * 16;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
        const size_t e = id >> 4;
        const int c = 8 * (int)(id & 15);
        const float* src = raw + e * RD_EDGEP + c;
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = c + q < RD_EDGE ? src[q] : 0.f;
        reinterpret_cast<rbu4*>(F)[id] = rbu4{rb_pack2(v[0], v[1]), rb_pack2(v[2], v[3]), rb_pack2(v[4], v[5]), rb_pack2(v[6], v[7])};
    }
}

// ------------------------------------------------------------------------------------------ functional.Normalize on bf16 rows
// y = gain (x - mean) / (sqrt(var_unbiased + 1e-6) + 1e-6) + bias (k_rd_rownorm mode 0) with x and y bf16: one wave per row, lane = two adjacent channels
__global__ void __launch_bounds__(256) k_rdb_normalize16(const int* __restrict__ ntot_p, int mul, const tb16* __restrict__ x, const float* __restrict__ gain,
                                                         const float* __restrict__ bias, tb16* __restrict__ y) {
    const size_t R = (size_t)*ntot_p * mul;
    const int lane = threadIdx.x & 63, c = 2 * lane;
    const rbf2 gw = *reinterpret_cast<const rbf2*>(gain + c), bw = *reinterpret_cast<const rbf2*>(bias + c);
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (size_t)gridDim.x * 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(x + row * RD_H + c);
        const float v0 = rb_lo(w), v1 = rb_hi(w);
        float s = v0 + v1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mu = s / 128.f;
        const float d0 = v0 - mu, d1 = v1 - mu;
        float q = d0 * d0 + d1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float inv = 1.0f / (sqrtf(q / 127.f + 1e-6f) + 1e-6f);
        *reinterpret_cast<unsigned*>(y + row * RD_H + c) = rb_pack2(gw[0] * d0 * inv + bw[0], gw[1] * d1 * inv + bw[1]);
    }
}

// ------------------------------------------------------------------------------------------ row-normalisation backward, bf16 or f32 rows
// The arithmetic of k_rdt_rownorm_bwd (rdesign_train.hip) with the taped input x bf16 (XB: the per-edge embE) or f32 (+ res), dx written as bf16
// (OB) or f32, and the two parameter gradients folded in: every block leaves the column sums of t = dy d / sig (d gain) and of dy (d bias) over
// ITS rows as one fixed-order partial [256]; k_rdb_norm_params adds the partials in block order.  (The f32 step writes t as an [R][128] tensor and
// sums it with t_colsum: 14 % of its kernel time.)  One wave per row, lane = two adjacent channels.
#define RDB_NORM_BLOCKS 512
template <bool XB, bool OB>
__global__ void __launch_bounds__(256) k_rdb_rownorm_bwd(const int* __restrict__ ntot_p, int mul, const void* __restrict__ xv, const float* __restrict__ res,
                                                         const float* __restrict__ dy, const float* __restrict__ gain, int mode, void* __restrict__ dxv,
                                                         float* __restrict__ part) {
    __shared__ float red[4][256];
    const size_t R = (size_t)*ntot_p * mul;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = 2 * lane;
    const rbf2 gw = *reinterpret_cast<const rbf2*>(gain + c);
    float sg0 = 0.f, sg1 = 0.f, sb0 = 0.f, sb1 = 0.f;
    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < R; row += (size_t)gridDim.x * 4) {
        float v0, v1;
        if constexpr (XB) {
            const unsigned w = *reinterpret_cast<const unsigned*>(reinterpret_cast<const tb16*>(xv) + row * RD_H + c);
            v0 = rb_lo(w); v1 = rb_hi(w);
        } else {
            const rbf2 w = *reinterpret_cast<const rbf2*>(reinterpret_cast<const float*>(xv) + row * RD_H + c);
            v0 = w[0]; v1 = w[1];
            if (res) { const rbf2 r2 = *reinterpret_cast<const rbf2*>(res + row * RD_H + c); v0 += r2[0]; v1 += r2[1]; }
        }
        const rbf2 yv = *reinterpret_cast<const rbf2*>(dy + row * RD_H + c);
        float s = v0 + v1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mu = s / 128.f;
        const float d0 = v0 - mu, d1 = v1 - mu;
        float q = d0 * d0 + d1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        float root, sig, n;
        if (mode == 0) { root = sqrtf(q / 127.f + 1e-6f); sig = root + 1e-6f; n = 127.f; }
        else { root = sqrtf(q / 128.f + 1e-5f); sig = root; n = 128.f; }
        const float inv = 1.0f / sig;
        const float g0 = yv[0] * gw[0], g1 = yv[1] * gw[1];
        float sg = g0 + g1, sgd = g0 * d0 + g1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o, 64); sgd += __shfl_xor(sgd, o, 64); }
        const float mg = sg / 128.f, k = sgd * inv * inv / (n * root);
        const float o0 = (g0 - mg) * inv - d0 * k, o1 = (g1 - mg) * inv - d1 * k;
        if constexpr (OB) *reinterpret_cast<unsigned*>(reinterpret_cast<tb16*>(dxv) + row * RD_H + c) = rb_pack2(o0, o1);
        else *reinterpret_cast<rbf2*>(reinterpret_cast<float*>(dxv) + row * RD_H + c) = rbf2{o0, o1};
        sg0 += yv[0] * d0 * inv; sg1 += yv[1] * d1 * inv;
        sb0 += yv[0]; sb1 += yv[1];
    }
    red[wave][c] = sg0; red[wave][c + 1] = sg1; red[wave][128 + c] = sb0; red[wave][128 + c + 1] = sb1;
    __syncthreads();
    const int t = threadIdx.x;
    part[(size_t)blockIdx.x * 256 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
// dgain[c] = sum over the blocks, in block order, of part[b][c]; dbias[c] likewise of part[b][128 + c]      (one 256-thread block)
__global__ void __launch_bounds__(256) k_rdb_norm_params(const float* __restrict__ part, int nblocks, float* __restrict__ dgain, float* __restrict__ dbias) {
    const int t = threadIdx.x;
    float s = 0.f;
#pragma unroll 8
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * 256 + t];
    if (t < 128) dgain[t] = s; else dbias[t - 128] = s;
}

// ------------------------------------------------------------------------------------------ segment sum with dropout on the bf16 tape
// dh[p][c] = sum over the valid slots of drop(GELU(pre[(p, s)][c]), site) / scale (mpnn.py:18,32-33) and, in place of pre, g = gelu'(pre) * mask for the
// valid slots, 0 for the absent ones: all the backward needs of the last message pre-activation.  One wave per residue, lane = two adjacent
// channels; the K validity flags in one load + ballot (K <= 64), unconditional row loads (the scheme of k_eseg_mean, kernels_train.hip).
__global__ void __launch_bounds__(256) k_rdb_segsum(PackInfo pk, int K, const int* __restrict__ nbr, tb16* pre, float inv_scale, float* __restrict__ out,
                                                    TDrop dr, unsigned site) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= pk.cu[pk.B]) return;
    const int lane = threadIdx.x & 63, c = 2 * lane;
    const unsigned key = drop_key(dr, site);
    const unsigned long long vm = __ballot(lane < K && nbr[(size_t)p * K + (lane < K ? lane : 0)] >= 0);
    tb16* base = pre + (size_t)p * K * RD_H + c;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 5
    for (int sl = 0; sl < K; ++sl) {
        const unsigned w = *reinterpret_cast<const unsigned*>(base + (size_t)sl * RD_H);
        float m0, m1;
        drop_pair(dr, key, (unsigned)(p * K + sl) * 64u + lane, m0, m1);
        const bool valid = (vm >> sl) & 1ull;               // (a select: an absent slot's row may hold anything)
        const float x0 = rb_lo(w), x1 = rb_hi(w);
        s0 += valid ? gelu_fast(x0) * m0 : 0.f;
        s1 += valid ? gelu_fast(x1) * m1 : 0.f;
        *reinterpret_cast<unsigned*>(base + (size_t)sl * RD_H) = valid ? rb_pack2(gelu_d_fast(x0) * m0, gelu_d_fast(x1) * m1) : 0u;
    }
    *reinterpret_cast<rbf2*>(out + (size_t)p * RD_H + c) = rbf2{s0 * inv_scale, s1 * inv_scale};
}

// ------------------------------------------------------------------------------------------ element-wise helpers of the edge chain
// pre[e][c] = TE_DROPPED where dropout site `site` drops element (e, c): the tape form te_gemm_bwd2 reads without a hash.  16-byte units.
__global__ void __launch_bounds__(256) k_rdb_mark_dropped(const int* __restrict__ ntot_p, int K, tb16* __restrict__ pre, TDrop dr, unsigned site) {
    const size_t n = (size_t)*ntot_p * K * 16;
    const unsigned key = drop_key(dr, site);
    const unsigned dropped = rb_pack2(TE_DROPPED, TE_DROPPED);
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
        rbu4 v = reinterpret_cast<const rbu4*>(pre)[id];
        float dm[8];
        drop8(dr, key, (unsigned)id, dm);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned lo = dm[2 * q] == 0.f ? (dropped & 0xffffu) : (v[q] & 0xffffu);
            const unsigned hi = dm[2 * q + 1] == 0.f ? (dropped & 0xffff0000u) : (v[q] & 0xffff0000u);
            v[q] = lo | hi;
        }
        reinterpret_cast<rbu4*>(pre)[id] = v;
    }
}
// acc[e][c] = (first ? 0 : acc[e][c]) + de[e][c];  de = 0: the f32 accumulator of d h_E over the L layers; te_gemm_bwd1 ADDS into its bf16 DE
// output, which therefore holds one layer's share only and is handed back zeroed.  One thread = 8 channels.
__global__ void __launch_bounds__(256) k_rdb_acc(const int* __restrict__ ntot_p, int K, tb16* __restrict__ de, float* __restrict__ acc, int first) {
    const size_t n = (size_t)*ntot_p * K * 16;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
        const rbu4 v = reinterpret_cast<const rbu4*>(de)[id];
        rbf4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (!first) { a = reinterpret_cast<const rbf4*>(acc)[2 * id]; b = reinterpret_cast<const rbf4*>(acc)[2 * id + 1]; }
        a[0] += rb_lo(v[0]); a[1] += rb_hi(v[0]); a[2] += rb_lo(v[1]); a[3] += rb_hi(v[1]);
        b[0] += rb_lo(v[2]); b[1] += rb_hi(v[2]); b[2] += rb_lo(v[3]); b[3] += rb_hi(v[3]);
        reinterpret_cast<rbf4*>(acc)[2 * id] = a; reinterpret_cast<rbf4*>(acc)[2 * id + 1] = b;
        reinterpret_cast<rbu4*>(de)[id] = rbu4{0u, 0u, 0u, 0u};
    }
}
// t[i] = v for i < n: the per-residue table of te_gemm_bwd2 mode 2 (1 / scale for every residue here, 1 / count in the main model)
__global__ void k_rdb_fill(float* __restrict__ t, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = v;
}

// ------------------------------------------------------------------------------------------ workspace
namespace {
struct RdbLayer { std::vector<tb16*> msg; std::vector<float*> dense; float *dh, *h1, *y; };
struct RdbWs {
    RdWs f;                                  // the forward's buffers; its three [E][128] f32 regions are split into six bf16 ones (below)
    float* embN; tb16* embE;                 // tape: embedding Linear outputs (inputs of the two Normalize)
    std::vector<float*> hv;                  // tape: h_V entering layer l (hv[L] = the stack's output)
    std::vector<RdbLayer> layers;
    std::vector<float*> rpre;
    float *logits, *dlogits, *part;
    float *gH, *gX, *bA, *bB, *bC;           // node-sized gradient / scratch buffers
    float *dhE, *dpq, *inv_scale, *npart;    // f32 accumulator of d h_E; [N][256] d P | d Q; the 1 / 30 table; partials of the norm parameter gradients
    tb16 *hE, *de, *eraw, *dA, *dB;          // bf16 [E][128]: h_E, one layer's d h_E, raw edge features, two gradient buffers (views of f.hE / f.E1 / f.E2)
    int *rdeg, *rstart, *rfill, *rlist;
    TScratch sc;
    size_t tape_bytes;
};
size_t rdb_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdbWs* out) {
    RdbWs tmp;
    RdbWs& w = out ? *out : tmp;
    size_t off = rd_carve(c, B, Nmax, base, &w.f);
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return base ? base + o : (char*)nullptr; };
    auto tf = [&](size_t floats) { return (float*)take(floats * sizeof(float)); };
    auto tb = [&](size_t halves) { return (tb16*)take(halves * sizeof(tb16)); };
    const RDesignConfig& g = c->cfg;
    const size_t E = Nmax * g.k_neighbors, NH = Nmax * RD_H, EH = E * RD_H, Dm = (size_t)rdt_dm(c);
    const size_t tape0 = off;
    w.embN = tf(NH); w.embE = tb(EH);
    w.hv.clear(); w.layers.clear(); w.rpre.clear();
    for (int l = 0; l <= g.num_mpnn_layers; ++l) w.hv.push_back(tf(NH));
    for (int l = 0; l < g.num_mpnn_layers; ++l) {
        RdbLayer L;
        for (int i = 0; i < g.num_message_layers; ++i) L.msg.push_back(tb(EH));
        for (int i = 0; i < g.num_dense_layers; ++i) L.dense.push_back(tf(Nmax * g.dim_dense_layers));
        L.dh = tf(NH); L.h1 = tf(NH); L.y = tf(NH);
        w.layers.push_back(L);
    }
    for (int j = 0; j + 1 < g.num_readout_layers; ++j) w.rpre.push_back(tf(Nmax * g.readout_hidden_dim));
    w.logits = tf(Nmax * 4);
    w.tape_bytes = off - tape0;
    w.dlogits = tf(Nmax * 4); w.part = tf(RDT_CE_BLOCKS);
    w.gH = tf(NH); w.gX = tf(NH); w.bA = tf(Nmax * Dm); w.bB = tf(Nmax * Dm); w.bC = tf(Nmax * Dm);
    w.dhE = tf(EH); w.dpq = tf(Nmax * 256); w.inv_scale = tf(Nmax); w.npart = tf((size_t)RDB_NORM_BLOCKS * 256);
    // each f32 [E][128] region of the forward's workspace holds two bf16 ones
    w.hE = reinterpret_cast<tb16*>(w.f.hE); w.de = base ? w.hE + EH : nullptr;
    w.eraw = reinterpret_cast<tb16*>(w.f.E1); w.dA = base ? w.eraw + EH : nullptr;
    w.dB = reinterpret_cast<tb16*>(w.f.E2);                                        // (before the first layer: scratch of t_build_reverse)
    w.rdeg = (int*)take((Nmax + 1) * sizeof(int)); w.rstart = (int*)take((Nmax + 1) * sizeof(int)); w.rfill = (int*)take((Nmax + 1) * sizeof(int));
    w.rlist = (int*)take((E + 1) * sizeof(int));
    w.sc.floats = RED_VIEW;
    w.sc.p = tf(w.sc.floats);
    return off;
}
int rdb_check(rdesign_handle h, int32_t B, int32_t T) {
    if (!h) return rd_fail(RDESIGN_ERR_BAD_ARG, "null handle");
    if (h->cfg.num_message_layers != 2 && h->cfg.num_message_layers != 3)
        return rd_fail(RDESIGN_ERR_UNSUPPORTED, "the bf16-mixed rdesign training step is built for num_message_layers 2 and 3 (got %d): train with RDESIGN_TRAIN_F32",
                       h->cfg.num_message_layers);
    return rdt_check_rows(h, B, T);
}
unsigned ew_grid(size_t units) { const size_t g = (units + 255) / 256; return (unsigned)(g < 16384 ? (g ? g : 1) : 16384); }
unsigned row_grid(size_t maxrows, size_t cap) { size_t g = (maxrows + 3) / 4; if (g > cap) g = cap; return (unsigned)(g ? g : 1); }

int rdb_loss_and_grad(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T, float dropout, uint64_t seed,
                      float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    if (const int rc = rdb_check(h, B, T)) return rc;
    if (!X || !mask || !labels || !loss || !grad || !ws) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_loss_and_grad_ex: null pointer");
    if (!(dropout >= 0.f && dropout < 1.f)) return rd_fail(RDESIGN_ERR_BAD_ARG, "dropout must be in [0, 1)");
    if (!h->arena) return rd_fail(RDESIGN_ERR_WEIGHTS, "no weight arena set");
    if (!h->finalized) return rd_fail(RDESIGN_ERR_WEIGHTS, "weights not finalized (call rdesign_finalize_weights)");
    if (((uintptr_t)grad & 15) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "gradient buffer must be 16-byte aligned");
    rdesign_ctx* c = h;
    const RDesignConfig& g = c->cfg;
    const size_t Nmax = (size_t)B * T;
    const int K = g.k_neighbors, L = g.num_mpnn_layers, M = g.num_message_layers, D = g.num_dense_layers;
    const size_t need = rdb_carve(c, B, Nmax, nullptr, nullptr);
    if (ws_bytes < need) return rd_fail(RDESIGN_ERR_WORKSPACE, "training workspace %zu bytes < required %zu", ws_bytes, need);
    if (((uintptr_t)ws & 255) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    if (rd_knn_lds_bytes(T) > 160 * 1024 - 256) return rd_fail(RDESIGN_ERR_UNSUPPORTED, "max_len %d too long for the LDS-resident k-NN row", T);
    RdbWs w;
    rdb_carve(c, B, Nmax, (char*)ws, &w);
    RdRun r;
    r.c = c; r.s = (hipStream_t)stream; r.mixed = true; r.nodrop = TDrop{0ull, 0u, 1.f, nullptr}; r.K = K; r.w = w.f;
    r.pk.len = w.f.len; r.pk.cu = w.f.cu; r.pk.node_b = w.f.node_b; r.pk.B = B; r.pk.T = T; r.pk.Nmax = (int)Nmax; r.pk.packed_in = 0;
    hipStream_t s = r.s;
    const PackInfo& pk = r.pk;
    const int* ntot = pk.cu + B;
    const TRows rn = r.rn(), re = r.re();
    const TDrop dr = t_drop(dropout, seed);
    const TDrop nodrop = r.nodrop;
    const size_t Emax = Nmax * K;
    auto site_msg = [&](int l, int i) { return (unsigned)(1 + l * (M + D) + i); };
    auto site_dense = [&](int l, int i) { return (unsigned)(1 + l * (M + D) + M + i); };
    auto site_ro = [&](int j) { return (unsigned)(1 + L * (M + D) + j); };
    bool bad = false;                        // an edge kernel refused its configuration: reported after the launch sequence (nothing of it ran)
    // the weights change every step: every fragment image registered so far is rebuilt from the arena, blocks first seen in this call build their own
    if (!c->wimg) c->wimg = t_wimg_create(256);
    if (c->wimg) { t_wimg_refresh(c->wimg, s); c->wimg_fresh = true; }
    t_wimg_bind(c->wimg);

    // Y = [drop(gelu(] X [))] . W^T + bias on the MFMA node GEMM; a shape it does not cover takes the f32 block on the K-major copy finalize built
    auto lin_fwd = [&](const float* Xin, int ldx, const RdLin& l, bool act, unsigned site, float* Y) {
        if (tm_gemm_nt(rn, Xin, ldx, l.in, rdp(c, l.w), l.in, rdp(c, l.b), l.out, Y, l.out, 0, act, dr, site, s)) return;
        const float* xin = Xin;
        if (act) { t_gelu_fwd(rn, Xin, w.bC, ldx, dr, site, s); xin = w.bC; }
        t_gemm(rn, xin, ldx, (l.in + 3) / 4 * 4, c->der + l.wt, l.out, rdp(c, l.b), l.out, Y, l.out, 0, s);
    };
    const unsigned seg_grid = (unsigned)((Nmax + 3) / 4);

    // ================================================================ taped forward
    rd_front(r, X, mask, nullptr);
    t_build_reverse(pk, K, w.f.nbr, w.rdeg, w.rstart, w.rfill, w.rlist, reinterpret_cast<int*>(w.f.E2), s);
    hipLaunchKernelGGL(k_rdb_fill, dim3((unsigned)((Nmax + 255) / 256)), dim3(256), 0, s, w.inv_scale, (int)Nmax, 1.0f / 30.0f);
    launch_zero_bytes(w.de, Emax * RD_H * sizeof(tb16), s);
    // node embedding (101 inputs: f32 block) + Normalize
    t_gemm(rn, w.f.node_raw, RD_NODEP, RD_NODEP, c->der + c->node_emb.wt, RD_H, rdp(c, c->node_emb.b), RD_H, w.embN, RD_H, 0, s);
    rd_rownorm(ntot, 1, Nmax, w.embN, nullptr, rdp(c, c->nn_g), rdp(c, c->nn_b), 0, w.hv[0], s);
    // edge embedding (115 inputs) on the MFMA edge GEMM + Normalize, bf16 rows
    hipLaunchKernelGGL(k_rdb_eraw16, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, w.f.edge_raw, w.eraw);
    bad |= !te_gemm(re, w.eraw, true, RD_H, rdp(c, c->edge_emb.w), RD_EDGE, true, rdp(c, c->edge_emb.b), w.embE, false, nullptr, nullptr, nodrop, 0u, s, RD_EDGE);
    hipLaunchKernelGGL(k_rdb_normalize16, dim3(row_grid(Emax, 8192)), dim3(256), 0, s, ntot, K, w.embE, rdp(c, c->ne_g), rdp(c, c->ne_b), w.hE);
    tb16* Pt = reinterpret_cast<tb16*>(w.f.pq);
    tb16* Qt = Pt + (Nmax + 1) * RD_H;                       // (row Nmax of Q: zeros, the gather target of absent slots - rd_front)
    for (int l = 0; l < L; ++l) {
        const RdLayer& Lw = c->layers[l];
        RdbLayer& t = w.layers[l];
        const float* hv = w.hv[l];
        const float* w0 = rdp(c, Lw.msg[0].w);               // [128][384] = [W_e | W_centre | W_neighbour]
        te_gemm_pq(rn, hv, w0 + RD_H, rdp(c, Lw.msg[0].b), Pt, Qt, s);
        const EFuse f{Pt, Qt, w.f.nbr, K, (int)Nmax, nullptr, nullptr, 0u};
        // Linears 0 and 1 in one kernel: msg[0] taped with TE_DROPPED marks, msg[1] plain
        te_mlp2_fwd(re, w.hE, w0, 3 * RD_H, rdp(c, Lw.msg[1].w), RD_H, rdp(c, Lw.msg[1].b), t.msg[0], t.msg[1], f, dr, site_msg(l, 0), s);
        if (M == 3) {
            bad |= !te_gemm(re, t.msg[1], true, RD_H, rdp(c, Lw.msg[2].w), RD_H, true, rdp(c, Lw.msg[2].b), t.msg[2], true, nullptr, nullptr, dr, site_msg(l, 1), s);
            if (dr.thresh) hipLaunchKernelGGL(k_rdb_mark_dropped, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, t.msg[1], dr, site_msg(l, 1));
        }
        hipLaunchKernelGGL(k_rdb_segsum, dim3(seg_grid), dim3(256), 0, s, pk, K, w.f.nbr, t.msg[M - 1], 1.0f / 30.0f, t.dh, dr, site_msg(l, M - 1));
        rd_rownorm(ntot, 1, Nmax, hv, t.dh, rdp(c, Lw.n1w), rdp(c, Lw.n1b), 1, t.h1, s);                    // norm1(h_V + dh)
        const float* x = t.h1;
        int ld = RD_H;
        for (int i = 0; i <= D; ++i) {
            float* y = i < D ? t.dense[i] : t.y;
            lin_fwd(x, ld, Lw.dense[i], i > 0, i > 0 ? site_dense(l, i - 1) : 0u, y);
            x = y; ld = Lw.dense[i].out;
        }
        rd_rownorm(ntot, 1, Nmax, t.h1, t.y, rdp(c, Lw.n2w), rdp(c, Lw.n2b), 1, w.hv[l + 1], s);            // norm2(h_V + dense(h_V))
    }
    const int R = (int)c->readout.size();
    {
        const float* x = w.hv[L];
        int ld = RD_H;
        for (int j = 0; j < R; ++j) {
            float* y = j + 1 < R ? w.rpre[j] : w.logits;
            lin_fwd(x, ld, c->readout[j], j > 0, j > 0 ? site_ro(j - 1) : 0u, y);
            x = y; ld = c->readout[j].out;
        }
    }
    if (logits) rd_copy_rows(pk.cu + B, 1, Nmax, w.logits, 4, logits, 4, 4, s);      // rows >= N of the caller's tensor stay untouched

    // ================================================================ loss and backward
    rdt_ce_loss(pk, w.logits, labels, w.dlogits, w.part, loss, s);
    launch_zero_bytes(grad, c->raw_floats * sizeof(float), s);
    auto G = [&](int i) { return grad + c->raw[i].off; };
    red_begin(w.sc, s);
    // dW += dy^T [drop(gelu(] x [))], db += colsum(dy) of one node-level Linear; x = the Linear's input, or the taped pre-activation behind it (act)
    auto lin_wb = [&](const float* dy, const RdLin& l, const float* x, int ldx, bool act, unsigned site) {
        if (tm_gemm_tn(rn, dy, l.out, l.out, x, ldx, l.in, G(l.w), l.in, act, dr, site, G(l.b), s)) return;
        const float* xin = x;
        if (act) { t_gelu_fwd(rn, x, w.bC, ldx, dr, site, s); xin = w.bC; }
        t_gemm_tn(rn, dy, l.out, l.out, xin, ldx, l.in, G(l.w), l.in, s);
        t_colsum(rn, dy, l.out, l.out, G(l.b), s);
    };
    // dx = [beta dx] + dy . W [* gelu'(pre) * mask]      (pre: the taped pre-activation the Linear's input was the activation of; beta = 0 with it)
    auto lin_dx = [&](const float* dy, const RdLin& l, float* dx, int beta, const float* pre, unsigned site) {
        if (tm_gemm_nn(rn, dy, l.out, l.out, rdp(c, l.w), l.in, nullptr, l.in, dx, l.in, beta, pre, l.in, dr, site, s)) return;
        if (!pre) { t_gemm(rn, dy, l.out, l.out, rdp(c, l.w), l.in, nullptr, l.in, dx, l.in, beta, s); return; }
        t_gemm(rn, dy, l.out, l.out, rdp(c, l.w), l.in, nullptr, l.in, w.bC, l.in, 0, s);
        t_gelu_bwd(rn, w.bC, pre, dx, l.in, dr, site, s);
    };
    // row-normalisation backward with the parameter gradients: fixed-order partials per block, then one block adds them in order
    auto norm_bwd = [&](bool edge, const void* x, const float* res, const float* dy, int gain_i, int bias_i, int mode, void* dx) {
        const unsigned grid = row_grid(edge ? Emax : Nmax, RDB_NORM_BLOCKS);
        if (edge) hipLaunchKernelGGL((k_rdb_rownorm_bwd<true, true>), dim3(grid), dim3(256), 0, s, ntot, K, x, res, dy, rdp(c, gain_i), mode, dx, w.npart);
        else hipLaunchKernelGGL((k_rdb_rownorm_bwd<false, false>), dim3(grid), dim3(256), 0, s, ntot, 1, x, res, dy, rdp(c, gain_i), mode, dx, w.npart);
        hipLaunchKernelGGL(k_rdb_norm_params, dim3(1), dim3(256), 0, s, w.npart, (int)grid, G(gain_i), G(bias_i));
    };
    // ---- read-out
    {
        const float* dy = w.dlogits;
        float* bufs[2] = {w.bA, w.bB};
        for (int j = R - 1; j >= 0; --j) {
            const RdLin& l = c->readout[j];
            lin_wb(dy, l, j > 0 ? w.rpre[j - 1] : w.hv[L], l.in, j > 0, j > 0 ? site_ro(j - 1) : 0u);
            if (j > 0) { float* dx = bufs[j & 1]; lin_dx(dy, l, dx, 0, w.rpre[j - 1], site_ro(j - 1)); dy = dx; }
            else lin_dx(dy, l, w.gH, 0, nullptr, 0u);
        }
    }
    // ---- L x MPNNLayer, last first; w.gH = d loss / d (h_V leaving the layer)
    for (int l = L - 1; l >= 0; --l) {
        const RdLayer& Lw = c->layers[l];
        RdbLayer& t = w.layers[l];
        norm_bwd(false, t.h1, t.y, w.gH, Lw.n2w, Lw.n2b, 1, w.gX);                                           // norm2(h1 + y)
        // dense FFN: w.gX is both d y and the residual part of d h1
        {
            const float* dy = w.gX;
            float* bufs[2] = {w.bA, w.bB};
            for (int i = D; i >= 0; --i) {
                const RdLin& lin = Lw.dense[i];
                lin_wb(dy, lin, i > 0 ? t.dense[i - 1] : t.h1, lin.in, i > 0, i > 0 ? site_dense(l, i - 1) : 0u);
                if (i > 0) { float* dx = bufs[i & 1]; lin_dx(dy, lin, dx, 0, t.dense[i - 1], site_dense(l, i - 1)); dy = dx; }
                else lin_dx(dy, lin, w.gX, dy == w.gX ? 0 : 1, nullptr, 0u);
            }
        }
        norm_bwd(false, w.hv[l], t.dh, w.gX, Lw.n1w, Lw.n1b, 1, w.gH);                                       // norm1(h_V + dh): w.gH <- d (h_V + dh)
        // last message Linear: d pre[M-1] = valid ? gH[row / K] / 30 * g : 0 formed while its tile is staged; dW, db, d pre[M-2] in one pass
        const RdLin& last = Lw.msg[M - 1];
        te_gemm_bwd2(re, nullptr, t.msg[M - 2], w.dA, rdp(c, last.w), RD_H, G(last.w), RD_H, dr, G(last.b), s,
                     EBwd2Src{2, t.msg[M - 1], w.f.nbr, w.gH, w.inv_scale, K});
        tb16* dpre0 = w.dA;
        if (M == 3) {       // the middle Linear takes its dY as given: weight gradient and input gradient as two passes over it
            const RdLin& mid = Lw.msg[1];
            te_gemm_tn(re, w.dA, t.msg[0], G(mid.w), RD_H, true, dr, site_msg(l, 0), G(mid.b), s);
            bad |= !te_gemm(re, w.dA, true, RD_H, rdp(c, mid.w), RD_H, false, nullptr, w.dB, false, t.msg[0], nullptr, dr, site_msg(l, 0), s);
            dpre0 = w.dB;
        }
        // factored first Linear: pre0 = W_e h_E + (W_c h_V + b)[centre] + (W_n h_V)[neighbour]
        const RdLin& l0 = Lw.msg[0];
        const float* w0 = rdp(c, l0.w);
        te_gemm_bwd1(re, dpre0, w.hE, w.de, w0, 3 * RD_H, G(l0.w), 3 * RD_H, s);                             // dW_e, this layer's d h_E
        hipLaunchKernelGGL(k_rdb_acc, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, w.de, w.dhE, l == L - 1 ? 1 : 0);
        te_edge_pq_bwd(pk, K, dpre0, w.rstart, w.rlist, w.dpq, s);                                           // dP = own slots, dQ = gather over the reverse adjacency
        tm_gemm_tn_pq(rn, w.dpq, w.hv[l], G(l0.w) + RD_H, G(l0.b), s);                                       // [dW_c ; dW_n], db (the bias rides in P)
        if (!tm_gemm_nn_pq(rn, w.dpq, w0 + RD_H, w.gH, s)) {                                                 // d h_V += dP W_c + dQ W_n
            t_gemm(rn, w.dpq, 256, RD_H, w0 + RD_H, l0.in, nullptr, RD_H, w.gH, RD_H, 1, s);
            t_gemm(rn, w.dpq + RD_H, 256, RD_H, w0 + 2 * RD_H, l0.in, nullptr, RD_H, w.gH, RD_H, 1, s);
        }
    }
    // ---- embeddings: Normalize backward, then the 101- / 115-input Linears (nothing flows into the raw features)
    norm_bwd(false, w.embN, nullptr, w.gH, c->nn_g, c->nn_b, 0, w.gX);
    t_gemm_tn(rn, w.gX, RD_H, RD_H, w.f.node_raw, RD_NODEP, RD_NODE, G(c->node_emb.w), RD_NODE, s);
    t_colsum(rn, w.gX, RD_H, RD_H, G(c->node_emb.b), s);
    norm_bwd(true, w.embE, nullptr, w.dhE, c->ne_g, c->ne_b, 0, w.dB);
    te_gemm_tn(re, w.dB, w.eraw, G(c->edge_emb.w), RD_EDGE, false, nodrop, 0u, G(c->edge_emb.b), s, RD_EDGE);
    const bool red_ok = red_end();
    t_wimg_bind(nullptr);
    if (!red_ok) return rd_fail(RDESIGN_ERR_HIP, "rdesign_loss_and_grad_ex: an ordered reduction was refused (reduction arena)");
    if (bad) return rd_fail(RDESIGN_ERR_UNSUPPORTED, "bf16-mixed training step: an MFMA edge GEMM variant this configuration needs is not built");
    RD_TRY(hipGetLastError());
    return RDESIGN_OK;
}
}  // namespace

extern "C" size_t rdesign_train_workspace_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags) {
    if (flags == RDESIGN_TRAIN_F32) return rdesign_train_workspace_bytes(h, B, T);
    if (flags != RDESIGN_TRAIN_BF16_MIXED) { rd_fail(RDESIGN_ERR_BAD_ARG, "unknown training flags %d", flags); return 0; }
    if (rdb_check(h, B, T) != RDESIGN_OK) return 0;
    return rdb_carve(h, B, (size_t)B * T, nullptr, nullptr);
}
extern "C" size_t rdesign_train_tape_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags) {
    if (flags == RDESIGN_TRAIN_F32) return rdesign_train_tape_bytes(h, B, T);
    if (flags != RDESIGN_TRAIN_BF16_MIXED) { rd_fail(RDESIGN_ERR_BAD_ARG, "unknown training flags %d", flags); return 0; }
    if (rdb_check(h, B, T) != RDESIGN_OK) return 0;
    RdbWs w;
    rdb_carve(h, B, (size_t)B * T, nullptr, &w);
    return w.tape_bytes;
}
extern "C" int rdesign_loss_and_grad_ex(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T, float dropout,
                                        uint64_t seed, int32_t flags, float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    if (flags == RDESIGN_TRAIN_F32) return rdesign_loss_and_grad(h, X, mask, labels, B, T, dropout, seed, loss, logits, grad, ws, ws_bytes, stream);
    if (flags != RDESIGN_TRAIN_BF16_MIXED) return rd_fail(RDESIGN_ERR_BAD_ARG, "unknown training flags %d", flags);
    return rdb_loss_and_grad(h, X, mask, labels, B, T, dropout, seed, loss, logits, grad, ws, ws_bytes, stream);
}
