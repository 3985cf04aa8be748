// bf16-MIXED TRAINING STEP of the `rdesign` model (C ABI: include/rdesign_hip.h, rdesign_loss_and_grad_ex with RDESIGN_TRAIN_BF16_MIXED): the edge
// sequence of the step on the kernels of the main model's bf16-mixed trainer (kernels_train.h: te_* MFMA edge GEMMs with P / Q, GELU and dropout
// fused in, the weight-image cache), readable top to bottom around what it shares with the exact-f32 step (rdesign_train.hip: checks, workspace,
// dropout sites, node side, loss, entry points; rd_mm* take the tm_* MFMA node GEMMs here).  Every [E][128] tensor is bf16 (`tb16`) in HBM: h_E,
// the embedding Linear's output, the M message pre-activations per layer and their gradients; f32 lives inside the kernels only.  Node-level
// tensors stay f32.  The exact-f32 step is this path's parity reference (tests/test_rdesign_train_bf16_gpu.py checks both against fp64).
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
// tm_gemm_tn_pq / tm_gemm_nn_pq for the factored node side.  An edge kernel that refuses (te_gemm returning false) fails the call with
// RDESIGN_ERR_UNSUPPORTED.
// No float atomics: weight gradients go through the ordered reductions (rdt_loss .. rdt_end), the row-normalisation parameter gradients through
// fixed-order per-block partials.  No runtime fill / copy nodes: launch_zero_bytes / launch_copy_bytes.  No host synchronisation.
#include "rdesign_internal.h"
#include "train_dev.h"

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
        reinterpret_cast<u32x4*>(F)[id] = pack8(v);
    }
}

// ------------------------------------------------------------------------------------------ functional.Normalize on bf16 rows
// y = gain (x - mean) / (sqrt(var_unbiased + 1e-6) + 1e-6) + bias (k_rd_rownorm mode 0) with x and y bf16: one wave per row, lane = two adjacent channels
__global__ void __launch_bounds__(256) k_rdb_normalize16(const int* __restrict__ ntot_p, int mul, const tb16* __restrict__ x, const float* __restrict__ gain,
                                                         const float* __restrict__ bias, tb16* __restrict__ y) {
    const size_t R = (size_t)*ntot_p * mul;
    const int lane = threadIdx.x & 63, c = 2 * lane;
    const f32x2 gw = *reinterpret_cast<const f32x2*>(gain + c), bw = *reinterpret_cast<const f32x2*>(bias + c);
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (size_t)gridDim.x * 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(x + row * RD_H + c);
        const float v0 = lo_bf(w), v1 = hi_bf(w);
        float s = v0 + v1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mu = s / 128.f;
        const float d0 = v0 - mu, d1 = v1 - mu;
        float q = d0 * d0 + d1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float inv = 1.0f / (sqrtf(q / 127.f + 1e-6f) + 1e-6f);
        *reinterpret_cast<unsigned*>(y + row * RD_H + c) = pack2(gw[0] * d0 * inv + bw[0], gw[1] * d1 * inv + bw[1]);
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
    const f32x2 gw = *reinterpret_cast<const f32x2*>(gain + c);
    float sg0 = 0.f, sg1 = 0.f, sb0 = 0.f, sb1 = 0.f;
    for (size_t row = (size_t)blockIdx.x * 4 + wave; row < R; row += (size_t)gridDim.x * 4) {
        float v0, v1;
        if constexpr (XB) {
            const unsigned w = *reinterpret_cast<const unsigned*>(reinterpret_cast<const tb16*>(xv) + row * RD_H + c);
            v0 = lo_bf(w); v1 = hi_bf(w);
        } else {
            const f32x2 w = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(xv) + row * RD_H + c);
            v0 = w[0]; v1 = w[1];
            if (res) { const f32x2 r2 = *reinterpret_cast<const f32x2*>(res + row * RD_H + c); v0 += r2[0]; v1 += r2[1]; }
        }
        const f32x2 yv = *reinterpret_cast<const f32x2*>(dy + row * RD_H + c);
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
        if constexpr (OB) *reinterpret_cast<unsigned*>(reinterpret_cast<tb16*>(dxv) + row * RD_H + c) = pack2(o0, o1);
        else *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(dxv) + row * RD_H + c) = f32x2{o0, o1};
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
        const float x0 = lo_bf(w), x1 = hi_bf(w);
        s0 += valid ? gelu_fast(x0) * m0 : 0.f;
        s1 += valid ? gelu_fast(x1) * m1 : 0.f;
        *reinterpret_cast<unsigned*>(base + (size_t)sl * RD_H) = valid ? pack2(gelu_d_fast(x0) * m0, gelu_d_fast(x1) * m1) : 0u;
    }
    *reinterpret_cast<f32x2*>(out + (size_t)p * RD_H + c) = f32x2{s0 * inv_scale, s1 * inv_scale};
}

// ------------------------------------------------------------------------------------------ element-wise helpers of the edge chain
// pre[e][c] = TE_DROPPED where dropout site `site` drops element (e, c): the tape form te_gemm_bwd2 reads without a hash.  16-byte units.
__global__ void __launch_bounds__(256) k_rdb_mark_dropped(const int* __restrict__ ntot_p, int K, tb16* __restrict__ pre, TDrop dr, unsigned site) {
    const size_t n = (size_t)*ntot_p * K * 16;
    const unsigned key = drop_key(dr, site);
    const unsigned dropped = pack2(TE_DROPPED, TE_DROPPED);
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
        u32x4 v = reinterpret_cast<const u32x4*>(pre)[id];
        float dm[8];
        drop8(dr, key, (unsigned)id, dm);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned lo = dm[2 * q] == 0.f ? (dropped & 0xffffu) : (v[q] & 0xffffu);
            const unsigned hi = dm[2 * q + 1] == 0.f ? (dropped & 0xffff0000u) : (v[q] & 0xffff0000u);
            v[q] = lo | hi;
        }
        reinterpret_cast<u32x4*>(pre)[id] = v;
    }
}
// acc[e][c] = (first ? 0 : acc[e][c]) + de[e][c];  de = 0: the f32 accumulator of d h_E over the L layers; te_gemm_bwd1 ADDS into its bf16 DE
// output, which therefore holds one layer's share only and is handed back zeroed.  One thread = 8 channels.
__global__ void __launch_bounds__(256) k_rdb_acc(const int* __restrict__ ntot_p, int K, tb16* __restrict__ de, float* __restrict__ acc, int first) {
    const size_t n = (size_t)*ntot_p * K * 16;
    for (size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (size_t)gridDim.x * blockDim.x) {
        const u32x4 v = reinterpret_cast<const u32x4*>(de)[id];
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (!first) { a = reinterpret_cast<const f32x4*>(acc)[2 * id]; b = reinterpret_cast<const f32x4*>(acc)[2 * id + 1]; }
        a[0] += lo_bf(v[0]); a[1] += hi_bf(v[0]); a[2] += lo_bf(v[1]); a[3] += hi_bf(v[1]);
        b[0] += lo_bf(v[2]); b[1] += hi_bf(v[2]); b[2] += lo_bf(v[3]); b[3] += hi_bf(v[3]);
        reinterpret_cast<f32x4*>(acc)[2 * id] = a; reinterpret_cast<f32x4*>(acc)[2 * id + 1] = b;
        reinterpret_cast<u32x4*>(de)[id] = u32x4{0u, 0u, 0u, 0u};
    }
}
// t[i] = v for i < n: the per-residue table of te_gemm_bwd2 mode 2 (1 / scale for every residue here, 1 / count in the main model)
__global__ void k_rdb_fill(float* __restrict__ t, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = v;
}

// ------------------------------------------------------------------------------------------ the step: edge sequence around the node side
namespace {
struct RdbEdges {
    tb16* embE; std::vector<std::vector<tb16*>> msg;      // tape: edge embedding output, message pre-activations
    float *dhE, *dpq, *inv_scale, *npart;    // f32 accumulator of d h_E; [N][256] d P | d Q; the 1 / 30 table; partials of the norm parameter gradients
    tb16 *hE, *de, *eraw, *dA, *dB;          // bf16 [E][128]: h_E, one layer's d h_E, raw edge features, two gradient buffers (views of f.hE / f.E1 / f.E2)
};
size_t rdb_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdtWs& w, RdbEdges& e) {
    rdt_carve(c, B, Nmax, base, w);
    const size_t EH = Nmax * c->cfg.k_neighbors * RD_H;
    auto tb = [&](size_t halves) { return (tb16*)w.take(halves * sizeof(tb16), true); };
    e.embE = tb(EH);
    e.msg.assign(c->cfg.num_mpnn_layers, {});
    for (auto& m : e.msg)
        for (int i = 0; i < c->cfg.num_message_layers; ++i) m.push_back(tb(EH));
    e.dhE = w.tf(EH); e.dpq = w.tf(Nmax * 256); e.inv_scale = w.tf(Nmax); e.npart = w.tf((size_t)RDB_NORM_BLOCKS * 256);
    // each f32 [E][128] region of the forward's workspace holds two bf16 ones
    e.hE = reinterpret_cast<tb16*>(w.f.hE); e.de = base ? e.hE + EH : nullptr;
    e.eraw = reinterpret_cast<tb16*>(w.f.E1); e.dA = base ? e.eraw + EH : nullptr;
    e.dB = reinterpret_cast<tb16*>(w.f.E2);                                        // (before the first layer: scratch of t_build_reverse)
    return w.off;
}
unsigned row_grid(size_t maxrows, size_t cap) { size_t g = (maxrows + 3) / 4; if (g > cap) g = cap; return (unsigned)(g ? g : 1); }
}  // namespace

int rdb_step(rdesign_handle h, const RdtArgs& a, size_t* sizes) {
    static const char* const who = "rdesign_loss_and_grad_ex";
    RdtStep t;
    RdbEdges e;
    const size_t Nmax = (size_t)a.B * a.T;
    const size_t need = rdb_carve(h, a.B, Nmax, (char*)a.ws, t.w, e);      // (addresses only: checked before anything is launched)
    if (sizes) { sizes[0] = need; sizes[1] = t.w.tape_bytes; return RDESIGN_OK; }
    if (const int rc = rdt_begin(t, h, a, true, need, who)) return rc;
    rdesign_ctx* c = h;
    RdRun& r = t.r;
    RdtWs& w = t.w;
    hipStream_t s = r.cx.s;
    const PackInfo& pk = r.pk;
    const int K = r.K, L = t.L, M = t.M;
    const int* ntot = pk.cu + pk.B;
    const TRows rn = r.rn(), re = r.re();
    const TDrop dr = t.dr;
    const TDrop nodrop = r.nodrop;
    const size_t Emax = Nmax * K;
    bool bad = false;                        // an edge kernel refused its configuration: reported after the launch sequence (nothing of it ran)
    // the weights change every step: every fragment image registered so far is rebuilt from the arena, blocks first seen in this call build their own
    if (!c->wimg) c->wimg = t_wimg_create(256);
    if (c->wimg) { t_wimg_refresh(c->wimg, s); c->wimg_fresh = true; }
    r.cx.wimg = c->wimg;
    const unsigned seg_grid = (unsigned)((Nmax + 3) / 4);
    // row-normalisation backward with the parameter gradients: fixed-order partials per block, then one block adds them in order
    auto norm_bwd = [&](bool edge, const void* x, const float* res, const float* dy, int gain_i, int bias_i, int mode, void* dx) {
        const unsigned grid = row_grid(edge ? Emax : Nmax, RDB_NORM_BLOCKS);
        if (edge) hipLaunchKernelGGL((k_rdb_rownorm_bwd<true, true>), dim3(grid), dim3(256), 0, s, ntot, K, x, res, dy, rdp(c, gain_i), mode, dx, e.npart);
        else hipLaunchKernelGGL((k_rdb_rownorm_bwd<false, false>), dim3(grid), dim3(256), 0, s, ntot, 1, x, res, dy, rdp(c, gain_i), mode, dx, e.npart);
        hipLaunchKernelGGL(k_rdb_norm_params, dim3(1), dim3(256), 0, s, e.npart, (int)grid, t.G(gain_i), t.G(bias_i));
    };

    // ================================================================ taped forward
    rd_front(r, a.X, a.mask, nullptr);
    t_build_reverse(pk, K, w.f.nbr, w.rdeg, w.rstart, w.rfill, w.rlist, reinterpret_cast<int*>(w.f.E2), s);
    hipLaunchKernelGGL(k_rdb_fill, dim3((unsigned)((Nmax + 255) / 256)), dim3(256), 0, s, e.inv_scale, (int)Nmax, 1.0f / 30.0f);
    launch_zero_bytes(e.de, Emax * RD_H * sizeof(tb16), s);
    // node embedding (101 inputs: f32 block) + Normalize
    t_gemm(rn, w.f.node_raw, RD_NODEP, RD_NODEP, c->der + c->node_emb.wt, RD_H, rdp(c, c->node_emb.b), RD_H, w.embN, RD_H, 0, s);
    rd_rownorm(ntot, 1, Nmax, w.embN, nullptr, rdp(c, c->nn_g), rdp(c, c->nn_b), 0, w.hv[0], s);
    // edge embedding (115 inputs) on the MFMA edge GEMM + Normalize, bf16 rows
    hipLaunchKernelGGL(k_rdb_eraw16, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, w.f.edge_raw, e.eraw);
    bad |= !te_gemm(re, e.eraw, true, RD_H, rdp(c, c->edge_emb.w), RD_EDGE, true, rdp(c, c->edge_emb.b), e.embE, false, nullptr, nullptr, nodrop, 0u, r.cx, RD_EDGE);
    hipLaunchKernelGGL(k_rdb_normalize16, dim3(row_grid(Emax, 8192)), dim3(256), 0, s, ntot, K, e.embE, rdp(c, c->ne_g), rdp(c, c->ne_b), e.hE);
    tb16* Pt = reinterpret_cast<tb16*>(w.f.pq);
    tb16* Qt = Pt + (Nmax + 1) * RD_H;                       // (row Nmax of Q: zeros, the gather target of absent slots - rd_front)
    for (int l = 0; l < L; ++l) {
        const RdLayer& Lw = c->layers[l];
        RdtLayer& tl = w.layers[l];
        const std::vector<tb16*>& msg = e.msg[l];
        const float* hv = w.hv[l];
        const float* w0 = rdp(c, Lw.msg[0].w);               // [128][384] = [W_e | W_centre | W_neighbour]
        te_gemm_pq(rn, hv, w0 + RD_H, rdp(c, Lw.msg[0].b), Pt, Qt, r.cx);
        const EFuse f{Pt, Qt, w.f.nbr, K, (int)Nmax, nullptr, nullptr, 0u};
        // Linears 0 and 1 in one kernel: msg[0] taped with TE_DROPPED marks, msg[1] plain
        te_mlp2_fwd(re, e.hE, w0, 3 * RD_H, rdp(c, Lw.msg[1].w), RD_H, rdp(c, Lw.msg[1].b), msg[0], msg[1], f, dr, t.site_msg(l, 0), r.cx);
        if (M == 3) {
            bad |= !te_gemm(re, msg[1], true, RD_H, rdp(c, Lw.msg[2].w), RD_H, true, rdp(c, Lw.msg[2].b), msg[2], true, nullptr, nullptr, dr, t.site_msg(l, 1), r.cx);
            if (dr.thresh) hipLaunchKernelGGL(k_rdb_mark_dropped, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, msg[1], dr, t.site_msg(l, 1));
        }
        hipLaunchKernelGGL(k_rdb_segsum, dim3(seg_grid), dim3(256), 0, s, pk, K, w.f.nbr, msg[M - 1], 1.0f / 30.0f, tl.dh, dr, t.site_msg(l, M - 1));
        rd_rownorm(ntot, 1, Nmax, hv, tl.dh, rdp(c, Lw.n1w), rdp(c, Lw.n1b), 1, tl.h1, s);                  // norm1(h_V + dh)
        rdt_ffn_fwd(t, Lw.dense, tl.h1, tl.dense, tl.y, t.site_dense(l, 0));
        rd_rownorm(ntot, 1, Nmax, tl.h1, tl.y, rdp(c, Lw.n2w), rdp(c, Lw.n2b), 1, w.hv[l + 1], s);          // norm2(h_V + dense(h_V))
    }
    rdt_ffn_fwd(t, c->readout, w.hv[L], w.rpre, w.logits, t.site_ro(0));

    // ================================================================ loss and backward
    rdt_loss(t, a);
    rdt_ffn_bwd(t, c->readout, w.hv[L], w.rpre, w.dlogits, w.gH, false, t.site_ro(0));
    // ---- L x MPNNLayer, last first; w.gH = d loss / d (h_V leaving the layer)
    for (int l = L - 1; l >= 0; --l) {
        const RdLayer& Lw = c->layers[l];
        RdtLayer& tl = w.layers[l];
        const std::vector<tb16*>& msg = e.msg[l];
        norm_bwd(false, tl.h1, tl.y, w.gH, Lw.n2w, Lw.n2b, 1, w.gX);                                         // norm2(h1 + y)
        rdt_ffn_bwd(t, Lw.dense, tl.h1, tl.dense, w.gX, w.gX, true, t.site_dense(l, 0));     // w.gX is both d y and the residual part of d h1
        norm_bwd(false, w.hv[l], tl.dh, w.gX, Lw.n1w, Lw.n1b, 1, w.gH);                                      // norm1(h_V + dh): w.gH <- d (h_V + dh)
        // last message Linear: d pre[M-1] = valid ? gH[row / K] / 30 * g : 0 formed while its tile is staged; dW, db, d pre[M-2] in one pass
        const RdLin& last = Lw.msg[M - 1];
        te_gemm_bwd2(re, nullptr, msg[M - 2], e.dA, rdp(c, last.w), RD_H, t.G(last.w), RD_H, dr, t.G(last.b), r.cx,
                     EBwd2Src{2, msg[M - 1], w.f.nbr, w.gH, e.inv_scale, K});
        tb16* dpre0 = e.dA;
        if (M == 3) {       // the middle Linear takes its dY as given: weight gradient and input gradient as two passes over it
            const RdLin& mid = Lw.msg[1];
            te_gemm_tn(re, e.dA, msg[0], t.G(mid.w), RD_H, true, dr, t.site_msg(l, 0), t.G(mid.b), r.cx);
            bad |= !te_gemm(re, e.dA, true, RD_H, rdp(c, mid.w), RD_H, false, nullptr, e.dB, false, msg[0], nullptr, dr, t.site_msg(l, 0), r.cx);
            dpre0 = e.dB;
        }
        // factored first Linear: pre0 = W_e h_E + (W_c h_V + b)[centre] + (W_n h_V)[neighbour]
        const RdLin& l0 = Lw.msg[0];
        const float* w0 = rdp(c, l0.w);
        te_gemm_bwd1(re, dpre0, e.hE, e.de, w0, 3 * RD_H, t.G(l0.w), 3 * RD_H, r.cx);                        // dW_e, this layer's d h_E
        hipLaunchKernelGGL(k_rdb_acc, dim3(ew_grid(Emax * 16)), dim3(256), 0, s, ntot, K, e.de, e.dhE, l == L - 1 ? 1 : 0);
        te_edge_pq_bwd(pk, K, dpre0, w.rstart, w.rlist, e.dpq, s);                                           // dP = own slots, dQ = gather over the reverse adjacency
        tm_gemm_tn_pq(rn, e.dpq, w.hv[l], t.G(l0.w) + RD_H, t.G(l0.b), r.cx);                                // [dW_c ; dW_n], db (the bias rides in P)
        if (!tm_gemm_nn_pq(rn, e.dpq, w0 + RD_H, w.gH, s)) {                                                 // d h_V += dP W_c + dQ W_n
            t_gemm(rn, e.dpq, 256, RD_H, w0 + RD_H, l0.in, nullptr, RD_H, w.gH, RD_H, 1, s);
            t_gemm(rn, e.dpq + RD_H, 256, RD_H, w0 + 2 * RD_H, l0.in, nullptr, RD_H, w.gH, RD_H, 1, s);
        }
    }
    // ---- embeddings: Normalize backward, then the 101- / 115-input Linears (nothing flows into the raw features)
    norm_bwd(false, w.embN, nullptr, w.gH, c->nn_g, c->nn_b, 0, w.gX);
    rdt_node_emb_bwd(t);
    norm_bwd(true, e.embE, nullptr, e.dhE, c->ne_g, c->ne_b, 0, e.dB);
    te_gemm_tn(re, e.dB, e.eraw, t.G(c->edge_emb.w), RD_EDGE, false, nodrop, 0u, t.G(c->edge_emb.b), r.cx, RD_EDGE);
    if (const int rc = rdt_end(t, who)) return rc;
    if (bad) return rd_fail(RDESIGN_ERR_UNSUPPORTED, "bf16-mixed training step: an MFMA edge GEMM variant this configuration needs is not built");
    RD_TRY(hipGetLastError());
    return RDESIGN_OK;
}
