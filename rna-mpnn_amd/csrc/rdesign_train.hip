// TRAINING STEP of the `rdesign` model (C ABI: include/rdesign_hip.h, rdesign_loss_and_grad[_ex]): `training_step` + `loss.backward()` of the
// reference (rdesign/model/rdesign.py:95-104) in one call.  The reference's rdesign trainer sets no `precision` (rdesign/utils/train.py:107-115), so
// f32 IS its arithmetic and RDESIGN_TRAIN_F32 the default; RDESIGN_TRAIN_BF16_MIXED is the opt-in step of rdesign_train_bf16.hip.  Forward = the
// forward of rdesign.hip with every pre-activation kept in the workspace (the tape) and dropout after every GELU the reference follows with
// nn.Dropout (mpnn.py:16-18,24-26, functional.py:113-121); loss = CrossEntropyLoss()(logits, S) over the valid residues (ONE softmax, mean over N);
// backward walks the tape.  The gradient lands in ONE flat buffer laid out like the weight arena.  No float atomics: every cross-workgroup sum is
// an ordered reduction (red_begin .. red_end) or a fixed-order per-block partial, so two calls give bit-identical results.  No runtime fill / copy
// nodes: launch_zero_bytes / launch_copy_bytes.
// Layout of this file: the kernels of the f32 step and the cross-entropy; what both steps share (rdesign_internal.h) - row limits, the workspace
// both carve alike, the argument checks and run set-up, the backward companions of the node-level Linear dispatch (rd_mm, rdesign.hip), the node
// side (dense FFN and read-out forward / backward, node embedding backward), loss and the reduction bracket; the f32 edge sequence, readable top to
// bottom without a precision flag (its bf16-mixed twin: rdesign_train_bf16.hip); the one dispatch on `flags` and the C entry points.
// PARITY: the p = 0 loss and gradients are pinned to the reference's own float64 autograd (tests/golden/rdesign_*.npz); the dropout masks are not
// (torch's RNG cannot be matched): with dropout the checker is the restatement tests/_rdesign_train_ref.py, itself pinned at p = 0.
#include "rdesign_internal.h"
#include "train_dev.h"      // gelu_erf, gelu_d, drop_mul: the dropout hash the element-wise kernels of kernels_train.hip use - one definition

// ------------------------------------------------------------------------------------------ row-normalisation backward
// One wave per 128-wide row, two channels per lane; the row statistics are recomputed from the taped input v = x (+ res).
//   y = gain d / sig + bias, d = v - mean(v);  mode 0 (functional.Normalize): sig = sqrt(q / 127 + 1e-6) + 1e-6;  mode 1 (LayerNorm): sig = sqrt(q / 128 + 1e-5)
//   with g = dy gain, r = the square root in sig, n = 127 | 128:   dv = (g - mean(g)) / sig - d sum(g d) / (n r sig^2)
// t = dy d / sig: its column sums are d gain (the column sums of dy are d bias); both go through the ordered reduction path (t_colsum).  (The
// bf16-mixed step folds per-block partials instead - k_rdb_rownorm_bwd; merging the two would change the f32 bits.)
__global__ void __launch_bounds__(256) k_rdt_rownorm_bwd(const int* __restrict__ ntot_p, int mul, const float* __restrict__ x, const float* __restrict__ res,
                                                         const float* __restrict__ dy, const float* __restrict__ gain, int mode,
                                                         float* __restrict__ dx, float* __restrict__ t) {
    const size_t R = (size_t)*ntot_p * mul;
    const int lane = threadIdx.x & 63;
    const float g0w = gain[lane], g1w = gain[64 + lane];
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += (size_t)gridDim.x * 4) {
        float v0 = x[row * RD_H + lane], v1 = x[row * RD_H + 64 + lane];
        if (res) { v0 += res[row * RD_H + lane]; v1 += res[row * RD_H + 64 + lane]; }
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
        const float y0 = dy[row * RD_H + lane], y1 = dy[row * RD_H + 64 + lane];
        const float g0 = y0 * g0w, g1 = y1 * g1w;
        float sg = g0 + g1, sgd = g0 * d0 + g1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o, 64); sgd += __shfl_xor(sgd, o, 64); }
        const float mg = sg / 128.f, k = sgd * inv * inv / (n * root);
        dx[row * RD_H + lane] = (g0 - mg) * inv - d0 * k;
        dx[row * RD_H + 64 + lane] = (g1 - mg) * inv - d1 * k;
        t[row * RD_H + lane] = y0 * d0 * inv;
        t[row * RD_H + 64 + lane] = y1 * d1 * inv;
    }
}
static void rdt_rownorm_bwd(const int* ntot, int mul, size_t maxrows, const float* x, const float* res, const float* dy, const float* gain, int mode,
                            float* dx, float* t, hipStream_t s) {
    size_t g = (maxrows + 3) / 4;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_rdt_rownorm_bwd, dim3((unsigned)g), dim3(256), 0, s, ntot, mul, x, res, dy, gain, mode, dx, t);
}

// ------------------------------------------------------------------------------------------ segment sum with dropout, and its backward
// dh[p][c] = sum over the valid slots of drop(GELU(pre[(p, s)][c])) / scale      (mpnn.py:18,32-33: the Dropout behind the last message Linear, scatter_sum / 30)
__global__ void __launch_bounds__(128) k_rdt_segsum(PackInfo pk, int K, const int* __restrict__ nbr, const float* __restrict__ pre, float inv_scale,
                                                    float* __restrict__ out, TDrop dr, unsigned site) {
    const int c = threadIdx.x;
    const int ntot = pk.cu[pk.B];
    for (int p = blockIdx.x; p < ntot; p += gridDim.x) {
        float s = 0.f;
        for (int sl = 0; sl < K; ++sl)
            if (nbr[(size_t)p * K + sl] >= 0) {
                const size_t o = ((size_t)p * K + sl) * RD_H + c;
                s += gelu_erf(pre[o]) * drop_mul(dr, site, o);
            }
        out[(size_t)p * RD_H + c] = s * inv_scale;
    }
}
// dpre[(p, s)][c] = valid ? ddh[p][c] / scale * mask * GELU'(pre) : 0      (absent slots get zeros: the P / Q gather sums whole rows)
__global__ void __launch_bounds__(128) k_rdt_segsum_bwd(PackInfo pk, int K, const int* __restrict__ nbr, const float* __restrict__ ddh,
                                                        const float* __restrict__ pre, float inv_scale, float* __restrict__ dpre, TDrop dr, unsigned site) {
    const int c = threadIdx.x;
    const int ntot = pk.cu[pk.B];
    for (int p = blockIdx.x; p < ntot; p += gridDim.x) {
        const float g = ddh[(size_t)p * RD_H + c] * inv_scale;
        for (int sl = 0; sl < K; ++sl) {
            const size_t o = ((size_t)p * K + sl) * RD_H + c;
            dpre[o] = nbr[(size_t)p * K + sl] >= 0 ? g * gelu_d(pre[o]) * drop_mul(dr, site, o) : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------ cross-entropy on packed rows
// loss = mean over the valid residues of -log softmax(logits[p])[S[b][t]] (nn.CrossEntropyLoss(), rdesign.py:73,101) and d loss / d logits.  The label of
// packed row p is read from the padded (B, T) tensor (packing on the fly); per-block partial losses, summed in block order by one thread.
__global__ void __launch_bounds__(256) k_rdt_ce(PackInfo pk, const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                float* __restrict__ dlogits, float* __restrict__ part) {
    __shared__ float red[4];
    const int ntot = pk.cu[pk.B];
    const float inv_n = 1.0f / (float)(ntot > 0 ? ntot : 1);
    float local = 0.f;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < ntot; p += gridDim.x * blockDim.x) {
        const int b = pk.node_b[p];
        const int y = labels[(size_t)b * pk.T + (p - pk.cu[b])] & 3;
        const float4 z = reinterpret_cast<const float4*>(logits)[p];
        const float zz[4] = {z.x, z.y, z.z, z.w};
        const float mx = fmaxf(fmaxf(zz[0], zz[1]), fmaxf(zz[2], zz[3]));
        float e[4], s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { e[c] = expf(zz[c] - mx); s += e[c]; }
        const float zy = y == 0 ? zz[0] : (y == 1 ? zz[1] : (y == 2 ? zz[2] : zz[3]));
        local += logf(s) - (zy - mx);
        const float r = inv_n / s;
        float4 o;
        o.x = e[0] * r - (y == 0 ? inv_n : 0.f); o.y = e[1] * r - (y == 1 ? inv_n : 0.f);
        o.z = e[2] * r - (y == 2 ? inv_n : 0.f); o.w = e[3] * r - (y == 3 ? inv_n : 0.f);
        reinterpret_cast<float4*>(dlogits)[p] = o;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}
__global__ void k_rdt_loss_sum(const float* __restrict__ part, int n, float* __restrict__ loss) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[i];
    *loss = s;
}
static void rdt_ce_loss(const PackInfo& pk, const float* logits, const int32_t* labels, float* dlogits, float* part, float* loss, hipStream_t s) {
    int grid = (pk.Nmax + 255) / 256;
    if (grid > RDT_CE_BLOCKS) grid = RDT_CE_BLOCKS;
    hipLaunchKernelGGL(k_rdt_ce, dim3(grid), dim3(256), 0, s, pk, logits, labels, dlogits, part);
    hipLaunchKernelGGL(k_rdt_loss_sum, dim3(1), dim3(1), 0, s, part, grid, loss);
}

// ------------------------------------------------------------------------------------------ shared by the two steps: workspace, checks, run
int rdt_dm(const rdesign_ctx* c) {
    int d = RD_H;
    if (c->cfg.dim_dense_layers > d) d = c->cfg.dim_dense_layers;
    if (c->cfg.num_readout_layers > 1 && c->cfg.readout_hidden_dim > d) d = c->cfg.readout_hidden_dim;
    return d;
}
void rdt_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdtWs& w) {
    w.base = base; w.tape_bytes = 0;
    w.off = rd_carve(c, B, Nmax, base, &w.f);
    const RDesignConfig& g = c->cfg;
    const size_t E = Nmax * g.k_neighbors, NH = Nmax * RD_H, Dm = (size_t)rdt_dm(c);
    w.embN = w.tf(NH, true);
    w.hv.clear(); w.layers.clear(); w.rpre.clear();
    for (int l = 0; l <= g.num_mpnn_layers; ++l) w.hv.push_back(w.tf(NH, true));
    for (int l = 0; l < g.num_mpnn_layers; ++l) {
        RdtLayer L;
        for (int i = 0; i < g.num_dense_layers; ++i) L.dense.push_back(w.tf(Nmax * g.dim_dense_layers, true));
        L.dh = w.tf(NH, true); L.h1 = w.tf(NH, true); L.y = w.tf(NH, true);
        w.layers.push_back(L);
    }
    for (int j = 0; j + 1 < g.num_readout_layers; ++j) w.rpre.push_back(w.tf(Nmax * g.readout_hidden_dim, true));
    w.logits = w.tf(Nmax * 4, true);
    w.dlogits = w.tf(Nmax * 4); w.part = w.tf(RDT_CE_BLOCKS);
    w.gH = w.tf(NH); w.gX = w.tf(NH); w.bA = w.tf(Nmax * Dm); w.bB = w.tf(Nmax * Dm); w.bC = w.tf(Nmax * Dm);
    w.rdeg = (int*)w.take((Nmax + 1) * sizeof(int)); w.rstart = (int*)w.take((Nmax + 1) * sizeof(int)); w.rfill = (int*)w.take((Nmax + 1) * sizeof(int));
    w.rlist = (int*)w.take((E + 1) * sizeof(int));
    w.sc.floats = RED_VIEW;                  // one producer budget: no single extent is larger (kernels_train.h)
    w.sc.p = w.tf(w.sc.floats);
}
int rdt_begin(RdtStep& t, rdesign_handle h, const RdtArgs& a, bool mixed, size_t need, const char* who) {
    if (!a.X || !a.mask || !a.labels || !a.loss || !a.grad || !a.ws) return rd_fail(RDESIGN_ERR_BAD_ARG, "%s: null pointer", who);
    if (!(a.dropout >= 0.f && a.dropout < 1.f)) return rd_fail(RDESIGN_ERR_BAD_ARG, "dropout must be in [0, 1)");
    if (!h->arena) return rd_fail(RDESIGN_ERR_WEIGHTS, "no weight arena set");
    if (!h->finalized) return rd_fail(RDESIGN_ERR_WEIGHTS, "weights not finalized (call rdesign_finalize_weights)");
    if (((uintptr_t)a.grad & 15) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "gradient buffer must be 16-byte aligned");
    if (a.ws_bytes < need) return rd_fail(RDESIGN_ERR_WORKSPACE, "training workspace %zu bytes < required %zu", a.ws_bytes, need);
    if (((uintptr_t)a.ws & 255) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    if (rd_knn_lds_bytes(a.T) > 160 * 1024 - 256) return rd_fail(RDESIGN_ERR_UNSUPPORTED, "max_len %d too long for the LDS-resident k-NN row", a.T);
    t.r = rd_run(h, a.stream, mixed, t.w.f, a.B, a.T);
    t.dr = t_drop(a.dropout, a.seed);
    t.grad = a.grad;
    t.L = h->cfg.num_mpnn_layers; t.M = h->cfg.num_message_layers; t.D = h->cfg.num_dense_layers;
    return RDESIGN_OK;
}

// ------------------------------------------------------------------------------------------ shared: node-level Linear backward, node side
void rd_mm_wb(RdRun& r, const TRows& rows, const float* dy, const RdLin& l, const float* x, bool act, float* scratch, const TDrop& dr, unsigned site,
              float* grad) {
    float *dW = grad + r.c->raw[l.w].off, *db = grad + r.c->raw[l.b].off;
    if (r.mixed && tm_gemm_tn(rows, dy, l.out, l.out, x, l.in, l.in, dW, l.in, act, dr, site, db, r.cx)) return;
    if (act) { t_gelu_fwd(rows, x, scratch, l.in, dr, site, r.cx.s); x = scratch; }
    t_gemm_tn(rows, dy, l.out, l.out, x, l.in, l.in, dW, l.in, r.cx);
    t_colsum(rows, dy, l.out, l.out, db, r.cx);
}
void rd_mm_dx(RdRun& r, const TRows& rows, const float* dy, const RdLin& l, float* dx, int beta, const float* pre, float* scratch, const TDrop& dr,
              unsigned site) {
    const float* W = rdp(r.c, l.w);          // as nn.Linear stores it, [out][in]: K-major for this product
    if (r.mixed && tm_gemm_nn(rows, dy, l.out, l.out, W, l.in, nullptr, l.in, dx, l.in, beta, pre, l.in, dr, site, r.cx)) return;
    t_gemm(rows, dy, l.out, l.out, W, l.in, nullptr, l.in, pre ? scratch : dx, l.in, pre ? 0 : beta, r.cx.s);
    if (pre) t_gelu_bwd(rows, scratch, pre, dx, l.in, dr, site, r.cx.s);
}
void rdt_ffn_fwd(RdtStep& t, const std::vector<RdLin>& lin, const float* x, const std::vector<float*>& pre, float* out, unsigned site0) {
    const int n = (int)lin.size();
    for (int i = 0; i < n; ++i) {            // (the GELU of a taped pre-activation goes to w.bC: the tape is never overwritten)
        float* y = i + 1 < n ? pre[i] : out;
        rd_mm(t.r, t.r.rn(), x, lin[i].in, lin[i], 0, lin[i].in, true, y, lin[i].out, 0, i > 0, t.w.bC, t.dr, i > 0 ? site0 + i - 1 : 0u);
        x = y;
    }
}
void rdt_ffn_bwd(RdtStep& t, const std::vector<RdLin>& lin, const float* x, const std::vector<float*>& pre, const float* dy, float* dx, bool acc,
                 unsigned site0) {
    const TRows rn = t.r.rn();
    float* bufs[2] = {t.w.bA, t.w.bB};       // d pre alternates between the two: a Linear reads its dy while it writes its dx
    for (int i = (int)lin.size() - 1; i >= 0; --i) {
        const unsigned site = i > 0 ? site0 + i - 1 : 0u;
        rd_mm_wb(t.r, rn, dy, lin[i], i > 0 ? pre[i - 1] : x, i > 0, t.w.bC, t.dr, site, t.grad);
        if (i > 0) { float* d = bufs[i & 1]; rd_mm_dx(t.r, rn, dy, lin[i], d, 0, pre[i - 1], t.w.bC, t.dr, site); dy = d; }
        else rd_mm_dx(t.r, rn, dy, lin[i], dx, acc && dy != dx ? 1 : 0, nullptr, nullptr, t.dr, 0u);
    }
}
void rdt_node_emb_bwd(RdtStep& t) {         // 101 inputs: the f32 blocks in both precisions (nothing flows into the raw features)
    const rdesign_ctx* c = t.r.c;
    t_gemm_tn(t.r.rn(), t.w.gX, RD_H, RD_H, t.w.f.node_raw, RD_NODEP, RD_NODE, t.G(c->node_emb.w), RD_NODE, t.r.cx);
    t_colsum(t.r.rn(), t.w.gX, RD_H, RD_H, t.G(c->node_emb.b), t.r.cx);
}
void rdt_loss(RdtStep& t, const RdtArgs& a) {
    const PackInfo& pk = t.r.pk;
    if (a.logits) rd_copy_rows(pk.cu + pk.B, 1, pk.Nmax, t.w.logits, 4, a.logits, 4, 4, t.r.cx.s);      // rows >= N of the caller's tensor stay untouched
    rdt_ce_loss(pk, t.w.logits, a.labels, t.w.dlogits, t.w.part, a.loss, t.r.cx.s);
    launch_zero_bytes(t.grad, t.r.c->raw_floats * sizeof(float), t.r.cx.s);
    red_begin(t.r.cx, t.w.sc);
}
int rdt_end(RdtStep& t, const char* who) {
    return red_end(t.r.cx) ? RDESIGN_OK : rd_fail(RDESIGN_ERR_HIP, "%s: an ordered reduction was refused (reduction arena)", who);
}

// ------------------------------------------------------------------------------------------ the exact-f32 step: edge sequence around the node side
namespace {
// f32 [E][128]; tape: edge embedding Linear output (input of Normalize), message pre-activations per layer; scratch: a third edge buffer next to
// f.E1 / f.E2, d h_E accumulated over the layers
struct RdtEdges { float* embE; std::vector<std::vector<float*>> msg; float *eS, *dhE; };
size_t rdt_f32_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdtWs& w, RdtEdges& e) {
    rdt_carve(c, B, Nmax, base, w);
    const size_t EH = Nmax * c->cfg.k_neighbors * RD_H;
    e.embE = w.tf(EH, true);
    e.msg.assign(c->cfg.num_mpnn_layers, {});
    for (auto& m : e.msg)
        for (int i = 0; i < c->cfg.num_message_layers; ++i) m.push_back(w.tf(EH, true));
    e.eS = w.tf(EH); e.dhE = w.tf(EH);
    return w.off;
}
int rdt_f32_step(rdesign_handle h, const RdtArgs& a, size_t* sizes) {
    static const char* const who = "rdesign_loss_and_grad";
    RdtStep t;
    RdtEdges e;
    const size_t Nmax = (size_t)a.B * a.T;
    const size_t need = rdt_f32_carve(h, a.B, Nmax, (char*)a.ws, t.w, e);      // (addresses only: checked before anything is launched)
    if (sizes) { sizes[0] = need; sizes[1] = t.w.tape_bytes; return RDESIGN_OK; }
    if (const int rc = rdt_begin(t, h, a, false, need, who)) return rc;
    rdesign_ctx* c = h;
    RdRun& r = t.r;
    RdtWs& w = t.w;
    hipStream_t s = r.cx.s;
    const PackInfo& pk = r.pk;
    const int K = r.K, L = t.L, M = t.M;
    const int* ntot = pk.cu + pk.B;
    const TRows rn = r.rn(), re = r.re();
    const TDrop dr = t.dr;
    const float inv_scale = 1.0f / 30.0f;
    // Y = X . W[:, k0:k0+Kc]^T (+ bias): the forward's GEMM on the K-major copy finalize built
    auto fwd = [&](const TRows& rows, const float* Xin, int ldx, const RdLin& l, int k0, int Kc, bool use_bias, float* Y, int ldy) {
        rd_mm(r, rows, Xin, ldx, l, k0, Kc, use_bias, Y, ldy, 0, false, nullptr, r.nodrop, 0u);
    };
    // dx = [beta dx] + dy . W[:, k0:k0+128] of the factored first message Linear
    auto dx0 = [&](const TRows& rows, const float* dy, int ldy, const RdLin& l, int k0, float* dx, int beta) {
        t_gemm(rows, dy, ldy, l.out, rdp(c, l.w) + k0, l.in, nullptr, RD_H, dx, RD_H, beta, s);
    };
    const unsigned seg_grid = (unsigned)(Nmax < 65536 ? Nmax : 65536);

    // ================================================================ taped forward
    rd_front(r, a.X, a.mask, nullptr);
    t_build_reverse(pk, K, w.f.nbr, w.rdeg, w.rstart, w.rfill, w.rlist, reinterpret_cast<int*>(w.f.E2), s);
    fwd(rn, w.f.node_raw, RD_NODEP, c->node_emb, 0, RD_NODE, true, w.embN, RD_H);
    rd_rownorm(ntot, 1, Nmax, w.embN, nullptr, rdp(c, c->nn_g), rdp(c, c->nn_b), 0, w.hv[0], s);
    fwd(re, w.f.edge_raw, RD_EDGEP, c->edge_emb, 0, RD_EDGE, true, e.embE, RD_H);
    rd_rownorm(ntot, K, Nmax * K, e.embE, nullptr, rdp(c, c->ne_g), rdp(c, c->ne_b), 0, w.f.hE, s);
    for (int l = 0; l < L; ++l) {
        const RdLayer& Lw = c->layers[l];
        RdtLayer& tl = w.layers[l];
        const std::vector<float*>& msg = e.msg[l];
        const float* hv = w.hv[l];
        // message Linear 0 on cat[h_E, h_V[centre], h_V[neighbour]] = W_e.h_E + P[centre] + Q[neighbour]
        fwd(rn, hv, RD_H, Lw.msg[0], RD_H, RD_H, true, w.f.pq, 256);
        fwd(rn, hv, RD_H, Lw.msg[0], 2 * RD_H, RD_H, false, w.f.pq + RD_H, 256);
        fwd(re, w.f.hE, RD_H, Lw.msg[0], 0, RD_H, false, msg[0], RD_H);
        t_edge_add_pq(pk, K, w.f.nbr, w.f.pq, msg[0], s);
        for (int i = 1; i < M; ++i)
            rd_mm(r, re, msg[i - 1], RD_H, Lw.msg[i], 0, RD_H, true, msg[i], RD_H, 0, true, w.f.E1, dr, t.site_msg(l, i - 1));
        hipLaunchKernelGGL(k_rdt_segsum, dim3(seg_grid), dim3(128), 0, s, pk, K, w.f.nbr, msg[M - 1], inv_scale, tl.dh, dr, t.site_msg(l, M - 1));
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
        const std::vector<float*>& msg = e.msg[l];
        // norm2(h1 + y)
        rdt_rownorm_bwd(ntot, 1, Nmax, tl.h1, tl.y, w.gH, rdp(c, Lw.n2w), 1, w.gX, w.bA, s);
        t_colsum(rn, w.bA, RD_H, RD_H, t.G(Lw.n2w), r.cx);
        t_colsum(rn, w.gH, RD_H, RD_H, t.G(Lw.n2b), r.cx);
        rdt_ffn_bwd(t, Lw.dense, tl.h1, tl.dense, w.gX, w.gX, true, t.site_dense(l, 0));     // w.gX is both d y and the residual part of d h1
        // norm1(h_V + dh): w.gH <- d (h_V + dh)
        rdt_rownorm_bwd(ntot, 1, Nmax, w.hv[l], tl.dh, w.gX, rdp(c, Lw.n1w), 1, w.gH, w.bA, s);
        t_colsum(rn, w.bA, RD_H, RD_H, t.G(Lw.n1w), r.cx);
        t_colsum(rn, w.gX, RD_H, RD_H, t.G(Lw.n1b), r.cx);
        // segment sum, then the message Linears M-1 .. 1: dW, db from GELU(pre[i-1]) in e.eS; d pre[i-1] through w.f.E2, in place of d pre[i]
        float* dpre = w.f.E1;
        hipLaunchKernelGGL(k_rdt_segsum_bwd, dim3(seg_grid), dim3(128), 0, s, pk, K, w.f.nbr, w.gH, msg[M - 1], inv_scale, dpre, dr, t.site_msg(l, M - 1));
        for (int i = M - 1; i >= 1; --i) {
            rd_mm_wb(r, re, dpre, Lw.msg[i], msg[i - 1], true, e.eS, dr, t.site_msg(l, i - 1), t.grad);
            rd_mm_dx(r, re, dpre, Lw.msg[i], dpre, 0, msg[i - 1], w.f.E2, dr, t.site_msg(l, i - 1));
        }
        // factored first Linear: pre0 = W_e h_E + (W_c h_V + b)[centre] + (W_n h_V)[neighbour]
        const RdLin& l0 = Lw.msg[0];
        t_gemm_tn(re, dpre, RD_H, RD_H, w.f.hE, RD_H, RD_H, t.G(l0.w), 3 * RD_H, r.cx);                       // dW_e
        dx0(re, dpre, RD_H, l0, 0, e.dhE, l == L - 1 ? 0 : 1);                                                // d h_E (shared by all layers)
        t_edge_pq_bwd(pk, K, dpre, w.rstart, w.rlist, w.f.pq, s);                                             // dP = own slots, dQ = gather over the reverse adjacency
        t_colsum(rn, w.f.pq, 256, RD_H, t.G(l0.b), r.cx);                                                     // db (the bias rides in P)
        t_gemm_tn(rn, w.f.pq, 256, RD_H, w.hv[l], RD_H, RD_H, t.G(l0.w) + RD_H, 3 * RD_H, r.cx);              // dW_c
        t_gemm_tn(rn, w.f.pq + RD_H, 256, RD_H, w.hv[l], RD_H, RD_H, t.G(l0.w) + 2 * RD_H, 3 * RD_H, r.cx);   // dW_n
        dx0(rn, w.f.pq, 256, l0, RD_H, w.gH, 1);                                                              // d h_V += dP W_c + dQ W_n
        dx0(rn, w.f.pq + RD_H, 256, l0, 2 * RD_H, w.gH, 1);
    }
    // ---- embeddings: Normalize backward, then the 101- / 115-input Linears (nothing flows into the raw features)
    rdt_rownorm_bwd(ntot, 1, Nmax, w.embN, nullptr, w.gH, rdp(c, c->nn_g), 0, w.gX, w.bA, s);
    t_colsum(rn, w.bA, RD_H, RD_H, t.G(c->nn_g), r.cx);
    t_colsum(rn, w.gH, RD_H, RD_H, t.G(c->nn_b), r.cx);
    rdt_node_emb_bwd(t);
    rdt_rownorm_bwd(ntot, K, Nmax * K, e.embE, nullptr, e.dhE, rdp(c, c->ne_g), 0, w.f.E1, e.eS, s);
    t_colsum(re, e.eS, RD_H, RD_H, t.G(c->ne_g), r.cx);
    t_colsum(re, e.dhE, RD_H, RD_H, t.G(c->ne_b), r.cx);
    t_gemm_tn(re, w.f.E1, RD_H, RD_H, w.f.edge_raw, RD_EDGEP, RD_EDGE, t.G(c->edge_emb.w), RD_EDGE, r.cx);
    t_colsum(re, w.f.E1, RD_H, RD_H, t.G(c->edge_emb.b), r.cx);
    if (const int rc = rdt_end(t, who)) return rc;
    RD_TRY(hipGetLastError());
    return RDESIGN_OK;
}

// ------------------------------------------------------------------------------------------ one dispatch on `flags`, C entry points
// sizes != null: the host-only size query (sizes[0] = workspace bytes, sizes[1] = bytes of the tape alone, a figure for tools/rdesign_probe.py)
int rdt_dispatch(rdesign_handle h, const RdtArgs& a, int32_t flags, size_t* sizes) {
    if (flags != RDESIGN_TRAIN_F32 && flags != RDESIGN_TRAIN_BF16_MIXED) return rd_fail(RDESIGN_ERR_BAD_ARG, "unknown training flags %d", flags);
    if (!h) return rd_fail(RDESIGN_ERR_BAD_ARG, "null handle");
    if (flags == RDESIGN_TRAIN_F32 && h->cfg.precision != RDESIGN_PREC_F32)
        return rd_fail(RDESIGN_ERR_UNSUPPORTED, "the rdesign training step is built for the exact-f32 path only (create the handle with RDESIGN_PREC_F32)");
    if (flags == RDESIGN_TRAIN_BF16_MIXED && h->cfg.num_message_layers != 2 && h->cfg.num_message_layers != 3)
        return rd_fail(RDESIGN_ERR_UNSUPPORTED, "the bf16-mixed rdesign training step is built for num_message_layers 2 and 3 (got %d): train with RDESIGN_TRAIN_F32",
                       h->cfg.num_message_layers);
    if (a.B <= 0 || a.T <= 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "training step: non-positive B/T");
    // 32-bit element-pair indices of the dropout hash (kernels_train.h) and 32-bit edge-row indexing: rows * width / 2 < 2^32
    if ((long long)a.B * a.T * h->cfg.k_neighbors >= (1LL << 26) || (long long)a.B * a.T * rdt_dm(h) >= (1LL << 32))
        return rd_fail(RDESIGN_ERR_BAD_ARG, "row count out of range for the training path (B*T*k < 2^26); split the batch");
    return flags == RDESIGN_TRAIN_F32 ? rdt_f32_step(h, a, sizes) : rdb_step(h, a, sizes);
}
size_t rdt_size(rdesign_handle h, int32_t B, int32_t T, int32_t flags, int which) {
    RdtArgs a{};
    a.B = B; a.T = T;
    size_t sizes[2];
    return rdt_dispatch(h, a, flags, sizes) == RDESIGN_OK ? sizes[which] : 0;
}
}  // namespace

extern "C" size_t rdesign_train_workspace_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags) { return rdt_size(h, B, T, flags, 0); }
extern "C" size_t rdesign_train_tape_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags) { return rdt_size(h, B, T, flags, 1); }
extern "C" int rdesign_loss_and_grad_ex(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T, float dropout,
                                        uint64_t seed, int32_t flags, float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    return rdt_dispatch(h, RdtArgs{X, mask, labels, B, T, dropout, seed, loss, logits, grad, ws, ws_bytes, stream}, flags, nullptr);
}
// the entry points older than `flags`: the exact-f32 step
extern "C" size_t rdesign_train_workspace_bytes(rdesign_handle h, int32_t B, int32_t T) { return rdesign_train_workspace_bytes_ex(h, B, T, RDESIGN_TRAIN_F32); }
extern "C" size_t rdesign_train_tape_bytes(rdesign_handle h, int32_t B, int32_t T) { return rdesign_train_tape_bytes_ex(h, B, T, RDESIGN_TRAIN_F32); }
extern "C" int rdesign_loss_and_grad(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T, float dropout,
                                     uint64_t seed, float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    return rdesign_loss_and_grad_ex(h, X, mask, labels, B, T, dropout, seed, RDESIGN_TRAIN_F32, loss, logits, grad, ws, ws_bytes, stream);
}
