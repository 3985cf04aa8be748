// Exact-f32 TRAINING STEP of the `rdesign` model (C ABI: include/rdesign_hip.h, rdesign_loss_and_grad): `training_step` + `loss.backward()` of the
// reference (rdesign/model/rdesign.py:95-104) in one call.  The reference's rdesign trainer sets no `precision` (rdesign/utils/train.py:107-115), so
// f32 IS its arithmetic.  Forward = the f32 branch of rdesign_forward (rdesign.hip) with every pre-activation kept in the workspace (the tape) and
// dropout after every GELU the reference follows with nn.Dropout (mpnn.py:16-18,24-26, functional.py:113-121); loss = CrossEntropyLoss()(logits, S)
// over the valid residues (ONE softmax, mean over N); backward walks the tape with the trainer's f32 blocks (kernels_train.h: t_gemm, t_gemm_tn,
// t_colsum, t_gelu_fwd / t_gelu_bwd, t_build_reverse, t_edge_pq_bwd) and the kernels below.  The gradient lands in ONE flat buffer laid out like
// the weight arena.  No float atomics: every cross-workgroup sum is an ordered reduction (red_begin .. red_end) or a fixed-order per-block partial, so
// two calls give bit-identical results.  No runtime fill / copy nodes: launch_zero_bytes / launch_copy_bytes.
// Dropout addressing (restated by tests/_rdesign_train_ref.py): the TDrop counter hash; site = index of the Dropout module in forward order from 1 -
// layer l, message Linear i: 1 + l (M + D) + i; layer l, hidden dense Linear i: 1 + l (M + D) + M + i; hidden read-out Linear j: 1 + L (M + D) + j;
// element = row * width + channel, row = packed node row p or packed edge row p K + slot.
// PARITY: the p = 0 loss and gradients are pinned to the reference's own float64 autograd (tests/golden/rdesign_*.npz); the dropout masks are not
// (torch's RNG cannot be matched): with dropout the checker is the restatement tests/_rdesign_train_ref.py, itself pinned at p = 0.
#include "rdesign_internal.h"
#include "train_dev.h"      // gelu_f, gelu_d, drop_mul: the dropout hash the element-wise kernels of kernels_train.hip use - one definition

// ------------------------------------------------------------------------------------------ row-normalisation backward
// One wave per 128-wide row, two channels per lane; the row statistics are recomputed from the taped input v = x (+ res).
//   y = gain d / sig + bias, d = v - mean(v);  mode 0 (functional.Normalize): sig = sqrt(q / 127 + 1e-6) + 1e-6;  mode 1 (LayerNorm): sig = sqrt(q / 128 + 1e-5)
//   with g = dy gain, r = the square root in sig, n = 127 | 128:   dv = (g - mean(g)) / sig - d sum(g d) / (n r sig^2)
// t = dy d / sig: its column sums are d gain (the column sums of dy are d bias); both go through the ordered reduction path (t_colsum).
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
                s += gelu_f(pre[o]) * drop_mul(dr, site, o);
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
void rdt_ce_loss(const PackInfo& pk, const float* logits, const int32_t* labels, float* dlogits, float* part, float* loss, hipStream_t s) {
    int grid = (pk.Nmax + 255) / 256;
    if (grid > RDT_CE_BLOCKS) grid = RDT_CE_BLOCKS;
    hipLaunchKernelGGL(k_rdt_ce, dim3(grid), dim3(256), 0, s, pk, logits, labels, dlogits, part);
    hipLaunchKernelGGL(k_rdt_loss_sum, dim3(1), dim3(1), 0, s, part, grid, loss);
}

// ------------------------------------------------------------------------------------------ workspace
int rdt_dm(const rdesign_ctx* c) {
    int d = RD_H;
    if (c->cfg.dim_dense_layers > d) d = c->cfg.dim_dense_layers;
    if (c->cfg.num_readout_layers > 1 && c->cfg.readout_hidden_dim > d) d = c->cfg.readout_hidden_dim;
    return d;
}
int rdt_check_rows(rdesign_handle h, int32_t B, int32_t T) {
    if (B <= 0 || T <= 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "training step: non-positive B/T");
    // 32-bit element-pair indices of the dropout hash (kernels_train.h) and 32-bit edge-row indexing: rows * width / 2 < 2^32
    if ((long long)B * T * h->cfg.k_neighbors >= (1LL << 26) || (long long)B * T * rdt_dm(h) >= (1LL << 32))
        return rd_fail(RDESIGN_ERR_BAD_ARG, "row count out of range for the training path (B*T*k < 2^26); split the batch");
    return RDESIGN_OK;
}
namespace {
struct RdtLayer { std::vector<float*> msg, dense; float *dh, *h1, *y; };      // pre-activations of the message / hidden dense Linears, dh, norm1 output, dense output
struct RdtWs {
    RdWs f;                                  // the forward's buffers: features, k-NN table, h_E, P/Q table; E1 / E2 are edge scratch of the backward
    float *embN, *embE;                      // tape: embedding Linear outputs (inputs of the two Normalize)
    std::vector<float*> hv;                  // tape: h_V entering layer l (hv[L] = the stack's output)
    std::vector<RdtLayer> layers;
    std::vector<float*> rpre;                // tape: hidden read-out pre-activations
    float *logits, *dlogits, *part;
    float *gH, *gX, *bA, *bB, *bC;           // node-sized gradient / scratch buffers ([N][128] and [N][Dm])
    float *eS, *dhE;                         // edge-sized: third scratch buffer, d h_E accumulated over the layers
    int *rdeg, *rstart, *rfill, *rlist;      // reverse adjacency (t_build_reverse)
    TScratch sc;                             // arena of the ordered reductions
    size_t tape_bytes;
};
size_t rdt_carve(const rdesign_ctx* c, int B, size_t Nmax, char* base, RdtWs* out) {
    RdtWs tmp;
    RdtWs& w = out ? *out : tmp;
    size_t off = rd_carve(c, B, Nmax, base, &w.f);
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return base ? base + o : (char*)nullptr; };
    auto tf = [&](size_t floats) { return (float*)take(floats * sizeof(float)); };
    const RDesignConfig& g = c->cfg;
    const size_t E = Nmax * g.k_neighbors, NH = Nmax * RD_H, EH = E * RD_H, Dm = (size_t)rdt_dm(c);
    const size_t tape0 = off;
    w.embN = tf(NH); w.embE = tf(EH);
    w.hv.clear(); w.layers.clear(); w.rpre.clear();
    for (int l = 0; l <= g.num_mpnn_layers; ++l) w.hv.push_back(tf(NH));
    for (int l = 0; l < g.num_mpnn_layers; ++l) {
        RdtLayer L;
        for (int i = 0; i < g.num_message_layers; ++i) L.msg.push_back(tf(EH));
        for (int i = 0; i < g.num_dense_layers; ++i) L.dense.push_back(tf(Nmax * g.dim_dense_layers));
        L.dh = tf(NH); L.h1 = tf(NH); L.y = tf(NH);
        w.layers.push_back(L);
    }
    for (int j = 0; j + 1 < g.num_readout_layers; ++j) w.rpre.push_back(tf(Nmax * g.readout_hidden_dim));
    w.logits = tf(Nmax * 4);
    w.tape_bytes = off - tape0;
    w.dlogits = tf(Nmax * 4); w.part = tf(RDT_CE_BLOCKS);
    w.gH = tf(NH); w.gX = tf(NH); w.bA = tf(Nmax * Dm); w.bB = tf(Nmax * Dm); w.bC = tf(Nmax * Dm);
    w.eS = tf(EH); w.dhE = tf(EH);
    w.rdeg = (int*)take((Nmax + 1) * sizeof(int)); w.rstart = (int*)take((Nmax + 1) * sizeof(int)); w.rfill = (int*)take((Nmax + 1) * sizeof(int));
    w.rlist = (int*)take((E + 1) * sizeof(int));
    w.sc.floats = RED_VIEW;                  // one producer budget: no single extent is larger (kernels_train.h)
    w.sc.p = tf(w.sc.floats);
    return off;
}
int rdt_check(rdesign_handle h, int32_t B, int32_t T) {
    if (!h) return rd_fail(RDESIGN_ERR_BAD_ARG, "null handle");
    if (h->cfg.precision != RDESIGN_PREC_F32)
        return rd_fail(RDESIGN_ERR_UNSUPPORTED, "the rdesign training step is built for the exact-f32 path only (create the handle with RDESIGN_PREC_F32)");
    return rdt_check_rows(h, B, T);
}
}  // namespace

extern "C" size_t rdesign_train_workspace_bytes(rdesign_handle h, int32_t B, int32_t T) {
    if (rdt_check(h, B, T) != RDESIGN_OK) return 0;
    return rdt_carve(h, B, (size_t)B * T, nullptr, nullptr);
}

extern "C" int rdesign_loss_and_grad(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T, float dropout,
                                     uint64_t seed, float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream) {
    if (const int rc = rdt_check(h, B, T)) return rc;
    if (!X || !mask || !labels || !loss || !grad || !ws) return rd_fail(RDESIGN_ERR_BAD_ARG, "rdesign_loss_and_grad: null pointer");
    if (!(dropout >= 0.f && dropout < 1.f)) return rd_fail(RDESIGN_ERR_BAD_ARG, "dropout must be in [0, 1)");
    if (!h->arena) return rd_fail(RDESIGN_ERR_WEIGHTS, "no weight arena set");
    if (!h->finalized) return rd_fail(RDESIGN_ERR_WEIGHTS, "weights not finalized (call rdesign_finalize_weights)");
    if (((uintptr_t)grad & 15) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "gradient buffer must be 16-byte aligned");
    rdesign_ctx* c = h;
    const RDesignConfig& g = c->cfg;
    const size_t Nmax = (size_t)B * T;
    const int K = g.k_neighbors, L = g.num_mpnn_layers, M = g.num_message_layers, D = g.num_dense_layers, DD = g.dim_dense_layers;
    const size_t need = rdt_carve(c, B, Nmax, nullptr, nullptr);
    if (ws_bytes < need) return rd_fail(RDESIGN_ERR_WORKSPACE, "training workspace %zu bytes < required %zu", ws_bytes, need);
    if (((uintptr_t)ws & 255) != 0) return rd_fail(RDESIGN_ERR_BAD_ARG, "workspace must be 256-byte aligned");
    if (rd_knn_lds_bytes(T) > 160 * 1024 - 256) return rd_fail(RDESIGN_ERR_UNSUPPORTED, "max_len %d too long for the LDS-resident k-NN row", T);
    RdtWs w;
    rdt_carve(c, B, Nmax, (char*)ws, &w);
    RdRun r;
    r.c = c; r.s = (hipStream_t)stream; r.mixed = false; r.nodrop = TDrop{0ull, 0u, 1.f, nullptr}; r.K = K; r.w = w.f;
    r.pk.len = w.f.len; r.pk.cu = w.f.cu; r.pk.node_b = w.f.node_b; r.pk.B = B; r.pk.T = T; r.pk.Nmax = (int)Nmax; r.pk.packed_in = 0;
    hipStream_t s = r.s;
    const PackInfo& pk = r.pk;
    const int* ntot = pk.cu + B;
    const TRows rn = r.rn(), re = r.re();
    const TDrop dr = t_drop(dropout, seed);
    const float inv_scale = 1.0f / 30.0f;
    auto site_msg = [&](int l, int i) { return (unsigned)(1 + l * (M + D) + i); };
    auto site_dense = [&](int l, int i) { return (unsigned)(1 + l * (M + D) + M + i); };
    auto site_ro = [&](int j) { return (unsigned)(1 + L * (M + D) + j); };
    // Y = X . W[:, k0:k0+Kc]^T (+ bias) on the K-major copy finalize built: the forward's GEMM (rdesign.hip: rd_mm, f32 branch)
    auto fwd = [&](const TRows& rows, const float* Xin, int ldx, const RdLin& l, int k0, int Kc, bool use_bias, float* Y, int ldy) {
        t_gemm(rows, Xin, ldx, (Kc + 3) / 4 * 4, c->der + l.wt + (size_t)k0 * l.out, l.out, use_bias ? rdp(c, l.b) : nullptr, l.out, Y, ldy, 0, s);
    };
    const unsigned seg_grid = (unsigned)(Nmax < 65536 ? Nmax : 65536);

    // ================================================================ taped forward
    rd_front(r, X, mask, nullptr);
    t_build_reverse(pk, K, w.f.nbr, w.rdeg, w.rstart, w.rfill, w.rlist, reinterpret_cast<int*>(w.f.E2), s);
    fwd(rn, w.f.node_raw, RD_NODEP, c->node_emb, 0, RD_NODE, true, w.embN, RD_H);
    rd_rownorm(ntot, 1, Nmax, w.embN, nullptr, rdp(c, c->nn_g), rdp(c, c->nn_b), 0, w.hv[0], s);
    fwd(re, w.f.edge_raw, RD_EDGEP, c->edge_emb, 0, RD_EDGE, true, w.embE, RD_H);
    rd_rownorm(ntot, K, Nmax * K, w.embE, nullptr, rdp(c, c->ne_g), rdp(c, c->ne_b), 0, w.f.hE, s);
    for (int l = 0; l < L; ++l) {
        const RdLayer& Lw = c->layers[l];
        RdtLayer& t = w.layers[l];
        const float* hv = w.hv[l];
        // message Linear 0 on cat[h_E, h_V[centre], h_V[neighbour]] = W_e.h_E + P[centre] + Q[neighbour]
        fwd(rn, hv, RD_H, Lw.msg[0], RD_H, RD_H, true, w.f.pq, 256);
        fwd(rn, hv, RD_H, Lw.msg[0], 2 * RD_H, RD_H, false, w.f.pq + RD_H, 256);
        fwd(re, w.f.hE, RD_H, Lw.msg[0], 0, RD_H, false, t.msg[0], RD_H);
        t_edge_add_pq(pk, K, w.f.nbr, w.f.pq, t.msg[0], s);
        for (int i = 1; i < M; ++i) {
            t_gelu_fwd(re, t.msg[i - 1], w.f.E1, RD_H, dr, site_msg(l, i - 1), s);
            fwd(re, w.f.E1, RD_H, Lw.msg[i], 0, RD_H, true, t.msg[i], RD_H);
        }
        hipLaunchKernelGGL(k_rdt_segsum, dim3(seg_grid), dim3(128), 0, s, pk, K, w.f.nbr, t.msg[M - 1], inv_scale, t.dh, dr, site_msg(l, M - 1));
        rd_rownorm(ntot, 1, Nmax, hv, t.dh, rdp(c, Lw.n1w), rdp(c, Lw.n1b), 1, t.h1, s);                    // norm1(h_V + dh)
        const float* x = t.h1;
        int ld = RD_H;
        for (int i = 0; i <= D; ++i) {
            if (i > 0) { t_gelu_fwd(rn, t.dense[i - 1], w.bA, DD, dr, site_dense(l, i - 1), s); x = w.bA; ld = DD; }
            fwd(rn, x, ld, Lw.dense[i], 0, Lw.dense[i].in, true, i < D ? t.dense[i] : t.y, Lw.dense[i].out);
        }
        rd_rownorm(ntot, 1, Nmax, t.h1, t.y, rdp(c, Lw.n2w), rdp(c, Lw.n2b), 1, w.hv[l + 1], s);            // norm2(h_V + dense(h_V))
    }
    const int R = (int)c->readout.size();
    {
        const float* x = w.hv[L];
        int ld = RD_H;
        for (int j = 0; j < R; ++j) {
            if (j > 0) { t_gelu_fwd(rn, w.rpre[j - 1], w.bA, c->readout[j].in, dr, site_ro(j - 1), s); x = w.bA; ld = c->readout[j].in; }
            fwd(rn, x, ld, c->readout[j], 0, c->readout[j].in, true, j + 1 < R ? w.rpre[j] : w.logits, c->readout[j].out);
        }
    }
    if (logits) rd_copy_rows(pk.cu + B, 1, Nmax, w.logits, 4, logits, 4, 4, s);      // rows >= N of the caller's tensor stay untouched

    // ================================================================ loss and backward
    rdt_ce_loss(pk, w.logits, labels, w.dlogits, w.part, loss, s);
    launch_zero_bytes(grad, c->raw_floats * sizeof(float), s);
    auto G = [&](int i) { return grad + c->raw[i].off; };
    red_begin(w.sc, s);
    // gradients of one Linear y = x W^T + b from dy [rows][out] and its input x [rows][>= in]:  dW += dy^T x,  db += colsum(dy)
    auto lin_wb = [&](const TRows& rows, const float* dy, int ldy, const RdLin& l, const float* x, int ldx) {
        t_gemm_tn(rows, dy, ldy, l.out, x, ldx, l.in, G(l.w), l.in, s);
        t_colsum(rows, dy, ldy, l.out, G(l.b), s);
    };
    // dx = [beta dx] + dy . W[:, k0:k0+n]      (W as nn.Linear stores it, [out][in]: K-major for this product)
    auto lin_dx = [&](const TRows& rows, const float* dy, int ldy, const RdLin& l, int k0, int n, float* dx, int ldx, int beta) {
        t_gemm(rows, dy, ldy, l.out, rdp(c, l.w) + k0, l.in, nullptr, n, dx, ldx, beta, s);
    };
    // ---- read-out
    {
        const float* dy = w.dlogits;
        for (int j = R - 1; j >= 0; --j) {
            const RdLin& l = c->readout[j];
            const float* x = w.hv[L];
            if (j > 0) { t_gelu_fwd(rn, w.rpre[j - 1], w.bC, l.in, dr, site_ro(j - 1), s); x = w.bC; }
            lin_wb(rn, dy, l.out, l, x, l.in);
            if (j > 0) {
                lin_dx(rn, dy, l.out, l, 0, l.in, w.bA, l.in, 0);
                t_gelu_bwd(rn, w.bA, w.rpre[j - 1], w.bB, l.in, dr, site_ro(j - 1), s);
                dy = w.bB;
            } else {
                lin_dx(rn, dy, l.out, l, 0, RD_H, w.gH, RD_H, 0);
            }
        }
    }
    // ---- L x MPNNLayer, last first; w.gH = d loss / d (h_V leaving the layer)
    for (int l = L - 1; l >= 0; --l) {
        const RdLayer& Lw = c->layers[l];
        RdtLayer& t = w.layers[l];
        // norm2(h1 + y)
        rdt_rownorm_bwd(ntot, 1, Nmax, t.h1, t.y, w.gH, rdp(c, Lw.n2w), 1, w.gX, w.bA, s);
        t_colsum(rn, w.bA, RD_H, RD_H, G(Lw.n2w), s);
        t_colsum(rn, w.gH, RD_H, RD_H, G(Lw.n2b), s);
        // dense FFN: w.gX is both d y and the residual part of d h1
        {
            const float* dy = w.gX;
            for (int i = D; i >= 0; --i) {
                const RdLin& lin = Lw.dense[i];
                const float* x = t.h1;
                if (i > 0) { t_gelu_fwd(rn, t.dense[i - 1], w.bC, DD, dr, site_dense(l, i - 1), s); x = w.bC; }
                lin_wb(rn, dy, lin.out, lin, x, lin.in);
                if (i > 0) {
                    lin_dx(rn, dy, lin.out, lin, 0, lin.in, w.bA, lin.in, 0);
                    t_gelu_bwd(rn, w.bA, t.dense[i - 1], w.bB, DD, dr, site_dense(l, i - 1), s);
                    dy = w.bB;
                } else {
                    lin_dx(rn, dy, lin.out, lin, 0, RD_H, w.gX, RD_H, dy == w.gX ? 0 : 1);
                }
            }
        }
        // norm1(h_V + dh): w.gH <- d (h_V + dh)
        rdt_rownorm_bwd(ntot, 1, Nmax, w.hv[l], t.dh, w.gX, rdp(c, Lw.n1w), 1, w.gH, w.bA, s);
        t_colsum(rn, w.bA, RD_H, RD_H, G(Lw.n1w), s);
        t_colsum(rn, w.gX, RD_H, RD_H, G(Lw.n1b), s);
        // segment sum, then the message Linears M-1 .. 1
        float* dpre = w.f.E1;
        float* da = w.f.E2;
        hipLaunchKernelGGL(k_rdt_segsum_bwd, dim3(seg_grid), dim3(128), 0, s, pk, K, w.f.nbr, w.gH, t.msg[M - 1], inv_scale, dpre, dr, site_msg(l, M - 1));
        for (int i = M - 1; i >= 1; --i) {
            const RdLin& lin = Lw.msg[i];
            t_gelu_fwd(re, t.msg[i - 1], w.eS, RD_H, dr, site_msg(l, i - 1), s);
            lin_wb(re, dpre, RD_H, lin, w.eS, RD_H);
            lin_dx(re, dpre, RD_H, lin, 0, RD_H, da, RD_H, 0);
            t_gelu_bwd(re, da, t.msg[i - 1], dpre, RD_H, dr, site_msg(l, i - 1), s);
        }
        // factored first Linear: pre0 = W_e h_E + (W_c h_V + b)[centre] + (W_n h_V)[neighbour]
        const RdLin& l0 = Lw.msg[0];
        t_gemm_tn(re, dpre, RD_H, RD_H, w.f.hE, RD_H, RD_H, G(l0.w), 3 * RD_H, s);                            // dW_e
        lin_dx(re, dpre, RD_H, l0, 0, RD_H, w.dhE, RD_H, l == L - 1 ? 0 : 1);                                 // d h_E (shared by all layers)
        t_edge_pq_bwd(pk, K, dpre, w.rstart, w.rlist, w.f.pq, s);                                             // dP = own slots, dQ = gather over the reverse adjacency
        t_colsum(rn, w.f.pq, 256, RD_H, G(l0.b), s);                                                          // db (the bias rides in P)
        t_gemm_tn(rn, w.f.pq, 256, RD_H, w.hv[l], RD_H, RD_H, G(l0.w) + RD_H, 3 * RD_H, s);                   // dW_c
        t_gemm_tn(rn, w.f.pq + RD_H, 256, RD_H, w.hv[l], RD_H, RD_H, G(l0.w) + 2 * RD_H, 3 * RD_H, s);        // dW_n
        lin_dx(rn, w.f.pq, 256, l0, RD_H, RD_H, w.gH, RD_H, 1);                                               // d h_V += dP W_c + dQ W_n
        lin_dx(rn, w.f.pq + RD_H, 256, l0, 2 * RD_H, RD_H, w.gH, RD_H, 1);
    }
    // ---- embeddings: Normalize backward, then the 101- / 115-input Linears (nothing flows into the raw features)
    rdt_rownorm_bwd(ntot, 1, Nmax, w.embN, nullptr, w.gH, rdp(c, c->nn_g), 0, w.gX, w.bA, s);
    t_colsum(rn, w.bA, RD_H, RD_H, G(c->nn_g), s);
    t_colsum(rn, w.gH, RD_H, RD_H, G(c->nn_b), s);
    lin_wb(rn, w.gX, RD_H, c->node_emb, w.f.node_raw, RD_NODEP);
    rdt_rownorm_bwd(ntot, K, Nmax * K, w.embE, nullptr, w.dhE, rdp(c, c->ne_g), 0, w.f.E1, w.eS, s);
    t_colsum(re, w.eS, RD_H, RD_H, G(c->ne_g), s);
    t_colsum(re, w.dhE, RD_H, RD_H, G(c->ne_b), s);
    lin_wb(re, w.f.E1, RD_H, c->edge_emb, w.f.edge_raw, RD_EDGEP);
    if (!red_end()) return rd_fail(RDESIGN_ERR_HIP, "rdesign_loss_and_grad: an ordered reduction was refused (reduction arena)");
    RD_TRY(hipGetLastError());
    return RDESIGN_OK;
}

// bytes of the tape alone (the pre-activations and layer inputs kept between forward and backward): a figure for tools/rdesign_probe.py
extern "C" size_t rdesign_train_tape_bytes(rdesign_handle h, int32_t B, int32_t T) {
    if (rdt_check(h, B, T) != RDESIGN_OK) return 0;
    RdtWs w;
    rdt_carve(h, B, (size_t)B * T, nullptr, &w);
    return w.tape_bytes;
}
