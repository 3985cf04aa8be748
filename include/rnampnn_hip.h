/*
 * rnampnn_hip.h - C ABI of the MI355X-native RNA-MPNN forward path (librnampnn_hip.so).
 *
 * The reference (givemeone1astkiss/RNA-MPNN) has no FFI: its boundary for this path is the
 * Python module surface of `rnampnn.model`.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference root).  The host-side mirror in
 * `rna-mpnn_amd/rnampnn/model/` binds these symbols with ctypes and re-exposes the
 * reference's class/method names; INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; all tensor pointers are DEVICE pointers (HBM) unless
 *     a parameter says "host"; tensors are dense row-major in the reference's layouts:
 *       coords (B,T,7,3) f32, mask (B,T) f32 0/1 prefix masks as produced by the reference
 *       collate (rnampnn/utils/data.py:110-142), logits (B,T,4) f32, edge_index (B,T,k) i64.
 *   - inputs are const, outputs/workspace are caller-owned; the library keeps no reference
 *     to them after return.  Weights are copied into library-owned HBM at set time.
 *   - every launch goes to the caller's stream (`stream` = hipStream_t passed as void*), is
 *     asynchronous and never synchronises the device (hipGraph-capturable).
 *   - return value: 0 on success, an RNAMPNN_ERR_* code otherwise;
 *     rnampnn_last_error() gives the message of the calling thread's last failure.
 *   - one handle may be used by one host thread at a time (the reference: one Python
 *     thread per process, one process per GPU).
 */
#ifndef RNAMPNN_HIP_H
#define RNAMPNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNAMPNN_OK               0
#define RNAMPNN_ERR_BAD_ARG      1  /* null pointer, negative size ...            -> ValueError        */
#define RNAMPNN_ERR_UNSUPPORTED  2  /* hyper-parameter outside kernel support     -> NotImplementedError */
#define RNAMPNN_ERR_T_GT_P       3  /* max_len > padding_len (functional.py:155)  -> RuntimeError      */
#define RNAMPNN_ERR_K_TOO_LARGE  4  /* num_res_neighbours > RNAMPNN_KMAX          -> NotImplementedError */
#define RNAMPNN_ERR_WORKSPACE    5  /* workspace smaller than rnampnn_workspace_bytes -> RuntimeError  */
#define RNAMPNN_ERR_WEIGHTS      6  /* unknown key / wrong shape / weight not set -> KeyError          */
#define RNAMPNN_ERR_HIP          7  /* HIP runtime error (message carries hipGetErrorString)           */

#define RNAMPNN_KMAX 32             /* neighbours per residue supported by the edge kernels */

#define RNAMPNN_PREC_F32  0         /* exact-f32 kernels (parity grade: |dlogit| <= 1e-4)   */
#define RNAMPNN_PREC_BF16 1         /* bf16 MFMA operands, f32 accumulate, bf16 edge tensor */

typedef struct rnampnn_ctx* rnampnn_handle;

/* Hyper-parameters of RNAMPNN.__init__ that shape the network (rnampnn/model/rnampnn.py:19-47).
 * Atom counts are fixed at the reference defaults 7/6/6 (28 node and 90 edge raw features). */
typedef struct RnaMpnnConfig {
    int32_t num_res_neighbours;
    int32_t res_embedding_dim;            /* must be 128 */
    int32_t num_embedding_attn_layers;
    int32_t num_embedding_heads;
    int32_t embedding_ffn_dim;
    int32_t num_embedding_ffn_layers;
    int32_t res_edge_embedding_dim;       /* must be 128 */
    int32_t depth_res_edge_feature;       /* 1..2 */
    int32_t num_res_mpnn_layers;
    int32_t depth_res_mpnn;               /* 1..2 */
    int32_t num_mpnn_edge_layers;         /* 1..2 */
    int32_t padding_len;
    int32_t num_post_fusion_attn_layers;
    int32_t num_post_fusion_heads;
    int32_t post_fusion_ffn_dim;
    int32_t num_post_fusion_ffn_layers;
    int32_t num_raw_ffn_dim;
    int32_t num_raw_ffn_layers;
    int32_t raw_embedding_dim;            /* must be 128 */
    int32_t readout_hidden_dim;
    int32_t num_readout_layers;
    int32_t precision;                    /* RNAMPNN_PREC_* */
} RnaMpnnConfig;

/* Inputs, outputs and optional intermediate taps of one forward pass.  Null taps are skipped.
 * All taps are written in the reference's padded layouts with the reference's padding values: every requested tap is written
 * in full, all B*T rows (the caller need not clear it).  A padded row (t >= n) holds 0 in logits, embedding, h0, e0, h_layer,
 * e_layer, h_post and raw_emb, -1 in edge_index, and in raw the reference's 1e6 in the 21 distances and 0 in the 7 cosines.
 * The workspace may hold anything on entry; nothing outside [workspace, workspace + rnampnn_workspace_bytes()) is written. */
typedef struct RnaMpnnForwardIO {
    const float* coords;      /* (B,T,7,3).  Of the padded rows (t >= n) exactly one belongs to the result: row t == n of an RNA with
                                 n - 1 < k is the record of its phantom neighbour (the T_norm text below) and holds what the collate
                                 left there, zeros.  No other padded row reaches an output: it may hold anything, NaN included
                                 (row n is loaded but unused when n - 1 >= k; rows t > n are loaded and dropped). */
    const float* mask;        /* (B,T)     */
    int32_t B, T;
    int32_t T_norm;           /* the padded length this call stands for; 0 = T.  A data-parallel shard passes the
                                 GLOBAL batch max_len here.  It is the node-axis length GraphNormalization sees
                                 (functional.py:33-38) AND the padded length of the phantom-edge rule (an RNA with
                                 n - 1 < k keeps an edge to a padded residue iff n < max(T, T_norm)), so an
                                 edge_index tap may name index T: a padded residue that exists only in the global batch.
                                 The rule is unconditional: where max(T, T_norm) - n is 1 or 2 the reference's topk tie-break leaves -1
                                 in that slot in part of the rows ("The k-NN tie class"). */
    int32_t stop_after;       /* 0 = whole forward; 1 = stop after ResFeature.forward (feature.py:573-592) */
    float*   logits;          /* (B,T,4)    RNAMPNN.forward          rnampnn.py:161-185 (required if stop_after==0) */
    float*   embedding;       /* (B,T,256)  RNAMPNN.embedding        rnampnn.py:269-278 */
    int64_t* edge_index;      /* (B,T,k)    ResFeature._get_res_graph feature.py:205-256 */
    float*   raw;             /* (B,T,28)   ResFeature._res_embedding feature.py:531-535 */
    float*   h0;              /* (B,T,128)  node embedding after ResFeature.graph_norm feature.py:591 */
    float*   e0;              /* (B,T,k,128) ResFeature._res_edge_embedding feature.py:540-571 */
    int32_t  tap_layer;       /* 1-based ResMPNN layer whose outputs go to h_layer/e_layer; 0 = none */
    float*   h_layer;         /* (B,T,128)   ResMPNN.forward h  mpnn.py:283-294 */
    float*   e_layer;         /* (B,T,k,128) ResMPNN.forward e (valid edges; invalid slots are 0) */
    float*   h_post;          /* (B,T,128)  RNABert post_fusion      functional.py:161-172 */
    float*   raw_emb;         /* (B,T,128)  RawFFN                    functional.py:200-202 */
} RnaMpnnForwardIO;

/* -- lifetime / weights ------------------------------------------------------------------ */
/* RNAMPNN.__init__ (rnampnn.py:94-134): validates hyper-parameters, allocates weight storage. */
int rnampnn_create(const RnaMpnnConfig* cfg, rnampnn_handle* out);
int rnampnn_destroy(rnampnn_handle h);
/* nn.Module.load_state_dict for one entry: `key` is the reference state_dict key (SURVEY.md
 * row A1), `data` an f32 tensor with `numel` elements on the device (is_host=0) or host (1). */
int rnampnn_set_weight(rnampnn_handle h, const char* key, const float* data, int64_t numel,
                       int32_t is_host, void* stream);
/* Number of state-dict entries the configuration expects; key/numel of entry i (host strings). */
int rnampnn_num_weights(rnampnn_handle h);
int rnampnn_weight_info(rnampnn_handle h, int32_t i, const char** key, int64_t* numel);
/* Builds the kernel-side layouts (transposes, bf16 fragment images) from the weights set so far. */
int rnampnn_finalize_weights(rnampnn_handle h, void* stream);

/* -- forward ----------------------------------------------------------------------------- */
size_t rnampnn_workspace_bytes(rnampnn_handle h, int32_t B, int32_t T);
/* RNAMPNN.forward / RNAMPNN.embedding / ResFeature.forward, by `io->stop_after` and taps. */
int rnampnn_forward(rnampnn_handle h, const RnaMpnnForwardIO* io, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Packed (var-len) form of the same forward - SURVEY.md section 8 row F1: the reference's collate pads every
 * RNA to the batch max_len (rnampnn/utils/data.py:110-142); here the caller hands over the valid residues
 * only, back to back: coords_packed (N_total,7,3) f32, cu_seqlens (B+1) i32 on the device (exclusive prefix
 * sum of the lengths), T_max = longest RNA (host value; when T_norm is 0 it decides the phantom-edge rule exactly
 * as a batch padded to T_max would), T_norm as above (0 = T_max; otherwise it decides the phantom edge, like a batch
 * padded to T_norm).  Outputs are packed rows as well:
 * logits_packed (N_total,4), embedding_packed (N_total,256); either may be null. */
size_t rnampnn_workspace_bytes_packed(rnampnn_handle h, int32_t B, int32_t N_total);
int rnampnn_forward_packed(rnampnn_handle h, const float* coords_packed, const int32_t* cu_seqlens, int32_t B,
                           int32_t N_total, int32_t T_max, int32_t T_norm, float* logits_packed,
                           float* embedding_packed, void* workspace, size_t workspace_bytes, void* stream);

/* -- stage entry points (parity tests and the standalone reference classes) -------------- */
/* ResMPNN.forward / ResMPNN.message (mpnn.py:154-194, 267-294) for layer `layer` (0-based) on
 * caller-supplied h (B,T,128), e (B,T,k,128), edge_index (B,T,k) i64.  msg_out (B,T,k,128),
 * h_out, e_out are optional (null = skip). */
int rnampnn_mpnn_layer(rnampnn_handle h, int32_t layer, const float* h_in, const float* e_in,
                       const int64_t* edge_index, const float* mask, int32_t B, int32_t T, int32_t T_norm,
                       float* msg_out, float* h_out, float* e_out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* GraphNormalization.forward (functional.py:18-48); T_tot = node-axis length entering the variance. */
int rnampnn_graph_norm(const float* x, const float* mask, const float* scale, const float* shift,
                       int32_t B, int32_t T, int32_t T_tot, int32_t D, float* y, void* stream);
/* RNABert.forward (functional.py:161-172): which = 0 res_feature.res_embedding, 1 post_fusion. */
int rnampnn_rnabert(rnampnn_handle h, int32_t which, const float* x, const float* mask, int32_t B, int32_t T,
                    float* y, void* workspace, size_t workspace_bytes, void* stream);
/* RawFFN.forward (functional.py:200-202): raw (B,T,28) -> (B,T,128). */
int rnampnn_raw_ffn(rnampnn_handle h, const float* raw, const float* mask, int32_t B, int32_t T, int32_t T_norm,
                    float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Readout.forward (functional.py:86-90): emb (B,T,256) -> logits (B,T,4). */
int rnampnn_readout(rnampnn_handle h, const float* emb, const float* mask, int32_t B, int32_t T,
                    float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* -- decode ------------------------------------------------------------------------------ */
/* argmax decode + recovery (rnampnn.py:223-230, utils/train.py:18-21): per-RNA counts of correct
 * and valid positions, pred (B,T) int8 (-1 on padding).  labels (B,T) int32 class ids. */
int rnampnn_argmax_recovery(const float* logits, const float* mask, const int32_t* labels,
                            int32_t B, int32_t T, int8_t* pred, int32_t* correct, int32_t* valid, void* stream);
/* sample(): independent categorical draw per position from softmax(logits / temperature)
 * (no reference counterpart).  out (n_samples,B,T) int8, -1 on padding.
 * Counter-based RNG: draw = f(seed, sample, b, t) - reproducible and graph-replay safe. */
int rnampnn_sample(const float* logits, const float* mask, int32_t B, int32_t T, float temperature,
                   int32_t n_samples, uint64_t seed, int8_t* out, void* stream);
/* Same, with the seed read from DEVICE memory at kernel time: a hipGraph that captured this launch
 * draws fresh samples on every replay once the caller has updated *seed_device (BASELINE config 5:
 * "hipGraph-captured decode step"). */
int rnampnn_sample_dev_seed(const float* logits, const float* mask, int32_t B, int32_t T, float temperature,
                            int32_t n_samples, const uint64_t* seed_device, int8_t* out, void* stream);
/* Per-RNA scores of one batch of f32 logits in ONE launch (csrc/score.hip): what validation_step / test_step reduce (rnampnn.py:209-236)
 * and the likelihood of given sequences.  Two layouts of the logits, the same kernel and the same per-RNA reduction order (so the same
 * bytes for the same rows): padded - logits (B,T,4) + the prefix `mask` (B,T), cu_seqlens null; packed - logits (n_rows,4) + `cu_seqlens`
 * (B+1), mask null (what rnampnn_forward_packed writes; n_rows is ignored in the padded layout).  `labels` (B,T) int32 class ids and `seqs`
 * (S,B,T) int8 (the output of rnampnn_sample) are PADDED in both layouts; their entries at t >= n_b are never read.  Outputs, each nullable:
 *   valid (B) i32        n_b
 *   pred (B,T) i8        argmax, first maximum wins as rnampnn_argmax_recovery; -1 at t >= n_b
 *   correct (B) i32      #(argmax == label)
 *   label_nll (B) f32    sum_t logsumexp(x_t) - x_t[y_t]
 *   label_loss (B) f32   sum_t -log_softmax(softmax(x_t))[y_t]: the reference's mix_loss (cross-entropy of PROBABILITIES, rnampnn.py:151-154)
 *   seq_nll (S,B) f32    label_nll of candidate sequence s;   seq_match (S,B) i32   #(seq == label)
 * An RNA with n_b = 0 gives zeros.  Lengths and cu are clamped to the tensors' extents: a malformed mask gives meaningless numbers, never an
 * out-of-bounds access.  Fixed reduction order (per-thread ascending rows, wave butterfly, one LDS hop), no atomics, no workspace, no
 * runtime fill / copy node, no synchronisation: two calls give identical bytes and the call can sit inside a captured graph.
 * RNAMPNN_ERR_BAD_ARG: neither or both of mask and cu_seqlens, logits not 16-byte aligned, S < 0, S > 0 without seqs (or seqs with S = 0),
 * seq_nll / seq_match without seqs, correct / seq_match / label_nll / label_loss without labels, B or T <= 0. */
int rnampnn_score(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, const int32_t* labels,
                  const int8_t* seqs, int32_t S, int32_t B, int32_t T, int32_t* valid, int8_t* pred, int32_t* correct,
                  float* label_nll, float* label_loss, float* seq_nll, int32_t* seq_match, void* stream);
/* Constrained sequence design in ONE launch (csrc/design.hip): S sequences per RNA drawn from f32 logits under three kinds of constraint,
 * each draw scored.  The logits come in either layout of rnampnn_score (exactly one of `mask` and `cu_seqlens`; lengths and row offsets are
 * found and clamped as there).  `allowed`, `partner`, a per-position `bias` and `seqs` are PADDED (B,T) in both layouts.  Class ids: AUCG = 0..3.
 *   allowed (B,T) u8, nullable   bit c set = class c may be drawn (0xF free, one bit = a fixed nucleotide, IUPAC codes / omitted letters =
 *                                other masks); bits above 3 are ignored
 *   partner (B,T) i32, nullable  partner[b,t] = j pairs t with j; t counts as paired only if 0 <= j < n_b, j != t and partner[b,j] == t,
 *                                anything else (-1 by convention) is unpaired - a malformed table never causes an out-of-range access
 *   wobble                       != 0 admits GU and UG next to AU, UA, GC and CG
 *   bias, nullable               bias_per_position = 0: four device floats, one per class; 1: (B,T,4) padded, 16-byte aligned
 *   seed_dev, nullable           when present, *seed_dev (device memory, read at kernel time) replaces `seed`, as in rnampnn_sample_dev_seed
 * Outputs, each nullable:
 *   seqs (S,B,T) i8        the draws; -1 at t >= n_b; every valid position holds an id in 0..3 whatever the inputs hold (NaN included)
 *   seq_nll (S,B) f32      the model's own NLL of the draw (temperature 1, no bias, no constraints): byte for byte rnampnn_score's seq_nll
 *   infeasible (B) i32     valid positions whose constraint could not be honoured (below); the same for every sample
 * The draw.  z_t(c) = (logit_t(c) + bias_t(c)) / temperature for the classes `allowed` admits.  The uniform of (sample s, RNA b, position t),
 * with mix64 the splitmix64 finaliser and all arithmetic modulo 2^64:
 *   h = mix64(seed + 0x9E3779B97F4A7C15 * (s+1));  h = mix64(h ^ 0xD6E8FEB86659FD93 * (b+1));  h = mix64(h ^ 0xBF58476D1CE4E5B9 * (t+1));
 *   u24 = h >> 40
 * so a draw is a pure function of (seed, s, b, t) and the logits: it does not depend on B, T, S or the layout.
 *   Unpaired position: w(c) = exp(z(c) - max over the admitted classes) in class order 0..3; u = u24 * 2^-24 * (the running sum's final
 *     value); the first class whose running sum exceeds u is chosen; if none does (rounding, NaN) the last admitted class.
 *   Pair (i < j): cells (a,b) in a-major order, weight exp(z_i(a) + z_j(b) - m) over the compatible cells both masks admit, m the maximum
 *     over exactly those cells (the log domain: a feasible pair cannot underflow to a zero total at a low temperature); the uniform is
 *     that of (s, b, i); the same selection rule and fallback; i receives a, j receives b.
 *   Infeasible: a position whose mask admits no class is drawn as free and counts 1.  A pair without a compatible cell that both masks admit
 *     (two incompatible fixed nucleotides, say) makes both ends draw as unpaired positions, each with its own mask and its own (s,b,t)
 *     uniform, and counts 2.
 * No workspace, no runtime fill / copy node, no atomics, no host synchronisation: two calls give identical bytes and the call can sit inside
 * a captured graph.  RNAMPNN_ERR_BAD_ARG, before anything is launched: null logits; B, T or S <= 0; S + 1 > 65535; neither or both of mask
 * and cu_seqlens; a temperature that is not positive and finite; logits (or a per-position bias) not 16-byte aligned; n_rows < 0 with
 * cu_seqlens.  With every output null the call returns RNAMPNN_OK without a launch. */
int rnampnn_design(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                   float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                   const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position, int8_t* seqs,
                   float* seq_nll, int32_t* infeasible, void* stream);
/* Multi-state design in ONE launch (csrc/design_tied.hip): one sequence per sample for a GROUP of batch rows, its STATES (the conformers of
 * an ensemble, the two backbones of a switch), drawn exactly from the product of the states' distributions under the union of their
 * base-pair tables.  Layouts, the padded constraint tensors, seed_dev, the clamping of lengths and offsets and the alignment rules are
 * those of rnampnn_design; rnampnn_design itself is unchanged.
 *   group_cu (G+1) i32, device   group g = the consecutive rows [group_cu[g], group_cu[g+1]); values are clamped to [0, B], a decreasing
 *                                pair is an empty group.  An empty group writes nothing; rows no group covers are not written.
 *   weight (B) f32, nullable     per state row (null = 1 everywhere); may be negative (design AGAINST a state) or zero
 * Group quantities.  n_g = the minimum of the states' lengths (states of different lengths give the common prefix).
 *   z_t(c) = (sum_m weight_m * logit_{m,t}(c) + bias_t(c)) / temperature, summed in state order; a per-position bias is read from the group's
 *   first row.  (A product of experts: the states' log-partition terms are constant in c and cancel.)  The mask of t is the AND of the
 *   states' `allowed` sets; an empty AND is drawn as free and counts 1.
 * Dependency graph.  t is adjacent to j if in at least one state partner[m,t] = j is well formed (0 <= j < n_g, j != t, partner[m,j] == t).
 *   A position KEEPS its first two distinct neighbours in state order; one with more counts 1.  An edge is LIVE iff both ends keep it, so
 *   every component of the live graph is an isolated position, a path or a cycle.  Every walk is capped at n_g steps.
 * The draw, all of it in fp64 (z, the weights, the running sums).  The uniform of position t is u24(seed, s, b0, t) of rnampnn_design with b0
 * the group's first row.  SELECT(cells, w, u24) is the documented rule: the first cell whose running sum of w exceeds u24 * 2^-24 * total,
 * else the last cell.  omega_t(c) = exp(z_t(c) - max over the classes the mask admits), 0 for the others.  C(a,c) = 1 iff a pairs with c
 * (wobble as in rnampnn_design).  For the chain draws the cells are the classes the node's mask admits, in class order.
 *   Isolated position: SELECT over omega_t.
 *   2-node path: the pair rule of rnampnn_design (16 cells in a-major order, log-domain maximum, the uniform of the lower index).
 *   Path v_0 .. v_{L-1}, L >= 3, v_0 the end with the smaller index: alpha_0 = omega_0; alpha_k(c) = omega_k(c) * sum_a alpha_{k-1}(a) C(a,c),
 *     then divided by its largest component.  c_{L-1} = SELECT(alpha_{L-1}) with the uniform of v_{L-1}; then for k = L-2 .. 0
 *     c_k = SELECT(alpha_k(a) C(a, c_{k+1})) with the uniform of v_k.
 *   Cycle, v_0 its smallest index and v_1 the smaller of v_0's neighbours: for every head class h the mask of v_0 admits the forward pass from
 *     alpha_0 = omega_0(h) e_h, log Z_h = log sum_c alpha_{L-1}(c) C(c,h) + the sum of the logs of the normalisers; h = SELECT(exp(log Z_h -
 *     max)) with the uniform of v_0; the forward pass again with h fixed; c_{L-1} = SELECT(alpha_{L-1}(c) C(c,h)), then backwards down to
 *     k = 1 as for a path.
 *   The log domain, as for the pair: the recursion is carried as lambda_k = log alpha_k - lambda_k(c) = z_k(c) + log sum_{a: C(a,c)}
 *     exp(lambda_{k-1}(a)), -inf for a class the mask does not admit, minus its largest component - and the weights of a chain SELECT are
 *     exp(lambda_k(c) - max over the classes eligible in that draw), 0 for the others.  The distribution is the one above; what changes is
 *     that nothing underflows: at temperature 1e-3 omega is 0 for every class but one and the constrained optimum need not use that one.
 *   Infeasible component (no assignment that the masks admit is compatible along every edge: a largest component of some lambda_k that is
 *     not above -inf; no head with log Z_h above -inf; a 2-node path without a cell): every node draws as an isolated position with its own
 *     uniform and counts 1.
 * Outputs, each nullable:
 *   seqs (S,B,T) i8       every state row of a group receives the same sequence; -1 at t >= n_g
 *   seq_nll (S,B) f32     the NLL of the group's draw under THAT row's own logits (temperature 1, no bias): byte for byte rnampnn_score's
 *                         seq_nll of the written row (a row longer than n_g reads class 3 at its -1 entries, as rnampnn_score does)
 *   infeasible (B) i32    the group's count, written to each of its rows; the same for every sample
 * One workgroup per (group, sample); alpha lives in dynamic LDS indexed by position (32 bytes per position, requested only with a partner
 * table, + 1 byte per position always): RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB (T <= 4962 with a partner table).  No atomics, no
 * workspace, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured graph,
 * and a draw is a pure function of (seed, s, b0, t) and the rows of its group - independent of B, T, S, G, the layout and the other groups.
 * RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design; group_cu null; G <= 0.  With every output null the call
 * returns RNAMPNN_OK without a launch. */
int rnampnn_design_tied(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                        const int32_t* group_cu, int32_t G, const float* weight,
                        float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev,
                        const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                        int8_t* seqs, float* seq_nll, int32_t* infeasible, void* stream);
/* Design under a G+C content window in ONE launch (csrc/design_gc.hip): the draws of rnampnn_design, conditioned EXACTLY on the number of
 * C and G among the n_b nucleotides of RNA b lying in [gc_lo[b], gc_hi[b]].  The arguments are those of rnampnn_design plus
 *   gc_lo, gc_hi (B) i32, device   absolute counts per RNA, read at kernel time
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   gc_count (S,B) i32   the number of C or G ids actually written for that draw
 *   gc_miss (B) i32      0 when the window is reachable, else the distance from the window to the nearest reachable count; the same for
 *                        every sample
 * Extent, masks, bias, temperature, z_t(c), `allowed`, the validation of `partner`, wobble, "an empty mask is drawn free and counts 1" and "a
 * pair without an admitted compatible cell makes both ends single positions and counts 2" are rnampnn_design's.  All arithmetic is fp64, as
 * in rnampnn_design_tied: z_t(c) = ((double) logit_t(c) + (double) bias_t(c)) / (double) temperature.  G+C of a class: A, U = 0; C, G = 1.
 * LSE(x_1 .. x_k) = m + log(sum_i exp(x_i - m)) with m the maximum (NaN ignored), summed in the order given; -inf when m is not above -inf.
 *   Leaf polynomials, log domain, p_t(d), d = 0..2.  A single position: p_t(d) = LSE of z_t(c) over the admitted classes with G+C d in class
 *     order (d = 2: -inf).  A feasible pair i < j: p_i(d) = LSE of z_i(a) + z_j(b) over its admitted compatible cells with G+C(a) + G+C(b) = d
 *     in a-major order; p_j = "1" (0 at d = 0, -inf otherwise).
 *   Tree.  Node (l, i) covers the positions [i 2^l, min((i+1) 2^l, n_b)), has degree deg = min(2 * positions covered, n_b) and, for l >= 1,
 *     coefficients c(k) = LSE over a = max(0, k - deg_R) .. min(k, deg_L) of L(a) + R(k - a), L and R its halves (l-1, 2i) and (l-1, 2i+1); a node
 *     whose right half is empty equals its left half.  The root is node (ceil(log2 n_b), 0).  The shape depends on n_b only.
 *   Window.  lo and hi are clamped to [0, n_b], then hi = max(hi, lo).  If no count in the window has a finite root coefficient the target is
 *     the nearest count that has one, the lower count on a tie, and gc_miss is its distance (0 when no count at all has one: the target is lo).
 *   SELECT(candidates in order, log-weights x, u24): w = exp(x - max x) (NaN ignored in the maximum); the first candidate whose running sum of
 *     w exceeds u24 * 2^-24 * (the sum of w); else the last candidate with a finite x; else the first candidate.  The ORDER in which a
 *     node's weights are summed is not part of the contract (the total and the splits of the top levels are summed by a wave-wide scan), so
 *     a uniform within rounding (about 1e-15, relative) of a cumulative boundary may fall on either side of it.
 *   Draw, top down.  The total K = SELECT(lo .. hi, root coefficients).  A node holding k hands its left half a = SELECT(max(0, k - deg_R) ..
 *     min(k, deg_L), L(a) + R(k - a)) and its right half k - a (an empty right half: all of k, no uniform).  A leaf holding d draws its class -
 *     a pair its cell, in a-major order - among the admitted ones with G+C d by rnampnn_design's rule in fp64 (weights exp(z - max over those
 *     candidates), the first whose running sum exceeds u24 * 2^-24 * total, else the last of them); i receives a, j receives b.
 *   Uniforms, u24 of rnampnn_design: a leaf uses u24(seed, s, b, t), a pair that of its lower index; a split uses u24(seed ^ SALT, s, b, first
 *     position of the right half); the total uses u24(seed ^ SALT, s, b, 0) - position 0 never starts a right half.  With seed_dev the XOR is
 *     taken on the device.
 *   Robustness.  NaN or +-inf logits, a NaN bias or a malformed partner table still give ids in 0..3; every index and every count is clamped
 *     before use.  A leaf that cannot realise the count it was handed draws as rnampnn_design would (its whole admitted set).  Such a miss
 *     (non-finite inputs only) does not change gc_miss, which comes from the root alone; gc_count reports what was written.
 * seq_nll is byte for byte rnampnn_score's for the written draw and `infeasible` keeps its meaning, as in rnampnn_design.  One workgroup per
 * (RNA, sample); the levels 1 .. ceil(log2 T) live in dynamic LDS, node (l, i) at min(2 * (its extent within T), T) + 1 doubles (14,328 bytes at
 * T = 128, 73,720 at 512, 159,816 at 1000), + T rounded up to 16 bytes of class ids + 96 bytes: RNAMPNN_ERR_UNSUPPORTED when that exceeds
 * 160 KiB = 163,840 bytes (T <= 1017, which needs 163,800); the message names the byte count and that T.  Longer RNAs: rnampnn_design_count_long with counted = 12 everywhere and count_cap >= T, the tree in global memory.  No workspace, no
 * atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured graph,
 * and a draw is a pure function of (seed, s, b) and the rows of RNA b - independent of B, T, S and the layout.
 * RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design; null gc_lo or gc_hi.  With every output null the call
 * returns RNAMPNN_OK without a launch. */
#define RNAMPNN_DESIGN_GC_SALT 0xA0761D6478BD642Full
int rnampnn_design_gc(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                      float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                      const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                      const int32_t* gc_lo, const int32_t* gc_hi, int8_t* seqs, float* seq_nll, int32_t* infeasible,
                      int32_t* gc_count, int32_t* gc_miss, void* stream);
/* Design within a count window in ONE launch (csrc/design_count.hip): the draws of rnampnn_design, conditioned EXACTLY on the number of
 * positions of RNA b whose class falls in that position's COUNTED SET lying in [count_lo[b], count_hi[b]].  With the sets 15 ^ (1 << id of a
 * reference sequence) the count is the number of mutations against the reference and the window a mutation budget; with 12 (C|G) everywhere
 * and count_cap >= T the call returns the bytes of rnampnn_design_gc.  The arguments are those of rnampnn_design_gc with gc_lo / gc_hi
 * replaced by
 *   counted (B,T) u8, device, non-null   padded in both layouts; bits 0..3 mark the classes (AUCG) that count 1 at this position, the higher
 *                                        bits are ignored; 0: the position never counts.  bit(m, c) = (m >> c) & 1
 *   count_lo, count_hi (B) i32, device   absolute counts per RNA, read at kernel time
 *   count_cap i32, host                  no count above it is ever targeted or stored; it sizes the tree.  cap = min(count_cap, T) below
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   count (S,B) i32        the sum over the ids written for that draw of bit(counted[b,t], id_t)
 *   count_miss (B) i32     0 when the window is reachable, else the distance from the window to the target (below); the same for every sample
 * Extent, masks, bias, temperature, z_t(c), `allowed`, the validation of `partner`, wobble, "an empty mask is drawn free and counts 1" and "a
 * pair without an admitted compatible cell makes both ends single positions and counts 2" are rnampnn_design's.  All arithmetic is fp64, LSE,
 * SELECT, the uniforms and the salt (RNAMPNN_DESIGN_GC_SALT) are rnampnn_design_gc's.
 *   Leaf polynomials, log domain, p_t(d), d = 0..2.  A single position: p_t(d) = LSE of z_t(c) over the admitted classes with
 *     bit(counted_t, c) = d in class order (d = 2: -inf).  A feasible pair i < j: p_i(d) = LSE of z_i(a) + z_j(b) over its admitted compatible
 *     cells with bit(counted_i, a) + bit(counted_j, b) = d in a-major order; p_j = "1" (0 at d = 0, -inf otherwise).
 *   Tree.  Node (l, i) covers the positions [i 2^l, min((i+1) 2^l, n_b)), has degree deg = min(2 * positions covered, n_b, cap) and, for
 *     l >= 1, coefficients c(k), k = 0..deg, = LSE over a = max(0, k - deg_R) .. min(k, deg_L) of L(a) + R(k - a), L and R its halves; a node
 *     whose right half is empty equals its left half.  The root is node (ceil(log2 n_b), 0).  Truncation is exact: c(k) reads child
 *     coefficients of index <= k only, and for k <= cap the candidate range is the same with and without the cap, so the outputs of an RNA
 *     do not depend on count_cap, byte for byte, as long as its window and its target (below) lie within the cap.
 *   Window.  lo and hi are clamped to [0, min(n_b, cap)], then hi = max(hi, lo).  If no count in the window has a finite root coefficient
 *     the target is the nearest count within 0 .. min(n_b, cap) that has one, the lower count on a tie, and count_miss is its distance.  If no
 *     count at all is finite there, the target is k_min = the sum over the leaves of the smallest d with a finite p_t(d) (0 for a leaf with
 *     none) - the smallest reachable count - every leaf draws at its own smallest d (no total, no split, no salted uniform), which is the
 *     exact conditional on "count = k_min", and count_miss is the distance from the window to k_min (k_min - hi when k_min > hi, lo - k_min
 *     when k_min < lo, else 0).  When every input is finite this rule is used only when k_min > cap.
 *   Draw, top down, as in rnampnn_design_gc: the total K = SELECT(lo .. hi, root coefficients) or the target; a node holding k hands its
 *     left half a = SELECT(max(0, k - deg_R) .. min(k, deg_L), L(a) + R(k - a)) and its right half k - a; a leaf holding d draws its class - a
 *     pair its cell, in a-major order - among the admitted ones that count d by rnampnn_design's rule in fp64; i receives a, j receives b.
 *   Robustness.  NaN or +-inf logits, a NaN bias or a malformed partner table still give ids in 0..3; every index and every count is clamped
 *     before use.  A leaf that cannot realise the count it was handed draws as rnampnn_design would (its whole admitted set); `count` reports
 *     what was written.
 * seq_nll is byte for byte rnampnn_score's for the written draw and `infeasible` keeps its meaning, as in rnampnn_design.  One 256-thread
 * workgroup per (RNA, sample).  Dynamic LDS: 8 * doubles(T, cap) + T rounded up to 16 + 96 bytes (the k_min reduction borrows the 96),
 * doubles(T, cap) = the sum over the nodes of the levels 1 .. ceil(log2 T) of min(2 * (extent within T), T, cap) + 1: 7,320 bytes at
 * (T = 128, cap 8), 14,552 at (128, 128), 57,176 at (1000, 8).  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes; the message
 * names the bytes, the limit and the largest T at that cap: T <= 2867 at cap 8 (163,808 bytes), 2236 at cap 16, 1833 at cap 32, 1551 at cap 64,
 * 1017 for cap >= T.  Longer RNAs: rnampnn_design_count_long, the tree in global memory.  No workspace, no atomics, no runtime fill / copy node, no host
 * synchronisation: two calls give identical bytes, the call can sit inside a captured graph, and a draw is a pure function of (seed, s, b)
 * and the rows of RNA b - independent of B, T, S and the layout.
 * RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design; null counted, count_lo or count_hi; count_cap < 0.  With
 * every output null the call returns RNAMPNN_OK without a launch. */
int rnampnn_design_count(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                         float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                         const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                         const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap,
                         int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* count, int32_t* count_miss, void* stream);
/* rnampnn_design_count on a count tree in GLOBAL memory (csrc/design_long.hip), for RNAs whose tree does not fit the LDS of a workgroup.
 * The arguments are those of rnampnn_design_count plus, before the outputs,
 *   workspace, device, non-null, 8-byte aligned   at least rnampnn_design_count_long_workspace_bytes(B, T, count_cap) bytes; its contents
 *   workspace_bytes, host                         before the call do not matter, after it they are unspecified
 * and the outputs are rnampnn_design_count's.  The contract is rnampnn_design_count's, word for word - leaves, tree, window, target, k_min
 * rule, draw, uniforms, robustness, seq_nll and `infeasible` - and whenever rnampnn_design_count accepts the call every output of this entry
 * equals its output, byte for byte: each coefficient is one LSE over the same terms in the same order whoever computes it, the total and the
 * splits of a level with at most four nodes are selected by a wave-wide scan, every other split by one thread, as there.  G+C has no entry of
 * its own: counted = 12 everywhere and count_cap >= T gives the bytes of rnampnn_design_gc.
 *   Workspace.  The tree of RNA b - the levels 1 .. ceil(log2 T), [level][node][coefficient], node (l, i) at min(2 * (its extent within T), T,
 *     cap) + 1 doubles - lies at workspace + 8 b doubles(T, cap) bytes, doubles as in rnampnn_design_count: 172,288 bytes per RNA at T = 1025
 *     uncapped, 888,608 at T = 4417 uncapped, 247,728 at (4417, cap 8).  It is built ONCE per RNA and read by all S samples; a sample's
 *     per-node counts live in the LDS of its workgroup, never in the tree.  rnampnn_design_count_long_workspace_bytes returns
 *     8 B doubles(T, min(count_cap, T)), and 0 when an argument is <= 0; a call with count_cap = 0 (nothing may count) needs the bytes of
 *     count_cap = 1.
 *   Launches, all on `stream`, stream order between them: level 1 from the rows, one node per thread; one launch per level l = 2 .. ceil(log2 T)
 *     dealt flat over (RNA, node, coefficient), so the top levels of one long RNA spread over the device (13 launches at T = 4417); then one
 *     256-thread workgroup per (RNA, sample) that recomputes `infeasible` and k_min from the leaves, reads the root, walks down reading the
 *     halves from the workspace and writes the rows.  Dynamic LDS of that workgroup: 2 * (4 * ceil(T / 2) rounded up to 16) + T rounded up to
 *     16 + 96 bytes - the counts of the level being split and of the level below it, the class ids, the scratch: 41,056 bytes at T = 8192.  It
 *     does not depend on the cap.  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes: T <= 32744 (163,824 bytes) at every cap;
 *     the message names the bytes, the limit and that T.
 * No atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured graph,
 * and a draw is a pure function of (seed, s, b) and the rows of RNA b - independent of B, T, S, the layout and the workspace; the first S' of
 * S slots are the call with S'.
 * RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design_count; a null, too small or not 8-byte aligned workspace.
 * With every output null the call returns RNAMPNN_OK without a launch. */
size_t rnampnn_design_count_long_workspace_bytes(int32_t B, int32_t T, int32_t count_cap);
int rnampnn_design_count_long(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                              float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                              const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                              const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap,
                              void* workspace, size_t workspace_bytes, int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* count,
                              int32_t* count_miss, void* stream);
/* Distinct designs in ONE launch (csrc/design_distinct.hip): S pairwise DIFFERENT sequences per RNA under the constraints of rnampnn_design -
 * with noise != 0 an exact sample WITHOUT replacement from the constrained, tempered distribution, in sampling order; with noise == 0 the S
 * most probable admitted sequences, in descending order - each with its log-probability under that distribution.  One algorithm, a beam of
 * width S over the units with conditioned Gumbel keys (Kool, van Hoof, Welling 2019, "Stochastic Beams and Where to Find Them"); it is exact
 * because the units are independent.  The arguments are those of rnampnn_design plus
 *   noise                 != 0: sample without replacement; 0: the S best
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   logp (S,B) f32        phi of the slot (below), rounded once: the log-probability of the sequence under the constrained, tempered
 *                         distribution it was drawn from; -inf for an empty slot
 *   n_distinct (B) i32    slots filled = min(S, the number of admitted sequences); filled slots are pairwise different
 * with  seqs (S,B,T) i8   the sequence of slot s; -1 at t >= n_b and -1 everywhere in a slot s >= n_distinct[b]; every valid position of a
 *                         filled slot holds an id in 0..3 whatever the inputs hold
 *       seq_nll (S,B) f32 byte for byte rnampnn_score's seq_nll of a filled slot; +inf for an empty one
 *       infeasible (B)    as in rnampnn_design.
 * Both layouts, the padded `allowed` / `partner` / per-position `bias`, wobble, seed_dev, the clamping of lengths and offsets, the alignment
 * rules, "an empty mask is drawn free and counts 1" and "a pair without an admitted compatible cell makes both ends single positions and
 * counts 2" are rnampnn_design's.  All arithmetic is fp64: z_t(c) = ((double) logit_t(c) + (double) bias_t(c)) / (double) temperature.
 *   Units, walking t = 0 .. n_b - 1.  A single position is a unit; its cells are the admitted classes in class order.  The lower end of a
 *     feasible pair i < j is a unit; its cells are the admitted compatible cells (a,b) in a-major order (at most 6), z = z_i(a) + z_j(b);
 *     i receives a, j receives b.  The upper end of a feasible pair is no unit.  l_u(c) = z(c) - LSE(z over the unit's cells), LSE as in
 *     rnampnn_design_gc.  phi(prefix) = the sum of l over its units, added in unit order.
 *   Beam.  One empty prefix at slot 0 with phi = 0, G = 0.  At a unit every slot i, in slot order, gives one candidate per cell c with
 *     phi_ic = phi_i + l_u(c) and the key
 *       noise == 0:  kappa_ic = phi_ic
 *       noise != 0:  g_ic = phi_ic - log(-log u_ic);  Z_i = max_c g_ic (NaN ignored);  the children with g_ic == Z_i get kappa_ic = G_i exactly;
 *                    the others v = G_i - g_ic + log1p(-exp(g_ic - Z_i)),  kappa_ic = G_i - max(0, v) - log1p(exp(-|v|))
 *     and a NaN key is replaced by -inf.  The candidates with the S largest keys survive, ordered by key descending, then parent slot
 *     ascending, then cell ascending; they become slots 0, 1, .. in that order with G = kappa.  A unit with ONE cell makes no selection: every
 *     slot keeps its place, phi += l (0 for a finite z), G stays (noise == 0: G = phi).  After the last unit slot s is output s.  An RNA
 *     of length 0 has the one empty sequence: n_distinct = 1, logp = 0, seq_nll = 0.
 *   Uniforms, keyed by the PREFIX, not by the slot; mix64 as in rnampnn_design, arithmetic modulo 2^64, SALT the constant below:
 *       H(empty) = mix64(mix64(seed ^ SALT) ^ 0xD6E8FEB86659FD93 * (b+1))
 *       H(child) = mix64(H(parent) ^ 0xBF58476D1CE4E5B9 * (16 * (t+1) + cell)),  t the unit's position, cell = c or 4 a + b
 *       u = ((double) (H(child) >> 11) + 0.5) * 2^-53
 *     With seed_dev the XOR is taken on the device.
 *   Consequences.  The result is a pure function of (seed, b, the rows of RNA b, S): it does not depend on B, T or the layout.  Slots
 *     0 .. S'-1 of a call with S are the call with S' (the survivors of a narrower beam are the best of the wider one's, by induction over the
 *     units).  With noise, slot 0 is ONE exact draw from the constrained tempered distribution and slots 0..s are an exact sample without
 *     replacement in sampling order: P(slot 1 = y | slot 0 = x) = p(y) / (1 - p(x)).  A device result differs from a float64 restatement
 *     only where two keys that a selection compared lie within the rounding of exp / log of one another (about 1e-14, relative).
 * One 256-thread workgroup per RNA.  The beam lives in dynamic LDS, whose size depends on (S, T) alone:
 *       bytes(S, T) = 144 S + 16 ceil(S / 8) + 6,752 + 16 ceil((S + ceil(S / 2)) T / 16)
 *     (slot state 48 S, two candidate arrays 96 S, the survivors' table, the cells of 128 positions and the reduction's scratch, the history
 *     of 12 bits per slot and position): 61,920 at (S = 8, T = 4500), 113,728 at (64, 1017), 93,280 at (256, 128), 159,328 at (256, 300).
 *     RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes; the message names the bytes, the limit and the largest T at that S
 *     (1539 at S = 64, 311 at S = 256).
 *   S <= RNAMPNN_DESIGN_DISTINCT_MAX_S = 256; a larger S is RNAMPNN_ERR_BAD_ARG and the message names the limit.
 * No workspace, no atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes and the call can sit inside
 * a captured graph.  RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design; S > 256.  The LDS check comes next; then,
 * with every output null, the call returns RNAMPNN_OK without a launch. */
#define RNAMPNN_DESIGN_DISTINCT_SALT 0xE7037ED1A0B428DBull
#define RNAMPNN_DESIGN_DISTINCT_MAX_S 256
int rnampnn_design_distinct(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                            float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                            const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position, int32_t noise,
                            int8_t* seqs, float* seq_nll, int32_t* infeasible, float* logp, int32_t* n_distinct, void* stream);
/* Design that avoids forbidden motifs in ONE launch (csrc/design_avoid.hip): the draws of rnampnn_design, conditioned EXACTLY on the sequence
 * containing none of a set of substrings (no GGGG, no homopolymer run, no restriction site).  The set comes as an Aho-Corasick automaton with
 * the failure links compiled out (rnampnn/utils/motifs.py builds it).  The arguments are those of rnampnn_design plus
 *   delta (A,4) u8, device, non-null   delta[a,c] = the state after reading class c (AUCG = 0..3) in state a; state 0 is the start
 *   n_states i32, host                 A, 1 .. RNAMPNN_DESIGN_AVOID_MAX_STATES = 64 (one lane of a wave per state)
 *   terminal u64, host                 bit a set = a motif ends in state a; bits at and above A are ignored; bit 0 must be clear
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   hits (S,B) i32         the positions of the written draw after which the automaton, following delta from state 0, is in a terminal state
 *                          (for a delta built from motifs: the positions at which a motif ends)
 *   avoid_miss (B) i32     1 when no admitted sequence of RNA b avoids the motifs, else 0; the same for every sample
 * Extent, masks, bias, temperature, `allowed`, seed_dev and "an empty mask is drawn free and counts 1 in `infeasible`" are rnampnn_design's.
 * All arithmetic is fp64: z_t(c) = ((double) logit_t(c) + (double) bias_t(c)) / (double) temperature; LSE and SELECT (weights exp(x - max over
 * the admitted), the first whose running sum exceeds u24 * 2^-24 * total, else the last admitted) are rnampnn_design_gc's; m_t is the mask of t.
 *   Live and dead.  A state is DEAD when its bit of `terminal` is set; a delta entry >= A is read as a dead state.  The other states are LIVE.
 *   Backward.  l_n(a) = 0 for a live a.  For t = n-1 .. 0 and a live a: l_t(a) = LSE over the classes c in class order of
 *     z_t(c) + l_{t+1}(delta(a,c)), a cell being admitted iff m_t has c and delta(a,c) is live.  l of a dead state is -inf.
 *   Feasibility.  avoid_miss[b] = !(l_0(0) > -inf) (a NaN counts as not above -inf); an RNA of length 0 is feasible.
 *   Draw of sample s, feasible RNA.  a = 0; for t = 0 .. n-1: the admitted cells are those above that also have l_{t+1}(delta(a,c)) > -inf;
 *     c = SELECT over z_t(c) + l_{t+1}(delta(a,c)) with the uniform u24(seed, s, b, t) of rnampnn_design; a <- delta(a,c).  Every hits is 0.
 *   Infeasible RNA (avoid_miss = 1).  Every position is drawn as rnampnn_design draws an unpaired position in fp64, with the same uniform,
 *     ignoring the motifs; `hits` reports what the draw contains.  (Counting follows delta through dead states; after an entry >= A, which
 *     counts, it goes on from state 0.)
 *   Base pairs.  A non-null `partner` is RNAMPNN_ERR_UNSUPPORTED: a pair couples two distant positions, so an exact chain over (position,
 *     state) would have to carry the class of every open pair in its state - 4^depth states.  That is not built; fixed / IUPAC sets, omitted
 *     letters and either bias all combine with the motifs.
 * seq_nll is byte for byte rnampnn_score's for the written draw.  One 256-thread workgroup per RNA: the rows in LDS, one wave (lane = state)
 * runs the backward pass into an LDS table of the live states, then 64 samples at a time walk forward, one lane each.  Dynamic LDS, with
 * L = the live states among 0 .. A-1:
 *       bytes(T, L) = (32 + 8 L) T + 256 (ceil(T / 16) | 1) + 16 ceil(T / 16) + 864
 *     (the fp64 rows, the table, 2 bits per position for 64 samples, the masks; the automaton, the hit counts and the reduction's scratch):
 *     20,704 at (T = 128, L = 13), 46,832 at (300, 13).  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes; the message names
 *     the bytes, the limit and the largest T at that automaton: T <= 2857 at L = 1, 1064 at L = 13 (no run longer than 3), 532 at L = 32,
 *     290 at L = 64.  A table in global memory for longer RNAs is not built.
 * No workspace, no atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a
 * captured graph, and a draw is a pure function of (seed, s, b), the rows of RNA b and the automaton - independent of B, T, S and the layout;
 * the first S' of S slots are the call with S'.  RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design; null delta;
 * n_states outside 1 .. 64; bit 0 of terminal set.  Then the partner check, then the LDS check; then, with every output null, the call
 * returns RNAMPNN_OK without a launch. */
#define RNAMPNN_DESIGN_AVOID_MAX_STATES 64
int rnampnn_design_avoid(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                         float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                         const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                         const uint8_t* delta, int32_t n_states, uint64_t terminal, int8_t* seqs, float* seq_nll,
                         int32_t* infeasible, int32_t* hits, int32_t* avoid_miss, void* stream);
/* Design with REQUIRED motifs in ONE launch (csrc/design_dfa.hip): the draws of rnampnn_design, conditioned EXACTLY on the sequence being
 * accepted by a deterministic finite automaton - every one of a list of motifs occurs somewhere (a GNRA tetraloop, a Shine-Dalgarno stretch,
 * a primer word), none of another list does.  rnampnn/utils/motifs.py builds it (DesignAutomaton: the Aho-Corasick automaton of all words,
 * times the set of required motifs seen so far).  rnampnn_design_avoid is the special case "every live state accepts"; this entry adds the
 * acceptance set, automata of up to 256 states, and a table of partition sums that lives in GLOBAL memory.  The arguments are those of
 * rnampnn_design up to bias_per_position, plus
 *   delta (A,4) u8, device, non-null   as rnampnn_design_avoid's
 *   kind (A) u8, HOST, non-null        bit 0 = the state is dead, bit 1 = it accepts (read only where bit 0 is clear); read during the call,
 *                                      on the host (it sizes the table and travels to the kernel as 2 x 256 bits of launch arguments), so
 *                                      the call stays free of host synchronisation; the array may be freed when the call returns;
 *                                      kind[0] & 1 must be clear
 *   n_states i32, host                 A, 1 .. RNAMPNN_DESIGN_DFA_MAX_STATES = 256 (one thread of the workgroup per state)
 *   workspace, workspace_bytes         device memory, 8-byte aligned, at least rnampnn_design_dfa_workspace_bytes(B, T, L) =
 *                                      8 B T L bytes, L = the states among 0 .. A-1 whose bit 0 is clear (0 when an argument is <= 0).  It
 *                                      holds the table l_t(a) as [b][t][live column] and nothing else; its contents before the call do not
 *                                      matter (every entry that is read was written by the same launch before), after it they are unspecified
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   hits (S,B) i32         the dead states the written draw enters, following delta from state 0 (as rnampnn_design_avoid counts them)
 *   accepted (S,B) i32     1 iff the state after the last position is live and accepting
 *   dfa_miss (B) i32       1 when no admitted sequence of RNA b is accepted, else 0; the same for every sample
 * Everything not named here is rnampnn_design_avoid's, word for word: extent, masks, bias, temperature, `allowed`, seed_dev, "an empty mask
 * is drawn free and counts 1 in `infeasible`", z_t(c) in fp64, LSE in class order, SELECT, u24(seed, s, b, t), live and dead (a delta entry
 * >= A is read as a dead state), and the refusal of a non-null `partner` (RNAMPNN_ERR_UNSUPPORTED, for the same reason).
 *   Backward.  l_n(a) = 0 for a live ACCEPTING a, -inf for every other state.  For t = n-1 .. 0 and a live a: l_t(a) = LSE over the classes
 *     c in class order of z_t(c) + l_{t+1}(delta(a,c)), a cell being admitted iff m_t has c and delta(a,c) is live.
 *   Feasibility.  dfa_miss[b] = !(l_0(0) > -inf); an RNA of length 0 is feasible iff state 0 accepts.
 *   Draw of sample s, feasible RNA.  rnampnn_design_avoid's walk over z_t(c) + l_{t+1}(delta(a,c)).  Every hits is 0, every accepted 1.
 *   Infeasible RNA (dfa_miss = 1).  Every position is drawn as rnampnn_design draws an unpaired position in fp64, with the same uniform,
 *     ignoring the automaton; `hits` and `accepted` report what was written (after a delta entry >= A, which counts, it goes on from 0).
 *   Anchor.  With A <= 64 and every live state accepting, seqs, seq_nll, infeasible, hits and dfa_miss are byte for byte the outputs of
 *     rnampnn_design_avoid on (delta, A, terminal = the dead states).
 * One 256-thread workgroup per RNA: thread = state runs the backward pass with l_{t+1} and l_t in two LDS rows (one barrier per step) and
 * stores l_t to the workspace; then 256 samples at a time walk forward, one lane each, reading their four candidates from the workspace
 * (written by the same workgroup: a barrier orders them).  LDS does not grow with T x L.  Dynamic LDS:
 *       bytes(T) = 32 T + 16 ceil(T / 16) + 1024 (ceil(T / 16) | 1) + 8,032
 *     (the fp64 rows, the masks, 2 bits per position for 256 samples; the two rows of l, the automaton and the reduction's scratch):
 *     37,392 at T = 300, 124,432 at T = 1200.  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes, for every automaton alike:
 *     T <= 1587 (163,840 bytes); the message names the bytes, the limit and that T.  One code path: an LDS table for small T x L is not built.
 * No atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured
 * graph, and a draw is a pure function of (seed, s, b), the rows of RNA b and the automaton - independent of B, T, S, the layout and the
 * workspace; the first S' of S slots are the call with S'.  RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design;
 * null delta; null kind; n_states outside 1 .. 256; bit 0 of kind[0] set; a null, misaligned or too small workspace.  Then the partner
 * check, then the LDS check; then, with every output null, the call returns RNAMPNN_OK without a launch. */
#define RNAMPNN_DESIGN_DFA_MAX_STATES 256
size_t rnampnn_design_dfa_workspace_bytes(int32_t B, int32_t T, int32_t n_live);
int rnampnn_design_dfa(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                       float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                       const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                       const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace, size_t workspace_bytes,
                       int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits, int32_t* accepted, int32_t* dfa_miss, void* stream);
/* Design with motifs UNDER A COUNT WINDOW in ONE launch (csrc/design_dfa_count.hip): the draws of rnampnn_design, conditioned EXACTLY on
 * BOTH the sequence being accepted by the automaton of rnampnn_design_dfa AND the count of rnampnn_design_count lying in its window - no
 * G-quadruplex run, no restriction site and a primer word with G+C between 45 % and 60 %; at most 6 mutations and no GAAUUC.  The count
 * joins the automaton's chain as a third index.  The arguments are those of rnampnn_design up to bias_per_position, then
 *   delta, kind (HOST), n_states                    as rnampnn_design_dfa's
 *   counted, count_lo, count_hi, count_cap          as rnampnn_design_count's; cap = min(count_cap, T) and K = min(cap, n_b) below
 *   workspace, workspace_bytes                      device memory, 8-byte aligned, at least 8 B T L (cap + 1) bytes, L the live states.  It
 *                                                   holds the table l_t(a, k) as [b][t][live column][k], k = 0 .. cap, and nothing else; its
 *                                                   contents before the call do not matter (every entry that is read was written by the same
 *                                                   launch before), after it they are unspecified.
 *                                                   rnampnn_design_dfa_count_workspace_bytes(B, T, L, count_cap) returns that size, and 0 when
 *                                                   an argument is <= 0; a call with cap 0 (nothing may count) needs the bytes of ONE slab
 *                                                   per position, 8 B T L, which the size at count_cap = 1 covers.  The table grows with
 *                                                   the cap: about 33 MB at (B = 256, T = 140, L = 13) with a budget of 8, about 525 MB with
 *                                                   a G+C window (cap = T) - the price of a draw that is exact in both conditions
 * and the outputs, each nullable, are those of rnampnn_design plus
 *   hits, accepted (S,B) i32   as rnampnn_design_dfa's, of what was written
 *   count (S,B) i32            the sum over the ids written for that draw of bit(counted[b,t], id_t)
 *   dfa_miss (B) i32           1 when no admitted sequence of RNA b is accepted with a count in 0 .. K, else 0
 *   count_miss (B) i32         0 when a count of the window is reachable (and when dfa_miss), else the distance from the window to the target
 *   log_z (B) f64              the log partition sum of what the draws come from: the LSE over the window's counts of root(k), root(target)
 *                              when a target is used, -inf when dfa_miss
 * Taken word for word from rnampnn_design_dfa: extent, masks, bias, temperature, `allowed`, seed_dev, "an empty mask is drawn free and counts 1
 * in `infeasible`", z_t(c) in fp64, the LSE of four terms in class order, the weights and SELECT of a position, u24(seed, s, b, t), live and
 * dead states (a delta entry >= A is read as dead) and the refusal of a non-null `partner` (RNAMPNN_ERR_UNSUPPORTED, for the same reason).
 * From rnampnn_design_count: bit(counted[b,t], c), the clamping of lo and hi to [0, K] followed by hi = max(hi, lo), SELECT over counts and
 * RNAMPNN_DESIGN_GC_SALT.
 *   Backward.  l_n(a, k) = 0 for a live accepting a and k = 0, -inf otherwise.  For t = n-1 .. 0, a live a and k = 0 .. K:
 *     l_t(a, k) = LSE over the classes c in class order of z_t(c) + l_{t+1}(delta(a,c), k - d_t(c)), d_t(c) = bit(counted_t, c); a cell is
 *     admitted iff m_t has c, delta(a,c) is live and k - d_t(c) >= 0.  An entry with k > n - t is -inf (a suffix of n - t positions counts no
 *     more) and may be written without arithmetic.
 *   Total.  root(k) = l_0(0, k).  If a count of lo .. hi has a finite root, sample s draws K_s = SELECT(lo .. hi in count order, root,
 *     u24(seed ^ SALT, s, b, 0)).  Otherwise, if a count of 0 .. K has one, the target is the nearest such count, the lower one on a tie,
 *     count_miss its distance to the window, and every sample holds the target.  Otherwise dfa_miss = 1, count_miss = 0 and every position
 *     is drawn as rnampnn_design draws an unpaired position in fp64 with u24(seed, s, b, t), ignoring both conditions.  hits, accepted and
 *     count always report what was written.  An RNA of length 0 is feasible iff state 0 accepts.
 *   Walk.  a = 0, r = K_s.  At t the admitted cells are those above (with k = r) that also have l_{t+1}(delta(a,c), r - d_t(c)) > -inf - at
 *     the last position that value is 0 iff delta(a,c) accepts and r - d_t(c) = 0; c = SELECT over z_t(c) + that value with u24(seed, s, b, t);
 *     a <- delta(a,c), r <- r - d_t(c).
 *   Anchors.  With nothing counted (counted = 0 everywhere, at any count_cap, 0 included) and the window (0, 0), seqs, seq_nll, infeasible,
 *     hits, accepted and dfa_miss are the bytes of rnampnn_design_dfa on the same automaton; count and count_miss are 0.  (A class that
 *     counts is not admitted at count_cap = 0: that call conditions on "none of them occurs".)  The outputs of an RNA do not
 *     depend on count_cap as long as its window lies within the cap and a count of the window is reachable.
 * One 256-thread workgroup per RNA.  The items (live column, k) of step t, L (K + 1) of them, are dealt flat over the threads, each one LSE
 * over four entries of the slab of t + 1; that slab is read from two slabs in LDS when 16 L (cap + 1) bytes fit beside the rest, otherwise
 * from the workspace (written by the same workgroup: a barrier orders them) - the same four-term LSE either way, so the two homes give the
 * same bytes; every entry goes to the workspace, from which 256 samples at a time, one lane each, read the four candidates of their walk.
 * Dynamic LDS without the slabs:
 *       bytes(T) = 32 T + 32 ceil(T / 16) + 1024 (ceil(T / 16) | 1) + 4,192
 *     (the fp64 rows, the masks and the counted sets, 2 bits per position for 256 samples; the automaton and the scratch): 33,856 at
 *     T = 300.  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes, for every automaton and every cap alike: T <= 1616
 *     (162,560 bytes); the message names the bytes, the limit and that T.  LDS bounds neither L x K nor T x L.
 * No atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured
 * graph, and a draw is a pure function of (seed, s, b), the rows of RNA b, the automaton and the RNA's counted, lo and hi - independent of
 * B, T, S, the layout and the workspace's previous contents; the first S' of S slots are the call with S'.
 * RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of rnampnn_design_dfa; null counted, count_lo or count_hi; count_cap < 0; a
 * null, misaligned or too small workspace (the message names the bytes needed).  Then the partner check, then the LDS check; then, with
 * every output null, the call returns RNAMPNN_OK without a launch. */
size_t rnampnn_design_dfa_count_workspace_bytes(int32_t B, int32_t T, int32_t n_live, int32_t count_cap);
int rnampnn_design_dfa_count(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                             float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                             const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                             const uint8_t* delta, const uint8_t* kind, int32_t n_states, const uint8_t* counted,
                             const int32_t* count_lo, const int32_t* count_hi, int32_t count_cap, void* workspace, size_t workspace_bytes,
                             int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits, int32_t* accepted, int32_t* count,
                             int32_t* dfa_miss, int32_t* count_miss, double* log_z, void* stream);
/* Design with motifs UNDER BASE PAIRS in ONE launch (csrc/design_nested.hip): the draws of rnampnn_design on a NESTED (pseudoknot-free)
 * structure, conditioned EXACTLY on the sequence being accepted by the automaton of rnampnn_design_dfa.  A nested structure is a tree, and
 * on a tree the automaton is carried as a transfer table per enclosed interval (state before its first position -> state after its last):
 * L^2 per position at L live states, whatever the depth.  The arguments are rnampnn_design_dfa's, in its order, and mean what they mean
 * there - but `partner` is honoured instead of refused - with
 *   n_states i32, host                 A, 1 .. 256, of which at most RNAMPNN_DESIGN_NESTED_MAX_LIVE = 64 live (bit 0 of kind clear)
 *   workspace, workspace_bytes         device memory, 8-byte aligned, at least rnampnn_design_nested_workspace_bytes(B, T, L) =
 *                                      8 B T L^2 + 256 B (floor(T / 2) + 1) bytes (0 when an argument is <= 0): the tables R_t as
 *                                      [b][t][L][G] (G = L inside a pair, 1 at the top level: a top-level vector lies at the start of its
 *                                      slot), then one byte per (b, open pair, lane) for the goals of a walking sample's open pairs.  Its
 *                                      contents before the call do not matter (every byte that is read was written by the same launch
 *                                      before), after it they are unspecified
 * and the outputs, each nullable, are rnampnn_design_dfa's plus
 *   nest_miss (B) i32      1 when two of the RNA's pairs cross (a pseudoknot), else 0
 * z, masks, bias, temperature, `allowed`, seed_dev, u24, LSE, SELECT, live and dead states and "an empty mask is drawn free and counts 1 in
 * `infeasible`" are rnampnn_design_dfa's, word for word; all arithmetic is fp64.  A delta entry >= A is read as a dead state.
 *   Pairs.  `partner` is validated as in rnampnn_design (symmetric, inside the RNA, not itself).  A pair without a compatible cell that
 *     both masks admit becomes two unpaired positions and counts 2 in `infeasible`, as in rnampnn_design.  After that nest_miss[b] = 1 iff
 *     two remaining pairs cross: i < k < j < l.
 *   Loops.  The loop of a pair (i, j): the positions strictly between i and j that lie inside no deeper pair, plus the openers of its child
 *     pairs; the top level is the loop of the whole RNA.  Its elements are its unpaired positions and its child pairs, in position order.
 *   Tables.  For a position t that is unpaired or an opener, R_t(a, g) = the log of the total weight of everything from t to the end of
 *     t's loop that starts in live state a before t, stays live, and ends in goal g.  In an inner loop g ranges over the live states (the
 *     state after the loop's last position) and the table behind the last element is the identity (0 on the diagonal, -inf elsewhere).  At
 *     the top level there is one goal, "accepted", and the table behind position n-1 is 0 for a live accepting state, -inf for every other.
 *   Recurrence, t = n-1 .. 0, N = the table of the next element of the same loop.
 *     Unpaired t: R_t(a, g) = LSE over the classes c in class order of z_t(c) + N(delta(a,c), g); admitted iff m_t has c and delta(a,c) is live.
 *     Opener t of the pair (t, j): P_t(a, b) = LSE over the compatible cells (c, c') in a-major order that both masks admit, and within a
 *       cell over the live b' ascending with delta(b', c') = b, of z_t(c) + z_j(c') + R^in(delta(a,c), b'); R^in = the table of the first
 *       element inside (t, j), the identity when j = t + 1.  Then R_t(a, g) = LSE over the live b ascending of P_t(a, b) + N(b, g), N the
 *       table behind j in t's loop.  A top-level position thus holds exactly rnampnn_design_dfa's vector l_t.
 *   Feasibility.  dfa_miss[b] = !(R_0(0, accepted) > -inf); an RNA of length 0 is feasible iff state 0 accepts.  On an RNA with
 *     nest_miss = 1 no table is built and dfa_miss = 0.
 *   Draw of sample s, feasible nested RNA.  Walk t = 0 .. n-1 with a state a, a goal g and a stack of goals.  Unpaired: SELECT over
 *     z_t(c) + N(delta(a,c), g), only finite cells admitted, u24(seed, s, b, t); a <- delta(a, c).  Opener: ONE SELECT over (c, c', b') in
 *     the order of P_t of z_t(c) + z_j(c') + R^in(delta(a,c), b') + N(delta(b',c'), g), only finite cells admitted, u24(seed, s, b, t) (the
 *     pair's lower index, as in rnampnn_design); t receives c, j receives c'; push g, g <- b', a <- delta(a, c).  Closer j: a <- delta(a,
 *     its class), pop g.  Every hits is 0, every accepted 1.
 *   Miss (dfa_miss or nest_miss).  The RNA is drawn as rnampnn_design draws it, in fp64, ignoring the automaton: pairs jointly, unpaired
 *     positions singly; `hits` and `accepted` report what was written, as in rnampnn_design_dfa.
 *   Anchor.  On an RNA without a valid pair (a null `partner` included) every output is rnampnn_design_dfa's byte for byte.
 * One 256-thread workgroup per RNA: the L x G entries of a step are dealt over the threads; an opener forms P_t in an LDS tile next to a
 * second one that holds R^in and then N; barriers of the workgroup order the workspace accesses.  Then 256 samples at a time walk, one lane
 * each.  Dynamic LDS:
 *       bytes(T, L) = 36 T + max(16 L^2, 1024 (ceil(T / 16) | 1)) + 1,952
 *     (the fp64 rows, the partners, masks and level flags; two L x L tiles, over which later lie 2 bits per position for 256 samples; the
 *     automaton and the reduction's scratch): 103,488 at (T = 1000, L = 64), 102,464 at (1000, 13).  RNAMPNN_ERR_UNSUPPORTED when that exceeds
 *     160 KiB = 163,840 bytes: T <= 1616 (163,552 bytes) at every L <= 64; the message names the bytes, the limit and that T.  More than 64 live states:
 *     RNAMPNN_ERR_UNSUPPORTED, the message names the count and the limit.
 * No atomics, no runtime fill / copy node, no host synchronisation: two calls give identical bytes, the call can sit inside a captured
 * graph, and a draw is a pure function of (seed, s, b), the rows of RNA b, its pairs and the automaton - independent of B, T, S, the layout
 * and the workspace; the first S' of S slots are the call with S'.  RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of
 * rnampnn_design_dfa.  Then the live-state check, then the LDS check; then, with every output null, the call returns RNAMPNN_OK without a
 * launch. */
#define RNAMPNN_DESIGN_NESTED_MAX_LIVE 64
size_t rnampnn_design_nested_workspace_bytes(int32_t B, int32_t T, int32_t n_live);
int rnampnn_design_nested(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                          float temperature, int32_t S, uint64_t seed, const uint64_t* seed_dev, const uint8_t* allowed,
                          const int32_t* partner, int32_t wobble, const float* bias, int32_t bias_per_position,
                          const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace, size_t workspace_bytes,
                          int8_t* seqs, float* seq_nll, int32_t* infeasible, int32_t* hits, int32_t* accepted, int32_t* dfa_miss,
                          int32_t* nest_miss, void* stream);
/* Design PROFILES in ONE launch each (csrc/design_profile.hip): what rnampnn_design_count and rnampnn_design_avoid draw FROM, not draws - the
 * exact per-position marginals, log partition sums and entropy of the distribution the draw entry of the same mode samples, in fp64.  The
 * inputs mean exactly what they mean in that draw entry: both layouts, z_t(c) = ((double) logit_t(c) + (double) bias_t(c)) / (double)
 * temperature, the admitted sets, "an empty mask is drawn free and counts 1 in `infeasible`", "a pair without an admitted compatible cell
 * becomes two single positions and counts 2", wobble and the validation of `partner`, the clamping of the window and the target rule, the live
 * and the dead states.  There is no S, no seed and no seqs.  Outputs, each nullable:
 *   marginals (B,T,4) f64  padded in both layouts, 16-byte aligned; P(x_t = c) under the distribution the draw entry samples from; written as 0
 *                          at t >= n_b, so stale bytes are overwritten
 *   log_z (B) f64          the log partition sum of z over the set drawn from
 *   log_z_free (B) f64     the sum over t of the LSE over all four classes of z_t(c): no `allowed`, no pairs, no window, no motifs;
 *                          log_z - log_z_free <= 0 is the log of the mass the constraints keep (0 to the rounding of two sums added in
 *                          different orders when they keep all of it)
 *   entropy (B) f64        log_z - sum over t, c of P_t(c) z_t(c), in nats; a term with P_t(c) = 0 is skipped
 *   infeasible (B) i32, count_miss / avoid_miss (B) i32   the draw entry's values, byte for byte
 * An RNA of length 0 has log_z = log_z_free = entropy = 0.
 *   rnampnn_design_count_profile.  Leaves p_t(d), tree, window and target are rnampnn_design_count's.  K* = the counts of the window with a
 *     finite root coefficient; on a miss, the target alone.  log_z = LSE over K* of the root coefficients.  Outside pass, top down, log domain:
 *     O_root(k) = 0 for k in K*, else -inf; a node with outside O and halves L, R gives O_L(a) = LSE over k of O(k) + R(k - a) and
 *     O_R(b) = LSE over k of O(k) + L(k - b), k over the node's coefficients with k - a (k - b) among the sibling's; a node whose right half is
 *     empty hands O to its left half.  With the cap every index stays <= cap and O is -inf above K*, so truncation is exact as it is for the
 *     inside pass.  A single position: P_t(c) = exp(z_t(c) + O_t(bit(counted_t, c)) - log_z) for the admitted c, else 0.  A feasible pair
 *     i < j: cell (a, b) has probability exp(z_i(a) + z_j(b) + O_i(d_ab) - log_z); P_i(a) and P_j(b) are its row and column sums.  Under
 *     the k_min rule (no finite root coefficient) every leaf is restricted to the admitted cells of its own smallest d and normalised over
 *     them; log_z is the sum over the leaves of p_t(that d).
 *   rnampnn_design_avoid_profile.  The backward table l_t(a) is rnampnn_design_avoid's.  Forward: alpha_0(0) = 0, alpha_0(a != 0) = -inf;
 *     alpha_{t+1}(a') = LSE over the admitted cells (a, c) with delta(a,c) = a' live of alpha_t(a) + z_t(c).  log_z = l_0(0).
 *     P_t(c) = the sum over a of exp(alpha_t(a) + z_t(c) + l_{t+1}(delta(a,c)) - log_z) over the admitted cells.  With avoid_miss = 1
 *     every position is the softmax over its admitted classes - what the draw entry falls back to - and log_z is the sum of their LSEs.
 *     A non-null `partner` is RNAMPNN_ERR_UNSUPPORTED, as in the draw entry.
 * The order of summation is not part of the contract: the outputs agree with a float64 restatement to rounding (tests hold marginals to 1e-8
 * absolute and the scalars to 1e-8 max(1, |value|)) and are byte-identical between two calls, between the layouts and between batches.
 * Non-finite logits or bias of one RNA may make THAT RNA's outputs NaN; nothing faults, no index leaves its array, no other RNA changes.
 * One 256-thread workgroup per RNA.  Dynamic LDS:
 *   count:  bytes(T, cap) = 16 * doubles(T, cap) + 240, doubles as in rnampnn_design_count (the inside AND the outside tree: a child's outside
 *           reads its sibling's inside): 14,432 bytes at (T = 128, cap 8), 83,296 at (300, 300); T <= 1457 at cap 8, 1128 at cap 16, 535 for cap >= T
 *   avoid:  bytes(T, L) = (32 + 8 L) T + 16 ceil(T / 16) + 3,680, L the live states: 44,784 bytes at (T = 300, L = 13); T <= 1168 at L = 13 (163,696 bytes), 554 at L = 32, 293 at L = 64
 * RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes; the message names the bytes, the limit and the largest T.  No workspace,
 * no atomics, no runtime fill / copy node, no host synchronisation; the call can sit inside a captured graph.  RNAMPNN_ERR_BAD_ARG, before
 * anything is launched: the cases of the draw entry but those about S; marginals not 16-byte aligned.  Then, in both entries
 * alike: the `partner` refusal (avoid); with every output null RNAMPNN_OK without a launch, whatever T is; the LDS check. */
int rnampnn_design_count_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                 float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                 int32_t bias_per_position, const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi,
                                 int32_t count_cap, double* marginals, double* log_z, double* log_z_free, double* entropy,
                                 int32_t* infeasible, int32_t* count_miss, void* stream);
int rnampnn_design_avoid_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                 float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                 int32_t bias_per_position, const uint8_t* delta, int32_t n_states, uint64_t terminal,
                                 double* marginals, double* log_z, double* log_z_free, double* entropy, int32_t* infeasible,
                                 int32_t* avoid_miss, void* stream);
/* rnampnn_design_count_profile on trees in GLOBAL memory (csrc/design_long.hip).  The arguments and the outputs are those of
 * rnampnn_design_count_profile plus, before the outputs, `workspace` and `workspace_bytes` as in rnampnn_design_count_long, sized by
 * rnampnn_design_count_profile_long_workspace_bytes = twice rnampnn_design_count_long_workspace_bytes: the inside trees of the B RNAs, then
 * their outside trees, each in rnampnn_design_count_long's layout.  The contract is rnampnn_design_count_profile's, and whenever that entry
 * accepts the call every output of this one equals its output, byte for byte.  Launches on `stream`: the inside pass of
 * rnampnn_design_count_long; one workgroup per RNA for the target and the root's outside; the outside pass, one launch per level top down, dealt
 * flat over (RNA, child node, coefficient); one workgroup per RNA for the leaves, the marginals and the scalars (27 launches at T = 4417).
 * No dynamic LDS, so T is bound by the 16 levels the argument block addresses alone: T <= 65536, RNAMPNN_ERR_UNSUPPORTED naming it beyond.
 * No atomics, no runtime fill / copy node, no host synchronisation.  RNAMPNN_ERR_BAD_ARG, before anything is launched: the cases of
 * rnampnn_design_count_profile; a null, too small or not 8-byte aligned workspace.  With every output null RNAMPNN_OK without a launch. */
size_t rnampnn_design_count_profile_long_workspace_bytes(int32_t B, int32_t T, int32_t count_cap);
int rnampnn_design_count_profile_long(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                                      float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                                      int32_t bias_per_position, const uint8_t* counted, const int32_t* count_lo, const int32_t* count_hi,
                                      int32_t count_cap, void* workspace, size_t workspace_bytes, double* marginals, double* log_z,
                                      double* log_z_free, double* entropy, int32_t* infeasible, int32_t* count_miss, void* stream);
/* The profile of REQUIRED motifs in ONE launch (csrc/design_dfa_profile.hip): what rnampnn_design_dfa draws FROM, on its automaton of up to
 * 256 states, with the backward table in GLOBAL memory.  The arguments are rnampnn_design_avoid_profile's up to bias_per_position; then
 * delta, kind (HOST) and n_states exactly as rnampnn_design_dfa takes them; then workspace and workspace_bytes as in rnampnn_design_dfa,
 * sized by rnampnn_design_dfa_profile_workspace_bytes(B, T, L) = 8 B T L bytes at L live states (0 when an argument is <= 0): the table
 * l_t(a) as [b][t][live column] and nothing else; what it held before the call does not matter, what it holds after is unspecified.  Then
 * the outputs of the profile family, each nullable: marginals (B,T,4) f64 16-byte aligned, log_z, log_z_free, entropy, infeasible and
 * dfa_miss (B) i32.  The contract is the profile family's (above, at "Design PROFILES"), applied to the distribution rnampnn_design_dfa
 * samples:
 *   Backward.  The table l_t(a) is rnampnn_design_dfa's: l_n(a) = 0 for a live accepting state, -inf otherwise; LSE in class order; a cell
 *     (a, c) is admitted iff m_t has c and delta(a,c) is live.  log_z = l_0(0).  dfa_miss and infeasible are the draw entry's values, byte
 *     for byte.
 *   Forward.  alpha_0(0) = 0, alpha_0(a != 0) = -inf; alpha_{t+1}(a') = LSE over the admitted cells (a, c) with delta(a,c) = a' live of
 *     alpha_t(a) + z_t(c).  P_t(c) = the sum over a of exp(alpha_t(a) + z_t(c) + l_{t+1}(delta(a,c)) - log_z) over the admitted cells whose
 *     l_{t+1} is finite.  entropy and log_z_free are the family's; marginals is written as 0 at t >= n_b.  (The kernel walks
 *     q_t(a) = exp(alpha_t(a) + l_t(a) - log_z), the probability that the draw is in state a before position t, through the draw's own
 *     conditionals exp(z_t(c) + l_{t+1}(delta(a,c)) - l_t(a)): the same sums in [0, 1]; a state whose posterior is below 1e-308 counts 0.)
 *   Miss.  With dfa_miss = 1 every position is the softmax over its admitted classes - what the draw entry falls back to - and log_z is
 *     the sum of the positions' LSEs.  An RNA of length 0 has log_z = log_z_free = entropy = 0 and dfa_miss = !(state 0 accepts).
 *   Anchor.  With A <= 64 and every live state accepting the outputs agree with rnampnn_design_avoid_profile on (delta, A, terminal = the
 *     dead states) to the family's tolerances (the two sum in different orders) and the flags byte for byte.
 * The order of summation is not part of the contract; the family's rule of determinism is: two calls give identical bytes, so do the
 * padded and the packed layout, an RNA alone and in a batch, and whatever the workspace and the outputs held before.  Non-finite logits or
 * bias of one RNA may make THAT RNA's outputs NaN; nothing faults, no index leaves its array, no other RNA changes.
 * One 256-thread workgroup per RNA: thread = state runs rnampnn_design_dfa's backward pass into the workspace, then walks forward with
 * q_t(a) in its register, reading l_t(a) and l_{t+1}(delta(a, .)) from the workspace (written by the same workgroup: a barrier orders
 * them).  The marginals of a step are a fixed-order reduction of the 1,024 cells by class; the scatter along delta is a segmented sum
 * over the cells sorted by target, whose time does not depend on the in-degree of a state.  LDS does not grow with T x L.  Dynamic LDS:
 *       bytes(T) = 32 T + 16 ceil(T / 16) + 15,392
 *     (the fp64 rows, the masks; the cells of a step, q_{t+1}, the sorted cells, the automaton and the scratch): 25,296 at T = 300,
 *     68,720 at T = 1616.  RNAMPNN_ERR_UNSUPPORTED when that exceeds 160 KiB = 163,840 bytes, for every automaton alike: T <= 4498
 *     (163,840 bytes); the message names the bytes, the limit and that T.
 * No atomics, no runtime fill / copy node, no host synchronisation; the call can sit inside a captured graph.  RNAMPNN_ERR_BAD_ARG, before
 * anything is launched: the cases of rnampnn_design_dfa but those about S; marginals not 16-byte aligned.  Then the partner refusal
 * (RNAMPNN_ERR_UNSUPPORTED, in the draw entry's words); with every output null RNAMPNN_OK without a launch, whatever T is; the LDS check. */
size_t rnampnn_design_dfa_profile_workspace_bytes(int32_t B, int32_t T, int32_t n_live);
int rnampnn_design_dfa_profile(const float* logits, int64_t n_rows, const float* mask, const int32_t* cu_seqlens, int32_t B, int32_t T,
                               float temperature, const uint8_t* allowed, const int32_t* partner, int32_t wobble, const float* bias,
                               int32_t bias_per_position, const uint8_t* delta, const uint8_t* kind, int32_t n_states, void* workspace,
                               size_t workspace_bytes, double* marginals, double* log_z, double* log_z_free, double* entropy,
                               int32_t* infeasible, int32_t* dfa_miss, void* stream);

/* -- training ---------------------------------------------------------------------------- */
/* The training surface of RNAMPNN (rnampnn.py:187-207 + Lightning's loss.backward()):
 *   rnampnn_train_forward  - `self(coords, mask)` in train mode.  Dropout with probability `dropout` after every GELU
 *       (mpnn.py:140,150; feature.py:200; functional.py:69,124,184) and on the attention probabilities
 *       (nn.MultiheadAttention(dropout=...), functional.py:109).  The reference draws its masks from torch's global RNG;
 *       here the keep decision of an element is a pure function of (seed, site, element index) - one 32-bit counter hash per
 *       PAIR of elements, its low / high 16 bits deciding the even / odd one (csrc/kernels_train.h: TDrop), restated by
 *       oracle/rnampnn_oracle.py - so a step is reproducible and testable against autograd.  A call accepts
 *       B*T*k < 2^26 edge rows and B*T < 2^23 residues (32-bit pair indices); larger batches return RNAMPNN_ERR_BAD_ARG.  The
 *       activations the backward needs (the "tape") stay in `workspace`, which must be left untouched until
 *       rnampnn_train_backward has run.  logits (B,T,4) out; *tape_id receives the identity of this tape (ids grow
 *       monotonically per handle, 0 is never issued).  A later forward / loss_and_grad into the SAME workspace destroys the
 *       tape; forwards into different workspaces may be outstanding together (gradient accumulation over micro-batches,
 *       `(loss1 + loss2).backward()`).
 *   rnampnn_train_backward - gradient of every parameter from dlogits (B,T,4) = d loss / d logits of ANY loss the
 *       caller built on the logits (torch autograd: torch.autograd.Function in rnampnn/model/rnampnn.py), for the tape
 *       `tape_id` living in `workspace`; RNAMPNN_ERR_BAD_ARG when that tape has been overwritten or belongs to another
 *       workspace / shape - never a silent backward through another forward's activations.  A tape may be walked more than once
 *       (retain_graph).  accumulate = 0 overwrites `grad`, 1 adds to it.
 *   rnampnn_loss_and_grad  - both in one call around the reference loss: cross_entropy(softmax(logits)[valid], label)
 *       (softmax twice, rnampnn.py:151-154), mean over valid nucleotides.  labels (B,T) int32 class ids (ignored on
 *       padding); loss: device scalar; logits optional; grad overwritten.
 *   Padding: the padded rows of coords follow the rule of RnaMpnnForwardIO.coords; the padded rows of labels and of dlogits are
 *   never read; logits come back with all B*T rows written, zeros on padding; floats of grad that belong to no parameter are 0.
 *   grad: flat f32 buffer of rnampnn_grad_numel() elements; parameter i of rnampnn_weight_info() lies at
 *   rnampnn_weight_offset(i) - one buffer = ONE RCCL all-reduce per step (what Lightning DDP does for the reference,
 *   rnampnn/utils/train.py:106-117).  Every cross-workgroup sum of the backward is an ordered two-stage reduction (no
 *   float atomics): the same inputs give bit-identical gradients. */
size_t  rnampnn_train_workspace_bytes(rnampnn_handle h, int32_t B, int32_t T);
int64_t rnampnn_grad_numel(rnampnn_handle h);
int     rnampnn_weight_offset(rnampnn_handle h, int32_t i, int64_t* offset);
#define RNAMPNN_TRAIN_F32        0  /* exact-f32 GEMMs: the parity-grade path (gradients vs oracle autograd to 2e-3)         */
#define RNAMPNN_TRAIN_BF16_MIXED 1  /* the reference's `bf16-mixed` (rnampnn/utils/train.py:109): GEMM operands bf16 on MFMA, */
                                    /* f32 accumulate; as under autocast, every per-edge activation and its gradient is a bf16 */
                                    /* tensor in HBM (the tape), node-sized tensors and all reductions stay f32                */
int     rnampnn_train_forward(rnampnn_handle h, const float* coords, const float* mask, int32_t B, int32_t T,
                              int32_t T_norm, float dropout, uint64_t seed, int32_t flags, float* logits,
                              void* workspace, size_t workspace_bytes, void* stream, int64_t* tape_id);
int     rnampnn_train_backward(rnampnn_handle h, int64_t tape_id, const float* dlogits, int32_t B, int32_t T, int32_t accumulate,
                               float* grad, void* workspace, size_t workspace_bytes, void* stream);
int     rnampnn_loss_and_grad(rnampnn_handle h, const float* coords, const float* mask, const int32_t* labels,
                              int32_t B, int32_t T, int32_t T_norm, float dropout, uint64_t seed, int32_t flags,
                              float* loss, float* logits, float* grad, void* workspace, size_t workspace_bytes, void* stream);
/* Overlap of the data-parallel gradient all-reduce with the backward (Lightning DDP's bucketed overlap in the
 * reference, rnampnn/utils/train.py:106-117).  The flat gradient is final in three contiguous chunks, in this order:
 * 0 = [post_fusion .. readout], 1 = ResMPNN layers L/2 .. L-1, 2 = the rest (end of the backward).  rnampnn_grad_chunks reports
 * their float ranges (begin[3], end[3]); rnampnn_set_grad_events registers two hipEvent_t (or null) that every later backward
 * records on its stream when chunk 0 / chunk 1 is final: the caller's side stream waits on them and all-reduces that range
 * while the rest of the backward runs. */
int     rnampnn_grad_chunks(rnampnn_handle h, int64_t* begin, int64_t* end);
int     rnampnn_set_grad_events(rnampnn_handle h, void* ev0, void* ev1);
/* hipGraph capture of a training step (the size-independent part of a small-batch step is ~600 launches): with a device seed source set,
 * the training kernels read the dropout seed from *seed_device at kernel time (the `seed` arguments are ignored), so ONE captured
 * rnampnn_loss_and_grad replays with fresh masks after the caller has updated the word.  No reference counterpart (the reference draws
 * from torch's global RNG, which CUDA graphs handle by the same device-side-offset idea).  null restores the argument. */
int     rnampnn_set_seed_source(rnampnn_handle h, const uint64_t* seed_device);
/* Optimiser support (F2).  rnampnn_use_weight_arena: the caller's flat f32 buffer (rnampnn_grad_numel() elements, tensor i
 * at rnampnn_weight_offset(i)) becomes the library's weight storage - the nn.Parameters of the Python module are views
 * of it, so an optimiser step needs no re-upload.  rnampnn_adam_step: torch.optim.Adam (betas, eps, L2 weight decay:
 * rnampnn.py:156-159) as ONE launch over the flat parameter / gradient / moment buffers; `step` counts from 1. */
int     rnampnn_use_weight_arena(rnampnn_handle h, float* arena, void* stream);
int     rnampnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* -- training-set augmentation ----------------------------------------------------------- */
/* Gaussian coordinate noise on a padded batch, on the device (csrc/augment.hip): the role of RNADataset.noise_augmentation
 * (rnampnn/utils/data.py:278-295: stored copies with coordinates + N(0, 1e-2)) and of RNAFeatures(augment_eps) of the rdesign sibling
 * (rdesign/model/feature.py:157-158: X + eps * randn_like(X) on every training forward).  The reference draws from torch's global RNG;
 * here the noise of a value is a pure function of (stream of its row, residue index in the SOURCE RNA, atom, axis), so a noisy copy is a
 * row of the (sigma, key, offset) table and never a stored array.  coords / out (B,T,atoms,3) f32, atoms = 6 or 7; sigma (B) f32,
 * key (B) u64 or null, offset (B) i32 >= 0 or null (= 0): DEVICE arrays, read at kernel time.  For a valid residue t (mask[b,t] != 0) of a
 * row with sigma[b] != 0:
 *     out[b,t,a,x] = coords[b,t,a,x] + sigma[b] * normal01(stream_b, ((offset[b] + t) * atoms + a) * 3 + x)      (one f32 product, one f32 add)
 * with the generator of rnampnn/utils/synth.py restated in f32 (logf, sqrtf, cospif; mix64 = the splitmix64 finaliser, 64-bit wrap-around):
 *     uniform01(s, i) = (mix64(mix64((i + 1) * 0x9E3779B97F4A7C15 + s) ^ (s * 0xD6E8FEB86659FD93)) >> 40) * 2^-24
 *     normal01(s, i)  = sqrt(-2 * log(1 - uniform01(s, 2 i))) * cos(2 pi * uniform01(s, 2 i + 1))
 *     stream_b        = key[b] when key is given, else mix64(mix64(seed) + (b + 1) * 0x9E3779B97F4A7C15)   (seed is ignored with a key)
 * A slice of a noisy copy that starts at residue s of its source passes offset = s and gets that copy's noise.  Padded residues and every
 * row with sigma[b] == 0 are copied bit for bit (-0.0 stays -0.0); a NaN coordinate stays NaN and its neighbours are noised.  out == coords
 * (in place) is allowed; any other overlap is not.  One kernel whose launch depends on (B, T, atoms) only: no runtime fill / copy node, no
 * atomics, no synchronisation, so the call can sit inside a captured training step.  RNAMPNN_ERR_BAD_ARG: atoms outside {6, 7}, B or
 * T <= 0, null coords / mask / sigma / out.  rnampnn/utils/augment.py: noise_reference restates it in numpy (the checker). */
int rnampnn_augment_coords(const float* coords, const float* mask, int32_t B, int32_t T, int32_t atoms,
                           const float* sigma      /* (B) */,
                           const uint64_t* key     /* (B) or null */,
                           const int32_t* offset   /* (B) or null = 0 */,
                           uint64_t seed, float* out, void* stream);

/* -- measurement ------------------------------------------------------------------------- */
/* Live timing of the dominant kernel (the fused ResMPNN edge kernel, mpnn.py:154-265): when
 * enabled, HIP events bracket its launches on the caller's stream - every `enable`-th launch (1 = all; an event
 * pair costs ~12 us of stream idle, so a timed production loop samples, e.g. 7 against the 10 launches of a forward);
 * _read synchronises the recorded events and returns the summed duration and the number of TIMED launches since the
 * last reset.
 * No reference counterpart (the reference has no profiling hooks). */
int rnampnn_profile_enable(rnampnn_handle h, int32_t enable);
int rnampnn_profile_read(rnampnn_handle h, double* kernel_ms, int64_t* launches, int32_t reset);
/* The same split by launch kind: index 0 = launches that run the edge update of layer l AND the message of layer l + 1 (L - 1 per forward),
 * index 1 = the other fused launches (the message-only launch of layer 1, an edge-only launch of a tap). */
int rnampnn_profile_read_kinds(rnampnn_handle h, double* kernel_ms2, int64_t* launches2, int32_t reset);

const char* rnampnn_last_error(void);
const char* rnampnn_version(void);

/* Test tap of the 90 raw edge features of ResFeature (rnampnn/model/feature.py:386-517: `_cross_dists` 49, `_cross_angles` 25,
 * `_cross_dihedrals` 16) - the tensor the inference kernels keep in registers.  feats (B,T,k,96) f32: columns 90..95, padded residues and
 * absent neighbour slots are zero (the reference holds 1e6 distances there); edge_index (B,T,k) i64 optional. */
size_t rnampnn_edge_raw_workspace_bytes(rnampnn_handle h, int32_t B, int32_t T);
int rnampnn_edge_raw_features(rnampnn_handle h, const float* coords, const float* mask, int32_t B, int32_t T, int64_t* edge_index,
                              float* feats, void* ws, size_t ws_bytes, void* stream);

/* ---- Gradient-boosted-tree read-out (PARITY UNPINNED: xgboost is not installed, no fitted model ships).
 * Replaces `self.xgb_readout.predict(embedding)` (rnampnn/model/rnampnn.py:136-145,297-298) for a fitted `multi:softmax` gbtree model
 * given as the arrays of XGBoost's JSON model format (`learner.gradient_booster.model.trees[*].{left_children,right_children,
 * split_indices,split_conditions,default_left}` concatenated over the trees, `tree_info` = class of each tree).  Host arrays, copied.
 * Rule: at an internal node go left iff x[split_index] < split_condition (NaN: default_left); a leaf adds split_conditions[leaf] to the
 * margin of its tree's class; prediction = first argmax of the margins.  X (n_rows, ldx >= num_feature) f32 device, outputs device. */
typedef struct rnampnn_gbdt* rnampnn_gbdt_handle;
int rnampnn_gbdt_create(int32_t num_trees, int32_t num_class, int32_t num_feature, float base_score, const int32_t* tree_offsets,
                        const int32_t* tree_class, const int32_t* left_children, const int32_t* right_children,
                        const int32_t* split_indices, const float* split_conditions, const uint8_t* default_left,
                        rnampnn_gbdt_handle* out);
int rnampnn_gbdt_destroy(rnampnn_gbdt_handle g);
int rnampnn_gbdt_predict(rnampnn_gbdt_handle g, const float* X, int32_t n_rows, int32_t ldx, float* margin /* (n_rows,num_class) or null */,
                         int32_t* argmax_out /* (n_rows) or null */, void* stream);
const char* rnampnn_gbdt_last_error(void);

/* ---- Fitting that read-out on the device (PARITY UNPINNED as above: XGBoost's published multi:softmax gradient /
 * hessian, split gain and leaf weight are restated, the cuts, the binning and the sampling are this library's own).
 * Histogram method: X is binned once into uint8 with per-feature cuts, gradients are quantised onto the grid 2^-20 and summed as integers,
 * the split search is fp64, trees grow level by level to max_depth; the result is bit-reproducible for one seed and independent of ldx.
 * `cuts` (num_feature, 255) f32 and `n_cuts` (num_feature) i32 are DEVICE arrays the caller prepares (the library holds no sort): per
 * feature the ascending distinct values v[floor(i * n_rows / max_bin)], i = 1 .. max_bin - 1, of the sorted column v, without any equal
 * to v[0]; bin(x) = number of cuts <= x, and a split at cut j (bin <= j goes left) carries split_condition = cuts[j].
 * Sampling: row i takes part in round r iff u(seed, 2r, i) < subsample; tree t = r * num_class + c keeps the
 * max(1, floor(colsample_bytree * num_feature)) features of smallest u(seed, 2t + 1, f), ties to the lower index (u: DESIGN section 9).
 * X (n_rows, ldx >= num_feature) f32 and y (n_rows) i32 in [0, num_class) are device arrays; a non-finite X or a label out of range is
 * RNAMPNN_ERR_BAD_ARG, found by the one check that precedes the fit.  All work is enqueued on `stream`; the call synchronises it twice
 * (after that check, and at the end to learn the model's size).  The handle is the evaluator's: rnampnn_gbdt_predict / _destroy take it. */
typedef struct rnampnn_gbdt_params {
    int32_t num_class, n_estimators, max_depth /* 1..10 */, max_bin /* 2..256 */;
    double learning_rate, subsample, colsample_bytree, reg_lambda, gamma, min_child_weight, base_score;
    uint64_t seed;
} rnampnn_gbdt_params;
int rnampnn_gbdt_fit(const rnampnn_gbdt_params* params, const float* X, int32_t n_rows, int32_t ldx, int32_t num_feature, const int32_t* y,
                     const float* cuts, const int32_t* n_cuts, void* stream, rnampnn_gbdt_handle* out);
/* A model leaves the process as the arrays rnampnn_gbdt_create reads.  Every pointer may be null: call once for the sizes
 * (tree_offsets holds num_trees + 1 entries, tree_class num_trees, the five node arrays total_nodes), then with host buffers. */
int rnampnn_gbdt_export(rnampnn_gbdt_handle g, int32_t* num_trees, int32_t* total_nodes, int32_t* num_class, int32_t* num_feature,
                        float* base_score, int32_t* tree_offsets, int32_t* tree_class, int32_t* left_children, int32_t* right_children,
                        int32_t* split_indices, float* split_conditions, uint8_t* default_left);
/* Stage taps of the fit.  _bin: X, cuts -> bins (n_rows, num_feature) u8, device, on `stream`.
 * _grow_tree: ONE tree from integer gradients g, h (n_rows) i32 on the grid 2^-20 over the rows with row_mask != 0 and the features with
 * feat_mask != 0 (device bytes, null = all); uses max_depth, learning_rate, reg_lambda, gamma, min_child_weight of `params`.  The tree
 * comes back in HOST arrays of capacity 2^(max_depth + 1) - 1, nodes numbered breadth-first, leaves with left = right = -1 and their
 * value in split_conditions; the call synchronises `stream`. */
int rnampnn_gbdt_bin(const float* X, int32_t n_rows, int32_t ldx, int32_t num_feature, const float* cuts, const int32_t* n_cuts,
                     uint8_t* bins, void* stream);
int rnampnn_gbdt_grow_tree(const rnampnn_gbdt_params* params, const uint8_t* bins, int32_t n_rows, int32_t num_feature, const float* cuts,
                           const int32_t* n_cuts, const int32_t* g, const int32_t* h, const uint8_t* row_mask, const uint8_t* feat_mask,
                           int32_t* left_children, int32_t* right_children, int32_t* split_indices, float* split_conditions,
                           int32_t* n_nodes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RNAMPNN_HIP_H */
