/*
 * rdesign_hip.h - C ABI of the MI355X path of the reference's sibling model `rdesign`,
 * exported by the same librnampnn_hip.so as rnampnn_hip.h.
 *
 * The reference boundary is the Python module surface of `rdesign.model` (the model `main.py:24-31` and
 * `train.py:67-80` of the reference run today).  Every entry point names the reference interface it replaces;
 * `rna-mpnn_amd/rdesign/model/rdesign.py` binds these symbols with ctypes and re-exposes the reference's names.
 *
 * PARITY: the eval-mode forward, the graph, the raw features and the p = 0 gradients are pinned to the reference's own
 * `RNAFeatures` / `MPNNLayer` / `Readout` through `tests/golden/rdesign_*.npz` (tools/gen_golden_rdesign.py,
 * tests/test_rdesign_golden_{cpu,gpu}.py); the CPU restatement `oracle/rdesign_oracle.py` is pinned to the same fixtures.
 * Not pinned: dropout masks (torch's RNG), the xgboost branch of `predict`, the Lightning plumbing.
 *
 * Inference (rdesign_forward / rdesign_readout, f32 or bf16), the exact-f32 training step (rdesign_loss_and_grad), the opt-in
 * bf16-mixed training step (rdesign_loss_and_grad_ex with RDESIGN_TRAIN_BF16_MIXED) and the per-RNA validation metrics on the device
 * (rdesign_score: what the epoch trainer's `validate` and `RNAModel.score_batch` / `predict_sequences` run after one forward).
 *
 * Conventions: as rnampnn_hip.h (device pointers, caller's stream, no synchronisation, 0 = success).
 *   X (B,T,6,3) f32 backbone atoms P, O5', C5', C4', C3', O3' (rdesign/utils/data.py:90-115, zero-filled padding),
 *   mask (B,T) f32 0/1 prefix masks.  Padded rows of X and labels are never read: "zero-filled padding" says what the result
 *   equals (the reference's, which does read those zeros), it is no precondition - the rows may hold anything, NaN included.
 *   A workspace may hold anything on entry.  Outputs are PACKED: the reference drops padded residues
 *   (feature.py:206 `mask_select`), row p = (number of valid residues of RNAs < b) + t, N = mask.sum().
 */
#ifndef RDESIGN_HIP_H
#define RDESIGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDESIGN_OK               0
#define RDESIGN_ERR_BAD_ARG      1
#define RDESIGN_ERR_UNSUPPORTED  2
#define RDESIGN_ERR_WORKSPACE    5
#define RDESIGN_ERR_WEIGHTS      6
#define RDESIGN_ERR_HIP          7

#define RDESIGN_PREC_F32  0   /* exact-f32 GEMMs                                                              */
#define RDESIGN_PREC_BF16 1   /* bf16 MFMA operands, f32 accumulate (the embeddings' 101/115-wide GEMMs stay f32) */

typedef struct rdesign_ctx* rdesign_handle;

/* Hyper-parameters of RNAModel.__init__ (rdesign/model/rdesign.py:19-50). */
typedef struct RDesignConfig {
    int32_t hidden_dim;           /* must be 128 */
    int32_t k_neighbors;          /* 1..64 (reference default 25) */
    int32_t num_mpnn_layers;      /* reference default 9 */
    int32_t num_message_layers;   /* Linears of MPNNLayer.message_layers (mpnn.py:13-19), default 3 */
    int32_t num_dense_layers;     /* hidden Linears of MPNNLayer.dense (mpnn.py:21-29), default 3 */
    int32_t dim_dense_layers;     /* default 256 */
    int32_t num_readout_layers;   /* Readout (functional.py:98-121): num_layers - 1 hidden Linears + the 4-way Linear; default 0 */
    int32_t readout_hidden_dim;   /* default 256 */
    int32_t precision;            /* RDESIGN_PREC_* */
} RDesignConfig;

/* RNAModel.__init__ (rdesign.py:19-64): validates the configuration and builds the parameter table. */
int rdesign_create(const RDesignConfig* cfg, rdesign_handle* out);
int rdesign_destroy(rdesign_handle h);
const char* rdesign_last_error(void);

/* state_dict() surface (the keys of RNAModel.state_dict(), registration order): key, element count and the offset
 * (in floats) of the tensor inside the flat parameter arena. */
int rdesign_num_weights(rdesign_handle h);
int rdesign_weight_info(rdesign_handle h, int32_t index, const char** key, int64_t* numel, int64_t* offset);
int64_t rdesign_param_numel(rdesign_handle h);
/* load_state_dict(): the caller owns ONE flat f32 device buffer of rdesign_param_numel() floats (16-byte aligned)
 * whose slices are the parameters (torch Parameters are views of it); the library reads it in place. */
int rdesign_use_weight_arena(rdesign_handle h, float* arena, void* stream);
/* derive the kernel-side weight images after the arena changed (optimizer step, load_state_dict). */
int rdesign_finalize_weights(rdesign_handle h, void* stream);

size_t rdesign_workspace_bytes(rdesign_handle h, int32_t B, int32_t T);

/* RNAModel.forward (rdesign.py:82-88) followed by Readout (rdesign.py:104): every output is optional (null = skipped).
 *   h_V      (B*T,128) packed node embeddings after the MPNN stack (rows >= N untouched)
 *   logits   (B*T,4)   packed read-out logits (rows >= N untouched)
 *   edge_index (B,T,k) i64: neighbour position inside the RNA per slot, -1 for padded residues and for the slots
 *            beyond the RNA's length (the edges the reference's `mask_attend` filter removes, feature.py:186-194)
 *   node_raw (B*T,101) / edge_raw (B*T*k,115): raw geometric features (feature.py:221-236), test taps; rows >= N / >= N*k untouched,
 *            the slots of edge_raw that edge_index marks -1 are zero */
int rdesign_forward(rdesign_handle h, const float* X, const float* mask, int32_t B, int32_t T, float* h_V, float* logits,
                    int64_t* edge_index, float* node_raw, float* edge_raw, void* ws, size_t ws_bytes, void* stream);

/* Readout.forward (functional.py:123-126) on n_rows caller rows of 128 floats -> logits (n_rows,4).
 * Workspace: rdesign_readout_workspace_bytes(h, n_rows) (node-sized buffers only). */
size_t rdesign_readout_workspace_bytes(rdesign_handle h, int32_t n_rows);
int rdesign_readout(rdesign_handle h, const float* h_V, int32_t n_rows, float* logits, void* ws, size_t ws_bytes, void* stream);

/* Exact-f32 training step: `training_step` + `loss.backward()` of the reference (rdesign.py:95-104) in ONE call - taped forward with
 * dropout after every GELU the reference follows with nn.Dropout, loss = CrossEntropyLoss()(readout(h_V), S) over the valid residues
 * (one softmax, mean over N) and the gradient of every parameter.  RDESIGN_PREC_F32 handles only (the reference's rdesign trainer runs
 * Lightning's 32-bit default): a RDESIGN_PREC_BF16 handle gets RDESIGN_ERR_UNSUPPORTED (the two size queries return 0 and set the error text).
 *   labels   (B,T) i32 class ids 0..3, padding ignored
 *   dropout  in [0,1); the keep masks are a pure function of (seed, site, element) - csrc/rdesign_train.hip states the addressing
 *   loss     device scalar;  logits optional, packed (B*T,4), rows >= N untouched
 *   grad     rdesign_param_numel() floats laid out like the weight arena (rdesign_weight_info offsets), OVERWRITTEN; padding floats are zero
 * Bit-reproducible (no float atomics); rows are bounded by the 32-bit pair index of the dropout hash: B*T*k < 2^26, else RDESIGN_ERR_BAD_ARG.
 * rdesign_train_tape_bytes: the part of the workspace that holds the tape (a figure for reports).
 * RNAFeatures(augment_eps) (feature.py:157-158: X + eps * randn_like(X) on a training forward) is not part of this call: the step reads X
 * as given.  RNAModel(augment_eps) noises X ahead of it with rnampnn_augment_coords (include/rnampnn_hip.h: atoms = 6, sigma = eps for every
 * row, no keys, seed = this call's seed), as do the noisy copies of a training set (rnampnn/utils/augment.py). */
size_t rdesign_train_workspace_bytes(rdesign_handle h, int32_t B, int32_t T);
size_t rdesign_train_tape_bytes(rdesign_handle h, int32_t B, int32_t T);
int rdesign_loss_and_grad(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T,
                          float dropout, uint64_t seed, float* loss, float* logits, float* grad, void* ws, size_t ws_bytes, void* stream);

/* The training step with its arithmetic chosen per call.  flags = RDESIGN_TRAIN_F32: exactly the three entry points above (a
 * RDESIGN_PREC_BF16 handle is refused).  flags = RDESIGN_TRAIN_BF16_MIXED: the same step - same dropout sites and addressing, same loss,
 * same gradient layout, bit-reproducible - with every per-edge tensor stored as bf16 and the GEMMs on the MFMA kernels of the main model's
 * bf16-mixed trainer (f32 accumulate; node-level tensors and every reduction stay f32; csrc/rdesign_train_bf16.hip states the tape).  It
 * reads the nn.Linear-layout weights of the arena and accepts a handle of either precision; it is built for num_message_layers 2 and 3,
 * any other depth gets RDESIGN_ERR_UNSUPPORTED (size queries: 0 and the error text), as does a configuration an MFMA edge kernel does not
 * cover.  The row limits are those of rdesign_loss_and_grad.  Any other flags value: RDESIGN_ERR_BAD_ARG (size queries: 0). */
#define RDESIGN_TRAIN_F32        0
#define RDESIGN_TRAIN_BF16_MIXED 1
size_t rdesign_train_workspace_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags);
size_t rdesign_train_tape_bytes_ex(rdesign_handle h, int32_t B, int32_t T, int32_t flags);
int rdesign_loss_and_grad_ex(rdesign_handle h, const float* X, const float* mask, const int32_t* labels, int32_t B, int32_t T,
                             float dropout, uint64_t seed, int32_t flags, float* loss, float* logits, float* grad, void* ws,
                             size_t ws_bytes, void* stream);

/* The metrics of validation_step / test_step (rdesign.py:106-141) per RNA, on the device: argmax against the labels, and the cross-entropy.
 * Exactly one of
 *   logits   (n_rows,4) f32 packed as rdesign_forward writes them (16-byte aligned), or
 *   pred     (n_rows) i32 packed class ids (the tree read-out's route)
 * is non-null; n_rows = rows the packed buffers hold (>= mask.sum(); rows beyond it are never touched).
 *   mask (B,T) f32 prefix masks, labels (B,T) i32 in the padded layout of the training step (padding ignored)
 *   correct (B) i32, valid (B) i32: matches and length per RNA (an RNA of length 0 gives 0 / 0 / 0)
 *   nll     (B) f32, optional, logits only (non-null with pred: RDESIGN_ERR_BAD_ARG): per-RNA SUM of logsumexp(x) - x[label]
 *   pred_out (n_rows) i32, optional: the packed argmax (ties to the lowest class, as numpy.argmax) / a copy of pred
 * Both or neither of logits / pred, B <= 0 or T <= 0: RDESIGN_ERR_BAD_ARG.  Needs no handle.  Fixed-order reductions without atomics (two
 * calls give identical bytes), no runtime memset / memcpy, no synchronisation.  ws: rdesign_score_workspace_bytes(B), 16-byte aligned. */
size_t rdesign_score_workspace_bytes(int32_t B);
int rdesign_score(const float* logits, const int32_t* pred, int32_t n_rows, const float* mask, const int32_t* labels, int32_t B, int32_t T,
                  int32_t* correct, int32_t* valid, float* nll, int32_t* pred_out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
