/* abnet3_hip.h -- C ABI of libabnet3_hip.so, the MI355X (gfx950) implementation
 * of bootphon/abnet3's Siamese training hot path.
 *
 * The reference has no FFI, plugin registry or native code: its boundary for
 * this path is Python duck-typing (abnet3/gridsearch.py:145-202 builds the
 * objects by class name).  This header is therefore NEW: it is what a
 * maintainer of the reference would bind with ctypes to replace the torch op
 * sequences cited per function below (citations are file:line relative to the
 * reference checkout).  INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch / C++ types.
 *  - Every pointer named in a signature is a DEVICE pointer unless the comment
 *    says "host".  The caller owns all buffers; the library never allocates device
 *    memory, frees or synchronises (graph-capturable).  Process state it keeps: a
 *    thread-local error string, per-kernel "attribute already set" flags (dynamic LDS
 *    opt-in, set once per device), and the A/B switches it reads from the environment ONCE,
 *    when the library is loaded (ABN_PLANES, ABN_FUSED, ABN_FUSED_MIN_ROWS, ABN_BN_PLANES,
 *    ABN_WGRAD_XCD, ABN_BF16X3_PLANES, ABN_GEMM_TILE, ABN_BWD_PAIR, ABN_DTW_F40, ABN_DTW_PC:
 *    kernel choice only, never results beyond fp32 summation order; no call reads the
 *    environment, and none of them makes a call do less than its contract).  No streams, no events.
 *  - Row-major contiguous fp32 tensors; sizes are int64_t; `stream` is a
 *    hipStream_t passed as void* (NULL = the null stream).
 *  - Return value: 0 = ok, negative = error (ABN_E_*); abn_last_error() gives
 *    the message.  Nothing throws across the ABI.
 */
#ifndef ABNET3_HIP_H
#define ABNET3_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABN_ABI_VERSION 20
#define ABN_MAX_LAYERS 16

enum { ABN_OK = 0, ABN_E_ARG = -1, ABN_E_LAUNCH = -2, ABN_E_WORKSPACE = -3,
       ABN_E_UNSUPPORTED = -4 };

/* activation_functions table, abnet3/model.py:19-23.  'softmax' (last_non_linearity only,
 * model.py:161-166) is not an epilogue: the tower ends with ABN_ACT_NONE and abn_softmax_rows follows.
 * ABN_ACT_SOFTMAX is no tower activation either (abn_tower_desc takes 0-3): only abn_pair_loss_dz with
 * ABN_LOSS_KL takes it, meaning "e1 / e2 are the softmax's inputs" (added within ABI 20, backward compatible). */
enum { ABN_ACT_NONE = 0, ABN_ACT_SIGMOID = 1, ABN_ACT_RELU = 2, ABN_ACT_TANH = 3, ABN_ACT_SOFTMAX = 4 };

/* abnet3/loss.py:37 (coscos2), :70 (cosmargin), :108 (KLLoss; added within ABI 20: abn_pair_loss,
 * abn_pair_loss_padded and abn_pair_loss_dz take it, abn_tower_backward_loss answers ABN_E_UNSUPPORTED) */
enum { ABN_LOSS_COSCOS2 = 0, ABN_LOSS_COSMARGIN = 1, ABN_LOSS_KL = 2 };

/* label element types accepted by the pair loss: the reference compares with
 * torch.eq(y, 1) / torch.eq(y, -1) on whatever dtype arrives (int64 in
 * test/test_loss.py:28, float64 from abnet3/dataloader.py:206,231) */
enum { ABN_Y_I8 = 0, ABN_Y_I32 = 1, ABN_Y_I64 = 2, ABN_Y_F32 = 3, ABN_Y_F64 = 4 };

/* optimizer_type, abnet3/trainer.py:68-87 (torch.optim defaults otherwise) */
enum { ABN_OPT_SGD = 0, ABN_OPT_ADADELTA = 1, ABN_OPT_ADAM = 2,
       ABN_OPT_ADAGRAD = 3, ABN_OPT_RMSPROP = 4 };

/* abn_tower_desc.precision: arithmetic of the tower GEMMs (see the field's comment) */
enum { ABN_PREC_F32 = 0, ABN_PREC_BF16 = 1, ABN_PREC_BF16X3 = 2, ABN_PREC_F16X2 = 3 };

/* abn_tower_desc.bn_sync_fn: SUM-all-reduces n float64 values at a DEVICE pointer in place over the replicas, in the
 * stream's order (torch.distributed.all_reduce / ncclAllReduce on that stream); returns 0 on success. */
typedef int (*abn_allreduce_fn)(void* ctx, void* device_doubles, int64_t n, void* stream);

int abn_abi_version(void);
const char* abn_last_error(void);          /* host string, thread-local */

/* One SiameseNetwork tower (abnet3/model.py:110-170): n_layers Linear layers
 * dims[0] -> dims[1] -> ... -> dims[n_layers], each followed by Dropout (caller-
 * drawn masks, see drop_mask), optional BatchNorm1d, and an activation (`act`, or `last_act` for
 * the output layer, model.py:161-166).  W[l] is [dims[l+1], dims[l]] row-major
 * exactly as nn.Linear stores it; gradients are written to dW/db/dbn_* (same
 * shapes).  All pointers are device pointers held in this HOST struct. */
typedef struct abn_tower_desc {
    int32_t n_layers;
    int32_t act;
    int32_t last_act;
    int32_t batch_norm;
    int64_t dims[ABN_MAX_LAYERS + 1];
    const float* W[ABN_MAX_LAYERS];
    const float* b[ABN_MAX_LAYERS];
    const float* bn_w[ABN_MAX_LAYERS];     /* gamma; NULL when !batch_norm */
    const float* bn_b[ABN_MAX_LAYERS];     /* beta */
    float* bn_rm[ABN_MAX_LAYERS];          /* running_mean (updated in train) */
    float* bn_rv[ABN_MAX_LAYERS];          /* running_var */
    float* dW[ABN_MAX_LAYERS];             /* backward outputs; may be NULL   */
    float* db[ABN_MAX_LAYERS];             /* when only forward is called     */
    float* dbn_w[ABN_MAX_LAYERS];
    float* dbn_b[ABN_MAX_LAYERS];
    /* nn.Dropout(p) between Linear and BatchNorm/activation (model.py:137,148,157):
     * per layer a [rows, dims[l+1]] multiplier (0 or 1/(1-p)) drawn by the caller;
     * NULL = identity (p = 0 or eval mode).  The same masks must be passed to
     * the backward call. */
    const float* drop_mask[ABN_MAX_LAYERS];
    /* 0 = fp32 on the exact-fp32 MFMA (the parity path, default); 1 = throughput mode:
     * matrix operands rounded to bf16 at fragment time, fp32 accumulation, everything
     * else (storage, BatchNorm, loss, optimizer) still fp32.  NOT within the 1e-5 bar.
     * 2 = bf16 x 3: every operand split into three bf16 terms, six bf16 MFMAs per product
     * block: fp32-grade results (as close to a float64 evaluation as mode 0 is) that are not
     * bit-identical to mode 0.
     * 3 = fp16 x 2 (the Python classes' default): every operand scaled by a power of two (per operand row /
     * 32-row weight block) and split into two fp16 terms (22 significant bits), three fp16 MFMAs per product
     * block, the scales taken out again in the epilogue (exactly): the same grade at half the MFMAs and two
     * thirds of the operand stream.  On the operand-plane kernels only; where a call falls back to the GEMM
     * kernels it runs as mode 2. */
    int32_t precision;
    /* backward only: d_out already IS d loss / d z of the output layer (abn_pair_loss_dz), so
     * the activation derivative / dropout step in front of the last layer's GEMMs is skipped.
     * Not with batch_norm (its backward needs d loss / d a). */
    int32_t d_out_is_dz;
    /* backward only: leave the weight gradients as unreduced split-K slabs in `scratch`; the
     * caller finishes with abn_tower_reduce_step (reduction + optimizer step in one launch;
     * BatchNorm's gamma / beta gradients are final either way). */
    int32_t defer_reduce;
    /* Optional persistent image of the weights as MFMA operand fragments (the split arithmetics, precision 1-3):
     * wpack = abn_tower_wpack_floats() floats owned by the caller, zero before the first use, or
     * NULL (the forward then builds the image inside its workspace every call).  wpack_valid != 0:
     * the caller vouches that the image matches W as it stands -- it does after a forward that
     * was given the buffer with wpack_valid = 0 (which rebuilds it: ~6 us) until anything writes
     * to W (abn_optimizer_step and abn_tower_reduce_step included).  What it buys: repeated
     * forwards with unchanged weights (embedding extraction) skip the rebuild.  (Keeping the image
     * in step inside abn_tower_reduce_step was measured: the transposed half is 2-byte scattered
     * stores, +10 us on that launch against the 6 us saved.) */
    int32_t wpack_valid;
    /* forward only: no backward will follow this forward (inference): it may skip whatever it
     * would store for one (the default arithmetic writes more than half of its bytes for the
     * backward).  A backward after such a forward reads garbage. */
    int32_t forward_only;
    /* backward only, data-parallel overlap (operand-plane launches without BatchNorm; ABN_E_UNSUPPORTED elsewhere):
     * the backward in two calls on the same workspace and scratch so that the caller can start the all-reduce of the
     * upper layers' gradients while the lower layers' are still being computed.  0 = everything (default);
     * 1 = the data-gradient launches and the weight gradients (with their slab reduction) of layers >= wgrad_split;
     * 2 = the weight gradients (and reduction) of layers < wgrad_split -- after a part-1 call (d_out is not read and may be
     * NULL), no defer_reduce. */
    int32_t wgrad_part;
    void* wpack;
    /* Dropout drawn inside the kernels instead of read from drop_mask (the split arithmetics only;
     * where drop_mask[l] is given it wins): drop_seed = device pointer to one uint64 the caller
     * draws per forward (NULL: off), drop_p = nn.Dropout's p.  The multiplier of element
     * (layer, row, feature) is a hash of (seed, layer, row, feature): 0 with probability p
     * (to 2^-16), else 1 / (1 - p) -- the backward, given the same descriptor fields, regenerates
     * it.  A forward / backward that cannot run on the operand-plane kernels
     * (abn_tower_uses_planes) returns ABN_E_UNSUPPORTED when only a seed is given. */
    const void* drop_seed;
    float drop_p;
    int32_t reserved2_;
    /* Cross-replica BatchNorm statistics (data-parallel training; SURVEY.md 8e's exact mode): bn_sync_fn != NULL with bn_sync_world >= 1
     * (a group of ONE replica is a group: its reduction is the identity, the launches are the group's)
     * makes a TRAINING forward / backward of a BatchNorm tower sum its per-call statistics -- [sum z, sum z^2] per
     * layer in the forward, [sum dy, sum dy xhat] in the backward, float64 -- over the replicas through bn_sync_fn
     * (called on the host between two launches, once per layer and direction) and normalise with the replicas' row
     * count, which travels with the forward's sums (n_calls more values: the replicas' batches may differ in size):
     * R replicas on B_r rows each then step like one process on sum B_r rows.  EVERY replica of the group must make the
     * same calls (the exchange is a collective: the caller agrees beforehand which steps take this path).
     * bn_sync_fn NULL or bn_sync_world 0: per-replica statistics.  Operand-plane launches only (ABN_E_UNSUPPORTED otherwise). */
    int32_t bn_sync_world;
    int32_t wgrad_split;                   /* see wgrad_part */
    abn_allreduce_fn bn_sync_fn;
    void* bn_sync_ctx;
    /* A PADDED batch through a BatchNorm tower in training (device int32, or NULL: every row is real): only the first
     * *n_valid rows of EVERY forward_once call are real (abn_gather_pairs writes such batches: zero rows behind the real
     * ones, tower 2 starting at row rows / n_calls).  The batch statistics, the running statistics' update and the backward
     * then span the real rows only and the padded rows get no gradient and give none, so that one captured step serves
     * every batch size of a bucket (see abn_tower_backward_loss's n_valid: the same pointer).  The forward and the
     * backward of a step must be given the same value.  Only on the BatchNorm layer launches (abn_tower_path =
     * ABN_PATH_BN_LAYERS) with per-replica statistics: ABN_E_UNSUPPORTED elsewhere.  Towers without BatchNorm and
     * inference forwards ignore it (their rows do not see each other). */
    const int32_t* n_valid;
    /* BatchNorm1d.num_batches_tracked of every layer (device int64 each, or NULL): a TRAINING forward of a batch_norm tower
     * adds n_calls to each -- torch's BatchNorm1d counts its training calls, and the reference's forward runs forward_once
     * twice (abnet3/model.py:194-195) -- inside the forward's own launches where it can (ABN_PATH_BN_TOWER), else in one
     * small launch behind them.  Nothing else reads them (momentum is the fixed 0.1). */
    void* bn_nbt[ABN_MAX_LAYERS];
    /* Optional sync buffer of the resident BatchNorm tower (ABN_PATH_BN_TOWER): abn_tower_sync_ws_bytes() bytes, 16-byte
     * aligned, owned by the caller, ZERO before its first use and never written by the caller afterwards; one per tower
     * and stream (the forward and the backward of a step share it; two streams driving one tower need two).  It holds the
     * launch counter the kernels' hand-over tags derive from and the hand-over granules themselves.  NULL: BatchNorm
     * training runs one launch per layer (ABN_PATH_BN_LAYERS).  Should a launch ever give up on a hand-over (the grid was
     * not resident: the outputs then read NaN) the buffer's failure word stays set: zero the buffer again.  While it is
     * set abn_tower_reduce_step drops its step (parameters, state and gradients untouched), and a backward WITHOUT
     * defer_reduce (the data-parallel step: the caller all-reduces the gradient next) writes a ZERO gradient. */
    void* sync_ws;
    /* Optional, backward with defer_reduce only (ABI v19): the workspace of the forward whose gradients are pending (the
     * `ws` both calls were given) and that forward's n_calls, lent to abn_tower_reduce_step.  Small batches on the
     * layer-per-launch kernels (ABN_PATH_WIDE, fp16 x 2) then skip the split-K weight-gradient launch in the backward:
     * abn_tower_reduce_step computes every layer's weight gradient over ALL rows and applies the optimizer's rule in ONE
     * launch (csrc/tower_wgrad_step.h: a workgroup per 64 x 64 tile of [dW | db], no slabs).  The workspace must stay
     * untouched until that call.  NULL: weight gradients as slabs in the backward, their sum in abn_tower_reduce_step. */
    const float* fwd_ws;
    int64_t fwd_calls;
    /* Optional (ABI v19): the step reads its batch from a PLAN of the whole pass instead of from x1 / x2 / y -- see
     * abn_step_source below.  Layer-per-launch kernels (ABN_PATH_WIDE) in training, two forward_once calls, the pair loss
     * inside the backward (abn_tower_backward_loss); ABN_E_UNSUPPORTED elsewhere. */
    const struct abn_step_source* source;
} abn_tower_desc;

/* A pass's batches as the trainer's batch plan holds them (abnet3/dataloader.py:166-261: every batch = the frame pairs of
 * some word pairs, in the order the reference's iterator yields them): pair p of the plan aligns row idx1[p] of `table`
 * (tower 1) with row idx2[p] (tower 2) under label labels[p]; step s of the pass takes pairs [steps[2 s], steps[2 s] +
 * steps[2 s + 1]).  With abn_tower_desc.source set, a training step needs NO gather launch and no per-step argument: the
 * first layer's launch stages its 32 rows straight from the table (rows behind the step's last pair: zero rows, as
 * abn_gather_pairs pads them), the pair loss reads its labels and its real-pair count from here, and the step's last launch
 * (abn_tower_reduce_step) advances *step_ctr -- a captured hipGraph replays unchanged for every batch of its size.
 * x1 / x2 still name the (unused) input buffers of the padded size: rows = 2 x the padded pair count as before.
 * All arrays on the device; the struct itself is host memory read during the calls. */
typedef struct abn_step_source {
    const float* table;            /* [table_rows, dims[0]] */
    int64_t table_rows;
    const int64_t* idx1;
    const int64_t* idx2;
    const void* labels;            /* dtype: abn_tower_backward_loss's y_dtype (its y argument is ignored) */
    const int64_t* steps;          /* [n_steps][2]: first pair, pairs */
    int32_t* step_ctr;             /* the step being run; += 1 by abn_tower_reduce_step */
} abn_step_source;

/* A ready-made abn_allreduce_fn for abn_tower_desc.bn_sync_fn over RCCL, so that no host language stands between
 * two launches of a data-parallel BatchNorm step: ctx = an abn_rccl_ctx the caller fills once -- `comm` its ncclComm_t,
 * `all_reduce` the address of RCCL's ncclAllReduce (the library does not link RCCL: the caller already has it loaded,
 * e.g. torch's librccl.so) -- and the function issues ncclAllReduce(buf, buf, n, ncclFloat64, ncclSum, comm, stream)
 * in place on the launch stream.  Returns 0, or 1 when RCCL reports an error. */
typedef struct abn_rccl_ctx {
    void* comm;
    void* all_reduce;       /* ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) */
    int64_t calls;          /* counts the all-reduces issued through this context (the caller's to read and reset) */
} abn_rccl_ctx;
int abn_rccl_allreduce_f64(void* ctx, void* device_doubles, int64_t n, void* stream);

/* Workspace of one forward call (what the backward needs: the saved activations, for the
 * default arithmetic also the weights as MFMA operand fragments; its layout is the library's
 * own and depends on the descriptor), in floats, and the offset inside it of the
 * [rows, dims[n_layers]] output embedding -- the only public position in it. */
int64_t abn_tower_ws_floats(const abn_tower_desc* t, int64_t rows, int64_t n_calls);
int64_t abn_tower_out_offset(const abn_tower_desc* t, int64_t rows, int64_t n_calls);
/* Scratch of one backward call (split-K slabs + the dZ of every layer), in floats. */
int64_t abn_tower_bwd_scratch_floats(const abn_tower_desc* t, int64_t rows);
/* Size of the optional abn_tower_desc.sync_ws buffer, in bytes (host function, no device call). */
int64_t abn_tower_sync_ws_bytes(void);
/* Size of the optional abn_tower_desc.wpack buffer, in floats (0: this tower has no such image). */
int64_t abn_tower_wpack_floats(const abn_tower_desc* t);
/* 1 when abn_tower_forward(train) / the backward after it with these arguments run on the
 * operand-plane kernels (the ones that read, and with wpack_valid = 0 rebuild, wpack), 0 when on
 * the per-layer GEMMs, < 0 on a bad descriptor.  Depends on the descriptor, the row count, pointer
 * alignment and the library's environment switches.  train = 0 asks about the inference forward:
 * a batch_norm tower takes the operand-plane kernel there (forward_only descriptors: running
 * statistics folded into the epilogue), and only there. */
int abn_tower_uses_planes(const abn_tower_desc* t, int64_t rows, const float* x1, const float* x2,
                          const float* ws, int train);

/* Which kernel family a call takes, and the arithmetic its GEMMs compute in -- a PURE function of
 * the arguments and the environment switches (the library keeps no record of past calls):
 * backward = 0 asks about abn_tower_forward(t, x1, x2, rows, n_calls, train, ws), backward = 1 about
 * the abn_tower_backward / abn_tower_backward_loss after it.  Returns one of ABN_PATH_* (< 0: bad
 * descriptor); *precision_out (may be NULL) receives the abn_tower_desc.precision code actually
 * used: a 'f16x2' tower that falls to the GEMM kernels (widths > 512 or not multiples of 4,
 * BatchNorm on < 256 rows, ABN_PLANES=0) computes in bf16x3 there, and this is where a caller
 * learns it. */
enum {
    ABN_PATH_PER_LAYER = 0,        /* one GEMM launch per layer (gemm_f32.h) */
    ABN_PATH_FUSED_F32 = 1,        /* the fp32 tower in one launch (tower_fused.h) */
    ABN_PATH_PLANES = 2,           /* operand-plane chain, everything a backward needs is kept */
    ABN_PATH_PLANES_INFER = 3,     /* operand-plane chain, inference (forward_only) */
    ABN_PATH_PLANES_INFER_BN = 4,  /* ... with BatchNorm's running statistics in the epilogue */
    ABN_PATH_BN_LAYERS = 5,        /* BatchNorm training: one operand-plane launch per layer */
    ABN_PATH_WIDE = 6,             /* small batches: one launch per layer over up to 8 workgroups per row block */
    ABN_PATH_BN_TOWER = 7          /* BatchNorm training: the whole tower in ONE resident launch per direction, grid barriers
                                      between the layers (csrc/tower_bn_persist.h): batches of 256 .. 32 x (CUs of the device)
                                      tower rows with per-replica statistics and a sync buffer (abn_tower_desc.sync_ws);
                                      ABN_BN_PERSIST=0 keeps ABN_PATH_BN_LAYERS.  The answer therefore also depends on the
                                      current device's CU count. */
};
int abn_tower_path(const abn_tower_desc* t, const float* x1, const float* x2, int64_t rows,
                   int64_t n_calls, int train, const float* ws, int backward,
                   int32_t* precision_out);

/* Float offset of one of the library's operand images, for callers that decode them (the tests'
 * decoders, tests/planes_decode.py) -- which = 0 packed W_l, 1 packed W_l^T (relative to
 * abn_tower_desc.wpack when given, else to the forward workspace), 2 the transposed image of
 * [input of layer l | 1], 4 a BatchNorm layer's z_l, 5 the row-major output of layer l (forward
 * workspace), 3 the transposed image of dZ_l (backward scratch); -1 when there is no such image.
 * The formats are csrc/tower_planes.h's; they change with ABN_ABI_VERSION. */
int64_t abn_tower_image_offset(const abn_tower_desc* t, int64_t rows, int64_t n_calls, int which,
                               int l);

/* The library reads its A/B switches (ABN_PLANES, ABN_WIDE, ABN_DTW_PC, ... : kernel choice only)
 * from the environment once, when it is loaded; this reads them again (tests and A/B tools that
 * change one inside a process). */
void abn_reload_switches(void);

/* SiameseNetwork.forward_once / forward, abnet3/model.py:179-196.
 * `rows` input rows in total, made of `n_calls` forward_once calls of
 * rows/n_calls rows each (1 = embed, 2 = Siamese pair): call c reads rows
 * [c*rows/n_calls, ...) from x1 (c == 0) or x2 (c == 1; x2 may be NULL when
 * x1 already holds all rows contiguously).  BatchNorm statistics and running
 * stat updates are per call, as in the reference (two updates per Siamese
 * forward).  train != 0: batch statistics, activations saved in ws;
 * train == 0: running statistics.  Output: ws + abn_tower_out_offset().
 * A batch_norm tower in the default arithmetic runs one operand-plane launch per layer in
 * training (its backward likewise), and the single-launch forward with the running statistics folded in
 * when train == 0 and forward_only != 0; otherwise the per-layer kernels.  (ABN_PATH_BN_TOWER: where the whole grid is
 * resident at once -- at most one workgroup of 32 rows per CU -- training runs as ONE launch per direction with grid
 * hand-overs between the layers; a hand-over that cannot complete gives up after a bounded spin and the launch leaves NaN
 * in the embeddings / the loss instead of hanging.)  Results agree to
 * rounding; forward and backward of one pass must see the same environment switches. */
int abn_tower_forward(const abn_tower_desc* t, const float* x1, const float* x2,
                      int64_t rows, int64_t n_calls, int train, float* ws,
                      void* stream);

/* Autograd of the above (what loss.backward() runs, abnet3/trainer.py:239).
 * d_out: [rows, dims[n_layers]] gradient w.r.t. the output embeddings.
 * Writes dW/db (+dbn_w/dbn_b) summed over all rows (both towers), and dx
 * ([rows, dims[0]], may be NULL: the reference never needs it).  t, x1, x2, rows, n_calls and
 * ws must be the forward call's (ws unchanged since). */
int abn_tower_backward(const abn_tower_desc* t, const float* x1, const float* x2,
                       const float* d_out, int64_t rows, int64_t n_calls,
                       const float* ws, float* scratch, int64_t scratch_floats,
                       float* dx, void* stream);

/* ONE of the two launches of an ABN_PATH_PLANES backward, for per-launch measurements (bench.py's
 * roofline legs): part = 1 the data-gradient chain, 2 the weight gradients of every layer -- after
 * a complete abn_tower_backward with the same arguments has left the other launch's output in
 * place.  The split-K slabs are never reduced (dW / db are not written).  ABN_E_UNSUPPORTED on
 * every other path. */
int abn_tower_backward_launch(const abn_tower_desc* t, const float* x1, const float* x2,
                              const float* d_out, int64_t rows, int64_t n_calls, const float* ws,
                              float* scratch, int64_t scratch_floats, int part, void* stream);

/* abn_pair_loss_dz + abn_tower_backward in the backward's own launches (abnet3/trainer.py:238-239:
 * loss = self.loss(emb1, emb2, y); loss.backward()): rows = 2 B tower rows, [tower 1: pairs 0..B-1 |
 * tower 2: pairs 0..B-1], whose embeddings the forward left in ws; the first phase of the data
 * gradient chain computes the loss and d loss / d z of the output layer (same arithmetic, fp64 per
 * pair) instead of reading d_out; for a BatchNorm tower on its layer launches (per-replica statistics,
 * wgrad_part 0) the launch that sums the output layer's dy and dy xhat does, and leaves d loss / d a for
 * the top layer's launch.  Only for towers the operand-plane kernels take (default arithmetic, widths <= 512
 * and multiples of 4): ABN_E_UNSUPPORTED otherwise, and the caller uses the two separate calls.  loss_ws: abn_tower_backward_loss_ws_bytes(rows) bytes whose
 * first 8 (a ticket counter) are zero before the first call and are left zero.
 * n_valid (device int32, or NULL): a PADDED batch -- only the first *n_valid pairs of the B = rows / 2
 * are real (abn_gather_pairs writes such batches: zero rows behind the real ones, tower 2 starting at
 * row B); the others contribute no loss term and their d loss / d z is zero, so nothing of them reaches
 * a gradient, and avg divides by *n_valid.  One captured step then serves every batch size of a bucket
 * (the reference's batches of 8 word pairs have a different number of frame pairs every step,
 * abnet3/dataloader.py:248-255).  loss_accum (device double, or NULL): the call's loss is also added to
 * it -- the epoch's running sum the reference keeps on the host (abnet3/trainer.py:242). */
int64_t abn_tower_backward_loss_ws_bytes(int64_t rows);
int abn_tower_backward_loss(const abn_tower_desc* t, const float* x1, const float* x2, const void* y,
                            int y_dtype, int loss_kind, float margin, int avg, int64_t rows,
                            const float* ws, float* scratch, int64_t scratch_floats,
                            float* loss_out, void* loss_ws, const int32_t* n_valid,
                            double* loss_accum, void* stream);

/* Finishes an abn_tower_backward that ran with defer_reduce = 1 (same descriptor, rows and
 * scratch): sums the split-K slabs in their fixed order, writes the gradients to dW / db AND
 * applies abn_optimizer_step's update to the same elements -- one launch for what is otherwise
 * the slab reduction followed by the optimizer step (abnet3/trainer.py:239-240 back to back, no
 * gradient exchange in between: single process).  With batch_norm the BatchNorm tensors (whose gradients
 * the backward wrote directly) are stepped by the same launch.  params / grads / state1 / state2 are the flat
 * buffers (n floats each) that hold every tensor of the descriptor at the same offsets: element j
 * of layer l's weight lives at (dW[l] - grads) + j in all four. */
int abn_tower_reduce_step(const abn_tower_desc* t, int64_t rows, const float* scratch,
                          int64_t scratch_floats, int kind, float* params, float* grads,
                          float* state1, float* state2, int64_t n, float lr, float hp0,
                          float hp1, float eps, int64_t step, float grad_scale, void* stream);

/* The data-parallel step's gradient exchange (the reference has no multi-process path: this sits
 * between loss.backward() and optimizer.step(), abnet3/trainer.py:239 -> :240) as a ONE-SHOT all-reduce over peer-mapped
 * mailboxes instead of a ring: every rank pushes shard s of its bucket into rank s's mailbox, sums the world's contributions
 * to its own shard in RANK ORDER (deterministic: replicas stay bit-identical) and pushes the reduced shard to everybody --
 * two hops over all xGMI links at once, one kernel launch per rank on the caller's stream (graph-capturable, no host call
 * inside).  The caller owns the mailboxes: rank s allocates abn_oneshot_mail_bytes(world, cap_floats) bytes of FINE-GRAINED
 * device memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained)), zeroes it once, exports it (hipIpcGetMemHandle) and maps
 * every peer's (hipIpcOpenMemHandle) into mail[]; mail[rank] is its own.  Every rank of the group makes the same sequence of
 * calls (same n).  SUM of fp32 in place over buf[0 .. n), n % 4 == 0, n <= cap_floats, buf 16-byte aligned.  A rank whose
 * peer never arrives gives up after a bounded spin, leaves NaN in buf and its mailbox's failure word set (zero the mailboxes
 * again before the next use). */
#define ABN_ONESHOT_MAX_RANKS 8
typedef struct abn_oneshot_ctx {
    int32_t rank, world;
    void* mail[ABN_ONESHOT_MAX_RANKS];     /* mail[s]: rank s's mailbox as mapped in THIS process */
    int64_t cap_floats;                    /* most floats one call reduces (what the mailboxes were sized for) */
} abn_oneshot_ctx;
int64_t abn_oneshot_mail_bytes(int32_t world, int64_t cap_floats);
int abn_allreduce_oneshot(const abn_oneshot_ctx* ctx, float* buf, int64_t n, void* stream);

/* One nn.Linear at a time with the same kernels (what abn_tower_* chains):
 *   forward  y = act(x W^T + b)                       (addmm + activation)
 *   dgrad    dx = (dz W) * act'(a_prev)  [a_prev NULL: plain dz W]
 *   wgrad    dW = dz^T a_in, db = colsum(dz); scratch: split-K slabs
 * x [rows,in], W [out,in], y/dz [rows,out], a_prev/dx/a_in [rows,in]. */
int abn_linear_forward(const float* x, const float* W, const float* b, int64_t rows,
                       int64_t in_dim, int64_t out_dim, int act, float* y, void* stream);
int abn_linear_dgrad(const float* dz, const float* W, int64_t rows, int64_t in_dim,
                     int64_t out_dim, const float* a_prev, int act_prev, float* dx,
                     void* stream);
int64_t abn_linear_wgrad_scratch_floats(int64_t rows, int64_t in_dim, int64_t out_dim);
int abn_linear_wgrad(const float* dz, const float* a_in, int64_t rows, int64_t in_dim,
                     int64_t out_dim, float* dW, float* db, float* scratch,
                     int64_t scratch_floats, void* stream);
/* dgrad + wgrad of one nn.Linear the way abn_tower_backward issues them: both read dz
 * only, so they go out as ONE grid (the dgrad's workgroups take over the CUs as the
 * wgrad's retire), followed by the slab reduction.  a_in [rows,in] is the layer's input =
 * the previous activation (act_prev = 0: no activation derivative).  scratch as for
 * abn_linear_wgrad. */
int abn_linear_backward(const float* dz, const float* W, const float* a_in, int64_t rows,
                        int64_t in_dim, int64_t out_dim, int act_prev, float* dW,
                        float* db, float* dx, float* scratch, int64_t scratch_floats,
                        void* stream);
/* ... in the arithmetic abn_tower_desc.precision names (0 exact fp32 = abn_linear_backward,
 * 1 bf16 operands, 2 bf16 x 3, 3 = run as 2: fp16 x 2 exists on the operand planes only): the grid abn_tower_backward
 * issues for that network.  dW and db
 * both NULL: only that grid runs and the split-K slabs stay unreduced in scratch (bench.py times
 * the grid alone this way). */
int abn_linear_backward_prec(const float* dz, const float* W, const float* a_in, int64_t rows,
                             int64_t in_dim, int64_t out_dim, int act_prev, int precision,
                             float* dW, float* db, float* dx, float* scratch,
                             int64_t scratch_floats, void* stream);

/* coscos2.forward / cosmargin.forward fused with their backward,
 * abnet3/loss.py:46-67 and :85-105 (nn.CosineSimilarity(dim=1, eps=1e-6)).
 * loss_out: device scalar (fp32).  de1/de2: [B, D] gradients of the (already
 * /B-scaled when avg) loss; both may be NULL for a forward-only call.
 * ws: abn_pair_loss_ws_bytes(B) bytes of device scratch whose FIRST 8 bytes (a ticket
 * counter) must be zero before the first call on this buffer; every call leaves them zero
 * (ONE launch: the workgroup that finishes last sums the per-workgroup partial losses in a
 * fixed order).  Calls sharing a ws buffer must be ordered on one stream. */
int64_t abn_pair_loss_ws_bytes(int64_t B);
/* kind = ABN_LOSS_KL (KLLoss, abnet3/loss.py:108-137): e1 / e2 are probability rows p / q, the loss is
 * H(KL(p||q)) + H(KL(q||p)) with H = nn.HingeEmbeddingLoss(margin) (a mean over B with avg), any margin; label 1
 * takes KL, -1 max(0, margin - KL), any other label KL + max(0, margin - KL).  Every per-row sum in fp64. */
int abn_pair_loss(const float* e1, const float* e2, const void* y, int y_dtype,
                  int64_t B, int64_t D, int kind, float margin, int avg,
                  float* loss_out, float* de1, float* de2, void* ws,
                  void* stream);
/* abn_pair_loss on a PADDED batch (see abn_gather_pairs / abn_tower_backward_loss): only the first *n_valid
 * (device int32, NULL = all B) pairs are real -- the others add nothing to the loss and get zero gradient
 * rows, a mean loss divides by *n_valid -- and the loss is also added to *loss_accum (device double, may be
 * NULL): the evaluation pass of a trainer whose batches sit in bucket-sized static buffers
 * (abnet3/trainer.py:244-248: the dev loss summed over the batches). */
int abn_pair_loss_padded(const float* e1, const float* e2, const void* y, int y_dtype,
                         int64_t B, int64_t D, int kind, float margin, int avg,
                         const int32_t* n_valid, float* loss_out, double* loss_accum,
                         float* de1, float* de2, void* ws, void* stream);
/* The same with the output layer's activation derivative (and dropout multipliers, mask1 /
 * mask2 [B, D] or NULL) folded in: e1 / e2 are the tower's outputs act(z), and dz1 / dz2
 * receive d loss / d z = d loss / d e * act'(e) [* mask] -- the first step of
 * loss.backward() (abnet3/trainer.py:239) through a tower without BatchNorm.  Hand
 * [dz1; dz2] to abn_tower_backward with abn_tower_desc.d_out_is_dz = 1.
 * kind = ABN_LOSS_KL with act = ABN_ACT_SOFTMAX: e1 / e2 are LOGITS z1 / z2, the loss is KLLoss of
 * p = softmax(z1), q = softmax(z2) (nn.Softmax of a 'softmax' last_non_linearity, abnet3/model.py:161-166), and
 * dz1 / dz2 receive d loss / d z1, d z2 [* mask] (softmax, loss and gradient in one launch).  ABN_ACT_SOFTMAX
 * with any other kind, or in abn_pair_loss / abn_pair_loss_padded: ABN_E_UNSUPPORTED. */
int abn_pair_loss_dz(const float* e1, const float* e2, const void* y, int y_dtype,
                     int64_t B, int64_t D, int kind, float margin, int avg, int act,
                     const float* mask1, const float* mask2, float* loss_out,
                     float* dz1, float* dz2, void* ws, void* stream);

/* torch.optim.{SGD(momentum),Adadelta,Adam,Adagrad,RMSprop}.step over one flat
 * fp32 parameter buffer (abnet3/trainer.py:68-87, :240).  state1/state2: flat
 * buffers of n floats, zero-initialised by the caller before the first step
 * (momentum_buffer | square_avg, acc_delta | exp_avg, exp_avg_sq | sum | -).
 * `step` counts from 1.  hp0/hp1: momentum | rho=0.9 | beta1,beta2 | - | alpha.
 * grad_scale multiplies the gradient first (1/world_size for avg=True DP). */
int abn_optimizer_step(int kind, float* params, const float* grads, float* state1,
                       float* state2, int64_t n, float lr, float hp0, float hp1,
                       float eps, int64_t step, float grad_scale, void* stream);

/* abnet3/utils.py:40-60 (cosine_distance) + :147-153 (get_dtw_alignment ->
 * third-party dtw.DTW) for a batch of token pairs.  Pair p aligns rows
 * [off1[p], off1[p]+n1[p]) of feats1 ([rows1, D] fp32, device) with rows
 * [off2[p], off2[p]+n2[p]) of feats2.  The per-pair metadata (off*, n*) are
 * HOST arrays -- token boundaries come from the pairs file, host data in the
 * reference too -- which the call stages into `ws` through `host_stage` (a
 * caller-owned host buffer, ideally pinned, that must stay untouched until the
 * stream has passed this call).  path1/path2: [npairs, path_stride] int32 (device);
 * the path of pair p, from (0,0) to (n1-1,n2-1), is RIGHT-ALIGNED in its row: entries
 * [path_stride - path_len[p], path_stride), in forward order (the traceback walks from the
 * end and writes each cell where it belongs; the rest of the row is not touched).
 * path_len[p] = 0 marks a pair the reference would have dropped (NaN distance,
 * abnet3/dataloader.py:188-191) or an empty token.  total_cost (device, [npairs] f64) may be
 * NULL.  Tokens of any length.  path_stride >= max(n1 + n2 - 1).
 * One fused kernel per call (distances on the fp32 matrix cores, the reference's division /
 * acosf / pi per cell, float64 dynamic programme, 2-bit back-pointers) plus a traceback
 * kernel, all on `stream`: no library-owned streams, events or other global state.  path_len and total_cost need no
 * clearing by the caller: every pair's entries are written by one of the call's launches.  The cost
 * matrix is never materialised: the workspace holds ~0.26 B per cell (back-pointers) plus
 * per-workgroup boundary rows.  rows1 / rows2 bound the offsets (checked). */
int64_t abn_dtw_ws_bytes(const int32_t* n1_host, const int32_t* n2_host,
                         int64_t npairs, int64_t rows1, int64_t rows2);
int64_t abn_dtw_host_stage_bytes(const int32_t* n1_host, const int32_t* n2_host,
                                 int64_t npairs);
int abn_dtw_batched(const float* feats1, int64_t rows1, const float* feats2,
                    int64_t rows2, const int64_t* off1_host, const int32_t* n1_host,
                    const int64_t* off2_host, const int32_t* n2_host, int64_t npairs,
                    int64_t D, int32_t* path1, int32_t* path2, int32_t* path_len,
                    int64_t path_stride, double* total_cost, void* ws,
                    int64_t ws_bytes, void* host_stage, int64_t host_stage_bytes,
                    void* stream);
/* The same call with the traceback BESIDE the fill kernel instead of behind it (ABI v19): `side_stream` is a second
 * stream of the caller's (same device; NULL or == stream: exactly abn_dtw_batched).  The fill kernel stores what the
 * traceback reads of a pair write-through and flags the pair when it is complete; a traceback launch on `side_stream`
 * polls the flags (bounded, asleep in between) and walks each pair as it completes, so that the ~0.2 ms a 10 000-pair
 * traceback takes -- one pair's chain of dependent window fetches, a few per cent of the chip -- run under the fill's
 * 2.7 ms; `stream` then waits for it and sweeps up whatever it left (normally nothing).  Same results, bit for bit.
 * The library orders the two streams with two events it keeps per host thread and device (made at the first call, the
 * only state this entry point adds to the process); on return both streams carry work of this call and `stream` alone is
 * behind all of it: the caller
 * synchronises with `stream` as before and need not look at `side_stream` again.  40-value frames (the gang kernel);
 * every other frame width runs as abn_dtw_batched. */
int abn_dtw_batched_overlap(const float* feats1, int64_t rows1, const float* feats2,
                            int64_t rows2, const int64_t* off1_host, const int32_t* n1_host,
                            const int64_t* off2_host, const int32_t* n2_host, int64_t npairs,
                            int64_t D, int32_t* path1, int32_t* path2, int32_t* path_len,
                            int64_t path_stride, double* total_cost, void* ws,
                            int64_t ws_bytes, void* host_stage, int64_t host_stage_bytes,
                            void* stream, void* side_stream);
/* DTW cost and path length without the path (ABX evaluation, abnet3_amd/abx.py), for a pair table that lives on
 * the DEVICE: pair p aligns rows [off1[p], off1[p]+n1[p]) of feats1 with rows [off2[p], off2[p]+n2[p]) of feats2
 * ([rows, D] fp32; off*, n*: device arrays).  total_cost[p] (f64) and path_len[p] (int32) equal, bit for bit, what
 * abn_dtw_batched writes for the same pair: the same cell function, the same float64 recurrence and tie-break, the
 * length of the path its traceback would walk; 0 and 0 for a pair it drops (a NaN distance, an empty token).  A pair
 * whose token 2 has more than abn_dtw_cost_max_n2() frames, a negative length or rows outside the arrays is refused:
 * path_len = -1, total_cost = 0, nothing is read (callers send long pairs to abn_dtw_batched).  Token 1 has no limit,
 * any D >= 1.  One launch on `stream`, no workspace. */
#define ABN_DTW_COST_MAX_N2 256
int64_t abn_dtw_cost_max_n2(void);
int abn_dtw_cost_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                         const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                         int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, void* stream);
/* abn_dtw_cost_batched, except that a cosine which rounds beyond +-1 -- parallel or opposite frames, identical ones
 * among them: a finite dot product over a finite non-zero product of the norms -- is read as distance 0 (1 when
 * opposite), the rule of abn_dtw_search_batched, instead of dropping the pair.  Every pair without such a cell gets
 * the same bits as from abn_dtw_cost_batched.  For corpora made of repeated frames (KMeansQuantizer.quantize); added
 * within ABI 20: a new symbol only. */
int abn_dtw_cost_parallel_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                                  const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                                  int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, void* stream);
/* The tables of the symmetrised Kullback-Leibler frame distance (ABX of posteriorgrams, abnet3_amd/abx.py; added
 * within ABI 20: new symbols only).  x: [rows, D] fp32 on the device; floor > 0.  P[r, k] = max(x[r, k], floor),
 * L[r, k] = (float)log((double)P[r, k]) (both [rows, D] fp32, no renormalisation); bad_row[r] (uint8 [rows], written
 * for every row) = 1 when row r holds a non-finite or a negative value (the contents of its P / L rows are then
 * unspecified), else 0.  Zeros are legal and are floored.  One launch on `stream`. */
int abn_kl_tables(const float* x, int64_t rows, int64_t D, float floor, float* P, float* L,
                  uint8_t* bad_row, void* stream);
/* abn_dtw_cost_batched with the symmetrised Kullback-Leibler divergence as the frame distance: the same pair-table
 * contract (device tables, a pair with a negative length, rows outside the tables or a token 2 of more than
 * abn_dtw_cost_max_n2() frames is refused with path_len = -1, total_cost = 0 and nothing read; an empty token gives
 * 0 and 0; one launch on `stream`, no workspace), the same float64 recurrence, tie-break and carried path length.  The
 * cell of frames p (token 1) and q (token 2) over abn_kl_tables' P and L tables, in fp32 without fused multiply-add,
 * in ascending k: acc = acc + ((P_p[k] - P_q[k]) * (L_p[k] - L_q[k])), d = 0.5f * acc -- d >= 0 always, d == 0 for
 * identical frames.  bad1 / bad2: abn_kl_tables' row flags ([rows1] / [rows2]); a pair with a flagged row in either
 * token is dropped: path_len = 0, total_cost = 0.  There is no second kernel for longer tokens 2. */
int abn_dtw_cost_kl_batched(const float* P1, const float* L1, int64_t rows1, const float* P2,
                            const float* L2, int64_t rows2, const int64_t* off1, const int32_t* n1,
                            const int64_t* off2, const int32_t* n2, int64_t npairs, int64_t D,
                            const uint8_t* bad1, const uint8_t* bad2, double* total_cost,
                            int32_t* path_len, void* stream);
/* Subsequence DTW for query-by-example search (abnet3_amd/qbe.py; added within ABI 20: new symbols only).  The pair
 * table lives on the DEVICE: pair p aligns ALL of query rows [q_off[p], q_off[p]+q_n[p]) of qry with ANY contiguous run
 * of utterance rows [u_off[p], u_off[p]+u_n[p]) of utt ([rows, D] fp32).  Cells: abn_dtw_cost_batched's angular
 * distance, except that no pair is dropped: a NaN cell with a finite dot product and a finite non-zero product of
 * the norms is |cos| rounded above 1 and counts 0 (dot > 0) or 1 (dot < 0); any other NaN cell is blocked (+inf).
 * Recurrence: float64, cost = d + min(diag, up, left), first minimum in that order, length and start row carried along
 * the chosen predecessor; in query column 0 the diagonal predecessor of every utterance row i is a virtual cell of
 * cost 0, length 0 and start i, and there is no left predecessor.  Result: among the utterance rows i whose cell in the
 * last query column is finite, the first that minimises cost / length (float64): total_cost[p], path_len[p], start[p],
 * end[p] = i (utterance-relative, inclusive).  No such row: path_len = 0, total_cost = 0, start = end = -1; the same
 * for an empty query or utterance.  A pair with a negative length, rows outside the tables, a query of more than
 * abn_dtw_search_max_query() frames or profile entries outside [0, prof_rows) is refused: path_len = -1,
 * total_cost = 0, start = end = -1, nothing is read and no profile entry is written.  The utterance has no limit.
 * Profile (prof_cost == NULL: none; else all four pointers): for utterance row i of pair p, entry prof_off[p] + i of
 * prof_cost / prof_len / prof_start ([prof_rows]) holds the row's cell of the last query column: cost, length, start;
 * +inf, 0, -1 where it is not finite.  One launch on `stream`, no workspace. */
#define ABN_DTW_SEARCH_MAX_QUERY 256
int64_t abn_dtw_search_max_query(void);
int abn_dtw_search_batched(const float* utt, int64_t rows_u, const float* qry, int64_t rows_q,
                           const int64_t* u_off, const int32_t* u_n, const int64_t* q_off, const int32_t* q_n,
                           int64_t npairs, int64_t D, double* total_cost, int32_t* path_len, int32_t* start,
                           int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                           int32_t* prof_len, int32_t* prof_start, void* stream);
/* abn_dtw_search_batched over the symmetrised Kullback-Leibler cell of abn_dtw_cost_kl_batched (abn_kl_tables' P, L
 * and row flags of each side).  A cell that touches a flagged row is blocked (+inf); the pair is kept. */
int abn_dtw_search_kl_batched(const float* PU, const float* LU, int64_t rows_u, const float* PQ, const float* LQ,
                              int64_t rows_q, const int64_t* u_off, const int32_t* u_n, const int64_t* q_off,
                              const int32_t* q_n, int64_t npairs, int64_t D, const uint8_t* bad_u,
                              const uint8_t* bad_q, double* total_cost, int32_t* path_len, int32_t* start,
                              int32_t* end, const int64_t* prof_off, int64_t prof_rows, double* prof_cost,
                              int32_t* prof_len, int32_t* prof_start, void* stream);
/* Local-alignment DTW for spoken-term discovery (abnet3_amd/terms.py, whose module docstring is the definition; added
 * within ABI 20: new symbols only).  The pair table lives on the DEVICE: pair p aligns ANY stretch of rows
 * [off1[p], off1[p]+n1[p]) of feats1 with ANY stretch of rows [off2[p], off2[p]+n2[p]) of feats2 ([rows, D] fp32).
 * Cells: abn_dtw_search_batched's d(i, j), blocked cells included.  exclude > 0 also blocks every cell with
 * |(off1[p] + i) - (off2[p] + j)| < exclude -- table rows, so it needs both sides to be ONE table: feats1 == feats2
 * and rows1 == rows2, else ABN_E_ARG.  Similarity s = (double)theta - (double)d (theta finite and > 0, else
 * ABN_E_ARG), -inf for a blocked cell.  Recurrence in float64 (Smith-Waterman): best = the first MAXIMUM of H(i-1, j-1),
 * H(i-1, j), H(i, j-1) in that order (a cell outside the matrix is dead: H = 0, length 0); best > 0: H = best + s, the
 * length and the start cell are carried; else H = s, length 1, start (i, j); a cell whose H is not > 0 is dead.
 * Result: the cell of largest H > 0, ties to the smallest i, then the smallest j: score[p] = H, path_len[p],
 * start1[p], start2[p] (the path's first cell), end1[p] = i, end2[p] = j, stretch-relative and inclusive.  No live cell
 * or an empty side: path_len = 0, score = 0, the four bounds -1.  A pair with a negative length, rows outside the
 * tables or side 2 of more than abn_dtw_local_max_n2() frames is refused: path_len = -1, score = 0, bounds -1, nothing
 * is read.  Side 1 has no limit.  One launch on `stream`, no workspace. */
#define ABN_DTW_LOCAL_MAX_N2 512
int64_t abn_dtw_local_max_n2(void);
int abn_dtw_local_batched(const float* feats1, int64_t rows1, const float* feats2, int64_t rows2,
                          const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                          int64_t npairs, int64_t D, float theta, int64_t exclude, double* score,
                          int32_t* path_len, int32_t* start1, int32_t* start2, int32_t* end1, int32_t* end2,
                          void* stream);
/* abn_dtw_local_batched over the symmetrised Kullback-Leibler cell (abn_kl_tables' P, L and row flags of each side).
 * A cell that touches a flagged row is blocked.  exclude > 0 needs P1 == P2, L1 == L2, bad1 == bad2, rows1 == rows2. */
int abn_dtw_local_kl_batched(const float* P1, const float* L1, int64_t rows1, const float* P2, const float* L2,
                             int64_t rows2, const int64_t* off1, const int32_t* n1, const int64_t* off2,
                             const int32_t* n2, int64_t npairs, int64_t D, const uint8_t* bad1,
                             const uint8_t* bad2, float theta, int64_t exclude, double* score, int32_t* path_len,
                             int32_t* start1, int32_t* start2, int32_t* end1, int32_t* end2, void* stream);
/* Batched Levenshtein distance over int32 symbol sequences (abnet3_amd/tde.py: the normalised edit distance of
 * discovered term pairs; added within ABI 20: new symbols only).  All tables live on the DEVICE; sym1 == sym2 is
 * allowed.  A symbol is any int32, compared by equality only.  dist[p] = the Levenshtein distance, insertion, deletion
 * and substitution costing 1 each, of sym1[off1[p] .. off1[p]+n1[p]) and sym2[off2[p] .. off2[p]+n2[p]).  An empty side
 * is legal: the distance is the other side's length.  The distance is symmetric and the kernel itself puts the SHORTER
 * side where its cap applies: a pair is refused when min(n1[p], n2[p]) > max_short, when a length is negative or when
 * its rows lie outside their table -- dist[p] = -1 and nothing is read.  The longer side has no limit.
 * max_short is the caller's promise, 1 .. ABN_EDIT_MAX_SHORT (else ABN_E_ARG): the host picks the kernel from it
 * without reading device memory (<= 32, <= 64, <= 256).  One launch on `stream`, no workspace, any npairs (a
 * grid-stride loop over at most ABN_EDIT_GRID_BLOCKS workgroups of ABN_EDIT_BLOCK_PAIRS pairs); npairs == 0 returns at
 * once.  Null pointers (a table of 0 rows may be NULL) and a max_short out of range are ABN_E_ARG before any launch,
 * with a message in abn_last_error(). */
#define ABN_EDIT_MAX_SHORT 256
#define ABN_EDIT_GRID_BLOCKS 4096
#define ABN_EDIT_BLOCK_PAIRS 64
int64_t abn_edit_max_short(void);
int abn_edit_distance_batched(const int32_t* sym1, int64_t rows1, const int32_t* sym2, int64_t rows2,
                              const int64_t* off1, const int32_t* n1, const int64_t* off2, const int32_t* n2,
                              int64_t npairs, int64_t max_short, int32_t* dist, void* stream);
/* The prefilter of term discovery (abnet3_amd/prefilter.py, whose module docstring is the definition; added within
 * ABI 20: new symbols only).  Neither entry uses atomics or a workspace; one launch each on `stream`.
 *
 * abn_lsh_signatures: random-hyperplane signatures of the rows of table [rows][D] fp32 under planes [bits][D] fp32.
 * sig [rows][bits / 32] uint32: bit b is bit b % 32 of word b / 32 (least significant first) and is 1 iff the fp32 dot
 * product <table[r], planes[b]> is > 0 (fused multiply-adds in ascending column order).  live [rows] uint8: 1 iff every
 * element of the row is finite and at least one is non-zero -- exact, whatever the dot products are; a dead row's words
 * are 0.  bits: a multiple of 32 in 32 .. ABN_LSH_MAX_BITS; D in 1 .. ABN_LSH_MAX_D; else ABN_E_ARG, like null pointers,
 * before any launch.  rows == 0 returns at once.  The table is read from memory once.
 *
 * abn_lsh_diag_hits_batched: the pair table lives on the DEVICE, as abn_dtw_local_batched's: pair p is rows
 * [off1[p], off1[p]+n1[p]) of (sig1, live1) [rows1] against rows [off2[p], off2[p]+n2[p]) of (sig2, live2) [rows2], the
 * signatures `words` uint32 wide (1 .. ABN_LSH_MAX_BITS / 32).  For 0 <= i < n1, 0 <= j < n2:
 *   hit(i, j) = live1[off1+i] and live2[off2+j] and popcount(sig1[off1+i] ^ sig2[off2+j]) <= max_hamming and
 *               (exclude == 0 or |(off1+i) - (off2+j)| >= exclude)
 *   hd(i, j)  = OR of hit(i, j+t) over |t| <= dilate with 0 <= j+t < n2
 *   run(i, j) = the sum over s = 0 .. span-1 of hd(i-s, j-s), the terms inside the matrix only
 * best[p] = the largest run, diag[p] = i - j and end1[p] = i of the cell that reaches it, ties to the smallest i - j,
 * then the smallest i.  No hit or an empty side: best 0, diag 0, end1 -1.  A pair with a negative length, rows outside
 * its tables or side 2 of more than abn_dtw_local_max_n2() frames is refused: best -1, diag 0, end1 -1, nothing is read.
 * Side 1 has no limit.  max_hamming in 0 .. 32 words, span in 1 .. ABN_LSH_MAX_SPAN, dilate in 0 .. ABN_LSH_MAX_DILATE,
 * exclude >= 0, and exclude > 0 needs sig1 == sig2, live1 == live2 and rows1 == rows2: else ABN_E_ARG, like null
 * pointers (a table of 0 rows may be NULL), before any launch.  npairs == 0 returns at once.  Any npairs: a grid-stride
 * loop over at most ABN_LSH_GRID_BLOCKS workgroups, one pair each at a time. */
#define ABN_LSH_MAX_BITS 256
#define ABN_LSH_MAX_D 4096
#define ABN_LSH_MAX_SPAN 64
#define ABN_LSH_MAX_DILATE 8
#define ABN_LSH_GRID_BLOCKS 2048
int abn_lsh_signatures(const float* table, int64_t rows, int64_t D, const float* planes, int64_t bits,
                       uint32_t* sig, uint8_t* live, void* stream);
int abn_lsh_diag_hits_batched(const uint32_t* sig1, const uint8_t* live1, int64_t rows1, const uint32_t* sig2,
                              const uint8_t* live2, int64_t rows2, const int64_t* off1, const int32_t* n1,
                              const int64_t* off2, const int32_t* n2, int64_t npairs, int64_t words,
                              int64_t max_hamming, int64_t span, int64_t dilate, int64_t exclude, int32_t* best,
                              int32_t* diag, int32_t* end1, void* stream);
/* ABX triplet scores (abnet3_amd/abx.py).  Row r is one X of ABX cell row_cell[r]: the distances d(A, X) over its A
 * are dist[a_off[r] .. a_off[r] + a_len[r]), the d(B, X) over its B dist[b_off[r] .. b_off[r] + b_len[r]) (device
 * arrays, dist: [ndist] f64).  For every cell c: score2[c] = the sum over its rows and their A x B triplets of 2 when
 * d(A, X) < d(B, X), 1 when equal, 0 otherwise; count[c] = its number of triplets (both int64 [ncells] on the device,
 * cleared by the call; integer sums: the same values in any order).  A row that reads outside dist or names no cell
 * is skipped and counted in *refused (device int32, cleared by the call; may be NULL). */
int abn_abx_score(const double* dist, int64_t ndist, const int64_t* a_off, const int32_t* a_len,
                  const int64_t* b_off, const int32_t* b_len, const int32_t* row_cell, int64_t nrows,
                  int64_t ncells, int64_t* score2, int64_t* count, int32_t* refused, void* stream);
/* The distance matrix alone (utils.py:40-60), one pair, float64 [N, M] out.  The
 * reference computes in the precision of its inputs (utils.py:41-42: both float32 or
 * both float64): abn_cosine_distance is the float32 arithmetic of the hot path (the
 * same cell function as abn_dtw_batched: numpy's norm summation order, one fma chain
 * per dot product, one division, glibc's acosf, / float32(pi) -- bit-identical to the
 * reference's output on its plain numpy/libm path), abn_cosine_distance_f64 the same
 * statements in double.  *bad_flag (device int32, may be NULL) is set when an entry is
 * NaN or negative -- the reference's `assert np.all(d >= 0)` (utils.py:59). */
int abn_cosine_distance(const float* x, int64_t N, const float* y, int64_t M,
                        int64_t D, double* d, int32_t* bad_flag, void* stream);
int abn_cosine_distance_f64(const double* x, int64_t N, const double* y, int64_t M,
                            int64_t D, double* d, int32_t* bad_flag, void* stream);

/* np.arccos on float32 as the reference's cosine_distance evaluates it on numpy's plain
 * path (utils.py:50,53: scipy.arccos = np.arccos = libm acosf): out[i] = acosf(x[i]),
 * bit-identical to glibc 2.35's acosf for every float32 argument (NaN outside [-1, 1]);
 * over_pi != 0: out[i] = acosf(x[i]) / float32(pi), the correctly rounded float32 quotient
 * (utils.py:53).  The cell function of abn_dtw_batched, exposed for verification.
 * over_pi bit 0: divide by pi; bit 1: arguments with 2^-26 < |x| < 0.5 take the straight-line
 * statements the gang kernel uses when a wavefront's cells all lie in that range (same bits). */
int abn_arccos_f32(const float* x, int64_t n, int over_pi, float* out, void* stream);

/* last_non_linearity='softmax' (abnet3/model.py:161-166: nn.Softmax() after the output
 * layer's Linear/Dropout/BatchNorm = softmax over each row of a [rows, n] matrix), and
 * its autograd: dz = a * (da - sum_c(da * a)).  out may alias z; dz may alias da. */
int abn_softmax_rows(const float* z, int64_t rows, int64_t n, float* out, void* stream);
int abn_softmax_rows_backward(const float* a, const float* da, int64_t rows, int64_t n,
                              float* dz, void* stream);

/* The integration unit of MultimodalSiameseNetwork (abnet3/integration.py:71-475), one launch per direction
 * over the rows of both towers.  x1 [rows, d1], x2 [rows, d2] (dense, fp32):
 *   ABN_INTEGRATE_SUM     out [rows, d1] = w * x1 + (1 - w) * x2          (d1 == d2)
 *   ABN_INTEGRATE_CONCAT  out [rows, d1 + d2] = [w * x1 | (1 - w) * x2]
 * weight_kind: NONE (SumIntegration / ConcatenationIntegration: w = 1 - w = 1, no products); FIXED (w_fixed and
 * w_complement as given: BiWeightedFixed, a headstart); SCALAR (w = *w_scalar, 1 - w in fp32:
 * BiWeightedScalarLearnt); ATTENTION (w [rows, K] = act(z1 + z2), act = ABN_ACT_SIGMOID | ABN_ACT_TANH, K = 1 or
 * K = d1 = d2: BiWeightedDeepLearnt).  Every product and sum is one fp32 operation in torch's order, no FMA
 * contraction.  w_out (may be NULL): receives w [rows, K] (the row weight for the non-attention kinds, K = 1).
 * The backward takes g = d loss / d out and writes dx1, dx2 (either may be NULL), for ATTENTION dz [rows, K] =
 * d loss / d z1 = d loss / d z2 (w = the forward's w_out), for SCALAR *dw = the sum over all rows and features of
 * g1 x1 - g2 x2 (fp64, fixed order: bit-identical from run to run; `ws` = abn_integrate_ws_bytes(rows) bytes whose
 * first 4 are zero before the first call -- every call leaves them zero).  Both are NULL-safe at rows = 0 (*dw = 0). */
enum { ABN_INTEGRATE_SUM = 0, ABN_INTEGRATE_CONCAT = 1 };
enum { ABN_INTEGRATE_W_NONE = 0, ABN_INTEGRATE_W_FIXED = 1, ABN_INTEGRATE_W_SCALAR = 2, ABN_INTEGRATE_W_ATTENTION = 3 };
int64_t abn_integrate_ws_bytes(int64_t rows);
int abn_integrate_forward(const float* x1, int64_t d1, const float* x2, int64_t d2, int64_t rows, int mode,
                          int weight_kind, float w_fixed, float w_complement, const float* w_scalar,
                          const float* z1, const float* z2, int64_t K, int act, float* out, float* w_out,
                          void* stream);
int abn_integrate_backward(const float* x1, int64_t d1, const float* x2, int64_t d2, int64_t rows, int mode,
                           int weight_kind, float w_fixed, float w_complement, const float* w_scalar,
                           const float* w, int64_t K, int act, const float* g, float* dx1, float* dx2,
                           float* dz, float* dw, void* ws, void* stream);

/* X[path] gathers of abnet3/dataloader.py:204-205, :673-684: out[i] = table[idx[i]] */
int abn_gather_rows(const float* table, const int64_t* idx, int64_t n, int64_t D,
                    float* out, void* stream);

/* One training batch of frame pairs, gathered straight into the layout a (captured) train step reads
 * (abnet3/dataloader.py:204-205,227-233 + the vstack / permutation of :248-255, with the index lists
 * prepared once per dataset): x12 is [2 n_pad, D] --
 *   x12[r]         = table[idx1[first + r]]   (tower 1),   x12[n_pad + r] = table[idx2[first + r]]   (tower 2)
 * for r < n, zero rows for n <= r < n_pad.  labels (device, `label_bytes` per element: 8 = the float64 /
 * int64 labels of the loaders; may be NULL together with y_out): y_out[r] = labels[first + r], zero
 * padding.  n_valid (device int32, may be NULL) receives n: abn_tower_backward_loss's n_valid.  An index outside
 * [0, table_rows) reads as a zero row. */
int abn_gather_pairs(const float* table, int64_t table_rows, int64_t D, const int64_t* idx1, const int64_t* idx2,
                     int64_t first, int64_t n, int64_t n_pad, const void* labels,
                     int32_t label_bytes, float* x12, void* y_out, int32_t* n_valid, void* stream);

/* FeaturesGenerator.stack_fbanks, abnet3/features.py:135-159 */
int abn_stack_frames(const float* feats, int64_t T, int64_t D, int32_t nframes,
                     float* out, void* stream);
/* ... for a batch of utterances laid end to end in one [T, D] table (what the reference's
 * h5features_feats2stackedfeats loop does file by file, features.py:299-320): utt_frame_off =
 * cumulative frame counts, device int64 [n_utts + 1]; the window never crosses an utterance boundary. */
int abn_stack_frames_batched(const float* feats, const int64_t* utt_frame_off, int64_t n_utts,
                             int64_t T, int64_t D, int32_t nframes, float* out, void* stream);

/* FeaturesGenerator.mean_variance_normalisation / mean_var_norm_per_file,
 * abnet3/features.py:205-244, :263-297: mean = np.mean, std = np.std over axis 0
 * (per_channel: [D] outputs) or over everything (whole spectrum: [1] outputs),
 * then out = (x - mean) / (std + eps).  ws: abn_mvn_ws_bytes(T, D) bytes. */
int64_t abn_mvn_ws_bytes(int64_t T, int64_t D);
int abn_mvn_stats(const float* feats, int64_t T, int64_t D, int per_channel,
                  float* mean, float* stdv, void* ws, void* stream);
int abn_mvn_apply(const float* feats, int64_t T, int64_t D, const float* mean,
                  const float* stdv, int per_channel, float eps, float* out,
                  void* stream);

/* FeaturesGenerator.do_fbank, abnet3/features.py:99-114 (-> third-party
 * spectral.Spectral): int16 or fp32 mono samples -> [nframes, nfilt] log mel
 * energies (framing of that package's Sphinx-III lineage: a frame's pre-emphasis starts from the
 * last sample of the previous frame, a tail frame repeats its samples cyclically;
 * oracle/features_np.py).  melbank: [nfft/2+1, nfilt] fp32 weights (host side builds it,
 * abnet3_amd/features.py), window: [wlen] fp32.  band: [nfilt][2] int32 (device), first and
 * last bin with a non-zero weight of every filter; with it (and nfft = 1024, the
 * reference's value, nfilt <= 64) a frame is one wavefront's real-input FFT and a sparse mel
 * projection; NULL selects the general (any power-of-two nfft, dense projection) kernel. */
int abn_fbank(const void* samples, int sample_is_i16, int64_t nsamples,
              int32_t wlen, double fshift, int32_t nfft, int32_t nfilt,
              float alpha, const float* window, const float* melbank, const int32_t* band,
              int64_t nframes, float* out, void* stream);

/* ... for a batch of utterances in ONE launch (the reference's h5features_compute loop calls do_fbank
 * file by file, features.py:160-203): the utterances' samples laid end to end in `samples`,
 * utt_sample_off / utt_frame_off = cumulative sample / frame counts (device int64 [n_utts + 1],
 * frames of utterance u = int(len_u / fshift + 1)); out [nframes = utt_frame_off[n_utts], nfilt].
 * Every utterance is framed on its own, as if abn_fbank had been called on it alone. */
int abn_fbank_batched(const void* samples, int sample_is_i16, const int64_t* utt_sample_off,
                      const int64_t* utt_frame_off, int64_t n_utts, int32_t wlen, double fshift,
                      int32_t nfft, int32_t nfilt, float alpha, const float* window,
                      const float* melbank, const int32_t* band, int64_t nframes, float* out,
                      void* stream);

/* do_deltas / do_deltasdeltas of the same call (abnet3/features.py:110-111 -> spectral):
 * the slope over +-4 frames, out[t] = sum_{n=1..4} n (x[t+n] - x[t-n]) / 60, the sequence
 * padded with copies of frame 1 in front and of frame T-2 behind.  Apply twice for the
 * second-order deltas.  feats, out: [T, D] fp32, distinct buffers. */
int abn_deltas(const float* feats, int64_t T, int64_t D, float* out, void* stream);

/* ... for a batch of utterances laid end to end in ONE launch (ABI v20): utt_frame_off = cumulative frame
 * counts (device int64 [n_utts + 1], utt_frame_off[n_utts] = T); no slope crosses an utterance boundary, and
 * every utterance's rows are bit for bit what abn_deltas gives on that utterance alone.  feats and out are
 * [T, D] column slices of wider tables with row strides ld_in / ld_out (>= D, in floats): the slopes can be
 * written straight into their columns of the final table.  out may share rows with feats, never elements. */
int abn_deltas_batched(const float* feats, int64_t ld_in, const int64_t* utt_frame_off, int64_t n_utts,
                       int64_t T, int64_t D, float* out, int64_t ld_out, void* stream);

/* FeaturesGenerator.do_mfccs, abnet3/features.py:116-133 (-> spectral.Spectral with nfft=512, ncep=13,
 * lowerf=100, upperf=6855.4976, do_dct on) (ABI v20): abn_fbank's log mel energies, then the cepstra
 * out[t][i] = sum_f dct[i][f] logspec[t][f] for i < ncep.  dct: [ncep][nfilt] fp32 (device), built by the
 * host (abnet3_amd/features.py, dct_table: the Sphinx-III "legacy" DCT of spectral's lineage, 1/nfilt folded
 * in).  A window longer than nfft is cropped to its first nfft samples (what rfft(frame, nfft) does); the
 * pre-emphasis history of the next frame stays the frame's element wlen - 1.  band: as abn_fbank's, required.
 * out: [nframes, ncep] with row stride ld_out >= ncep (floats), so the cepstra can land in the first columns
 * of a table that also holds their deltas.  Kernel: abn_mfcc_path. */
int abn_mfcc(const void* samples, int sample_is_i16, int64_t nsamples, int32_t wlen, double fshift,
             int32_t nfft, int32_t nfilt, int32_t ncep, float alpha, const float* window,
             const float* melbank, const int32_t* band, const float* dct, int64_t nframes,
             float* out, int64_t ld_out, void* stream);

/* ... for a batch of utterances in ONE launch, with abn_fbank_batched's utterance tables. */
int abn_mfcc_batched(const void* samples, int sample_is_i16, const int64_t* utt_sample_off,
                     const int64_t* utt_frame_off, int64_t n_utts, int32_t wlen, double fshift,
                     int32_t nfft, int32_t nfilt, int32_t ncep, float alpha, const float* window,
                     const float* melbank, const int32_t* band, const float* dct, int64_t nframes,
                     float* out, int64_t ld_out, void* stream);

/* Which kernel abn_mfcc / abn_mfcc_batched take for these arguments (a pure query, no GPU needed);
 * -1 when the call would be refused (nfft not a power of two in [64, 2048], nfilt not in [1, 128],
 * ncep not in [1, nfilt]). */
enum {
    ABN_MFCC_GENERAL = 0,          /* one workgroup per frame, radix-2 FFT, dense mel projection */
    ABN_MFCC_WAVE512 = 1           /* nfft = 512 (the reference's value), nfilt <= 64: one wavefront per frame,
                                      radix-4 FFT, sparse mel projection, the DCT in the epilogue */
};
int abn_mfcc_path(int32_t nfft, int32_t nfilt, int32_t ncep);

/* k nearest neighbours by cosine similarity, for pair discovery (abnet3_amd/discovery.py writes the pairs file that
 * PairsDataLoader, abnet3/dataloader.py:355-546, reads; the program that wrote the reference's
 * test/data/dataloader/pairs_knn.txt is not part of it) (added within ABI 20, backward compatible).
 * Q [nq][d], C [nc][d]: row-major fp32, rows L2-normalised by the caller, 16-byte aligned; sim(i, j) = <Q_i, C_j>,
 * accumulated in fp32 on the matrix cores (v_mfma_f32_32x32x2_f32, k ascending).  q_meta / c_meta: int32 [n][3] =
 * file, begin, end per row, or NULL; when BOTH are given candidate j is excluded for query i if the files are equal
 * and the half-open intervals intersect (b_i < e_j && b_j < e_i) -- which covers i == j when Q and C are one table.
 * idx / sim [nq][k]: the k non-excluded candidates of largest sim, by descending sim, ties by ascending j; unused
 * places hold idx = -1, sim = -inf.  1 <= k <= 32, d a multiple of 4 in [4, 4096]: anything else is
 * ABN_E_UNSUPPORTED (ABN_E_ARG for null pointers and sizes < 1), before any launch.  The nq x nc similarities are
 * never written to memory; the candidates of a query block are split over several workgroups (ABN_KNN_SPLIT, or by
 * the grid) whose partial lists go through ws (abn_knn_ws_bytes; 0 bytes when the split is 1) and are merged by the
 * same order, so the output is bit-identical for any split. */
int64_t abn_knn_ws_bytes(int64_t nq, int64_t nc, int k);      /* host; -1 for sizes abn_knn_topk refuses */
int abn_knn_topk(const float* Q, int64_t nq, const float* C, int64_t nc, int d,
                 const int32_t* q_meta, const int32_t* c_meta, int k, int32_t* idx, float* sim,
                 void* ws, int64_t ws_bytes, void* stream);

/* The segment vectors abn_knn_topk searches: segment g covers rows seg_row0[g] .. + seg_len[g] - 1 of table
 * [rows][D]; its vector is the K rows seg_row0[g] + ((2j + 1) seg_len[g]) / (2K), j = 0 .. K - 1, concatenated to
 * K D floats and scaled to unit L2 norm (sum of squares in float64, scale applied in fp32).  out [nseg][K D];
 * keep [nseg] bytes: 0 where the segment is all zero (its vector is then zero and the caller leaves it out).
 * seg_row0: device int64, seg_len: device int32; the caller guarantees that every segment lies inside the table. */
int abn_segment_vectors(const float* table, int64_t D, const int64_t* seg_row0, const int32_t* seg_len,
                        int64_t nseg, int K, float* out, uint8_t* keep, void* stream);

/* Pair sampling from word clusters (abnet3/sampler.py:404-688 without its K^2 table; added within ABI 20, backward
 * compatible).  A CELL is a (speaker, word type) with at least one token.  The tables are O(cells + tokens) and
 * hold the cells twice, sorted by (type, speaker) -- "T order" -- and by (speaker, type) -- "S order"; all weights
 * are integers (abnet3_amd/sampler.py builds them and states what they quantise):
 *   u = g(tokens of the type) f(tokens of the cell), sum over all cells < 2^32;  f = f(tokens of the cell),
 *   sum over the cells of any one type < 2^32.
 * cum_* are INCLUSIVE running sums over the whole order.  cum_m[q] is the running sum of configuration q's
 * first-cell marginal (q = 0, 1 in T order, q = 2, 3 in S order), total[q] its last entry (0: empty support):
 *   0 Stype_Sspk  u [tokens >= 2]                        2 Dtype_Sspk  u (U_speaker - u)
 *   1 Stype_Dspk  u (F_type - f)                         3 Dtype_Dspk  u (U - U_speaker - U_type + u)
 * All pointers are device pointers. */
typedef struct abn_sampler_tables {
    int32_t n_cells, n_spk, n_type, n_tok;
    uint64_t total[4];
    /* T order */
    const int32_t* spk_t;      /* [n_cells] speaker index */
    const int32_t* type_t;     /* [n_cells] type index */
    const int32_t* type_beg;   /* [n_type + 1] first cell of each type */
    const uint32_t* f_t;       /* [n_cells] */
    const uint64_t* cum_u_t;   /* [n_cells] */
    const uint64_t* cum_f_t;   /* [n_cells] */
    const int32_t* tok_beg;    /* [n_cells + 1] first token of each cell in toks */
    const int32_t* toks;       /* [n_tok] token ids, cell after cell */
    /* S order */
    const int32_t* spk_s;      /* [n_cells] */
    const int32_t* type_s;     /* [n_cells] */
    const int32_t* s2t;        /* [n_cells] the cell's index in T order */
    const int32_t* spk_beg;    /* [n_spk + 1] first cell of each speaker */
    const uint32_t* u_s;       /* [n_cells] */
    const uint64_t* cum_u_s;   /* [n_cells] */
    const uint64_t* cum_spk;   /* [n_spk] running sum of the speakers' totals of u */
    const uint64_t* cum_m;     /* [4][n_cells] */
} abn_sampler_tables;

/* Draws n[q] pairs of configuration q = 0 .. 3 in ONE launch, one lane per pair; pair i of configuration q is
 * element n[0] + .. + n[q-1] + i of tok1 / tok2 (int32 token ids; -1 where total[q] == 0) and of key (a 63-bit
 * shuffle key: the caller orders the lines by ascending key, ties by index).  Every random number is
 * Philox4x32-10 with key (seed low, seed high) and counter (i low, i high, q, slot): slot 0 the first cell, 1 the
 * second cell, 2 the two tokens, 3 the shuffle key -- the output does not depend on `block`, the workgroup size (a
 * multiple of 64 in 64 .. 1024).  A 128-bit draw r is mapped onto a range M < 2^64 as floor(r M / 2^128); the
 * first cell comes from cum_m[q], the second by binary searches in the running sums with the excluded cell /
 * speaker / type cut out (no rejection, every loop is a binary search).  Different-type pairs come lower type
 * index first.  ABN_E_ARG before any launch for null pointers, sizes out of range (1 <= n_cells < 2^24,
 * n[q] >= 0, sum n < 2^31) or a bad `block`. */
int abn_sample_pairs(const abn_sampler_tables* tables, const int64_t* n, uint64_t seed, int32_t* tok1,
                     int32_t* tok2, int64_t* key, int block, void* stream);

/* ---- temporal-coherence pairs (abnet3/dataloader.py:324-352; added within ABI 20) -------------------------------
 * Draws the temporal-coherence pairs of a pass in ONE launch, one lane per iteration, into the index arrays of a
 * batch plan.  Iteration i = 0 .. n_iter - 1 draws a file f uniformly among n_files -- file f = rows
 * file_row0[f] .. file_row0[f] + file_len[f] - 1 of the corpus table -- and a frame t uniformly in
 * [0, file_len[f] - max(deltas)), and writes n_deltas consecutive elements from dst[i] on (n_deltas * i when dst is
 * NULL):  idx1 = file_row0[f] + t,  idx2 = file_row0[f] + t + deltas[j],  labels = +1 for j < n_same, -1 after --
 * int64, or float64 when labels_f64 is not 0.  An iteration whose elements would not lie inside [0, out_len), the
 * length of idx1 / idx2 / labels, writes nothing.
 * The draw is one Philox4x32-10 call with key (seed low, seed high) and counter (g low, g high, epoch, 'TCL1' =
 * 0x54434C31), g = first_iter + i the iteration's index in the whole pass: a rank's share, launched with its
 * first_iter, reproduces its slice of the single-process pass.  Words 0, 1 of the output, as a 64-bit r, give
 * f = floor(r n_files / 2^64); words 2, 3 give t the same way.  Integer arithmetic only, no rejection.
 * file_row0 / file_len / dst / idx1 / idx2 / labels are device pointers; deltas (n_deltas values) and
 * file_len_host (the n_files values of file_len) are HOST arrays read during the call.  ABN_E_ARG before any
 * launch for n_files < 1, n_deltas outside 1 .. 16, n_same outside 0 .. n_deltas, a negative delta, a file with
 * file_len <= max(deltas), negative counts, null pointers, or (dst NULL) n_deltas * n_iter > out_len.
 * n_iter == 0 launches nothing. */
int abn_tcl_pairs(const int64_t* file_row0, const int64_t* file_len, const int64_t* file_len_host,
                  int64_t n_files, const int32_t* deltas, int n_deltas, int n_same, int64_t n_iter,
                  int64_t first_iter, uint64_t seed, uint32_t epoch, const int64_t* dst, int64_t* idx1,
                  int64_t* idx2, void* labels, int labels_f64, int64_t out_len, void* stream);

/* ---- Gaussian-mixture posteriorgrams (no counterpart in the reference; added within ABI 20) ----------------------
 * A diagonal-covariance mixture of K components over D-dimensional frames, as abnet3_amd/gmm.py defines it.  The
 * model reaches the kernels as three fp32 score tables (m = mean - shift, v = variance, w = weight):
 *   A [K][D] = m / v,   B [K][D] = -0.5 / v,   c [K] = log w - 0.5 sum_d (log(2 pi v) + m^2 / v),
 * and the frames x [T][D] are centred on load, xc = x - shift in fp32.  The score
 *   s[t][k] = c[k] + sum_d xc A + sum_d xc^2 B
 * is one fp32 GEMM of depth 2 D + 1 on the matrix cores (v_mfma_f32_32x32x2_f32, the augmented row
 * [xc | xc^2 | 1] formed on the way into LDS, columns in that order).  lse[t] = log sum_k exp s[t][k]; a frame with
 * a non-finite xc^2 is BAD: lse[t] = NaN, its posteriors are 0, it adds nothing to the statistics.
 * D <= abn_gmm_max_d(), K <= abn_gmm_max_k(): beyond them ABN_E_UNSUPPORTED; T < 2^31 - 128; null pointers and
 * sizes < 1 are ABN_E_ARG -- all before any launch.  No floating-point atomics: every call is bit-reproducible. */
int64_t abn_gmm_max_d(void);               /* host */
int64_t abn_gmm_max_k(void);               /* host */

/* lse [T]; post [T][K] = exp(s - lse), or NULL for the likelihoods alone.  One launch; the T x K matrix is written
 * here and nowhere else. */
int abn_gmm_posteriors(const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                       const float* c, int64_t K, float* lse, float* post, void* stream);

/* Sufficient statistics N[k] = sum_t g, S1[k][d] = sum_t g xc, S2[k][d] = sum_t g xc^2 with g = exp(s - lse[t])
 * recomputed tile by tile from lse (abn_gmm_posteriors' output for the same tables), never stored.  A workgroup owns
 * 128 components and one of n_ranges ranges of 128-frame blocks (0: chosen from the grid, at most 256) and leaves
 * one fp32 slab [128][2 D + 1] in ws (abn_gmm_ws_bytes, host, -1 for refused sizes).  One launch. */
int64_t abn_gmm_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges);
int abn_gmm_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* A, const float* B,
                       const float* c, int64_t K, const float* lse, int n_ranges, void* ws, int64_t ws_bytes,
                       void* stream);

/* Sums the slabs of abn_gmm_accumulate (same T, K, D, n_ranges) in range order in float64 into
 * sums [K][2 D + 1] = [S1 | S2 | N], then the M-step in float64 with Tg = T - (BAD frames):
 *   w = N / Tg, renormalised to sum 1;  m = S1 / N;  v = max(S2 / N - m^2, var_floor gv[d]);
 * a component with N < min_count keeps its mu / var.  w [K], mu [K][D] (centred means), var [K][D]: float64, mu and
 * var in / out; A, B, c: the next tables, rounded once from float64; gv [D] float64.
 * stats [4] float64: sum of lse over the good frames, BAD frames, starved components, Tg.  Two small launches. */
int abn_gmm_mstep(const void* ws, int64_t ws_bytes, const float* lse, int64_t T, int64_t K, int64_t D, int n_ranges,
                  const double* gv, double var_floor, double min_count, double* sums, double* w, double* mu,
                  double* var, float* A, float* B, float* c, double* stats, void* stream);

/* ---- k-means discrete units (no counterpart in the reference; added within ABI 20) ---------------------------------
 * K centroids over D-dimensional frames, as abnet3_amd/kmeans.py defines it.  The model reaches the kernels as two
 * fp32 tables, m [K][D] = centroid - shift and b [K] = -|m|^2 / 2 (0 for spherical k-means, whose caller passes unit
 * rows and a zero shift); the frames x [T][D] are centred on load, xc = x - shift in fp32.  The score
 *   s[t][k] = sum_d xc m + b[k]
 * is one fp32 GEMM of depth D + 1 on the matrix cores (v_mfma_f32_32x32x2_f32, the augmented row [xc | 1] formed on
 * the way into LDS), and ids[t] = argmax_k s, equal scores to the lowest k; a frame with a non-finite xc^2 is BAD:
 * ids[t] = -1, it adds nothing to the statistics.
 * D <= abn_kmeans_max_d(), K <= abn_kmeans_max_k(): beyond them ABN_E_UNSUPPORTED; T < 2^31 - 128; n_ranges 0 .. 1024;
 * null pointers and sizes < 1 are ABN_E_ARG -- all before any launch.  No floating-point atomics: every call is
 * bit-reproducible. */
int64_t abn_kmeans_max_d(void);            /* host */
int64_t abn_kmeans_max_k(void);            /* host */

/* ids [T] int32; best [T] = the winning score (NaN for a BAD frame), or NULL.  With prev_ids [T] (which may be ids
 * itself) the number of frames whose id differs from it is ADDED to *changed (int32, device; the caller zeroes it).
 * One launch; no T x K array. */
int abn_kmeans_assign(const float* x, int64_t T, int64_t D, const float* shift, const float* m, const float* b,
                      int64_t K, const int32_t* prev_ids, int32_t* ids, float* best, int32_t* changed, void* stream);

/* Partial statistics of the hard assignment ids (an id outside 0 .. K - 1 is skipped): per range of 128-frame blocks
 * (n_ranges, 0: chosen from the grid) and centroid the count (int32) and the fp32 sum of xc over its frames in frame
 * order, and partial sums (float64) of the frames' distortions |xc - m[ids[t]]|^2, formed directly.  A memory-bound
 * pass: every row of x is loaded once.  ws: abn_kmeans_ws_bytes (host, -1 for refused sizes), 16-byte aligned.
 * One launch. */
int64_t abn_kmeans_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges);
int abn_kmeans_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* m, int64_t K,
                          const int32_t* ids, int n_ranges, void* ws, int64_t ws_bytes, void* stream);

/* Sums the partials of abn_kmeans_accumulate (same T, K, D, n_ranges, ids) in range order in float64 into
 * sums [K][D + 1] = [S | N] and stats [4] float64: sum of the distortions, BAD frames, empty centroids, good frames.
 * Then the update in float64: mu [K][D] (centred centroids, in / out) = S / N, a centroid with N = 0 keeps its mu;
 * cosine != 0 renormalises each new mu to unit length; m, b: the next tables, rounded once (b from the rounded m).
 * mu, m and b all NULL: the statistics alone.  Two small launches. */
int abn_kmeans_update(const void* ws, int64_t ws_bytes, const int32_t* ids, int64_t T, int64_t K, int64_t D,
                      int n_ranges, int cosine, double* sums, double* mu, float* m, float* b, double* stats,
                      void* stream);

/* ---- penalised unit segmentation (added within ABI 20) ---------------------------------------------------------------
 * The same scores s[t][k], smoothed by a constant cost per change of unit (abnet3_amd/kmeans.py states the recurrence):
 * utterance u is the len[u] rows from off[u] (off int64, len int32, device arrays; utterances must not overlap: each
 * is written by a workgroup of its own); over its good frames the ids
 * maximise  sum_t s[t][a_t] - penalty_score * #{changes}, penalty_score = penalty / 2 for a penalty in units of the
 * distortion |xc - m|^2.  BAD frames keep id -1 and cost nothing; rows outside every utterance keep what ids held.
 * objective [n_utt] float64 and n_switch [n_utt] int32 may be NULL.  penalty_score = 0 gives abn_kmeans_assign's ids.
 * One launch of persistent workgroups; fp32 recurrence, bit-reproducible; no T x K array: the workspace holds, per
 * workgroup (at most 256), a 128-frame slab of scores, one stay bit per (frame, centroid) and an int32 per frame of
 * the longest utterance.  An utterance that does not lie in 0 .. T, or is longer than the workspace was sized for,
 * is left untouched: objective NaN, n_switch -1.
 * abn_kmeans_viterbi_ws_bytes: -1 (abn_last_error) for refused sizes; max_len 0 .. abn_kmeans_viterbi_max_len(),
 * K <= abn_kmeans_viterbi_max_k(), D <= abn_kmeans_max_d().  Null pointers, sizes < 1, a negative or non-finite
 * penalty_score: ABN_E_ARG; limits: ABN_E_UNSUPPORTED; a workspace too small for one frame: ABN_E_WORKSPACE -- all
 * before any launch. */
int64_t abn_kmeans_viterbi_max_len(void);  /* host */
int64_t abn_kmeans_viterbi_max_k(void);    /* host */
int64_t abn_kmeans_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);
int abn_kmeans_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                       const float* shift, const float* m, const float* b, int64_t K, float penalty_score,
                       int32_t* ids, double* objective, int32_t* n_switch, void* ws, int64_t ws_bytes, void* stream);

/* ---- sticky-HMM posteriorgram smoothing (added within ABI 20) --------------------------------------------------------
 * Forward-backward of the HMM over a mixture's K components with one stay probability (abnet3_amd/hmm.py states the
 * recursion): initial distribution w, transitions a[j][k] = rho [j == k] + (1 - rho) w[k], emissions
 * logN[t][k] = c0[k] + sum_d xc A + sum_d xc^2 B -- abn_gmm_posteriors' score with c0 = c without the log weight.
 * Utterance u is the len[u] rows from off[u] (off int64, len int32, device arrays; utterances must not overlap).
 * post [T][K] fp32: mode 0 the smoothed gamma, mode 1 the filtered ahat (no backward sweep); a BAD frame's row is all
 * zeros and the chain passes over it; rows outside every utterance are not touched.  loglik [n_utt] float64 (the sum
 * over the good frames), stays [n_utt] float64 (the expected number of stays; may be NULL; 0 in mode 1), n_good [n_utt]
 * int32.  An utterance that does not lie in 0 .. T, or is longer than the workspace was sized for, is left
 * untouched: loglik (and stays) NaN, n_good -1.
 * One launch of persistent workgroups; fp32 recursion with fixed reduction orders, bit-reproducible, no atomics; no
 * T x K array beyond post, which holds ahat between the sweeps: the workspace holds, per workgroup (at most 256), a
 * 128-frame slab of scores and one float per frame of the longest utterance.
 * abn_hmm_ws_bytes: -1 (abn_last_error) for refused sizes; max_len 0 .. abn_hmm_max_len(), K <= abn_hmm_max_k()
 * (= abn_gmm_max_k()), D <= abn_gmm_max_d().  Null pointers, sizes < 1, rho outside [0, 1) or non-finite, a mode other
 * than 0 / 1: ABN_E_ARG; limits: ABN_E_UNSUPPORTED; a workspace too small for one frame: ABN_E_WORKSPACE -- all before
 * any launch.  The caller keeps float32(1 - rho) * min{w > 0} >= 2^-100 (abnet3_amd/hmm.py refuses otherwise). */
int64_t abn_hmm_max_len(void);             /* host */
int64_t abn_hmm_max_k(void);               /* host */
int64_t abn_hmm_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);
int abn_hmm_forward_backward(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                             const float* shift, const float* A, const float* B, const float* c0, const float* w,
                             int64_t K, float rho, int mode, float* post, double* loglik, double* stays,
                             int32_t* n_good, void* ws, int64_t ws_bytes, void* stream);

/* ---- Baum-Welch statistics of the sticky HMM (added within ABI 20) ----------------------------------------------------
 * abn_hmm_forward_backward_stats: abn_hmm_forward_backward with one more output.  post, loglik, stays and n_good are the
 * same bits for the same inputs; stay_k [n_utt][K] float64 holds the per-component terms of stays,
 *   stay_k[u][k] = sum over the transitions (p -> t) of utterance u of rho ahat_p[k] e_t[k]
 * (fp32 sums over a block of 128 frames, float64 across the blocks, in one fixed order: per utterance, independent of the
 * grid and of the other utterances, no atomics).  Mode 1, an utterance with fewer than two good frames and a component of
 * weight 0 give zeros; a refused utterance a row of NaN.  stay_k must not be null; everything else as above.
 * abn_hmm_accumulate: sums [K][2 D + 1] float64 = [S1 | S2 | N], sum over the rows t of post[t][k] [xc | xc^2 | 1] with
 * abn_gmm_accumulate's fp32 xc = x - shift and xc^2 -- the second GEMM of that kernel on the fp32 matrix cores, its A
 * operand read from post [T][K] (fp32, once: T K 4 bytes) instead of recomputed.  A non-finite x entry contributes 0
 * (never 0 x NaN); the caller's table has zero rows at BAD frames (abn_hmm_forward_backward writes them).  One fp32 slab
 * [128][2 D + 1] per (128-component tile, frame range) in ws, then summed in range order in float64: two launches, no
 * atomics, bit-reproducible for a given n_ranges (0: chosen from the grid).  ws: abn_hmm_accumulate_ws_bytes (-1 for
 * refused sizes).  Null pointers, sizes < 1, n_ranges outside 0 .. 256: ABN_E_ARG; K > abn_hmm_max_k(),
 * D > abn_gmm_max_d(), T >= 2^31 - 128: ABN_E_UNSUPPORTED; a short workspace: ABN_E_WORKSPACE -- all before any launch. */
int abn_hmm_forward_backward_stats(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len,
                                   int64_t n_utt, const float* shift, const float* A, const float* B, const float* c0,
                                   const float* w, int64_t K, float rho, int mode, float* post, double* loglik,
                                   double* stays, int32_t* n_good, double* stay_k, void* ws, int64_t ws_bytes,
                                   void* stream);
int64_t abn_hmm_accumulate_ws_bytes(int64_t T, int64_t K, int64_t D, int n_ranges);
int abn_hmm_accumulate(const float* x, int64_t T, int64_t D, const float* shift, const float* post, int64_t K,
                       int n_ranges, double* sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- Viterbi decoding of the sticky HMM (added within ABI 20) ----------------------------------------------------------
 * The max-product path of the same model (abnet3_amd/hmm.py states the recurrence): the best state sequence of every
 * utterance under initial distribution w, transitions rho [j == k] + (1 - rho) w[k] and abn_hmm_forward_backward's
 * emissions logN[t][k].  The kernel takes no logarithm: lw = log w, ls = log(rho + (1 - rho) w), lr = log((1 - rho) w),
 * each [K] fp32 (hmm.viterbi_tables; lw = lr = -inf for a component of weight 0, which is then never chosen; the caller
 * keeps lr <= ls).  Over the good frames, fp32, every operation one rounded add or a compare:
 *   first: u = logN + lw;  later: a = W + ls, stay = a > lr (a tie switches), u = logN + (stay ? a : lr);
 *   M = max_k u at its lowest index j*,  W = u - M,  log_prob += M (float64).
 * ids [T] int32: the path; a BAD frame gets -1 and the chain passes over it; rows outside every utterance keep what ids
 * held.  log_prob [n_utt] float64 (the log joint probability of the path and the good frames), n_switch [n_utt] int32
 * (changes of id between consecutive good frames) and n_good [n_utt] int32 may each be NULL.  An utterance that does not
 * lie in 0 .. T, or is longer than the workspace was sized for, is left untouched: log_prob NaN, n_switch and n_good -1.
 * One launch of persistent workgroups, abn_kmeans_viterbi's shape: bit-reproducible, independent of the grid, no atomics,
 * no T x K array: the workspace holds, per workgroup (at most 256), a 128-frame slab of scores, one stay bit per
 * (frame, component) and an int32 per frame of the longest utterance.
 * abn_hmm_viterbi_ws_bytes: -1 (abn_last_error) for refused sizes; max_len 0 .. abn_hmm_max_len(), K <= abn_hmm_max_k(),
 * D <= abn_gmm_max_d().  Null pointers, sizes < 1: ABN_E_ARG; limits: ABN_E_UNSUPPORTED; a workspace too small for one
 * frame: ABN_E_WORKSPACE -- all before any launch. */
int64_t abn_hmm_viterbi_ws_bytes(int64_t n_utt, int64_t max_len, int64_t K, int64_t D);
int abn_hmm_viterbi(const float* x, int64_t T, int64_t D, const int64_t* off, const int32_t* len, int64_t n_utt,
                    const float* shift, const float* A, const float* B, const float* c0,
                    const float* lw, const float* ls, const float* lr, int64_t K,
                    int32_t* ids, double* log_prob, int32_t* n_switch, int32_t* n_good,
                    void* ws, int64_t ws_bytes, void* stream);

/* ---- embedded segmental k-means (added within ABI 20) ----------------------------------------------------------------
 * Full-coverage word segmentation (abnet3_amd/eskmeans.py states the definitions).  Landmarks: lm [n_lm] int64 row
 * indices into table [T][D]; utterance u owns lm[lm_off[u] .. lm_off[u + 1]) (lm_off [n_utt + 1] int64), at least two
 * entries, strictly increasing, the first its first row and the last one past its last row.  The candidate (g, s),
 * 1 <= s <= S, runs from landmark g to g + s inside one utterance, covers rows lm[g] .. lm[g + s] - 1 (n of them), lives
 * at index g S + s - 1 and is allowed if s == 1 or n <= max_frames.  All arrays are device arrays.
 *
 * abn_esk_score: cand_best [n_lm S] fp32 and cand_id [n_lm S] int32 = the best score <v, m_k> + b_k and the lowest k
 * attaining it, v the candidate's unit vector exactly as abn_segment_vectors forms it (`frames` sampled rows, sum of
 * squares in float64, scale in fp32), scored exactly as abn_kmeans_assign scores a row of depth frames D under a zero
 * shift (m [K][frames D], b [K]): the same bits, but no candidate table is formed -- the rows are gathered on the way
 * into LDS.  A candidate that crosses an utterance, is not allowed, lies outside 0 .. T, is longer than
 * INT_MAX / (2 frames) rows, is all zero or has a non-finite sampled value: id -1, best NaN.
 * frames D <= abn_kmeans_max_d(), K <= abn_kmeans_max_k(), S <= abn_esk_max_span(): beyond them ABN_E_UNSUPPORTED;
 * null pointers, sizes < 1, n_lm < 2, n_lm S >= 2^31 - 128: ABN_E_ARG -- all before the launch.  One launch, no
 * workspace, no floating-point atomics: bit-reproducible.
 *
 * abn_esk_segment: per utterance with L = (its landmarks) - 1, in fp32,
 *   c(g, s) = (float)n * (1.0f - 2.0f * best)  (each operation rounded once; +inf where id < 0),
 *   gamma[0] = 0,  gamma[j] = min_s gamma[j - s] + c(j - s, s),  equal sums to the smallest s,
 * and the traceback from L: cut [n_lm] uint8 = 1 at every chosen boundary (first and last included), word [n_lm] int32 =
 * the segment's cluster id and span [n_lm] int32 = its span at every chosen start, both -1 elsewhere; objective [n_utt]
 * float64 = gamma[L] and n_seg [n_utt] int32 (either may be NULL).  An utterance whose end cannot be reached: objective
 * NaN, n_seg -1, nothing marked.  One launch, one wavefront per utterance.  S <= abn_esk_max_span(): beyond it
 * ABN_E_UNSUPPORTED; null pointers and sizes < 1: ABN_E_ARG. */
int64_t abn_esk_max_span(void);            /* host */
int abn_esk_score(const float* table, int64_t T, int64_t D, const int64_t* lm, const int64_t* lm_off, int64_t n_utt,
                  int64_t n_lm, int frames, int S, int64_t max_frames, const float* m, const float* b, int64_t K,
                  float* cand_best, int32_t* cand_id, void* stream);
int abn_esk_segment(const float* cand_best, const int32_t* cand_id, const int64_t* lm, const int64_t* lm_off,
                    int64_t n_utt, int64_t n_lm, int S, uint8_t* cut, int32_t* word, int32_t* span, double* objective,
                    int32_t* n_seg, void* stream);

/* ---- same-different word discrimination (added within ABI 20) --------------------------------------------------------
 * Every pair i < j of the n rows of X [n][d] (row-major fp32, 16-byte aligned; unit rows for a cosine), scored behind
 * the tile that forms its similarity (abnet3_amd/samediff.py states the task and its scores).  sim(i, j) = <X_i, X_j>
 * is accumulated exactly as abn_knn_topk accumulates it (v_mfma_f32_32x32x2_f32, k ascending, 128 x 128 tiles at
 * multiples of 128): the same bits there, in abn_sd_collect and in abn_sd_count.  Only tiles on or above the diagonal
 * are formed and the n x n matrix is never written.
 * The rows are sorted by word type: row i carries the half-open range [cbeg[i], cend[i]) of its type (int32, device;
 * cbeg[i] <= i < cend[i] <= n, equal for all rows of the range -- the caller guarantees it; the kernels read cend
 * only, because j > i >= cbeg[i]).  The pair (i, j) is of one type when j < cend[i].
 * d a multiple of 4 in [4, 4096], n <= ABN_SD_MAX_N, n_thr <= ABN_SD_MAX_THR: anything else is ABN_E_UNSUPPORTED;
 * null pointers, n < 1, n_thr < 0, an unknown condition or a speaker condition without spk are ABN_E_ARG -- all before
 * any launch.  ABN_SD_TILES (1 .. 4096; unset or 0: chosen from the grid) sets the column tiles per workgroup; the
 * results do not depend on it.
 *
 * abn_sd_collect: writes sim(i, j) of every same-type pair to pos_sim[pos_off[i] + (j - i - 1)] (pos_off [n] int64,
 * device; the caller sizes pos_sim as the sum over types of n_c (n_c - 1) / 2 and lays the rows out without gaps).
 * One launch; column tiles past the end of a row block's last type are skipped.
 *
 * abn_sd_count: hist [n_thr + 1] and n_bad [1] (uint64, device) are cleared by the call.  thr [n_thr]: fp32,
 * descending (NULL when n_thr == 0).  A same-type pair is left out when condition is ABN_SD_SWDP and
 * spk[i] == spk[j], or ABN_SD_SWSP and spk[i] != spk[j] (spk [n] int32, device; may be NULL under ABN_SD_ALL).
 * Of the others, a pair whose similarity is NaN or +-inf adds 1 to n_bad and nothing else; every other pair adds 1 to
 * hist[#{r : thr[r] > sim}].  Integer atomics only: the counts are the same for any grid. */
#define ABN_SD_MAX_N (1 << 22)
#define ABN_SD_MAX_THR (1 << 30)
enum { ABN_SD_ALL = 0, ABN_SD_SWDP = 1, ABN_SD_SWSP = 2 };
int64_t abn_sd_grid_runs(int64_t n);       /* host: the grid's x extent (runs of column tiles per row block) for n rows
                                              under the current ABN_SD_TILES; -1 for an n the kernels refuse */
int abn_sd_collect(const float* X, int64_t n, int d, const int32_t* cbeg, const int32_t* cend,
                   const int64_t* pos_off, float* pos_sim, void* stream);
int abn_sd_count(const float* X, int64_t n, int d, const int32_t* cbeg, const int32_t* cend, const int32_t* spk,
                 int condition, const float* thr, int64_t n_thr, uint64_t* hist, uint64_t* n_bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ABNET3_HIP_H */
