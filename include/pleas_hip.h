/*
 * pleas_hip.h -- C ABI of libpleas_hip.so: the MI355X (gfx950) kernels behind the
 * PLeaS activation-matching + least-squares merging hot path.
 *
 * Conventions (all entry points):
 *   - plain C types only; every data pointer is a DEVICE pointer borrowed for the
 *     duration of the call unless marked HOST; nothing is retained after return;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and the call returns without synchronising;
 *   - no hidden device allocation: scratch comes from a caller-sized workspace
 *     (`*_ws_bytes` tells how much);
 *   - return value: 0 on success, negative PLEAS_E* on error; never throws.
 *
 * The reference has no native code: each entry point replaces the
 * vendor-library kernels that the cited reference Python line dispatches to.
 */
#ifndef PLEAS_HIP_H
#define PLEAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLEAS_OK 0
#define PLEAS_EINVAL (-22)   /* bad argument (shape, null pointer, unsupported size) */
#define PLEAS_ENOMEM (-12)   /* workspace too small */
#define PLEAS_EHIP (-5)      /* a HIP runtime call failed (see pleas_last_error) */

/* Library / build identification: "pleas_hip <version> gfx950". */
const char* pleas_version(void);
/* Text of the last HIP error seen by this thread's calls ("" if none). */
const char* pleas_last_error(void);

/* ------------------------------------------------------------------------------------
 * Cross features: Gram / negative Euclidean distance between the channels of two
 * activation (or weight) tensors, accumulated into a C x C matrix.
 *
 * Replaces: pleas/methods/activation_matching.py:31-46 (cross_features_cdist:
 *   movedim+reshape copies, torch.cdist mm-path) and :14-28 (cross_features_inner_product),
 *   plus the per-batch / per-node accumulation at :123-127 and :129-134.
 *
 * x, y: contiguous fp32 tensors viewed as [B][C][HW] (for NCHW activations: B = batch,
 *   HW = H*W; for axis `a` of any contiguous tensor: B = prod(shape[:a]), C = shape[a],
 *   HW = prod(shape[a+1:])).  The contraction runs over all (b, hw).
 * epilogue: PLEAS_EPI_INNER  -> v = sum_k x_ik y_jk
 *           PLEAS_EPI_NEG_CDIST -> v = -sqrt(max(0, |x_i|^2 + |y_j|^2 - 2 sum_k x_ik y_jk))
 * accumulate: 0 -> acc = v ; 1 -> acc += v           (acc: C x C fp32, row-major)
 * ws: workspace of at least pleas_gram_ws_bytes(B, C, HW) bytes.
 * Deterministic: a fixed (B, C, HW) always reduces in the same order.
 */
#define PLEAS_EPI_INNER 0
#define PLEAS_EPI_NEG_CDIST 1
size_t pleas_gram_ws_bytes(int B, int C, int64_t HW);
int pleas_gram_accum(const float* x, const float* y, int B, int C, int64_t HW, int epilogue, int accumulate,
                     float* acc, void* ws, size_t ws_bytes, void* stream);
/* Host only (no GPU): the plan pleas_gram_accum makes for a shape, given whether both operands are 16-byte aligned:
 * info[0] tile (64 / 128), [1] floats per load (4 / 1), [2] S, the split-K slabs, [3] chunks of 32 k per slab.  Shapes the
 * launch refuses are refused with the same message. */
int pleas_gram_plan_info(int B, int C, int64_t HW, int aligned, int* info);

/* Grouped form: ALL tracked nodes of one batch in one contraction grid plus one reduce grid.
 *
 * Replaces one whole iteration of the hot loop at activation_matching.py:120-127 plus the
 * per-group sum at :129-134: node i contributes epilogue(x_i, y_i) to the matrix of its group.
 * nodes[i]      : HOST array; x, y as in pleas_gram_accum ([B][C][HW] views), group index
 * group_acc[g]  : DEVICE C_g x C_g fp32 matrices (HOST array of pointers); group_C[g] HOST sizes
 * accumulate    : 0 -> group matrices are overwritten by this batch's sum, 1 -> added to
 * Work is cut into (node, tile, K-range) items of near-equal length, sorted longest first; each
 * node's partial products go to its own slab in `ws`, and the reduce grid sums slabs and nodes in a
 * FIXED order (deterministic, no atomics).  ws >= pleas_gram_batch_ws_bytes(...).
 * The work list is cached per (shape sequence, ws, group matrices) and its device tables live at the
 * start of `ws`: pass ws_fresh = 1 on the first call with a workspace (or whenever its content may
 * have been overwritten since the previous call), 0 otherwise; then only operand pointers are sent.
 */
typedef struct pleas_gram_node {
    const float* x;
    const float* y;
    int B;
    int C;
    int64_t HW;
    int group;
    /* Derived node (derived != 0): its operands are per-channel affine images of node `source`'s operands,
     *   x' = scale_x[c] * x + shift_x[c],  y' = scale_y[c] * y + shift_y[c]   (DEVICE arrays of length C)
     * -- an eval-mode BatchNorm of a tracked convolution output.  Its inner products and norms follow from the
     * source's products, squared norms and row sums, so it is NOT contracted: x / y are ignored, `source` must be a
     * contracted node of the same shape in this list.  Zero-initialised fields = an ordinary node. */
    int derived;
    int source;
    const float* scale_x;
    const float* shift_x;
    const float* scale_y;
    const float* shift_y;
} pleas_gram_node;
size_t pleas_gram_batch_ws_bytes(const pleas_gram_node* nodes, int n_nodes, const int* group_C, int n_groups);
/* Host only (no GPU, pointers may be NULL except a derived node's scale / shift): what the plan builder of pleas_gram_batch
 * decides, six ints per node: [0] the tile form `variant` (0: 128-row tiles, 16-byte loads; 1: 128, 4-byte loads; 2 / 3: the
 * same with 64 rows; 4 / 5: 128 / 64 rows on the K axis padded to four pixels per group, HW % 4 != 0 and HW >= 4), [1] S, the
 * slabs of the K axis (0 for a derived node), [2] chunks of 32 k per slab, [3] tiles per side, [4] HWp, the pixels per sample
 * on the K axis (HW outside the padded forms), [5] 1 when the node also writes row sums (a derived node's source).  A list
 * the launch refuses is refused with the same message.  Returns 0 or a negative error code. */
int pleas_gram_batch_plan_info(const pleas_gram_node* nodes, int n_nodes, const int* group_C, int n_groups, int* info);
int pleas_gram_batch(const pleas_gram_node* nodes, int n_nodes, float* const* group_acc, const int* group_C,
                     int n_groups, int epilogue, int accumulate, void* ws, size_t ws_bytes, int ws_fresh, void* stream);

/* ------------------------------------------------------------------------------------
 * Batched linear assignment (square, dense), one workgroup per problem.
 *
 * Replaces: pleas/core/solvers.py:18-33 (scipy_solve_lsa -> D2H copy +
 *   scipy.optimize.linear_sum_assignment), called at activation_matching.py:173 and
 *   weight_matching.py:78.
 *
 * cost[p]   : DEVICE pointer to an n[p] x n[p] row-major fp32 matrix (HOST array of pointers)
 * n[p]      : HOST array, 1 <= n[p] <= PLEAS_LSAP_MAX_N
 * col_ind[p]: DEVICE pointer to n[p] int64 (HOST array of pointers); on completion row i is
 *             assigned to column col_ind[p][i]
 * Arithmetic: costs are widened to fp64; duals and path lengths are fp64; the scan order and
 * tie rule are those of scipy's shortest-augmenting-path solver, so the output is the same
 * assignment scipy returns, including on degenerate (tied) inputs.
 */
#define PLEAS_LSAP_MAX_N 4096
int pleas_lsap_batched(const float* const* cost, const int* n, int nprob, int maximize, int64_t* const* col_ind,
                       void* stream);
/* The same solver for ONE problem whose cost matrix is in HOST memory (fp32 when is_double == 0, else fp64; n >= 1, no
 * upper limit), synchronous, no GPU involved: the explicit host entry point for callers that hold host data
 * (weight matching of CPU state dicts: reference weight_matching.py:78 with CPU tensors, BASELINE.json configs[0]).
 * Same scan order and tie rule, hence the same col_ind as scipy.optimize.linear_sum_assignment. */
int pleas_lsap_host(const void* cost, int is_double, int n, int maximize, int64_t* col_ind);

/* ------------------------------------------------------------------------------------
 * Batched lexicographic bottleneck assignment (square, dense), the GPU form of
 * scipy_solve_minimax_assignment (reference pleas/core/solvers.py:88-115).
 *
 * Contract, for an n x n fp32 matrix A, 1 <= n <= PLEAS_LSAP_MAX_N, finite entries, maximize = 1:
 *   1. t* = max over permutations p of min_i A[i, p(i)], comparing fp32 values (-0 == +0);
 *   2. among the permutations that reach t*, the one with the largest sum, scipy's LAP tie rule for the rest.
 *      Exactly: with M, m the largest and smallest entries, L = t* - (n (M - m) + max(1, |t*|)) in fp64, L32 = L
 *      rounded toward -inf to fp32 (the call is refused if L32 is not finite), A_hat = A with every entry < t*
 *      replaced by L32, the result is linear_sum_assignment(A_hat, maximize=True).
 * maximize = 0 is the same call on -A (minimise the largest entry, then the sum).
 *
 * cost[p], n[p], col_ind[p]: as for pleas_lsap_batched (DEVICE matrices / outputs, HOST pointer arrays).
 * t_out: DEVICE float[nprob] or NULL; receives min_i A[i, col_ind[i]] (maximize = 1) or max_i A[i, col_ind[i]]
 *   (maximize = 0), a zero always as +0.
 * ws: DEVICE workspace of at least pleas_bottleneck_ws_bytes(n, nprob) bytes.  It begins with int32 status[nprob],
 *   written by the kernels: 0 ok, 1 a NaN or +-inf entry, 2 an iteration cap was hit, 3 L32 not finite.  A problem
 *   whose status is not 0 gets col_ind = -1 everywhere and t_out = NaN.  Everything is enqueued on `stream` with no
 *   host synchronisation, so these errors are seen by reading status once the stream has reached them.
 * pleas_bottleneck_ws_bytes returns 0 for invalid sizes.
 */
size_t pleas_bottleneck_ws_bytes(const int* n, int nprob);
int pleas_bottleneck_batched(const float* const* cost, const int* n, int nprob, int maximize, int64_t* const* col_ind,
                             float* t_out, void* ws, size_t ws_bytes, void* stream);
/* The same contract for ONE problem in HOST memory (fp32 when is_double == 0, else fp64: entries are then compared in
 * fp64; L32 is rounded to fp32 all the same), synchronous, no GPU involved; returns the same col_ind as the device path.
 * t_out (HOST, nullable) as above.  PLEAS_EINVAL for a NULL pointer, n out of [1, PLEAS_LSAP_MAX_N], a non-finite
 * entry or a non-finite L32. */
int pleas_bottleneck_host(const void* cost, int is_double, int n, int maximize, int64_t* col_ind, double* t_out);

/* ------------------------------------------------------------------------------------
 * Block gather / average used by partial merging and by the PLeaS regression targets.
 *
 * Replaces: pleas/methods/partial_matching.py:122-129 (1-axis tensors) and :157-172
 *   (2-axis block matrix), and pleas/methods/pleas_merging.py:116-147 (index_select x8 + cat).
 *
 * Tensors are viewed as [outer][rows][cols][inner] (contiguous).  For every output
 * (o, r, c, i):   out = coef(r) * ( [row1[r]>=0 && col1[c]>=0] w1[o, row1[r], col1[c], i]
 *                                 + [row2[r]>=0 && col2[c]>=0] w2[o, row2[r], col2[c], i] )
 * with coef(r) = 0.5 for r < n_merged_rows and 1 otherwise.  row1/row2 (length rows_out) and
 * col1/col2 (length cols_out) are DEVICE int32 maps with -1 = "absent"; col1 == NULL means
 * cols are passed through unchanged (cols_out must equal cols_src).
 */
int pleas_merge_blocks(const float* w1, const float* w2, float* out, int64_t outer, int rows_out, int cols_out,
                       int64_t inner, int rows_src, int cols_src, const int32_t* row1, const int32_t* row2,
                       const int32_t* col1, const int32_t* col2, int n_merged_rows, void* stream);

/* Grouped form: the 1-axis block merge of MANY tensors (the merged layer inputs of one PLeaS update,
 * pleas_merging.py:125-147) in ONE launch.  items: HOST array; tensor pointers and maps are DEVICE pointers.
 * Tensors are viewed [outer][rows][inner]; semantics per tensor as pleas_merge_blocks without column maps.
 * Tensors with inner % 4 == 0 must be 16-byte aligned.  ws / ws_fresh as in pleas_gram_batch.
 * sub_stride > 1 (the input of a 1x1 convolution with that stride, which reads every sub_stride-th pixel of every
 * sub_stride-th line): the sources are images of sub_h x sub_w pixels (inner_src = sub_h * sub_w) and `out` holds only the
 * pixels the layer reads, inner = ceil(sub_h / sub_stride) * ceil(sub_w / sub_stride) -- the layer then is a dense 1x1
 * stride-1 convolution for pleas_fwd_batch / pleas_wgrad_batch.  0 or 1: inner is the sources' inner size. */
typedef struct pleas_merge_item {
    const float* w1;      /* [outer][rows_src][inner] */
    const float* w2;
    float* out;           /* [outer][rows_out][inner] */
    const int32_t* row1;  /* [rows_out], -1 = absent */
    const int32_t* row2;
    int64_t outer, inner;
    int rows_out, rows_src, n_merged;
    int sub_stride, sub_h, sub_w;
} pleas_merge_item;
size_t pleas_merge_batch_ws_bytes(const pleas_merge_item* items, int n_items);
int pleas_merge_batch(const pleas_merge_item* items, int n_items, void* ws, size_t ws_bytes, int ws_fresh, void* stream);

/* ------------------------------------------------------------------------------------
 * Frozen-source forward: inference BatchNorm (+ residual add) (+ ReLU / ReLU6) in one pass.
 *
 * Replaces: the BatchNorm2d -> (out += identity) -> ReLU module chain inside `model1(x); model2(x)`
 *   (pleas/methods/pleas_merging.py:267-268, models put in eval() at :352-353): three vendor
 *   kernels and seven tensor passes per chain become one kernel, one read (two with a residual)
 *   and one write.
 *
 * x, res (nullable), y: [n][channels][inner] contiguous fp32;  scale[c] = weight[c] / sqrt(var[c] + eps),
 * shift[c] = bias[c] - mean[c] * scale[c]  (DEVICE, prepared once by the caller).
 *   y = act(x * scale[c] + shift[c] (+ res));   y must not alias x.
 *
 * `relu` is an activation code, here and in every entry point below that has the parameter (pleas_bn_act_tracked,
 * pleas_bn_act_tracked_batches, pleas_bn_act_maxpool, pleas_conv2d_bn_act_fwd, pleas_conv2d_act_fwd, pleas_dwconv2d_fwd):
 *   PLEAS_ACT_NONE   the sum itself;
 *   PLEAS_ACT_RELU   torch.relu's rule in these four passes: v < 0 -> 0, a NaN stays a NaN;
 *   PLEAS_ACT_RELU6  F.relu6 / torch.clamp(v, 0, 6) for every fp32 input, the same in all seven entry points:
 *                    v < 0 ? 0 : (v > 6 ? 6 : v) -- a NaN stays a NaN, +inf -> 6, -inf -> 0, no rounding;
 *   any other value is taken as PLEAS_ACT_RELU (the parameter used to be a 0 / 1 flag).
 * The code is a runtime operand of the same kernels: no kernel form, plan entry or workspace depends on it.
 */
#define PLEAS_ACT_NONE 0
#define PLEAS_ACT_RELU 1
#define PLEAS_ACT_RELU6 2
int pleas_bn_act(const float* x, const float* scale, const float* shift, const float* res, float* y, int64_t n,
                 int channels, int64_t inner, int relu, void* stream);
/* Same pass with the intermediate values kept, for activation matching (activation_matching.py:49-100 measures EVERY
 * node of the chain): y_bn = x * scale + shift and y_sum = y_bn + res are written when non-NULL, y is the final value under
 * activation code `relu` (PLEAS_ACT_*); y_bn and y_sum do not depend on the code. */
int pleas_bn_act_tracked(const float* x, const float* scale, const float* shift, const float* res, float* y_bn,
                         float* y_sum, float* y, int64_t n, int channels, int64_t inner, int relu, void* stream);

/* The tracked pass on a tensor that holds `batches` batches back to back along n, each with its OWN affine map: scale /
 * shift are [batches][channels] (pleas_bn_train_fold_batches).  Replaces the same module chains when the twin forward of
 * activation_matching.py:49-100 carries several matching batches and the models are in train mode (batch statistics are
 * per batch: run_domainnet.py:172-186 never calls .eval()).  `relu`: a PLEAS_ACT_* code. */
int pleas_bn_act_tracked_batches(const float* x, const float* scale, const float* shift, const float* res, float* y_bn,
                                 float* y_sum, float* y, int64_t n_per_batch, int batches, int channels, int64_t inner,
                                 int relu, void* stream);

/* The same map followed by a max pooling window, one pass (a ResNet's stem: bn1 -> relu -> maxpool); `relu`: a PLEAS_ACT_* code.
 *
 * Replaces: BatchNorm2d -> ReLU -> nn.MaxPool2d(kernel, stride, padding) of a frozen source forward
 *   (pleas/methods/pleas_merging.py:267-268 runs the whole model; only Conv2d / Linear inputs and outputs are hooked,
 *   :197-243, so the full-resolution activation between ReLU and the pooling is consumed by nothing and is not written).
 *   y[n][c][oh][ow] = max over the KH x KW window at (oh * stride - pad, ow * stride - pad) of act(x * scale[c] + shift[c]);
 *   out-of-range taps never win (torch pads with -inf), a NaN tap does, under every activation code; floor-mode output size, dilation 1.
 *   scale == NULL: plain max pooling of x.  y: [n][channels][Ho][Wo], must not alias x. */
int pleas_bn_act_maxpool(const float* x, const float* scale, const float* shift, float* y, int64_t n, int channels, int H,
                         int W, int KH, int KW, int stride, int pad, int relu, void* stream);

/* Head of an evaluation forward: global average pooling with an optional channel gather, one pass.
 *
 * Replaces: AdaptiveAvgPool2d((1, 1)) -> flatten(1) at the end of `model(x)` and, with a map, permute_final_features
 *   (pleas/methods/pleas_merging.py:436-466: two slices, a cat and an index by argsort) in eval_perm_model (:469-496).
 *   y[n][k] = (sum over p of x[n][src[k]][p]) / HW      x: [N][C][HW], y: [N][K] contiguous fp32
 * src: DEVICE int32[K], entries in [0, C) -- they may repeat or reorder channels; the CALLER checks the range before the
 *   launch (an entry outside it reads nothing and yields NaN);  NULL = identity, K == C.
 * Fixed summation order, no atomics: the same bits run after run.  16-byte loads when HW % 4 == 0 and x is 16-byte aligned. */
int pleas_pool_gather(const float* x, const int32_t* src, float* y, int64_t N, int C, int64_t HW, int K, void* stream);

/* Top-1 accuracy counting on the device.
 *
 * Replaces: `logits.argmax(1)` + compare + sum of eval_perm_model (pleas/methods/pleas_merging.py:469-496, torchmetrics'
 *   Accuracy) and the per-batch `.argmax(1).cpu()` of eval_whole_model (:574-586) -- one host synchronisation per batch there,
 *   none here.
 *   top[n] = the FIRST index of the largest value of logits[n][0 .. C) (torch.argmax's tie rule; a NaN counts as largest)
 *   pred[n] = top[n] when pred != NULL;      *hits += number of rows with top[n] == labels[n]
 * logits [N][C] contiguous fp32, labels / pred DEVICE int64[N], hits a DEVICE int64 (8-byte aligned) that the caller zeroes
 * once and reads back once after its loop.  Integer atomics only: deterministic.  C = 1 and N = 1 are legal. */
int pleas_top1_count(const float* logits, const int64_t* labels, int64_t N, int C, int64_t* hits, int64_t* pred, void* stream);

/* Softmax cross-entropy of a classification head: loss, gradient of the logits and the top-1 hit count from one pass.
 *
 * Replaces: nn.CrossEntropyLoss()(logits, y), its backward down to the logits, and `(logits.argmax(1) == y).sum()` of the
 *   linear probe's training step (pleas/methods/pleas_merging.py:499-570) -- log_softmax, nll_loss, their two backward
 *   kernels, argmax, compare, sum, and the `float(loss)` read-back per step there; no host synchronisation here.
 *   per row n:  m = max_c x_c;  lse = m + log(sum_c exp(x_c - m));  row_loss[n] = lse - x[labels[n]]
 *               dlogits[n][c] = scale * (exp(x_c - lse) - [c == labels[n]])            (skipped when dlogits == NULL)
 *   loss[0] = scale * sum_n row_loss[n];  loss[1] += loss[0]     (skipped when loss == NULL; scale = 1 / N is torch's "mean")
 *   counts[0] += rows whose top-1 (pleas_top1_count's rule) is their label;  counts[1] += rows with a label outside [0, C)
 * A label outside [0, C) never indexes memory: its row has loss 0, a zero dlogits row and no hit (torch's ignore_index is NOT
 * implemented: the caller reads counts[1] back with its other results and treats a non-zero value as an error).
 * logits / dlogits [N][C] contiguous fp32, labels DEVICE int64[N], row_loss DEVICE fp32[N] (scratch the caller owns),
 * loss DEVICE fp32[2], counts DEVICE int64[2] (8-byte aligned; the caller zeroes them once and reads them once per loop).
 * -inf logits are legal (probability 0; at the label: +inf loss).  Every floating-point sum has a fixed order (the sum over
 * rows is a second, one-workgroup grid; loss[1] is updated by one thread) and the counters are integer atomics, one per
 * workgroup: the same call gives the same bits.  16-byte accesses when C % 4 == 0 and logits / dlogits are 16-byte aligned.
 * N == 0: nothing is enqueued, returns 0.  C < 1, N * C >= 2^30 or dlogits == logits: PLEAS_EINVAL. */
int pleas_softmax_xent(const float* logits, const int64_t* labels, int64_t N, int C, float scale, float* dlogits,
                       float* row_loss, float* loss, int64_t* counts, void* stream);

/* Train-mode BatchNorm of the matching forward, folded to the same per-channel affine map.
 *
 * Replaces: the BatchNorm2d modules inside the cross module's forward when the caller's models are in train mode --
 *   which is what both reference drivers do: no .eval() before activation_matching
 *   (experiments/shared_label_space/run_domainnet.py:172-186, :257-264; pleas/methods/activation_matching.py:119-122
 *   never touches the mode) -- i.e. torch.nn.functional.batch_norm(training=True): batch statistics for the
 *   normalisation, running statistics updated as a side effect.
 *
 * One streaming pass over x [n][channels][inner] (fp64 accumulation, deterministic two-stage reduce) gives, per channel,
 *   mean, var_b (biased);  scale = gamma / sqrt(var_b + eps);  shift = beta - mean * scale     (gamma / beta NULL = 1 / 0)
 * and, when running_mean / running_var are non-NULL,
 *   running <- (1 - f) running + f {mean, var_b * count / (count - 1)},   f = momentum, or 1 / (batches so far + 1) when
 *   momentum < 0 (torch's momentum=None);   *num_batches_tracked += 1 when non-NULL.
 * The chain's values then come from pleas_bn_act_tracked(x, scale, shift, ...) exactly as in eval mode.
 * ws: >= pleas_bn_train_ws_bytes(n, channels) bytes, 8-byte aligned, caller-owned.
 */
size_t pleas_bn_train_ws_bytes(int64_t n, int channels);
int pleas_bn_train_fold(const float* x, int64_t n, int channels, int64_t inner, const float* gamma, const float* beta,
                        double eps, double momentum, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float* scale, float* shift, void* ws, size_t ws_bytes,
                        void* stream);
/* `batches` batches of n samples each, back to back along the sample axis: every batch is folded on its own samples, IN
 * ORDER -- scale / shift are [batches][channels]; running statistics and counter end where `batches` successive forwards
 * of the module leave them.  ws: batches * pleas_bn_train_ws_bytes(n, channels) bytes. */
int pleas_bn_train_fold_batches(const float* x, int64_t n, int batches, int channels, int64_t inner, const float* gamma,
                                const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float* scale, float* shift, void* ws, size_t ws_bytes,
                                void* stream);

/* ------------------------------------------------------------------------------------
 * Fused masked Adam step over a flat parameter arena.
 *
 * Replaces: pleas/methods/pleas_merging.py:288-291 (`param.grad *= mask` for every
 *   parameter, then torch.optim.Adam.step with default betas/eps, no weight decay).
 *
 * g <- g * mask (mask may be NULL = all ones); m <- m + (1-b1)(g - m); v <- b2 v + (1-b2) g g;
 * p <- p - (lr / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).   step counts from 1.
 */
int pleas_masked_adam(float* p, const float* g, const float* mask, float* m, float* v, int64_t n, float lr,
                      float b1, float b2, float eps, int step, void* stream);

/* ------------------------------------------------------------------------------------
 * Squared-error reduction: out[0] (+)= scale * sum_k (a[k] - b[k])^2 ; also writes
 * diff[k] = dscale * (a[k] - b[k]) if diff != NULL.
 *
 * Replaces: pleas/methods/pleas_merging.py:282 (`((out - target)**2).mean()`) and the
 *   first node of its autograd backward (2 (out - target) / numel).
 * ws: at least pleas_sqerr_ws_bytes(n) bytes.  Deterministic two-stage reduction.
 */
size_t pleas_sqerr_ws_bytes(int64_t n);
int pleas_sqerr(const float* a, const float* b, int64_t n, float scale, int accumulate, float* out, float dscale,
                float* diff, void* ws, size_t ws_bytes, void* stream);

/* Bias gradient of a merged layer: out[c] = sum_{n, p} x[n][c][p] for x = the layer's residual [N][C][HW] (Linear: HW = 1).
 * Replaces the bias node of autograd's backward (pleas_merging.py:287).  Deterministic (fixed order, no atomics). */
int pleas_channel_sum(const float* x, int N, int C, int64_t HW, float* out, void* stream);

/* Host only (no GPU): the launch shape of a streaming kernel for a geometry -- made by the function its launcher makes it with.
 * op and its geometry geo[0 .. n_geo):
 *   PLEAS_STREAM_MERGE_BLOCKS    outer, rows_out, cols_out, inner, rows_src, cols_src, column maps given (0 / 1)
 *   PLEAS_STREAM_BN_ACT          n, channels, inner, n_per_map (0: one map; pleas_bn_act, _tracked and _tracked_batches)
 *   PLEAS_STREAM_BN_ACT_MAXPOOL  n, channels, H, W, KH, KW, stride, pad
 *   PLEAS_STREAM_MASKED_ADAM     n
 *   PLEAS_STREAM_SQERR           n
 *   PLEAS_STREAM_TARGET_RESIDUAL N, C, Csrc, HW
 *   PLEAS_STREAM_CHANNEL_SUM     N, C, HW
 *   PLEAS_STREAM_POOL_GATHER     N, C, HW, K, channel map given (0 / 1)
 *   PLEAS_STREAM_TOP1_COUNT      N, C
 *   PLEAS_STREAM_BN_TRAIN_FOLD   n (samples per batch), batches, channels, inner
 * aligned: whether every pointer that enters the launch's 16-byte predicate is 16-byte aligned.
 * info[0] floats per load / store (4 / 1), [1] kernel form (bn_act_maxpool: 0 general, 1 stem; else 0), [2] workgroups (0: the
 * launch enqueues nothing), [3] threads per workgroup, [4] sweeps = ceil(work items / what one pass of the grid covers) of the
 * grid-stride loop -- channel_sum and bn_train_fold have none: the trips of a thread's loop over one (sample, channel) slab --,
 * [5] bn_train_fold: S, the sample slabs per channel (else 0).  A geometry the launch refuses is refused with its message. */
#define PLEAS_STREAM_MERGE_BLOCKS 0
#define PLEAS_STREAM_BN_ACT 1
#define PLEAS_STREAM_BN_ACT_MAXPOOL 2
#define PLEAS_STREAM_MASKED_ADAM 3
#define PLEAS_STREAM_SQERR 4
#define PLEAS_STREAM_TARGET_RESIDUAL 5
#define PLEAS_STREAM_CHANNEL_SUM 6
#define PLEAS_STREAM_POOL_GATHER 7
#define PLEAS_STREAM_TOP1_COUNT 8
#define PLEAS_STREAM_BN_TRAIN_FOLD 9
#define PLEAS_STREAM_OPS 10
int pleas_stream_plan_info(int op, const int64_t* geo, int n_geo, int aligned, int* info);

/* ------------------------------------------------------------------------------------
 * Forward of an nn.Linear: y[n][c] = bias[c] + sum_k x[n][k] * w[c][k]   (csrc/linear.hip).
 *
 * Replaces: `fc(feats)` of the linear probe's step and of the merged model's classifier (pleas/methods/pleas_merging.py:499-570,
 *   :469-496), which the library ran through pleas_conv2d_fwd with H = W = KH = KW = 1 -- a convolution tile on one pixel per
 *   sample.  Here: one 64 x 64 NT tile form whose K axis is cut into S ranges of whole 32-float chunks, S a pure function of
 *   (N, C, K) that brings the grid to about two workgroups per CU.
 * Layout: x [N][K], w [C][K], y [N][C], all row-major contiguous fp32; bias fp32[C] or NULL.  Any 4-byte alignment is legal:
 *   16-byte loads when K % 4 == 0 and x and w are 16-byte aligned, 4-byte loads otherwise (same results).
 * Workspace: ws of at least pleas_linear_ws_bytes(N, C, K) bytes, the partial tiles [S][N][C]; 0 bytes (ws may be NULL) when
 *   S == 1, where the tile writes y itself and no second grid runs.  The call leaves nothing in ws that a later call needs.
 * Determinism: the slabs are added in slab order, then the bias, by a second grid; no floating-point atomics.  The same call
 *   gives the same bits.
 * Arithmetic: exact fp32 MFMA in EVERY pleas_arith mode; the switch does not reach this kernel.
 * Limits: x, w and y each hold fewer than 2^30 elements (PLEAS_EINVAL otherwise).  Negative sizes, a NULL y, or a NULL x / w with
 *   K > 0: PLEAS_EINVAL; a workspace that is too small: PLEAS_ENOMEM; all before anything is enqueued.  N == 0 (or C == 0):
 *   PLEAS_OK, nothing is enqueued.  K == 0: y = bias, or zeros.
 * pleas_linear_plan_info: info[0 .. 4] = sample tiles, class tiles, S, chunks per range, chunks of the last range (host
 *   arithmetic only: no device is touched).  Ranges 0 .. S-2 hold `chunks per range` chunks each; none is empty. */
size_t pleas_linear_ws_bytes(int64_t N, int C, int K);
int pleas_linear_plan_info(int64_t N, int C, int K, int* info);
int pleas_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int C, int K, void* ws,
                     size_t ws_bytes, void* stream);

/* Bias gradient of a Linear: out[c] = sum_n x[n][c] for x [N][C] contiguous fp32, out fp32[C].
 * Replaces the bias node of autograd's backward for a Linear (pleas_channel_sum with HW = 1 walks the N rows with one thread).
 * Row-parallel: lanes run along c, a thread adds a fixed stripe of rows (n = stripe, stripe + 32, ...) in increasing n, the 32
 * stripes of a column are added in stripe order.  Deterministic, no atomics.  C = 1 and N = 1 are legal; N <= 0, C <= 0 or
 * N * C >= 2^30: PLEAS_EINVAL. */
int pleas_column_sum(const float* x, int64_t N, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * uint8 image batches to normalised fp32 NCHW: table lookup, crop and horizontal flip in one pass (csrc/image.hip).
 *
 * Replaces: `x.cuda()` of batches that CPU workers have already run through ToTensor / Normalize / RandomCrop /
 *   RandomHorizontalFlip (pleas/methods/activation_matching.py:121, pleas/methods/pleas_merging.py:266, and the transforms of
 *   the drivers' datasets): 12 bytes per pixel over PCIe there, 3 here, and no per-image host arithmetic.
 *   dst[n][c][y][x] = lut[c][ src[n][y0 + y][x0 + xs][c] ],   xs = Wo-1-x when flip[n] != 0, else x;   (y0, x0) = origin[n]
 * Layout: src uint8, [N][H][W][C] for layout == PLEAS_IMAGE_NHWC, [N][C][H][W] for PLEAS_IMAGE_NCHW, C in 1 .. 4, contiguous,
 *   any alignment.  dst fp32 [N][C][Ho][Wo] contiguous, 16-byte aligned.  lut DEVICE fp32 [C][256].  origin DEVICE int32 [N][2]
 *   or NULL = (0, 0).  flip DEVICE uint8 [N] or NULL = none.
 * Arithmetic: a table lookup and nothing else -- the result has the bits of the table under every compiler flag and is free
 *   of NaN / inf whenever the table is.  A table built as ((v / 255) - mean[c]) / std[c] in fp32 reproduces ToTensor +
 *   Normalize bit for bit.
 * Determinism: no atomics, no floating-point sums; every output element is written once.
 * Form: the table (at most 4 KB) is copied to LDS once per workgroup.  A row of the output belongs to a team of lanes (the power
 *   of two at or above Wo / 16) that reads its window byte by byte, the lanes side by side along x, four pixels of loads in
 *   flight per lane, and writes each plane in 4-byte runs: one path for every C, layout, alignment, crop and flip.  (A second
 *   path for 16-byte aligned 3-channel rows -- 16-byte loads, de-interleaved in registers, 16-byte stores -- was measured at
 *   0.97 to 1.01 of the byte path's time and is not kept: profiles/image_batch_fast_vs_byte.json.)
 * Limits: sizes are `int`, indexing is 64-bit: no 2^30 bound on src or dst.  The origins are NOT checked here: an origin with
 *   y0 < 0, x0 < 0, y0 > H - Ho or x0 > W - Wo reads outside src; the check is the caller's, on the host, before the upload.
 * PLEAS_EINVAL, before anything is enqueued: a NULL src, dst or lut with N > 0; C outside 1 .. 4; Ho > H or Wo > W; a
 *   non-positive H, W, Ho or Wo or a negative N; a dst that is not 16-byte aligned; an unknown layout.  N == 0: PLEAS_OK,
 *   nothing is enqueued. */
#define PLEAS_IMAGE_NHWC 0
#define PLEAS_IMAGE_NCHW 1
int pleas_image_batch(const uint8_t* src, float* dst, const float* lut, const int32_t* origin, const uint8_t* flip,
                      int64_t N, int C, int H, int W, int Ho, int Wo, int layout, void* stream);

/* ------------------------------------------------------------------------------------
 * uint8 images of MIXED sizes to normalised fp32 NCHW of one size: PIL's 8-bit bilinear resampling, flip and table lookup
 * (csrc/image.hip; the plan and the host executor: csrc/resample_plan.hpp).
 *
 * Replaces: RandomResizedCrop / RandomHorizontalFlip and Resize / CenterCrop on the CPU workers of the drivers' loaders
 *   (experiments/shared_label_space/run_domainnet.py:204-214, experiments/datasets/interface.py:14-18), in front of the
 *   ToTensor / Normalize that pleas_image_batch's table already reproduces.  Those transforms resample PIL images, and PIL
 *   resamples 8-bit images in integer arithmetic, so the result here has the bits of Normalize(ToTensor(PIL chain)).
 * Layout: src one packed uint8 buffer; sample s is [H_s][W_s][C] at byte src_offset[s], any alignment, C in 1 .. 4 common to the
 *   batch.  geom int32 [N][10] per sample: H, W, then the box y0, x0, h, w inside the image, then the virtual output size Hv, Wv
 *   the box is resampled to, then the origin oy, ox of the Ho x Wo window of that output which is produced.
 *     resized crop    box = the crop, (Hv, Wv) = (Ho, Wo), origin (0, 0):  img.crop((x0, y0, x0+w, y0+h)).resize((Wo, Ho), BILINEAR)
 *     resize + window box = the whole image, origin = the window's:        img.resize((Wv, Hv), BILINEAR).crop(window)
 *   dst fp32 [N][C][Ho][Wo] contiguous, 16-byte aligned; lut fp32 [C][256]; flip uint8 [N] or NULL = none (dst[.., x] takes the
 *   resampled pixel Wo-1-x: RandomHorizontalFlip after the crop).
 * Arithmetic, one pass along an axis of `in` samples to `out` (PIL's, weights in double, taps in int32):
 *     scale = in / out;  fs = max(scale, 1);  ksize = 2 * ceil(fs) + 1;   output i:  center = (i + 0.5) * scale,
 *     lo = max(0, (int)(center - fs + 0.5)),  hi = min(in, (int)(center + fs + 0.5)),
 *     w_j = max(0, 1 - |(lo + j - center + 0.5) * (1 / fs)|) summed in order of j into ww, divided by ww when ww != 0,
 *     k_j = (int)(0.5 + w_j * 2^22);   value = clamp((2^21 + sum_j k_j * in[lo + j]) >> 22, 0, 255)
 *   horizontal pass first, stored as uint8, vertical pass second; only the source rows the window's vertical pass reads are
 *   resampled horizontally.  The sum stays below 2^31: 2^21 + 255 * (2^22 + ksize).
 * Determinism: integer sums, no atomics, every byte of the workspace and every element of dst written once; the plan is a pure
 *   function of its arguments.
 * Form: a plan built on the host (pleas_resample_plan) holds, per sample and axis, the (first tap, taps) bounds and the int32
 *   coefficients, the sample's place in src and in the workspace, and two tables of work items (sample, first row, rows).  Two
 *   launches for the whole batch: rows (src -> uint8 [rows_s][Wo][C] in the workspace) and planes (workspace -> flip, table in
 *   LDS, fp32 planes in 4-byte runs side by side).  Workgroups take items with a grid stride, so samples of very different
 *   sizes balance by their rows.  The plan is position independent: copy it to the device with the batch.
 * Limits: a side of an image or of a virtual output is at most 16384 (a table stays below 2^31 words), N at most 2^20, the
 *   plan below 2^31 bytes; offsets into src, the workspace and dst are 64-bit.  The kernels index with nothing that does not
 *   come from the plan: hand pleas_image_resample the device copy of the plan whose host copy it checks.
 * pleas_resample_plan_bytes: bytes of the plan of geom (0 and a message when geom is refused).  pleas_resample_plan: writes
 *   it into caller memory (4-byte aligned).  pleas_resample_plan_info: info[0 .. 7] = N, C, Ho, Wo, bytes of src, bytes of the
 *   workspace, items of the rows launch, items of the planes launch.  pleas_image_resample_host: executes a plan on the CPU, item
 *   by item as the kernels do (an explicit host entry point like pleas_lsap_host; dst_u8, or NULL, receives the resampled
 *   bytes [N][Ho][Wo][C] after the flip).  These four touch no device.
 * PLEAS_EINVAL, before anything is written or enqueued: a box outside its image; a window outside its virtual output; a
 *   non-positive size; a side above 16384; C outside 1 .. 4; a sample whose src_offset + H * W * C exceeds src_bytes or is
 *   negative; plan memory that is NULL, unaligned or too small; a host plan without the magic word, longer than plan_bytes or
 *   with a damaged header; a NULL src, plan, lut or dst with N > 0; a dst that is not 16-byte aligned.  A workspace below the
 *   plan's: PLEAS_ENOMEM.  N == 0: PLEAS_OK, nothing is enqueued. */
size_t pleas_resample_plan_bytes(const int32_t* geom, int64_t N, int Ho, int Wo);
int pleas_resample_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo, int64_t src_bytes,
                        void* plan, size_t plan_bytes);
int pleas_resample_plan_info(const void* plan, size_t plan_bytes, int64_t* info);
int pleas_image_resample_host(const uint8_t* src, const void* plan, size_t plan_bytes, const float* lut, const uint8_t* flip,
                              float* dst_f32, uint8_t* dst_u8);
int pleas_image_resample(const uint8_t* src, const void* plan_dev, const void* plan_host, size_t plan_bytes, const float* lut,
                         const uint8_t* flip, float* dst, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * A CHAIN of two resamplings on uint8 images of mixed sizes: Resize, then a resized crop, then flip and table lookup
 * (csrc/image.hip; the chain plan and its host executor: csrc/resample_plan.hpp).
 *
 * Replaces: Resize(256) -> RandomResizedCrop(224) -> ToTensor -> Normalize on the CPU workers of the train loaders
 *   (experiments/datasets/interface.py, cub.py, nabird.py, oxford_pets.py, stanford_dogs.py, domainnet.py).  Per sample
 *     img.resize((W1, H1), BILINEAR).crop((x0, y0, x0+w, y0+h)).resize((Wo, Ho), BILINEAR)
 *   then the flip, then the table: the bits of Normalize(ToTensor(PIL chain)).
 * Layout: src, src_offset, lut, flip, dst as pleas_image_resample's.  geom int32 [N][8] per sample: H, W (image), H1, W1 (size
 *   after the first resize, taken as given: torchvision's Resize rule is the caller's), y0, x0, h, w (box inside H1 x W1).
 *   mid_u8 (host executor, or NULL): the image between the two resizes, uint8 [h_s][w_s][C] per sample, samples end to end.
 * Arithmetic: each resize is the one-axis pass of pleas_image_resample, horizontal first, stored as uint8, then vertical; the
 *   image between the two resizes is uint8 as PIL's is.  Of the first resize only the box is computed: columns x0 .. x0+w and
 *   rows y0 .. y0+h of the virtual H1 x W1 image, from only the source rows their vertical pass reads.  The second resize reads
 *   nothing outside the box (torchvision's resized_crop crops first).
 * Determinism: integer sums, no atomics, every byte of the workspace and every element of dst written once; the plan is a pure
 *   function of its arguments.
 * Form: one position-independent blob: a chain header, a stage-1 section (laid out like a plan, with the output width and the
 *   place in the intermediate per sample) and an ordinary stage-2 plan whose source is the intermediate.  Four launches for the
 *   batch: rows 1 (src -> scratch [rows_s][w_s][C]), bytes 1 (scratch -> intermediate, no table, no flip; a row is w_s * C
 *   bytes, one kernel for every C), then the rows and planes kernels of pleas_image_resample on the intermediate.  Workgroups
 *   take items (sample, first row, rows) with a grid stride.  The two scratches and the intermediate are three regions of ws,
 *   each on a 16-byte boundary, at 64-bit offsets the plan holds.
 * Limits: as pleas_image_resample's, with H1, W1 among the sides of at most 16384.  The kernels index with nothing that does
 *   not come from the plan: hand pleas_image_resample_chain the device copy of the plan whose host copy it checks.
 * pleas_resample_chain_plan_bytes: bytes of the chain plan of geom (0 and a message when geom is refused).
 *   pleas_resample_chain_plan: writes it into caller memory (4-byte aligned).  pleas_resample_chain_plan_info: info[0 .. 10] =
 *   N, C, Ho, Wo, bytes of src, bytes of the workspace, bytes of the intermediate, items of rows 1, bytes 1, rows 2, planes 2.
 *   pleas_image_resample_chain_host: executes a chain plan on the CPU, launch by launch and item by item as the kernels do
 *   (dst_u8, or NULL: the final bytes [N][Ho][Wo][C] after the flip).  These four touch no device.
 * PLEAS_EINVAL, before anything is written or enqueued: a box outside H1 x W1; a non-positive size; a side (H, W, H1, W1, Ho,
 *   Wo) above 16384; C outside 1 .. 4; a sample whose src_offset + H * W * C exceeds src_bytes or is negative; plan memory that
 *   is NULL, unaligned or too small; a host plan without the magic word, longer than plan_bytes or with a damaged header or
 *   section; a NULL src, plan, lut or dst with N > 0; a dst that is not 16-byte aligned.  A workspace below the plan's:
 *   PLEAS_ENOMEM.  N == 0: PLEAS_OK, nothing is enqueued. */
size_t pleas_resample_chain_plan_bytes(const int32_t* geom, int64_t N, int Ho, int Wo);
int pleas_resample_chain_plan(const int32_t* geom, const int64_t* src_offset, int64_t N, int C, int Ho, int Wo, int64_t src_bytes,
                              void* plan, size_t plan_bytes);
int pleas_resample_chain_plan_info(const void* plan, size_t plan_bytes, int64_t* info);
int pleas_image_resample_chain_host(const uint8_t* src, const void* plan, size_t plan_bytes, const float* lut, const uint8_t* flip,
                                    float* dst_f32, uint8_t* dst_u8, uint8_t* mid_u8);
int pleas_image_resample_chain(const uint8_t* src, const void* plan_dev, const void* plan_host, size_t plan_bytes, const float* lut,
                               const uint8_t* flip, float* dst, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * PLeaS layer fitting: fused target/residual/loss pass and grouped weight-gradient launch.
 *
 * Replaces, for merging='perm_gradmask': the output half of get_model_orig_activations
 *   (pleas_merging.py:116-123, :147), the per-layer MSE (:282) and the whole autograd backward
 *   of the merged layers (:287).
 *
 * pleas_target_residual: out = merged layer output [N][C][HW]; o1, o2 = source layer outputs
 *   [N][Csrc][HW]; row1/row2/n_merged = block maps as in pleas_merge_blocks.
 *   resid = dscale * (out - target)   (resid may alias out);   partials[0..*n_partials) receive this
 *   call's per-workgroup sums of (out - target)^2 (*n_partials <= pleas_target_residual_max_partials()).
 * pleas_loss_final: loss[l] = scale[l] * sum(partials[l*stride .. +n_partials[l]))  (all DEVICE arrays).
 * pleas_wgrad_batch: for every layer  grad[co][ci][kh][kw] = sum_{n,oh,ow} resid[n][co][oh][ow] *
 *   ip[n][ci][oh*stride+kh-pad][ow*stride+kw-pad]  (a Linear layer is Hin=Win=KH=KW=1).
 *   layers: HOST array; resid/ip/grad DEVICE pointers (16-byte aligned); ws >= pleas_wgrad_batch_ws_bytes.
 *   Deterministic; the work list is cached per (geometry sequence, ws); ws_fresh as in pleas_gram_batch.
 */
/* pleas_fwd_batch: forward of every merged layer of one update with the target, residual and loss fused:
 *   out   = conv(ip, w) (+ bias)                      (never stored)
 *   tgt   = coef(co) * ([row1[co]>=0] o1[n][row1[co]] + [row2[co]>=0] o2[n][row2[co]]),  coef = 0.5 for co < n_merged
 *   resid = dscale * (out - tgt)      -> layers[i].resid  (the input of pleas_wgrad_batch)
 *   loss[i] = loss_scale * sum (out - tgt)^2           (DEVICE float[n_layers], fixed summation order)
 * A Linear layer is Hin = Win = KH = KW = 1.  w and ip must be 16-byte aligned.  ws / ws_fresh as in pleas_gram_batch.
 * Stride-1 "same" convolutions with Cin % 32 == 0 (k x k: with PLEAS_FWD_KPOS_MAJOR) take the flat-shift tile forms; the
 * forms of a call run as separate grids on the caller's stream and up to three side streams of the library, joined
 * before the call's last kernel (fwd_loss) is enqueued on `stream`.
 */
typedef struct pleas_fwd_layer {
    const float* ip;     /* [N][Cin][Hin][Win] merged input */
    const float* w;      /* [Cout][Cin][KH][KW], or [Cout][KH][KW][Cin] with PLEAS_FWD_KPOS_MAJOR */
    const float* bias;   /* [Cout] or NULL */
    const float* o1;     /* [N][Csrc][Hout*Wout] source-layer outputs */
    const float* o2;
    const int32_t* row1; /* [Cout] block maps (DEVICE) */
    const int32_t* row2;
    float* resid;        /* [N][Cout][Hout*Wout] */
    int N, Cout, Cin, Hin, Win, KH, KW, stride, pad, Csrc, n_merged;
    float dscale, loss_scale;
    int flags;           /* PLEAS_FWD_* */
} pleas_fwd_layer;
/* Weights stored kernel-position-major (the layout pleas_wgrad_batch writes with PLEAS_WGRAD_KPOS_MAJOR); needs
 * Cin % 32 == 0.  Every 32-deep K chunk then has ONE tap: per-thread addressing is as cheap as for a 1x1 layer and
 * the taps of a channel block re-read the same input rows back to back. */
#define PLEAS_FWD_KPOS_MAJOR 1
size_t pleas_fwd_batch_ws_bytes(const pleas_fwd_layer* layers, int n_layers);
/* Diagnostics of the latest pleas_fwd_batch plan: per tile form (10 entries each) the duration measured on its lane by
 * the plan's calibration launch [ms] (0 before it), the lane it runs on (0 = the caller's stream) and its work items.
 * Returns 0 = lanes still dealt from static weights, 1 = calibration launch in flight, 2 = lanes dealt from measurements. */
int pleas_fwd_plan_lanes(double* form_ms, int* form_lane, int* form_items);
/* Host only (no GPU): the launch units of the grouped forward of `layers` -- one kernel launch each: a tile form over a
 * contiguous slice of that form's work items, on a lane -- as 4 ints per unit (form, first item, items, lane) in launch
 * order.  form_ms == NULL: the units of a fresh plan (one per form, lanes from static weights); else the units after a
 * calibration launch that measured form_ms[10] milliseconds per form (long forms cut into slices of equal work).
 * Returns the number of units (> max_units: only the first max_units were written) or a negative error code. */
int pleas_fwd_plan_units(const pleas_fwd_layer* layers, int n_layers, const double* form_ms, int* units, int max_units);
int pleas_fwd_batch(const pleas_fwd_layer* layers, int n_layers, float* loss, void* ws, size_t ws_bytes, int ws_fresh,
                    void* stream);
/* pleas_conv2d_fwd: a plain convolution  y = conv(x, w) (+ bias)  on the tile forms of pleas_fwd_batch (fp32 MFMA 32x32x2,
 * fixed summation order: bit-for-bit repeatable, unlike MIOpen's split-K 3 x 3 kernels).  Replaces the vendor convolution under
 * the frozen sources' k x k layers -- the two `model(x)` calls of pleas/methods/pleas_merging.py:267-268 and of the twin
 * graph, activation_matching.py:49-100 -- so that the same job returns the same assignment and weights run after run.
 *   x [N][Cin][Hin][Win], w [Cout][Cin][KH][KW] (or [Cout][KH][KW][Cin] with PLEAS_FWD_KPOS_MAJOR), y [N][Cout][Hout][Wout];
 *   x and w 16-byte aligned; square kernels up to 64 taps; no workspace, no tables: the layer rides in the kernel arguments. */
int pleas_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hin, int Win, int Cout,
                     int KH, int KW, int stride, int pad, int flags, void* stream);
/* pleas_conv2d_bn_act_fwd: the same convolution with the eval-mode BatchNorm / residual add / ReLU that follows it in a frozen
 * source (torchvision Bottleneck: conv -> bn -> relu, conv3 -> bn3 -> (+ identity) -> relu, downsample conv -> bn) in its
 * epilogue:  y = conv(x, w) (+ bias)  is stored for the hooks of pleas_merging.py:197-231 (the layer's OUTPUT is a regression
 * target), and  z = act(y * scale[c] + shift[c] (+ res))  -- bit for bit what pleas_bn_act makes of y -- is stored beside it
 * from the registers, so y is not read back.  res (or NULL) and z are shaped like y; y, z, res 16-byte aligned.
 * `relu`: a PLEAS_ACT_* code.  The stored y does not depend on it.  Under PLEAS_ACT_RELU6 z is bit for bit pleas_bn_act's, a NaN
 * included; the ReLU arm of this epilogue is fmaxf(v, 0), which turns a NaN into 0 where pleas_bn_act keeps it. */
int pleas_conv2d_bn_act_fwd(const float* x, const float* w, const float* bias, float* y, const float* scale,
                            const float* shift, const float* res, float* z, int relu, int N, int Cin, int Hin, int Win,
                            int Cout, int KH, int KW, int stride, int pad, int flags, void* stream);
/* pleas_conv2d_act_fwd: the arithmetic of pleas_conv2d_bn_act_fwd with the activated image as its ONLY output:
 *   z = act(fma(conv(x, w) (+ bias), scale[c], shift[c]) (+ res))
 * -- bit for bit the z of pleas_conv2d_bn_act_fwd on the same inputs, under every pleas_arith mode and weight layout; y is
 * neither an argument nor stored (a third of the output traffic of a 1 x 1 layer).
 * Replaces: the Conv2d -> BatchNorm2d -> (+ identity) -> ReLU module chains of `model(x)` in the evaluation helpers
 *   (pleas/methods/pleas_merging.py:469-496 eval_perm_model, :575-586 eval_whole_model, :499-570 the linear probe's frozen
 *   backbone), where no hook reads the convolution's output.
 * Same argument checks, alignment rules (x, w, z, res 16-byte aligned), per-call size limits and activation codes (`relu`) as
 * its sibling. */
int pleas_conv2d_act_fwd(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                         const float* res, float* z, int relu, int N, int Cin, int Hin, int Win, int Cout, int KH, int KW,
                         int stride, int pad, int flags, void* stream);
/* pleas_conv2d_bn_stats_fwd: the convolution of pleas_conv2d_fwd followed by a TRAIN-mode BatchNorm2d's fold, with the batch
 * statistics taken in the convolution's epilogue instead of from a second pass over y:
 *   y = conv(x, w) (+ bias)                            stored, bit for bit what pleas_conv2d_fwd stores
 *   scale, shift [batches][Cout], running statistics and counter: as pleas_bn_train_fold_batches on y would leave them
 * Replaces: Conv2d -> BatchNorm2d(training) of the BN-statistics reset that every driver runs on the merged model
 *   (experiments/shared_label_space/run_domainnet.py:327-341): the vendor convolution (its 3 x 3 kernels split K with atomics:
 *   not repeatable) and the statistics pass over its output.
 * Three kernels on `stream`: the convolution, whose work items leave fp64 sums of y and y^2 per channel over their tile's pixels
 * (y = the stored fp32 value; two segments per tile, for the batch of its first pixel and for the next one); a reduce over the
 * tiles per (batch, channel); the finalize kernel of pleas_bn_train_fold_batches.  Fixed orders, no atomics.
 *   N: ALL samples, N % batches == 0, batch b = samples b * N / batches ..; geometry limits, flags and pleas_arith modes as
 *   pleas_conv2d_fwd; gamma / beta / eps / momentum / running_* / num_batches_tracked as pleas_bn_train_fold_batches.
 * Refused with PLEAS_EINVAL before anything is enqueued: NULL x / w / y / scale / shift, batches < 1, N % batches != 0, one value
 *   per channel and batch, one running pointer without the other, a misaligned ws, and batches > 1 with fewer than 128 output
 *   pixels per batch (a tile would touch more than two batches: fold those after pleas_conv2d_fwd).  PLEAS_ENOMEM: ws NULL or
 *   smaller than pleas_conv2d_bn_stats_ws_bytes(N, Cout, Hout, Wout, batches) (8-byte aligned, caller-owned; 0 for empty shapes). */
size_t pleas_conv2d_bn_stats_ws_bytes(int N, int Cout, int Hout, int Wout, int batches);
int pleas_conv2d_bn_stats_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hin, int Win,
                              int Cout, int KH, int KW, int stride, int pad, int flags, int batches, const float* gamma,
                              const float* beta, double eps, double momentum, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, float* scale, float* shift, void* ws, size_t ws_bytes, void* stream);
typedef struct pleas_wgrad_layer {
    const float* resid; /* [N][Cout][Hout*Wout] */
    const float* ip;    /* [N][Cin][Hin][Win]   */
    float* grad;        /* [Cout][Cin][KH][KW]  */
    int N, Cout, Cin, Hin, Win, KH, KW, stride, pad;
    int flags;          /* PLEAS_WGRAD_* */
} pleas_wgrad_layer;
#define PLEAS_WGRAD_ACCUMULATE 1  /* grad += instead of grad = (normal equations: B^T over many batches) */
#define PLEAS_WGRAD_KPOS_MAJOR 2  /* write grad as [Cout][KH*KW][Cin] (kernel-position-major columns) */
int pleas_target_residual(const float* out, const float* o1, const float* o2, const int32_t* row1, const int32_t* row2,
                          int n_merged, int N, int C, int Csrc, int64_t HW, float dscale, float* resid, float* partials,
                          int* n_partials, void* stream);
int pleas_target_residual_max_partials(void);
int pleas_loss_final(const float* partials, const int* n_partials, const float* scale, int stride, int n_layers,
                     float* loss, void* stream);
size_t pleas_wgrad_batch_ws_bytes(const pleas_wgrad_layer* layers, int n_layers);
int pleas_wgrad_batch(const pleas_wgrad_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh,
                      void* stream);
/* Host only (no GPU): what the plan builder of pleas_wgrad_batch decides for `layers` under the current pleas_arith, six ints
 * per layer: [0] the tile form `variant` (bit 0: 64-row tiles, bit 1: 64-column tiles, bit 2: scalar loads of the residual,
 * bit 3: shifted one-pixel loader of the input, bit 4: shifted through aligned 16-byte loads, bit 5: "virtual channels" --
 * rows are (channel, tap) pairs, layers with fewer than 16 input channels --, bit 6: split-bf16 kernel, either product count), [1] S, the slabs of
 * the pixel axis (> 1: slabs + reduce), [2] / [3] output-channel / input-channel tiles, [4] work items, [5] 1 when the
 * epilogue stages the tile through LDS and writes 16-byte rows (the pointers may be NULL: a 16-byte aligned gradient and
 * workspace are assumed then).  Returns 0 or a negative error code. */
int pleas_wgrad_plan_info(const pleas_wgrad_layer* layers, int n_layers, int* info);

/* ------------------------------------------------------------------------------------
 * Depthwise convolutions (nn.Conv2d with groups == in_channels == out_channels): csrc/dwconv.hip.
 *
 * Replaces: the vendor's grouped convolution under every depthwise layer of the frozen source / twin / evaluation forwards
 *   (pleas/methods/pleas_merging.py:267-268, activation_matching.py:49-100, the evaluation helpers :469-586), and -- for the fit --
 *   `layer(ip)`, the MSE and autograd's backward of such a layer (pleas_merging.py:281-287), which the library ran on the vendor's
 *   operators one layer at a time.
 * Layout: x [N][C][Hin][Win], w [C][1][K][K], y / z / res [N][C][Ho][Wo], Ho = (Hin + 2 pad - K) / stride + 1; bias, scale, shift
 *   fp32[C].  Only the tensor BASES must be 16-byte aligned (bias / scale / shift: 4-byte): rows of any width are legal.
 * Arithmetic: fp32, plain FMA, the same code under every pleas_arith mode.
 *   pleas_dwconv2d_fwd:  y = dwconv(x, w) (+ bias), stored when y != NULL;  z = act(fma(y, scale[c], shift[c]) (+ res)), stored
 *     when z != NULL -- bit for bit what pleas_bn_act makes of the stored y (scale == NULL: z = act(y (+ res))).  The three uses
 *     are y alone (pleas_conv2d_fwd), y and z (pleas_conv2d_bn_act_fwd) and z alone (pleas_conv2d_act_fwd).
 *   pleas_dw_fwd_batch: per layer the contract of pleas_fwd_batch -- out = dwconv(ip, w) (+ bias) is never stored; tgt from o1, o2,
 *     row1, row2, n_merged as there; resid = dscale * (out - tgt) stored; loss[i] = loss_scale * sum (out - tgt)^2.  This kernel
 *     alone accumulates in fp64 (the forward's chain and order, every fp32 product exact): a residual and a loss are each rounded
 *     to fp32 once, which is what keeps the loss of a layer with a single output within 2^-24 of the fp64 value.
 *   pleas_dw_wgrad_batch: grad[c][ky][kx] = sum_{n,oy,ox} resid[n][c][oy][ox] * ip[n][c][oy*stride+ky-pad][ox*stride+kx-pad]  (the
 *     bias gradient stays with pleas_channel_sum).
 * Determinism: no atomics, every output element written once, one stated summation order per kernel (header of csrc/dwconv.hip):
 *   forward -- taps ky outer, kx inner, ascending, one fmaf chain from 0, taps outside the image times 0, bias last; loss --
 *   per-workgroup partials, then one ordered pass; gradient -- per (channel, slab of output rows) K*K partial sums, then the slabs
 *   in order, the slab split a function of the geometry alone.  Grouped and alone give the same bits.
 * Form: a thread owns one output column of a strip of 4 output rows of one (n, c) plane and walks the strip's input rows once;
 *   lanes run along the row, then over strips and planes; the channel's K*K weights sit in registers.
 * Limits: K odd in 1 .. 7, stride 1 or 2, pad <= K / 2, square kernel / stride / padding; every per-call element count (input,
 *   output, a source output) below 2^30.
 * EINVAL (before anything is enqueued): NULL x or w; both y and z NULL; scale without shift (or the reverse); scale / shift / res
 *   without z; non-positive sizes (a kernel larger than the padded image included); even K or K > 7; a stride outside {1, 2};
 *   pad > K / 2; a misaligned base pointer; an element count at or above 2^30; grouped: an empty list, a NULL pointer of a layer
 *   (bias excepted), N <= 0, n_merged outside 0 .. C.  N == 0 (pleas_dwconv2d_fwd): PLEAS_OK, nothing is enqueued.  A workspace
 *   that is NULL or smaller than the *_ws_bytes answer: PLEAS_ENOMEM.  *_ws_bytes returns 0 (message in pleas_last_error) for a
 *   list the launch would refuse on its geometry; it reads no pointer of a layer.  ws / ws_fresh as in pleas_gram_batch.
 * pleas_dwconv2d_fwd's `relu` is a PLEAS_ACT_* code: z = act(fma(y, scale[c], shift[c]) (+ res)); PLEAS_ACT_RELU6 gives pleas_bn_act's
 *   bits, a NaN included; the ReLU arm is fmaxf(v, 0) as in the dense epilogue.  y does not depend on the code. */
int pleas_dwconv2d_fwd(const float* x, const float* w, const float* bias, float* y, const float* scale, const float* shift,
                       const float* res, float* z, int relu, int N, int C, int Hin, int Win, int K, int stride, int pad,
                       void* stream);
typedef struct pleas_dw_layer {
    const float* ip;     /* [N][C][Hin][Win] merged input */
    const float* w;      /* [C][1][K][K] */
    const float* bias;   /* [C] or NULL */
    const float* o1;     /* [N][Csrc][Ho*Wo] source-layer outputs */
    const float* o2;
    const int32_t* row1; /* [C] block maps (DEVICE), -1 = absent */
    const int32_t* row2;
    float* resid;        /* [N][C][Ho*Wo] */
    int N, C, Hin, Win, K, stride, pad, Csrc, n_merged;
    float dscale, loss_scale;
} pleas_dw_layer;
size_t pleas_dw_fwd_batch_ws_bytes(const pleas_dw_layer* layers, int n_layers);
int pleas_dw_fwd_batch(const pleas_dw_layer* layers, int n_layers, float* loss, void* ws, size_t ws_bytes, int ws_fresh,
                       void* stream);
typedef struct pleas_dw_wgrad_layer {
    const float* resid;  /* [N][C][Ho*Wo] */
    const float* ip;     /* [N][C][Hin][Win] */
    float* grad;         /* [C][1][K][K] */
    int N, C, Hin, Win, K, stride, pad;
} pleas_dw_wgrad_layer;
size_t pleas_dw_wgrad_batch_ws_bytes(const pleas_dw_wgrad_layer* layers, int n_layers);
int pleas_dw_wgrad_batch(const pleas_dw_wgrad_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * Closed-form fit of depthwise layers (csrc/dw_normal_eq.hip): per-channel normal equations.  The objective of a depthwise layer
 * separates per channel; each channel is a least-squares problem in K*K (+ 1 with a bias) unknowns.
 * Per channel c and output pixel r = (n, oy, ox), v_r in R^D, D = K*K + 2:
 *   v_r[ky*K + kx] = ip[n][c][oy*stride + ky - pad][ox*stride + kx - pad] (0 outside the image; the layer's tap order),
 *   v_r[K*K] = 1,  v_r[K*K + 1] = tgt[n][c][oy][ox], the fp32 value pleas_merge_blocks stores for (o1, o2, row1, row2, n_merged):
 *   coef * ([row1[c] >= 0] o1 + [row2[c] >= 0] o2), coef = 0.5 below n_merged, the sum rounded to fp32 once; never materialised.
 * pleas_dw_normal_eq_accum: S[c] += sum_r v_r v_r^T for every listed layer, ONE grouped launch.  double S[C][D][D] row-major; only
 *   the LOWER triangle with the diagonal is written, the strict upper triangle is left untouched.  The entries: G (taps x taps),
 *   row K*K the column sums of U and the count M, row K*K + 1 h = sum u * t, sum t and sum t^2.  The bias column is always
 *   accumulated.  Two entries of one launch may not share an S.
 * Arithmetic: every fp32 x fp32 product exact in fp64 (v_mfma_f64_16x16x4_f64), every sum in fp64.
 * Determinism: no atomics; per (channel, slab of 4096 output pixels) partial tiles, then the slabs in slab order from 0 and S +=
 *   that sum; the split is a function of the geometry alone, grouped and alone give the same bits (header of the .hip file).
 * Limits, alignment and errors are those of pleas_dw_fwd_batch: K odd in 1 .. 7, stride 1 or 2, pad <= K / 2, every per-call element
 *   count below 2^30; ip, o1, o2 and S 16-byte aligned; EINVAL before anything is enqueued for an empty list, a NULL pointer, a
 *   misaligned base, N <= 0, n_merged outside 0 .. C, a refused geometry; a NULL or short workspace: PLEAS_ENOMEM.
 *   pleas_dw_normal_eq_ws_bytes is host only, reads no pointer of a layer, and returns 0 (message in pleas_last_error) for a list
 *   the launch would refuse on its geometry.  ws / ws_fresh as in pleas_gram_batch.
 * pleas_dw_normal_eq_solve: per channel, T = K*K + has_bias unknowns,  (G_T + ridge * mean(diag G_T) I) x = h_T  by fp64 Cholesky
 *   (the rule of pleas_cholesky_solve_batched; with a bias the count M is on the diagonal); x is rounded once to fp32 into w[c][:]
 *   (w [C][1][K][K]) and bias[c].  A pivot that is not positive sets status[c] = 1 and leaves that channel's w and bias untouched
 *   (an all-zero channel without bias); otherwise status[c] = 0.  S, w, bias, status: DEVICE memory; one wave per channel.
 * pleas_dw_normal_eq_solve_host: the same routine (csrc/dw_neq_solve.hpp) on HOST memory; `stream` is ignored. */
typedef struct pleas_dw_neq_layer {
    const float* ip;     /* [N][C][Hin][Win] merged input */
    const float* o1;     /* [N][Csrc][Ho*Wo] source-layer outputs */
    const float* o2;
    const int32_t* row1; /* [C] block maps (DEVICE), -1 = absent */
    const int32_t* row2;
    double* S;           /* [C][D][D], accumulated in place */
    int N, C, Hin, Win, K, stride, pad, Csrc, n_merged;
} pleas_dw_neq_layer;
size_t pleas_dw_normal_eq_ws_bytes(const pleas_dw_neq_layer* layers, int n_layers);
int pleas_dw_normal_eq_accum(const pleas_dw_neq_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh, void* stream);
int pleas_dw_normal_eq_solve(const double* S, int C, int K, int has_bias, double ridge, float* w, float* bias, int* status,
                             void* stream);
int pleas_dw_normal_eq_solve_host(const double* S, int C, int K, int has_bias, double ridge, float* w, float* bias, int* status,
                                  void* stream);

/* ------------------------------------------------------------------------------------
 * The path's exchange step under data parallelism (no reference counterpart -- the reference is
 * single-GPU): buf[0..n) := sum over the ranks of `comm`, in place, ONE RCCL all-reduce (fp32, sum) enqueued on `stream`.
 * What is exchanged: the flat cost arena of activation matching (all group matrices back to back, ResNet-101: 41 MB) before
 * the LAPs; the A / B arenas of the closed form before the solve; the gradient arena of an Adam update.
 * `comm` is the CALLER's ncclComm_t (RCCL is resolved at run time from the instance already loaded in the process, else
 * $PLEAS_RCCL_LIB, else librccl.so.1 -- a communicator is only valid in the library instance that created it).
 * The Python host side uses torch.distributed (backend "nccl" = RCCL) for the same step. */
int pleas_allreduce_sum(float* buf, int64_t n, void* comm, void* stream);

/* ------------------------------------------------------------------------------------
 * Normal equations of the per-layer PLeaS objective (closed form of what the reference's Adam
 * loop, pleas_merging.py:281-291 + :357-358, approximates):  W^T = A^-1 B  with
 *   A = sum_batches U^T U   (K x K, K = KH*KW*Cin, index k = (kh*KW + kw)*Cin + ci)
 *   B^T = sum_batches op . U  -> pleas_wgrad_batch(resid := op, flags = ACCUMULATE | KPOS_MAJOR).
 * pleas_normal_eq_accum adds one batch's U^T U of EVERY listed layer into its A (LOWER triangle of
 * 64/128-wide block tiles only -- see pleas_normal_eq_finalize for the blocks it leaves to that call; the strict
 * upper part of A is left untouched), one grouped
 * fp32-MFMA launch, U = im2col(ip) never materialised.  ws / ws_fresh as in pleas_gram_batch.
 */
typedef struct pleas_neq_layer {
    const float* ip; /* [N][Cin][Hin][Win] merged layer input */
    float* A;        /* [K][K] fp32, accumulated in place */
    int N, Cin, Hin, Win, KH, KW, stride, pad;
} pleas_neq_layer;
size_t pleas_normal_eq_ws_bytes(const pleas_neq_layer* layers, int n_layers);
int pleas_normal_eq_accum(const pleas_neq_layer* layers, int n_layers, void* ws, size_t ws_bytes, int ws_fresh,
                          void* stream);
/* Stride-1 "same" k x k layers: the block of A between two kernel positions depends only on their LAG and on which
 * border rows / columns the pair can reach, so the 45 lower-triangle blocks of a 3x3 layer hold 29 distinct matrices
 * (up to transposition).  pleas_normal_eq_accum contracts only those; pleas_normal_eq_finalize copies / transposes
 * them into the remaining blocks of the lower triangle.  Call it ONCE after the last batch (after the all-reduce of A
 * in a multi-GPU run) and before the solve; it overwrites (idempotent).  Layers of other geometries are left alone.
 * pleas_normal_eq_plan_info (host only, no GPU): info[0] = the path's flops per call (K^2 * N*HWo per layer),
 * info[1] = flops the grid executes, info[2] = work items, info[3] = blocks left to finalize. */
int pleas_normal_eq_finalize(const pleas_neq_layer* layers, int n_layers, void* stream);
int pleas_normal_eq_plan_info(const pleas_neq_layer* layers, int n_layers, double* info);
/* Host only (no GPU, pointers may be NULL): per layer what the plan builder of pleas_normal_eq_accum decides, five ints:
 * [0] the tile form `variant` (bit 0: 64-wide tiles, bit 1: 4-byte loads, bits 2-3: 0 direct (1x1, stride 1, no padding),
 * 1 shifted loader, 2 lag classes -- the values 0-3, 6-7, 8-11), [1] S, the slabs of the pixel axis, [2] tiles per side of a
 * block, [3] block tiles contracted, [4] blocks left to pleas_normal_eq_finalize.  A geometry the launch refuses is refused
 * with the same message. */
int pleas_normal_eq_layer_info(const pleas_neq_layer* layers, int n_layers, int* info);

/* Batched SPD solve of the normal equations (blocked Cholesky + forward/back substitution, panel 64,
 * trailing updates on fp32 MFMA tiles).  For every problem p:  X (A_p + lambda*mean(diag A_p) I) = Bt_p,
 * i.e. each of the N_p rows of Bt_p (length K_p) is one right-hand side and is overwritten by its
 * solution.  A_p: K_p x K_p row-major, LOWER triangle read; overwritten (L below the diagonal, L^T
 * above).  A, Bt, K, N: HOST arrays (of DEVICE pointers / sizes); info: DEVICE int[nprob], 0 = ok,
 * j > 0 = pivot j not positive in fp32 (the caller should redo that problem in higher precision).
 * N_p = 0 factors A_p only (Bt_p may then be null).
 * Problems of different sizes share the launches: cost = 5 * max(K)/64 launches per 96 problems.
 */
int pleas_cholesky_solve_batched(float* const* A, float* const* Bt, const int* K, const int* N, int nprob, float lambda,
                                 int* info, void* stream);

/* ------------------------------------------------------------------------------------
 * Opt-in live timing of the library's kernels with HIP events recorded on the launch stream
 * (used by bench.py for the roofline figure; off by default, no cost when off).
 * kernel ids: 0 gram_partial, 1 gram_finalize, 2 lsap, 3 merge_blocks, 4 masked_adam, 5 sqerr,
 *             6 conv_fwd, 7 conv_wgrad, 8 normal_eq, 9 solve, 10 bn_act.
 * pleas_prof_collect waits for the recorded events of that kernel and returns the number of
 * launches, their summed duration, and the summed ALGORITHMIC flops / bytes of those launches.
 */
void pleas_prof_enable(int on);
void pleas_prof_select(unsigned kernel_mask); /* bit k: record kernel id k (default all); many-launch kernels can be left out */
void pleas_prof_reset(void);
int pleas_prof_collect(int kernel, int64_t* launches, double* total_ms, double* flops, double* bytes);

/* Tuning hook for experiments (tools/hipbench): K chunks per work item of the grouped contraction (<= 0: unchanged) and its
 * item order, 0 = longest first, anything else = the XCD-aware order (< 0: unchanged). */
void pleas_gram_batch_tune(int item_chunks, int xcd_order);
/* Arithmetic of the contraction kernels (matching contraction, grouped forward, weight gradient, plain convolution).
 *   PLEAS_ARITH_FP32       (default) exact fp32 MFMA, v_mfma_f32_32x32x2_f32: bitwise an fmaf chain;
 *   PLEAS_ARITH_SPLIT_BF16 every fp32 operand as the exact sum of three bf16 values, six v_mfma_f32_32x32x16_bf16 products per
 *                          k step with fp32 accumulation.  The three dropped terms (x2 y3 + x3 y2 + x3 y3) sum to as much as
 *                          about 2^-25 .. 2^-24 of the product, half to one fp32 ulp: marginally narrower than an fmaf chain,
 *                          at 2.67x less matrix-pipe time.  Tile forms without a split variant (scalar-load forms: 7 x 7
 *                          images, strided layers, the stem) keep the exact arithmetic inside the same launch.
 *   PLEAS_ARITH_SPLIT_BF16_EXACT  the same split with all nine products: every bf16 x bf16 product is exact in fp32 and the
 *                          three planes sum exactly to the operand, so every fp32 product enters the sum exactly; the only
 *                          rounding is the fp32 accumulation (one per MFMA, 16 k deep).  1.78x less matrix-pipe time than
 *                          fp32 MFMA.  Same forms, plans, LDS images and exact-only forms as PLEAS_ARITH_SPLIT_BF16; kernels
 *                          of its own.
 * Any other value selects PLEAS_ARITH_FP32.  Process-wide; plans are keyed by it.  PLEAS_ARITH=split_bf16 (or 1) /
 * PLEAS_ARITH=split_bf16_exact (or 2) in the environment sets the initial value.  The headline numbers and every default-path
 * test run with PLEAS_ARITH_FP32; bench.py reports PLEAS_ARITH_SPLIT_BF16 as `alt_arith`. */
#define PLEAS_ARITH_FP32 0
#define PLEAS_ARITH_SPLIT_BF16 1
#define PLEAS_ARITH_SPLIT_BF16_EXACT 2
void pleas_arith(int mode);
int pleas_arith_get(void);

#ifdef __cplusplus
}
#endif
#endif /* PLEAS_HIP_H */
