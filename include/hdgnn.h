/*
 * hdgnn.h -- C ABI of the MI355X-native HD-GNN training-step engine (libhdgnn.so).
 *
 * The reference has no FFI: its only boundary is Python -> TF1 C++ runtime at
 * sess.run().  These entry points are what that boundary would bind for the
 * north-star path, one per sess.run() the reference issues:
 *
 *   hdg_train_step   sess.run([C_edge_output2, loss_Hedge_mse, loss_map, theta, trainer],
 *                             feed_dict)                      model_2.py:369-383
 *                    = hdg_fwd_bwd + hdg_adam_tf (single process)
 *   hdg_fwd_bwd      forward + backward of train_loss (model_2.py:336) -> flat gradient
 *                    of the data term + CE sum; the DP all-reduce sits between this
 *                    and hdg_adam_tf
 *   hdg_adam_tf      AdamOptimizer(0.0003).minimize(train_loss) (model_2.py:337-338):
 *                    adds the loss_para / loss_map gradients, applies TF1 ApplyAdam
 *   hdg_forward      sess.run([loss_Hedge_mse, loss_map, C_edge_output2], feed_dict)
 *                    model_2.py:486-502 (test path, forward only)
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer (the library never allocates);
 *     `stream` is a hipStream_t passed as void*; all work is enqueued on it, no host
 *     synchronisation happens inside any call (graph-capturable).  The one exception:
 *     `thresholds` of hdg_refine_ladder, hdg_refine_merge_ladder and
 *     hdg_refine_split_ladder is a HOST array, read during the call only.
 *   - return 0 on success, HDG_EINVAL for a shape/argument error, or the hipError_t
 *     of a failed launch; hdg_last_error() gives a thread-local message.
 *   - parameters are one flat fp32 vector in tf.global_variables() order with TF
 *     (in,out) row-major weights (hdg_param_count()).
 *   - the library keeps no global mutable state apart from the thread-local error and
 *     memos of per-device queries (kernel attributes set, occupancy per kernel and LDS
 *     size): idempotent, the same answer for every caller.
 */
#ifndef HDGNN_H
#define HDGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDG_ABI_VERSION 9
#define HDG_EINVAL 1000

/* Per-launch problem shape (one rank's share of the commit batch). */
typedef struct hdg_shape {
    int32_t batch;      /* commits in this call (Mini_batch per rank)              */
    int32_t ne;         /* entity nodes per commit   (main.py --Ne, 2 <= ne <= 4096) */
    int32_t nc;         /* hunk nodes per commit     (main.py --Nc, 2 <= nc <= 2048) */
    int32_t variant;    /* model_<variant>.py: 1 HD-GNN/ES, 2 HD-GNN/S, 3 HD-GNN/E,
                           4 HD-GNN                                      */
    int32_t batch_global; /* commits summed by the CE mean across all ranks         */
    int32_t path;       /* HDG_PATH_AUTO / _FUSED / _GENERAL (see below)           */
    int32_t flags;      /* HDG_FLAG_* bits, 0 for the defaults                      */
} hdg_shape;
/* HDG_FLAG_NO_SPLIT: the fused path runs one block per commit even where split mode
 * (two co-resident blocks per commit, see hdg_workspace_bytes) would apply: what a
 * caller retries with after HDG_STATUS_XCH_TIMEOUT.  Same results up to fp32
 * re-association of the block-pair sums.                                              */
#define HDG_FLAG_NO_SPLIT 1
/* General path, hunk pair sums of the first hunk MLP layer (forward relu sums, backward mask
 * sums): a dense sweep of the pair grid, or per-unit sorted thresholds (a binary search per
 * node and unit plus the label pairs one by one) from nc >= HDG_HUNK_SORTED_MIN_NC; these
 * flags force one form (same results up to fp32 re-association; the layout of
 * hdg_workspace_bytes follows the choice, so keep the flags fixed for a workspace).      */
#define HDG_FLAG_HUNK_DENSE 2
#define HDG_FLAG_HUNK_SORTED 4
/* HDG_FLAG_HUNK_TILED: the hunk pair passes (relu sums, MLP and classifier mask sums) as
 * one sweep over blocks of the pair grid giving row and column sums together (the fused
 * kernel's pair tiles), instead of a row pass and a column pass over every pair.        */
#define HDG_FLAG_HUNK_TILED 8
/* HDG_FLAG_HUNK_GROUP (ABI 9): the sorted form's per-node passes as one block per unit group
 * (their shape for nc > 512) at any nc; below that the default is one block for all 20 units,
 * which sums each node's label walk in two halves -- the two shapes differ by fp32
 * re-association only (a diagnostic / test flag).                                         */
#define HDG_FLAG_HUNK_GROUP 16
/* Without a form flag the general path picks by nc: tiled from HDG_HUNK_TILED_MIN_NC, sorted
 * from HDG_HUNK_SORTED_MIN_NC below that, dense otherwise (the measured crossovers at the
 * default 10% label density).                                              */
#define HDG_HUNK_SORTED_MIN_NC 384
#define HDG_HUNK_TILED_MIN_NC 1024

/* Engine paths.  FUSED: one block per commit with the commit's state in LDS; model_2
 * and model_4 with ne <= 256, nc <= 160 (the benchmark shapes; model_4's entity-edge
 * stage runs on the GENERAL path's kernels around the fused step kernel, so its prepared
 * tables and workspace hold both paths' parts).  GENERAL: one launch per phase, many
 * blocks per commit, state in HBM; every variant and shape.  AUTO picks FUSED when it
 * applies.  hdg_prep_bytes / hdg_workspace_bytes depend on the path. */
#define HDG_PATH_AUTO 0
#define HDG_PATH_FUSED 1
#define HDG_PATH_GENERAL 2

/* One batch of commits in compact device form (replaces the 12-tuple feed of
 * utils2.read_data, utils2.py:248-253, bit-exactly).       */
typedef struct hdg_batch {
    const float*    x;      /* [B][ne]     node attribute = diag(CAdjs)  (E_node_train)   */
    const uint32_t* abits;  /* [B][ne][ceil(ne/32)] entity class bits: bit j of row i =
                               (E_edge class of relation (i,j) == 1); diagonal bits 0     */
    const uint32_t* ybits;  /* [B][nc][ceil(nc/32)] hunk class bits (C_edge), diag 0      */
    const int32_t*  hid;    /* [B][ne] Esc/Etc hunk row of index line i' (-1 = none)      */
    const int32_t*  nlen;   /* [B] n = len(readlines()[:Ne]) of the commit's index file   */
    void*           prep;   /* hdg_prep_bytes(shape) of device scratch, filled once per
                               uploaded batch by hdg_prepare (sorted x, transposed bits,
                               cross-graph count matrices, per-node neighbour id lists);
                               read by every step after                                 */
} hdg_batch;

/* Adam / parameter state (all device, fp32). */
typedef struct hdg_state {
    float* params;       /* [P] */
    float* adam_m;       /* [P] */
    float* adam_v;       /* [P] */
    float* beta_pow;     /* [2] beta1^t, beta2^t (TF beta1_power/beta2_power vars) */
} hdg_state;

/* Per-step outputs (device). Any pointer may be NULL to skip that output. */
typedef struct hdg_outputs {
    float* probs;        /* [B][2][nc(nc-1)]  C_edge_output2        */
    float* logits;       /* [B][2][nc(nc-1)]  C_edge_output2_logits */
    float* stats;        /* [8] ce (loss_Hedge_mse), loss_map, loss_para, train_loss
                            (pre-update values, as sess.run returns them), then the
                            step's gradient trailer slots HDG_TR_COUNT..HDG_TR_FAULT
                            (top_ACC count parts, fault count): a training loop points
                            each step at its own row and reads a whole epoch at once  */
    uint32_t* status;    /* [1] sticky device status word: the library ORs HDG_STATUS_*
                            bits into it (write-through store) and never clears it; the
                            caller zeroes it and reads it whenever it synchronises     */
    float* ehr;          /* [1] loss_E_HR = 0.001 l2_loss(C_edge_output) of the call's
                            commits (model_2.py:122; computed by the reference graph but
                            fetched by neither of its sess.run calls): written by
                            hdg_forward only, ignored by the training entry points      */
} hdg_outputs;

/* Status bits (hdg_outputs.status).  HDG_STATUS_XCH_TIMEOUT: in the fused path's split
 * mode a block waited ~20 ms for its partner block's exchange words and gave up (the pair
 * was not co-resident: another process holding CUs, CU masking).  The launch's CE sum
 * is NaN; a forward-only launch also writes NaN over the timed-out block's probs / logits
 * rows; a training launch's gradient trailer carries the fault count (HDG_TR_FAULT) and
 * the Adam update of that step is skipped on every rank (parameters, moments and beta
 * powers unchanged).  Outputs of a launch with this bit set are void.                  */
#define HDG_STATUS_XCH_TIMEOUT 1u

/* Gradient trailer: hdg_fwd_bwd's grad buffer is [param_count + HDG_TRAILER] floats.
 * Every slot sums exactly under a float all-reduce (SUM) over up to 256 ranks.          */
#define HDG_TRAILER 8
#define HDG_TR_CE 0      /* CE sum over this call's relations                              */
#define HDG_TR_COUNT 1   /* slots 1..3: number of relations whose argmax prediction equals
                            the label (EvaluationFuncs.top_ACC numerator, np.argmax tie
                            rule), as three 16-bit parts: count = s1 + s2 2^16 + s3 2^32  */
#define HDG_TR_FAULT 4   /* blocks whose pair exchange timed out (0 = clean step)          */

int         hdg_version(void);
const char* hdg_last_error(void);
/* the path AUTO resolves to for this shape (HDG_PATH_FUSED / _GENERAL), or -1 */
int         hdg_resolve_path(const hdg_shape* shape);
/* flat parameter count of model_<variant> (SURVEY Appendix A order), or -1 (message in
 * hdg_last_error) for a variant outside 1..4                                         */
int         hdg_param_count(int32_t variant);
/* length of the gradient buffer hdg_fwd_bwd fills: param_count + HDG_TRAILER (the
 * trailer slots above); all-reduce the whole buffer.                                */
int         hdg_grad_len(int32_t variant);
/* Scratch the library carves per call (parked node rows, partial gradient rows, the
 * block-pair inboxes and per-commit launch epochs of the fused path's split mode).  Keep
 * it per shape across calls; its initial content does not matter (exchange tags derive
 * from the epoch word and differ from the word's own bit pattern, everything else is
 * written before it is read).  Split mode (two blocks per commit) runs whenever
 * 2 * batch <= the device's CU count and one 1024-thread block of the step kernel fits
 * a CU; HDG_FUSED_SPLIT=0 forces one block per commit.  The two blocks of a pair must
 * run at the same time: plain launches do not guarantee it, so a pair that cannot meet
 * is detected (HDG_STATUS_XCH_TIMEOUT) instead of producing silent garbage.          */
size_t      hdg_workspace_bytes(const hdg_shape* shape);
/* bytes of batch->prep for this shape (0 on a shape error).  It depends on the path the
 * shape resolves to (fused, fused + entity-edge, general), never on the flags: prepare a
 * batch with a shape that resolves to the same path as the steps that read it.      */
size_t      hdg_prep_bytes(const hdg_shape* shape);
/* Where hdg_prepare puts the cross-graph count tables of commit b inside batch->prep
 * (4-byte words from prep + b * stride_words): K_s at ks, K_t at kt (u16 [Nc][Ne]),
 * class counts at ncst (f32 [Nc][2]).  K_s = (Esc + Etc) . Es^T and K_t = (Esc + Etc) .
 * Et^T of utils2.py:111-137 (the marshalling_B2 maps, model_2.py:146-150), so tests can
 * check the index bookkeeping bit-exactly.  0, or an error code on a shape error.    */
int         hdg_prep_counts_layout(const hdg_shape* shape, int64_t* stride_words,
                                   int64_t* ks, int64_t* kt, int64_t* ncst);

/* Build batch->prep from x / abits / hid / nlen (the parameter-independent per-commit
 * tables the step kernel reads).  Call once after uploading a batch, before any step;
 * re-call whenever the batch contents change.  Replaces nothing in the reference: it is
 * the device-side half of the feed_dict marshalling (utils2.py:111-137, 248-253).    */
int hdg_prepare(const hdg_shape* shape, const hdg_batch* batch, void* stream);
/* Upload helper: a (batch, n, n) u8 class grid on the device (class of relation (i, j),
 * 0 or 1: the E_edge / C_edge one-hots of utils2.py:82, 105) -> the (batch, n,
 * ceil(n/32)) u32 bit rows hdg_batch.abits / ybits hold (bit j of row i = class 1,
 * diagonal cleared).  Lets a caller ship the compact grids and pack them on the GPU. */
int hdg_pack_classes(const uint8_t* cls, int32_t batch, int32_t n, uint32_t* bits,
                     void* stream);

int hdg_fwd_bwd(const hdg_shape* shape, const hdg_batch* batch, const float* params,
                float* grad, hdg_outputs* out, void* workspace, void* stream);

/* hdg_fwd_bwd with hipEvent_t events[3] recorded on `stream` before k_commit_step,
 * before k_grad_reduce and after it (per-kernel timing for bench.py; may be NULL). */
int hdg_fwd_bwd_events(const hdg_shape* shape, const hdg_batch* batch, const float* params,
                       float* grad, hdg_outputs* out, void* workspace, void* stream,
                       void* const* events);

/* hdg_fwd_bwd with per-kernel timing of every engine path (bench.py's roofline): events
 * [n_events] hipEvent_t; events[0] is recorded on `stream` before the first launch and
 * events[k + 1] right after the k-th kernel launch, whose name goes to names[k] (static
 * strings).  *n_kernels = the kernels bracketed (at most n_events - 1; later launches run
 * untimed).  Replaces nothing in the reference (its only clock is time.time(),
 * model_2.py:358, 423-424).                                                          */
int hdg_fwd_bwd_kernel_events(const hdg_shape* shape, const hdg_batch* batch,
                              const float* params, float* grad, hdg_outputs* out,
                              void* workspace, void* stream, void* const* events,
                              int32_t n_events, const char** names, int32_t* n_kernels);

/* Diagnostic: run k_commit_step alone with s_memrealtime (100 MHz) stamps at every
 * phase barrier, stamps[2B][32] (device; row = the block's partial-gradient row, 2b + h
 * in split mode).  Overwrites the workspace.                                        */
int hdg_debug_step_stamps(const hdg_shape* shape, const hdg_batch* batch, const float* params,
                         void* workspace, unsigned long long* stamps, void* stream);

/* TF ApplyAdam from an (all-reduced) gradient buffer; skips the whole update (parameters,
 * moments, beta powers) when grad[P + HDG_TR_FAULT] != 0.                            */
int hdg_adam_tf(const hdg_shape* shape, hdg_state* state, const float* grad,
                float lr, float* stats, void* stream);

int hdg_train_step(const hdg_shape* shape, const hdg_batch* batch, hdg_state* state,
                   float lr, hdg_outputs* out, float* grad, void* workspace, void* stream);

int hdg_forward(const hdg_shape* shape, const hdg_batch* batch, const float* params,
                hdg_outputs* out, float* ce_sum, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * On-device evaluation (csrc/eval.hip).  The reference scores a model on the host after
 * fetching every probability (EvaluationFuncs.py on C_edge_output2, model_2.py:486-548);
 * hdg_eval reduces the probabilities where they are to HDG_EV_SLOTS integers per commit,
 * from which accuracy, precision, recall, F1 and the exact ROC-AUC follow
 * (hdgnn.metrics.scores_from_counts): AUC of a commit = U2 / (2 P N), P = TP + FN,
 * N = FP + TN (ties count half, as sklearn.metrics.roc_auc_score).
 *
 *   probs   the [B][2][nc(nc-1)] array hdg_forward / hdg_fwd_bwd write (any device array
 *           of that shape); the score of relation r is probs[b][1][r]
 *   batch   only batch->ybits is read: the label of relation r = (i, j) (i = r / (nc-1),
 *           jj = r % (nc-1), j = jj + (jj >= i)) is bit j of ybits[b][i]
 *   ev      [batch][HDG_EV_SLOTS] u64, zeroed by the call itself
 * Predicted class 1 means p1 > p0 (np.argmax: a tie picks class 0, the rule of the
 * HDG_TR_COUNT trailer count, which TP + TN summed over the commits equals for a launch
 * without NaNs).  Only shape->batch and shape->nc are used.  Integer sums throughout: the
 * same bits on every run, whatever order the blocks run in.  One launch after a memset
 * node, no workspace, no host synchronisation.                                          */
#define HDG_EV_SLOTS 8
#define HDG_EV_TP 0      /* label 1, predicted 1                                   */
#define HDG_EV_FP 1      /* label 0, predicted 1                                   */
#define HDG_EV_FN 2      /* label 1, predicted 0                                   */
#define HDG_EV_TN 3      /* label 0, predicted 0                                   */
#define HDG_EV_U2 4      /* sum over (positive p, negative n) pairs of the commit of
                            2*[s_p > s_n] + [s_p == s_n], s = probs[b][1][r]       */
#define HDG_EV_NAN 5     /* relations with a NaN in either channel: counted here and
                            in no other slot, and in no pair                       */
#define HDG_EVAL_CHUNK 16384   /* relations per block: each block sorts the negatives of
                                  its chunk in LDS (64 KiB) and streams every positive of
                                  the commit past them                              */

int hdg_eval(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
             uint64_t* ev /* [batch][HDG_EV_SLOTS] */, void* stream);

/* ---------------------------------------------------------------------------------
 * On-device untangling (csrc/untangle.hip): from the same probabilities, per commit, WHICH
 * hunks belong together -- the groups the model is for (--Step is "the number of
 * commits/groups") -- and how well that partition matches the true one.  Not a reference
 * flow: the reference stops at the pair scores.
 *
 *   score    of the directed relation (p, q), p != q: s_pq = probs[b][1][r(p, q)] with
 *            r(p, q) = p (nc-1) + q - [q > p] (hdg_eval's layout); channel 0 is not read
 *   link     the unordered pair {p, q} is linked iff, by `rule`,
 *              HDG_UT_RULE_MEAN  fl32(s_pq + s_qp) > fl32(threshold + threshold)
 *                                (the right side once on the host; fp32 addition commutes, so
 *                                the rule is symmetric bit for bit, and nothing is multiplied)
 *              HDG_UT_RULE_ANY   s_pq > threshold || s_qp > threshold
 *              HDG_UT_RULE_BOTH  s_pq > threshold && s_qp > threshold
 *            every comparison is strict (a score equal to the threshold does not link).  A
 *            pair with a NaN in either direction is never linked and counts in HDG_UT_NAN,
 *            under every rule
 *   groups   predicted groups = connected components of the link graph; true groups =
 *            connected components of the label graph y_pq | y_qp from batch->ybits (bit j of
 *            row i; bits at j >= nc or j == i are not relations and are ignored, as hdg_eval)
 *   ids      dense, 0 .. G-1, ordered by each group's smallest member: the id of a group is
 *            the number of groups whose smallest member is smaller, so hunk 0 is always in
 *            group 0 and the output is unique (device and host compare for equality).
 *            Padded hunks are ordinary nodes: singletons on both sides
 *   groups   [batch][nc] i32 predicted id per hunk; tgroups the true ids, or NULL
 *   ut       [batch][HDG_UT_SLOTS] u64, every slot written by the call (nothing to zero)
 *   workspace  hdg_untangle_workspace_bytes(shape) bytes; its content before the call does
 *            not matter
 * Two launches on `stream` (k_ut_link: a commit's blocks sweep 64 x 64 tiles of the
 * pair grid into block-local union-find forests; k_ut_close: one block per commit merges
 * them, labels both partitions and counts the pairs), no host synchronisation, no block
 * waits for another, integer results: the same bits on every run.  Blocks per commit depend
 * on nc alone: T = ceil(nc / 64) tile rows, T (T + 1) / 2 tile pairs I <= J,
 * min(ceil(pairs / HDG_UT_TILES_PER_BLOCK), HDG_UT_MAX_BLOCKS) blocks, tile pair k (row-major
 * over I <= J) on block k mod blocks.  Only shape->batch and shape->nc are used, and of the
 * batch only ybits.  HDG_EINVAL (message in hdg_last_error) for batch outside [1, 65535], nc
 * outside [2, 2048], an unknown rule, a NaN threshold, or a NULL probs, groups, ut,
 * workspace or ybits.                                                                   */
#define HDG_UT_SLOTS 8
#define HDG_UT_GROUPS 0    /* number of predicted groups                                 */
#define HDG_UT_TGROUPS 1   /* number of true groups                                      */
#define HDG_UT_SS 2        /* unordered pairs p < q in the same predicted group and the
                              same true group                                            */
#define HDG_UT_SD 3        /* same predicted group, different true groups                */
#define HDG_UT_DS 4        /* different predicted groups, same true group                */
#define HDG_UT_DD 5        /* different in both: SS + SD + DS + DD = nc (nc-1) / 2       */
#define HDG_UT_LINKS 6     /* linked unordered pairs                                     */
#define HDG_UT_NAN 7       /* unordered pairs with a NaN score in either direction       */
#define HDG_UT_RULE_MEAN 0
#define HDG_UT_RULE_ANY 1
#define HDG_UT_RULE_BOTH 2
#define HDG_UT_TILE 64             /* hunks per tile side                                */
#define HDG_UT_TILES_PER_BLOCK 4   /* tile pairs a block takes before a commit gets more
                                      blocks                                             */
#define HDG_UT_MAX_BLOCKS 16       /* ... up to this many per commit                     */

size_t hdg_untangle_workspace_bytes(const hdg_shape* shape);   /* 0 on a shape error */
int    hdg_untangle(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                    float threshold, int32_t rule,
                    int32_t* groups   /* [batch][nc] */,
                    int32_t* tgroups  /* [batch][nc] or NULL */,
                    uint64_t* ut      /* [batch][HDG_UT_SLOTS] */,
                    void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * On-device linkage (csrc/linkage.hip): the partition hdg_untangle gives is a step function
 * of the threshold; hdg_linkage returns all its steps at once -- the single-linkage merge
 * tree of each commit and the pair counts of every cut -- so the best threshold of a whole
 * split follows on the host from nc - 1 rows per commit (hdgnn.metrics.best_threshold) and
 * the probabilities never leave the device.
 *
 *   weight   of the unordered pair {p, q}, p < q, from hdg_untangle's scores s_pq, by `rule`:
 *              HDG_UT_RULE_MEAN  w = fl32(s_pq + s_qp)
 *              HDG_UT_RULE_ANY   w = max(s_pq, s_qp)
 *              HDG_UT_RULE_BOTH  w = min(s_pq, s_qp)
 *            a pair with a NaN in either direction is not an edge and counts in HDG_LK_NAN
 *            (so does a pair whose weight is NaN from +inf and -inf under MEAN, which
 *            hdg_untangle never links either but does not count in HDG_UT_NAN); a weight of
 *            -0 is taken as +0.  hdg_untangle links {p, q} exactly when w > t',
 *            t' = fl32(threshold + threshold) under MEAN and t' = threshold otherwise, so the
 *            link graphs are the same
 *   order    edges are ordered by (w descending, p ascending, q ascending): a total order
 *   merges   the maximum spanning forest under that order is unique; its M <= nc - 1 edges in
 *            that order (Kruskal's acceptance order) are the commit's merges, level[k] the
 *            weight of merge k
 *   cuts     after merges 0 .. k the partition is that of the link graph's components for
 *            every t' with level[k+1] <= t' < level[k] (level[M] = -inf).  A state k with
 *            level[k+1] == level[k] is reached by no threshold, nor is a merge at level -inf
 *
 *   merges   [batch][nc-1][2] i32, (p_k, q_k) with p < q; rows k >= M hold -1
 *   levels   [batch][nc-1] f32; rows k >= M hold NaN
 *   curve    [batch][nc-1][2] u32, (SP_k, SS_k): the unordered pairs in the same predicted
 *            group after merges 0 .. k, and those of them that are also in the same true
 *            group (true groups as hdg_untangle's); rows k >= M repeat row M - 1, or hold 0
 *            when M = 0.  The group count after merge k is nc - (k + 1)
 *   tgroups  [batch][nc] i32 true group ids as hdg_untangle's, or NULL
 *   lk       [batch][HDG_LK_SLOTS] u64; with it DS_k = ST - SS_k, SD_k = SP_k - SS_k and
 *            DD_k = PAIRS - SP_k - ST + SS_k
 *   workspace  hdg_linkage_workspace_bytes(shape) bytes, 8-byte aligned; its content before
 *            the call does not matter
 * Every slot of every output is written by the call (nothing to zero).  Two launches on
 * `stream` (k_lk_forest: hdg_untangle's blocks and tile pairs, each block reducing its tiles
 * to a spanning forest by Boruvka rounds in LDS; k_lk_close: one block per commit reduces
 * the blocks' forests to the commit's, sorts it, orders the hunks as the dendrogram's
 * leaves and counts the pairs each merge joins), no host synchronisation, no block waits for
 * another, no float atomics: the same bits on every run.  Only shape->batch, shape->nc and
 * batch->ybits are read.  HDG_EINVAL (message in hdg_last_error) as hdg_untangle, without a
 * threshold: batch outside [1, 65535], nc outside [2, 2048], an unknown rule, a NULL probs,
 * merges, levels, curve, lk, workspace or ybits, or a workspace that is not 8-byte aligned. */
#define HDG_LK_SLOTS 8
#define HDG_LK_MERGES 0    /* M: edges of the commit's spanning forest                   */
#define HDG_LK_TGROUPS 1   /* number of true groups                                      */
#define HDG_LK_ST 2        /* unordered pairs in the same true group                     */
#define HDG_LK_NAN 3       /* unordered pairs that are not edges (a NaN score)           */
#define HDG_LK_PAIRS 4     /* nc (nc-1) / 2; slots 5 .. 7 are written as 0               */

size_t hdg_linkage_workspace_bytes(const hdg_shape* shape);    /* 0 on a shape error */
int    hdg_linkage(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                   int32_t rule,
                   int32_t* merges   /* [batch][nc-1][2] */,
                   float* levels     /* [batch][nc-1] */,
                   uint32_t* curve   /* [batch][nc-1][2] */,
                   int32_t* tgroups  /* [batch][nc] or NULL */,
                   uint64_t* lk      /* [batch][HDG_LK_SLOTS] */,
                   void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * On-device agglomeration (csrc/agglo.hip): hdg_linkage's tree is single linkage, which
 * chains -- one wrong high score between two groups fuses them at every threshold below
 * it.  hdg_agglomerate builds the merge tree of each commit under single, complete or
 * average linkage (UPGMA) in hdg_linkage's output format, and hdg_cut turns any such tree
 * into groups at a threshold, so best_threshold, cut_table and calibration apply unchanged.
 *
 *   weight   w of the unordered pair {p, q} under `rule`, and the pairs that are not edges:
 *            exactly hdg_linkage's (a NaN score in either direction, NaN from +inf and -inf
 *            under MEAN, -0 taken as +0; they count in HDG_LK_NAN)
 *   clusters start as the nc singletons; a cluster is named by its smallest member.  The
 *            similarity D(A, C) of two clusters, by `method`:
 *              HDG_AG_SINGLE    the largest weight over the pairs between them that are
 *                               edges; no edge when none of them is
 *              HDG_AG_COMPLETE  the smallest weight over the pairs between them; no edge when
 *                               any pair between them is no edge
 *              HDG_AG_AVERAGE   v = (double)S / (double)(|A| |C|), one IEEE double division;
 *                               S of two singletons is the pair's fp32 weight and
 *                               S(A u C, X) = fl32(S(A, X) + S(C, X)), one fp32 addition
 *                               (commutative: the value depends on the merge tree alone); no
 *                               edge when either summand is no edge or the sum is NaN
 *   step     among all cluster pairs (a, c), a < c, that have an edge, the first under
 *            (D descending, a ascending, c ascending) -- under AVERAGE D is compared as the
 *            double v -- merges: a absorbs c.  Its raw level r_k is D as fp32 ((float)v under
 *            AVERAGE); merges[k] = (a, c), levels[k] = min(r_0 .. r_k).  Steps repeat until no
 *            cluster pair has an edge: M <= nc - 1
 *   levels   are non-increasing by construction.  Under SINGLE and COMPLETE the raw levels
 *            already are; under AVERAGE they can invert by an ulp through the fp32 sums.
 *            With the running minimum "the merges with level > t'" is a prefix of the merges:
 *            what a greedy agglomeration stopped at the first best similarity <= t' has done
 *   curve, tgroups, lk and the padding of rows k >= M: hdg_linkage's, slot for slot
 *   SINGLE   gives hdg_linkage's levels bit for bit and its curve at every k with
 *            level[k+1] < level[k]; the merge pairs differ (cluster minima here, edge ends
 *            there)
 *   workspace  hdg_agglomerate_workspace_bytes(shape, flags) bytes (batch * nc * nc floats),
 *            8-byte aligned; its content before the call does not matter
 * Three launches on `stream`: k_ag_weights (one block per 64 x 64 tile pair of a commit,
 * hdg_untangle's staging) writes the commit's pair weights, packed by rows of the upper
 * triangle, into the commit's region of the workspace; k_ag_merge, one block per commit,
 * keeps the cluster-pair matrix in LDS for nc <= HDG_AG_LDS_MAX_NC and works on the
 * workspace copy above that (HDG_AG_FLAG_GLOBAL forces the latter at any nc: a test and
 * diagnostic flag, the results are bit-identical), each live row caching its best partner;
 * k_ag_close is hdg_linkage's closing phase.  No host synchronisation, no block waits for
 * another, no float atomics: the same bits on every run.  The step loop is bounded by
 * nc - 1 and every inner loop by nc.  Only shape->batch, shape->nc and batch->ybits are
 * read.  Every slot of every output is written by the call.  HDG_EINVAL (message in
 * hdg_last_error) for what hdg_linkage rejects, an unknown method or an unknown flag bit;
 * nothing is launched then.                                                               */
#define HDG_AG_SINGLE 0
#define HDG_AG_COMPLETE 1
#define HDG_AG_AVERAGE 2
#define HDG_AG_FLAG_GLOBAL 1       /* keep the cluster-pair matrix in the workspace        */
#define HDG_AG_LDS_MAX_NC 256      /* largest nc whose matrix k_ag_merge keeps in LDS: 32640
                                      floats of the 160 KiB, the rest for its row caches   */

/* 0 on a shape error only; the size is the same under every flag */
size_t hdg_agglomerate_workspace_bytes(const hdg_shape* shape, int32_t flags);
int    hdg_agglomerate(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                       int32_t rule, int32_t method, int32_t flags,
                       int32_t* merges   /* [batch][nc-1][2] */,
                       float* levels     /* [batch][nc-1] */,
                       uint32_t* curve   /* [batch][nc-1][2] */,
                       int32_t* tgroups  /* [batch][nc] or NULL */,
                       uint64_t* lk      /* [batch][HDG_LK_SLOTS] */,
                       void* workspace, void* stream);

/* hdg_cut: the groups of a merge tree (hdg_linkage's or hdg_agglomerate's) at a threshold.
 * With t' from (threshold, rule) as hdg_untangle forms it (fl32(threshold + threshold) under
 * MEAN, threshold otherwise), per commit the merges with levels[k] > t' are united; rows of
 * -1 / NaN are skipped.  groups gets hdg_untangle's dense ids, ordered by smallest member.
 * With `ut` given, `curve` and `lk` are required and the row holds hdg_untangle's slots
 * (HDG_CUT_GROUPS .. HDG_CUT_DD as HDG_UT_GROUPS .. HDG_UT_DD) read off curve[k-1] and lk
 * for the k merges done -- except slot HDG_CUT_MERGES, which holds k (a tree does not know
 * the linked pairs), and HDG_CUT_NAN, which is lk's HDG_LK_NAN (it also counts a pair of
 * +inf and -inf under MEAN, which HDG_UT_NAN does not).  On hdg_linkage's tree the groups
 * and the other slots are hdg_untangle's at the same threshold.  One launch, one block per
 * commit, only shape->batch and shape->nc are read.  HDG_EINVAL for a bad shape, a NaN
 * threshold, an unknown rule, a NULL merges, levels or groups, or ut without curve and lk. */
#define HDG_CUT_SLOTS 8
#define HDG_CUT_GROUPS 0
#define HDG_CUT_TGROUPS 1
#define HDG_CUT_SS 2
#define HDG_CUT_SD 3
#define HDG_CUT_DS 4
#define HDG_CUT_DD 5
#define HDG_CUT_MERGES 6   /* merges done: the rows with level > t'                      */
#define HDG_CUT_NAN 7      /* lk's HDG_LK_NAN                                            */

int    hdg_cut(const hdg_shape* shape, const int32_t* merges, const float* levels,
               const uint32_t* curve /* or NULL */, const uint64_t* lk /* or NULL */,
               float threshold, int32_t rule,
               int32_t* groups   /* [batch][nc] */,
               uint64_t* ut      /* [batch][HDG_CUT_SLOTS] or NULL */,
               void* stream);

/* ---------------------------------------------------------------------------------
 * On-device refinement (csrc/refine.hip): every decode above is greedy -- a merge is never
 * undone, so a wrong pair with the highest score of a commit is merged first by every tree
 * and no threshold repairs it.  hdg_refine is local search on the objective the linkages
 * approximate (correlation clustering: the sum of w_pq - t' over the pairs kept in one
 * group), from any starting partition: best-move sweeps over the hunks.  Device and host
 * (hdgnn.metrics.refine) agree integer for integer.
 *
 *   weight   w of the unordered pair {p, q} under `rule`, and the pairs that are no edge:
 *            exactly hdg_linkage's (they count in HDG_RF_NAN as in HDG_LK_NAN)
 *   bound    t' as hdg_untangle and hdg_cut form it, once on the host:
 *            fl32(threshold + threshold) under MEAN, threshold otherwise; it must be finite
 *   gain     a_pq = a_qp, fixed point: d = fl32(w - t'), one fp32 subtraction, and
 *            a = (int32) rintf(fminf(fmaxf(d, -2.f), 2.f) * 262144.f).  The scale is a power of
 *            two, so only rintf (ties to even) rounds.  A pair that is no edge has a = 0, and
 *            so has the diagonal.  |a| <= 2^19, so a sum over at most 2047 partners stays
 *            below 2^31: node sums are int32, totals int64, and every result is independent
 *            of the order of summation.  For probabilities the clamp never binds under any
 *            rule; pairs within 2^-19 of t' are neutral
 *   start    with groups_in NULL every hunk starts alone; otherwise hunks with the same id in
 *            [0, nc) start together and a hunk whose id is outside [0, nc) starts alone (no
 *            id is used as an index before it is range-checked).  Groups live in slots
 *            0 .. nc-1; a starting group sits in the slot of its smallest member, so the
 *            numbering of the input does not matter
 *   Q        the sum of a_pq over the pairs p < q in the same slot
 *   sweep    visits p = 0, 1, .., nc-1 in that order, each visit seeing the moves of the
 *            earlier visits of the same sweep.  For p in slot g and any slot h, S[h] is the
 *            sum of a_pq over the q != p in slot h.  The candidates: stay, at S[g]; every
 *            other non-empty slot h, at S[h]; if p is not alone in g, the smallest empty slot,
 *            at 0.  p moves only to a candidate whose value is strictly above S[g], and to the
 *            largest such value; among equal non-empty slots the lowest slot number wins, and
 *            a non-empty slot beats the empty one at equal value
 *   stop     after the first sweep without a move, or after max_sweeps sweeps, max_sweeps in
 *            [1, HDG_RF_MAX_SWEEPS].  Every move raises Q by at least 1, so the process ends
 *            without the cap; the cap bounds the kernel
 *   groups   [batch][nc] i32, hdg_untangle's dense ids ordered by each group's smallest
 *            member; may be the same array as groups_in
 *   ut       [batch][HDG_RF_SLOTS] u64: slots 0 .. 5 are HDG_UT_GROUPS .. HDG_UT_DD of the final
 *            partition against the true groups from batch->ybits (true groups as
 *            hdg_untangle's), then HDG_RF_MOVES and HDG_RF_NAN
 *   rq       [batch][HDG_RF_Q_SLOTS] i64: Q at the start, Q at the end, the sweeps run (the
 *            final sweep without a move counts), and 1 if the last sweep made no move, else 0
 *   workspace  hdg_refine_workspace_bytes(shape, flags) bytes (per commit nc * nc gains and
 *            one count per tile pair), 8-byte aligned; its content before the call does not
 *            matter
 * Every slot of every output is written by the call.  Two launches on `stream`: k_rf_weights
 * (one block per 64 x 64 tile pair of a commit, hdg_agglomerate's staging) writes the gains as
 * a full nc x nc int32 matrix, both triangles, into the commit's region of the workspace;
 * k_rf_sweep, one block per commit, keeps slots, sizes and the per-slot sums in LDS and reads
 * row p of the matrix one step ahead: per step an int32 LDS atomic add per hunk, a block
 * arg-max under the tie rules above, and one move.  The matrix has one home, the workspace,
 * and no flag is defined.  No host synchronisation, no block waits for another, no float
 * atomics: the same bits on every run.  The sweep loop is bounded by max_sweeps, the step
 * loop by nc and every inner loop by nc.  Only shape->batch, shape->nc and batch->ybits are
 * read.  HDG_EINVAL (message in hdg_last_error) for what hdg_untangle rejects, a NULL groups,
 * ut, rq or workspace, a workspace that is not 8-byte aligned, max_sweeps out of range, any
 * flag bit, or a threshold or t' that is not finite; nothing is launched then.            */
#define HDG_RF_SLOTS 8
#define HDG_RF_MOVES 6         /* moves made                                               */
#define HDG_RF_NAN 7           /* unordered pairs that are no edge: HDG_LK_NAN's count      */
#define HDG_RF_Q_SLOTS 4
#define HDG_RF_Q_START 0       /* Q of the starting partition                              */
#define HDG_RF_Q_END 1         /* Q of the final partition                                 */
#define HDG_RF_Q_SWEEPS 2      /* sweeps run                                               */
#define HDG_RF_Q_CONVERGED 3   /* 1: the last sweep made no move                           */
#define HDG_RF_MAX_SWEEPS 64

size_t hdg_refine_workspace_bytes(const hdg_shape* shape, int32_t flags);   /* 0 on a shape error */
int    hdg_refine(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                  float threshold, int32_t rule, int32_t max_sweeps, int32_t flags,
                  const int32_t* groups_in /* [batch][nc] or NULL */,
                  int32_t* groups          /* [batch][nc] */,
                  uint64_t* ut             /* [batch][HDG_RF_SLOTS] */,
                  int64_t* rq              /* [batch][HDG_RF_Q_SLOTS] */,
                  void* workspace, void* stream);

/* hdg_refine_ladder: hdg_refine at every rung of a ladder of thresholds in one call, each
 * rung starting from the cut of a merge tree at that rung -- what calibrating a threshold for
 * the refined result needs (hdgnn.metrics.refine_ladder restates it, metrics.best_rung picks).
 *
 *   thresholds  a HOST array of n_rungs floats, n_rungs in [1, HDG_RL_MAX_RUNGS]: the one
 *            argument of this header that is not a device pointer.  It is read during the
 *            call only; each rung's t' is formed once on the host exactly as hdg_refine forms
 *            it, and the bounds travel to the kernel as a by-value argument.  Rungs need not be
 *            sorted or distinct; each threshold and each t' must be finite
 *   start    with merges ([batch][nc-1][2]) and levels ([batch][nc-1]) of hdg_linkage or
 *            hdg_agglomerate given, rung k starts from the groups hdg_cut gives on that tree
 *            at thresholds[k] under `rule` (the merges with level > t' united, rows of -1 /
 *            NaN skipped); with both NULL every hunk starts alone, as hdg_refine with
 *            groups_in NULL.  One without the other is an error
 *   outputs  rung k of groups ([n_rungs][batch][nc], or NULL: not stored), ut
 *            ([n_rungs][batch][HDG_RF_SLOTS]) and rq ([n_rungs][batch][HDG_RF_Q_SLOTS]) holds,
 *            integer for integer and slot for slot, what hdg_cut(merges, levels,
 *            thresholds[k], rule) followed by hdg_refine(thresholds[k], rule, max_sweeps,
 *            groups_in = those groups) writes -- or hdg_refine with groups_in NULL without a
 *            tree.  Weights, pairs that are no edge, gains, tie rules, sweep order, stop rule
 *            and every slot are hdg_refine's, above
 *   workspace  hdg_refine_ladder_workspace_bytes(shape, flags) bytes, hdg_refine's size
 *            whatever n_rungs is, 8-byte aligned; its content before the call does not matter
 * Every slot of every rung is written by the call.  Two launches on `stream`: k_rl_weights is
 * k_rf_weights storing the fp32 weight of every pair (one canonical NaN for a pair that is no
 * edge and on the diagonal) instead of its gain at one bound; the sweep kernel runs
 * k_rf_sweep's block on a grid (n_rungs, batch), forming a_pq from the stored weight and its
 * rung's t' with hdg_refine's own expression -- the same function of the same w, so no new
 * rounding -- after uniting the tree's merges above t' in LDS as hdg_cut does.  The call
 * allocates nothing, does not synchronise, no block waits for another; it is graph-capturable,
 * and a captured graph replays the captured ladder (the bounds are part of the launch).  The
 * sweep loop is bounded by max_sweeps, the step loop by nc, the unions by nc - 1.  HDG_EINVAL
 * (the message starts "hdg_refine_ladder:"; nothing is launched) for everything hdg_refine
 * rejects except a NULL groups, n_rungs out of range, a NULL thresholds, a rung whose
 * threshold or t' is not finite (the message names the rung), exactly one of merges and
 * levels, or any flag bit.                                                                */
#define HDG_RL_MAX_RUNGS 64

size_t hdg_refine_ladder_workspace_bytes(const hdg_shape* shape, int32_t flags);   /* 0 on a shape error */
int    hdg_refine_ladder(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                         const float* thresholds /* HOST, [n_rungs] */, int32_t n_rungs,
                         int32_t rule, int32_t max_sweeps, int32_t flags,
                         const int32_t* merges /* [batch][nc-1][2] or NULL */,
                         const float* levels   /* [batch][nc-1]    or NULL */,
                         int32_t* groups  /* [n_rungs][batch][nc] or NULL */,
                         uint64_t* ut     /* [n_rungs][batch][HDG_RF_SLOTS] */,
                         int64_t* rq      /* [n_rungs][batch][HDG_RF_Q_SLOTS] */,
                         void* workspace, void* stream);

/* hdg_refine_merge, hdg_refine_merge_ladder: hdg_refine and hdg_refine_ladder with ROUNDS.
 * hdg_refine's only move is one hunk to another slot, so two groups that belong together but
 * are each internally tight stay apart: every single hunk loses more by leaving its half than
 * it gains from the other, no move is accepted and the search reports "converged".  A round
 * is hdg_refine's node sweeps followed by one GROUP SWEEP, in which whole groups merge
 * (hdgnn.metrics.refine_merge and refine_merge_ladder restate the calls, integer for integer).
 * Everything not restated here -- weights, pairs that are no edge, the gain a_pq, the bound t',
 * the start and the slots, the node sweep and its tie rules, the dense output ids, the ut row
 * and its HDG_RF_NAN count -- is hdg_refine's, above.
 *
 *   group sweep  visits the slots g = 0, 1, .., nc-1 in that order, each visit seeing the merges
 *            of the earlier visits of the same sweep.  A slot that is empty when its turn
 *            comes is skipped.  For a non-empty g and every other non-empty slot h,
 *            C[h] = the sum of a_pq over p in g and q in h (int64; a pair that is no edge adds
 *            0).  If the largest C[h] is strictly above 0, g merges with that h; among equal
 *            values the lowest h wins.  The members of slot max(g, h) move into slot
 *            min(g, h), and Q rises by C[h].  One merge per visit; there is no empty-slot
 *            candidate
 *   bounds   |C| <= (nc / 2)^2 * 2^19 <= 2^39, so a 64-bit key holds the value biased by 2^40
 *            and an 11-bit tie field
 *   rounds   max_sweeps in [1, HDG_RF_MAX_SWEEPS] is the call's total budget of node sweeps,
 *            max_rounds is in [1, HDG_RM_MAX_ROUNDS].  Repeat: (1) the node phase, hdg_refine's
 *            sweeps until a sweep makes no move or the total of sweeps reaches max_sweeps;
 *            (2) one group sweep; (3) stop if that group sweep merged nothing, or max_rounds
 *            rounds have run, or the total of sweeps has reached max_sweeps.  Every move and
 *            every merge raises Q by at least 1
 *   rq       rows of HDG_RM_Q_SLOTS i64: slots 0 .. 3 as HDG_RF_Q_START / END / SWEEPS /
 *            CONVERGED, where SWEEPS is the total of node sweeps and CONVERGED is 1 iff the
 *            last node phase ended on a sweep without a move and the last group sweep merged
 *            nothing; then HDG_RM_Q_ROUNDS, HDG_RM_Q_MERGES, HDG_RM_Q_NODE (Q after the first
 *            node phase) and one slot written as 0
 *   ut       hdg_refine's row of the final partition; HDG_RF_MOVES counts node moves only
 * Two consequences: (A) the state after the first node phase is exactly hdg_refine's final
 * state at the same max_sweeps, so HDG_RM_Q_NODE equals hdg_refine's HDG_RF_Q_END, and if the
 * first group sweep merges nothing then groups, ut and rq[0 .. 3] equal hdg_refine's, with
 * ROUNDS = 1 and MERGES = 0; (B) Q_END - Q_NODE >= MERGES.
 * hdg_refine_merge_ladder: rung k of groups ([n_rungs][batch][nc], or NULL), ut
 * ([n_rungs][batch][HDG_RF_SLOTS]) and rq ([n_rungs][batch][HDG_RM_Q_SLOTS]) holds, integer
 * for integer, what hdg_cut(merges, levels, thresholds[k], rule) followed by
 * hdg_refine_merge(thresholds[k], rule, max_sweeps, max_rounds, groups_in = those groups)
 * writes -- or hdg_refine_merge with groups_in NULL without a tree; thresholds is a HOST array
 * as hdg_refine_ladder's.
 * The workspaces are hdg_refine_workspace_bytes and hdg_refine_ladder_workspace_bytes.  Two
 * launches each: the weights kernel of hdg_refine / hdg_refine_ladder, unchanged, and the
 * sweep block with rounds (k_rm_sweep, k_rml_sweep).  In a group sweep the members of every
 * slot are chained in LDS once; a visit sums the rows of g's members per hunk in registers
 * (int32), then per slot with two int32 LDS atomics on a 16-bit split (exact), picks the block
 * maximum of the keys, and a merge appends one chain to the other: at most nc row reads per
 * group sweep and two barriers per non-empty slot.  The round loop is bounded by max_rounds,
 * the visits by nc, a chain walk by the slot's size, the total of sweeps by max_sweeps.  No
 * host synchronisation, no block waits for another, no float atomics, no allocation:
 * graph-capturable, the same bits on every run.  HDG_EINVAL (the message starts
 * "hdg_refine_merge:" or "hdg_refine_merge_ladder:"; nothing is launched) for everything
 * hdg_refine or hdg_refine_ladder rejects, max_rounds out of range, or any flag bit.       */
#define HDG_RM_Q_SLOTS 8
#define HDG_RM_Q_ROUNDS 4      /* rounds run                                               */
#define HDG_RM_Q_MERGES 5      /* merges made by the group sweeps                          */
#define HDG_RM_Q_NODE 6        /* Q after the first node phase                             */
#define HDG_RM_MAX_ROUNDS 16

int    hdg_refine_merge(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                        float threshold, int32_t rule, int32_t max_sweeps, int32_t max_rounds,
                        int32_t flags,
                        const int32_t* groups_in /* [batch][nc] or NULL */,
                        int32_t* groups          /* [batch][nc] */,
                        uint64_t* ut             /* [batch][HDG_RF_SLOTS] */,
                        int64_t* rq              /* [batch][HDG_RM_Q_SLOTS] */,
                        void* workspace, void* stream);
int    hdg_refine_merge_ladder(const hdg_shape* shape, const hdg_batch* batch,
                               const float* probs,
                               const float* thresholds /* HOST, [n_rungs] */, int32_t n_rungs,
                               int32_t rule, int32_t max_sweeps, int32_t max_rounds,
                               int32_t flags,
                               const int32_t* merges /* [batch][nc-1][2] or NULL */,
                               const float* levels   /* [batch][nc-1]    or NULL */,
                               int32_t* groups  /* [n_rungs][batch][nc] or NULL */,
                               uint64_t* ut     /* [n_rungs][batch][HDG_RF_SLOTS] */,
                               int64_t* rq      /* [n_rungs][batch][HDG_RM_Q_SLOTS] */,
                               void* workspace, void* stream);

/* hdg_refine_split, hdg_refine_split_ladder: the rounds of hdg_refine_merge with a third move,
 * the SPLIT of one group in two.  Single linkage, or a tree cut below the right threshold,
 * fuses two tight groups through one wrong high score; a hunk of such a group keeps a positive
 * sum towards it (its own half outweighs the other), so it never leaves for the empty slot,
 * group sweeps only merge, and the search reports "converged" although cutting the group would
 * raise Q by the negative sum between the halves.  A SPLIT SWEEP bisects a slot from two seeds
 * (hdgnn.metrics.refine_split and refine_split_ladder restate the calls, integer for integer).
 * Everything not restated here is hdg_refine's and hdg_refine_merge's, above: weights, pairs
 * that are no edge, a_pq, t', the start and the slots, the node sweep, the group sweep, the
 * dense output ids and the ut row (HDG_RF_MOVES counts node moves only).
 *
 *   kinds    HDG_RS_MERGE, HDG_RS_SPLIT or both: the sweeps a round runs after its node phase
 *   rounds   repeat: (1) the node phase, as hdg_refine_merge's; (2) with HDG_RS_MERGE one group
 *            sweep; (3) with HDG_RS_SPLIT one split sweep; (4) stop if this round merged nothing
 *            and split nothing, or max_rounds rounds have run, or the total of node sweeps has
 *            reached max_sweeps.  Every move, merge and split raises Q by at least 1
 *   split sweep  visits the slots g = 0, 1, .., nc-1 in that order, each visit seeing the splits
 *            of the earlier visits.  A slot is skipped if it holds fewer than 2 hunks when its
 *            turn comes, or if it received its members by a split of this same sweep (so every
 *            hunk is in at most one attempt per sweep).  Otherwise, with e the smallest empty
 *            slot (one exists whenever a slot holds 2 hunks):
 *            seeds: the pair (s1, s2), s1 < s2, both in g, with the smallest a_pq; among equals
 *              the lowest p, then the lowest q.  If that gain is >= 0 the visit ends and
 *              nothing changes (every cut of g sums non-negative gains)
 *            assignment pass: side G = {s1}, side E = {s2}; the other members of g take their
 *              turns in index order; for member m, T_G = the sum of a_mx over x already on side
 *              G and T_E likewise (members not yet assigned do not count); m joins E iff
 *              T_E > T_G strictly, else G
 *            correction passes: at most HDG_RS_PASSES - 1.  A pass visits the members other than
 *              the two seeds in index order, each seeing the earlier moves; m on side X changes
 *              side iff the sum over the other side is strictly above the sum over X \ {m}.  A
 *              pass without a change ends them
 *            decision: C = the sum of a_xy over x in G, y in E (int64).  If C < 0 the members of
 *              E take slot e, G keeps slot g, Q rises by -C, the split counts and e is marked
 *              as filled by this sweep; otherwise nothing changes
 *   bounds   every side sum is an int32 (at most 2047 partners of magnitude 2^19); |C| <= 2^39
 *            as a merge gain; the seed key holds the gain biased into 21 bits and two 11-bit
 *            indices
 *   rq       rows of HDG_RS_Q_SLOTS i64: slots 0 .. 6 as hdg_refine_merge's, CONVERGED being
 *            1 iff the last node phase ended on a sweep without a move and the last round
 *            merged nothing and split nothing; HDG_RS_Q_SPLITS counts the accepted splits
 * Consequences: (A) with kinds = HDG_RS_MERGE, groups, ut and rq equal hdg_refine_merge's
 * integer for integer (slot 7 is 0 in both); (B) HDG_RM_Q_NODE equals hdg_refine's
 * HDG_RF_Q_END at the same max_sweeps under every kinds; (C) Q_END - Q_NODE >= MERGES + SPLITS;
 * (D) Q_END equals Q recomputed from the returned groups.
 * hdg_refine_split_ladder: rung k holds what hdg_cut(merges, levels, thresholds[k], rule)
 * followed by hdg_refine_split(thresholds[k], .., groups_in = those groups) writes -- or the
 * singleton start without a tree, as hdg_refine_merge_ladder; thresholds is a HOST array.
 * Argument types, array shapes and workspaces are hdg_refine_merge's and
 * hdg_refine_merge_ladder's.  Two launches each: the weights kernel, unchanged, and the sweep
 * block with the chosen sweeps (k_rs_sweep, k_rsl_sweep), one 1024-thread block per commit
 * (per rung and commit).  A split visit compacts the slot's members in index order in LDS,
 * finds the seeds in one walk over the members' rows, and makes one step per member and pass:
 * the member's row read one member ahead, the two side sums by a wave reduction and one int32
 * LDS atomic per wave and side, one barrier, the same decision in every thread; C is carried
 * along.  The visits are bounded by nc, the passes by HDG_RS_PASSES, a pass's steps by the
 * slot's size.  No host synchronisation, no block waits for another, no float atomics, no
 * allocation: graph-capturable, the same bits on every run.  HDG_EINVAL (the message starts
 * "hdg_refine_split:" or "hdg_refine_split_ladder:"; nothing is launched) for everything the
 * merge calls reject, kinds outside {1, 2, 3}, or any flag bit.                            */
#define HDG_RS_MERGE 1         /* kinds bit: a round runs hdg_refine_merge's group sweep   */
#define HDG_RS_SPLIT 2         /* kinds bit: a round runs a split sweep                    */
#define HDG_RS_PASSES 4        /* passes of one split attempt: 1 assignment + 3 correction */
#define HDG_RS_Q_SLOTS 8       /* = HDG_RM_Q_SLOTS; slots 0 .. 6 as HDG_RM_Q_*             */
#define HDG_RS_Q_SPLITS 7      /* splits accepted                                          */

int    hdg_refine_split(const hdg_shape* shape, const hdg_batch* batch, const float* probs,
                        float threshold, int32_t rule, int32_t max_sweeps, int32_t max_rounds,
                        int32_t kinds, int32_t flags,
                        const int32_t* groups_in /* [batch][nc] or NULL */,
                        int32_t* groups          /* [batch][nc] */,
                        uint64_t* ut             /* [batch][HDG_RF_SLOTS] */,
                        int64_t* rq              /* [batch][HDG_RS_Q_SLOTS] */,
                        void* workspace, void* stream);
int    hdg_refine_split_ladder(const hdg_shape* shape, const hdg_batch* batch,
                               const float* probs,
                               const float* thresholds /* HOST, [n_rungs] */, int32_t n_rungs,
                               int32_t rule, int32_t max_sweeps, int32_t max_rounds,
                               int32_t kinds, int32_t flags,
                               const int32_t* merges /* [batch][nc-1][2] or NULL */,
                               const float* levels   /* [batch][nc-1]    or NULL */,
                               int32_t* groups  /* [n_rungs][batch][nc] or NULL */,
                               uint64_t* ut     /* [n_rungs][batch][HDG_RF_SLOTS] */,
                               int64_t* rq      /* [n_rungs][batch][HDG_RS_Q_SLOTS] */,
                               void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * On-device matching (csrc/match.hip): how many hunks ended up in the right group.  Every
 * decoder above is scored by pair counts; hdg_match scores sets of group ids, whatever made
 * them, by the clustering accuracy under the best one-to-one assignment of predicted groups
 * to true groups -- the assignment problem on the contingency table of the two partitions
 * (hdgnn.metrics.match_counts restates the call, integer for integer).  Not a reference flow.
 *
 *   groups   [n_sets][batch][nc] i32, n_sets in [1, HDG_MT_MAX_SETS]: e.g. the rungs a ladder
 *            call left on the device.  Predicted groups by hdg_refine's start rule: hunks
 *            with the same id in [0, nc) are together, a hunk whose id is outside [0, nc) is
 *            alone (no id is used as an index before it is range-checked).  The numbering
 *            does not matter: any renumbering of a set gives the same mt row
 *   true groups  hdg_untangle's: the components of y_pq | y_qp from batch->ybits, dense ids
 *            ordered by smallest member; written to tgroups ([batch][nc]) when it is given
 *   table    n_gt = the hunks in predicted group g and true group t.  Never built densely:
 *            at most nc cells are non-zero.  Every sum below is at most nc <= 2048, all
 *            arithmetic is integer, no result depends on an order of summation
 *   mt       [n_sets][batch][HDG_MT_SLOTS] u64, every slot written by the call
 *   HDG_MT_MATCHED  the optimum of the assignment problem on the table: the smaller side is
 *            fully assigned, an empty cell counts 0.  The value is unique even where the
 *            assignment is not.  accuracy = MATCHED / nc
 *   mate     (optional) [n_sets][batch][nc] i32: per hunk the dense true-group id its predicted
 *            group is assigned to, -1 if the group is unassigned or assigned through an
 *            empty cell.  ONE optimal assignment: under ties it is not unique and not
 *            canonical (the same bits on every run, but another implementation may return
 *            another optimum).  What holds: it is constant on each predicted group,
 *            injective over the groups where it is not -1, and
 *            #{p : mate[p] == tgroups[p]} == MATCHED
 *   workspace  hdg_match_workspace_bytes(shape, n_sets) bytes, 8-byte aligned: the true ids,
 *            computed once for all sets; its content before the call does not matter
 * Consequences: (A) max cell <= MATCHED <= min(PURITY, COVER) <= nc; (B) MATCHED == nc iff the
 * two partitions are equal (SD = DS = 0 in hdg_untangle's row of the same groups), and then
 * CELLS == ISOLATED == GROUPS == TGROUPS; (C) MATCHED >= the sum of the isolated cells.
 * Two launches on `stream`.  k_mt_truth: one 1024-thread block per commit labels the true
 * groups (ut_true_groups).  k_mt_match: grid (n_sets, batch), one 256-thread block per set and
 * commit, all state in LDS: a predicted group is named by its smallest member; one walk over
 * the nc hunks gives every hunk the size of its cell and whether it is the cell's first hunk;
 * integer LDS atomics give row and column maxima and degrees; the isolated cells are taken
 * as they are; on the residual graph (the other cells) the assignment is solved exactly by
 * shortest augmenting paths with integer potentials, rows on the smaller residual side K',
 * ties between equal slacks to the lowest column.
 *   bounds   a component of the residual graph with c >= 2 cells has at most c + 1 rows and
 *            columns together, so both sides together have at most 3 nc / 2 groups and
 *            K' <= 3 nc / 4 (reached by components of two cells, rows and columns doubled in
 *            turn); augmentations <= K'; a path takes at most K' + 1 columns, two barriers
 *            each (the loops are capped at nc rows and nc + 1 steps); every scan of a step is
 *            ceil(nc / 256) columns per thread; the cell walk is nc steps.  A potential is the
 *            length of a shortest path of at most K' cells of weight <= nc: |potential| <=
 *            nc K' < 2^22, far below the 2^30 that marks a column no path has reached
 * No host synchronisation, no block waits for another, no float anywhere, no allocation:
 * graph-capturable, the same bits on every run.  Only shape->batch, shape->nc and
 * batch->ybits are read.  HDG_EINVAL (the message starts "hdg_match:"; nothing is launched)
 * for batch outside [1, 65535], nc outside [2, 2048], n_sets outside [1, HDG_MT_MAX_SETS], a
 * NULL groups, mt, batch, batch->ybits or workspace, or a workspace that is not 8-byte
 * aligned.                                                                              */
#define HDG_MT_SLOTS 8
#define HDG_MT_GROUPS 0    /* predicted groups                                           */
#define HDG_MT_TGROUPS 1   /* true groups                                                */
#define HDG_MT_MATCHED 2   /* max over one-to-one assignments of predicted to true groups
                              of the sum of n_gt over the assigned pairs: the hunks in the
                              right group.  accuracy = MATCHED / nc                      */
#define HDG_MT_PURITY 3    /* sum over predicted groups g of max_t n_gt                  */
#define HDG_MT_COVER 4     /* sum over true groups t of max_g n_gt                       */
#define HDG_MT_CELLS 5     /* cells with n_gt > 0                                        */
#define HDG_MT_ISOLATED 6  /* cells that are the only non-zero cell of their row AND of
                              their column (every optimum contains them); slot 7 is 0
                              (non-zero only if a path of the solver found no column,
                              which the bounds exclude: such a row's MATCHED is void)   */
#define HDG_MT_MAX_SETS 64 /* = HDG_RL_MAX_RUNGS                                         */

size_t hdg_match_workspace_bytes(const hdg_shape* shape, int32_t n_sets);  /* 0 on an error */
int    hdg_match(const hdg_shape* shape, const hdg_batch* batch,
                 const int32_t* groups  /* [n_sets][batch][nc] */, int32_t n_sets,
                 int32_t* mate          /* [n_sets][batch][nc] or NULL */,
                 int32_t* tgroups       /* [batch][nc] or NULL */,
                 uint64_t* mt           /* [n_sets][batch][HDG_MT_SLOTS] */,
                 void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * Data parallelism over xGMI (one all-reduce of the flat gradient per step).
 *
 * Instead of an RCCL call between hdg_fwd_bwd and hdg_adam_tf, the step's reduction
 * kernel exchanges the gradient itself: every rank owns a MAILBOX (uncached device
 * memory, hdg_dp_mailbox_alloc) that every other rank of the node maps through HIP IPC
 * (hdg_dp_mailbox_open on the 64-byte handle, exchanged by the caller, e.g. with
 * torch.distributed.all_gather).  Each block of the tail kernel writes its gradient
 * slots as tagged words straight into every peer's mailbox over xGMI (one hop), polls
 * its own mailbox for the peers' words, sums the world's values in rank order (the same
 * bits on every rank: replicas stay bitwise equal) and applies TF Adam -- one kernel, no
 * collective launch.  A peer that does not arrive within wait_ticks fails the launch
 * loudly, but only where the wait happened: each tail block waits for the peers' words of
 * ITS OWN slots, and a block that times out sets HDG_STATUS_DP_TIMEOUT in this rank's
 * status word, writes a NaN loss and skips the update of its slots.  The other blocks of
 * the same rank (block 0's beta-power update included) and every peer that did receive
 * the words still apply the step, so after a timeout the parameters are partly updated
 * and the ranks disagree: DP_TIMEOUT is unrecoverable -- no retry; restore every rank
 * from a checkpoint.  (The split-mode pair timeout, HDG_STATUS_XCH_TIMEOUT, is different:
 * its step is skipped whole and a one-block retry is exact.)  The deadline counts from
 * the moment each block starts waiting, so host-side skew between ranks (data loading,
 * rank-0 file writes) counts against it: callers barrier the ranks before the first step
 * and after rank-only host work (graph2graph.train does).  All ranks must issue the same
 * sequence of hdg_*_dp calls (per-block launch counters in the mailbox tag the words).
 * The mailbox calls are the one place the library allocates device memory (IPC needs an
 * allocation of its own); everything else stays caller-owned.
 * --------------------------------------------------------------------------------- */
#define HDG_DP_MAX_WORLD 16
#define HDG_DP_HANDLE_BYTES 64
#define HDG_DP_MAX_LEN 3152          /* longest vector hdg_dp_allreduce accepts          */
#define HDG_STATUS_DP_TIMEOUT 2u     /* a peer's gradient words never arrived            */

typedef struct hdg_dp {
    int32_t  rank;        /* this process's rank, 0 <= rank < world                      */
    int32_t  world;       /* ranks on this node, 1 <= world <= HDG_DP_MAX_WORLD          */
    uint64_t wait_ticks;  /* 100 MHz ticks a block waits for a peer (0: 10 s)            */
    void*    mailbox[HDG_DP_MAX_WORLD];  /* rank r's mailbox as mapped in this process   */
    int32_t  flags;       /* HDG_DP_* bits (ABI 9), 0 for one rank per device            */
    int32_t  reserved;    /* 0                                                            */
} hdg_dp;
/* HDG_DP_SHARED: several ranks share one device (a rehearsal of the node's DP step on a
 * box with fewer GPUs).  A waiting tail block spins on a CU; with one rank per device
 * nothing else needs that CU, but a peer rank on the SAME device still has to place its
 * step kernel, whose 1024-thread blocks each take a whole CU (all VGPRs, up to all of the
 * LDS).  The tails of W-1 waiting ranks must therefore never cover every CU: with this
 * flag every exchange runs as G light blocks per rank that loop over the slot groups (all
 * of a block's words sent first, then its groups received in order), G chosen so that the
 * W-1 waiting ranks hold at most half of the device's CUs (G >= HDG_DP_SHARED_BLOCKS:
 * (HDG_DP_MAX_WORLD - 1) * 8 = 120 <= 128), and the fused path reduces its partial rows
 * with the non-spinning k_grad_reduce before the exchange (hdg_fwd_bwd -> hdg_adam_dp)
 * instead of inside the spinning tail.  Same bits as the one-rank-per-device calls.    */
#define HDG_DP_SHARED 1
#define HDG_DP_SHARED_BLOCKS 8

size_t hdg_dp_mailbox_bytes(void);
/* Host utility: CRC-32C (Castagnoli) of n bytes, continuing from crc (0 to start) -- the
 * record checksum of the TF V2 checkpoint bundles graph2graph.saver writes.          */
uint32_t hdg_crc32c(const void* data, size_t n, uint32_t crc);
/* Host utility: write one TF V2 checkpoint bundle of float32 tensors from a prebuilt
 * template (hdgnn.tfckpt.BundleTemplate; replaces the Python encoder of saver.save,
 * model_2.py:427-437, so the caller's thread runs it without holding the GIL):
 *   data file  = state[gather[i]] for i < n_floats (the tensors' bytes, sorted by name;
 *                every gather index is checked against the n_state floats of state)
 *   index file = index_img with each entry's masked CRC-32C of its bytes written at
 *                entries[3e + 2] (the tensor spans [entries[3e], +entries[3e + 1]) bytes of
 *                the data file), then each block's trailer CRC (blocks[2b] offset,
 *                blocks[2b + 1] length; type byte at offset + length) -- index_img is
 *                modified in place.  Both files are written under "<path>.tmp" and renamed
 *                into place, data before index.  0, or HDG_EINVAL (hdg_last_error).    */
int hdg_bundle_write(const char* data_path, const char* index_path, const float* state,
                     int64_t n_state, const int32_t* gather, int64_t n_floats,
                     uint8_t* index_img, int64_t index_len, const int64_t* entries,
                     int32_t n_entries, const int64_t* blocks, int32_t n_blocks);
/* Host utility: background checkpoint writer (saver.save off the training thread).  One
 * native thread runs the submitted jobs in order; a job writes a bundle of `state` exactly
 * as hdg_bundle_write does with the writer's template (gather / index image / entries /
 * blocks, copied at create), then removes the '\n'-separated `removes` paths (bundles that
 * fell out of max_to_keep; missing files are fine), then writes `text` to `text_path`
 * (appended when text_append != 0, else replacing it: the 'checkpoint' state file, a
 * result line).  NULL state / removes / text_path skip that part.  submit copies
 * everything it is given (n_state floats of state) and returns at once; flush waits for
 * the queue and returns the first failure since the last flush (HDG_EINVAL, message in
 * hdg_last_error); destroy flushes, stops the thread and frees the writer.              */
int hdg_ckpt_writer_create(const int32_t* gather, int64_t n_floats, int64_t n_state,
                           const uint8_t* index_img, int64_t index_len, const int64_t* entries,
                           int32_t n_entries, const int64_t* blocks, int32_t n_blocks,
                           void** writer);
int hdg_ckpt_writer_submit(void* writer, const float* state, const char* data_path,
                           const char* index_path, const char* removes, const char* text_path,
                           const char* text, int32_t text_append);
int hdg_ckpt_writer_flush(void* writer);
/* the first failure since the last flush / poll without waiting for the queue (ABI 9): 0 or
 * the failed job's code (message in hdg_last_error), reported once.  A job whose bundle
 * write fails skips its removals and text, so the caller re-books its keep-list.        */
int hdg_ckpt_writer_poll(void* writer);
int hdg_ckpt_writer_destroy(void* writer);
/* Host utility: hipMemcpyAsync (kind default) and completion events without timing, for
 * the training loop's stream-ordered reads into pinned host memory.                     */
int hdg_memcpy_async(void* dst, const void* src, size_t bytes, void* stream);
int hdg_event_create(void** event);
int hdg_event_record(void* event, void* stream);
int hdg_event_synchronize(void* event);
int hdg_event_destroy(void* event);
/* allocate + zero this rank's mailbox on the current device; handle: 64 bytes out */
int hdg_dp_mailbox_alloc(void** mailbox, void* handle);
/* map a peer's mailbox (its handle) into this process; close / free undo the calls */
int hdg_dp_mailbox_open(const void* handle, void** mailbox);
int hdg_dp_mailbox_close(void* mailbox);
int hdg_dp_mailbox_free(void* mailbox);

/* One data-parallel training step: hdg_fwd_bwd -> xGMI all-reduce -> TF Adam with the
 * exchange inside the reduction kernel.  grad receives the world-summed gradient +
 * trailer (as hdg_fwd_bwd + all_reduce would leave it); out->stats the world's loss.   */
int hdg_train_step_dp(const hdg_shape* shape, const hdg_batch* batch, hdg_state* state,
                      float lr, hdg_outputs* out, float* grad, void* workspace,
                      const hdg_dp* dp, void* stream);
/* xGMI all-reduce of a local gradient (hdg_fwd_bwd's buffer) fused with TF Adam:
 * grad_out = sum over ranks of grad_local (must not overlap), then hdg_adam_tf's update. */
int hdg_adam_dp(const hdg_shape* shape, hdg_state* state, const float* grad_local,
                float* grad_out, float lr, float* stats, uint32_t* status, const hdg_dp* dp,
                void* stream);
/* out[i] = sum over ranks (rank order) of in[i], n <= HDG_DP_MAX_LEN, in / out disjoint. */
int hdg_dp_allreduce(const hdg_dp* dp, const float* in, float* out, int32_t n,
                     uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDGNN_H */
