/*
 * pocketflow_hip.h -- C ABI of the MI355X (gfx950) kernel library for the PocketFlow
 * compression-training hot path.
 *
 * The reference (Tencent/PocketFlow) has NO native boundary: every "kernel" is a chain of stock
 * TensorFlow ops stitched into the graph from Python.  This header is therefore the boundary a
 * maintainer would bind (ctypes / cffi / pybind) in place of those op chains; each entry point
 * cites the reference op chain (file:line under /root/reference) it replaces.  See INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / TF types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - functions never allocate, never synchronise, never own memory; they enqueue kernels and
 *     return 0 (hipSuccess) or a hipError_t value.  pf_error_string() names it.
 *   - dtype codes: PF_F32 = 0, PF_BF16 = 1 (storage type; arithmetic is always float32).
 *   - activation codes: PF_ACT_NONE = 0, PF_ACT_RELU = 1, PF_ACT_RELU6 = 2.
 *   - weight layout: KRSC = [cout][kh][kw][cin] (dense: [out][in]); the reference's HWIO flat
 *     index (needed by 'split' buckets) is recovered by index arithmetic, never by a transpose.
 *   - activation layout: NHWC, i.e. a [rows = N*H*W][C] row-major matrix.
 *   - min/max slots are pairs of uint32 holding an order-preserving encoding of a float
 *     ({enc(min), ~enc(max)}), initialised to 0xFFFFFFFF (one memset) so that both are updated with
 *     atomicMin and the result is independent of the order of arrival (bit-deterministic).
 */
#ifndef POCKETFLOW_HIP_H_
#define POCKETFLOW_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PF_F32 = 0, PF_BF16 = 1 };
enum { PF_ACT_NONE = 0, PF_ACT_RELU = 1, PF_ACT_RELU6 = 2 };
enum { PF_BUCKET_TENSOR = 0, PF_BUCKET_CHANNEL = 1, PF_BUCKET_SPLIT = 2 };

/* One weight tensor inside the flat parameter buffer (64 bytes, mirrored by ctypes/numpy). */
typedef struct PfSeg {
  int64_t offset;       /* first element in the flat buffers                                  */
  int64_t len;          /* RS*I*O                                                             */
  int32_t RS;           /* kh*kw of the reference HWIO = [kh][kw][I][O] kernel (dense: 1)     */
  int32_t layout;       /* storage: 0 = KRSC [O][kh][kw][I] (dense [O][I]); 1 = CRS depthwise */
  int32_t I, O;         /* reference cin / cout (depthwise: I = C, O = channel multiplier 1)  */
  int32_t mode;         /* PF_BUCKET_*                                                        */
  int32_t bits;         /* quantisation bits of this tensor (fed per step in the reference)   */
  int32_t bucket_size;  /* 'split' buckets only                                               */
  int32_t n_bucket;     /* number of (alpha,beta) pairs: 1 | O | ceil(len/bucket_size)        */
  int64_t slot_offset;  /* first min/max slot (pair index) of this tensor                     */
  int64_t cb_offset;    /* NUQ: first codebook float; layout [k][n_bucket]                    */
} PfSeg;

/* block -> (segment, chunk) map entry; built once per model on the host.  For the apply kernels in
 * channel mode, row0 / nrows are the first output channel and the number of output channels the
 * chunk touches (their alpha/beta are staged in LDS); 0 / 1 otherwise.                        */
typedef struct PfBlock { int32_t seg; int32_t chunk; int32_t row0; int32_t nrows; } PfBlock;

#define PF_CHUNK 4096   /* elements per block in the segment kernels (256 threads x 16) */

const char* pf_error_string(int err);
int pf_version(void);
/* The launchers' PF_* tuning / A-B environment switches are read once, on first use (csrc/pf_api.hip, struct PfTuning); a tool or
 * test that changes one in-process calls this to have them read again.  No reference counterpart (tuning service). */
int pf_tuning_reload(void);

/* ---- K1: min/max calibration -------------------------------------------------------------
 * replaces tf.reduce_max / tf.reduce_min (+stop_gradient) of __scale,
 * learners/uniform_quantization/utils.py:224-225 == learners/nonuniform_quantization/utils.py:411-412 */
int pf_minmax_slots_init(uint32_t* slots, int64_t n_pairs, void* stream);
/* whole-tensor min/max of act(x); one pass, wave-shuffle + LDS block reduce, 2 atomics / block */
int pf_minmax_tensor(const void* x, int64_t n, int dtype, int act, uint32_t* slot, void* stream);
/* decode slots -> alpha = max - min + 1e-10, beta = min (float pairs), for logging / tests */
int pf_minmax_decode(const uint32_t* slots, int64_t n_pairs, float* alpha_beta, void* stream);

/* ---- K2/K4: uniform fake-quant, forward ----------------------------------------------------
 * replaces (x-beta)/alpha -> *k -> round -> /k -> alpha*.+beta of __uniform_quantize,
 * learners/uniform_quantization/utils.py:163-199, 228-245, and the activation variant
 * insert_quant_op_for_activations :51-79 (act(x) recomputed, per-tensor min/max).            */
int pf_uq_apply(const void* x, void* y, int64_t n, int in_dtype, int out_dtype, int act,
                const uint32_t* slot, int bits, void* stream);
/* backward of act -> fake-quant: STE through round, then ReluGrad / Relu6Grad: dx = g * mask(u) */
int pf_act_grad(const void* g, const void* u, void* dx, int64_t n, int dtype, int act,
                void* stream);

/* ---- K1+K2+K3 over ALL weight tensors of a model in two launches ---------------------------
 * replaces insert_quant_op_for_weights (uq utils.py:81-113) incl. __split_bucket / __channel_bucket
 * (:247-289).  w_flat is the fp32 master buffer, qw_flat the fake-quantised copy the convolutions
 * read (fp32 or bf16).                                                                        */
int pf_seg_minmax(const float* w_flat, const PfSeg* segs, const PfBlock* blocks, int n_blocks,
                  uint32_t* slots, void* stream);
int pf_seg_uq_apply(const float* w_flat, void* qw_flat, int out_dtype, const PfSeg* segs,
                    const PfBlock* blocks, int n_blocks, const uint32_t* slots, void* stream);

/* ---- K5: non-uniform (codebook) fake-quant -------------------------------------------------
 * replaces tile/abs/argmin/gather of __build_norm_quant_point / __build_bucket_norm_quant_point,
 * learners/nonuniform_quantization/utils.py:284-347.  idx (uint8, k <= 256) is kept for backward. */
int pf_seg_nuq_apply(const float* w_flat, void* qw_flat, int out_dtype, uint8_t* idx_flat,
                     const float* codebooks, const PfSeg* segs, const PfBlock* blocks,
                     int n_blocks, const uint32_t* slots, void* stream);
/* dL/dc[j][b] = sum_{i in bucket b, idx_i = j} alpha_b * g_i   (gather-grad scatter-add under the
 * override map {'Mul':'Add','Sign':'Identity'}, nuq utils.py:305-306, 345-346).  The sums are ADDED to dcodebooks
 * [n_codebook] (zeroed by the caller).  Bit-deterministic: terms are accumulated as 2^-36 fixed-point integers with
 * 64-bit integer atomics in acc_ws [n_codebook] (scratch; zeroed here), then converted once.                   */
int pf_seg_nuq_codebook_grad(const void* g_flat, int g_dtype, const uint8_t* idx_flat,
                             float* dcodebooks, int64_t* acc_ws, int64_t n_codebook, const PfSeg* segs,
                             const PfBlock* blocks, int n_blocks, const uint32_t* slots, void* stream);
/* normalised weights x_hat = (w - beta) / alpha of ONE tensor (for the quantile initialiser,
 * nuq utils.py:349-366, which then sorts them).                                               */
int pf_seg_normalize(const float* w_flat, float* xn_out, const PfSeg* segs, int seg_index,
                     const uint32_t* slots, void* stream);

/* ---- K7/K9: weight sparsification ----------------------------------------------------------
 * replaces the prune_op chain of WeightSparseLearner.__build_masks,
 * learners/weight_sparsification/learner.py:283-288.                                          */
int pf_ws_bkup_merge_abs(const float* var, float* bkup, const float* mask, float* abs_out,
                         int64_t n, void* stream);
/* k-th largest of a non-negative float array by 4-pass radix select on the bit pattern
 * (tf.contrib.distributions.percentile = descending sort + index).  workspace: 1024 uint32.   */
int pf_kth_largest_nonneg(const float* a, int64_t n, int64_t k_desc_index, float* out,
                          uint32_t* workspace, void* stream);
int pf_ws_mask_apply(float* var, const float* bkup, float* mask, const float* thr, int64_t n,
                     void* stream);
/* count_nonzero (ws learner.py:51-65) */
int pf_count_nonzero(const float* x, int64_t n, unsigned long long* out, void* stream);

/* ---- K8 (channel pruning): per-channel binary gradient masks -------------------------------
 * replaces mask = ones; mask[:,:,~keep_in,:]=0; mask[:,:,:,~keep_out]=0 ; g*mask of
 * ChannelPrunedLearner.__calc_grads_pruned, learners/channel_pruning/learner.py:406-419.
 * KRSC storage; keep_in[I], keep_out[O] are staged in LDS.                                     */
int pf_cp_build_mask(float* mask, const uint8_t* keep_in, const uint8_t* keep_out, int O, int RS,
                     int I, void* stream);
int pf_cp_mask_grad(float* g, const uint8_t* keep_in, const uint8_t* keep_out, int O, int RS,
                    int I, void* stream);

/* ---- K8+K14: fused (L2-coupled, masked) optimiser steps over a flat buffer ------------------
 * replaces tf.train.AdamOptimizer / MomentumOptimizer + `grad * mask` + the L2 term of calc_loss:
 *   uq learner.py:244-253, ws learner.py:201-212,314-332, cp learner.py:357-368,
 *   nets/resnet_at_ilsvrc12.py:132-135 (loss_w_dcy * sum l2_loss).
 * g_eff = (g * g_scale + wd * p) * mask for the first n_decay elements, (g * g_scale) * mask after;
 * mask may be NULL.  g may be fp32 or bf16.  g_scale = 1/world_size folds the all-reduce average. */
int pf_adam_flat(float* p, const void* g, int g_dtype, float* m, float* v, const float* mask,
                 int64_t n, int64_t n_decay, float wd, float g_scale, float lr, float beta1,
                 float beta2, float eps, float beta1_power, float beta2_power, void* stream);
int pf_momentum_flat(float* p, const void* g, int g_dtype, float* acc, const float* mask,
                     int64_t n, int64_t n_decay, float wd, float g_scale, float lr, float momentum,
                     void* stream);
/* The same two updates for a step that was captured in a hipGraph (pocketflow_amd/step_graph.py; the reference's counterpart is
 * the ONE `sess.run(train_op)` of uq learner.py:172 -- a TF session also replays a compiled graph whose learning rate is a tensor,
 * every learner's `setup_lrn_rate`): the per-step scalars are read from device memory, hp[0] = Adam's
 * alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) (float32, computed by the host exactly as pf_adam_flat does), hp[1] = lr.
 * pf_set_floats writes dst[0..3] from by-value kernel arguments (no staging buffer the host could overrun). */
int pf_adam_flat_dev(float* p, const void* g, int g_dtype, float* m, float* v, const float* mask,
                     int64_t n, int64_t n_decay, float wd, float g_scale, const float* hp, float beta1,
                     float beta2, float eps, void* stream);
int pf_momentum_flat_dev(float* p, const void* g, int g_dtype, float* acc, const float* mask,
                         int64_t n, int64_t n_decay, float wd, float g_scale, const float* hp,
                         float momentum, void* stream);
int pf_set_floats(float* dst, float a, float b, float c, float d, void* stream);

/* ---- K10+K11: distillation + hard-label losses, forward and backward in one kernel ---------
 * replaces tf.losses.softmax_cross_entropy(labels, logits) (nets/<model>.py calc_loss) and
 * DistillationHelper.calc_loss (learners/distillation_helper.py:86-103).
 *   L_model = mean_n CE(labels_n, z_s_n) ; L_dst = loss_w * mean_n CE(softmax(z_t/T), z_s/T)
 *   dz_s = (softmax(z_s)*sum(labels) - labels)/B + loss_w/(B*T) * (softmax(z_s/T) - softmax(z_t/T))
 * labels: float one-hot / soft [B][C].  z_t may be NULL (no distillation).  losses[0] = L_model,
 * losses[1] = L_dst.  row_ws: B*2 floats of scratch.  One workgroup per row, wave-shuffle
 * reductions, fixed summation order (bit-deterministic).                                      */
int pf_ce_distill_fwd_bwd(const void* z_s, int zs_dtype, const float* labels, const void* z_t,
                          int zt_dtype, int B, int C, float tempr, float loss_w, float* losses,
                          void* dz_s, int dz_dtype, float* row_ws, void* stream);

/* The training step's ONE loss launch (the network head): both losses, the top-1 / top-5 accuracy and the two terms of dz_s.
 *   losses[0] = L_model, losses[1] = L_dst (0 without z_t), losses[2] / losses[3] = the fraction of rows whose label is in the
 *   top 1 / top 5 (tf.nn.in_top_k: fewer than k logits STRICTLY greater than the logit at the FIRST arg-max of the label row).
 *   dz_hard = T((softmax(z_s)*sum(labels) - labels)/B), dz_soft = T(loss_w/(B*T) * (softmax(z_s/T) - softmax(z_t/T))), each
 *   rounded to the dz type: bit for bit the dz_s of one pf_ce_distill_fwd_bwd call without z_t and of one with z_t and all-zero
 *   labels.  z_t, dz_soft may be NULL (no distillation).  row_ws: B*3 floats of scratch.                                   */
int pf_ce_distill_head(const void* z_s, int zs_dtype, const float* labels, const void* z_t,
                       int zt_dtype, int B, int C, float tempr, float loss_w, float* losses /*[4]*/,
                       void* dz_hard, void* dz_soft, int dz_dtype, float* row_ws, void* stream);
/* Its backward: dz = T( T(dz_hard * T(g0)) + T(dz_soft * T(g1)) ), g0 / g1 the upstream gradients of L_model / L_dst (float32
 * DEVICE scalars) -- what autograd makes of the two calls above.  g0 or (dz_soft, g1) may be NULL: that term is dropped.      */
int pf_ce_combine(const void* dz_hard, const void* dz_soft, const float* g0, const float* g1, void* dz,
                  int dtype, int64_t n, void* stream);

/* ---- K13 fused with K4: batch-norm (training) + ReLU + activation fake-quant ----------------
 * replaces tf.layers.batch_normalization(fused=True) -> tf.nn.relu -> (min/max, quantise) of
 * utils/external/resnet_model.py:55-62 + uq utils.py:51-79 for the BN->ReLU->conv chains of
 * ResNet-v2 / MobileNet-v1.  x is [rows][C] (NHWC).
 * pass 1 (pf_bn_stats): per-channel sum, sum of squares, min, max of x in ONE read.
 * finalize: mean/var -> scale/shift, moving averages (unbiased variance), and -- because
 *   y = act(scale*x+shift) is monotone in x per channel -- the exact whole-tensor min/max of y
 *   from the per-channel min/max of x, written into the activation's min/max slot.
 * pass 2 (pf_bn_act_quant_apply): read x, write q = fake_quant(act(scale*x+shift)).
 * pf_bn_vector_ok(C): 1 where the passes of this section, pf_bn_act_quant_codes and pf_bn_act_quant_static
 *   take their 16-byte route on 16-byte aligned tensors (a lane owns 8 consecutive channels of a row):
 *   C % 8 == 0 and 8 <= C <= 2048.  Any other C, or a misaligned tensor, runs their scalar loops:
 *   the same bits out of the element-wise passes, another summation order in the two reductions.
 *   (pf_bn_act_quant_pool takes its vector form only where C / 8 is a power of two as well.)     */
int pf_bn_vector_ok(int C);
int pf_bn_stats(const void* x, int dtype, int64_t rows, int C, float* partial /*[nblk][4][C]*/,
                int n_blocks, void* stream);
int pf_bn_finalize(const float* partial, int n_blocks, int64_t rows, int C, const void* x_row0,
                   int dtype, const float* gamma, const float* beta, float* moving_mean,
                   float* moving_var, float momentum, float eps, int training /*0: use moving stats*/,
                   int act, float* scale_shift /*[2][C]*/, float* mean_invstd /*[2][C]*/,
                   uint32_t* slot /*may be NULL*/, void* stream);
int pf_bn_act_quant_apply(const void* x, void* q, int dtype, int64_t rows, int C,
                          const float* scale_shift, int act, const uint32_t* slot, int bits,
                          int quantize, void* stream);
/* pass 2 of a BN whose output feeds nothing but the spatial mean (the network head; rows = B*HW, image-major):
 *   pooled[b][c] = T( (sum_p q[b][p][c]) * float32(1/HW) ), q = the value pf_bn_act_quant_apply would have stored (rounded to T),
 *   summed in float32 in ascending pixel order and scaled as aten's mean scales its sum; q itself is never written.
 *   pooled: [B][C] of x's type.                                                                                           */
int pf_bn_act_quant_pool(const void* x, void* pooled, int dtype, int64_t rows, int C,
                         const float* scale_shift, int act, const uint32_t* slot, int bits,
                         int quantize, int HW, void* stream);
/* ... and its backward passes: pf_bn_bwd_stats / pf_bn_bwd_apply with dq[(b,p)][c] = T(float(g[b][c]) * float32(1/HW)) rebuilt
 * from the [B][C] gradient g of the pooled tensor instead of read (the value autograd's mean / cast chain expands on the device:
 * aten divides by a host scalar as a product with its rounded reciprocal); same row order, splits and partial layout, so partial,
 * dgamma, dbeta and dx are bit-identical.  rows < 2^31, rows % HW == 0.                                                      */
int pf_bn_bwd_stats_pooled(const void* g, const void* x, int dtype, int64_t rows, int C, int HW,
                           const float* scale_shift, const float* mean_invstd, int act,
                           float* partial /*[nblk][2][C]*/, int n_blocks, void* stream);
int pf_bn_bwd_apply_pooled(const void* g, const void* x, void* dx, int dtype, int64_t rows, int C, int HW,
                           const float* scale_shift, const float* mean_invstd,
                           const float* dgamma, const float* dbeta, int act, void* stream);
/* backward: dy = dq * actmask(scale*x+shift) (STE); per-channel sum(dy), sum(dy*xhat) */
int pf_bn_bwd_stats(const void* dq, const void* x, int dtype, int64_t rows, int C,
                    const float* scale_shift, const float* mean_invstd, int act,
                    float* partial /*[nblk][2][C]*/, int n_blocks, void* stream);
int pf_bn_bwd_finalize(const float* partial, int n_blocks, int C, float* dgamma, float* dbeta,
                       void* stream);
int pf_bn_bwd_apply(const void* dq, const void* x, void* dx, int dtype, int64_t rows, int C,
                    const float* scale_shift, const float* mean_invstd,
                    const float* dgamma, const float* dbeta, int act, void* stream);
/* inference-mode BN + act (teacher forward, eval graphs): y = act(scale*x+shift) */
/* pf_bn_bwd_apply + the gradient that reaches the same tensor through an identity shortcut:
 * dx = bn_backward(dq, x) + addend  (replaces the AddN of the two gradient paths TF inserts for a tensor
 * with two consumers, utils/external/resnet_model.py:257-314 `inputs + shortcut`).  addend may be NULL. */
int pf_bn_bwd_apply_add(const void* dq, const void* x, const void* addend, void* dx, int dtype,
                        int64_t rows, int C, const float* scale_shift, const float* mean_invstd,
                        const float* dgamma, const float* dbeta, int act, void* stream);
int pf_bn_eval_scale_shift(const float* gamma, const float* beta, const float* moving_mean,
                           const float* moving_var, float eps, int C, float* scale_shift,
                           void* stream);

/* ---- the residual join of a ResNet-v1 block: BN (no activation of its own) + shortcut + ReLU (pf_bn_join.hip) ----------
 * utils/external/resnet_model.py:250-252  inputs = batch_norm(inputs); inputs += shortcut; inputs = tf.nn.relu(inputs).
 * x, r, u, dq, g: [rows][C] of `dtype` (PF_F32 / PF_BF16), C % 8 == 0, every pointer 16-byte aligned; scale_shift / mean_invstd the
 * [2][C] float32 tables of pf_bn_finalize / pf_bn_eval_scale_shift; act = PF_ACT_NONE or PF_ACT_RELU.
 * pf_bn_add_act_fwd: u = act(fmaf(scale[c], x, shift[c]) + r), one rounding on the store: float32 storage runs these float32
 *   operations as written (bit for bit pf_bn_act_quant_apply without activation, a float32 add and a ReLU); bf16 storage evaluates
 *   them in float64 and stores the exact value rounded once (two float32 roundings in front of the bf16 one would move several
 *   times as many elements by a bf16 ulp as the single fmaf of pf_bn_act_quant_apply does).  slot != NULL: the min / max of
 *   u AS STORED (after the rounding to `dtype`) are folded into the slot, in the encoding of pf_minmax_tensor (pf_minmax_decode /
 *   pf_uq_apply read it unchanged).
 * pf_bn_add_act_bwd_gate: g = dq * [fmaf(scale, x, shift) + r > 0] (act none: g = dq), the gate recomputed from x and r, and
 *   partial[G][2][C] = {sum g, sum g * xhat} per row split, G = pf_bn_add_act_groups(rows, C), in the layout pf_bn_bwd_finalize
 *   reads (fixed summation order: deterministic).  pf_bn_bwd_finalize and pf_bn_bwd_apply(act = none) on g then give the BN's dx /
 *   dgamma / dbeta; g is the shortcut's gradient.
 * pf_bn_add_act_bwd_gate_add: the same with dq + addend in the place of dq -- the gradients of the TWO consumers of a block's output
 *   (the next block's first convolution and its shortcut), summed in float32 and rounded to `dtype` as autograd's accumulation would
 *   store the sum.  addend may be NULL.
 * pf_bn_add_act_groups: the number of row splits of both launches (0 for a shape they refuse).  A workgroup covers
 *   256 / min(C / 8, 8) rows per trip and every split makes one trip until the cap min(256, 2048 / ceil(C / 64)) is reached; more rows
 *   run in a grid-stride loop.
 * Both launches return hipErrorInvalidValue WITHOUT launching for a null or misaligned pointer, C % 8 != 0, rows <= 0, an unknown
 * dtype or an activation other than none / ReLU. */
int pf_bn_add_act_groups(int64_t rows, int C);
int pf_bn_add_act_fwd(const void* x, const void* r, void* u, int dtype, int64_t rows, int C, const float* scale_shift, int act,
                      uint32_t* slot, void* stream);
int pf_bn_add_act_bwd_gate(const void* dq, const void* x, const void* r, void* g, int dtype, int64_t rows, int C,
                           const float* scale_shift, const float* mean_invstd, int act, float* partial, void* stream);
int pf_bn_add_act_bwd_gate_add(const void* dq, const void* addend, const void* x, const void* r, void* g, int dtype, int64_t rows,
                               int C, const float* scale_shift, const float* mean_invstd, int act, float* partial, void* stream);

/* ---- K12 fused with K13/K4: 1x1 convolutions with BN/ReLU/fake-quant prologue and residual-add /
 * BN-statistics epilogue (bf16 NHWC, fp32 accumulate) -------------------------------------------
 * replaces, per bottleneck block, the chain  tf.layers.batch_normalization -> tf.nn.relu ->
 * __uniform_quantize(activation) -> tf.nn.conv2d(1x1) [-> + shortcut] of
 * utils/external/resnet_model.py:257-314 + learners/uniform_quantization/utils.py:51-79,92-103 and the
 * Conv2DBackpropInput / Conv2DBackpropFilter gradients of that convolution.
 *
 * pf_conv1x1_fwd:  Y[m][n] = sum_k Q(X)[row(m)][k] * W[n][k]  (+ R[m][n])
 *   X [rows_in][K], W [N][K], Y / R [M][N], all bf16.  Prologue (scale_shift != NULL):
 *   Q(x) = fake_quant(act(scale[k]*x + shift[k])) with scale_shift = {scale[K], shift[K]} as written by
 *   pf_bn_finalize / pf_bn_eval_scale_shift and the activation range in `slot` (NULL: no fake-quant).
 *   Epilogue: R != NULL adds the residual; partial != NULL receives per-channel {sum, sumsq, min, max} of
 *   the stored Y values as [G][4][N] floats, G = pf_conv1x1_stats_groups_k(M, N, K, scale_shift != NULL), in the layout
 *   pf_bn_finalize consumes (pivot 0).  stride > 1: output pixel (img, ho, wo) of an [.., Ho, Wo] grid
 *   reads input pixel (img, ho*stride, wo*stride) of an [.., H, Wd] grid; ymap != 0 maps the OUTPUT rows
 *   instead (backward-data of a strided conv: X = dY dense, Y = dX pre-zeroed).
 *   Backward-data of a stride-1 conv is the same call with W = the transposed kernel [K][N].
 * pf_conv1x1_wrw:  dW[n][k] = sum_m dY[m][n] * Q(X)[row(m)][k], dW float32 or bf16 [N][K];
 *   workspace: (pf_conv1x1_wrw_splits(M, N, K) + 32) * N * K floats (deterministic staged reduction).
 * Requirements: K % 8 == 0, N % 8 == 0, 16-byte aligned pointers; hipErrorInvalidValue otherwise.     */
/* G of the partial-statistics array for an [M][K] x [N][K] problem.  Three kernels serve these products (the barrier-free
 * resident-kernel variant, the direct-to-LDS staged GEMM, the register-staged tiles), each with its own G; ONE host-side plan
 * names the kernel, and this query and the launch both read it, so the rows a launch writes are the rows this names.
 * prologue: scale_shift != NULL.  The query reads a stride-1 launch; a launch whose row map moves it to a kernel with another
 * G (an input beyond a kernel's 31-bit addressing) returns hipErrorInvalidValue and writes nothing.                         */
int pf_conv1x1_stats_groups_k(int M, int N, int K, int prologue);
int pf_conv1x1_fwd(const void* X, const void* W, void* Y, const void* R, const float* scale_shift,
                   int act, const uint32_t* slot, int bits, float* partial, int M, int N, int K,
                   int Ho, int Wo, int H, int Wd, int stride, int ymap, void* stream);
/* pf_conv1x1_fwd with the CONSUMER's inference-mode BN + activation folded into the epilogue (round 6):
 *   Y[m][n] = bf16( act_out( out_scale[n] * bf16(conv)[m][n] + out_shift[n] ) ),  out_scale_shift = [2][N] float32
 * -- bit for bit what pf_bn_act_quant_apply(quantize = 0) makes of the stored convolution output, without the write + read of
 * that output in between.  No residual, no statistics.  Used by forward_eval networks: tf.layers.batch_normalization(training=False)
 * behind a convolution (utils/external/resnet_model.py:55-66 under the distillation teacher, learners/distillation_helper.py:60-84).
 * Shapes outside the fused kernels run the plain launch and the stand-alone pass in place (same result). */
int pf_conv1x1_fwd_affine(const void* X, const void* W, void* Y, const float* scale_shift, int act,
                          const float* out_scale_shift, int out_act, int M, int N, int K, int Ho, int Wo, int H, int Wd,
                          int stride, void* stream);
/* backward-data of a stride-1 1x1 convolution, dQ[M][K] = dY[M][N] * W[N][K] (Wt = transposed kernel [K][N]),
 * with the statistics pass of the BN backward of the layer that produced Q fused into the epilogue
 * (replaces FusedBatchNormGrad's reduction over dy, utils/external/resnet_model.py:55-62):
 * partial[G][2][K] = {sum dy, sum dy*xhat}, dy = dQ * act'(scale*x+shift), G = pf_conv1x1_stats_groups_k(M, K, N, 0),
 * in the layout pf_bn_bwd_finalize consumes.                                                              */
int pf_conv1x1_bwd_data_bnstats(const void* dY, const void* Wt, void* dQ, const void* bn_x,
                                const float* bn_scale_shift, const float* bn_mean_invstd, int bn_act,
                                float* partial, int M, int N, int K, void* stream);
/* The same backward-data for a consumer that needs only the BN backward of dQ (an identity bottleneck block: bn1's apply pass is
 * dQ's one reader), as a PAIR of launches that never stores dQ (bf16 only):
 *   pf_conv1x1_bwd_data_bnsums   the launch above without its store: the same partial[G][2][K], bit for bit;
 *   (pf_bn_bwd_finalize on the partials: dgamma, dbeta)
 *   pf_conv1x1_bwd_data_bnapply  the product again, with pf_bn_bwd_apply_add as its row pass on the tile rounded to bf16 as it would
 *                                have been stored: dx[M][K] = bf16( scale * (dy - dbeta/M - xhat * dgamma/M) [+ addend] ), the bits of
 *                                the three-launch route.  act: PF_ACT_RELU / PF_ACT_RELU6.  addend ([M][K], the shortcut's gradient)
 *                                may be NULL: then nothing is added.
 * pf_conv1x1_bwd_apply_plan(M, N, K): non-zero where the pair is offered -- the plan of the launch above names the resident kernel
 * in a compiled slice width, and K >= 2 * N.  Elsewhere both entries return hipErrorInvalidValue; the three launches remain.   */
int pf_conv1x1_bwd_apply_plan(int M, int N, int K);
int pf_conv1x1_bwd_data_bnsums(const void* dY, const void* Wt, const void* bn_x, const float* bn_scale_shift,
                               const float* bn_mean_invstd, int bn_act, float* partial, int M, int N, int K, void* stream);
int pf_conv1x1_bwd_data_bnapply(const void* dY, const void* Wt, const void* x, const float* scale_shift,
                                const float* mean_invstd, int act, const float* dgamma, const float* dbeta,
                                const void* addend, void* dx, int M, int N, int K, void* stream);
/* backward-data of a stride-1 1x1 convolution that JOINS the gradient of a second consumer of Q (a projection block: conv1 and the
 * shortcut convolution both read bn1's output):  dQ[m][k] = bf16( sum_n dY[m][n] * W[n][k] + R(m)[k] ), one rounding.
 *   r_stride == 1: R is dense, [M][K], R(m) = R[m] (the other arguments of the geometry are ignored).
 *   r_stride  > 1: R is COMPACT, [imgs][r_Ho][r_Wo][K] with r_Ho = ceil(r_H / r_stride), r_Wo = ceil(r_W / r_stride) and
 *     M = imgs * r_H * r_W: row m = (img, h, w) takes row (img, h / r_stride, w / r_stride) of R when h and w are multiples of
 *     r_stride and exactly +0.0f otherwise -- bit for bit what a zero-filled [M][K] tensor with the rows scattered into it gives,
 *     without writing and reading the zeros.
 *   bn_x != NULL: the BN-backward sums of pf_conv1x1_bwd_data_bnstats, taken from the stored (joined, rounded) dQ:
 *     partial[G][2][K], G = pf_conv1x1_stats_groups_k(M, K, N, 0).  bn_x == NULL: no sums, partial is ignored.
 * Only the shapes pf_conv1x1_join_plan(M, N, K, 0) accepts; hipErrorInvalidValue otherwise (there is no slower route behind it).
 * pf_conv1x1_join_plan(M, N, K, with_stats): 0 = refused, 1 = resident-kernel variant, 2 = staged GEMM.  With with_stats it also
 * refuses the shapes on which the sums in the launch measured slower than the separate pf_bn_bwd_stats pass (the staged GEMM below
 * 2^17 rows): advice to the caller -- the entry itself computes the sums on every shape whose kernel carries them.           */
int pf_conv1x1_join_plan(int M, int N, int K, int with_stats);
int pf_conv1x1_bwd_data_join(const void* dY, const void* Wt, void* dQ, const void* R, int r_Ho, int r_Wo, int r_H, int r_W,
                             int r_stride, const void* bn_x, const float* bn_scale_shift, const float* bn_mean_invstd,
                             int bn_act, float* partial, int M, int N, int K, void* stream);
int pf_conv1x1_wrw_splits(int M, int N, int K);
int pf_conv1x1_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace,
                   const float* scale_shift, int act, const uint32_t* slot, int bits, int M, int N,
                   int K, int Ho, int Wo, int H, int Wd, int stride, void* stream);

/* ---- K12: dense RxS convolutions as implicit GEMMs on the matrix cores (pf_igemm.hip) ----------------------------
 * replaces tf.nn.conv2d / Conv2DBackpropInput of the 3x3 convolutions of the ResNet blocks
 * (utils/external/resnet_model.py:92-103 conv2d_fixed_padding, :257-314 conv2 of _bottleneck_block_v2) and serves
 * as the plain GEMM of the 1x1 convolutions that carry no prologue.
 *
 * pf_conv2d_fwd:  Y[img][ho][wo][n] = sum_{r,s,c} X[img][ho*stride + r - pad_h][wo*stride + s - pad_w][c] * W[n][r][s][c]
 *   X [imgs][H][Wd][C] bf16 NHWC, W [N][th][tw][C] bf16 (KRSC), Y [imgs][Ho][Wo][N] bf16; taps outside the image read
 *   zeros (`zero`: >= 128 zero bytes in device memory, 16-byte aligned).  C % 64 == 0, N % 8 == 0.
 *   Epilogue: R != NULL adds a residual [M][N]; partial != NULL receives per-channel {sum, sumsq, min, max} of the stored
 *   values as [G][4][N], G = pf_conv2d_stats_groups_geom(<the arguments of this call>), M = imgs*Ho*Wo (layout of
 *   pf_bn_finalize, pivot 0); with
 *   bn_x != NULL instead the BN-backward sums {sum dy, sum dy*xhat} [G][2][N] of the BN whose input is bn_x [M][N]
 *   (dy = Y * act'(scale*x + shift)), as pf_conv1x1_bwd_data_bnstats.
 *   Backward-data of a stride-1 convolution is the same call on dY with the kernel flipped and transposed:
 *   W'[c][r][s][n] = W[n][th-1-r][tw-1-s][c], pad' = th-1-pad.                                                      */
/* rows G for the pf_conv2d_fwd call with these arguments (the kernel, and with it G, depends on the geometry)                 */
int pf_conv2d_stats_groups_geom(int imgs, int H, int Wd, int C, int N, int th, int tw, int stride, int pad_h, int pad_w,
                                int Ho, int Wo);
int pf_conv2d_fwd(const void* X, const void* W, void* Y, const void* zero, const void* R, float* partial,
                  const void* bn_x, const float* bn_scale_shift, const float* bn_mean_invstd, int bn_act,
                  int imgs, int H, int Wd, int C, int N, int th, int tw, int stride, int pad_h, int pad_w,
                  int Ho, int Wo, void* stream);
/* pf_conv2d_fwd with the consumer's inference-mode BN + activation folded into the epilogue: see pf_conv1x1_fwd_affine */
int pf_conv2d_fwd_affine(const void* X, const void* W, void* Y, const void* zero, const float* out_scale_shift, int out_act,
                         int imgs, int H, int Wd, int C, int N, int th, int tw, int stride, int pad_h, int pad_w, int Ho, int Wo,
                         void* stream);

/* pf_conv2d_wrw: backward-filter of the same convolutions (Conv2DBackpropFilter), dW[n][r][s][c] = sum_m dY[m][n] *
 * X[pix(m, r, s)][c], dW float32 or bf16 in KRSC layout; deterministic (fixed-order reductions, no atomics).
 * C % 64 == 0, N % 64 == 0, M = imgs*Ho*Wo >= 2048; workspace: (pf_conv2d_wrw_splits(M, N, C, th*tw) + 32) * N*th*tw*C
 * floats (pf_conv2d_wrw_splits returns 0 for unsupported shapes).                                                   */
int pf_conv2d_wrw_splits(int M, int N, int C, int taps);
int pf_conv2d_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H, int Wd, int C,
                  int N, int th, int tw, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- backward-data layout of all convolution kernels in one launch -------------------------------------------------
 * Conv2DBackpropInput needs W'[c][R-1-r][S-1-s][n] = W[n][r][s][c]; one 64 x 64 tile of one (kernel, tap) matrix per
 * workgroup, described by a PfTransposeTile (built once on the host).  src / dst: flat buffers of `dtype`.            */
typedef struct PfTransposeTile {
  int64_t src_off, dst_off;   /* element offsets of the [O][I] source matrix / the [I][O] destination matrix        */
  int32_t O, I, src_ld, dst_ld;
  int32_t o0, i0;             /* tile origin                                                                        */
  int32_t reserved0, reserved1;
} PfTransposeTile;
int pf_seg_transpose(const void* src_flat, void* dst_flat, int dtype, const void* tiles, int n_tiles, void* stream);

/* ---- K13: max-pooling of the ResNet stem (tf.layers.max_pooling2d, padding SAME: utils/external/resnet_model.py:522-526)
 * and MaxPoolGrad, NHWC float32 / bf16, C % 8 == 0.  Padding is -inf (clipped windows).  idx[B][Ho][Wo][C] (uint8, may be
 * NULL in the forward call) holds r*k+s of the FIRST maximum of each window, the element the gradient is routed to.
 * pf_maxpool_bwd writes every dx element exactly once (gather over the windows that contain it): no atomics.           */
int pf_maxpool_fwd(const void* x, void* y, void* idx, int dtype, int B, int H, int W, int C, int k, int stride,
                   int pad_h, int pad_w, int Ho, int Wo, void* stream);
int pf_maxpool_bwd(const void* dy, const void* idx, void* dx, int dtype, int B, int H, int W, int C, int k, int stride,
                   int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- the ResNet stem: 7x7 / stride 2 / pad 3 convolution of a 3-channel image to 64 channels --------------------
 * replaces the initial conv2d_fixed_padding of utils/external/resnet_model.py:478-486 (tf.pad + tf.layers.conv2d VALID).
 * X [imgs][H][Wd][3] bf16 (NHWC), W [64][7][7][3] bf16 (KRSC), Y [imgs][H/2][Wd/2][64] bf16.  H even, Wd % 32 == 0:
 * pf_conv_stem_supported tells whether a (H, Wd, C, N, k, stride, pad) convolution is this one.                        */
int pf_conv_stem_supported(int H, int Wd, int C, int N, int k, int stride, int pad);
int pf_conv_stem_fwd(const void* X, const void* W, void* Y, int imgs, int H, int Wd, void* stream);
/* backward-filter of the same convolution (Conv2DBackpropFilter): dW [64][7][7][3] in dw_dtype (PF_F32 / PF_BF16) from
 * dY [imgs][H/2][Wd/2][64] bf16 and X; deterministic (fixed-order slab reduction).  Wd <= 256.  workspace:
 * (pf_conv_stem_wrw_slabs(imgs, H, Wd) + 32) * 64 * 147 floats (pf_conv_stem_wrw_slabs returns 0 for unsupported shapes). */
int pf_conv_stem_wrw_slabs(int imgs, int H, int Wd);
int pf_conv_stem_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H, int Wd,
                     void* stream);

/* ---- the MobileNet-v1 stem (round 5): 3x3 / stride 2 convolution of a 3-channel image to 16 or 32 channels, 'SAME' padding -----
 * replaces the first slim.conv2d of utils/external/mobilenet_v1.py:233-262 (conv_defs[0] = Conv(kernel=[3, 3], stride=2, depth=32);
 * depth multipliers 1.0 and 0.5) and its Conv2DBackpropFilter.  X [imgs][H][Wd][3] bf16 (NHWC), W [N][3][3][3] bf16 (KRSC),
 * Y / dY [imgs][Ho][Wo][N] bf16.  pad_h / pad_w are TensorFlow's FRONT pads (0 | 1); positions behind the image read zeros
 * (no padded copy of the image).  Wd even, Wo % 16 == 0 (pf_conv_stem3_supported).  Backward-filter: dW in dw_dtype, deterministic;
 * workspace (pf_conv_stem3_wrw_slabs(...) + 32) * N * 27 floats (0 slabs: unsupported shape).
 * Pixels must be FINITE: the forward kernel pads its contraction from 27 to 96 with zero weights against real neighbouring pixels, so a
 * NaN / Inf pixel would reach (as 0 * Inf) outputs whose window does not contain it (decoded images are finite).      */
int pf_conv_stem3_supported(int H, int Wd, int C, int N, int k, int stride, int pad_h, int pad_w, int Ho, int Wo);
int pf_conv_stem3_fwd(const void* X, const void* W, void* Y, int imgs, int H, int Wd, int N, int pad_h, int pad_w, int Ho, int Wo,
                      void* stream);
int pf_conv_stem3_wrw_slabs(int imgs, int H, int Wd, int N, int pad_h, int pad_w, int Ho, int Wo);
int pf_conv_stem3_wrw(const void* dY, const void* X, void* dW, int dw_dtype, float* workspace, int imgs, int H, int Wd, int N,
                      int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- K12 (MobileNet): depthwise 3x3 convolutions, NHWC float32 / bf16, kernel [C][3][3] in the activation dtype ----------
 * replaces DepthwiseConv2dNative / ...BackpropInput / ...BackpropFilter behind slim.separable_conv2d(num_outputs=None)
 * (utils/external/mobilenet_v1.py:264-292).  stride 1 | 2; pad_h / pad_w are TensorFlow's FRONT pads of 'SAME'
 * (floor(total / 2); the rest behind is implied by Ho / Wo).  C % 8 == 0 and 8 <= C <= 2048 (pf_depthwise_supported).
 * pf_depthwise_fwd: partial (may be NULL) receives the per-channel {sum, sum of squares, min, max} of the stored outputs,
 * [G][4][C] with G = pf_depthwise_groups(B, Ho, Wo, C) -- the statistics of the BatchNorm behind the layer (pf_bn_finalize).
 * pf_depthwise_wrw: slabs = workspace of (pf_depthwise_groups(B, Ho, Wo, C) + 32) * C * 9 floats; fixed-order reduction.  */
int pf_depthwise_supported(int C, int k, int stride);
int pf_depthwise_groups(int B, int Ho, int Wo, int C);
int pf_depthwise_fwd(const void* X, const void* W, void* Y, int dtype, float* partial, int B, int H, int Wd, int C, int k,
                     int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);
int pf_depthwise_bwd_data(const void* dY, const void* W, void* dX, int dtype, int B, int H, int Wd, int C, int k,
                          int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);
int pf_depthwise_wrw(const void* dY, const void* X, void* dW, int dtype, int dw_dtype, float* slabs, int B, int H, int Wd,
                     int C, int k, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);
/* MobileNet-v2 (the 6x expansion has the depthwise layer as its only reader): pf_depthwise_fwd / pf_depthwise_wrw with the producer
 * BatchNorm's normalise / activation / fake-quant as their prologue, the argument set of the 1x1 prologue (pf_conv1x1_fwd).  X is the
 * RAW tensor in front of the BatchNorm, scale_shift float32 [2][C], act PF_ACT_NONE | PF_ACT_RELU6 (no ReLU form is built: refused), slot the quantiser's range (NULL: no quantiser;
 * bits 1..32 with one).  A tap inside the image has exactly the value pf_bn_act_quant_apply would have stored (rounded to the storage
 * type); a tap outside contributes 0.  Outputs, statistics, slabs and reduction orders are those of the plain entries: bit-identical
 * to pf_bn_act_quant_apply followed by pf_depthwise_fwd / pf_depthwise_wrw.                                                        */
int pf_depthwise_fwd_act(const void* X, const float* scale_shift, int act, const uint32_t* slot, int bits, const void* W, void* Y,
                         int dtype, float* partial, int B, int H, int Wd, int C, int k, int stride, int pad_h, int pad_w, int Ho,
                         int Wo, void* stream);
int pf_depthwise_wrw_act(const void* dY, const void* X, const float* scale_shift, int act, const uint32_t* slot, int bits, void* dW,
                         int dtype, int dw_dtype, float* slabs, int B, int H, int Wd, int C, int k, int stride, int pad_h, int pad_w,
                         int Ho, int Wo, void* stream);

/* ---- K13: input pipeline tail -----------------------------------------------------------
 * replaces, per image, the preprocessing chain of utils/external/imagenet_preprocessing.py:226-260 behind the JPEG
 * decoder: training  random_flip_left_right -> tf.image.resize_images(BILINEAR, align_corners=False) -> - means;
 *          eval      _aspect_preserving_resize(256) -> _central_crop(224, 224) -> - means
 * (ilsvrc12_dataset.py:75-93 parse_fn).  `src` holds the decoded uint8 HWC (3-channel) images of one mini-batch back
 * to back; desc[i] describes image i.  Output: [B][OH][OW][3] in out_dtype (PF_F32 / PF_BF16).
 * Resize semantics: TF-1.x legacy bilinear (in = out * scale, no half-pixel offset); the flip mirrors the SOURCE.  */
typedef struct PfImageDesc {
  int64_t offset;          /* first byte of the image inside src                                                  */
  int32_t h, w;            /* source height / width                                                               */
  float scale_y, scale_x;  /* float32(in_size / out_size) of the (virtual) resized image                          */
  int32_t off_y, off_x;    /* top-left corner of the output window inside the resized image (central crop)        */
  int32_t flip;            /* 1: mirror the source horizontally before resizing                                   */
  int32_t reserved;
} PfImageDesc;
int pf_image_resize_bilinear(const void* src, const PfImageDesc* desc, void* out, int out_dtype, int B, int OH,
                             int OW, float mean_r, float mean_g, float mean_b, void* stream);

/* Backward-data of a STRIDED R x S convolution (resnet_model.py:92-103 conv2d_fixed_padding with strides 2; TF's
 * Conv2DBackpropInput) by output-parity classes: stride * stride stride-1 launches of the implicit-GEMM kernel over dY, each walking
 * a sub-grid of the flipped / transposed kernel buffer Wt[C][R][S][N] (Wt[c][r'][s'][n] = W[n][R-1-r'][S-1-s'][c]) in place and
 * scattering its rows to the class's input pixels.  bf16; N % 64 == 0, C % 8 == 0, H % stride == W % stride == 0, R, S >= stride. */
int pf_conv2d_bwd_data_strided(const void* dY, const void* Wt, void* dX, const void* zero, int imgs, int H, int Wd, int C, int N,
                               int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);
/* ... with the BN-backward sums {sum dy, sum dy * xhat} of the BN whose OUTPUT the convolution read (its input bn_x has dX's shape) in
 * the epilogues, as pf_conv1x1_bwd_data_bnstats: partial [G][2][C], G = pf_conv2d_bwd_data_strided_stats_groups(imgs, H, Wd, C, stride)
 * (one slice of workgroup rows per parity class); replaces a pf_bn_bwd_stats pass over dX and bn_x. */
int pf_conv2d_bwd_data_strided_stats_groups(int imgs, int H, int Wd, int C, int stride);
int pf_conv2d_bwd_data_strided_bnstats(const void* dY, const void* Wt, void* dX, const void* zero, const void* bn_x,
                                       const float* bn_scale_shift, const float* bn_mean_invstd, int bn_act, float* partial,
                                       int imgs, int H, int Wd, int C, int N, int R, int S, int stride, int pad_h, int pad_w,
                                       int Ho, int Wo, void* stream);

/* ---- K12, general form: convolutions of any shape and stride, the dense layer; float32 or bf16 storage, float32 accumulation --
 * replaces tf.nn.conv2d / tf.layers.conv2d / slim.conv2d, their Conv2DBackpropInput / Conv2DBackpropFilter and tf.layers.dense for
 * every shape the MFMA kernels above do not take, and ALL of them in the float32 parity mode:
 *   utils/external/resnet_model.py:92-103 (conv2d_fixed_padding), :552 (dense); utils/external/mobilenet_v1.py:233-292 (slim.conv2d);
 *   nets/lenet_at_cifar10.py:34-68.
 * NHWC activations [imgs][H][W][C], KRSC kernels [N][R][S][C]; pad_h / pad_w are the BEGIN pads (positions outside the image read 0,
 * whatever Ho / Wo say about the end).  A dense layer is the 1x1 convolution of a [imgs][1][1][C] tensor.  Deterministic: one fused
 * multiply-add per term in a fixed order; the backward-filter pixel splits are summed in ascending order.
 * pf_convg_wrw: `slab` = float32 workspace of pf_convg_wrw_splits(...) * N * R * S * C elements; dw [N][R][S][C] in dw_dtype.
 * pf_convg_fwd / _bwd_data: `slab` (optional, may be null) = float32 workspace of slab_elems elements: an output with fewer than 256
 * tiles of 64 x 64 (the dense layer) then splits its contraction over pf_convg_small_splits(M, Nc, K) slabs (0: no split; M = output
 * rows, Nc = output columns, K = contraction length -- a function of the shape alone), summed in ascending order; a workspace
 * smaller than splits * M * Nc elements is hipErrorInvalidValue. */
int pf_convg_small_splits(int M, int Nc, int K);
int pf_convg_fwd(const void* x, const void* w, const float* bias, void* y, int dtype, int imgs, int H, int W, int C, int N, int R,
                 int S, int stride, int pad_h, int pad_w, int Ho, int Wo, float* slab, int64_t slab_elems, void* stream);
int pf_convg_bwd_data(const void* dy, const void* w, void* dx, int dtype, int imgs, int H, int W, int C, int N, int R, int S,
                      int stride, int pad_h, int pad_w, int Ho, int Wo, float* slab, int64_t slab_elems, void* stream);
int pf_convg_wrw_splits(int imgs, int C, int N, int R, int S, int Ho, int Wo);
int pf_convg_wrw(const void* dy, const void* x, void* dw, int dtype, int dw_dtype, float* slab, int imgs, int H, int W, int C, int N,
                 int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- channel-gather convolution: the forward pass of a physically shrunk channel-pruned layer (pf_conv_gather.hip) ----------------
 * replaces tf.gather(input, nnz, axis=channel) + the smaller convolution of the reference's exported models
 * (tools/conversion/export_chn_pruned_tflite_model.py:236-276); inference only.
 *   Y[img][ho][wo][n] = sum_{r,s} sum_{j < Ck} X[img][ho*stride + r - pad_h][wo*stride + s - pad_w][gather[j]] * w[n][r][s][j]
 * x: NHWC with all C channels; w: KRSC cut along C to [N][R][S][Ck]; gather: int32[Ck], strictly ascending, values in [0, C)
 * (validated by the caller once, when the model is loaded; an out-of-range entry is skipped, never dereferenced); float32 or bf16
 * storage (dtype), float32 accumulation, bf16 on the matrix cores; pad_h / pad_w are symmetric pads (positions outside the image
 * read 0).  Optional epilogue, in this order: + bias[N] (float32), + res[imgs][Ho][Wo][N] (storage type, added before the one
 * rounding), act(scale_shift[n] * y + scale_shift[N + n]) (a folded inference-mode BatchNorm; `act` is ignored without scale_shift);
 * all three act on the float32 accumulator, the result is rounded to the storage type once.  C <= 8192.  Deterministic: no atomics, fixed summation order. */
int pf_conv_gather_fwd(const void* x, const void* w, const int32_t* gather, const float* bias, const void* res,
                       const float* scale_shift, int act, void* y, int dtype, int imgs, int H, int W, int C, int Ck, int N, int R,
                       int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- int8 inference of a uniformly quantised convolution (pf_conv_i8.hip) -----------------------------------------------------------
 * The reference quantises weights and activations to unsigned codes on affine grids (learners/uniform_quantization/utils.py:163-245:
 * x_q = alpha * round((x - beta) / alpha * k) / k + beta, k = 2^bits - 1) and then multiplies the DECODED floats
 * (utils.py:51-79 insert the quantisers in front of every Conv2D / MatMul); its integer deployment goes through TF-Lite
 * (tools/conversion/export_quant_tflite_model.py:196-249).  These entries multiply the codes themselves on the i8 matrix cores:
 *   y[m][n] = (alpha_a/k_a)(alpha_w[n]/k_w) P + (alpha_a/k_a) beta_w[n] Sc + beta_a ((alpha_w[n]/k_w) Dv + beta_w[n] V),
 *   P = sum_window c d and Sc = sum_window c exact in integers (padding taps hold code 0), Dv = the sum of d[n] over the taps inside the
 *   image, V = their count * C; the float32 terms are added in this order, then the residual, then one rounding to the output type.
 * pf_bn_act_quant_codes: the twin of pf_bn_act_quant_apply that stores code = rint((act(scale * x + shift) - beta) / alpha * k) as
 *   one byte per element (NHWC, bits <= 8) -- the same float32 arithmetic up to that rounding -- and the decoded (alpha, beta) of the
 *   slot to alpha_beta[2].
 * pf_conv_i8_fwd: x uint8 codes [imgs][H][W][C]; w signed bytes d - 128 as [N][Kp], Kp = R*S*C rounded up to 64, KRSC order, zero beyond
 *   R*S*C; act_alpha_beta the pair the producer wrote; w_scale_beta [N][2] = (alpha_w/k_w, beta_w); w_tsum [N] = sum over the window of
 *   (d - 128); w_tapsum [N][R*S] = per-tap sums of d (read only when beta_a != 0); res / y [imgs][Ho][Wo][N] of out_dtype (res may be
 *   NULL); symmetric pads.  All pointers 16-byte aligned.  Deterministic: no atomics, fixed summation order.
 * pf_conv_i8_supported (host): C % 16 == 0, N % 8 == 0, stride 1 or 2, R*S*C * 2^14 < 2^31 (the int32 accumulator).            */
int pf_bn_act_quant_codes(const void* x, uint8_t* codes, int dtype, int64_t rows, int C, const float* scale_shift, int act,
                          const uint32_t* slot, int bits, float* alpha_beta, void* stream);
int pf_conv_i8_supported(int C, int N, int R, int S, int stride);
int pf_conv_i8_fwd(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                   const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, void* y, int out_dtype, int imgs, int H, int W,
                   int C, int N, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- int8 inference of MobileNet-v1's depthwise 3x3 layers (pf_depthwise_i8.hip) -------------------------------------------------------
 * slim.separable_conv2d(num_outputs=None) (utils/external/mobilenet_v1.py:264-292) behind a quantising BatchNorm + ReLU6, on the
 * producer's uint8 CODES (pf_bn_act_quant_codes) and the exported kernel's codes d[c][r][s], one (alpha_w, beta_w) per kernel:
 *   y[b][ho][wo][c] = (alpha_a/k_a)(alpha_w/k_w) P + (alpha_a/k_a) beta_w Sc + beta_a ((alpha_w/k_w) Dv + beta_w V),
 *   P = sum over the taps inside the image of code * d[c][r][s], Sc = the sum of those codes, Dv = the sum of those d[c][r][s], V =
 *   their number; P, Sc, Dv exact in int32 (v_dot4_u32_u8), the float32 terms added in this order, one rounding to the output type.
 * pf_dw_i8_fwd: x uint8 codes [B][H][W][C]; w_cols uint32 [C][3], entry [c][s] = d[c][0][s] | d[c][1][s] << 8 | d[c][2][s] << 16;
 *   w_scale_beta [2] = (alpha_w / k_w, beta_w); act_alpha_beta the pair the producer wrote (never read by the host); y [B][Ho][Wo][C]
 *   of `dtype`; pad_h / pad_w are the FRONT pads of TensorFlow 'SAME' (0..2; positions outside the image on either side contribute
 *   nothing).  x and y 16-byte aligned, fewer than 2^31 elements each.  Returns non-zero without launching for a shape
 *   pf_dw_i8_supported rejects or a null pointer.  Deterministic: no atomics, no workspace.
 * pf_dw_i8_supported (host): C % 16 == 0, k == 3, stride 1 or 2. */
int pf_dw_i8_supported(int C, int k, int stride);
int pf_dw_i8_fwd(const uint8_t* x, const uint32_t* w_cols, const float* w_scale_beta, const float* act_alpha_beta, int act_bits, void* y,
                 int dtype, int B, int H, int W, int C, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- fixed (calibrated) activation ranges for int8 inference (pf_act_static.hip, pf_conv_i8_q.hip, pf_depthwise_i8_q.hip) ----------
 * The static quantiser: t = ((u - beta) / alpha) * k, t = min(max(t, 0), k), level = rint(t), value = alpha * (level / k) + beta --
 * the float32 chain of pf_bn_act_quant_apply / _codes plus ONE clamp in front of the rounding -- against out_alpha_beta[2], a DEVICE
 * pair (alpha, beta) = ((max - min) + 1e-10f, min) of a range calibrated once; it is never read by the host and no slot is written.
 * out_kind: 0 = uint8 levels (bits <= 8), 1 = the value in float32, 2 = the value in bf16.
 * pf_bn_act_quant_static: out[rows][C] = the static quantiser of act(scale * x + shift), x float32 / bf16 (`dtype`); bits 1..32 for
 *   values.  The 8-channel vector map where C % 8 == 0 and C / 8 divides 256 and the pointers are aligned, a scalar loop otherwise.
 * pf_conv_i8_fwd_q / pf_dw_i8_fwd_q: pf_conv_i8_fwd / pf_dw_i8_fwd whose epilogue applies the ONE consumer's folded BatchNorm
 *   (out_scale_shift [2][N or C], 16-byte aligned), activation and static quantiser (out_bits <= 8) to the float32 output and stores
 *   `out_kind`: bit for bit pf_bn_act_quant_static applied to the float32 output of the parent entry.  pf_conv_i8_fwd_q refuses a
 *   residual (res must be NULL).  All three return non-zero without launching for a null pointer, an unknown out_kind or a shape
 *   their parent rejects.  Deterministic. */
int pf_bn_act_quant_static(const void* x, void* out, int dtype, int out_kind, int64_t rows, int C, const float* scale_shift, int act,
                           const float* out_alpha_beta, int bits, void* stream);
int pf_conv_i8_fwd_q(const uint8_t* x, const int8_t* w, const float* act_alpha_beta, int act_bits, const float* w_scale_beta,
                     const int32_t* w_tsum, const int32_t* w_tapsum, const void* res, const float* out_scale_shift, int out_act,
                     const float* out_alpha_beta, int out_bits, void* out, int out_kind, int imgs, int H, int W, int C, int N, int R,
                     int S, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);
int pf_dw_i8_fwd_q(const uint8_t* x, const uint32_t* w_cols, const float* w_scale_beta, const float* act_alpha_beta, int act_bits,
                   const float* out_scale_shift, int out_act, const float* out_alpha_beta, int out_bits, void* out, int out_kind, int B,
                   int H, int W, int C, int stride, int pad_h, int pad_w, int Ho, int Wo, void* stream);

/* ---- R x S convolutions with few input channels (ResNet-20 @ CIFAR-10: resnet_model.py:156-199 with 16 / 32 filters) --------------
 * bf16, C % 8 == 0.  pf_im2col gathers Xcol[imgs*Ho*Wo][R*S*C] (taps outside the image: zeros) so that the convolution and its two
 * gradients are 1x1 products on pf_conv1x1_fwd / pf_conv1x1_wrw over Xcol and the [N][R*S*C] view of the KRSC kernel; pf_col2im is
 * the inverse gather of backward-data (per input pixel: float32 sum of its <= R*S terms in tap order, one rounding). */
int pf_im2col(const void* x, void* xcol, int imgs, int H, int W, int C, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo,
              void* stream);
int pf_col2im(const void* dxcol, void* dx, int imgs, int H, int W, int C, int R, int S, int stride, int pad_h, int pad_w, int Ho, int Wo,
              void* stream);

/* ---- proximal-gradient channel selection of the 'chn-pruned-gpu' learner ----------------------------------------------------------
 * replaces learners/channel_pruning_gpu/learner.py:379-383 (var_prnd_new = var - lr * grad; var_norm = sqrt(reduce_sum(square, axes
 * [0, 1, 3])); threshold = percentile(var_norm, p); shrk_vec = maximum(1 - threshold / var_norm, 0); assign(var_prnd_new * shrk_vec)).
 * w: float32 master kernel in KRSC storage = [rows = O*R*S][I] with the input channel innermost; g: its gradient (float32 / bf16).
 * pf_prox_norms: norms[I] of W - lr * G (partial: float32 workspace of pf_prox_groups(rows, I) * I elements; deterministic).
 * The threshold is pf_kth_largest_nonneg over `norms` at the nearest-rank index of the percentile (host arithmetic as for K7).
 * pf_prox_apply: W <- (W - lr * G) * max(1 - thr[0] / norms[c], 0). */
int pf_prox_groups(int64_t rows, int I);
int pf_prox_norms(const float* w, const void* g, int g_dtype, float lr, int64_t rows, int I, float* partial, float* norms, void* stream);
int pf_prox_apply(float* w, const void* g, int g_dtype, float lr, int64_t rows, int I, const float* norms, const float* thr, void* stream);

/* ---- channel selection of the 'chn-pruned-rmt' learner (pf_cpr.hip; reference learners/channel_pruning_rmt/learner.py) -------------
 * pf_cpr_gather: rows row0 + crop * B + b of P[rows][kh*kw][C] (input patches of x, zeros outside the image) and Y[rows][Co] (output
 *   vectors of y) at the drawn output positions pos[crops][2] = (oh, ow); x [B][H][W][C] and y [B][OH][OW][Co] NHWC, float32 / bf16.
 * pf_cpr_gram: over the secondary sample idx[n] of those rows, X[i*Co + o][c] = sum_k P[idx[i]][k][c] * W[o][k][c] (W: KRSC float32),
 *   X^T X and X^T y in float64, divided by ||X^T X||_F and written as float32 xtx[C][C], xty[C]; ws: pf_cpr_gram_ws(C) doubles.
 * pf_cpr_ista: `iters` ISTA iterations from m0 with threshold gamma * lr; the result in mask[C], its non-zero count in nnz[0];
 *   m_ws: 2 * C floats.
 * pf_cpr_lstsq_step: one Adam step on W[K][Co] (HWIO kernel matrix, K = kh*kw*C) for the kept rows kidx[Kp] (pos[K]: position in kidx
 *   or -1); R: N x Co residual workspace; part: pf_cpr_lstsq_splits(N, Kp, Co) * Kp * Co floats.  pf_cpr_lstsq_resid: R alone. */
int pf_cpr_gather(const void* x, int x_dtype, const void* y, int y_dtype, const int* pos, int crops, int B, int H, int W, int C, int OH, int OW,
                  int Co, int kh, int kw, int stride, int pad_t, int pad_l, float* P, float* Y, int64_t row0, void* stream);
int64_t pf_cpr_gram_ws(int C);
int pf_cpr_gram(const float* P, const float* Y, const int* idx, int64_t n, int kk, int C, int Co, const float* w, double* ws, int64_t ws_elems,
                float* xtx, float* xty, void* stream);
int pf_cpr_ista(const float* A, const float* b, const float* m0, float* m_ws, float* mask, int C, float gamma, float lr, int iters, int* nnz,
                void* stream);
int pf_cpr_lstsq_splits(int64_t N, int Kp, int Co);
int pf_cpr_lstsq_step(const float* P, int K, const int* kidx, const int* pos, int Kp, const float* Y, float* R, int64_t N, int Co, float* W,
                      float* m, float* v, float* part, float wd, float lr_t, float beta1, float beta2, float c1, float c2, float eps,
                      void* stream);
int pf_cpr_lstsq_resid(const float* P, int K, const int* kidx, int Kp, const float* W, const float* Y, float* R, int64_t N, int Co,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* POCKETFLOW_HIP_H_ */
