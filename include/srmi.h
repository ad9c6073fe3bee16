/* srmi -- MI355X-native (gfx950) engine for the RCAN / EDSR tiled
 * super-resolution hot path of nasa-nccs-hpda/super-resolution-climate.
 *
 * C ABI: plain pointers, sizes and a hipStream_t (passed as void*).  No torch
 * types.  All device memory is owned by the caller (PyTorch's caching
 * allocator on the Python side) and handed in as workspace; the library's only
 * allocation is host-side: the srmi_engine object (plan, workspace layout, pack
 * tables), created by srmi_engine_create and released by srmi_engine_destroy.
 * It creates no streams and no events: every launch goes to the caller's stream
 * (group events for a bucketed all-reduce are the caller's).  Every entry point returns 0
 * on success or a negative status (SRMI_ERR_*, or -hipError_t), which the
 * Python binding raises as RuntimeError (the reference raises Python
 * exceptions; sres/controller/dual_trainer.py:557 @exception_handled).
 *
 * Reference interface each group replaces (paths relative to the reference):
 *   srmi_param_*, srmi_engine_*  -> sres/model/manager.py:93-96 get_model plugin
 *                                   + sres/model/common/common.py:22-48 FModule
 *   srmi_forward                 -> RCAN.forward sres/model/rcan/network.py:22-27,
 *                                   EDSR.forward sres/model/edsr/network.py:27-32
 *   srmi_backward                -> autograd of the above (dual_trainer.py:322)
 *   srmi_rmse_*, srmi_loss_*     -> l2loss sres/controller/stats.py:5-8
 *   srmi_charbonnier_partial     -> ModelTrainer.charbonnier dual_trainer.py:196-198
 *   srmi_downsample/_upsample    -> sres/base/util/array.py:72-76 / :84-87
 *   srmi_interpolate             -> the same with torch_interp_mode, array.py:37-41
 *   srmi_adam_step               -> torch.optim.Adam, dual_trainer.py:126,323
 *   srmi_grad_norm_workspace,
 *   srmi_grad_norm               -> torch.nn.utils.clip_grad_norm_ (norm, coefficient) and
 *                                   a finite-norm flag.  The reference never clips.
 *   srmi_adam_step_guarded       -> torch.optim.Adam on the clipped gradient, skipped when
 *                                   the norm is not finite, and in the same pass
 *                                   torch.optim.swa_utils.get_ema_multi_avg_fn's update of
 *                                   averaged weights.  The reference keeps no average.
 *   srmi_conv3x3* / srmi_wgrad*  -> nn.Conv2d of default_conv
 *                                   sres/model/common/cnn.py:8-9 (op level)
 *   srmi_ca_*                    -> CALayer sres/model/rcan/network.py:31-47
 *   srmi_region_to_tiles         -> get_tiles + 'lnorm' norm
 *                                   sres/base/source/swot/raw.py:216-233, :169-181
 *   srmi_batch_prep              -> norm 'lnorm' (swot/raw.py:169-181) + xyflip
 *                                   sres/base/source/batch.py:37-49 + downsample
 *   srmi_*_norm                  -> every branch of norm, swot/raw.py:169-214
 *   srmi_tile_stats*             -> _compute_normalization + globalize_norm
 *                                   sres/base/source/swot/raw.py:89-106, :23-30
 *   srmi_llc_*, srmi_tiles_*     -> SWOTRawDataLoader.load_file + get_tiles
 *                                   sres/base/source/swot/raw.py:133-145, :216-233
 *   srmi_tiles_to_region         -> denorm + assemble_images
 *                                   sres/controller/dual_trainer.py:67-77, :482-512
 *   srmi_region_to_tiles_overlap,
 *   srmi_tiles_blend,
 *   srmi_overlap_count           -> generalise get_tiles (swot/raw.py:216-233) and
 *                                   assemble_images (dual_trainer.py:482-512) to
 *                                   overlapping tiles and a feathered blend.  The
 *                                   reference has no overlapped form: its tiles are the
 *                                   disjoint floor grid and its mosaic a concatenation.
 *                                   An extension, not a parity item.
 *   srmi_region_to_tiles_overlap_masked,
 *   srmi_tiles_blend_masked,
 *   srmi_rmse_partial_masked     -> the three above and the RMSE for regions with land
 *                                   (NaN): masked statistics, a flood fill, a re-masking
 *                                   blend, a masked score.  No reference counterpart:
 *                                   the reference drops every tile that touches land.
 *   srmi_tiles_dihedral,
 *   srmi_tiles_blend_ensemble    -> geometric self-ensemble of the overlapped tiles: the
 *                                   dihedral variants of xyflip (batch.py:37-49), their
 *                                   back-transformed mean and spread.  No reference
 *                                   counterpart: the reference flips training batches only.
 *   srmi_spectra_workspace,
 *   srmi_spectra                 -> windowed radial power spectra of a prediction against
 *                                   a truth.  No reference counterpart: the reference
 *                                   scores a field by its RMSE alone.
 *   srmi_ssim_workspace,
 *   srmi_ssim                    -> Gaussian-window SSIM of a prediction against a truth,
 *                                   with its per-pixel map, and the mean square error that
 *                                   PSNR needs.  No reference counterpart: the reference
 *                                   scores a field by its RMSE alone.
 *   srmi_distribution_workspace,
 *   srmi_distribution            -> histograms of a prediction and of a truth on the truth's
 *                                   range, their joint histogram, and the Perkins score,
 *                                   Wasserstein-1 distance and quantiles formed from them.
 *                                   No reference counterpart: the reference scores a field
 *                                   by its RMSE alone.
 *   srmi_quantile_map_accumulate_workspace,
 *   srmi_quantile_map_accumulate,
 *   srmi_quantile_map_fit,
 *   srmi_quantile_map_apply      -> empirical quantile mapping of a super-resolved field: the
 *                                   histograms of output and truth accumulated over a
 *                                   calibration set, the monotone transfer table built from
 *                                   them, and the field mapped through it.  No reference
 *                                   counterpart: the reference never calibrates its output.
 *   srmi_spectral_loss_workspace,
 *   srmi_spectral_loss_parts,
 *   srmi_spectral_loss_from_parts,
 *   srmi_spectral_loss_dy        -> a Fourier-amplitude term beside the pixel loss of a
 *                                   training step.  No reference counterpart: the
 *                                   reference trains on a pixel loss alone.
 *   srmi_consistency_residual,
 *   srmi_consistency_iterate,
 *   srmi_consistency_apply       -> back-projection of a super-resolved field onto its
 *                                   coarse input, iterated in LR space.  No reference
 *                                   counterpart: the reference never starts from a coarse
 *                                   field.
 *   srmi_consistency_adjoint_gather,
 *   srmi_consistency_adjoint_iterate,
 *   srmi_consistency_adjoint_apply -> the transpose of that correction, for training
 *                                   through it as the model's last layer.  No reference
 *                                   counterpart: the reference's networks are free regressors.
 *   srmi_gradient_workspace,
 *   srmi_gradient                -> Sobel gradients of a prediction and of a truth: mean
 *                                   magnitudes, sharpness, magnitude and vector RMSE, cosine,
 *                                   and the two magnitude maps.  No reference counterpart:
 *                                   the reference scores a field by its RMSE alone.
 *   srmi_gradient_loss_workspace,
 *   srmi_gradient_loss_parts,
 *   srmi_gradient_loss_from_parts,
 *   srmi_gradient_loss_dy        -> a term on the Sobel gradient of the error beside the pixel
 *                                   loss of a training step.  No reference counterpart: the
 *                                   reference trains on a pixel loss alone.
 *   srmi_fss_workspace,
 *   srmi_fss                     -> the fractions skill score: event fractions of a prediction
 *                                   and of a truth in n x n neighbourhoods, for a ladder of n,
 *                                   and the skilful scale.  No reference counterpart: the
 *                                   reference scores a field by its RMSE alone.
 *   srmi_ensemble_score_workspace,
 *   srmi_ensemble_score          -> an ensemble of K fields against a truth: CRPS (plain and
 *                                   fair), the rank histogram, the spread-skill ratio with a
 *                                   spread-binned reliability table, the spread-|error|
 *                                   correlation and a per-pixel CRPS map.  No reference
 *                                   counterpart: the reference has no ensemble.
 */
#ifndef SRMI_H
#define SRMI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRMI_OK 0
#define SRMI_ERR_ARG (-10001)
#define SRMI_ERR_SHAPE (-10002)
#define SRMI_ERR_WORKSPACE (-10003)
#define SRMI_ERR_UNSUPPORTED (-10004)

#define SRMI_ARCH_RCAN 0
#define SRMI_ARCH_EDSR 1

/* operand type of the engine (srmi_model_config.dtype, and the op-level entry
 * points' dtype argument):
 *   SRMI_DTYPE_BF16: activations / gradient maps / filter packs in bf16, fp32
 *     accumulation (v_mfma_f32_16x16x32_bf16), fp32 residual stream and master
 *     weights -- BASELINE configs 2, 3, 5;
 *   SRMI_DTYPE_F32: everything fp32, exact f32 MFMA (v_mfma_f32_16x16x4_f32) --
 *     the reference's own arithmetic (array2tensor fp32, sres/base/util/array.py:70;
 *     nn.Conv2d fp32, sres/model/common/cnn.py:8-9), BASELINE config 4. */
#define SRMI_DTYPE_BF16 0
#define SRMI_DTYPE_F32 1

typedef struct srmi_model_config {
  int arch;          /* SRMI_ARCH_RCAN | SRMI_ARCH_EDSR                     */
  int nchannels_in;  /* len(task.input_variables)   (1..4)                  */
  int nchannels_out; /* len(task.target_variables)  (1..4)                  */
  int nfeatures;     /* model.nfeatures (64)                                */
  int nlayers;       /* RCAN residual groups / EDSR resblocks               */
  int nblocks;       /* RCAN RCABs per group (ignored for EDSR)             */
  int reduction;     /* RCAN model.cbottleneck (channel-attention reduction): 64 / reduction
                        in 4 .. 32 and a multiple of 4 (else SRMI_ERR_UNSUPPORTED) */
  int scale;         /* prod(model.downscale_factors): 2, 4 or 8            */
  float res_scale;   /* EDSR model.res_scale                                */
  int batch;         /* max tiles per call (workspace capacity)             */
  int lr_h, lr_w;    /* LR tile size, e.g. 48 x 48                          */
  int cu_budget;     /* CUs one launch should fill (0 = the whole GPU); two
                        engines on two streams each take half the chip     */
  int dtype;         /* SRMI_DTYPE_BF16 | SRMI_DTYPE_F32                    */
  int flags;         /* SRMI_FLAG_* (0 = defaults)                           */
} srmi_model_config;
/* flags (bits 0 and 3 are retired: the CA-backward fold and the separate CA-scale
 * launch, both measured slower on MI355X and removed) */
/* SRMI_FLAG_NO_RCAB_INFER: inference engines run each RCAB as three launches (conv1,
 * conv2 + pool, CA) instead of one launch with a workgroup per image (A/B, tests) */
#define SRMI_FLAG_NO_RCAB_INFER 2
/* training forward (A/B, tests): SRMI_FLAG_CA_PASS runs each RCAB's channel attention as
 * a pass of its own after conv2 (conv1, conv2 + pool writing u, CA pass) instead of inside
 * conv2's launch */
#define SRMI_FLAG_CA_PASS 4
/* training backward (A/B, tests): SRMI_FLAG_DU_PASS has the CA backward write du = g s +
   dm / HW to memory for the conv2 backward to read (round 6), instead of the fused conv2
   backward forming du from the bf16 gradient stream in LDS (the same values, bit for bit) */
#define SRMI_FLAG_DU_PASS 16

typedef struct srmi_param_info {
  long long offset; /* element offset in the flat fp32 parameter buffer     */
  long long numel;
  int ndim;
  int shape[4];
} srmi_param_info;

typedef struct srmi_engine srmi_engine;

int srmi_version(void);

/* parameters, in state_dict order (identical keys to the reference model) */
int srmi_param_count(const srmi_model_config* cfg, long long* n_params, int* n_tensors);
int srmi_param_table(const srmi_model_config* cfg, srmi_param_info* out, int cap);

/* workspace for `train` (saves activations) or inference */
int srmi_workspace_size(const srmi_model_config* cfg, int train, size_t* bytes);
int srmi_engine_create(const srmi_model_config* cfg, void* workspace, size_t ws_bytes, int train,
                       srmi_engine** out);
int srmi_engine_destroy(srmi_engine* e);

/* fp32 master weights -> MFMA filter packs of the engine's dtype (call after every update) */
int srmi_pack_weights(srmi_engine* e, const float* params, void* stream);

/* lr: NCHW fp32 [n][Cin][lr_h][lr_w] -> sr: NCHW fp32 [n][Cout][lr_h*s][lr_w*s] */
int srmi_forward(srmi_engine* e, const float* params, const float* lr, float* sr, int n, void* stream);

/* backward of the last forward (train engines).  Either
 *   dy != NULL : upstream gradient NCHW fp32 like sr, or
 *   dy == NULL : RMSE gradient (sr - hr) * loss4[2] formed on the fly.
 * Writes every parameter gradient into grads (flat, state_dict order).
 * One event per residual group is recorded into group_events[g] (if not NULL,
 * hipEvent_t*) as soon as that group's gradients are final -- the hook for
 * bucketed all-reduce overlapped with the rest of backward. */
int srmi_backward(srmi_engine* e, const float* params, const float* lr, const float* sr, const float* hr,
                  const float* loss4, const float* dy, float* grads, void** group_events, void* stream);

/* the same backward in stages, so that a caller can enqueue work between them (a
 * residual group's gradient all-reduce right behind that group, srmi.trainer): stages
 * 0 = tail conv, upsamplers and body tail; 1 .. nlayers = residual groups nlayers-1 ..
 * 0; nlayers + 1 = head (RCAN; EDSR has one stage).  srmi_backward_stages runs stages
 * first .. last (in order, each exactly once per backward); group_events as above.
 * The engine tracks the next stage: `first` must be it (0 after a forward or a
 * completed backward), else SRMI_ERR_ARG and nothing is enqueued; srmi_backward is
 * refused while a staged backward is half-way through. */
int srmi_backward_stage_count(srmi_engine* e);
int srmi_backward_stages(srmi_engine* e, const float* params, const float* lr, const float* sr, const float* hr,
                         const float* loss4, const float* dy, float* grads, void** group_events, int first, int last,
                         void* stream);

/* diagnostic (bench roofline): re-issue `reps` times on `stream` the fused backward
 * launch of RCAB (0, 2) exactly as srmi_backward issues it (same shapes, CU split,
 * row chunks) -- which = 1: dgrad of conv1 accumulating into the gradient stream
 * (+ CA sums) beside conv1's filter gradient; which = 2: the ReLU-mask dgrad of
 * conv2 beside conv2's filter gradient -- on the buffers of the last backward
 * (their contents are overwritten).  RCAN train engines; which = 3: an RCAN
 * inference engine's one-launch RCAB (0, 2) on the buffers of the last forward;
 * which = 4 (nothing launched, reps ignored): 1 if the engine's backward runs the CA
 * backward inside the fused conv2 backward (du formed from the bf16 gradient stream),
 * 0 if as a launch of its own (SRMI_FLAG_DU_PASS, exact fp32, unfusable shapes);
 * which = 5 / 6 (nothing launched): the row chunks per image of the filter gradient
 * beside conv1's dgrad (F1, and the group tail's) / beside conv2's dgrad (F2) at the last
 * forward's n -- the partial slabs of such a launch are one per (image, row chunk,
 * 48-column block); which = 7 (nothing launched): bit 0 the RCAB backward's dgrad and
 * filter gradient run as one fused launch, bit 1 the RCAB filter gradients' partial
 * slabs are bf16, bit 2 = which 4; which = 8 (nothing launched, any RCAN engine): how the
 * forward runs an RCAB -- 0 three launches (conv1, conv2 + pool writing u, the CA pass), 1 the
 * training form with the CA inside conv2's launch, 2 the one-launch inference RCAB. */
int srmi_engine_probe(srmi_engine* e, int which, int reps, void* stream);

/* diagnostic (tests): device address, element count and element size of one of the
 * engine's saved maps, valid until the next forward / backward call on this engine.
 * Maps are [batch][lr_h][lr_w][64] (the first n images of the last forward are
 * meaningful), element size 4 for the fp32 maps and the exact-fp32 engine's, 2 (bf16)
 * else; the CA records are fp32 [batch][160] / [batch][224].  g = residual group,
 * b = RCAB 1 .. nblocks (HB: b = 0 .. nblocks, the input of RCAB b + 1; HB(nlayers, 0)
 * is the body tail's input); EDSR: g = resblock, b = 0 (HB) / 1 (T).  GROUP_IN_GRAD(g)
 * is the fp32 gradient w.r.t. group g's input, where the backward stage of group g
 * leaves it (the engine alternates two buffers; the accessor resolves which).  A
 * buffer this engine does not have (an inference engine's backward maps or per-RCAB
 * slots, EDSR's CA state), or g / b out of range: SRMI_ERR_ARG. */
#define SRMI_BUF_X0F 0
#define SRMI_BUF_HB 1
#define SRMI_BUF_T 2
#define SRMI_BUF_U 3
#define SRMI_BUF_REC 4
#define SRMI_BUF_BREC 5
#define SRMI_BUF_DU 6
#define SRMI_BUF_DZ 7
#define SRMI_BUF_DRESF 8
#define SRMI_BUF_GROUP_IN_GRAD 9
/* RESB: the body tail's output in the operand type (the upsamplers' input); PS(g = k): upsampler
 * k's pixel-shuffled output [batch][lr_h 2^(k+1)][lr_w 2^(k+1)][64], k = 0 .. log2(scale) - 1.
 * Both persist after a forward, in inference engines too. */
#define SRMI_BUF_RESB 10
#define SRMI_BUF_PS 11
/* The backward's maps outside the residual groups (train engines; else SRMI_ERR_ARG), read-only
 * views for the per-launch tests:
 *   DPS(g = k): the gradient w.r.t. PS(k), operand type, shaped as PS(k); DPS(nups - 1) is the
 *     tail conv's dgrad, DPS(k - 1) upsampler k's.  Valid after backward stage 0 until the next
 *     backward.
 *   DRESB: the operand-type copy of DRESF (upsampler 0's dgrad writes both), same validity.
 *   BODY_GRAD(b = 0 fp32 | b = 1 operand type): the gradient w.r.t. the body's last block
 *     output, as the body tail's dgrad leaves it.  RCAN: valid after stage 0 until stage 1 runs
 *     (the groups' stages alternate this buffer with a second one).  EDSR's one-stage backward
 *     reuses it for every second ResBlock: it is that gradient at nlayers == 1 only.
 *   HEAD_GRAD: the fp32 gradient w.r.t. the head's output, what the head's filter gradient
 *     reads.  RCAN: the same buffer as GROUP_IN_GRAD(0), valid after stage nlayers; EDSR: after
 *     the backward.
 * b outside 0 .. 1 (BODY_GRAD), g outside 0 .. log2(scale) - 1 (DPS): SRMI_ERR_ARG. */
#define SRMI_BUF_DPS 12
#define SRMI_BUF_DRESB 13
#define SRMI_BUF_BODY_GRAD 14
#define SRMI_BUF_HEAD_GRAD 15
int srmi_engine_buffer(srmi_engine* e, int which, int g, int b, void** ptr, size_t* elems, int* elem_bytes);

/* diagnostic (tests): trace of the RCAN backward's in-group state, which every RCAB of a
 * residual group rewrites in place.  With a buffer set (256-byte aligned, at least
 * srmi_engine_trace_size bytes, the caller's; NULL = off, the default), the backward
 * enqueues asynchronous device-to-device copies on its own stream, between its launches
 * (no kernel, no synchronisation; no launch, operand or order changes), into the slot
 * (which, g, b) at srmi_engine_trace_slot's byte offset:
 *   GRB    (b = 0): the bf16 copy of group g's output gradient at the start of its stage
 *          (the group tail's dgrad and filter-gradient operand);
 *   STREAM (b = 0 .. nblocks): the in-group gradient stream w.r.t. RCAB b's output, in the
 *          engine's operand type -- b = nblocks after the group tail's launch, b - 1 after
 *          RCAB b's conv1 backward (b = 0: the bf16 copy of the group input gradient);
 *   PACC   (b = 1 .. nblocks): fp32 [batch][nstrips][128], the CA sums (sum g | sum g u per
 *          strip) of RCAB b, copied at the same points as STREAM b;
 *   DZ     (b = 1 .. nblocks): after RCAB b's conv2 backward;
 *   DU     (b = 1 .. nblocks): copied only where the engine writes du to memory
 *          (srmi_engine_probe which = 4 returns 0).
 * Maps are [batch][lr_h][lr_w][64]; the first n images are copied.  Not while a staged
 * backward is half-way through (SRMI_ERR_ARG); RCAN train engines only. */
#define SRMI_TRACE_GRB 0
#define SRMI_TRACE_STREAM 1
#define SRMI_TRACE_PACC 2
#define SRMI_TRACE_DZ 3
#define SRMI_TRACE_DU 4
int srmi_engine_trace_size(srmi_engine* e, size_t* bytes);
int srmi_engine_trace(srmi_engine* e, void* buf, size_t bytes);
int srmi_engine_trace_slot(srmi_engine* e, int which, int g, int b, size_t* offset, size_t* elems, int* elem_bytes);

/* diagnostic (tests): trace of the bf16 RCAN forward's transient state, under the backward
 * trace's contract (the caller's 256-byte aligned buffer of at least srmi_engine_fwd_trace_size
 * bytes, NULL = off, the default; asynchronous device-to-device copies on the forward's stream,
 * between its launches; no launch, operand or order changes; one host branch per copy site when
 * off).  Slots (which, g, b), g = residual group, b = RCAB 1 .. nblocks:
 *   LO    the pair's lo8 remainder bytes [batch][lr_h][lr_w][64] after RCAB b (every RCAB
 *         rewrites them in place);
 *   PPOOL fp32 [batch][nstrips][64], the CA strip records after the launch that writes them:
 *         conv1 where the CA runs inside conv2 and in the one-launch inference RCAB (sums of
 *         the bf16 t), conv2 in the CA-pass forms (sums of its fp32 output);
 *   RF    (b = 0) the fp32 output of group g after its tail conv;
 * and, inference engines only (their hb / t / record slots rotate):
 *   HB    (b = 0 .. nblocks; and g = nlayers, b = 0) as SRMI_BUF_HB of a train engine;
 *   T     conv1's output of RCAB b;
 *   REC   fp32 [batch][160], the CA record m | z1 | s of RCAB b.
 * The first n images' share of each is copied.  bf16 RCAN engines, train or inference (the
 * exact-fp32 engine and EDSR: SRMI_ERR_ARG).  srmi.inference and the trainers never set it. */
#define SRMI_FTRACE_LO 0
#define SRMI_FTRACE_PPOOL 1
#define SRMI_FTRACE_RF 2
#define SRMI_FTRACE_HB 3
#define SRMI_FTRACE_T 4
#define SRMI_FTRACE_REC 5
int srmi_engine_fwd_trace_size(srmi_engine* e, size_t* bytes);
int srmi_engine_fwd_trace(srmi_engine* e, void* buf, size_t bytes);
int srmi_engine_fwd_trace_slot(srmi_engine* e, int which, int g, int b, size_t* offset, size_t* elems,
                               int* elem_bytes);

/* RMSE (l2loss, squared=False).  loss4[0] = sum of squares (this rank),
 * loss4[1] = global element count; after the optional all-reduce of loss4[0],
 * srmi_rmse_finalize sets loss4[3] = L = sqrt(S/count), loss4[2] = 1/(count L). */
int srmi_rmse_partial(srmi_engine* e, const float* pred, const float* target, size_t n, double count_global,
                      float* loss4, void* stream);
int srmi_rmse_finalize(float* loss4, void* stream);

/* Charbonnier loss (model.loss_fn 'charbonnier', ModelTrainer.charbonnier
 * sres/controller/dual_trainer.py:196-198): loss4[0] = sum sqrt(d^2 + eps) (this
 * rank), loss4[1] = count_global; dy (optional, like pred) = d / sqrt(d^2 + eps) /
 * count_global -- the upstream gradient srmi_backward takes.  Finalise with
 * srmi_loss_finalize(loss4, SRMI_LOSS_MEAN): loss4[3] = loss4[0] / loss4[1].
 * loss4 NULL (dy required): dy only, no loss sums (the trainer takes the loss from
 * srmi_tile_loss_parts). */
#define SRMI_LOSS_RMSE 0
#define SRMI_LOSS_MEAN 1
int srmi_charbonnier_partial(srmi_engine* e, const float* pred, const float* target, size_t n, double count_global,
                             float eps, float* loss4, float* dy, void* stream);
int srmi_loss_finalize(float* loss4, int kind, void* stream);
/* per-batch losses of process_image / evaluate (dual_trainer.py:417-446, :509-532):
 * pred/target [ntiles][tile_elems] scored in batches of batch_size tiles (the last
 * one may be short), loss of a batch over all its elements (kind RMSE or MEAN =
 * Charbonnier with eps); out[0] = mean of the batch losses, out[1 + b] = batch b's
 * loss (at most 1024 batches); work: ntiles floats */
int srmi_batch_losses(const float* pred, const float* target, int ntiles, long long tile_elems, int batch_size,
                      int kind, float eps, float* work, float* out, void* stream);
/* the second half of srmi_batch_losses on per-tile sums already formed (its `work`
 * output, e.g. gathered from the ranks of a multi-rank tiled inference, srmi.inference):
 * out[0] = mean of the batch losses, out[1 + b] = batch b's loss, the same arithmetic
 * (process_image's np.array(batch_losses).mean(), dual_trainer.py:443-446) */
int srmi_batch_loss_means(const float* sums, int ntiles, long long tile_elems, int batch_size, int kind, float* out,
                          void* stream);
/* loss sums that do not depend on how a batch is split over calls / micro-batch
 * engines: srmi_tile_loss_parts writes parts[ntiles][16] (per tile, 16 fixed slices,
 * fixed reduction order; kind RMSE: (p - t)^2, MEAN: sqrt((p - t)^2 + eps)) -- each
 * call writes its tiles' rows of one batch-wide array; srmi_loss_from_parts then sums
 * the ntiles x 16 parts in order (fp64) into loss4 ([0] = S, [1] = count_global) and
 * finalises it as `kind` (-1: not finalised, before a data-parallel all-reduce) */
int srmi_tile_loss_parts(const float* pred, const float* target, int ntiles, long long tile_elems, int kind,
                         float eps, float* parts, void* stream);
int srmi_loss_from_parts(const float* parts, int ntiles, double count_global, int kind, float* loss4, void* stream);
/* loss4 = the sum over nparts micro-batch records parts4[k][4] (S summed in a fixed
 * order, the count of part 0), then finalised as `kind` (-1: not finalised, e.g.
 * before a data-parallel all-reduce of loss4[0]) */
int srmi_loss_combine(float* loss4, const float* parts4, int nparts, int kind, void* stream);

/* interp baseline / data path */
int srmi_downsample(const float* hr, int N, int C, int H, int W, int scale, float* lr, void* stream);
int srmi_upsample(const float* lr, int N, int C, int h, int w, int scale, float* hr, void* stream);
/* torch.nn.functional.interpolate(x, scale_factor=f, mode) with align_corners=False,
 * any factor: the downsample / upsample of array.py:72-76 / :84-87 under
 * task.downsample_mode / upsample_mode (torch_interp_mode, array.py:37-41: 'linear'
 * -> SRMI_INTERP_BILINEAR, 'cubic' -> SRMI_INTERP_BICUBIC) and data_downsample's
 * factors (dual_trainer.py:561-563).  x NCHW [N][C][H][W] -> y [N][C][Ho][Wo] with
 * Ho = floor(H f), Wo = floor(W f) chosen by the caller and rh = rw = (float)(1 / f),
 * the source-coordinate scale ATen uses (UpSample.h area_pixel_compute_scale) */
#define SRMI_INTERP_BILINEAR 1
#define SRMI_INTERP_BICUBIC 2
int srmi_interpolate(const float* x, int N, int C, int H, int W, int Ho, int Wo, float rh, float rw, int mode, float* y,
                     void* stream);

/* Adam on flat buffers, step counted from 1 */
int srmi_adam_step(float* p, const float* g, float* m, float* v, size_t n, int step, float lr, float beta1,
                   float beta2, float eps, float weight_decay, void* stream);

/* ---- optimizer guards ("Optimizer guards") ----
 * The control record ctl[4] (fp32, device; the caller zeroes it once) joins the two:
 *   ctl[0]  the L2 norm of the flat gradient
 *   ctl[1]  the clip coefficient min(1, max_norm / (norm + 1e-6)): clip_grad_norm_'s
 *           formula, evaluated in fp64 and rounded; 0 when ctl[2] is 0
 *   ctl[2]  1.0 if ctl[0] is finite, else 0.0
 *   ctl[3]  the running count of calls that found it non-finite (a whole number held in
 *           fp32, as the masked loss counts are): read, incremented, written back
 * srmi_grad_norm: every square and every sum in fp64 (the product of two fp32 values is
 * exact there): one partial per block into the workspace (srmi_grad_norm_workspace bytes,
 * 8-byte aligned), added in index order by a second, single-workgroup launch.  No atomics;
 * the number of partials depends on n alone; the same g gives the same bits on every run.
 * A NaN or an infinity anywhere in g gives ctl[2] = 0.  max_norm = +inf: measure and
 * guard, never clip (ctl[1] is exactly 1).  max_norm <= 0 or NaN, n < 1, a missing
 * buffer or a workspace that is too small: SRMI_ERR_ARG, and nothing is launched. */
int srmi_grad_norm_workspace(size_t n, size_t* bytes);
int srmi_grad_norm(const float* g, size_t n, float max_norm, void* workspace, size_t ws_bytes, float* ctl,
                   void* stream);
/* srmi_adam_step on g' = fl(g * ctl[1]), the coefficient read from the device (the host
 * never sees it): the same kernel body, so ctl[1] = 1 and ema = NULL give srmi_adam_step's
 * bits.  ctl[2] == 0: the launch writes nothing, and p, m, v, ema stay bit for bit as they
 * were.  The caller still counts the step: the bias corrections of the next one are those
 * of step + 1, which keeps the host free of any read of ctl.  ema != NULL: the same pass
 * does ema += (1 - ema_decay) * (p_new - ema), ema_decay in [0, 1) (SRMI_ERR_ARG otherwise)
 * (torch.optim.swa_utils.get_ema_multi_avg_fn: ema.lerp_(p, 1 - decay)). */
int srmi_adam_step_guarded(float* p, const float* g, float* m, float* v, float* ema, size_t n, int step, float lr,
                           float beta1, float beta2, float eps, float weight_decay, float ema_decay, const float* ctl,
                           void* stream);

/* y += a * x (flat fp32; sums micro-batch gradients) */
int srmi_axpy(float* y, const float* x, float a, size_t n, void* stream);

/* ---- op-level entry points (kernel parity tests, custom graphs) ---------- */
/* dtype: SRMI_DTYPE_BF16 (x / yb / aux / packs bf16) or SRMI_DTYPE_F32 (fp32) */
/* forward conv: x NHWC [N][H][W][Cin], packed filters (srmi_pack_conv),
 * epi: 0 relu, 1 + channel sums (part[N][strips][64]), 2 alpha*(y+b)+r1
 * -> yf fp32 (opt) + yb, 3 PixelShuffle(2), 4 dgrad * (aux > 0), 5 dgrad + r1 + r2
 * + r3 -> yf (+ sums of g, g*aux), 6 plain (+ bias).  (The engine's own epilogues
 * 7-13 -- the CA forward, the bf16 in-group gradient stream -- take operands this
 * entry point does not pass; they are reached through srmi_forward / _backward.)  */
int srmi_conv3x3(const void* x, const void* wpack, const float* bias, int N, int H, int W, int Cin, int Cout,
                 int in_unshuffle, int epi, void* yb, float* yf, const float* r1, const float* r2, const float* r3,
                 const void* aux, float* part, float alpha, int dtype, void* stream);
int srmi_conv3x3_nstrips(int H, int W);
/* diagnostic: record s_memtime phase stamps of the Cin=64 conv kernel into buf
 * (64 x u64 per workgroup); NULL turns it off */
int srmi_debug_conv_stamps(void* buf);
int srmi_debug_wgrad_stamps(void* buf);
/* fp32 torch filter [Cout][Cin][3][3] -> packs of dtype: fwd [Cin/64][9][Cout][64],
 * dgrad [Cout/64][9][Cin][64] (flipped), bias [Cout]; ps != 0 permutes the
 * PixelShuffle channel order (packed c'' = 64q + c <- torch 4c + q)         */
int srmi_pack_conv(const float* w, const float* b, int Cout, int Cin, int ps, void* fpack, void* dpack, float* pbias,
                   int dtype, void* stream);
/* filter + bias gradient of a 3x3 conv (nn.Conv2d backward, weight half):
 * x NHWC [N][H][W][64], dy NHWC [N][H][W][Cout] (or, dy_unshuffle,
 * the PixelShuffle output [N][2H][2W][64] with Cout = 256); slab: workspace of
 * N*rs*Cout*577 floats; gw torch layout [Cout][64][3][3], gb [Cout] (both NULL:
 * leave the per-chunk partial slabs, skip the reduction) */
int srmi_wgrad3x3(const void* x, const void* dy, int N, int H, int W, int Cout, int dy_unshuffle, int row_splits,
                  float* slab, size_t slab_bytes, int ps, float alpha, float* gw, float* gb, int dtype, void* stream);
int srmi_ca_forward(const void* u, const float* part, int nstrips, const float* w1, const float* b1, const float* w2,
                    const float* b2, int N, int HW, int C, int R, const float* h_in, float* h_out, void* hb_out,
                    float* rec, int dtype, void* stream);
/* the same CALayer forward on the bf16 engine's residual-stream pair: h = h_in
 * (fp32, when non-NULL) or the pair hi_in (bf16) + lo_in (int8 remainder); out, for
 * the fp32 bit pattern A of h + s*u: hi = (A + 0x8000) >> 16 (bf16, rounded half away
 * from zero), lo = byte 1 of A; the pair's value has the bits ((hi << 16) | 0x80) +
 * (sext8(lo) << 8), i.e. h + s*u to within 128 fp32 steps (16 significant bits) (in
 * place allowed: lo_out == lo_in) */
int srmi_ca_forward_pair(const void* u, const float* part, int nstrips, const float* w1, const float* b1,
                         const float* w2, const float* b2, int N, int HW, int C, int R, const float* h_in,
                         const void* hi_in, const void* lo_in, void* hi_out, void* lo_out, float* rec, void* stream);
/* brec: N*(2C + C/R) floats (dz2 | dz1 | conv2 bias grad per image) followed by
 * N*C floats of dm (gradient of the pooled mean) -- N*(3C + C/R) in total */
int srmi_ca_backward(const float* g, const float* part, int nstrips, const float* rec, const float* w1,
                     const float* w2, int N, int HW, int C, int R, void* du, float* brec, int dtype, void* stream);
int srmi_head_forward(const float* lr, const float* w, const float* b, int N, int C, int H, int W, float* x0f,
                      void* x0b, int dtype, void* stream);
int srmi_tail_forward(const void* x, const float* w, const float* b, int N, int C, int H, int W, float* y, int dtype,
                      void* stream);

/* ---- tiled-region inference data path --------------------------------- */
/* region [C][H][W] fp32 -> floor grid gy = H/ty, gx = W/tx; tiles
 * [gy*gx][C][ty][tx] normalised per tile and channel ((x - mean) / std over the
 * tile, ddof 0); mean/std [gy*gx][C]; bad[gy*gx] (optional) = 1 where the tile
 * holds a non-finite value (the reference drops those tiles) */
int srmi_region_to_tiles(const float* region, int C, int H, int W, int ty, int tx, float* tiles, float* mean,
                         float* std, int* bad, void* stream);
/* tiles [n][C][ty][tx] -> out [C][gy*ty][gx*tx]: x * std + mean (mean == NULL:
 * no denorm); inv[gy*gx] = tile index of each grid cell or -1 (NaN cell);
 * inv == NULL: tile i is cell i */
int srmi_tiles_to_region(const float* tiles, const float* mean, const float* std, const int* inv, int C, int ty,
                         int tx, int gy, int gx, float* out, void* stream);

/* ---- overlapping tiles, blended mosaic (no reference counterpart) ------- */
/* The plan of one axis is three integers: length L, tile t, stride S, 1 <= S <= t
 * <= L.  It has n = ceil((L - t) / S) + 1 tiles, tile i at the origin min(i S, L - t):
 * the last tile is shifted inward, so the axis is covered completely (a pixel may lie
 * in three tiles of an axis even at S > t / 2).  srmi_overlap_count (host only)
 * returns n, or SRMI_ERR_ARG for a plan outside those bounds. */
int srmi_overlap_count(int L, int t, int S);
/* region [C][H][W] fp32 -> tiles [ny*nx][C][ty][tx] cut at the plan's origins (tile
 * iy * nx + ix) and normalised per tile and channel by `mode`, with the arithmetic of
 * srmi_region_to_tiles_norm: off / div / off_out / div_out are [ny*nx][C], bad[ny*nx]
 * (optional) = 1 where the tile holds a non-finite value.  With sy == ty, sx == tx on
 * a region the tile divides, the result is srmi_region_to_tiles_norm's bit for bit.
 * Any origin alignment (the float4 form is taken only where W, tx and sx are multiples
 * of 4 and the buffers 16-byte aligned).  ny*nx <= 65535 (SRMI_ERR_SHAPE); a plan or
 * mode out of range, or a missing buffer: SRMI_ERR_ARG. */
int srmi_region_to_tiles_overlap(const float* region, int C, int H, int W, int ty, int tx, int sy, int sx, int mode,
                                 const float* off, const float* div, float* tiles, float* off_out, float* div_out,
                                 int* bad, void* stream);
/* tiles [ny*nx][C][Ty][Tx] of the plan (Ho, Ty, Sy) x (Wo, Tx, Sx) -> out [C][Ho][Wo]:
 * out = sum_k w_k v_k / sum_k w_k over the tiles k covering the pixel with bad[k] == 0
 * (bad == NULL: all), v = x * div + off as srmi_tiles_to_region forms it (off == NULL:
 * no denorm), w = wy * wx with the integer ramp w(p) = min(p + 1, t - p, t - S + 1) at
 * tile-local position p.  One thread per pixel (or quad) gathers its tiles in ascending
 * (iy, ix) order: fp32 sums, one division, no atomics -- deterministic.  A bad tile
 * contributes nothing and is not read; a pixel with no tile left is NaN; a pixel with
 * exactly one is a copy of v, so at S == T on a divisible region the result is
 * srmi_tiles_to_region's bit for bit.  At S == T on a ragged region the shifted last
 * tile is averaged with its neighbour where the two overlap.  Ho <= 65535
 * (SRMI_ERR_SHAPE); a plan out of range or a missing buffer: SRMI_ERR_ARG. */
int srmi_tiles_blend(const float* tiles, const float* off, const float* div, const int* bad, int C, int Ty, int Tx,
                     int Sy, int Sx, int Ho, int Wo, float* out, void* stream);

/* ---- land-aware forms (no reference counterpart) ------------------------ */
/* srmi_region_to_tiles_overlap for regions with land: the same plan, tile order, modes
 * and off / div / off_out / div_out, plus min_wet >= 1 and nwet [ny*nx][C] (optional).
 * Per tile k and channel c, with "wet" = the finite pixels of the ty x tx plane:
 *   nwet[k][c] = number of wet pixels; bad[k] = 1 iff some channel of the tile has
 *   nwet < min_wet (an all-land tile is always bad); a bad tile's planes are 0.0f (it
 *   still rides through the forward, and the blend never reads it).
 *   Statistics over the wet pixels only.  LNORM: mean and 2-pass variance (ddof 0, / nwet)
 *   as fp64 fixed-order block reductions, off_out = (float)mean, div_out = (float)std,
 *   x' = (float)(((double)x - mean) * (1 / std)) -- deliberately NOT the fp32 two-pass
 *   of the unmasked LNORM cut (srmi_region_to_tiles), so LNORM results differ from it in
 *   the last bits even without land.  LSCALE (min, max over the wet pixels) and AFFINE:
 *   the arithmetic of srmi_region_to_tiles_norm; on a region with no non-finite value
 *   tiles, off_out, div_out and bad are srmi_region_to_tiles_overlap's bit for bit.
 *   Zero spread gives the IEEE result.
 *   Dry pixels are flood-filled in normalised space: pass j = 1, 2, ... gives every pixel
 *   not yet filled that has a filled 8-neighbour inside the tile the mean of those
 *   neighbours -- fp32 adds from 0.0f in the order (dy, dx) = (-1,-1) (-1,0) (-1,1) (0,-1)
 *   (0,1) (1,-1) (1,0) (1,1), then one fp32 multiply by fp32(1 / count).  Passes are
 *   simultaneous (a pass reads only what was filled before it); at most max(ty, tx) - 1.
 * One workgroup per (channel, tile); the plane lives in LDS with a 16-bit pass stamp per
 * pixel, 6 bytes a pixel: ty * tx <= 25600 (160 x 160), else SRMI_ERR_SHAPE, as for
 * ny*nx > 65535.  The trip count is decided on the device: no host read, capturable.
 * min_wet < 1, a plan or mode out of range, a missing buffer: SRMI_ERR_ARG. */
int srmi_region_to_tiles_overlap_masked(const float* region, int C, int H, int W, int ty, int tx, int sy, int sx,
                                        int mode, const float* off, const float* div, float* tiles, float* off_out,
                                        float* div_out, int* bad, int min_wet, int* nwet, void* stream);
/* srmi_tiles_blend that puts the land back: output pixel (c, Y, X) is the canonical NaN
 * where mask_src[c][Y / scale][X / scale] (mask_src [C][Ho / scale][Wo / scale], the LR
 * region itself) is not finite -- decided before any tile is read -- and exactly
 * srmi_tiles_blend's value elsewhere (the same kernel, a compile-time flag).  The quad
 * form additionally needs scale % 4 == 0.  mask_src NULL, scale < 1, or Ho, Wo not
 * multiples of scale: SRMI_ERR_ARG; otherwise as srmi_tiles_blend. */
int srmi_tiles_blend_masked(const float* tiles, const float* off, const float* div, const int* bad, int C, int Ty,
                            int Tx, int Sy, int Sx, int Ho, int Wo, const float* mask_src, int scale, float* out,
                            void* stream);
/* srmi_rmse_partial over the elements where pred and target are both finite: loss4[0] =
 * S = sum (p - t)^2, loss4[1] = their count, both written by the device (two stages,
 * fixed order, fp64 differences and partials, no atomics); srmi_rmse_finalize then works
 * unchanged.  count == 0 gives the IEEE result: loss4[3] = sqrt(0 / 0) = NaN.  The count
 * is stored as a float: exact up to 2^24 elements. */
int srmi_rmse_partial_masked(srmi_engine* e, const float* pred, const float* target, size_t n, float* loss4,
                             void* stream);

/* ---- geometric self-ensemble (no reference counterpart) ------------------ */
/* The "+" variant of the RCAN / EDSR papers: the model runs on dihedral variants of every
 * tile, the outputs are transformed back and averaged, and their standard deviation is a
 * per-pixel spread.  `variants` is a bit mask, 1 .. 255: bit f selects variant f of xyflip
 * (sres/base/source/batch.py:37-49 -- bit 0 of f flips x, bit 1 flips y, bit 2 then swaps
 * the axes), K = popcount(variants), and the selected variants are stored in ascending f. */
/* in [nplanes][h][w] fp32 -> out [K][nplanes][h][w]: variant f at output pixel (y, x) is
 * `in` at the source pixel srmi_batch_prep reads there (the same index map) -- in numpy
 * terms flip x if bit 0, flip y if bit 1, then swap the last two axes if bit 2.  A pure
 * permutation: every bit pattern is kept, NaN payloads and -0 included.  A 64 x 64 block
 * of a source plane is read once, row by row, into LDS (padded pitch) and written once
 * per variant, row by row: no lane walks a column of HBM.  The float4 form is taken where
 * w % 4 == 0 and both buffers are 16-byte aligned, a scalar one otherwise.  A variant
 * >= 4 with h != w, or nplanes, h, w < 1, or more than 2^31 - 1 blocks: SRMI_ERR_SHAPE;
 * `variants` outside 1 .. 255, a missing buffer, or in == out: SRMI_ERR_ARG. */
int srmi_tiles_dihedral(const float* in, long long nplanes, int h, int w, int variants, float* out, void* stream);
/* tiles [K][ny*nx][C][Ty][Tx]: slab j holds the model outputs of variant f_j of every
 * tile, still in the transformed frame; off / div / bad [ny*nx].. as for srmi_tiles_blend,
 * shared by the variants.  Per output pixel (c, Y, X) and slab j, B_j is
 * srmi_tiles_blend's value of the back-transformed slab (mask_src != NULL:
 * srmi_tiles_blend_masked's, with `scale`; mask_src == NULL: scale is ignored), bit for
 * bit: the same plan, cover, integer ramp, ascending (iy, ix) order, bad tiles skipped
 * before any read, no cover -> canonical NaN, one cover -> a copy, one division.  The
 * back-transformed slab is never materialised: for covering tile k and tile-local
 * (qy, qx) the kernel reads slab j at (y, x) with a = (f & 2) ? Ty - 1 - qy : qy,
 * b = (f & 1) ? Tx - 1 - qx : qx, (y, x) = (f & 4) ? (b, a) : (a, b).  Then, in fp32 and
 * ascending j,
 *   mean   [C][Ho][Wo] = (B_0 + ... + B_{K-1}) / (float)K
 *   spread [C][Ho][Wo] = sqrtf(((B_0 - mean)^2 + ...) / (float)K)      (ddof 0; optional)
 * Both sums add their terms pairwise in ascending j -- ((t0 + t1) + (t2 + t3)) + ((t4 + t5)
 * + (t6 + t7)), the terms j >= K left out -- so K = 1, 2, 4 or 8 identical variants give
 * mean == B_0 bit for bit and spread == +0 (a running sum rounds at 3 B, 5 B, 7 B).
 * NaN propagates into both.  No atomics, deterministic.  A workgroup owns 16 rows x 64
 * pixels of the output (quad form; 16 x 16 in the scalar form), so a wave's loads cover
 * whole 64-byte segments of a slab whether or not its axes are swapped.  `variants`
 * outside 1 .. 255: SRMI_ERR_ARG; a variant >= 4 with Ty != Tx: SRMI_ERR_SHAPE; otherwise
 * the errors of srmi_tiles_blend (mask_src given: of srmi_tiles_blend_masked). */
int srmi_tiles_blend_ensemble(const float* tiles, int variants, const float* off, const float* div, const int* bad,
                              int C, int Ty, int Tx, int Sy, int Sx, int Ho, int Wo, const float* mask_src, int scale,
                              float* mean, float* spread, void* stream);

/* ---- land in training (no reference counterpart: the reference drops every tile that
 * touches land, and its losses know no mask) ------------------------------------ */
/* srmi_tiles_nonfinite with a threshold, on the same floor grid (ncells = (H/ty) (W/tx)):
 * nwet[c*ncells + t] (optional) = the finite pixels of tile t of channel c;
 * bad[c*ncells + t] = 1 iff SOME channel of tile t has nwet < min_wet -- the same flag in
 * every channel's row, so srmi_tiles_keep / srmi_tiles_gather_dev take it unchanged and
 * the keep list stays channel-aligned.  Every flag and count is stored (no memset
 * needed), no atomics.  With min_wet = ty * tx and channels that share a mask it equals
 * srmi_tiles_nonfinite.  min_wet < 1: SRMI_ERR_ARG. */
int srmi_tiles_dry(const float* region, int C, int H, int W, int ty, int tx, int min_wet, int* bad, int* nwet,
                   void* stream);
/* The flood fill of srmi_region_to_tiles_overlap_masked (the same device function: add
 * order, fp32(1 / count), simultaneous passes), in place on tiles [nplanes][h][w]: every
 * non-finite pixel of a plane is filled from the finite ones.  A plane without a
 * non-finite pixel is not written; a plane without a finite pixel becomes 0.0f.  passes
 * [nplanes] (optional) = the pass count, 0 for the former, -1 for the latter.  Any
 * nplanes; h * w <= 25600 (the plane and its stamps in LDS), else SRMI_ERR_SHAPE.  The
 * trip count is decided on the device: no host read, capturable. */
int srmi_tiles_fill(float* tiles, long long nplanes, int h, int w, int* passes, void* stream);
/* srmi_batch_prep_norm for tiles with land (non-finite = dry).  The statistics run over
 * the wet pixels with the arithmetic of the masked cut: LNORM fp64 mean and 2-pass
 * variance / nwet, x' = (float)(((double)x - mean) * (1 / std)), off_out = mean, div_out =
 * std; LSCALE (min, max over the wet pixels) and AFFINE as srmi_batch_prep_norm, whose
 * hr, lr, off_out and div_out they give bit for bit when no input is non-finite.  hr =
 * the normalised, xy-flipped tile with the canonical NaN at the dry pixels; lr (optional)
 * = srmi_downsample's arithmetic on that tile (an LR pixel is non-finite iff one of its
 * 4 x 4 taps is dry) and then srmi_tiles_fill, a second launch; nwet [B][C] (optional) = the
 * wet pixels.  A plane without a wet pixel: hr all NaN, lr all 0.0f, IEEE statistics.
 * Errors as srmi_batch_prep_norm (every mode takes any B with B * C < 2^31 and needs
 * 16-byte aligned raw and hr); (T / scale)^2 > 25600 with lr: SRMI_ERR_SHAPE. */
int srmi_batch_prep_masked(const float* raw, long long B, int C, int T, int flip_index, int scale, int mode,
                           const float* off, const float* div, float* hr, float* lr, float* off_out, float* div_out,
                           int* nwet, void* stream);
/* srmi_tile_loss_parts over the elements where pred and target are both finite: the same
 * slices, reduction tree and parts[ntiles][16], plus cparts[ntiles][16] = the number of
 * such elements per slice as floats (exact: a slice holds tile_elems / 16 elements).  On
 * all-finite inputs parts is srmi_tile_loss_parts' bit for bit. */
int srmi_tile_loss_parts_masked(const float* pred, const float* target, int ntiles, long long tile_elems, int kind,
                                float eps, float* parts, float* cparts, void* stream);
/* srmi_loss_from_parts with the count read from the device: loss4[1] = the sum of the
 * ntiles x 16 cparts (fp64; whole numbers, exact).  kind -1: not finalised.  On
 * all-finite inputs loss4 is srmi_loss_from_parts' with the host count, bit for bit; a
 * count of 0 gives the IEEE result, as srmi_rmse_partial_masked. */
int srmi_loss_from_parts_masked(const float* parts, const float* cparts, int ntiles, int kind, float* loss4,
                                void* stream);
/* The upstream gradient srmi_backward takes as dy, from a finalised loss4, +0.0f where
 * pred or target is not finite.  RMSE: (p - t) * loss4[2] in fp32 -- exactly what the tail
 * kernels form on the fly from sr / hr / loss4.  MEAN (Charbonnier): d / sqrt(d^2 + eps) *
 * (float)(1 / loss4[1]), srmi_charbonnier_partial's dy. */
int srmi_loss_dy_masked(const float* pred, const float* target, size_t n, int kind, float eps, const float* loss4,
                        float* dy, void* stream);

/* ---- the spectral score (no reference counterpart) ---------------------- */
/* Windowed (Welch) isotropic wavenumber spectra of a (prediction) and b (truth), both
 * [C][H][W] fp32 on the device, possibly with NaN / Inf.
 *   Windows: side P, a power of two in 16 .. 256 with P <= min(H, W); stride Q in 1 .. P on
 *   both axes; origins min(i Q, L - P), i < srmi_overlap_count(L, P, Q), row-major.  A
 *   window is skipped, for all channels, when any of its pixels is non-finite in a or in b
 *   in any channel; nused = the windows not skipped.
 *   Per used window and channel, for a and for b: subtract the window's mean (fp64 sum,
 *   fp64 subtraction, rounded to fp32), multiply by the periodic Hann taper h(y) h(x),
 *   h(p) = 0.5 - 0.5 cos(2 pi p / P), take the 2-D DFT Fa, Fb.  With W2 = sum (h(y) h(x))^2
 *   the densities per bin are Eaa = |Fa|^2, Ebb = |Fb|^2, Eee = |Fa - Fb|^2 and
 *   Cab = Re(Fa conj Fb), each / (P^2 W2): summed over ALL bins a density is the mean square
 *   of the detrended, tapered window / mean((h h)^2) (Parseval).
 *   Shells: signed wavenumbers ky, kx in [-P/2, P/2), shell j = floor(sqrt(ky^2 + kx^2) +
 *   0.5); shells 0 .. P/2 are kept (K = P/2 + 1), the corner bins beyond are dropped.
 * out [C][4][K] fp32 = the shell sums of Eaa, Ebb, Eee, Cab averaged over the used windows
 * (nused == 0: NaN everywhere), nused one int32; both written by the device.  One complex
 * fp32 FFT per window and channel serves both fields; shell sums and the average over
 * windows are fp64 in a fixed order, no atomics: bit-identical from run to run.
 * srmi_spectra_workspace (host only) gives the bytes of `workspace` (16-byte aligned; it
 * need not be initialised): the skip flags, the [windows][C][4][K] fp64 partial sums and,
 * for P >= 128, one P x P complex plane per launched workgroup (at most 512, whatever the
 * window count).  No host synchronisation, no allocation: capturable.  P not a power of
 * two or outside 16 .. 256 or > min(H, W), Q outside 1 .. P, C < 1, a missing buffer or a
 * workspace that is too small: SRMI_ERR_ARG, and nothing is launched. */
int srmi_spectra_workspace(int C, int H, int W, int P, int Q, size_t* bytes);
int srmi_spectra(const float* a, const float* b, int C, int H, int W, int P, int Q, void* workspace,
                 size_t workspace_bytes, float* out, int* nused, void* stream);

/* ---- the SSIM score (no reference counterpart) -------------------------- */
/* Structural similarity (Wang, Bovik, Sheikh, Simoncelli 2004, Gaussian form: scikit-image's
 * structural_similarity(gaussian_weights=True, use_sample_covariance=False)) of a
 * (prediction) against b (truth), both [C][H][W] fp32 on the device, possibly with NaN / Inf,
 * per channel; tests/ssim_oracle.py restates it in numpy.
 *   Window: 11 taps g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), normalised to sum 1 in fp64 and then
 *   rounded to fp32; G = g (x) g.  Only VALID positions are evaluated, 5 <= y < H - 5 and
 *   5 <= x < W - 5: there is no padding.
 *   Mask: a position is USED, for that channel, iff all 121 pixels of its window are finite
 *   in a and in b in that channel.  The decision is per channel (srmi_spectra skips a window
 *   for all channels; this score does not).  One NaN removes exactly the 121 positions whose
 *   window holds it.
 *   Range and pivot: lo, hi = the min and max of b's finite pixels in the channel; L = hi - lo
 *   (fp32), or data_range for every channel where data_range > 0; the pivot r = 0.5 lo +
 *   0.5 hi (fp32) is always b's.  All moments are formed on a - r and b - r (fp32): variances
 *   and the covariance do not change with the shift and the means get r added back.  The
 *   pivot is part of the definition: ocean fields sit at 290 +- 1.5, where E[x^2] - mu^2
 *   without it loses the variance in fp32.  min and max do not depend on the order of the
 *   reduction, so r and L are exact and reproducible.
 *   Quantities: mu_a = G * a, mu_b = G * b, s_aa = G * a^2 - mu_a^2, s_bb likewise, s_ab =
 *   G * (a b) - mu_a mu_b; C1 = (0.01 L)^2, C2 = (0.03 L)^2;
 *   cs = (2 s_ab + C2) / (s_aa + s_bb + C2), ssim = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1)
 *   * cs, in fp32: the horizontal pass, then the vertical one, taps in ascending order.
 * out [C][4] fp32 = {the mean of ssim over the used positions, the mean of cs over them,
 * mse = the mean of (a - b)^2 over the pixels finite in both (every pixel of the plane, the
 * border included; the difference and its square in fp64), L}; count [C][2] int64 = {nwin,
 * the used positions; npix, the pixels of mse}.  The sums are fp64 per workgroup and over
 * the workgroups, in a fixed order, no atomics: bit-identical from run to run, exact counts
 * at 4096^2 and beyond.  nwin == 0 or npix == 0 gives the IEEE 0 / 0 = NaN; a channel of b
 * without a finite pixel has L = NaN.
 * map, when not NULL, [C][H][W] fp32: ssim at the used positions and the canonical NaN
 * (0x7fc00000) everywhere else -- the 5-pixel border and the positions not used.  Every
 * element is written.  out and count do not depend on whether map is given.
 * Any C in 1 .. 65535 and H, W >= 11 with H W < 2^31; no alignment requirement on a, b or
 * map.  srmi_ssim_workspace (host only) gives the bytes of `workspace` (16-byte aligned; it
 * need not be initialised): five partial sums per 24 x 64 rectangle of every plane and the
 * min / max pairs.  Three launches on `stream`; no host synchronisation, no allocation:
 * capturable.  data_range NaN or +-Inf (<= 0 means "from the truth"), a missing a, b,
 * workspace, out or count, a workspace that is too small, H or W below 11, C below 1:
 * SRMI_ERR_ARG, and nothing is launched. */
int srmi_ssim_workspace(int C, int H, int W, size_t* bytes);
int srmi_ssim(const float* a, const float* b, int C, int H, int W, float data_range, void* workspace,
              size_t workspace_bytes, float* out, long long* count, float* map, void* stream);

/* ---- the distribution score (no reference counterpart) ------------------- */
/* Does the prediction a have the truth b's distribution of values?  Both [C][H][W] fp32 on
 * the device, possibly with NaN / Inf, per channel; tests/distribution_oracle.py restates it
 * in numpy.  B = nbins in 2 .. 4096, J = njoint in 0 .. 64 (0: no joint histogram).
 *   Used pixel: finite in a and in b.  N is their count.
 *   Range: lo, hi = the min and max of b over the used pixels (exact: they do not depend on
 *   the order of the reduction), or lo_hi[0], lo_hi[1] where lo_hi (a HOST pointer to two
 *   floats, finite, hi > lo) is given.  scale = hi > lo ? fp32(B) / (hi - lo) : 0, the
 *   subtraction and the division each rounded once, correctly, in fp32.
 *   Bin of a value x, an index into B + 2 entries: 0 (under) if x < lo; B + 1 (over) if
 *   x > hi; B if x == hi (what the formula gives whenever hi > lo, and the bin of every used
 *   pixel of b when hi == lo); otherwise 1 + min((int)t, B - 1) with t = (x - lo) * scale in
 *   fp32 -- one subtraction, one multiplication, truncation.  The comparisons decide under and
 *   over before any conversion and the converted value is clamped as an integer, so no input
 *   indexes outside the table.  With the range b's own, b has no under and no over.
 *   Joint bin: ja, jb = the same formula with J in place of B (its own scale fp32(J) / (hi -
 *   lo)), minus 1, clamped into 0 .. J - 1: a prediction outside the range goes to the edge
 *   bin.  The count goes to joint[c][ja][jb].
 * hist [C][2][B + 2] int64 (0: a, 1: b), joint [C][J][J] int64 (may be NULL when J == 0), range
 * [C][2] fp32 = {lo, hi} (NaN, NaN for a channel without a used pixel), count [C] int64 = N,
 * derived [C][4 + 2 nprobs] fp64 = {pss, w1, under, over, q_a[nprobs], q_b[nprobs]}, formed by
 * the last launch from the int64 tables alone, with w = (hi - lo) / B in fp64:
 *   pss = sum_k min(ha[k], hb[k]) / N (Perkins et al. 2007), the sum an integer;
 *   w1 = w * sum_k |cumA[k] - cumB[k]| / N over the B + 2 entries, the sum an integer: the
 *   Wasserstein-1 distance of the two histograms with under and over taken as bins of one
 *   width beside the range -- a LOWER bound on the fields' distance when a leaves the range;
 *   under = ha[0] / N, over = ha[B + 1] / N;
 *   the quantile at probs[i] (HOST array, nprobs in 0 .. 16, each strictly inside (0, 1);
 *   passed to the kernel by value): r = p N in fp64, k the smallest entry with cum[k] >= r,
 *   value = left(k) + w (r - cum[k - 1]) / h[k], left(k) = lo + (k - 1) w, so that under
 *   spans [lo - w, lo] and over [hi, hi + w].
 *   N == 0: every entry of derived is NaN.
 * Every count is an integer sum, so the result is exact and bit-identical from run to run.
 * Launches on `stream`: range partials (skipped when lo_hi is given), histogram partials
 * (LDS integer atomics, one int32 table per workgroup, plain stores), finish (the tables in
 * workgroup order, then the derived values).  No global atomics, no host synchronisation, no allocation: capturable.
 * srmi_distribution_workspace (host only) gives the bytes of `workspace` (16-byte aligned; it
 * need not be initialised).  No alignment requirement on a or b; H, W >= 1 with H W <= 2^31
 * - 1.  flags: 0, or SRMI_DISTRIBUTION_* bits that select the measured alternatives of the
 * histogram kernel (DESIGN.md "Distribution score"); the result does not depend on them.
 * A missing a, b, workspace, hist, range, count or derived (joint with J > 0, probs with
 * nprobs > 0), a workspace that is too small or not aligned, B, J, nprobs or a probability out
 * of range (NaN included), a lo_hi that is not finite with hi > lo, unknown flags, C < 1, H or
 * W < 1 or H W > 2^31 - 1: SRMI_ERR_ARG, and nothing is launched. */
#define SRMI_DISTRIBUTION_MERGE_RUNS 1   /* a lane adds a run of equal bins among its 8 pixels once */
#define SRMI_DISTRIBUTION_ONE_COPY 2     /* one copy of the tables per workgroup */
#define SRMI_DISTRIBUTION_COPY_BY_WAVE 4 /* the copy chosen by the wave, not by the lane */
int srmi_distribution_workspace(int C, int H, int W, int nbins, int njoint, size_t* bytes);
int srmi_distribution(const float* a, const float* b, int C, int H, int W, int nbins, int njoint, const float* lo_hi,
                      const double* probs, int nprobs, void* workspace, size_t workspace_bytes, long long* hist,
                      long long* joint, float* range, long long* count, double* derived, int flags, void* stream);

/* ---- the gradient score (no reference counterpart) ----------------------- */
/* Are the prediction's fronts as sharp as the truth's, in the right place and pointing the
 * right way?  pred and truth [C][H][W] fp32 on the device, possibly with NaN / Inf, per
 * channel; tests/gradient_oracle.py restates it in numpy.
 *   Operator: the Sobel derivative at unit scale on a plane f[H][W], differences before sums
 *   (a field at 290 +- 1.5 loses nothing in fp32):
 *     dX(y, x) = f(y, x+1) - f(y, x-1)            dY(y, x) = f(y+1, x) - f(y-1, x)
 *     Gx(y, x) = ((dX(y-1, x) + dX(y+1, x)) + 2 dX(y, x)) / 8
 *     Gy(y, x) = ((dY(y, x-1) + dY(y, x+1)) + 2 dY(y, x)) / 8
 *   at the VALID positions only, 1 <= y <= H - 2 and 1 <= x <= W - 2: Hv Wv = (H - 2)(W - 2).
 *   A position is USED iff the nine pixels of its window are finite in pred and in truth of
 *   that plane: NaN and Inf are the mask, a coast costs a one-pixel rim, windows never cross
 *   planes.  There is one operator and no option for another.
 *   gx = Gx inv_dx, gy = Gy inv_dy (inv_dy, inv_dx: the reciprocals of the grid spacing, fp32,
 *   finite and > 0), |g|^2 = gx gx + gy gy and |g| = sqrt(|g|^2), every operation rounded once
 *   in fp32, none contracted.
 * Per channel over the used positions, in fp64 from those fp32 values, in a fixed order
 * (positions within a workgroup's 16 x 64 rectangle by a fixed tree, rectangles in 256
 * contiguous shares and a fixed tree), without atomics: count [C] int64 = n and
 *   sums [C][7] = {sum |g_p|, sum |g_t|, sum (|g_p| - |g_t|)^2, sum |g_p - g_t|^2 (the vector
 *   difference), sum g_p . g_t, sum |g_p|^2, sum |g_t|^2};
 *   stats [C][6] = {mean_pred = sums[0] / n, mean_truth = sums[1] / n, sharpness = mean_pred /
 *   mean_truth (below 1: too smooth), rmse_mag = sqrt(sums[2] / n), rmse_vec = sqrt(sums[3] /
 *   n), cosine = sums[4] / sqrt(sums[5] sums[6])}, formed on the device.
 *   n == 0: count 0 and NaN in every entry of sums and stats.
 * gmag_pred, gmag_truth [C][H][W] fp32, each optional (NULL): |g_p| and |g_t| at the used
 * positions, NaN at every other pixel, the one-pixel border included.
 * srmi_gradient_workspace (host only) gives the bytes of `workspace` (16-byte aligned; it need
 * not be initialised).  Two launches on `stream`, no global atomics, no host synchronisation,
 * no allocation: capturable, and bit-identical from run to run.  Rows are loaded and the maps
 * stored 16 bytes at a time when W % 4 == 0 and every buffer is 16-byte aligned, one float at
 * a time otherwise: the same bits.  H or W < 3, H W >= 2^31, C < 1, a factor that is not
 * finite or not positive, a missing pred, truth, workspace, count, sums or stats, a workspace
 * that is too small or misaligned: SRMI_ERR_ARG, nothing launched and no output touched. */
int srmi_gradient_workspace(int C, int H, int W, size_t* bytes);
int srmi_gradient(const float* pred, const float* truth, int C, int H, int W, float inv_dy, float inv_dx,
                  void* workspace, size_t workspace_bytes, long long* count, double* sums, double* stats,
                  float* gmag_pred, float* gmag_truth, void* stream);

/* ---- the fractions skill score (no reference counterpart) ---------------- */
/* Is a feature of the truth there in the prediction, nearly in the right place, and how near?
 * The fractions skill score (FSS, Roberts & Lean 2008) of the event "the value is at or above
 * a threshold", for a ladder of neighbourhood sizes; tests/fss_oracle.py restates it in numpy.
 *   Inputs: pred, truth [C][H][W] fp32 on the device, NaN / Inf allowed; thresholds [C][T] fp32
 *   ON THE DEVICE (so that a device-side quantile can fill them without a host read), T in 1 ..
 *   8; scales, a HOST array of N neighbourhood sizes n, N in 1 .. 16, each n odd, in 1 .. 255,
 *   strictly increasing (passed to the kernels by value).
 *   Per channel c.  Used pixel: finite in pred and in truth; used[c] is their count.  Event:
 *   Ip(y, x) = used && pred >= thr[c][t], It(y, x) = used && truth >= thr[c][t], one fp32
 *   comparison, so a NaN threshold gives no event; events[c][t] = {sum Ip, sum It}.
 *   Window counts, h = (n - 1) / 2: Sp(y, x) = the sum of Ip over rows y - h .. y + h and columns
 *   x - h .. x + h clipped to the plane -- what lies outside the plane or is not used is "no
 *   event" in both fields (scipy.ndimage.uniform_filter(I, n, mode="constant") n^2, and pysteps'
 *   convention for missing values); St the same of It.  Windows never cross planes.
 *   Sums over ALL H W positions of the plane, int64: num[c][t][k] = sum (Sp - St)^2,
 *   den[c][t][k] = sum (Sp^2 + St^2).  The n^4 of the fractions cancels: only integers are
 *   summed, so every table is exact and the same bits from run to run.
 *   derived [C][T][N + 6] fp64 = {fss[N], f_pred, f_truth, bias, target, afss, skilful}, formed
 *   on the device from the integer tables alone: fss[k] = 1 - num / den (NaN when den == 0);
 *   f_pred = ep / used, f_truth = et / used, bias = ep / et (IEEE: Inf or NaN when et == 0);
 *   target = 0.5 + f_truth / 2, the "uniform" FSS and the usual bar for a skilful scale; afss =
 *   2 ep et / (ep^2 + et^2), what fss tends to when the window covers the plane; skilful = the
 *   smallest n of scales with fss >= target as a double, NaN when there is none.  A channel
 *   without a used pixel has NaN in every derived entry and 0 in every table.
 * Outputs on the device: num, den [C][T][N], events [C][T][2], used [C] int64; derived as above.
 * Three launches on `stream`: events (one read of the fields; per 64-pixel row segment and
 * threshold the wave's 64-bit ballot is the packed word of a bit plane in the workspace, bits
 * past W zero; used and events from popcounts, as workgroup partials), windows (the grid covers
 * channel x threshold x scale x tile, a tile 512 rows of one 64-pixel word column; the count of
 * a row's events in columns x - h .. x + h is a popcount of at most five masked words and the
 * window count slides down the rows, so the work per position does not depend on n; 64-bit
 * accumulators), finish (the partials in plain sums, the tables and the derived values).  No
 * global atomics, no host synchronisation, no allocation: capturable.
 * srmi_fss_workspace (host only) gives the bytes of `workspace` (16-byte aligned; it need not
 * be initialised): the 2 C T bit planes (rows padded by two words either side, which are never
 * written and never counted), 17 uint32 per workgroup of the events launch, and two
 * int64 per (channel, threshold, scale, tile).  pred, truth and thresholds have no alignment
 * requirement.  A missing pointer, T or N or an n out of range, even or not increasing, a
 * workspace that is too small or misaligned, C < 1, H or W < 1, H W > 2^31 - 1, or H W n_max^4 >
 * 2^62 (the sums would leave int64; a 4096^2 plane at n = 255 is far inside): SRMI_ERR_ARG,
 * nothing launched and no output touched.  launches: 0 for all three, or SRMI_FSS_* bits for
 * some of them alone, in their order (for timing a launch by itself: a later launch reads what
 * the earlier ones of a previous call left in the workspace); unknown bits: SRMI_ERR_ARG.
 * Even n, thresholds on anomalies and a loss term are out of scope. */
#define SRMI_FSS_EVENTS 1
#define SRMI_FSS_WINDOWS 2
#define SRMI_FSS_FINISH 4
int srmi_fss_workspace(int C, int H, int W, int T, int N, size_t* bytes);
int srmi_fss(const float* pred, const float* truth, int C, int H, int W, const float* thresholds, int T,
             const int* scales, int N, void* workspace, size_t workspace_bytes, long long* num, long long* den,
             long long* events, long long* used, double* derived, int launches, void* stream);

/* ---- the ensemble score (no reference counterpart) ---------------------- */
/* Does an ensemble's spread say where to trust its mean?  K fields against a truth: the CRPS of
 * the empirical distribution (plain and fair, Ferro 2014), the rank (Talagrand) histogram, the
 * spread-skill ratio (Fortin et al. 2014) with a reliability table binned by the spread, the
 * Pearson correlation of spread and |error|, and a per-pixel CRPS map;
 * tests/ensemble_score_oracle.py restates it in numpy.  The K = 1 case of
 * srmi_tiles_blend_ensemble (one slab, its single-bit mask, spread == NULL) returns B_j bit for
 * bit (mean = B_j / 1.0f), which is how the members of a self-ensemble are materialised.
 *   Inputs: members [K][C][H][W] fp32, 2 <= K <= 8, and truth [C][H][W] fp32 on the device, NaN /
 *   Inf allowed; edges [C][B - 1] fp32 ON THE DEVICE (so that a device-side quantile can fill
 *   them without a host read): the interior edges of B spread bins, 1 <= B <= 16; with B == 1 the
 *   pointer is not read and may be NULL.
 *   Per channel c.  Used pixel: the truth and all K members are finite there.  Per used pixel,
 *   with m_j the members and y the truth converted to fp64 (exact), every operation below one
 *   IEEE fp64 operation rounded to nearest, never fused, so numpy's float64 elementwise
 *   operations give the same bits; tree(t) = ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7))
 *   with the terms j >= K left out, as srmi_tiles_blend_ensemble adds:
 *     a     = tree(|m_j - y|)
 *     b     = the running sum, from 0, of |m_j - m_l| over j < l in lexicographic (j, l)
 *     crps  = a / K - b / (K K)                 crps_fair = a / K - b / (K (K - 1))
 *     mean  = tree(m_j) / K                     var = tree((m_j - mean) (m_j - mean)) / K
 *     e     = mean - y                          s   = sqrt(var)
 *     rank  = the number of j with m_j < y and tied = any m_j == y, by fp32 comparisons
 *     bin   = the number of i < B - 1 with (float)s >= edges[c][i]   (a NaN edge never counts;
 *             edges that ascend make this the bin of s, but nothing requires them to)
 *   counts [C][K + 3 + B] int64 = {used, rank_hist[K + 1], tied, bin_count[B]}: exact.
 *   sums [C][9 + 2 B] fp64 = the sums over the used pixels of {crps, crps_fair, a, b, var, e e,
 *   |e|, s, s |e|}, then per bin {var, e e}.  The order of the additions is fixed (a lane's
 *   pixels ascending, a fixed tree over the lanes of a workgroup, then in the finish launch a
 *   lane's workgroups ascending and a fixed tree over the lanes of a wave): the same bits on every run.  All terms
 *   are >= 0, so a sum of T terms is within T 2^-53 of the exact one, relatively.
 *   derived [C][9 + 2 B] fp64, written by one thread of the finish launch from counts and sums
 *   alone, each operation rounded once, in this order: n = (double)used, f = (double)(K + 1) /
 *   (double)(K - 1), mse = S_ee / n, mvar = S_var / n, rmse = sqrt(mse); then
 *     [0] crps = S_crps / n                     [1] crps_fair = S_fair / n
 *     [2] rmse_mean = rmse                      [3] spread_rms = sqrt(mvar)
 *     [4] ssr = sqrt(f mvar) / rmse     (Fortin et al. 2014 with the ddof-1 variance: 1 when the
 *         truth is exchangeable with the members)
 *     [5] spread_error_corr = cov / sqrt(vs va) with ms = S_s / n, ma = S_|e| / n, cov = S_s|e| / n
 *         - ms ma, vs = mvar - ms ms, va = mse - ma ma  (the IEEE result: NaN for 0 / 0 or a
 *         negative product)
 *     [6] outliers = (double)(h_0 + h_K) / n    [7] its expectation 2.0 / (double)(K + 1)
 *     [8] reliability_index = the running sum, from 0 in ascending r, of |(double)h_r / n - u|, u =
 *         1.0 / (double)(K + 1)
 *     [9 + b] bin_spread = sqrt(f (S_var,b / n_b))     [9 + B + b] bin_rmse = sqrt(S_ee,b / n_b)
 *         (an empty bin: NaN in both)
 *   A channel without a used pixel has NaN in every derived entry and 0 in every table and sum.
 *   crps_map [C][H][W] fp32 (optional, NULL: not written) = (float)crps, the canonical NaN
 *   0x7fc00000 where the pixel is not used.
 * Two launches on `stream`: main (one read of the K + 1 fields, (K + 1) C H W 4 bytes, plus C H W 4
 * with the map; a workgroup owns 4096 consecutive pixels of a plane and a lane four consecutive
 * ones per step, loaded and stored as 16 bytes where the channel's K + 1 (+ 1) planes all start
 * on 16-byte boundaries, one by one otherwise and in a ragged last quad -- the same values and
 * order either way) and finish.  No global atomics, no host synchronisation, no allocation:
 * capturable.  srmi_ensemble_score_workspace (host only) gives the bytes of `workspace` (16-byte
 * aligned; it need not be initialised): per channel and workgroup of the main launch, ceil(H W /
 * 4096) of them, 9 + 2 B doubles and K + 3 + B uint32.  members, truth, edges and crps_map have no
 * alignment requirement.  K, B, C, H or W out of range, a missing members, truth, edges (B > 1),
 * workspace, counts, sums or derived, a workspace that is too small or misaligned, unknown
 * `launches` bits: SRMI_ERR_ARG; H W > 2^31 - 1: SRMI_ERR_SHAPE; nothing launched and no output
 * touched.  launches: 0 for both, or SRMI_ENSEMBLE_SCORE_* bits for one alone (for timing a launch
 * by itself: finish reads what the main launch of a previous call left in the workspace).
 * K > 8, randomised tie-breaking of ranks and a loss term are out of scope. */
#define SRMI_ENSEMBLE_SCORE_MAIN 1
#define SRMI_ENSEMBLE_SCORE_FINISH 2
int srmi_ensemble_score_workspace(int K, int C, int H, int W, int B, size_t* bytes);
int srmi_ensemble_score(const float* members, const float* truth, int K, int C, int H, int W, const float* edges,
                        int B, void* workspace, size_t workspace_bytes, long long* counts, double* sums,
                        double* derived, float* crps_map, int launches, void* stream);

/* ---- quantile mapping (no reference counterpart) ------------------------- */
/* Empirical quantile mapping: a monotone transfer function T = F_truth^-1 o F_src, calibrated
 * on fields whose truth is known and applied to later ones, so that the mapped output has the
 * truth's distribution of values (or of detail, value minus an interpolated base).
 * tests/quantile_map_oracle.py restates the three entry points in numpy.  Shared conventions:
 * B = nbins in 2 .. 4096, M = B + 2 entries {under, B bins, over}, C in 1 .. 16; `range` is a
 * HOST array [C][2] of finite fp32 {lo, hi} with hi > lo and hi - lo finite in fp32, one pair per
 * channel (the fixed range is what lets the tables of many fields add); H, W >= 1 with H W <= 2^31 - 1.  An argument
 * outside this: SRMI_ERR_ARG, nothing is launched and every output is left as it was.  No
 * global atomics, no host synchronisation, no allocation: all three are capturable.  No
 * reference counterpart.
 *
 * srmi_quantile_map_accumulate: src, truth, base [C][H][W] fp32 on the device, base may be
 * NULL.  The binned values are src - base and truth - base (one fp32 subtraction each,
 * rounded once), or src and truth without base.  A pixel is used iff both binned values are
 * finite.  The bin is srmi_distribution's, exactly: scale = fp32(B) / (hi - lo), entry 0 below
 * lo, entry B + 1 above hi, x == hi in entry B, the comparisons before any conversion.  hist
 * [C][2][B + 2] int64 (0: src, 1: truth), count [C] int64 = the used pixels.  first != 0
 * overwrites hist and count, first == 0 adds to them.  Launches: histogram partials (LDS
 * integer atomics, one int32 table per workgroup, plain stores), then finish, the single
 * writer of every entry, which reads the partial tables in workgroup order: exact and
 * bit-identical from run to run.  srmi_quantile_map_accumulate_workspace (host only) gives the
 * bytes of `workspace` (16-byte aligned; it need not be initialised).  No alignment
 * requirement on src, truth or base.  A missing src, truth, workspace, hist, count or range, a
 * workspace that is too small or not aligned, B, C or a range outside the above, H or W < 1
 * or H W > 2^31 - 1: SRMI_ERR_ARG.
 *
 * srmi_quantile_map_fit: one launch, one workgroup per channel, from the int64 tables alone
 * (count is what accumulate wrote beside them; N below is the tables' own sum, which equals
 * it).  With w = (hi - lo) / B in fp64 and edge[j] = lo + (j - 1) w for j = 0 .. M, edge[B + 1]
 * = hi exactly: ca[j], cb[j] = the cumulative counts of the src and truth tables before entry
 * j (ca[0] = 0, ca[M] = N).  T[j] = F_truth^-1(ca[j]) by the score's piecewise-linear
 * quantile: if cb[k] < ca[j] < cb[k + 1] for some k, T[j] = edge[k] + w (ca[j] - cb[k]) /
 * hb[k]; the search is over integers, only that line is fp64 arithmetic.  Tie rule (minimal
 * displacement): if ca[j] == cb[k] for k in k0 .. k1 (empty truth bins), the quantile is any
 * point of [edge[k0], edge[k1]], the left end -Inf when ca[j] == 0 and the right end +Inf
 * when ca[j] == N; T[j] is the point nearest to edge[j], clamp(edge[j], left, right).  Equal
 * tables therefore give T = edge, and T is non-decreasing for any pair of tables.  Tails:
 * tail_count >= 0; a knot with ca[j] < tail_count or N - ca[j] < tail_count is not trusted;
 * with j0, j1 the first and last trusted knots, the knots below j0 are edge[j] + (T[j0] -
 * edge[j0]) and those above j1 edge[j] + (T[j1] - edge[j1]), the constant-shift extrapolation
 * of quantile-mapping practice; no trusted knot, or N == 0: T = edge, the identity.  knots
 * [C][M + 1] fp64 = T; table [C][M + 1] fp32 = fp32(T); meta [C][4] fp32 = {lo, hi, fp32(T[0] -
 * edge[0]), fp32(T[M] - edge[M])}.  A missing hist, count, range, knots, table or meta, B, C
 * or a range outside the above, tail_count < 0: SRMI_ERR_ARG.
 *
 * srmi_quantile_map_apply: x, base, out [C][H][W] fp32 on the device; out may be x (in place)
 * and must otherwise not overlap it; base may be NULL and must not overlap out.  table and
 * meta are fit's, on the device.  Per pixel, every operation fp32 and rounded once, none
 * fused, with scale = fp32(B) / (hi - lo):
 *   v = x - base (x without base); v NaN: out = x, the same bits;
 *   u = (v - lo) * scale + 1; u < 0: out = x + strength * meta[2]; u >= M: out = x + strength
 *   * meta[3] (decided before any conversion: +-Inf and huge values index nothing);
 *   otherwise k = min((int)u, M - 1), f = u - (float)k, y = table[k] + f * (table[k + 1] -
 *   table[k]), out = x + strength * (y - v).
 * The correction is added to x in both modes: base only locates v.  strength finite in [0, 1].
 * One launch: the channel's table as (value, slope) pairs in LDS, one 8-byte LDS read per
 * pixel; 16-byte global accesses where x, base and out of a plane are 16-byte aligned, scalar
 * ones where not.  A missing x, table, meta or out, out overlapping base or partly
 * overlapping x, strength outside [0, 1] (NaN included), B or C outside the above, H or W < 1
 * or H W > 2^31 - 1: SRMI_ERR_ARG. */
int srmi_quantile_map_accumulate_workspace(int C, int H, int W, int nbins, size_t* bytes);
int srmi_quantile_map_accumulate(const float* src, const float* truth, const float* base, int C, int H, int W,
                                 int nbins, const float* range, int first, void* workspace, size_t workspace_bytes,
                                 long long* hist, long long* count, void* stream);
int srmi_quantile_map_fit(const long long* hist, const long long* count, int C, int nbins, const float* range,
                          long long tail_count, double* knots, float* table, float* meta, void* stream);
int srmi_quantile_map_apply(const float* x, const float* base, int C, int H, int W, int nbins, const float* table,
                            const float* meta, float strength, float* out, void* stream);

/* ---- consistency with the coarse input (no reference counterpart) -------- */
/* Iterative back-projection x <- x + U(lr - D x) of an HR field x [C][h s][w s] onto the LR
 * field lr [C][h][w] it was made from, D = F.interpolate at 1 / s in `dmode`, U =
 * F.interpolate at s in `umode` (SRMI_INTERP_*, align_corners=False).  At an even s, D
 * reads only the s x s children of an LR pixel (bicubic: taps s/2 - 2 .. s/2 + 1 per axis
 * with [-3, 19, 19, -3] / 32, which needs s >= 4; bilinear: s/2 - 1 and s/2 with 1/2 each),
 * so with r0 = lr - D x0 and E = I - D U the K-th iterate is x_K = x0 + U(R_K), R_K = sum_{k
 * < K} E^k r0, and its residual lr - D x_K = E^K r0: the loop runs on LR-size buffers.
 * Along one axis D U is the stencil g[-2 .. 2] (g[-2] = g[2] = 0 when U is bilinear) read
 * at indices clamped to the field -- U's own edge rule; in 2-D it is g (x) g.
 * Mask rule: an LR cell is ACTIVE iff lr is finite there and every tap of D in x0 is
 * finite; r is 0 at the other cells at every step (the operator is M E M), and the apply
 * step adds U(R) to every finite HR pixel and never writes a non-finite one.
 * All three: fp32, on `stream`, no host synchronisation, no atomics, no allocation --
 * capturable and bit-identical from run to run.  A missing buffer or a mode that is not
 * SRMI_INTERP_BILINEAR / _BICUBIC: SRMI_ERR_ARG; C, h, w < 1, a scale that is odd, above
 * 64 or below 4 (2 where only bilinear taps are read), or (h s)(w s) >= 2^31:
 * SRMI_ERR_SHAPE; nothing is enqueued in either case. */
/* r0 [C][h][w] = lr - D(hr) at the active cells, 0 elsewhere; active [C][h][w] int32 = 1 /
 * 0.  Every element of both is written.  Per cell the tap rows of its block are read once
 * (16-byte loads along rows where scale is 4 or 8 and hr is 16-byte aligned) and summed as
 * srmi_downsample does: per row the taps in ascending x, then the rows in ascending y. */
int srmi_consistency_residual(const float* hr, const float* lr, int C, int h, int w, int scale, int dmode, float* r0,
                              int* active, void* stream);
/* One step on LR-size buffers: R = (first ? 0 : R) + r, then r_out = r - (D U) r at the
 * active cells and 0 elsewhere -- the (2 radius + 1)^2-tap clamped-index stencil, radius 2
 * (U bicubic) or 1 (U bilinear), x taps summed per row, rows then summed; g is derived on
 * the host in double from ATen's cubic (A = -0.75) / linear weights of (scale, umode,
 * dmode) and rounded to fp32.  Started from r = r0 with first = 1 and ping-ponged, K
 * launches leave R = R_K and r_out = E^K r0, the residual of the corrected field.  Every
 * element of R and r_out is written.  r, R and r_out must be three different buffers:
 * SRMI_ERR_ARG otherwise. */
int srmi_consistency_iterate(const float* r, const int* active, int C, int h, int w, int scale, int umode, int dmode,
                             int first, float* R, float* r_out, void* stream);
/* hr [C][h s][w s] += U(R) at every finite pixel of hr, with srmi_upsample's (bicubic) /
 * srmi_interpolate's (bilinear) coordinate and weight arithmetic evaluated in the kernel;
 * U(R) is never materialised.  A thread owns the `scale` pixels of one row that share an
 * LR parent and reads their 4 x 5 (2 x 3) neighbourhood of R once, combined along y first.
 * A non-finite pixel of hr is never stored to: its bits (NaN payloads included) stay.  R
 * must be finite (srmi_consistency_iterate's is).  16-byte accesses where scale % 4 == 0
 * and hr is 16-byte aligned. */
int srmi_consistency_apply(const float* R, int C, int h, int w, int scale, int umode, float* hr, void* stream);

/* The adjoint of the correction, for training through it.  With M the active mask, G the
 * clamped D U stencil above and E = M (I - G), the three calls above compute x_K = x0 + U P M
 * (lr - D x0), P = sum_{k < K} E^k, which is affine in x0 with Jacobian J = I - U P M D.  For
 * a gradient g [C][h s][w s] with respect to x_K, J^T g is
 *     q = U^T g;   t_0 = q, t_{k+1} = (I - G^T)(M t_k), Q = sum_{k < K} t_k;   g0 = g - D^T (M Q)
 * (lr takes no gradient).  The same conventions hold: C counts planes, fp32, on `stream`, no
 * host synchronisation, no atomics, no allocation, a fixed summation order -- capturable and
 * bit-identical from run to run -- and the same refusals, with nothing enqueued. */
/* q [C][h][w] = U^T g: each LR cell sums the HR pixels whose clamped taps reach it (those of
 * the blocks within 2 of it per axis, 1 for bilinear), with the weights of srmi_upsample /
 * srmi_interpolate at that pixel, taps that clamp onto one cell added in ascending tap order.
 * Separable: a workgroup owns a band of up to 8 LR rows and a strip of up to 64 LR columns,
 * keeps the per-axis weights in an LDS table, reduces the band's HR rows along x into LDS
 * (ascending X) and those along y (ascending Y).  Band and strip shrink until the LDS fits
 * 48 KB (a band of one row and a strip of 8 columns at scale 64 take 31.6 KB), so there is no
 * limit on w s.  16-byte loads of g where scale % 4 == 0 and g is 16-byte aligned.  g must be
 * finite.  Every element of q is written. */
int srmi_consistency_adjoint_gather(const float* g, int C, int h, int w, int scale, int umode, float* q,
                                    void* stream);
/* One step on LR-size buffers: Q = (first ? 0 : Q) + t, then t_out = M t - G^T (M t), at every
 * cell (t_out is not masked; an inactive cell of t is read as an exact zero).  Along an axis
 * G^T gathers from i = j - 2 .. j + 2 with w^T[j, i] = sum_o g_o [clamp(i + o) = j], g as in
 * srmi_consistency_iterate.  Started from t = q with first = 1 and ping-ponged, K launches
 * leave Q = sum_{k < K} t_k.  `active` is srmi_consistency_residual's.  t, Q and t_out must be
 * three different buffers: SRMI_ERR_ARG otherwise. */
int srmi_consistency_adjoint_iterate(const float* t, const int* active, int C, int h, int w, int scale, int umode,
                                     int dmode, int first, float* Q, float* t_out, void* stream);
/* g [C][h s][w s] -= D^T (M Q), in place: g[Y][X] -= k(Y mod s) k(X mod s) Q[Y / s][X / s] at
 * the tap phases of D inside the blocks of the active cells.  Pixels at the other phases (at
 * scale 8 under a bicubic D: 0, 1, 6, 7) and the blocks of inactive cells are neither read
 * nor written.  16- or 8-byte accesses where the taps fill an aligned quad or pair (scale %
 * 4 == 0, bicubic D, g 16-byte aligned). */
int srmi_consistency_adjoint_apply(const float* Q, const int* active, int C, int h, int w, int scale, int dmode,
                                   float* g, void* stream);

/* ---- the spectral loss term (no reference counterpart) ------------------ */
/* A Fourier-space term beside the pixel loss of a training step: the windowed amplitudes
 * of the error of pred against target, both [nplanes][H][W] fp32 on the device (nplanes =
 * N C), possibly with NaN / Inf.
 *   Jobs: windows of side P in {16, 32, 64}, P <= min(H, W), stride Q in 1 .. P, origins
 *   min(i Q, L - P), i < srmi_overlap_count(L, P, Q), row-major, nwin per plane.  A job is one
 *   window of one plane; it is skipped when any of its P^2 pixels is non-finite in pred or
 *   in target (per plane, not across channels).
 *   Per used job: d = pred - target (fp32), z = h(y) h(x) d with the periodic Hann taper
 *   h(q) = 0.5 - 0.5 cos(2 pi q / P) (the mean is NOT removed), D = DFT2(z), unnormalised;
 *   c = P^2 W2, W2 = sum (h(y) h(x))^2; A_k = sqrt(|D_k|^2 / c + eps) for each of the P^2
 *   bins.  S = the sum of A_k over the bins of the used jobs, Nused = the used jobs, and
 *   L_spec = S / (Nused P); Nused = 0: L_spec = 0 and its gradient is 0.
 *   Gradient: with G_k = D_k / (c A_k) (Hermitian), d L_spec / d pred (y, x) =
 *   1 / (Nused P) * the sum over the used jobs w covering (y, x) of h(y - y0_w) h(x - x0_w)
 *   Re IDFT2(G) (y - y0_w, x - x0_w), the inverse unnormalised.  The taper is 0 at q = 0: a
 *   plane's first row and column get no spectral gradient.
 * Arithmetic: fp32 transforms (two jobs of a plane share one complex transform), the bins
 * and every sum in fp64 in a fixed order, no atomics: bit-identical from run to run, and
 * the same bits whether the planes go through one call or several.
 * srmi_spectral_loss_workspace (host only): the bytes of `workspace` (16-byte aligned,
 * need not be initialised) for nplanes planes; it is laid out plane by plane, bytes /
 * nplanes each, so a call over planes p0 .. p0 + n - 1 of a batch takes the batch's
 * workspace + p0 * (bytes / nplanes).
 * srmi_spectral_loss_parts: per plane the job sums added in window order (fp64, rounded
 * once) into parts[nplanes] and the used jobs into cparts[nplanes] (floats, exact); the
 * gradient windows of the used jobs, tapered and not yet scaled, and the used flags stay
 * in the workspace for srmi_spectral_loss_dy.
 * srmi_spectral_loss_from_parts: parts and cparts summed over the nplanes of the (global)
 * batch in fp64 in a fixed grouping (that of srmi_gradient_loss_from_parts below), spec4 =
 * {S, Nused, 1 / (Nused P), L_spec} (all 0 when Nused = 0) and total[0] = fma(weight, spec4[3],
 * base[0]).  base: one device float, the finalised pixel loss (&loss4[3]), as its siblings
 * below take it; it is only read.
 * srmi_spectral_loss_dy: dy [nplanes][H][W] = fma(weight * spec4[2], the fp32 sum of the used
 * windows' gradients covering the pixel in ascending window index, dy); the scale is read
 * from the device.  A pixel no used window covers is not written; weight == 0 launches nothing.
 * All three: no allocation, no host read, capturable.  SRMI_ERR_ARG, nothing launched: P
 * not 16, 32 or 64 or > min(H, W); Q outside 1 .. P; nplanes < 1; eps <= 0; weight < 0 or
 * not finite; a missing buffer; a workspace that is too small or not 16-byte aligned. */
int srmi_spectral_loss_workspace(long long nplanes, int H, int W, int P, int Q, size_t* bytes);
int srmi_spectral_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, int P, int Q,
                             float eps, float* parts, float* cparts, void* workspace, size_t workspace_bytes,
                             void* stream);
int srmi_spectral_loss_from_parts(const float* parts, const float* cparts, long long nplanes, int P, float weight,
                                  const float* base, float* spec4, float* total, void* stream);
int srmi_spectral_loss_dy(const void* workspace, size_t workspace_bytes, long long nplanes, int H, int W, int P, int Q,
                          float weight, const float* spec4, float* dy, void* stream);

/* ---- the SSIM loss term (no reference counterpart) ---------------------- */
/* A structural term beside the pixel loss of a training step: 1 - the mean SSIM of pred = a
 * against target = b, both [nplanes][H][W] fp32 on the device (nplanes = N C), possibly with
 * NaN / Inf.  Everything of "the SSIM score" above holds per plane: the 11 fp32 taps g, G = g
 * (x) g; the valid positions only (Hv = H - 10 rows of Wv = W - 10); a position is USED iff
 * the 121 pixels of its window are finite in a and in b of that plane; lo, hi the min / max of
 * b's finite pixels in the plane, L = hi - lo, or data_range where data_range > 0; the pivot
 * r = 0.5 lo + 0.5 hi (always b's); C1 = (0.01 L)^2, C2 = (0.03 L)^2.  A plane contributes no
 * position when it has no finite target pixel or when L is 0 or not finite (a constant
 * target).  With a' = a - r, b' = b - r (0 where a pixel is not finite in both):
 *   m_a = G * a', m_b = G * b', s_aa = G * a'^2 - m_a^2, s_bb likewise, s_ab = G * (a' b') -
 *   m_a m_b; mu_a = m_a + r, mu_b = m_b + r; D_l = mu_a^2 + mu_b^2 + C1, l = (2 mu_a mu_b + C1)
 *   / D_l; D_c = s_aa + s_bb + C2, cs = (2 s_ab + C2) / D_c; ssim = l cs.
 *   S = the sum of ssim over the used positions of all planes of the (global) batch, Nused
 *   their number, L_ssim = 1 - S / Nused; Nused = 0: L_ssim = 0 and its gradient is 0.
 *   Gradient (L and r are constants).  At a used position p: B_p = -2 l cs / D_c, C_p = 2 l /
 *   D_c, A_p = 2 cs (mu_b - mu_a l) / D_l - B_p m_a - C_p m_b; A = B = C = 0 at every other
 *   position.  dS / da (q) = (G^T * A)(q) + a'(q) (G^T * B)(q) + b'(q) (G^T * C)(q), G^T * the
 *   zero-extended ("full") correlation of an [Hv][Wv] map back onto [H][W].  The pivoted form
 *   is part of the definition: at 290 +- 1.5 the unpivoted terms cancel in fp32.
 * Arithmetic: fp32 as the score's (separable, the horizontal pass first, taps ascending, FMA),
 * every sum over positions, tiles and planes in fp64 or integers in a fixed order, no atomics:
 * bit-identical from run to run, and the same bits whether the planes go through one call or
 * several.
 * srmi_ssim_loss_workspace (host only): the bytes of `workspace` (16-byte aligned, need not
 * be initialised) for nplanes planes; it is laid out plane by plane, bytes / nplanes each, so
 * a call over planes p0 .. p0 + n - 1 of a batch takes the batch's workspace + p0 * (bytes /
 * nplanes).  Per plane it holds r and L, the range pass's min / max pairs, the position tiles'
 * sums and counts, and the maps A, B, C [Hv][Wv].
 * srmi_ssim_loss_parts: three launches (range pass, tile pass, per-plane sum).  pred, target
 * [nplanes][H][W]; data_range: L of every plane, <= 0: the target's own range per plane;
 * parts[nplanes]: per plane the fp64 sum of ssim over its used positions in a fixed order,
 * rounded once to fp32; cparts[nplanes]: their count as a float (exact: H W <= 2^24).  Every
 * element of the workspace that srmi_ssim_loss_dy reads is written here.
 * srmi_ssim_loss_from_parts: parts and cparts [nplanes] summed over the planes of the
 * (global) batch in fp64 in a fixed grouping (that of srmi_gradient_loss_from_parts below);
 * ssim4 = {S, Nused, 1 / Nused, L_ssim} (all 0 when Nused = 0) and total[0] = fma(weight,
 * ssim4[3], base[0]).  base: one device float, the finalised pixel loss (&loss4[3]) or the
 * total of the term before this one; it is only read.
 * srmi_ssim_loss_dy: workspace as srmi_ssim_loss_parts left it for these planes, pred and
 * target the same fields; dy [nplanes][H][W] = fma(-weight ssim4[2], dS / da, dy), the scale
 * read from the device, one rounding.  A pixel that is not finite in both pred and target is
 * not written; weight == 0 launches nothing.
 * All three: `stream`, no allocation, no host read, capturable.  SRMI_ERR_ARG, nothing
 * launched and no output touched: H or W < 11; H W > 2^24; nplanes < 1; data_range NaN or
 * +-Inf; weight < 0 or not finite; a missing buffer; a workspace that is too small or not
 * 16-byte aligned. */
int srmi_ssim_loss_workspace(long long nplanes, int H, int W, size_t* bytes);
int srmi_ssim_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, float data_range,
                         float* parts, float* cparts, void* workspace, size_t workspace_bytes, void* stream);
int srmi_ssim_loss_from_parts(const float* parts, const float* cparts, long long nplanes, float weight,
                              const float* base, float* ssim4, float* total, void* stream);
int srmi_ssim_loss_dy(const void* workspace, size_t workspace_bytes, const float* pred, const float* target,
                      long long nplanes, int H, int W, float weight, const float* ssim4, float* dy, void* stream);

/* ---- the gradient loss term (no reference counterpart) ------------------ */
/* A first-derivative term beside the pixel loss of a training step: the mean Charbonnier
 * magnitude of the Sobel gradient of the error.  pred and target [nplanes][H][W] fp32 on the
 * device (nplanes = N C), possibly with NaN / Inf; tests/gradient_oracle.py restates it in
 * fp64.  The operator, the valid positions and the rule for a USED position are those of "the
 * gradient score" above, at unit spacing (training tiles are normalised).
 *   e = pred - target in fp32, 0 where the pixel is not finite in both.  At a used position:
 *   a = Gx[e], b = Gy[e], phi = sqrt(a a + b b + eps), eps under the root as in the reference's
 *   Charbonnier (dual_trainer.py:122, :197), every operation rounded once in fp32 in that
 *   order, none contracted.
 *   S = the sum of phi over the used positions of all planes of the (global) batch, Nused
 *   their number, L_grad = S / Nused; Nused = 0: L_grad = 0 and its gradient is 0, not NaN.
 *   Gradient: U = a / phi, V = b / phi at the used positions, 0 at every other.  dS / dpred (q)
 *   = (Gx^T U)(q) + (Gy^T V)(q), the transposes the zero-extended ("full") correlations of the
 *   [Hv][Wv] maps back onto [H][W]; since the operator is antisymmetric this is -(Gx[U] +
 *   Gy[V])(q) with the operator applied to the zero-extended maps, which is how it is formed:
 *   the same operation order, then one addition, then the sign.
 * Every sum over positions, tiles and planes is in fp64 or integers in a fixed order, no
 * atomics: bit-identical from run to run, whatever the workspace held, and the same bits
 * whether the planes go through one call or several.
 * srmi_gradient_loss_workspace (host only): the bytes of `workspace` (16-byte aligned, need
 * not be initialised) for nplanes planes; it is laid out plane by plane, bytes / nplanes each,
 * so a call over planes p0 .. p0 + n - 1 of a batch takes the batch's workspace + p0 * (bytes
 * / nplanes).  It holds the per-workgroup sums and counts of srmi_gradient_loss_parts only.
 * srmi_gradient_loss_parts: two launches (tile pass, per-plane sum).  parts[nplanes]: per
 * plane the fp64 sum of phi over its used positions, rounded once to fp32; cparts[nplanes]:
 * their count as a float (exact: H W <= 2^24).
 * srmi_gradient_loss_from_parts: parts and cparts [nplanes] summed over the planes of the
 * (global) batch in fp64 in a fixed grouping -- 256 contiguous shares of ceil(nplanes / 256)
 * planes, each in plane order, then the shares in order: the plain sum in plane order up to
 * 256 planes, and for any nplanes independent of how the planes were split over calls (the
 * three terms' finalizes are one piece of device code); grad4 = {S, Nused, 1 / Nused, L_grad}
 * (all 0 when Nused = 0) and total[0] = fma(weight, grad4[3], base[0]).  base: one device
 * float, the finalised pixel loss (&loss4[3]) or the total of the term before this one; it is
 * only read.
 * srmi_gradient_loss_dy: dy [nplanes][H][W] = fma(weight grad4[2], dS / dpred, dy), the scale
 * read from the device, one rounding, one writer per pixel.  It RECOMPUTES U and V from pred
 * and target (a workgroup stages its rectangle of e with a two-pixel halo in LDS) and so takes
 * no workspace: storing the two maps would move 8 plane-sized transfers over the two launches
 * instead of 6.  A pixel that is not finite in both pred and target is not written; weight ==
 * 0 launches nothing.
 * Rows are loaded and stored 16 bytes at a time when W % 4 == 0 and pred, target (and dy) are
 * 16-byte aligned, one float at a time otherwise: the same bits.
 * All three: `stream`, no allocation, no host read, capturable.  SRMI_ERR_ARG, nothing
 * launched and no output touched: H or W < 3; H W > 2^24; nplanes < 1; eps <= 0 or not finite;
 * weight < 0 or not finite; a missing buffer; a workspace that is too small or not 16-byte
 * aligned. */
int srmi_gradient_loss_workspace(long long nplanes, int H, int W, size_t* bytes);
int srmi_gradient_loss_parts(const float* pred, const float* target, long long nplanes, int H, int W, float eps,
                             float* parts, float* cparts, void* workspace, size_t workspace_bytes, void* stream);
int srmi_gradient_loss_from_parts(const float* parts, const float* cparts, long long nplanes, float weight,
                                  const float* base, float* grad4, float* total, void* stream);
int srmi_gradient_loss_dy(const float* pred, const float* target, long long nplanes, int H, int W, float eps,
                          float weight, const float* grad4, float* dy, void* stream);

/* ---- training batch preparation ------------------ */
/* raw [B][C][T][T] fp32 tiles (select_batch, sres/base/source/swot/raw.py:160-166)
 * -> hr [B][C][T][T] = xyflip(lnorm(raw)) (norm 'lnorm' raw.py:169-181: per tile
 * and channel (x - mean) / std, ddof 0; xyflip sres/base/source/batch.py:37-49
 * with the drawn flip_index 0..7), lr [B][C][T/scale][T/scale] = downsample(hr)
 * (array.py:72-76; NULL: skipped), mean/std [B][C] (norm's ncstats attrs; NULL:
 * skipped).  T even. */
int srmi_batch_prep(const float* raw, int B, int C, int T, int flip_index, int scale, float* hr, float* lr,
                    float* mean, float* std, void* stream);

/* ---- every task.norm mode, and the dataset tile statistics ------------- */
/* norm() (sres/base/source/swot/raw.py:169-214) has six branches.  On the device
 * they are three modes: the two that take their statistics from the tile itself,
 * and one that is handed an offset and a divisor per (tile, channel) -- 'gnorm'
 * (raw.py:187-191), 'gscale' (:192-195), 'tnorm' (:196-203) and 'tscale'
 * (:204-209) differ only in which statistics the caller puts there
 * (srmi.norm.NormStats.offsets). */
#define SRMI_NORM_LNORM 0  /* (x - mean) / std of the tile          (raw.py:177-181) */
#define SRMI_NORM_LSCALE 1 /* (x - min) / (max - min) of the tile   (raw.py:182-186) */
#define SRMI_NORM_AFFINE 2 /* (x - off[b][c]) / div[b][c], caller's (raw.py:187-209) */

/* srmi_batch_prep with a norm mode.  LNORM is srmi_batch_prep itself (off_out =
 * mean, div_out = std; B <= 65535).  LSCALE: off_out [B][C] = min, div_out =
 * max - min in fp32 (NULL: skipped); the tile is divided by the exact difference,
 * so its extremes are exactly 0 and 1.  AFFINE: hr = fp32(((double)x - off) / div)
 * to within one fp32 ulp (the quotient is a product with the fp64 reciprocal);
 * off / div [B][C]; off_out / div_out are not written.  LSCALE and AFFINE take any
 * B with B * C < 2^31 (a whole time slice); their raw and hr must be 16-byte
 * aligned (SRMI_ERR_ARG otherwise).  div == 0 gives the IEEE result, as in the
 * reference.  xyflip and the LR tile are srmi_batch_prep's. */
int srmi_batch_prep_norm(const float* raw, long long B, int C, int T, int flip_index, int scale, int mode,
                         const float* off, const float* div, float* hr, float* lr, float* off_out, float* div_out,
                         void* stream);
/* srmi_region_to_tiles with a norm mode (get_tiles raw.py:216-233 + norm
 * raw.py:169-214); off / div / off_out / div_out are [gy*gx][C], indexed by grid
 * cell.  LNORM is srmi_region_to_tiles itself (off_out = mean, div_out = std, both
 * required).  srmi_tiles_to_region (x * std + mean) undoes LSCALE with mean :=
 * off_out, std := div_out, and AFFINE with off / div -- denorm's two branches
 * (sres/controller/dual_trainer.py:67-77). */
int srmi_region_to_tiles_norm(const float* region, int C, int H, int W, int ty, int tx, int mode, const float* off,
                              const float* div, float* tiles, float* off_out, float* div_out, int* bad,
                              void* stream);
/* _compute_normalization (raw.py:89-106) for one time slice: tiles [n][C][ty][tx]
 * (srmi_tiles_gather's result), acc [n][C][4] fp64 = {sum over calls of the
 * plane's mean, sum of its variance (ddof 0), running max, running min} --
 * NormData.add_entry (raw.py:55-60).  first != 0 initialises acc (max from -inf,
 * min from +inf) instead of accumulating.  n * C < 2^31.  Deterministic. */
int srmi_tile_stats(const float* tiles, long long n, int C, int ty, int tx, double* acc, int first, void* stream);
/* tstats [n][C][4] = {sum mean / ntimes, sum var / ntimes, max, min}, the STATS
 * order of NormData.get_norm_stats (raw.py:18, :62-63); gstats [C][4] =
 * globalize_norm (raw.py:23-30): mean over the tiles of the means and of the
 * variances, max of the max, min of the min, reduced in fp64 in a fixed order.
 * Either output may be NULL; both must be 16-byte aligned. */
int srmi_tile_stats_finalize(const double* acc, long long n, int C, int ntimes, float* tstats, float* gstats,
                             void* stream);

/* ---- on-disk LLC4320 source -> tiles --------------- */
/* Replaces SWOTRawDataLoader.load_file (sres/base/source/swot/raw.py:133-145):
 * template_be = the raw bytes of the '>f4' mask template (13 nx^2 words, 0 =
 * land), data_be = the raw bytes of a '>f4' wet-value file.  The index map of
 * the ROI [y0, y0+ys) x [x0, x0+xs) of the east | west.T[::-1] image (mds2d,
 * swot/util.py:3-7; subset_roi raw.py:38-45) is built once per template:
 * idx_map[ys*xs] = wet-value index or -1; *n_wet (device) = wet cell count.
 * workspace: srmi_llc_index_map_workspace bytes (n_template int32 ranks + scan). */
int srmi_llc_index_map_workspace(long long n_template, size_t* bytes);
int srmi_llc_index_map(const void* template_be, long long n_template, int nx, int y0, int ys, int x0, int xs,
                       int* idx_map, long long* n_wet, void* workspace, size_t workspace_bytes, void* stream);
/* out[p] = decoded data[idx_map[p]], NaN for land: one time slice of one variable */
int srmi_llc_gather(const void* data_be, long long n_values, const int* idx_map, long long npix, float* out,
                    void* stream);
/* get_tiles (raw.py:216-233): bad[c*gy*gx + t] = 1 where tile t of channel c of
 * region [C][H][W] holds a non-finite value (floor grid gy = H/ty, gx = W/tx) */
int srmi_tiles_nonfinite(const float* region, int C, int H, int W, int ty, int tx, int* bad, void* stream);
/* out[m] (ty x tx plane m of the [n/C][C][ty][tx] result) = tile plane src[m]
 * (= c*gy*gx + t of the channel-major flattening) */
int srmi_tiles_gather(const float* region, int C, int H, int W, int ty, int tx, const int* src, int nslots,
                      float* out, void* stream);

/* Sparse reads of a wet-value file (SWOTRawDataLoader.load_file, raw.py:133-145,
 * reads the whole file; a ROI needs a small share of it).  The file is cut into
 * blocks of 2^block_shift words.  mask[n_blocks] (int32) is zeroed, then
 * mask[idx >> block_shift] = 1 for every idx_map entry >= 0.  SRMI_ERR_SHAPE if
 * an index lies past n_blocks << block_shift.  Once per template and ROI;
 * synchronises the stream (the error comes back from the device). */
int srmi_llc_block_mask(const int* idx_map, long long npix, int block_shift, int* mask, int n_blocks, void* stream);
/* load_file (raw.py:133-145) over the blocks that were read: block_base[b] = the
 * word offset of file block b in the compact staging buffer, -1 = not read.
 * idx_out[p] = idx < 0 ? -1 : block_base[idx >> shift] + (idx & (2^shift - 1)),
 * and -1 where the block was not read: srmi_llc_gather(data = the compact words,
 * n_values = their count, idx_map = idx_out) then gives the ROI image, NaN there.
 * Once per template and ROI. */
int srmi_llc_compact_map(const int* idx_map, long long npix, int block_shift, const int* block_base, int n_blocks,
                         int* idx_out, void* stream);
/* get_tiles' keep list (raw.py:216-233) on the device: keep = flatnonzero(bad == 0)
 * over the C * ncells flags of srmi_tiles_nonfinite, n = len(keep) / C;
 * src[0 .. n*C) = keep[0 .. n*C), count[0] = n, count[1] = len(keep).  An
 * order-preserving compaction by one workgroup, no atomics: deterministic. */
int srmi_tiles_keep(const int* bad, int C, int ncells, int* src, int* count, void* stream);
/* srmi_tiles_gather (get_tiles, raw.py:216-233) with the slot count count[0] * C
 * read on the device (srmi_tiles_keep's count): launched for max_slots planes of
 * out; a plane at or past the count neither reads src nor writes out. */
int srmi_tiles_gather_dev(const float* region, int C, int H, int W, int ty, int tx, const int* src, const int* count,
                          int max_slots, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRMI_H */
