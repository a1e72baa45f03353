/* sln_hip.h - C ABI of libsln_hip.so, the MI355X (gfx950) implementation of the 3D_SLN hot path.
 *
 * The reference (aluo-x/3D_SLN) has no FFI layer: its boundary for this path is a set of Python
 * call surfaces.  This header is what those surfaces bind to; the Python mirror
 * in 3d_sln_amd/host/ loads the library with ctypes and passes raw device pointers
 * (torch.Tensor.data_ptr()) plus the current HIP stream.  No torch types cross this boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; tensors are dense
 *     row-major fp32 unless stated; index tensors are int64 exactly as the reference's
 *     suncg_collate_fn produces them (data/suncg_dataset.py:295-337);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued, nothing synchronises;
 *   - every function returns 0 on success, a hipError_t value (>0) for a HIP failure, or a
 *     negative SLN_E_* code for a contract violation (nothing is launched in that case).
 *
 * Each entry point cites the reference interface it stands behind (paths relative to the
 * reference repository root).
 */
#ifndef SLN_HIP_H
#define SLN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLN_E_BADARG (-1)      /* null pointer / size that violates the contract below            */
#define SLN_E_UNSUPPORTED (-2) /* configuration outside the HIP path (e.g. gconv_num_layers == 0) */
#define SLN_E_STATE (-3)       /* call order violated (e.g. backward before forward)             */
#define SLN_E_NOGPU (-4)       /* no gfx950 device visible                                       */
#define SLN_E_NOMEM (-5)       /* a host staging buffer / event could not be allocated           */
#define SLN_E_CAPTURE (-6)     /* the caller's stream is being captured and the call needs an eager upload (new batch shape) */

int sln_version(void);                 /* ABI version, bumped on any signature change */
const char* sln_build_arch(void);      /* "gfx950" */
int sln_device_ok(void);               /* 0 when a gfx950 device is usable, SLN_E_NOGPU otherwise */

/* =============================================================================================
 * A. Scene-graph VAE  (models/graph.py:10-143, models/Sg2ScVAE_model.py:7-188, utils.py:12-33,
 *    train.py:62-84)
 * ============================================================================================= */

typedef struct SlnVaeConfig {
  int embedding_dim;     /* Sg2ScVAE_model.py:8; must be a multiple of 16                         */
  int gconv_num_layers;  /* >= 1                                                                   */
  int recurrent;         /* gconv_mode == 'recurrent' (weights shared by all layers)               */
  int batch_norm;        /* mlp_normalization == 'batch' (1) or 'none' (0)                         */
  int decoder_cat;       /* 1: z is concatenated in front of the decoder's gconv net (train.py default,
                          * options/options.py:55); 0: behind it (the class default, Sg2ScVAE_model.py:9,157-164) */
  int use_ae;            /* use_AE: z = mu, no KL term                                             */
  int box_dim;           /* 6 (train_3d) or 4                                                      */
  int n_angle;           /* Nangle = 24                                                            */
  int num_objs;          /* rows of obj_embeddings_* (len(object_idx_to_name) + 1)                 */
  int num_preds;         /* rows of pred_embeddings_*                                              */
  int num_attrs;         /* rows of attr_embedding_* (0 with no_attr)                              */
  int no_attr;           /* 1 = use_attr=False (Sg2ScVAE_model.py:17,35-37,48-50,97-98): no attribute
                          * embeddings, the class embedding is E wide, box_net reads 2E columns     */
} SlnVaeConfig;

/* Number of Linear(+BatchNorm) units and their canonical order:
 *   box_mean_var.{0,1}, box_mean.0, box_var.0, angle_mean_var.{0,1}, angle_mean.0, angle_var.0,
 *   gconv_net_ec.gconvs.i.{net1.0, net1.1, net2.0, net2.1} for each module i,
 *   gconv_net_dc.gconvs.i.{...}, box_net.{0,1}, angle_net.{0,1}
 * ("X.1" is the second Linear of the MLP, state_dict index 3 with BatchNorm, 2 without). */
int sln_vae_num_units(const SlnVaeConfig* cfg);

typedef struct SlnVaeUnit {        /* one Linear [+ BatchNorm1d] */
  float* weight;  float* bias;                 /* [out, in], [out]                               */
  float* bn_weight; float* bn_bias;            /* [out] or NULL                                  */
  float* bn_running_mean; float* bn_running_var; int64_t* bn_num_batches_tracked;
  float* d_weight; float* d_bias; float* d_bn_weight; float* d_bn_bias;   /* gradients (+=)      */
} SlnVaeUnit;

typedef struct SlnVaeTensors {
  /* embeddings, Sg2ScVAE_model.py:44-58 (parameter, gradient) */
  float* obj_emb_ec;  float* d_obj_emb_ec;
  float* pred_emb_ec; float* d_pred_emb_ec;
  float* obj_emb_dc;  float* d_obj_emb_dc;
  float* pred_emb_dc; float* d_pred_emb_dc;
  float* attr_emb_ec; float* d_attr_emb_ec;
  float* attr_emb_dc; float* d_attr_emb_dc;
  float* box_emb_w;   float* d_box_emb_w;
  float* box_emb_b;   float* d_box_emb_b;
  float* angle_emb;   float* d_angle_emb;
  const SlnVaeUnit* units_host;    /* HOST array of sln_vae_num_units() entries                  */
  /* flat views used by zero_grad / Adam / the data-parallel all-reduce: every parameter above
   * must live inside [flat_params, flat_params + n_flat) at the same offset as its gradient in
   * flat_grads.  adam_m / adam_v may be NULL when sln_vae_train_step is never called.           */
  float* flat_params; float* flat_grads; float* adam_m; float* adam_v; int64_t n_flat;
} SlnVaeTensors;

typedef struct SlnVaeBatch {       /* suncg_collate_fn's tuple, data/suncg_dataset.py:327-337     */
  const int64_t* objs;       /* [O]                                                              */
  const int64_t* triples;    /* [T,3] (s, p, o) with global row ids                              */
  const float*   boxes;      /* [O, box_dim]                                                     */
  const int64_t* angles;     /* [O]                                                              */
  const int64_t* attributes; /* [O]                                                              */
  int O, T;
} SlnVaeBatch;

typedef struct SlnVae SlnVae;      /* opaque engine: kernel plan + workspace carve-up             */

int sln_vae_create(const SlnVaeConfig* cfg, SlnVae** out);
void sln_vae_destroy(SlnVae* h);
/* bytes of device workspace needed for batches up to (max_objs, max_triples) */
int64_t sln_vae_workspace_bytes(const SlnVae* h, int max_objs, int max_triples);
/* workspace must be zero-filled once by the caller - the fill must have COMPLETED: bind writes into it with blocking copies
 * that are not ordered behind work on other streams - and stay alive while the engine is used */
int sln_vae_bind(SlnVae* h, const SlnVaeTensors* t, void* workspace, int64_t workspace_bytes,
                 int max_objs, int max_triples);

/* Build the per-batch graph structure (int32 ids, degrees, CSR of incident triples).  Must
 * precede encoder/decoder calls for a new batch.  Replaces the index/scatter_add bookkeeping of
 * GraphTripleConv.forward (models/graph.py:70-72,89-108), hoisted out of the 10 layers.  All five inputs are copied
 * (stream-ordered) into the workspace: the caller's tensors are not read after this call, and a captured iteration
 * (sln_vae_train_step with use_graph) replays on whatever batch was bound last. */
int sln_vae_set_batch(SlnVae* h, const SlnVaeBatch* b, void* stream);
/* Synchronising check of the bound batch: SLN_E_BADARG when a triple / class / attribute / angle id is out of range
 * (the reference's embedding and index ops raise IndexError there; the kernels neutralise such rows). */
int sln_vae_check_batch(SlnVae* h, void* stream);

/* Sg2ScVAEModel.encoder (Sg2ScVAE_model.py:115-143): writes mu, logvar [O, embedding_dim].
 * training != 0: BatchNorm uses batch statistics and updates running stats (train()). */
int sln_vae_encoder(SlnVae* h, float* mu, float* logvar, int training, void* stream);
/* Sg2ScVAEModel.decoder (:145-172).  z [O, embedding_dim]; boxes_pred [O, box_dim];
 * angles_pred [O, n_angle] = log_softmax. */
int sln_vae_decoder(SlnVae* h, const float* z, float* boxes_pred, float* angles_pred, int training, void* stream);
/* Sg2ScVAEModel.forward (:174-188) with the N(0,1) draw supplied by the caller (eps [O, E];
 * torch.randn_like in the reference).  z_out may be NULL. */
int sln_vae_forward(SlnVae* h, const float* eps, float* mu, float* logvar, float* z_out, float* boxes_pred,
                    float* angles_pred, int training, void* stream);

/* calculate_model_losses (utils.py:12-33): losses_out[4] = {bbox_pred, angle_pred, KLD*w, total}.
 * When with_grads != 0 the gradients w.r.t. boxes_pred / logits are kept for sln_vae_backward. */
int sln_vae_loss(SlnVae* h, const float* boxes_pred, const float* angles_pred, const float* mu,
                 const float* logvar, float kl_weight, float* losses_out, int with_grads, void* stream);

/* Backward of the decoder given d(boxes_pred) [O, box_dim] and d(angles_pred) [O, n_angle]
 * (gradient w.r.t. the log-softmax OUTPUT).  Accumulates parameter gradients, writes dz [O, E]. */
int sln_vae_decoder_backward(SlnVae* h, const float* d_boxes_pred, const float* d_angles_pred, float* dz, void* stream);
/* Backward of the encoder given d(mu), d(logvar) [O, E]; accumulates parameter gradients. */
int sln_vae_encoder_backward(SlnVae* h, const float* d_mu, const float* d_logvar, void* stream);
/* total_loss.backward() of train.py:83 after sln_vae_forward + sln_vae_loss(with_grads=1). */
int sln_vae_backward(SlnVae* h, void* stream);

/* Tell the engine that parameters were modified outside of it (load_state_dict, a torch optimizer):
 * cached transposed weights are rebuilt before the next backward. */
int sln_vae_params_changed(SlnVae* h);
int sln_vae_zero_grad(SlnVae* h, void* stream);                       /* optimizer.zero_grad(), train.py:82 */
/* torch.optim.Adam(lr).step(), train.py:15,84 (betas .9/.999, eps 1e-8, no weight decay) */
int sln_vae_adam_step(SlnVae* h, float lr, void* stream);
int sln_vae_adam_reset(SlnVae* h, int64_t step, void* stream);       /* restore the step counter (checkpoint resume) */
/* The device's own step counter (synchronises): after an iteration skipped for a non-finite loss it is one behind
 * the number of sln_vae_adam_step calls (train.py:79-81 skips the optimizer step too). */
int sln_vae_adam_get_step(SlnVae* h, int64_t* step_out, void* stream);
/* Data-parallel NaN guard (the reference is single-GPU: build_dataset_model.py:54-55 asserts).  `slot` = one device float
 * that the trainer all-reduces together with flat_grads (in practice flat_grads[n_flat]): SLN_TRAIN_BACKWARD /
 * SLN_TRAIN_UPTO_DECODER store the rank's total loss there, sln_vae_adam_step skips the update when the slot - by then
 * the average over the ranks - is not finite, so all replicas skip or step together.  NULL restores the per-rank guard.
 * Call while the engine is idle (captured iterations are dropped). */
int sln_vae_set_grad_guard(SlnVae* h, float* slot);
/* The reparameterisation draw, Sg2ScVAE_model.py:180-183 (eps = randn_like(std)).  sln_vae_forward / sln_vae_train_step
 * called with eps == NULL draw eps on the device: Philox-4x32-10 keyed by `seed`, one `offset` per draw (advanced by
 * the draw kernel itself, so a replayed hipGraph sees a new draw every iteration).  sln_vae_last_eps copies the eps of
 * the last forward / iteration (the injected one or the drawn one) to eps_out[O, embedding_dim]. */
int sln_vae_seed(SlnVae* h, uint64_t seed, uint64_t offset, void* stream);
int sln_vae_last_eps(SlnVae* h, float* eps_out, void* stream);
/* n values ~ N(0,1) from the engine's Philox stream (one offset per call, as the reparameterisation draws): the z draws of
 * posterior sampling (testing/test_VAE.py:83-84, testing/test_heatmap.py:57-58 call np.random.multivariate_normal on the host and
 * copy the sample to the device once per decode) */
int sln_vae_randn(SlnVae* h, float* out, int64_t n, void* stream);
/* The accumulation of testing/test_heatmap.py:80-99 for all trials in one launch: boxes_pred [n_trials, O, 6] (room row last in
 * every trial) -> counts [O - 1, container_size, container_size] += 1 at (floor(cz (cs - 1)), floor(cx (cs - 1))) of every object
 * centre in the room's own frame (clip_coor: centres clamped to [0, 1]; otherwise trials with a centre outside (0, 1) are dropped). */
int sln_layout_heatmap(const float* boxes_pred, int64_t n_trials, int O, int box_dim, int container_size, int clip_coor, float* counts,
                       void* stream);

/* One iteration of the train.py:62-84 loop on the bound batch: zero_grad, forward, loss, backward and
 * (with_adam == SLN_TRAIN_FULL) the Adam update.  `use_graph`: replay a captured hipGraph while shapes are unchanged
 * (needs a non-default stream).  The data-parallel trainer either calls it with SLN_TRAIN_BACKWARD, all-reduces
 * flat_grads and calls sln_vae_adam_step, or - to overlap the collective with the backward pass - runs the iteration
 * in two halves: SLN_TRAIN_UPTO_DECODER returns (enqueues) everything up to the point where the gradients of the
 * decoder-side parameters are final, SLN_TRAIN_ENCODER_BWD the rest; the all-reduce of the decoder half of flat_grads
 * runs on another stream in between.  `losses_out` is written by every mode except SLN_TRAIN_ENCODER_BWD. */
enum { SLN_TRAIN_BACKWARD = 0, SLN_TRAIN_FULL = 1, SLN_TRAIN_UPTO_DECODER = 2, SLN_TRAIN_ENCODER_BWD = 3 };
/* BatchNorm mode of sln_vae_train_step: 1 (default) = batch statistics + running-stat update, 0 = running statistics as a fixed
 * affine map (train.py:63-65: after --eval_mode_after the reference calls model.eval() and keeps training). */
int sln_vae_set_training(SlnVae* h, int training);
/* Precision of the eval-mode forward Linears (opt-in; DESIGN.md section 4, "A-half").  mode 0 (default): fp32 MFMA, the launches and
 * bits of every earlier version.  1 ("f16"): operands rounded to fp16, one v_mfma_f32_32x32x16_f16 product, fp32 accumulation - a
 * preview mode with its own error budget (tools/vae_half_budget.py).  3 ("f16x3"): fp16 hi / lo split of both operands, three
 * products - fp32-grade while every staged operand lies inside +-65504 (larger values are clamped) and above fp16's subnormal
 * range (lo is subnormal below 2^-14).  Taken by sln_vae_encoder / sln_vae_decoder / sln_vae_forward with training == 0 for the
 * Linears csrc/gemm_half.hip accepts (N % 32 == 0, K % 16 == 0, segment widths % 16 == 0); the narrow heads (box_net.1,
 * angle_net.1, mu / logvar) stay on fp32.  Never taken by training-mode forwards, sln_vae_train_step, any backward pass,
 * sln_vae_group_* (recorded steps), sln_linear_forward or sln_gconv_*.  Any other mode value: SLN_E_BADARG. */
int sln_vae_set_gemm_precision(SlnVae* h, int mode);
int sln_vae_train_step(SlnVae* h, const float* eps, float kl_weight, float lr, float* losses_out, int use_graph,
                       int with_adam, void* stream);

/* R rooms in flight: the decoder of R engines as one launch sequence (layout refinement, testing/test_render_refine.py:250-263:
 * every trial - room - reloads the checkpoint, model.eval(), and :279-359 runs 60 dependent iterations of
 * decoder -> render -> loss -> backward -> SGD on z AND on its own copy of the parameters; trials are independent).
 * `engines`: R handles created and bound by the caller on R parameter copies (sln_vae_create / sln_vae_bind) with their rooms'
 * graphs set (sln_vae_set_batch; the boxes / angles of a decoder-only room are not read); same SlnVaeConfig; eval-mode BatchNorm.
 * The group takes the engines over: their decoder outputs and gradient inputs become slices [row0[r], row0[r] + O_r) of the
 * row-concatenated arrays below, and sln_vae_group_decoder / _backward run sln_vae_decoder(training = 0) /
 * sln_vae_decoder_backward of all rooms - one launch per step for all rooms instead of one per step and room.  A room's results
 * do not depend on R (same kernel bodies, one room per grid slice).  The engines must outlive the group; destroy the group first. */
typedef struct SlnVaeGroup SlnVaeGroup;
typedef struct SlnVaeGroupIO {
  int rows_total;                 /* sum over the rooms of their object rows                                            */
  const int* row0_host;           /* HOST [R]: first row of room r                                                       */
  const float* z;                 /* [rows_total, E]        decoder input, read by every forward                         */
  float* boxes_pred;              /* [rows_total, box_dim]  written by forward                                           */
  float* angles_pred;             /* [rows_total, n_angle]  log-softmax, written by forward, read by backward            */
  float* d_boxes_pred;            /* [rows_total, 8]        gradient w.r.t. boxes_pred, row stride 8 (columns >= box_dim 0) */
  float* d_angles_pred;           /* [rows_total, n_angle]  gradient w.r.t. the log-softmax output                       */
  float* dz;                      /* [rows_total, E]        written by backward                                          */
  const float* sgd_step;          /* optional DEVICE scalar: when set, the wgrads of backward apply  W -= step * dW,  b -= step * db
                                   * to every room's Linear parameters in their epilogue instead of accumulating into the
                                   * gradient buffers (sln_vae_group_fused_params lists the tensors; the caller's optimizer
                                   * steps the others: sln_refine_sgd_rooms over the remaining ranges)                     */
} SlnVaeGroupIO;
/* While a group exists its engines' decoder outputs / gradient inputs are slices of the group's arrays; a failed create and
 * sln_vae_group_destroy put the engines' own buffers back (destroy a group BEFORE its engines). */
int sln_vae_group_create(SlnVae* const* engines, int R, const SlnVaeGroupIO* io, SlnVaeGroup** out);
/* forward also rebuilds W^T of the decoder's weights for the following backward; a backward that is not preceded by a forward of
 * the same group since the last backward (the parameters have been stepped in between) rebuilds it itself.  Parameters changed by
 * the caller BETWEEN a forward and its backward are not noticed. */
int sln_vae_group_decoder(SlnVaeGroup* g, void* stream);
/* parameter gradients are accumulated (+=) into every room's gradient buffer (but see SlnVaeGroupIO::sgd_step), dz is written */
int sln_vae_group_decoder_backward(SlnVaeGroup* g, void* stream);
/* the tensors of ROOM 0's parameter copy that backward steps itself (SlnVaeGroupIO::sgd_step; the same tensors of every room):
 * returns their number, writes at most `max` (pointer, element count) pairs */
int sln_vae_group_fused_params(const SlnVaeGroup* g, const float** params, int64_t* numel, int max);
/* launches per forward / backward pass and how many of them are single-room fallbacks (diagnostics) */
int sln_vae_group_launches(const SlnVaeGroup* g, int* fwd, int* bwd, int* single_room_fallbacks);
/* how many times the group has built W^T of the decoder's weights so far (one per forward, plus one per backward that found none valid) */
int64_t sln_vae_group_transposes(const SlnVaeGroup* g);
void sln_vae_group_destroy(SlnVaeGroup* g);

/* Diagnostics: the pooled side stream the library runs next to `stream` (wgrads of a room group, the depth chain of the scene
 * backward): its index in the per-device pool and whether a probe sees the two streams overlap.  Two streams that share a hardware
 * queue do not - the runtime deals streams to a few queues round-robin - so the library probes once per caller stream and keeps a
 * pooled stream that does (csrc/streams.hip). */
int sln_debug_side_stream(void* stream, int* index, int* overlapped);
/* The probe is a HOST SYNCHRONISATION of `stream` (hipStreamSynchronize + a ~150 us spin kernel per candidate).  Without a prepare call
 * it happens inside the first sln_scene_backward / sln_vae_group_decoder[_backward] on a stream (never inside a capture: a stream first
 * met while captured gets the pool's first stream unprobed).  sln_side_stream_prepare probes now: 1 = a pooled stream overlaps with
 * `stream`, 0 = none (side work runs on `stream`), < 0 error (SLN_E_STATE inside a capture).  A pick is probed again after 4 096
 * look-ups; sln_side_stream_forget drops it (call it before destroying the stream: the next stream with the same handle may sit on
 * another hardware queue); returns the number of entries dropped. */
int sln_side_stream_prepare(void* stream);
int sln_side_stream_forget(void* stream);

/* Per-kernel-family timing with HIP events on the launch stream (bench.py roofline figures).
 * Families: 0 gemm_nt (forward/dgrad), 1 gemm_tn (wgrad), 2 edge scatter/gather, 3 other.
 * enable=1 starts recording (eager launches only, not under graph capture); sln_prof_read
 * synchronises, sums and clears the recorded intervals. work = FLOPs for GEMM families, bytes else. */
int sln_prof_enable(int enable);
/* Deterministic mode (also: environment SLN_DETERMINISTIC=1 at load time).  The reference's CPU path is run-to-run deterministic;
 * the default HIP path adds partial sums with atomics in arrival order (wgrad row chunks, embedding tables, the renderer's face
 * gradients).  With the switch on, every such sum is taken in a fixed order: two runs on the same inputs are bit-identical
 * (scene-graph VAE step and scene backward; cost in DESIGN.md).  Takes effect at the next launch; captured iterations are
 * re-captured. */
int sln_set_deterministic(int on);
int sln_get_deterministic(void);
/* Store policy of the NT GEMM epilogues (also: environment SLN_STORE_POLICY=<bits> at load time).  bit 0 (the default, 1): the
 * forward Linears and dgrads store Y write-through, so the bytes leave the producing XCD's L2 while the launch still runs instead
 * of behind its last workgroup.  0 = plain stores everywhere.  Values never depend on it.  An unknown bit is SLN_E_BADARG and
 * leaves the policy as it was.  The word is process-wide: every single-problem and grouped NT launch reads it when it is ISSUED -
 * the training step, the forward / inference passes, the bare GraphTripleConv calls and the single-launch fallback of a room group
 * (the multi-room NT launches keep plain stores).  Only sln_vae_train_step follows a change through a graph: it drops the iterations
 * it captured under the other word and captures again (sln_debug_vae_graph_captures counts).  A graph a CALLER captured around
 * launches of this library (torch.cuda.graph around a refinement iteration, say) replays the instantiations it recorded: set the
 * policy before capturing.
 * sln_parse_store_policy_env: what the loader makes of a value of the environment variable when `dflt` is the built-in default
 * (host only; NULL, empty, malformed or unknown bits = dflt). */
int sln_set_store_policy(int bits);
int sln_get_store_policy(void);
int sln_parse_store_policy_env(const char* value, int dflt);
/* Split word of the wgrad (TN GEMM) launches (also: environment SLN_TN_SPLIT=0|1 at load time; anything else reads as the default).
 * 1 (the default): a wgrad splits each operand value into three bf16 parts while staging it and sums six products per k-step on
 * the 16-bit matrix pipe into fp32 accumulators - errors of the fp32 route's size at a fifth of its matrix-pipe time.  0: every
 * wgrad on the fp32 matrix pipe.  Which body a problem runs depends on the word, on deterministic mode (always fp32) and on the
 * problem (those that step the parameters in their epilogue, and the multi-room programs' problems, stay fp32) - never on the launch
 * that carries it.  Any other value is SLN_E_BADARG and leaves the word as it was.  Read when a launch is ISSUED, like the store
 * policy; sln_vae_train_step drops the iterations it captured under the other word (sln_debug_vae_graph_captures counts).
 * sln_parse_tn_split_env: what the loader makes of a value of the environment variable (host only). */
int sln_set_tn_split(int word);
int sln_get_tn_split(void);
int sln_parse_tn_split_env(const char* value, int dflt);
/* Test hook (host only, no device work): the workgroup table of the per-pass wgrad launch (csrc/sln_gemm.h: TnMultiMeta) for n
 * problems given as (rows, outputs, inputs).  Returns the number of workgroups (< 0: error), fills rows_per_block[n] and
 * items[3 * workgroup] = (problem or -1 for padding, output tile, row chunk). */
int sln_debug_tn_plan(const int* R, const int* Nout, const int* Kin, int n, int* rows_per_block, int* items, int max_items);
/* The same for the ONE wgrad launch of a whole iteration (gathered and plain problems in one table; 1 <= n <= 128):
 * gathers[i] != 0 marks a problem whose input rows are gathered; items[4 * workgroup] = (problem or -1, output tile, row chunk,
 * gather bit).  -1 also when the list does not fit the table at the target chunk length (the engine then keeps one launch per kind). */
int sln_debug_tn_plan_mixed(const int* R, const int* Nout, const int* Kin, const int* gathers, int n, int* rows_per_block, int* items,
                            int max_items);
int sln_prof_read(double* ms_by_family, double* work_by_family, int64_t* launches_by_family, int n_families);

/* Debug/test tap: copy an internal activation to `dst` (device).  what: 0 A1,1 A2,2 M,3 A3,4 A4 of
 * gconv instance `layer` (0..L-1 encoder, L..2L-1 decoder).  Returns the element count or <0. */
int64_t sln_vae_tap(SlnVae* h, int layer, int what, float* dst, void* stream);

/* GraphTripleConv.forward / GraphTripleConvNet.forward (models/graph.py:57-111,136-143) on their own (inference /
 * feature extraction; training goes through the VAE engine).  units_host: 4 SlnVaeUnit per module in the order
 * net1.0, net1.1, net2.0, net2.1 (gradient fields unused); layer l uses module (n_modules == 1 ? 0 : l).
 * edges [T,2] int64 (s, o).  D % 32 == 0; num_layers > 1 requires Dout == D. */
int64_t sln_gconv_workspace_bytes(int D, int H, int Dout, int O, int T, int num_layers);
int sln_gconv_forward(int D, int H, int Dout, int num_layers, int n_modules, int batch_norm, const SlnVaeUnit* units_host,
                      const float* obj_vecs, const float* pred_vecs, const int64_t* edges, int O, int T, int training, void* workspace,
                      int64_t workspace_bytes, float* new_obj, float* new_pred, void* stream);

/* GraphTripleConvNet on its own WITH autograd (models/graph.py:57-143 is differentiable): an engine handle whose units are
 * the modules' four Linears (net1.0, net1.1, net2.0, net2.1 per module; `recurrent` = one shared module).  Dout != D (a bare
 * GraphTripleConv(input_dim, output_dim), models/graph.py:36-56) needs num_layers == 1.
 * Life cycle: sln_gconv_net_create -> sln_vae_workspace_bytes / sln_vae_bind (SlnVaeTensors: only units_host, with the
 * gradient pointers filled) -> per graph sln_gconv_net_set_edges -> sln_gconv_net_forward -> sln_gconv_net_backward (parameter
 * gradients are accumulated into the units' d_* pointers; input gradients written) -> sln_vae_destroy. */
int sln_gconv_net_create(int D, int H, int Dout, int num_layers, int recurrent, int batch_norm, SlnVae** out);
int sln_gconv_net_set_edges(SlnVae* h, const int64_t* edges, int O, int T, void* stream);
int sln_gconv_net_forward(SlnVae* h, const float* obj_vecs, const float* pred_vecs, float* new_obj, float* new_pred, int training,
                          void* stream);
int sln_gconv_net_backward(SlnVae* h, const float* d_new_obj, const float* d_new_pred, float* d_obj_vecs, float* d_pred_vecs,
                           void* stream);

/* Standalone Linear kernels (parity tests of the GEMM family):
 *   y[M,N] = x[M,K] W[N,K]^T + bias, optional fp64 column sums of y and y^2 in sums[2][N] */
int sln_linear_forward(const float* x, int M, int K, const float* W, const float* bias, float* y, int N, double* sums,
                       int tile, void* stream);
/*   dW[N,K] += g[R,N]^T x[R,K];  db[N] += colsum(g) */
int sln_linear_wgrad(const float* g, const float* x, int R, int N, int K, float* dW, float* db, void* stream);

/* Test hooks of the fused GEMM family (csrc/gemm_f32.hip, gemm_group.hip): an ARBITRARY operand through the engine's own
 * dispatcher.  The descriptions are plain-C mirrors of the argument blocks in csrc/sln_gemm.h / sln_common.h; all pointers are
 * device pointers.  Operand value of logical column c of a segment, row r:
 *     v = max(c0 * x1[r', c1 + c] + c1coef * x2[r', c2 + c] + c2coef, floor),   r' = r | idx_a[r] | idx_b[r]  (which = 0 | 1 | 2)
 * with the coefficients of `coef` (0 identity, 1 BatchNorm forward + ReLU, 2 BatchNorm forward, 3 BatchNorm backward
 * dX = p0 g + p1 x + p2 with g = x1 and x = x2) taken from the segment's BatchNorm view.  The hooks check what the engine
 * guarantees by construction and return SLN_E_BADARG without launching otherwise: 1..3 segments, every len > 0 and a multiple of 4
 * (a segment but the last that is no multiple of 32 puts a boundary inside a k-tile: box_net's form, which only the 64x64 body
 * takes - the dispatcher sends it there), the lens adding up to K (NT) / Nout, Kin (TN), ld / first columns multiples of 4 (rows
 * are read as float4), pointers present where a mode reads them, G never gathered.  1 / n_rows is taken on the host. */
typedef struct SlnDbgBn {
  const double* sums;   /* [2][cstride]: sum x, sum x^2 over n_rows rows (mode 1) */
  const double* gsums;  /* [2][cstride]: sum g, sum g * xhat (coef 3, mode 1) */
  const float* gamma;
  const float* beta;
  const float* rmean;   /* mode 2 */
  const float* rvar;
  int cstride;
  int mode;             /* 0 none, 1 train (statistics from sums), 2 eval (running statistics) */
  float n_rows;
  float eps;
} SlnDbgBn;
typedef struct SlnDbgSeg {
  const float* x1;
  const float* x2;
  int ld1, ld2, c1, c2, len, which, coef, pad_;
  SlnDbgBn bn;          /* aligned with the segment's first column */
} SlnDbgSeg;
typedef struct SlnDbgOperand {
  SlnDbgSeg seg[3];
  const int* idx_a;
  const int* idx_b;
  int nseg, pad_;
} SlnDbgOperand;
/* Y[:, ycol0 .. ycol0 + N) = op(A) W^T + bias + addend[:, addcol0 ..); epi 1: osums[2][ocstride] += column sums of y, y^2;
 * epi 2: y *= [scale * xprev[:, xcol0 + col] + shift > 0] (obn's forward coefficients, aligned with output column 0) and
 * ogsums[2][ocstride] += column sums of y, y * xhat.  tile: -1 the dispatcher's choice, 0 / 1 / 2 = 64x64 / 128x64 / 128x128. */
typedef struct SlnDbgGemmNT {
  SlnDbgOperand A;
  const float* W;
  const float* bias;
  float* Y;
  const float* addend;
  const float* xprev;
  double* osums;
  double* ogsums;
  SlnDbgBn obn;
  int M, N, K, ldw, ldy, ycol0, ldadd, addcol0, ocstride, ldx, xcol0, epi, tile, pad_;
} SlnDbgGemmNT;
/* dW[Nout, Kin] += op(G)^T op(X), db += colsum(op(G)); with sgd_step (device pointer to the step) dW / db are the PARAMETERS and
 * receive -step * (the gradient).  rows_per_block <= 0: the launcher's choice. */
typedef struct SlnDbgGemmTN {
  SlnDbgOperand G, X;
  float* dW;
  float* db;
  const float* sgd_step;
  int lddw, R, Nout, Kin, rows_per_block, pad_;
} SlnDbgGemmTN;
/* body: 0 64x64, 1 128x64, 2 128x128, 3 16x16-MFMA J = 3, 4 16x16-MFMA J = 5, 5 32x32 split-K one segment, 6 32x32 split-K
 * three segments; multi: 0 one segment, 1 boundaries on k-tiles, 2 a boundary inside a k-tile; amode: 0 per-column affine,
 * 1 two sources, 2 identity; threads: workgroup size (512 with helper wavefronts). */
typedef struct SlnDbgNTRoute { int body, multi, amode, threads; } SlnDbgNTRoute;
/* n = 1: sln_launch_gemm_nt.  n = 2: the grouped launch, and two separate launches when the pair cannot share a kernel - as the
 * engine does; *grouped (may be NULL) then says which happened. */
int sln_debug_gemm_nt(const SlnDbgGemmNT* desc, int n, int* grouped, void* stream);
/* multi == 0 (n must be 1): sln_launch_gemm_tn.  multi != 0 (1 <= n <= 64): the planner and the one-launch-per-pass kernel; the
 * problem table lives in device memory the hook owns and frees after synchronising the stream. */
int sln_debug_gemm_tn(const SlnDbgGemmTN* desc, int n, int multi, void* stream);
/* The iteration's one wgrad launch on caller-built problems (1 <= n <= 128): problems that gather their input rows and problems that
 * do not (their index arrays may be NULL) share one grid, each workgroup running the body its problem needs.  Here the last
 * segment of an operand may have a length that is no multiple of 4 when its rows are stored up to the next multiple (ld >= c +
 * the rounded length): the engine's box_net.1 gradient, 6 columns in rows of 8. */
int sln_debug_gemm_tn_mixed(const SlnDbgGemmTN* desc, int n, void* stream);
/* Host only: the kernel sln_launch_gemm_nt would run for this description (the launcher's own decision function). */
int sln_debug_gemm_nt_route(const SlnDbgGemmNT* desc, SlnDbgNTRoute* out);
/* The fp16-MFMA launcher (csrc/gemm_half.hip) on a caller-built problem; terms: 1 = "f16", 3 = "f16x3".  SLN_E_UNSUPPORTED, with
 * nothing launched, when its route predicate refuses the description (tile is not read). */
int sln_debug_gemm_nt_half(const SlnDbgGemmNT* desc, int terms, void* stream);
/* Host only: 1 when the fp16-MFMA launcher takes the description, 0 when it refuses, SLN_E_BADARG for a malformed one. */
int sln_debug_gemm_nt_half_takes(const SlnDbgGemmNT* desc);
/* sizeof of the description structs, in the order SlnDbgBn, SlnDbgSeg, SlnDbgOperand, SlnDbgGemmNT, SlnDbgGemmTN, SlnDbgNTRoute;
 * returns how many there are (fills at most max). */
int sln_debug_gemm_sizes(int* out, int max);

/* Test hooks of the VAE path's non-GEMM kernels (csrc/vae_kernels.hip) through their own launchers (csrc/vae_debug.hip).  All
 * pointers are device pointers the caller allocates.  The hooks return SLN_E_BADARG without launching for what the launchers
 * assume by construction (pointers present where a form reads them, positive widths, strides that hold the logical width,
 * statistics strides that hold the columns); a misaligned edge argument is passed on and comes back as the launcher's own -2. */
typedef struct SlnDbgCsr {   /* GraphCsr: s, p, o [T]; deg, invdeg, cursor [O]; rowptr [O + 1]; ent [2 T] */
  int* s; int* p; int* o; int* deg; float* invdeg; int* rowptr; int* cursor; int* ent;
  int T, O;
} SlnDbgCsr;
/* sln_launch_graph_prep: triples [T, 3] int64 (s, p, o), or edges [T, 2] (s, o) with edges_only; deg_is_zero: the caller has
 * cleared deg.  *err (may be NULL) receives bit 1 for an id out of range. */
int sln_debug_vae_csr(const int64_t* triples, int num_preds, int edges_only, int deg_is_zero, const SlnDbgCsr* g, int* err, void* stream);
/* kind 0 scatter_avg_fwd: out[O = rows, H] from a = A2 (lda), bn, g
 *      1 scatter_avg_bwd: out = g2 [T = rows, ldc] from a = dM [O, H], b = dP (ldb, first column col0; may be NULL), c = A2 (ldc)
 *      2 gather_bwd:      out (ldo) [O = rows, D] from a = dG (lda), b = add1 (ldb; may be NULL), c = xprev (ldc), masked
 *      3 mask_gstats:     out (ldo) [rows, cols] from a = d1 (lda), b = d2 (ldb; may be NULL), c = xprev (ldc)
 *      4 bn_relu_apply:   out (ldo) [rows, cols] = relu(bn(a[:, col0 + c]))
 *      5 add2:            out (ldo) [rows, cols] = a + b
 * gsums [2][cstride] (may be NULL) receives += the column sums of the result and of result * xhat (kinds 1, 2 masked, 3). */
typedef struct SlnDbgEdge {
  SlnDbgCsr g;
  SlnDbgBn bn;
  const float* a; const float* b; const float* c;
  float* out;
  double* gsums;
  int kind, lda, ldb, ldc, ldo, H, D, rows, cols, col0, cstride, masked;
} SlnDbgEdge;
/* multi == 0 (n must be 1): the single-room launcher.  multi != 0 (kinds 0, 1, 2, 3, 5; 1 <= n <= 64 rooms of one kind): the
 * planner per room and ONE *_multi launch off a room table in device memory the hook owns and frees after synchronising the
 * stream; rooms whose planners disagree on the variant are refused with SLN_E_UNSUPPORTED (the engine splits such a step).
 * *variant (may be NULL): what the planner chose, -1 for the single-room launch. */
int sln_debug_vae_edge(const SlnDbgEdge* desc, int n, int multi, int* variant, void* stream);
/* kind 0 loss (LossArgs); 1 log_softmax: angles_pred = log_softmax(logits); 2 log_softmax_bwd: d_logits from angles_pred and
 * d_logprob; 3 latent_bwd: dmu, dlogvar from mu, logvar, eps, dz, kl_weight */
typedef struct SlnDbgLoss {
  const float* boxes; const float* boxes_pred; const int64_t* angles; const float* logits; float* angles_pred;
  const float* mu; const float* logvar; const float* eps; const float* dz; const float* d_logprob; const float* kl_weight;
  double* acc; float* losses; float* d_boxes_pred; float* d_logits; float* dmu; float* dlogvar;
  int kind, O, box_dim, n_angle, n_z, use_ae, ld_dbp, acc_prezeroed, from_logits, pad_;
} SlnDbgLoss;
int sln_debug_vae_loss(const SlnDbgLoss* desc, void* stream);
typedef struct SlnDbgBnEntry {   /* BnTableEntry; rows -1 / -2: rows_t / rows_o of the call */
  const double* sums; const double* gsums; float* rmean; float* rvar; int64_t* nbt; float* dgamma; float* dbeta;
  int cstride, C, rows, pad_;
} SlnDbgBnEntry;
typedef struct SlnDbgTranspose { const float* src; float* dst; int rows, cols, dst_ld, pad_; } SlnDbgTranspose;   /* dst[c * dst_ld + r] = src[r * cols + c] */
/* kind 0 bn_running_update, 1 bn_param_grads (entries: SlnDbgBnEntry [n], width: the largest C), 2 transpose_table (entries:
 * SlnDbgTranspose [n], width: max_tiles).  `entries` is a HOST array; the hook uploads the table and frees it after synchronising. */
int sln_debug_vae_tables(int kind, const void* entries_host, int n, int width, float momentum, int independent, int rows_t, int rows_o,
                         void* stream);
/* The embedding group.  kind 0 enc_assemble:     x0 [O, n_obj + n_attr + n_box + n_angle] (n_attr == 0: no attribute columns)
 *      1 enc_assemble_bwd: the three tables, d_wb [n_box, box_dim] and d_bb [n_box] += from dx0; rows_* are the tables' row counts
 *                          (all > 0 and at most 10 240 floats of tables: accumulated in LDS first; 0: plain atomics)
 *      2 dec_assemble:     z [O, n_z] (may be NULL) = z_in, or mu (use_ae), or eps * exp(logvar / 2) + mu; x0 = [obj | attr | z]
 *                          (z_in_x0 == 0: x0 = [obj | attr])
 *      3 dec_assemble_bwd: the two tables += from dx0, dz [O, n_z] (may be NULL) = its z columns when z_in_x0
 *      4 embed_gather_i32: dst [O, n] = src[idx[r], :]               (idx int32 [O])
 *      5 embed_bwd_i32, 6 embed_bwd_i64: dst[idx[r], :] += src[r, col0 : col0 + n] (row stride ld); table_rows > 0 allows the
 *                          LDS form (table_rows * n <= 8 192) and the deterministic one (sln_set_deterministic)
 *      7 i64_to_i32:       dst int32 [O] = idx int64 [O]
 *      8 stage_batch:      st_* = copies of objs / attrs / angles / boxes, attrs32, deg = 0, *err |= 2 / 4 / 8 for an object class /
 *                          attribute / angle bin outside rows_obj / rows_attr / rows_angle (rows_attr == 0: attributes not looked at)
 *      9 validate_ids:     *err as above (angles may be NULL)
 * The index VALUES are the caller's to keep inside the tables: the hooks cannot see them.  T, src2, dst2, n2, zero_ptr and
 * zero_bytes belong to the step prologue (sln_debug_vae_opt, kind 2) only. */
typedef struct SlnDbgEmbed {
  const int64_t* objs; const int64_t* attrs; const int64_t* angles; const float* boxes;
  const float* obj_emb; const float* attr_emb; const float* angle_emb; const float* wb; const float* bb;
  const float* mu; const float* logvar; const float* eps; const float* z_in; float* z;
  float* x0; const float* dx0;
  float* d_obj_emb; float* d_attr_emb; float* d_angle_emb; float* d_wb; float* d_bb; float* dz;
  const void* idx; const float* src; void* dst; const float* src2; void* dst2;
  int64_t* st_objs; int64_t* st_attrs; int64_t* st_angles; float* st_boxes; int* attrs32; int* deg; int* err;
  void* zero_ptr; int64_t zero_bytes;
  int kind, O, n_obj, n_attr, n_box, n_angle, box_dim, n_z, use_ae, z_in_x0, rows_obj, rows_attr, rows_angle, ld, col0, n, table_rows,
      T, n2, pad_;
} SlnDbgEmbed;
/* multi as in sln_debug_vae_edge (kinds 2 - 6): the planner per room, one *_multi launch.  *variant: MV_ASM_BWD_* (kind 3),
 * MV_EMBED_* (+ 4 for int64 indices; kinds 5, 6), 0 (kinds 2, 4); a planner that has no multi form for a room (deterministic mode or
 * more than 8 192 rows in kind 3) and rooms of different variants are refused with SLN_E_UNSUPPORTED. */
int sln_debug_vae_embed(const SlnDbgEmbed* desc, int n, int multi, int* variant, void* stream);
/* kind 0 adam (params, grads, m, v [n]; total_loss may be NULL), 1 randn (params = the output [n]), 2 step_prologue (params = eps [n],
 * may be NULL: no draw; pro = the encoder assembly as in kind 0 of SlnDbgEmbed, plus p0e [T, n] = src[idx] and p0d [T, n2] =
 * src2[idx] into dst / dst2 (idx int32 [T]; T may be 0) and zero_bytes (a multiple of 16) cleared at zero_ptr (16-byte aligned; may be
 * NULL)).  The hook owns a device AdamScalars filled from step .. offset, makes `calls` launches in a row on it and reports its
 * contents afterwards. */
typedef struct SlnDbgOpt {
  float* params; const float* grads; float* m; float* v; const float* total_loss; const SlnDbgEmbed* pro;
  int64_t n, step;
  uint64_t seed, offset;
  float lr, beta1, beta2, eps;
  int kind, calls;
  int64_t out_step; uint64_t out_offset; float out_bc1, out_bc2; int out_skip, pad_;
} SlnDbgOpt;
int sln_debug_vae_opt(SlnDbgOpt* desc, void* stream);
/* sizeof of SlnDbgCsr, SlnDbgEdge, SlnDbgLoss, SlnDbgBnEntry, SlnDbgTranspose, SlnDbgOpt, SlnDbgEmbed; returns how many there are. */
int sln_debug_vae_sizes(int* out, int max);
/* How many times an engine issued the one-launch form of an iteration's leaf kernels (embedding-table, box-embedding and
 * BatchNorm bookkeeping gradients deferred to the end of a full iteration); 0 while it keeps the per-kernel sequence
 * (SLN_LEAF_MERGE=0, deterministic mode, tables past the LDS caps, the two-half form).  A captured iteration counts once.  The
 * jobs count whether they ran as a launch of their own or as trailing workgroups of the iteration's wgrad launch (below). */
int64_t sln_debug_vae_leaf_launches(const SlnVae* h);
/* Running count of the iterations whose wgrads ran as ONE launch (gathered and plain problems in one table); 0 while an engine
 * keeps one launch per kind (SLN_TN_MIXED=0, SLN_NO_MERGE=1, SLN_LEAF_MERGE=0, deterministic mode, shared 'recurrent' weights,
 * the two-half form, a problem list past the table).  A captured iteration counts once.  By default the leaf jobs and the
 * decoder's assembly backward ride in that launch (SLN_TN_MIXED=1: neither, =2: the leaf jobs only). */
int64_t sln_debug_vae_tail_launches(const SlnVae* h);
/* Running count of the iterations sln_vae_train_step captured into a graph for this engine (first use of a mode, a new batch shape,
 * and every change that drops the captured iterations: deterministic mode, the store policy, the eps source, ...). */
int64_t sln_debug_vae_graph_captures(const SlnVae* h);
/* Running count of the fp16-MFMA Linear launches an engine issued (sln_vae_set_gemm_precision). */
int64_t sln_debug_vae_half_launches(const SlnVae* h);


/* =============================================================================================
 * B. Differentiable rasterizer  (third-party `neural_renderer`, un-vendored; reference call sites
 *    models/misc.py:7, models/diff_render.py:359-361 (ctor), :366 (mode='depth'), :398 (mode="rgb"))
 *
 * The host mirror does the camera projection / fill_back / vertices_to_faces with torch ops; the C ABI
 * starts at faces[B, F, 3, 3] fp32 = (x_ndc, y_ndc, z_cam) of the three vertices of every face.
 * All maps are [B, is, is] in RASTER order (row 0 = bottom; the package flips rows afterwards).
 * ============================================================================================= */
/* neural_renderer.projection (K [B,3,3], R [B,3,3], t [B,1,3], orig_size; dist_coeffs dropped as the reference README asks,
 * README.md:12-18) followed by vertices_to_faces: faces_xyz [B,F,3,3] = (x_ndc, y_ndc, z_cam) per corner; and its adjoint. */
int sln_project_faces(const float* vertices, const int32_t* faces, const float* K, const float* R, const float* t, int B, int V, int F,
                      float orig_size, float eps, float* faces_xyz, void* stream);
int sln_project_faces_backward(const float* vertices, const int32_t* faces, const float* K, const float* R, const float* t, int B, int V,
                               int F, float orig_size, float eps, const float* grad_faces_xyz, float* grad_vertices, void* stream);
int64_t sln_raster_workspace_bytes(int B, int F);
/* rasterize / rasterize_depth: face_index int32 (-1 = background), weight [B,is,is,3], depth (far where empty) */
int sln_raster_forward(const float* faces, int B, int F, int image_size, float near, float far, void* workspace,
                       int32_t* face_index, float* weight, float* depth, void* stream);
/* one geometry pass, two z-buffers with different near planes (depth pass 0.1 / rgb passes ctor value) */
int sln_raster_forward_dual(const float* faces, int B, int F, int image_size, float near_a, float near_b, float far,
                            void* workspace, int32_t* fi_a, float* w_a, float* d_a, int32_t* fi_b, float* w_b,
                            float* d_b, void* stream);
/* forward_texture_sampling: textures [B,F,ts,ts,ts,3] -> rgb [B,is,is,3] (background 0).  The index map is an operand: any values in
 * [-1, F) are legal (not only a map sln_raster_forward wrote); anything else is the caller's error - the kernel forms the face and
 * texture addresses from the map and tests only its sign. */
int sln_raster_texture_sample(const float* faces, const float* textures, const int32_t* face_index, const float* weight,
                              const float* depth, int B, int F, int image_size, int texture_size, float eps, float* rgb,
                              void* stream);
/* backward_depth_map: grad_faces[B,F,3,3] += ... (atomics) */
int sln_raster_backward_depth(const float* faces, const int32_t* face_index, const float* weight, const float* depth,
                              const float* grad_depth, int B, int F, int image_size, float* grad_faces, void* stream);
/* backward_pixel_map for a `channels`-channel image rgb/grad_rgb [B,is,is,channels]: grad_faces += ... */
int sln_raster_backward_rgb(const float* faces, const int32_t* face_index, const float* rgb, const float* grad_rgb, int B,
                            int F, int image_size, int channels, float eps, float* grad_faces, void* stream);
/* Renderer.__call__(mode="rgb") (models/diff_render.py:398) behind cached maps, one launch: forward_texture_sampling + ambient
 * light (factor `scale`) + the package's permute / row flip -> rgb_chw [B,3,is,is].  textures [B,F_tex,ts,ts,ts,3] with
 * F_tex == F, or F_tex == F / 2 for fill_back: face f >= F_tex samples cube f - F_tex with texture axes 0 and 2 swapped
 * (the package's torch.cat((textures, textures.permute((0, 1, 4, 3, 2, 5))), dim=1)).  The index map is an operand here too: any
 * values in [-1, F) are legal, anything else is the caller's error (tests/test_raster_texture_chw_gpu.py holds both halves: a
 * random in-range map, and a host check of every map before the launch). */
int sln_raster_texture_sample_chw(const float* faces, const float* textures, const int32_t* face_index, const float* weight,
                                  const float* depth, int B, int F, int F_tex, int image_size, int texture_size, float eps, float scale,
                                  float* rgb_chw, void* stream);
/* backward_pixel_map of P <= 64 rgb passes rendered over the SAME face-index map (the 32 class passes of mesh_render_func,
 * models/diff_render.py:381-398, back-propagated together): grad_faces += sum over the passes of the package's per-pass
 * gradient, in one edge walk.  rgb_chw / grad_chw: device arrays of P device pointers to [B,3,is,is] images as returned by
 * sln_raster_texture_sample_chw / handed back by autograd; mask_ws: 8 * B * is * is bytes of scratch. */
int sln_raster_backward_rgb_multi(const float* faces, const int32_t* face_index, const float* const* rgb_chw,
                                  const float* const* grad_chw, int P, int B, int F, int image_size, float eps, void* mask_ws,
                                  float* grad_faces, void* stream);

/* Fused scene pass = models/diff_render.py:359-434 (1 depth + one rgb pass per class, masks, per-class mean
 * depth, wall_max normalisation, 70-channel layout) in ONE rasterisation.
 *   face_class [B,F] int32: class id (0 = wall, ids follow the reference's sorted class list) or -1
 *   class_channel [num_classes]: NYU-40 index of each class (final channel 1 + index)
 *   class_depth_channel [num_classes]: index into the 29 depth channels (final channel 41 + index) or -1
 *   final_out [B,70,is,is] image order (rows flipped), grad_faces [B,F,3,3] (overwritten). */
int64_t sln_scene_workspace_bytes(int B, int F, int image_size);
int sln_scene_forward(const float* faces, const int32_t* face_class, int B, int F, int image_size, int num_classes,
                      const int32_t* class_channel, const int32_t* class_depth_channel, float near_depth, float near_rgb,
                      float far, float tex_eps, void* workspace, float* final_out, void* stream);
/* sln_scene_forward for a consumer that reads the image through its flags (SlnRefineLoss::live_planes): `live` [B, 70] receives
 * the flags described below, and only the planes flagged 3 of final_out are written (a plane flagged 0 would hold zeros, a plane
 * flagged 1 the constant 1: their memory is left as it was). */
int sln_scene_forward_live(const float* faces, const int32_t* face_class, int B, int F, int image_size, int num_classes,
                           const int32_t* class_channel, const int32_t* class_depth_channel, float near_depth, float near_rgb,
                           float far, float tex_eps, void* workspace, float* final_out, unsigned char* live,
                           unsigned char* null_mask /* optional [B, S, S]: SlnRefineLoss::null_mask */, void* stream);
/* live [B, 70] (bytes) of the last sln_scene_forward on `workspace`, two bits per channel: bit 0 clear = the plane is all zeros
 * (semantic channels of classes without a visible pixel in that image), bit 1 clear = sln_scene_backward never reads the
 * plane's gradient (those, and the depth-hot planes of such classes, which hold the constant 1).  The refinement loss skips
 * what the bits allow (SlnRefineLoss::live_planes). */
int sln_scene_live_channels(void* workspace, int B, int F, int image_size, int num_classes, const int32_t* class_channel,
                            const int32_t* class_depth_channel, unsigned char* live, void* stream);
int sln_scene_backward(const float* faces, const int32_t* face_class, int B, int F, int image_size, int num_classes,
                       const int32_t* class_channel, const int32_t* class_depth_channel, float pix_eps, void* workspace,
                       const float* grad_final, float* grad_faces, void* stream);


/* Object placement of mesh_render_func for one room with device-resident meshes (models/diff_render.py:76-159), fused with
 * the projection (as sln_project_faces), the near-plane cull (:346-356, culled faces are degenerated to a point) and
 * fill_back: boxes [n,6] (room-normalised rows, visible object k is row vis[k]), angles [n] (bins, fractional) ->
 * faces_out [2F,3,3] = (x_ndc, y_ndc, z_cam) (faces F..2F-1: corners (2,1,0)), sizes [n_vis,3], size_loss [1] =
 * sum_k mean_j (size - size_target)^2 (0 when size_target is NULL).  The face list is grouped by object (obj_face_ptr
 * [n_vis+1], the room shell's faces last); object faces index model_v [n_vis*Vm,3], shell faces n_vis*Vm + shell_v [Vs,3].
 * backward: grad_faces [2F,3,3], grad_size_loss [1] (device, may be NULL) -> grad_boxes [n,6], grad_angles [n]. */
typedef struct {
  int n, n_vis, Vm, Vs, F, reserved;
  const int32_t* vis; const float* model_v; const float* msize; const float* mcenter; const float* shell_v;
  const int32_t* faces; const int32_t* obj_face_ptr;
  float ext[3];                    /* room extent (boxes[-1][3:]) */
  float K[9], R[9], t[3];          /* camera of get_cam_mat (diff_render.py:13-46) */
  float orig_size, proj_eps, cull_eps;
} SlnPlacement;
int sln_place_forward(const SlnPlacement* P /* host struct */, const float* boxes, const float* angles, const float* size_target,
                      float* faces_out, float* sizes, float* size_loss, void* stream);
int sln_place_backward(const SlnPlacement* P, const float* boxes, const float* angles, const float* size_target, const float* grad_faces,
                       const float* grad_size_loss, float* grad_boxes, float* grad_angles, void* stream);

/* The tensor glue between the decoder and the placement in one launch each way (testing/test_render_refine.py:296-306):
 *   boxes_full [n,6] = [boxes_pred[:-1] ; box_last],  idx [n] = [softargmax(angles_pred, beta)[:-1] + noise[:-1] / 10 ; angle_last[0]]
 * with softargmax(x) = sum_j softmax(beta * x)_j * (j + 1) - 1 (:20-25); noise may be NULL.  backward folds the reference's two
 * gradient hooks in: quad_grad (d idx * 4, :226-228) and fix_grad (both halves of a box row get the mean of their two
 * gradients, :217-224); the frozen last row gets zero gradients.  grad_boxes_pred [n,6], grad_angles_pred [n,n_angle]. */
int sln_refine_head_forward(int n, int n_angle, const float* boxes_pred, const float* angles_pred, const float* noise,
                            const float* box_last, const float* angle_last, float beta, float* boxes_full, float* idx, void* stream);
int sln_refine_head_backward(int n, int n_angle, const float* angles_pred, const float* grad_boxes_full, const float* grad_idx,
                             float beta, float* grad_boxes_pred, float* grad_angles_pred, void* stream);
/* params -= step * grads; grads = 0; z -= step_z * grad_z  (one launch).  The reference builds a NEW SGD(momentum=0.1,
 * nesterov=True) every iteration (:286-292), whose single step is p -= lr * 1.1 * grad: pass step = lr * 1.1.
 * params / grads 16-byte aligned. */
int sln_refine_sgd(float* params, float* grads, int64_t n, float step, float* z, const float* grad_z, int64_t nz, float step_z,
                   void* stream);

/* ---- R rooms per launch (the rooms of testing/test_render_refine.py:250-263 are independent: one iteration of all of them) ----
 * Rows of all rooms concatenated (rows_total); room_of_row [rows_total] int32; last_row [R] = the room's frozen last row.
 * head forward / backward as sln_refine_head_forward / _backward per room: box_last [R,6], angle_last [R]; the backward writes
 * grad_boxes_pred with row stride ld_gb (8 = the engine's padded gradient layout, the padding columns are zeroed). */
int sln_refine_head_forward_rooms(int rows_total, int n_angle, const int32_t* room_of_row, const int32_t* last_row, const float* boxes_pred,
                                  const float* angles_pred, const float* noise, const float* box_last, const float* angle_last, float beta,
                                  float* boxes_full, float* idx, void* stream);
int sln_refine_head_backward_rooms(int rows_total, int n_angle, const int32_t* room_of_row, const int32_t* last_row, const float* angles_pred,
                                   const float* grad_boxes_full, const float* grad_idx, float beta, float* grad_boxes_pred, int ld_gb,
                                   float* grad_angles_pred, void* stream);
/* sln_place_forward / _backward of R rooms in one launch each: `rooms` is a DEVICE array of R blocks (the room's descriptor and its
 * tensors); F_max / n_max the largest face / row count (grid sizing). */
typedef struct {
  SlnPlacement P;
  const float* boxes; const float* angles; const float* size_target;      /* [n,6], [n], [n_vis,3] or NULL */
  float* faces_out; float* sizes; float* size_loss;                        /* [2F,3,3], [n_vis,3], [1] */
  const float* grad_faces; const float* grad_size_loss; float* grad_boxes; float* grad_angles;   /* backward */
  /* optional head (boxes_pred != NULL; needs P.n <= 128): the two placement launches then do sln_refine_head_forward / _backward of
   * the room themselves - forward derives `boxes` / `angles` from the decoder's outputs (and stores them there), backward turns
   * grad_boxes / grad_angles into the gradients of the decoder's outputs - with the stand-alone kernels' arithmetic */
  const float* boxes_pred; const float* angles_pred; const float* noise;     /* [n,6], [n,n_angle] log-softmax, [n] or NULL */
  int* noise_step; int64_t noise_stride;                                      /* optional device counter k: forward reads noise + k * noise_stride,
                                                                               * backward (room 0 of the launch) advances it by one */
  const float* box_last; const float* angle_last;                             /* [6], [1]: the frozen last row */
  float* grad_boxes_pred; float* grad_angles_pred;                            /* [n,ld_gb], [n,n_angle] */
  int n_angle, ld_gb; float beta; int pad_;
} SlnPlacementRoom;
int sln_place_forward_rooms(const SlnPlacementRoom* rooms /* device */, int R, int F_max, void* stream);
int sln_place_backward_rooms(const SlnPlacementRoom* rooms /* device */, int R, int n_max, void* stream);
/* Several target views per room: the placement of sln_place_forward / _backward_rooms (models/diff_render.py:76-159, once per room)
 * projected through V cameras per room instead of get_cam_mat's one (:13-46; the projection, the cull :346-356 and fill_back per view).
 * Image b = r * V + v; `cams` is a DEVICE array [R * V] in get_cam_mat's convention (p_cam = R p_world + t, K in pixels of orig_size).
 * A room's faces_out / grad_faces point at its view 0; view v lies v * view_stride floats behind it.  P.K / P.R / P.t and the head
 * fields of the table are not read (boxes / angles are).  A face culled in a view is (0, 0, 0) in that view only and adds nothing
 * to the gradients from it; face rows beyond a room's 2 P.F stay untouched in every view.  sizes / size_loss / the size-loss
 * gradient once per room; grad_boxes / grad_angles = the sum over the views, one writer per row, no atomics.  With V = 1 and the room's
 * own camera in `cams`: the bits of sln_place_forward_rooms / sln_place_backward_rooms.  One launch each, no allocation, no
 * synchronisation: legal in a linear capture.  SLN_E_BADARG, nothing launched: a null pointer, R < 1, V < 1, V > SLN_PLACE_MAX_VIEWS,
 * F_max < 1 / n_max < 1, view_stride < 18. */
#define SLN_PLACE_MAX_VIEWS 64
typedef struct { float K[9], R[9], t[3]; } SlnPlacementCamera;
int sln_place_forward_views(const SlnPlacementRoom* rooms /* device [R] */, const SlnPlacementCamera* cams /* device [R * V] */, int R, int V,
                            int F_max, int64_t view_stride, void* stream);
int sln_place_backward_views(const SlnPlacementRoom* rooms, const SlnPlacementCamera* cams, int R, int V, int n_max, int64_t view_stride,
                             void* stream);
/* Refinement of the camera poses of the target views (DESIGN §4 "Camera poses of the target views"; the camera of
 * models/diff_render.py:13-46, the cull of :346-356).  Issued AFTER sln_place_backward_views of the iteration, on the same operands:
 * per (room, view) the camera-space adjoint of every corner of every face the view keeps (sln_place_backward_views' own, before its
 * multiplication by R; the shell's faces count) is reduced to the gradient of a rigid motion applied in the camera frame,
 * p_cam' = exp([w]x) p_cam + tau, at w = tau = 0:  grad_pose [R * V, 6] = (sum p_cam x g_cam, sum g_cam), float64 sums of float32 products,
 * written on every call.  A view with pose_free != 0 (NULL: every view) is then moved by w = -rot_step dL/dw, tau = -trans_step dL/dtau:
 * R <- E R, t <- E t + tau with E = exp([w]x), in the float64 master `pose` [R * V, 12] (R row-major, then t; the caller fills it with
 * double(cams entry)), and the view's cams entry receives the float32 rounding of the master's R and t.  K is never written; with both
 * steps 0, or for a view that is not free, neither pose nor cams is written.  grad_faces carries the loss's 1 / V: the gradient is that
 * of the ROOM's loss.  Grid (V, R), one writer per (room, view), no atomics, no allocation, no synchronisation: legal in a linear
 * capture.  SLN_E_BADARG, nothing launched: a null rooms / cams / pose / grad_pose, R < 1, V < 1, V > SLN_PLACE_MAX_VIEWS,
 * view_stride < 18, a negative or non-finite step. */
int sln_place_pose_step_views(const SlnPlacementRoom* rooms /* device [R] */, SlnPlacementCamera* cams /* device [R * V], updated in place */,
                              double* pose /* device [R * V, 12] */, double* grad_pose /* device [R * V, 6]: d omega, d tau */,
                              const uint8_t* pose_free /* device [R * V] or NULL = all */, int R, int V, int64_t view_stride,
                              float rot_step, float trans_step, void* stream);
/* Refinement of the intrinsics of the target views together with their poses (DESIGN §4 "Intrinsics of the target views"): ONE launch in
 * the place of sln_place_pose_step_views, since two launches would each read the camera the other has just overwritten.  Per (room,
 * view), over the corners that sln_place_pose_step_views sums, with (gu, gv) a corner's image gradient, s2 = 2 / orig_size and
 * xh = x / (z + proj_eps), yh = y / (z + proj_eps) its normalised camera coordinates:
 *   grad_intr [R * V, 4] = (dL/dfx, dL/dfy, dL/dcx, dL/dcy) = (sum s2 gu xh, sum -s2 gv yh, sum s2 gu, sum -s2 gv)
 * for fx = K[0], fy = K[4], cx = K[2], cy = K[5]: float64 sums of float32 products, written on every call like grad_pose, which has
 * sln_place_pose_step_views' bits.  The pose update is that entry point's, from the same arguments.  A view with intr_free != 0 (NULL:
 * every view) is then stepped in the float64 master `intr` [R * V, 4] = (fx, fy, cx, cy), which the caller fills with double(cams entry):
 *   fx <- fx exp(sx), fy <- fy exp(sy);  sx = -focal_step fx dL/dfx, sy = -focal_step fy dL/dfy, or with tie_focal != 0 the one log-scale
 *   sx = sy = -focal_step (fx dL/dfx + fy dL/dfy);  sx, sy are held to [-SLN_FOCAL_LOG_MAX, SLN_FOCAL_LOG_MAX];
 *   cx <- cx - center_step dL/dcx, cy <- cy - center_step dL/dcy   (pixels of orig_size)
 * and K[0], K[4], K[2], K[5] of the view's cams entry receive the float32 rounding of the master.  Both updates use the gradients of
 * the camera the call found.  K[1], K[3] and K[6..8] are read and never written; with focal_step == center_step == 0, or for a view that
 * is not intr_free, neither intr nor any K entry is written.  intr, grad_intr and intr_free may be NULL together: the call is then
 * sln_place_pose_step_views.  One writer per (room, view), no atomics, no allocation, no synchronisation: legal in a linear capture.
 * SLN_E_BADARG, nothing launched: what sln_place_pose_step_views refuses, intr without grad_intr or the reverse, intr_free without intr,
 * a negative or non-finite focal_step / center_step. */
#define SLN_FOCAL_LOG_MAX 1.0
int sln_place_camera_step_views(const SlnPlacementRoom* rooms /* device [R] */, SlnPlacementCamera* cams /* device [R * V], updated in place */,
                                double* pose /* device [R * V, 12] */, double* grad_pose /* device [R * V, 6] */,
                                const uint8_t* pose_free /* device [R * V] or NULL = all */, double* intr /* device [R * V, 4] or NULL */,
                                double* grad_intr /* device [R * V, 4] or NULL */, const uint8_t* intr_free /* device [R * V] or NULL = all */,
                                int R, int V, int64_t view_stride, float rot_step, float trans_step, float focal_step, float center_step,
                                int tie_focal, void* stream);
/* sln_refine_sgd over R parameter copies: for every room r and every range k: p[r * stride + off_k + i] -= step * g[...], g = 0
 * (i < len_k; off_k, len_k multiples of 4 floats; n_ranges <= 96: the decoder's parameters are the three *_dc embedding tables in
 * front and the trailing gconv_net_dc / box_net / angle_net run - encoder-only parameters have zero gradients in this loop and are
 * not touched - or, with SlnVaeGroupIO::sgd_step, what is left of those runs between the Linear tensors the wgrads step
 * themselves); z [nz] -= step_z * grad_z. */
int sln_refine_sgd_rooms(float* params, float* grads, int R, int64_t stride, const int64_t* off_host, const int64_t* len_host, int n_ranges,
                         float step, float* z, const float* grad_z, int64_t nz, float step_z, void* stream);

/* Refinement loss of the layout-refinement loop (testing/test_render_refine.py:192-215 PSP_pool_new, :332-356):
 * null-fill of the last depth channel, bilinear(align_corners=True) resampling of the 40 semantic and 29 depth channels of
 * the [B,70,S,S] scene tensor to each scale and bilinear resampling to pooled_size, L1 against the pooled target depth * 0.5,
 * sum over the scales of cross-entropy against the target's labels / 800;  loss_out = {100 * depth + 100 * sem, depth, sem}
 * (the caller adds 2 * size_loss; per_room: one such triple per image).  All table pointers are DEVICE arrays the caller builds once per geometry:
 *   stage 2 (scale -> pooled, align_corners=False), per scale and pooled index: source rows k0, k1 and the weight of k1;
 *   stage 1 (image -> scale, align_corners=True), per scale and scale index (row stride stage1_stride): i0, i1, weight of i1;
 *   transposed composite operator for backward, CSR per scale over the image index: col_ptr [n_scales][S+1] (global offsets),
 *   col_out (pooled index), col_w.
 * forward leaves d loss / d pooled in the workspace, backward gathers it into grad_image [B,70,S,S] (overwritten) times
 * grad_scale[0] (device scalar: the incoming gradient of loss_out[0]). */
typedef struct {
  int B, image_size, pooled_size, channels;     /* 70 channels: diff_render.py:400-434 */
  int sem0, n_sem, dep0, n_dep;                 /* 1, 40, 41, 29 */
  int n_scales, stage1_stride;                  /* <= 4 scales (32, 48, 64, 96) */
  const int32_t* s2_k0; const int32_t* s2_k1; const float* s2_l1;     /* [n_scales][pooled_size] */
  const int32_t* s1_i0; const int32_t* s1_i1; const float* s1_l1;     /* [n_scales][stage1_stride] */
  const int32_t* col_ptr; const int32_t* col_out; const float* col_w;
  int max_col_entries;                          /* longest CSR row (selects the register-list backward kernel when <= 5); 0 = unknown */
  int per_room;                                 /* != 0: the B images are B independent rooms (one refinement loop each): loss_out is
                                                 * [B][3], every room's L1 mean runs over its own elements, inv_count is [B][n_scales] */
  const unsigned char* live_planes;             /* optional [B, channels] (device), as written by sln_scene_live_channels for `image`:
                                                 * bit 0 clear - the plane is all zeros: forward does not read it (a semantic plane
                                                 * enters the cross-entropy as zeros, unpooled; a depth-hot plane gets a zero pooled
                                                 * plane); value 1 - the plane is the constant 1: pooled from 1.f without loads (or not at
                                                 * all, see pooled_ones); bit 1 clear - nobody reads the plane's gradient: backward
                                                 * leaves that plane of grad_image as it is.  NULL: every plane is processed.  Honoured
                                                 * for the shapes of the refinement loop (P <= 96, 40 semantic channels), ignored else. */
  const unsigned char* null_mask;               /* optional [B, S, S] (device), with live_planes: 1 where the 29 depth-hot values of the pixel sum
                                                 * to < 0.5 (test_render_refine.py:332), as sln_scene_forward_live writes it - the loss then
                                                 * does not compute it */
  const float* pooled_ones;                     /* optional [n_scales, P, P] (device): sln_refine_pool of an all-ones plane.  With live_planes,
                                                 * the planes flagged "constant 1" are then not pooled per image: the loss reads this table */
  /* The validity mask of the target (all three or none: anything else is SLN_E_BADARG), as sln_refine_loss_mask leaves them */
  const unsigned char* valid_pooled;            /* optional [B, n_scales, P, P] (device): 0 - the pooled pixel addresses an image pixel the
                                                 * target says nothing about: its depth difference is neither formed nor summed, its depth
                                                 * gradient is exactly 0 (its label is -100 already).  NULL: no mask, the launches of before */
  const unsigned char* valid_image;             /* [B, S, S] (device): the mask itself - sln_refine_report's depth_l1 runs over its non-zero pixels */
  const int32_t* depth_count;                   /* [2, B] (device): row 0 the number N of valid pooled pixels room b's depth mean is divided by
                                                 * (all scales; per_room: the room's own, else the batch's in every entry), row 1 the number of
                                                 * non-zero pixels of valid_image[b] */
  const int64_t* conf_sum;                      /* optional [2, B] (device), as sln_refine_loss_confidence leaves it; needs the three mask fields
                                                 * (without all of them: SLN_E_BADARG).  Non-NULL: the per-pixel confidence route - valid_pooled
                                                 * holds pooled confidence bytes c (weight c / 255.f, 0 as on the masked route), valid_image the
                                                 * confidence image, and the means are divided by these sums / 255 instead of the counts: row 0
                                                 * the sum of c over room b's pooled pixels (all scales; per_room: the room's own, else the
                                                 * batch's in every entry), row 1 the sum over the image's pixels.  NULL: the fields mean what
                                                 * they meant */
} SlnRefineLoss;
int64_t sln_refine_loss_workspace_bytes(int B, int image_size, int pooled_size, int n_scales, int n_sem, int n_dep);
/* 1 when live_planes / null_mask / pooled_ones of L would be honoured (the refinement loop's shapes), 0 when every plane is processed
 * whatever they say: a producer that leaves dead planes unwritten (sln_scene_forward_live) must only be paired with a loss that
 * does not read them */
int sln_refine_loss_live_ok(const SlnRefineLoss* L);
int sln_refine_loss_init(const SlnRefineLoss* L /* host struct */, void* workspace, void* stream);   /* validates L; once per workspace */
/* The resampling alone: pooled_out [B][n_scales][n_sem + n_dep][P][P] of `image` (null_fill != 0: with the null-fill of the
 * last depth channel).  The caller derives the target's pooled depth and labels from it, so that regions where the iterate
 * equals the target give a difference of exactly 0 (and sign(0) = 0 in the L1 gradient), as in the reference where both go
 * through the same resampling code. */
int sln_refine_pool(const SlnRefineLoss* L, const float* image, int null_fill, void* workspace, float* pooled_out, void* stream);
/* target_depth_pooled [B][n_scales*n_dep][P][P], labels [B][n_scales][P][P] int32 (-100 = ignored), inv_count [n_scales]
 * (1 / number of non-ignored labels of the scale over the batch) */
int sln_refine_loss_forward(const SlnRefineLoss* L, const float* image, const float* target_depth_pooled, const int32_t* labels,
                            const float* inv_count, void* workspace, float* loss_out, void* stream);
int sln_refine_loss_backward(const SlnRefineLoss* L, const void* workspace, const float* grad_scale, float* grad_image, void* stream);
/* The validity mask of a target, once per target (four launches, the first of which clears the counters; integer sums only: the same
 * from call to call whatever sln_set_deterministic says; no allocation, synchronisation or read-back, legal under a capture).
 *   valid        [B, S, S] uint8 in the planes' row order: non-zero - the target means something at this pixel
 *   valid_pooled [B, n_scales, P, P] (out): 1 iff EVERY image pixel the two resampling stages address for the pooled pixel is valid,
 *                whatever the tap's weight (0 * NaN is NaN): the 16 taps {s1_i0[k], s1_i1[k] : k in {s2_k0[o], s2_k1[o]}} of rows x columns
 *   labels       [B, n_scales, P, P] (in-out): -100 wherever valid_pooled is 0
 *   inv_count    [B, n_scales] (per_room) or [n_scales] (out): 1.f / the number of labels >= 0 that are left (inf for none)
 *   depth_count  [2, B] (out): SlnRefineLoss::depth_count
 *   mask_status  [B] (out): bit 0 - depth_count[0][b] is 0 (depth and its gradient are then 0, not NaN); bit 1 - a scale keeps no label
 *                (of the room under per_room, of the batch otherwise)
 * The mask fields of L itself are not read (L may or may not carry them yet); `workspace` is the loss's, whose contents between a
 * forward and its backward this call destroys. */
int sln_refine_loss_mask(const SlnRefineLoss* L, const unsigned char* valid, int32_t* labels, unsigned char* valid_pooled, float* inv_count,
                         int32_t* depth_count, int32_t* mask_status, void* workspace, void* stream);
/* The per-pixel confidence of a target, once per target: the mask call with a graded weight (four launches, the first of which clears
 * the counters; integer sums only, 64-bit: the same from call to call whatever sln_set_deterministic says; no allocation,
 * synchronisation or read-back, legal under a capture).
 *   conf         [B, S, S] uint8 in the planes' row order: 0 - the target says nothing here (as valid == 0), 255 - full trust; a
 *                pixel's weight is conf / 255
 *   conf_pooled  [B, n_scales, P, P] (out): the MINIMUM of conf over the 16 taps of the pooled pixel (sln_refine_loss_mask's tap sets,
 *                whatever a tap's weight); for a {0, 255} image 255 * the mask call's valid_pooled
 *   labels       [B, n_scales, P, P] (in-out): -100 wherever conf_pooled is 0
 *   inv_count    [B, n_scales] (per_room) or [n_scales] (out): 1.f / (float)((double)(sum of conf_pooled over the labels >= 0 left) / 255.0)
 *   depth_count  [2, B] (out): the non-zero counts, as the mask call gives them for the mask conf != 0
 *   conf_sum     [2, B] (out): SlnRefineLoss::conf_sum
 *   mask_status  [B] (out): bit 0 - conf_sum[0][b] is 0 (depth and its gradient are then 0); bit 1 - a scale keeps no label
 * The mask fields of L itself are not read; `workspace` is the loss's, whose contents between a forward and its backward this call
 * destroys.  With every byte in {0, 255} the loss, its gradient and the report are the masked route's bits; all 255: the unmasked ones. */
int sln_refine_loss_confidence(const SlnRefineLoss* L, const unsigned char* conf, int32_t* labels, unsigned char* conf_pooled, float* inv_count,
                               int32_t* depth_count, int64_t* conf_sum, int32_t* mask_status, void* workspace, void* stream);

/* =============================================================================================
 * C. SPADE generator (models/SPADE_related.py: SPADEGenerator4 :1507-1605, SPADEResnetBlock4 :1457-1505,
 *    SPADE4 :1404-1454, LayerNorm2D :128-149, SEBlock2 :70-85; driver testing/test_SPADE_shade.py:9-13,77-79)
 * Tensors are NCHW fp32.  Conv weights are PRE-PACKED by the host once per checkpoint:
 *   wp[ks*ks][Cin][rows_pad] (output rows contiguous, rows_pad % 64 == 0), spectral norm already folded
 *   (W = W_orig / (u . (W_mat v))); for the modulation conv the rows of gamma and beta are interleaved in
 *   groups of 32: rows [64 g, 64 g + 32) = gamma of channels [32 g, 32 g + 32), the next 32 rows their beta.
 * ============================================================================================= */
/* Small convolution launches (< 192 workgroups: the batch-1 calls of testing/test_SPADE_shade.py:77-79) split their input channels
 * over several workgroups and add the partial sums in a fixed order; the partial sums live in a 48 MB scratch slot per (device,
 * stream) - at most 16 slots, the least recently used one is freed for a new stream.
 * sln_spade_prepare allocates `stream`'s slot now (optional: the first eager split launch on a stream does the same).  A slot cannot
 * be allocated while the stream is being captured: a split launch on a stream first seen during its capture fails with SLN_E_STATE
 * (-3) - call sln_spade_prepare (or run one eager forward) on the stream before capturing it.  An allocation failure is SLN_E_NOMEM.
 * A split launch recorded while its stream is captured PINS the stream's slot: the graph holds the slot's address, so a pinned slot
 * is never freed for a new stream (if all 16 are pinned, a new stream's slot is allocated beyond the cap) nor by a plain release.
 * sln_spade_release frees the slot of `stream` on the current device (`all` & SLN_SPADE_RELEASE_ALL: every slot of the process)
 * unless it is pinned; with `all` & SLN_SPADE_RELEASE_PINNED pinned slots are freed too - only once every graph that recorded a
 * launch on them has been destroyed.  It waits for the device.  Returns the number of slots freed.  Call it before destroying a
 * stream that ran SPADE launches (a recycled handle would otherwise inherit the slot, which is harmless, or keep 48 MB alive). */
#define SLN_SPADE_RELEASE_ALL 1
#define SLN_SPADE_RELEASE_PINNED 2
int sln_spade_prepare(void* stream);
int sln_spade_release(void* stream, int all);
/* y = act(conv_ks(x) + bias): ks = 3 (ReflectionPad2d(1)) or 1; act 0 none, 1 ReLU, 2 LeakyReLU(slope) */
int sln_spade_conv(const float* x, int B, int Cin, int H, int W, const float* wp, const float* bias, int rows, int rows_pad,
                   int ksize, int act, float slope, float* y, void* stream);
/* SPADE4 tail fused: out = LayerNorm2D(xin) * (1 + gamma) + beta [LeakyReLU(slope) when act == 2] with
 * [gamma | beta] = conv3x3_reflect(actv); stats[b] = (mean, 1 / (std + eps)) from sln_layernorm_stats */
int sln_spade_modulate(const float* actv, int B, int Cin, int H, int W, const float* wp, const float* bias, int C, int rows_pad,
                       const float* xin, const float* stats, int act, float slope, float* out, void* stream);
/* sln_spade_conv that also accumulates, from the values its epilogue writes, the sums the next layers need (fp64 atomics into
 * buffers the caller zeroed; either may be NULL): ln_acc [B][16] doubles = (sum y, sum y^2) of sample b -> LayerNorm2D
 * statistics of the following SPADE layer (:128-149) through sln_layernorm_finalize; gap_acc [B, rows] doubles = sum over
 * pixels -> SEBlock2's average pool (:70-85) through sln_block_tail. */
int sln_spade_conv_sums(const float* x, int B, int Cin, int H, int W, const float* wp, const float* bias, int rows, int rows_pad,
                        int ksize, int act, float slope, float* y, double* ln_acc, double* gap_acc, void* stream);
/* sln_spade_modulate with xin_up = 1: xin is [B, C, H/2, W/2] and stands for nn.Upsample(scale_factor=2) (nearest) of itself
 * (SPADEGenerator4.forward :1585-1597) - the upsampled tensor is never written; stats must be those of the upsampled tensor. */
int sln_spade_modulate_up(const float* actv, int B, int Cin, int H, int W, const float* wp, const float* bias, int C, int rows_pad,
                          const float* xin, int xin_up, const float* stats, int act, float slope, float* out, void* stream);
/* stats[b] = (mean, 1 / (unbiased std + eps)) from accumulated sums: acc [B][16] doubles (sum, sum of squares of n_acc values),
 * every value standing for `rep` elements of the normalised tensor (4 = its nearest x2 upsampling) */
int sln_layernorm_finalize(const double* acc, int B, int64_t n_acc, int rep, float eps, float* stats, void* stream);
/* fp16-MFMA forms of sln_spade_conv / _conv_sums / _modulate / _modulate_up (opt-in precision modes): same sizes,
 * same epilogues, ksize must be 3 (SLN_E_UNSUPPORTED otherwise, nothing launched).  Weights are packed fp16 (IEEE binary16 bits)
 * [ceil(Cin / 16)][9][rows_pad][16] (input channels zero padded to a multiple of 16): wp_hi = fp16(w), wp_lo = fp16(w - wp_hi).
 * wp_lo != NULL: three products per term (w_hi x_hi + w_hi x_lo + w_lo x_hi, the activations split the same way on the fly),
 * fp32-grade; wp_lo == NULL: one product (w_hi x_hi), fp16 operands with fp32 accumulation. */
int sln_spade_conv_f16(const float* x, int B, int Cin, int H, int W, const uint16_t* wp_hi, const uint16_t* wp_lo, const float* bias,
                       int rows, int rows_pad, int ksize, int act, float slope, float* y, void* stream);
int sln_spade_conv_sums_f16(const float* x, int B, int Cin, int H, int W, const uint16_t* wp_hi, const uint16_t* wp_lo, const float* bias,
                            int rows, int rows_pad, int ksize, int act, float slope, float* y, double* ln_acc, double* gap_acc, void* stream);
int sln_spade_modulate_f16(const float* actv, int B, int Cin, int H, int W, const uint16_t* wp_hi, const uint16_t* wp_lo, const float* bias,
                           int C, int rows_pad, const float* xin, const float* stats, int act, float slope, float* out, void* stream);
int sln_spade_modulate_up_f16(const float* actv, int B, int Cin, int H, int W, const uint16_t* wp_hi, const uint16_t* wp_lo, const float* bias,
                              int C, int rows_pad, const float* xin, int xin_up, const float* stats, int act, float slope, float* out,
                              void* stream);
/* TEST HOOK, host only (no HIP call): which convolution kernel the four entry points above launch for a problem - the decision of
 * csrc/spade.hip's conv_route, the one place where it is taken.  terms: 0 fp32, 1 / 3 the half modes (wp_lo NULL / given); epi: 0
 * bias + activation (sln_spade_conv*), 1 modulation (sln_spade_modulate*; ksize must be 3); rows: the entry point's Cout, or C.
 * force: -1 the process's own switches (SLN_CONV_STAGED, SLN_CONV_DMA, SLN_CONV_KSPLIT, read once per process), 0 no switch,
 * 1 SLN_CONV_STAGED alone, 2 SLN_CONV_DMA alone.  Returns 0, or what the entry point's size checks return for the problem
 * (SLN_E_BADARG also for a NULL out or a terms / epi / force value outside the lists above).
 * kernel: 0 conv_mfma_kernel (operands staged through registers), 1 conv_glds_kernel (DMA into LDS), 2 conv_f16_kernel; bmc: packed
 * rows per workgroup (64 / 128); tile_h: pixel rows per workgroup (8 / 16, by 16 columns); gk: input channels per chunk; blk: chunks
 * per accumulation block (0: one chain); shares: workgroups sharing the input channels of a tile (> 1: the input-channel split). */
typedef struct SlnDbgConvRoute { int kernel, bmc, tile_h, gk, blk, terms, shares; } SlnDbgConvRoute;
int sln_debug_conv_route(int terms, int epi, int B, int Cin, int H, int W, int rows, int rows_pad, int ksize, int force, SlnDbgConvRoute* out);
/* sizeof of SlnDbgConvRoute; returns how many sizes there are. */
int sln_debug_conv_sizes(int* out, int max);
/* Tail of SPADEResnetBlock4.forward (:1492-1493) and the nn.Upsample after it (:1585-1600) in one pass:
 *   out = up(xs + dx * sigmoid(W2 relu(W0 GAP(dx)))),  stats = LayerNorm2D statistics of the next block's input.
 * xs [B,C,H,W] (xs_up = 1: [B,C,H/2,W/2] read through nearest x2); gap_sums = the gap_acc of sln_spade_conv_sums or NULL;
 * up_mode -1: out [B,C,H,W], 0 nearest / 1 bilinear: out [B,C,2H,2W]; stats_rep 4 when the consumers read `out` through
 * nearest x2 themselves; stats may be NULL; scratch 2*B*C floats; acc 16*B doubles. */
int sln_block_tail(const float* xs, int xs_up, const float* dx, int B, int C, int H, int W, const double* gap_sums, const float* w0,
                   const float* w2, float* scratch, int up_mode, float* out, double* acc, int stats_rep, float eps, float* stats,
                   void* stream);
/* The same modulation when ONE semantic map drives the whole batch (colorize_with_spade, testing/test_SPADE_shade.py:30-79:
 * 50 z vectors per room): gb [rows_pad, H, W] = sln_spade_conv(actv of that map, the packed gamma|beta weights, act 0) is
 * computed once, then out[b] = LayerNorm2D(xin[b]) * (1 + gamma) + beta for every sample.  H*W % 4 == 0. */
int sln_spade_apply(const float* xin, const float* gb, int B, int C, int H, int W, int rows_pad, const float* stats, int act,
                    float slope, float* out, void* stream);
/* sln_spade_apply with xin_up = 1: xin is [B, C, H/2, W/2] and stands for its nearest x2 upsampling (W % 4 == 0, H % 2 == 0) */
int sln_spade_apply_up(const float* xin, int xin_up, const float* gb, int B, int C, int H, int W, int rows_pad, const float* stats,
                       int act, float slope, float* out, void* stream);
/* stats[b] = (mean, 1 / (unbiased std + eps)) over the n elements of sample b; scratch: 16 * B doubles */
int sln_layernorm_stats(const float* x, int B, int64_t n, float eps, double* scratch, float* stats, void* stream);
/* F.interpolate(size=...): mode 0 nearest (source = min(floor(dst * ((float)in / out)), in - 1), torch's float rule), 1
 * bilinear(align_corners=False) over BC planes.  src [BC, Hi, Wi], dst [BC, Ho, Wo].
 * Sizes: BC, Hi, Wi, Ho, Wo >= 1, else SLN_E_BADARG (nothing launched). */
int sln_resize(const float* src, int BC, int Hi, int Wi, int Ho, int Wo, int mode, float* dst, void* stream);
/* [LeakyReLU_0.01(conv3x3_reflect(seg[:,0:1])) | seg[:,1:]] (SPADE4.mlp_preshared_depth + cat, :1445-1446) into
 * out [B, nd + Cs - 1, H, W].  copy_masks = 0 writes the nd depth features only: the mask channels of a per-resolution
 * buffer are filled once (copy_masks = 1) and shared by every SPADE layer of that resolution.
 * Sizes: 1 <= B <= 65535, Cs >= 1, nd >= 0, H >= 2 and W >= 2 (ReflectionPad2d(1)), H * W <= 2^30, and 1 <= channels written
 * (nd, or nd + Cs - 1 with copy_masks) <= 65535, else SLN_E_BADARG (nothing launched).  seg [B, Cs, H, W], wpd [nd, 9], bpd [nd]. */
int sln_spade_depth_concat(const float* seg, int B, int Cs, int H, int W, const float* wpd, const float* bpd, int nd, float* out,
                           int copy_masks, void* stream);
/* x_s + SEBlock2(dx) (:1492-1493); xs, dx, out [B, C, hw]; w0 [C/8, C], w2 [C, C/8]; scratch 2*B*C floats (the pool values, then
 * the scale vector in scratch[B*C:]).  Sizes: B >= 1, C >= 8 and C % 8 == 0, hw >= 1, else SLN_E_BADARG (nothing launched). */
int sln_se_scale_add(const float* xs, const float* dx, int B, int C, int64_t hw, const float* w0, const float* w2, float* scratch,
                     float* out, void* stream);
/* nn.Upsample(scale_factor=2): mode 0 nearest, 1 bilinear (align_corners=False); x [BC, H, W], y [BC, 2H, 2W].
 * Sizes: BC, H, W >= 1, else SLN_E_BADARG (nothing launched). */
int sln_upsample2x(const float* x, int BC, int H, int W, int mode, float* y, void* stream);
/* tanh(conv5x5_zero_pad(LeakyReLU_0.2(x))) (:1602-1603); w [Cout,Cin,5,5], Cout <= 4 */
int sln_conv_img_tanh(const float* x, int B, int Cin, int H, int W, const float* w, const float* bias, int Cout, float* y, void* stream);

/* =============================================================================================
 * Scene-graph builder: SuncgDataset.__getitem__ + suncg_collate_fn for a batch of rooms
 * (reference data/suncg_dataset.py:110-353; compute_rel utils.py:36-80).  The reference builds one room at a
 * time in python; here the room table is resident in HBM and a batch of B rooms is two launches + one emit.
 * All pointers are device pointers unless noted.
 * ============================================================================================= */
typedef struct {
  const int* room_off;            /* [n_rooms+1] first object of each room in the flat arrays */
  const int* cls;                 /* [N] vocabulary index of every object (>= 1; 0 is '__room__') */
  const float* bbox;              /* [N,6] raw x0,y0,z0,x1,y1,z1 ('new_bbox', suncg_dataset.py:116-123) */
  const int* rot;                 /* [N] 'rotation' bin */
  const float* room_bbox;         /* [n_rooms,3] (suncg_dataset.py:131-137) */
  const int64_t* room_id;         /* [n_rooms] ids returned as all_ids, or NULL: the table index */
  const float* size_thr;          /* [n_classes,4]: use_attr_30 = 0: (height, volume, -, -) of size_info_many.json;
                                     = 1: (height_7, height_3, volume_7, volume_3) of 30_size_info_many.json */
  const unsigned char* has_size;  /* [n_classes] class present in that json */
  int n_rooms, n_classes, use_attr_30, reserved;
} SlnRoomTable;

/* The random decisions of __getitem__, one entry per NON-room object of the batch, batch order
 * (suncg_dataset.py:189-196: random.choice / random.random; :236-282: attribute draws). */
typedef struct {
  const int* other;               /* partner, as an object index inside its room (!= the object itself) */
  const unsigned char* swap;      /* 1: (s, o) = (cur, other)  [random.random() > 0.5],  0: (other, cur) */
  const unsigned char* attr_mode; /* 0: 'none' [first draw > 0.5 or class without statistics], 1: height test, 2: volume test */
} SlnGraphDraws;

/* Outputs with the dtypes of suncg_collate_fn (suncg_dataset.py:310-353). */
typedef struct {
  int64_t* ids;                   /* [B] or NULL */
  int64_t* objs;                  /* [O] */
  float* boxes;                   /* [O,6] room-normalised, the room row last in every graph */
  int64_t* triples;               /* [T,3] (s, p, o) with batch-global rows */
  int64_t* angles;                /* [O] */
  int64_t* attributes;            /* [O] */
  int64_t* obj_to_img;            /* [O] */
  int64_t* triple_to_img;         /* [T] */
} SlnGraphBatch;

/* counts [2B] (rows, triples per room; rows < 0 marks a room index outside the table); offsets [2B+3]:
 * [0..B] exclusive scan of rows (offsets[B] = O), [B+1..2B+1] of triples (offsets[2B+1] = T), [2B+2] = bad room indices.
 * room_idx [B] indexes the table.  The caller reads O and T back (3 ints) to size the outputs. */
int sln_graph_plan(const SlnRoomTable* tab /* host struct */, const int* room_idx, int B, int* counts, int* offsets, void* stream);
int sln_graph_emit(const SlnRoomTable* tab /* host struct */, const int* room_idx, int B, const int* offsets,
                   const SlnGraphDraws* draws /* host struct */, const SlnGraphBatch* out /* host struct */, void* stream);
/* The decisions of SlnGraphDraws drawn on the device (the reference draws them with python's `random`, suncg_dataset.py:189-196,
 * 236-282): Philox keyed by key[0..1] (two 64-bit words in DEVICE memory - e.g. taken from a torch generator, which keeps its own
 * stream position), one counter per non-room object of the batch (offsets as written by sln_graph_plan / planned on the host). */
int sln_graph_draw(const SlnRoomTable* tab /* host struct */, const int* room_idx, int B, const int* offsets, const int64_t* key,
                   int* other, unsigned char* swap, unsigned char* attr_mode, void* stream);

/* Layout evaluation: the --measure_acc_l1_std mode of test.py (testing/test_acc_mean_std.py:10-125: get_std, get_acc_l1) on the
 * device.  Layouts are [S, O, 6] (box_dim must be 6: anything else is SLN_E_BADARG, nothing launched); objs [O] and triples [T, 3]
 * are one collated batch (suncg_collate_fn); the layouts are read, never written.
 *
 * scene_graph_acc (testing/test_utils.py:135-152) for S layouts in one launch: restore_box (:119-132: every non-room row scaled by
 * the first '__room__' row at or after it; room rows and rows behind the last room row unscaled), then compute_rel (utils.py:36-80,
 * '__in_room__' when the object is a room row; None - a NaN centre difference - matches nothing) compared with the triple's
 * predicate BY NAME: pred_table_host[16] maps compute_rel's relation order (the builder's predicate order) to the vocabulary's
 * predicate index, -1 where the vocabulary lacks the name.  good[S] (int64) += matches.  confusion [S, 16, 17] (int64, or NULL)
 * += one count per triple at (relation of the ground-truth name, relation computed | 16 = None); triples whose ground-truth name
 * is not one of the 16 relations are not entered.  room_cls is the index of '__room__' in object_idx_to_name. */
int sln_layout_relation_acc(const float* boxes, int S, int O, int box_dim, const int64_t* objs, const int64_t* triples, int T, int room_cls,
                            const int* pred_table_host, int64_t* good, int64_t* confusion, void* stream);
/* get_std (testing/test_acc_mean_std.py:39-69) of one batch: S decodes [S, O, 6] (un-restored) + their angle bins [S, O] (int64);
 * np.std over the samples (ddof 0, two-pass in fp64) of the angle bins, the centres b[:3]/2 + b[3:]/2 and the sizes |b[:3] - b[3:]|
 * (float32 as numpy forms them), then the mean over the elements of each kind: out[0..2] += (angle, position, size).  Fixed-order
 * reduction: bit-identical run to run. */
int sln_layout_spread(const float* boxes, const int64_t* angle_bins, int S, int O, int box_dim, double* out, void* stream);
/* F.l1_loss(layout, gt) of each of S layouts against gt [O, 6] (testing/test_acc_mean_std.py:111-113): fp64 sum of the float32
 * |a - b|, fixed order; out[S] += sum / (6 O). */
int sln_layout_l1(const float* boxes, int S, int O, int box_dim, const float* gt, double* out, void* stream);
/* The baselines of get_acc_l1 (testing/test_acc_mean_std.py:108-110) from the ground truth gt [O, 6]: out[0] = random_scene
 * (testing/test_utils.py:93-116: rows of class room_cls copied, every other row re-centred at a uniform (x, y, z) keeping its
 * extent), out[1] = gt + float32([off, off]) with off ~ N(0, 0.1).  out is [2, O, 6].  Draws: injected (uniforms, normals [O, 3]
 * float32, row-indexed; the uniforms of room rows are not read) or, with key != NULL, drawn on the device: Philox keyed by
 * key[0..1] (two 64-bit words in DEVICE memory, as sln_graph_draw), one counter per row. */
int sln_layout_baselines(const float* gt, const int64_t* objs, int O, int box_dim, int room_cls, const float* uniforms,
                         const float* normals, const int64_t* key, float* out, void* stream);

/* Rotated-cuboid IoU of S layouts against the ground truth - the figure of the reference's refinement table (get_boxes
 * testing/test_render_refine.py:78-116, get_eight_coors_bbox_new / get_iou_cuboid testing/test_utils.py:7-40, the print_iou block
 * :360-368).  boxes [S, O, 6] and angles [S, O] (float angle bins, fractional allowed), gt_boxes [O, 6], gt_angles [O].  Row i is
 * scaled by the [3:6] of ITS layout's room row room_of_row[i] (int32 [O]: the row index of the last row of the row's room, >= i; the
 * rows of a room are consecutive, as suncg_collate_fn lays them out), centred, rotated about y by -angle * (2 pi / 24) and moved back
 * (:90-110); iou = inter2d * max(0, min(h1) - max(h0)) / (vol_a + vol_b - inter + 1e-5) with the unsigned areas of shapely (the
 * winding of a ring does not matter, zero-width boxes have area 0) and the SIGNED height of the reference.  NaN input gives NaN.
 * iou_out [S, O] (float, or NULL) receives every row's IoU (NaN for a row whose room_of_row entry is not a row at or behind it).
 * mean_out (float64, or NULL; one of the two is needed) is PER ROOM: [S, n_rooms], mean_out[s][room_id[room row]] += the mean over the
 * room's rows with visible[row] != 0 (uint8 [O]), NaN for a room without a visible row (np.mean([])); room_id is int32 [O] with
 * values in [0, n_rooms), distinct per room (one room: all zeros, n_rooms 1).  Fixed summation order: bit-identical run to run.
 * One lane per (layout, row); S <= 65535 per call. */
int sln_layout_cuboid_iou(const float* boxes, const float* angles, const float* gt_boxes, const float* gt_angles,
                          const int32_t* room_of_row, const unsigned char* visible, const int32_t* room_id, int n_rooms, int S, int O,
                          float* iou_out, double* mean_out, void* stream);
/* How much of a layout's furniture interpenetrates: over the unordered pairs (i < j) of visible rows of the same room (cuboids as
 * above), vol_out[s] (float64) += the sum of the intersection volumes and pairs_out[s] (int64) += the number of pairs whose IoU
 * exceeds thresh.  One workgroup per layout (several layouts per workgroup when O <= 128), the cuboids staged once in LDS in tiles
 * of whole rooms; a room of more than 1024 rows (or a room_of_row table that is not as described above) gives vol_out = NaN. */
int sln_layout_overlap(const float* boxes, const float* angles, const int32_t* room_of_row, const unsigned char* visible, int S, int O,
                       float thresh, double* vol_out, int64_t* pairs_out, void* stream);
/* The same quantity as a loss term with a gradient: penalty_out[s][room_id[room row]] (float64 [S, n_rooms], WRITTEN) = the sum over
 * the unordered pairs (i < j) of rows of one room with collide[row] != 0 (uint8 [O]) of V_ij = A(ring_i, ring_j) * max(0, min(h1) -
 * max(h0)) - the intersection volumes sln_layout_overlap sums, cuboids (testing/test_render_refine.py:90-110), room_of_row and room_id
 * as in sln_layout_cuboid_iou - and grad_boxes [S, O, 6] / grad_angles [S, O] = weight * d penalty / d (boxes, angles).  The extent
 * (the room row's [3:6]) is a constant: the gradient of a room row and of a row that does not collide is exactly 0.  d A / d ring_a
 * with ring b fixed: both rings in counter-clockwise order, every edge p -> q of a (d = q - p) clipped to [s0, s1] of [0, 1] by b's
 * four half planes (the inside rule of the area function), w = (s1^2 - s0^2) / 2: dA/dp += (d.y, -d.x) ((s1 - s0) - w), dA/dq +=
 * (d.y, -d.x) w.  Heights: the derivative of max(0, min(.,.) - max(.,.)), one half to each row on an exact tie (torch.minimum /
 * torch.maximum); nothing from a pair whose height overlap is <= 0.  Then through the corner expressions to box[0:6] and angle.
 * accumulate = 0 writes every element of the two gradients (zeros for rows that take no part), 1 adds onto what is there with one
 * float32 add per element.  One launch in the frame of sln_layout_overlap (cuboids staged in LDS in tiles of whole rooms; the tiles
 * of a layout are dealt to several workgroups): a row walks all colliding partners of its room - four adjacent lanes split the list
 * and meet in a fixed butterfly - and one lane owns its seven values (no atomics); the value comes from the partners behind the
 * row, the per-room sum runs in fp64 in row order with one writer per (layout, room): bit-identical from call to call, and a room's
 * bits do not depend on the rooms around it.  No allocation, no synchronisation: legal inside a capture.  A room of more than 1024
 * rows (or a broken room_of_row table) gives a NaN penalty - for it and the rooms behind it - and zero gradients.  Finite input gives
 * finite gradients; a NaN input may give
 * NaN in its own room's outputs only.  SLN_E_BADARG: a null pointer, a negative size, n_rooms < 1, !(weight >= 0), accumulate not
 * 0 or 1. */
int sln_layout_overlap_penalty(const float* boxes, const float* angles, const int32_t* room_of_row, const unsigned char* collide,
                               const int32_t* room_id, int n_rooms, int S, int O, float weight, int accumulate, double* penalty_out,
                               float* grad_boxes, float* grad_angles, void* stream);
/* The top-down picture of testing/test_plot2d.py:9-141 (plot2d) for S layouts x n_rooms rooms in one launch.  boxes [S, O, 6], angles
 * [S, O], room_of_row and room_id (int32 [O]) as in sln_layout_cuboid_iou.  A row's ring is the (x, z) corners of the cuboid above
 * (:88-110 are the statements of get_boxes).  rank (int32 [O]) is the class's index in nyu_class_order (:25-29, at most 127), < 0 for
 * a row that is not drawn (do_not_vis :74,86, room rows); rgb (uint32 [O]) is mapped_colors[nyu_class_orig.index(name)] (:30-71,122)
 * packed r | g << 8 | b << 16 - both tables are the caller's, the kernel knows no vocabulary.  The image of a room is N x N over
 * [0, 1]^2, the pixel of row r, column c centred at x = (c + 0.5) / N, z = (r + 0.5) / N (row 0 at z ~ 0: what `1 - z` :124 under
 * matplotlib's y-up axes shows).  A pixel is covered by a ring q when the four edge functions (q[k+1].x - q[k].x)(z - q[k].z) -
 * (q[k+1].z - q[k].z)(x - q[k].x) are all >= 0 or all <= 0 (either winding, edges inclusive, float32, contraction off); a ring whose
 * shoelace sum is exactly 0 and a ring with a NaN coordinate cover nothing.  Among the drawn rows of the room that cover a pixel
 * the greatest (rank, row) wins - the order sorted(zip(current_types, iter_idx)) paints in (:118-126).  winner (int32
 * [S, n_rooms, N, N], or NULL) receives the winning row, -1 where nothing covers; image (uint8 [S, n_rooms, N, N, 3], or NULL; one of
 * the two is needed, image needs rgb) its colour, the floor's (152, 223, 138) (:115-117) where nothing covers.  Rooms are staged
 * 256 rows at a time, of any length.  1 <= N <= 1024, S <= 65535 per call, n_rooms <= 65535, O <= 2^24. */
int sln_layout_plot(const float* boxes, const float* angles, const int32_t* room_of_row, const int32_t* room_id, const int32_t* rank,
                    const uint32_t* rgb, int n_rooms, int S, int O, int N, int32_t* winner, unsigned char* image, void* stream);
/* Footprint heat map: counts[o][r][c] (int32 [O, N, N]) += the number of the S layouts whose ring of row o covers pixel (r, c) (ring,
 * pixel and coverage as above), for the rows with rank[o] >= 0; the planes of the other rows are not touched.  Where
 * sln_layout_heatmap (testing/test_heatmap.py:80-99) counts an object's centre, this counts everywhere the object is.  Integer
 * atomics only: exact, and the same from run to run.  1 <= N <= 1024, O <= 65535. */
int sln_layout_footprint_counts(const float* boxes, const float* angles, const int32_t* room_of_row, const int32_t* rank, int S, int O,
                                int N, int32_t* counts, void* stream);
/* The refinement report of testing/test_render_refine.py:369-374 (what the reference pickles into bbox_rot_0.pkl) for the rooms of a
 * per_room descriptor (or the single image of a B = 1 one), after sln_refine_loss_forward on `image` with the same descriptor and
 * workspace and before the next one: report_out [B, 3] (float) = (iou, depth_l1, ce_last).
 *   depth_l1 = L1Loss(iter[:, 41:], target[:, 41:]) at full resolution: the iterate after the null fill of its last depth channel
 *              (:332), target_depth [B, n_dep, S, S] the target's depth-hot planes as rendered (not filled).  Planes of `image` that
 *              live_planes flags dead are not read (zeros, respectively the constant 1).
 *   ce_last  = the cross-entropy of the last pooling scale without the / 800, from the partial sums the loss forward left in the
 *              workspace (needs pooled_size^2 % 128 == 0: SLN_E_UNSUPPORTED otherwise).
 *   iou      = iou_mean[b] (float64 [B], e.g. the mean_out of sln_layout_cuboid_iou), which is then RESET to 0 for the next
 *              accumulation; NaN when iou_mean is NULL.
 *   With the mask fields of L set, depth_l1 is the mean over the valid image pixels of the 29 planes (0 when the room has none) and
 *   the target is not read elsewhere; ce_last follows from the masked labels.
 * scratch: sln_refine_report_scratch_doubles(B) float64.  Fixed summation order. */
int sln_refine_report(const SlnRefineLoss* L, const float* image, const float* target_depth, const void* workspace, double* scratch,
                      double* iou_mean, float* report_out, void* stream);
int sln_refine_report_scratch_doubles(int B);

/* The [B, 41, size, size] float32 tensor SPADEGenerator4 consumes, from the file arrays of colorize_with_spade
 * (testing/test_SPADE_shade.py:50-76): channel 0 = ((clip(d - min d, 0, dmax) / dmax) - 0.5) * 2 with dmax = max{d - min d < 20} per
 * room (float32, the reference's operation order), channel 1 + c = the mask of NYU class c (< 120 -> 0, > 120 -> 1, exactly 120 stays),
 * every channel resized by Rh . X . Rw^T in float64.  depth [B, H, W] float32.  `planes` by mode:
 *   SLN_SPADE_INPUT_MASKS_U8 / _F32   [B, n_live, H, W] uint8 / float32 masks; channels [B, n_live] int32 = the NYU class (0..39) each
 *                                     plane fills, < 0 for a padding plane (not read); n_live 0..40
 *   SLN_SPADE_INPUT_LABELS            [B, H, W] uint8 class-index image: 0 no class, 1 + c NYU class c (channels, n_live unused)
 * A channel no plane fills is written as exact 0.0.  The resize operators are banded tables: first_h [size] int32 and w_h
 * [size, width_h] float64 with Rh[o, first_h[o] + k] = w_h[o, k] (first_h[o] + width_h <= H), first_w [size] and w_w TRANSPOSED
 * [width_w, size] for Rw.  status [B] int32: 1 when no depth value of the room lies below min + 20 (the reference raises there; the
 * room's depth channel is NaN), else 0.  Three launches on `stream`; no allocation, no synchronisation, no host read, no atomics:
 * legal inside a stream capture and bit-identical from call to call.  workspace: sln_spade_input_workspace_bytes(B) bytes, 8-byte
 * aligned.  SLN_E_UNSUPPORTED when a [4, W] float64 row tile does not fit 64 KiB of LDS (W above about 1 900). */
enum { SLN_SPADE_INPUT_MASKS_U8 = 0, SLN_SPADE_INPUT_MASKS_F32 = 1, SLN_SPADE_INPUT_LABELS = 2 };
int64_t sln_spade_input_workspace_bytes(int B);
int sln_spade_input_forward(const float* depth, const void* planes, int mode, const int32_t* channels, int n_live, int B, int H, int W,
                            int size, const int32_t* first_h, const double* w_h, int width_h, const int32_t* first_w, const double* w_w,
                            int width_w, void* workspace, float* out, int32_t* status, void* stream);

/* The pictures of the refinement loop (testing/test_render_refine.py: save_images :144-163, save_label_depth :118-142 and the label
 * statements :343-344) from a scene tensor image [B, channels, S, S] float32 on the device; channels is 70, or 41 (depth plus the 40
 * semantic planes: target[:, :41]).  Per room, all float32, in this order of operations:
 *   depth8 [B, S, S]       d = x - min x over channel 0; m = max{d : d < 10}; every d > 10 becomes m; byte = trunc((d / m) * 255) with a
 *                          correctly rounded division.  A d of exactly 10 is outside the reference's defined behaviour (its uint8 cast
 *                          overflows): the byte saturates at 255.
 *   labels [B, S, S]       0 where the sum of channels 1..40 (channel order) is < 0.5, else 1 + argmax over them (the first maximum wins):
 *                          the class-index image of sln_spade_input_forward's SLN_SPADE_INPUT_LABELS.  NULL: not computed.
 *   rgb    [B, S, S, 3]    palette[labels]; palette [41] (device) = r | g << 8 | b << 16, entry 0 = no class.  NULL: not computed.
 *   masks8 [B, 40, S, S]   trunc(255 * plane) of channels 1..40 for planes in [0, 1] (saturated outside).  NULL: not computed.
 *   status [B] int32       bit 0: no d < 10 exists (the reference's np.max raises), bit 1: m == 0 (the reference divides by zero); the
 *                          room's depth bytes are 0 in both cases.
 * live_planes [B, channels] (or NULL: every plane is read) are the flags of SlnRefineLoss::live_planes: a plane with bit 0 clear is
 * all zeros, a plane with the value 1 the constant 1; neither is read.  At most three launches on `stream`; no allocation, no
 * synchronisation, no host read, no atomics: legal inside a stream capture and bit-identical from call to call.  workspace:
 * sln_scene_pictures_workspace_bytes(B, S) bytes; image 16-byte, every other buffer 4-byte aligned (SLN_E_BADARG otherwise).
 * SLN_E_UNSUPPORTED, nothing launched: S % 4 != 0, S * S > 2^30, B < 1 or > 65535, channels not 41 or 70. */
int64_t sln_scene_pictures_workspace_bytes(int B, int S);
int sln_scene_pictures(const float* image, int B, int channels, int S, const unsigned char* live_planes, const uint32_t* palette,
                       void* workspace, unsigned char* depth8, unsigned char* labels, unsigned char* rgb, unsigned char* masks8,
                       int32_t* status, void* stream);

/* Mesh retrieval (models/misc.py:34-64 suncg_retrieve): for every object row the model of the row's class whose bounding-box edge
 * ratios are nearest to the predicted box's.  boxes [S, N, 6] float32: S >= 1 layouts of the same N row-concatenated rows; room_row
 * [N] int32: every row's room row (the last row of its room); objs [N] int32: the class index (object_idx_to_name); class_ptr
 * [n_classes + 1] int32: models class_ptr[c] .. class_ptr[c + 1] of model_ratio [M, 2] float64 (16-byte aligned) belong to class c,
 * model_ratio[m] = (size_y / size_x, size_z / size_x) of the table's bbox_max - bbox_min, formed in float64 on the host (:58-59).
 * Per row, in the reference's order: float32 - the six box entries times the room row's [3], [4], [5] (one multiplication each), the
 * three differences, the correctly rounded quotients dy/dx, dz/dx; float64 - |t0 - r0| + |t1 - r1| per model; np.argmin: the first
 * minimum wins, a NaN distance beats everything and the first NaN is kept.  choice [S, N] int32: the index WITHIN the class, -1 for
 * a room row (room_row[i] == i or outside [0, N)), a class without models and a class outside [0, n_classes).  dist [S, N] float64
 * (or NULL): the winning distance, NaN where choice is -1.  One launch on `stream`, one row per lane, the table staged through LDS in
 * chunks of 2048 models; no atomics, no allocation, nothing read back: legal inside a stream capture.  S <= 65535 per call. */
int sln_mesh_retrieve(const float* boxes, const int32_t* room_row, const int32_t* objs, const int32_t* class_ptr, int n_classes,
                      const double* model_ratio, int M, int S, int N, int32_t* choice, double* dist, void* stream);
/* wall_retrieve / floor_retrieve (models/misc.py:123-152) for R rooms: boxes [N, 6] float32, last_row [R] int32 the rooms' room rows.
 * With (X, Y, Z) the room row's [3:6] promoted to float64: out[r][0] = argmin_j |wall_ratio[j][0] - Y / X| + |wall_ratio[j][1] - Z / X|
 * over wall_ratio [W, 2], out[r][1] = argmin_j |floor_ratio[j] - Z / X| over floor_ratio [W] (both float64, host-formed), the argmin
 * rules above; -1 for W == 0 or a last_row entry outside [0, N).  out [R, 2] int32.  One launch, one room per lane. */
int sln_shell_retrieve(const float* boxes, const int32_t* last_row, int R, int N, const double* wall_ratio, const double* floor_ratio,
                       int W, int32_t* out, void* stream);

/* =============================================================================================
 * Viewpoint render of render/render_semantic_depth.py::render_test (:152-377), the hand-off between the placed meshes and the SPADE
 * input (csrc/shade_view.hip; host/shade.py).  Rasterisation in between is sln_raster_forward.
 * ============================================================================================= */
/* R rooms of N rows each (rows beyond a room's length are padding), V candidate views per room.  Face slot f of a room:
 *   f <  N * Fm : row f / Fm, face f % Fm of the row's model (bank.f, corner indices local to the model);
 *   f >= N * Fm : face f - N * Fm of the shell (shell_f over the room's Vs placed shell vertices).
 * so F = N * Fm + Fs for every room and every shape is fixed.  Pointers are device pointers unless named *_host. */
typedef struct SlnViewPlace {
  /* the bank's resident models: model m owns vertices voff[m] .. voff[m + 1] of v [Vtot, 3] and faces foff[m] .. foff[m + 1] of f */
  const float* bank_v;
  const int32_t* bank_f;          /* [Ftot, 3] */
  const int32_t* voff;            /* [M + 1] */
  const int32_t* foff;            /* [M + 1] */
  const int32_t* voff_host;       /* the same two tables on the host: what the call checks before it launches */
  const int32_t* foff_host;
  /* per row [R * N]: v' = A v + tr (fp32, row-major 3 x 3), the bank model of the row (< 0: none - not imported, no model, padding),
   * the class byte of its faces (1 + NYU class; 0 with row_model < 0) */
  const float* A;
  const float* tr;
  const int32_t* row_model;
  const unsigned char* row_label;
  /* the shell: placed vertices [R, Vs, 3], one topology for all rooms */
  const float* shell_v;
  const int32_t* shell_f;         /* [Fs, 3] */
  const int32_t* shell_f_host;    /* [Fs, 3] on the host (checked against Vs) */
  const unsigned char* shell_label; /* [Fs] */
  const float* K;                 /* [R * V, 3, 3] */
  const float* Rm;                /* [R * V, 3, 3] */
  const float* t;                 /* [R * V, 3] */
  int32_t M, Vtot, Ftot, Fm, Vs, Fs, R, V, N, reserved;
  float orig_size, near;
} SlnViewPlace;
/* faces_xyz [R * V, F, 3, 3] = (x_ndc, y_ndc, z_cam) per corner, as sln_project_faces defines them (eps 1e-9) for the row's
 * placed model; a face with a corner nearer than `near`, a slot beyond its model's face count and every slot of a row without a
 * model collapse to the point (0, 0, 0): they cover no pixel.  face_label [R, F] uint8: the row's class byte on the slots of its
 * model's faces, the shell's bytes, 0 on empty slots.  One launch, forward only, no atomics, no allocation: legal inside a stream
 * capture.  Checked on the host before the launch (SLN_E_BADARG, nothing launched): null pointers, sizes < 1 (Fs, Vs, M may be 0),
 * R * V > 65535, voff_host / foff_host not starting at 0, decreasing, ending past Vtot / Ftot, a model with more than Fm faces,
 * a shell corner outside [0, Vs), F > 2^24, orig_size <= 0.  What only the device holds (row_model, the
 * corner indices in bank_f, the device copies of the tables) is range-checked per lane: a value outside its range makes the slot
 * an empty one, never an out-of-bounds read. */
int sln_view_place_project(const SlnViewPlace* d, float* faces_xyz, unsigned char* face_label, void* stream);
/* From the rasterizer's maps (raster order: row 0 = bottom) of B = R * V views: labels [B, S, S] uint8 and depth_out [B, S, S]
 * float32 in IMAGE row order (row 0 = top): face_label [B / V, F] of the hit face and its depth, 0 and 1e10 (Blender's empty Z)
 * where face_index is outside [0, F); per view sum [B] float64 and count [B] int64 of the depth_out entries below 1e5.  The
 * reduction is fixed-order (per-workgroup partials into the workspace, one last pass): repeatable, whatever sln_set_deterministic
 * says.  Two launches, no atomics, no allocation.  workspace: sln_view_compose_workspace_bytes(B) bytes, 8-byte aligned. */
int64_t sln_view_compose_workspace_bytes(int B);
int sln_view_compose(const int32_t* face_index, const float* depth, const unsigned char* face_label, int B, int V, int F, int S,
                     void* workspace, unsigned char* labels, float* depth_out, double* sum, int64_t* count, void* stream);

/* =============================================================================================
 * The refinement target of an observed room (csrc/observed_target.hip; host/observe.py): the 70-plane tensor sln_scene_forward
 * composes from its rasterisation, composed from a depth image and a class-index image instead.
 * ============================================================================================= */
/* depth [B, S, S] float32 (metric, the refinement camera's: plane 0 of a scene tensor) and labels [B, S, S] uint8 (0 = no class,
 * 1 + c = NYU class c: sln_scene_pictures' labels) on the device, both in the row order of the scene tensor's planes (no row is
 * flipped).  chan / dch [NC] int32 are the VALUES of the tables sln_scene_forward takes (class 0 is the wall; chan = NYU channel,
 * dch = depth-hot channel or -1), read on the HOST: they are checked before anything is launched and travel as launch arguments.
 * out [B, nch, S, S] float32, every plane written; status [B] int32.  Per room, d the depth and y the byte of a pixel:
 *   reading      0 < d <= 15; a NaN, an infinity, d <= 0 and d > 15 are none.  d0 = d with a reading, else -1 (the renderer's
 *                background value); l = y where y <= 40 and the pixel has a reading, else 0.
 *   out[0]       d0
 *   out[1 + c]   exactly 1.0 where l == 1 + c, else exactly 0.0, c = 0 .. 39 - whether or not a class of the tables has channel c
 *   mask_c       {l == chan[c] + 1};  cnt_c its pixel count;  sum_c = (double)(sum over the mask of rint((double)d0 * 2^32), a 64-bit
 *                integer: order-independent) * 2^-32 - the fixed point of the scene pass's statistics;  wall_max = max of d0 over
 *                mask_0, 10 where mask_0 is empty
 *   out[41 + k]  for the class c with dch[c] == k:  d0 / wall_max inside mask_c,  fill_c / wall_max outside,
 *                fill_c = cnt_c > 0 ? (float)(sum_c / cnt_c) : wall_max  (the scene pass's compose expressions: float32, correctly
 *                rounded quotients);  all 0 for a k no class owns
 *   status       bit 0: a byte > 40;  bit 1: an l > 0 whose NYU channel no class of the tables has;  bit 2: mask_0 is empty (no wall
 *                pixel);  bit 3: a byte in 1 .. 40 on a pixel without a reading
 * Two launches on `stream` (at most three); no allocation, no synchronisation, nothing read back, no floating-point atomics: legal
 * inside a stream capture and bit-identical from call to call.  workspace: sln_observed_target_workspace_bytes(B, S) bytes.
 * SLN_E_UNSUPPORTED, nothing launched: S % 4 != 0, S < 4 or S > 4096 (the integer sum stays below 2^63), B < 1 or > 65535, NC < 1 or
 * > 64, nch > 72 or nch != 41 + (number of dch >= 0).  SLN_E_BADARG, nothing launched: a null pointer; depth or out not 16-byte, any
 * other buffer not 4-byte aligned; chan[c] outside [0, 40), dch[c] outside [-1, nch - 41), a depth channel owned by two classes. */
int64_t sln_observed_target_workspace_bytes(int B, int S);
int sln_observed_target(const float* depth, const unsigned char* labels, int B, int S, int NC, const int32_t* chan, const int32_t* dch,
                        int nch, void* workspace, float* out, int32_t* status, void* stream);

/* =============================================================================================
 * An observed frame of any pinhole camera, brought into the refinement view (csrc/observed_reproject.hip; host/reproject.py): the
 * step in front of sln_observed_target.  The frame is a triangle mesh over its pixel grid; rasterisation in between is
 * sln_raster_forward.  DESIGN §4 "Observed frames from any camera" is the definition.
 * ============================================================================================= */
/* B frames of Hs x Ws pixels, all device pointers.  Pixel (i, j) - row i from the top - with depth d has a READING when 0 < d <= 15
 * (a NaN, an infinity and anything outside have none) and is the point ((j + 0.5 - cx) / fx * d, (i + 0.5 - cy) / fy * d, d) of the
 * source camera (x right, y down, z forward); pose takes it to the frame sln_project_faces projects from (R p + t of the target view),
 * and K_tgt, orig_size project it with that function's expressions (eps 1e-9). */
typedef struct SlnReproject {
  const float* depth_src;         /* [B, Hs, Ws] metric depth along the optical axis */
  const float* k_src;             /* [B, 4] fx, fy, cx, cy in source pixels; read on the device only */
  const float* pose;              /* [B, 3, 4] source camera -> target camera, [R | t] row-major */
  const float* K_tgt;             /* [B, 3, 3] */
  int32_t B, Hs, Ws, reserved;
  float orig_size, near, gap, reserved_f;
} SlnReproject;
/* faces_xyz [B, F, 3, 3] = (x_ndc, y_ndc, z_cam) per corner, F = 2 (Hs - 1) (Ws - 1): the cell of the pixels a = (i, j), b = (i + 1, j),
 * c = (i, j + 1), d = (i + 1, j + 1) owns the slots 2 (i (Ws - 1) + j) + {0, 1} = (a, b, c), (d, c, b) - front-facing for
 * sln_raster_forward when source and target see the surface from the same side.  A slot collapses to the point (0, 0, 0) - it covers
 * no pixel - when one of its three pixels has no reading, when dmax - dmin > gap * dmin over its three depths (one float32 difference
 * against one float32 product: a depth step, not a surface), when a projected corner has !(z >= near), or when its frame has
 * !(fx > 0 && fy > 0).  One launch, no atomics, no allocation: legal inside a stream capture.  SLN_E_BADARG, nothing launched: a null
 * pointer, B < 1 or > 65535, Hs < 2, Ws < 2, F > 2^24, orig_size <= 0, !(gap >= 0), !(near > 0), faces_xyz not 8-byte aligned. */
int sln_reproject_faces(const SlnReproject* d, float* faces_xyz, void* stream);
/* From the rasterizer's maps (raster order: row 0 = bottom) of the B frames' faces: depth_out [B, S, S] float32 and labels_out
 * [B, S, S] uint8 in the row order of the scene tensor's planes (row 0 = top), hits [B] int64.  A pixel is HIT when its face_index
 * lies in [0, F) and none of its three weights is a NaN: depth_out takes raster_depth's bits and labels_out the byte of labels_src
 * [B, Hs, Ws] at the face's corner of largest weight (ties: the lower corner number in the emitted order) - nearest neighbour in the
 * source image, any byte passes through.  Elsewhere depth_out = -1 (the renderer's background) and labels_out = 0.  hits counts the hit
 * pixels per frame with integer additions only: the same from call to call.  Two launches (hits is cleared first), no allocation,
 * nothing read back: legal inside a stream capture.  Every index read from a map is compared with its range before it addresses
 * anything.  SLN_E_BADARG, nothing launched: a null pointer, B < 1 or > 65535, Hs < 2, Ws < 2, F > 2^24, S < 1 or > 4096, hits not
 * 8-byte aligned. */
int sln_reproject_compose(const int32_t* face_index, const float* weight, const float* raster_depth, const unsigned char* labels_src, int B,
                          int Hs, int Ws, int S, float* depth_out, unsigned char* labels_out, int64_t* hits, void* stream);
/* Several observed frames per room (csrc/observed_fuse.hip; DESIGN §4 "Several observed frames per room").  R rooms, V frames per
 * room: frame b = r * V + v is reprojected as above - sln_reproject_faces over B = R * V frames with a k_src, pose and labels_src of its
 * own and the room's K_tgt, then sln_raster_forward with B = R * V.  From the rasterizer's maps (raster order) of the V frames of a
 * room, per target pixel, into the planes' row order (sln_reproject_compose's row flip):
 *   frame v CONTRIBUTES iff it is a hit by sln_reproject_compose's rule (face_index in [0, F), no NaN among the three weights) and its
 *   rasterizer depth d_v is not a NaN.  The WINNER is the contributing frame of smallest d_v, walking v upwards with a strict <: equal
 *   depths go to the lowest v.  This is the z-buffer rule: of several surfaces on one ray the target view sees the nearest; a frame that
 *   saw a farther one looked past the nearer from elsewhere - it is occluded, not wrong.
 *   depth_out  [R, S, S] float32  the winner's depth, bits untouched; -1.0f where no frame contributes
 *   labels_out [R, S, S] uint8    the byte of the winner's labels_src at the winning face's corner of largest weight (ties: the lower
 *                                 corner number - sln_reproject_compose's rule); 0 where no frame contributes.  A byte of 0 in the
 *                                 winning frame stays 0: no other frame lends a label
 *   source_out [R, S, S] uint8    1 + v of the winner, 0 without one
 *   count_out  [R, S, S] uint8    the number of contributing frames
 *   agree_out  [R, S, S] uint8    the number of contributing frames with !((d_v - dmin) > gap * dmin), dmin the winner's depth: one
 *                                 float32 difference against one float32 product, sln_reproject_faces' depth-step test with the same
 *                                 gap.  The winner counts itself
 *   hits       [R] int64          the pixels with a winner
 *   wins       [R, V] int64       the pixels each frame wins; their sum over v is hits
 * hits and wins are integer sums: the same from call to call under either deterministic setting.  A room with fewer than V frames pads
 * with frames whose k_src has fx = 0: they yield nothing.  With V = 1, depth_out, labels_out and hits are sln_reproject_compose's bit
 * for bit.  source_out, count_out, agree_out and wins are optional (NULL: not computed, nothing written).  The weights of a frame are
 * loaded only when it would become the nearest so far, and - for count_out / agree_out - for the NaN rule of the other in-range
 * candidates.  Two or three launches (hits and wins are cleared first), no allocation, synchronisation, read-back or floating-point
 * atomic: legal inside a stream capture.  Every index read from a map is compared with its range before it addresses anything.
 * SLN_E_BADARG, nothing launched and nothing written: a null required pointer, R < 1, V < 1, V > 255, R * V > 65535, Hs < 2, Ws < 2,
 * S < 1, S > 4096, F > 2^24, !(gap >= 0), hits or wins not 8-byte aligned, depth_out not 4-byte aligned. */
int sln_reproject_fuse(const int32_t* face_index, const float* weight, const float* raster_depth, const unsigned char* labels_src, int R,
                       int V, int Hs, int Ws, int S, float gap, float* depth_out, unsigned char* labels_out, unsigned char* source_out,
                       unsigned char* count_out, unsigned char* agree_out, int64_t* hits, int64_t* wins, void* stream);
/* An observed frame finer than the target, decimated by an integer factor f in [1, 8] in front of sln_reproject_faces
 * (csrc/observed_prefilter.hip; DESIGN §4 "Observed frames finer than the target").  B frames, all device pointers: depth_src
 * [B, Hs, Ws] float32 (a READING iff 0 < d <= 15), labels_src [B, Hs, Ws] uint8 (any byte), k_src [B, 4].  Hd = Hs / f, Wd = Ws / f
 * (integer division); coarse pixel (I, J) owns the n = f * f source pixels [f I, f I + f) x [f J, f J + f); the rows and columns
 * behind f Hd, f Wd are not read.  With r the number of readings of the block:
 *   2 r < n:   depth_out = 0.0f, labels_out = 0 (no reading: the majority of the area says nothing).  Otherwise
 *   dref       the lower median of the block's readings, rank (r - 1) / 2 in ascending order
 *   MEMBERS    the readings d with !((max(d, dref) - min(d, dref)) > gap * min(d, dref)): one float32 difference against one float32
 *              product, sln_reproject_faces' depth-step test; m >= 1 of them
 *   depth_out  [B, Hd, Wd] float32  (float)((double)m / sum), sum adding 1.0 / (double)d over the members in row-major order of the
 *                                   block, every operation a correctly rounded double operation: the harmonic mean - exact at the
 *                                   block's centre on a plane, never a blend of two surfaces
 *   labels_out [B, Hd, Wd] uint8    the most frequent byte among the members, ties to the smallest byte; 0 competes like any other
 *   k_out      [B, 4] float32       k_src / (float)f, four float32 divisions: the exact pinhole of the coarse grid
 *   counts     [B, 3] int64         coarse pixels with m == n, with a reading and m < n, without a reading; or NULL
 * With f = 1 a reading keeps its bits and everything else becomes 0.0f with label 0.  One launch, and a zero-fill launch in front when
 * counts is given; counts are integer sums: the same from call to call under either deterministic setting.  No allocation,
 * synchronisation, read-back or floating-point atomic: legal inside a stream capture.  Every index is formed from the sizes given
 * here.  SLN_E_BADARG, nothing launched and nothing written: a null required pointer, B < 1, B > 65535, f < 1, f > 8, Hs < f, Ws < f,
 * !(gap >= 0), counts not 8-byte aligned, depth_src, depth_out, k_src or k_out not 4-byte aligned, more than 2^31 - 1 tiles of
 * 32 x 2 coarse pixels in a frame. */
int sln_observed_prefilter(const float* depth_src, const unsigned char* labels_src, const float* k_src, int B, int Hs, int Ws, int f,
                           float gap, float* depth_out, unsigned char* labels_out, float* k_out, int64_t* counts, void* stream);

/* =============================================================================================
 * The --draw_3d picture (render/render_room_color.py::render_test): a lit colour picture with hard shadows of the view the viewpoint
 * render accepted (csrc/draw3d.hip; host/draw3d.py).  The shading model is this project's, stated in DESIGN §4 "3-D drawing".
 * ============================================================================================= */
/* What sln_view_place_project, sln_raster_forward and the choice leave on the device, all device pointers.  Room r is drawn from view
 * b = r * V + chosen[r] (chosen is read on the device and clamped to [0, V)). */
typedef struct SlnDraw3D {
  const float* faces_xyz;           /* [R * V, F, 3, 3] (x_ndc, y_ndc, z_cam) */
  const int32_t* face_index;        /* [R * V, S, S] raster order (row 0 = bottom); outside [0, F): background */
  const float* depth;               /* [R * V, S, S] the rasterizer's depth */
  const unsigned char* face_label;  /* [R, F]; a byte above 40 reads albedo entry 0 */
  const int64_t* chosen;            /* [R] */
  const float* K;                   /* [R * V, 3, 3]: fx, fy, cx, cy are read, no skew, orig_size = S */
  const float* light_cam;           /* [R, 3] the lamp in the drawn view's camera frame */
  const float* albedo;              /* [41, 3] linear colour per class byte */
  int32_t R, V, F, S, k, shadows;   /* k: samples per output pixel and axis, P = S / k */
  float ambient, intensity, min_dist, bias, background[3];
} SlnDraw3D;
/* picture [R, P, P, 3] uint8 in image row order (row 0 = top): per output pixel the mean of its k x k linear samples (added row by
 * row), clamped to [0, 1], sRGB-encoded, times 255, rounded to nearest.  linear [R, S, S, 3] float32 in raster order, or NULL.  A
 * sample's linear colour: background where face_index is outside [0, F); else albedo[label] * (ambient + intensity * vis * c / d^2)
 * with p = ray(pixel centre) * depth, n the face's normal turned towards the camera, l = light - p, d^2 = max(|l|^2, min_dist^2),
 * c = max(0, n.l / |l|), and vis = 0 when the segment from p + bias * n to the light meets another face of the view (two-sided
 * Moller-Trumbore, t in (0, 1), barycentrics in [0, 1], a zero determinant is no hit), tested only with `shadows` and c > 0.
 * Two launches (faces of the chosen view into the workspace; lighting and picture), no atomics, no allocation, fixed-order sums:
 * legal inside a stream capture, the same bytes from call to call.  workspace: sln_draw3d_workspace_bytes(R, F) bytes, 16-byte
 * aligned.  SLN_E_BADARG, nothing launched: a null pointer (linear may be NULL), a size < 1, S % k != 0, k > 16, S > 32768,
 * R * V > 65535, F > 2^24, a misaligned workspace. */
int64_t sln_draw3d_workspace_bytes(int R, int F);
int sln_draw3d(const SlnDraw3D* d, void* workspace, unsigned char* picture, float* linear, void* stream);

/* =============================================================================================
 * Splitting long mesh edges before models enter the bank (csrc/mesh_split.hip; host/mesh_prep.py): one pass of the rule of DESIGN §4
 * "Splitting long edges" is three launches, with the host's sort / unique of the keys and scan of the counts between them.  All
 * pointers are device pointers.  No atomics, no allocation, nothing read back; the same bytes from call to call whatever
 * sln_set_deterministic says.  status [4] int32, zeroed by the caller once: word 0 = 1 after a face with an index outside [0, V)
 * (mark), word 1 = 2 after a key that names a vertex outside [0, V) (midpoints), word 2 = 4 after an offset outside the output or
 * a new vertex index outside [V, V + U) (emit).  Nothing is ever read outside v.
 * ============================================================================================= */
/* v [V, 3] float32, f [F, 3] int32.  Edge k of a face joins corners k and (k + 1) % 3; its squared length is (dx*dx + dy*dy) + dz*dz
 * in float64 from the float32 coordinates; it is marked when that exceeds max_edge_sq.  mask [F] int32: bit k = edge k marked;
 * count [F] int32 = 1 + marked edges (the face's children); keys [F, 3] int64 = (min(i, j) << 32) | max(i, j) of a marked edge, -1
 * otherwise.  A face with an index outside [0, V) gets mask 0, count 1, keys -1: it is copied through unsplit.  SLN_E_BADARG,
 * nothing launched: a null pointer, F < 1, V < 1, max_edge_sq not finite or <= 0, V + 3 F >= 2^31. */
int sln_mesh_split_mark(const float* v, int V, const int32_t* f, int F, double max_edge_sq, int32_t* mask, int32_t* count,
                        int64_t* keys, int32_t* status, void* stream);
/* ukeys [U] int64: the sorted unique marked keys.  v_new [U, 3]: float32((double(a) + double(b)) * 0.5) per coordinate of the key's
 * two vertices - vertex V + u of the pass's output; (0, 0, 0) for a key outside the table.  SLN_E_BADARG: a null pointer, V < 1,
 * U < 1, V + U >= 2^31. */
int sln_mesh_split_midpoints(const float* v, int V, const int64_t* ukeys, int U, float* v_new, int32_t* status, void* stream);
/* v_out [V + U, 3]: the old vertices followed by v_new.  mid [F, 3] int32: the new vertex index of every marked edge; offsets [F]
 * int64: the exclusive prefix sum of count; F_out its total.  Writes the children of face i (in the order of DESIGN §4, winding
 * kept) to f_out [F_out, 3] at offsets[i] and origin[i] to origin_out [F_out] beside each.  The quad of a face with two marked
 * edges is cut by the shorter diagonal, compared as squared float64 lengths of the float32 positions in v_out, a tie going to
 * A-M1.  SLN_E_BADARG: a null pointer, F < 1, V < 1, U < 0, V + 3 F or V + U >= 2^31, F_out outside [F, 4 F]. */
int sln_mesh_split_emit(const float* v_out, int V, int U, const int32_t* f, const int32_t* origin, const int32_t* mask,
                        const int64_t* offsets, const int32_t* mid, int F, int F_out, int32_t* f_out, int32_t* origin_out,
                        int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLN_HIP_H */
