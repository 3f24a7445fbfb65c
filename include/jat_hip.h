/*
 * jat_hip.h — C ABI of libjat_hip.so: the MI355X (gfx950) DiT flow-matching sampling path of JaTSR.
 *
 * The reference (HUSRCF/JaTSR) has no plugin/FFI layer; the interface this library replaces is the
 * Python module API of src/models/jat_audiosr_v3.py and the sampler in infer_test_v3m2.py.
 * Each entry point cites the reference symbol it stands in for (file:line relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *   - tensors are dense row-major fp32 unless a comment says otherwise;
 *   - every call enqueues its work on the caller's hipStream_t (passed as void*) and returns without
 *     synchronising; no allocation happens after *_create / *_load_weights;
 *   - return value: 0 = ok, negative = error (JAT_E_*), message via jat_last_error() (thread-local);
 *   - nothing throws across the ABI; a handle is used from one host thread at a time (one per device).
 */
#ifndef JAT_HIP_H
#define JAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_OK 0
#define JAT_E_INVALID (-1)   /* bad argument / unsupported shape (mirrors ValueError / AssertionError) */
#define JAT_E_HIP (-2)       /* a HIP runtime call failed */
#define JAT_E_STATE (-3)     /* weights not loaded, workspace too small, ... */
#define JAT_E_SEQLEN (-4)    /* N = ceil(T/4) > max_len (2048): jat_audiosr_v3.py:451-452 raises ValueError */

#define JAT_NORM_RMS_W 0        /* nn.RMSNorm(D, eps=1e-6) with weight: jat_audiosr_v3.py:261,264,384 */
#define JAT_NORM_LN_NOAFFINE 1  /* nn.LayerNorm(D, elementwise_affine=False, eps=1e-6): jat_audiosr_v2.py:242,245,361 */

typedef struct jat_model jat_model;
typedef struct jat_sampler jat_sampler;

/* Constructor arguments of JaT_AudioSR_V3 (jat_audiosr_v3.py:320-331); dropout / drop_path are
 * training-only and have no effect on this (eval) path. */
typedef struct jat_config {
  int32_t input_channels;  /* 1024 */
  int32_t cond_channels;   /* 1024 */
  int32_t patch_len;       /* 4 (the only supported value) */
  int32_t hidden_size;     /* D, multiple of 256 */
  int32_t depth;
  int32_t num_q_heads;     /* hidden_size / num_q_heads must be 64 */
  int32_t num_kv_heads;
  int32_t bottleneck_dim;  /* multiple of 128 */
  int32_t mlp_hidden;      /* int(hidden_size * mlp_ratio), multiple of 128 */
  int32_t norm_mode;       /* JAT_NORM_* */
} jat_config;

/* One named fp32 parameter of the reference state_dict (device pointer, [out,in] row-major for Linear
 * weights).  Names are the reference's keys, e.g. "blocks.3.attn.q_proj.weight". */
typedef struct jat_tensor_ref {
  const char* name;   /* [host] */
  const float* data;  /* device */
  int64_t numel;
} jat_tensor_ref;

const char* jat_last_error(void);
int jat_version(void);
/* Operand dtype this library was built for: 0 = bf16 (libjat_hip.so: the sampler and the V3-class trainers' autocast,
 * train_ddp_v3m2.py:545), 1 = fp16 (libjat_hip_fp16.so: torch.amp.autocast('cuda') of train_ddp_v3mod2.py:854). */
int jat_operand_dtype(void);

/* ---- model: JaT_AudioSR_V3 / _V2 (jat_audiosr_v3.py:311-471) ------------------------------------ */
int jat_model_create(const jat_config* cfg, jat_model** out);
void jat_model_destroy(jat_model* m);
/* == load_state_dict (infer_test_v3m2.py:61-74): borrows the fp32 tensors for the duration of the call
 * (synchronises `stream` before returning), packs them once into bf16 (fused [Wq;Wk;Wv], all layers'
 * adaLN weights concatenated) plus fp32 copies of biases / norm weights / t_embedder.  Unknown names
 * (e.g. the persistent RoPE buffers) are ignored; missing names are an error unless norm weights in
 * LN_NOAFFINE mode. */
int jat_model_load_weights(jat_model* m, const jat_tensor_ref* named, int32_t n, void* stream);
int jat_model_workspace_bytes(const jat_model* m, int32_t B, int32_t T, size_t* out);
/* Behaviour switches of this handle.  Their defaults come from the JAT_* environment variables, which are read ONCE, in
 * jat_model_create (INTEGRATION.md "Environment switches"); nothing on the enqueue path reads the environment.  Names:
 * "fuse_qkv_attn" (0 / 1 / 2), "qkv_split", "fuse_finish", "fold_norm" (0 / 1 / 2), "split_patch", "patch_split", "fold_cap_mb",
 * "fuse_euler" (CFG sampler: CFG combine + Euler step inside the final Linear, the latent kept in patch layout over the steps).
 * Takes effect for forwards enqueued and samplers created afterwards. */
int jat_model_set_switch(jat_model* m, const char* name, int32_t value);

/* == JaT_AudioSR_V3.forward(x_t, t, x_cond) in eval mode (jat_audiosr_v3.py:422-471).
 * x_t, x_cond, x_pred: [B, input_channels, T]; t: [B].  Pads T to a multiple of 4 internally (:435-439),
 * trims on output (:468-469).  Inputs are not modified. */
int jat_forward(jat_model* m, const float* x_t, const float* t, const float* x_cond, float* x_pred,
                int32_t B, int32_t T, void* workspace, size_t workspace_bytes, void* stream);

/* == DiTBlock_GQA.forward(x, t_emb) (jat_audiosr_v3.py:284-308): x,y [B,N,D], t_emb [B,D]. */
int jat_block_forward(jat_model* m, int32_t layer, const float* x, const float* t_emb, float* y,
                      int32_t B, int32_t N, void* workspace, size_t workspace_bytes, void* stream);
/* == GroupedQueryAttention.forward(x) (jat_audiosr_v3.py:144-184): x,y [B,N,D]. */
int jat_attn_forward(jat_model* m, int32_t layer, const float* x, float* y, int32_t B, int32_t N,
                     void* workspace, size_t workspace_bytes, void* stream);
/* == t_embedder(t) (jat_audiosr_v3.py:364-369,455): t [B] -> t_emb [B,D]. */
int jat_time_embed(jat_model* m, const float* t, float* t_emb, int32_t B, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- sampler: flow_matching_sample (infer_test_v3m2.py:107-185) ------------------------------------ */
/* Builds, for a fixed (B, T, steps, cfg_scale): the schedule linspace(0,1,steps+1) (:136) as host floats,
 * the [steps, depth, 6D] adaLN modulation table (all rows of a step share one t, :150), private state
 * buffers, and ONE hipGraph holding all `steps` CFG double-batch forwards + Euler updates. */
int jat_sampler_create(jat_model* m, int32_t B, int32_t T, int32_t steps, float cfg_scale,
                       jat_sampler** out);
/* ---- solvers and time grids ----
 * x^(z, t) = CFG combine of the two predictions; den(t) = fp32(fp32(1 - t) + 1e-5); v(z, t) = (x^ - z) / den(t).  A grid is fp32,
 * strictly increasing, from exactly 0 to exactly 1.  Step i: t = times[i], dt = fp32(times[i+1] - t), h = fp32(dt / 2).
 *   JAT_SOLVER_EULER:    z' = z + dt v(z, t); from t >= 0.999 on z' = x^ (the reference's step, infer_test_v3m2.py:161-179)
 *   JAT_SOLVER_MIDPOINT: z~ = z + h v(z, t);   z' = z + dt v(z~, t2),              t2 = fp32(t + h)
 *   JAT_SOLVER_HEUN:     z~ = z + dt v(z, t);  z' = z/2 + z~/2 + h v(z~, t2),      t2 = times[i+1]
 * A step whose t2 is not < 0.999 is taken as the Euler step (v is singular at t = 1): Heun on N steps costs 2N - 1 evaluations. */
#define JAT_SOLVER_EULER 0
#define JAT_SOLVER_MIDPOINT 1
#define JAT_SOLVER_HEUN 2
/* One model evaluation of a run.  stage 0: the Euler step of length c (direct != 0: z' = x^).  stage 1: z_base = z, then the Euler
 * formula with step length c (save != 0).  stage 2: z' = a z_base + b z + c (x^ - z) / den.  time_index: the position of t among
 * the run's distinct evaluation times (bit-equal fp32 values share one modulation row and one folded-weight entry). */
typedef struct jat_solver_eval {
  float t;
  int32_t time_index;
  float den, a, b, c;
  int32_t stage, save, direct;
} jat_solver_eval;
/* The evaluation list of `solver` over times[n] (NULL: torch.linspace(0, 1, n) in fp32).  Host code only: no device is touched.
 * evals / distinct (either may be NULL) have room for `cap` entries; 2 (n - 1) always suffice.  *n_evals / *n_distinct (may be
 * NULL) are set whenever the grid and the solver are valid.  JAT_E_INVALID: n < 2, a grid that does not start at 0, end at 1 and
 * strictly increase (a NaN never does), an unknown solver, or too little room. */
int jat_solver_plan(const float* times, int32_t n, int32_t solver, jat_solver_eval* evals, int32_t cap, int32_t* n_evals,
                    float* distinct, int32_t* n_distinct);
/* jat_sampler_create with a solver and a time grid of n_times values (times == NULL: linspace(0, 1, n_times));
 * jat_sampler_create(m, B, T, steps, s, out) is jat_sampler_create_ex(m, B, T, NULL, steps + 1, JAT_SOLVER_EULER, s, out).
 * The whole evaluation list is captured as one graph; the folded-weight table is shared between samplers of one model whose
 * lists of distinct times are equal.  The LR latent is the condition and has the sampled latent's shape [B, input_channels, T]: a
 * model with cond_channels != input_channels is JAT_E_INVALID here (its forward, jat_forward, takes both counts). */
int jat_sampler_create_ex(jat_model* m, int32_t B, int32_t T, const float* times, int32_t n_times, int32_t solver,
                          float cfg_scale, jat_sampler** out);
void jat_sampler_destroy(jat_sampler* s);
/* What the sampler's captured graph runs: *folded != 0 = per-step folded weights (0 after the fallback to the
 * norm kernels: not an RMSNorm model, over the "fold_cap_mb" switch, or the table did not fit the device), *fused_attn != 0 = the
 * fused QKV + RoPE + attention kernel, *fold_bytes = size of the folded-weight table shared through the model.  Any pointer
 * may be NULL. */
int jat_sampler_info(const jat_sampler* sampler, int32_t* folded, int32_t* fused_attn, int64_t* fold_bytes);
/* 1 when the sampler's steps run the fused tail: the final Linear walks the cond / uncond rows in pairs and applies
 * the CFG combine + Euler update (:161-179) in its epilogue to the latent kept in patch layout, so no unpatchify store, no
 * jat_cfg_euler_step launch and no per-step patchify run.  Needs cfg_scale != 1, the "split_patch" and "fuse_euler" switches, T % 4 == 0
 * and a final-Linear tile that has the epilogue; 0: the separate launches.  Both produce the same bits. */
int jat_sampler_tail_fused(const jat_sampler* sampler);
/* Rows of the bucket that are SHORTER than T (the last chunk of a file, infer_test_v3m2.py:353-361,370-398, batched with
 * the full-length chunks instead of sampled alone): frames[b] in (0, T] valid latent frames of row b; the caller zero-pads
 * lr_latent / z0 beyond them and ignores z_out there.  Attention masks the padded keys, every other operator is row-wise,
 * so the valid frames equal a stand-alone run of frames[b] frames.  Sticky until set again.  Not available for buckets of
 * exactly 128 tokens that run the fused QKV+attention kernel (JAT_E_STATE). */
int jat_sampler_set_lengths(jat_sampler* sampler, const int32_t* frames, int32_t n, void* stream);

/* lr_latent, z0_noise, z_out: [B, C, T].  z0_noise replaces torch.randn at :133 (caller-supplied so that
 * results are reproducible).  use_graph=0 replays the same kernels eagerly (debug / A-B timing). */
int jat_sampler_run(jat_sampler* s, const float* lr_latent, const float* z0_noise, float* z_out,
                    int32_t use_graph, void* stream);
/* One CFG combine + Euler update (infer_test_v3m2.py:161-179) in place on z [B,C,T];
 * x_pred_2B = [cond; uncond] is [2B,C,T] when cfg_scale != 1, else [B,C,T]. */
int jat_cfg_euler_step(const float* x_pred_2B, float* z, float cfg_scale, float t, float dt, int32_t B,
                       int32_t C, int32_t T, void* stream);

/* One stage of a two-stage solver in place on z [B,C,T], z_base [B,C,T] beside it; den = fp32(fp32(1 - t) + 1e-5).
 * save != 0: z_base = z, z += (x^ - z) / den * c.   save == 0: z = a z_base + b z + c (x^ - z) / den. */
int jat_cfg_stage_step(const float* x_pred_2B, float* z, float* z_base, float cfg_scale, float t, float a, float b, float c,
                       int32_t save, int32_t B, int32_t C, int32_t T, void* stream);

/* ---- chunk driver pieces (infer_test_v3m2.py:188-233, 381-394) ------------------------------------- */
/* out[c,t] = (in[c,t] - mean[c]) / std[c]   (inverse=0)  |  in[c,t]*std[c] + mean[c]   (inverse=1) */
int jat_channel_affine(const float* in, const float* mean, const float* std, float* out, int32_t B,
                       int32_t C, int32_t T, int32_t inverse, void* stream);
/* Linear crossfade of `prev` tail with `cur` head over `overlap` frames into out [rows, Tp+Tc-overlap]. */
int jat_crossfade_pair(const float* prev, int32_t Tp, const float* cur, int32_t Tc, int32_t overlap,
                       float* out, int32_t rows, void* stream);

/* ---- training step (train_ddp_v3m2.py:533-622) ------------------------------------ */
/* The step is split at its only cross-device boundary, the DDP gradient all-reduce (train_ddp_v3m2.py:486,610):
 *   jat_trainer_prepare   z_t = t x + (1-t) eps, cond noise, CFG condition dropout            (:548-579)
 *   jat_trainer_fwd_bwd   pred = model(z_t, t, cond); loss = mse_loss(pred, target); backward  (:582-610)
 *   [caller: all-reduce(grads_flat) / world_size over RCCL when world_size > 1]
 *   jat_trainer_optim     unscale, clip_grad_norm_(max_norm), AdamW, re-pack bf16 operands     (:613-619)
 * Parameters, gradients and the two AdamW moments are four caller-owned flat fp32 device buffers of `total` floats
 * (total % 4 == 0); `params` names the reference state_dict tensors as 16-byte aligned slices of params_flat, and the
 * gradient / moment of a tensor lives at the same offset of its buffer.  Gaps between tensors must be zero-filled.
 * Dropout (attention probabilities :175, MLP :269,271) and DropPath (:38-64, :300,306) draw their masks from a
 * counter-based generator keyed by (rng_seed of the step, layer, site, element index) — the same Bernoulli(1-p) / (1-p)
 * semantics as nn.Dropout / drop_path, a different random stream than torch's Philox.  Per-rank batch B <= 32.  The condition
 * is a latent of the target's shape: a model with cond_channels != input_channels is JAT_E_INVALID at creation. */
typedef struct jat_trainer jat_trainer;
int jat_trainer_create(jat_model* m, const jat_tensor_ref* params, int32_t n_params, float* params_flat,
                       float* grads_flat, float* exp_avg, float* exp_avg_sq, int64_t total, int32_t B, int32_t T,
                       void* stream, jat_trainer** out);
void jat_trainer_destroy(jat_trainer* tr);
/* Overlap of the gradient all-reduce with the backward (what DDP's bucket hooks do, train_ddp_v3m2.py:486): `hook` is
 * called on the host thread, during enqueue, each time the last kernel writing a contiguous slice grads_flat[off, off+n)
 * has been enqueued on the step's stream — the final layer first, then blocks depth-1 .. 0 (one slice per block,
 * 109 MB for v3mod2), then patch_embed + t_embedder; the slices tile [0, total) exactly once per jat_trainer_fwd_bwd.
 * The callee orders a collective behind the work enqueued so far (event on the stream) and returns.  NULL: off. */
int jat_trainer_set_grad_hook(jat_trainer* tr, void (*hook)(int64_t off, int64_t n, void* user), void* user);
/* Per-layer rates (host arrays [depth]): dropout[l] = the block's nn.Dropout p (jat_audiosr_v3.py:262,269,271),
 * drop_path[l] = linspace(0, drop_path_rate, depth)[l] (:372-377).  Default: all zero. */
int jat_trainer_set_regularisers(jat_trainer* tr, const float* dropout, const float* drop_path);
/* Loss of the v3mod2 trainer (train_ddp_v3mod2.py:53-321,889-896):
 *   loss = mse + latent_weight * (freq_weight * FrequencyDomainLatentLoss + ms_weight * MultiScaleLatentLoss
 *                                 + consistency_weight * HybridConsistencyLoss(pred, clean LR latent))
 * with the reference's defaults 0.3 / 0.5 / 0.5 / 0.1 and band ratios 0.3 / 0.30 / 0.36 (TrainConfig :362-372); fp32 rFFT
 * over T as in the reference (:90-95).  latent_weight == 0 (the default) is the MSE-only loss of train_ddp_v3m2.py:585. */
int jat_trainer_set_latent_loss(jat_trainer* tr, double latent_weight, double freq_weight, double ms_weight,
                                double consistency_weight, double low_freq_phase_ratio, double strict_cutoff,
                                double soft_cutoff);
/* Reconstruction loss of the V3M2-MOD1 trainer (train_ddp_v3m2mod1.py:72-101,150-151,666-672):
 *   charbonnier_loss(pred, target, eps) = mean(sqrt((pred - target)^2 + eps)),  eps = 1e-6 (ADDED to the squared difference)
 * eps > 0 selects it, eps == 0 returns to F.mse_loss.  Not combinable with the latent perceptual loss (JAT_E_STATE). */
int jat_trainer_set_charbonnier(jat_trainer* tr, double eps);
/* The whole loss of the V3-MOD3 trainer in one call (train_ddp_v3mod3.py:57-85,400-434,955-969; validation :1138-1159):
 *   loss = recon_weight * recon + latent_weight * (freq_weight * freq + ms_weight * ms + consistency_weight * consistency)
 * recon = charbonnier_loss(pred, target, recon_eps) for recon_eps > 0 (`use_charbonnier_loss`), F.mse_loss for recon_eps == 0;
 * the reference's defaults are 1e-6 / 1.0 / 0.3 / 0.5 / 0.5 / 0.1 and the band ratios of jat_trainer_set_latent_loss.  With a latent
 * weight the reconstruction term is computed inside the latent loss kernels (no pass of its own over the prediction); with
 * latent_weight == 0 the plain MSE / Charbonnier kernels run and recon_weight scales their result.  (0, 1, ...) is exactly
 * jat_trainer_set_latent_loss.  Everything is validated before anything is stored: JAT_E_INVALID for a negative or non-finite
 * recon_eps, a non-finite weight or bad band ratios; recon_weight == 0 is legal.  The two setters above keep rejecting each other
 * (JAT_E_STATE) whatever this call stored. */
int jat_trainer_set_loss_ex(jat_trainer* tr, double recon_eps, double recon_weight, double latent_weight, double freq_weight,
                            double ms_weight, double consistency_weight, double low_freq_phase_ratio, double strict_cutoff,
                            double soft_cutoff);
/* out6 (device): {total, mse, freq, ms, consistency, weighted latent sum} of the latest jat_trainer_fwd_bwd.  Slot 1 is the
 * reconstruction term, un-weighted, whatever its kind (the Charbonnier mean after jat_trainer_set_loss_ex with recon_eps > 0). */
int jat_trainer_loss_terms(jat_trainer* tr, float* out6, void* stream);
int jat_trainer_workspace_bytes(const jat_trainer* tr, size_t* out);
/* Re-derive every operand copy (bf16 weights and their transposes, fp32 operand tensors) from params_flat after the
 * caller overwrote parameters — checkpoint resume, train_ddp_v3m2.py:443-500. */
int jat_trainer_repack(jat_trainer* tr, void* stream);
/* hr_norm, noise, z_t: [B,C,T]; cond [B,Cc,T] is modified in place: cond = (cond + cond_noise * ratio *
 * (adaptive ? clamp(std(cond), 0.5, 2) : 1)) * keep[b]   (cond_noise / keep may be NULL); t [B]. */
int jat_trainer_prepare(jat_trainer* tr, const float* hr_norm, float* cond, const float* noise,
                        const float* cond_noise, float cond_noise_ratio, int32_t adaptive, const float* keep,
                        const float* t, float* z_t, void* stream);
/* Overwrites grads_flat with d(loss * loss_scale)/d(param); loss_out (device, 1 float, nullable) = unscaled loss;
 * x_pred_out (device [B,C,T], nullable) = the prediction.  cond_clean [B,C,T]: the normalised LR latent before the
 * condition noise (lr_norm_original, train_ddp_v3mod2.py:861), read only by the consistency loss (may be NULL otherwise). */
int jat_trainer_fwd_bwd(jat_trainer* tr, const float* z_t, const float* t, const float* x_cond, const float* target,
                        const float* cond_clean, float loss_scale, uint64_t rng_seed, float* loss_out, float* x_pred_out,
                        void* stream);
/* Gradient accumulation over the micro-batches of one optimiser step: jat_trainer_fwd_bwd with `flags` (0 = that call).
 *   JAT_FB_ACCUMULATE: every kernel that writes a parameter gradient computes the fp32 value it would have stored and adds it
 *     to the resident one, grads_flat = grads_flat + d(loss * loss_scale)/d(param): one rounded add per element, no atomics (a
 *     step stays bit-reproducible), no extra buffer, no pass of its own over grads_flat.  loss_out and the six terms behind
 *     jat_trainer_loss_terms add to their previous values as well: after k calls (the first without the flag) they hold the
 *     sums over the k micro-batches, and the host divides by k after its one read-back.  The 1/k of the gradients rides on
 *     jat_trainer_optim's un-scale factor: pass loss_scale * k there.  A trainer one of whose weight-gradient paths cannot
 *     accumulate fails with JAT_E_STATE before anything is queued; nothing ever overwrites silently.
 *   JAT_FB_NO_HOOK: the gradient-ready hook (jat_trainer_set_grad_hook) is not called: this is not the last micro-batch, so
 *     an overlapped gradient exchange runs once per optimiser step, on the summed gradients.
 * With the second (weight-gradient) stream, an accumulating call reads what the previous call's second stream wrote; every
 * call, failed ones included, ends with that stream joined into `stream`.  Other flag bits: JAT_E_INVALID. */
#define JAT_FB_ACCUMULATE 1   /* add d(loss*loss_scale)/d(param) to grads_flat instead of overwriting it */
#define JAT_FB_NO_HOOK    2   /* do not call the gradient-ready hook: this is not the last micro-batch */
int jat_trainer_fwd_bwd_ex(jat_trainer* tr, const float* z_t, const float* t, const float* x_cond, const float* target,
                           const float* cond_clean, float loss_scale, uint64_t rng_seed, float* loss_out, float* x_pred_out,
                           int32_t flags, void* stream);
/* grads_flat is read, not modified (clip_grad_norm_'s in-place scaling of .grad is not reproduced: nothing reads it).
 * grad_norm_out (device, 1 float, nullable) = L2 norm of the loss-SCALED gradients (divide by loss_scale).  A
 * non-finite norm leaves parameters and moments untouched (GradScaler.step).  `step` is 1-based (bias correction). */
int jat_trainer_optim(jat_trainer* tr, float lr, float beta1, float beta2, float eps, float weight_decay,
                      float max_grad_norm, float loss_scale, int32_t step, float* grad_norm_out, void* stream);
/* Exponential moving average of the parameters (the reference trainers keep none).  ema_flat: a caller-owned device buffer
 * of `total` floats in the layout of params_flat (16-byte aligned, not params_flat itself), which the caller initialises;
 * NULL turns the average off (the default).  While one is set, jat_trainer_optim's AdamW pass also does
 *   ema += (1 - decay) * (p_new - ema)
 * on the float4 it has just updated; a skipped step (non-finite norm) leaves ema untouched.  decay in [0, 1), else
 * JAT_E_INVALID; may be called again at any time to change the decay (a warm-up schedule sets it before every step). */
int jat_trainer_set_ema(jat_trainer* tr, float* ema_flat, float decay);
/* Exchange the contents of params_flat and ema_flat in place (no temporary), then re-derive every operand copy as
 * jat_trainer_repack does: forwards and samplers created afterwards run on the average; a second call restores the training
 * weights bit for bit.  JAT_E_STATE when no average is set. */
int jat_trainer_swap_ema(jat_trainer* tr, void* stream);

/* ---- per-kernel entry points (unit parity tests; bench roofline leg) --------------------------------- */
/* y_bf16[M,D] = norm(x[M,D]) (* w) * (1 + scale[b]) + shift[b], b = row / rows_per_batch;
 * shift/scale may be NULL (no modulation); mod_bstride = element stride between batches (0 = shared). */
int jat_k_norm_modulate(const float* x, const float* w, const float* shift, const float* scale,
                        int64_t mod_bstride, uint16_t* y_bf16, int32_t M, int32_t D, int32_t rows_per_batch,
                        int32_t norm_mode, void* stream);
/* C[M,N] (+bias) = A_bf16[M,K] * W_bf16[N,K]^T ; epilogue: 0 = fp32 out, 1 = bf16 out, 2 = bf16 GELU(erf),
 * 3 = fp32 out += gate[b]*(acc+bias) (gate [B, N] with stride gate_bstride).  variant: the id of a live tile variant
 * (csrc/gemm_variants.h; there is no default: retired and unknown ids, 0 among them, are rejected). */
int jat_k_gemm(const uint16_t* A, const uint16_t* W, const float* bias, void* C, int32_t M, int32_t N,
               int32_t K, int32_t epilogue, const float* gate, int64_t gate_bstride, int32_t rows_per_batch,
               int32_t variant, void* stream);
/* The same GEMM with the sampler's norm folding (computes jat_audiosr_v3.py:297-306 for rows that share one
 * modulation): the residual stream lives as two 16-bit planes x = hi + lo.
 *   producer (hi != NULL; epilogue 0 or 3): x_new = acc + bias (0) | (hi + lo) + gate[b] * (acc + bias) (3), written back
 *     as hi = round(x_new), lo = round(x_new - hi), plus part_out[M, N / jat_k_gemm_wave_n(variant)]: partial row sums of
 *     x_new^2 in fixed order.  C is not touched.
 *   consumer (part_in != NULL; any epilogue): accumulator row m scaled by rsqrt(sum_j part_in[m][j] / K + 1e-6) before the
 *     bias; part_in_np in {4, 8, 16}.
 * Variants with the coalesced epilogue only (CE != 0 in csrc/gemm_variants.h: every live one but 10). */
int jat_k_gemm_fold(const uint16_t* A, const uint16_t* W, const float* bias, void* C, int32_t M, int32_t N, int32_t K,
                    int32_t epilogue, const float* gate, int64_t gate_bstride, int32_t rows_per_batch, uint16_t* hi,
                    uint16_t* lo, float* part_out, const float* part_in, int32_t part_in_np, int32_t variant, void* stream);
/* The CFG sampler's step tail on caller buffers: the final Linear [M = 2 B ntok, N = 4 C, K] over A = [cond rows ; uncond rows]
 * (rows_per_batch = ntok tokens per sample; part_in as in jat_k_gemm_fold's consumer side), the CFG combine + Euler update of
 * jat_cfg_euler_step(t, dt) and the next step's bf16 patch operand a_patch [M/2, N] (frames: optional [B] valid frames per
 * sample, a_patch reads zero from there on; NULL: all).
 *   fused != 0: ONE launch; z is the latent in PATCH layout [M/2, N] (element [(b, tok)][c*4 + p] = latent[b][c][4 tok + p]),
 *     updated in place; xpred is not used.  Variants 20, 28, 33, 35 (csrc/gemm_variants.h).
 *   fused == 0: the three launches it replaces: unpatchify store into xpred [2B, C, 4 ntok], jat_cfg_euler_step on z [B, C, 4 ntok],
 *     patchify of z.  Same bits as the fused form, in the other layout. */
int jat_k_gemm_cfg_euler(const uint16_t* A, const uint16_t* W, const float* bias, int32_t M, int32_t N, int32_t K,
                         int32_t rows_per_batch, const float* part_in, int32_t part_in_np, float* z, uint16_t* a_patch,
                         float* xpred, const int32_t* frames, float cfg_scale, float t, float dt, int32_t variant, int32_t fused,
                         void* stream);
/* The same tail for one stage of a two-stage solver (jat_cfg_stage_step): z_base has the layout z has (patch layout when
 * fused != 0, [B, C, 4 ntok] otherwise).  Same variants, same bits in both forms. */
int jat_k_gemm_cfg_stage(const uint16_t* A, const uint16_t* W, const float* bias, int32_t M, int32_t N, int32_t K,
                         int32_t rows_per_batch, const float* part_in, int32_t part_in_np, float* z, float* z_base,
                         uint16_t* a_patch, float* xpred, const int32_t* frames, float cfg_scale, float t, float a, float b,
                         float c, int32_t save, int32_t variant, int32_t fused, void* stream);
/* Split-K slices of the same product: parts[z][M][N] fp32 = A[:, z K/ksplit : (z+1) K/ksplit] W[:, same]^T, z < ksplit, no
 * bias; summed in order by the caller / the finishing pass.  This is what the un-folded forward's fc2 and out_proj
 * (jat_audiosr_v3.py:300,306) launch when their tiles would leave CUs idle; variant 39 = the 224 x 160 k-step-pair tile
 * (M % 224 == 0, N % 160 == 0, K / ksplit a multiple of 64 and >= 192). */
int jat_k_gemm_splitk(const uint16_t* A, const uint16_t* W, float* parts, int32_t M, int32_t N, int32_t K, int32_t ksplit,
                      int32_t variant, void* stream);
/* Fused QKV projection + RoPE + GQA attention for 128-token samples (the sampler's form of jat_audiosr_v3.py:154-181 when
 * B * Hkv blocks fill the chip): A [M, K] (M % 128 == 0), Wg = the group-major fused weight [Hkv][5*64 + 64 + 64][K] with q / k rows
 * pair-interleaved per head (as jat_model_load_weights packs it), out [M, Hkv*320] = attention output; bias / part_in as in
 * jat_k_gemm_fold's consumer side (folded norms). */
int jat_k_qkv_attn(const uint16_t* A, const uint16_t* Wg, const float* bias, uint16_t* out, int32_t M, int32_t Hkv, int32_t K,
                   const float* rope_inv_freq, const float* part_in, int32_t part_in_np, void* stream);
/* columns per wave tile of a GEMM tile variant (the slot width of part_out); 0 for an unknown variant */
int jat_k_gemm_wave_n(int32_t variant);
/* The tile variant and the K-slice count (1 = none) the forward of `m` launches for a GEMM [M, N, K] at a call site: 0 qkv,
 * 1 out_proj, 2 fc1, 3 fc2, 4 everything else.  The split-K plans apply where N is the width the site has in the model (qkv:
 * D + 2 kvD; out_proj, fc2: D; 4 with N = bottleneck_dim: the first patch-embed Linear); any other N is planned as a plain GEMM.
 * folding != 0: as in a sampler bucket that runs with folded norms.  Host arithmetic only: needs no weights and no GPU. */
int jat_k_gemm_plan(const jat_model* m, int32_t site, int32_t M, int32_t N, int32_t K, int32_t folding, int32_t* variant,
                    int32_t* ksplit);
/* Weight gradient of y = x W^T + b from token-major operands: dW[out,in] = dY[tokens,out]^T X[tokens,in] (fp32), db[out] =
 * column sums of dY (db may be NULL).  out and in multiples of 128; ksplit >= 1 slices of the token axis summed in order
 * (0 = the count that fills the chip, at most 16); work: 256 + (ksplit > 1 ? ksplit*out*in*4 : 0) + 32*out*4 bytes.  (The backward of every nn.Linear of
 * models/JaT_V3.py under train_ddp_v3m2.py:601.) */
int jat_k_weight_grad(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int32_t tokens, int32_t out, int32_t in,
                      int32_t ksplit, void* work, size_t work_bytes, void* stream);
/* The same with the accumulate mode of JAT_FB_ACCUMULATE: accumulate != 0 adds the result to what dW (and db) hold, dW = dW +
 * dY^T X — in the GEMM's epilogue when ksplit == 1, else in the ordered sum of the slices; bit for bit the overwrite result
 * added to the old contents.  accumulate == 0 is jat_k_weight_grad. */
int jat_k_weight_grad_ex(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int32_t tokens, int32_t out, int32_t in,
                         int32_t ksplit, void* work, size_t work_bytes, int32_t accumulate, void* stream);
/* The launch jat_k_weight_grad (ksplit == 0) and the trainer make of a weight [out, in] over `tokens` rows: tile = 128 or 256
 * (the square output tile of the GEMM kernel), ksplit = the K slices (1..16).  JAT_E_INVALID for a NULL output, a non-positive
 * size, or widths that are not multiples of 128.  Host arithmetic only: launches nothing and needs no GPU. */
int jat_k_weight_grad_plan(int32_t out, int32_t in, int32_t tokens, int32_t* tile, int32_t* ksplit);
/* GQA attention on bf16 q[M,Hq*64], k[M,Hkv*64], vt[B,Hkv,64,Npad] -> o[M,Hq*64]; softmax(q k^T / 8) v. */
int jat_k_attention(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, int32_t B,
                    int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, void* stream);
/* jat_k_attention with per-sample key counts, as Sampler.run(lengths=...) runs a short chunk in a bucket of longer ones: lens
 * [B] int32 on the device; every query row of sample b (the rows past lens[b] included: the next layer reads them) attends to
 * the keys < lens[b] alone, whatever k and vt hold beyond them.  Same launch as jat_k_attention (jat_k_attention_route).
 * Precondition: lens[b] >= 1 (a sample without a key has no softmax; the sampler refuses such a length); values above N act
 * as N.  JAT_E_INVALID for a NULL lens. */
int jat_k_attention_lens(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, const int32_t* lens, int32_t B,
                         int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, void* stream);
/* The kernel jat_k_attention / jat_k_attention_train, the forward, the sampler and the trainer launch for N tokens per sample with
 * V padded to Npad keys, for a call with (training forward) or without an lse output and with or without dropout: group = 1: the
 * group kernel (K / V staged once per KV head, N <= 128); group = 0: the streaming kernel with qt * 16 queries per wave (qt 1
 * or 2) and kvb keys per staged block (64 or 128).  Follows JAT_ATTN_GROUP / JAT_ATTN_QT / JAT_ATTN_KVB, which are read once
 * per process.  JAT_E_INVALID for a NULL output, N <= 0, or an Npad that is no multiple of 64 or below N.  Host arithmetic only:
 * launches nothing and needs no GPU. */
int jat_k_attention_route(int32_t N, int32_t Npad, int32_t has_lse, int32_t has_dropout, int32_t* group, int32_t* qt,
                          int32_t* kvb);
/* The v3mod2 loss (see jat_trainer_set_latent_loss) on pred / target / clean-LR tensors [rows, T]: dpred = d(total *
 * loss_scale)/d pred, out6 = {total, mse, freq, ms, consistency, weighted latent sum}; work: align_up(T*8, 256) + rows*32
 * bytes of device scratch. */
int jat_k_latent_loss(const float* pred, const float* target, const float* lr, float* dpred, float* out6,
                      int32_t rows, int32_t T, double latent_weight, double freq_weight, double ms_weight,
                      double consistency_weight, double low_freq_phase_ratio, double strict_cutoff, double soft_cutoff,
                      float loss_scale, void* work, size_t work_bytes, void* stream);
/* jat_k_latent_loss with the reconstruction term of jat_trainer_set_loss_ex: total = recon_weight * recon + latent_weight * (...),
 * out6[1] = recon, un-weighted (Charbonnier mean for recon_eps > 0, MSE for 0).  The same work buffer, and the same rejections
 * before anything is launched, plus JAT_E_INVALID for a negative or non-finite recon_eps or a non-finite weight.  recon_eps == 0
 * with recon_weight == 1 runs the very kernels of jat_k_latent_loss. */
int jat_k_latent_loss_ex(const float* pred, const float* target, const float* lr, float* dpred, float* out6, int32_t rows,
                         int32_t T, double recon_eps, double recon_weight, double latent_weight, double freq_weight,
                         double ms_weight, double consistency_weight, double low_freq_phase_ratio, double strict_cutoff,
                         double soft_cutoff, float loss_scale, void* work, size_t work_bytes, void* stream);
/* The code path the v3mod2 loss takes at sequence length T, which depends on T alone: kind 0 = rejected (T too long for the
 * kernels' LDS image; jat_k_latent_loss and the trainer fail), 1 = direct DFT kernel with (a, b) = (bins, samples) per thread
 * (1, 2), (2, 4) or (3, 6), the last looping in chunks beyond 768 bins / 1536 samples, 2 = DFT factored T = a * b with a the
 * largest divisor of T not above sqrt(T).  lds_bytes = dynamic LDS of that launch (kind 0: what the direct kernel would need).
 * Host arithmetic only: launches nothing and needs no GPU. */
int jat_k_latent_loss_plan(int32_t T, int32_t* kind, int32_t* a, int32_t* b, int64_t* lds_bytes);
/* Reconstruction loss on n elements: eps == 0: F.mse_loss (train_ddp_v3m2.py:585), eps > 0: charbonnier_loss
 * (train_ddp_v3m2mod1.py:72-101); dpred = d(loss * loss_scale)/d pred, loss_out: 1 float; work: >= 4104 bytes. */
int jat_k_recon_loss(const float* pred, const float* target, float* dpred, float* loss_out, int64_t n, double eps,
                     float loss_scale, void* work, size_t work_bytes, void* stream);
/* fp32 -> bf16 (round-to-nearest-even) */
int jat_k_cast_bf16(const float* in, uint16_t* out, int64_t n, void* stream);

/* ---- per-kernel entry points of the training step (the kernels jat_trainer_fwd_bwd / jat_trainer_optim launch) ----------
 * Dropout sites are (seed, site, p): the mask of element e is the counter hash of jat_rng.h, as the trainer draws it with
 * site = layer * 8 + kind.  p in [0, 1); p == 0 disables the site.  A shape the kernel does not take is JAT_E_INVALID;
 * `work` is device scratch of at least the stated size (JAT_E_INVALID when smaller). */
/* Training attention forward: o as jat_k_attention with dropout on the probabilities (element ((b*Hq + h)*N + i)*N + j),
 * lse [B, Hq, N] fp32 = log2-domain log-sum-exp of the un-dropped scaled scores.  1 <= N <= 2048. */
int jat_k_attention_train(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, float* lse, int32_t B,
                          int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, uint64_t seed, int32_t site, float p, void* stream);
/* Its backward: dqkv [B*N, (Hq + 2 Hkv)*64] = (dQ | dK | dV) with the inverse RoPE of rope_cos / rope_sin [2048, 32] (token
 * position = row within the sample) applied to dQ and dK.  split_heads = 1: the query heads of a KV group go to separate
 * blocks whose fp32 partials are reduced afterwards (the trainer's form); 0: one block per KV group.
 * work: align256(B*Hq*N*4) + (split_heads ? B*Hq*N*128*4 : 0) bytes. */
int jat_k_attention_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* vt, const uint16_t* o, const uint16_t* dout,
                        const float* lse, uint16_t* dqkv, const float* rope_cos, const float* rope_sin, int32_t B, int32_t N,
                        int32_t Hq, int32_t Hkv, int32_t Npad, uint64_t seed, int32_t site, float p, int32_t split_heads,
                        void* work, size_t work_bytes, void* stream);
/* Backward of y = norm(x) (* w) * (1 + scale[b]) + shift[b] on x [B*ntok, D] (D = 256..2048 in steps of 256): dx (+)= dL/dx;
 * dshift / dscale rows b at dmod_bstride; dw [D] summed over all rows.  w, scale, dshift, dscale, dw each nullable; mode 1
 * (LayerNorm, no affine) takes no w / dw.  work: (B*ceil(ntok/16)*3*D + B*D)*4 bytes. */
int jat_k_norm_bwd(const float* x, const uint16_t* dy, const float* w, const float* scale, int64_t mod_bstride, float* dx,
                   int32_t accumulate, float* dshift, float* dscale, int64_t dmod_bstride, float* dw, int32_t B, int32_t D,
                   int32_t ntok, int32_t mode, void* work, size_t work_bytes, void* stream);
/* Backward of x_out = x_in + gate[b] * pm[b] * (m o y): dy = dx * gate * pm * m (16-bit), dgate[b] = sum_tok dx * y * pm * m;
 * pm = DropPath draw of sample b (path site), m = element dropout of [B, ntok, D] (elem site).  work: B*ceil(ntok/16)*D*4 bytes. */
int jat_k_gate_bwd(const float* dx, const uint16_t* y, const float* gate, int64_t gate_bstride, uint16_t* dy, float* dgate,
                   int64_t dgate_bstride, int32_t B, int32_t D, int32_t ntok, uint64_t seed, int32_t path_site, float path_p,
                   int32_t elem_site, float elem_p, void* work, size_t work_bytes, void* stream);
/* The forward it differentiates: x_out [M, D] = x_in + gate[row / ntok] * pm * (m o y) (D % 8 == 0). */
int jat_k_resid_gate(const float* x_in, const uint16_t* y, const float* gate, int64_t gate_bstride, float* x_out, int32_t M,
                     int32_t D, int32_t ntok, uint64_t seed, int32_t path_site, float path_p, int32_t elem_site, float elem_p,
                     void* stream);
/* out = m o gelu_erf(in) and its backward in place: d = d * m * gelu'(pre); n % 8 == 0. */
int jat_k_gelu(const uint16_t* in, uint16_t* out, int64_t n, uint64_t seed, int32_t site, float p, void* stream);
int jat_k_gelu_bwd(const uint16_t* pre, uint16_t* d, int64_t n, uint64_t seed, int32_t site, float p, void* stream);
/* clip_grad_norm_(max_grad_norm) of g / loss_scale + one AdamW step on p, m, v (the kernels of jat_trainer_optim, same
 * semantics); grad_norm_out (device, nullable) = L2 norm of the SCALED g.  n % 4 == 0; work: 4104 bytes. */
int jat_k_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, float max_grad_norm, float loss_scale, int32_t step, float* grad_norm_out, void* work,
                size_t work_bytes, void* stream);
/* The same step with the moving average of jat_trainer_set_ema fused into the AdamW pass: p, m, v get the bits jat_k_adamw
 * gives, and ema += (1 - ema_decay) * (p_new - ema) (one subtraction, one fma).  ema not NULL and none of p, g, m, v;
 * 0 <= ema_decay < 1. */
int jat_k_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float max_grad_norm, float loss_scale, float ema_decay, int32_t step,
                    float* grad_norm_out, void* work, size_t work_bytes, void* stream);
/* Small-batch Linear backward (adaLN modulation, t_embedder): dW [N, K] = dy[B, N]^T x'[B, K] with x' = silu(x) if silu_x,
 * db [N] = column sums of dy (nullable); B <= 64, K % 4 == 0. */
int jat_k_small_dw(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* dW, float* db, int32_t B, int32_t N,
                   int32_t K, int32_t silu_x, void* stream);
/* dx [B, K] (+)= dy[B, N] W[N, K] (W 16-bit if w_is_bf16, else fp32), then times silu'(silu_pre) when silu_pre is given;
 * B <= 32, K % 4 == 0; work: ceil(N / slab)*B*K*4 bytes, slab = 256 for N >= 16384, else 32. */
int jat_k_small_dx(const float* dy, int64_t ldy, const void* W, int32_t w_is_bf16, float* dx, int32_t B, int32_t N, int32_t K,
                   int32_t accumulate, const float* silu_pre, void* work, size_t work_bytes, void* stream);

/* ---- measurement aid (bench.py roofline leg; no reference counterpart) ------------------------------------ */
/* (state lives in the model handle: two models in one process do not share a bracket)
 * Bracket every GEMM launch of one call site (0 qkv, 1 out_proj, 2 MLP fc1, 3 MLP fc2, 4 other; -1 = off) with a
 * HIP event pair on the launch stream, for at most max_launches launches.  Eager calls only. */
int jat_prof_gemm_site(jat_model* m, int32_t site, int32_t max_launches);
/* Sum of the bracketed launch durations [host ms], their count, algorithmic FLOPs and the tile variant used;
 * synchronises on the recorded events and switches the bracket off. */
int jat_prof_collect(jat_model* m, double* total_ms, int32_t* launches, double* flops, int32_t* variant);

/* ---- DAC 44.1 kHz decoder: latent [B, 1024, T] -> audio [B, 1, T*512] ------------------------------------ */
/* The reference decodes with the Descript Audio Codec (infer_test_v3m2.py:97-104, :408-437); the computation is
 * transformers' DacDecoder.forward (models/dac/modeling_dac.py:407-441).  bf16 MFMA in both operand-dtype builds. */
typedef struct jat_dac_decoder jat_dac_decoder;
#define JAT_DAC_BF16X3 0   /* operands split bf16 hi + lo, three MFMA passes, fp32 accumulation (matches fp32) */
#define JAT_DAC_BF16 1     /* one bf16 pass */
typedef struct jat_dac_config {
  int32_t latent_channels;   /* DacConfig.hidden_size: 1024 */
  int32_t channels;          /* DacConfig.decoder_hidden_size: 1536 (every channels >> i a multiple of 32) */
  int32_t n_blocks;          /* len(upsampling_ratios), 1..4 */
  int32_t strides[4];        /* upsampling_ratios: 8, 8, 4, 2 (even) */
} jat_dac_config;
/* named: the decoder's folded (plain `weight`) fp32 parameters under transformers' DacDecoder names (modeling_dac.py:
 * 416-433): conv1.{weight,bias}, block.{i}.snake1.alpha, block.{i}.conv_t1.{weight,bias},
 * block.{i}.res_unit{1,2,3}.{snake1.alpha,conv1.weight,conv1.bias,snake2.alpha,conv2.weight,conv2.bias}, snake1.alpha,
 * conv2.{weight,bias}.  Weights are re-laid out per tap / per phase and split into bf16 planes here; device memory for
 * batches up to max_B x max_T frames is allocated here.  A missing or mis-sized key fails with its name. */
int jat_dac_decoder_create(const jat_dac_config* cfg, const jat_tensor_ref* named, int32_t n, int32_t max_B,
                           int32_t max_T, void* stream, jat_dac_decoder** out);
void jat_dac_decoder_destroy(jat_dac_decoder* d);
/* device bytes the handle holds (weights + activations for max_B x max_T) */
int jat_dac_workspace_bytes(const jat_dac_decoder* d, size_t* bytes);
/* DacDecoder.forward (modeling_dac.py:427-441): z fp32 [B, latent_channels, T] -> audio fp32 [B, 1, T * prod(strides)];
 * 1 <= B <= max_B, 1 <= T <= max_T, precision JAT_DAC_*. */
int jat_dac_decode(jat_dac_decoder* d, const float* z, float* audio, int32_t B, int32_t T, int32_t precision, void* stream);
/* Per-kernel entry points (unit tests).  [host] fp32 torch-layout weight -> [N, taps, Cin] GEMM layout:
 * kind 0: Conv1d weight [cout, cin, k] (taps = k, N = cout); kind 1: ConvTranspose1d weight [cin, cout, 2 s] with
 * padding s / 2 (k_or_stride = s; polyphase, taps = 3, N = s * cout); kind 2: strided Conv1d weight [cout, cin, 2 s], stride s,
 * padding s / 2, over super-rows of s input rows (taps = 3, N = cout, GEMM cin = s * cin; out [cout, 3, s * cin]). */
int jat_dac_pack_weight(int32_t kind, const float* w, int32_t cin, int32_t cout, int32_t k_or_stride, float* out);
/* fp32 -> bf16 planes hi = bf16(x), lo = bf16(x - hi) */
int jat_k_dac_split(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, void* stream);
/* One decoder convolution on channels-last operand planes a [B*T, cin] and packed weight planes w [N, taps, cin]:
 *   taps 7, dil d:  Conv1d k7 padding 3d (modeling_dac.py:180,197) — with alpha: the snake epilogue;
 *   taps 3, dil 1:  ConvTranspose1d polyphase (modeling_dac.py:244-250), N = s * cch, out rows [B, T*s, cch];
 *   taps 1 + res:   residual-unit conv2 plus the fp32 residual (modeling_dac.py:198,208; out32 may equal res).
 * Epilogue: v = acc + bias[n % cch] (+ res); out32 = v if non-null; o_hi/o_lo = planes of snake_alpha(v) if o_hi. */
int jat_k_dac_conv(const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* w_hi, const uint16_t* w_lo,
                   const float* bias, const float* res, float* out32, const float* alpha, uint16_t* o_hi, uint16_t* o_lo,
                   int32_t B, int32_t T, int32_t cin, int32_t N, int32_t cch, int32_t taps, int32_t dil,
                   int32_t precision, void* stream);
/* Tail (modeling_dac.py:436-439): x fp32 [B*T, C] -> tanh(conv_k7(snake(x))) fp32 [B, 1, T]; w [7][C] (tap-major), C <= 96 */
int jat_k_dac_tail(const float* x, const float* alpha, const float* w, const float* bias, float* out, int32_t B, int32_t T,
                   int32_t C, void* stream);

/* ---- DAC 44.1 kHz encoder: audio [B, 1, T*512] -> latent z [B, 1024, T] + codes --------------------------------- */
/* The reference encodes its training pairs with the Descript Audio Codec (prepare_dataset_v5.py:206-219,
 * refine_dataset_lr_only.py:189-194: `z, _, _, _, _ = dac_model.encode(audio)`); the computation is transformers'
 * DacEncoder.forward + DacResidualVectorQuantizer.forward in eval mode (models/dac/modeling_dac.py:103-173, 283-345,
 * 444-475).  Convs in bf16 MFMA (JAT_DAC_* precision), the quantizer in fp32; the same bits in both operand-dtype builds. */
typedef struct jat_dac_encoder jat_dac_encoder;
#define JAT_DAC_MAX_CODEBOOKS 9
typedef struct jat_dac_encoder_config {
  int32_t channels;        /* DacConfig.encoder_hidden_size: 64 (a multiple of 32) */
  int32_t hidden_size;     /* DacConfig.hidden_size: 1024 (the only size the quantizer kernel takes) */
  int32_t n_blocks;        /* len(downsampling_ratios), 1..4; block i runs on channels << i */
  int32_t strides[4];      /* downsampling_ratios: 2, 4, 8, 8 (even) */
  int32_t n_codebooks;     /* 1..JAT_DAC_MAX_CODEBOOKS: 9 */
  int32_t codebook_size;   /* 1024 */
  int32_t codebook_dim;    /* 8 */
} jat_dac_encoder_config;
/* named: folded (plain `weight`) fp32 parameters under transformers' DacModel names: encoder.conv1.{weight,bias},
 * encoder.block.{i}.res_unit{1,2,3}.{snake1.alpha,conv1.weight,conv1.bias,snake2.alpha,conv2.weight,conv2.bias},
 * encoder.block.{i}.snake1.alpha, encoder.block.{i}.conv1.{weight,bias}, encoder.snake1.alpha, encoder.conv2.{weight,bias},
 * quantizer.quantizers.{i}.{in_proj.weight,in_proj.bias,out_proj.weight,out_proj.bias,codebook.weight}.  A missing or
 * mis-sized key fails with its name.  Device memory for batches up to max_B x max_T frames is allocated here. */
int jat_dac_encoder_create(const jat_dac_encoder_config* cfg, const jat_tensor_ref* named, int32_t n, int32_t max_B,
                           int32_t max_T, void* stream, jat_dac_encoder** out);
void jat_dac_encoder_destroy(jat_dac_encoder* e);
/* device bytes the handle holds (weights + activations for max_B x max_T) */
int jat_dac_encoder_workspace_bytes(const jat_dac_encoder* e, size_t* bytes);
/* audio fp32 [B, 1, T * prod(strides)] -> z fp32 [B, hidden, T] (sum of the first n_quantizers quantized codebooks),
 * codes int32 [B, n_quantizers, T] (or null), latents fp32 [B, 8 n_quantizers, T] (in_proj outputs, or null), hidden fp32
 * [B, hidden, T] (the encoder output before the quantizer, or null).  1 <= B <= max_B, 1 <= T <= max_T,
 * 1 <= n_quantizers <= n_codebooks, precision JAT_DAC_* (convs only; the quantizer is fp32). */
int jat_dac_encode(jat_dac_encoder* e, const float* audio, float* z, int32_t* codes, float* latents, float* hidden,
                   int32_t B, int32_t T, int32_t n_quantizers, int32_t precision, void* stream);
/* Encoder per-kernel entry points (unit tests); the strided convs run through jat_k_dac_conv (taps 3, dil 1, cin = s * Cin,
 * T = output frames) with jat_dac_pack_weight kind 2.
 * Head (modeling_dac.py:450): audio fp32 [B, L] -> conv1 = Conv1d(1, C, k7, pad 3) per sample; w [C, 1, 7]; out32 [B*L, C]
 * and / or o_hi (+ o_lo, may be null) planes of snake_alpha(out); C a multiple of 32. */
int jat_k_dac_head(const float* audio, const float* w, const float* bias, const float* alpha, float* out32, uint16_t* o_hi,
                   uint16_t* o_lo, int32_t B, int32_t L, int32_t C, void* stream);
/* Residual vector quantizer in fp32: hidden [B*T, 1024] channels-last; w_in [nq, 8, 1024], b_in [nq, 8], codebook
 * [nq, 1024, 8] (un-normalized), w_out [nq, 1024, 8], b_out [nq, 1024]; outputs as jat_dac_encode (hidden_cm: hidden
 * re-laid out as [B, 1024, T]).  hidden_size must be 1024. */
int jat_k_dac_rvq(const float* hidden, const float* w_in, const float* b_in, const float* codebook, const float* w_out,
                  const float* b_out, float* z, int32_t* codes, float* latents, float* hidden_cm, int32_t B, int32_t T,
                  int32_t hidden_size, int32_t n_quantizers, void* stream);

/* ---- sample-rate converter: audio [B, L] -> [B, ceil(n L / o)] ------------------------------------------------ */
/* The reference resamples its training audio with torchaudio (prepare_dataset_v5.py:198,203: AF.resample); the
 * computation is torchaudio.functional.resample with resampling_method "sinc_interp_hann" (functional.py,
 * _get_sinc_resample_kernel + _apply_sinc_resample_kernel).  With g = gcd(orig, new), o = orig / g, n = new / g,
 * base = min(o, n) * rolloff, width = ceil(lowpass_filter_width * o / base) and K = 2 width + o taps per phase:
 *   t       = clamp((-p / n + (k - width) / o) * base, -lpw, +lpw)                       p in [0, n), k in [0, K)
 *   h[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / lpw / 2)^2 * (base / o)     (fp64, stored as fp32)
 *   y[f n + p] = sum_k h[p][k] * x[f o + k - width]   (x = 0 outside [0, L)),   L_out = ceil(n L / o)
 * fp32 in both operand-dtype builds; every output is one ascending sum over k: the same bits from run to run and for
 * a row alone or in a batch.  orig == new is a copy. */
typedef struct jat_resampler jat_resampler;
/* [host, no GPU needed] the dimensions and, when table is non-null, the tap table h as [n][K] fp32 [host].  o, n, width
 * and K must be non-null.  Fails on orig or new_ < 1, lowpass_filter_width < 1, rolloff outside (0, 1], or a table of more
 * than 2^26 entries (nearly coprime rates). */
int jat_resample_table(int32_t orig, int32_t new_, int32_t lowpass_filter_width, double rolloff, float* table, int32_t* o,
                       int32_t* n, int32_t* width, int32_t* K);
/* Builds the table, uploads it on `stream` and waits for the upload; the same argument checks as the table call. */
int jat_resampler_create(int32_t orig, int32_t new_, int32_t lowpass_filter_width, double rolloff, void* stream,
                         jat_resampler** out);
void jat_resampler_destroy(jat_resampler* r);
/* [host] L_out = ceil(n L / o); fails when L_out or L + K does not fit in 31 bits. */
int jat_resample_out_length(const jat_resampler* r, int64_t L, int64_t* L_out);
/* x fp32 [B, L] -> y fp32 [B, L_out], both dense; 1 <= B <= 65535; L = 0 does nothing. */
int jat_resample(jat_resampler* r, const float* x, float* y, int32_t B, int64_t L, void* stream);
/* [host, no GPU needed] how jat_resample launches a conversion, from the functions it launches by (resample_geometry,
 * resample_launch_shape of csrc/resample.hip).  The block shape: K taps per phase; a thread owns ph phases (1 or 4); a block
 * holds pn phases, so gridDim.y = slices = ceil(n / pn); lanes = ceil(pn / ph) threads per frame group; at most groups_max
 * frame groups of 8 frames per block (the most whose window of (8 groups - 1) o + K samples fits 12288 floats of LDS).  The
 * launch for rows of L samples: groups frame groups per block, gridDim.x = grid_x blocks of 8 groups frames along a row,
 * block = lanes * groups threads, lds_bytes of dynamic LDS; all four are 0 for L = 0, and every field but K is 0 for
 * orig == new (a copy: no kernel).  Fails exactly where jat_resampler_create (the arguments, a table of more than 2^26
 * entries, no block shape whose window fits) or jat_resample_out_length (L) does.  Any output pointer may be null. */
int jat_k_resample_geometry(int32_t orig, int32_t new_, int32_t lowpass_filter_width, double rolloff, int64_t L, int32_t* K,
                            int32_t* ph, int32_t* pn, int32_t* slices, int32_t* lanes, int32_t* groups_max, int32_t* groups,
                            int32_t* grid_x, int32_t* block, int32_t* lds_bytes);

/* ---- per-channel latent statistics (prepare_dataset_v5.py:251-253, recalculate_stats.py:60-110) -------------------- */
/* sum[c] += sum_{b,t} v, sq_sum[c] += sum_{b,t} v^2 with v = z[b, c, t] rounded to fp16 (what the latent files store), in
 * fp64: z fp32 [B, C, T], sum and sq_sum fp64 [C] device buffers the caller owns and zeroes, so that many files fold into
 * one running total.  Two stages (JAT_STATS_SLICES partial sums per channel in `work`, then one thread per channel adds
 * them in order), no atomics: the same bits from run to run.  work: at least C * JAT_STATS_SLICES * 16 bytes. */
#define JAT_STATS_SLICES 16
int jat_channel_stats(const float* z, int32_t B, int32_t C, int32_t T, double* sum, double* sq_sum, void* work,
                      size_t work_bytes, void* stream);

/* ---- audio-quality metrics: log-spectral distance and mel-spectrogram losses -------------------------------------- */
/* What the reference's calculate_metrics.py computes with librosa >= 0.10, on mono fp32 audio [B, L] pairs (pred, gt):
 *   STFT   periodic Hann w[i] = 0.5 - 0.5 cos(2 pi i / n_fft), win_length = n_fft, center=True with n_fft / 2 zeros a side,
 *          frames = 1 + L / hop, bins = 1 + n_fft / 2,  X[k, f] = sum_i w[i] x_pad[f hop + i] e^{-2 pi i k i / n_fft}
 *   LSD    d = log10 max(|X_pred|, 1e-8) - log10 max(|X_gt|, 1e-8),  lsd_frames[f] = sqrt(mean_k d[k, f]^2),
 *          lsd_db = 20 mean_f lsd_frames[f]                                                  (calculate_metrics.py:23-62)
 *   mel    S = M |X|^2, M = librosa.filters.mel (Slaney scale, fmin 0, fmax sr / 2, norm "slaney"),
 *          dB = max(10 log10 max(1e-10, S) - 10 log10 max(1e-10, max S), -80), the maximum over one signal's whole
 *          spectrogram;  mel_l1 = mean |a - b|,  mel_l2 = sqrt(mean (a - b)^2)                              (:64-101)
 * One pass transforms pred + i gt per frame in LDS and reduces in place (no spectrogram reaches memory), a second sums in
 * fp64.  fp32 in both operand-dtype builds, no atomics: the same bits from run to run and for a row alone or in a batch. */
typedef struct jat_audio_metrics jat_audio_metrics;
/* [host, no GPU needed] the filterbank as [n_mels][1 + n_fft / 2] fp32 (computed in fp64), when out is non-null.  Fails on
 * sr < 1, n_fft not a power of two in 64..4096, n_mels < 0 or above the bin count. */
int jat_mel_filterbank(int32_t sr, int32_t n_fft, int32_t n_mels, float* out);
/* [host] frames = 1 + L / hop; fails on L < 1 or hop < 1 */
int jat_stft_frames(int64_t L, int32_t hop, int64_t* frames);
/* Builds window, twiddles and the sparse filterbank, uploads them on `stream` and waits.  n_mels = 0: no mel bands (STFT
 * and LSD only).  The same argument checks as jat_mel_filterbank, and hop >= 1. */
int jat_audio_metrics_create(int32_t sr, int32_t n_fft, int32_t hop, int32_t n_mels, void* stream, jat_audio_metrics** out);
void jat_audio_metrics_destroy(jat_audio_metrics* h);
/* Device bytes jat_audio_metrics_run needs for B rows of L samples.  Fails on L < 1, B outside 1..65535, or frames * bins
 * or L + n_fft beyond 31 bits. */
int jat_audio_metrics_workspace_bytes(const jat_audio_metrics* h, int32_t B, int64_t L, size_t* bytes);
/* pred, gt fp32 [B, L] (device) -> out fp64 [B, 3] (device): lsd_db (0 unless want_lsd), mel_l1, mel_l2 (0 when the handle
 * has no mel bands).  Optional device outputs: lsd_frames fp32 [B, frames] (needs want_lsd); pred_db and gt_db fp32
 * [B, n_mels, frames] (both or neither).  JAT_E_STATE when work_bytes is below jat_audio_metrics_workspace_bytes. */
int jat_audio_metrics_run(jat_audio_metrics* h, const float* pred, const float* gt, int32_t B, int64_t L, int32_t want_lsd,
                          double* out, float* lsd_frames, float* pred_db, float* gt_db, void* work, size_t work_bytes,
                          void* stream);
/* The transform alone, through the same kernel: x fp32 [B, L] -> X complex64 [B, bins, frames].  With y (and Y) a second
 * signal rides in the imaginary part of the same transforms; y and Y are null together. */
int jat_stft(jat_audio_metrics* h, const float* x, const float* y, int32_t B, int64_t L, void* X, void* Y, void* stream);

/* ---- inverse STFT, long-term spectrum and low-band splice --------------------------------------------------------- */
/* The counterpart of jat_stft and the closing stage of the audio path, on the window and twiddles of a jat_audio_metrics
 * handle (conventions as above: periodic Hann w, center=True, frames = 1 + L / hop, bins = 1 + n_fft / 2).
 *   inverse  y_pad[f hop + i] += w[i] irfft(X[:, f])[i],  env[f hop + i] += w[i]^2,
 *            y[t] = y_pad[t + n_fft / 2] / env[t + n_fft / 2] for t in [0, L)
 *            (what torch.istft(X, n_fft, hop, window=w, center=True, length=L) computes; the imaginary parts of the DC and
 *            Nyquist bins are ignored).  hop must divide n_fft with 4 <= n_fft / hop <= 64: env > 0 on all of [0, L).
 *   splice   g = generated, s = source, both cut to n = min(L_gen, L_src); a[k] in [0, 1] a real gain per bin (1 = source):
 *            out[t] = g[t] + iSTFT(a STFT(s - g))[t] = iSTFT(a S + (1 - a) G)[t] for t < n,  out[t] = g[t] for t in [n, L_gen)
 *   gain     f_k = k sr / n_fft, lo = cutoff_hz - transition_hz:  a[k] = 0 for f_k >= cutoff_hz, 1 for f_k <= lo,
 *            0.5 + 0.5 cos(pi (f_k - lo) / transition_hz) between: the transition lies below the cutoff
 *   ltas     P[k] = mean_f |X[k, f]|^2 in fp64
 * Two real frames (2 p, 2 p + 1) share one complex transform; the windowed output frames go to the workspace
 * [B, frames, n_fft] fp32 and a gather pass sums the covering frames of every sample in ascending frame order and divides
 * by a host-made envelope table.  fp32 in both operand-dtype builds, no atomics: the same bits from run to run, for a row
 * alone or in a batch, whatever the launch shape.  A gain of zeros returns `generated` bit for bit. */
/* [host, no GPU needed] bytes of the frames workspace of jat_istft for B rows of L samples.  Fails on n_fft not a power of
 * two in 64..4096, hop not dividing n_fft, hop > n_fft / 4, n_fft / hop > 64, B outside 1..65535, L < 1, or sizes beyond
 * 31 bits. */
int jat_istft_workspace_bytes(int32_t n_fft, int32_t hop, int32_t B, int64_t L, size_t* bytes);
/* X complex64 [B, bins, 1 + L / hop] (device) -> y fp32 [B, L].  The handle's hop must pass the checks above.
 * JAT_E_STATE when work_bytes is below jat_istft_workspace_bytes. */
int jat_istft(jat_audio_metrics* h, const void* X, int32_t B, int64_t L, float* y, void* work, size_t work_bytes, void* stream);
/* x fp32 [B, L] -> P fp64 [B, bins] (device).  Partial spectra over JAT_LTAS_SLICES fixed slices of the frames are added in
 * frame order, then slice by slice; no spectrogram reaches memory.  work: at least B * JAT_LTAS_SLICES * bins * 8 bytes. */
#define JAT_LTAS_SLICES 64
int jat_ltas(jat_audio_metrics* h, const float* x, int32_t B, int64_t L, double* P, void* work, size_t work_bytes, void* stream);
/* [host, no GPU needed] the gain table a[bins] fp32 (computed in fp64).  cutoff_hz <= 0 gives zeros; cutoff_hz -
 * transition_hz >= sr / 2 gives ones.  Fails on sr < 1, a bad n_fft, a negative transition or non-finite arguments. */
int jat_band_gain(int32_t sr, int32_t n_fft, double cutoff_hz, double transition_hz, float* a);
/* [host, no GPU needed] bytes of the frames workspace of jat_band_splice; the checks of jat_istft_workspace_bytes on both
 * lengths (each at least 1). */
int jat_band_splice_workspace_bytes(int32_t n_fft, int32_t hop, int32_t B, int64_t L_gen, int64_t L_src, size_t* bytes);
/* generated fp32 [B, L_gen], source fp32 [B, L_src], a fp32 [bins] (all device) -> out fp32 [B, L_gen]; out may be
 * `generated` itself.  JAT_E_STATE when work_bytes is below jat_band_splice_workspace_bytes. */
int jat_band_splice(jat_audio_metrics* h, const float* generated, const float* source, int32_t B, int64_t L_gen, int64_t L_src,
                    const float* a, float* out, void* work, size_t work_bytes, void* stream);

/* ---- training data: batch assembly from a device-resident fp16 latent store, per-step monitor sums ---------------- */
/* Replaces LatentDataset / ValidationDataset.__getitem__ + collate + the host-to-device copy + the two normalisations
 * (train_ddp_v3mod2.py:509-535, 561-597, 849-857) by one launch.  For sample b of B the device tables give the address of
 * its HR and LR source (fp16, row-major [C, len[b]], as the latent files store them; 2-byte aligned), its length len[b] >= 1
 * and its crop start start[b] >= 0.  For every b, c, j < T:
 *   out[b, c, j] = (float(src_b[c, (start[b] + j) mod len[b]]) - mean[c]) / std[c]
 * in fp32, the expression of jat_channel_affine, so the result has the bits of jat_channel_affine(crop.float()); with the
 * four statistics vectors null (all or none) it is the plain conversion.  A crop that does not wrap is fetched as whole
 * aligned 16-byte lines: the kernel reads the 16-byte-aligned lines that enclose each crop row, up to 14 bytes before the
 * first and after the last element of the [C, len] array, so those lines must be readable (true of any array inside a
 * device allocation that starts and ends on 16-byte boundaries, as hipMalloc's and PyTorch's do; not of an array placed by
 * a 2-byte sub-allocator at the very edge of a mapping).  The bytes outside the crop are never used.  The mod is the loop-repeat of clips shorter
 * than T (:520-524); with start[b] + T <= len[b] nothing wraps and the row is fetched with 16-byte loads.  hr_out, lr_out:
 * fp32 [B, C, T], 16-byte aligned, written with plain 16-byte (T % 4 == 0) or 8-byte vector stores.  T <= 8176.  No
 * atomics: the output depends on the inputs alone.  A table entry with len < 1 or a null address leaves its rows as they were. */
int jat_latent_gather(const void* const* hr_src, const void* const* lr_src, const int64_t* len, const int64_t* start,
                      const float* hr_mean, const float* hr_std, const float* lr_mean, const float* lr_std, float* hr_out,
                      float* lr_out, int32_t B, int32_t C, int32_t T, void* stream);
/* The sums behind the per-step figures the reference logs (train_ddp_v3mod2.py:902-919: PredictionMean, PredictionStd,
 * SNR_dB, CondNoiseStd) in one pass over pred, target (= hr_norm) and the optional cond_clean (= lr_norm before the condition
 * noise), each fp32 [n], 16-byte aligned:  out[6] fp64 (device) = sum p, sum p^2, sum h^2, sum (p - h)^2, sum l, sum l^2
 * (the last two 0 without cond_clean).  Terms are formed and added in fp64; two stages in a fixed order (a constant number
 * of partial sums in `work`, then one block), no atomics: the same bits from run to run.  work: JAT_MONITOR_WORK_BYTES. */
#define JAT_MONITOR_WORK_BYTES 49152
int jat_train_monitor(const float* pred, const float* target, const float* cond_clean, int64_t n, double* out, void* work,
                      size_t work_bytes, void* stream);

/* ---- latent retrieval: exact nearest-neighbour bank and index-rate blend ------------------------------ */
/* A bank holds up to `capacity` latent frames as fp16 rows [size, channels] with one fp32 squared norm per key row, computed
 * from the stored fp16 values.  The stored rows ARE the bank: search and blend are defined on them.  A paired bank keeps
 * separate key rows (what is searched) and value rows (what is blended in) at the same indices; otherwise they are one buffer.
 * channels: a multiple of 32 in 32..1024.  All device memory is allocated at creation; every later call only enqueues on the
 * caller's stream, never synchronises and may be captured into a graph.  The host-side size advances when a call is enqueued. */
typedef struct jat_bank jat_bank;
#define JAT_BANK_SLAB 4096   /* key rows per search workgroup: results do not depend on it, tests size banks across it */
#define JAT_BANK_KEYS 0
#define JAT_BANK_VALUES 1
int jat_bank_create(int32_t channels, int32_t capacity, int32_t paired, jat_bank** out);
void jat_bank_destroy(jat_bank* bank);
int jat_bank_size(const jat_bank* bank, int32_t* size);
int jat_bank_clear(jat_bank* bank);
/* Appends `count` frames first, first + stride, ... of a [channels, len] latent array (fp16 or fp32, as the files store it):
 *   row[size + i, c] = fp16((float(src[c, first + i stride]) - mean[c]) / std[c])      (the fp32 expression of the channel
 * affine above, rounded to nearest even).  A paired bank takes value_src (same layout and len) with the value statistics; any
 * other bank takes value_src NULL.  JAT_E_STATE, with the bank as it was, when size + count > capacity; JAT_E_INVALID when a
 * frame lies outside the source. */
int jat_bank_add(jat_bank* bank, const void* key_src, const void* value_src, int32_t src_is_fp16, int64_t len, int64_t first,
                 int64_t stride, int32_t count, const float* key_mean, const float* key_std, const float* value_mean,
                 const float* value_std, void* stream);
/* Device pointers of the key or value rows (fp16 [capacity, channels]) and the key norms (fp32; NULL for the values of a
 * paired bank), for saving a bank.  `norms` may be NULL. */
int jat_bank_rows(const jat_bank* bank, int32_t which, const void** rows, const float** norms);
/* Appends `count` ready fp16 rows (device; values exactly when the bank is paired) and recomputes their norms on the device. */
int jat_bank_load_rows(jat_bank* bank, const void* keys, const void* values, int32_t count, void* stream);
int jat_bank_search_workspace_bytes(const jat_bank* bank, int64_t n_queries, size_t* bytes);
/* x fp32 [B, channels, T]: query (b, t) is the column x[b, :, t], normalised as (x - mean[c]) / std[c] when mean and std are
 * given (both NULL: x is used as it is).  With d(q, i) = |q|^2 + |k_i|^2 - 2 q.k_i over key rows i < size:
 *   idx[b, t] = argmin_i d, the lowest index on equal d, always in [0, size);  dist2[b, t] = max(d, 0)  (dist2 may be NULL).
 * The product is exact in the fp16 keys and carries the query as two fp16 terms (error 2^-22 |q|), accumulated in fp32 in a
 * fixed channel order: a query's result does not depend on B, on its neighbours or on how the key range is split, and two
 * runs give the same bits.  A query component beyond the fp16 range (65504) makes that query's distances meaningless.
 * work: 8-byte aligned, at least the bytes the query function above returns for B T queries; JAT_E_INVALID when smaller. */
int jat_bank_search(jat_bank* bank, const float* x, const float* mean, const float* std, int32_t B, int32_t T, int32_t* idx,
                    float* dist2, void* work, size_t work_bytes, void* stream);
/* y[b, c, t] = (1 - rate) x[b, c, t] + rate v,  v = float(values[idx[b, t], c]), or that times value_std[c] plus
 * value_mean[c] when both are given; each product and sum rounded once, nothing fused, so rate 0 returns x and rate 1 returns
 * v.  y may be x.  rate in [0, 1]. */
int jat_bank_blend(jat_bank* bank, const float* x, const int32_t* idx, const float* value_mean, const float* value_std,
                   float rate, float* y, int32_t B, int32_t T, void* stream);

/* ---- top-k latent retrieval: the k nearest rows, inverse-square blend ------------------------------- */
#define JAT_BANK_MAX_K 8
/* Device bytes jat_bank_search_topk needs for n_queries queries and k in 1..JAT_BANK_MAX_K (k = 1: what
 * jat_bank_search_workspace_bytes returns). */
int jat_bank_topk_workspace_bytes(const jat_bank* bank, int64_t n_queries, int32_t k, size_t* bytes);
/* The search above for the k nearest key rows.  With the rows i < size ordered by (d(q, i), i), d exactly as in
 * jat_bank_search, query n = b T + t gets the first k of them in that order:
 *   idx[n, j] the row, dist2[n, j] = max(d, 0) (dist2 may be NULL);  size < k: the places j >= size hold idx -1, dist2 +inf.
 * The first j columns of a result for k are the result for j, bit for bit; k = 1 is jat_bank_search.  The same
 * independence of B, of the query's neighbours, of the split of the key range and of the run.  work: 8-byte aligned, at
 * least the bytes the query function above returns for B T queries and this k. */
int jat_bank_search_topk(jat_bank* bank, const float* x, const float* mean, const float* std, int32_t B, int32_t T, int32_t k,
                         int32_t* idx, float* dist2, void* work, size_t work_bytes, void* stream);
/* idx int32 / dist2 fp32 [B T, k] as jat_bank_search_topk writes them (any caller-made lists of that form do).  Per frame,
 * in fp32:  dt_j = max(dist2_j, dist2_floor),  u_j = (dt_0 / dt_j)^2 where idx_j >= 0 and 0 elsewhere,  w_j = u_j / sum_j u_j
 * (sum over ascending j),  v = sum_j w_j float(values[idx_j, c]) (an fmaf chain over ascending j), then v de-normalised and
 * mixed exactly as in jat_bank_blend:  y = (1 - rate) x + rate (v value_std + value_mean).  Where every dist2_j exceeds the
 * floor, w is square(1 / dist2) normalised to sum 1.  An index >= size is clamped into the bank, a negative one carries
 * weight 0 and is not read; a frame without any usable entry gets v = 0.  k = 1 computes jat_bank_blend bit for bit.
 * dist2_floor > 0 and finite (1e-6 suits squared distances of normalised latents); rate in [0, 1]; y may be x. */
int jat_bank_blend_topk(jat_bank* bank, const float* x, const int32_t* idx, const float* dist2, int32_t k,
                        const float* value_mean, const float* value_std, float rate, float dist2_floor, float* y, int32_t B,
                        int32_t T, void* stream);

/* ---- pitch tracking (YIN) and F0-preservation counts ------------------------------------------------ */
/* Steps 1-5 of de Cheveigne & Kawahara (2002) on mono fp32 audio x[B, L], framed as the STFT above frames it:
 * W = frame_length / 2, frames = 1 + L / hop_length, frame f = x_pad[f hop : f hop + frame_length] with frame_length / 2
 * zeros a side; min_period = floor(sr / fmax), max_period = min(ceil(sr / fmin), frame_length - W - 1).  Per frame:
 *   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2, tau = 1 .. max_period, summed in this direct form
 *   c(tau) = d(tau) / ((1 / tau) sum_{u = 1 .. tau} d(u) + FLT_MIN);   y[i] = c(min_period + i), i = 0 .. max_period - min_period
 *   trough: y[i] < y[i - 1] && y[i] <= y[i + 1] inside, y[0] < y[1] at i = 0, never at the last index
 *   voiced = some trough has y < trough_threshold;  k = the first such trough, else the lowest-index minimum of y
 *   shift = -b / a with a = y[k + 1] + y[k - 1] - 2 y[k], b = (y[k + 1] - y[k - 1]) / 2 when |b| < |a|, else 0; 0 at either end
 *   f0 = sr / (min_period + k + shift) (reported for every frame),  aperiodicity = y[k]
 * A frame of zeros is unvoiced.  fp32 in both operand-dtype builds, every sum in one fixed order, no atomics: the same
 * bits from run to run, for a row alone or in a batch, whatever the launch shape.  Samples outside [0, L) of a row are
 * never read. */
typedef struct {
  double fmin, fmax;
  int32_t sr, frame_length, hop_length;
  float trough_threshold;
} jat_yin_params;
/* [host, no GPU needed] the period range above.  Fails on sr < 1, a frame_length that is odd or outside 16..8192, fmin <= 0,
 * fmax <= fmin, fmax >= sr / 2, or max_period - min_period < 2. */
int jat_yin_periods(int32_t sr, double fmin, double fmax, int32_t frame_length, int32_t* min_period, int32_t* max_period);
/* x fp32 [B, L] (device) -> f0, aperiodicity fp32 [B, frames], voiced uint8 [B, frames].  Optional outputs for unit tests
 * (NULL: not written): index int32 [B, frames] = k; d and cmndf fp32 [B, frames, max_period + 1] with d[0] = 0, cmndf[0] = 1.
 * Fails (never faults) on what the period range refuses, hop_length < 1, a threshold that is not finite, L < 1, B outside
 * 1..65535, or a frame count or frames * (max_period + 1) beyond 31 bits. */
int jat_yin(const jat_yin_params* params, const float* x, int32_t B, int64_t L, float* f0, float* aperiodicity, uint8_t* voiced,
            int32_t* index, float* d, float* cmndf, void* stream);
/* Two tracks (f0 fp32, voiced uint8) [B, frames] -> out fp64 [B, 6] (device), b being the reference track:
 *   n_ref_voiced (voiced_b), n_both_voiced, n_voicing_errors (the flags differ), n_gross (both voiced, |cents| > gross_cents),
 *   sum |cents| over the both-voiced frames, sum |cents| over the both-voiced frames that are not gross,
 * cents = 1200 log2(f0_a / f0_b) in fp64.  One block per row adds in a fixed order; no atomics.  A frame voiced in both
 * tracks must carry positive f0 in both. */
int jat_f0_compare(const float* f0_a, const uint8_t* voiced_a, const float* f0_b, const uint8_t* voiced_b, int32_t B,
                   int32_t frames, double gross_cents, double* out, void* stream);

/* ---- pYIN: threshold prior and Viterbi decoding on YIN's normalised difference ----------------------- */
/* Mauch & Dixon (2014), arranged as librosa.pyin arranges it; the fp64 statement is tests/pyin_ref.py, and equality with
 * librosa is not claimed.  Departures from librosa are marked (D).  c is the cmndf above, y[i] = c[min_period + i].
 *  1 candidates: every trough of y by the rule above, each with its parabolic shift(y, i) (taken in fp64 on the fp32 y).
 *  2 threshold prior: theta_m = fp32(m / N), m = 1 .. N = n_thresholds; beta_m = the Beta(beta_a, beta_b) mass on
 *    ((m - 1) / N, m / N].  Trough i of height h_i is under threshold m when h_i < theta_m; n(m) = troughs under m,
 *    p_i(m) = those of them with a smaller lag;
 *      P_i = sum_{m: h_i < theta_m} beta_m (1 - e^-lambda) e^(-lambda p_i(m)) / (1 - e^(-lambda n(m))),  lambda = boltzmann_parameter,
 *    and the lowest-index trough of minimum height also receives no_trough_prob * sum_{m: h_i >= theta_m} beta_m.  A frame
 *    without troughs contributes nothing.  The factors come from fp32 tables made in fp64 (values under FLT_MIN are 0);
 *    the sum over m runs in one fixed order.
 *  3 pitch bins: bps = ceil(1 / resolution), n_bins = floor(12 bps log2(fmax / fmin)) + 1; a trough's bin is
 *    clip(rint(12 bps log2(f0_i / fmin)), 0, n_bins - 1) with f0_i = sr / (min_period + i + shift), in fp64.  (D) librosa
 *    clips to n_bins, which lands in the unvoiced half and is overwritten.  Where troughs of a frame share a bin the largest
 *    lag wins.  obs[f, b] is that P;  voiced_prob[f] = clip(sum_b obs[f, b], 0, 1);  every unvoiced state observes
 *    (1 - voiced_prob) / n_bins.
 *  4 transition: H = round_half_even(max_transition_rate * 12 * hop_length / sr) * bps;  w(d) = 1 - |d| / (H + 1), |d| <= H;
 *    from bin r to bin s: w(s - r) / Z_r with Z_r summed over the s inside [0, n_bins); times 1 - switch_prob inside a half
 *    (voiced / unvoiced), switch_prob across.  (D) a move outside the band is impossible, not log(tiny).  Every one of the
 *    2 n_bins states is equally likely at the start.
 *  5 Viterbi in fp32 on the tables logw[2 H + 1], logZ[n_bins], lk = log(1 - switch_prob), ls = log(switch_prob),
 *    logpi = log(1 / (2 n_bins)), made in fp64 and rounded once:  lo_f[s] = log(obs + FLT_MIN), one value per frame for
 *    the unvoiced half;  V_0 = lo_0 + logpi;  per frame and half h: U_h[r] = V[r] - logZ[r],
 *    M_h[s] = max_r (U_h[r] + logw[s - r]) with the lowest r on a tie;  V'[s] = lo_f[s] + max(M_same[s] + lk, M_other[s] + ls),
 *    the voiced source on a tie;  V' -= max_s V'.  Every step is one rounded fp32 add, subtract or max; nothing is
 *    contracted or reassociated, so a numpy fp32 replica follows it bit for bit.  The last state is the lowest-index
 *    maximum (voiced half first), followed back through the back-pointers.
 *  6 per frame: voiced = state < n_bins;  f0 = freqs[state] where voiced with the host table fp32(fmin 2^(b / (12 bps))),
 *    (D) 0 where unvoiced (librosa: NaN);  voiced_prob.  f0 is quantised to bins of 100 resolution cents.
 * The same bits from run to run, for a row alone or in a batch, and from both operand-dtype builds. */
typedef struct {
  double fmin, fmax;
  int32_t sr, frame_length, hop_length, n_thresholds;
  double beta_a, beta_b, boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob;
} jat_pyin_params;
typedef struct jat_pyin jat_pyin;
/* [host, no GPU needed] out[m - 1] = beta_m, m = 1 .. n: the regularised incomplete beta function by its continued fraction,
 * fp64.  Fails on a or b that is not positive and finite, n outside 1..65536. */
int jat_pyin_beta_probs(double a, double b, int32_t n, double* out);
/* [host, no GPU needed]  A handle serves ONE device and one thread at a time: the first track or decode allocates the
 * tables on the device that is current then and copies them with a synchronous hipMalloc + hipMemcpy (so that first call
 * must not lie inside a stream capture), and every later call on another current device fails with JAT_E_STATE before
 * anything is launched.  The profile switch and its events are state of the handle too.  Fails with JAT_E_INVALID on everything the
 * period range and the YIN entry point refuse, n_thresholds outside 1..256, beta_a, beta_b, boltzmann_parameter or
 * max_transition_rate that is not positive and finite, switch_prob or no_trough_prob outside (0, 1), resolution outside
 * (0, 1], and beyond the sizes the kernels are built for: n_bins <= 1024, H <= 128, max_period - min_period + 1 <= 4096
 * candidates (every frame_length up to 8192 stays inside). */
int jat_pyin_create(const jat_pyin_params* params, jat_pyin** out);
void jat_pyin_destroy(jat_pyin* h);
/* each output may be NULL */
int jat_pyin_shape(const jat_pyin* h, int32_t* n_bins, int32_t* H, int32_t* min_period, int32_t* max_period);
/* [host] copies of the tables, each may be NULL: beta fp64 [n_thresholds]; logw fp32 [2 H + 1] (index d + H); logZ and freqs
 * fp32 [n_bins]; scalars fp32 [3] = lk, ls, logpi */
int jat_pyin_tables(const jat_pyin* h, double* beta, float* logw, float* logZ, float* freqs, float* scalars);
/* Fails as the track does on B, L and sizes beyond 31 bits. */
int jat_pyin_workspace_bytes(const jat_pyin* h, int32_t B, int64_t L, size_t* bytes);
/* x fp32 [B, L] (device) -> f0 fp32, voiced uint8, voiced_prob fp32, each [B, frames], frames = 1 + L / hop_length.
 * Optional outputs for unit tests (NULL: not written): cmndf fp32 [B, frames, max_period + 1]; prob fp32 [B, frames, ny]
 * (0 where there is no trough) and bin int32 [B, frames, ny] (-1 where there is none), ny = max_period - min_period + 1;
 * obs fp32 [B, frames, n_bins]; log_obs fp32 [B, frames, n_bins + 1] (the last entry is the unvoiced value); state int32
 * [B, frames] in 0 .. 2 n_bins - 1, the voiced half first.  work: 16-byte aligned device memory of at least the bytes the
 * query above returns (the difference function, the log observations, 16-bit back-pointers).
 * Fails, writing nothing, with JAT_E_INVALID on B outside 1..65535, L < 1, a frame count or frames times the values per
 * frame beyond 31 bits, a NULL x, f0, voiced, voiced_prob or work; with JAT_E_STATE on a workspace that is too small. */
int jat_pyin_track(jat_pyin* h, const float* x, int32_t B, int64_t L, float* f0, uint8_t* voiced, float* voiced_prob, float* cmndf,
                   float* prob, int32_t* bin, float* obs, float* log_obs, int32_t* state, void* work, size_t work_bytes,
                   void* stream);
/* Stages 5 and 6 alone, on log observations the caller supplies (the decoder's unit tests drive it with constructed ties):
 * log_obs fp32 [B, frames, n_bins + 1] (device) -> state int32, f0 fp32, voiced uint8, each [B, frames].  work: 16-byte
 * aligned, at least B * frames * n_bins * 4 bytes (the back-pointers).  Fails as the track does. */
int jat_pyin_decode(jat_pyin* h, const float* log_obs, int32_t B, int32_t frames, int32_t* state, float* f0, uint8_t* voiced,
                    void* work, size_t work_bytes, void* stream);
/* measurement aid (tools/pyin_bench.py): with on != 0 every track records device events around its four launches */
int jat_pyin_set_profile(jat_pyin* h, int32_t on);
/* waits for the latest profiled track; us[4] = difference function, observation, Viterbi forward, back-trace, in microseconds */
int jat_pyin_profile(jat_pyin* h, float* us);

#ifdef __cplusplus
}
#endif
#endif /* JAT_HIP_H */
