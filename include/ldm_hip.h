/* ldm_hip.h — C-ABI of the MI355X-native LayoutDM sampling hot path (libldm_hip.so).
 *
 * The reference (CyberAgentAILab/layout-dm) is 100 % Python/PyTorch and has no FFI layer;
 * its narrowest seam that contains exactly the hot path is the Python method
 *   ConstrainedMaskAndReplaceDiffusion.sample(batch_size, cond, sampling_cfg, ...)
 *     src/trainer/trainer/models/categorical_diffusion/base.py:293-371
 * reached from LayoutDM.sample (models/layoutdm.py:77-88) and test.py:195-200.
 * These entry points are what a ctypes binding placed at that seam calls (the binding is
 * shown in INTEGRATION.md and implemented in layout_dm_amd/binding.py).
 *
 * Conventions: every pointer named d_* is a DEVICE pointer owned by the caller (e.g. a torch
 * tensor's data_ptr()); h_* are host pointers.  `stream` is a hipStream_t passed as void*.
 * Return value 0 = OK, negative = error (text via ldm_last_error).  A handle is bound to one
 * device and is not thread-safe.  No entry point synchronises the device except
 * ldm_create / ldm_finalize_weights / ldm_destroy and the *_sync helpers.
 */
#ifndef LDM_HIP_H
#define LDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDM_ABI_VERSION 5

typedef struct ldm_handle ldm_handle;

/* numerics mode of the denoiser GEMMs / attention */
enum {
  LDM_PREC_EXACT_F32 = 0, /* v_mfma_f32_32x32x2_f32: exact fp32 (== fmaf chain) */
  LDM_PREC_FAST_F16 = 1,  /* fp16 operands, fp32 accumulate (v_mfma_f32_32x32x16_f16) */
  LDM_PREC_SPLIT_F16 = 2, /* fp16 hi+lo split operands, 3 MFMA passes, ~fp32 accuracy */
  LDM_PREC_MIXED_F16 = 3, /* the split mode with fp16-ONLY weights: activations (and the attention's q, k, v, P) stay hi+lo, the four
                             weight GEMMs and the head drop the W_lo product — 2 MFMA passes there, 3 inside the attention.  Logits
                             error 1e-4 .. 6e-4 of max |logit| on checkpoints whose fp16 error is ~1e-3;
                             reference backbone geometry only (ldm_create fails otherwise) */
  LDM_PREC_HYBRID_F16 = 4 /* mixed with the FFN and the vocabulary head in PLAIN fp16 (LayerNorm output, hidden activations and weights
                             rounded once: one MFMA pass there); the attention path — AdaLN output into in_proj, q, k, v, P, the attention
                             output into out_proj — keeps hi+lo activations.  Logits error 2.3e-4 on a trained checkpoint whose fp16 error
                             is 1.2e-3 (the fp16 error lives on the attention-score path: DESIGN.md section 3.5); same geometry rule */
};

/* transition-matrix family == Q_TYPES of the reference (models/layoutdm.py:20-23) */
enum {
  LDM_Q_CONSTRAINED = 0, /* ConstrainedMaskAndReplaceDiffusion: one sub-vocabulary per attribute
                            (categorical_diffusion/constrained.py) — the LayoutDM default */
  LDM_Q_VANILLA = 1      /* VanillaMaskAndReplaceDiffusion: one vocabulary of all C classes, MASK last,
                            un-prefixed schedule buffers (categorical_diffusion/vanilla.py) */
};

/* what a block's first normalisation (norm1) takes its statistics over == the timestep_type of the reference's Block
 * (models/transformer_utils.py:124-156).  A state dict does not tell the two apart, so the kind is a create-time argument
 * (ldm_create_variant).  Everything else of a denoiser variant — pos_emb, the *_abs sinusoid, timestep_type None — is
 * read from the checkpoint's key set by ldm_finalize_weights. */
enum {
  LDM_NORM1_LAYER = 0,   /* AdaLayerNorm / nn.LayerNorm: per row over d_model (adalayernorm, adalayernorm_abs, None) */
  LDM_NORM1_INSTANCE = 1 /* AdaInsNorm = InstanceNorm1d(d_model) over the sequence axis: per (layout, channel) over the
                            layout's S rows, biased variance, eps 1e-5, no affine (adainnorm, adainnorm_abs).
                            LDM_PREC_EXACT_F32 / LDM_PREC_SPLIT_F16 only, on the tiled kernels */
};

/* sampler kinds: trainer/helpers/sampling.py:13-59,81-130 */
enum {
  LDM_SAMPLE_DETERMINISTIC = 0,
  LDM_SAMPLE_RANDOM = 1,
  LDM_SAMPLE_TOP_P = 2,
  LDM_SAMPLE_TOP_K = 3,
  LDM_SAMPLE_GUMBEL = 4
};

/* Model geometry.  Mirrors what the reference derives from its hydra config:
 * vocabulary (helpers/layout_tokenizer.py:79-82,152-153), backbone
 * (config/backbone/medium.yaml shrunk 29/32 at models/layoutdm.py:54), T (layoutdm.py:33). */
typedef struct {
  int32_t abi_version; /* LDM_ABI_VERSION */
  int32_t n_category;  /* 25 (Rico25) / 5 (PubLayNet) */
  int32_t n_bin;       /* bins per coordinate (32) */
  int32_t max_elem;    /* 25 */
  int32_t n_attr;      /* 5 : c,x,y,w,h */
  int32_t d_model;     /* 464 */
  int32_t n_head;      /* 8 */
  int32_t d_ff;        /* 1856 */
  int32_t n_layer;     /* 4 */
  int32_t n_step;      /* T = 100 */
  int32_t precision;   /* LDM_PREC_* */
  int32_t max_batch;   /* largest B any call will use (workspace is sized for it) */
  int32_t chunk;       /* layouts processed per pass through the network (0 = auto = 256) so that the
                          activation working set stays inside the 256 MiB Infinity Cache */
  int32_t q_type;      /* LDM_Q_* (ABI 2) */
  int32_t lanes;       /* chunk pipelines run concurrently, each on its own stream / hipGraph, phase-shifted so that
                          their HBM-bound phases do not coincide (0 = auto = 2, 1 = one pipeline; ABI 3) */
} ldm_config;

/* sampling_cfg of the reference (helpers/sampling.py dataclasses) */
typedef struct {
  int32_t kind;      /* LDM_SAMPLE_* */
  float temperature; /* logits / temperature (stochastic kinds only), > 0.  ldm_sample_step / ldm_sample_loop draw on a
                      * token's own sub-vocabulary only and return an error when the classes outside it — log(1e-30)
                      * each, divided by the temperature like every class — would hold more than 2^-24 of the mass:
                      * n_class * exp(log(1e-30) / temperature) > 2^-24, i.e. temperature > 69.08 / log(2^24 * n_class)
                      * (3.19 for 155 classes).  ldm_sample_tokens draws over the full vocabulary: any temperature > 0. */
  float top_p;       /* LDM_SAMPLE_TOP_P */
  int32_t top_k;     /* LDM_SAMPLE_TOP_K */
} ldm_sampler;

/* Optional constraints == the `cond` dict consumed at base.py:243-284. All may be NULL/0. */
typedef struct {
  const int32_t* d_cond_seq;    /* (B,S) cond["seq"] */
  const uint8_t* d_strong_mask; /* (B,S) cond["mask"]: 1 = token fixed to cond_seq (base.py:245-251) */
  const float* d_weak_logits;   /* (B,C,S) refinement prior, added where !strong (base.py:254-258) */
  int32_t pad_disable;          /* cond["type"] in {c,cwh,refinement,relation} (base.py:272-284) */
} ldm_cond;

/* cond=relation: the graph of cond["batch_w_canvas"] (helpers/task.py:112-114) re-indexed per layout — node 0 =
 * canvas, node k = k-th element whose conditioned category is not PAD — plus the hyper-parameters of the logit
 * adjustment the reference applies between the posterior and the draw (base.py:261-269 -> update(),
 * categorical_diffusion/logit_adjustment.py:88-126, losses models/clg/const.py:221-236), relation_mode = "average". */
typedef struct {
  const int32_t* d_edge_offsets; /* (B+1) CSR offsets into the edge arrays */
  const int32_t* d_edge_src;     /* (n_edges) node id inside its layout's graph */
  const int32_t* d_edge_dst;
  const int32_t* d_edge_attr;    /* 1<<RelSize | 1<<RelLoc bitmasks (trainer/data/util.py:14-27,168) */
  const float* d_centres;        /* (4, n_bin) cluster centres in x,y,w,h order (float32, as update() casts them) */
  int32_t canvas_bins[4];        /* bbox_tokenizer.encode([0.5,0.5,1,1]) per coordinate, 0..n_bin-1 */
  float relation_lambda;         /* sampling_cfg.relation_lambda (SGD learning rate) */
  int32_t num_update;            /* sampling_cfg.relation_num_update */
  int32_t n_graph_total;         /* batch size of the whole sampling call: the loss is a mean over 14*B terms */
} ldm_relation;

/* ---- lifecycle ----------------------------------------------------------------------
 * ldm_create validates the whole geometry BEFORE it touches a device and returns -1 with ldm_last_error(NULL) naming
 * the field: n_attr == 5; d_model, d_ff multiples of 16, d_model <= 1024; d_model % n_head == 0, head dimension <= 64;
 * n_bin <= 128 and n_category + 4 n_bin + 2 <= 576 classes in LDM_PREC_EXACT_F32 / LDM_PREC_SPLIT_F16, <= 192 classes in
 * the fp16 modes (fast / mixed / hybrid: the message names the precision and points to split / exact; cond=relation
 * stays at n_bin <= 32 in every mode, rc -4); max_elem * n_attr <= 128 tokens in LDM_PREC_FAST_F16 (one score tile per
 * head; longer sequences: LDM_PREC_EXACT_F32, bounded by the LDS: 2 * S * head_dim floats <= 160 KiB).  The reference's
 * own configurations (rico25 / publaynet on the 464 / 8 / 1856 backbone, S = 125) run on the layout-resident kernels,
 * every other accepted geometry on generic tiled kernels (same numerics contract, lower throughput). */
int ldm_create(const ldm_config* cfg, int device, ldm_handle** out);
/* ldm_create with the norm1 kind (LDM_NORM1_*; additive export, ABI 5).  ldm_create(cfg, ..) is
 * ldm_create_variant(cfg, LDM_NORM1_LAYER, ..).  LDM_NORM1_INSTANCE in LDM_PREC_FAST_F16 / MIXED / HYBRID fails with -1: the
 * message names the precision and points to split / exact.  ldm_describe reports norm1=instance (nothing for layer). */
int ldm_create_variant(const ldm_config* cfg, int norm1_kind, int device, ldm_handle** out);
void ldm_destroy(ldm_handle* h);
const char* ldm_last_error(const ldm_handle* h); /* h may be NULL: last create error */

/* ---- weights: the reference checkpoint format ------------------------
 * key = reference state_dict key with or without the "model.module." prefix; data = host
 * float32, C-contiguous, shape as in the checkpoint.  Replaces model.load_state_dict
 * (models/common/util.py:47-57, test.py:144-149).  The handle owns repacked device copies. */
int ldm_load_weight(ldm_handle* h, const char* key, const float* h_data, const int64_t* shape, int ndim);
/* builds the (S,D) positional table (nn_lib.py:112-127), the [T][L][2D] AdaLN table
 * (transformer_utils.py:79-81), fp16 weight copies; fails if a required key is missing.
 * The denoiser variant is read from the key set:
 *   transformer.pos_emb.pos_emb (rows >= S, D)      pos_emb=default (nn_lib.py:73-88): the table is its first S rows;
 *                                                   exactly one of it and the elem_emb / attr_emb pair must be present
 *   norm1.emb.weight + norm1.linear.*               adalayernorm / adainnorm (learned timestep embedding)
 *   norm1.linear.* alone                            adalayernorm_abs / adainnorm_abs: the [T][D] sinusoid of
 *                                                   SinusoidalPosEmb (transformer_utils.py:34-49) is built on the device
 *   norm1.weight + norm1.bias                       timestep_type None: the AdaLN table holds scale = w - 1, shift = b at every t
 *   norm1.emb.<n>.*                                 the *_mlp kinds: refused (the reference itself cannot run them) */
int ldm_finalize_weights(ldm_handle* h);

/* ---- parity hooks (one stage each) --------------------------------------------------- */
/* CategoricalTransformer.forward (nn_lib.py:191-237): tokens (B,S) -> logits (B,S,C) fp32 */
int ldm_denoise_logits(ldm_handle* h, const int32_t* d_tokens, int t, int B, float* d_logits, void* stream);
/* predict_start tail + q_posterior + cond overrides (base.py:131-144, constrained.py:135-206,
 * base.py:243-284): logits (B,S,C), tokens (B,S) -> log p(x_{t-1}|x_t) (B,C,S) fp32.
 * t_post = the timestep handed to q_posterior (noise_t [- skip_step], base.py:218-240). */
int ldm_posterior(ldm_handle* h, const float* d_logits, const int32_t* d_tokens, int t_post, int B,
                  const ldm_cond* cond, float* d_logp, void* stream);
/* helpers/sampling.py:81-130 on a (B,C,S) log-prob tensor -> (B,S) int32 tokens.  cond (may be NULL): only
 * d_cond_seq + pad_disable are used — the [PAD] disabling of base.py:272-284, which the reference applies right
 * before the draw (for cond=relation: after the logit adjustment). */
int ldm_sample_tokens(ldm_handle* h, const float* d_logp, const ldm_cond* cond, const ldm_sampler* s, uint64_t seed,
                      uint64_t first_layout, int step, int B, int32_t* d_tokens_out, void* stream);

/* ---- the hot path -------------------------------------------------------------------- */
/* One reverse step (_sample_single_step, base.py:205-291), fused: tokens (B,S) -> tokens.
 * rel (may be NULL): cond["type"] == "relation" — the step then runs posterior (+ strong mask) -> logit adjustment
 * (t_model >= 10) -> [PAD] disable -> draw, exactly the reference's order. */
int ldm_sample_step(ldm_handle* h, const int32_t* d_tokens_in, int32_t* d_tokens_out, int t_model,
                    int t_post, const ldm_cond* cond, const ldm_relation* rel, const ldm_sampler* s, uint64_t seed,
                    uint64_t first_layout, int step, int B, void* stream);
/* The T-step reverse loop (BaseMaskAndReplaceDiffusion.sample, base.py:293-371).
 * d_tokens_inout: initial state (all [MASK] for unconditional, cond["seq"] otherwise) -> final.
 * h_t_model / h_t_post: host arrays of n_steps timesteps (diffusion_list and the posterior's t).
 * rel: NULL, or the relation graph of the B layouts (cond must then carry d_cond_seq).
 * d_intermediates: optional (n_steps,B,S) int32 (get_intermediate_results=True).
 * In LDM_PREC_FAST_F16 on the reference's backbone (and without rel) the whole loop is ONE launch: every layout's
 * workgroup runs all its steps (tokens in LDS, the step's tail behind the vocabulary head); use_graph is then moot.
 * Otherwise, use_graph != 0: the whole loop is captured once per (B, schedule, sampler, cond / relation layout) into
 * a hipGraph and replayed (seed / first_layout live in device memory so replays may change them; cond tensors,
 * the relation graph and the intermediates are staged through handle-owned buffers at fixed addresses). */
int ldm_sample_loop(ldm_handle* h, int32_t* d_tokens_inout, const ldm_cond* cond, const ldm_relation* rel,
                    const int32_t* h_t_model, const int32_t* h_t_post, int n_steps, const ldm_sampler* s,
                    uint64_t seed, uint64_t first_layout, int B, int32_t* d_intermediates, int use_graph,
                    void* stream);

/* ---- scoring GIVEN layouts: held-out loss / variational bound ---------------------------------
 * ConstrainedMaskAndReplaceDiffusion.forward (constrained.py:232-333) / VanillaMaskAndReplaceDiffusion.forward
 * (vanilla.py:160-240) as evaluation of a trained model: no gradients, nothing is written to the handle's weights.
 * Every call checks its tokens on the device and reads the result back before it returns (one stream synchronisation):
 * a token outside [0, C), a [MASK] in x_0, or a token that is not of its position's sub-vocabulary fails with -6.
 * t outside [0, n_step) fails with -1. */
/* x_t ~ q(x_t | x_0) (q_sample, constrained.py:223-230): (B,S) int32 -> (B,S) int32.  Inverse CDF on one Philox4x32-10
 * uniform per token, keyed by (seed, first_layout + b, t, position), over the reference's exp(q_pred) — not the
 * reference's Gumbel-argmax stream on torch's generator, which cannot be reproduced.  Independent of how a batch is cut. */
int ldm_q_sample(ldm_handle* h, const int32_t* d_x0, int t, uint64_t seed, uint64_t first_layout, int B, int32_t* d_xt,
                 void* stream);
/* The bound's terms of timestep t for given x_0, x_t (B,S) int32 and the denoiser's logits (B,S,C) of (x_t, t).
 * d_sums (B,4) float64: per layout the SUMS over its tokens of kl (base.py:117-119 of the two posteriors), decoder nll
 * (util.py:30-31), the auxiliary kl (constrained.py:317-319) and the number of tokens whose argmax log_x0_recon is x_0;
 * the 1 / S of mean_except_batch, the t == 0 selection and the loss weights are the caller's.  Fixed summation order
 * (lane tree per token in float32, then positions left to right in float64), no atomics: the bits repeat.
 * d_tok: NULL or (3,B,S) float32 per-token kl, nll, aux. */
int ldm_vb_terms(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, int t, int B,
                 double* d_sums, float* d_tok, void* stream);
/* ldm_q_sample (d_xt == NULL; else the given state) -> the denoiser pass of the handle's numerics mode -> ldm_vb_terms,
 * chunk by chunk through the handle's own workspace. */
int ldm_vb_step(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, int t, uint64_t seed, uint64_t first_layout,
                int B, double* d_sums, void* stream);

/* ---- the same at a timestep PER LAYOUT, one denoiser pass for the whole call (additive exports, ABI 5) ------------
 * The reference's forward() gives every layout of a batch its own t.  h_t: HOST array of B timesteps, as ldm_sample_loop takes
 * h_t_model; a value outside [0, n_step) fails with -1 and names its index.  The array is read before the call returns and
 * staged in a handle-owned device buffer of max_batch ints (allocated by the first such call: make that one outside a stream
 * capture).  Row b of the result has the bits the single-t call at t = h_t[b] gives row b of the same batch: only the AdaLN
 * parameters, the schedule rows and the Philox counter depend on t, and each takes the row's value.
 * h_layout: NULL, or B host values — the layout index in the Philox key of row b is first_layout + (h_layout ? h_layout[b] : b),
 * so that one layout may stand in several rows of a call, at several t, and still draw what
 * ldm_q_sample(.., t, seed, first_layout + its index, ..) draws for it.
 * Token checks and the error-word read-back as above.  -4: the handle's denoiser has no per-layout form — LDM_PREC_FAST_F16 on
 * the reference's backbone (the stack kernel); ldm_describe reports per_layout_t=0|1. */
int ldm_denoise_logits_t(ldm_handle* h, const int32_t* d_tokens, const int32_t* h_t, int B, float* d_logits, void* stream);
int ldm_q_sample_t(ldm_handle* h, const int32_t* d_x0, const int32_t* h_t, const uint64_t* h_layout, uint64_t seed,
                   uint64_t first_layout, int B, int32_t* d_xt, void* stream);
int ldm_vb_terms_t(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, int B,
                   double* d_sums, float* d_tok, void* stream);
int ldm_vb_step_t(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, const uint64_t* h_layout,
                  uint64_t seed, uint64_t first_layout, int B, double* d_sums, void* stream);

/* ---- the training loss's gradient with respect to the logits it is computed from (additive export, ABI 5) ------------
 * d/dlogits of  sum_b  coef[b][0] * (t_b == 0 ? nll_b : kl_b) + coef[b][1] * (t_b == 0 ? nll_b : aux_b)   (token SUMS, as d_sums
 * reports them; the 1/S, 1/pt, 1/B, the auxiliary weight and the upstream gradient are folded into coef by the caller:
 * constrained.py:299-330).  h_t: HOST array of B timesteps as in ldm_vb_terms_t.  d_coef (B,2) float64 on the device (a coefficient
 * rounded to float32 moves the gradient further from the reference's float64 one than the reference's own float32 autograd is);
 * may be NULL when d_grad is.  d_grad (B,S,C) float32 or NULL (values only): every element is written, the [MASK] column and the
 * rows of refused tokens as 0.  d_sums (B,4) float64 or NULL, with the bits ldm_vb_terms_t gives on an LDM_PREC_EXACT_F32 handle.
 * Always the reference-precision (float64) log-softmax, whatever the handle's numerics mode: the logits are the caller's.  Runs no
 * denoiser; works on every handle, wide vocabularies and per_layout_t=0 included.  No floating-point atomics: two calls give the
 * same bits, and a layout's rows do not depend on the batch around it.  Return codes as ldm_vb_terms_t: -1 for a t out of range,
 * -6 for refused tokens. */
int ldm_vb_grad(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, int B,
                const double* d_coef, float* d_grad, double* d_sums, void* stream);

/* ---- near-tie report of deterministic decoding (ABI 4; tie_abs: ABI 5) ------------------------
 * north star: "token indices bit-exact under greedy/argmax decoding".  LDM_PREC_FAST_F16's logits carry an error that
 * depends on the checkpoint (3e-4 of max |logit| on the reference's init, 1e-3 on wider weights, more once attention rows
 * saturate: DESIGN.md section 3.5), so its argmax (sampling.py:88-90) can differ from the reference's where two classes
 * are closer than that error can move them.  With the report enabled every deterministic ldm_sample_step /
 * ldm_sample_loop marks, per (step, layout), whether some token of the layout was decided with a log-probability lead
 * over the runner-up below  max(tie_rel * max |logit of that token|, tie_abs).  The lead moves by at most 6 x the largest
 * absolute logits error of the token: with tie_abs = 6 x a bound on that error — MEASURED on the
 * checkpoint by the caller, layout_dm_amd/verified.py calibrate() — an unmarked token is the exact mode's token; the
 * caller re-checks the marked (step, layout) pairs in LDM_PREC_EXACT_F32.  tie_rel = tie_abs = 0 disables.  Not defined
 * for cond=relation (the draw follows an SGD on the log-probabilities): such calls fail while the report is enabled. */
int ldm_set_tie_report(ldm_handle* h, float tie_rel, float tie_abs);
/* flags of the most recent deterministic call: d_flags (n_steps, B) uint8, row i = i-th step of that call */
int ldm_get_tie_flags(ldm_handle* h, uint8_t* d_flags, int n_steps, int B, void* stream);
/* Development hook: which layouts of the most recent ldm_sample_loop call read their first step's logits from the handle's
 * step-0 table instead of running the denoiser (one-launch loop, all-[MASK] layouts: ldm_describe `step0_cache`).  host_out
 * (n) uint8 on the HOST, n <= max_batch; synchronises the device.  Fails where the handle has no such loop. */
int ldm_dev_step0_flags(ldm_handle* h, uint8_t* host_out, int n);
/* Development hook: the handle's cache of captured sampling loops (per-step path, use_graph): *entries = graphs held now (at most 8
 * keys, the oldest evicted), *captures = keys captured since ldm_create (one count per key, not per lane).  A call that replays a
 * cached key changes neither.  Touches no device state. */
int ldm_dev_graph_cache(ldm_handle* h, int* entries, int* captures);

/* ---- cond=relation, split-step form ------------------------------------------------------- */
/* The logit adjustment alone (`num_update` SGD steps on the mean relational-constraint loss, analytic gradient;
 * no-op for t < 10, logit_adjustment.py:107), for callers that drive the step stage by stage: call between
 * ldm_posterior (cond without pad_disable) and ldm_sample_tokens (cond with pad_disable). */
int ldm_relation_update(ldm_handle* h, float* d_logp_inout, const int32_t* d_cond_seq, const ldm_relation* rel,
                        int t, int B, void* stream);

/* ---- result packaging ----------------------------------------------------------------- */
/* ids -> {bbox, label, mask}: LayoutSequenceTokenizer.decode (helpers/layout_tokenizer.py:255-266) +
 * BboxTokenizer.decode (helpers/bbox_tokenizer.py:117-168) for var_order c-x-y-w-h with the stacked
 * x-y-w-h bbox vocabulary and no bos/eos (the LayoutDM configuration), which LayoutDM.sample
 * (models/layoutdm.py:77-88) runs on the host inside the reference's timed region (test.py:194-203).
 * d_tokens: (B,S) int32.  d_centres: NULL for bbox_quantization=linear, else the (4,n_bin) float64
 * cluster centres in x,y,w,h order (kmeans / percentile).  box_f64: 0 -> d_bbox is (B,E,4) float32
 * (what the reference returns for linear), 1 -> float64 (what it returns for kmeans/percentile).
 * d_label: (B,E) int64, d_mask: (B,E) uint8 (bool). */
int ldm_decode_layouts(ldm_handle* h, const int32_t* d_tokens, int B, const double* d_centres, int box_f64,
                       void* d_bbox, int64_t* d_label, uint8_t* d_mask, void* stream);

/* ---- FID feature extractor ------------------------------------------------
 * FIDNetV3.extract_features (trainer/fid/model.py:123-164): {bbox, label, padding_mask} -> the 256-d feature of the
 * [token] slot, which trainer/eval.py feeds to compute_generative_model_scores (helpers/metric.py:37-59: FID,
 * precision / recall / density / coverage).  Own handle: the network has its own checkpoint (model.py:182-193).
 * d_bbox (B,N,4) float32, d_label (B,N) int64, d_padding_mask (B,N) uint8 (1 = padded, i.e. ~mask), d_feat (B,256). */
typedef struct ldm_fid ldm_fid;
int ldm_fid_create(int num_label, int max_bbox, int d_model, int n_head, int n_layer, int device, ldm_fid** out);
void ldm_fid_destroy(ldm_fid* h);
const char* ldm_fid_last_error(const ldm_fid* h); /* h may be NULL: last create error */
/* key = FIDNetV3 state_dict key (emb_label.weight, fc_bbox.*, enc_fc_in.*, enc_transformer.token,
 * enc_transformer.core.layers.<i>.{self_attn.in_proj_*, self_attn.out_proj.*, linear1.*, linear2.*, norm1.*, norm2.*});
 * decoder-half keys are accepted and ignored.  host float32, C-contiguous. */
int ldm_fid_load_weight(ldm_fid* h, const char* key, const float* h_data, const int64_t* shape, int ndim);
int ldm_fid_finalize(ldm_fid* h);
int ldm_fid_features(ldm_fid* h, const float* d_bbox, const int64_t* d_label, const uint8_t* d_padding_mask, int B,
                     int N, float* d_feat, void* stream);

/* Precision / recall / density / coverage of two feature sets (the other four entries of compute_generative_model_scores,
 * helpers/metric.py:37-59, which the reference takes from prdc.compute_prdc(real_features, fake_features, nearest_k=5)):
 * d_real (n_real, dim), d_fake (n_fake, dim) float32 device; h_out4 = {precision, recall, density, coverage} on the HOST
 * (the call synchronises `stream`); 1 <= nearest_k <= 7.  Uses the current device; workspace is allocated and freed
 * inside the call (max(n_real, n_fake)^2 floats; at most 65 536 features per set, -6 beyond). */
int ldm_prdc(const float* d_real, int n_real, const float* d_fake, int n_fake, int dim, int nearest_k, float* h_out4,
             void* stream);

/* ---- alignment / overlap of generated layouts (r05; the remaining per-layout metrics of eval.py) ---------------------
 * compute_alignment + compute_overlap (trainer/helpers/metric.py:98-203, called on every generated batch at
 * eval.py:153-155,203-205) on decoded layouts resident in HBM — what ldm_decode_layouts wrote: d_bbox (B,S,4) float32
 * (xc, yc, w, h), d_mask (B,S) uint8 (1 = valid element), 1 <= S <= 256.  d_out6 (B,6) float32, per layout:
 * alignment-ACLayoutGAN, alignment-LayoutGAN++, alignment-NDN, overlap-ACLayoutGAN, overlap-LayoutGAN++,
 * overlap-LayoutGAN (the reference's dictionary keys, in its order).  fp32 like the reference; sums in index order
 * (parity to fp32 rounding).  Uses the current device; no handle.  Returns 0, -1 (bad argument) or -2 (launch failed). */
int ldm_layout_metrics(const float* d_bbox, const uint8_t* d_mask, int B, int S, float* d_out6, void* stream);

/* ---- average IoU, DocSim, Max-IoU (the IoU-family metrics of eval.py) --------------------------------------------------
 * trainer/helpers/metric.py:300-507 (eval.py:173-176,211-215).  Device pointers in and out, no handle, the current device.
 * box_f64 as in ldm_decode_layouts: 0 -> float32 boxes, 1 -> float64 (xc, yc, w, h), (rows, S, 4).  The compute type is
 * double if any input is float64 (numpy's promotion); each box's l / t / r / b / area in its own dtype.  1 <= S <= 32.
 * Returns 0, -1 (bad argument: nothing launched) or -2 (launch failed).  Results are float64. */
/* per layout: d_out2 (B,2) = {average_iou-BLT, average_iou-VTN}; d_mask (B,S) uint8 (1 = element; any slots). */
int ldm_eval_average_iou(const void* d_bbox, int box_f64, const uint8_t* d_mask, int B, int S, double* d_out2, void* stream);
/* per pair b: DocSim of (layout b of set 1, layout b of set 2); d_n1 / d_n2 (B) int32 element counts, the elements first in
 * their rows; d_label* (B,S) int64.  d_out (B).  *d_err (int32, zeroed by the call): bit 0 = a non-finite similarity. */
int ldm_eval_docsim(const void* d_bbox1, int box1_f64, const int64_t* d_label1, const int32_t* d_n1, const void* d_bbox2,
                    int box2_f64, const int64_t* d_label2, const int32_t* d_n2, int B, int S, double* d_out, int32_t* d_err,
                    void* stream);
/* Max-IoU pair scores of groups of layouts that share a label multiset, every layout's elements sorted stably by label:
 * d_bbox1 (R1,S,4) + d_label1 (R1,S) int64, d_bbox2 (R2,S,4).  d_groups (G,6) int64 rows {first1, n1, first2, n2, n_elem,
 * out_offset}, ordered by out_offset; group g fills d_out[out_offset + j * n1 + i] with the score of (set-1 row first1 + i,
 * set-2 row first2 + j) (the reference's flat order), n_pairs = sum n1 * n2.  max_seg (<= S): the longest run of equal labels.
 * *d_err (zeroed by the call): bit 0 = a NaN / infinite IoU (the reference raises there), bit 1 = a run longer than
 * max_seg, bit 2 = a malformed group row. */
int ldm_eval_max_iou_pairs(const void* d_bbox1, int box1_f64, const int64_t* d_label1, int R1, const void* d_bbox2, int box2_f64,
                           int R2, int S, const int64_t* d_groups, int G, int64_t n_pairs, int max_seg, double* d_out,
                           int32_t* d_err, void* stream);

/* ---- relation violation score (compute_violation of the sampling entry point) -------------------------------------------
 * trainer/helpers/metric.py:62-95 (test.py:230-254): per layout, failures / valid over the edges of its relation graph, with
 * detect_size_relation / detect_loc_relation (data/util.py:33-69) on the sampled boxes.  Device pointers in and out, no handle,
 * the current device; box_f64 as above.  The graph is the per-layout CSR edge list of cond["batch_w_canvas"]:
 * d_edge_off (n_graph+1) int32, d_src / d_dst (n_edge) int32 LOCAL node ids, d_attr (n_edge) int32 relation bitmasks,
 * d_first_node (n_graph) int64 = the global id of each graph's node 0 as `batch` defines it, d_canvas (n_nodes) uint8 =
 * (y == 0).  The box row of an edge end is first_node[graph] + local id.  d_out (n_graph) float32 (NaN where no relation is
 * known, like the reference); d_edge_out (n_edge,3) int32 {size code, loc code, failures} in CSR edge order, or NULL.
 * *d_err (int32, zeroed by the call): bit 0 = an edge names a row beyond the box rows (the reference raises an IndexError),
 * bit 1 = malformed graph (offsets, node ids); the scores of such layouts are NaN.  n_graph >= 1; n_edge may be 0.
 * Returns 0, -1 (bad argument: nothing launched) or -2 (launch failed). */
/* flattened form: d_bbox (n_rows,4) = bbox_flatten. */
int ldm_relation_violation(const void* d_bbox, int box_f64, int64_t n_rows, const uint8_t* d_canvas, int64_t n_nodes,
                           const int32_t* d_edge_off, const int32_t* d_src, const int32_t* d_dst, const int32_t* d_attr,
                           const int64_t* d_first_node, int n_graph, int n_edge, float* d_out, int32_t* d_edge_out,
                           int32_t* d_err, void* stream);
/* dense form: d_bbox (B,S,4) + d_mask (B,S) uint8 as ldm_decode_layouts leaves them; rows are those of bbox_c[mask_c] with the
 * canvas box (0.5, 0.5, 1, 1) in front of every layout (test.py:232-250).  d_row_start (B+1) int32 is filled with the first
 * row of every layout (workspace and by-product).  B >= 1, S >= 1. */
int ldm_relation_violation_dense(const void* d_bbox, int box_f64, const uint8_t* d_mask, int B, int S, int32_t* d_row_start,
                                 const uint8_t* d_canvas, int64_t n_nodes, const int32_t* d_edge_off, const int32_t* d_src,
                                 const int32_t* d_dst, const int32_t* d_attr, const int64_t* d_first_node, int n_graph,
                                 int n_edge, float* d_out, int32_t* d_edge_out, int32_t* d_err, void* stream);

/* ---- cond= inputs from raw layouts (tokenizer.encode, get_cond and the relation transforms) --------------------------------
 * helpers/layout_tokenizer.py:208-253 + helpers/bbox_tokenizer.py:84-115 (encode), helpers/task.py:27-151 (get_cond),
 * data/util.py:111-177 (AddCanvasElement + AddRelationConstraints, use_v1=False) for the LayoutDM tokenizer configuration
 * ldm_decode_layouts assumes (c-x-y-w-h, stacked x-y-w-h vocabulary, [pad, mask], pad_until_max, no bos / eos).  Device
 * pointers in and out, no handle, the current device.  Layouts are dense: d_bbox (B,E,4) float32 / float64 by box_f64 (16- /
 * 32-byte aligned), d_label (B,E) int64, d_mask (B,E) uint8 (1 = element; a prefix of every row), 1 <= E <= 32.
 * *d_err (int32, zeroed by the call): bit 0 = a mask that is not a prefix, bit 1 = a non-finite coordinate on a valid element,
 * bit 2 = a label outside [0, n_category) on a valid element.  Returns 0, -1 (bad argument: nothing launched) or -2 (launch
 * failed).
 * Own draws use Philox4x32-10 keyed by (seed, first_layout + layout index, purpose, slot): the result does not depend on how
 * a batch is cut.  They follow the reference's DISTRIBUTIONS, not its random / torch streams. */
#define LDM_QUANT_LINEAR 0
#define LDM_QUANT_PERCENTILE 1
#define LDM_QUANT_KMEANS 2
#define LDM_COND_NONE 0        /* the plain tokenizer.encode ("gt") */
#define LDM_COND_C 1
#define LDM_COND_CWH 2
#define LDM_COND_PARTIAL 3
#define LDM_COND_REFINEMENT 4
#define LDM_COND_RELATION 5
/* encode + the cond rule in one pass.  quant / d_centres: LDM_QUANT_LINEAR with NULL, else (4,n_bin) float64 sorted centres in
 * x, y, w, h order (n_bin <= 128); kmeans picks the nearest centre by |float32(x) - c| in float64, lowest index on a tie.
 * d_keep (B,E) uint8: the per-element keep mask of LDM_COND_PARTIAL, or NULL = drawn (k = randint(1, vmax) if vmax > 1 else 1,
 * vmax = int((n - 1) * 0.3), then a uniform k-subset of the n elements).  d_noise (B,E,4) float32: the noise LDM_COND_REFINEMENT
 * adds to the boxes, or NULL = drawn (iid normal, sigma 0.1); d_noise_out (B,E,4) or NULL receives what was added.
 * d_seq (B,5E) int32, d_cond_mask (B,5E) uint8, d_seq_orig (B,5E) int32 (refinement; else may be NULL), d_num_element (B)
 * int32 or NULL. */
int ldm_encode_cond(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int E,
                    int n_category, int n_bin, int quant, const double* d_centres, int rule, const uint8_t* d_keep,
                    const float* d_noise, uint64_t seed, uint64_t first_layout, int32_t* d_seq, uint8_t* d_cond_mask,
                    int32_t* d_seq_orig, int32_t* d_num_element, float* d_noise_out, int32_t* d_err, void* stream);
/* cond["batch_w_canvas"]: node 0 of every layout is the canvas box (0.5, 0.5, 1, 1) with label 0, element labels + 1; for every
 * pair i < j in combinations order, attr = 1 << size | 1 << loc with UNKNOWN for a relation that is not sampled; an edge exists
 * where attr != both-unknown.  d_selection (B,2,E+1,E+1) uint8 [kind: 0 size, 1 loc][i][j] != 0 = sampled, or NULL = drawn:
 * exactly int(2 * C(n + 1, 2) * edge_ratio) of a layout's (kind, pair) candidates, uniformly without replacement.
 * With P = (E + 1) * E / 2: d_work (B, 2 P + 1) int32 workspace; the per-layout CSR ldm_relation_update and
 * ldm_relation_violation take: d_edge_off (B+1), d_src / d_dst / d_attr (capacity B * P) int32, d_first_node (B) int64; the
 * nodes (capacity B * (E + 1) rows): d_node_box (rows,4) in the boxes' dtype, d_node_label / d_node_batch int64, d_canvas
 * uint8; d_totals (2) int32 = {edges, nodes} actually written.  B >= 1. */
int ldm_relation_graph(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int E,
                       int n_category, const uint8_t* d_selection, double edge_ratio, uint64_t seed, uint64_t first_layout,
                       int32_t* d_work, int32_t* d_edge_off, int32_t* d_src, int32_t* d_dst, int32_t* d_attr,
                       int64_t* d_first_node, void* d_node_box, int64_t* d_node_label, int64_t* d_node_batch,
                       uint8_t* d_canvas, int32_t* d_totals, int32_t* d_err, void* stream);

/* cond["weak_logits"] of cond=refinement (set_additional_conditions_for_refinement, helpers/task.py:154-224) from the tokens of
 * cond["seq_orig"]:  d_out[b][c][s] = d_table[tok(b', s) * C + c] * weight, one float32 multiply (the sign of zero under a
 * negative weight included), b' = b when B_seq == B and b' = 0 when B_seq == 1 (duplicate_cond: one conditioning layout, B
 * samples).  d_seq_orig (B_seq,S) int64 (seq_i64 = 1, the reference's dtype) or int32 (0); d_table (C,C) float32 row-major
 * [token][class], the table of _index_to_smoothed_log_onehot BEFORE refine_lambda; weight = refine_lambda (negated for
 * refine_mode = negative); d_out (B,C,S) float32, what ldm_cond.d_weak_logits takes — any 4-byte aligned address.  S >= 1 and
 * C >= 1 are otherwise free (the output is limited to 2^31 - 1 pieces of 16 KiB).  *d_err (int32, zeroed by the call): bit 0 = a
 * token outside [0, C) (F.embedding raises an IndexError); its column of d_out is +0.0 and no table entry is read for it.
 * B == 0: nothing is launched or touched, 0.  Returns 0, -1 (bad argument: nothing launched) or -2 (launch failed). */
int ldm_refinement_prior(const void* d_seq_orig, int seq_i64, int B_seq, int B, int S, int C, const float* d_table, float weight,
                         float* d_out, int32_t* d_err, void* stream);

/* ---- coordinate bins from raw boxes (bin/clustering_coordinates.py) -------------------------------------------------------
 * The cluster centres the kmeans / percentile tokenizers read, fitted one coordinate at a time: sklearn KMeans(n_init
 * restarts of greedy k-means++ + Lloyd, the lowest inertia wins) and the reference's Percentile.fit.  Device pointers, no
 * handle, the current device.  The rules and every summation order: layout_dm_amd/csrc/ldm_cluster_core.h; all sums are
 * float64 in a fixed order and no floating-point atomic is used, so two runs give the same bits.  Own draws are Philox4x32-10
 * keyed by (random_state, problem id, restart): sklearn's distribution, not its stream.
 * A arrays of n float32 values each, row-major (A, n), 1 <= n <= 2^30; cluster counts 1 <= k <= 256, k <= n.
 * d_work: a 256-byte aligned workspace of at least ldm_cluster_workspace_bytes(A, n, P, n_init) bytes (P problems of n_init
 * restarts each; P = 0 measures ldm_cluster_sort alone).  One size serves every call below with those A, n, P, n_init.
 * Problems are rows {array, k, problem id} of an int32 (P, 3) table with k non-increasing, given twice: h_prob on the host
 * (launch shapes, checks) and d_prob, the same rows on the device.  Centres come back as (P, 256) rows, sorted, k valid.
 * Every call returns 0, -1 (bad argument: nothing launched) or -2 (launch failed). */
int ldm_cluster_workspace_bytes(int A, int64_t n, int P, int n_init, size_t* bytes);
/* Sorts each array ascending (clip01 = 1: clipped to [0, 1] first, what Percentile.fit does) and derives what the fits read:
 * d_sorted (A, n); d_ps / d_ps2 (A, n + 1) float64 prefix sums of x and x^2, [0] = 0; d_unique (A, n) the distinct values in
 * front and zeros behind; d_ps_unique (A, n + 1) their prefix sums; d_n_unique (A) int64.  *d_err (int32, zeroed by the call):
 * bit 0 = a NaN or an infinity in the input.  stages: LDM_CLUSTER_STAGE_SORT | LDM_CLUSTER_STAGE_DERIVE for the whole of
 * it; one of the two runs that half alone (for timing them apart; the error word belongs to the sort half). */
#define LDM_CLUSTER_STAGE_SORT 1   /* d_x -> d_sorted */
#define LDM_CLUSTER_STAGE_DERIVE 2 /* d_sorted -> prefix sums, distinct values (d_sorted as an earlier call left it) */
int ldm_cluster_sort(const float* d_x, int A, int64_t n, int clip01, int stages, float* d_sorted, double* d_ps, double* d_ps2, float* d_unique,
                     double* d_ps_unique, int64_t* d_n_unique, void* d_work, size_t work_bytes, int32_t* d_err, void* stream);
/* P problems x n_init restarts (1 <= n_init <= 64, P * n_init <= 65535) in one batch: seeding, Lloyd until sklearn's stopping
 * rule (tol * var(X), no boundary moved, max_iter), inertia by a direct pass; per problem the restart of the lowest inertia,
 * the lowest restart index on a tie.  first_restart: the restart index of the first of the n_init (a fit cut into several
 * calls draws the same numbers).  An empty cluster keeps its centre.  The caller makes sure every array holds at least k
 * distinct values (d_n_unique).  d_centres (P, 256) float64, d_inertia (P) float64, d_n_iter / d_best_restart (P) int32. */
int ldm_kmeans1d_fit(const float* d_sorted, const double* d_ps, const double* d_ps2, int A, int64_t n, const int32_t* h_prob,
                     const int32_t* d_prob, int P, int n_init, int first_restart, uint64_t random_state, int max_iter, double tol,
                     double* d_centres, double* d_inertia, int32_t* d_n_iter, int32_t* d_best_restart, void* d_work,
                     size_t work_bytes, void* stream);
/* Lloyd alone from explicit start centres d_start (P, 256) float64, each row's first k sorted ascending: the parity hook
 * against sklearn KMeans(init=..., n_init=1).  d_trace (max_iter, k) float64 or NULL: the centres after every iteration run
 * (P == 1 only). */
int ldm_kmeans1d_lloyd(const float* d_sorted, const double* d_ps, const double* d_ps2, int A, int64_t n, const int32_t* h_prob,
                       const int32_t* d_prob, int P, const double* d_start, int max_iter, double tol, double* d_centres,
                       double* d_inertia, int32_t* d_n_iter, double* d_trace, void* d_work, size_t work_bytes, void* stream);
/* Percentile.fit on the distinct values ldm_cluster_sort(clip01 = 1) left: h_n_unique (A) int64 on the host (the k rank
 * thresholds int(t_i * m) are evaluated there, in float64); d_centres (P, 256) float32, -1.0f for an empty bin.  Waits for
 * the stream. */
int ldm_percentile_fit(const double* d_ps_unique, int A, int64_t n, const int64_t* h_n_unique, const int32_t* h_prob,
                       const int32_t* d_prob, int P, float* d_centres, void* d_work, size_t work_bytes, void* stream);
/* predict: d_ids[i] = the bin ldm_encode_cond gives value d_x[i] under d_centres (k) float64 sorted centres; quant =
 * LDM_QUANT_KMEANS or LDM_QUANT_PERCENTILE.  The same routine, not a second rule. */
int ldm_nearest_centre(const float* d_x, int64_t n, const double* d_centres, int k, int quant, int32_t* d_ids, void* stream);
/* Development hook: one run (one array, one k, one restart) with every stage kept.  d_sorted (n), d_ps / d_ps2 (n + 1); per
 * seeding step s < k, 7 slots each of which the first L are written (L = 1 at s = 0, else 2 + int(ln k)): d_unif the uniforms,
 * d_cand (int64) the candidate indices into d_sorted, d_pots the potential each would leave; d_pick (k) int64 the index kept;
 * d_dist (k, n) float64 or NULL: the squared distances the draws of step s >= 1 were made over (row 0 is not written);
 * d_lloyd (max_iter, k) the centres after each iteration run; d_centres (256), d_inertia (1), d_n_iter (1). */
int ldm_dev_cluster_stages(const float* d_x, int64_t n, int k, uint64_t random_state, int problem_id, int restart, int max_iter,
                           double tol, float* d_sorted, double* d_ps, double* d_ps2, double* d_unif, int64_t* d_cand,
                           double* d_pots, int64_t* d_pick, double* d_dist, double* d_lloyd, double* d_centres, double* d_inertia,
                           int32_t* d_n_iter, void* d_work, size_t work_bytes, int32_t* d_err, void* stream);

/* ---- generated layouts as pictures (save_image of the sampling entry point) ---------------------------------------------
 * trainer/helpers/visualization.py:17-115 (test.py:205-214): every layout on a white H x W canvas, its elements drawn from
 * the larger to the smaller area (stable) as Pillow's ImageDraw.rectangle draws them — fill blended with alpha 100, opaque
 * outline — pixel for pixel.  Device pointers in and out, no handle, the current device; box_f64 as above.
 * d_bbox (B,S,4) xc yc w h, d_label (B,S) int64, d_mask (B,S) uint8 as ldm_decode_layouts leaves them; d_colors (n_colors,3)
 * uint8 RGB per label.  1 <= S <= 256, 1 <= H, W <= 16384, 0 <= pad <= 16384, cols >= 1.
 * d_out is a (GH, GW, 3) uint8 mosaic of B tiles in `cols` columns with `pad` black pixels around every tile, torchvision's
 * make_grid(nrow, padding, pad_value = 0) for cols = min(nrow, B):
 *   GH = ceil(B / cols) * (H + pad) + pad,  GW = cols * (W + pad) + pad   (ldm_render_grid_shape),
 *   tile k starts at row (k / cols) * (H + pad) + pad, column (k % cols) * (W + pad) + pad.
 * cols = 1, pad = 0 is the batch form (B, H, W, 3).  The padding and the empty tiles of a last row are zeroed by the call.
 * *d_err (int32, zeroed by the call): bit 0 = an unmasked box is not finite or has a negative w or h (Pillow raises a
 * ValueError), bit 1 = an unmasked label is outside [0, n_colors) (an IndexError); such an element is not drawn, every
 * other one is.  Returns 0, -1 (bad argument: nothing launched) or -2 (launch failed). */
int ldm_render_layouts(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int S,
                       const uint8_t* d_colors, int n_colors, int H, int W, int cols, int pad, uint8_t* d_out, int32_t* d_err,
                       void* stream);
/* (GH, GW) of the mosaic above; -1 when an argument is out of range.  Host only: no device is touched. */
int ldm_render_grid_shape(int B, int H, int W, int cols, int pad, int64_t* GH, int64_t* GW);

/* ---- introspection ------------------------------------------------------------------- */
/* average device time (ms) of the most recent ldm_sample_loop, measured with HIP events on the
 * stream it ran on; blocks until that loop has finished. */
int ldm_last_loop_ms(ldm_handle* h, float* ms);
/* name + accumulated ms + launches of every kernel class timed when profiling is enabled
 * (ldm_set_profiling(h,1) brackets each launch with HIP events; slow, for bench/roofline only) */
int ldm_set_profiling(ldm_handle* h, int enable);
int ldm_profile_count(ldm_handle* h);
int ldm_profile_get(ldm_handle* h, int idx, const char** name, double* total_ms, int64_t* launches,
                    double* flops, double* bytes);
int ldm_profile_reset(ldm_handle* h);
int ldm_abi_version(void);
/* "key=value;..." description of what the handle runs — numerics mode, kernel family, one-launch loop or per-step
 * graphs, chunk / lanes, near-tie thresholds — and the development knobs the library honoured in this process.
 * Environment knobs (LDM_STACK_LOOP, LDM_FUSED_ATTN, ...: INTEGRATION.md section 5) select development / ablation paths;
 * they are honoured only together with LDM_DEV=1, and ldm_create fails while one is set without it.
 * Writes at most cap - 1 characters + NUL; returns the length needed (ABI 5). */
int ldm_describe(const ldm_handle* h, char* buf, int cap);

/* Build provenance: "LDM_SRC_DIGEST=" followed by the sha256 (64 hex digits) of the sources this library was built from
 * (layout_dm_amd/build.py source_digest(): csrc, this header, the source list and the flags).  build.py and binding.py compare
 * it with the tree before loading a prebuilt library; ldm_describe reports it as src_digest. */
extern const char ldm_build_source_digest[];
/* layouts per chunk and number of concurrent lanes the handle was created with (after the 0 = auto defaults) */
int ldm_get_layout(const ldm_handle* h, int* chunk, int* lanes);

#ifdef __cplusplus
}
#endif
#endif /* LDM_HIP_H */
