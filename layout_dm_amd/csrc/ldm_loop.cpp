// Host side of libldm_hip.so: the hot path — one reverse step (_sample_single_step, base.py:205-291), the one-launch loop of
// the fast mode, and the per-lane hipGraph loop of the per-step path (BaseMaskAndReplaceDiffusion.sample, base.py:293-371).
#include "ldm_handle.h"

using namespace ldm_host;

void ldm_host::fill_post(ldm_handle* h, PostArgs& p, const ldm_cond* cond, const ldm_sampler* s, size_t layout_off,
                      int Bc) {
  p.sched = h->sched;
  p.f32_lse = h->plan.fast() ? 1 : 0;
  p.T = h->T;
  p.B = Bc;
  p.S = h->plan.S;
  p.v = h->vocab;
  p.rng = h->rng;
  if (cond) {
    const size_t ro = layout_off * h->plan.S;
    p.cond_seq = cond->d_cond_seq ? cond->d_cond_seq + ro : nullptr;
    p.strong = cond->d_strong_mask ? cond->d_strong_mask + ro : nullptr;
    p.weak = cond->d_weak_logits ? cond->d_weak_logits + layout_off * h->plan.C * h->plan.S : nullptr;
    p.pad_disable = cond->pad_disable;
  }
  if (s) {
    p.kind = s->kind;
    p.temperature = s->temperature;
    p.top_p = s->top_p;
    p.top_k = s->top_k;
  }
}

int ldm_host::check_ready(ldm_handle* h, int B) {
  if (!h) return -1;
  if (!h->finalized) return h->fail(-5, "weights not finalized: call ldm_finalize_weights first");
  if (B < 1 || B > h->cfg.max_batch) return h->fail(-1, "batch %d outside [1, max_batch=%d]", B, h->cfg.max_batch);
  return 0;
}

int ldm_host::check_sampler(ldm_handle* h, const ldm_sampler* s) {
  if (!s) return h->fail(-1, "null sampler");
  if (s->kind < 0 || s->kind > 4) return h->fail(-1, "unknown sampler kind %d", s->kind);
  if (s->kind != LDM_SAMPLE_DETERMINISTIC && !(s->temperature > 0.f)) return h->fail(-1, "temperature must be > 0");
  if (s->kind == LDM_SAMPLE_TOP_P && !(s->top_p > 0.f && s->top_p <= 1.f)) return h->fail(-1, "top_p must be in (0,1]");
  if (s->kind == LDM_SAMPLE_TOP_K && (s->top_k < 1 || s->top_k > h->plan.C)) return h->fail(-1, "top_k out of range");
  return 0;
}

// ldm_sample_step / ldm_sample_loop draw on a token's LIVE classes only (SlotMap<., ., LIVE> of ldm_post_token.h: the tail
// of the stack kernel and posterior_sample_k's 16-lane form) and skip strong-masked positions.  The reference divides the
// dead classes' log(1e-30) by the temperature like every other class (helpers/sampling.py:90), so together they hold up to
// C * exp(log(1e-30) / T) of the mass.  While that stays within the 2^-24 resolution of the draw's uniform the forms agree
// draw for draw; above (T > 3.19 for 155 classes) the live-class forms would sample another distribution than the
// reference and than ldm_sample_tokens' full-vocabulary form: refused, never approximated.
int ldm_host::check_live_temperature(ldm_handle* h, const ldm_sampler* s) {
  if (s->kind == LDM_SAMPLE_DETERMINISTIC) return 0;
  const double log_eps = std::log(1e-30);  // util.py:8
  const double dead_mass = (double)h->plan.C * std::exp(log_eps / (double)s->temperature);
  if (dead_mass > std::ldexp(1.0, -24))
    return h->fail(-1, "temperature %g puts %.3g of the mass on classes outside a token's sub-vocabulary (more than 2^-24): "
                       "the step / loop draw on the live classes only and must be given temperature <= %.4f for %d classes",
                   (double)s->temperature, dead_mass,
                   -log_eps / std::log(std::ldexp(1.0, 24) * (double)h->plan.C), h->plan.C);
  return 0;
}

// where ldm_sample_step's and ldm_sample_loop's checks coincide: the stretch in front of their argument checks
static int check_call(ldm_handle* h, const ldm_sampler* s, int B) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if ((rc = check_sampler(h, s))) return rc;
  return check_live_temperature(h, s);
}

static int check_timestep_range(ldm_handle* h, const int32_t* t_model, const int32_t* t_post, int n) {
  return check_timesteps(t_model, t_post, n, h->T) ? 0 : h->fail(-1, kTimestepRangeMsg, h->T);
}

static int check_relation(ldm_handle* h, const ldm_relation* rel, const ldm_cond* cond, int B) {
  if (!rel) return 0;
  if (!cond || !cond->d_cond_seq) return h->fail(-1, "cond=relation needs cond->d_cond_seq (the conditioned sequence)");
  if (!rel->d_edge_offsets || !rel->d_centres) return h->fail(-1, "ldm_relation: null edge offsets / centres");
  if (rel->n_graph_total < B) return h->fail(-1, "ldm_relation.n_graph_total smaller than B");
  if (h->cfg.max_elem > 32 || h->cfg.n_bin > 32) return h->fail(-4, "relation kernel: max_elem and n_bin must be <= 32");
  for (int x = 0; x < 4; ++x)
    if (rel->canvas_bins[x] < 0 || rel->canvas_bins[x] >= h->cfg.n_bin) return h->fail(-1, "canvas bin out of range");
  // The (chunk, C, S) log-probability buffer exists only for the three-launch form of an adjusted step (posterior ->
  // relation_update -> draw): the one-launch loop and relation_step_k keep the rows in LDS.  Allocated here, never inside
  // step_all (which may run under stream capture), and only when that form can be reached.
  PostArgs probe{};
  fill_post(h, probe, nullptr, nullptr, 0, 1);
  const bool three_launch = !loop_fusable(h, rel) && !relation_step_supported(probe);
  for (int l = 0; three_launch && l < h->plan.n_lanes; ++l) {
    if (h->ws[l].rel_logp) continue;
    float* buf = nullptr;
    int rc = h->dalloc(&buf, (size_t)h->plan.chunk * h->plan.C * h->plan.S, false);
    if (rc) return rc;
    h->ws[l].rel_logp = buf;
  }
  return 0;
}

void ldm_host::fill_rel(ldm_handle* h, RelArgs& a, const ldm_relation* rel, size_t layout_off, int Bc) {
  a.edge_off = rel->d_edge_offsets + layout_off;  // offsets are absolute positions in the edge arrays
  a.edge_src = rel->d_edge_src; a.edge_dst = rel->d_edge_dst; a.edge_attr = rel->d_edge_attr;
  a.centres = rel->d_centres;
  for (int x = 0; x < 4; ++x) a.canvas_bins[x] = rel->canvas_bins[x];
  a.step = rel->relation_lambda / (14.0f * (float)rel->n_graph_total);
  a.num_update = rel->num_update; a.B = Bc; a.C = h->plan.C; a.S = h->plan.S; a.A = h->cfg.n_attr;
  a.n_category = h->cfg.n_category; a.n_bin = h->cfg.n_bin; a.pad_id = h->vocab.pad_id;
}

// one fused reverse step over the whole batch, chunk by chunk through the workspace `ws`.  `cond` / `rel` describe layouts
// 0..B of THIS call (the loop body hands over pointers already advanced to its chunk); rel_layout_off = position of row 0
// inside the relation graph's CSR offsets.  The timesteps are the entry point's, already through check_timestep_range; the
// chunk loop is the workspace's capacity (a pass of the loop body is one chunk at most), not a cut of the call.
static int step_all(ldm_handle* h, Workspace& ws, const int32_t* tin, int32_t* tout, int t_model, int t_post, const ldm_cond* cond,
                    const ldm_relation* rel, size_t rel_layout_off, const ldm_sampler* s, int step, int B,
                    size_t rng_layout_off, hipStream_t st, bool skip_embed = false, bool embed_next = false,
                    int tie_row = -1) {
  for (int off = 0; off < B; off += h->plan.chunk) {
    const int Bc = std::min(h->plan.chunk, B - off);
    int rc = denoise_chunk(h, ws, tin + (size_t)off * h->plan.S, t_model, Bc, st, skip_embed);
    if (rc) return rc;
    PostArgs p{};
    fill_post(h, p, cond, s, off, Bc);
    p.logits = ws.logits;
    p.ldl = h->plan.Cp;
    p.tokens = tin + (size_t)off * h->plan.S;
    p.t_post = t_post;
    p.step = step;
    p.layout_off = (int)(rng_layout_off + off);
    // the launch that draws the step's tokens also writes the next step's embedding rows (one chunk per call: run_loop_body)
    auto embed_into = [&](PostArgs& q) {
      if (embed_next) { q.x_next = ws.P; q.emb = h->emb; q.pos = h->pos; q.D = h->D; q.ldx = h->D; }
    };
    // cond=relation adjusts the log-probabilities only while t >= 10 (logit_adjustment.py:107); the remaining steps are
    // a plain constrained step with the [PAD] disable, i.e. the fused posterior + draw launch
    const bool adjust = rel && t_model >= 10 && rel->num_update > 0;
    if (!adjust) {
      if (rel) p.pad_disable = 1;
      p.tokens_out = tout + (size_t)off * h->plan.S;
      embed_into(p);
      if (tie_row >= 0 && h->tie_rel > 0.f && h->tie_flags && s->kind == LDM_SAMPLE_DETERMINISTIC) {
        p.tie_flags = h->tie_flags + (size_t)tie_row * h->cfg.max_batch + rng_layout_off + off;
        p.tie_rel = h->tie_rel;
        p.tie_abs = h->tie_abs;
      }
      ldm_handle::Scope sc(h, st, "posterior_sample", 0, (double)Bc * h->plan.S * (h->plan.Cp * 4 + 8));
      launch_posterior_sample(p, st);
      continue;
    }
    // cond=relation (base.py:243-291): posterior + strong mask -> logit adjustment -> [PAD] disable -> draw
    if (relation_step_supported(p)) {  // ... in ONE launch (r04)
      PostArgs q = p;
      q.pad_disable = 1;
      q.tokens_out = tout + (size_t)off * h->plan.S;
      embed_into(q);
      RelArgs a{};
      a.cond_seq = cond->d_cond_seq + (size_t)off * h->plan.S;
      fill_rel(h, a, rel, rel_layout_off + off, Bc);
      ldm_handle::Scope sc(h, st, "relation_step", 0, (double)Bc * h->plan.S * (h->plan.Cp * 4 + 8));
      launch_relation_step(q, a, st);
      continue;
    }
    if (!ws.rel_logp) return h->fail(-5, "cond=relation: the three-launch step has no log-probability buffer (check_relation)");
    {
      PostArgs q = p;
      q.pad_disable = 0;  // applied after the adjustment, below
      q.logp_out = ws.rel_logp;
      q.logp_tm = 1;  // (the handle's own buffer: token-major, a token's classes contiguous)
      q.tokens_out = nullptr;
      ldm_handle::Scope sc(h, st, "posterior", 0, (double)Bc * h->plan.S * (h->plan.Cp * 4 + h->plan.C * 4));
      launch_posterior_sample(q, st);
    }
    {
      RelArgs a{};
      a.logp = ws.rel_logp;
      a.logp_tm = 1;
      a.cond_seq = cond->d_cond_seq + (size_t)off * h->plan.S;
      fill_rel(h, a, rel, rel_layout_off + off, Bc);
      ldm_handle::Scope sc(h, st, "relation_update", 0, (double)Bc * 4 * h->cfg.n_bin * h->cfg.max_elem * 8);
      launch_relation_update(a, st);
    }
    {
      PostArgs q{};
      fill_post(h, q, cond, s, off, Bc);
      q.strong = nullptr;  // already imposed on rel_logp
      q.weak = nullptr;
      q.pad_disable = 1;
      q.logp_in = ws.rel_logp;
      q.logp_tm = 1;
      q.tokens_out = tout + (size_t)off * h->plan.S;
      q.step = step;
      q.layout_off = (int)(rng_layout_off + off);
      embed_into(q);
      ldm_handle::Scope sc(h, st, "pad_disable_sample", 0, (double)Bc * h->plan.S * (h->plan.C * 4 + 8));
      launch_posterior_sample(q, st);
    }
  }
  return 0;
}

// ---- the whole reverse loop in one launch (kernels_stack.hip HEAD == 2) -----------------------------------------
// Eligible: fast numerics on the layout-resident kernels (the reference's backbone, S <= 128), a vocabulary of 5 head
// tiles whose attribute sub-vocabularies fit the fused tail.  cond=relation (r04): its logit adjustment couples the
// elements of a layout through an SGD on the log-probabilities — the layout's workgroup holds them in LDS behind the
// vocabulary head, so the adjusted steps run posterior -> SGD -> [PAD] disable -> draw in the same launch
// (stack_stream_k<., 2, true>); needs the constrained vocabulary with <= 32 bins and <= 32 elements.
bool ldm_host::loop_fusable(const ldm_handle* h, const ldm_relation* rel) {
  // (the geometry half: ldm_engine_plan.h loop_geometry / rel_loop_geometry; here what ldm_finalize_weights has to have built)
  return (rel ? h->plan.rel_loop_geometry : h->plan.loop_geometry) && h->head_img_ks && !h->fast.empty() && h->tbl_att_dyn;
}

// The step-0 logits table of (t0, S) for a launch on `st` (ldm_handle.h Step0Entry), built on first use; *tab = nullptr
// where this call has to run without it: the cache is off, the stream is being captured and the table is not known to be
// complete (the build must not be recorded into the caller's graph), or another stream's build is still in flight.
static int step0_table(ldm_handle* h, const StackWeights& sw, int t0, int t_post0, hipStream_t st,
                       const float** tab) {
  *tab = nullptr;
  if (!h->plan.step0_cache || !h->step0_tab) return 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  bool capturing = false;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {  // (e.g. the null stream while another stream captures globally)
    (void)hipGetLastError();
    capturing = true;
  } else {
    capturing = cs != hipStreamCaptureStatusNone;
  }
  for (auto& e : h->step0) {
    if (e.t != t0 || e.S != h->plan.S) continue;
    if (!e.settled && !capturing && hipEventQuery(h->step0_ev[e.slot]) == hipSuccess) e.settled = true;
    (void)hipGetLastError();  // (hipErrorNotReady is not an error of this call)
    if (e.settled || (!capturing && e.built_on == st)) *tab = h->step0_tab + (size_t)e.slot * kStackStep0Floats;
    return 0;
  }
  if (capturing) return 0;
  ldm_handle::Step0Entry e;
  e.t = t0; e.S = h->plan.S; e.built_on = st;
  if ((int)h->step0.size() >= kStep0Slots) {  // replace the oldest, once no launch of any stream can still read it
    e.slot = h->step0.front().slot;
    h->step0.erase(h->step0.begin());
    HIP_OK(h, hipDeviceSynchronize());
  } else {
    e.slot = (int)h->step0.size();
  }
  if (!h->step0_ev[e.slot]) HIP_OK(h, hipEventCreateWithFlags(&h->step0_ev[e.slot], hipEventDisableTiming));
  // the SAME instantiation as the real launch, one all-[MASK] layout, one step: the table holds what that kernel's registers held
  ldm_sampler det{};
  det.kind = LDM_SAMPLE_DETERMINISTIC;
  det.temperature = 1.f;
  PostArgs p{};
  fill_post(h, p, nullptr, &det, 0, 1);
  p.tokens = h->step0_tok;
  p.tokens_out = h->step0_tok + h->plan.S;
  p.emb = h->emb; p.pos = h->pos; p.D = h->D;
  const int32_t tm = t0, tp = t_post0;
  StackLoop lp{};
  lp.tables = sw.tables;
  lp.post = &p; lp.adaln = h->adaln; lp.t_model = &tm; lp.t_post = &tp;
  lp.n_steps = 1; lp.inter_ld = 1; lp.tie_ld = h->cfg.max_batch;
  lp.logits0_out = h->step0_tab + (size_t)e.slot * kStackStep0Floats;
  {
    ldm_handle::Scope sc(h, st, "step0_logits_build", 0, (double)kStackStep0Floats * 4);
    launch_stack_loop(sw.ls, h->F, h->D, 1, h->plan.S, h->H, h->plan.dh, sw.head, lp, st);
  }
  HIP_OK(h, hipEventRecord(h->step0_ev[e.slot], st));
  h->step0.push_back(e);
  *tab = lp.logits0_out;
  return 0;
}

// tokens_in -> tokens_out (may alias) through n_steps reverse steps; step0 = loop index of the first one (RNG counter
// word); cond pointers describe layout 0..B of this call; d_inter (n_steps, B, S) or nullptr; tie_row0 >= 0: near-tie
// flags of step i go to row tie_row0 + i of h->tie_flags; from_start: tokens_in is the start of a sampling call
// (ldm_sample_loop), whose all-[MASK] layouts may read their first step's logits from the handle's table
static int run_loop_fused(ldm_handle* h, const int32_t* tin, int32_t* tout, const ldm_cond* cond, const ldm_relation* rel,
                          const int32_t* t_model, const int32_t* t_post, int n_steps, const ldm_sampler* s, int step0, int B,
                          int32_t* d_inter, int tie_row0, hipStream_t st, bool from_start = false) {
  const int D = h->D, F = h->F, M = B * h->plan.S;
  const StackWeights sw = stack_weights(h, -1, nullptr);   // (the AdaLN rows of a step come from the kernel's tables)
  // (the roofline stays against the algorithmic work: n * step_flops, although the first pass of an all-[MASK] layout is a table read)
  const double step_flops = h->L * (gemm_flops(M, 3 * D, D) + 4.0 * B * h->H * (double)h->plan.S * h->plan.S * h->plan.dh +
                                    gemm_flops(M, D, D) + 2 * gemm_flops(M, F, D)) + gemm_flops(M, h->plan.C, D);
  const float* logits0 = nullptr;
  if (from_start && h->step0_flags) {
    int rc = step0_table(h, sw, t_model[0], t_post[0], st, &logits0);
    if (rc) return rc;
    HIP_OK(h, hipMemsetAsync(h->step0_flags, 0, (size_t)B, st));
  }
  for (int i0 = 0; i0 < n_steps; i0 += kStackLoopMaxSteps) {  // (timesteps travel in the kernel arguments)
    const int n = std::min(kStackLoopMaxSteps, n_steps - i0);
    PostArgs p{};
    fill_post(h, p, cond, s, 0, B);
    p.tokens = i0 == 0 ? tin : tout;
    p.tokens_out = tout;
    p.step = step0 + i0;
    p.layout_off = 0;
    p.emb = h->emb; p.pos = h->pos; p.D = D;
    RelArgs ra{};
    if (rel) {
      p.pad_disable = 1;  // cond type relation (base.py:272)
      fill_rel(h, ra, rel, 0, B);
    }
    if (tie_row0 >= 0 && h->tie_rel > 0.f && h->tie_flags && s->kind == LDM_SAMPLE_DETERMINISTIC) {
      p.tie_flags = h->tie_flags + (size_t)(tie_row0 + i0) * h->cfg.max_batch;
      p.tie_rel = h->tie_rel;
      p.tie_abs = h->tie_abs;
    }
    StackLoop lp{};
    lp.tables = sw.tables;
    lp.post = &p; lp.adaln = h->adaln; lp.t_model = t_model + i0; lp.t_post = t_post + i0;
    lp.inter = d_inter ? d_inter + (size_t)i0 * B * h->plan.S : nullptr;
    lp.n_steps = n; lp.inter_ld = B; lp.tie_ld = h->cfg.max_batch;
    lp.rel = rel ? &ra : nullptr;
    // (only the first segment of a call can start all-[MASK]; the kernel tests the tokens itself either way)
    lp.logits0 = i0 == 0 ? logits0 : nullptr;
    lp.step0_flags = i0 == 0 && from_start ? h->step0_flags : nullptr;
    ldm_handle::Scope sc(h, st, "layers_fused_loop", n * step_flops, (double)B * h->plan.S * 8);
    launch_stack_loop(sw.ls, F, D, B, h->plan.S, h->H, h->plan.dh, sw.head, lp, st);
  }
  return 0;
}

// clears the rows a deterministic call is about to fill
static int tie_begin(ldm_handle* h, const ldm_sampler* s, const ldm_relation* rel, int n_steps, int B, hipStream_t st) {
  (void)B;
  if (!(h->tie_rel > 0.f) || !h->tie_flags || s->kind != LDM_SAMPLE_DETERMINISTIC) return 0;
  // the adjusted steps of cond=relation draw from the SGD's output, where the lead of the winner is no longer a
  // function of the logits with a known Lipschitz bound: no report exists for them, so none may be assumed
  if (rel) return h->fail(-1, "near-tie report is not defined for cond=relation: decode in LDM_PREC_EXACT_F32 instead");
  if (n_steps > h->tie_steps) return h->fail(-1, "near-tie report: at most %d steps per call", h->tie_steps);
  HIP_OK(h, hipMemsetAsync(h->tie_flags, 0, (size_t)n_steps * h->cfg.max_batch, st));
  return 0;
}

// ------------------------------------------------------------------------------------------ hot path
extern "C" int ldm_sample_step(ldm_handle* h, const int32_t* d_tokens_in, int32_t* d_tokens_out, int t_model,
                               int t_post, const ldm_cond* cond, const ldm_relation* rel, const ldm_sampler* s,
                               uint64_t seed, uint64_t first_layout, int step, int B, void* stream) {
  int rc = check_call(h, s, B);
  if (rc) return rc;
  if (!d_tokens_in || !d_tokens_out) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  if ((rc = check_relation(h, rel, cond, B))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = set_rng(h, seed, first_layout, st))) return rc;
  const int32_t tm = t_model, tp = t_post;
  if ((rc = check_timestep_range(h, &tm, &tp, 1))) return rc;
  if ((rc = tie_begin(h, s, rel, 1, B, st))) return rc;
  if (loop_fusable(h, rel)) {
    if ((rc = run_loop_fused(h, d_tokens_in, d_tokens_out, cond, rel, &tm, &tp, 1, s, step, B, nullptr, 0, st))) return rc;
  } else if ((rc = step_all(h, h->ws[0], d_tokens_in, d_tokens_out, t_model, t_post, cond, rel, 0, s, step, B, 0, st, false, false, 0)))
    return rc;
  HIP_OK(h, hipGetLastError());
  return 0;
}

// The T-step loop of the passes of ONE lane of the cut (lane < 0: every pass, in order, through lane 0's workspace).
static int run_loop_body(ldm_handle* h, const LoopCut& cut, const ldm_cond* cond, const ldm_relation* rel, const int32_t* t_model,
                         const int32_t* t_post, int n_steps, const ldm_sampler* s, int32_t* d_inter, int lane, hipStream_t st) {
  // state lives in tok_a / tok_b (ping-pong); chunk-major order keeps one chunk's activations and the weights resident in L2 / Infinity Cache for all T steps
  const size_t S = h->plan.S;
  Workspace& ws = h->ws[lane < 0 ? 0 : lane];
  for (int k = 0; k < cut.n_pass; ++k) {
    if (!cut.owns(lane, k)) continue;
    const int off = cut.offset(k), Bc = cut.size(k);
    ldm_cond cc{};
    if (cond) {
      cc = *cond;
      if (cc.d_cond_seq) cc.d_cond_seq += off * S;
      if (cc.d_strong_mask) cc.d_strong_mask += off * S;
      if (cc.d_weak_logits) cc.d_weak_logits += (size_t)off * h->plan.C * S;
    }
    int32_t *cur = h->tok_a + off * S, *nxt = h->tok_b + off * S;
    // the stack kernel takes raw rows and computes its own row statistics, so the posterior kernel of step i can write
    // step i + 1's embedding itself (no separate embedding launch inside the loop)
    const bool fuse_embed = h->plan.structure == Structure::Stack;
    for (int i = 0; i < n_steps; ++i) {
      int rc = step_all(h, ws, cur, nxt, t_model[i], t_post[i], cond ? &cc : nullptr, rel, off, s, i, Bc, off, st,
                        fuse_embed && i > 0, fuse_embed && i + 1 < n_steps, i);
      if (rc) return rc;
      if (d_inter)
        HIP_OK(h, hipMemcpyAsync(d_inter + ((size_t)i * cut.B + off) * S, nxt, (size_t)Bc * S * 4, hipMemcpyDeviceToDevice, st));
      std::swap(cur, nxt);
    }
    if (n_steps % 2 == 1)  // result sits in tok_b: bring it back to tok_a
      HIP_OK(h, hipMemcpyAsync(h->tok_a + off * S, h->tok_b + off * S, (size_t)Bc * S * 4, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// ---- the per-lane hipGraph loop, step by step
// A captured graph only ever sees fixed addresses: the caller's constraints are copied into handle-owned staging buffers, so
// the graph is reused across batches whose cond tensors live elsewhere.  *staged describes the copies.
static int stage_cond(ldm_handle* h, const ldm_cond* cond, int B, hipStream_t st, ldm_cond* staged) {
  const size_t nS = (size_t)B * h->plan.S;
  staged->pad_disable = cond->pad_disable;
  if (cond->d_cond_seq) {
    HIP_OK(h, hipMemcpyAsync(h->st_cond_seq, cond->d_cond_seq, nS * 4, hipMemcpyDeviceToDevice, st));
    staged->d_cond_seq = h->st_cond_seq;
  }
  if (cond->d_strong_mask) {
    HIP_OK(h, hipMemcpyAsync(h->st_strong, cond->d_strong_mask, nS, hipMemcpyDeviceToDevice, st));
    staged->d_strong_mask = h->st_strong;
  }
  if (cond->d_weak_logits) {
    int rc = 0;
    if (!h->st_weak && (rc = h->dalloc(&h->st_weak, (size_t)h->cfg.max_batch * h->plan.C * h->plan.S, false))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->st_weak, cond->d_weak_logits, nS * h->plan.C * 4, hipMemcpyDeviceToDevice, st));
    staged->d_weak_logits = h->st_weak;
  }
  return 0;
}

// Room for n_edges edges in the relation edge staging.  A grown buffer has a new address: graphs keyed on the old one can never
// hit again — drop them and release the old buffer, once NOTHING on the device can still be reading it (an earlier replay may
// run on another stream than the one the caller synchronised).
static int grow_rel_edges(ldm_handle* h, size_t n_edges) {
  if (n_edges <= h->st_rel_cap) return 0;
  int32_t* old = h->st_rel_edges;
  if (old) HIP_OK(h, hipDeviceSynchronize());
  const size_t cap = std::max<size_t>(1024, n_edges * 2);
  int rc = h->dalloc(&h->st_rel_edges, 3 * cap);
  if (rc) return rc;
  h->st_rel_cap = cap;
  if (old) {
    h->graphs.drop_where_rel_edges(old);
    h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), (void*)old), h->owned.end());
    (void)hipFree(old);
  }
  return 0;
}

// ... and the relation graph: CSR offsets are read back once (host) to size the edge staging
static int stage_relation(ldm_handle* h, const ldm_relation* rel, int B, hipStream_t st, ldm_relation* staged) {
  int rc = 0;
  *staged = *rel;
  std::vector<int32_t> off(B + 1);
  HIP_OK(h, hipMemcpyAsync(off.data(), rel->d_edge_offsets, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(h, hipStreamSynchronize(st));
  const int32_t e0 = off[0], ne = off[B] - off[0];
  if (ne < 0) return h->fail(-1, "ldm_relation: edge offsets are not monotonic");
  if (!h->st_rel_off && (rc = h->dalloc(&h->st_rel_off, (size_t)h->cfg.max_batch + 1))) return rc;
  if (!h->st_rel_centres && (rc = h->dalloc(&h->st_rel_centres, (size_t)4 * h->cfg.n_bin))) return rc;
  if ((rc = grow_rel_edges(h, (size_t)ne))) return rc;
  for (auto& o : off) o -= e0;
  HIP_OK(h, hipMemcpyAsync(h->st_rel_off, off.data(), (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  HIP_OK(h, hipStreamSynchronize(st));  // `off` is pageable host memory
  const size_t cap = h->st_rel_cap;
  if (ne > 0) {
    HIP_OK(h, hipMemcpyAsync(h->st_rel_edges, rel->d_edge_src + e0, (size_t)ne * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->st_rel_edges + cap, rel->d_edge_dst + e0, (size_t)ne * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->st_rel_edges + 2 * cap, rel->d_edge_attr + e0, (size_t)ne * 4, hipMemcpyDeviceToDevice, st));
  }
  HIP_OK(h, hipMemcpyAsync(h->st_rel_centres, rel->d_centres, (size_t)4 * h->cfg.n_bin * 4, hipMemcpyDeviceToDevice, st));
  staged->d_edge_offsets = h->st_rel_off;
  staged->d_edge_src = h->st_rel_edges;
  staged->d_edge_dst = h->st_rel_edges + cap;
  staged->d_edge_attr = h->st_rel_edges + 2 * cap;
  staged->d_centres = h->st_rel_centres;
  return 0;
}

// intermediates are captured into a handle-owned buffer (fixed address) and copied out after the launch, so
// get_intermediate_results=True replays the same graph instead of re-capturing for every caller pointer
static int stage_intermediates(ldm_handle* h, int n_steps, int32_t** inter_dst) {
  if (n_steps > h->T) return h->fail(-1, "intermediates: n_steps %d > T %d", n_steps, h->T);
  int rc = 0;
  if (!h->st_inter && (rc = h->dalloc(&h->st_inter, (size_t)h->T * h->cfg.max_batch * h->plan.S, false))) return rc;
  *inter_dst = h->st_inter;
  return 0;
}

// One linear graph per lane of the cut into *entry, each captured on a private stream so that the caller's stream state is
// untouched.  Whatever ends the function early, the guard ends an open capture (discarding its graph), destroys the private
// stream and destroys the graphs *entry holds so far: nothing between begin and end of a capture returns past it.
static int capture_lanes(ldm_handle* h, const LoopCut& cut, const GraphKey& key, const ldm_cond* cond, const ldm_relation* rel,
                         const int32_t* t_model, const int32_t* t_post, int n_steps, const ldm_sampler* s, int32_t* inter_dst,
                         GraphEntry* entry) {
  struct Guard {
    GraphEntry* entry;
    hipStream_t cap = nullptr;
    bool capturing = false, done = false;
    hipError_t end_capture(hipGraph_t* graph) {   // ... and the private stream with it
      const hipError_t e = capturing ? hipStreamEndCapture(cap, graph) : hipSuccess;
      capturing = false;
      if (cap) (void)hipStreamDestroy(cap);
      cap = nullptr;
      return e;
    }
    ~Guard() {
      hipGraph_t graph = nullptr;
      (void)end_capture(&graph);
      if (graph) (void)hipGraphDestroy(graph);
      if (!done) entry->destroy();
    }
  } guard{entry};
  entry->key = key;
  for (int lane = 0; lane < cut.lanes; ++lane) {
    HIP_OK(h, hipStreamCreateWithFlags(&guard.cap, hipStreamNonBlocking));
    HIP_OK(h, hipStreamBeginCapture(guard.cap, hipStreamCaptureModeThreadLocal));
    guard.capturing = true;
    if (lane > 0 && h->plan.lane_offset_us > 0) launch_delay_us(lane * h->plan.lane_offset_us, guard.cap);
    const int rc = run_loop_body(h, cut, cond, rel, t_model, t_post, n_steps, s, inter_dst, cut.lanes > 1 ? lane : -1, guard.cap);
    hipGraph_t graph = nullptr;
    hipError_t e = guard.end_capture(&graph);
    if (graph) entry->graph.push_back(graph);   // the entry's from here on
    if (rc) return rc;
    if (e != hipSuccess) return h->fail(-2, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) return h->fail(-2, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    entry->exec.push_back(exec);
  }
  guard.done = true;
  return 0;
}

// lane 0 replays on the caller's stream, the others on their own streams between a fork and a join event
static int replay(ldm_handle* h, const GraphEntry& ge, hipStream_t st) {
  if (ge.exec.size() > 1) HIP_OK(h, hipEventRecord(h->fork_ev, st));
  for (size_t lane = 1; lane < ge.exec.size(); ++lane) {
    HIP_OK(h, hipStreamWaitEvent(h->lane_stream[lane], h->fork_ev, 0));
    HIP_OK(h, hipGraphLaunch(ge.exec[lane], h->lane_stream[lane]));
    HIP_OK(h, hipEventRecord(h->lane_done[lane], h->lane_stream[lane]));
  }
  HIP_OK(h, hipGraphLaunch(ge.exec[0], st));
  for (size_t lane = 1; lane < ge.exec.size(); ++lane) HIP_OK(h, hipStreamWaitEvent(st, h->lane_done[lane], 0));
  return 0;
}

extern "C" int ldm_sample_loop(ldm_handle* h, int32_t* d_tokens_inout, const ldm_cond* cond, const ldm_relation* rel,
                               const int32_t* h_t_model, const int32_t* h_t_post, int n_steps, const ldm_sampler* s,
                               uint64_t seed, uint64_t first_layout, int B, int32_t* d_intermediates, int use_graph,
                               void* stream) {
  int rc = check_call(h, s, B);
  if (rc) return rc;
  if (!d_tokens_inout || !h_t_model || !h_t_post || n_steps < 1) return h->fail(-1, "bad argument");
  if ((rc = check_timestep_range(h, h_t_model, h_t_post, n_steps))) return rc;
  ON_DEVICE(h);
  if ((rc = check_relation(h, rel, cond, B))) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t nbytes = (size_t)B * h->plan.S * 4;
  HIP_OK(h, hipEventRecord(h->loop_a, st));
  if ((rc = set_rng(h, seed, first_layout, st))) return rc;
  if ((rc = tie_begin(h, s, rel, n_steps, B, st))) return rc;
  if (loop_fusable(h, rel)) {
    // one launch: every layout's workgroup runs all its steps in place on the caller's tokens (no staging, no graph)
    if ((rc = run_loop_fused(h, d_tokens_inout, d_tokens_inout, cond, rel, h_t_model, h_t_post, n_steps, s, 0, B, d_intermediates, 0, st, true))) return rc;
  } else {
    const LoopCut cut = cut_call(B, h->plan.chunk, h->plan.n_lanes, h->plan.balanced_chunks);
    HIP_OK(h, hipMemcpyAsync(h->tok_a, d_tokens_inout, nbytes, hipMemcpyDeviceToDevice, st));
    if (use_graph && !h->profiling) {
      ldm_cond staged{};
      ldm_relation staged_rel{};
      int32_t* inter_dst = nullptr;
      if (cond && (rc = stage_cond(h, cond, B, st, &staged))) return rc;
      if (rel && (rc = stage_relation(h, rel, B, st, &staged_rel))) return rc;
      if (d_intermediates && (rc = stage_intermediates(h, n_steps, &inter_dst))) return rc;
      if (cond) cond = &staged;
      if (rel) rel = &staged_rel;
      const GraphKey key = graph_key(B, n_steps, *s, cond, inter_dst != nullptr, h->tie_flags != nullptr, h->tie_rel, h->tie_abs, rel,
                                     h_t_model, h_t_post);
      const GraphEntry* ge = h->graphs.find(key);
      if (!ge) {
        GraphEntry captured;
        if ((rc = capture_lanes(h, cut, key, cond, rel, h_t_model, h_t_post, n_steps, s, inter_dst, &captured))) return rc;
        ge = h->graphs.insert(captured);
      }
      if ((rc = replay(h, *ge, st))) return rc;
      if (inter_dst)
        HIP_OK(h, hipMemcpyAsync(d_intermediates, inter_dst, (size_t)n_steps * B * h->plan.S * 4, hipMemcpyDeviceToDevice, st));
    } else if ((rc = run_loop_body(h, cut, cond, rel, h_t_model, h_t_post, n_steps, s, d_intermediates, -1, st)))
      return rc;
    HIP_OK(h, hipMemcpyAsync(d_tokens_inout, h->tok_a, nbytes, hipMemcpyDeviceToDevice, st));
  }
  HIP_OK(h, hipEventRecord(h->loop_b, st));
  h->loop_timed = true;
  HIP_OK(h, hipGetLastError());
  return 0;
}
