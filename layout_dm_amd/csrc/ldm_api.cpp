// Host side of libldm_hip.so: the C-ABI declared in include/ldm_hip.h — lifecycle, parity hooks, result packaging, near-tie
// report, introspection.  (Weights: ldm_weights.cpp; one denoiser pass: ldm_denoise.cpp; the hot path: ldm_loop.cpp.)
// No torch types cross this boundary.
#include "ldm_handle.h"

using namespace ldm_host;

std::string& ldm_host::create_error() {
  static thread_local std::string e;
  return e;
}

// ------------------------------------------------------------------------------------------ create
extern "C" int ldm_abi_version(void) { return LDM_ABI_VERSION; }

extern "C" int ldm_get_layout(const ldm_handle* h, int* chunk, int* lanes) {
  if (!h) return -1;
  if (chunk) *chunk = h->plan.chunk;
  if (lanes) *lanes = h->plan.n_lanes;
  return 0;
}

extern "C" const char* ldm_last_error(const ldm_handle* h) { return h ? h->err.c_str() : create_error().c_str(); }

// validate -> probe the device -> plan (ldm_engine_plan.h: everything that depends on the configuration and the knobs alone) -> allocate what the
// plan counts -> streams and events
extern "C" int ldm_create(const ldm_config* cfg, int device, ldm_handle** out) { return ldm_create_variant(cfg, LDM_NORM1_LAYER, device, out); }

extern "C" int ldm_create_variant(const ldm_config* cfg, int norm1_kind, int device, ldm_handle** out) {
  auto bad = [&](const std::string& msg) {
    create_error() = msg;
    return -1;
  };
  if (!cfg || !out) return bad("null argument");
  std::string why;
  if (validate_config(*cfg, knob_refused(), why)) return bad(why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return bad("no HIP device visible: the MI355X path has no CPU fallback");
  if (device < 0 || device >= ndev) return bad("device index out of range");
  DeviceGuard create_guard(device);
  if (create_guard.err != hipSuccess) return bad("hipSetDevice failed");
  // The create-time knobs (ldm_knobs.h: honoured in dev mode only; what was read is what ldm_describe reports as honoured).  A knob is read
  // only where the plan made without it shows that it can take effect — the geometry has the kernels it switches off — so the plan is made
  // again behind each group; plan_engine itself never sees the environment.
  Knobs kn;
  EnginePlan plan;
  int refused = plan_engine(*cfg, kn, plan, why, norm1_kind);
  if (plan.chunk) {   // (decided as far as the chunk: every refusal but an unknown q_type)
    kn.chunk = knob_int("LDM_CHUNK", Knobs::kUnset);
    kn.balanced_chunks = knob_int("LDM_BALANCED_CHUNKS", Knobs::kUnset);
    kn.lanes = knob_int("LDM_LANES", Knobs::kUnset);
    kn.lane_offset_us = knob_int("LDM_LANE_OFFSET_US", Knobs::kUnset);
    if (plan.fast()) {
      kn.stack_kernel = knob_int("LDM_FUSED_ATTN", Knobs::kUnset);
      kn.stack_loop = knob_int("LDM_STACK_LOOP", Knobs::kUnset);
      kn.rel_loop = knob_int("LDM_REL_LOOP", Knobs::kUnset);
      kn.step0_cache = knob_int("LDM_STEP0_CACHE", Knobs::kUnset);
    }
    if (plan.structure == Structure::RowResident) kn.x3_lngemm = knob_int("LDM_X3_LNGEMM", Knobs::kUnset);
    refused = plan_engine(*cfg, kn, plan, why, norm1_kind);
    if (plan.hid_panels) kn.x3_hidpanel = knob_int("LDM_X3_HIDPANEL", Knobs::kUnset);
    if (plan.attnout) kn.x3_attnout = knob_int("LDM_X3_ATTNOUT", Knobs::kUnset);
    refused = plan_engine(*cfg, kn, plan, why, norm1_kind);
    if (plan.ffn_fused) kn.hyb_ffn = knob_int("LDM_HYB_FFN", Knobs::kUnset);
    refused = plan_engine(*cfg, kn, plan, why, norm1_kind);
  }
  if (refused) {
    create_error() = why;
    return refused;
  }

  auto* h = new ldm_handle();
  h->cfg = *cfg;
  h->plan = plan;
  h->device = device;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) h->n_cu = ncu;
  }
  h->D = cfg->d_model;
  h->F = cfg->d_ff;
  h->H = cfg->n_head;
  h->L = cfg->n_layer;
  h->T = cfg->n_step;
  // vocabulary geometry: helpers/layout_tokenizer.py:79-82,429-467
  h->vocab.n_class = plan.C;
  h->vocab.n_attr = cfg->n_attr;
  h->vocab.pad_id = plan.C - 2;
  h->vocab.mask_id = plan.C - 1;
  for (int a = 0; a < cfg->n_attr; ++a) {
    if (cfg->q_type == LDM_Q_VANILLA) {  // one vocabulary: every class is live at every position (vanilla.py)
      h->vocab.start[a] = 0;
      h->vocab.count[a] = plan.C - 2;
    } else {
      h->vocab.start[a] = (a == 0) ? 0 : cfg->n_category + (a - 1) * cfg->n_bin;
      h->vocab.count[a] = (a == 0) ? cfg->n_category : cfg->n_bin;
    }
  }
  int rc = 0;
  auto A = [&](auto** p, size_t n) {
    if (rc == 0 && n) rc = h->dalloc(p, n);
  };
  h->ws.resize(plan.n_lanes);
  for (Workspace& ws : h->ws) {   // one workspace per lane (ldm_handle.h Workspace)
    const WorkspaceCounts& n = plan.ws;
    A(&ws.P, n.P); A(&ws.Q, n.Q); A(&ws.logits, n.logits);
    A(&ws.qkv32, n.qkv32); A(&ws.att32, n.att32); A(&ws.h32, n.h32); A(&ws.hid32, n.hid32);
    A(&ws.a16, n.a16); A(&ws.att16, n.att16); A(&ws.h16, n.h16); A(&ws.hid16, n.hid16); A(&ws.qkv16, n.qkv16);
    A(&ws.a16lo, n.a16lo); A(&ws.att16lo, n.att16lo); A(&ws.h16lo, n.h16lo); A(&ws.hid16lo, n.hid16lo);
    A(&ws.qkvp_hi, n.qkvp_hi); A(&ws.qkvp_lo, n.qkvp_lo);
    A(&ws.stats_a, n.stats_a);
  }
  const HandleCounts& n = plan.bufs;
  A(&h->tok_a, n.tok_a); A(&h->tok_b, n.tok_b);
  A(&h->st_cond_seq, n.st_cond_seq); A(&h->st_strong, n.st_strong);
  A(&h->rng, n.rng);
  A(&h->sched, n.sched);
  A(&h->step0_tab, n.step0_tab); A(&h->step0_tok, n.step0_tok); A(&h->step0_flags, n.step0_flags);   // step-0 logits cache of the one-launch loop (ldm_handle.h)
  if (rc != 0) {
    create_error() = h->err;
    ldm_destroy(h);
    return rc;
  }
  if (h->step0_tok) {
    const std::vector<int32_t> row((size_t)plan.S, h->vocab.mask_id);
    if (hipMemcpy(h->step0_tok, row.data(), row.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      create_error() = "hipMemcpy of the all-[MASK] row failed";
      ldm_destroy(h);
      return -2;
    }
  }
  if (hipEventCreate(&h->loop_a) != hipSuccess || hipEventCreate(&h->loop_b) != hipSuccess ||
      hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) != hipSuccess) {
    create_error() = "event creation failed";
    ldm_destroy(h);
    return -2;
  }
  h->lane_stream.assign(plan.n_lanes, nullptr);
  h->lane_done.assign(plan.n_lanes, nullptr);
  for (int l = 1; l < plan.n_lanes; ++l) {
    if (hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->lane_done[l], hipEventDisableTiming) != hipSuccess) {
      create_error() = "lane stream / event creation failed";
      ldm_destroy(h);
      return -2;
    }
  }
  *out = h;
  return 0;
}

extern "C" void ldm_destroy(ldm_handle* h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  (void)hipDeviceSynchronize();
  h->drain_profile();
  h->graphs.drop_all();
  for (auto& kv : h->raw)
    if (kv.second.d) (void)hipFree(kv.second.d);
  for (void* p : h->owned) (void)hipFree(p);
  for (void* p : h->derived) (void)hipFree(p);
  if (h->loop_a) (void)hipEventDestroy(h->loop_a);
  if (h->loop_b) (void)hipEventDestroy(h->loop_b);
  if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
  for (auto ev : h->step0_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto st : h->lane_stream)
    if (st) (void)hipStreamDestroy(st);
  for (auto ev : h->lane_done)
    if (ev) (void)hipEventDestroy(ev);
  delete h;
}

// ------------------------------------------------------------------------------------------ parity hooks
// Per-layout timesteps of a call: checked on the host, copied to a pageable array of the handle's (an upload from pageable memory has
// read its source when it returns, so neither the caller's array nor a following call's copy can race it) and uploaded on `st`.
int ldm_host::stage_timesteps(ldm_handle* h, const int32_t* h_t, int B, hipStream_t st, const int32_t** d_t) {
  if (!h_t) return h->fail(-1, "null argument");
  if (!h->plan.per_layout_t())
    return h->fail(-4, "per-layout timesteps: precision fast_f16 on the stack kernel has no per-layout form (ldm_describe per_layout_t=0)");
  for (int b = 0; b < B; ++b)
    if (h_t[b] < 0 || h_t[b] >= h->T) return h->fail(-1, "timestep %d of layout %d out of range [0,%d)", h_t[b], b, h->T);  // constrained.py:139
  if (!h->st_t) {
    int rc = h->dalloc(&h->st_t, (size_t)h->cfg.max_batch);
    if (rc) return rc;
    h->st_t_host.resize((size_t)h->cfg.max_batch);
  }
  std::copy(h_t, h_t + B, h->st_t_host.begin());
  HIP_OK(h, hipMemcpyAsync(h->st_t, h->st_t_host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  *d_t = h->st_t;
  return 0;
}

// the denoiser's logits of B layouts, chunk by chunk through ws[0]: every layout at timestep t, or (h_t) each at its own
static int denoise_logits(ldm_handle* h, const int32_t* d_tokens, int t, const int32_t* h_t, bool per_layout, int B, float* d_logits, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_tokens || !d_logits) return h->fail(-1, "null argument");
  if (!per_layout && (t < 0 || t >= h->T)) return h->fail(-1, "timestep out of range");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  const int32_t* d_t = nullptr;
  if (per_layout && (rc = stage_timesteps(h, h_t, B, st, &d_t))) return rc;
  Workspace& ws = h->ws[0];
  for (int off = 0; off < B; off += h->plan.chunk) {
    const int Bc = std::min(h->plan.chunk, B - off);
    if ((rc = denoise_chunk(h, ws, d_tokens + (size_t)off * h->plan.S, t, Bc, st, false, d_t ? d_t + off : nullptr))) return rc;
    HIP_OK(h, hipMemcpy2DAsync(d_logits + (size_t)off * h->plan.S * h->plan.C, (size_t)h->plan.C * 4, ws.logits, (size_t)h->plan.Cp * 4,
                               (size_t)h->plan.C * 4, (size_t)Bc * h->plan.S, hipMemcpyDeviceToDevice, st));
  }
  HIP_OK(h, hipGetLastError());
  return 0;
}
extern "C" int ldm_denoise_logits(ldm_handle* h, const int32_t* d_tokens, int t, int B, float* d_logits, void* stream) {
  return denoise_logits(h, d_tokens, t, nullptr, false, B, d_logits, stream);
}
extern "C" int ldm_denoise_logits_t(ldm_handle* h, const int32_t* d_tokens, const int32_t* h_t, int B, float* d_logits, void* stream) {
  return denoise_logits(h, d_tokens, 0, h_t, true, B, d_logits, stream);
}

extern "C" int ldm_posterior(ldm_handle* h, const float* d_logits, const int32_t* d_tokens, int t_post, int B,
                             const ldm_cond* cond, float* d_logp, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_logits || !d_tokens || !d_logp) return h->fail(-1, "null argument");
  if (t_post < 0 || t_post >= h->T) return h->fail(-1, "timestep out of range");
  ON_DEVICE(h);
  PostArgs p{};
  fill_post(h, p, cond, nullptr, 0, B);
  p.logits = d_logits;
  p.ldl = h->plan.C;
  p.tokens = d_tokens;
  p.logp_out = d_logp;
  p.t_post = t_post;
  launch_posterior_sample(p, (hipStream_t)stream);
  HIP_OK(h, hipGetLastError());
  return 0;
}

int ldm_host::set_rng(ldm_handle* h, uint64_t seed, uint64_t first_layout, hipStream_t st) {
  launch_set_rng(h->rng, seed, first_layout, st);  // kernel args are captured by value at launch
  return 0;
}

extern "C" int ldm_sample_tokens(ldm_handle* h, const float* d_logp, const ldm_cond* cond, const ldm_sampler* s,
                                 uint64_t seed, uint64_t first_layout, int step, int B, int32_t* d_tokens_out,
                                 void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if ((rc = check_sampler(h, s))) return rc;
  if (!d_logp || !d_tokens_out) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = set_rng(h, seed, first_layout, st))) return rc;
  PostArgs p{};
  fill_post(h, p, nullptr, s, 0, B);
  if (cond) {  // only the [PAD] disabling applies at this stage (base.py:272-284)
    p.cond_seq = cond->d_cond_seq;
    p.pad_disable = cond->pad_disable;
  }
  p.logp_in = d_logp;
  p.tokens_out = d_tokens_out;
  p.step = step;
  launch_posterior_sample(p, st);
  HIP_OK(h, hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ relation
extern "C" int ldm_relation_update(ldm_handle* h, float* d_logp_inout, const int32_t* d_cond_seq,
                                   const ldm_relation* rel, int t, int B, void* stream) {
  if (!h) return -1;
  if (B <= 0) return B == 0 ? 0 : h->fail(-1, "negative batch");
  if (!d_logp_inout || !d_cond_seq || !rel) return h->fail(-1, "null argument");
  if (!rel->d_edge_offsets || !rel->d_centres) return h->fail(-1, "ldm_relation: null edge offsets / centres");
  if (rel->n_graph_total < B) return h->fail(-1, "ldm_relation.n_graph_total smaller than B");
  if (h->cfg.max_elem > 32 || h->cfg.n_bin > 32) return h->fail(-4, "relation kernel: max_elem and n_bin must be <= 32");
  for (int x = 0; x < 4; ++x)
    if (rel->canvas_bins[x] < 0 || rel->canvas_bins[x] >= h->cfg.n_bin) return h->fail(-1, "canvas bin out of range");
  if (t < 10 || rel->num_update <= 0) return 0;  // logit_adjustment.py:107
  ON_DEVICE(h);
  RelArgs a{};
  a.logp = d_logp_inout;
  a.cond_seq = d_cond_seq;
  fill_rel(h, a, rel, 0, B);
  launch_relation_update(a, (hipStream_t)stream);
  HIP_OK(h, hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ decode
extern "C" int ldm_decode_layouts(ldm_handle* h, const int32_t* d_tokens, int B, const double* d_centres, int box_f64,
                                  void* d_bbox, int64_t* d_label, uint8_t* d_mask, void* stream) {
  if (!h) return -1;
  if (B < 0) return h->fail(-1, "negative batch");
  if (B == 0) return 0;
  if (!d_tokens || !d_bbox || !d_label || !d_mask) return h->fail(-1, "null argument");
  ON_DEVICE(h);  // (n_attr == 5, i.e. c-x-y-w-h, is enforced by ldm_create)
  launch_decode_layouts(d_tokens, B, h->cfg.max_elem, h->cfg.n_attr, h->cfg.n_category, h->cfg.n_bin, d_centres,
                        box_f64, d_bbox, d_label, d_mask, (hipStream_t)stream);
  HIP_OK(h, hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ near-tie report
// Deterministic decoding in the fp16 mode is bit-exact against the reference wherever the winning class leads the
// runner-up by more than the mode's logits error can move.  With the report enabled every deterministic step marks
// the layouts in which some token was decided inside that band; the caller re-decides exactly those in the exact
// mode (layout_dm_amd.verified: greedy decoding is RNG-free and layouts are independent).
extern "C" int ldm_set_tie_report(ldm_handle* h, float tie_rel, float tie_abs) {
  if (!h) return -1;
  if (!(tie_rel >= 0.f) || !(tie_abs >= 0.f)) return h->fail(-1, "tie_rel / tie_abs must be >= 0");
  if (tie_abs > 0.f && !(tie_rel > 0.f)) tie_rel = 1e-30f;  // (the report is keyed on tie_rel > 0)
  ON_DEVICE(h);
  if (tie_rel > 0.f && !h->tie_flags) {
    h->tie_steps = std::max(h->T, 1);
    int rc = h->dalloc(&h->tie_flags, (size_t)h->tie_steps * h->cfg.max_batch);
    if (rc) return rc;
  }
  if ((tie_rel != h->tie_rel || tie_abs != h->tie_abs) && !h->graphs.empty()) {
    // captured graphs carry the flag pointers / thresholds of their capture; a replay on another stream may still be
    // executing one of them
    HIP_OK(h, hipDeviceSynchronize());
    h->graphs.drop_all();
  }
  h->tie_rel = tie_rel;
  h->tie_abs = tie_abs;
  return 0;
}
extern "C" int ldm_get_tie_flags(ldm_handle* h, uint8_t* d_flags, int n_steps, int B, void* stream) {
  if (!h || !d_flags) return h ? h->fail(-1, "null argument") : -1;
  if (!h->tie_flags) return h->fail(-1, "near-tie report not enabled (ldm_set_tie_report)");
  if (n_steps < 1 || n_steps > h->tie_steps || B < 1 || B > h->cfg.max_batch) return h->fail(-1, "n_steps / B out of range");
  ON_DEVICE(h);
  HIP_OK(h, hipMemcpy2DAsync(d_flags, (size_t)B, h->tie_flags, (size_t)h->cfg.max_batch, (size_t)B, (size_t)n_steps,
                             hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}
// ------------------------------------------------------------------------------------------ introspection
// "key=value;..." description of what this handle runs: numerics mode, kernel family, chunk / lanes, near-tie thresholds,
// the batch-shape rule of the one-launch loop (one workgroup per layout on the chip's compute units: a call costs whole
// rounds of `round` layouts, so B = round + 1 costs what B = 2 * round costs) and the development knobs the library has
// honoured in this process (ldm_knobs.h; always the LAST key: its value may itself contain ';').  Returns the length
// needed (excluding the terminator), whatever `cap` is: call again with a larger buffer when the result is >= cap.
#ifndef LDM_SRC_DIGEST
#define LDM_SRC_DIGEST "unknown"
#endif
// sha256 over the sources this library was built from (layout_dm_amd/build.py source_digest(), passed at compile time): the
// marker is what build.py / the tests scan a built .so for — a pushed tree whose prebuilt library lags its sources is rebuilt
// (or refused), not silently used
extern "C" const char ldm_build_source_digest[] = "LDM_SRC_DIGEST=" LDM_SRC_DIGEST;

extern "C" int ldm_describe(const ldm_handle* h, char* buf, int cap) {
  if (!h) return -1;
  const bool loop = loop_fusable(h, nullptr);
  char num[96];
  std::string s = "abi=" + std::to_string(LDM_ABI_VERSION) + ";precision=" + h->plan.describe_precision() + ";kernels=" + h->plan.describe_kernels();
  s += std::string(";loop=") + (loop ? "one_launch" : "per_step_graph");
  s += ";chunk=" + std::to_string(h->plan.chunk) + ";lanes=" + std::to_string(h->plan.n_lanes) + ";lane_offset_us=" + std::to_string(h->plan.lane_offset_us);
  snprintf(num, sizeof(num), ";tie_rel=%g;tie_abs=%g", (double)h->tie_rel, (double)h->tie_abs);
  s += num;
  // batch quantum: the loop kernel runs one workgroup per layout, one workgroup per compute unit; the per-step path runs
  // `chunk` layouts per pass on `lanes` concurrent pipelines
  s += ";round=" + std::to_string(loop ? h->n_cu : h->plan.chunk * std::max(h->plan.n_lanes, 1));
  s += std::string(";batch_rule=") + (loop ? "whole_rounds_of_one_workgroup_per_layout" : "whole_chunks");
  s += std::string(";src_digest=") + (ldm_build_source_digest + sizeof("LDM_SRC_DIGEST=") - 1);
  // step-0 logits cache of the one-launch loop: on / off, and the (first timestep : S) keys it holds, oldest first
  s += std::string(";step0_cache=") + (loop && h->plan.step0_cache && h->step0_tab ? "on" : "off") + ";step0_entries=";
  for (size_t i = 0; i < h->step0.size(); ++i)
    s += (i ? "," : "") + std::to_string(h->step0[i].t) + ":" + std::to_string(h->step0[i].S);
  // the denoiser takes per-layout timesteps (ldm_denoise_logits_t, ldm_vb_step_t): every engine but fast_f16 on the stack kernel
  s += std::string(";per_layout_t=") + (h->plan.per_layout_t() ? "1" : "0");
  // the denoiser variant, named only where it is not the default (elem_attr positions, adalayernorm): ldm_create_variant's norm1 kind and what
  // ldm_finalize_weights read from the checkpoint's key set
  if (h->plan.instance_norm) s += ";norm1=instance";
  if (h->wplan.pos_default) s += ";pos_emb=default";
  if (h->wplan.timestep_kind != kTimestepLearned) s += std::string(";timestep_emb=") + (h->wplan.timestep_kind == kTimestepAbs ? "abs" : "none");
  s += ";knobs=" + knobs_honoured();
  if (buf && cap > 0) {
    const size_t n = std::min((size_t)cap - 1, s.size());
    memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int)s.size();
}

extern "C" int ldm_last_loop_ms(ldm_handle* h, float* ms) {
  if (!h || !ms) return -1;
  if (!h->loop_timed) return h->fail(-1, "no loop has run yet");
  HIP_OK(h, hipEventSynchronize(h->loop_b));
  HIP_OK(h, hipEventElapsedTime(ms, h->loop_a, h->loop_b));
  return 0;
}

extern "C" int ldm_set_profiling(ldm_handle* h, int enable) {
  if (!h) return -1;
  h->drain_profile();
  h->profiling = enable != 0;
  return 0;
}
extern "C" int ldm_profile_count(ldm_handle* h) {
  if (!h) return -1;
  h->drain_profile();
  return (int)h->prof.size();
}
extern "C" int ldm_profile_get(ldm_handle* h, int idx, const char** name, double* total_ms, int64_t* launches,
                               double* flops, double* bytes) {
  if (!h || idx < 0 || idx >= (int)h->prof.size()) return -1;
  h->drain_profile();
  const ProfEntry& e = h->prof[idx];
  if (name) *name = e.name.c_str();
  if (total_ms) *total_ms = e.ms;
  if (launches) *launches = e.launches;
  if (flops) *flops = e.flops;
  if (bytes) *bytes = e.bytes;
  return 0;
}
extern "C" int ldm_profile_reset(ldm_handle* h) {
  if (!h) return -1;
  h->drain_profile();
  h->prof.clear();
  return 0;
}

