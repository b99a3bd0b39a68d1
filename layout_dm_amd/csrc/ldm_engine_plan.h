// What a handle runs, decided in ONE place: plan_engine maps (ldm_config, create-time knob values) to the engine structure, its options,
// the derived geometry and every workspace size — or to the refusal ldm_create reports.  Pure host arithmetic: no HIP, no environment, no
// allocation, so tests/cpu_engine_plan_check.cpp enumerates the geometry -> engine table and the size rules on the CPU.  ldm_create
// allocates what the plan counts; every other host file reads the plan (ldm_handle::plan) and never re-derives a choice from the
// configuration.  The geometry rules the launchers state for themselves (kernels_lngemm.hip, kernels_attnout.hip) live here as well, so
// that the plan and the launch cannot disagree.
#pragma once
#include "../../include/ldm_hip.h"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <string>

namespace ldm {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- sizes the kernels fix (kernels_stack.hip static_asserts the first)
constexpr int kStackStep0Floats = 5 * 16 * 256;   // step-0 logits of one layout: the loop kernel's five head tiles in register order
constexpr int kStackPostMaxLive = 48;             // largest sub-vocabulary (body + [PAD] + [MASK]) the fused tail takes: 3 class slots on each of a group's 16 lanes
constexpr int kStep0Slots = 4;                    // (first timestep, S) keys of the step-0 logits cache
constexpr int kSchedRows = 8;                     // schedule buffers per attribute (ldm_kernels.h ScheduleRow)
// parameter tables of the loop kernel as LDS images, in floats (kernels_stack.hip HEAD == 2)
constexpr int kStackTblAttStatic = 1536;  // in_proj bias [3 * 8 heads * 64]
constexpr int kStackTblAttDyn = 1536;     // 1 + AdaLN scale [512] | shift [512] | b_out + W_out b_v + shift [512]
constexpr int kStackTblFfn = 3584;        // linear1 bias [2048] | norm2 gamma [512] | beta [512] | linear2 bias [512]

// ---- geometry rules shared with the launchers (which add their pointer, stride and alignment checks)
// fused attention + out_proj (kernels_attnout.hip): one 128-row tile per layout, the reference's 8 heads of 58
inline bool attnout16x3_supported(int S, int H, int dh, int D) { return S >= 1 && S <= 128 && H == 8 && dh == 58 && D == 464; }
// one row-resident LayerNorm + GEMM launch (kernels_lngemm.hip): d_model 464 (29 k16-steps), N columns as an even number of 32-column tiles
// within 2048 columns, 4 columns per epilogue access
inline bool lngemm16x3_supported(int D, int N, int n_tiles) {
  return D == 464 && n_tiles >= 2 && !(n_tiles & 1) && n_tiles * 32 <= 2048 && N <= n_tiles * 32 && !(N & 3);
}
inline int x3_tiles(int N) { return ((N + 31) / 32 + 1) & ~1; }   // 32-column tiles of an N-column weight image, rounded up to even

// rows of a q / k / v panel for a chunk of Mc = chunk * S rows: the fused attention kernel reads 128 keys / query rows from a layout's first
// row whatever S is — the last layout of a chunk reaches 128 - S rows past the chunk's last row (the slack was once 8 rows whatever S: at
// S = 50 the last panel was over-read by 8 rows, a memory fault whenever the allocation ended on a page boundary)
inline size_t x3_panel_rows(int Mc, int S) { return (size_t)round_up(Mc + std::max(8, 128 - S), 64); }
// rows of the split-type hidden activations: whole 256-row tiles + 64 (their panel-major form has its rows rounded up to 64)
inline size_t x3_hidden_rows(int Mc) { return (size_t)round_up(Mc, 256) + 64; }

// The four launch sequences of ldm_denoise.cpp
enum class Structure {
  Stack,        // fast on the reference's backbone: all layers + the vocabulary head in one layout-resident launch (kernels_stack.hip)
  Generic16,    // fast, every other accepted geometry: LayerNorm -> gemm16 -> attention16 -> ...
  Tiled,        // exact; split without the row-resident kernels: LayerNorm -> GEMM -> attention -> GEMM -> LayerNorm -> GEMM -> GEMM
  RowResident,  // split / mixed / hybrid on the reference's backbone: LayerNorm-fed GEMMs as row-resident launches (kernels_lngemm.hip)
};

// Create-time knob values (ldm_knobs.h) as ldm_create read them; kUnset = not in the environment, or not in dev mode
struct Knobs {
  static constexpr int kUnset = INT_MIN;
  int chunk = kUnset, lanes = kUnset, lane_offset_us = kUnset, balanced_chunks = kUnset;        // LDM_CHUNK, LDM_LANES, LDM_LANE_OFFSET_US, LDM_BALANCED_CHUNKS
  int stack_kernel = kUnset, stack_loop = kUnset, rel_loop = kUnset, step0_cache = kUnset;        // LDM_FUSED_ATTN, LDM_STACK_LOOP, LDM_REL_LOOP, LDM_STEP0_CACHE
  int x3_lngemm = kUnset, x3_attnout = kUnset, x3_hidpanel = kUnset, hyb_ffn = kUnset;          // LDM_X3_LNGEMM, LDM_X3_ATTNOUT, LDM_X3_HIDPANEL, LDM_HYB_FFN
  std::string refused;   // first knob present although LDM_DEV=1 is not set ("" = none): the create is refused on it
  static bool on(int v) { return v == kUnset || v != 0; }   // the switches default to on
};

// Element counts of a lane's Workspace members (ldm_handle.h), 0 = the engine does not use it
struct WorkspaceCounts {
  size_t P = 0, Q = 0, logits = 0;
  size_t qkv32 = 0, att32 = 0, h32 = 0, hid32 = 0;
  size_t a16 = 0, att16 = 0, h16 = 0, hid16 = 0, qkv16 = 0;
  size_t a16lo = 0, att16lo = 0, h16lo = 0, hid16lo = 0;
  size_t qkvp_hi = 0, qkvp_lo = 0;
  size_t stats_a = 0;
};
// ... and of the handle's own create-time buffers
struct HandleCounts {
  size_t tok_a = 0, tok_b = 0, st_cond_seq = 0, st_strong = 0, rng = 0, sched = 0;
  size_t step0_tab = 0, step0_tok = 0, step0_flags = 0;   // Stack only
};

struct EnginePlan {
  int precision = LDM_PREC_EXACT_F32;   // as the caller requested it
  Structure structure = Structure::Tiled;
  // RowResident options
  bool attnout = false;      // attention + out_proj as ONE layout-resident launch behind an in_proj that writes hi / lo panels (kernels_attnout.hip);
                             // LDM_DEV=1 LDM_X3_ATTNOUT=0: attn16x3_k + the out_proj launch of gemm16x3_k
  bool hid_panels = false;   // hidden activations panel-major between linear1 and the linear2 GEMM prologue; LDM_DEV=1 LDM_X3_HIDPANEL=0: row-major
  bool ffn_fused = false;    // hybrid: linear1 + ReLU + linear2 + residual in plain fp16 behind the attention, in the SAME launch (two launches per
                             // block); LDM_DEV=1 LDM_HYB_FFN=0: linear1 -> plain-fp16 panels -> linear2 as the GEMM prologue of the next launch
  bool w2p = false;          // two-product form of the WEIGHT GEMMs: activations hi + lo, weights fp16 only (mixed / hybrid)
  // products per k16-step (kernels_lngemm.hip NPM / NPP) of the attention path's GEMMs (in_proj; out_proj: w2p) and of linear1 / linear2 / the head:
  // split 3 / 3, mixed 2 / 2, hybrid 2 / 1 (the FFN and the head in plain fp16)
  int np_w = 3, np_ffn = 3;
  // Stack: the static part of the loop form (ldm_loop.cpp loop_fusable adds what depends on loaded weights)
  bool stack_loop = true;    // the WHOLE reverse loop of a layout in its workgroup, one launch per sampling call; LDM_DEV=1 LDM_STACK_LOOP=0: per step
  bool rel_loop = true;      // cond=relation inside that launch; LDM_DEV=1 LDM_REL_LOOP=0: the per-step path
  bool step0_cache = true;   // all-[MASK] layouts read their first step's logits from the handle's table; LDM_DEV=1 LDM_STEP0_CACHE=0: off
  bool loop_geometry = false;      // the one-launch loop exists for this configuration ...
  bool rel_loop_geometry = false;  // ... and takes cond=relation
  // geometry
  int S = 0, C = 0, Cp = 0, Dp = 0, Fp = 0, dh = 0;
  int Dq = 0, HD = 0, Fq = 0;   // fast: K padded to 64, heads padded to 64
  int x3_qkv_tiles = 0, x3_ffn1_tiles = 0, x3_head_tiles = 0;   // split-type: 32-column tiles of the row-resident launches' weight images
  int chunk = 0, n_lanes = 1, lane_offset_us = 0;
  bool instance_norm = false;    // norm1 = AdaInsNorm (timestep_type adainnorm / adainnorm_abs: statistics per (layout, channel) over the layout's S rows): the
                                 // block's first normalisation is the per-layout launch of kernels_norm.hip (in_rows), which only the tiled sequence has
  bool balanced_chunks = true;   // ldm_loop.cpp run_loop_body: a call's passes share its layouts evenly; LDM_DEV=1 LDM_BALANCED_CHUNKS=0: full chunks + a remainder
  size_t panel_rows = 0;         // split-type: rows of a q / k / v (and hidden) panel
  WorkspaceCounts ws;            // per lane
  HandleCounts bufs;

  bool fast() const { return precision == LDM_PREC_FAST_F16; }
  bool split_type() const { return precision == LDM_PREC_SPLIT_F16 || precision == LDM_PREC_MIXED_F16 || precision == LDM_PREC_HYBRID_F16; }
  bool fp16_engine() const { return precision != LDM_PREC_EXACT_F32 && precision != LDM_PREC_SPLIT_F16; }   // fast / mixed / hybrid
  // the denoiser takes per-layout timesteps: every engine but the stack kernel, whose workgroups take ONE set of AdaLN rows per layer
  bool per_layout_t() const { return structure != Structure::Stack; }
  const char* describe_precision() const {
    static const char* prec[5] = {"exact_f32", "fast_f16", "split_f16", "mixed_f16", "hybrid_f16"};
    return prec[precision];
  }
  std::string describe_kernels() const {
    switch (structure) {
      case Structure::Stack: return "stack";
      case Structure::Generic16: return "generic16";
      case Structure::Tiled: return std::string("tiled_gemm+attn") + (instance_norm ? "+instance_norm" : "");
      default:
        return std::string("row_resident_ln_gemm") + (ffn_fused ? "+attn_ffn_fused_fp16" : "+linear2_prologue") +
               (attnout ? "+attn_out_proj_fused" : "+tiled_gemm+attn");
    }
  }
};

// The refusals ldm_create reports in front of its device probe, in its order: 0, or its return code and message.  `refused_knob`: the first
// knob present although LDM_DEV=1 is not set ("" = none).  (The first error of a bad configuration on a machine without a device is one of
// these or "no HIP device visible"; what plan_engine refuses beyond them comes behind the probe.)
inline int validate_config(const ldm_config& cfg, const std::string& refused_knob, std::string& err) {
  auto bad = [&](const std::string& msg) {
    err = msg;
    return -1;
  };
  char msg[256];
  if (cfg.abi_version != LDM_ABI_VERSION) return bad("ldm_config.abi_version mismatch");
  if (cfg.n_attr != 5) return bad("only the c-x-y-w-h (5 attribute) vocabulary is supported");
  if (cfg.n_category < 1 || cfg.n_bin < 1 || cfg.n_layer < 1 || cfg.n_step < 1 || cfg.n_head < 1 || cfg.d_model < 16)
    return bad("n_category / n_bin / n_layer / n_step / n_head must be >= 1, d_model >= 16");
  {
    // vocabulary: the fp16 engines (fast / mixed / hybrid) run the step tail on at most 192 classes (the stack kernel's fused tail, the
    // 16-lane form of posterior_sample_k); the reference-precision engines (exact / split) have the wide forms of kernels_post.hip /
    // kernels_vb.hip: 9 classes per lane of a wavefront = 576 classes = 18 head tiles, and the encode kernel's 128 bins (ldm_cond_core.h)
    const long n_class = (long)cfg.n_category + 4L * cfg.n_bin + 2;
    if (cfg.n_bin > 128) {
      snprintf(msg, sizeof(msg), "n_bin = %d: more than 128 bins per coordinate are not supported", cfg.n_bin);
      return bad(msg);
    }
    if (n_class > 576) {
      snprintf(msg, sizeof(msg), "n_category + 4 * n_bin + 2 = %ld classes: vocabulary > 576 classes not supported", n_class);
      return bad(msg);
    }
    if (n_class > 192 && cfg.precision != LDM_PREC_EXACT_F32 && cfg.precision != LDM_PREC_SPLIT_F16) {
      static const char* names[5] = {"exact", "fast", "split", "mixed", "hybrid"};
      const char* nm = cfg.precision >= 0 && cfg.precision <= 4 ? names[cfg.precision] : "unknown";
      snprintf(msg, sizeof(msg), "precision %s: vocabulary > 192 classes not supported by the fp16 engines (%ld classes); use precision split or exact",
               nm, n_class);
      return bad(msg);
    }
  }
  if (cfg.d_model % 16 || cfg.d_ff % 16 || cfg.d_model > 1024) return bad("d_model/d_ff must be multiples of 16, d_model <= 1024");
  if (cfg.d_model % cfg.n_head) return bad("d_model must be divisible by n_head");
  if (cfg.d_model / cfg.n_head > 64) return bad("head_dim > 64 not supported");
  if (cfg.precision < 0 || cfg.precision > 4) return bad("unknown precision mode");
  if (cfg.max_batch < 1) return bad("max_batch must be >= 1");
  // development knobs are refused outside dev mode (ldm_knobs.h): no stray variable changes the shipped path
  if (!refused_knob.empty())
    return bad("environment knob " + refused_knob + " is set but LDM_DEV=1 is not: development / ablation paths are refused");
  const int S = cfg.max_elem * cfg.n_attr, dh = cfg.d_model / cfg.n_head;
  // sequence length: the fp16 attention kernels hold a layout's scores in ONE 128 x 128 tile; the fp32 row kernel
  // keeps K and V of a (layout, head) in LDS (2 x S x head_dim floats <= 160 KiB).  The reference's datasets: S = 125.
  if (S < 1) return bad("max_elem must be >= 1");
  if (cfg.precision == LDM_PREC_FAST_F16 && S > 128) return bad("precision fast: at most 128 tokens per layout (max_elem * n_attr); use precision exact");
  if ((size_t)2 * S * ((dh + 3) & ~3) * sizeof(float) > 160 * 1024)
    return bad("sequence too long for the attention kernels (2 * S * head_dim floats must fit 160 KiB of LDS)");
  return 0;
}

// 0 and the plan, or ldm_create's return code and message: validate_config's refusals first, then the decision and what it refuses.
// A refusal of the decision (the last two below) leaves the plan filled as far as it was decided — geometry, sizes, options: what the
// configuration was refused on.
// norm1_kind (LDM_NORM1_*, ldm_create_variant; ldm_create: LDM_NORM1_LAYER, which leaves every plan as it was): what a block's first
// normalisation computes its statistics over.  LDM_NORM1_INSTANCE runs the tiled sequence in exact / split and is refused elsewhere.
inline int plan_engine(const ldm_config& cfg, const Knobs& kn, EnginePlan& p, std::string& err, int norm1_kind = LDM_NORM1_LAYER) {
  p = EnginePlan{};
  if (int rc = validate_config(cfg, kn.refused, err)) return rc;
  auto bad = [&](const std::string& msg) {
    err = msg;
    return -1;
  };
  p.precision = cfg.precision;
  if (norm1_kind != LDM_NORM1_LAYER && norm1_kind != LDM_NORM1_INSTANCE) return bad("unknown norm1 kind");
  p.instance_norm = norm1_kind == LDM_NORM1_INSTANCE;
  if (p.instance_norm && p.fp16_engine()) {
    static const char* names[5] = {"exact", "fast", "split", "mixed", "hybrid"};
    return bad(std::string("precision ") + names[cfg.precision] +
               ": timestep_type adainnorm / adainnorm_abs (instance norm over a layout's rows) has no kernel in the fp16 engines; use precision split or exact");
  }
  const int D = cfg.d_model, F = cfg.d_ff, H = cfg.n_head;
  const int S = p.S = cfg.max_elem * cfg.n_attr, dh = p.dh = D / H;
  const int C = p.C = cfg.n_category + 4 * cfg.n_bin + 2;
  // K axes of the fp16 operand copies: whole 128-byte rows per 64-wide K tile in the split mode (the LDS-DMA split GEMM reads
  // operand rows one K tile at a time: a 64-byte row segment is half a cache line and doubles the L2 traffic)
  p.Dp = round_up(D, p.split_type() ? 64 : 32);
  p.Fp = round_up(F, p.split_type() ? 64 : 32);
  p.Cp = round_up(C, 32);
  if (cfg.q_type != LDM_Q_CONSTRAINED && cfg.q_type != LDM_Q_VANILLA) return bad("unknown q_type");
  // chunk: layouts per pass.  auto: 256 layouts (M = 32 000 rows = 250 row blocks / 256 per-layout workgroups: one full round of the
  // 256 CUs; P + Q of a chunk = 119 MB stay inside the 256 MiB Infinity Cache) and two lanes (ldm_handle.h Workspace)
  // wide vocabularies (> 192 classes): a chunk's logits grow to chunk * S * Cp floats — 74 MB per lane at 576 classes, against 20 MB at
  // 155 — and auto stays at 256 all the same: split at 283 / 539 classes, B = 512, T = 100 runs 1 171 / 1 158 layouts/s with 256-layout
  // chunks, 1 125 / 1 108 with 128, 720 / 710 with 64 (tools/wide_vocab_bench.py --chunk, one session)
  int chunk = kn.chunk != Knobs::kUnset ? kn.chunk : cfg.chunk;
  if (chunk <= 0) chunk = 256;
  p.chunk = chunk = std::min(chunk, cfg.max_batch);
  p.balanced_chunks = Knobs::on(kn.balanced_chunks);
  // lanes: the knobs override cfg.lanes (experiments); more lanes than chunks make no sense
  p.n_lanes = cfg.lanes > 0 ? cfg.lanes : 2;
  if (kn.lanes != Knobs::kUnset) p.n_lanes = std::max(1, kn.lanes);
  p.n_lanes = std::min(p.n_lanes, std::max(1, (cfg.max_batch + chunk - 1) / chunk));
  p.lane_offset_us = kn.lane_offset_us != Knobs::kUnset ? std::max(0, kn.lane_offset_us) : 50;

  const size_t Mc = (size_t)chunk * S;
  // P / Q carry padding rows up to the next multiple of 256: the row-stationary kernels write whole 128-row blocks (rows >= M land in
  // the padding instead of being exec-masked), and the LDS-DMA GEMMs load whole 128-row operand tiles without bounds checks
  const size_t Mt = (size_t)round_up((int)Mc, 256);
  WorkspaceCounts& w = p.ws;
  w.P = w.Q = Mt * D;
  w.logits = Mc * p.Cp;
  if (p.fast()) {
    p.Dq = round_up(D, 64);
    p.HD = H * 64;
    p.Fq = round_up(F, 64);
    // stack kernel: one 128-row tile per layout, and every one of its 4 waves must own at least one real row (its
    // exec-masked stores are counted by the vmcnt waits) => 96 < S <= 128; d_model 464 in 8 heads, K padded to 512
    const bool stack_geometry = S <= 128 && S > 96 && dh <= 64 && D == 464 && p.Dq == 512 && p.HD == 512 && H == 8 && F % 32 == 0 &&
                                F <= 2048 && cfg.n_layer <= 8 && p.Cp % 32 == 0;
    p.structure = stack_geometry && Knobs::on(kn.stack_kernel) ? Structure::Stack : Structure::Generic16;
    p.stack_loop = Knobs::on(kn.stack_loop);
    p.rel_loop = Knobs::on(kn.rel_loop);
    p.step0_cache = Knobs::on(kn.step0_cache);
    w.att16 = Mt * p.HD;
    w.qkv16 = Mt * 3 * p.HD;
    w.stats_a = Mt;
    if (p.structure == Structure::Generic16) {   // LayerNorm outputs and the FFN hidden activation only exist on the generic path
      w.a16 = w.h16 = Mt * p.Dq;
      w.hid16 = Mt * p.Fq;
    }
  } else if (p.split_type()) {
    w.a16 = w.att16 = w.h16 = w.a16lo = w.att16lo = w.h16lo = Mt * p.Dp;
    w.hid16 = w.hid16lo = x3_hidden_rows((int)Mc) * p.Fp;
    w.qkv32 = Mc * 3 * D;
    p.panel_rows = x3_panel_rows((int)Mc, S);
    // q / k / v panels of the fused attention + out_proj kernel: 3 x 8 heads x 2 panels of 32 halfs, hi and lo
    const bool panels = attnout16x3_supported(S, H, dh, D);
    if (panels) w.qkvp_hi = w.qkvp_lo = (size_t)48 * p.panel_rows * 32;
    // the LayerNorm-fed GEMMs as row-resident launches (kernels_lngemm.hip): d_model 464 (K padded to 512), every N within 2048 columns;
    // LDM_DEV=1 LDM_X3_LNGEMM=0: LayerNorm launches + gemm16x3_k (the r04 structure)
    p.x3_qkv_tiles = x3_tiles(3 * D);
    p.x3_ffn1_tiles = x3_tiles(F);
    p.x3_head_tiles = x3_tiles(p.Cp);
    const bool lngemm = p.Dp == 512 && lngemm16x3_supported(D, 3 * D, p.x3_qkv_tiles) && lngemm16x3_supported(D, F, p.x3_ffn1_tiles) &&
                        lngemm16x3_supported(D, p.Cp, p.x3_head_tiles) && p.x3_qkv_tiles * 32 <= round_up(3 * D, 256) &&
                        p.x3_ffn1_tiles * 32 <= round_up(F, 256) && p.x3_head_tiles * 32 <= round_up(C, 256) && Knobs::on(kn.x3_lngemm) &&
                        !p.instance_norm;   // (the row-resident launches normalise a ROW: no per-layout statistics there)
    p.structure = lngemm ? Structure::RowResident : Structure::Tiled;
    // linear2 runs as the GEMM PROLOGUE of the row-resident kernel that normalises its sum (kernels_lngemm.hip PRE: the next layer's AdaLN +
    // in_proj, or the head) instead of as a gemm16x3_k launch: 28 us per layer cheaper than the two launches it replaces, +4 % whole-job
    // same-box.  Fusing out_proj the same way saved nothing per launch and cost the overlap between the two chunk pipelines (a fused launch
    // fills every CU alone): -5 % (profiles/r05_call24_31_*); the attention + out_proj launch replaced it.
    // (a panel is one whole 32-column tile of linear1: d_ff % 32 != 0 keeps the row-major form — launch_lngemm16x3 refuses panels with a
    //  partly masked last tile, and the hybrid mode, which needs the panels, is then refused below)
    p.hid_panels = lngemm && F % 32 == 0 && p.panel_rows <= x3_hidden_rows((int)Mc) && Knobs::on(kn.x3_hidpanel);
    p.attnout = lngemm && panels && p.panel_rows * 64 * 2 < (1ull << 32) && Knobs::on(kn.x3_attnout);
    const bool mixed = cfg.precision == LDM_PREC_MIXED_F16, hybrid = cfg.precision == LDM_PREC_HYBRID_F16;
    p.w2p = lngemm && p.attnout && (mixed || (hybrid && p.hid_panels));
    if (p.w2p) {
      p.np_w = 2;
      p.np_ffn = hybrid ? 1 : 2;
      p.ffn_fused = hybrid && F % 32 == 0 && F <= 2048 && Knobs::on(kn.hyb_ffn);
    }
    if (hybrid && !p.w2p && lngemm && p.attnout && F % 32)
      return bad("precision hybrid: d_ff must be a multiple of 32 (its plain-fp16 hidden activations travel as 32-column panels); use precision mixed or split");
    // (hybrid needs hid_panels, and hid_panels needs panel_rows <= x3_hidden_rows: at S < 64 that fails for a chunk of 256 layouts — 15 488 >
    //  15 424 rows at S = 60 — and holds for one of 8.  The refusal then blames the backbone's geometry; pinned as it is by
    //  tests/cpu_engine_plan_check.cpp)
    if ((mixed || hybrid) && !p.w2p)
      return bad("precision mixed / hybrid: only the reference backbone's geometry (d_model 464, 8 heads, <= 128 tokens per layout) has the two-product kernels; use precision split");
  } else {
    w.qkv32 = Mc * 3 * D;
    w.att32 = w.h32 = Mc * D;
    w.hid32 = Mc * F;
  }
  HandleCounts& b = p.bufs;
  b.tok_a = b.tok_b = b.st_cond_seq = b.st_strong = (size_t)cfg.max_batch * S;
  b.rng = 2;
  b.sched = (size_t)kSchedRows * cfg.n_attr * (cfg.n_step + 1);
  if (p.structure == Structure::Stack) {
    b.step0_tab = (size_t)kStep0Slots * kStackStep0Floats;
    b.step0_tok = (size_t)2 * S;
    b.step0_flags = (size_t)cfg.max_batch;
    // The one-launch loop (kernels_stack.hip HEAD == 2): a vocabulary of 5 head tiles whose attribute sub-vocabularies (+ [PAD], [MASK])
    // fit the fused tail (C - 1 > 128: the row log-softmax guards `class < C - 1` in the last of the five head tiles only).
    // cond=relation: the constrained vocabulary with <= 32 bins and <= 32 elements.
    const int live_max = (cfg.q_type == LDM_Q_VANILLA ? C - 2 : std::max(cfg.n_category, cfg.n_bin)) + 2;
    p.loop_geometry = p.stack_loop && p.Cp == 160 && C - 1 > 128 && live_max <= kStackPostMaxLive && cfg.n_step < 32768;
    p.rel_loop_geometry = p.loop_geometry && p.rel_loop && cfg.q_type == LDM_Q_CONSTRAINED && cfg.n_bin <= 32 && cfg.max_elem <= 32;
  }
  return 0;
}

}  // namespace ldm
