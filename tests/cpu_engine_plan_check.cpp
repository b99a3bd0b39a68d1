// Host check of layout_dm_amd/csrc/ldm_engine_plan.h — the header ldm_create plans a handle with — built with plain g++ (and as the
// ASan + UBSan build) and run as its own process by tests/test_engine_plan.py.  One line per case on stdout.
//   table    the geometry -> engine table and its refusals against values WRITTEN DOWN BY HAND from the ldm_create this header replaced
//            (flags, padded sizes, buffer counts, messages byte for byte), and that knobs which were never read change nothing
//   arith    the workspace size rules as arithmetic: every S in 1..128, chunk in {1, 8, 150, 256}, every split-type precision
//   plan ... one configuration from the command line (tests/test_engine_plan.py feeds it tests/test_launch_sequence_gpu.py's CASES)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../layout_dm_amd/csrc/ldm_engine_plan.h"

using namespace ldm;

static int g_failed = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      printf("FAIL %s: ", #c);                 \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      ++g_failed;                              \
    }                                          \
  } while (0)

static ldm_config backbone(int precision, int max_batch = 256) {
  ldm_config c{};
  c.abi_version = LDM_ABI_VERSION;
  c.n_category = 25; c.n_bin = 32; c.max_elem = 25; c.n_attr = 5;
  c.d_model = 464; c.n_head = 8; c.d_ff = 1856; c.n_layer = 4; c.n_step = 100;
  c.q_type = LDM_Q_CONSTRAINED; c.precision = precision; c.max_batch = max_batch;
  return c;
}
static ldm_config small(int precision, int max_batch = 256) {
  ldm_config c = backbone(precision, max_batch);
  c.d_model = 256; c.n_head = 4; c.d_ff = 1024; c.n_layer = 2;
  return c;
}

static const char* structure_name(Structure s) {
  switch (s) {
    case Structure::Stack: return "Stack";
    case Structure::Generic16: return "Generic16";
    case Structure::Tiled: return "Tiled";
    case Structure::RowResident: return "RowResident";
  }
  return "?";
}

static void print_plan(const char* id, int rc, const EnginePlan& p, const std::string& err, bool late = false) {
  if (rc) {
    printf("case=%s rc=%d late=%d err=%s\n", id, rc, (int)late, err.c_str());
    return;
  }
  printf("case=%s rc=0 structure=%s precision=%s kernels=%s attnout=%d hid_panels=%d ffn_fused=%d w2p=%d np=%d/%d loop=%d rel_loop=%d step0=%d plt=%d "
         "S=%d C=%d Cp=%d Dp=%d Fp=%d Dq=%d HD=%d Fq=%d dh=%d tiles=%d/%d/%d chunk=%d lanes=%d offset_us=%d balanced=%d panel_rows=%zu\n",
         id, structure_name(p.structure), p.describe_precision(), p.describe_kernels().c_str(), (int)p.attnout, (int)p.hid_panels, (int)p.ffn_fused,
         (int)p.w2p, p.np_w, p.np_ffn, (int)p.loop_geometry, (int)p.rel_loop_geometry, (int)p.step0_cache, (int)p.per_layout_t(), p.S, p.C, p.Cp, p.Dp,
         p.Fp, p.Dq, p.HD, p.Fq, p.dh, p.x3_qkv_tiles, p.x3_ffn1_tiles, p.x3_head_tiles, p.chunk, p.n_lanes, p.lane_offset_us, (int)p.balanced_chunks,
         p.panel_rows);
}

// ---- the parent's table, by hand.  Backbone: C = 25 + 4 * 32 + 2 = 155, Cp = 160, S = 125, dh = 58.
static const char* kMixedMsg =
    "precision mixed / hybrid: only the reference backbone's geometry (d_model 464, 8 heads, <= 128 tokens per layout) has the two-product kernels; use "
    "precision split";
static const char* kHybridFfMsg =
    "precision hybrid: d_ff must be a multiple of 32 (its plain-fp16 hidden activations travel as 32-column panels); use precision mixed or split";
static const char* kFast128Msg = "precision fast: at most 128 tokens per layout (max_elem * n_attr); use precision exact";

struct Accepted {   // what the parent's ldm_create left on the handle
  Structure structure;
  const char* kernels;
  bool attnout, hid_panels, ffn_fused, w2p;
  int np_w, np_ffn;
  bool loop;   // the geometry half of the parent's loop_fusable
  int chunk, lanes, Dp, Fp, Dq, HD, Fq;
  size_t panel_rows;
  // counts of the parent's A(&ws.…, n) calls (0: not allocated): P, logits, qkv32, a16, att16, hid16, hid16lo, qkv16, qkvp_hi, stats_a, hid32; and step0_tab
  size_t P, logits, qkv32, a16, att16, hid16, hid16lo, qkv16, qkvp_hi, stats_a, hid32, step0_tab;
};

static void expect(const char* id, const ldm_config& c, const Knobs& kn, const Accepted& e) {
  EnginePlan p;
  std::string err;
  const int rc = plan_engine(c, kn, p, err);
  print_plan(id, rc, p, err);
  CHECK(rc == 0, "%s: refused: %s", id, err.c_str());
  if (rc) return;
  CHECK(p.structure == e.structure, "%s", id);
  CHECK(p.describe_kernels() == e.kernels, "%s: %s", id, p.describe_kernels().c_str());
  CHECK(p.precision == c.precision, "%s: the requested precision is never rewritten", id);
  CHECK(p.attnout == e.attnout && p.hid_panels == e.hid_panels && p.ffn_fused == e.ffn_fused && p.w2p == e.w2p, "%s: options", id);
  CHECK(p.np_w == e.np_w && p.np_ffn == e.np_ffn, "%s: products %d/%d", id, p.np_w, p.np_ffn);
  CHECK(p.loop_geometry == e.loop && p.per_layout_t() == (e.structure != Structure::Stack), "%s: loop form", id);
  CHECK(p.chunk == e.chunk && p.n_lanes == e.lanes && p.lane_offset_us == 50 && p.balanced_chunks, "%s: chunk %d lanes %d", id, p.chunk, p.n_lanes);
  CHECK(p.S == c.max_elem * 5 && p.C == c.n_category + 4 * c.n_bin + 2 && p.Cp == (p.C + 31) / 32 * 32 && p.dh == c.d_model / c.n_head, "%s: geometry", id);
  CHECK(p.Dp == e.Dp && p.Fp == e.Fp && p.Dq == e.Dq && p.HD == e.HD && p.Fq == e.Fq, "%s: padded axes %d %d %d %d %d", id, p.Dp, p.Fp, p.Dq, p.HD, p.Fq);
  CHECK(p.panel_rows == e.panel_rows, "%s: panel_rows %zu", id, p.panel_rows);
  const WorkspaceCounts& w = p.ws;
  CHECK(w.P == e.P && w.Q == e.P && w.logits == e.logits, "%s: P %zu logits %zu", id, w.P, w.logits);
  CHECK(w.qkv32 == e.qkv32 && w.hid32 == e.hid32 && w.att32 == (e.hid32 ? e.logits / p.Cp * c.d_model : 0) && w.h32 == w.att32, "%s: fp32 %zu %zu %zu", id, w.qkv32, w.hid32, w.att32);
  CHECK(w.a16 == e.a16 && w.h16 == e.a16 && w.att16 == e.att16 && w.hid16 == e.hid16 && w.qkv16 == e.qkv16, "%s: fp16 %zu %zu %zu %zu", id, w.a16, w.att16, w.hid16, w.qkv16);
  CHECK(w.hid16lo == e.hid16lo && w.a16lo == (e.hid16lo ? e.a16 : 0) && w.att16lo == w.a16lo && w.h16lo == w.a16lo, "%s: lo %zu %zu", id, w.hid16lo, w.a16lo);
  CHECK(w.qkvp_hi == e.qkvp_hi && w.qkvp_lo == e.qkvp_hi && w.stats_a == e.stats_a, "%s: panels %zu stats %zu", id, w.qkvp_hi, w.stats_a);
  const HandleCounts& b = p.bufs;
  const size_t BS = (size_t)c.max_batch * p.S;
  CHECK(b.tok_a == BS && b.tok_b == BS && b.st_cond_seq == BS && b.st_strong == BS && b.rng == 2 && b.sched == (size_t)8 * 5 * (c.n_step + 1), "%s: handle buffers", id);
  CHECK(b.step0_tab == e.step0_tab && b.step0_tok == (e.step0_tab ? (size_t)2 * p.S : 0) && b.step0_flags == (e.step0_tab ? (size_t)c.max_batch : 0), "%s: step-0 buffers", id);
}

static void expect_refused(const char* id, const ldm_config& c, const Knobs& kn, const char* msg, bool whole, bool late) {
  EnginePlan p;
  std::string err;
  const int rc = plan_engine(c, kn, p, err);
  // in front of ldm_create's device probe: validate_config's refusals, which plan_engine repeats; behind it: the decision's own
  std::string early;
  const int rc_early = validate_config(c, kn.refused, early);
  print_plan(id, rc, p, err, rc_early == 0);
  CHECK(rc == -1, "%s: rc %d", id, rc);
  CHECK(whole ? err == msg : err.find(msg) != std::string::npos, "%s: message: %s", id, err.c_str());
  CHECK(late ? rc_early == 0 : rc_early == rc && early == err, "%s: reported %s the device probe", id, late ? "behind" : "in front of");
}

static const char* ROW = "row_resident_ln_gemm+linear2_prologue+attn_out_proj_fused";

static int table() {
  const Knobs none;
  // ---- the eleven cases of tests/test_launch_sequence_gpu.py, at its max_batch = 8: chunk = 8, one lane, Mc = 1000 rows, Mt = 1024
  // fast: Dp / Fp to 32 (480 / 1856), Dq = HD = 512, Fq = 1856; step-0 table 4 slots x 5 * 16 * 256 floats
  const Accepted fast8{Structure::Stack, "stack", false, false, false, false, 3, 3, true, 8, 1, 480, 1856, 512, 512, 1856, 0,
                       1024 * 464, 1000 * 160, 0, 0, 1024 * 512, 0, 0, 1024 * 1536, 0, 1024, 0, 4 * 20480};
  expect("fast", backbone(LDM_PREC_FAST_F16, 8), none, fast8);
  // small: dh = 64, HD = 256, Dq = 256, Fq = 1024: the generic kernels keep LayerNorm outputs and the hidden activations
  const Accepted fast_small8{Structure::Generic16, "generic16", false, false, false, false, 3, 3, false, 8, 1, 256, 1024, 256, 256, 1024, 0,
                             1024 * 256, 1000 * 160, 0, 1024 * 256, 1024 * 256, 1024 * 1024, 0, 1024 * 768, 0, 1024, 0, 0};
  expect("fast_generic_geometry", small(LDM_PREC_FAST_F16, 8), none, fast_small8);
  const Accepted exact8{Structure::Tiled, "tiled_gemm+attn", false, false, false, false, 3, 3, false, 8, 1, 480, 1856, 0, 0, 0, 0,
                        1024 * 464, 1000 * 160, 1000 * 1392, 0, 0, 0, 0, 0, 0, 0, 1000 * 1856, 0};
  expect("exact", backbone(LDM_PREC_EXACT_F32, 8), none, exact8);
  // small, exact: Dp / Fp to 32 are d_model / d_ff themselves; fp32 activations only: qkv32 1000 x 768, att32 / h32 1000 x 256, hid32 1000 x 1024
  const Accepted exact_small8{Structure::Tiled, "tiled_gemm+attn", false, false, false, false, 3, 3, false, 8, 1, 256, 1024, 0, 0, 0, 0,
                              1024 * 256, 1000 * 160, 1000 * 768, 0, 0, 0, 0, 0, 0, 0, 1000 * 1024, 0};
  expect("exact_generic_geometry", small(LDM_PREC_EXACT_F32, 8), none, exact_small8);
  // split-type: Dp / Fp to 64 (512 / 1856); hid16 has Mt + 64 rows; panel_rows = round_up(1000 + 8, 64) = 1024; 48 panels of 32 halves
  Accepted split8{Structure::RowResident, ROW, true, true, false, false, 3, 3, false, 8, 1, 512, 1856, 0, 0, 0, 1024,
                  1024 * 464, 1000 * 160, 1000 * 1392, 1024 * 512, 1024 * 512, 1088 * 1856, 1088 * 1856, 0, 48 * 1024 * 32, 0, 0, 0};
  expect("split", backbone(LDM_PREC_SPLIT_F16, 8), none, split8);
  Accepted mixed8 = split8;
  mixed8.w2p = true; mixed8.np_w = 2; mixed8.np_ffn = 2;
  expect("mixed", backbone(LDM_PREC_MIXED_F16, 8), none, mixed8);
  Accepted hybrid8 = mixed8;
  hybrid8.np_ffn = 1; hybrid8.ffn_fused = true; hybrid8.kernels = "row_resident_ln_gemm+attn_ffn_fused_fp16+attn_out_proj_fused";
  expect("hybrid", backbone(LDM_PREC_HYBRID_F16, 8), none, hybrid8);
  {
    Knobs k; k.x3_lngemm = 0;   // the tiled launches on the same buffers (the panels stay allocated, as in the parent)
    Accepted e = split8;
    e.structure = Structure::Tiled; e.kernels = "tiled_gemm+attn"; e.attnout = e.hid_panels = false;
    expect("split_lngemm_0", backbone(LDM_PREC_SPLIT_F16, 8), k, e);
  }
  {
    Knobs k; k.x3_attnout = 0;
    Accepted e = split8;
    e.attnout = false; e.kernels = "row_resident_ln_gemm+linear2_prologue+tiled_gemm+attn";
    expect("split_attnout_0", backbone(LDM_PREC_SPLIT_F16, 8), k, e);
  }
  {
    Knobs k; k.x3_hidpanel = 0;
    Accepted e = split8;
    e.hid_panels = false;
    expect("split_hidpanel_0", backbone(LDM_PREC_SPLIT_F16, 8), k, e);
  }
  {
    Knobs k; k.hyb_ffn = 0;   // linear1 -> plain-fp16 panels -> linear2 as the next launch's prologue: split's launch table
    Accepted e = hybrid8;
    e.ffn_fused = false; e.kernels = ROW;
    expect("hybrid_ffn_0", backbone(LDM_PREC_HYBRID_F16, 8), k, e);
  }
  // small, split-type: Dp = 256; no panels (4 heads); the tile counts are computed all the same
  const Accepted split_small8{Structure::Tiled, "tiled_gemm+attn", false, false, false, false, 3, 3, false, 8, 1, 256, 1024, 0, 0, 0, 1024,
                              1024 * 256, 1000 * 160, 1000 * 768, 1024 * 256, 1024 * 256, 1088 * 1024, 1088 * 1024, 0, 0, 0, 0, 0};
  expect("split_generic_geometry", small(LDM_PREC_SPLIT_F16, 8), none, split_small8);

  // ---- at the default batch (max_batch 256): chunk = 256 = one chunk, so ONE lane; Mc = 32 000, Mt = 32 000
  {
    Accepted e = fast8;
    e.chunk = 256; e.P = (size_t)32000 * 464; e.logits = (size_t)32000 * 160; e.att16 = (size_t)32000 * 512; e.qkv16 = (size_t)32000 * 1536; e.stats_a = 32000;
    expect("fast_256", backbone(LDM_PREC_FAST_F16), none, e);
    ldm_config c = backbone(LDM_PREC_FAST_F16);
    c.max_elem = 20;   // S = 100: Mc = 25 600 = Mt
    e.P = (size_t)25600 * 464; e.logits = (size_t)25600 * 160; e.att16 = (size_t)25600 * 512; e.qkv16 = (size_t)25600 * 1536; e.stats_a = 25600;
    expect("fast_S100", c, none, e);
    c.max_elem = 19;   // S = 95: the stack kernel needs 96 < S <= 128 (each of its 4 waves owns a real row); Mc = 24 320, Mt = 24 320
    e = fast_small8;
    e.chunk = 256; e.Dp = 480; e.Fp = 1856; e.Dq = 512; e.HD = 512; e.Fq = 1856;
    e.P = (size_t)24320 * 464; e.logits = (size_t)24320 * 160; e.a16 = (size_t)24320 * 512; e.att16 = (size_t)24320 * 512; e.hid16 = (size_t)24320 * 1856;
    e.qkv16 = (size_t)24320 * 1536; e.stats_a = 24320;
    expect("fast_S95", c, none, e);
    c.max_elem = 26;
    expect_refused("fast_S130", c, none, kFast128Msg, true, false);
  }
  {
    // two lanes need two chunks: max_batch 512
    Accepted e = split8;
    e.chunk = 256; e.lanes = 2; e.panel_rows = 32064;   // round_up(32 000 + 8, 64)
    e.P = (size_t)32000 * 464; e.logits = (size_t)32000 * 160; e.qkv32 = (size_t)32000 * 1392; e.a16 = e.att16 = (size_t)32000 * 512;
    e.hid16 = e.hid16lo = (size_t)32064 * 1856; e.qkvp_hi = (size_t)48 * 32064 * 32;
    expect("split_512", backbone(LDM_PREC_SPLIT_F16, 512), none, e);
  }
  expect_refused("small_mixed", small(LDM_PREC_MIXED_F16), none, kMixedMsg, true, true);
  expect_refused("small_hybrid", small(LDM_PREC_HYBRID_F16), none, kMixedMsg, true, true);
  {
    ldm_config c = backbone(LDM_PREC_HYBRID_F16);
    c.d_ff = 1840;   // % 16 == 0, % 32 != 0: linear1's last tile would be partly masked, no panels
    expect_refused("hybrid_dff1840", c, none, kHybridFfMsg, true, true);
  }
  {
    // hybrid needs hid_panels, and hid_panels needs panel_rows <= round_up(chunk S, 256) + 64.
    //   S = 65, chunk 256: panel_rows = round_up(16 640 + 63, 64) = 16 704 <= 16 640 + 64
    //   S = 60, chunk 256: panel_rows = round_up(15 360 + 68, 64) = 15 488  > 15 360 + 64 = 15 424: refused, and the message blames the geometry
    //   S = 60, chunk 8:   panel_rows = round_up(480 + 68, 64) = 576 <= 512 + 64
    ldm_config c = backbone(LDM_PREC_HYBRID_F16);
    Accepted e = hybrid8;
    e.chunk = 256; e.loop = false;
    c.max_elem = 13;
    e.panel_rows = 16704; e.P = (size_t)16640 * 464; e.logits = (size_t)16640 * 160; e.qkv32 = (size_t)16640 * 1392; e.a16 = e.att16 = (size_t)16640 * 512;
    e.hid16 = e.hid16lo = (size_t)16704 * 1856; e.qkvp_hi = (size_t)48 * 16704 * 32;
    expect("hybrid_S65", c, none, e);
    c.max_elem = 12;
    expect_refused("hybrid_S60", c, none, kMixedMsg, true, true);
    {
      EnginePlan p;
      std::string err;
      plan_engine(c, none, p, err);
      CHECK(p.panel_rows == 15488 && p.ws.hid16 == (size_t)15424 * 1856 && !p.hid_panels && p.attnout, "hybrid_S60: panel_rows %zu", p.panel_rows);
    }
    c.max_batch = 8;
    e.chunk = 8; e.panel_rows = 576; e.P = (size_t)512 * 464; e.logits = (size_t)480 * 160; e.qkv32 = (size_t)480 * 1392; e.a16 = e.att16 = (size_t)512 * 512;
    e.hid16 = e.hid16lo = (size_t)576 * 1856; e.qkvp_hi = (size_t)48 * 576 * 32;
    expect("hybrid_S60_batch8", c, none, e);
    // mixed does not need the panels: hidden activations row-major, hi and lo
    c = backbone(LDM_PREC_MIXED_F16);
    c.max_elem = 12;
    e = mixed8;
    e.chunk = 256; e.hid_panels = false; e.panel_rows = 15488; e.P = (size_t)15360 * 464; e.logits = (size_t)15360 * 160; e.qkv32 = (size_t)15360 * 1392;
    e.a16 = e.att16 = (size_t)15360 * 512; e.hid16 = e.hid16lo = (size_t)15424 * 1856; e.qkvp_hi = (size_t)48 * 15488 * 32;
    expect("mixed_S60", c, none, e);
  }
  for (int prec : {LDM_PREC_FAST_F16, LDM_PREC_MIXED_F16, LDM_PREC_HYBRID_F16, LDM_PREC_EXACT_F32, LDM_PREC_SPLIT_F16}) {
    ldm_config c = backbone(prec);
    c.n_bin = 64;   // 283 classes, Cp = 288
    const std::string id = std::string("n_bin64_") + std::to_string(prec);
    if (prec == LDM_PREC_EXACT_F32 || prec == LDM_PREC_SPLIT_F16) {
      EnginePlan p;
      std::string err;
      const int rc = plan_engine(c, none, p, err);
      print_plan(id.c_str(), rc, p, err);
      CHECK(rc == 0 && p.C == 283 && p.Cp == 288 && p.x3_head_tiles == (prec == LDM_PREC_SPLIT_F16 ? 10 : 0) &&
                p.structure == (prec == LDM_PREC_SPLIT_F16 ? Structure::RowResident : Structure::Tiled),
            "%s", id.c_str());
    } else {
      static const char* names[5] = {"exact", "fast", "split", "mixed", "hybrid"};
      const std::string msg = std::string("precision ") + names[prec] +
                              ": vocabulary > 192 classes not supported by the fp16 engines (283 classes); use precision split or exact";
      expect_refused(id.c_str(), c, none, msg.c_str(), true, false);
    }
  }
  {
    // the early refusals keep their order and their place in front of the device probe
    ldm_config c = backbone(LDM_PREC_FAST_F16);
    c.abi_version = LDM_ABI_VERSION + 1;
    expect_refused("abi", c, none, "ldm_config.abi_version mismatch", true, false);
    c = backbone(LDM_PREC_FAST_F16);
    c.n_bin = 129; c.precision = 9;
    expect_refused("bins_129", c, none, "n_bin = 129: more than 128 bins per coordinate are not supported", true, false);
    c.n_bin = 128; c.n_category = 63;
    expect_refused("classes_577", c, none, "n_category + 4 * n_bin + 2 = 577 classes: vocabulary > 576 classes not supported", true, false);
    c.n_bin = 64;
    expect_refused("precision_9_wide", c, none, "precision unknown: vocabulary > 192 classes", false, false);
    c.n_bin = 32; c.n_category = 25;
    expect_refused("precision_9", c, none, "unknown precision mode", true, false);
    c = backbone(LDM_PREC_EXACT_F32);
    c.max_batch = 0;
    expect_refused("max_batch_0", c, none, "max_batch must be >= 1", true, false);
    c = backbone(LDM_PREC_EXACT_F32);
    Knobs k; k.refused = "LDM_CHUNK";
    expect_refused("knob_outside_dev", c, k, "environment knob LDM_CHUNK is set but LDM_DEV=1 is not: development / ablation paths are refused", true, false);
    c.max_elem = 2000;   // 2 * 10 000 * 60 floats > 160 KiB
    expect_refused("too_long", c, none, "sequence too long for the attention kernels (2 * S * head_dim floats must fit 160 KiB of LDS)", true, false);
    c = backbone(LDM_PREC_EXACT_F32);
    c.q_type = 7;
    expect_refused("q_type", c, none, "unknown q_type", true, true);
  }
  {
    // knobs: outside dev mode ldm_create reads none (every field unset) — and one that is set to what it defaults to, or that belongs to
    // another engine, changes nothing either
    auto same = [](const ldm_config& c, const Knobs& k, const char* id) {
      EnginePlan a, b;
      std::string ea, eb;
      const int ra = plan_engine(c, Knobs{}, a, ea), rb = plan_engine(c, k, b, eb);
      printf("case=%s rc=%d\n", id, rb);
      CHECK(ra == rb && ea == eb && a.structure == b.structure && a.describe_kernels() == b.describe_kernels() && a.attnout == b.attnout &&
                a.hid_panels == b.hid_panels && a.ffn_fused == b.ffn_fused && a.w2p == b.w2p && a.np_w == b.np_w && a.np_ffn == b.np_ffn &&
                a.loop_geometry == b.loop_geometry && a.rel_loop_geometry == b.rel_loop_geometry && a.step0_cache == b.step0_cache &&
                a.chunk == b.chunk && a.n_lanes == b.n_lanes && a.lane_offset_us == b.lane_offset_us && a.balanced_chunks == b.balanced_chunks &&
                a.panel_rows == b.panel_rows && !memcmp(&a.ws, &b.ws, sizeof(a.ws)) && !memcmp(&a.bufs, &b.bufs, sizeof(a.bufs)),
            "%s", id);
    };
    Knobs k;
    k.x3_lngemm = 1; k.x3_attnout = 1; k.x3_hidpanel = 5; k.hyb_ffn = 1; k.balanced_chunks = 1; k.lane_offset_us = 50; k.chunk = 0;
    same(backbone(LDM_PREC_HYBRID_F16, 512), k, "knobs_at_their_defaults");
    Knobs f;
    f.stack_kernel = 0; f.stack_loop = 0; f.rel_loop = 0; f.step0_cache = 0;
    same(backbone(LDM_PREC_SPLIT_F16, 512), f, "fast_knobs_on_split");
    Knobs x;
    x.x3_lngemm = 0; x.x3_attnout = 0; x.x3_hidpanel = 0; x.hyb_ffn = 0;
    same(backbone(LDM_PREC_FAST_F16, 512), x, "split_knobs_on_fast");
  }
  {
    // ... and the knobs that are honoured: the parent's overrides
    Knobs k; k.chunk = 64; k.lanes = 7; k.lane_offset_us = -3; k.balanced_chunks = 0; k.stack_loop = 0;
    EnginePlan p;
    std::string err;
    const int rc = plan_engine(backbone(LDM_PREC_FAST_F16, 200), k, p, err);
    print_plan("overrides", rc, p, err);
    CHECK(rc == 0 && p.chunk == 64 && p.n_lanes == 4 && p.lane_offset_us == 0 && !p.balanced_chunks && p.structure == Structure::Stack &&
              !p.loop_geometry && !p.rel_loop_geometry && p.step0_cache,
          "overrides: chunk %d lanes %d", p.chunk, p.n_lanes);   // (lanes: at most ceil(200 / 64) = 4 chunks)
    Knobs g; g.stack_kernel = 0;
    const int rc2 = plan_engine(backbone(LDM_PREC_FAST_F16, 200), g, p, err);
    print_plan("fused_attn_0", rc2, p, err);
    CHECK(rc2 == 0 && p.structure == Structure::Generic16 && p.per_layout_t() && !p.loop_geometry && p.bufs.step0_tab == 0 && p.ws.a16 == p.ws.P / 464 * 512,
          "fused_attn_0");
    Knobs r; r.rel_loop = 0;
    plan_engine(backbone(LDM_PREC_FAST_F16), r, p, err);
    CHECK(p.loop_geometry && !p.rel_loop_geometry, "rel_loop_0");
    ldm_config c = backbone(LDM_PREC_FAST_F16);
    c.q_type = LDM_Q_VANILLA;   // every class live at every position: 155 > 48 live classes, no fused step tail
    plan_engine(c, none, p, err);
    CHECK(p.structure == Structure::Stack && !p.loop_geometry, "vanilla");
  }
  return g_failed;
}

// The size rules as arithmetic.  The fused attention launch reads 128 rows of every panel from each layout's first row: the last layout's
// read starts at row (chunk - 1) S, so a panel needs chunk S + 128 - S rows (8 rows short of it at S = 50 once, a fault at a page boundary).
static int arith() {
  long cases = 0;
  for (int chunk : {1, 8, 150, 256})
    for (int S = 1; S <= 128; ++S) {
      const int Mc = chunk * S;
      const size_t rows = x3_panel_rows(Mc, S);
      ++cases;
      CHECK(rows >= (size_t)Mc + 128 - S && rows % 64 == 0, "S %d chunk %d: panel_rows %zu", S, chunk, rows);
      CHECK(x3_hidden_rows(Mc) >= (size_t)(Mc + 255) / 256 * 256, "S %d chunk %d: whole GEMM tiles of hidden rows", S, chunk);
      if (S % 5) continue;   // (n_attr is 5: a configuration reaches the multiples of 5)
      for (int prec : {LDM_PREC_SPLIT_F16, LDM_PREC_MIXED_F16, LDM_PREC_HYBRID_F16}) {
        ldm_config c = backbone(prec);
        c.chunk = chunk;
        c.max_elem = S / 5;
        EnginePlan p;
        std::string err;
        const int rc = plan_engine(c, Knobs{}, p, err);
        ++cases;
        CHECK(rc == 0 || (prec == LDM_PREC_HYBRID_F16 && p.panel_rows && !p.hid_panels), "S %d chunk %d precision %d: %s", S, chunk, prec, err.c_str());
        CHECK(p.S == S && p.chunk == chunk && p.panel_rows == rows, "S %d chunk %d: the plan's panel_rows %zu", S, chunk, p.panel_rows);
        CHECK(p.ws.qkvp_hi == 48 * rows * 32 && p.ws.qkvp_lo == p.ws.qkvp_hi, "S %d chunk %d: panels", S, chunk);
        CHECK(p.ws.hid16 == x3_hidden_rows(Mc) * p.Fp && p.ws.hid16lo == p.ws.hid16, "S %d chunk %d: hid16 %zu", S, chunk, p.ws.hid16);
        CHECK(p.hid_panels == (rows <= x3_hidden_rows(Mc)), "S %d chunk %d: hid_panels %d", S, chunk, (int)p.hid_panels);
        if (p.hid_panels) CHECK(p.ws.hid16 >= rows * p.Fp && p.ws.hid16lo >= rows * p.Fp, "S %d chunk %d: hid16 %zu", S, chunk, p.ws.hid16);
      }
    }
  printf("arith cases=%ld failed=%d\n", cases, g_failed);
  return g_failed;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "table")) return table() ? 1 : 0;
  if (argc >= 2 && !strcmp(argv[1], "arith")) return arith() ? 1 : 0;
  if (argc >= 12 && !strcmp(argv[1], "plan")) {
    // plan n_category n_bin max_elem d_model n_head d_ff n_layer n_step precision max_batch [KNOB=value ...]
    ldm_config c = backbone(atoi(argv[10]), atoi(argv[11]));
    c.n_category = atoi(argv[2]); c.n_bin = atoi(argv[3]); c.max_elem = atoi(argv[4]); c.d_model = atoi(argv[5]); c.n_head = atoi(argv[6]);
    c.d_ff = atoi(argv[7]); c.n_layer = atoi(argv[8]); c.n_step = atoi(argv[9]);
    Knobs k;
    for (int i = 12; i < argc; ++i) {
      const char* eq = strchr(argv[i], '=');
      if (!eq) return 2;
      const std::string name((const char*)argv[i], eq);
      const int v = atoi(eq + 1);
      if (name == "LDM_X3_LNGEMM") k.x3_lngemm = v;
      else if (name == "LDM_X3_ATTNOUT") k.x3_attnout = v;
      else if (name == "LDM_X3_HIDPANEL") k.x3_hidpanel = v;
      else if (name == "LDM_HYB_FFN") k.hyb_ffn = v;
      else if (name == "LDM_FUSED_ATTN") k.stack_kernel = v;
      else return 2;
    }
    EnginePlan p;
    std::string err;
    const int rc = plan_engine(c, k, p, err);
    print_plan("plan", rc, p, err);
    return 0;
  }
  fprintf(stderr, "usage: %s table | arith | plan <geometry> <precision> <max_batch> [KNOB=value ...]\n", argv[0]);
  return 2;
}
