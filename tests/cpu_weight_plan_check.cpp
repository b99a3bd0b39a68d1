// Host check of layout_dm_amd/csrc/ldm_weight_plan.h — the header ldm_finalize_weights plans a checkpoint with — built with plain g++ (and
// as the ASan + UBSan build) and run as its own process by tests/test_weight_plan.py.  One line per case on stdout.
//   table          the accepted checkpoints (variant, keys read), every refusal byte for byte — the strings WRITTEN DOWN from the
//                  ldm_finalize_weights this header replaced — and the derived-buffer counts against that function's allocation expressions
//   cast in out    in: n floats; out: the split scale (one float), then hi[n] and lo[n] as fp16 bit patterns (tests/test_weight_plan.py
//                  holds them against NumPy's float16)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../layout_dm_amd/csrc/ldm_weight_plan.h"

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

static ldm_config backbone(int precision) {
  ldm_config c{};
  c.abi_version = LDM_ABI_VERSION;
  c.n_category = 25; c.n_bin = 32; c.max_elem = 25; c.n_attr = 5;
  c.d_model = 464; c.n_head = 8; c.d_ff = 1856; c.n_layer = 4; c.n_step = 100;
  c.q_type = LDM_Q_CONSTRAINED; c.precision = precision; c.max_batch = 8;
  return c;
}
static ldm_config small(int precision) {   // tests/test_launch_sequence_gpu.py SMALL
  ldm_config c = backbone(precision);
  c.d_model = 256; c.n_head = 4; c.d_ff = 1024; c.n_layer = 2; c.n_step = 20;
  return c;
}

// ---- the reference's checkpoints as name -> shape, in the order ldm_finalize_weights reads them
enum Pos { kPair, kDefault };
enum Ts { kLearned, kAbs, kNone };
typedef std::vector<std::pair<std::string, std::vector<int64_t>>> KeyList;

static KeyList checkpoint(const ldm_config& c, Pos pos, Ts ts, int pos_rows = 0) {
  const int64_t D = c.d_model, F = c.d_ff, C = c.n_category + 4 * c.n_bin + 2, T = c.n_step;
  KeyList k;
  k.push_back({"transformer.cat_emb.weight", {C, D}});
  if (pos == kDefault) {
    k.push_back({"transformer.pos_emb.pos_emb", {pos_rows ? pos_rows : c.max_elem * c.n_attr, D}});
  } else {
    k.push_back({"transformer.pos_emb.elem_emb", {c.max_elem, D}});
    k.push_back({"transformer.pos_emb.attr_emb", {c.n_attr, D}});
  }
  k.push_back({"transformer.head.0.weight", {D}});
  k.push_back({"transformer.head.0.bias", {D}});
  k.push_back({"transformer.head.1.weight", {C, D}});
  for (int i = 0; i < c.n_layer; ++i) {
    const std::string b = "transformer.backbone.layers." + std::to_string(i) + ".";
    k.push_back({b + "self_attn.in_proj_weight", {3 * D, D}});
    k.push_back({b + "self_attn.in_proj_bias", {3 * D}});
    k.push_back({b + "self_attn.out_proj.weight", {D, D}});
    k.push_back({b + "self_attn.out_proj.bias", {D}});
    k.push_back({b + "linear1.weight", {F, D}});
    k.push_back({b + "linear1.bias", {F}});
    k.push_back({b + "linear2.weight", {D, F}});
    k.push_back({b + "linear2.bias", {D}});
    if (ts == kNone) {
      k.push_back({b + "norm1.weight", {D}});
      k.push_back({b + "norm1.bias", {D}});
    } else {
      if (ts == kLearned) k.push_back({b + "norm1.emb.weight", {T, D}});
      k.push_back({b + "norm1.linear.weight", {2 * D, D}});
      k.push_back({b + "norm1.linear.bias", {2 * D}});
    }
    k.push_back({b + "norm2.weight", {D}});
    k.push_back({b + "norm2.bias", {D}});
  }
  static const char* names[8] = {"log_at", "log_bt", "log_ct", "log_cumprod_at", "log_cumprod_bt", "log_cumprod_ct", "log_1_min_ct", "log_1_min_cumprod_ct"};
  static const char* attrs[5] = {"c", "x", "y", "w", "h"};
  for (int s = 0; s < 8; ++s) {
    const int64_t n = (s >= 3 && s != 6) ? T + 1 : T;   // the cumulative products carry T + 1 entries
    if (c.q_type == LDM_Q_VANILLA) {
      k.push_back({names[s], {n}});   // vanilla.py:66-73: ONE un-prefixed set
    } else {
      for (int a = 0; a < 5; ++a) k.push_back({std::string(attrs[a]) + "_" + names[s], {n}});
    }
  }
  return k;
}

static KeyShapes as_map(const KeyList& k) {
  KeyShapes m(k.begin(), k.end());
  m["transformer.not_read.weight"] = {3, 3};   // a key nothing reads is nobody's business
  return m;
}

static int plan(const ldm_config& c, const KeyShapes& keys, WeightPlan& wp, std::string& err, int norm1 = LDM_NORM1_LAYER) {
  EnginePlan p;
  std::string e;
  if (plan_engine(c, Knobs{}, p, e, norm1)) {
    err = "plan_engine: " + e;
    return -99;
  }
  return plan_weights(c, p, keys, wp, err);
}

static void accepted(const char* id, const ldm_config& c, Pos pos, Ts ts, int norm1 = LDM_NORM1_LAYER, int pos_rows = 0) {
  const KeyList k = checkpoint(c, pos, ts, pos_rows);
  WeightPlan wp;
  std::string err;
  const int rc = plan(c, as_map(k), wp, err, norm1);
  printf("case=%s rc=%d pos_default=%d timestep_kind=%d reads=%zu err=%s\n", id, rc, (int)wp.pos_default, wp.timestep_kind, wp.reads.size(), err.c_str());
  CHECK(rc == 0, "%s: refused: %s", id, err.c_str());
  CHECK(wp.pos_default == (pos == kDefault) && wp.timestep_kind == (int)ts, "%s: variant", id);
  CHECK(wp.reads == k, "%s: the keys read, in reading order, with their shapes", id);
}

static void refused(const char* id, const ldm_config& c, const KeyShapes& keys, const std::string& msg, int norm1 = LDM_NORM1_LAYER) {
  WeightPlan wp;
  std::string err;
  const int rc = plan(c, keys, wp, err, norm1);
  printf("case=%s rc=%d err=%s\n", id, rc, err.c_str());
  CHECK(rc == -4 && err == msg, "%s: rc %d, message: %s", id, rc, err.c_str());
}

static void variants(const char* geo, ldm_config (*make)(int)) {
  auto id = [&](const char* v) { return std::string(geo) + "/" + v; };
  const ldm_config c = make(LDM_PREC_EXACT_F32);
  accepted(id("default").c_str(), c, kPair, kLearned);
  accepted(id("pos_default").c_str(), c, kDefault, kLearned);
  accepted(id("pos_default_longer_table").c_str(), c, kDefault, kLearned, LDM_NORM1_LAYER, 130);
  accepted(id("abs").c_str(), c, kPair, kAbs);
  accepted(id("none").c_str(), c, kPair, kNone);
  accepted(id("adainnorm").c_str(), c, kPair, kLearned, LDM_NORM1_INSTANCE);
  accepted(id("adainnorm_abs").c_str(), make(LDM_PREC_SPLIT_F16), kPair, kAbs, LDM_NORM1_INSTANCE);
  ldm_config v = make(LDM_PREC_SPLIT_F16);
  v.q_type = LDM_Q_VANILLA;
  accepted(id("vanilla").c_str(), v, kPair, kLearned);
  accepted(id("vanilla_pos_default").c_str(), v, kDefault, kLearned);
}

// ---- every refusal, the strings from the replaced ldm_finalize_weights (its `need` and its own h->fail calls)
static void refusals() {
  const ldm_config c = backbone(LDM_PREC_EXACT_F32);
  const KeyShapes good = as_map(checkpoint(c, kPair, kLearned));
  const std::string l0 = "transformer.backbone.layers.0.", l1 = "transformer.backbone.layers.1.";
  KeyShapes k = good;
  k.erase(l1 + "linear1.bias");
  refused("missing_key", c, k, "missing checkpoint key: transformer.backbone.layers.1.linear1.bias");
  k = good;
  k[l0 + "self_attn.in_proj_weight"] = {1392, 400};
  refused("wrong_shape", c, k, "checkpoint key transformer.backbone.layers.0.self_attn.in_proj_weight has shape (1392,400,) — does not match the configured geometry");
  k = good;
  k["transformer.head.0.bias"] = {};
  refused("scalar_shape", c, k, "checkpoint key transformer.head.0.bias has shape () — does not match the configured geometry");
  const char* kEither =
      "checkpoint must carry either transformer.pos_emb.pos_emb (pos_emb=default) or transformer.pos_emb.elem_emb + transformer.pos_emb.attr_emb "
      "(pos_emb=elem_attr): ";
  k = good;
  k["transformer.pos_emb.pos_emb"] = {125, 464};
  refused("pos_both", c, k, std::string(kEither) + "both are present");
  k.erase("transformer.pos_emb.elem_emb");   // attr_emb alone still counts as the pair
  refused("pos_both_half_a_pair", c, k, std::string(kEither) + "both are present");
  k = good;
  k.erase("transformer.pos_emb.elem_emb");
  k.erase("transformer.pos_emb.attr_emb");
  refused("pos_neither", c, k, std::string(kEither) + "neither is present");
  k = good;
  k.erase("transformer.pos_emb.attr_emb");
  refused("pos_half_a_pair", c, k, "missing checkpoint key: transformer.pos_emb.attr_emb");
  const char* kPosShape = "checkpoint key transformer.pos_emb.pos_emb must be (max_token_length >= 125, 464) — does not match the configured geometry";
  refused("pos_default_shorter_table", c, as_map(checkpoint(c, kDefault, kLearned, 124)), kPosShape);
  k = as_map(checkpoint(c, kDefault, kLearned));
  k["transformer.pos_emb.pos_emb"] = {125, 400};
  refused("pos_default_wrong_width", c, k, kPosShape);
  k["transformer.pos_emb.pos_emb"] = {125 * 464};
  refused("pos_default_flat", c, k, kPosShape);
  k = good;
  k[l0 + "norm1.emb.1.weight"] = {464, 1};
  k[l0 + "norm1.emb.3.weight"] = {464, 464};
  refused("mlp", c, k,
          "checkpoint key transformer.backbone.layers.0.norm1.emb.1.weight: timestep_type adalayernorm_mlp / adainnorm_mlp is not supported (the reference "
          "cannot run it either: its nn.Linear receives the integer timestep)");
  k = good;
  k[l0 + "norm1.weight"] = {464};
  refused("plain_and_linear", c, k,
          "checkpoint carries both transformer.backbone.layers.0.norm1.weight (timestep_type None) and transformer.backbone.layers.0.norm1.linear.weight (an Ada "
          "norm)");
  refused("none_on_instance_norm", c, as_map(checkpoint(c, kPair, kNone)),
          "checkpoint key transformer.backbone.layers.0.norm1.weight: timestep_type None is a LayerNorm, but the handle was created with LDM_NORM1_INSTANCE",
          LDM_NORM1_INSTANCE);
  k = as_map(checkpoint(c, kPair, kAbs));
  k.erase(l1 + "norm1.linear.bias");
  refused("abs_layer_disagrees", c, k, "missing checkpoint key: transformer.backbone.layers.1.norm1.linear.bias");
  k = as_map(checkpoint(c, kPair, kNone));
  k.erase(l1 + "norm1.weight");
  refused("none_layer_disagrees", c, k, "missing checkpoint key: transformer.backbone.layers.1.norm1.weight");
  k = good;
  k.erase("w_log_cumprod_ct");
  refused("schedule_constrained", c, k, "missing checkpoint key: w_log_cumprod_ct");
  k = good;
  k["c_log_at"] = {101};
  refused("schedule_length", c, k, "checkpoint key c_log_at has shape (101,) — does not match the configured geometry");
  ldm_config v = c;
  v.q_type = LDM_Q_VANILLA;
  k = as_map(checkpoint(v, kPair, kLearned));
  k.erase("log_1_min_ct");
  refused("schedule_vanilla", v, k, "missing checkpoint key: log_1_min_ct");
  refused("schedule_constrained_keys_on_vanilla", v, good, "missing checkpoint key: log_at");
  refused("schedule_vanilla_keys_on_constrained", c, as_map(checkpoint(v, kPair, kLearned)), "missing checkpoint key: c_log_at");
  // ---- two things wrong: the one read first is reported
  k = good;
  k.erase("transformer.cat_emb.weight");
  k["transformer.pos_emb.pos_emb"] = {125, 464};
  refused("order_embedding_before_positions", c, k, "missing checkpoint key: transformer.cat_emb.weight");
  k = good;
  k.erase("transformer.head.1.weight");
  k[l0 + "norm1.emb.1.weight"] = {464, 1};
  refused("order_head_before_norm1", c, k, "missing checkpoint key: transformer.head.1.weight");
  k = good;
  k[l0 + "norm1.emb.1.weight"] = {464, 1};
  k[l0 + "norm1.weight"] = {464};
  k.erase(l0 + "self_attn.in_proj_bias");
  refused("order_mlp_before_both_before_layers", c, k,
          "checkpoint key transformer.backbone.layers.0.norm1.emb.1.weight: timestep_type adalayernorm_mlp / adainnorm_mlp is not supported (the reference "
          "cannot run it either: its nn.Linear receives the integer timestep)");
  k = good;
  k.erase(l1 + "norm2.bias");
  k.erase("c_log_at");
  refused("order_layers_before_schedule", c, k, "missing checkpoint key: transformer.backbone.layers.1.norm2.bias");
  k = good;
  k.erase(l0 + "linear2.bias");
  k.erase(l1 + "self_attn.in_proj_weight");
  refused("order_layer_0_before_layer_1", c, k, "missing checkpoint key: transformer.backbone.layers.0.linear2.bias");
  {
    // *_abs where the sinusoid has no frequencies to step through: no configuration ldm_create accepts reaches it (d_model >= 16, a
    // multiple of 16), so the plan is asked directly, on a two-channel model
    ldm_config t = c;
    t.d_model = 2; t.n_head = 1; t.d_ff = 16; t.n_layer = 1;
    EnginePlan p;
    p.S = 125; p.C = 155;
    WeightPlan wp;
    std::string err;
    const int rc = plan_weights(t, p, as_map(checkpoint(t, kPair, kAbs)), wp, err);
    printf("case=abs_two_channels rc=%d err=%s\n", rc, err.c_str());
    CHECK(rc == -4 && err == "timestep_type *_abs needs an even d_model >= 4", "abs_two_channels: %s", err.c_str());
    const int rc2 = plan_weights(t, p, as_map(checkpoint(t, kPair, kLearned)), wp, err);
    CHECK(rc2 == 0, "learned_two_channels: %s", err.c_str());
  }
}

// ---- derived-buffer counts, from the replaced ldm_weights.cpp's allocation expressions.  Backbone: D 464, F 1856, H 8, L 4, T 100, C 155,
// Cp 160, S 125.  dalloc(hi / lo, round_up(N, 256) * Kp); image sizes: what the ldm_pack.h packer of that call returned
static void expect_counts(const char* id, const ldm_config& c, const Knobs& kn, const WeightCounts& e, Ts ts = kLearned) {
  EnginePlan p;
  std::string err;
  WeightPlan wp;
  int rc = plan_engine(c, kn, p, err);
  if (!rc) rc = plan_weights(c, p, as_map(checkpoint(c, kPair, ts)), wp, err);
  const WeightCounts& n = wp.counts;
  printf("counts=%s rc=%d pos=%zu adaln=%zu sinus=%zu sched=%zu w16=%zu/%zu/%zu/%zu/%zu x3=%zu/%zu/%zu/%zu pad=%zu/%zu/%zu ffn16=%zu generic=%zu/%zu/%zu/%zu/%zu b_in=%zu "
         "stack=%zu/%zu/%zu/%zu tbl=%zu/%zu/%zu/%zu\n",
         id, rc, n.pos, n.adaln, n.sinus, n.sched, n.w_in16, n.w_out16, n.w1_16, n.w2_16, n.head_w16, n.x3_qkv, n.x3_ffn1, n.x3_ffn2_slab, n.x3_head, n.x3_qkv_pad,
         n.b_in_pad, n.x3_out_kstep, n.ffn16_img, n.f_w_in, n.f_w_out, n.f_w1, n.f_w2, n.fast_head, n.f_b_in, n.attn_head_img_ks, n.ffn_img_pipe, n.b_out_v,
         n.head_img_ks, n.tbl_att_static, n.tbl_att_dyn, n.tbl_ffn, n.tbl_head);
  CHECK(rc == 0, "%s: %s", id, err.c_str());
  CHECK(n.pos == e.pos && n.adaln == e.adaln && n.sinus == e.sinus && n.sched == e.sched, "%s: tables", id);
  CHECK(n.w_in16 == e.w_in16 && n.w_out16 == e.w_out16 && n.w1_16 == e.w1_16 && n.w2_16 == e.w2_16 && n.head_w16 == e.head_w16, "%s: split copies", id);
  CHECK(n.x3_qkv == e.x3_qkv && n.x3_ffn1 == e.x3_ffn1 && n.x3_ffn2_slab == e.x3_ffn2_slab && n.x3_head == e.x3_head, "%s: row-resident images", id);
  CHECK(n.x3_qkv_pad == e.x3_qkv_pad && n.b_in_pad == e.b_in_pad && n.x3_out_kstep == e.x3_out_kstep && n.ffn16_img == e.ffn16_img, "%s: attention + out_proj images", id);
  CHECK(n.f_w_in == e.f_w_in && n.f_w_out == e.f_w_out && n.f_w1 == e.f_w1 && n.f_w2 == e.f_w2 && n.fast_head == e.fast_head && n.f_b_in == e.f_b_in, "%s: generic fp16 copies", id);
  CHECK(n.attn_head_img_ks == e.attn_head_img_ks && n.ffn_img_pipe == e.ffn_img_pipe && n.b_out_v == e.b_out_v && n.head_img_ks == e.head_img_ks, "%s: stack images", id);
  CHECK(n.tbl_att_static == e.tbl_att_static && n.tbl_att_dyn == e.tbl_att_dyn && n.tbl_ffn == e.tbl_ffn && n.tbl_head == e.tbl_head, "%s: loop tables", id);
  CHECK(wp.loop_tables() == (e.tbl_att_dyn != 0), "%s: loop_tables()", id);
}

static void counts() {
  const Knobs none;
  WeightCounts base;   // what every engine builds on the backbone: pos [S][D], adaln [T][L][2 D], sched [8][5][T + 1]
  base.pos = 125 * 464; base.adaln = 100 * 4 * 2 * 464; base.sched = 8 * 5 * 101;
  WeightCounts small_base;
  small_base.pos = 125 * 256; small_base.adaln = 20 * 2 * 2 * 256; small_base.sched = 8 * 5 * 21;
  {
    // stack: pack_ffn_image_pipelined (F / 32 + 1 = 59 stages of 64 KiB), pack_attn_head_image (8 heads x 8 + 2 stages of 32 KiB), bias [3 * 512],
    // b_out_v [D], pack_head_image (Cp / 32 = 5 tiles of 32 KiB); tables [L][1536], [T][L][1536], [L][3584], [1536]
    WeightCounts e = base;
    e.ffn_img_pipe = 59 * 32768; e.attn_head_img_ks = 66 * 16384; e.f_b_in = 1536; e.b_out_v = 464; e.head_img_ks = 5 * 16384;
    e.tbl_att_static = 4 * 1536; e.tbl_att_dyn = 100 * 4 * 1536; e.tbl_ffn = 4 * 3584; e.tbl_head = 1536;
    expect_counts("fast", backbone(LDM_PREC_FAST_F16), none, e);
  }
  {
    // generic fast, small: HD = Dq = 256, Fq = 1024: pack_w16(Np = round_up(3 HD, 256) = 768, Dq), (256, HD), (1024, Dq), (256, Fq), head (256, Dq)
    WeightCounts e = small_base;
    e.f_w_in = 768 * 256; e.f_w_out = 256 * 256; e.f_w1 = 1024 * 256; e.f_w2 = 256 * 1024; e.fast_head = 256 * 256; e.f_b_in = 768;
    expect_counts("fast_generic_geometry", small(LDM_PREC_FAST_F16), none, e);
  }
  expect_counts("exact", backbone(LDM_PREC_EXACT_F32), none, base);
  // split-type on the backbone: Dp 512, Fp 1856; make_w16: round_up(1392, 256) = 1536, round_up(464, 256) = 512, round_up(1856, 256) = 2048,
  // round_up(155, 256) = 256 rows
  WeightCounts tiled = base;
  tiled.w_in16 = 1536 * 512; tiled.w_out16 = 512 * 512; tiled.w1_16 = 2048 * 512; tiled.w2_16 = 512 * 1856; tiled.head_w16 = 256 * 512;
  // row-resident: pack_x3_tile_image of 44 / 58 / 6 tiles (64 KiB each), pack_x3_slab_image of x3_slab_stages(1856) = 60 stages
  WeightCounts row = tiled;
  row.x3_qkv = 44 * 32768; row.x3_ffn1 = 58 * 32768; row.x3_head = 6 * 32768; row.x3_ffn2_slab = 60 * 32768;
  // attention + out_proj: 3 * 8 * 2 = 48 tiles, bias [3 * 8 * 64], pack_x3_kstep_image 8 heads x 4 stages of 32 KiB
  WeightCounts split = row;
  split.x3_qkv_pad = 48 * 32768; split.b_in_pad = 1536; split.x3_out_kstep = 32 * 16384;
  WeightCounts hybrid = split;
  hybrid.ffn16_img = 59 * 32768;
  expect_counts("split", backbone(LDM_PREC_SPLIT_F16), none, split);
  expect_counts("mixed", backbone(LDM_PREC_MIXED_F16), none, split);
  expect_counts("hybrid", backbone(LDM_PREC_HYBRID_F16), none, hybrid);
  {
    Knobs k; k.x3_lngemm = 0;
    expect_counts("split_lngemm_0", backbone(LDM_PREC_SPLIT_F16), k, tiled);
  }
  {
    Knobs k; k.x3_attnout = 0;
    expect_counts("split_attnout_0", backbone(LDM_PREC_SPLIT_F16), k, row);
  }
  {
    Knobs k; k.x3_hidpanel = 0;
    expect_counts("split_hidpanel_0", backbone(LDM_PREC_SPLIT_F16), k, split);
  }
  {
    Knobs k; k.hyb_ffn = 0;
    expect_counts("hybrid_ffn_0", backbone(LDM_PREC_HYBRID_F16), k, split);
  }
  {
    WeightCounts e = small_base;   // Dp 256, Fp 1024, tiled
    e.w_in16 = 768 * 256; e.w_out16 = 256 * 256; e.w1_16 = 1024 * 256; e.w2_16 = 256 * 1024; e.head_w16 = 256 * 256;
    expect_counts("split_generic_geometry", small(LDM_PREC_SPLIT_F16), none, e);
  }
  {
    // wide vocabulary: 64 bins, 283 classes, Cp 288: the head's copies grow to round_up(283, 256) = 512 rows, its image to x3_tiles(288) = 10 tiles
    ldm_config c = backbone(LDM_PREC_SPLIT_F16);
    c.n_bin = 64;
    WeightCounts e = split;
    e.head_w16 = 512 * 512; e.x3_head = 10 * 32768;
    expect_counts("split_bins64", c, none, e);
  }
  {
    WeightCounts e = split;   // *_abs: the sinusoid [T][D]
    e.sinus = 100 * 464;
    expect_counts("split_abs", backbone(LDM_PREC_SPLIT_F16), none, e, kAbs);
  }
}

static int cast(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 2;
  std::vector<float> w;
  float x;
  while (fread(&x, 4, 1, f) == 1) w.push_back(x);
  fclose(f);
  const float scale = split_scale(w.data(), w.size());
  std::vector<uint16_t> hi(w.size()), lo(w.size());
  for (size_t i = 0; i < w.size(); ++i) split_f16(w[i], scale, hi[i], lo[i]);
  f = fopen(out, "wb");
  if (!f) return 2;
  fwrite(&scale, 4, 1, f);
  fwrite(hi.data(), 2, hi.size(), f);
  fwrite(lo.data(), 2, lo.size(), f);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "table")) {
    variants("backbone", backbone);
    variants("small", small);
    refusals();
    counts();
    printf("failed=%d\n", g_failed);
    return g_failed ? 1 : 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "cast")) return cast(argv[2], argv[3]);
  fprintf(stderr, "usage: %s table | cast in.bin out.bin\n", argv[0]);
  return 2;
}
