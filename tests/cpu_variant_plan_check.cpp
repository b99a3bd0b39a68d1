// Host check of what layout_dm_amd/csrc/ldm_engine_plan.h decides for the norm1 kind (ldm_create_variant, include/ldm_hip.h LDM_NORM1_*),
// built with plain g++ (and as the ASan + UBSan build) and run as its own process by tests/test_denoiser_variants.py.  One line per case.
//   instance   LDM_NORM1_INSTANCE: exact and split run the tiled sequence (on the reference's backbone too, where split otherwise runs the
//              row-resident launches), with the sizes of the tiled plan of the same configuration; fast / mixed / hybrid are refused, byte for byte,
//              behind the device probe; an unknown kind is refused
//   default    LDM_NORM1_LAYER passed explicitly gives, field for field, the plan of the four-argument call: every configuration of
//              tests/cpu_engine_plan_check.cpp's table, accepted or refused, knob rows included
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

static bool same_plan(const EnginePlan& a, const EnginePlan& b) {
  return a.precision == b.precision && a.structure == b.structure && a.describe_kernels() == b.describe_kernels() && a.attnout == b.attnout &&
         a.hid_panels == b.hid_panels && a.ffn_fused == b.ffn_fused && a.w2p == b.w2p && a.np_w == b.np_w && a.np_ffn == b.np_ffn &&
         a.stack_loop == b.stack_loop && a.rel_loop == b.rel_loop && a.step0_cache == b.step0_cache && a.loop_geometry == b.loop_geometry &&
         a.rel_loop_geometry == b.rel_loop_geometry && a.S == b.S && a.C == b.C && a.Cp == b.Cp && a.Dp == b.Dp && a.Fp == b.Fp && a.dh == b.dh &&
         a.Dq == b.Dq && a.HD == b.HD && a.Fq == b.Fq && a.x3_qkv_tiles == b.x3_qkv_tiles && a.x3_ffn1_tiles == b.x3_ffn1_tiles &&
         a.x3_head_tiles == b.x3_head_tiles && a.chunk == b.chunk && a.n_lanes == b.n_lanes && a.lane_offset_us == b.lane_offset_us &&
         a.balanced_chunks == b.balanced_chunks && a.panel_rows == b.panel_rows && a.per_layout_t() == b.per_layout_t() &&
         !memcmp(&a.ws, &b.ws, sizeof(a.ws)) && !memcmp(&a.bufs, &b.bufs, sizeof(a.bufs));
}

static const char* kRefusal[5] = {
    nullptr,
    "precision fast: timestep_type adainnorm / adainnorm_abs (instance norm over a layout's rows) has no kernel in the fp16 engines; use precision split or exact",
    nullptr,
    "precision mixed: timestep_type adainnorm / adainnorm_abs (instance norm over a layout's rows) has no kernel in the fp16 engines; use precision split or exact",
    "precision hybrid: timestep_type adainnorm / adainnorm_abs (instance norm over a layout's rows) has no kernel in the fp16 engines; use precision split or exact",
};

static int instance() {
  const Knobs none;
  for (int max_batch : {8, 512})
    for (int prec : {LDM_PREC_EXACT_F32, LDM_PREC_SPLIT_F16}) {
      for (bool reference_backbone : {true, false}) {
        const ldm_config c = reference_backbone ? backbone(prec, max_batch) : small(prec, max_batch);
        EnginePlan p, tiled;
        std::string err, err2;
        const int rc = plan_engine(c, none, p, err, LDM_NORM1_INSTANCE);
        printf("case=instance_%d_%d_%d rc=%d structure=%d kernels=%s\n", prec, max_batch, (int)reference_backbone, rc, (int)p.structure, p.describe_kernels().c_str());
        CHECK(rc == 0 && p.instance_norm && p.structure == Structure::Tiled, "precision %d: rc %d %s", prec, rc, err.c_str());
        CHECK(p.describe_kernels() == "tiled_gemm+attn+instance_norm", "%s", p.describe_kernels().c_str());
        CHECK(!p.attnout && !p.hid_panels && !p.ffn_fused && !p.w2p && p.np_w == 3 && p.np_ffn == 3 && p.per_layout_t(), "precision %d: options", prec);
        // the tiled plan of the same configuration (split on the backbone: the row-resident launches switched off) has the same sizes
        Knobs k;
        k.x3_lngemm = 0;
        const int rc2 = plan_engine(c, k, tiled, err2);
        CHECK(rc2 == 0 && tiled.structure == Structure::Tiled && !tiled.instance_norm, "precision %d: the tiled plan", prec);
        CHECK(!memcmp(&p.ws, &tiled.ws, sizeof(p.ws)) && !memcmp(&p.bufs, &tiled.bufs, sizeof(p.bufs)) && p.chunk == tiled.chunk &&
                  p.n_lanes == tiled.n_lanes && p.Dp == tiled.Dp && p.Fp == tiled.Fp && p.panel_rows == tiled.panel_rows,
              "precision %d: sizes of the tiled plan", prec);
      }
    }
  for (int prec : {LDM_PREC_FAST_F16, LDM_PREC_MIXED_F16, LDM_PREC_HYBRID_F16}) {
    const ldm_config c = backbone(prec);
    EnginePlan p;
    std::string err, early;
    const int rc = plan_engine(c, none, p, err, LDM_NORM1_INSTANCE);
    printf("case=instance_refused_%d rc=%d err=%s\n", prec, rc, err.c_str());
    CHECK(rc == -1 && err == kRefusal[prec], "precision %d: %s", prec, err.c_str());
    CHECK(validate_config(c, none.refused, early) == 0, "precision %d: the refusal waits behind the device probe", prec);
  }
  {
    EnginePlan p;
    std::string err;
    const int rc = plan_engine(backbone(LDM_PREC_EXACT_F32), none, p, err, 2);
    printf("case=kind_2 rc=%d err=%s\n", rc, err.c_str());
    CHECK(rc == -1 && err == "unknown norm1 kind", "%s", err.c_str());
    // validate_config's refusals still come first
    ldm_config c = backbone(LDM_PREC_FAST_F16);
    c.max_batch = 0;
    CHECK(plan_engine(c, none, p, err, LDM_NORM1_INSTANCE) == -1 && err == "max_batch must be >= 1", "%s", err.c_str());
  }
  return g_failed;
}

// every configuration of cpu_engine_plan_check.cpp's table
struct Row {
  const char* id;
  ldm_config c;
  Knobs k;
};
static std::vector<Row> rows;
__attribute__((noinline)) static void add(const char* id, const ldm_config& c, const Knobs& k = Knobs{}) { rows.push_back({id, c, k}); }

static int defaults() {
  for (int prec = 0; prec < 5; ++prec) {
    add("backbone_8", backbone(prec, 8));
    add("backbone_256", backbone(prec));
    add("backbone_512", backbone(prec, 512));
    add("small_8", small(prec, 8));
    add("small_256", small(prec));
    ldm_config c = backbone(prec);
    c.n_bin = 64;
    add("n_bin64", c);
    for (int me : {12, 13, 19, 20, 26}) {
      c = backbone(prec);
      c.max_elem = me;
      add("max_elem", c);
      c.max_batch = 8;
      add("max_elem_8", c);
    }
    c = backbone(prec);
    c.d_ff = 1840;
    add("dff1840", c);
    c = backbone(prec);
    c.q_type = LDM_Q_VANILLA;
    add("vanilla", c);
    Knobs k;
    k.x3_lngemm = 0; add("lngemm_0", backbone(prec, 8), k);
    k = Knobs{}; k.x3_attnout = 0; add("attnout_0", backbone(prec, 8), k);
    k = Knobs{}; k.x3_hidpanel = 0; add("hidpanel_0", backbone(prec, 8), k);
    k = Knobs{}; k.hyb_ffn = 0; add("hyb_ffn_0", backbone(prec, 8), k);
    k = Knobs{}; k.stack_kernel = 0; add("fused_attn_0", backbone(prec, 200), k);
    k = Knobs{}; k.chunk = 64; k.lanes = 7; k.lane_offset_us = -3; k.balanced_chunks = 0; k.stack_loop = 0; add("overrides", backbone(prec, 200), k);
    k = Knobs{}; k.rel_loop = 0; k.step0_cache = 0; add("rel_loop_0", backbone(prec), k);
  }
  {
    ldm_config c = backbone(LDM_PREC_FAST_F16);
    c.abi_version = LDM_ABI_VERSION + 1; add("abi", c);
    c = backbone(LDM_PREC_FAST_F16); c.n_bin = 129; c.precision = 9; add("bins_129", c);
    c.n_bin = 128; c.n_category = 63; add("classes_577", c);
    c.n_bin = 32; c.n_category = 25; add("precision_9", c);
    c = backbone(LDM_PREC_EXACT_F32); c.max_batch = 0; add("max_batch_0", c);
    c = backbone(LDM_PREC_EXACT_F32); c.max_elem = 2000; add("too_long", c);
    c = backbone(LDM_PREC_EXACT_F32); c.q_type = 7; add("q_type", c);
    Knobs k; k.refused = "LDM_CHUNK"; add("knob_outside_dev", backbone(LDM_PREC_EXACT_F32), k);
  }
  for (const Row& r : rows) {
    EnginePlan a, b;
    std::string ea, eb;
    const int ra = plan_engine(r.c, r.k, a, ea), rb = plan_engine(r.c, r.k, b, eb, LDM_NORM1_LAYER);
    CHECK(ra == rb && ea == eb && same_plan(a, b) && !a.instance_norm && !b.instance_norm, "%s precision %d", r.id, r.c.precision);
    CHECK(a.describe_kernels().find("instance_norm") == std::string::npos, "%s: %s", r.id, a.describe_kernels().c_str());
  }
  printf("default cases=%zu failed=%d\n", rows.size(), g_failed);
  return g_failed;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "instance")) return instance() ? 1 : 0;
  if (argc >= 2 && !strcmp(argv[1], "default")) return defaults() ? 1 : 0;
  fprintf(stderr, "usage: %s instance | default\n", argv[0]);
  return 2;
}
