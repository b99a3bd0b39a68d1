// What a checkpoint is to a handle, decided in ONE place: plan_weights maps (ldm_config, EnginePlan, the checkpoint's key -> shape map) to
// the denoiser variant the key set names, the keys ldm_finalize_weights reads with their shapes, and the element count of every buffer it
// derives — or to the refusal ldm_finalize_weights reports.  Pure host code: no HIP, no environment, no allocation on a device, so
// tests/cpu_weight_plan_check.cpp pins the variants, every refusal byte for byte and the counts on the CPU.  Several kernels load whole
// weight tiles without bounds checks: ldm_weights.cpp uploads a buffer only where its size IS the plan's count.
// Also here, for the same reason: the split mode's scale rule and fp32 -> fp16 as host arithmetic (ldm_weights.cpp takes the scale and the
// fast mode's fp16 copies from them; the hi / lo cast of 10^7 weights stays on the device, and split_f16 states what it computes).
#pragma once
#include "ldm_engine_plan.h"
#include "ldm_pack.h"
#include "ldm_variant_core.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace ldm {

// ---- fp32 -> fp16, round to nearest even, and back: the bits of the device's conversions.  Written without branches — selects between
// results that are all computed — so that the cast loops of ldm_weights.cpp vectorise: a checkpoint is 10^7 weights.
inline uint16_t f16_bits(float x) {
  uint32_t u, s;
  memcpy(&u, &x, 4);
  const uint32_t sign = u & 0x80000000u;
  u ^= sign;
  // normal fp16 (>= 2^-14): exponent bias 127 -> 15, round to nearest even on the 13 bits that go (a carry moves into the exponent:
  // 65 520 and above, the tie included, come out as infinity)
  const uint32_t normal = (u - 0x38000000u + 0xfffu + ((u >> 13) & 1u)) >> 13;
  // subnormal fp16: |x| + 0.5 has an ulp of 2^-24, fp16's subnormal spacing — the addition rounds to nearest even and leaves the count
  // of 2^-24 units (up to 1024, the smallest normal number) in the low bits
  float f;
  memcpy(&f, &u, 4);
  f += 0.5f;
  memcpy(&s, &f, 4);
  uint32_t r = u < 0x38800000u ? s - 0x3f000000u : normal;
  r = u >= 0x47800000u ? 0x7c00u : r;   // 2^16 and above, infinity
  r = u > 0x7f800000u ? 0x7e00u : r;    // NaN, quiet
  return (uint16_t)((sign >> 16) | r);
}
inline float f16_float(uint16_t h) {
  const uint32_t em = h & 0x7fffu;
  uint32_t u = (em << 13) + 0x38000000u;               // normal: exponent bias 15 -> 127
  u = em >= 0x7c00u ? u | 0x7f800000u : u;             // infinity, NaN
  const float sub = (float)(int32_t)em * 5.9604644775390625e-08f;   // subnormal: the mantissa in units of 2^-24 (exact)
  float x;
  memcpy(&x, &u, 4);
  x = em < 0x400u ? sub : x;
  return h & 0x8000u ? -x : x;
}

// ---- split mode: a weight tensor as fp16 hi + lo.  The weights are multiplied by the exact power of two 2^k that brings max |w| into
// [1, 2) before the split — lo is stored unscaled (kSplitLoScale = 1) and fp16's denormal spacing 2^-24 must be small against the weights
// — and 1 / scale = 2^-k goes to the GEMM's epilogue.  1 where the maximum is 0 or not finite.
inline float split_scale(const float* w, size_t n) {
  uint32_t top = 0;   // max |w| as its bit pattern, which orders as the value does; a NaN takes no part (as in std::max(mx, |w|))
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    memcpy(&u, &w[i], 4);
    u &= 0x7fffffffu;
    u = u > 0x7f800000u ? 0u : u;
    top = u > top ? u : top;
  }
  float mx;
  memcpy(&mx, &top, 4);
  return mx > 0.f && std::isfinite(mx) ? std::ldexp(1.0f, -(int)std::floor(std::log2(mx))) : 1.0f;
}
// x = w * scale (exact: a power of two), hi = fp16(x), lo = fp16(x - hi): what cast_f32_f16 (kernels_norm.hip) computes on the device for
// ldm_weights.cpp make_split16.  The host statement of it, held against NumPy's float16 by tests/test_weight_plan.py; no load runs it (18 ms
// of one host thread per checkpoint against a device cast that costs nothing: profiles/weights_refactor_parent_vs_change.txt)
inline void split_f16(float w, float scale, uint16_t& hi, uint16_t& lo) {
  const float x = w * scale;
  hi = f16_bits(x);
  lo = f16_bits(x - f16_float(hi));
}

// ---- the plan
using KeyShapes = std::map<std::string, std::vector<int64_t>>;   // checkpoint keys, prefix stripped -> shape

enum TimestepKind { kTimestepLearned = 0, kTimestepAbs = 1, kTimestepNone = 2 };   // norm1.emb.weight | the sinusoid | nn.LayerNorm, constant in t

// Element counts of what ldm_finalize_weights derives (ldm_handle.h names the members), 0 = this engine does not build it.  Members of
// LayerW / FastLayer: of ONE layer.  fp16 images count halves, tables floats.
struct WeightCounts {
  size_t pos = 0, adaln = 0, sinus = 0, sched = 0;                            // every engine (sinus: timestep_type *_abs)
  size_t w_in16 = 0, w_out16 = 0, w1_16 = 0, w2_16 = 0, head_w16 = 0;         // split-type: [round_up(N, 256)][Kp], hi and lo EACH
  size_t x3_qkv = 0, x3_ffn1 = 0, x3_ffn2_slab = 0, x3_head = 0;              // RowResident: hi | lo tile images, linear2's K-slab image
  size_t x3_qkv_pad = 0, b_in_pad = 0, x3_out_kstep = 0;                      // attnout: head-padded in_proj (+ bias), out_proj's k-step image
  size_t ffn16_img = 0;                                                       // ffn_fused: the plain-fp16 chunk image
  size_t f_w_in = 0, f_w_out = 0, f_w1 = 0, f_w2 = 0, fast_head = 0;          // Generic16: head-padded fp16 copies
  size_t f_b_in = 0;                                                          // fast: head-padded in_proj bias
  size_t attn_head_img_ks = 0, ffn_img_pipe = 0, b_out_v = 0, head_img_ks = 0;   // Stack: LDS images, b_out + W_out b_v
  size_t tbl_att_static = 0, tbl_att_dyn = 0, tbl_ffn = 0, tbl_head = 0;      // Stack with the loop kernel's geometry: its parameter tables
};

struct WeightPlan {
  bool pos_default = false;   // transformer.pos_emb.pos_emb instead of the elem_emb / attr_emb pair
  int timestep_kind = kTimestepLearned;
  std::vector<std::pair<std::string, std::vector<int64_t>>> reads;   // every key the build reads, once, in reading order, with its shape
  WeightCounts counts;
  bool loop_tables() const { return counts.tbl_att_dyn != 0; }
};

inline WeightCounts count_weights(const ldm_config& cfg, const EnginePlan& p, int timestep_kind) {
  const size_t D = cfg.d_model, F = cfg.d_ff, H = cfg.n_head, L = cfg.n_layer, T = cfg.n_step, C = p.C;
  auto rows = [](size_t n) { return (size_t)round_up((int)n, 256); };   // whole 128-row tiles: the LDS-DMA GEMMs load W without bounds checks
  const size_t stage = 16384;                                          // halves of a 32-KiB LDS stage
  WeightCounts c;
  c.pos = (size_t)p.S * D;
  c.adaln = T * L * 2 * D;
  c.sinus = timestep_kind == kTimestepAbs ? T * D : 0;
  c.sched = (size_t)kSchedRows * cfg.n_attr * (T + 1);
  if (p.split_type()) {
    c.w_in16 = rows(3 * D) * p.Dp;
    c.w_out16 = rows(D) * p.Dp;
    c.w1_16 = rows(F) * p.Dp;
    c.w2_16 = rows(D) * p.Fp;
    c.head_w16 = rows(C) * p.Dp;
    if (p.structure == Structure::RowResident) {
      c.x3_qkv = (size_t)p.x3_qkv_tiles * 2 * stage;
      c.x3_ffn1 = (size_t)p.x3_ffn1_tiles * 2 * stage;
      c.x3_ffn2_slab = (size_t)((p.Fp / 32 + 2) / 3 * 3) * 2 * stage;   // one stage per 32 k, rounded up to the three the kernel walks at a time
      c.x3_head = (size_t)p.x3_head_tiles * 2 * stage;
    }
    if (p.attnout) {
      c.x3_qkv_pad = 3 * H * 2 * 2 * stage;
      c.b_in_pad = 3 * H * 64;
      c.x3_out_kstep = H * 4 * stage;
    }
    if (p.ffn_fused) c.ffn16_img = (F / 32 + 1) * 2 * stage;
  } else if (p.fast()) {
    c.f_b_in = (size_t)3 * p.HD;
    if (p.structure == Structure::Stack) {
      c.attn_head_img_ks = (H * 8 + 2) * stage;
      c.ffn_img_pipe = (F / 32 + 1) * 2 * stage;
      c.b_out_v = D;
      c.head_img_ks = (size_t)p.Cp / 32 * stage;
      if (H * 64 * 3 == (size_t)kStackTblAttStatic && D <= 512 && F <= 2048) {
        c.tbl_att_static = L * kStackTblAttStatic;
        c.tbl_att_dyn = T * L * kStackTblAttDyn;
        c.tbl_ffn = L * kStackTblFfn;
        c.tbl_head = kStackTblAttDyn;
      }
    } else {
      c.f_w_in = rows((size_t)3 * p.HD) * p.Dq;
      c.f_w_out = rows(D) * p.HD;
      c.f_w1 = rows(F) * p.Dq;
      c.f_w2 = rows(D) * p.Fq;
      c.fast_head = rows(C) * p.Dq;
    }
  }
  return c;
}

// schedule row k (ldm_kernels.h ScheduleRow) of attribute a: its checkpoint key — vanilla.py:66-73 registers ONE un-prefixed set, which is
// replicated into every attribute's row — and its length (the cumulative rows carry T + 1 entries)
inline std::string sched_key(const ldm_config& cfg, int k, int a) {
  static const char* names[kSchedRows] = {"log_at",         "log_bt",         "log_ct",       "log_cumprod_at",
                                          "log_cumprod_bt", "log_cumprod_ct", "log_1_min_ct", "log_1_min_cumprod_ct"};
  static const char* attrs[5] = {"c", "x", "y", "w", "h"};
  return cfg.q_type == LDM_Q_VANILLA ? std::string(names[k]) : std::string(attrs[a]) + "_" + names[k];
}
inline int64_t sched_len(const ldm_config& cfg, int k) { return k == 3 || k == 4 || k == 5 || k == 7 ? cfg.n_step + 1 : cfg.n_step; }

// 0 and the plan, or ldm_finalize_weights' return code (-4) and message: the first thing wrong in the order the keys are read
inline int plan_weights(const ldm_config& cfg, const EnginePlan& p, const KeyShapes& keys, WeightPlan& wp, std::string& err) {
  wp = WeightPlan{};
  const int64_t D = cfg.d_model, F = cfg.d_ff, C = p.C, T = cfg.n_step;
  const std::string tr = "transformer.";
  auto refuse = [&](const std::string& msg) {
    err = msg;
    return -4;
  };
  auto has = [&](const std::string& key) { return keys.count(key) != 0; };
  auto need = [&](const std::string& key, std::vector<int64_t> want) {
    auto it = keys.find(key);
    if (it == keys.end()) return refuse("missing checkpoint key: " + key);
    if (it->second != want) {
      std::string got;
      for (auto s : it->second) got += std::to_string(s) + ",";
      return refuse("checkpoint key " + key + " has shape (" + got + ") — does not match the configured geometry");
    }
    for (const auto& r : wp.reads)
      if (r.first == key) return 0;   // (q_type vanilla reads its one schedule set for every attribute)
    wp.reads.emplace_back(key, std::move(want));
    return 0;
  };
  int rc;
  if ((rc = need(tr + "cat_emb.weight", {C, D}))) return rc;
  // pos_emb: ElementPositionalEmbedding (elem_emb + attr_emb, nn_lib.py:91-127) or PositionalEmbedding (one learned table whose first S
  // rows are the positions, nn_lib.py:73-88) — a checkpoint carries exactly one of the two
  wp.pos_default = has(tr + "pos_emb.pos_emb");
  if (wp.pos_default == (has(tr + "pos_emb.elem_emb") || has(tr + "pos_emb.attr_emb")))
    return refuse("checkpoint must carry either " + tr + "pos_emb.pos_emb (pos_emb=default) or " + tr + "pos_emb.elem_emb + " + tr +
                  "pos_emb.attr_emb (pos_emb=elem_attr): " + (wp.pos_default ? "both are present" : "neither is present"));
  if (wp.pos_default) {
    const std::vector<int64_t>& s = keys.at(tr + "pos_emb.pos_emb");
    if (s.size() != 2 || s[1] != D || s[0] < p.S)
      return refuse("checkpoint key " + tr + "pos_emb.pos_emb must be (max_token_length >= " + std::to_string(p.S) + ", " + std::to_string(D) +
                    ") — does not match the configured geometry");
    wp.reads.emplace_back(tr + "pos_emb.pos_emb", s);
  } else {
    if ((rc = need(tr + "pos_emb.elem_emb", {cfg.max_elem, D}))) return rc;
    if ((rc = need(tr + "pos_emb.attr_emb", {cfg.n_attr, D}))) return rc;
  }
  if ((rc = need(tr + "head.0.weight", {D}))) return rc;
  if ((rc = need(tr + "head.0.bias", {D}))) return rc;
  if ((rc = need(tr + "head.1.weight", {C, D}))) return rc;
  // timestep_type, from layer 0's norm1 keys (every layer must then agree: `need` below names what is missing):
  //   norm1.emb.weight          adalayernorm / adainnorm          the learned [T][D] embedding
  //   norm1.linear.* alone      adalayernorm_abs / adainnorm_abs  the sinusoid, built once for all layers (ldm_variant_core.h)
  //   norm1.weight / .bias      None                              nn.LayerNorm: the table holds w - 1 | b at every t
  //   norm1.emb.<n>.*           *_mlp                             refused: the reference feeds the Long timestep to nn.Linear and raises
  const std::string n1 = tr + "backbone.layers.0.norm1.";
  for (const auto& kv : keys)
    if (kv.first.compare(0, n1.size() + 4, n1 + "emb.") == 0 && kv.first != n1 + "emb.weight")
      return refuse("checkpoint key " + kv.first + ": timestep_type adalayernorm_mlp / adainnorm_mlp is not supported (the reference cannot run it either: its "
                    "nn.Linear receives the integer timestep)");
  const bool plain = has(n1 + "weight");
  if (plain && has(n1 + "linear.weight"))
    return refuse("checkpoint carries both " + n1 + "weight (timestep_type None) and " + n1 + "linear.weight (an Ada norm)");
  wp.timestep_kind = plain ? kTimestepNone : has(n1 + "emb.weight") ? kTimestepLearned : kTimestepAbs;
  if (plain && p.instance_norm)
    return refuse("checkpoint key " + n1 + "weight: timestep_type None is a LayerNorm, but the handle was created with LDM_NORM1_INSTANCE");
  if (wp.timestep_kind == kTimestepAbs && !ldm_variant::sinusoid_args_ok((int)T, (int)D)) return refuse("timestep_type *_abs needs an even d_model >= 4");
  for (int i = 0; i < cfg.n_layer; ++i) {
    const std::string b = tr + "backbone.layers." + std::to_string(i) + ".";
    if ((rc = need(b + "self_attn.in_proj_weight", {3 * D, D}))) return rc;
    if ((rc = need(b + "self_attn.in_proj_bias", {3 * D}))) return rc;
    if ((rc = need(b + "self_attn.out_proj.weight", {D, D}))) return rc;
    if ((rc = need(b + "self_attn.out_proj.bias", {D}))) return rc;
    if ((rc = need(b + "linear1.weight", {F, D}))) return rc;
    if ((rc = need(b + "linear1.bias", {F}))) return rc;
    if ((rc = need(b + "linear2.weight", {D, F}))) return rc;
    if ((rc = need(b + "linear2.bias", {D}))) return rc;
    if (wp.timestep_kind == kTimestepNone) {
      if ((rc = need(b + "norm1.weight", {D}))) return rc;
      if ((rc = need(b + "norm1.bias", {D}))) return rc;
    } else {
      if (wp.timestep_kind == kTimestepLearned && (rc = need(b + "norm1.emb.weight", {T, D}))) return rc;
      if ((rc = need(b + "norm1.linear.weight", {2 * D, D}))) return rc;
      if ((rc = need(b + "norm1.linear.bias", {2 * D}))) return rc;
    }
    if ((rc = need(b + "norm2.weight", {D}))) return rc;
    if ((rc = need(b + "norm2.bias", {D}))) return rc;
  }
  // schedule buffers are taken from the checkpoint, not recomputed
  for (int k = 0; k < kSchedRows; ++k)
    for (int a = 0; a < cfg.n_attr; ++a)
      if ((rc = need(sched_key(cfg, k, a), {sched_len(cfg, k)}))) return rc;
  wp.counts = count_weights(cfg, p, wp.timestep_kind);
  return 0;
}

}  // namespace ldm
