// cond= inputs from raw layouts — LayoutSequenceTokenizer.encode + BboxTokenizer.encode (helpers/layout_tokenizer.py:208-253,
// helpers/bbox_tokenizer.py:84-115, helpers/clustering.py:43-55), the per-token rules of get_cond (helpers/task.py:27-151) and
// the pair walk of AddCanvasElement + AddRelationConstraints (data/util.py:111-177, use_v1=False) — ONE source of the
// arithmetic, compiled for the device (kernels_cond.hip) and for the host (tests/cpu_cond_check.cpp).
//
// Scope: the LayoutDM tokenizer configuration the device-side decode assumes — var_order c-x-y-w-h, stacked x-y-w-h bbox
// vocabulary, special tokens [pad, mask], pad_until_max, no bos / eos, sort_by=None.
//
// Quantisation of one coordinate (k = 0..3 for x, y, w, h), templated on the box type TB (float, double):
//   * linear      torch's operation order in TB: d = TB(1 / N) (a Python double rounded to the tensor's dtype, as torch does
//                 with a scalar); x, y: clamp(v, 0, TB(1 - 1/N)); w, h: clamp(v, d, 1) - d; then TB(N) * q, rounded half to
//                 even (rint).  Every product is rounded (no FMA contraction: see the pragma below).
//   * percentile  clip to [0, 1], cast to float32, |c - x| in float32 over the sorted float32 centres (the reference's -1
//                 sentinel centres included), first minimum wins (numpy argmin).
//   * kmeans      x cast to float32; the nearest sorted centre by |x - c| evaluated in float64, lowest index on a tie.
//                 sklearn's predict evaluates c^2 - 2xc through BLAS in float32 and is not reproducible bit for bit AT a
//                 midpoint of two centres; away from midpoints both name the same centre.
// token = n_category + k * N + bin; every token of a padding slot (label and box) is pad_id.
//
// Error bits (an int32 word the call zeroes): kErrPrefix — a layout's mask is not a prefix (the reference asserts,
// layout_tokenizer.py:230-232); kErrNonFinite — a valid element has a NaN / infinite coordinate; kErrLabel — a valid
// element's label lies outside [0, n_category).
//
// Own draws (no keep mask / noise / selection supplied): Philox4x32-10 of ldm_post_token.h, counter = (slot, purpose,
// global layout index lo, hi), key = seed — independent of batch cuts and rank count, like the sampler's.  They reproduce the
// DISTRIBUTIONS of the reference's random / torch draws (task.py:62-75,127; data/util.py:140-142), not their streams.
#pragma once
#include <cmath>
#include <cstdint>

#include "ldm_post_token.h"
#include "ldm_relation_detect_core.h"

#if defined(__HIPCC__)
#define LDM_CD_HD __host__ __device__ __forceinline__
#else
#define LDM_CD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // torch rounds every product and sum
#endif

namespace ldm_condb {

enum Quant : int { kLinear = 0, kPercentile = 1, kKMeans = 2 };
// get_cond's cond_type; kRuleNone = "gt" = the plain tokenizer.encode
enum Rule : int { kRuleNone = 0, kRuleC = 1, kRuleCWH = 2, kRulePartial = 3, kRuleRefinement = 4, kRuleRelation = 5, kNumRules = 6 };
enum : int { kErrPrefix = 1, kErrNonFinite = 2, kErrLabel = 4 };
enum : uint32_t { kDrawPartialCount = 1, kDrawPartialScore = 2, kDrawNoise = 3, kDrawRelation = 4 };  // Philox counter word 1

constexpr int kAttr = 5;            // c x y w h
constexpr int kMaxElem = 32;        // elements per layout the kernels take
constexpr int kMaxBin = 128;        // bins per coordinate (centres live in LDS)
constexpr float kPartialRatio = 0.3f;   // MAX_PARTIAL_RATIO, task.py:15
constexpr float kNoiseStd = 0.1f;       // task.py:127

struct Geometry {
  int n_category, n_bin, quant;
  int pad_id, mask_id;
  const double* centres;  // [4][n_bin] sorted cluster centres (x, y, w, h), or nullptr for linear bins
};

template <typename TB>
LDM_CD_HD bool finite(TB v) { return v - v == TB(0); }

template <typename TB>
LDM_CD_HD TB clamp(TB v, TB lo, TB hi) { return v < lo ? lo : (v > hi ? hi : v); }  // (NaN stays NaN, like torch.clamp)

// bin of coordinate k; a NaN answers 0 (the caller raises kErrNonFinite)
template <typename TB>
LDM_CD_HD int quantise(const Geometry& g, int k, TB v) {
  const int N = g.n_bin;
  if (g.quant == kLinear) {
    const double dd = 1.0 / N;
    const TB d = TB(dd);
    const TB q = k < 2 ? clamp(v, TB(0.0), TB(1.0 - dd)) : clamp(v, d, TB(1.0)) - d;
    const TB r = TB(N) * q;
    const TB n = sizeof(TB) == 4 ? TB(rintf((float)r)) : TB(rint((double)r));
    return n == n ? (int)n : 0;
  }
  const double* c = g.centres + (size_t)k * N;
  int best = 0;
  if (g.quant == kPercentile) {
    const float x = (float)clamp(v, TB(0.0), TB(1.0));
    float bd = fabsf((float)c[0] - x);
    for (int i = 1; i < N; ++i) {
      const float di = fabsf((float)c[i] - x);
      if (di < bd) bd = di, best = i;
    }
  } else {
    const double x = (double)(float)v;
    double bd = fabs(x - c[0]);
    for (int i = 1; i < N; ++i) {
      const double di = fabs(x - c[i]);
      if (di < bd) bd = di, best = i;
    }
  }
  return best;
}

// tokens of one element slot (tokenizer.encode); returns the error bits of the slot
template <typename TB>
LDM_CD_HD int encode_element(const Geometry& g, const TB* box, int64_t label, bool valid, int32_t* tok) {
  if (!valid) {
    for (int a = 0; a < kAttr; ++a) tok[a] = g.pad_id;
    return 0;
  }
  int err = 0;
  if (label < 0 || label >= g.n_category) err |= kErrLabel;
  tok[0] = (int32_t)label;
  for (int k = 0; k < 4; ++k) {
    if (!finite(box[k])) err |= kErrNonFinite;
    tok[1 + k] = g.n_category + k * g.n_bin + quantise(g, k, box[k]);
  }
  return err;
}

LDM_CD_HD bool keep_attr(int rule, int a) { return a == 0 || (rule == kRuleCWH && a >= 3); }

// get_cond on the encoded tokens of one element slot: tok -> seq / mask (and seq_orig for refinement, where tok is the encode
// of bbox + noise).  kept: the element's entry of the per-element keep mask (partial only).
LDM_CD_HD void apply_rule(const Geometry& g, int rule, const int32_t* tok, bool valid, bool kept, int32_t* seq, uint8_t* mask,
                          int32_t* seq_orig) {
  for (int a = 0; a < kAttr; ++a) {
    switch (rule) {
      case kRuleC:
      case kRuleCWH:
      case kRuleRelation: {
        const bool keep = keep_attr(rule, a);
        seq[a] = valid ? (keep ? tok[a] : g.mask_id) : g.pad_id;
        mask[a] = (valid && keep) || !valid;
        break;
      }
      case kRulePartial:
        seq[a] = kept ? tok[a] : g.mask_id;   // (padding slots too: cond["seq"][~keep] = mask_id)
        mask[a] = kept;
        break;
      case kRuleRefinement: {
        const bool m = (valid && a == 0) || !valid;
        seq[a] = valid ? (m ? tok[a] : g.mask_id) : g.pad_id;
        mask[a] = m;
        if (seq_orig) seq_orig[a] = tok[a];
        break;
      }
      default:
        seq[a] = tok[a];
        mask[a] = valid;
    }
  }
}

// ---- own draws ------------------------------------------------------------------------------------------------------
LDM_CD_HD void draw4(uint64_t seed, uint64_t layout, uint32_t purpose, uint32_t slot, uint32_t (&r)[4]) {
  ldm_post::philox4x32_10(slot, purpose, (uint32_t)layout, (uint32_t)(layout >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
}
LDM_CD_HD uint32_t pick4(const uint32_t (&r)[4], int w) { return w == 0 ? r[0] : (w == 1 ? r[1] : (w == 2 ? r[2] : r[3])); }

// partial (task.py:62-75): k = randint(1, vmax) if vmax > 1 else 1, vmax = int((n - 1) * 0.3) in float32 like the reference's
// 0-dim tensor product; then the k elements with the largest uniform scores among the n valid ones (ties: lower index first)
LDM_CD_HD int partial_vmax(int n) { return (int)((float)(n - 1) * kPartialRatio); }
LDM_CD_HD int partial_count(uint64_t seed, uint64_t layout, int n) {
  const int vmax = partial_vmax(n);
  if (vmax <= 1) return 1;
  uint32_t r[4];
  draw4(seed, layout, kDrawPartialCount, 0, r);
  return 1 + (int)(((uint64_t)r[0] * (uint64_t)vmax) >> 32);
}
// is valid element e of a layout whose valid elements are mask[0..E) among the `count` best?
LDM_CD_HD bool partial_keep(uint64_t seed, uint64_t layout, const uint8_t* mask, int E, int e, int count) {
  uint32_t r[4];
  draw4(seed, layout, kDrawPartialScore, (uint32_t)(e >> 2), r);
  const uint32_t mine = pick4(r, e & 3);
  int ahead = 0;
  for (int q = 0; 4 * q < E; ++q) {
    draw4(seed, layout, kDrawPartialScore, (uint32_t)q, r);
    for (int w = 0; w < 4; ++w) {
      const int o = 4 * q + w;
      if (o < E && o != e && mask[o]) {
        const uint32_t s = pick4(r, w);
        ahead += s > mine || (s == mine && o < e);
      }
    }
  }
  return ahead < count;
}

// refinement: four iid N(0, 0.1^2) of element e by Box-Muller in float32
LDM_CD_HD void noise4(uint64_t seed, uint64_t layout, int e, float* z) {
  uint32_t r[4];
  draw4(seed, layout, kDrawNoise, (uint32_t)e, r);
  for (int p = 0; p < 2; ++p) {
    const float rad = kNoiseStd * sqrtf(-2.0f * logf(ldm_post::u01(r[2 * p])));
    const float ang = 6.283185307179586f * ldm_post::u01(r[2 * p + 1]);
    z[2 * p] = rad * cosf(ang);
    z[2 * p + 1] = rad * sinf(ang);
  }
}

// ---- relation graph -------------------------------------------------------------------------------------------------
// pairs (i, j), i < j, of N nodes in itertools.combinations order
LDM_CD_HD int n_pairs(int N) { return N * (N - 1) / 2; }
LDM_CD_HD void pair_of(int N, int p, int& i, int& j) {
  int row = 0, left = p;
  while (left >= N - 1 - row) left -= N - 1 - row, ++row;
  i = row, j = row + 1 + left;
}
// how many of the 2 * P (kind, pair) candidates AddRelationConstraints samples: int(len(rel_all) * edge_ratio), in double
LDM_CD_HD int relation_sample_size(int N, double edge_ratio) { return (int)((double)(2 * n_pairs(N)) * edge_ratio); }
constexpr int kRelUnknown = (1 << ldm_reldet::kSizeUnknown) | (1 << ldm_reldet::kLocUnknown);

// edge_attr of pair (i, j); bi / bj: the node boxes, node 0 = the canvas (its label is 0: the thirds rule)
template <typename TB>
LDM_CD_HD int pair_attr(const TB* bi, const TB* bj, bool i_is_canvas, bool sel_size, bool sel_loc) {
  const int size = sel_size ? ldm_reldet::detect_size_relation(bi, bj) : ldm_reldet::kSizeUnknown;
  const int loc = sel_loc ? ldm_reldet::detect_loc_relation(bi, bj, i_is_canvas) : ldm_reldet::kLocUnknown;
  return (1 << size) | (1 << loc);
}

}  // namespace ldm_condb
