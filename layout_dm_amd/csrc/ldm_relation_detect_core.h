// Relation detection of the reference's violation score — detect_size_relation / detect_loc_relation
// (trainer/data/util.py:33-69) and the per-edge failure / valid counts of compute_violation (trainer/helpers/metric.py:62-95)
// — ONE source of the arithmetic, compiled for the device (kernels_violation.hip: one lane per edge) and for the host
// (tests/cpu_relation_detect_check.cpp).
//
// Numerics follow torch on the reference's own inputs, templated on the box type TB (float, double):
//   * areas w * h are rounded in TB.  The reference multiplies the Python floats (1 - 0.1) and (1 + 0.1) into a 0-dim
//     tensor, so the factors are those doubles ROUNDED TO TB before the multiply (float32(0.9) * a1, not the double
//     product); every product is rounded (no FMA contraction: see the pragma below).
//   * a canvas source compares b2's yc against the doubles 1.0 / 3 and 2.0 / 3.  float32(1/3) and float32(2/3) lie above
//     the doubles, so the float32 comparison torch does and the double comparison here agree on every float32 value.
//   * otherwise xc -/+ w / 2, yc -/+ h / 2 in TB (convert_xywh_to_ltrb, helpers/util.py:16-22) and the reference's chain
//     TOP, BOTTOM, LEFT, RIGHT, CENTER in that order, with <=.
//   * per edge (metric.py:71-86): the size part counts when bit RelSize.UNKNOWN (0) of gt is clear, the loc part when bit
//     RelLoc.UNKNOWN (4) is clear; a counted part fails when gt & (1 << pred) == 0.
//   * per layout: failures / valid, integer sums converted to float32 and divided in float32 (torch's long / long);
//     0 / 0 is NaN.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LDM_RD_HD __host__ __device__ __forceinline__
#else
#define LDM_RD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // torch rounds every product: bit-exact thresholds need no fused multiply-adds
#endif

namespace ldm_reldet {

// RelSize / RelLoc (data/util.py:14-27)
enum : int {
  kSizeUnknown = 0, kSmaller = 1, kEqual = 2, kLarger = 3,
  kLocUnknown = 4, kLeft = 5, kTop = 6, kRight = 7, kBottom = 8, kCenter = 9,
};

constexpr double kSizeAlpha = 0.1;  // REL_SIZE_ALPHA

// boxes are {xc, yc, w, h}
template <typename TB>
LDM_RD_HD int detect_size_relation(const TB* b1, const TB* b2) {
  const TB a1 = b1[2] * b1[3];
  const TB a2 = b2[2] * b2[3];
  const TB lo = TB(1 - kSizeAlpha) * a1, hi = TB(1 + kSizeAlpha) * a1;
  if (lo < a2 && a2 < hi) return kEqual;
  return a1 < a2 ? kLarger : kSmaller;
}

template <typename TB>
LDM_RD_HD int detect_loc_relation(const TB* b1, const TB* b2, bool is_canvas) {
  if (is_canvas) {
    const double yc = (double)b2[1];
    if (yc < 1.0 / 3) return kTop;
    return yc < 2.0 / 3 ? kCenter : kBottom;
  }
  const TB hw1 = b1[2] / TB(2), hh1 = b1[3] / TB(2), hw2 = b2[2] / TB(2), hh2 = b2[3] / TB(2);
  const TB l1 = b1[0] - hw1, t1 = b1[1] - hh1, r1 = b1[0] + hw1, bo1 = b1[1] + hh1;
  const TB l2 = b2[0] - hw2, t2 = b2[1] - hh2, r2 = b2[0] + hw2, bo2 = b2[1] + hh2;
  if (bo2 <= t1) return kTop;
  if (bo1 <= t2) return kBottom;
  if (r2 <= l1) return kLeft;
  if (r1 <= l2) return kRight;
  return kCenter;
}

struct EdgeResult {
  int size_code, loc_code;  // what the two detectors say, whether or not gt asks for them
  int failure, valid;       // 0..2 each
};

// gt: the edge's relation bitmask (edge_attr); src_is_canvas: y[src] == 0
template <typename TB>
LDM_RD_HD EdgeResult detect_edge(const TB* b1, const TB* b2, bool src_is_canvas, int64_t gt) {
  EdgeResult r;
  r.size_code = detect_size_relation(b1, b2);
  r.loc_code = detect_loc_relation(b1, b2, src_is_canvas);
  r.failure = r.valid = 0;
  if (((~gt) & (int64_t(1) << kSizeUnknown)) != 0) {
    r.failure += (gt & (int64_t(1) << r.size_code)) == 0;
    r.valid += 1;
  }
  if (((~gt) & (int64_t(1) << kLocUnknown)) != 0) {
    r.failure += (gt & (int64_t(1) << r.loc_code)) == 0;
    r.valid += 1;
  }
  return r;
}

// failures.sum() / valid.sum() of one layout, as torch divides two int64 tensors
LDM_RD_HD float violation_score(int64_t failures, int64_t valid) { return (float)failures / (float)valid; }

}  // namespace ldm_reldet
