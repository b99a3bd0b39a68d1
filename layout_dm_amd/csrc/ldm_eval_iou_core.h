// IoU-family evaluation metrics of the reference's eval.py — average IoU (BLT perceptual + VTN), Max-IoU and DocSim
// (trainer/helpers/metric.py:206-507; eval.py:173-176,211-215) — ONE source of the arithmetic, compiled for the device
// (kernels_eval_iou.hip: one lane per layout / layout pair) and for the host (tests/cpu_eval_iou_check.cpp).
//
// Numerics follow numpy on the reference's own inputs (numpy >= 2 promotion rules):
//   * every box is turned into l, t, r, b and its area (r - l) * (b - t) in ITS OWN dtype (convert_xywh_to_ltrb, util.py:16-22),
//     then widened to the compute type C (double if either box is float64, else float): a float32 dataset layout against a
//     float64 kmeans-decoded one computes exactly what numpy computes.  Box IoU keeps compute_iou's order (metric.py:206-247),
//     so IoU entries are bit-exact in both precisions (no FMA contraction: see the pragma below).
//   * the perceptual union (metric.py:250-297) rasterises the boxes on a 32 x 32 canvas with numpy's half-to-even round
//     (rint), astype(int32) (NaN / out-of-range -> INT_MIN) and clip to [0, 32]; rows are 32-bit column masks + popcount.
//     The canvas sum is float64, so a BLT entry is double(ai) / (count / 1024).
//   * __compute_bbox_sim (metric.py:434-455): C_S = 2, C = 0.5, 0 for different categories; w * h in each box's own dtype.
//   * assignments: an exact maximum-weight solver (shortest augmenting path, Jonker-Volgenant / Hungarian) for n x m, n <= m
//     <= kMaxS, potentials in double; the value is summed in double from the ORIGINAL weights along the assignment.
//     Any non-finite weight sets the caller's error flag (scipy's linear_sum_assignment raises ValueError there).
//   * sums of kept IoUs / assigned weights run in double (numpy sums float32 in float32 with pairwise blocking: parity is
//     to float32 rounding there, ~1e-7 relative, and to ~1e-15 in float64).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LDM_EV_HD __host__ __device__ __forceinline__
#else
#define LDM_EV_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // numpy rounds every product and sum: bit-exact IoU needs no fused multiply-adds
#endif

namespace ldm_eval {

using std::fabs;
using std::pow;
using std::rint;
using std::sqrt;

constexpr int kMaxS = 32;  // elements per layout (the reference's datasets have <= 25)

// l, t, r, b and (r - l) * (b - t), computed in the box's dtype TB, widened to C
template <typename C>
struct Ltrb {
  C l, t, r, b, a;
};
template <typename C, typename TB>
LDM_EV_HD Ltrb<C> ltrb(const TB* x) {
  const TB hw = x[2] / TB(2), hh = x[3] / TB(2);
  const TB l = x[0] - hw, t = x[1] - hh, r = x[0] + hw, b = x[1] + hh;
  const TB a = (r - l) * (b - t);
  return Ltrb<C>{C(l), C(t), C(r), C(b), C(a)};
}

template <typename C>
LDM_EV_HD C intersection(const Ltrb<C>& p, const Ltrb<C>& q) {
  const C l_max = p.l > q.l ? p.l : q.l, r_min = p.r < q.r ? p.r : q.r;
  const C t_max = p.t > q.t ? p.t : q.t, b_min = p.b < q.b ? p.b : q.b;
  return (l_max < r_min && t_max < b_min) ? (r_min - l_max) * (b_min - t_max) : C(0);
}

// compute_iou (metric.py:206-247): ai / (a1 + a2 - ai)
template <typename C>
LDM_EV_HD C box_iou(const Ltrb<C>& p, const Ltrb<C>& q) {
  const C ai = intersection(p, q);
  const C au = p.a + q.a - ai;
  return ai / au;
}

// (x * 32).round().astype(np.int32).clip(0, 32)
template <typename TB>
LDM_EV_HD int raster_coord(TB x) {
  const TB v = rint(x * TB(32));
  const int i = (v >= TB(-2147483648.0) && v < TB(2147483648.0)) ? (int)v : INT32_MIN;
  return i < 0 ? 0 : (i > 32 ? 32 : i);
}
LDM_EV_HD uint32_t col_mask(int l, int r) {  // bits [l, r) of a canvas row; empty when l >= r
  if (l >= r) return 0u;
  const uint32_t hi = r >= 32 ? 0xffffffffu : ((1u << r) - 1u);
  return hi & ~((1u << l) - 1u);
}
LDM_EV_HD int popcount32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// number of painted cells of the 32 x 32 canvas (canvas[t:b, l:r] = 1 for every valid box); the canvas rows live in 32
// registers (fully unrolled, static indices), boxes are read once each
template <typename TB, typename Valid>
LDM_EV_HD int union_cells(const TB* bbox, int n, Valid valid) {
  uint32_t row[32];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int y = 0; y < 32; ++y) row[y] = 0u;
  for (int i = 0; i < n; ++i) {
    if (!valid(i)) continue;
    const TB* x = bbox + 4 * i;
    const TB hw = x[2] / TB(2), hh = x[3] / TB(2);
    const int l = raster_coord<TB>(x[0] - hw), t = raster_coord<TB>(x[1] - hh);
    const int r = raster_coord<TB>(x[0] + hw), b = raster_coord<TB>(x[1] + hh);
    const uint32_t m = col_mask(l, r);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int y = 0; y < 32; ++y) row[y] |= (y >= t && y < b) ? m : 0u;
  }
  int cells = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int y = 0; y < 32; ++y) cells += popcount32(row[y]);
  return cells;
}

// __compute_average_iou (metric.py:374-411) of one layout, perceptual (BLT) and plain (VTN): the mean of the off-diagonal
// IoUs above float32 eps, 0 if none / fewer than two elements.  IoU is symmetric bit for bit (a1 + a2 commutes), so the
// ordered pairs are the unordered ones counted twice: same mean.  valid(i): slot i holds an element.
template <typename TB, typename Valid>
LDM_EV_HD void average_iou(const TB* bbox, int S, Valid valid, double* blt, double* vtn) {
  int n = 0;
  for (int i = 0; i < S; ++i) n += valid(i) ? 1 : 0;
  *blt = 0.0;
  *vtn = 0.0;
  if (n < 2) return;
  const int cells = union_cells(bbox, S, valid);
  const double area_union = (double)cells / 1024.0;
  const double eps = (double)FLT_EPSILON;
  double sb = 0.0, sv = 0.0;
  int nb = 0, nv = 0;
  for (int i = 0; i < S; ++i) {
    if (!valid(i)) continue;
    const Ltrb<TB> p = ltrb<TB>(bbox + 4 * i);
    for (int j = i + 1; j < S; ++j) {
      if (!valid(j)) continue;
      const Ltrb<TB> q = ltrb<TB>(bbox + 4 * j);
      const TB ai = intersection(p, q);
      const TB iou = ai / (p.a + q.a - ai);
      if (iou > TB(FLT_EPSILON)) {
        sv += (double)iou;
        ++nv;
      }
      if (cells > 0) {
        const double pi = (double)ai / area_union;
        if (pi > eps) {
          sb += pi;
          ++nb;
        }
      }
    }
  }
  if (nb > 0) *blt = sb / (double)nb;
  // numpy's float32 mean ends in float32: sum rounded to TB, divided by the count in TB
  if (nv > 0) *vtn = (double)((TB)(2.0 * sv) / (TB)(2 * nv));
}

// __compute_bbox_sim (metric.py:434-455)
template <typename C, typename TB1, typename TB2>
LDM_EV_HD C bbox_sim(const TB1* x1, int64_t c1, const TB2* x2, int64_t c2) {
  if (c1 != c2) return C(0);
  const C dx = C(x1[0]) - C(x2[0]), dy = C(x1[1]) - C(x2[1]);
  const C delta_c = sqrt(dx * dx + dy * dy);
  const C delta_s = fabs(C(x1[2]) - C(x2[2])) + fabs(C(x1[3]) - C(x2[3]));
  const C a1 = C(x1[2] * x1[3]), a2 = C(x2[2] * x2[3]);  // w * h in each box's own dtype
  C area = a1 < a2 ? a1 : a2;
  area = area > C(0) ? area : C(0);
  const C alpha = pow(area, C(0.5));
  return alpha * pow(C(2), -delta_c - C(2) * delta_s);
}

// ------------------------------------------------------------------------------------------------ assignment
// Solver state of one problem: u [n + 1] (rows), v / minv [m + 1] (columns) in double, p / way [m + 1]
// (columns, 1-based row / column indices).  St maps index k to the storage (LDS with a lane stride on the device).
// Maximum-weight assignment of the n x m matrix w(i, j) (0-based), n <= m: shortest augmenting paths on the cost -w with
// double potentials.  Returns the assignment's value from the original weights; *err |= 1 on a non-finite weight.
template <typename St, typename W>
LDM_EV_HD double assign_max(int n, int m, St& st, W w, int* err) {
  const double inf = HUGE_VAL;
  for (int j = 0; j <= m; ++j) {
    st.v(j) = 0.0;
    st.p(j) = 0;
    st.way(j) = 0;
  }
  for (int i = 0; i <= n; ++i) st.u(i) = 0.0;
  for (int i = 1; i <= n; ++i) {
    st.p(0) = (uint8_t)i;
    int j0 = 0;
    uint64_t used = 0;
    for (int j = 0; j <= m; ++j) st.minv(j) = inf;
    do {
      used |= 1ull << j0;
      const int i0 = st.p(j0);
      int j1 = 0;
      double delta = inf;
      const double ui0 = st.u(i0);
      for (int j = 1; j <= m; ++j) {
        if ((used >> j) & 1ull) continue;
        const double wij = (double)w(i0 - 1, j - 1);
        if (!(wij - wij == 0.0)) {  // NaN or inf
          *err |= 1;
          return 0.0;
        }
        const double cur = -wij - ui0 - st.v(j);
        double mv = st.minv(j);
        if (cur < mv) {
          mv = cur;
          st.minv(j) = cur;
          st.way(j) = (uint8_t)j0;
        }
        if (mv < delta) {
          delta = mv;
          j1 = j;
        }
      }
      if (j1 == 0) {  // no reachable column: cannot happen with finite weights and n <= m
        *err |= 1;
        return 0.0;
      }
      for (int j = 0; j <= m; ++j) {
        if ((used >> j) & 1ull) {
          st.u(st.p(j)) += delta;
          st.v(j) -= delta;
        } else {
          st.minv(j) -= delta;
        }
      }
      j0 = j1;
    } while (st.p(j0) != 0);
    do {
      const int j1 = st.way(j0);
      st.p(j0) = st.p(j1);
      j0 = j1;
    } while (j0 != 0);
  }
  double value = 0.0;
  for (int j = 1; j <= m; ++j)
    if (st.p(j) != 0) value += (double)w(st.p(j) - 1, j - 1);
  return value;
}

// Square n x n problems of n <= 3 by enumeration (no state); larger ones through assign_max
template <typename St, typename W>
LDM_EV_HD double assign_max_square(int n, St& st, W w, int* err) {
  if (n > 3) return assign_max(n, n, st, w, err);
  if (n <= 0) return 0.0;
  const double w00 = (double)w(0, 0);
  if (n == 1) {
    if (!(w00 - w00 == 0.0)) *err |= 1;
    return w00;
  }
  const double w01 = (double)w(0, 1), w10 = (double)w(1, 0), w11 = (double)w(1, 1);
  if (n == 2) {
    if (!(w00 - w00 + w01 - w01 + w10 - w10 + w11 - w11 == 0.0)) *err |= 1;
    const double a = w00 + w11, b = w01 + w10;
    return a >= b ? a : b;
  }
  const double w02 = (double)w(0, 2), w12 = (double)w(1, 2), w20 = (double)w(2, 0), w21 = (double)w(2, 1),
               w22 = (double)w(2, 2);
  if (!(w00 - w00 + w01 - w01 + w02 - w02 + w10 - w10 + w11 - w11 + w12 - w12 + w20 - w20 + w21 - w21 + w22 - w22 == 0.0))
    *err |= 1;
  double best = w00 + w11 + w22, s;
  s = w00 + w12 + w21;
  best = s > best ? s : best;
  s = w01 + w10 + w22;
  best = s > best ? s : best;
  s = w01 + w12 + w20;
  best = s > best ? s : best;
  s = w02 + w10 + w21;
  best = s > best ? s : best;
  s = w02 + w11 + w20;
  best = s > best ? s : best;
  return best;
}

// __compute_maximum_iou_for_layout (metric.py:300-314) of two layouts with the same label multiset, both sorted stably by
// label (equal labels form the same segments at the same offsets): sum over segments of the segment's optimal IoU
// assignment, / N.  b1 / b2: [N][4] boxes, lab: [N] labels of layout 1.  *err |= 2 on a segment longer than max_seg.
template <typename C, typename TB1, typename TB2, typename St>
LDM_EV_HD double max_iou_pair(const TB1* b1, const TB2* b2, const int64_t* lab, int N, int max_seg, St& st, int* err) {
  if (N <= 0) return 0.0;
  double score = 0.0;
  for (int s = 0; s < N;) {
    int e = s + 1;
    while (e < N && lab[e] == lab[s]) ++e;
    const int n = e - s;
    if (n > max_seg) {
      *err |= 2;
      return 0.0;
    }
    auto w = [&](int i, int j) { return box_iou(ltrb<C>(b1 + 4 * (s + i)), ltrb<C>(b2 + 4 * (s + j))); };
    score += assign_max_square(n, st, w, err);
    s = e;
  }
  return score / (double)N;
}

// __compute_docsim_between_two_layouts (metric.py:458-489): N x M similarity matrix, 0 when |N - M| >= 3, else the mean of
// its optimal assignment's min(N, M) entries (0 for an empty one).  The reference builds the matrix from a
// meshgrid(range(N), range(M)) flattened in (j, i) order and reshaped to (N, M): entry (r, c) is the pair of flat index
// k = r * M + c, i.e. element k % N of layout 1 against element k / N of layout 2 (the plain (i, j) matrix when N == M).
// The solver sees exactly that matrix.
template <typename C, typename TB1, typename TB2, typename St>
LDM_EV_HD double docsim_pair(const TB1* b1, const int64_t* c1, int N, const TB2* b2, const int64_t* c2, int M, St& st,
                             int* err) {
  if (N >= M + 3 || N <= M - 3) return 0.0;
  if (N == 0 || M == 0) return 0.0;
  auto w = [&](int r, int c) {
    const int k = r * M + c, i = k % N, j = k / N;
    return bbox_sim<C>(b1 + 4 * i, c1[i], b2 + 4 * j, c2[j]);
  };
  double v;
  if (N <= M) {
    v = assign_max(N, M, st, w, err);
  } else {
    auto wt = [&](int r, int c) { return w(c, r); };
    v = assign_max(M, N, st, wt, err);
  }
  return v / (double)(N < M ? N : M);
}

}  // namespace ldm_eval
