// Average IoU (BLT + VTN), DocSim and Max-IoU pair scores on the device (trainer/helpers/metric.py:300-507, called at
// eval.py:173-176,211-215).  The arithmetic is the one source of ldm_eval_iou_core.h (also compiled for the host:
// tests/cpu_eval_iou_check.cpp).
//
// One lane per problem: a layout (average IoU), a (gt, generated) pair (DocSim) or a (set-1, set-2) layout pair of a Max-IoU
// group.  Boxes are read from global memory (neighbouring lanes share a layout, so the reads hit the caches); the
// assignment solver's state lives in LDS, [index][lane] so that a wavefront's accesses fall in distinct banks, sized by
// the longest problem of the call (kSeg = 8 or 32).  Max-IoU segments of <= 3 equal labels (the common case) are solved by
// enumeration without touching LDS.  Every kernel is templated on the box types of its two inputs; the compute type is
// double if either is float64 (numpy's promotion), each box's l / t / r / b / area in its own dtype.
#include "ldm_kernels.h"
#include "ldm_eval_iou_core.h"

namespace ldm {

namespace {

constexpr int kEvalLanes = 64;

template <int kSeg>
struct LdsSolverState {
  static constexpr int kLen = kSeg + 1;
  double* d;   // [3][kLen][kEvalLanes] + lane: u, v, minv
  uint8_t* b;  // [2][kLen][kEvalLanes] + lane: p, way
  __device__ double& u(int k) { return d[k * kEvalLanes]; }
  __device__ double& v(int k) { return d[(kLen + k) * kEvalLanes]; }
  __device__ double& minv(int k) { return d[(2 * kLen + k) * kEvalLanes]; }
  __device__ uint8_t& p(int k) { return b[k * kEvalLanes]; }
  __device__ uint8_t& way(int k) { return b[(kLen + k) * kEvalLanes]; }
};

#define LDM_EVAL_LDS(kSeg)                                                         \
  __shared__ double s_d[3 * ((kSeg) + 1) * kEvalLanes];                            \
  __shared__ uint8_t s_b[2 * ((kSeg) + 1) * kEvalLanes];                           \
  LdsSolverState<kSeg> st{s_d + threadIdx.x, s_b + threadIdx.x};

// per layout: out[b] = {BLT, VTN}
template <typename TB>
__global__ __launch_bounds__(kEvalLanes) void eval_average_iou_k(const TB* __restrict__ bbox, const uint8_t* __restrict__ mask,
                                                                 int B, int S, double* __restrict__ out) {
  const int b = blockIdx.x * kEvalLanes + threadIdx.x;
  if (b >= B) return;
  const uint8_t* m = mask + (size_t)b * S;
  double blt, vtn;
  ldm_eval::average_iou(bbox + (size_t)b * S * 4, S, [&](int i) { return m[i] != 0; }, &blt, &vtn);
  out[2 * (size_t)b] = blt;
  out[2 * (size_t)b + 1] = vtn;
}

// per pair b: DocSim of (set1[b], set2[b]); n1 / n2 elements each, first in their rows
template <typename C, typename T1, typename T2, int kSeg>
__global__ __launch_bounds__(kEvalLanes) void eval_docsim_k(const T1* __restrict__ bbox1, const int64_t* __restrict__ label1,
                                                            const int32_t* __restrict__ n1, const T2* __restrict__ bbox2,
                                                            const int64_t* __restrict__ label2, const int32_t* __restrict__ n2,
                                                            int B, int S, double* __restrict__ out, int32_t* __restrict__ err) {
  LDM_EVAL_LDS(kSeg)
  const int b = blockIdx.x * kEvalLanes + threadIdx.x;
  if (b >= B) return;
  const int N = min(max(n1[b], 0), S), M = min(max(n2[b], 0), S);
  int e = 0;
  out[b] = ldm_eval::docsim_pair<C>(bbox1 + (size_t)b * S * 4, label1 + (size_t)b * S, N, bbox2 + (size_t)b * S * 4,
                                    label2 + (size_t)b * S, M, st, &e);
  if (e) atomicOr(err, e);
}

// per pair p of a group table row {first1, n1, first2, n2, n_elem, out_offset} (rows ordered by out_offset): local index
// q = p - out_offset, set-2 layout q / n1, set-1 layout q % n1 (the reference's flat order, metric.py:317-329)
template <typename C, typename T1, typename T2, int kSeg>
__global__ __launch_bounds__(kEvalLanes) void eval_max_iou_k(const T1* __restrict__ bbox1, const int64_t* __restrict__ label1,
                                                             int R1, const T2* __restrict__ bbox2, int R2, int S,
                                                             const int64_t* __restrict__ groups, int G, int64_t n_pairs,
                                                             int max_seg, double* __restrict__ out, int32_t* __restrict__ err) {
  LDM_EVAL_LDS(kSeg)
  const int64_t p = (int64_t)blockIdx.x * kEvalLanes + threadIdx.x;
  if (p >= n_pairs) return;
  int lo = 0, hi = G - 1;  // last group whose offset is <= p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[6 * (size_t)mid + 5] <= p) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* g = groups + 6 * (size_t)lo;
  const int64_t q = p - g[5], n1 = g[1], n2 = g[3];
  const int64_t a = n1 > 0 ? q % n1 : 0, c = n1 > 0 ? q / n1 : 0;
  const int64_t r1 = g[0] + a, r2 = g[2] + c;
  int e = 0;
  double v = 0.0;
  if (q < 0 || n1 <= 0 || c >= n2 || r1 < 0 || r1 >= R1 || r2 < 0 || r2 >= R2 || g[4] < 0 || g[4] > S) {
    e = 4;  // malformed group table
  } else {
    v = ldm_eval::max_iou_pair<C>(bbox1 + (size_t)r1 * S * 4, bbox2 + (size_t)r2 * S * 4, label1 + (size_t)r1 * S, (int)g[4],
                                  max_seg < kSeg ? max_seg : kSeg, st, &e);
  }
  out[p] = v;
  if (e) atomicOr(err, e);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kEvalLanes - 1) / kEvalLanes); }

template <typename C, typename T1, typename T2>
void docsim_typed(const void* b1, const int64_t* l1, const int32_t* n1, const void* b2, const int64_t* l2, const int32_t* n2,
                  int B, int S, double* out, int32_t* err, hipStream_t st) {
  const T1* p1 = static_cast<const T1*>(b1);
  const T2* p2 = static_cast<const T2*>(b2);
  if (S <= 8)
    hipLaunchKernelGGL((eval_docsim_k<C, T1, T2, 8>), dim3(blocks_for(B)), dim3(kEvalLanes), 0, st, p1, l1, n1, p2, l2, n2, B,
                       S, out, err);
  else
    hipLaunchKernelGGL((eval_docsim_k<C, T1, T2, 32>), dim3(blocks_for(B)), dim3(kEvalLanes), 0, st, p1, l1, n1, p2, l2, n2, B,
                       S, out, err);
}

template <typename C, typename T1, typename T2>
void max_iou_typed(const void* b1, const int64_t* l1, int R1, const void* b2, int R2, int S, const int64_t* groups, int G,
                   int64_t n_pairs, int max_seg, double* out, int32_t* err, hipStream_t st) {
  const T1* p1 = static_cast<const T1*>(b1);
  const T2* p2 = static_cast<const T2*>(b2);
  if (max_seg <= 8)
    hipLaunchKernelGGL((eval_max_iou_k<C, T1, T2, 8>), dim3(blocks_for(n_pairs)), dim3(kEvalLanes), 0, st, p1, l1, R1, p2, R2, S,
                       groups, G, n_pairs, max_seg, out, err);
  else
    hipLaunchKernelGGL((eval_max_iou_k<C, T1, T2, 32>), dim3(blocks_for(n_pairs)), dim3(kEvalLanes), 0, st, p1, l1, R1, p2, R2,
                       S, groups, G, n_pairs, max_seg, out, err);
}

}  // namespace

void launch_eval_average_iou(const void* bbox, int box_f64, const uint8_t* mask, int B, int S, double* out, hipStream_t st) {
  if (box_f64)
    hipLaunchKernelGGL(eval_average_iou_k<double>, dim3(blocks_for(B)), dim3(kEvalLanes), 0, st,
                       static_cast<const double*>(bbox), mask, B, S, out);
  else
    hipLaunchKernelGGL(eval_average_iou_k<float>, dim3(blocks_for(B)), dim3(kEvalLanes), 0, st, static_cast<const float*>(bbox),
                       mask, B, S, out);
}

void launch_eval_docsim(const void* bbox1, int box1_f64, const int64_t* label1, const int32_t* n1, const void* bbox2,
                        int box2_f64, const int64_t* label2, const int32_t* n2, int B, int S, double* out, int32_t* err,
                        hipStream_t st) {
  if (!box1_f64 && !box2_f64) docsim_typed<float, float, float>(bbox1, label1, n1, bbox2, label2, n2, B, S, out, err, st);
  else if (box1_f64 && box2_f64) docsim_typed<double, double, double>(bbox1, label1, n1, bbox2, label2, n2, B, S, out, err, st);
  else if (box1_f64) docsim_typed<double, double, float>(bbox1, label1, n1, bbox2, label2, n2, B, S, out, err, st);
  else docsim_typed<double, float, double>(bbox1, label1, n1, bbox2, label2, n2, B, S, out, err, st);
}

void launch_eval_max_iou(const void* bbox1, int box1_f64, const int64_t* label1, int R1, const void* bbox2, int box2_f64, int R2,
                         int S, const int64_t* groups, int G, int64_t n_pairs, int max_seg, double* out, int32_t* err,
                         hipStream_t st) {
  if (!box1_f64 && !box2_f64)
    max_iou_typed<float, float, float>(bbox1, label1, R1, bbox2, R2, S, groups, G, n_pairs, max_seg, out, err, st);
  else if (box1_f64 && box2_f64)
    max_iou_typed<double, double, double>(bbox1, label1, R1, bbox2, R2, S, groups, G, n_pairs, max_seg, out, err, st);
  else if (box1_f64)
    max_iou_typed<double, double, float>(bbox1, label1, R1, bbox2, R2, S, groups, G, n_pairs, max_seg, out, err, st);
  else
    max_iou_typed<double, float, double>(bbox1, label1, R1, bbox2, R2, S, groups, G, n_pairs, max_seg, out, err, st);
}

}  // namespace ldm
