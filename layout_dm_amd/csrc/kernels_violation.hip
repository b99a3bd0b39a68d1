// Relation violation score on the device (compute_violation, trainer/helpers/metric.py:62-95, called at
// trainer/test.py:230-254).  The arithmetic is the one source of ldm_relation_detect_core.h (also compiled for the host:
// tests/cpu_relation_detect_check.cpp).
//
// One wavefront per layout, one lane per edge: a layout's edges are contiguous in the CSR edge list, so its 64 lanes walk
// them in strides of 64 (no cap on edges or nodes), each lane runs the two detectors on its edge, and the per-layout
// `failures` and `valid` are INTEGER sums reduced across the wavefront — no float atomics, no dependence on any order.
// The score is float32(failures) / float32(valid), what torch's long / long gives; 0 / 0 is NaN like the reference.
//
// Two ways to name a box row.  Flattened: row first_node[graph] + local id of `bbox_flatten`, the reference's global
// index whatever the generated masks are.  Dense: the same global index resolved against the (B,S) mask of
// ldm_decode_layouts with a canvas row (0.5, 0.5, 1, 1) in front of every layout — violation_rows_k scans the per-layout
// row counts, an edge end finds its layout by bisection and its slot by counting mask bytes — which is bbox_c[mask_c] of
// test.py:232-250 without building it.  Every row index is checked against the number of rows: a miss sets *err and
// reads nothing (the reference raises an IndexError there).
#include <cmath>

#include "ldm_kernels.h"
#include "ldm_relation_detect_core.h"

namespace ldm {

namespace {

constexpr int kVioBlock = 256;                 // 4 wavefronts = 4 layouts
constexpr int kVioWaves = kVioBlock / 64;
constexpr int kErrRow = 1;                     // an edge names a box row beyond the flattened rows
constexpr int kErrGraph = 2;                   // malformed graph: offsets not ascending within [0, E], node id outside y

template <typename TB>
struct FlatRows {
  const TB* bbox;
  int64_t n_rows;
  __device__ bool load(int64_t r, TB* box) const {
    if (r < 0 || r >= n_rows) return false;
    const TB* p = bbox + 4 * r;
    box[0] = p[0], box[1] = p[1], box[2] = p[2], box[3] = p[3];
    return true;
  }
};

template <typename TB>
struct DenseRows {
  const TB* bbox;              // (B,S,4)
  const uint8_t* mask;         // (B,S)
  const int32_t* row_start;    // (B+1): exclusive scan of 1 + the layout's mask count
  int B, S;
  __device__ bool load(int64_t r, TB* box) const {
    if (r < 0 || r >= row_start[B]) return false;
    int lo = 0, hi = B - 1;  // last layout whose first row is <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (row_start[mid] <= r) lo = mid;
      else hi = mid - 1;
    }
    int k = (int)(r - row_start[lo]);
    if (k == 0) {  // the canvas element test.py puts in front of every layout
      box[0] = TB(0.5), box[1] = TB(0.5), box[2] = TB(1), box[3] = TB(1);
      return true;
    }
    const uint8_t* m = mask + (size_t)lo * S;
    for (int s = 0; s < S; ++s) {
      if (m[s] && --k == 0) {
        const TB* p = bbox + ((size_t)lo * S + s) * 4;
        box[0] = p[0], box[1] = p[1], box[2] = p[2], box[3] = p[3];
        return true;
      }
    }
    return false;  // not reached: k <= the layout's mask count
  }
};

// row_start[b] = sum over b' < b of (1 + mask count of b'), row_start[B] = all rows.  One block; thread t owns a contiguous
// chunk of layouts, the chunk sums are scanned in LDS.
__global__ __launch_bounds__(kVioBlock) void violation_rows_k(const uint8_t* __restrict__ mask, int B, int S,
                                                              int32_t* __restrict__ row_start) {
  __shared__ int32_t s_sum[kVioBlock];
  const int t = threadIdx.x;
  const int chunk = (B + kVioBlock - 1) / kVioBlock;
  const int b0 = min(t * chunk, B), b1 = min(b0 + chunk, B);
  int32_t sum = 0;
  for (int b = b0; b < b1; ++b) {
    const uint8_t* m = mask + (size_t)b * S;
    int32_t c = 1;
    for (int s = 0; s < S; ++s) c += m[s] != 0;
    sum += c;
  }
  s_sum[t] = sum;
  __syncthreads();
  for (int o = 1; o < kVioBlock; o <<= 1) {
    const int32_t add = t >= o ? s_sum[t - o] : 0;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  int32_t run = s_sum[t] - sum;
  for (int b = b0; b < b1; ++b) {
    row_start[b] = run;
    const uint8_t* m = mask + (size_t)b * S;
    int32_t c = 1;
    for (int s = 0; s < S; ++s) c += m[s] != 0;
    run += c;
  }
  if (t == kVioBlock - 1) row_start[B] = s_sum[t];
}

template <typename TB, typename Rows>
__global__ __launch_bounds__(kVioBlock) void relation_violation_k(Rows rows, const uint8_t* __restrict__ canvas, int64_t n_nodes,
                                                                  const int32_t* __restrict__ off, const int32_t* __restrict__ src,
                                                                  const int32_t* __restrict__ dst, const int32_t* __restrict__ attr,
                                                                  const int64_t* __restrict__ first_node, int n_graph, int E,
                                                                  float* __restrict__ out, int32_t* __restrict__ edge_out,
                                                                  int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * kVioWaves + (threadIdx.x >> 6);  // uniform within a wavefront
  if (g >= n_graph) return;
  const int e0 = off[g], e1 = off[g + 1];
  if (e0 < 0 || e1 < e0 || e1 > E) {
    if (lane == 0) {
      atomicOr(err, kErrGraph);
      out[g] = NAN;
    }
    return;
  }
  const int64_t base = first_node[g];
  int failures = 0, valid = 0, bad = 0;
  for (int e = e0 + lane; e < e1; e += 64) {
    const int64_t i = base + src[e], j = base + dst[e];
    TB b1[4], b2[4];
    int code[3] = {-1, -1, -1};
    if (src[e] < 0 || dst[e] < 0 || i >= n_nodes || j >= n_nodes) {
      bad |= kErrGraph;
    } else if (!rows.load(i, b1) || !rows.load(j, b2)) {
      bad |= kErrRow;
    } else {
      const ldm_reldet::EdgeResult r = ldm_reldet::detect_edge(b1, b2, canvas[i] != 0, (int64_t)attr[e]);
      failures += r.failure;
      valid += r.valid;
      code[0] = r.size_code, code[1] = r.loc_code, code[2] = r.failure;
    }
    if (edge_out) {
      int32_t* o = edge_out + 3 * (size_t)e;
      o[0] = code[0], o[1] = code[1], o[2] = code[2];
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    failures += __shfl_xor(failures, o, 64);
    valid += __shfl_xor(valid, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (lane == 0) {
    if (bad) atomicOr(err, bad);
    out[g] = bad ? NAN : ldm_reldet::violation_score(failures, valid);
  }
}

inline unsigned blocks_for(int n_graph) { return (unsigned)((n_graph + kVioWaves - 1) / kVioWaves); }

template <typename TB, typename Rows>
void score(const Rows& rows, const ViolationGraph& g, float* out, int32_t* edge_out, int32_t* err, hipStream_t st) {
  hipLaunchKernelGGL((relation_violation_k<TB, Rows>), dim3(blocks_for(g.n_graph)), dim3(kVioBlock), 0, st, rows, g.canvas,
                     g.n_nodes, g.edge_off, g.src, g.dst, g.attr, g.first_node, g.n_graph, g.n_edge, out, edge_out, err);
}

}  // namespace

void launch_relation_violation(const void* bbox, int box_f64, int64_t n_rows, const ViolationGraph& g, float* out,
                               int32_t* edge_out, int32_t* err, hipStream_t st) {
  if (box_f64) score<double>(FlatRows<double>{static_cast<const double*>(bbox), n_rows}, g, out, edge_out, err, st);
  else score<float>(FlatRows<float>{static_cast<const float*>(bbox), n_rows}, g, out, edge_out, err, st);
}

void launch_relation_violation_dense(const void* bbox, int box_f64, const uint8_t* mask, int B, int S, int32_t* row_start,
                                     const ViolationGraph& g, float* out, int32_t* edge_out, int32_t* err, hipStream_t st) {
  hipLaunchKernelGGL(violation_rows_k, dim3(1), dim3(kVioBlock), 0, st, mask, B, S, row_start);
  if (box_f64)
    score<double>(DenseRows<double>{static_cast<const double*>(bbox), mask, row_start, B, S}, g, out, edge_out, err, st);
  else
    score<float>(DenseRows<float>{static_cast<const float*>(bbox), mask, row_start, B, S}, g, out, edge_out, err, st);
}

}  // namespace ldm
