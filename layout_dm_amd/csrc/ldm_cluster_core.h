// Coordinate bins from raw boxes — bin/clustering_coordinates.py: sklearn KMeans on one coordinate at a time and the reference's
// Percentile.fit (helpers/clustering.py:18-41) — ONE source of the arithmetic, compiled for the device (kernels_cluster.hip)
// and for the host (tests/cpu_cluster_check.cpp).  Everything works on ONE SORTED float32 array per coordinate, shared by every
// cluster count and restart; all sums are float64 in an order fixed here, so a device run repeats itself bit for bit and the
// host build repeats the device.  No floating-point atomics anywhere.
//
//   sort      LSD radix sort, 8 bits a pass, on order_key(x): an order-preserving map of the float32 bits (-0.0 sorts in front
//             of +0.0; both compare equal).  A NaN or an infinity sets kErrNonFinite.
//   prefix    PS[i] = sum of x[0..i), PS2 likewise of x^2 (exact products: a float32 squared fits a double), PS[0] = 0.  Order:
//             a tile of kScanTile elements is cut into kBlock chunks of kScanChunk consecutive elements; a chunk is summed left
//             to right from 0; the chunks of a tile are summed left to right from 0; the tiles are summed left to right from 0;
//             PS[i + 1] = (tiles in front + chunks in front) + running sum of the chunk.  (prefix_host)
//   seeding   greedy k-means++ (sklearn _kmeans_plusplus): the first centre is data point floor(u n); every further centre draws
//             n_candidates(k) = 2 + int(ln k) data points by inverse CDF over d(i) = squared distance to the nearest chosen centre
//             and keeps the one that leaves the smallest potential, the first drawn on equal potentials.  d(i) is recomputed from
//             the sorted centre list (the nearest centre of a point is one of the two around it), never stored.  The cumulative
//             weight is taken in a fixed order — tile_sum over tiles of kSeedTile points, the tiles left to right, then the points
//             of the tile left to right (inverse_cdf_pick) — and the pick is the FIRST index whose cumulative weight EXCEEDS
//             u * total, so a zero-weight point (a chosen centre, a duplicate of one) is never drawn; where rounding leaves no
//             such index it is the last point of positive weight.  sklearn's searchsorted takes the first index that REACHES the
//             value and can draw a zero-weight point; the distributions agree except on that null set.
//             Uniforms: Philox4x32-10, key = random_state, counter = (step, candidate, problem id, restart): the distribution
//             of sklearn's draws, not its stream.
//   Lloyd     centres stay sorted; cluster j is the index range (b[j-1], b[j]] cut at the float64 midpoints (c[j] + c[j+1]) / 2,
//             x <= midpoint going to the LOWER cluster (the lowest index on a tie, as kmeans encode in ldm_cond_core.h); each
//             boundary is a binary search; the new centre is (PS[hi] - PS[lo]) / (hi - lo).  An EMPTY cluster keeps its centre
//             (sklearn relocates it to the point farthest from its centre; the order of the centres is kept either way here).
//             sklearn's stopping rule (_kmeans_single_lloyd): after an iteration, stop if no boundary moved against the previous
//             iteration's, else if the sum of squared centre shifts <= tol * var(X); n_iter counts the iterations run.
//   inertia   one direct pass of (x - c)^2 over the final assignment (prefix sums would lose ~12 k^2 ulps to cancellation).
//   percentile  on the sorted DISTINCT values X[0..m) of clip(x, 0, 1): thresholds X[int(t_i m)], t_i = i * (1 / k) in float64
//             (numpy's linspace(0, 1, k + 1)[:-1]); value r belongs to the LAST i with int(t_i m) <= r, so bin i is the rank range
//             [idx_i, idx_{i+1}) and is empty where the two are equal; centre = float32(mean in float64), -1.0f for an empty bin.
#pragma once
#include <cmath>
#include <cstdint>

#include "ldm_post_token.h"

#if defined(__HIPCC__)
#define LDM_CL_HD __host__ __device__ __forceinline__
#else
#define LDM_CL_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum is rounded: host and device builds give the same bits
#endif

namespace ldm_cluster {

constexpr int kMaxK = 256;        // the tool's largest cluster count
constexpr int kBlock = 256;       // threads per workgroup of every kernel
constexpr int kSortTile = 2048;   // keys per workgroup of a radix pass
constexpr int kScanChunk = 16;    // consecutive elements one thread sums
constexpr int kScanTile = kBlock * kScanChunk;
constexpr int kSeedPer = 4;       // consecutive points per thread of a seeding / inertia tile
constexpr int kSeedTile = kBlock * kSeedPer;
constexpr int kMaxCand = 7;       // n_candidates(kMaxK)
enum : int { kErrNonFinite = 1 };

LDM_CL_HD int64_t n_tiles(int64_t n, int tile) { return (n + tile - 1) / tile; }

// ---- sort keys ----------------------------------------------------------------------------------------------------------
LDM_CL_HD uint32_t float_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}
LDM_CL_HD float bits_float(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}
LDM_CL_HD uint32_t order_key(float v) {
  const uint32_t b = float_bits(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LDM_CL_HD float key_value(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
LDM_CL_HD bool finite_bits(float v) { return (float_bits(v) & 0x7f800000u) != 0x7f800000u; }
LDM_CL_HD float clip01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// ---- randomness ---------------------------------------------------------------------------------------------------------
// 2 + int(ln k) for 1 <= k <= 402, in integers (e, e^2, ... e^5 = 2.72, 7.39, 20.09, 54.60, 148.41)
LDM_CL_HD int n_candidates(int k) { return 2 + (k >= 3) + (k >= 8) + (k >= 21) + (k >= 55) + (k >= 149); }
// uniform in [0, 1) with 53 random bits
LDM_CL_HD double uniform(uint64_t random_state, uint32_t problem, uint32_t restart, uint32_t step, uint32_t cand) {
  uint32_t r[4];
  ldm_post::philox4x32_10(step, cand, problem, restart, (uint32_t)random_state, (uint32_t)(random_state >> 32), r);
  return (double)(((uint64_t)(r[0] >> 5) << 26) | (uint64_t)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
}
LDM_CL_HD int64_t first_centre_index(double u, int64_t n) {
  const int64_t i = (int64_t)(u * (double)n);
  return i < n ? i : n - 1;
}

// ---- distances to a sorted centre list ----------------------------------------------------------------------------------
// squared distance of x to the nearest of the m sorted centres c (m >= 1)
LDM_CL_HD double nearest_d2(const double* c, int m, double x) {
  int lo = 0, hi = m;   // first centre >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] < x) lo = mid + 1; else hi = mid;
  }
  double best = INFINITY;
  if (lo < m) { const double t = x - c[lo]; best = t * t; }
  if (lo > 0) { const double t = x - c[lo - 1]; const double d = t * t; if (d < best) best = d; }
  return best;
}
// cluster of x under the midpoint rule: the first j whose upper midpoint is >= x, else k - 1
LDM_CL_HD int assign(const double* c, int k, double x) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x <= (c[mid] + c[mid + 1]) / 2) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// first index of the sorted x whose value exceeds `mid` (= the number of points <= mid)
LDM_CL_HD int64_t count_le(const float* x, int64_t n, double mid) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t m = lo + ((hi - lo) >> 1);
    if ((double)x[m] <= mid) lo = m + 1; else hi = m;
  }
  return lo;
}
LDM_CL_HD double new_centre(const double* ps, int64_t lo, int64_t hi, double old) {
  return hi > lo ? (ps[hi] - ps[lo]) / (double)(hi - lo) : old;
}
// var(X) from the prefix sums (the stopping threshold only)
LDM_CL_HD double variance(const double* ps, const double* ps2, int64_t n) {
  const double mean = ps[n] / (double)n;
  const double v = ps2[n] / (double)n - mean * mean;
  return v > 0.0 ? v : 0.0;
}

// ---- fixed-order tile sum: the order of the seeding kernels' reductions --------------------------------------------------
// part[t] = ((w[4t] + w[4t+1]) + w[4t+2]) + w[4t+3] (elements past `count` are 0), then part[t] += part[t + s], s = 128 .. 1
inline double tile_sum(const double* w, int count) {
  double part[kBlock];
  for (int t = 0; t < kBlock; ++t) {
    double s = 0.0;
    for (int e = 0; e < kSeedPer; ++e) {
      const int i = t * kSeedPer + e;
      s += i < count ? w[i] : 0.0;
    }
    part[t] = s;
  }
  for (int s = kBlock / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) part[t] += part[t + s];
  return part[0];
}

// the tile of the pick: the first tile whose inclusive cumulative sum exceeds target; *front = the sum of the tiles before it.
// None: the last tile of positive weight with target = +inf (its last positive point is taken), or tile 0 if all are zero.
LDM_CL_HD int64_t pick_tile(const double* tile_w, int64_t tiles, double& target, double* front) {
  double cum = 0.0, last_front = 0.0;
  int64_t last = 0;
  for (int64_t t = 0; t < tiles; ++t) {
    const double nc = cum + tile_w[t];
    if (nc > target) { *front = cum; return t; }
    if (tile_w[t] > 0.0) last = t, last_front = cum;
    cum = nc;
  }
  target = INFINITY;
  *front = last_front;
  return last;
}
// inside the tile: W(i) = weight of point i of the tile (i < count), walked left to right from `front`
template <class W>
LDM_CL_HD int pick_in_tile(const W& w, int count, double front, double target) {
  double cum = front;
  int last = count - 1;
  for (int i = 0; i < count; ++i) {
    const double wi = w(i);
    cum += wi;
    if (cum > target) return i;
    if (wi > 0.0) last = i;
  }
  return last;
}

// ---- percentile ---------------------------------------------------------------------------------------------------------
LDM_CL_HD int64_t percentile_index(int i, int k, int64_t m) {
  if (i >= k) return m;
  const double t = (double)i * (1.0 / (double)k);
  const int64_t r = (int64_t)(t * (double)m);
  return r < m ? r : m - 1;
}
LDM_CL_HD float percentile_centre(const double* ps_unique, int64_t lo, int64_t hi) {
  return hi > lo ? (float)((ps_unique[hi] - ps_unique[lo]) / (double)(hi - lo)) : -1.0f;
}

// ==== host forms (the device kernels repeat these orders) ================================================================
#if !defined(__HIP_DEVICE_COMPILE__)

inline void prefix_host(const float* x, int64_t n, double* ps, double* ps2) {
  ps[0] = 0.0, ps2[0] = 0.0;
  double tf = 0.0, tf2 = 0.0;   // tiles in front
  for (int64_t t0 = 0; t0 < n; t0 += kScanTile) {
    double cf = 0.0, cf2 = 0.0;   // chunks in front, inside the tile
    for (int c = 0; c < kBlock; ++c) {
      const double base = tf + cf, base2 = tf2 + cf2;
      double run = 0.0, run2 = 0.0;
      for (int e = 0; e < kScanChunk; ++e) {
        const int64_t i = t0 + (int64_t)c * kScanChunk + e;
        if (i >= n) break;
        const double v = (double)x[i];
        run += v, run2 += v * v;
        ps[i + 1] = base + run, ps2[i + 1] = base2 + run2;
      }
      cf += run, cf2 += run2;
    }
    tf += cf, tf2 += cf2;
  }
}

// weights w[0..n) -> index of the pick for uniform u (the seeding's inverse CDF, on explicit weights)
inline int64_t inverse_cdf_pick(const double* w, int64_t n, double u) {
  const int64_t tiles = n_tiles(n, kSeedTile);
  double* tw = new double[tiles];
  double total = 0.0;
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t rest = n - t * kSeedTile;
    tw[t] = tile_sum(w + t * kSeedTile, rest < kSeedTile ? (int)rest : kSeedTile);
    total += tw[t];
  }
  double target = u * total, front = 0.0;
  const int64_t t = pick_tile(tw, tiles, target, &front);
  delete[] tw;
  const int64_t rest = n - t * kSeedTile;
  const double* wt = w + t * kSeedTile;
  return t * kSeedTile + pick_in_tile([wt](int i) { return wt[i]; }, rest < kSeedTile ? (int)rest : kSeedTile, front, target);
}

// Lloyd from explicit sorted start centres; trace (max_iter, k) receives the centres after each iteration (or nullptr).
// tol_abs = tol * var(X).  Returns n_iter.
inline int lloyd_host(const float* x, const double* ps, int64_t n, int k, double* c, int max_iter, double tol_abs, double* trace) {
  int64_t* prev = new int64_t[k];
  int64_t* b = new int64_t[k];
  double* nc = new double[k];
  for (int j = 0; j < k; ++j) prev[j] = -1;
  int n_iter = 0;
  for (int it = 0; it < max_iter; ++it) {
    for (int j = 0; j < k; ++j) b[j] = j < k - 1 ? count_le(x, n, (c[j] + c[j + 1]) / 2) : n;
    bool moved = false;
    double shift = 0.0;
    for (int j = 0; j < k; ++j) {
      nc[j] = new_centre(ps, j ? b[j - 1] : 0, b[j], c[j]);
      moved |= b[j] != prev[j];
      const double d = nc[j] - c[j];
      shift += d * d;
    }
    for (int j = 0; j < k; ++j) c[j] = nc[j], prev[j] = b[j];
    if (trace)
      for (int j = 0; j < k; ++j) trace[(int64_t)it * k + j] = c[j];
    n_iter = it + 1;
    if (!moved || shift <= tol_abs) break;
  }
  delete[] prev, delete[] b, delete[] nc;
  return n_iter;
}

inline double inertia_host(const float* x, int64_t n, const double* c, int k) {
  double total = 0.0;
  for (int64_t t0 = 0; t0 < n; t0 += kSeedTile) {
    double w[kSeedTile];
    const int count = n - t0 < kSeedTile ? (int)(n - t0) : kSeedTile;
    for (int i = 0; i < count; ++i) {
      const double v = (double)x[t0 + i], d = v - c[assign(c, k, v)];
      w[i] = d * d;
    }
    total += tile_sum(w, count);
  }
  return total;
}

// sorted distinct values u[0..m) -> k float32 centres
inline void percentile_host(const float* u, int64_t m, int k, float* centres) {
  double* ps = new double[m + 1];
  double* ps2 = new double[m + 1];
  prefix_host(u, m, ps, ps2);
  for (int i = 0; i < k; ++i) centres[i] = percentile_centre(ps, percentile_index(i, k, m), percentile_index(i + 1, k, m));
  delete[] ps, delete[] ps2;
}

#endif  // host forms

}  // namespace ldm_cluster
