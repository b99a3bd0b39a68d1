// Coordinate bins on the device: sort, prefix sums, greedy k-means++ seeding, Lloyd on the sorted array, direct inertia, the
// percentile fit and the nearest-centre ids (ldm_cluster_sort, ldm_kmeans1d_fit, ldm_kmeans1d_lloyd, ldm_percentile_fit,
// ldm_nearest_centre, ldm_dev_cluster_stages).  The arithmetic and every summation order is ldm_cluster_core.h, one source for
// these kernels and the host build the CPU tests run; this file adds what only the device has: the grids and the LDS staging.
//
// Every kernel is plain HIP C++.  Reductions are per-thread serial sums and LDS trees in a fixed order, tiles are combined by
// one thread left to right: no floating-point atomics, two runs give the same bits.  The only atomics are the integer LDS
// counters of the radix histogram, whose result does not depend on their order.  Grids run over (tile, problem); a run whose
// cluster count is already seeded leaves at once (the API sorts the problems by k so that these are a suffix never launched).
#include "ldm_kernels.h"
#include "ldm_cluster_core.h"
#include "ldm_cond_core.h"

namespace ldm {

namespace {

namespace K = ldm_cluster;
using K::kBlock;
using K::kMaxCand;
using K::kMaxK;
using K::kSeedPer;
using K::kSeedTile;

// ---- sort -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void to_keys_k(const float* __restrict__ x, int64_t total, int clip, uint32_t* __restrict__ keys,
                                                    int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  float v = x[i];
  if (!K::finite_bits(v)) *err = K::kErrNonFinite;   // (every thread that meets one stores the same value)
  if (clip) v = K::clip01(v);
  keys[i] = K::order_key(v);
}

__global__ __launch_bounds__(kBlock) void from_keys_k(const uint32_t* __restrict__ keys, int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < total) out[i] = K::key_value(keys[i]);
}

// hist[a][digit][block]
__global__ __launch_bounds__(kBlock) void radix_hist_k(const uint32_t* __restrict__ keys, int64_t n, int shift, int nb,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const int a = blockIdx.y, blk = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blk * K::kSortTile;
  for (int e = threadIdx.x; e < K::kSortTile; e += kBlock) {
    const int64_t i = t0 + e;
    if (i < n) atomicAdd(&h[(keys[(int64_t)a * n + i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[((int64_t)a * 256 + threadIdx.x) * nb + blk] = h[threadIdx.x];
}

// in place: counts -> first output index of (digit, block), digits in order and the blocks of a digit in order (stable)
__global__ __launch_bounds__(kBlock) void radix_scan_k(uint32_t* __restrict__ hist, int nb) {
  __shared__ uint32_t tot[256];
  const int a = blockIdx.x, d = threadIdx.x;
  uint32_t* row = hist + ((int64_t)a * 256 + d) * nb;
  uint32_t s = 0;
  for (int b = 0; b < nb; ++b) s += row[b];
  tot[d] = s;
  __syncthreads();
  uint32_t base = 0;
  for (int e = 0; e < d; ++e) base += tot[e];
  for (int b = 0; b < nb; ++b) {
    const uint32_t c = row[b];
    row[b] = base;
    base += c;
  }
}

// thread d walks the tile in order and writes the keys of digit d one after the other: stable by construction
__global__ __launch_bounds__(kBlock) void radix_scatter_k(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n,
                                                          int shift, int nb, const uint32_t* __restrict__ offs) {
  __shared__ uint32_t tile[K::kSortTile];
  const int a = blockIdx.y, blk = blockIdx.x;
  const int64_t t0 = (int64_t)blk * K::kSortTile;
  const int count = n - t0 < K::kSortTile ? (int)(n - t0) : K::kSortTile;
  for (int e = threadIdx.x; e < count; e += kBlock) tile[e] = in[(int64_t)a * n + t0 + e];
  __syncthreads();
  const uint32_t d = threadIdx.x;
  int64_t pos = (int64_t)a * n + offs[((int64_t)a * 256 + d) * nb + blk];
  for (int e = 0; e < count; ++e) {
    const uint32_t key = tile[e];
    if (((key >> shift) & 255u) == d) out[pos++] = key;   // pos stays below a * n + n: the offsets count exactly these keys
  }
}

// ---- prefix sums (K::prefix_host is the order) ----------------------------------------------------------------------------
struct ValueLoad {
  const float* x;
  __device__ __forceinline__ double operator()(int64_t i) const { return (double)x[i]; }
};
struct FlagLoad {   // 1 where a sorted value differs from the one in front of it: the prefix sum is the rank among distinct values
  const float* x;
  __device__ __forceinline__ double operator()(int64_t i) const { return i == 0 || x[i] != x[i - 1] ? 1.0 : 0.0; }
};

// WRITE = false: tile totals only; true: PS / PS2 with the tiles in front known
template <class LOAD, bool WRITE>
__global__ __launch_bounds__(kBlock) void scan_tile_k(const float* __restrict__ x, int64_t n, int64_t ntile, double* __restrict__ tile_tot,
                                                      const double* __restrict__ tile_front, double* __restrict__ ps,
                                                      double* __restrict__ ps2) {
  __shared__ double part[kBlock], part2[kBlock];
  const int a = blockIdx.y, t = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const LOAD load{x + (int64_t)a * n};
  const int64_t i0 = tile * K::kScanTile + (int64_t)t * K::kScanChunk;
  double run = 0.0, run2 = 0.0;
  for (int e = 0; e < K::kScanChunk; ++e) {
    const int64_t i = i0 + e;
    if (i >= n) break;
    const double v = load(i);
    run += v, run2 += v * v;
  }
  part[t] = run, part2[t] = run2;
  __syncthreads();
  double cf = 0.0, cf2 = 0.0;   // chunks in front, left to right from 0
  for (int c = 0; c < t; ++c) cf += part[c], cf2 += part2[c];
  if (!WRITE) {
    if (t == kBlock - 1) {
      tile_tot[((int64_t)a * ntile + tile) * 2] = cf + run;
      tile_tot[((int64_t)a * ntile + tile) * 2 + 1] = cf2 + run2;
    }
    return;
  }
  const double base = tile_front[((int64_t)a * ntile + tile) * 2] + cf;
  const double base2 = tile_front[((int64_t)a * ntile + tile) * 2 + 1] + cf2;
  double* o = ps + (int64_t)a * (n + 1);
  double* o2 = ps2 ? ps2 + (int64_t)a * (n + 1) : nullptr;
  if (tile == 0 && t == 0) {
    o[0] = 0.0;
    if (o2) o2[0] = 0.0;
  }
  run = 0.0, run2 = 0.0;
  for (int e = 0; e < K::kScanChunk; ++e) {
    const int64_t i = i0 + e;
    if (i >= n) break;
    const double v = load(i);
    run += v, run2 += v * v;
    o[i + 1] = base + run;
    if (o2) o2[i + 1] = base2 + run2;
  }
}

__global__ void scan_front_k(const double* __restrict__ tile_tot, int64_t ntile, double* __restrict__ tile_front) {
  const int a = blockIdx.x, w = threadIdx.x;   // two threads: the sum and the sum of squares
  double tf = 0.0;
  for (int64_t t = 0; t < ntile; ++t) {
    tile_front[((int64_t)a * ntile + t) * 2 + w] = tf;
    tf += tile_tot[((int64_t)a * ntile + t) * 2 + w];
  }
}

__global__ __launch_bounds__(kBlock) void compact_k(const float* __restrict__ sorted, const double* __restrict__ rank, int64_t n,
                                                    float* __restrict__ uniq, int64_t* __restrict__ m_out) {
  const int a = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* x = sorted + (int64_t)a * n;
  const double* r = rank + (int64_t)a * (n + 1);
  if (i == 0 || x[i] != x[i - 1]) uniq[(int64_t)a * n + (int64_t)r[i]] = x[i];   // r[i] < r[n] <= n
  if (i == n - 1) m_out[a] = (int64_t)r[n];
}

// ---- seeding --------------------------------------------------------------------------------------------------------------
struct Run {
  int q, p, r, arr, k, pid;
  const float* x;
};
__device__ __forceinline__ Run run_of(const ClusterFitArgs& a, int q) {
  Run u;
  u.q = q, u.p = q / a.n_init, u.r = q % a.n_init;
  u.arr = a.prob[3 * u.p], u.k = a.prob[3 * u.p + 1], u.pid = a.prob[3 * u.p + 2];
  u.x = a.sorted + (int64_t)u.arr * a.n;
  return u;
}
__device__ __forceinline__ double* wc_row(const ClusterFitArgs& a, int parity, int q, int cand) {
  return a.wc + (((int64_t)parity * a.Q + q) * kMaxCand + cand) * a.tiles;
}

// The draws of one step.  Lanes l < L find their candidate's tile (pick_tile, serial over the tile sums); the whole workgroup then
// recomputes the weights of those tiles into LDS, one row per candidate; lane l walks its row left to right (pick_in_tile).
__global__ __launch_bounds__(kBlock) void seed_pick_k(ClusterFitArgs a, int step) {
  __shared__ double cs[kMaxK], dl[kMaxCand][kSeedTile], front[kMaxCand], target[kMaxCand], un[kMaxCand];
  __shared__ int64_t tile[kMaxCand];
  const Run u = run_of(a, blockIdx.x);
  if (step >= u.k) return;
  const int tid = threadIdx.x, m = step, L = step == 0 ? 1 : K::n_candidates(u.k);
  for (int j = tid; j < m; j += kBlock) cs[j] = a.cs[(int64_t)u.q * kMaxK + j];
  if (tid < L) {
    un[tid] = K::uniform(a.random_state, (uint32_t)u.pid, (uint32_t)(a.first_restart + u.r), (uint32_t)step, (uint32_t)tid);
    if (step > 0) {
      const double* W = wc_row(a, (step - 1) & 1, u.q, a.best[u.q]);
      double tg = un[tid] * a.pot[u.q], fr = 0.0;
      tile[tid] = K::pick_tile(W, a.tiles, tg, &fr);
      target[tid] = tg, front[tid] = fr;
    }
  }
  __syncthreads();
  if (step > 0) {
    for (int l = 0; l < L; ++l) {
      const int64_t i0 = tile[l] * kSeedTile;
      for (int e = tid; e < kSeedTile; e += kBlock)
        if (i0 + e < a.n) dl[l][e] = K::nearest_d2(cs, m, (double)u.x[i0 + e]);
    }
    __syncthreads();
  }
  if (tid >= L) return;
  int64_t idx;
  if (step == 0) {
    idx = K::first_centre_index(un[tid], a.n);
  } else {
    const int64_t rest = a.n - tile[tid] * kSeedTile;
    const double* w = dl[tid];
    idx = tile[tid] * kSeedTile + K::pick_in_tile([w](int i) { return w[i]; }, rest < kSeedTile ? (int)rest : kSeedTile, front[tid],
                                                  target[tid]);
  }
  a.cand[(int64_t)u.q * kMaxCand + tid] = idx;
  if (a.t_unif) a.t_unif[(int64_t)step * kMaxCand + tid] = un[tid], a.t_cand[(int64_t)step * kMaxCand + tid] = idx;
}

__global__ __launch_bounds__(kBlock) void seed_pot_k(ClusterFitArgs a, int step) {
  __shared__ double cs[kMaxK], cc[kMaxCand], part[kMaxCand][kBlock];
  const Run u = run_of(a, blockIdx.y);
  if (step >= u.k) return;
  const int tid = threadIdx.x, m = step, L = step == 0 ? 1 : K::n_candidates(u.k);
  for (int j = tid; j < m; j += kBlock) cs[j] = a.cs[(int64_t)u.q * kMaxK + j];
  if (tid < L) cc[tid] = (double)u.x[a.cand[(int64_t)u.q * kMaxCand + tid]];
  __syncthreads();
  double s[kMaxCand];
#pragma unroll
  for (int l = 0; l < kMaxCand; ++l) s[l] = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * kSeedTile + (int64_t)tid * kSeedPer;
  for (int e = 0; e < kSeedPer; ++e) {
    const int64_t i = i0 + e;
    if (i >= a.n) break;
    const double v = (double)u.x[i];
    const double d = m ? K::nearest_d2(cs, m, v) : INFINITY;
    if (a.t_dist && m) a.t_dist[(int64_t)step * a.n + i] = d;
#pragma unroll
    for (int l = 0; l < kMaxCand; ++l)
      if (l < L) {
        const double t = v - cc[l], t2 = t * t;
        s[l] += t2 < d ? t2 : d;
      }
  }
#pragma unroll
  for (int l = 0; l < kMaxCand; ++l) part[l][tid] = s[l];
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int l = 0; l < L; ++l) part[l][tid] += part[l][tid + st];
    __syncthreads();
  }
  if (tid < L) wc_row(a, step & 1, u.q, tid)[blockIdx.x] = part[tid][0];
}

__global__ __launch_bounds__(64) void seed_choose_k(ClusterFitArgs a, int step) {
  __shared__ double sp[kMaxCand];
  const Run u = run_of(a, blockIdx.x);
  if (step >= u.k) return;
  const int tid = threadIdx.x, m = step, L = step == 0 ? 1 : K::n_candidates(u.k);
  if (tid < L) {
    const double* W = wc_row(a, step & 1, u.q, tid);
    double s = 0.0;
    for (int64_t t = 0; t < a.tiles; ++t) s += W[t];
    sp[tid] = s;
    if (a.t_pots) a.t_pots[(int64_t)step * kMaxCand + tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  int best = 0;
  for (int l = 1; l < L; ++l)
    if (sp[l] < sp[best]) best = l;   // the first drawn on equal potentials
  a.best[u.q] = best;
  a.pot[u.q] = sp[best];
  const int64_t idx = a.cand[(int64_t)u.q * kMaxCand + best];
  if (a.t_pick) a.t_pick[step] = idx;
  const double v = (double)u.x[idx];
  double* c = a.cs + (int64_t)u.q * kMaxK;
  int j = m;
  while (j > 0 && c[j - 1] > v) c[j] = c[j - 1], --j;   // m < k <= kMaxK: c[m] is inside the run's row
  c[j] = v;
}

// ---- Lloyd ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void lloyd_k(ClusterFitArgs a) {
  __shared__ double c[kMaxK], sh[kMaxK];
  __shared__ int64_t b[kMaxK];
  __shared__ int mv[kMaxK];
  __shared__ int stop;
  const Run u = run_of(a, blockIdx.x);
  const int j = threadIdx.x, k = u.k;
  const double* ps = a.ps + (int64_t)u.arr * (a.n + 1);
  const double tol_abs = a.tol * K::variance(ps, a.ps2 + (int64_t)u.arr * (a.n + 1), a.n);
  if (j < k) c[j] = a.cs[(int64_t)u.q * kMaxK + j];
  int64_t prev = -1;
  int n_iter = 0;
  __syncthreads();
  for (int it = 0; it < a.max_iter; ++it) {
    int64_t bj = a.n;
    if (j < k - 1) bj = K::count_le(u.x, a.n, (c[j] + c[j + 1]) / 2);
    if (j < k) b[j] = bj;
    __syncthreads();
    double ncj = 0.0;
    if (j < k) {
      ncj = K::new_centre(ps, j ? b[j - 1] : 0, bj, c[j]);
      const double d = ncj - c[j];
      sh[j] = d * d;
      mv[j] = bj != prev;
      prev = bj;
    }
    __syncthreads();
    if (j == 0) {
      double s = 0.0;
      int moved = 0;
      for (int jj = 0; jj < k; ++jj) s += sh[jj], moved |= mv[jj];
      stop = !moved || s <= tol_abs;
    }
    if (j < k) {
      c[j] = ncj;
      if (a.t_lloyd) a.t_lloyd[(int64_t)it * k + j] = ncj;
    }
    __syncthreads();
    n_iter = it + 1;
    if (stop) break;   // (uniform: written before the barrier above, rewritten only after two more)
  }
  if (j < k) a.cs[(int64_t)u.q * kMaxK + j] = c[j];
  if (j == 0) a.n_iter_q[u.q] = n_iter;
}

__global__ __launch_bounds__(kBlock) void inertia_tile_k(ClusterFitArgs a) {
  __shared__ double cs[kMaxK], part[kBlock];
  const Run u = run_of(a, blockIdx.y);
  const int tid = threadIdx.x;
  if (tid < u.k) cs[tid] = a.cs[(int64_t)u.q * kMaxK + tid];
  __syncthreads();
  double s = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * kSeedTile + (int64_t)tid * kSeedPer;
  for (int e = 0; e < kSeedPer; ++e) {
    const int64_t i = i0 + e;
    if (i >= a.n) break;
    const double v = (double)u.x[i], d = v - cs[K::assign(cs, u.k, v)];
    s += d * d;
  }
  part[tid] = s;
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  if (tid == 0) wc_row(a, 0, u.q, 0)[blockIdx.x] = part[0];
}

// per problem: the inertia of every restart (tiles left to right), the lowest wins, the lowest restart on a tie
__global__ __launch_bounds__(64) void finish_k(ClusterFitArgs a) {
  __shared__ double in[64];
  const int p = blockIdx.x, r = threadIdx.x;
  if (r < a.n_init) {
    const double* W = wc_row(a, 0, p * a.n_init + r, 0);
    double s = 0.0;
    for (int64_t t = 0; t < a.tiles; ++t) s += W[t];
    in[r] = s;
  }
  __syncthreads();
  int best = 0;
  for (int e = 1; e < a.n_init; ++e)
    if (in[e] < in[best]) best = e;
  const int q = p * a.n_init + best, k = a.prob[3 * p + 1];
  for (int j = r; j < kMaxK; j += 64) a.centres[(int64_t)p * kMaxK + j] = j < k ? a.cs[(int64_t)q * kMaxK + j] : 0.0;
  if (r == 0) a.inertia[p] = in[best], a.n_iter[p] = a.n_iter_q[q], a.best_restart[p] = a.first_restart + best;
}

// ---- percentile, nearest centre ---------------------------------------------------------------------------------------------
// idx (P, kMaxK + 1) int64: K::percentile_index evaluated by the host
__global__ __launch_bounds__(kBlock) void percentile_k(const double* __restrict__ ps_unique, int64_t n, const int32_t* __restrict__ prob,
                                                       const int64_t* __restrict__ idx, float* __restrict__ centres) {
  const int p = blockIdx.x, i = threadIdx.x, arr = prob[3 * p], k = prob[3 * p + 1];
  const int64_t* ix = idx + (int64_t)p * (kMaxK + 1);
  centres[(int64_t)p * kMaxK + i] = i < k ? K::percentile_centre(ps_unique + (int64_t)arr * (n + 1), ix[i], ix[i + 1]) : 0.0f;
}

__global__ __launch_bounds__(kBlock) void nearest_k(const float* __restrict__ x, int64_t n, const double* __restrict__ centres, int k,
                                                    int quant, int32_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  ldm_condb::Geometry g{0, k, quant, 0, 0, centres};
  ids[i] = ldm_condb::quantise(g, 0, x[i]);   // the rule of ldm_encode_cond, not a second one
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

static void launch_sort_stage(const ClusterSortArgs& s, hipStream_t st) {
  const int64_t n = s.n, total = n * s.A;
  const int nb = (int)K::n_tiles(n, K::kSortTile);
  hipLaunchKernelGGL(to_keys_k, dim3(blocks_of(total, kBlock)), dim3(kBlock), 0, st, s.x, total, s.clip, s.keys_a, s.err);
  uint32_t *in = s.keys_a, *out = s.keys_b;
  for (int shift = 0; shift < 32; shift += 8) {
    hipLaunchKernelGGL(radix_hist_k, dim3(nb, s.A), dim3(kBlock), 0, st, in, n, shift, nb, s.hist);
    hipLaunchKernelGGL(radix_scan_k, dim3(s.A), dim3(kBlock), 0, st, s.hist, nb);
    hipLaunchKernelGGL(radix_scatter_k, dim3(nb, s.A), dim3(kBlock), 0, st, in, out, n, shift, nb, s.hist);
    uint32_t* t = in;
    in = out, out = t;
  }
  hipLaunchKernelGGL(from_keys_k, dim3(blocks_of(total, kBlock)), dim3(kBlock), 0, st, in, total, s.sorted);   // (4 passes: `in` is keys_a)
}

void launch_cluster_sort(const ClusterSortArgs& s, int stages, hipStream_t st) {
  const int64_t n = s.n, total = n * s.A;
  if (stages & 1) launch_sort_stage(s, st);
  if (!(stages & 2)) return;
  const int64_t ntile = K::n_tiles(n, K::kScanTile);
  const dim3 grid((unsigned)ntile, s.A), block(kBlock);
  hipLaunchKernelGGL((scan_tile_k<ValueLoad, false>), grid, block, 0, st, s.sorted, n, ntile, s.tile_tot, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(scan_front_k, dim3(s.A), dim3(2), 0, st, s.tile_tot, ntile, s.tile_front);
  hipLaunchKernelGGL((scan_tile_k<ValueLoad, true>), grid, block, 0, st, s.sorted, n, ntile, nullptr, s.tile_front, s.ps, s.ps2);
  // distinct values: rank = prefix sum of the "differs from the value in front" flags (exact in float64), then compaction
  hipLaunchKernelGGL((scan_tile_k<FlagLoad, false>), grid, block, 0, st, s.sorted, n, ntile, s.tile_tot, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(scan_front_k, dim3(s.A), dim3(2), 0, st, s.tile_tot, ntile, s.tile_front);
  hipLaunchKernelGGL((scan_tile_k<FlagLoad, true>), grid, block, 0, st, s.sorted, n, ntile, nullptr, s.tile_front, s.rank, nullptr);
  (void)hipMemsetAsync(s.unique, 0, (size_t)total * sizeof(float), st);
  hipLaunchKernelGGL(compact_k, dim3(blocks_of(n, kBlock), s.A), block, 0, st, s.sorted, s.rank, n, s.unique, s.n_unique);
  hipLaunchKernelGGL((scan_tile_k<ValueLoad, false>), grid, block, 0, st, s.unique, n, ntile, s.tile_tot, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(scan_front_k, dim3(s.A), dim3(2), 0, st, s.tile_tot, ntile, s.tile_front);
  hipLaunchKernelGGL((scan_tile_k<ValueLoad, true>), grid, block, 0, st, s.unique, n, ntile, nullptr, s.tile_front, s.ps_unique, nullptr);
}

void launch_cluster_fit(const ClusterFitArgs& a, const int32_t* h_k, int seed, hipStream_t st) {
  if (seed) {
    for (int step = 0; step < h_k[0]; ++step) {
      int live = 0;   // problems are sorted by k, largest first: the runs still seeding are a prefix
      while (live < a.P && h_k[live] > step) ++live;
      const unsigned q = (unsigned)(live * a.n_init);
      hipLaunchKernelGGL(seed_pick_k, dim3(q), dim3(kBlock), 0, st, a, step);
      hipLaunchKernelGGL(seed_pot_k, dim3((unsigned)a.tiles, q), dim3(kBlock), 0, st, a, step);
      hipLaunchKernelGGL(seed_choose_k, dim3(q), dim3(64), 0, st, a, step);
    }
  }
  hipLaunchKernelGGL(lloyd_k, dim3(a.Q), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(inertia_tile_k, dim3((unsigned)a.tiles, a.Q), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(finish_k, dim3(a.P), dim3(64), 0, st, a);
}

void launch_percentile(const double* ps_unique, int64_t n, const int32_t* prob, const int64_t* idx, int P, float* centres,
                       hipStream_t st) {
  hipLaunchKernelGGL(percentile_k, dim3(P), dim3(kBlock), 0, st, ps_unique, n, prob, idx, centres);
}

void launch_nearest_centre(const float* x, int64_t n, const double* centres, int k, int quant, int32_t* ids, hipStream_t st) {
  hipLaunchKernelGGL(nearest_k, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, x, n, centres, k, quant, ids);
}

}  // namespace ldm
