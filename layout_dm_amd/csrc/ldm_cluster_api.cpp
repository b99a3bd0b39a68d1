// C-ABI of the coordinate-bin fits (include/ldm_hip.h, section "coordinate bins from raw boxes").  Handle-free like the cond=
// builder: device pointers, sizes, a caller-owned workspace, a stream; every argument is checked before anything is launched.
#include "../../include/ldm_hip.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "ldm_kernels.h"

#include "ldm_cluster_core.h"
#include "ldm_cond_core.h"

using namespace ldm;
namespace K = ldm_cluster;

namespace {

constexpr int kMaxInit = 64;          // restarts of one call (finish_k: one thread each)
constexpr int64_t kMaxN = 1ll << 30;  // values per array

struct Carver {   // hands out 256-byte aligned pieces of the workspace; with base == nullptr it only measures
  char* base;
  size_t used = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (count * sizeof(T) + 255) & ~size_t(255);
    return p;
  }
};

bool sizes_ok(int A, int64_t n, int P, int n_init) {
  return A >= 1 && A <= 1024 && n >= 1 && n <= kMaxN && P >= 0 && P <= 4096 && n_init >= 1 && n_init <= kMaxInit &&
         (int64_t)P * n_init <= 65535;
}

void carve_sort(Carver& c, int A, int64_t n, ClusterSortArgs& s) {
  s.keys_a = c.take<uint32_t>((size_t)A * n);
  s.keys_b = c.take<uint32_t>((size_t)A * n);
  s.hist = c.take<uint32_t>((size_t)A * 256 * K::n_tiles(n, K::kSortTile));
  s.tile_tot = c.take<double>((size_t)A * K::n_tiles(n, K::kScanTile) * 2);
  s.tile_front = c.take<double>((size_t)A * K::n_tiles(n, K::kScanTile) * 2);
  s.rank = c.take<double>((size_t)A * (n + 1));
}

void carve_fit(Carver& c, int64_t n, int P, int n_init, ClusterFitArgs& a) {
  const size_t Q = (size_t)P * n_init;
  a.n = n, a.tiles = K::n_tiles(n, K::kSeedTile), a.P = P, a.n_init = n_init, a.Q = (int)Q;
  a.cs = c.take<double>(Q * K::kMaxK);
  a.wc = c.take<double>(2 * Q * K::kMaxCand * (size_t)a.tiles);
  a.cand = c.take<int64_t>(Q * K::kMaxCand);
  a.pot = c.take<double>(Q);
  a.best = c.take<int32_t>(Q);
  a.n_iter_q = c.take<int32_t>(Q);
}

struct StageExtras {
  float* unique;
  double* ps_unique;
  int64_t* n_unique;
  int32_t* prob;
};
void carve_stage(Carver& c, int64_t n, StageExtras& e) {
  e.unique = c.take<float>((size_t)n);
  e.ps_unique = c.take<double>((size_t)n + 1);
  e.n_unique = c.take<int64_t>(1);
  e.prob = c.take<int32_t>(3);
}

// the one layout of the workspace, the same for every call: what a call does not use stays where it is
struct Pieces {
  ClusterSortArgs s{};
  ClusterFitArgs a{};
  StageExtras e{};
  int64_t* rank_table = nullptr;   // ldm_percentile_fit: (P, kMaxK + 1)
  size_t bytes = 0;
};
Pieces carve(void* d_work, int A, int64_t n, int P, int n_init) {
  Carver c{static_cast<char*>(d_work)};
  Pieces w;
  carve_sort(c, A, n, w.s);
  carve_fit(c, n, P, n_init, w.a);
  carve_stage(c, n, w.e);
  w.rank_table = c.take<int64_t>((size_t)P * (K::kMaxK + 1));
  w.bytes = c.used;
  return w;
}

// problems: array in [0, A), 1 <= k <= min(kMaxK, n), k non-increasing
bool problems_ok(const int32_t* h_prob, int P, int A, int64_t n) {
  if (P > 0 && !h_prob) return false;
  for (int p = 0; p < P; ++p) {
    const int arr = h_prob[3 * p], k = h_prob[3 * p + 1];
    if (arr < 0 || arr >= A || k < 1 || k > K::kMaxK || k > n) return false;
    if (p && k > h_prob[3 * p - 2]) return false;
  }
  return true;
}

int run_fit(ClusterFitArgs& a, const int32_t* h_prob, int seed, hipStream_t st) {
  std::vector<int32_t> ks(a.P);
  for (int p = 0; p < a.P; ++p) ks[p] = h_prob[3 * p + 1];
  (void)hipGetLastError();
  launch_cluster_fit(a, ks.data(), seed, st);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" int ldm_cluster_workspace_bytes(int A, int64_t n, int P, int n_init, size_t* bytes) {
  if (!bytes || !sizes_ok(A, n, P, n_init)) return -1;
  *bytes = carve(nullptr, A, n, P, n_init).bytes;
  return 0;
}

static bool work_ok(const void* d_work, size_t work_bytes, int A, int64_t n, int P, int n_init) {
  size_t need = 0;
  return d_work && (reinterpret_cast<uintptr_t>(d_work) & 255) == 0 && ldm_cluster_workspace_bytes(A, n, P, n_init, &need) == 0 &&
         work_bytes >= need;
}

extern "C" int ldm_cluster_sort(const float* d_x, int A, int64_t n, int clip01, int stages, float* d_sorted, double* d_ps, double* d_ps2,
                                float* d_unique, double* d_ps_unique, int64_t* d_n_unique, void* d_work, size_t work_bytes,
                                int32_t* d_err, void* stream) {
  if (!sizes_ok(A, n, 0, 1) || (int64_t)A * n > kMaxN || (clip01 != 0 && clip01 != 1) || stages < 1 || stages > 3) return -1;
  if (!d_x || !d_sorted || !d_ps || !d_ps2 || !d_unique || !d_ps_unique || !d_n_unique || !d_err) return -1;
  if (!work_ok(d_work, work_bytes, A, n, 0, 1)) return -1;
  ClusterSortArgs s = carve(d_work, A, n, 0, 1).s;
  s.x = d_x, s.A = A, s.n = n, s.clip = clip01, s.sorted = d_sorted, s.ps = d_ps, s.ps2 = d_ps2, s.unique = d_unique;
  s.ps_unique = d_ps_unique, s.n_unique = d_n_unique, s.err = d_err;
  (void)hipGetLastError();
  if ((stages & 1) && hipMemsetAsync(d_err, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return -2;
  launch_cluster_sort(s, stages, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

static int fit_common(const float* d_sorted, const double* d_ps, const double* d_ps2, int A, int64_t n, const int32_t* h_prob,
                      const int32_t* d_prob, int P, int n_init, int first_restart, uint64_t random_state, const double* d_start,
                      int max_iter, double tol, double* d_centres, double* d_inertia, int32_t* d_n_iter, int32_t* d_best_restart,
                      void* d_work, size_t work_bytes, void* stream) {
  if (!sizes_ok(A, n, P, n_init) || P < 1 || first_restart < 0 || max_iter < 1 || !(tol >= 0.0)) return -1;
  if (!d_sorted || !d_ps || !d_ps2 || !d_prob || !d_centres || !d_inertia || !d_n_iter || !d_best_restart) return -1;
  if (!problems_ok(h_prob, P, A, n) || !work_ok(d_work, work_bytes, A, n, P, n_init)) return -1;
  ClusterFitArgs a = carve(d_work, A, n, P, n_init).a;
  a.sorted = d_sorted, a.ps = d_ps, a.ps2 = d_ps2, a.first_restart = first_restart, a.prob = d_prob, a.random_state = random_state;
  a.max_iter = max_iter, a.tol = tol, a.centres = d_centres, a.inertia = d_inertia, a.n_iter = d_n_iter;
  a.best_restart = d_best_restart;
  if (d_start && hipMemcpyAsync(a.cs, d_start, (size_t)P * K::kMaxK * sizeof(double), hipMemcpyDeviceToDevice,
                                (hipStream_t)stream) != hipSuccess)
    return -2;
  return run_fit(a, h_prob, d_start == nullptr, (hipStream_t)stream);
}

extern "C" int ldm_kmeans1d_fit(const float* d_sorted, const double* d_ps, const double* d_ps2, int A, int64_t n,
                                const int32_t* h_prob, const int32_t* d_prob, int P, int n_init, int first_restart,
                                uint64_t random_state, int max_iter, double tol, double* d_centres, double* d_inertia,
                                int32_t* d_n_iter, int32_t* d_best_restart, void* d_work, size_t work_bytes, void* stream) {
  return fit_common(d_sorted, d_ps, d_ps2, A, n, h_prob, d_prob, P, n_init, first_restart, random_state, nullptr, max_iter, tol,
                    d_centres, d_inertia, d_n_iter, d_best_restart, d_work, work_bytes, stream);
}

extern "C" int ldm_kmeans1d_lloyd(const float* d_sorted, const double* d_ps, const double* d_ps2, int A, int64_t n,
                                  const int32_t* h_prob, const int32_t* d_prob, int P, const double* d_start, int max_iter,
                                  double tol, double* d_centres, double* d_inertia, int32_t* d_n_iter, double* d_trace,
                                  void* d_work, size_t work_bytes, void* stream) {
  if (!d_start || (d_trace && P != 1)) return -1;
  if (!sizes_ok(A, n, P, 1) || P < 1 || max_iter < 1 || !(tol >= 0.0)) return -1;
  if (!d_sorted || !d_ps || !d_ps2 || !d_prob || !d_centres || !d_inertia || !d_n_iter) return -1;
  if (!problems_ok(h_prob, P, A, n) || !work_ok(d_work, work_bytes, A, n, P, 1)) return -1;
  Pieces w = carve(d_work, A, n, P, 1);
  ClusterFitArgs& a = w.a;
  a.sorted = d_sorted, a.ps = d_ps, a.ps2 = d_ps2, a.prob = d_prob, a.max_iter = max_iter, a.tol = tol, a.centres = d_centres;
  a.inertia = d_inertia, a.n_iter = d_n_iter, a.t_lloyd = d_trace;
  a.best_restart = a.best;   // (rewritten last, by finish_k: not reported)
  (void)hipGetLastError();
  if (hipMemcpyAsync(a.cs, d_start, (size_t)P * K::kMaxK * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
      hipSuccess)
    return -2;
  return run_fit(a, h_prob, 0, (hipStream_t)stream);
}

extern "C" int ldm_percentile_fit(const double* d_ps_unique, int A, int64_t n, const int64_t* h_n_unique, const int32_t* h_prob,
                                  const int32_t* d_prob, int P, float* d_centres, void* d_work, size_t work_bytes, void* stream) {
  if (!sizes_ok(A, n, P, 1) || P < 1 || !d_ps_unique || !h_n_unique || !h_prob || !d_prob || !d_centres) return -1;
  if (!work_ok(d_work, work_bytes, A, n, P, 1)) return -1;
  std::vector<int64_t> idx((size_t)P * (K::kMaxK + 1), 0);
  for (int p = 0; p < P; ++p) {
    const int arr = h_prob[3 * p], k = h_prob[3 * p + 1];
    if (arr < 0 || arr >= A || k < 1 || k > K::kMaxK) return -1;
    const int64_t m = h_n_unique[arr];
    if (m < 1 || m > n) return -1;
    for (int i = 0; i <= k; ++i) idx[(size_t)p * (K::kMaxK + 1) + i] = K::percentile_index(i, k, m);
  }
  const Pieces w = carve(d_work, A, n, P, 1);
  int64_t* d_idx = w.rank_table;
  (void)hipGetLastError();
  if (hipMemcpyAsync(d_idx, idx.data(), idx.size() * sizeof(int64_t), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess)
    return -2;
  launch_percentile(d_ps_unique, n, d_prob, d_idx, P, d_centres, (hipStream_t)stream);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -2;   // `idx` is host memory of this call
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int ldm_nearest_centre(const float* d_x, int64_t n, const double* d_centres, int k, int quant, int32_t* d_ids,
                                  void* stream) {
  if (n < 0 || n > kMaxN || k < 1 || k > K::kMaxK || (quant != ldm_condb::kPercentile && quant != ldm_condb::kKMeans)) return -1;
  if (n == 0) return 0;
  if (!d_x || !d_centres || !d_ids) return -1;
  (void)hipGetLastError();
  launch_nearest_centre(d_x, n, d_centres, k, quant, d_ids, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int ldm_dev_cluster_stages(const float* d_x, int64_t n, int k, uint64_t random_state, int problem_id, int restart,
                                      int max_iter, double tol, float* d_sorted, double* d_ps, double* d_ps2, double* d_unif,
                                      int64_t* d_cand, double* d_pots, int64_t* d_pick, double* d_dist, double* d_lloyd,
                                      double* d_centres, double* d_inertia, int32_t* d_n_iter, void* d_work, size_t work_bytes,
                                      int32_t* d_err, void* stream) {
  if (!sizes_ok(1, n, 1, 1) || k < 1 || k > K::kMaxK || k > n || problem_id < 0 || restart < 0 || max_iter < 1 || !(tol >= 0.0))
    return -1;
  if (!d_x || !d_sorted || !d_ps || !d_ps2 || !d_unif || !d_cand || !d_pots || !d_pick || !d_lloyd || !d_centres || !d_inertia ||
      !d_n_iter || !d_err)
    return -1;
  if (!work_ok(d_work, work_bytes, 1, n, 1, 1)) return -1;
  hipStream_t st = (hipStream_t)stream;
  Pieces w = carve(d_work, 1, n, 1, 1);
  ClusterSortArgs& s = w.s;
  ClusterFitArgs& a = w.a;
  StageExtras& e = w.e;
  s.x = d_x, s.A = 1, s.n = n, s.clip = 0, s.sorted = d_sorted, s.ps = d_ps, s.ps2 = d_ps2, s.unique = e.unique;
  s.ps_unique = e.ps_unique, s.n_unique = e.n_unique, s.err = d_err;
  const int32_t h_prob[3] = {0, k, problem_id};
  (void)hipGetLastError();
  if (hipMemsetAsync(d_err, 0, sizeof(int32_t), st) != hipSuccess) return -2;
  if (hipMemcpyAsync(e.prob, h_prob, sizeof(h_prob), hipMemcpyHostToDevice, st) != hipSuccess) return -2;
  if (hipStreamSynchronize(st) != hipSuccess) return -2;   // `h_prob` is host memory of this call
  launch_cluster_sort(s, 3, st);
  a.sorted = d_sorted, a.ps = d_ps, a.ps2 = d_ps2, a.first_restart = restart, a.prob = e.prob, a.random_state = random_state;
  a.max_iter = max_iter, a.tol = tol, a.centres = d_centres, a.inertia = d_inertia, a.n_iter = d_n_iter;
  a.best_restart = a.best;   // (rewritten last, by finish_k: not reported)
  a.t_unif = d_unif, a.t_cand = d_cand, a.t_pots = d_pots, a.t_pick = d_pick, a.t_dist = d_dist, a.t_lloyd = d_lloyd;
  return run_fit(a, h_prob, 1, st);
}
