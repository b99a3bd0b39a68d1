// Host build of layout_dm_amd/csrc/ldm_cluster_core.h (the arithmetic and the summation orders of kernels_cluster.hip), driven by
// tests/test_clustering.py and, for the bit-for-bit comparisons with the device, by tests/test_clustering_gpu.py.
//
//   cpu_cluster_check MODE in.bin out.bin        (all integers int32 unless said, little endian)
//   percentile  in: n, k, float32 x[n]                          out: int64 m, float32 centres[k]
//   lloyd       in: n, k, max_iter, float64 tol, float32 x[n], float64 start[k]
//                                                               out: n_iter, float64 inertia, centres[k], trace[n_iter][k]
//   prefix      in: n, float32 x[n] (taken as it is)            out: float64 ps[n + 1], ps2[n + 1]
//   pick        in: n, nu, float64 w[n], float64 u[nu]          out: int64 index[nu]
//   philox      in: uint64 random_state, m, {problem, restart, step, cand}[m]   out: float64 u[m]
// exit 2: malformed input or refused sizes (n < 1, k < 1, k > 256); 3: a NaN or an infinity; 5: kmeans with fewer distinct
// values than k (out: int64 distinct count)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_cluster_core.h"
#include "cpu_check_io.h"

namespace {

namespace K = ldm_cluster;
using check_io::write_vec;

struct Reader {
  FILE* f;
  bool ok = true;
  template <class T>
  T one() {
    T v{};
    ok = ok && fread(&v, sizeof(T), 1, f) == 1;
    return v;
  }
  template <class T>
  std::vector<T> many(size_t n) {
    std::vector<T> v;
    ok = ok && check_io::read_vec(f, v, n);
    return v;
  }
};

// the device's sort: ascending order keys (-0.0 in front of +0.0)
bool sort_values(std::vector<float>& x, bool clip) {
  std::vector<uint32_t> keys(x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    if (!K::finite_bits(x[i])) return false;
    keys[i] = K::order_key(clip ? K::clip01(x[i]) : x[i]);
  }
  std::sort(keys.begin(), keys.end());
  for (size_t i = 0; i < x.size(); ++i) x[i] = K::key_value(keys[i]);
  return true;
}

std::vector<float> distinct(const std::vector<float>& sorted) {
  std::vector<float> u;
  for (size_t i = 0; i < sorted.size(); ++i)
    if (i == 0 || sorted[i] != sorted[i - 1]) u.push_back(sorted[i]);
  return u;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 1;
  const char* mode = argv[1];
  FILE* fi = fopen(argv[2], "rb");
  FILE* fo = fopen(argv[3], "wb");
  if (!fi || !fo) return 1;
  Reader in{fi};
  int rc = 0;
  if (!strcmp(mode, "percentile") || !strcmp(mode, "lloyd")) {
    const bool lloyd = mode[0] == 'l';
    const int n = in.one<int32_t>(), k = in.one<int32_t>();
    const int max_iter = lloyd ? in.one<int32_t>() : 0;
    const double tol = lloyd ? in.one<double>() : 0.0;
    if (!in.ok || n < 1 || k < 1 || k > K::kMaxK || (lloyd && max_iter < 1)) return 2;
    std::vector<float> x = in.many<float>(n);
    std::vector<double> c = in.many<double>(lloyd ? k : 0);
    if (!in.ok) return 2;
    if (!sort_values(x, !lloyd)) return 3;
    const std::vector<float> u = distinct(x);
    const int64_t m = (int64_t)u.size();
    if (!lloyd) {
      std::vector<float> centres(k);
      K::percentile_host(u.data(), m, k, centres.data());
      write_vec(fo, &m, 1), write_vec(fo, centres.data(), k);
    } else if (m < k) {
      write_vec(fo, &m, 1);
      rc = 5;
    } else {
      std::sort(c.begin(), c.end());
      std::vector<double> ps(n + 1), ps2(n + 1), trace((size_t)max_iter * k);
      K::prefix_host(x.data(), n, ps.data(), ps2.data());
      const int32_t n_iter = K::lloyd_host(x.data(), ps.data(), n, k, c.data(), max_iter, tol * K::variance(ps.data(), ps2.data(), n),
                                           trace.data());
      const double inertia = K::inertia_host(x.data(), n, c.data(), k);
      write_vec(fo, &n_iter, 1), write_vec(fo, &inertia, 1), write_vec(fo, c.data(), k), write_vec(fo, trace.data(), (size_t)n_iter * k);
    }
  } else if (!strcmp(mode, "prefix")) {
    const int n = in.one<int32_t>();
    if (!in.ok || n < 1) return 2;
    const std::vector<float> x = in.many<float>(n);
    if (!in.ok) return 2;
    std::vector<double> ps(n + 1), ps2(n + 1);
    K::prefix_host(x.data(), n, ps.data(), ps2.data());
    write_vec(fo, ps.data(), n + 1), write_vec(fo, ps2.data(), n + 1);
  } else if (!strcmp(mode, "pick")) {
    const int n = in.one<int32_t>(), nu = in.one<int32_t>();
    if (!in.ok || n < 1 || nu < 0) return 2;
    const std::vector<double> w = in.many<double>(n), u = in.many<double>(nu);
    if (!in.ok) return 2;
    for (int i = 0; i < nu; ++i) {
      const int64_t idx = K::inverse_cdf_pick(w.data(), n, u[i]);
      write_vec(fo, &idx, 1);
    }
  } else if (!strcmp(mode, "philox")) {
    const uint64_t state = in.one<uint64_t>();
    const int m = in.one<int32_t>();
    if (!in.ok || m < 0) return 2;
    const std::vector<int32_t> q = in.many<int32_t>((size_t)m * 4);
    if (!in.ok) return 2;
    for (int i = 0; i < m; ++i) {
      const double u = K::uniform(state, (uint32_t)q[4 * i], (uint32_t)q[4 * i + 1], (uint32_t)q[4 * i + 2], (uint32_t)q[4 * i + 3]);
      write_vec(fo, &u, 1);
    }
  } else {
    return 1;
  }
  fclose(fi), fclose(fo);
  return rc;
}
