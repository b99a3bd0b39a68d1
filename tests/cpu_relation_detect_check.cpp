// Host build of layout_dm_amd/csrc/ldm_relation_detect_core.h (the arithmetic of kernels_violation.hip).
// tests/test_relation_violation.py runs it against the reference-produced fixture tests/golden/relation_violation/reference.npz.
//
// in:  int32 {f64, n_rows, n_nodes, n_graph, n_edge}, box [n_rows][4] (float64 if f64 else float32), canvas uint8 [n_nodes],
//      edge_off int32 [n_graph + 1], src / dst / attr int32 [n_edge] (local node ids), first_node int64 [n_graph]
// out: int32 [n_edge][4] = {size code, loc code, failure, valid} in CSR edge order, then float32 [n_graph] scores
// exit 3: an edge names a row beyond the boxes or a node beyond the canvas flags (nothing is read there)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_relation_detect_core.h"
#include "cpu_check_io.h"

namespace {

using check_io::read_vec;

template <typename TB>
int run(const std::vector<TB>& box, int64_t n_rows, const std::vector<uint8_t>& canvas, const std::vector<int32_t>& off,
        const std::vector<int32_t>& src, const std::vector<int32_t>& dst, const std::vector<int32_t>& attr,
        const std::vector<int64_t>& first, std::vector<int32_t>& edge, std::vector<float>& score) {
  const int n_graph = (int)first.size();
  int err = 0;
  for (int g = 0; g < n_graph; ++g) {
    int64_t failures = 0, valid = 0;
    for (int e = off[g]; e < off[g + 1]; ++e) {
      const int64_t i = first[g] + src[e], j = first[g] + dst[e];
      if (i < 0 || j < 0 || i >= n_rows || j >= n_rows || i >= (int64_t)canvas.size()) {
        err = 3;
        continue;
      }
      const ldm_reldet::EdgeResult r = ldm_reldet::detect_edge(&box[4 * i], &box[4 * j], canvas[i] != 0, (int64_t)attr[e]);
      edge[4 * (size_t)e] = r.size_code, edge[4 * (size_t)e + 1] = r.loc_code;
      edge[4 * (size_t)e + 2] = r.failure, edge[4 * (size_t)e + 3] = r.valid;
      failures += r.failure;
      valid += r.valid;
    }
    score[g] = ldm_reldet::violation_score(failures, valid);
  }
  return err;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = check_io::open_or_exit(argv[1], "rb", 1);
  int32_t hdr[5];
  if (fread(hdr, 4, 5, f) != 5) return 2;
  const int f64 = hdr[0], n_rows = hdr[1], n_nodes = hdr[2], n_graph = hdr[3], n_edge = hdr[4];
  if (n_rows < 0 || n_nodes < 0 || n_graph < 0 || n_edge < 0) return 2;
  std::vector<float> b32;
  std::vector<double> b64;
  std::vector<uint8_t> canvas;
  std::vector<int32_t> off, src, dst, attr;
  std::vector<int64_t> first;
  if (!(f64 ? read_vec(f, b64, (size_t)n_rows * 4) : read_vec(f, b32, (size_t)n_rows * 4))) return 2;
  if (!read_vec(f, canvas, n_nodes) || !read_vec(f, off, (size_t)n_graph + 1) || !read_vec(f, src, n_edge) ||
      !read_vec(f, dst, n_edge) || !read_vec(f, attr, n_edge) || !read_vec(f, first, n_graph))
    return 2;
  fclose(f);
  for (int g = 0; g < n_graph; ++g)
    if (off[g] < 0 || off[g + 1] < off[g] || off[g + 1] > n_edge) return 2;
  std::vector<int32_t> edge((size_t)n_edge * 4, -1);
  std::vector<float> score(n_graph);
  const int err = f64 ? run(b64, n_rows, canvas, off, src, dst, attr, first, edge, score)
                      : run(b32, n_rows, canvas, off, src, dst, attr, first, edge, score);
  f = check_io::open_or_exit(argv[2], "wb", 1);
  check_io::write_vec(f, edge);
  check_io::write_vec(f, score);
  fclose(f);
  return err;
}
