// Host build of layout_dm_amd/csrc/ldm_eval_iou_core.h (the arithmetic of kernels_eval_iou.hip).  tests/test_eval_iou.py
// runs it against the reference-produced fixture tests/golden/eval_iou.npz.
//
// in:  int32 {mode, f64_1, f64_2, B, S}, bbox1 [B][S][4] (float64 if f64_1 else float32), label1 int64 [B][S], n1 int32 [B],
//      then the same for set 2 (f64_2).  Rows hold their n elements first.
// out (float64):
//   mode 0  average IoU of set 1:            [B][3] = BLT, VTN, painted cells of the 32 x 32 canvas
//   mode 1  DocSim of (set1[b], set2[b]):     [B]
//   mode 2  Max-IoU of (set1[b], set2[b]):    [B]   (rows sorted by label, same label multiset)
//   mode 3  IoU of set1[b][i] x set2[b][j]:   [B][S][S] in the compute type, widened (i < n1, j < n2; 0 elsewhere)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_eval_iou_core.h"
#include "cpu_check_io.h"

namespace {

struct HostState {
  double u_[ldm_eval::kMaxS + 1], v_[ldm_eval::kMaxS + 1], minv_[ldm_eval::kMaxS + 1];
  uint8_t p_[ldm_eval::kMaxS + 1], way_[ldm_eval::kMaxS + 1];
  double& u(int k) { return u_[k]; }
  double& v(int k) { return v_[k]; }
  double& minv(int k) { return minv_[k]; }
  uint8_t& p(int k) { return p_[k]; }
  uint8_t& way(int k) { return way_[k]; }
};

struct Set {
  bool f64 = false;
  std::vector<float> b32;
  std::vector<double> b64;
  std::vector<int64_t> label;
  std::vector<int32_t> n;
  template <typename T>
  const T* box(int b, int S) const;
};
template <>
const float* Set::box<float>(int b, int S) const { return b32.data() + (size_t)b * S * 4; }
template <>
const double* Set::box<double>(int b, int S) const { return b64.data() + (size_t)b * S * 4; }

bool read_set(FILE* f, Set& s, int f64, int B, int S) {
  s.f64 = f64 != 0;
  using check_io::read_vec;
  const size_t nb = (size_t)B * S * 4;
  if (!(s.f64 ? read_vec(f, s.b64, nb) : read_vec(f, s.b32, nb))) return false;
  return read_vec(f, s.label, (size_t)B * S) && read_vec(f, s.n, B);
}

template <typename C, typename T1, typename T2>
int run(int mode, const Set& s1, const Set& s2, int B, int S, std::vector<double>& out) {
  HostState st;
  int err = 0;
  for (int b = 0; b < B; ++b) {
    const T1* b1 = s1.box<T1>(b, S);
    const T2* b2 = s2.box<T2>(b, S);
    const int64_t* l1 = s1.label.data() + (size_t)b * S;
    const int64_t* l2 = s2.label.data() + (size_t)b * S;
    const int n1 = s1.n[b], n2 = s2.n[b];
    if (mode == 0) {
      double blt, vtn;
      auto valid = [&](int i) { return i < n1; };
      ldm_eval::average_iou(b1, S, valid, &blt, &vtn);
      out.push_back(blt);
      out.push_back(vtn);
      out.push_back((double)ldm_eval::union_cells(b1, S, valid));
    } else if (mode == 1) {
      out.push_back(ldm_eval::docsim_pair<C>(b1, l1, n1, b2, l2, n2, st, &err));
    } else if (mode == 2) {
      out.push_back(ldm_eval::max_iou_pair<C>(b1, b2, l1, n1, ldm_eval::kMaxS, st, &err));
    } else {
      for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j)
          out.push_back(i < n1 && j < n2 ? (double)ldm_eval::box_iou(ldm_eval::ltrb<C>(b1 + 4 * i), ldm_eval::ltrb<C>(b2 + 4 * j))
                                         : 0.0);
    }
  }
  return err;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = check_io::open_or_exit(argv[1], "rb", 1);
  int32_t hdr[5];
  if (fread(hdr, 4, 5, f) != 5) return 2;
  const int mode = hdr[0], B = hdr[3], S = hdr[4];
  if (S < 1 || S > ldm_eval::kMaxS || B < 0 || mode < 0 || mode > 3) return 2;
  Set s1, s2;
  if (!read_set(f, s1, hdr[1], B, S) || !read_set(f, s2, hdr[2], B, S)) return 2;
  fclose(f);
  std::vector<double> out;
  int err;
  if (mode == 0) {  // one layout set: its own dtype
    err = s1.f64 ? run<double, double, double>(0, s1, s1, B, S, out) : run<float, float, float>(0, s1, s1, B, S, out);
  } else if (!s1.f64 && !s2.f64) {
    err = run<float, float, float>(mode, s1, s2, B, S, out);
  } else if (s1.f64 && s2.f64) {
    err = run<double, double, double>(mode, s1, s2, B, S, out);
  } else if (s1.f64) {
    err = run<double, double, float>(mode, s1, s2, B, S, out);
  } else {
    err = run<double, float, double>(mode, s1, s2, B, S, out);
  }
  f = check_io::open_or_exit(argv[2], "wb", 1);
  check_io::write_vec(f, out);
  fclose(f);
  return err ? 3 : 0;
}
