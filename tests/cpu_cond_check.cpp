// Host build of layout_dm_amd/csrc/ldm_cond_core.h — the one source of the cond= builder's arithmetic (kernels_cond.hip
// compiles the same header for the device).  tests/test_cond_builder.py drives it:
//   cpu_cond_check <in.bin> <out.bin>
// in:  int32 head[12] = {mode (0 encode, 1 graph), box_f64, B, E, n_category, n_bin, quant, rule, has_keep, has_noise,
//      has_selection, 0}, double edge_ratio, uint64 seed, uint64 first_layout, then bbox (B,E,4), label (B,E) int64,
//      mask (B,E) uint8, centres (4,n_bin) float64 if quant != 0, keep (B,E) uint8 if has_keep, noise (B,E,4) float32 if
//      has_noise, selection (B,2,E+1,E+1) uint8 if has_selection.
// out (encode): int32 err, seq (B,5E) int32, mask (B,5E) uint8, seq_orig (B,5E) int32, num_element (B) int32.
// out (graph):  int32 {err, n_edge, n_nodes}, edge_off (B+1) int32, src / dst / attr (n_edge) int32, first_node (B) int64,
//               node_label / node_batch (n_nodes) int64, node_box (n_nodes,4) in the boxes' dtype.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_cond_core.h"
#include "cpu_check_io.h"

using namespace ldm_condb;

struct Reader {
  std::vector<unsigned char> buf;
  size_t at = 0;
  template <typename T>
  const T* take(size_t n) {
    if (at + n * sizeof(T) > buf.size()) {
      fprintf(stderr, "cpu_cond_check: input too short\n");
      exit(2);
    }
    const T* p = reinterpret_cast<const T*>(buf.data() + at);
    at = (at + n * sizeof(T) + 7) & ~(size_t)7;   // every array starts on an 8-byte boundary
    return p;
  }
};

template <typename T>
static void put(FILE* f, const T* p, size_t n) {
  if (!check_io::write_vec(f, p, n)) exit(2);
}

struct Inputs {
  int B, E, n_category, n_bin, quant, rule;
  double edge_ratio;
  uint64_t seed, first_layout;
  const int64_t* label;
  const uint8_t *mask, *keep, *selection;
  const double* centres;
  const float* noise;
};

template <typename TB>
static void encode(const Inputs& in, const TB* bbox, FILE* out) {
  const int B = in.B, E = in.E;
  const int pad = in.n_category + 4 * in.n_bin;
  Geometry g{in.n_category, in.n_bin, in.quant, pad, pad + 1, in.centres};
  std::vector<int32_t> seq((size_t)B * E * kAttr), orig(seq.size(), 0), num(B);
  std::vector<uint8_t> cm(seq.size());
  int32_t err = 0;
  for (int b = 0; b < B; ++b) {
    const uint8_t* m = in.mask + (size_t)b * E;
    int n = 0;
    for (int e = 0; e < E; ++e) {
      n += m[e] != 0;
      if (e > 0 && m[e] && !m[e - 1]) err |= kErrPrefix;
    }
    num[b] = n;
    const uint64_t layout = in.first_layout + (uint64_t)b;
    for (int e = 0; e < E; ++e) {
      const size_t slot = (size_t)b * E + e;
      const bool valid = m[e] != 0;
      TB box[4];
      for (int k = 0; k < 4; ++k) box[k] = bbox[slot * 4 + k];
      if (in.rule == kRuleRefinement) {
        float z[4];
        if (in.noise) memcpy(z, in.noise + slot * 4, sizeof z);
        else noise4(in.seed, layout, e, z);
        for (int k = 0; k < 4; ++k) box[k] = box[k] + TB(z[k]);
      }
      int32_t tok[kAttr];
      err |= encode_element(g, box, in.label[slot], valid, tok);
      bool kept = false;
      if (in.rule == kRulePartial)
        kept = in.keep ? in.keep[slot] != 0 : (valid && partial_keep(in.seed, layout, m, E, e, partial_count(in.seed, layout, n)));
      apply_rule(g, in.rule, tok, valid, kept, &seq[slot * kAttr], &cm[slot * kAttr], &orig[slot * kAttr]);
    }
  }
  put(out, &err, 1);
  put(out, seq.data(), seq.size());
  put(out, cm.data(), cm.size());
  put(out, orig.data(), orig.size());
  put(out, num.data(), num.size());
}

template <typename TB>
static void graph(const Inputs& in, const TB* bbox, FILE* out) {
  const int B = in.B, E = in.E;
  std::vector<int32_t> off(B + 1, 0), src, dst, attr;
  std::vector<int64_t> first(B), y, batch;
  std::vector<TB> x;
  int32_t err = 0;
  for (int b = 0; b < B; ++b) {
    const uint8_t* m = in.mask + (size_t)b * E;
    int n = 0;
    for (int e = 0; e < E; ++e) {
      n += m[e] != 0;
      if (e > 0 && m[e] && !m[e - 1]) err |= kErrPrefix;
    }
    const int N = n + 1, P = n_pairs(N);
    std::vector<TB> box(4 * N);
    box[0] = box[1] = TB(0.5), box[2] = box[3] = TB(1);
    for (int i = 0; i < 4 * n; ++i) {
      box[4 + i] = bbox[(size_t)b * E * 4 + i];
      if (!finite(box[4 + i])) err |= kErrNonFinite;
    }
    first[b] = (int64_t)y.size();
    for (int k = 0; k < N; ++k) {
      const int64_t l = k ? in.label[(size_t)b * E + k - 1] : -1;
      if (k && (l < 0 || l >= in.n_category)) err |= kErrLabel;
      y.push_back(l + 1);
      batch.push_back(b);
    }
    x.insert(x.end(), box.begin(), box.end());
    std::vector<uint8_t> sel(2 * P, 0);
    if (in.selection) {
      const uint8_t* s = in.selection + (size_t)b * 2 * (E + 1) * (E + 1);
      for (int c = 0; c < 2 * P; ++c) {
        int i, j;
        pair_of(N, c % P, i, j);
        sel[c] = s[((c / P) * (E + 1) + i) * (E + 1) + j] != 0;
      }
    } else {
      const int size = relation_sample_size(N, in.edge_ratio);
      std::vector<uint32_t> score(2 * P + 4);
      for (int q = 0; 4 * q < 2 * P; ++q) {
        uint32_t r[4];
        draw4(in.seed, in.first_layout + (uint64_t)b, kDrawRelation, (uint32_t)q, r);
        for (int k = 0; k < 4; ++k) score[4 * q + k] = r[k];
      }
      for (int c = 0; c < 2 * P; ++c) {
        int ahead = 0;
        for (int o = 0; o < 2 * P; ++o) ahead += score[o] < score[c] || (score[o] == score[c] && o < c);
        sel[c] = ahead < size;
      }
    }
    for (int p = 0; p < P; ++p) {
      int i, j;
      pair_of(N, p, i, j);
      const int a = pair_attr(&box[4 * i], &box[4 * j], i == 0, sel[p] != 0, sel[P + p] != 0);
      if (a != kRelUnknown) src.push_back(i), dst.push_back(j), attr.push_back(a);
    }
    off[b + 1] = (int32_t)attr.size();
  }
  const int32_t head[3] = {err, (int32_t)attr.size(), (int32_t)y.size()};
  put(out, head, 3);
  put(out, off.data(), off.size());
  put(out, src.data(), src.size());
  put(out, dst.data(), dst.size());
  put(out, attr.data(), attr.size());
  put(out, first.data(), first.size());
  put(out, y.data(), y.size());
  put(out, batch.data(), batch.size());
  put(out, x.data(), x.size());
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = check_io::open_or_exit(argv[1], "rb", 2);
  Reader r;
  fseek(f, 0, SEEK_END);
  r.buf.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (!check_io::read_vec(f, r.buf, r.buf.size())) return 2;
  fclose(f);
  const int32_t* h = r.take<int32_t>(12);
  const int mode = h[0], f64 = h[1];
  Inputs in{};
  in.B = h[2], in.E = h[3], in.n_category = h[4], in.n_bin = h[5], in.quant = h[6], in.rule = h[7];
  if (in.B < 0 || in.E < 1 || in.E > kMaxElem || in.n_bin < 1 || in.n_bin > kMaxBin) return 2;
  in.edge_ratio = *r.take<double>(1);
  in.seed = *r.take<uint64_t>(1);
  in.first_layout = *r.take<uint64_t>(1);
  const size_t slots = (size_t)in.B * in.E;
  const void* bbox = f64 ? (const void*)r.take<double>(slots * 4) : (const void*)r.take<float>(slots * 4);
  in.label = r.take<int64_t>(slots);
  in.mask = r.take<uint8_t>(slots);
  in.centres = in.quant != kLinear ? r.take<double>(4 * (size_t)in.n_bin) : nullptr;
  in.keep = h[8] ? r.take<uint8_t>(slots) : nullptr;
  in.noise = h[9] ? r.take<float>(slots * 4) : nullptr;
  in.selection = h[10] ? r.take<uint8_t>((size_t)in.B * 2 * (in.E + 1) * (in.E + 1)) : nullptr;
  FILE* out = check_io::open_or_exit(argv[2], "wb", 2);
  if (mode == 0) f64 ? encode(in, (const double*)bbox, out) : encode(in, (const float*)bbox, out);
  else f64 ? graph(in, (const double*)bbox, out) : graph(in, (const float*)bbox, out);
  fclose(out);
  return 0;
}
