// Host build of ldm_vb_core.h token_grad (the arithmetic of kernels_vb.hip vb_grad_k) on the one-lane group of ldm_post_token.h.
// tests/test_vb_grad_core.py runs it against the gradient the reference's own autograd recorded (tests/golden/vb_grad/reference.npz),
// and once more built with -fsanitize=address,undefined: every array is an exact-size allocation.
//
//   cpu_vb_grad_check grad in.bin out.bin     d loss / d logits of every token, the per-token terms and the per-layout sums
//   cpu_vb_grad_check terms in.bin out.bin    the terms and sums alone, through token_terms<true> (what the values-only call runs)
//
// in:  the case file of cpu_vb_check (its t and lse are ignored; C up to 576), then int32 t_rows [B], float64 coef [B][2]
// out: int32 error word, (grad) float32 [B][S][C], float32 [4][B][S] kl, nll, aux, hit, float64 sums [B][4]
// A refused token leaves a zero row.  exit 2: malformed input
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_vb_core.h"
#include "cpu_check_io.h"

namespace {

namespace P = ldm_post;
namespace V = ldm_vb;

// the slot maps of cpu_vb_check where it serves the vocabulary (C <= 192), the wide ones above
template <class F>
V::Terms with_map(const P::TokenArgs& a, F&& f) {
  if (a.count + 2 <= P::kHostMaxLive) return f(P::SlotMap<1, P::kHostMaxLive, true>{0});
  if (a.n_class <= 192) return f(P::SlotMap<1, 192, false>{0});   // vanilla: the full-vocabulary map
  if (a.count + 2 <= P::kHostMaxLiveWide) return f(P::SlotMap<1, P::kHostMaxLiveWide, true>{0});
  return f(P::SlotMap<1, 576, false>{0});
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 1;
  const bool grad = !strcmp(argv[1], "grad");
  if (!grad && strcmp(argv[1], "terms")) return 1;
  FILE* f = check_io::open_or_exit(argv[2], "rb", 1);
  int32_t hdr[9 + 16];
  uint64_t key[2];
  if (fread(hdr, 4, 25, f) != 25 || fread(key, 8, 2, f) != 2) return 2;
  const int C = hdr[0], n_attr = hdr[1], pad_id = hdr[2], mask_id = hdr[3], T = hdr[4], B = hdr[6], S = hdr[7];
  if (C < 3 || C > 576 || n_attr < 1 || n_attr > 8 || T < 1 || B < 0 || S < 1 || mask_id != C - 1) return 2;
  const size_t n = (size_t)B * S;
  std::vector<float> sched, rows;
  std::vector<double> coef;
  std::vector<int32_t> x0, xt, t_rows;
  if (!check_io::read_vec(f, sched, (size_t)8 * n_attr * (T + 1)) || !check_io::read_vec(f, x0, n)) return 2;
  if (!check_io::read_vec(f, xt, n) || !check_io::read_vec(f, rows, n * C)) return 2;
  if (!check_io::read_vec(f, t_rows, (size_t)B) || !check_io::read_vec(f, coef, (size_t)B * 2)) return 2;
  fclose(f);
  for (int b = 0; b < B; ++b)
    if (t_rows[b] < 0 || t_rows[b] >= T) return 2;

  int32_t err = 0;
  std::vector<float> out_grad(grad ? n * C : 0, 0.0f);
  std::vector<float> out_tok(4 * n);
  std::vector<double> sums((size_t)B * V::kNumSums);
  const P::HostLane g;
  for (int b = 0; b < B; ++b) {
    const int t = t_rows[b];
    for (int s = 0; s < S; ++s) {
      const size_t row = (size_t)b * S + s;
      const int attr = s % n_attr;
      P::TokenArgs a{};
      a.start = hdr[9 + attr];
      a.count = hdr[17 + attr];
      a.pad_id = pad_id;
      a.mask_id = mask_id;
      a.n_class = C;
      if (a.count < 0 || a.start < 0 || a.start + a.count > C) return 2;
      const int e = V::token_error(a, x0[row], true, xt[row]);
      err |= e;
      V::Terms r{0.f, 0.f, 0.f, 0};
      if (!e) {
        a.tok = xt[row];
        a.logits = rows.data() + row * C;
        const P::StepSchedule sc = V::step_schedule(sched.data(), n_attr, attr, T, t);
        const int x = x0[row];
        r = with_map(a, [&](auto m) {
          return grad ? V::token_grad(g, m, a, x, sc, coef[2 * b], coef[2 * b + 1], t == 0, out_grad.data() + row * C)
                      : V::token_terms<true>(g, m, a, x, sc);
        });
      }
      out_tok[V::kSumKl * n + row] = r.kl;
      out_tok[V::kSumNll * n + row] = r.nll;
      out_tok[V::kSumAux * n + row] = r.aux;
      out_tok[V::kSumHit * n + row] = (float)r.hit;
    }
    for (int q = 0; q < V::kNumSums; ++q) {   // positions left to right, in float64 (kernels_vb.hip)
      double acc = 0.0;
      for (int s = 0; s < S; ++s) acc += (double)out_tok[q * n + (size_t)b * S + s];
      sums[(size_t)b * V::kNumSums + q] = acc;
    }
  }
  f = check_io::open_or_exit(argv[3], "wb", 1);
  check_io::write_vec(f, &err, 1);
  check_io::write_vec(f, out_grad);
  check_io::write_vec(f, out_tok);
  check_io::write_vec(f, sums);
  fclose(f);
  return 0;
}
