// Host build of layout_dm_amd/csrc/ldm_vb_core.h with a timestep and a Philox layout index PER LAYOUT (row_t / row_layout: what
// kernels_vb.hip does when VbArgs.t_rows / layout_rows are set, the ldm_*_t entry points).  tests/test_per_layout_t_host.py holds
// its rows to tests/cpu_vb_check.cpp run at that row's t, and runs it once more built with -fsanitize=address,undefined.
//
//   cpu_vb_t_check logits in.bin out.bin    per-token kl / nll / aux / hit and the per-layout sums from logits
//   cpu_vb_t_check draw in.bin out.bin      x_t ~ q(x_t | x_0)
//
// in:  the case file of cpu_vb_check (its t is ignored), then int32 t_rows [B], uint64 layout_rows [B]
// out: as cpu_vb_check
// exit 2: malformed input
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_vb_core.h"
#include "cpu_check_io.h"

namespace {

namespace P = ldm_post;
namespace V = ldm_vb;

template <bool F64>
V::Terms one_token(const P::TokenArgs& a, int x0, const P::StepSchedule& s) {
  const P::HostLane g;
  if (a.count + 2 <= P::kHostMaxLive) return V::token_terms<F64, P::HostLane, P::SlotMap<1, P::kHostMaxLive, true>>(g, {0}, a, x0, s);
  return V::token_terms<F64, P::HostLane, P::SlotMap<1, 192, false>>(g, {0}, a, x0, s);   // vanilla: the full-vocabulary map
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 1;
  const bool draw = !strcmp(argv[1], "draw");
  if (!draw && strcmp(argv[1], "logits")) return 1;
  FILE* f = check_io::open_or_exit(argv[2], "rb", 1);
  int32_t hdr[9 + 16];
  uint64_t key[2];
  if (fread(hdr, 4, 25, f) != 25 || fread(key, 8, 2, f) != 2) return 2;
  const int C = hdr[0], n_attr = hdr[1], pad_id = hdr[2], mask_id = hdr[3], T = hdr[4], B = hdr[6], S = hdr[7], f64 = hdr[8];
  if (C < 3 || C > 192 || n_attr < 1 || n_attr > 8 || T < 1 || B < 0 || S < 1) return 2;
  const size_t n = (size_t)B * S;
  std::vector<float> sched, rows;
  std::vector<int32_t> x0, xt, t_rows;
  std::vector<uint64_t> layout_rows;
  if (!check_io::read_vec(f, sched, (size_t)8 * n_attr * (T + 1)) || !check_io::read_vec(f, x0, n)) return 2;
  if (!draw && (!check_io::read_vec(f, xt, n) || !check_io::read_vec(f, rows, n * C))) return 2;
  if (!check_io::read_vec(f, t_rows, (size_t)B) || !check_io::read_vec(f, layout_rows, (size_t)B)) return 2;
  fclose(f);
  for (int b = 0; b < B; ++b)
    if (t_rows[b] < 0 || t_rows[b] >= T) return 2;

  int32_t err = 0;
  std::vector<int32_t> out_xt(draw ? n : 0);
  std::vector<float> out_tok(draw ? 0 : 4 * n);
  std::vector<double> sums(draw ? 0 : (size_t)B * V::kNumSums);
  for (int b = 0; b < B; ++b) {
    const int t = V::row_t(t_rows.data(), -1, b);
    for (int s = 0; s < S; ++s) {
      const size_t row = (size_t)b * S + s;
      const int attr = s % n_attr;
      P::TokenArgs a{};
      a.start = hdr[9 + attr];
      a.count = hdr[17 + attr];
      a.pad_id = pad_id;
      a.mask_id = mask_id;
      a.n_class = C;
      if (a.count + 2 > 192) return 2;
      const int e = V::token_error(a, x0[row], !draw, draw ? 0 : xt[row]);
      err |= e;
      if (draw) {
        out_xt[row] = e ? mask_id
                        : V::q_sample_token(a, x0[row], V::noise_schedule(sched.data(), n_attr, attr, T, t), (uint32_t)s, (uint32_t)t,
                                            V::row_layout(key[1], layout_rows.data(), b), key[0]);
        continue;
      }
      V::Terms r{0.f, 0.f, 0.f, 0};
      if (!e) {
        a.tok = xt[row];
        a.logits = rows.data() + row * C;
        const P::StepSchedule sc = V::step_schedule(sched.data(), n_attr, attr, T, t);
        r = f64 ? one_token<true>(a, x0[row], sc) : one_token<false>(a, x0[row], sc);
      }
      out_tok[V::kSumKl * n + row] = r.kl;
      out_tok[V::kSumNll * n + row] = r.nll;
      out_tok[V::kSumAux * n + row] = r.aux;
      out_tok[V::kSumHit * n + row] = (float)r.hit;
    }
    if (!draw)
      for (int q = 0; q < V::kNumSums; ++q) {   // positions left to right, in float64 (kernels_vb.hip)
        double acc = 0.0;
        for (int s = 0; s < S; ++s) acc += (double)out_tok[q * n + (size_t)b * S + s];
        sums[(size_t)b * V::kNumSums + q] = acc;
      }
  }
  f = check_io::open_or_exit(argv[3], "wb", 1);
  check_io::write_vec(f, &err, 1);
  check_io::write_vec(f, out_xt);
  check_io::write_vec(f, out_tok);
  check_io::write_vec(f, sums);
  fclose(f);
  return 0;
}
