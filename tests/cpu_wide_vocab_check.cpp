// Host build of layout_dm_amd/csrc/ldm_post_token.h for the WIDE vocabularies (more than 192 classes: kernels_post.hip /
// kernels_vb.hip at CMAX = 576), driven by tests/test_wide_vocab_host.py.
//
//   slots n_category n_bin     the two slot maps the wide kernels instantiate — SlotMap<64, 3, LIVE> (step path) and
//                              SlotMap<64, 9, full> (parity hooks, vanilla) — over the 64 lanes of a wavefront, for every attribute
//                              of the vocabulary: every candidate is owned by exactly one (lane, slot), its class is the one the
//                              map's contract names (live: body in class order, [PAD], [MASK]; full: the class itself), nothing at
//                              or beyond n_cand is valid, and the scratch index stays inside the kernel's scratch rows (192 / 576).
//                              Prints "ok <candidates checked>"; exit code 5 with a message otherwise.
//   draw in.bin out.bin        the one-lane form step_token<true, kHostMaxLiveWide> (130 slots: a 128-bin attribute) on a case file
//                              in the layout of tests/cpu_post_token_check.cpp; writes the drawn tokens.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_post_token.h"
#include "cpu_check_io.h"

namespace P = ldm_post;

template <class M>
static long check_map(const P::TokenArgs& a, int scratch, const char* what) {
  const int n = M::LIVE ? a.count + 2 : a.n_class;
  if (n > M::NL * M::NJ) {
    fprintf(stderr, "%s: %d candidates exceed the map's %d slots\n", what, n, M::NL * M::NJ);
    exit(5);
  }
  std::vector<int> owners(M::NL * M::NJ, 0);
  for (int l = 0; l < M::NL; ++l) {
    const M m{l};
    if (m.n_cand(a) != n) exit(5);
    for (int j = 0; j < M::NJ; ++j) {
      const int i = m.sidx(j);
      if (i < 0 || i >= M::NL * M::NJ) exit(5);
      if (m.valid(a, j) != (i < n)) {
        fprintf(stderr, "%s: lane %d slot %d (candidate %d of %d): valid = %d\n", what, l, j, i, n, (int)m.valid(a, j));
        exit(5);
      }
      if (!m.valid(a, j)) {
        if (m.live(a, j)) exit(5);
        continue;
      }
      if (i >= scratch) {
        fprintf(stderr, "%s: candidate %d outside the %d scratch slots\n", what, i, scratch);
        exit(5);
      }
      owners[i] += 1;
      const int want = M::LIVE ? (i < a.count ? a.start + i : i == a.count ? a.pad_id : a.mask_id) : i;
      if (m.cls(a, j) != want || m.cls(a, j) < 0 || m.cls(a, j) >= a.n_class) {
        fprintf(stderr, "%s: candidate %d is class %d, expected %d\n", what, i, m.cls(a, j), want);
        exit(5);
      }
      if (m.live(a, j) != P::is_live(a, want)) exit(5);
    }
  }
  for (int i = 0; i < M::NL * M::NJ; ++i)
    if (owners[i] != (i < n ? 1 : 0)) {
      fprintf(stderr, "%s: candidate %d owned %d times\n", what, i, owners[i]);
      exit(5);
    }
  return n;
}

static int slots(int n_category, int n_bin) {
  const int C = n_category + 4 * n_bin + 2;
  long checked = 0;
  for (int attr = 0; attr < 5; ++attr) {
    P::TokenArgs a{};
    a.start = attr == 0 ? 0 : n_category + (attr - 1) * n_bin;
    a.count = attr == 0 ? n_category : n_bin;
    a.pad_id = C - 2;
    a.mask_id = C - 1;
    a.n_class = C;
    checked += check_map<P::SlotMap<64, 3, true>>(a, 192, "live map");
    checked += check_map<P::SlotMap<64, 9, false>>(a, 576, "full map");
    checked += check_map<P::SlotMap<1, P::kHostMaxLiveWide, true>>(a, P::kHostMaxLiveWide, "host map");
  }
  {  // vanilla: one vocabulary, every class live
    P::TokenArgs a{};
    a.start = 0;
    a.count = C - 2;
    a.pad_id = C - 2;
    a.mask_id = C - 1;
    a.n_class = C;
    checked += check_map<P::SlotMap<64, 9, false>>(a, 576, "full map (vanilla)");
  }
  printf("ok %ld\n", checked);
  return 0;
}

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v;
  if (!check_io::read_vec(f, v, n)) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

static int draw(const char* in, const char* outp) {
  FILE* f = check_io::open_or_exit(in, "rb", 1);
  const auto hdr = rd<int32_t>(f, 10);
  if (hdr[0] != 0x4C444D31) return 3;
  const int N = hdr[1], C = hdr[2];
  const auto fl = rd<float>(f, 2);
  const auto seed = rd<uint64_t>(f, 1);
  const auto tok = rd<int32_t>(f, N), start = rd<int32_t>(f, N), count = rd<int32_t>(f, N), cond_tok = rd<int32_t>(f, N),
             strong = rd<int32_t>(f, N), pad_dis = rd<int32_t>(f, N), pos = rd<int32_t>(f, N), step = rd<int32_t>(f, N);
  const auto layout = rd<uint64_t>(f, N);
  const auto sched = rd<float>(f, (size_t)N * 10);
  const auto logits = rd<float>(f, (size_t)N * C);
  const auto weak = rd<float>(f, hdr[8] ? (size_t)N * C : 0);
  fclose(f);
  std::vector<int32_t> out(N);
  for (int i = 0; i < N; ++i) {
    if (count[i] + 2 > P::kHostMaxLiveWide) return 4;
    P::TokenArgs a{};
    a.logits = &logits[(size_t)i * C];
    a.tok = tok[i]; a.start = start[i]; a.count = count[i];
    a.pad_id = hdr[3]; a.mask_id = hdr[4]; a.n_class = C;
    a.cond_tok = cond_tok[i]; a.strong = strong[i] != 0;
    a.weak = hdr[8] ? &weak[(size_t)i * C] : nullptr;
    a.weak_stride = 1;
    a.pad_disable = pad_dis[i] != 0;
    a.kind = hdr[5]; a.temperature = fl[0]; a.top_p = fl[1]; a.top_k = hdr[6];
    a.pos = (uint32_t)pos[i]; a.step = (uint32_t)step[i]; a.layout = layout[i]; a.seed = seed[0];
    const float* s = &sched[(size_t)i * 10];
    const P::StepSchedule sc{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9]};
    std::vector<float> work(2 * (size_t)(count[i] + 2));   // exactly what the form asks for: the sanitized build sees one float more
    out[i] = P::step_token<true, P::kHostMaxLiveWide>(a, sc, work.data());
  }
  FILE* o = check_io::open_or_exit(outp, "wb", 1);
  check_io::write_vec(o, out);
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "slots")) return slots(atoi(argv[2]), atoi(argv[3]));
  if (argc == 4 && !strcmp(argv[1], "draw")) return draw(argv[2], argv[3]);
  return 1;
}
