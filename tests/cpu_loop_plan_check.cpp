// Host check of layout_dm_amd/csrc/ldm_loop_plan.h — what ldm_sample_loop decides on the host before it launches anything — built with
// plain g++ (and as the ASan + UBSan build) and run as its own process by tests/test_loop_plan.py.  Every mode ends with `cases=N failed=M`.
//   cut         every B in 1..600 x chunk in {1, 7, 8, 128, 256} x lanes in 1..4 x balanced on / off: the passes partition [0, B) in order,
//               none empty, none above the chunk, ceil(B / chunk) of them, min(n_lanes, passes) lanes, lane l owning passes l, l + lanes, ...
//   hand        the cuts the rule's comments and formula name, written down by hand
//   key         one base key; every field that decides a hit changed alone compares unequal, a copy compares equal
//   timesteps   -1 and T refused at the first, middle and last position of either array; 0 and T - 1 accepted
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../layout_dm_amd/csrc/ldm_loop_plan.h"

using namespace ldm;

static int g_cases = 0, g_failed = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    ++g_cases;                                 \
    if (!(c)) {                                \
      printf("FAIL %s: ", #c);                 \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      ++g_failed;                              \
    }                                          \
  } while (0)

static void check_cut(int B, int chunk, int n_lanes, bool balanced) {
  const LoopCut c = cut_call(B, chunk, n_lanes, balanced);
  const int want_pass = (B + chunk - 1) / chunk;
  bool ok = c.B == B && c.n_pass == want_pass && c.lanes == (n_lanes < want_pass ? n_lanes : want_pass);
  int next = 0;
  for (int k = 0; ok && k < c.n_pass; ++k) {   // in order, no gap, no overlap, no empty pass, none above the chunk
    ok = c.offset(k) == next && c.size(k) >= 1 && c.size(k) <= chunk;
    next += c.size(k);
  }
  ok = ok && next == B;
  // lane l owns passes l, l + lanes, ...: every pass has exactly one owner among the lanes, and the single-lane form owns them all
  for (int k = 0; ok && k < c.n_pass; ++k) {
    ok = c.owns(-1, k);
    for (int l = 0; ok && l < c.lanes; ++l) ok = c.owns(l, k) == (k % c.lanes == l);
  }
  for (int l = 0; ok && l < c.lanes; ++l) {   // ... so no lane that counts is idle
    int first = -1;
    for (int k = c.n_pass; k-- > 0;)
      if (c.owns(l, k)) first = k;
    ok = first == l;
  }
  CHECK(ok, "B=%d chunk=%d lanes=%d balanced=%d -> n_pass=%d cb=%d lanes=%d", B, chunk, n_lanes, (int)balanced, c.n_pass, c.cb, c.lanes);
}

static int mode_cut() {
  const int chunks[] = {1, 7, 8, 128, 256};
  for (int B = 1; B <= 600; ++B)
    for (int chunk : chunks)
      for (int lanes = 1; lanes <= 4; ++lanes)
        for (int balanced = 0; balanced < 2; ++balanced) check_cut(B, chunk, lanes, balanced != 0);
  return 0;
}

static void expect_cut(int B, int chunk, bool balanced, std::vector<int> sizes) {
  const LoopCut c = cut_call(B, chunk, 2, balanced);
  std::vector<int> got;
  for (int k = 0; k < c.n_pass; ++k) got.push_back(c.size(k));
  CHECK(got == sizes, "B=%d chunk=%d balanced=%d: %d passes, first %d", B, chunk, (int)balanced, c.n_pass, got.empty() ? -1 : got[0]);
}

static int mode_hand() {
  expect_cut(300, 256, true, {150, 150});
  expect_cut(400, 256, true, {200, 200});
  expect_cut(488, 256, true, {256, 232});   // the remainder is >= 3/4 of a chunk: full chunks
  expect_cut(13, 8, true, {7, 6});
  expect_cut(16, 8, true, {8, 8});
  expect_cut(300, 256, false, {256, 44});
  expect_cut(8, 8, true, {8});
  expect_cut(3, 8, true, {3});
  return 0;
}

static int mode_key() {
  const std::vector<int32_t> tm = {19, 14, 9, 4, 0}, tp = {18, 13, 8, 3, 0};
  ldm_sampler s{};
  s.kind = LDM_SAMPLE_DETERMINISTIC; s.temperature = 1.f; s.top_p = 0.9f; s.top_k = 5;
  int dummy[4] = {0, 0, 0, 0};   // addresses only: the key reads presence (and d_edge_src's value), never memory
  ldm_cond cond{};
  cond.d_cond_seq = (const int32_t*)&dummy[0];
  cond.pad_disable = 1;
  ldm_relation rel{};
  rel.d_edge_src = (const int32_t*)&dummy[1];
  rel.num_update = 3; rel.n_graph_total = 8; rel.relation_lambda = 3e6f;
  const int bins[4] = {16, 16, 31, 31};
  for (int x = 0; x < 4; ++x) rel.canvas_bins[x] = bins[x];
  const GraphKey base = graph_key(8, 5, s, &cond, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data());
  CHECK(base == GraphKey(base), "a copy of the base key compares unequal");
  CHECK(base == graph_key(8, 5, s, &cond, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()), "the base key built twice compares unequal");
  // the builder stored what it was given (a key of defaults would pass every `differs` below)
  CHECK(base.B == 8 && base.n_steps == 5 && base.kind == s.kind && base.top_k == 5 && base.temperature == 1.f && base.top_p == 0.9f, "sampler / shape");
  CHECK(base.has_cond == 1 && base.has_cond_seq == 1 && base.has_strong == 0 && base.has_weak == 0 && base.pad_disable == 1 && base.has_inter == 1, "cond");
  CHECK(base.tie_rel == 1e-3f && base.tie_abs == 1e-4f, "tie thresholds of a deterministic call with a report");
  CHECK(base.has_rel == 1 && base.rel_num_update == 3 && base.rel_n_graph == 8 && base.rel_lambda == 3e6f && base.rel_edges == (const void*)&dummy[1], "relation");
  CHECK(base.rel_bins[0] == 16 && base.rel_bins[1] == 16 && base.rel_bins[2] == 31 && base.rel_bins[3] == 31 && base.t_model == tm && base.t_post == tp, "bins / timesteps");
  // every field that decides a hit, by hand: a field dropped from operator== fails its line
  struct Change {
    const char* name;
    std::function<void(GraphKey&)> apply;
  };
  const Change changes[] = {
      {"B", [](GraphKey& k) { k.B = 7; }},
      {"n_steps", [](GraphKey& k) { k.n_steps = 6; }},
      {"kind", [](GraphKey& k) { k.kind = LDM_SAMPLE_TOP_K; }},
      {"top_k", [](GraphKey& k) { k.top_k = 6; }},
      {"temperature", [](GraphKey& k) { k.temperature = 0.5f; }},
      {"top_p", [](GraphKey& k) { k.top_p = 0.8f; }},
      {"has_cond", [](GraphKey& k) { k.has_cond = 0; }},
      {"has_cond_seq", [](GraphKey& k) { k.has_cond_seq = 0; }},
      {"has_strong", [](GraphKey& k) { k.has_strong = 1; }},
      {"has_weak", [](GraphKey& k) { k.has_weak = 1; }},
      {"pad_disable", [](GraphKey& k) { k.pad_disable = 0; }},
      {"has_inter", [](GraphKey& k) { k.has_inter = 0; }},
      {"tie_rel", [](GraphKey& k) { k.tie_rel = 2e-3f; }},
      {"tie_abs", [](GraphKey& k) { k.tie_abs = 2e-4f; }},
      {"has_rel", [](GraphKey& k) { k.has_rel = 0; }},
      {"rel_num_update", [](GraphKey& k) { k.rel_num_update = 4; }},
      {"rel_n_graph", [](GraphKey& k) { k.rel_n_graph = 9; }},
      {"rel_lambda", [](GraphKey& k) { k.rel_lambda = 2e6f; }},
      {"rel_edges", [&](GraphKey& k) { k.rel_edges = &dummy[2]; }},
      {"rel_bins[0]", [](GraphKey& k) { k.rel_bins[0] = 15; }},
      {"rel_bins[1]", [](GraphKey& k) { k.rel_bins[1] = 15; }},
      {"rel_bins[2]", [](GraphKey& k) { k.rel_bins[2] = 30; }},
      {"rel_bins[3]", [](GraphKey& k) { k.rel_bins[3] = 30; }},
      {"t_model[middle]", [](GraphKey& k) { k.t_model[2] = 10; }},
      {"t_post[middle]", [](GraphKey& k) { k.t_post[2] = 7; }},
      {"t_model length", [](GraphKey& k) { k.t_model.push_back(0); }},
      {"t_post length", [](GraphKey& k) { k.t_post.pop_back(); }},
  };
  for (const Change& c : changes) {
    GraphKey k = base;
    c.apply(k);
    CHECK(!(k == base) && !(base == k), "a key that differs in %s alone compares equal", c.name);
  }
  // ... and the same through the builder's inputs: what of cond is present, the report's masking, the relation
  auto differs = [&](const char* what, const GraphKey& k) { CHECK(!(k == base), "built key: %s does not change it", what); };
  ldm_cond c2 = cond;
  c2.d_strong_mask = (const uint8_t*)&dummy[2];
  differs("a strong mask", graph_key(8, 5, s, &c2, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()));
  c2 = cond;
  c2.d_weak_logits = (const float*)&dummy[2];
  differs("weak logits", graph_key(8, 5, s, &c2, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()));
  c2 = cond;
  c2.d_cond_seq = nullptr;
  differs("no cond_seq", graph_key(8, 5, s, &c2, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()));
  differs("no cond", graph_key(8, 5, s, nullptr, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()));
  differs("no relation", graph_key(8, 5, s, &cond, true, true, 1e-3f, 1e-4f, nullptr, tm.data(), tp.data()));
  differs("no intermediates", graph_key(8, 5, s, &cond, false, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()));
  // a moved cond tensor is the same key: only presence counts
  c2 = cond;
  c2.d_cond_seq = (const int32_t*)&dummy[3];
  CHECK(graph_key(8, 5, s, &c2, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data()) == base, "a cond tensor at another address changes the key");
  // the thresholds count only where flags are written: a deterministic call on a handle with a flag buffer
  const GraphKey no_report = graph_key(8, 5, s, &cond, true, false, 1e-3f, 1e-4f, &rel, tm.data(), tp.data());
  CHECK(no_report.tie_rel == 0.f && no_report.tie_abs == 0.f && !(no_report == base), "thresholds without a flag buffer");
  ldm_sampler rnd = s;
  rnd.kind = LDM_SAMPLE_RANDOM;
  const GraphKey r1 = graph_key(8, 5, rnd, &cond, true, true, 1e-3f, 1e-4f, &rel, tm.data(), tp.data());
  const GraphKey r2 = graph_key(8, 5, rnd, &cond, true, true, 5e-3f, 0.f, &rel, tm.data(), tp.data());
  CHECK(r1.tie_rel == 0.f && r1.tie_abs == 0.f && r1 == r2, "thresholds of a stochastic call");
  return 0;
}

static int mode_timesteps() {
  const int T = 20, n = 5;
  const std::vector<int32_t> good = {19, 14, 9, 4, 0};
  CHECK(check_timesteps(good.data(), good.data(), n, T), "0 and T - 1 are refused");
  CHECK(check_timesteps(good.data(), good.data(), 1, T), "a single T - 1 is refused");
  const int positions[] = {0, n / 2, n - 1};
  const int32_t bad[] = {-1, T};
  for (int which = 0; which < 2; ++which)
    for (int pos : positions)
      for (int32_t v : bad) {
        std::vector<int32_t> tm = good, tp = good;
        (which ? tp : tm)[pos] = v;
        CHECK(!check_timesteps(tm.data(), tp.data(), n, T), "%d at position %d of %s is accepted", v, pos, which ? "t_post" : "t_model");
      }
  char msg[64];
  snprintf(msg, sizeof(msg), kTimestepRangeMsg, T);
  CHECK(!strcmp(msg, "timestep out of range [0,20)"), "the message reads '%s'", msg);
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "cut")) mode_cut();
  else if (!strcmp(mode, "hand")) mode_hand();
  else if (!strcmp(mode, "key")) mode_key();
  else if (!strcmp(mode, "timesteps")) mode_timesteps();
  else {
    fprintf(stderr, "usage: %s cut | hand | key | timesteps\n", argv[0]);
    return 2;
  }
  printf("cases=%d failed=%d\n", g_cases, g_failed);
  return g_failed ? 1 : 0;
}
