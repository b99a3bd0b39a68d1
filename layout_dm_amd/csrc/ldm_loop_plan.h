// What ldm_sample_loop decides on the host before it launches anything, each in ONE place: how a call of B layouts is cut into passes and
// which lane runs each of them (cut_call), what makes two calls replay the same captured graphs (GraphKey / graph_key), and which timesteps
// a call may name (check_timesteps).  Pure host arithmetic like ldm_engine_plan.h: no HIP, no allocation beyond the key's two timestep
// arrays, so tests/cpu_loop_plan_check.cpp enumerates all three on the CPU.
#pragma once
#include "../../include/ldm_hip.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ldm {

// ---- the cut of a call into passes
// A call of B layouts needs ceil(B / chunk) passes through a lane's workspace.  BALANCED (r06): the passes share the layouts evenly — 300
// layouts at chunk 256 are 150 + 150, not 256 + 44 (the 44-layout pass kept 212 of 256 compute units idle for as long as the full one; a
// call's two passes also overlap on the lanes when each fills only part of the chip: same-box split 1 012 -> 1 105, hybrid 1 818 -> 2 011
// layouts/s at B = 300; + 6 % / + 1 % at B = 400).  Tokens do not depend on the cut (B = 300 as 150 + 150: tests/test_hip_parity.py
// test_split_mode_loop_properties, tests/test_r04_parity.py test_relation_in_the_loop_kernel_equals_the_per_step_path).  Only where the
// remainder is small: with a remainder of >= 3/4 of a chunk the uneven cut is 2 % FASTER for the short hybrid launches (488 = 256 + 232:
// 2 142 against 2 093 for 244 + 244 — passes of unequal length drift against each other on the lanes instead of running in lock-step;
// profiles/r06_call16_17_25_*).  Either way the cut has ceil(B / chunk) passes and none is empty: cb <= chunk, so (n_pass - 1) * cb < B.
struct LoopCut {
  int B = 0;
  int n_pass = 0;   // ceil(B / chunk)
  int cb = 0;       // layouts of every pass but the last
  int lanes = 0;    // lanes that own a pass: min(n_lanes, n_pass)
  int offset(int k) const { return k * cb; }                   // first layout of pass k ...
  int size(int k) const { return std::min(cb, B - k * cb); }   // ... and how many it holds
  // pass k belongs to lane k % lanes (its workspace, stream and captured graph); lane < 0 is the single-lane form: every pass, in order
  bool owns(int lane, int k) const { return lane < 0 || k % lanes == lane; }
};

inline LoopCut cut_call(int B, int chunk, int n_lanes, bool balanced) {
  LoopCut c;
  c.B = B;
  c.n_pass = (B + chunk - 1) / chunk;
  const int rem = B - (c.n_pass - 1) * chunk;
  c.cb = (balanced && c.n_pass > 1 && 4 * rem < 3 * chunk) ? (B + c.n_pass - 1) / c.n_pass : chunk;
  c.lanes = std::min(n_lanes, c.n_pass);
  return c;
}

// ---- what decides that a call replays the graphs of an earlier one
// A lane's graph records launches whose arguments hold the call's scalars and the handle's own staging addresses (ldm_handle.h st_*: the
// caller's cond tensors, relation graph and intermediates are copied through them), so presence flags stand for the staged cond tensors.
// rel_edges alone is an address: the edge staging grows, and a graph that recorded the old buffer must never be replayed.
struct GraphKey {
  int B = 0, n_steps = 0;
  int kind = 0, top_k = 0;
  float temperature = 0.f, top_p = 0.f;
  int has_cond = 0, has_cond_seq = 0, has_strong = 0, has_weak = 0, pad_disable = 0;
  int has_inter = 0;
  float tie_rel = 0.f, tie_abs = 0.f;
  int has_rel = 0, rel_num_update = 0, rel_n_graph = 0, rel_bins[4] = {0, 0, 0, 0};
  float rel_lambda = 0.f;
  const void* rel_edges = nullptr;
  std::vector<int32_t> t_model, t_post;
  bool operator==(const GraphKey& o) const {
    return B == o.B && n_steps == o.n_steps && kind == o.kind && top_k == o.top_k && temperature == o.temperature && top_p == o.top_p &&
           has_cond == o.has_cond && has_cond_seq == o.has_cond_seq && has_strong == o.has_strong && has_weak == o.has_weak &&
           pad_disable == o.pad_disable && has_inter == o.has_inter && tie_rel == o.tie_rel && tie_abs == o.tie_abs && has_rel == o.has_rel &&
           rel_num_update == o.rel_num_update && rel_n_graph == o.rel_n_graph && rel_bins[0] == o.rel_bins[0] &&
           rel_bins[1] == o.rel_bins[1] && rel_bins[2] == o.rel_bins[2] && rel_bins[3] == o.rel_bins[3] && rel_lambda == o.rel_lambda &&
           rel_edges == o.rel_edges && t_model == o.t_model && t_post == o.t_post;
  }
};

// cond / rel: the call's inputs (or nullptr); of cond's pointers only their presence is read, of rel's only d_edge_src (the handle's edge
// staging once staged).  tie_report: the handle has a near-tie flag buffer; the thresholds count for deterministic calls only, the only
// ones that write flags.
inline GraphKey graph_key(int B, int n_steps, const ldm_sampler& s, const ldm_cond* cond, bool intermediates, bool tie_report, float tie_rel,
                          float tie_abs, const ldm_relation* rel, const int32_t* t_model, const int32_t* t_post) {
  GraphKey k;
  k.B = B; k.n_steps = n_steps;
  k.kind = s.kind; k.top_k = s.top_k; k.temperature = s.temperature; k.top_p = s.top_p;
  if (cond) {
    k.has_cond = 1;
    k.has_cond_seq = cond->d_cond_seq != nullptr;
    k.has_strong = cond->d_strong_mask != nullptr;
    k.has_weak = cond->d_weak_logits != nullptr;
    k.pad_disable = cond->pad_disable;
  }
  k.has_inter = intermediates;
  const bool flags = tie_report && s.kind == LDM_SAMPLE_DETERMINISTIC;
  k.tie_rel = flags ? tie_rel : 0.f;
  k.tie_abs = flags ? tie_abs : 0.f;
  if (rel) {
    k.has_rel = 1;
    k.rel_num_update = rel->num_update;
    k.rel_n_graph = rel->n_graph_total;
    k.rel_lambda = rel->relation_lambda;
    k.rel_edges = rel->d_edge_src;
    for (int x = 0; x < 4; ++x) k.rel_bins[x] = rel->canvas_bins[x];
  }
  k.t_model.assign(t_model, t_model + n_steps);
  k.t_post.assign(t_post, t_post + n_steps);
  return k;
}

// ---- the timesteps a step or a loop may name: [0, T) for the denoiser's and the posterior's alike (constrained.py:139)
constexpr const char* kTimestepRangeMsg = "timestep out of range [0,%d)";
inline bool check_timesteps(const int32_t* t_model, const int32_t* t_post, int n, int T) {
  for (int i = 0; i < n; ++i)
    if (t_model[i] < 0 || t_model[i] >= T || t_post[i] < 0 || t_post[i] >= T) return false;
  return true;
}

}  // namespace ldm
