// Scoring given layouts (ldm_q_sample / ldm_vb_terms / ldm_vb_step): the forward noising draw q(x_t | x_0) and the terms of the
// variational bound for given (x_0, x_t, t) and the denoiser's logits — ConstrainedMaskAndReplaceDiffusion.forward
// (constrained.py:232-333) / VanillaMaskAndReplaceDiffusion.forward (vanilla.py:160-240) behind the denoiser pass, without
// the (B, C, S) log-one-hot tensors.  The arithmetic is ldm_vb_core.h (one source with the host check); this file supplies
// the lane groups, the memory traffic and the per-layout sums.
//
//   q_sample_k   one token per lane: x_0 and the schedule entries of t in, one int32 token out (xt given: its checked copy)
//   vb_terms_k   one workgroup per layout.  A token is processed by a lane group exactly as in posterior_sample_k: NL = 16 on
//                the token's live classes (constrained), NL = 64 over the full vocabulary (vanilla: live sets above 48).
//                The group's lane 0 leaves the token's kl / nll / aux / hit in LDS; after one barrier four lanes add a
//                quantity each over the positions, left to right, in float64.  No floating-point atomics: two runs give
//                the same bits, and a layout's sums do not depend on the batch around it.
//   vb_grad_k    the same walk; a token's lane group also writes the token's row of d loss / d logits (ldm_vb_grad)
// Per-layout timesteps (VbArgs.t_rows / layout_rows, the ldm_*_t entry points): the schedule rows and the Philox key take the
// layout's own t and layout index (ldm_vb_core.h row_t / row_layout); nullptr: the call's single t and the row position.
#include "ldm_kernels.h"
#include "ldm_post_dpp.h"
#include "ldm_vb_core.h"

namespace ldm {

namespace {
__device__ __forceinline__ ldm_post::TokenArgs position_args(const VocabTables& v, int attr) {
  ldm_post::TokenArgs a{};
  a.start = v.start[attr];
  a.count = v.count[attr];
  a.pad_id = v.pad_id;
  a.mask_id = v.mask_id;
  a.n_class = v.n_class;
  a.cond_tok = -1;
  return a;
}
}  // namespace

__global__ __launch_bounds__(256) void q_sample_k(VbArgs p) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= p.B * p.S) return;
  const int b = row / p.S, s = row % p.S;
  const int attr = s % p.v.n_attr;
  const ldm_post::TokenArgs a = position_args(p.v, attr);
  const int x0 = p.x0[row];
  const int e = ldm_vb::token_error(a, x0, p.xt != nullptr, p.xt ? p.xt[row] : 0);
  if (e) {  // the call is refused; what the denoiser pass behind this launch embeds stays inside the vocabulary
    atomicOr(p.err, e);
    p.xt_out[row] = p.v.mask_id;
    return;
  }
  if (p.xt) {  // a given state: checked copy
    p.xt_out[row] = p.xt[row];
    return;
  }
  const int t = ldm_vb::row_t(p.t_rows, p.t, b);
  const ldm_vb::NoiseSchedule ns = ldm_vb::noise_schedule(p.sched, p.v.n_attr, attr, p.T, t);
  p.xt_out[row] = ldm_vb::q_sample_token(a, x0, ns, (uint32_t)s, (uint32_t)t, ldm_vb::row_layout(p.first_layout, p.layout_rows, b), p.seed);
}

// CMAX: the widest vocabulary an instantiation serves, as in posterior_sample_k (192: the forms above; 576: one wavefront per token
// on live sets up to 192, or over the whole vocabulary with 9 slots per lane — vanilla)
template <int NL, bool LIVE, bool FAST, int CMAX = 192>
__global__ __launch_bounds__(256) void vb_terms_k(VbArgs p) {
  constexpr int GPB = 256 / NL;           // tokens in flight per workgroup
  constexpr int NJ = LIVE ? 3 : CMAX / NL; // class slots per lane
  static_assert(CMAX == 192 || (CMAX == 576 && NL == 64 && !FAST), "wide vocabularies: one wavefront per token, f64 log-softmax");
  static_assert(LIVE || NL == 64, "full-vocabulary map: one wavefront per token");
  extern __shared__ float sh[];           // [kNumSums][S]
  const int b = blockIdx.x;
  const int S = p.S;
  const int t_b = ldm_vb::row_t(p.t_rows, p.t, b);   // (uniform: one workgroup per layout)
  const int grp = threadIdx.x / NL;
  const ldm_post::DppGroup<NL, FAST> g{(int)threadIdx.x % NL};
  const ldm_post::SlotMap<NL, NJ, LIVE> m{(int)threadIdx.x % NL};
  for (int s = grp; s < S; s += GPB) {    // (whole groups — DPP rows / wavefronts — enter and leave together)
    const int row = b * S + s;
    const int attr = s % p.v.n_attr;
    ldm_post::TokenArgs a = position_args(p.v, attr);
    const int x0 = p.x0[row];
    a.tok = p.xt[row];
    a.logits = p.logits + (size_t)row * p.ldl;
    ldm_vb::Terms t{0.f, 0.f, 0.f, 0};
    const int e = ldm_vb::token_error(a, x0, true, a.tok);
    if (e) {
      if (g.lane() == 0) atomicOr(p.err, e);
    } else {
      t = ldm_vb::token_terms<!FAST>(g, m, a, x0, ldm_vb::step_schedule(p.sched, p.v.n_attr, attr, p.T, t_b));
    }
    if (g.lane() == 0) {
      sh[ldm_vb::kSumKl * S + s] = t.kl;
      sh[ldm_vb::kSumNll * S + s] = t.nll;
      sh[ldm_vb::kSumAux * S + s] = t.aux;
      sh[ldm_vb::kSumHit * S + s] = (float)t.hit;
      if (p.tok_out) {                    // (3, B, S) parity dump
        const size_t BS = (size_t)p.B * S;
        p.tok_out[0 * BS + row] = t.kl;
        p.tok_out[1 * BS + row] = t.nll;
        p.tok_out[2 * BS + row] = t.aux;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < ldm_vb::kNumSums) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += (double)sh[threadIdx.x * S + s];
    p.sums[(size_t)b * ldm_vb::kNumSums + threadIdx.x] = acc;
  }
}

// The training loss's gradient with respect to the logits (ldm_vb_grad; arithmetic: ldm_vb_core.h token_grad), in the lane-group
// forms of vb_terms_k and always with the float64 log-softmax.  A token's row of p.grad is written by its own lane group, every
// element once (a refused token: zeros), consecutive lanes consecutive classes: no atomics, two runs give the same bits, and a
// layout's rows do not depend on the batch around it.  The sums are vb_terms_k<.., FAST = false>'s, bit for bit: the terms come
// from the same token_terms<true> call.  p.grad == nullptr: that call alone.
template <int NL, bool LIVE, int CMAX = 192>
__global__ __launch_bounds__(256) void vb_grad_k(VbArgs p) {
  constexpr int GPB = 256 / NL;
  constexpr int NJ = LIVE ? 3 : CMAX / NL;
  static_assert(CMAX == 192 || (CMAX == 576 && NL == 64), "wide vocabularies: one wavefront per token");
  static_assert(LIVE || NL == 64, "full-vocabulary map: one wavefront per token");
  extern __shared__ float sh[];           // [kNumSums][S]
  const int b = blockIdx.x;
  const int S = p.S;
  const int t_b = ldm_vb::row_t(p.t_rows, p.t, b);   // (uniform: one workgroup per layout)
  const double c_kl = p.grad ? p.coef[2 * b] : 0.0, c_aux = p.grad ? p.coef[2 * b + 1] : 0.0;
  const int grp = threadIdx.x / NL;
  const ldm_post::DppGroup<NL, false> g{(int)threadIdx.x % NL};
  const ldm_post::SlotMap<NL, NJ, LIVE> m{(int)threadIdx.x % NL};
  for (int s = grp; s < S; s += GPB) {    // (whole groups — DPP rows / wavefronts — enter and leave together)
    const int row = b * S + s;
    const int attr = s % p.v.n_attr;
    ldm_post::TokenArgs a = position_args(p.v, attr);
    const int x0 = p.x0[row];
    a.tok = p.xt[row];
    a.logits = p.logits + (size_t)row * p.ldl;
    float* grad_row = p.grad ? p.grad + (size_t)row * p.v.n_class : nullptr;
    ldm_vb::Terms t{0.f, 0.f, 0.f, 0};
    const int e = ldm_vb::token_error(a, x0, true, a.tok);
    if (e) {
      if (g.lane() == 0) atomicOr(p.err, e);
      if (grad_row)
        for (int c = g.lane(); c < p.v.n_class; c += NL) grad_row[c] = 0.0f;
    } else {
      const ldm_post::StepSchedule sc = ldm_vb::step_schedule(p.sched, p.v.n_attr, attr, p.T, t_b);
      t = grad_row ? ldm_vb::token_grad(g, m, a, x0, sc, c_kl, c_aux, t_b == 0, grad_row) : ldm_vb::token_terms<true>(g, m, a, x0, sc);
    }
    if (g.lane() == 0) {
      sh[ldm_vb::kSumKl * S + s] = t.kl;
      sh[ldm_vb::kSumNll * S + s] = t.nll;
      sh[ldm_vb::kSumAux * S + s] = t.aux;
      sh[ldm_vb::kSumHit * S + s] = (float)t.hit;
    }
  }
  if (!p.sums) return;                     // (uniform)
  __syncthreads();
  if (threadIdx.x < ldm_vb::kNumSums) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += (double)sh[threadIdx.x * S + s];
    p.sums[(size_t)b * ldm_vb::kNumSums + threadIdx.x] = acc;
  }
}

void launch_q_sample(const VbArgs& p, hipStream_t st) {
  const int M = p.B * p.S;
  hipLaunchKernelGGL(q_sample_k, dim3((M + 255) / 256), dim3(256), 0, st, p);
}

void launch_vb_terms(const VbArgs& p, hipStream_t st) {
  int live_max = 0;
  for (int a = 0; a < p.v.n_attr; ++a) live_max = live_max > p.v.count[a] + 2 ? live_max : p.v.count[a] + 2;
  const size_t lds = (size_t)ldm_vb::kNumSums * p.S * sizeof(float);
  if (p.v.n_class > 192) {  // wide vocabularies (exact / split only): see launch_posterior_sample
    auto kern = live_max > 192 ? vb_terms_k<64, false, false, 576> : vb_terms_k<64, true, false, 576>;
    hipLaunchKernelGGL(kern, dim3(p.B), dim3(256), lds, st, p);
    return;
  }
  const bool wave = live_max > 48;
  auto kern = wave ? (p.f32_lse ? vb_terms_k<64, false, true> : vb_terms_k<64, false, false>)
                   : (p.f32_lse ? vb_terms_k<16, true, true> : vb_terms_k<16, true, false>);
  hipLaunchKernelGGL(kern, dim3(p.B), dim3(256), lds, st, p);
}

void launch_vb_grad(const VbArgs& p, hipStream_t st) {   // the forms of launch_vb_terms at the float64 log-softmax
  int live_max = 0;
  for (int a = 0; a < p.v.n_attr; ++a) live_max = live_max > p.v.count[a] + 2 ? live_max : p.v.count[a] + 2;
  const size_t lds = (size_t)ldm_vb::kNumSums * p.S * sizeof(float);
  auto kern = p.v.n_class > 192 ? (live_max > 192 ? vb_grad_k<64, false, 576> : vb_grad_k<64, true, 576>)
                                : (live_max > 48 ? vb_grad_k<64, false> : vb_grad_k<16, true>);
  hipLaunchKernelGGL(kern, dim3(p.B), dim3(256), lds, st, p);
}

}  // namespace ldm
