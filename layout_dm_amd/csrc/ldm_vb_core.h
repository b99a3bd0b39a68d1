// Scoring GIVEN layouts: the arithmetic of the forward noising draw and of the variational bound's terms for ONE token — one
// source for kernels_vb.hip and for the host check (tests/cpu_vb_check.cpp).
//
//   q_sample_token   x_t ~ q(x_t | x_0)                               constrained.py:112-133, 223-230; vanilla.py:90-110, 153-158
//   token_terms      log_x0_recon (predict_start tail, base.py:131-144) -> log_model_prob = q_posterior(log_x0_recon, x_t, t),
//                    log_true_prob = q_posterior(log_onehot(x_0), x_t, t)                       constrained.py:263-291
//                    kl = sum_c exp(true)(true - model)                                         base.py:117-119
//                    nll = -sum_c exp(log_onehot(x_0)) model                                    util.py:30-31
//                    aux = KL(log_onehot(x_0)[:-1] || log_x0_recon[:-1])                        constrained.py:317-319
//                    hit = argmax log_x0_recon == x_0                                           constrained.py:269-277
//   token_grad       d / d logits of  c_kl (t == 0 ? nll : kl) + c_aux (t == 0 ? nll : aux)  for the token: the training loss's
//                    backward behind the logits (constrained.py:292-330 under autograd), closed form, float64
//
// The lane groups, the slot maps, the schedule rows, QTerms and the posterior itself are those of ldm_post_token.h.  A token's
// sub-vocabulary (body + [PAD] + [MASK]; vanilla: every class) carries the posterior; every other class sits at log(1e-30) in
// BOTH posteriors, so it adds exactly 0 to kl and exp(log(1e-30)) log(1e-30) to nll — what the reference's sum over the full
// vocabulary gives it.  aux and hit read the whole row of C - 1 logits: log_x0_recon is a softmax over all of them.
//
// The reference draws x_t by Gumbel-argmax on torch's generator; that stream cannot be reproduced.  Here the draw is an inverse
// CDF on ONE Philox4x32-10 uniform keyed by (seed, global layout index, t, position) over the reference's own outcome
// probabilities exp(q_pred): the kept class alpha_bar_t + beta_bar_t, every other non-MASK class of the sub-vocabulary
// ([PAD] included) beta_bar_t, [MASK] gamma_bar_t.
#pragma once
#include "ldm_post_token.h"

namespace ldm_vb {

using ldm_post::kLogEps;
using ldm_post::StepSchedule;
using ldm_post::TokenArgs;

// error word of the entry points
constexpr int kErrRange = 1;     // a token outside [0, C)
constexpr int kErrMaskX0 = 2;    // [MASK] in x_0
constexpr int kErrSubVocab = 4;  // a token that is not of its position's sub-vocabulary

// a: start / count / pad_id / mask_id / n_class of the position
LDM_PT_HD int token_error(const TokenArgs& a, int x0, bool has_xt, int xt) {
  int e = 0;
  if (x0 < 0 || x0 >= a.n_class || (has_xt && (xt < 0 || xt >= a.n_class))) return kErrRange;
  if (x0 == a.mask_id) e |= kErrMaskX0;
  else if (!ldm_post::is_live(a, x0)) e |= kErrSubVocab;
  if (has_xt && !ldm_post::is_live(a, xt)) e |= kErrSubVocab;
  return e;
}

// Per-layout timesteps (ldm_*_t): layout b of a call is noised and scored at t_rows[b], and its Philox key carries the layout index
// first_layout + layout_rows[b] — nullptr: the call's single t / the row position b, what the single-t entry points use.  One
// layout may so stand in several rows of a call, at several t, and still draw what a single-t call at that t draws for it.
LDM_PT_HD int row_t(const int32_t* t_rows, int t, int b) { return t_rows ? t_rows[b] : t; }
LDM_PT_HD uint64_t row_layout(uint64_t first_layout, const uint64_t* layout_rows, int b) {
  return first_layout + (layout_rows ? layout_rows[b] : (uint64_t)b);
}

// schedule entries of (attribute, t) the draw reads: log_cumprod_at / bt / ct and log_1_min_cumprod_ct at t
struct NoiseSchedule {
  float LA, LB, LC, L1C;
};

// exp(q_pred(log_onehot(x_0), t)) of the sub-vocabulary's three kinds of class, in the reference's float32 (util.py:19-21)
struct NoiseProbs {
  float same, other, mask;
};
LDM_PT_HD NoiseProbs noise_probs(const NoiseSchedule& s) {
  const ldm_post::HostLane g;  // libm on the host and on the device (one token per lane: no group)
  NoiseProbs p;
  p.same = g.exp(ldm_post::log_add_exp(g, 0.0f + s.LA, s.LB));
  p.other = g.exp(ldm_post::log_add_exp(g, kLogEps + s.LA, s.LB));
  p.mask = g.exp(ldm_post::log_add_exp(g, kLogEps + s.L1C, s.LC));
  return p;
}

// inverse CDF in class order over the sub-vocabulary (body, [PAD], [MASK]); the normaliser cancels (u * total), like draw_token
LDM_PT_HD int q_sample_token(const TokenArgs& a, int x0, const NoiseSchedule& s, uint32_t pos, uint32_t t, uint64_t layout,
                             uint64_t seed) {
  const NoiseProbs p = noise_probs(s);
  const int K = a.count + 2;
  const int k0 = x0 == a.pad_id ? a.count : x0 - a.start;  // live index of x_0
  double total = 0.0;
  for (int i = 0; i < K; ++i) total += (double)(i == K - 1 ? p.mask : i == k0 ? p.same : p.other);
  uint32_t r[4];
  ldm_post::philox4x32_10(pos, t, (uint32_t)layout, (uint32_t)(layout >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const double thr = (double)ldm_post::u01(r[0]) * total;
  double acc = 0.0;
  int n = 0;
  for (int i = 0; i < K; ++i) {
    acc += (double)(i == K - 1 ? p.mask : i == k0 ? p.same : p.other);
    if (acc <= thr) n += 1;
  }
  n = n < K - 1 ? n : K - 1;
  return ldm_post::live_id(a, n);
}

LDM_PT_HD StepSchedule step_schedule(const float* sched, int n_attr, int attr, int T, int t) {
  const int T1 = T + 1;
  const int u = (t - 1 + T1) % T1;  // constrained.py:114 (t = 0 reads index T)
  // rows: ldm_kernels.h ScheduleRow {at, bt, ct, cum at, cum bt, cum ct, 1 - ct, 1 - cum ct}
  const float* b = sched + (size_t)attr * T1;
  const size_t r = (size_t)n_attr * T1;
  return StepSchedule{b[0 * r + t], b[1 * r + t], b[2 * r + t], b[3 * r + t], b[4 * r + t],
                      b[5 * r + t], b[3 * r + u], b[4 * r + u], b[5 * r + u], b[7 * r + u]};
}
LDM_PT_HD NoiseSchedule noise_schedule(const float* sched, int n_attr, int attr, int T, int t) {
  const int T1 = T + 1;
  const float* b = sched + (size_t)attr * T1;
  const size_t r = (size_t)n_attr * T1;
  return NoiseSchedule{b[3 * r + t], b[4 * r + t], b[5 * r + t], b[7 * r + t]};
}

struct Terms {
  float kl, nll, aux;
  int hit;
};

// a.logits: the token's row of C logits (the [MASK] column is ignored); a.tok = x_t; the cond and draw members are not read.
// F64_LSE: the reference's float64 log-softmax; otherwise fp32 (the fast numerics mode).  Every lane of the group returns the
// token's terms.  Float32 sums: a lane's slots / classes in increasing order, then the group's tree.
// RECON (host check only): a.logits IS log_x0_recon — the reference's own, so that the check isolates what follows it.
// rs (token_grad): receives the row's maximum and float64 log-sum-exp.
struct RowStats {
  float mx;
  double lse;
};
template <bool F64_LSE, class G, class M, bool RECON = false>
LDM_PT_HD Terms token_terms(const G& g, const M& m, const TokenArgs& a_in, int x0, const StepSchedule& s, RowStats* rs = nullptr) {
  constexpr int NJ = M::NJ;
  TokenArgs a = a_in;
  a.cond_tok = -1;
  a.strong = false;
  a.weak = nullptr;
  a.pad_disable = false;
  const int C1 = a.n_class - 1;
  const float e30 = g.exp(kLogEps);  // exp(log_onehot) of a class that is not x_0 (util.py:39)
  // ---- log-softmax over the C - 1 non-MASK classes (base.py:137)
  float mx = -INFINITY;
  for (int c = g.lane(); c < C1; c += G::NL) mx = fmaxf(mx, a.logits[c]);
  mx = g.gmax(mx);
  float lse0f = 0.f;
  double lse0d = 0.0;
  if (RECON) {
  } else if (F64_LSE) {
    double se = 0.0;
    for (int c = g.lane(); c < C1; c += G::NL) se += exp((double)a.logits[c] - (double)mx);
    lse0d = log(g.gsumd(se));
  } else {
    float se = 0.f;
    for (int c = g.lane(); c < C1; c += G::NL) se += g.exp(a.logits[c] - mx);
    lse0f = g.log(g.gsum(se));
  }
  if (rs) {
    rs->mx = mx;
    rs->lse = lse0d;
  }
  auto recon = [&](int c) {  // log_x0_recon of a non-MASK class
    return RECON ? a.logits[c] : F64_LSE ? ldm_post::l0_f64(a.logits[c], mx, lse0d) : ldm_post::l0_f32(a.logits[c], mx, lse0f);
  };
  // ---- aux and the argmax over the whole row (class C - 1 holds -70 and is the last: it never is the first maximum)
  float aux = 0.f, bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = g.lane(); c < C1; c += G::NL) {
    const float l = recon(c);
    aux += (c == x0) ? (0.0f - l) : e30 * (kLogEps - l);
    if (l > bv) {
      bv = l;
      bi = c;
    }
  }
  aux = g.gsum(aux);
  g.gargmax(bv, bi);
  // ---- the two posteriors on the token's slots
  float l0m[NJ], l0t[NJ], lpm[NJ], lpt[NJ];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < NJ; ++j) {
    const int c = m.cls(a, j);
    l0m[j] = (m.valid(a, j) && c < C1) ? recon(c) : -70.0f;
    l0t[j] = c == x0 ? 0.0f : kLogEps;
  }
  const ldm_post::QTerms kq = ldm_post::q_terms(g, a.tok == a.mask_id, s);
  ldm_post::token_log_probs(g, m, a, s, kq, l0m, lpm);
  ldm_post::token_log_probs(g, m, a, s, kq, l0t, lpt);
  float kl = 0.f, nll = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < NJ; ++j)
    if (m.valid(a, j)) {
      kl += g.exp(lpt[j]) * (lpt[j] - lpm[j]);
      nll += (m.cls(a, j) == x0 ? 1.0f : e30) * lpm[j];
    }
  // the classes a LIVE map leaves out: log(1e-30) in both posteriors (layout_tokenizer.py:544)
  if (M::LIVE && g.lane() == 0) nll += (float)(a.n_class - m.n_cand(a)) * (e30 * kLogEps);
  Terms out;
  out.kl = g.gsum(kl);
  out.nll = -g.gsum(nll);
  out.aux = aux;
  out.hit = bi == x0 ? 1 : 0;
  return out;
}

// The gradient of one token's share of the training loss with respect to its row of logits (constrained.py:292-330):
//   L = c_kl (t == 0 ? nll : kl) + c_aux (t == 0 ? nll : aux)
// with the token's terms as token_terms<true> computes them — the forward is that very call (float64 log-sum-exp, the
// reference's precision), so the returned terms carry its bits.  grad_row[c], c = 0 .. C - 1, receives dL/dlogit[c]; the [MASK]
// column is 0.  Every element of the row is written exactly once: a lane writes the classes of its own slots, and — LIVE maps —
// the classes outside the token's sub-vocabulary lane-strided, consecutive lanes consecutive classes.
//   upstream of the posterior   kl: dL/dlpm[j] = -c_kl exp(lpt[j]) (base.py:117-119; the true posterior is a constant);
//                               nll: -(c_kl + c_aux)(cls(j) == x0 ? 1 : e30); the log(1e-30) fill of dead classes carries nothing
//   through the posterior       ldm_post_token.h token_log_probs_f64 -> dL/dl0 on the live non-[MASK] slots
//   aux                         -c_aux (c == x0 ? 1 : e30) on every one of the C - 1 classes
//   through l0 = clamp(log_softmax, -70, 0)   gate by the clamp (both ends pass), then as the reference's
//                               log_softmax(out.double()) runs its backward: dlogit_c = gl0_c - softmax_c sum_k gl0_k
template <class G, class M>
LDM_PT_HD Terms token_grad(const G& g, const M& m, const TokenArgs& a_in, int x0, const StepSchedule& s, double c_kl, double c_aux,
                           bool t_is_zero, float* grad_row) {
  constexpr int NJ = M::NJ;
  TokenArgs a = a_in;
  a.cond_tok = -1;
  a.strong = false;
  a.weak = nullptr;
  a.pad_disable = false;
  RowStats rs;
  const Terms out = token_terms<true>(g, m, a, x0, s, &rs);
  const int C1 = a.n_class - 1;
  const float e30 = g.exp(kLogEps);
  const double w_post = t_is_zero ? c_kl + c_aux : c_kl;  // on nll (t == 0) or kl
  const double w_aux = t_is_zero ? 0.0 : c_aux;
  auto lsm = [&](int c) { return ((double)a.logits[c] - (double)rs.mx) - rs.lse; };  // log-softmax of a non-MASK class, float64
  auto passes = [&](double u) { return (float)u >= -70.0f && (float)u <= 0.0f; };
  auto aux_grad = [&](int c) { return w_aux == 0.0 ? 0.0 : -(w_aux * (double)(c == x0 ? 1.0f : e30)); };
  // ---- the posterior path on the token's slots, in float64 from the float32 l0 (ldm_post_token.h token_log_probs_f64)
  float l0m[NJ], l0t[NJ];
  double up[NJ], gs[NJ];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < NJ; ++j) {
    const int c = m.cls(a, j);
    l0m[j] = (m.valid(a, j) && c < C1) ? ldm_post::l0_f64(a.logits[c], rs.mx, rs.lse) : -70.0f;
    l0t[j] = c == x0 ? 0.0f : kLogEps;
    up[j] = -(w_post * (double)(c == x0 ? 1.0f : e30));
  }
  const ldm_post::QTermsF64 kq = ldm_post::q_terms_f64(a.tok == a.mask_id, s);
  if (!t_is_zero) {
    double lpt[NJ];
    ldm_post::token_log_probs_f64<false>(g, m, a, s, kq, l0t, up, lpt);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < NJ; ++j) up[j] = m.live(a, j) ? -(w_post * exp(lpt[j])) : 0.0;
  }
  ldm_post::token_log_probs_f64<true>(g, m, a, s, kq, l0m, up, gs);
  // ---- gl0 per class: both paths added, rounded to float32 (the type of the reference's log-softmax output, and so of its
  // gradient, whatever the module's), gated by the clamp; and its sum over the row
  double tot = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < NJ; ++j) {
    const int c = m.cls(a, j);
    gs[j] = (m.valid(a, j) && c < C1 && passes(lsm(c))) ? (double)(float)(gs[j] + aux_grad(c)) : 0.0;
    tot += gs[j];
  }
  if (M::LIVE && w_aux != 0.0)
    for (int c = g.lane(); c < C1; c += G::NL)
      if (!ldm_post::is_live(a, c) && passes(lsm(c))) tot += (double)(float)aux_grad(c);
  tot = g.gsumd(tot);
  // ---- through the log-softmax, and out
  if (M::LIVE)
    for (int c = g.lane(); c < a.n_class; c += G::NL)
      if (!ldm_post::is_live(a, c)) {  // (below C - 1: [MASK] is live)
        const double u = lsm(c);
        grad_row[c] = (float)((passes(u) ? (double)(float)aux_grad(c) : 0.0) - exp(u) * tot);
      }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < NJ; ++j)
    if (m.valid(a, j)) {
      const int c = m.cls(a, j);
      grad_row[c] = c < C1 ? (float)(gs[j] - exp(lsm(c)) * tot) : 0.0f;
    }
  return out;
}

// rows of the per-layout sums
enum { kSumKl = 0, kSumNll, kSumAux, kSumHit, kNumSums };

}  // namespace ldm_vb
