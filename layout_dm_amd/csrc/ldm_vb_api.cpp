// Host side of scoring GIVEN layouts (include/ldm_hip.h: ldm_q_sample, ldm_vb_terms, ldm_vb_step): the forward noising draw,
// the variational bound's terms of one timestep, and the two around one denoiser pass of the handle's own numerics mode — at ONE
// timestep for the call, or (ldm_q_sample_t, ldm_vb_terms_t, ldm_vb_step_t) at a timestep per layout, one body for both.
// Evaluation of a trained model, and (ldm_vb_grad) the training loss's gradient with respect to GIVEN logits: nothing of the handle's
// weights or schedule is written.
// Tokens are checked by the kernels (ldm_vb_core.h token_error) into an error word the call reads back before it returns:
// a refused call has synchronised the stream, like a successful one.
#include "ldm_handle.h"
#include "ldm_vb_core.h"

using namespace ldm_host;

namespace {

int err_begin(ldm_handle* h, hipStream_t st) {
  if (!h->vb_err) {
    int rc = h->dalloc(&h->vb_err, 1);
    if (rc) return rc;
  }
  HIP_OK(h, hipMemsetAsync(h->vb_err, 0, sizeof(int32_t), st));
  return 0;
}

int err_end(ldm_handle* h, hipStream_t st) {
  int32_t e = 0;
  HIP_OK(h, hipGetLastError());
  HIP_OK(h, hipMemcpyAsync(&e, h->vb_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_OK(h, hipStreamSynchronize(st));
  if (e & ldm_vb::kErrRange) return h->fail(-6, "a token is outside [0, %d)", h->plan.C);
  if (e & ldm_vb::kErrMaskX0) return h->fail(-6, "x_0 holds [MASK] (%d): only noised states do", h->vocab.mask_id);
  if (e & ldm_vb::kErrSubVocab) return h->fail(-6, "a token is not of its position's sub-vocabulary (attribute body, [PAD], [MASK])");
  return 0;
}

void fill_vb(const ldm_handle* h, VbArgs& p, int t, int B) {
  p.sched = h->sched;
  p.T = h->T;
  p.t = t;
  p.f32_lse = h->plan.fast() ? 1 : 0;
  p.B = B;
  p.S = h->plan.S;
  p.v = h->vocab;
  p.err = h->vb_err;
}

int check_t(ldm_handle* h, int t) {
  if (t < 0 || t >= h->T) return h->fail(-1, "timestep %d out of range [0,%d)", t, h->T);  // constrained.py:139
  return 0;
}

// The timesteps of a call: ONE t (h_t == nullptr, the single-t entry points), or B per-layout values staged on the device
// (the *_t entry points; h_layout: the layouts' indices in the Philox key, or nullptr: their row positions).
struct CallT {
  int t = 0;
  const int32_t* d_t = nullptr;
  const uint64_t* d_layout = nullptr;
};

int begin_t(ldm_handle* h, int t, const int32_t* h_t, bool per_layout, const uint64_t* h_layout, int B, hipStream_t st, CallT& c) {
  if (!per_layout) {
    c.t = t;
    return check_t(h, t);
  }
  if (int rc = stage_timesteps(h, h_t, B, st, &c.d_t)) return rc;
  if (!h_layout) return 0;
  if (!h->st_layout) {
    if (int rc = h->dalloc(&h->st_layout, (size_t)h->cfg.max_batch)) return rc;
    h->st_layout_host.resize((size_t)h->cfg.max_batch);
  }
  std::copy(h_layout, h_layout + B, h->st_layout_host.begin());   // (pageable: read by the time the upload returns, like stage_timesteps)
  HIP_OK(h, hipMemcpyAsync(h->st_layout, h->st_layout_host.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  c.d_layout = h->st_layout;
  return 0;
}

// rows [off, off + B) of the call
void fill_vb(const ldm_handle* h, VbArgs& p, const CallT& c, int off, int B) {
  fill_vb(h, p, c.t, B);
  p.t_rows = c.d_t ? c.d_t + off : nullptr;
  p.layout_rows = c.d_layout ? c.d_layout + off : nullptr;
}

int q_sample(ldm_handle* h, const int32_t* d_x0, int t, const int32_t* h_t, bool per_layout, const uint64_t* h_layout, uint64_t seed,
             uint64_t first_layout, int B, int32_t* d_xt, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_x0 || !d_xt) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  CallT c;
  if ((rc = begin_t(h, t, h_t, per_layout, h_layout, B, st, c))) return rc;
  if ((rc = err_begin(h, st))) return rc;
  VbArgs p{};
  fill_vb(h, p, c, 0, B);
  p.x0 = d_x0;
  p.xt_out = d_xt;
  p.seed = seed;
  p.first_layout = first_layout;
  launch_q_sample(p, st);
  return err_end(h, st);
}

int vb_terms(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, int t, const int32_t* h_t, bool per_layout,
             int B, double* d_sums, float* d_tok, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_logits || !d_x0 || !d_xt || !d_sums) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  CallT c;
  if ((rc = begin_t(h, t, h_t, per_layout, nullptr, B, st, c))) return rc;
  if ((rc = err_begin(h, st))) return rc;
  VbArgs p{};
  fill_vb(h, p, c, 0, B);
  p.logits = d_logits;
  p.ldl = h->plan.C;
  p.x0 = d_x0;
  p.xt = d_xt;
  p.sums = d_sums;
  p.tok_out = d_tok;
  launch_vb_terms(p, st);
  return err_end(h, st);
}

int vb_step(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, int t, const int32_t* h_t, bool per_layout, const uint64_t* h_layout,
            uint64_t seed, uint64_t first_layout, int B, double* d_sums, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_x0 || !d_sums) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  CallT c;
  if ((rc = begin_t(h, t, h_t, per_layout, h_layout, B, st, c))) return rc;
  if ((rc = err_begin(h, st))) return rc;
  {  // x_t ~ q(x_t | x_0) of the whole call — or the checked copy of a given x_t — into the handle's token buffer: the denoiser
     // embeds what it is handed, so a token outside the vocabulary must not reach it
    VbArgs q{};
    fill_vb(h, q, c, 0, B);
    q.x0 = d_x0;
    q.xt = d_xt;
    q.xt_out = h->tok_a;
    q.seed = seed;
    q.first_layout = first_layout;
    launch_q_sample(q, st);
    d_xt = h->tok_a;
  }
  Workspace& ws = h->ws[0];
  for (int off = 0; off < B; off += h->plan.chunk) {
    const int Bc = std::min(h->plan.chunk, B - off);
    const size_t ro = (size_t)off * h->plan.S;
    if ((rc = denoise_chunk(h, ws, d_xt + ro, c.t, Bc, st, false, c.d_t ? c.d_t + off : nullptr))) return rc;
    VbArgs p{};
    fill_vb(h, p, c, off, Bc);
    p.logits = ws.logits;
    p.ldl = h->plan.Cp;
    p.x0 = d_x0 + ro;
    p.xt = d_xt + ro;
    p.sums = d_sums + (size_t)off * ldm_vb::kNumSums;
    launch_vb_terms(p, st);
  }
  return err_end(h, st);
}

// ldm_vb_grad runs no denoiser, so it takes per-layout timesteps on every handle: stage_timesteps without its engine check
int stage_grad_timesteps(ldm_handle* h, const int32_t* h_t, int B, hipStream_t st, const int32_t** d_t) {
  for (int b = 0; b < B; ++b)
    if (h_t[b] < 0 || h_t[b] >= h->T) return h->fail(-1, "timestep %d of layout %d out of range [0,%d)", h_t[b], b, h->T);  // constrained.py:139
  if (!h->st_t) {
    int rc = h->dalloc(&h->st_t, (size_t)h->cfg.max_batch);
    if (rc) return rc;
    h->st_t_host.resize((size_t)h->cfg.max_batch);
  }
  std::copy(h_t, h_t + B, h->st_t_host.begin());
  HIP_OK(h, hipMemcpyAsync(h->st_t, h->st_t_host.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  *d_t = h->st_t;
  return 0;
}

}  // namespace

extern "C" int ldm_vb_grad(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, int B,
                           const double* d_coef, float* d_grad, double* d_sums, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_logits || !d_x0 || !d_xt || !h_t || (!d_grad && !d_sums) || (d_grad && !d_coef)) return h->fail(-1, "null argument");
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  CallT c;
  if ((rc = stage_grad_timesteps(h, h_t, B, st, &c.d_t))) return rc;
  if ((rc = err_begin(h, st))) return rc;
  VbArgs p{};
  fill_vb(h, p, c, 0, B);
  p.f32_lse = 0;   // the logits are the caller's: the reference's float64 log-softmax whatever the handle's numerics mode
  p.logits = d_logits;
  p.ldl = h->plan.C;
  p.x0 = d_x0;
  p.xt = d_xt;
  p.sums = d_sums;
  p.coef = d_coef;
  p.grad = d_grad;
  launch_vb_grad(p, st);
  return err_end(h, st);
}

extern "C" int ldm_q_sample(ldm_handle* h, const int32_t* d_x0, int t, uint64_t seed, uint64_t first_layout, int B,
                            int32_t* d_xt, void* stream) {
  return q_sample(h, d_x0, t, nullptr, false, nullptr, seed, first_layout, B, d_xt, stream);
}
extern "C" int ldm_q_sample_t(ldm_handle* h, const int32_t* d_x0, const int32_t* h_t, const uint64_t* h_layout, uint64_t seed,
                              uint64_t first_layout, int B, int32_t* d_xt, void* stream) {
  return q_sample(h, d_x0, 0, h_t, true, h_layout, seed, first_layout, B, d_xt, stream);
}

extern "C" int ldm_vb_terms(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, int t, int B,
                            double* d_sums, float* d_tok, void* stream) {
  return vb_terms(h, d_logits, d_x0, d_xt, t, nullptr, false, B, d_sums, d_tok, stream);
}
extern "C" int ldm_vb_terms_t(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, int B,
                              double* d_sums, float* d_tok, void* stream) {
  return vb_terms(h, d_logits, d_x0, d_xt, 0, h_t, true, B, d_sums, d_tok, stream);
}

extern "C" int ldm_vb_step(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, int t, uint64_t seed,
                           uint64_t first_layout, int B, double* d_sums, void* stream) {
  return vb_step(h, d_x0, d_xt, t, nullptr, false, nullptr, seed, first_layout, B, d_sums, stream);
}
extern "C" int ldm_vb_step_t(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, const int32_t* h_t, const uint64_t* h_layout,
                             uint64_t seed, uint64_t first_layout, int B, double* d_sums, void* stream) {
  return vb_step(h, d_x0, d_xt, 0, h_t, true, h_layout, seed, first_layout, B, d_sums, stream);
}
