// Host side of scoring GIVEN layouts (include/ldm_hip.h: ldm_q_sample, ldm_vb_terms, ldm_vb_step): the forward noising draw,
// the variational bound's terms of one timestep, and the two around one denoiser pass of the handle's own numerics mode.
// Evaluation of a trained model only: no gradients, nothing of the handle's weights or schedule is written.
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
  if (e & ldm_vb::kErrRange) return h->fail(-6, "a token is outside [0, %d)", h->C);
  if (e & ldm_vb::kErrMaskX0) return h->fail(-6, "x_0 holds [MASK] (%d): only noised states do", h->vocab.mask_id);
  if (e & ldm_vb::kErrSubVocab) return h->fail(-6, "a token is not of its position's sub-vocabulary (attribute body, [PAD], [MASK])");
  return 0;
}

void fill_vb(const ldm_handle* h, VbArgs& p, int t, int B) {
  p.sched = h->sched;
  p.T = h->T;
  p.t = t;
  p.f32_lse = h->cfg.precision == LDM_PREC_FAST_F16 ? 1 : 0;
  p.B = B;
  p.S = h->S;
  p.v = h->vocab;
  p.err = h->vb_err;
}

int check_t(ldm_handle* h, int t) {
  if (t < 0 || t >= h->T) return h->fail(-1, "timestep %d out of range [0,%d)", t, h->T);  // constrained.py:139
  return 0;
}

}  // namespace

extern "C" int ldm_q_sample(ldm_handle* h, const int32_t* d_x0, int t, uint64_t seed, uint64_t first_layout, int B,
                            int32_t* d_xt, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_x0 || !d_xt) return h->fail(-1, "null argument");
  if ((rc = check_t(h, t))) return rc;
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = err_begin(h, st))) return rc;
  VbArgs p{};
  fill_vb(h, p, t, B);
  p.x0 = d_x0;
  p.xt_out = d_xt;
  p.seed = seed;
  p.first_layout = first_layout;
  launch_q_sample(p, st);
  return err_end(h, st);
}

extern "C" int ldm_vb_terms(ldm_handle* h, const float* d_logits, const int32_t* d_x0, const int32_t* d_xt, int t, int B,
                            double* d_sums, float* d_tok, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_logits || !d_x0 || !d_xt || !d_sums) return h->fail(-1, "null argument");
  if ((rc = check_t(h, t))) return rc;
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = err_begin(h, st))) return rc;
  VbArgs p{};
  fill_vb(h, p, t, B);
  p.logits = d_logits;
  p.ldl = h->C;
  p.x0 = d_x0;
  p.xt = d_xt;
  p.sums = d_sums;
  p.tok_out = d_tok;
  launch_vb_terms(p, st);
  return err_end(h, st);
}

extern "C" int ldm_vb_step(ldm_handle* h, const int32_t* d_x0, const int32_t* d_xt, int t, uint64_t seed,
                           uint64_t first_layout, int B, double* d_sums, void* stream) {
  int rc = check_ready(h, B);
  if (rc) return rc;
  if (!d_x0 || !d_sums) return h->fail(-1, "null argument");
  if ((rc = check_t(h, t))) return rc;
  ON_DEVICE(h);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = err_begin(h, st))) return rc;
  {  // x_t ~ q(x_t | x_0) of the whole call — or the checked copy of a given x_t — into the handle's token buffer: the denoiser
     // embeds what it is handed, so a token outside the vocabulary must not reach it
    VbArgs q{};
    fill_vb(h, q, t, B);
    q.x0 = d_x0;
    q.xt = d_xt;
    q.xt_out = h->tok_a;
    q.seed = seed;
    q.first_layout = first_layout;
    launch_q_sample(q, st);
    d_xt = h->tok_a;
  }
  Workspace& ws = h->ws[0];
  for (int off = 0; off < B; off += h->chunk) {
    const int Bc = std::min(h->chunk, B - off);
    const size_t ro = (size_t)off * h->S;
    if ((rc = denoise_chunk(h, ws, d_xt + ro, t, Bc, st))) return rc;
    VbArgs p{};
    fill_vb(h, p, t, Bc);
    p.logits = ws.logits;
    p.ldl = h->Cp;
    p.x0 = d_x0 + ro;
    p.xt = d_xt + ro;
    p.sums = d_sums + (size_t)off * ldm_vb::kNumSums;
    launch_vb_terms(p, st);
  }
  return err_end(h, st);
}
