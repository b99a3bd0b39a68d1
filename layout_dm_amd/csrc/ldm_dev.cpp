// Development hooks of libldm_hip.so (NOT part of the public ABI in include/ldm_hip.h): the s_memtime phase sums of the instrumented
// kernels (tools/phase_probe.py, lngemm_probe.py, attnout_probe.py) and a unit check of the fused attention + out_proj launch on
// synthetic operands (tests/test_attnout_gpu.py), and one row-resident LayerNorm + GEMM launch of a live handle on the caller's rows
// (ldm_dev_lngemm_run, tests/test_lngemm_gpu.py), and one fused attention + out_proj (+ FFN) launch of a live handle on the caller's panels
// (ldm_dev_attnout_run, tests/test_attnout_kernel_gpu.py), and one launch of a LayerNorm / GEMM / attention kernel of the tiled engines on the caller's
// buffers (ldm_dev_layernorm_run, ldm_dev_gemm_run, ldm_dev_attention_run, tests/test_tiled_kernels_gpu.py), and one launch of the relation logit-adjustment kernel on the caller's buffers (ldm_dev_relation_run,
// tests/test_relation_kernel_gpu.py), and the counters of the
// handle's cache of captured loops (ldm_dev_graph_cache, tests/test_loop_graph_cache_gpu.py).  Nothing in the product path calls into this file.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "ldm_handle.h"
#include "ldm_kernels.h"

using namespace ldm;

namespace {

// device buffers of one call, released on every return path
struct DevScope {
  std::vector<void*> bufs;
  template <typename T>
  bool alloc(T** p, size_t bytes, const void* host = nullptr) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return false;
    bufs.push_back(d);
    *p = static_cast<T*>(d);
    return (host ? hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes)) == hipSuccess;
  }
  ~DevScope() {
    for (void* p : bufs) (void)hipFree(p);
  }
};

}  // namespace

// s_memtime phase sums of the instrumented stack kernel (LDM_ATTN_TM=1, per-step path); every read resets the counters
namespace ldm {
void stack_phase_read(unsigned long long* out16);
}  // namespace ldm
extern "C" void ldm_dev_stack_phases(unsigned long long* out16) { ldm::stack_phase_read(out16); }
extern "C" void ldm_dev_lngemm_phases(unsigned long long* out8) { ldm::lngemm_phase_read(out8); }
extern "C" void ldm_dev_attnout_phases(unsigned long long* out24) { ldm::attnout_phase_read(out24); }

// Which layouts of the most recent ldm_sample_loop call took the step-0 shortcut of the one-launch loop (their first step's logits
// read from the handle's table): the proof that the path ran (tests/test_step0_cache_gpu.py).  host_out: n bytes on the host.
extern "C" int ldm_dev_step0_flags(ldm_handle* h, uint8_t* host_out, int n) {
  if (!h || !host_out) return -1;
  if (!h->step0_flags) return h->fail(-1, "the handle has no one-launch loop (no step-0 flags)");
  if (n < 1 || n > h->cfg.max_batch) return h->fail(-1, "n outside [1, max_batch]");
  ON_DEVICE(h);
  HIP_OK(h, hipDeviceSynchronize());
  HIP_OK(h, hipMemcpy(host_out, h->step0_flags, (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// The handle's cache of captured loops (ldm_handle.h GraphCache): entries held now, and entries captured since create — one per key,
// whatever its lane count.  A hit leaves both as they were (tests/test_loop_graph_cache_gpu.py).
extern "C" int ldm_dev_graph_cache(ldm_handle* h, int* entries, int* captures) {
  if (!h || !entries || !captures) return -1;
  *entries = (int)h->graphs.entries.size();
  *captures = h->graphs.captures;
  return 0;
}

// Unit check of the split mode's fused attention + out_proj launch (kernels_attnout.hip) on synthetic operands against a float64
// host computation of the same block: q / k / v (amplitude qk_amp / 1) -> hi / lo panels as in_proj's epilogue writes them, out_proj
// weights with max |w| in [1, 2) (what ldm_weights.cpp make_w16's power-of-two pre-scale produces) -> k-step image, residual rows,
// bias.  err_out[0] = max |out - ref| / max |ref - res| over the B layouts (every row, every column), err_out[1] = the same for a
// computation from the fp16 hi parts only (what a dropped lo term would look like: the yardstick), err_out[2] = max |ref - res|.
// tests/test_attnout_gpu.py.
#include <cmath>

#include "ldm_pack.h"
// zero_lo (debugging aid): bit 0 / 1 / 2 / 3 = drop the lo halves of q / k / v / the weights from the INPUTS (kernel and reference alike)
extern "C" int ldm_dev_attnout_check(int B, int S, float qk_amp, uint32_t seed, double* err_out, int zero_lo) {
  const int H = 8, dh = 58, D = 464, NP = 48;
  if (B < 1 || S < 1 || S > 128) return -1;
  const size_t M = (size_t)B * S, rows = M + 128;   // (a layout reads 128 rows from its first one)
  const size_t PS = rows * 64;
  uint32_t s = seed * 2654435761u + 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return ((float)(s >> 8) / 8388608.0f) - 1.0f;
  };
  std::vector<float> q(M * H * dh), k(M * H * dh), v(M * H * dh), res(M * D), bias(D), wo((size_t)D * D);
  for (auto& x : q) x = rnd() * qk_amp;
  for (auto& x : k) x = rnd() * qk_amp;
  for (auto& x : v) x = rnd();
  for (auto& x : res) x = rnd() * 2.0f;
  for (auto& x : bias) x = rnd() * 0.1f;
  for (auto& x : wo) x = rnd() * 1.9f;
  if (zero_lo & 16)   // (debug: W = 32 I, so that out - res - bias IS the attention output)
    for (int n = 0; n < D; ++n)
      for (int kk = 0; kk < D; ++kk) wo[(size_t)n * D + kk] = n == kk ? 32.0f : 0.0f;
  const float out_scale = 1.0f / 32.0f;
  auto split = [&](float x, uint16_t& hi, uint16_t& lo) {
    const __half hh = __float2half(x);
    const __half ll = __float2half(x - __half2float(hh));
    memcpy(&hi, &hh, 2);
    memcpy(&lo, &ll, 2);
  };
  std::vector<uint16_t> ph((size_t)NP * rows * 32, 0), pl((size_t)NP * rows * 32, 0);
  const std::vector<float>* src[3] = {&q, &k, &v};
  for (int which = 0; which < 3; ++which)
    for (size_t r = 0; r < M; ++r)
      for (int h = 0; h < H; ++h)
        for (int d = 0; d < dh; ++d) {
          const size_t pn = (size_t)(which * H + h) * 2 + d / 32;
          split((*src[which])[(r * H + h) * dh + d], ph[(pn * rows + r) * 32 + d % 32], pl[(pn * rows + r) * 32 + d % 32]);
          if (zero_lo & (1 << which)) pl[(pn * rows + r) * 32 + d % 32] = 0;
        }
  std::vector<uint16_t> wh((size_t)D * 512, 0), wl((size_t)D * 512, 0);
  for (int n = 0; n < D; ++n)
    for (int kk = 0; kk < D; ++kk) {
      split(wo[(size_t)n * D + kk], wh[(size_t)n * 512 + kk], wl[(size_t)n * 512 + kk]);
      if (zero_lo & 8) wl[(size_t)n * 512 + kk] = 0;
    }
  const std::vector<uint16_t> img = ldm_pack::pack_x3_kstep_image(wh.data(), wl.data(), D, 512, H, dh);
  DevScope dv;
  char *dph = nullptr, *dpl = nullptr, *dimg = nullptr;
  float *dres = nullptr, *dbias = nullptr, *dout = nullptr;
  if (!dv.alloc(&dph, ph.size() * 2, ph.data()) || !dv.alloc(&dpl, pl.size() * 2, pl.data()) || !dv.alloc(&dimg, img.size() * 2, img.data()) ||
      !dv.alloc(&dres, res.size() * 4, res.data()) || !dv.alloc(&dbias, bias.size() * 4, bias.data()) || !dv.alloc(&dout, res.size() * 4))
    return -3;
  AttnOutArgs a{};
  a.qkv_hi = dph; a.qkv_lo = dpl; a.panel_stride = PS; a.w_img = dimg; a.res = dres; a.bias = dbias; a.out = dout;
  a.S = S; a.D = D; a.scale = 1.0f / sqrtf((float)dh); a.out_scale = out_scale;
  if (launch_attnout16x3(a, B, 0)) return -4;
  std::vector<float> out(res.size());
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess ||
      hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return -2;
  double e_full = 0, e_hi = 0, mag = 0;
  for (int i = 3; i < 25; ++i) err_out[i] = 0;   // (debug: [3..5] location of the maximum, [6..9] per wave, [10..24] per column tile)
  auto h2d = [&](uint16_t u) {
    __half hh;
    memcpy(&hh, &u, 2);
    return (double)__half2float(hh);
  };
  std::vector<double> att((size_t)S * H * dh), att_hi((size_t)S * H * dh), p(S);
  for (int b = 0; b < B; ++b) {
    for (int variant = 0; variant < 2; ++variant) {   // 0: full values, 1: fp16 hi parts only
      std::vector<double>& o = variant ? att_hi : att;
      auto val = [&](int which, size_t r, int h, int d) {
        const size_t pn = (size_t)(which * H + h) * 2 + d / 32, i = (pn * rows + r) * 32 + d % 32;
        return variant ? h2d(ph[i]) : h2d(ph[i]) + h2d(pl[i]);
      };
      for (int h = 0; h < H; ++h)
        for (int i = 0; i < S; ++i) {
          double mx = -1e300;
          for (int j = 0; j < S; ++j) {
            double sc = 0;
            for (int d = 0; d < dh; ++d) sc += val(0, (size_t)b * S + i, h, d) * val(1, (size_t)b * S + j, h, d);
            p[j] = sc * (double)a.scale;
            mx = std::max(mx, p[j]);
          }
          double sum = 0;
          for (int j = 0; j < S; ++j) sum += (p[j] = std::exp(p[j] - mx));
          for (int d = 0; d < dh; ++d) {
            double acc = 0;
            for (int j = 0; j < S; ++j) acc += p[j] * val(2, (size_t)b * S + j, h, d);
            o[((size_t)i * H + h) * dh + d] = acc / sum;
          }
        }
    }
    for (int i = 0; i < S; ++i)
      for (int n = 0; n < D; ++n) {
        double acc = 0, acc_hi = 0;
        for (int kk = 0; kk < D; ++kk) {
          acc += att[(size_t)i * D + kk] * (h2d(wh[(size_t)n * 512 + kk]) + h2d(wl[(size_t)n * 512 + kk]));
          acc_hi += att_hi[(size_t)i * D + kk] * h2d(wh[(size_t)n * 512 + kk]);
        }
        const size_t idx = ((size_t)b * S + i) * D + n;
        const double ref = (double)res[idx] + (double)bias[n] + acc * out_scale;
        const double ref_hi = (double)res[idx] + (double)bias[n] + acc_hi * out_scale;
        mag = std::max(mag, std::fabs(ref - (double)res[idx]));
        if (std::fabs((double)out[idx] - ref) > e_full) { err_out[3] = b; err_out[4] = i; err_out[5] = n; }
        e_full = std::max(e_full, std::fabs((double)out[idx] - ref));
        if ((zero_lo & 16) && std::fabs((double)out[idx] - ref) > 3e-6)
          printf("  row %d col %d (head %d d %d): got %.9g ref %.9g diff %.3e\n", i, n, n / dh, n % dh, (double)out[idx] - res[idx] - bias[n], ref - res[idx] - bias[n], (double)out[idx] - ref);
        err_out[6 + i / 32] = std::max(err_out[6 + i / 32], std::fabs((double)out[idx] - ref));          // per wave
        err_out[10 + n / 32] = std::max(err_out[10 + n / 32], std::fabs((double)out[idx] - ref));        // per column tile
        e_hi = std::max(e_hi, std::fabs(ref_hi - ref));
      }
  }
  err_out[0] = e_full / mag;
  err_out[1] = e_hi / mag;
  err_out[2] = mag;
  return 0;
}

// ONE lngemm16x3_k launch (kernels_lngemm.hip) of a live handle on the caller's device buffers: the arguments are the product's own
// (ldm_denoise.cpp lngemm_*_args: the handle's images, pre-scales, parameter tables and mode) with the workspace pointers and M swapped for
// the caller's.  No reference arithmetic here: tests/_lngemm_cases.py holds the float64 side.  0 on success; -1 when the handle has no
// row-resident kernels, the requested form does not exist for it, or launch_lngemm16x3 refuses the arguments; -2 on a HIP error.
struct ldm_dev_lngemm_io {
  int32_t launch;            // 0 AdaLN + in_proj of `layer` at timestep `t` | 1 norm2 + linear1 + ReLU of `layer` | 2 head LayerNorm + head
  int32_t layer, t;
  int32_t prologue;          // linear2 of the preceding layer (in_proj: layer - 1; the head: the last layer) in front of the LayerNorm
  int32_t M;
  int32_t pre_lda;           // row-major hidden activations: halves per row (0: the handle's Fp)
  const int32_t* tokens;     // [M]: in_proj of layer 0 gathers its rows
  const float* x;            // [M, 464] rows (no tokens, no prologue)
  const __half *hid_hi, *hid_lo;   // prologue: hidden activations in the form the handle keeps (panels or rows; lo unused in the one-product form)
  const float* res;          // prologue: fp32 residual rows [M, 464]
  float* y32;                // in_proj: AdaLN(x) [M, 464] (may alias x)
  float* C32;                // fp32 output rows [M, ldc32]
  __half *C16, *C16lo;       // fp16 hi / lo output, rows [M, ldc16] or panels
  int64_t ldc32, ldc16;      // 0: the product's
  uint64_t panel_stride;     // bytes between output panels (0: the product's)
  uint64_t pre_panel_stride; // bytes between hidden panels of the prologue (0: the product's)
};
extern "C" int ldm_dev_lngemm_run(ldm_handle* h, const ldm_dev_lngemm_io* io) {
  if (!h || !io) return -1;
  if (!h->finalized) return h->fail(-1, "weights not finalized");
  if (h->plan.structure != Structure::RowResident) return h->fail(-1, "the handle has no row-resident LayerNorm + GEMM kernels");
  if (io->M < 1 || io->launch < 0 || io->launch > 2) return h->fail(-1, "ldm_dev_lngemm_run: bad launch / M");
  const bool in_proj = io->launch == 0, lin1 = io->launch == 1, pre = io->prologue != 0;
  if (in_proj && (io->layer < 0 || io->layer >= h->L || io->t < 0 || io->t >= h->T)) return h->fail(-1, "ldm_dev_lngemm_run: layer / timestep out of range");
  if (lin1 && (io->layer < 0 || io->layer >= h->L)) return h->fail(-1, "ldm_dev_lngemm_run: layer out of range");
  // the forms the handle's own pass runs: no linear1 / linear2 launches behind the fused FFN, linear2 in front of in_proj from layer 1 on
  if ((lin1 || pre) && h->plan.ffn_fused) return h->fail(-1, "ldm_dev_lngemm_run: the handle's FFN runs behind the attention");
  if (pre && (lin1 || (in_proj && io->layer < 1))) return h->fail(-1, "ldm_dev_lngemm_run: no prologue in front of this launch");
  ON_DEVICE(h);
  Workspace ws{};   // the launch's view of the caller's buffers, under the names the product's pass gives them
  ws.P = in_proj ? io->y32 : const_cast<float*>(io->x);
  ws.Q = lin1 ? const_cast<float*>(io->x) : const_cast<float*>(io->res);
  ws.hid16 = lin1 ? io->C16 : const_cast<__half*>(io->hid_hi);
  ws.hid16lo = lin1 ? io->C16lo : const_cast<__half*>(io->hid_lo);
  ws.qkvp_hi = io->C16; ws.qkvp_lo = io->C16lo; ws.qkv32 = io->C32; ws.logits = io->C32;
  LnGemmArgs a = in_proj ? ldm_host::lngemm_in_proj_args(h, ws, io->tokens, io->t, io->layer, io->M, pre)
                 : lin1  ? ldm_host::lngemm_linear1_args(h, ws, io->layer, io->M)
                         : ldm_host::lngemm_head_args(h, ws, io->M, pre);
  if (in_proj) a.x = io->x;   // (the product normalises P in place; here the rows may come from a buffer of their own)
  if (io->ldc32) a.ldc32 = (int)io->ldc32;
  if (io->ldc16) a.ldc16 = (int)io->ldc16;
  if (io->panel_stride && a.panel_out) a.panel_stride = (size_t)io->panel_stride;
  if (pre && io->pre_panel_stride && a.pre_panel_stride) a.pre_panel_stride = (size_t)io->pre_panel_stride;
  if (pre && io->pre_lda) a.pre_lda = io->pre_lda;
  // the pointers launch_lngemm16x3 does not check itself: the rows (unless gathered or computed by the prologue), y32, an output
  const bool rows_missing = !a.tokens && !pre && !a.x;
  if (rows_missing || (a.ada && !a.y32) || (!a.C32 && !a.C16)) return h->fail(-1, "ldm_dev_lngemm_run: null operand");
  if (launch_lngemm16x3(a, 0)) return h->fail(-1, "row-resident LayerNorm + GEMM: geometry not supported");
  HIP_OK(h, hipStreamSynchronize(0));
  HIP_OK(h, hipGetLastError());
  return 0;
}

// ONE attnout16x3_k launch (kernels_attnout.hip: attention + out_proj, in the hybrid mode + LayerNorm-2 + the plain-fp16 FFN) of a live handle
// on the caller's device buffers: the arguments are the product's own for `layer` (ldm_denoise.cpp attnout_args: out_proj's
// k-step image, bias and pre-scale, the two-product flag, the FFN's chunk image and parameters, 1 / sqrt(dh)) with the panels, their stride,
// res, out / ffn_out, B and S swapped for the caller's — S as well: no weight depends on it and the launch takes any 1 <= S <= 128.  The io
// struct carries the capacity of every buffer; no reference arithmetic here (tests/_attnout_cases.py holds the float64 side).  -1, before any
// launch, for a handle without the kernel and for whatever the kernel's stated preconditions forbid; -2 on a HIP error.
struct ldm_dev_attnout_io {
  int32_t layer, B, S, pad_;
  const void *qkv_hi, *qkv_lo;   // [48 panels] of panel_stride bytes: 64 bytes per row
  uint64_t panel_stride;         // bytes between panels
  const float* res;              // [B S, 464] residual rows
  float* out;                    // [B S, 464]: `out` of the plain forms, `ffn_out` of the FFN form (which may alias res: the product's own use)
  int64_t panel_rows;            // capacities: rows (of 64 bytes) behind the start of EVERY panel, the last one included
  int64_t res_rows, out_rows;    // ... rows of 464 floats
};
extern "C" int ldm_dev_attnout_run(ldm_handle* h, const ldm_dev_attnout_io* io) {
  if (!h || !io) return -1;
  if (!h->finalized) return h->fail(-1, "weights not finalized");
  if (!h->plan.attnout) return h->fail(-1, "the handle has no fused attention + out_proj kernel");
  if (io->layer < 0 || io->layer >= h->L) return h->fail(-1, "ldm_dev_attnout_run: layer out of range");
  const int64_t B = io->B, S = io->S;
  if (B < 1 || S < 1 || S > 128 || B * S > INT32_MAX) return h->fail(-1, "ldm_dev_attnout_run: B < 1, S outside [1, 128] or B S beyond int");
  auto ok16 = [](const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (!ok16(io->qkv_hi) || !ok16(io->qkv_lo) || !ok16(io->res) || !ok16(io->out))
    return h->fail(-1, "ldm_dev_attnout_run: null or misaligned pointer");
  // every layout reads 128 rows from its first one in every panel (launch_attnout16x3 states the same bound on the stride)
  const uint64_t reach = (uint64_t)((B - 1) * S + 128);
  if ((io->panel_stride & 15) || io->panel_stride < reach * 64) return h->fail(-1, "ldm_dev_attnout_run: panel_stride");
  if (io->panel_rows < (int64_t)reach) return h->fail(-1, "ldm_dev_attnout_run: panels shorter than the launch's 128-row reach");
  if (io->res_rows < B * S || io->out_rows < B * S) return h->fail(-1, "ldm_dev_attnout_run: res / out shorter than B S rows");
  ON_DEVICE(h);
  Workspace ws{};   // the launch's view of the caller's buffers, under the names the product's pass gives them
  ws.qkvp_hi = static_cast<__half*>(const_cast<void*>(io->qkv_hi)); ws.qkvp_lo = static_cast<__half*>(const_cast<void*>(io->qkv_lo));
  ws.P = const_cast<float*>(io->res); ws.Q = io->out;
  AttnOutArgs a = ldm_host::attnout_args(h, ws, io->layer);
  a.panel_stride = (size_t)io->panel_stride; a.S = (int)S;
  if (a.ffn_img) a.ffn_out = io->out;   // (the product writes x + attention + FFN over res; here to the caller's `out`, which may alias it)
  if (launch_attnout16x3(a, (int)B, 0)) return h->fail(-1, "fused attention + out_proj: geometry not supported");
  HIP_OK(h, hipStreamSynchronize(0));
  HIP_OK(h, hipGetLastError());
  return 0;
}

// ONE launch of a kernel of the tiled engines (ldm_denoise.cpp denoise_chunk_tiled / denoise_chunk_fast) on the caller's device buffers, without
// a handle: launch_layernorm, launch_gemm / launch_gemm16x3 / launch_gemm16, launch_attention / launch_attention16 (tests/test_tiled_kernels_gpu.py).
// The io structs mirror LnArgs / GemmArgs / AttnArgs and carry the capacity of every buffer; no reference arithmetic here (tests/_tiled_cases.py
// holds the float64 side).  -1, before any launch, for whatever the kernels' stated preconditions forbid — the kernels themselves check nothing;
// the launch runs on the current device's null stream; -2 on a HIP error.
namespace {

bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
int64_t whole_tiles(int n, int tile) { return (int64_t)((n + tile - 1) / tile) * tile; }
int dev_launched() {
  if (hipStreamSynchronize(0) != hipSuccess) return -2;
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

struct ldm_dev_layernorm_io {   // LnArgs
  const float* x;
  const int32_t* tokens;
  const float *emb, *pos, *p0, *p1;
  float* y32;
  __half *y16, *y16lo;
  float* stats_out;             // [M] (mean, rstd) pairs
  int32_t M, D, S, ld16, ada, raw;
  int64_t x_rows, n_tokens, emb_rows, pos_rows, n_p, y32_rows, y16_rows, stats_rows;   // capacities: rows of D (y16 / y16lo: of ld16) or elements
};
extern "C" int ldm_dev_layernorm_run(const ldm_dev_layernorm_io* io) {
  if (!io) return -1;
  const int M = io->M, D = io->D;
  if (M < 1 || D < 4 || D % 4 || D > 1024) return -1;   // float4 per lane, at most ln_rows<4>'s 4 x 64 of them
  if (io->tokens) {
    if (!io->emb || !io->pos || io->S < 1 || io->n_tokens < M || io->pos_rows < std::min(M, io->S) || io->emb_rows < 1) return -1;
    if (!aligned(io->emb, 16) || !aligned(io->pos, 16)) return -1;
    std::vector<int32_t> tok(M);   // (the gather's row bound: the one check that needs the operand's values)
    if (hipMemcpy(tok.data(), io->tokens, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    for (int32_t t : tok)
      if (t < 0 || t >= io->emb_rows) return -1;
  } else if (!io->x || !aligned(io->x, 16) || io->x_rows < M) {
    return -1;
  }
  if (io->raw) {
    if (!io->y32) return -1;
  } else {
    if (!io->p0 || !io->p1 || !aligned(io->p0, 16) || !aligned(io->p1, 16) || io->n_p < D) return -1;
    if (!io->y32 && !io->y16) return -1;
  }
  if (io->y32 && (!aligned(io->y32, 16) || io->y32_rows < M)) return -1;
  if (io->y16lo && !io->y16) return -1;
  if (io->y16 && (!aligned(io->y16, 8) || (io->y16lo && !aligned(io->y16lo, 8)) || io->ld16 < D || io->ld16 % 4 || io->y16_rows < M)) return -1;
  if (io->stats_out && (!aligned(io->stats_out, 8) || io->stats_rows < M)) return -1;
  LnArgs a{};
  a.x = io->x; a.tokens = io->tokens; a.emb = io->emb; a.pos = io->pos; a.p0 = io->p0; a.p1 = io->p1;
  a.y32 = io->y32; a.y16 = io->y16; a.y16lo = io->y16lo; a.stats_out = reinterpret_cast<float2*>(io->stats_out);
  a.M = M; a.D = D; a.S = io->S; a.ld16 = io->ld16; a.ada = io->ada; a.raw = io->raw;
  (void)hipGetLastError();
  launch_layernorm(a, 0);
  return dev_launched();
}

struct ldm_dev_gemm_io {        // GemmArgs + tag + kind
  const void *A, *Alo, *W, *Wlo;
  const float *bias, *res;
  float* C32;
  __half *C16, *C16lo;
  int32_t M, N, K, lda, ldw, ldres, ldc32, ldc16, relu;
  int32_t tag;                  // Linear class of the fp16 kernels (0 qkv, 1 attn_out, 2 ffn1, 3 ffn2, 4 head)
  int32_t kind;                 // 0 launch_gemm (fp32) | 1 launch_gemm16x3 (fp16 hi / lo) | 2 launch_gemm16 (fp16)
  float out_scale;
  int64_t a_rows, w_rows, n_bias, res_rows, c32_rows, c16_rows;   // capacities: rows of the buffer's leading dimension, elements of bias
};
extern "C" int ldm_dev_gemm_run(const ldm_dev_gemm_io* io) {
  if (!io) return -1;
  const int M = io->M, N = io->N, K = io->K, kind = io->kind;
  if (M < 1 || N < 1 || K < 1 || kind < 0 || kind > 2 || io->tag < 0 || io->tag > 4) return -1;
  if (!io->A || !io->W || !aligned(io->A, 16) || !aligned(io->W, 16) || io->lda < K || io->ldw < K) return -1;   // 16-byte LDS-DMA segments
  if (kind == 0) {
    // gemm_f32_tile: 16-wide K tiles; rows past M / N are clamped to the last one, so M and N rows suffice; no out_scale in its epilogue
    if (K % 16 || io->lda % 4 || io->ldw % 4 || io->a_rows < M || io->w_rows < N) return -1;
    if (io->Alo || io->Wlo || (io->out_scale != 0.f && io->out_scale != 1.f)) return -1;
  } else {
    // gemm16x3_k / gemm16_k load whole tiles without a bounds check: 256 (x3, as launch_gemm16x3 states it) / 128 rows
    const int tile = kind == 1 ? 256 : 128;
    if (K % (kind == 1 ? 32 : kGemm16BK) || io->lda % 8 || io->ldw % 8) return -1;
    if (io->a_rows < whole_tiles(M, tile) || io->w_rows < whole_tiles(N, tile)) return -1;
    if (kind == 1 && (!io->Alo || !io->Wlo || !aligned(io->Alo, 16) || !aligned(io->Wlo, 16) || io->out_scale < 0.f)) return -1;
    if (kind == 2 && (io->Alo || io->Wlo || io->C16lo || (io->out_scale != 0.f && io->out_scale != 1.f))) return -1;
    if (N % 4 == 0) {   // their epilogues move 4 columns per access
      if ((io->bias && !aligned(io->bias, 16)) || (io->res && (!aligned(io->res, 16) || io->ldres % 4)) ||
          (io->C32 && (!aligned(io->C32, 16) || io->ldc32 % 4)) ||
          (io->C16 && (!aligned(io->C16, 8) || io->ldc16 % 4 || (io->C16lo && !aligned(io->C16lo, 8)))))
        return -1;
    }
  }
  if (!io->C32 && !io->C16) return -1;
  if (io->C16lo && !io->C16) return -1;
  if (io->bias && io->n_bias < N) return -1;
  if (io->res && (io->ldres < N || io->res_rows < M)) return -1;
  if (io->C32 && (io->ldc32 < N || io->c32_rows < M)) return -1;
  if (io->C16 && (io->ldc16 < N || io->c16_rows < M)) return -1;
  GemmArgs g{};
  g.A = io->A; g.Alo = io->Alo; g.W = io->W; g.Wlo = io->Wlo; g.bias = io->bias; g.res = io->res;
  g.C32 = io->C32; g.C16 = io->C16; g.C16lo = io->C16lo;
  g.M = M; g.N = N; g.K = K; g.lda = io->lda; g.ldw = io->ldw; g.ldres = io->ldres; g.ldc32 = io->ldc32; g.ldc16 = io->ldc16;
  g.relu = io->relu; g.precision = kind == 0 ? LDM_PREC_EXACT_F32 : kind == 1 ? LDM_PREC_SPLIT_F16 : LDM_PREC_FAST_F16;
  g.out_scale = io->out_scale;
  (void)hipGetLastError();
  if (kind == 0) launch_gemm(g, 0);
  else if (kind == 1) launch_gemm16x3(g, io->tag, 0);
  else launch_gemm16(g, io->tag, 0);
  return dev_launched();
}

struct ldm_dev_attention_io {   // AttnArgs + kind
  const void* qkv;
  float* out32;
  __half *out16, *out16lo;
  int32_t in_f16, B, S, H, dh, D, ld, ldo32, ldo16;
  int32_t kind;                 // 0 launch_attention | 1 launch_attention16 (head-padded fp16 layout: ld >= 3 H 64, ldo16 >= H 64; D is ignored)
  int64_t qkv_rows, out32_rows, out16_rows;   // capacities in rows of ld / ldo32 / ldo16
};
extern "C" int ldm_dev_attention_run(const ldm_dev_attention_io* io) {
  if (!io) return -1;
  const int B = io->B, S = io->S, H = io->H, dh = io->dh;
  if (B < 1 || S < 1 || H < 1 || dh < 1 || dh > 64 || (io->kind != 0 && io->kind != 1)) return -1;   // ldm_create: head_dim <= 64
  const int64_t M = (int64_t)B * S;
  if (M > (1 << 24) || !io->qkv || !aligned(io->qkv, 16) || io->qkv_rows < M) return -1;
  if (io->kind == 1) {
    // attn_mfma_k: one 128 x 128 score tile, 128-byte head rows read as 16-byte chunks, 8-byte stores
    if (!io->in_f16 || S > 128 || io->out32 || io->out16lo || !io->out16 || !aligned(io->out16, 16)) return -1;
    if (io->ld < 3 * H * 64 || io->ld % 8 || io->ldo16 < H * 64 || io->ldo16 % 8 || io->out16_rows < M) return -1;
    (void)hipGetLastError();
    launch_attention16(static_cast<const __half*>(io->qkv), io->out16, B, S, H, dh, io->ld, io->ldo16, 0);
    return dev_launched();
  }
  if (io->D != H * dh || io->ld < 3 * io->D) return -1;
  if ((size_t)2 * S * ((dh + 3) & ~3) * sizeof(float) > 160 * 1024) return -1;   // ldm_create: K and V of a (layout, head) in LDS
  if (!io->out32 && !io->out16) return -1;
  if (io->out16lo && !io->out16) return -1;
  if (io->out32 && (!aligned(io->out32, 16) || io->ldo32 < io->D || io->out32_rows < M)) return -1;
  if (io->out16 && (!aligned(io->out16, 16) || (io->out16lo && !aligned(io->out16lo, 16)) || io->ldo16 < io->D || io->out16_rows < M)) return -1;
  AttnArgs a{};
  a.qkv = io->qkv; a.in_f16 = io->in_f16; a.out32 = io->out32; a.out16 = io->out16; a.out16lo = io->out16lo;
  a.B = B; a.S = S; a.H = H; a.dh = dh; a.D = io->D; a.ld = io->ld; a.ldo32 = io->ldo32; a.ldo16 = io->ldo16;
  (void)hipGetLastError();
  launch_attention(a, 0);
  return dev_launched();
}

// ONE relation_update_k launch (kernels_relation.hip: the SGD of ldm_relation_core.h on a (B,C,S) or (B,S,C) tensor) on the caller's device
// buffers, without a handle (tests/test_relation_kernel_gpu.py).  The io struct mirrors RelArgs and carries the capacity of every buffer; no
// reference arithmetic here (tests/_relation_cases.py holds the float64 side).  -1, before any launch, for whatever the kernel's stated
// preconditions forbid — the kernel itself checks nothing, so the small integer arrays (offsets, node ids, the conditioned categories that
// decide which elements are nodes) are copied to the host and checked here; the launch runs on the current device's null stream; -2 on a
// HIP error.  num_update <= 0 and B == 0 go through launch_relation_update like any call: it launches nothing.
#include "ldm_relation_core.h"   // (REL_MAX_ELEM)
struct ldm_dev_relation_io {    // RelArgs
  float* logp;
  const int32_t *cond_seq, *edge_off, *edge_src, *edge_dst, *edge_attr;
  const float* centres;
  int32_t canvas_bins[4];
  float step;
  int32_t num_update, B, C, S, A, n_category, n_bin, pad_id, logp_tm;
  int64_t logp_floats, n_cond, n_edge_off, n_edge, n_centres;   // capacities in elements (n_edge: of each of the three edge arrays)
};
extern "C" int ldm_dev_relation_run(const ldm_dev_relation_io* io) {
  if (!io) return -1;
  const int64_t B = io->B, C = io->C, S = io->S, A = io->A, NB = io->n_bin;
  if (B < 0 || io->num_update < 0 || (io->logp_tm != 0 && io->logp_tm != 1)) return -1;
  // a token's four coordinates sit behind its category (position e A + 1 + x); one workgroup holds E x 4 x 32 logits and 33 boxes in LDS
  if (A != 5 || S < A || S % A || S / A > REL_MAX_ELEM || NB < 1 || NB > 32) return -1;
  if (io->n_category < 0 || C < io->n_category + 4 * NB) return -1;
  if (!io->logp || !io->cond_seq || !io->edge_off || !io->centres || !aligned(io->logp, 4) || !aligned(io->centres, 4)) return -1;
  if (io->n_edge < 0 || (io->n_edge > 0 && (!io->edge_src || !io->edge_dst || !io->edge_attr))) return -1;
  if (io->logp_floats < B * C * S || io->n_cond < B * S || io->n_edge_off < B + 1 || io->n_centres < 4 * NB) return -1;
  for (int x = 0; x < 4; ++x)
    if (io->canvas_bins[x] < 0 || io->canvas_bins[x] >= NB) return -1;
  if (B > 0) {   // (the bounds that need the operands' values)
    std::vector<int32_t> off((size_t)B + 1), seq((size_t)(B * S));
    if (hipMemcpy(off.data(), io->edge_off, off.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(seq.data(), io->cond_seq, seq.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
      return -2;
    if (off[0] < 0 || off[B] > io->n_edge) return -1;
    for (int64_t b = 0; b < B; ++b)
      if (off[b + 1] < off[b]) return -1;
    const size_t n = (size_t)(off[B] - off[0]);
    std::vector<int32_t> src(n), dst(n);
    if (n && (hipMemcpy(src.data(), io->edge_src + off[0], n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(dst.data(), io->edge_dst + off[0], n * 4, hipMemcpyDeviceToHost) != hipSuccess))
      return -2;
    for (int64_t b = 0; b < B; ++b) {
      int nodes = 0;   // node 0 is the canvas; elements with a category are nodes 1 .. nodes, in element order
      for (int64_t e = 0; e < S / A; ++e) nodes += seq[(size_t)(b * S + e * A)] != io->pad_id;
      for (int32_t k = off[b] - off[0]; k < off[b + 1] - off[0]; ++k)
        if (src[k] < 0 || src[k] > nodes || dst[k] < 0 || dst[k] > nodes) return -1;
    }
  }
  RelArgs a{};
  a.logp = io->logp; a.cond_seq = io->cond_seq; a.edge_off = io->edge_off; a.edge_src = io->edge_src; a.edge_dst = io->edge_dst;
  a.edge_attr = io->edge_attr; a.centres = io->centres;
  for (int x = 0; x < 4; ++x) a.canvas_bins[x] = io->canvas_bins[x];
  a.step = io->step; a.num_update = io->num_update; a.B = (int)B; a.C = (int)C; a.S = (int)S; a.A = (int)A;
  a.n_category = io->n_category; a.n_bin = (int)NB; a.pad_id = io->pad_id; a.logp_tm = io->logp_tm;
  (void)hipGetLastError();
  launch_relation_update(a, 0);
  return dev_launched();
}
