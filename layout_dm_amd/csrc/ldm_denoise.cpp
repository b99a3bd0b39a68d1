// Host side of libldm_hip.so: the launch sequence of ONE denoiser pass over a chunk of layouts, per numerics mode
// (CategoricalTransformer.forward, nn_lib.py:191-237 + transformer_utils.py:165-246).  One function per engine structure, each the
// launch list of that engine from top to bottom; denoise_chunk (last) picks among them.
// Per-layout timesteps (the ldm_*_t entry points): d_t, a device array of the chunk's Bc timesteps, or nullptr — then every layout runs
// at t, today's code.  With d_t the AdaLN launches take each row's parameters from the table at its layout's timestep (LnArgs /
// LnGemmArgs t_rows); nothing else of a pass depends on t.
#include "ldm_handle.h"
#include "ldm_pack.h"

using namespace ldm_host;

double ldm_host::gemm_flops(int M, int N, int K) { return 2.0 * M * N * K; }

static double attention_flops(const ldm_handle* h, int Bc) { return 4.0 * Bc * h->H * (double)h->plan.S * h->plan.S * h->plan.dh; }

// ------------------------------------------------------------------------------------------ the two launch helpers
// One LayerNorm launch (kernels_norm.hip) over x [M, D]: AdaLN (p0 / p1 = scale / shift; with `tokens`, x = emb[token] + pos first) or
// nn.LayerNorm (gamma / beta), into whichever of y32 / y16 / y16lo the mode keeps (the others nullptr); ld16 = width of the fp16 rows
// d_t / layer (ada only): per-layout timesteps — the parameters of row m are the AdaLN table's at (d_t[m / S], layer)
static void layernorm(ldm_handle* h, hipStream_t st, const char* name, int M, const float* x, const int32_t* tokens, const float* p0,
                      const float* p1, int ada, float* y32, __half* y16, __half* y16lo, int ld16, const int32_t* d_t = nullptr, int layer = 0) {
  LnArgs a{};
  a.x = x; a.tokens = tokens; a.emb = h->emb; a.pos = h->pos;
  a.p0 = p0; a.p1 = p1; a.ada = ada;
  if (ada && d_t) { a.t_rows = d_t; a.ada_tab = h->adaln; a.t_stride = h->L * 2 * h->D; a.layer_off = layer * 2 * h->D; }
  a.y32 = y32; a.y16 = y16; a.y16lo = y16lo;
  a.M = M; a.D = h->D; a.S = h->plan.S; a.ld16 = ld16;
  if (ada && h->plan.instance_norm) {   // norm1 = AdaInsNorm: statistics per (layout, channel) over the layout's rows — three reads of x
    ldm_handle::Scope sc(h, st, "adainsnorm", 0, (double)M * h->D * (12 + (y32 ? 4 : 0) + (y16 ? 2 : 0)));
    launch_instancenorm(a, st);
    return;
  }
  ldm_handle::Scope sc(h, st, name, 0, (double)M * h->D * (4 + (y32 ? 4 : 0) + (y16 ? 2 : 0)));
  launch_layernorm(a, st);
}

// An operand of the tiled GEMMs in the form its mode keeps: fp32 (exact: hi / lo are nullptr) or fp16 hi + lo with the K axis padded
// (split); scale = 2^-k of a split weight tensor's power-of-two pre-scale
struct Operand {
  const float* f32;
  const __half *hi, *lo;
  float scale = 1.f;
};

// One tiled GEMM launch of the exact / split engines:  C = act(scale · A W^T + bias) + res  with A [M, K], W [N, K] (split: K padded to
// Kp).  exact: fp32 MFMA tiles (kernels_gemm.hip); split: the fp16 x 3 LDS-DMA GEMM (kernels_gemm16.hip gemm16x3_k), whose tag names the
// Linear class (0 qkv, 1 attn_out, 2 ffn1, 3 ffn2, 4 head)
static int tiled_gemm(ldm_handle* h, hipStream_t st, const char* name, int tag, int M, int N, int K, int Kp, const Operand& A,
                      const Operand& W, const float* bias, int relu, const float* res, float* C32, int ldc32, __half* C16 = nullptr,
                      __half* C16lo = nullptr, int ldc16 = 0) {
  const bool split = h->plan.split_type();
  GemmArgs g{};
  g.A = split ? (const void*)A.hi : (const void*)A.f32; g.Alo = A.lo;
  g.W = split ? (const void*)W.hi : (const void*)W.f32; g.Wlo = W.lo; g.out_scale = W.scale;
  g.bias = bias; g.relu = relu; g.res = res; g.ldres = h->D;
  g.C32 = C32; g.ldc32 = ldc32; g.C16 = C16; g.C16lo = C16lo; g.ldc16 = ldc16;
  g.M = M; g.N = N; g.K = g.lda = g.ldw = split ? Kp : K; g.precision = split ? LDM_PREC_SPLIT_F16 : LDM_PREC_EXACT_F32;
  ldm_handle::Scope sc(h, st, name, gemm_flops(M, N, K), (double)M * K * (split ? 2 : 4) + (double)M * N * (res ? 8 : C32 ? 4 : 2));
  if (!split) {
    launch_gemm(g, st);
    return 0;
  }
  if (g.K % 32) return h->fail(-4, "split GEMM: K = %d is not a multiple of 32", g.K);   // (Dp / Fp are multiples of 64)
  launch_gemm16x3(g, tag, st);
  return 0;
}

// ------------------------------------------------------------------------------------------ fast, the reference's backbone
// The stack kernel (kernels_stack.hip) — ONE launch for all layers and the vocabulary head, a layout's rows in its workgroup's
// out-projection accumulators from the embedding output to the logits.  Normalisation is deferred into the kernel (no LayerNorm
// launch, no LN output tensor): the embedding writes raw rows, the kernel computes its own row statistics.  (The one-launch reverse
// loop, run_loop_fused, does not come here: it gathers the embedding itself.)
// The kernel's arguments from the loaded weights, for this launch and for the loop kernel's (ldm_loop.cpp): t < 0 = no AdaLN rows
StackWeights ldm_host::stack_weights(const ldm_handle* h, int t, float* logits) {
  StackWeights sw{};
  sw.ls.n_layer = h->L;
  for (int i = 0; i < h->L; ++i) {
    const LayerW& w = h->layers[i];
    const float* ss = t < 0 ? nullptr : h->adaln + ((size_t)t * h->L + i) * 2 * h->D;
    sw.ls.w[i] = FusedLayerW{h->fast[i].attn_head_img_ks, h->fast[i].b_in, ss, ss ? ss + h->D : nullptr, h->fast[i].b_out_v,
                             h->fast[i].ffn_img_pipe, w.b1, w.b2, w.g2, w.be2};
  }
  sw.head = StackHead{h->head_img_ks, h->head_g, h->head_b, logits, h->plan.Cp, h->plan.Cp / 32};
  sw.tables = StackTables{h->tbl_att_static, h->tbl_att_dyn, h->tbl_ffn, h->tbl_head};
  return sw;
}

static int denoise_chunk_stack(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, bool skip_embed) {
  const int M = Bc * h->plan.S, D = h->D, F = h->F;
  if (!skip_embed) {  // x0 = emb[token] + pos -> P (raw)   (skipped when the previous step's posterior wrote P)
    LnArgs a{};
    a.tokens = d_tokens; a.emb = h->emb; a.pos = h->pos; a.y32 = ws.P; a.stats_out = ws.stats_a; a.raw = 1;
    a.M = M; a.D = D; a.S = h->plan.S; a.ld16 = h->plan.Dq;
    ldm_handle::Scope sc(h, st, "embed_stats", 0, (double)M * D * 8);
    launch_layernorm(a, st);
  }
  const StackWeights sw = stack_weights(h, t, ws.logits);
  ldm_handle::Scope sc(h, st, "layers_fused",
                       h->L * (gemm_flops(M, 3 * D, D) + attention_flops(h, Bc) + gemm_flops(M, D, D) + 2 * gemm_flops(M, F, D)) +
                           gemm_flops(M, h->plan.C, D),
                       (double)M * (D * 4 + h->plan.Cp * 4));
  launch_stack_stream(sw.ls, F, ws.P, D, Bc, h->plan.S, h->H, h->plan.dh, sw.head, st);
  return 0;
}

// ------------------------------------------------------------------------------------------ fast, every other accepted geometry
// fp16 LDS-DMA GEMMs + MFMA attention on the head-padded layout
static int denoise_chunk_fast(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, const int32_t* d_t) {
  const int M = Bc * h->plan.S, D = h->D, F = h->F, C = h->plan.C, Dq = h->plan.Dq, HD = h->plan.HD, Fq = h->plan.Fq;
  auto gemm = [&](const char* name, int tag, const __half* A, int lda, int K, const __half* W, int ldw, int N,
                  const float* bias, int relu, const float* res, float* C32, int ldc32, __half* C16, int ldc16,
                  double flops, double bytes) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.relu = relu; g.res = res; g.ldres = D;
    g.C32 = C32; g.ldc32 = ldc32; g.C16 = C16; g.ldc16 = ldc16;
    g.M = M; g.N = N; g.K = round_up(K, kGemm16BK); g.lda = lda; g.ldw = ldw; g.precision = 1;
    ldm_handle::Scope sc(h, st, name, flops, bytes);
    launch_gemm16(g, tag, st);
  };
  for (int i = 0; i < h->L; ++i) {
    const LayerW& w = h->layers[i];
    const ldm_handle::FastLayer& f = h->fast[i];
    const float* ss = h->adaln + ((size_t)t * h->L + i) * 2 * D;
    layernorm(h, st, i == 0 ? "embed_adaln" : "adaln", M, ws.P, i == 0 ? d_tokens : nullptr, ss, ss + D, 1, ws.P, ws.a16, nullptr, Dq, d_t, i);
    gemm("gemm_qkv", 0, ws.a16, Dq, D, f.w_in, Dq, 3 * HD, f.b_in, 0, nullptr, nullptr, 0, ws.qkv16,
         3 * HD, gemm_flops(M, 3 * D, D), (double)M * (D * 2 + 3 * HD * 2));
    {
      ldm_handle::Scope sc(h, st, "attention", attention_flops(h, Bc), (double)M * (3 * HD + HD) * 2);
      launch_attention16(ws.qkv16, ws.att16, Bc, h->plan.S, h->H, h->plan.dh, 3 * HD, HD, st);
    }
    gemm("gemm_attn_out", 1, ws.att16, HD, HD, f.w_out, HD, D, w.b_out, 0, ws.P, ws.Q, D, nullptr, 0,
         gemm_flops(M, D, D), (double)M * (HD * 2 + D * 8));
    layernorm(h, st, "layernorm2", M, ws.Q, nullptr, w.g2, w.be2, 0, nullptr, ws.h16, nullptr, Dq);
    gemm("gemm_ffn1", 2, ws.h16, Dq, D, f.w1, Dq, F, w.b1, 1, nullptr, nullptr, 0, ws.hid16, Fq,
         gemm_flops(M, F, D), (double)M * (D * 2 + F * 2));
    gemm("gemm_ffn2", 3, ws.hid16, Fq, F, f.w2, Fq, D, w.b2, 0, ws.Q, ws.P, D, nullptr, 0,
         gemm_flops(M, D, F), (double)M * (F * 2 + D * 8));
  }
  layernorm(h, st, "layernorm_head", M, ws.P, nullptr, h->head_g, h->head_b, 0, nullptr, ws.h16, nullptr, Dq);
  gemm("gemm_head", 4, ws.h16, Dq, D, h->fast_head, Dq, h->plan.Cp, nullptr, 0, nullptr, ws.logits, h->plan.Cp,
       nullptr, 0, gemm_flops(M, C, D), (double)M * (D * 2 + C * 4));
  return 0;
}

// ------------------------------------------------------------------------------------------ tiled (exact; split without the row-resident kernels)
// Attention over qkv32 and the out-projection with the residual onto the normed x:  Q = P + att · Wo^T + bo.  The middle of a tiled
// block, and of a row-resident one under LDM_DEV=1 LDM_X3_ATTNOUT=0.
static int attention_out_proj(ldm_handle* h, Workspace& ws, const LayerW& w, int Bc, hipStream_t st) {
  const int M = Bc * h->plan.S, D = h->D;
  const bool split = h->plan.split_type();
  {
    AttnArgs a{};
    a.qkv = ws.qkv32;
    a.out32 = ws.att32; a.out16 = ws.att16; a.out16lo = ws.att16lo;   // (exact: fp32 out; split: hi / lo out)
    a.B = Bc; a.S = h->plan.S; a.H = h->H; a.dh = h->plan.dh; a.D = D; a.ld = 3 * D; a.ldo32 = D; a.ldo16 = h->plan.Dp;
    ldm_handle::Scope sc(h, st, "attention", attention_flops(h, Bc), (double)M * 3 * D * 4 + (double)M * D * (split ? 2 : 4));
    launch_attention(a, st);
  }
  return tiled_gemm(h, st, "gemm_attn_out", 1, M, D, D, h->plan.Dp, {ws.att32, ws.att16, ws.att16lo}, {w.w_out, w.w_out16, w.w_out16lo, w.s_out},
                    w.b_out, 0, ws.P, ws.Q, D);
}

// LayerNorm launch -> GEMM -> attention -> GEMM -> LayerNorm -> GEMM -> GEMM per block, then the head.  Every activation exists once, in
// the form of its mode (the Workspace members of the other form are nullptr, and so are the fp16 weight copies in the exact mode).
static int denoise_chunk_tiled(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, const int32_t* d_t) {
  const int M = Bc * h->plan.S, D = h->D, F = h->F, Dp = h->plan.Dp, Fp = h->plan.Fp;
  for (int i = 0; i < h->L; ++i) {
    const LayerW& w = h->layers[i];
    const float* ss = h->adaln + ((size_t)t * h->L + i) * 2 * D;
    // AdaLN (layer 0: fused with the embedding gather); P <- normed x (the residual base)
    layernorm(h, st, i == 0 ? "embed_adaln" : "adaln", M, ws.P, i == 0 ? d_tokens : nullptr, ss, ss + D, 1, ws.P, ws.a16, ws.a16lo, Dp, d_t, i);
    if (int rc = tiled_gemm(h, st, "gemm_qkv", 0, M, 3 * D, D, Dp, {ws.P, ws.a16, ws.a16lo}, {w.w_in, w.w_in16, w.w_in16lo, w.s_in}, w.b_in, 0,
                            nullptr, ws.qkv32, 3 * D))
      return rc;
    if (int rc = attention_out_proj(h, ws, w, Bc, st)) return rc;
    layernorm(h, st, "layernorm2", M, ws.Q, nullptr, w.g2, w.be2, 0, ws.h32, ws.h16, ws.h16lo, Dp);
    if (int rc = tiled_gemm(h, st, "gemm_ffn1", 2, M, F, D, Dp, {ws.h32, ws.h16, ws.h16lo}, {w.w1, w.w1_16, w.w1_16lo, w.s1}, w.b1, 1, nullptr,
                            ws.hid32, F, ws.hid16, ws.hid16lo, Fp))
      return rc;
    // FFN2 + residual:  P = Q + hid · W2^T + b2
    if (int rc = tiled_gemm(h, st, "gemm_ffn2", 3, M, D, F, Fp, {ws.hid32, ws.hid16, ws.hid16lo}, {w.w2, w.w2_16, w.w2_16lo, w.s2}, w.b2, 0, ws.Q,
                            ws.P, D))
      return rc;
  }
  // head: LayerNorm + vocabulary projection (no bias)
  layernorm(h, st, "layernorm_head", M, ws.P, nullptr, h->head_g, h->head_b, 0, ws.h32, ws.h16, ws.h16lo, Dp);
  return tiled_gemm(h, st, "gemm_head", 4, M, h->plan.C, D, Dp, {ws.h32, ws.h16, ws.h16lo}, {h->head_w, h->head_w16, h->head_w16lo, h->head_s}, nullptr,
                    0, nullptr, ws.logits, h->plan.Cp);
}

// ------------------------------------------------------------------------------------------ row-resident (split / mixed / hybrid on the reference's backbone)
// The LnGemmArgs of the row-resident launches, one builder per launch: denoise_chunk_row_resident below runs them on a lane's workspace, the
// development hook ldm_dev_lngemm_run (ldm_dev.cpp, tests/test_lngemm_gpu.py) on the caller's buffers — the same arguments but for the
// pointers `ws` holds and M.
// linear2 of layer `w` (+ bias + the residual Q) as the GEMM prologue of the launch that normalises its sum
static void ffn2_prologue(const ldm_handle* h, const Workspace& ws, const LayerW& w, LnGemmArgs& a) {
  a.preA = ws.hid16; a.preAlo = ws.hid16lo; a.pre_lda = h->plan.Fp; a.pre_astages = h->plan.Fp / 32; a.pre_stages = ldm_pack::x3_slab_stages(h->plan.Fp);
  a.pre_img = (const char*)w.x3_ffn2_slab; a.pre_bias = w.b2; a.pre_scale = w.s2;
  a.pre_res = ws.Q;
  a.pre_panel_stride = h->plan.hid_panels ? h->plan.panel_rows * 64 : 0;
  a.np_pre = h->plan.np_ffn;
  if (h->plan.np_ffn == 1) a.preAlo = nullptr;   // (plain-fp16 hidden activations: linear1 wrote no lo panels)
}

// AdaLN of layer i at timestep t (layer 0: fused with the embedding gather) + QKV projection; P <- normed x (the residual base).
// pre: x = Q + hid · W2^T + b2 of the PREVIOUS layer, computed in this launch (never stored)
LnGemmArgs ldm_host::lngemm_in_proj_args(const ldm_handle* h, const Workspace& ws, const int32_t* d_tokens, int t, int i, int M, bool pre,
                                         const int32_t* d_t) {
  const int D = h->D;
  const LayerW& w = h->layers[i];
  const float* ss = h->adaln + ((size_t)t * h->L + i) * 2 * D;
  LnGemmArgs a{};
  a.x = ws.P; a.ldx = D;
  a.tokens = (i == 0) ? d_tokens : nullptr;
  a.emb = h->emb; a.pos = h->pos; a.S = h->plan.S;
  a.p0 = ss; a.p1 = ss + D; a.ada = 1;
  if (d_t) { a.t_rows = d_t; a.ada_tab = h->adaln; a.t_stride = h->L * 2 * D; a.layer_off = i * 2 * D; }   // per-layout timesteps: p0 / p1 are not read
  a.y32 = ws.P;
  a.out_scale = w.s_in;
  a.M = M; a.D = D; a.np_main = h->plan.np_w;
  if (h->plan.attnout) {   // q / k / v as head-padded hi / lo panels for the fused attention + out_proj launch
    a.img = (const char*)w.x3_qkv_pad; a.n_tiles = 3 * h->H * 2;
    a.bias = w.b_in_pad; a.N = 3 * h->H * 64;
    a.C16 = ws.qkvp_hi; a.C16lo = ws.qkvp_lo; a.panel_out = 1; a.panel_stride = h->plan.panel_rows * 64;
  } else {
    a.img = (const char*)w.x3_qkv; a.n_tiles = h->plan.x3_qkv_tiles;
    a.bias = w.b_in; a.N = 3 * D;
    a.C32 = ws.qkv32; a.ldc32 = 3 * D;
  }
  if (pre) ffn2_prologue(h, ws, h->layers[i - 1], a);
  return a;
}

// LayerNorm 2 + FFN1 + ReLU of layer i: hi / lo hidden activations out
LnGemmArgs ldm_host::lngemm_linear1_args(const ldm_handle* h, const Workspace& ws, int i, int M) {
  const LayerW& w = h->layers[i];
  LnGemmArgs a{};
  a.x = ws.Q; a.ldx = h->D;
  a.p0 = w.g2; a.p1 = w.be2; a.ada = 0;
  a.img = (const char*)w.x3_ffn1; a.n_tiles = h->plan.x3_ffn1_tiles;
  a.bias = w.b1; a.out_scale = w.s1; a.relu = 1;
  a.C16 = ws.hid16; a.C16lo = ws.hid16lo; a.ldc16 = h->plan.Fp;
  if (h->plan.hid_panels) { a.panel_out = 1; a.panel_stride = h->plan.panel_rows * 64; }   // (read back by ffn2_prologue in the same form)
  a.M = M; a.N = h->F; a.D = h->D; a.S = h->plan.S; a.np_main = h->plan.np_ffn;
  if (h->plan.np_ffn == 1) a.C16lo = nullptr;   // hybrid: ReLU output rounded once (panel-major: plan_engine requires hid_panels for it)
  return a;
}

// head: LayerNorm + vocabulary projection (no bias); pre: behind the last layer's linear2
LnGemmArgs ldm_host::lngemm_head_args(const ldm_handle* h, const Workspace& ws, int M, bool pre) {
  LnGemmArgs a{};
  a.x = ws.P; a.ldx = h->D;
  a.p0 = h->head_g; a.p1 = h->head_b; a.ada = 0;
  a.img = (const char*)h->x3_head; a.n_tiles = h->plan.x3_head_tiles;
  a.out_scale = h->head_s;
  a.C32 = ws.logits; a.ldc32 = h->plan.Cp;
  a.np_main = h->plan.np_ffn;
  a.M = M; a.N = h->plan.Cp; a.D = h->D; a.S = h->plan.S;   // (columns C .. Cp of the image are zero rows: exact zeros in the padding)
  if (pre) ffn2_prologue(h, ws, h->layers[h->L - 1], a);
  return a;
}

// attention + out-proj + residual of layer i in ONE layout-resident launch:  Q = P + softmax(q k^T) v · Wo^T + bo
AttnOutArgs ldm_host::attnout_args(const ldm_handle* h, const Workspace& ws, int i) {
  const LayerW& w = h->layers[i];
  AttnOutArgs a{};
  a.qkv_hi = (const char*)ws.qkvp_hi; a.qkv_lo = (const char*)ws.qkvp_lo; a.panel_stride = h->plan.panel_rows * 64;
  a.w_img = (const char*)w.x3_out_kstep;
  a.res = ws.P; a.bias = w.b_out; a.out = ws.Q;
  a.S = h->plan.S; a.D = h->D; a.scale = 1.0f / sqrtf((float)h->plan.dh); a.out_scale = w.s_out; a.w2 = h->plan.w2p;
  if (h->plan.ffn_fused) {   // hybrid: the block's plain-fp16 FFN behind the attention in the same launch; P receives x + attention + FFN
    a.ffn_img = (const char*)w.ffn16_img; a.ffn_gamma = w.g2; a.ffn_beta = w.be2; a.ffn_b1 = w.b1; a.ffn_b2 = w.b2;
    a.ffn_out = ws.P; a.F = h->F; a.n_chunks = h->F / 32;
  }
  return a;
}

// The LayerNorm-fed GEMMs as ONE row-resident launch each (kernels_lngemm.hip), attention + out_proj as one layout-resident launch
// (kernels_attnout.hip).  linear2 has no launch of its own: it runs as the GEMM prologue of the next in_proj / of the head — or, in the
// hybrid mode (ffn_fused), the whole FFN runs behind the attention, two launches per block.
static int denoise_chunk_row_resident(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, const int32_t* d_t) {
  const int M = Bc * h->plan.S, D = h->D, F = h->F, C = h->plan.C;
  const bool pre_ffn2 = !h->plan.ffn_fused;
  for (int i = 0; i < h->L; ++i) {
    {
      const bool pre = pre_ffn2 && i > 0;
      const LnGemmArgs a = lngemm_in_proj_args(h, ws, d_tokens, t, i, M, pre, d_t);
      ldm_handle::Scope sc(h, st, pre ? "gemm_ffn2_qkv_ln" : "gemm_qkv_ln", gemm_flops(M, 3 * D, D) + (pre ? gemm_flops(M, D, F) : 0.0),
                           (double)M * D * 8 + (double)M * 3 * D * 4 + (pre ? (double)M * F * 4 : 0.0));
      if (launch_lngemm16x3(a, st)) return h->fail(-4, "row-resident LayerNorm + GEMM: geometry not supported");
    }
    if (h->plan.attnout) {
      const AttnOutArgs a = attnout_args(h, ws, i);
      ldm_handle::Scope sc(h, st, h->plan.ffn_fused ? "attn_out_ffn_fused" : "attn_out_fused",
                           attention_flops(h, Bc) + gemm_flops(M, D, D) + (h->plan.ffn_fused ? gemm_flops(M, F, D) + gemm_flops(M, D, F) : 0.0),
                           (double)M * 3 * h->H * 64 * 4 + (double)M * D * 8);
      if (launch_attnout16x3(a, Bc, st)) return h->fail(-4, "fused attention + out_proj: geometry not supported");
    } else if (int rc = attention_out_proj(h, ws, h->layers[i], Bc, st)) {   // (LDM_DEV=1 LDM_X3_ATTNOUT=0: in_proj wrote qkv32)
      return rc;
    }
    if (h->plan.ffn_fused) continue;   // (the FFN ran behind the attention)
    {
      const LnGemmArgs a = lngemm_linear1_args(h, ws, i, M);
      ldm_handle::Scope sc(h, st, "gemm_ffn1_ln", gemm_flops(M, F, D), (double)M * D * 4 + (double)M * F * 4);
      if (launch_lngemm16x3(a, st)) return h->fail(-4, "row-resident LayerNorm + GEMM: geometry not supported");
    }
  }
  const LnGemmArgs a = lngemm_head_args(h, ws, M, pre_ffn2);
  ldm_handle::Scope sc(h, st, pre_ffn2 ? "gemm_ffn2_head_ln" : "gemm_head_ln", gemm_flops(M, C, D) + (pre_ffn2 ? gemm_flops(M, D, F) : 0.0),
                       (double)M * D * 4 + (double)M * C * 4 + (pre_ffn2 ? (double)M * F * 4 : 0.0));
  if (launch_lngemm16x3(a, st)) return h->fail(-4, "row-resident LayerNorm + GEMM: geometry not supported");
  return 0;
}

// ------------------------------------------------------------------------------------------ one pass
// denoiser forward for `Bc` layouts whose tokens start at d_tokens -> ws.logits [Bc*S, Cp]   (skip_embed: the stack kernel's rows are
// already in ws.P — the previous step's posterior wrote them)
int ldm_host::denoise_chunk(ldm_handle* h, Workspace& ws, const int32_t* d_tokens, int t, int Bc, hipStream_t st, bool skip_embed,
                            const int32_t* d_t) {
  if (d_t && !h->plan.per_layout_t())   // the stack kernel's workgroups take ONE set of AdaLN rows per layer from its arguments
    return h->fail(-4, "per-layout timesteps: precision fast_f16 on the stack kernel has no per-layout form (ldm_describe per_layout_t=0)");
  switch (h->plan.structure) {
    case Structure::Stack: return denoise_chunk_stack(h, ws, d_tokens, t, Bc, st, skip_embed);
    case Structure::Generic16: return denoise_chunk_fast(h, ws, d_tokens, t, Bc, st, d_t);
    case Structure::Tiled: return denoise_chunk_tiled(h, ws, d_tokens, t, Bc, st, d_t);
    case Structure::RowResident: return denoise_chunk_row_resident(h, ws, d_tokens, t, Bc, st, d_t);
  }
  return h->fail(-4, "no engine");
}
