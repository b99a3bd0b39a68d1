// Host side of libldm_hip.so: the reference checkpoint -> device weights (ldm_load_weight / ldm_finalize_weights): fp32 views,
// fp16 / split copies, the LDS weight images and parameter tables of the layout-resident kernels (ldm_pack.h).
// ldm_weight_plan.h decides what the checkpoint is and how large every derived buffer is; here every image, padded copy and table is
// built on the host from the checkpoint's host copy (Raw::host) in one pass and uploaded once (upload): nothing that was uploaded is read
// back, and no intermediate of a packer lives on the device.  What the device builds stays with it: the tables (pos, AdaLN, the sinusoid)
// and the split mode's hi / lo cast, whose result comes to the host once where an image is packed from it (make_split16).
#include "ldm_handle.h"

using namespace ldm_host;

// ------------------------------------------------------------------------------------------ weights
static std::string strip_prefix(const char* key) {
  std::string k(key);
  for (const char* p : {"model.module.", "module.", "model."}) {
    const size_t n = strlen(p);
    if (k.compare(0, n, p) == 0) {
      k = k.substr(n);
      break;
    }
  }
  return k;
}

extern "C" int ldm_load_weight(ldm_handle* h, const char* key, const float* h_data, const int64_t* shape, int ndim) {
  if (!h || !key || !h_data || (ndim > 0 && !shape)) return h ? h->fail(-1, "null argument") : -1;
  ON_DEVICE(h);
  const std::string k = strip_prefix(key);
  Raw r;
  r.shape.assign(shape, shape + ndim);
  const int64_t n = r.numel();
  if (n <= 0) return h->fail(-1, "empty tensor for key %s", key);
  auto it = h->raw.find(k);
  if (it != h->raw.end()) {   // a reload keeps the device allocation and the storage of the host copy
    if (it->second.numel() != n) return h->fail(-1, "key %s reloaded with a different size", key);
    r.d = it->second.d;
  } else {
    HIP_OK(h, hipMalloc((void**)&r.d, n * sizeof(float)));
  }
  HIP_OK(h, hipMemcpy(r.d, h_data, n * sizeof(float), hipMemcpyHostToDevice));
  if (it != h->raw.end()) r.host.swap(it->second.host);
  if (ndim == 1 || h->plan.fast() || h->plan.ffn_fused) r.host.assign(h_data, h_data + n);   // (ldm_handle.h Raw: who builds from it)
  if (ndim == 2 && h->plan.split_type()) r.split_scale = split_scale(h_data, (size_t)n);
  h->raw[k] = std::move(r);
  h->finalized = false;
  h->step0.clear();  // (the step-0 logits tables are a function of the checkpoint)
  return 0;
}

// a tensor the plan has checked (ldm_weight_plan.h: present, of the configured shape)
static const Raw& tensor(const ldm_handle* h, const std::string& key) { return h->raw.find(key)->second; }
static const Raw& layer_tensor(const ldm_handle* h, int i, const char* name) {
  return tensor(h, "transformer.backbone.layers." + std::to_string(i) + "." + name);
}

// a synchronous copy between pageable host memory and the device, in 1-MiB slices (why: profiles/weights_refactor_parent_vs_change.txt section 3)
static hipError_t copy_sliced(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  constexpr size_t kSlice = 1 << 20;
  for (size_t off = 0; off < bytes; off += kSlice)
    if (hipError_t e = hipMemcpy((char*)dst + off, (const char*)src + off, std::min(kSlice, bytes - off), kind)) return e;
  return hipSuccess;
}

// The one way a derived buffer reaches the device: `v`, whose size must be the plan's `count` (several kernels load whole tiles without
// bounds checks), into a new allocation that h->derived owns
template <typename T, typename P>
static int upload(ldm_handle* h, const std::vector<T>& v, size_t count, P** out) {
  if (v.size() != count || !count) return h->fail(-2, "weight image of %zu elements where the plan counts %zu", v.size(), count);
  T* d = nullptr;
  if (int rc = h->dalloc(&d, count, false, &h->derived)) return rc;
  HIP_OK(h, copy_sliced(d, v.data(), count * sizeof(T), hipMemcpyHostToDevice));
  *out = reinterpret_cast<P*>(d);
  return 0;
}

// ---- index maps (ldm_pack.h — pure C++, unit-tested on the CPU by tests/cpu_pack_check.cpp)
static const auto id = [](int x) { return x; };
static const auto kslot = [](int k) { return ldm_pack::kslot(k); };
// in_proj row n = which*D + head*dh + d  ->  (which*H + head)*64 + d   (head slices padded to 64)
static auto qkv_row_of(const ldm_handle* h) {
  return [D = h->D, H = h->H, dh = h->plan.dh](int n) { return ldm_pack::qkv_row(n, D, H, dh); };
}
// out_proj column k = head*dh + d -> head*64 + d (matches the attention kernel's output layout)
static auto head_col_of(const ldm_handle* h) {
  return [dh = h->plan.dh](int k) { return ldm_pack::head_col(k, dh); };
}

// dst[Np][Kp] fp16 (zero filled) with dst[rmap(n)][cmap(k)] = src[n][k]
template <typename RM, typename CM>
static std::vector<uint16_t> pack16(const float* src, int N, int K, int Np, int Kp, RM rmap, CM cmap) {
  std::vector<uint16_t> dst((size_t)Np * Kp, 0);
  for (int n = 0; n < N; ++n) {
    const size_t ro = (size_t)rmap(n) * Kp;
    for (int k = 0; k < K; ++k) dst[ro + cmap(k)] = f16_bits(src[(size_t)n * K + k]);
  }
  return dst;
}

// split copies of a [N,K] weight: hi and lo [round_up(N, 256)][Kp] (`count` halves each), rows padded with zeros to whole 128-row tiles (the
// LDS-DMA GEMMs load W without bounds checks) and the K axis to Kp; *inv_scale = 2^-k of the tensor's pre-scale goes to the GEMM's epilogue.
// The scale was taken from the caller's data at load (Raw::split_scale); the cast itself stays with the device (cast_f32_f16 on the fp32 device
// copy): it is free there and 18 ms of a host thread per checkpoint (ldm_weight_plan.h split_f16 states it, tests/test_weight_plan.py pins
// that statement).  `host` (optional) receives the two copies back, once, for the image packers.
struct Split16 {
  std::vector<uint16_t> hi, lo;
};
struct LayerSplit16 {   // of one layer's four weights; one set serves every layer in turn
  Split16 in, out, l1, l2;
};
static int make_split16(ldm_handle* h, const Raw& w, int N, int K, int Kp, size_t count, __half** hi, __half** lo, float* inv_scale,
                        Split16* host = nullptr) {
  if (count < (size_t)N * Kp || K > Kp) return h->fail(-2, "split copy of %d x %d where the plan counts %zu halves", N, Kp, count);
  const float scale = w.split_scale;
  *inv_scale = 1.0f / scale;
  int rc;
  if ((rc = h->dalloc(hi, count, true, &h->derived)) || (rc = h->dalloc(lo, count, true, &h->derived))) return rc;
  if (K == Kp) {
    launch_f32_to_f16(w.d, *hi, *lo, (int64_t)N * K, 0, scale);
  } else {   // cast unpadded, then widen the rows
    struct Scratch {
      std::vector<void*> list;
      ~Scratch() {
        for (void* p : list) (void)hipFree(p);
      }
    } tmp;
    __half *thi = nullptr, *tlo = nullptr;
    if ((rc = h->dalloc(&thi, (size_t)N * K, false, &tmp.list)) || (rc = h->dalloc(&tlo, (size_t)N * K, false, &tmp.list))) return rc;
    launch_f32_to_f16(w.d, thi, tlo, (int64_t)N * K, 0, scale);
    HIP_OK(h, hipMemcpy2DAsync(*hi, (size_t)Kp * 2, thi, (size_t)K * 2, (size_t)K * 2, N, hipMemcpyDeviceToDevice, 0));
    HIP_OK(h, hipMemcpy2DAsync(*lo, (size_t)Kp * 2, tlo, (size_t)K * 2, (size_t)K * 2, N, hipMemcpyDeviceToDevice, 0));
    HIP_OK(h, hipStreamSynchronize(0));
  }
  if (host) {
    host->hi.resize(count);   // (the padding rows stay the zeros they start as)
    host->lo.resize(count);
    HIP_OK(h, copy_sliced(host->hi.data(), *hi, (size_t)N * Kp * 2, hipMemcpyDeviceToHost));
    HIP_OK(h, copy_sliced(host->lo.data(), *lo, (size_t)N * Kp * 2, hipMemcpyDeviceToHost));
  }
  return 0;
}

// hi | lo tile image of a split-mode weight for the row-resident x3 GEMM (kernels_lngemm.hip): the [>= 32 n_tiles][kX3K] hi / lo copies
// (natural K order) -> K axis in k-slot order -> ldm_pack::pack_x3_tile_image.  Image row rowmap(r) <- weight row r for the `rows` first
// rows, every other image row zero (the head-padded in_proj in front of kernels_attnout.hip: ldm_pack::qkv_row)
constexpr int kX3K = 512;   // K axis of the LDS tile images (ldm_pack.h: 1-KiB rows): plan.Dp of RowResident, plan.Dq of Stack — checked where they are built
template <typename RM>
static std::vector<uint16_t> x3_tile_image(const Split16& s, int n_tiles, int rows, RM rowmap) {
  std::vector<uint16_t> ak((size_t)n_tiles * 32 * kX3K, 0), bk(ak);
  for (int r = 0; r < rows; ++r) {
    const size_t d = (size_t)rowmap(r) * kX3K;
    for (int k = 0; k < kX3K; k += 4) {   // (the k-slot order moves aligned groups of four: kslot(k + j) = kslot(k) + j, j < 4)
      memcpy(&ak[d + ldm_pack::kslot(k)], &s.hi[(size_t)r * kX3K + k], 8);
      memcpy(&bk[d + ldm_pack::kslot(k)], &s.lo[(size_t)r * kX3K + k], 8);
    }
  }
  return ldm_pack::pack_x3_tile_image(ak.data(), bk.data(), n_tiles);
}

// FFN chunk image of the stack kernel and of the hybrid mode's fused FFN (kernels_attnout.hip): unscaled fp16 weights, K axes in MFMA k-slot
// order (position 16s + 8g + e <- index 16s + 8(e>>2) + 4g + (e&3): a lane's accumulator-layout registers of column groups 2ks, 2ks+1 ARE its
// fragment of k16-step ks), stage i = W1 tile i | W2 slab i - 1 (ldm_pack::pack_ffn_image_pipelined)
static std::vector<uint16_t> ffn_chunk_image(const float* w1, const float* w2, int D, int F) {
  const int Fq = round_up(F, 64);
  const std::vector<uint16_t> w1p = pack16(w1, F, D, round_up(F, 256), kX3K, id, kslot), w2p = pack16(w2, D, F, round_up(D, 256), Fq, id, kslot);
  return ldm_pack::pack_ffn_image_pipelined(ldm_pack::pack_ffn_image(w1p.data(), w2p.data(), Fq, F, 480), F / 32);
}

// in_proj bias with head-padded output columns [3 * H * 64]
static std::vector<float> padded_in_bias(const ldm_handle* h, const float* b) {
  std::vector<float> bp((size_t)3 * h->H * 64, 0.f);
  const auto qkv_row = qkv_row_of(h);
  for (int n = 0; n < 3 * h->D; ++n) bp[qkv_row(n)] = b[n];
  return bp;
}

// ---- fast-mode weights.  The stack kernel copies its weights global -> LDS with linear 1-KiB DMA instructions, so the global copy is stored
// in consumption order with the LDS bank swizzle already applied (ldm_pack.h).  b_in_pad / b_out_v: [L][3 HD] / [L][D], for the loop tables
static int build_fast_weights(ldm_handle* h, std::vector<float>& b_in_pad, std::vector<float>& b_out_v) {
  const int D = h->D, F = h->F, C = h->plan.C, H = h->H, HD = h->plan.HD, Dq = h->plan.Dq, Fq = h->plan.Fq;
  const WeightCounts& n = h->wplan.counts;
  const auto qkv_row = qkv_row_of(h);
  const auto head_col = head_col_of(h);
  const bool stack = h->plan.structure == Structure::Stack;
  if (stack && Dq != kX3K) return h->fail(-2, "the stack kernel's weight images need K padded to %d, the plan has %d", kX3K, Dq);
  const float* head_w = tensor(h, "transformer.head.1.weight").host.data();
  h->fast.assign(h->L, ldm_handle::FastLayer{});
  int rc;
  for (int i = 0; i < h->L; ++i) {
    ldm_handle::FastLayer& f = h->fast[i];
    const float *w_in = layer_tensor(h, i, "self_attn.in_proj_weight").host.data(), *w_out = layer_tensor(h, i, "self_attn.out_proj.weight").host.data(),
                *w1 = layer_tensor(h, i, "linear1.weight").host.data(), *w2 = layer_tensor(h, i, "linear2.weight").host.data(),
                *b = layer_tensor(h, i, "self_attn.in_proj_bias").host.data(), *bo = layer_tensor(h, i, "self_attn.out_proj.bias").host.data();
    if (!stack) {  // head-padded fp16 copies for the generic tiled GEMMs + attention16
      if ((rc = upload(h, pack16(w_in, 3 * D, D, round_up(3 * HD, 256), Dq, qkv_row, id), n.f_w_in, &f.w_in))) return rc;
      if ((rc = upload(h, pack16(w_out, D, D, round_up(D, 256), HD, id, head_col), n.f_w_out, &f.w_out))) return rc;
      if ((rc = upload(h, pack16(w1, F, D, round_up(F, 256), Dq, id, id), n.f_w1, &f.w1))) return rc;
      if ((rc = upload(h, pack16(w2, D, F, round_up(D, 256), Fq, id, id), n.f_w2, &f.w2))) return rc;
    } else {  // LDS images of the stack kernel, K axes in MFMA k-slot order
      if ((rc = upload(h, ffn_chunk_image(w1, w2, D, F), n.ffn_img_pipe, &f.ffn_img_pipe))) return rc;
      const std::vector<uint16_t> w_in_ks = pack16(w_in, 3 * D, D, round_up(3 * HD, 256), Dq, qkv_row, kslot),
                                  w_out_ks = pack16(w_out, D, D, round_up(D, 256), HD, id, [&](int k) { return kslot(head_col(k)); });
      const std::vector<uint16_t> slab_ks = ldm_pack::pack_attn_slab_image(w_in_ks.data(), w_out_ks.data(), H);
      if ((rc = upload(h, ldm_pack::pack_attn_head_image(slab_ks, H), n.attn_head_img_ks, &f.attn_head_img_ks))) return rc;
    }
    const std::vector<float> bp = padded_in_bias(h, b);
    if ((rc = upload(h, bp, n.f_b_in, &f.b_in))) return rc;
    b_in_pad.insert(b_in_pad.end(), bp.begin(), bp.end());
    if (stack) {
      // softmax rows sum to 1, so P (V + 1 b_v^T) = P V + 1 b_v^T and the V bias reaches the block output as the
      // constant W_out b_v: folded into the out-projection bias once, here (fp64 accumulate)
      std::vector<float> bov(D);
      for (int r = 0; r < D; ++r) {
        double acc = bo[r];
        for (int k = 0; k < D; ++k) acc += (double)w_out[(size_t)r * D + k] * (double)b[2 * D + k];
        bov[r] = (float)acc;
      }
      if ((rc = upload(h, bov, n.b_out_v, &f.b_out_v))) return rc;
      b_out_v.insert(b_out_v.end(), bov.begin(), bov.end());
    }
  }
  if (stack)
    return upload(h, ldm_pack::pack_head_image(pack16(head_w, C, D, round_up(C, 256), Dq, id, kslot).data(), h->plan.Cp / 32), n.head_img_ks,
                  &h->head_img_ks);
  return upload(h, pack16(head_w, C, D, round_up(C, 256), Dq, id, id), n.fast_head, &h->fast_head);
}

// Parameter tables of the loop kernel as LDS images (kernels_stack.hip HEAD == 2 copies them global -> LDS with the DMA,
// one phase ahead of their use, instead of 26 loads per thread behind a barrier at every layer entry):
//   att_static[l]      kStackTblAttStatic floats   head-padded in_proj bias
//   att_dyn[t][l]      kStackTblAttDyn floats      1 + AdaLN scale | AdaLN shift | b_out + W_out b_v + shift   (0 beyond d_model)
//   ffn[l]             kStackTblFfn floats         linear1 bias (0-padded to 2048) | norm2 gamma | norm2 beta | linear2 bias
//   head               kStackTblAttDyn floats      head LayerNorm gamma | beta | 0      (takes the att_dyn slot behind the last layer)
// Everything but the AdaLN rows, which the table kernels wrote on the device, comes from the host copies.
static int build_loop_tables(ldm_handle* h, const std::vector<float>& b_in_pad, const std::vector<float>& b_out_v) {
  const int D = h->D, F = h->F, L = h->L, T = h->T;
  const WeightCounts& n = h->wplan.counts;
  std::vector<float> ada(n.adaln);
  HIP_OK(h, hipDeviceSynchronize());  // (the AdaLN table kernels)
  HIP_OK(h, hipMemcpy(ada.data(), h->adaln, ada.size() * 4, hipMemcpyDeviceToHost));
  std::vector<float> att_dyn(n.tbl_att_dyn, 0.f), ffn(n.tbl_ffn, 0.f), head(n.tbl_head, 0.f);
  for (int l = 0; l < L; ++l) {
    const float* bov = &b_out_v[(size_t)l * D];
    for (int t = 0; t < T; ++t) {
      const float* ss = &ada[((size_t)t * L + l) * 2 * D];
      float* o = &att_dyn[((size_t)t * L + l) * kStackTblAttDyn];
      for (int i = 0; i < D; ++i) {
        o[i] = 1.0f + ss[i];           // multiplier (0 beyond d_model: padded columns come out as exact zeros)
        o[512 + i] = ss[D + i];        // shift
        o[1024 + i] = bov[i] + ss[D + i];
      }
    }
    float* f = &ffn[(size_t)l * kStackTblFfn];
    std::copy_n(layer_tensor(h, l, "linear1.bias").host.data(), F, f);
    std::copy_n(layer_tensor(h, l, "norm2.weight").host.data(), D, f + 2048);
    std::copy_n(layer_tensor(h, l, "norm2.bias").host.data(), D, f + 2048 + 512);
    std::copy_n(layer_tensor(h, l, "linear2.bias").host.data(), D, f + 2048 + 1024);
  }
  std::copy_n(tensor(h, "transformer.head.0.weight").host.data(), D, head.begin());
  std::copy_n(tensor(h, "transformer.head.0.bias").host.data(), D, head.begin() + 512);
  int rc;
  if ((rc = upload(h, b_in_pad, n.tbl_att_static, &h->tbl_att_static))) return rc;   // (H * 64 * 3 == kStackTblAttStatic: the padded biases ARE the table)
  if ((rc = upload(h, att_dyn, n.tbl_att_dyn, &h->tbl_att_dyn))) return rc;
  if ((rc = upload(h, ffn, n.tbl_ffn, &h->tbl_ffn))) return rc;
  return upload(h, head, n.tbl_head, &h->tbl_head);
}

// the split-type copies and images of layer i (kernels_gemm16.hip, kernels_lngemm.hip, kernels_attnout.hip)
static int build_split_layer(ldm_handle* h, int i, LayerSplit16& s) {
  const int D = h->D, F = h->F, H = h->H, Dp = h->plan.Dp, Fp = h->plan.Fp;
  const WeightCounts& n = h->wplan.counts;
  const bool row_resident = h->plan.structure == Structure::RowResident;
  LayerW& w = h->layers[i];
  const Raw &w1 = layer_tensor(h, i, "linear1.weight"), &w2 = layer_tensor(h, i, "linear2.weight");
  Split16 &in = s.in, &out = s.out, &l1 = s.l1, &l2 = s.l2;   // the copies back on the host, where an image is packed from them
  int rc;
  if (row_resident && Dp != kX3K) return h->fail(-2, "row-resident weight images need K padded to %d, the plan has %d", kX3K, Dp);
  if ((rc = make_split16(h, layer_tensor(h, i, "self_attn.in_proj_weight"), 3 * D, D, Dp, n.w_in16, &w.w_in16, &w.w_in16lo, &w.s_in, row_resident ? &in : nullptr))) return rc;
  if ((rc = make_split16(h, layer_tensor(h, i, "self_attn.out_proj.weight"), D, D, Dp, n.w_out16, &w.w_out16, &w.w_out16lo, &w.s_out, h->plan.attnout ? &out : nullptr))) return rc;
  if ((rc = make_split16(h, w1, F, D, Dp, n.w1_16, &w.w1_16, &w.w1_16lo, &w.s1, row_resident ? &l1 : nullptr))) return rc;
  if ((rc = make_split16(h, w2, D, F, Fp, n.w2_16, &w.w2_16, &w.w2_16lo, &w.s2, row_resident ? &l2 : nullptr))) return rc;
  if (row_resident) {
    if ((rc = upload(h, x3_tile_image(in, h->plan.x3_qkv_tiles, h->plan.x3_qkv_tiles * 32, id), n.x3_qkv, &w.x3_qkv))) return rc;
    if ((rc = upload(h, x3_tile_image(l1, h->plan.x3_ffn1_tiles, h->plan.x3_ffn1_tiles * 32, id), n.x3_ffn1, &w.x3_ffn1))) return rc;
    // K-slab image of linear2 for the GEMM prologue of kernels_lngemm.hip
    if ((rc = upload(h, ldm_pack::pack_x3_slab_image(l2.hi.data(), l2.lo.data(), D, Fp, Fp), n.x3_ffn2_slab, &w.x3_ffn2_slab))) return rc;
  }
  if (h->plan.attnout) {   // in_proj with head-padded output columns (+ bias), out_proj as per-(head, k16-step) stages
    if ((rc = upload(h, x3_tile_image(in, 3 * H * 2, 3 * D, qkv_row_of(h)), n.x3_qkv_pad, &w.x3_qkv_pad))) return rc;
    if ((rc = upload(h, padded_in_bias(h, layer_tensor(h, i, "self_attn.in_proj_bias").host.data()), n.b_in_pad, &w.b_in_pad))) return rc;
    if ((rc = upload(h, ldm_pack::pack_x3_kstep_image(out.hi.data(), out.lo.data(), D, Dp, H, h->plan.dh), n.x3_out_kstep, &w.x3_out_kstep))) return rc;
  }
  // hybrid: the FFN in plain fp16 behind the attention (kernels_attnout.hip) on the fast mode's chunk image
  if (h->plan.ffn_fused && (rc = upload(h, ffn_chunk_image(w1.host.data(), w2.host.data(), D, F), n.ffn16_img, &w.ffn16_img))) return rc;
  return 0;
}

// plan (refuse) -> drop the old derived set -> build -> upload -> finalized
extern "C" int ldm_finalize_weights(ldm_handle* h) {
  if (!h) return -1;
  ON_DEVICE(h);
  const int D = h->D, C = h->plan.C, T = h->T, L = h->L;
  KeyShapes keys;
  for (const auto& kv : h->raw) keys[kv.first] = kv.second.shape;
  std::string why;
  WeightPlan planned;   // (a refused checkpoint leaves the handle's plan, and what ldm_describe says, as they were)
  if (int rc = plan_weights(h->cfg, h->plan, keys, planned, why)) return h->fail(rc, "%s", why.c_str());
  h->wplan = std::move(planned);
  const WeightCounts& n = h->wplan.counts;
  const bool none = h->wplan.timestep_kind == kTimestepNone, learned = h->wplan.timestep_kind == kTimestepLearned;
  const std::string tr = "transformer.";
  int rc;
  if (!h->pos && (rc = h->dalloc(&h->pos, n.pos))) return rc;
  if (!h->adaln && (rc = h->dalloc(&h->adaln, n.adaln))) return rc;
  // everything below is derived from the checkpoint: drop what an earlier finalize built (nothing may still be running on it),
  // then collect the new allocations in h->derived
  HIP_OK(h, hipDeviceSynchronize());
  h->finalized = false;   // (a finalize that fails part-way must not leave an earlier success standing over freed images)
  h->graphs.drop_all();
  h->step0.clear();  // the step-0 logits tables of the loop kernel belong to the weights that are being replaced
  for (void* p : h->derived) (void)hipFree(p);
  h->derived.clear();
  h->fast.clear();
  h->fast_head = nullptr;
  h->head_img_ks = nullptr;
  h->head_w16 = h->head_w16lo = nullptr;
  h->x3_head = nullptr;
  h->tbl_att_static = h->tbl_att_dyn = h->tbl_ffn = h->tbl_head = nullptr;
  h->emb = tensor(h, tr + "cat_emb.weight").d;
  h->head_g = tensor(h, tr + "head.0.weight").d;
  h->head_b = tensor(h, tr + "head.0.bias").d;
  h->head_w = tensor(h, tr + "head.1.weight").d;
  // ---- tables the device builds: positions, the sinusoid of the *_abs kinds (once for all layers), AdaLN rows
  if (h->wplan.pos_default)
    HIP_OK(h, hipMemcpyAsync(h->pos, tensor(h, tr + "pos_emb.pos_emb").d, n.pos * sizeof(float), hipMemcpyDeviceToDevice, 0));
  else
    launch_pos_table(tensor(h, tr + "pos_emb.elem_emb").d, tensor(h, tr + "pos_emb.attr_emb").d, h->pos, h->cfg.max_elem, h->cfg.n_attr, D, 0);
  float* sinus = nullptr;
  if (n.sinus) {
    if ((rc = h->dalloc(&sinus, n.sinus, true, &h->derived))) return rc;
    launch_sinus_table(sinus, T, D, 0);
  }
  h->layers.assign(L, LayerW{});
  LayerSplit16 split_host;
  for (int i = 0; i < L; ++i) {
    LayerW& w = h->layers[i];
    w.w_in = layer_tensor(h, i, "self_attn.in_proj_weight").d;
    w.b_in = layer_tensor(h, i, "self_attn.in_proj_bias").d;
    w.w_out = layer_tensor(h, i, "self_attn.out_proj.weight").d;
    w.b_out = layer_tensor(h, i, "self_attn.out_proj.bias").d;
    w.w1 = layer_tensor(h, i, "linear1.weight").d;
    w.b1 = layer_tensor(h, i, "linear1.bias").d;
    w.w2 = layer_tensor(h, i, "linear2.weight").d;
    w.b2 = layer_tensor(h, i, "linear2.bias").d;
    w.g2 = layer_tensor(h, i, "norm2.weight").d;
    w.be2 = layer_tensor(h, i, "norm2.bias").d;
    if (none)
      launch_adaln_const_table(layer_tensor(h, i, "norm1.weight").d, layer_tensor(h, i, "norm1.bias").d, h->adaln, T, D, L, i, 0);
    else
      launch_adaln_table(learned ? layer_tensor(h, i, "norm1.emb.weight").d : sinus, layer_tensor(h, i, "norm1.linear.weight").d,
                         layer_tensor(h, i, "norm1.linear.bias").d, h->adaln, T, D, L, i, 0);
    if (h->plan.split_type() && (rc = build_split_layer(h, i, split_host))) return rc;
  }
  if (h->plan.fast()) {
    std::vector<float> b_in_pad, b_out_v;
    if ((rc = build_fast_weights(h, b_in_pad, b_out_v))) return rc;
    if (h->wplan.loop_tables() && (rc = build_loop_tables(h, b_in_pad, b_out_v))) return rc;
  } else if (h->plan.split_type()) {
    Split16 head;
    if ((rc = make_split16(h, tensor(h, tr + "head.1.weight"), C, D, h->plan.Dp, n.head_w16, &h->head_w16, &h->head_w16lo, &h->head_s, n.x3_head ? &head : nullptr))) return rc;
    if (n.x3_head && (rc = upload(h, x3_tile_image(head, h->plan.x3_head_tiles, h->plan.x3_head_tiles * 32, id), n.x3_head, &h->x3_head))) return rc;
  }
  // schedule buffers are taken from the checkpoint, not recomputed
  std::vector<float> sched(n.sched, 0.f);
  if (n.sched != h->plan.bufs.sched) return h->fail(-2, "schedule buffer of %zu floats where the handle holds %zu", n.sched, h->plan.bufs.sched);
  for (int k = 0; k < kNumSched; ++k)
    for (int a = 0; a < h->cfg.n_attr; ++a) {
      const std::vector<float>& row = tensor(h, sched_key(h->cfg, k, a)).host;
      std::copy(row.begin(), row.end(), sched.begin() + ((size_t)k * h->cfg.n_attr + a) * (T + 1));
    }
  HIP_OK(h, hipMemcpy(h->sched, sched.data(), sched.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(h, hipDeviceSynchronize());
  HIP_OK(h, hipGetLastError());
  // graphs captured against older weights stay valid (pointers unchanged) but drop them anyway
  h->graphs.drop_all();
  h->finalized = true;
  return 0;
}
