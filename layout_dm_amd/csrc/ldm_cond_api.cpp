// C-ABI of the cond= builder (include/ldm_hip.h, section "cond= inputs from raw layouts"): ldm_encode_cond,
// ldm_relation_graph and ldm_refinement_prior.  Handle-free like the metrics entry points: device pointers, sizes, a stream; every argument is checked
// before anything is launched.
#include "../../include/ldm_hip.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ldm_kernels.h"

#include "ldm_cond_core.h"
#include "ldm_refine_core.h"

using namespace ldm;

static bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

static bool layouts_ok(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int E) {
  if ((box_f64 != 0 && box_f64 != 1) || B < 0 || E < 1 || E > ldm_condb::kMaxElem) return false;
  if (B > 0 && (!d_bbox || !d_label || !d_mask || !aligned(d_bbox, box_f64 ? 32 : 16))) return false;
  return true;
}

extern "C" int ldm_encode_cond(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int E,
                               int n_category, int n_bin, int quant, const double* d_centres, int rule, const uint8_t* d_keep,
                               const float* d_noise, uint64_t seed, uint64_t first_layout, int32_t* d_seq,
                               uint8_t* d_cond_mask, int32_t* d_seq_orig, int32_t* d_num_element, float* d_noise_out,
                               int32_t* d_err, void* stream) {
  if (!layouts_ok(d_bbox, box_f64, d_label, d_mask, B, E) || !d_err) return -1;
  if (n_category < 1 || n_bin < 1 || n_bin > ldm_condb::kMaxBin || quant < 0 || quant > ldm_condb::kKMeans) return -1;
  if ((quant != ldm_condb::kLinear) != (d_centres != nullptr)) return -1;
  if (rule < 0 || rule >= ldm_condb::kNumRules) return -1;
  if ((int64_t)B * E * ldm_condb::kAttr > INT32_MAX) return -1;
  if (B > 0 && (!d_seq || !d_cond_mask)) return -1;
  if (B > 0 && rule == ldm_condb::kRuleRefinement && !d_seq_orig) return -1;
  if ((d_noise && !aligned(d_noise, 16)) || (d_noise_out && !aligned(d_noise_out, 16))) return -1;
  (void)hipGetLastError();
  if (hipMemsetAsync(d_err, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return -2;
  if (B == 0) return 0;
  const int pad_id = n_category + 4 * n_bin;
  CondEncodeArgs a{d_bbox, box_f64, d_label, d_mask, B, E, n_category, n_bin, quant, rule, pad_id, pad_id + 1, d_centres,
                   d_keep, d_noise, seed, first_layout, d_seq, d_cond_mask, d_seq_orig, d_num_element, d_noise_out, d_err};
  launch_encode_cond(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int ldm_relation_graph(const void* d_bbox, int box_f64, const int64_t* d_label, const uint8_t* d_mask, int B, int E,
                                  int n_category, const uint8_t* d_selection, double edge_ratio, uint64_t seed,
                                  uint64_t first_layout, int32_t* d_work, int32_t* d_edge_off, int32_t* d_src, int32_t* d_dst,
                                  int32_t* d_attr, int64_t* d_first_node, void* d_node_box, int64_t* d_node_label,
                                  int64_t* d_node_batch, uint8_t* d_canvas, int32_t* d_totals, int32_t* d_err, void* stream) {
  if (!layouts_ok(d_bbox, box_f64, d_label, d_mask, B, E) || B < 1 || n_category < 1 || !d_err) return -1;
  if (!(edge_ratio >= 0.0 && edge_ratio <= 1.0)) return -1;
  if (!d_work || !d_edge_off || !d_src || !d_dst || !d_attr || !d_first_node || !d_node_box || !d_node_label || !d_node_batch ||
      !d_canvas || !d_totals)
    return -1;
  if ((int64_t)B * (2 * ldm_condb::n_pairs(E + 1) + 1) > INT32_MAX) return -1;
  (void)hipGetLastError();
  if (hipMemsetAsync(d_err, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return -2;
  CondGraphArgs a{d_bbox, box_f64, d_label, d_mask, B, E, n_category, d_selection, edge_ratio, seed, first_layout, d_work,
                  d_edge_off, d_src, d_dst, d_attr, d_first_node, d_node_box, d_node_label, d_node_batch, d_canvas, d_totals,
                  d_err};
  launch_relation_graph(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int ldm_refinement_prior(const void* d_seq_orig, int seq_i64, int B_seq, int B, int S, int C, const float* d_table,
                                    float weight, float* d_out, int32_t* d_err, void* stream) {
  if (!ldm_refine::args_ok(seq_i64, B_seq, B, S, C)) return -1;
  if (B == 0) return 0;   // nothing to write, nothing launched
  if (!d_seq_orig || !d_table || !d_out || !d_err) return -1;
  if (!aligned(d_seq_orig, seq_i64 ? 8 : 4) || !aligned(d_table, 4) || ldm_refine::misalign_of(d_out) < 0) return -1;
  if ((int64_t)B * ldm_refine::chunks_per_layout(S, C) > INT32_MAX) return -1;   // (one workgroup per 16 KiB of output)
  (void)hipGetLastError();
  if (hipMemsetAsync(d_err, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return -2;
  launch_refinement_prior(d_seq_orig, seq_i64, B_seq, B, S, C, d_table, weight, d_out, d_err, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
