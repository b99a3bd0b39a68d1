// cond= inputs from raw layouts on the device: tokenizer.encode + get_cond (encode_cond_k) and the relation graph of
// AddCanvasElement + AddRelationConstraints (relation_graph_k, relation_scan_k, relation_fill_k).  The arithmetic is the one
// source of ldm_cond_core.h (also compiled for the host: tests/cpu_cond_check.cpp).
//
// encode_cond_k: one lane per element slot, 256 / E consecutive layouts per workgroup.  A lane reads its box as one 16- or
// 32-byte vector, runs encode and the cond rule, and parks its 5 tokens in LDS; the workgroup then writes its layouts' seq /
// mask / seq_orig rows — one contiguous range of the (B, 5E) arrays — with consecutive lanes on consecutive words.  Cluster
// centres sit in LDS.  Own draws (partial keep, refinement noise) come from Philox keyed by the global layout index.
//
// relation_graph_k: one wavefront per layout.  The node boxes (canvas first) and, for own draws, one Philox score per
// (kind, pair) candidate go to the wavefront's LDS; a candidate is selected when fewer than `size` candidates beat its
// (score, index) — a uniform subset of exactly int(2 P edge_ratio) candidates.  The lanes then walk the P <= 528 pairs in
// combinations order 64 at a time, and a ballot + popcount prefix packs the surviving edges in that order into the layout's
// slice of an upper-bound workspace.  relation_scan_k turns the per-layout counts into CSR offsets / first node ids / totals
// (one workgroup), relation_fill_k copies edges and node rows to their final places.  No host sync in here.
#include <cmath>

#include "ldm_kernels.h"

#include "ldm_cond_core.h"

namespace ldm {

namespace {

using namespace ldm_condb;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxNodes = kMaxElem + 1;
constexpr int kMaxPairs = kMaxNodes * (kMaxNodes - 1) / 2;   // 528
constexpr int kMaxCand = 2 * kMaxPairs;                       // 1056
constexpr int kCandPerLane = (kMaxCand + 63) / 64;            // 17

template <typename TB> struct Vec4;
template <> struct Vec4<float> { using type = float4; };
template <> struct Vec4<double> { using type = double4; };

template <typename TB>
__global__ __launch_bounds__(kBlock) void encode_cond_k(CondEncodeArgs a) {
  __shared__ double s_centres[4 * kMaxBin];
  __shared__ int32_t s_seq[kBlock * kAttr];
  __shared__ int32_t s_orig[kBlock * kAttr];
  __shared__ uint8_t s_mask[kBlock * kAttr];
  const int t = threadIdx.x;
  const int E = a.E, per = kBlock / E;                  // layouts per workgroup
  const int b0 = blockIdx.x * per;
  const int nb = min(per, a.B - b0);                    // >= 1 by the grid size
  Geometry g{a.n_category, a.n_bin, a.quant, a.pad_id, a.mask_id, s_centres};
  if (a.quant != kLinear) {
    for (int i = t; i < 4 * a.n_bin; i += kBlock) s_centres[i] = a.centres[i];
    __syncthreads();
  }
  const int lb = t / E, e = t - lb * E;
  if (lb < nb) {
    const int b = b0 + lb;
    const size_t slot = (size_t)b * E + e;
    const uint8_t* m = a.mask + (size_t)b * E;
    const bool valid = m[e] != 0;
    int n = 0, err = 0;
    for (int o = 0; o < E; ++o) n += m[o] != 0;
    if (e > 0 && valid && !m[e - 1]) err |= kErrPrefix;
    const uint64_t layout = a.first_layout + (uint64_t)b;
    const typename Vec4<TB>::type v = reinterpret_cast<const typename Vec4<TB>::type*>(a.bbox)[slot];
    TB box[4] = {v.x, v.y, v.z, v.w};
    if (a.rule == kRuleRefinement) {
      float z[4];
      if (a.noise) {
        const float4 nz = reinterpret_cast<const float4*>(a.noise)[slot];
        z[0] = nz.x, z[1] = nz.y, z[2] = nz.z, z[3] = nz.w;
      } else {
        noise4(a.seed, layout, e, z);
      }
      if (a.noise_out) reinterpret_cast<float4*>(a.noise_out)[slot] = make_float4(z[0], z[1], z[2], z[3]);
      for (int k = 0; k < 4; ++k) box[k] = box[k] + TB(z[k]);
    }
    int32_t tok[kAttr], seq[kAttr], orig[kAttr];
    uint8_t cm[kAttr];
    err |= encode_element(g, box, a.label[slot], valid, tok);
    bool kept = false;
    if (a.rule == kRulePartial)
      kept = a.keep ? a.keep[slot] != 0 : (valid && partial_keep(a.seed, layout, m, E, e, partial_count(a.seed, layout, n)));
    apply_rule(g, a.rule, tok, valid, kept, seq, cm, orig);
#pragma unroll
    for (int k = 0; k < kAttr; ++k) {
      s_seq[t * kAttr + k] = seq[k];
      s_mask[t * kAttr + k] = cm[k];
      if (a.rule == kRuleRefinement) s_orig[t * kAttr + k] = orig[k];
    }
    if (e == 0 && a.num_element) a.num_element[b] = n;
    if (err) atomicOr(a.err, err);
  }
  __syncthreads();
  // lanes lb * E + e are dense in t for the workgroup's layouts: its tokens are words [0, nb * 5E) of LDS and of the row range
  const int words = nb * E * kAttr;
  const size_t base = (size_t)b0 * E * kAttr;
  for (int i = t; i < words; i += kBlock) {
    a.seq[base + i] = s_seq[i];
    a.cond_mask[base + i] = s_mask[i];
    if (a.rule == kRuleRefinement && a.seq_orig) a.seq_orig[base + i] = s_orig[i];
  }
}

// ---- relation graph -----------------------------------------------------------------------------------------------------
template <typename TB>
__global__ __launch_bounds__(kBlock) void relation_graph_k(CondGraphArgs a) {
  __shared__ TB s_box[kWaves][kMaxNodes * 4];
  __shared__ uint32_t s_score[kWaves][kMaxCand];
  __shared__ uint8_t s_sel[kWaves][kMaxCand];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * kWaves + w;                // uniform within a wavefront
  if (b >= a.B) return;
  const int E = a.E, Pmax = n_pairs(E + 1);
  const uint8_t* m = a.mask + (size_t)b * E;
  int n = 0, err = 0;
  for (int o = 0; o < E; ++o) {
    n += m[o] != 0;
    if (o > 0 && m[o] && !m[o - 1]) err |= kErrPrefix;
  }
  const int N = n + 1, P = n_pairs(N);
  TB* box = s_box[w];
  if (lane < 4) box[lane] = lane < 2 ? TB(0.5) : TB(1);   // AddCanvasElement.x
  for (int i = lane; i < 4 * n; i += 64) {
    const TB v = static_cast<const TB*>(a.bbox)[(size_t)b * E * 4 + i];
    if (!finite(v)) err |= kErrNonFinite;
    box[4 + i] = v;
  }
  for (int o = lane; o < n; o += 64) {
    const int64_t l = a.label[(size_t)b * E + o];
    if (l < 0 || l >= a.n_category) err |= kErrLabel;
  }
  uint8_t* sel = s_sel[w];
  if (a.selection) {   // (B, 2, E+1, E+1): [kind][i][j]
    const uint8_t* s = a.selection + (size_t)b * 2 * (E + 1) * (E + 1);
    for (int c = lane; c < 2 * P; c += 64) {
      int i, j;
      pair_of(N, c >= P ? c - P : c, i, j);
      sel[c] = s[((c >= P ? 1 : 0) * (E + 1) + i) * (E + 1) + j] != 0;
    }
  } else {
    const uint64_t layout = a.first_layout + (uint64_t)b;
    const int size = relation_sample_size(N, a.edge_ratio);
    uint32_t* score = s_score[w];
    for (int q = lane; 4 * q < 2 * P; q += 64) {
      uint32_t r[4];
      draw4(a.seed, layout, kDrawRelation, (uint32_t)q, r);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * q + k < 2 * P) score[4 * q + k] = r[k];
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    uint32_t mine[kCandPerLane];
    int ahead[kCandPerLane];
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      const int c = lane + 64 * k;
      mine[k] = c < 2 * P ? score[c] : 0u;
      ahead[k] = 0;
    }
    for (int o = 0; o < 2 * P; ++o) {
      const uint32_t s = score[o];   // one address for the wavefront: a broadcast read
#pragma unroll
      for (int k = 0; k < kCandPerLane; ++k) ahead[k] += s < mine[k] || (s == mine[k] && o < lane + 64 * k);
    }
#pragma unroll
    for (int k = 0; k < kCandPerLane; ++k) {
      const int c = lane + 64 * k;
      if (c < 2 * P) sel[c] = ahead[k] < size;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  int32_t* work = a.work + (size_t)b * (2 * Pmax + 1);
  int count = 0;
  for (int p0 = 0; p0 < P; p0 += 64) {   // uniform trip count: the ballot sees the whole wavefront
    const int p = p0 + lane;
    int attr = kRelUnknown, i = 0, j = 0;
    if (p < P) {
      pair_of(N, p, i, j);
      attr = pair_attr(box + 4 * i, box + 4 * j, i == 0, sel[p] != 0, sel[P + p] != 0);
    }
    const bool edge = attr != kRelUnknown;
    const unsigned long long vote = __ballot(edge);
    if (edge) {
      const int at = count + __popcll(vote & ((1ull << lane) - 1ull));
      work[1 + at] = attr;
      work[1 + Pmax + at] = (i << 8) | j;
    }
    count += __popcll(vote);
  }
  for (int o = 32; o > 0; o >>= 1) err |= __shfl_xor(err, o, 64);
  if (lane == 0) {
    work[0] = count;
    if (err) atomicOr(a.err, err);
  }
}

// edge_off[b] / first_node[b] = exclusive scans of the edge counts / of 1 + the element counts; totals = {edges, nodes}.
// One workgroup; thread t owns a contiguous chunk of layouts, the chunk sums are scanned in LDS.
__global__ __launch_bounds__(kBlock) void relation_scan_k(CondGraphArgs a) {
  __shared__ int32_t s_e[kBlock], s_n[kBlock];
  const int t = threadIdx.x, E = a.E;
  const size_t stride = 2 * (size_t)n_pairs(E + 1) + 1;
  const int chunk = (a.B + kBlock - 1) / kBlock;
  const int b0 = min(t * chunk, a.B), b1 = min(b0 + chunk, a.B);
  int32_t se = 0, sn = 0;
  for (int b = b0; b < b1; ++b) {
    se += a.work[b * stride];
    sn += 1;
    for (int o = 0; o < E; ++o) sn += a.mask[(size_t)b * E + o] != 0;
  }
  s_e[t] = se, s_n[t] = sn;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const int32_t ae = t >= o ? s_e[t - o] : 0, an = t >= o ? s_n[t - o] : 0;
    __syncthreads();
    s_e[t] += ae, s_n[t] += an;
    __syncthreads();
  }
  int32_t re = s_e[t] - se, rn = s_n[t] - sn;
  for (int b = b0; b < b1; ++b) {
    a.edge_off[b] = re;
    a.first_node[b] = rn;
    re += a.work[b * stride];
    rn += 1;
    for (int o = 0; o < E; ++o) rn += a.mask[(size_t)b * E + o] != 0;
  }
  if (t == kBlock - 1) {
    a.edge_off[a.B] = s_e[t];
    a.totals[0] = s_e[t];
    a.totals[1] = s_n[t];
  }
}

// one wavefront per layout: its edges to [edge_off[b], edge_off[b+1]), its node rows to [first_node[b], ...)
template <typename TB>
__global__ __launch_bounds__(kBlock) void relation_fill_k(CondGraphArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int E = a.E, Pmax = n_pairs(E + 1);
  const int32_t* work = a.work + (size_t)b * (2 * Pmax + 1);
  const int e0 = a.edge_off[b], count = min(work[0], Pmax);
  for (int k = lane; k < count; k += 64) {
    const int ij = work[1 + Pmax + k];
    a.src[e0 + k] = ij >> 8;
    a.dst[e0 + k] = ij & 255;
    a.attr[e0 + k] = work[1 + k];
  }
  const int64_t r0 = a.first_node[b];
  int n = 0;
  for (int o = 0; o < E; ++o) n += a.mask[(size_t)b * E + o] != 0;
  TB* x = static_cast<TB*>(a.node_box);
  for (int k = lane; k <= n; k += 64) {   // node 0 = the canvas, label 0; element labels + 1
    a.node_label[r0 + k] = k == 0 ? 0 : a.label[(size_t)b * E + k - 1] + 1;
    a.node_batch[r0 + k] = b;
    a.canvas[r0 + k] = k == 0;
  }
  for (int i = lane; i < 4 * (n + 1); i += 64)
    x[4 * r0 + i] = i < 4 ? (i < 2 ? TB(0.5) : TB(1)) : static_cast<const TB*>(a.bbox)[(size_t)b * E * 4 + i - 4];
}

}  // namespace

void launch_encode_cond(const CondEncodeArgs& a, hipStream_t st) {
  const int per = kBlock / a.E;
  const unsigned grid = (unsigned)((a.B + per - 1) / per);
  if (a.box_f64) hipLaunchKernelGGL(encode_cond_k<double>, dim3(grid), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(encode_cond_k<float>, dim3(grid), dim3(kBlock), 0, st, a);
}

void launch_relation_graph(const CondGraphArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)((a.B + kWaves - 1) / kWaves);
  if (a.box_f64) hipLaunchKernelGGL(relation_graph_k<double>, dim3(grid), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(relation_graph_k<float>, dim3(grid), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(relation_scan_k, dim3(1), dim3(kBlock), 0, st, a);
  if (a.box_f64) hipLaunchKernelGGL(relation_fill_k<double>, dim3(grid), dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(relation_fill_k<float>, dim3(grid), dim3(kBlock), 0, st, a);
}

}  // namespace ldm
