// The refinement prior — cond["weak_logits"] of set_additional_conditions_for_refinement (trainer/helpers/task.py:154-224):
//   out[b][c][s] = table[tok(b', s) * C + c] * weight      (one float32 multiply, the sign of zero included)
// with table the (C, C) [token][class] table of _index_to_smoothed_log_onehot before the refine_lambda weight, tok the
// tokens of cond["seq_orig"], and b' = b (B_seq == B) or 0 (B_seq == 1: duplicate_cond, one conditioning layout for B samples).
// ONE source of the index, bounds and broadcast arithmetic, compiled for the device (kernels_refine.hip) and for the host
// (tests/cpu_refine_check.cpp).
//
// Work decomposition.  A layout's C * S floats are one contiguous slab of the output; the kernel is bound by its stores, so
// they are 16-byte stores wherever the slab allows.  C * S may be odd and d_out need only be 4-byte aligned (a slice of a
// larger buffer), so a slab does not start on a 16-byte boundary in general.  With mis = floats of d_out past the last
// 16-byte boundary, the float at slab index i of layout b sits at "flat" index f = mis + b * C * S + i, and f % 4 == 0 is a
// 16-byte boundary.  Layout b's window starts at its slab's flat start rounded DOWN to a multiple of 4 and is cut into chunks
// of kChunk floats, one workgroup each; thread tid owns the groups of 4 floats at window offsets (it * kBlock + tid) * 4.  A
// group that lies wholly inside the slab is one 16-byte store; a group that straddles the slab's first or last float stores
// its inside floats one by one; nothing outside [0, C * S) of the slab is ever touched.
//
// A token outside [0, C) (F.embedding raises there) sets kErrToken and yields +0.0 without a table read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LDM_RF_HD __host__ __device__ __forceinline__
#else
#define LDM_RF_HD inline
#endif
#if defined(__clang__)
#define LDM_RF_UNROLL _Pragma("unroll")
#else
#define LDM_RF_UNROLL
#endif

namespace ldm_refine {

constexpr int kBlock = 256;                      // threads of a workgroup
constexpr int kVec = 4;                          // floats of a 16-byte store
constexpr int kIter = 4;                         // groups per thread
constexpr int kChunk = kBlock * kVec * kIter;    // floats of a workgroup's piece of the window
constexpr int kMaxStaged = 1024;                 // longest sequence whose tokens a workgroup holds in LDS; longer: read in place

enum : int { kErrToken = 1 };  // bits of the error word

LDM_RF_HD bool args_ok(int seq_i64, int B_seq, int B, int S, int C) {
  return (seq_i64 == 0 || seq_i64 == 1) && B >= 0 && S >= 1 && C >= 1 && (B_seq == B || B_seq == 1);
}

// floats of `out` past the last 16-byte boundary; -1 if out is not a float address at all
LDM_RF_HD int misalign_of(const void* out) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(out);
  return (a & 3u) ? -1 : (int)((a >> 2) & 3u);
}

LDM_RF_HD int64_t slab_size(int S, int C) { return (int64_t)C * (int64_t)S; }

// workgroups per layout: the window is the slab plus the <= 3 floats in front of it
LDM_RF_HD int64_t chunks_per_layout(int S, int C) { return (slab_size(S, C) + (kVec - 1) + (kChunk - 1)) / kChunk; }

// row of seq_orig that layout b reads
LDM_RF_HD int64_t seq_row(int64_t b, int B_seq) { return B_seq == 1 ? 0 : b; }

// token idx of the (B_seq, S) array, int64 (the reference's dtype) or int32
LDM_RF_HD int64_t load_token(const void* seq, int seq_i64, int64_t idx) {
  return seq_i64 ? static_cast<const int64_t*>(seq)[idx] : (int64_t) static_cast<const int32_t*>(seq)[idx];
}

// the token as the table row it selects, or -1
LDM_RF_HD int32_t checked_token(int64_t t, int C) { return (uint64_t)t < (uint64_t)C ? (int32_t)t : -1; }

// slab index of the first float of window offset `off` of layout b (may be -3 .. -1 in front of the slab)
LDM_RF_HD int64_t slab_index(int mis, int64_t b, int64_t CS, int64_t off) {
  const int64_t g0 = (int64_t)mis + b * CS;
  return (g0 & ~(int64_t)(kVec - 1)) + off - g0;
}

// i = c * S + s
LDM_RF_HD void split(int64_t i, int S, int64_t* c, int* s) {
  if ((uint64_t)i <= 0xffffffffull) {  // the usual case on 32-bit arithmetic
    const uint32_t q = (uint32_t)i / (uint32_t)S;
    *c = q, *s = (int)((uint32_t)i - q * (uint32_t)S);
  } else {
    const int64_t q = i / S;
    *c = q, *s = (int)(i - q * S);
  }
}

LDM_RF_HD float value(const float* table, int32_t row, int64_t c, int C, float weight) {
  return row < 0 ? 0.0f : table[(int64_t)row * C + c] * weight;
}

LDM_RF_HD void store_group(float* p, const float* v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
#else
  if (reinterpret_cast<uintptr_t>(p) & 15u) __builtin_trap();  // the host build checks what the device relies on
  p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
#endif
}

// Everything thread `tid` of chunk k of layout b writes.  tok(s) -> the checked token (row or -1) of position s of the
// layout's row; slab = d_out + b * C * S.
template <typename Tok>
LDM_RF_HD void thread_work(int tid, int64_t k, int64_t b, int mis, int S, int C, const float* table, float weight,
                           float* slab, const Tok& tok) {
  const int64_t CS = slab_size(S, C);
  for (int it = 0; it < kIter; ++it) {
    const int64_t i0 = slab_index(mis, b, CS, k * kChunk + (int64_t)(it * kBlock + tid) * kVec);
    if (i0 >= CS) return;
    if (i0 + kVec <= 0) continue;
    const int64_t first = i0 < 0 ? 0 : i0;
    int64_t c;
    int s;
    split(first, S, &c, &s);
    float v[kVec];  // (indexed by the unrolled j only: registers)
    bool all = true;
LDM_RF_UNROLL
    for (int j = 0; j < kVec; ++j) {
      const bool inside = i0 + j >= 0 && i0 + j < CS;
      all = all && inside;
      v[j] = 0.0f;
      if (inside) {
        v[j] = value(table, tok(s), c, C, weight);
        if (++s == S) s = 0, ++c;
      }
    }
    if (all) {
      store_group(slab + i0, v);
    } else {
LDM_RF_UNROLL
      for (int j = 0; j < kVec; ++j)
        if (i0 + j >= 0 && i0 + j < CS) slab[i0 + j] = v[j];
    }
  }
}

// whether chunk k of layout b holds any float of the slab (uniform over the workgroup)
LDM_RF_HD bool chunk_live(int64_t k, int64_t b, int mis, int S, int C) {
  const int64_t CS = slab_size(S, C);
  const int64_t lo = slab_index(mis, b, CS, k * kChunk);
  return lo < CS && lo + kChunk > 0;
}

}  // namespace ldm_refine
