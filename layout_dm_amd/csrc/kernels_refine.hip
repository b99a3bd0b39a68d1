// cond=refinement prior on the device (ldm_refinement_prior): out[b][c][s] = table[seq_orig[b'][s]][c] * weight, the (B,C,S)
// tensor the loop kernels read as cond["weak_logits"].  The index, bounds and broadcast arithmetic is ldm_refine_core.h (one
// source for this kernel and the host build the CPU tests run); this file adds what only the device has.
//
// The kernel is bound by its stores (C * S floats per layout against a (C,C) table that stays in L2): a workgroup owns
// kChunk consecutive floats of a layout's slab and writes them as 16-byte stores, consecutive lanes on consecutive
// addresses.  The layout's tokens are read once per workgroup into LDS, range-checked on the way (sequences beyond
// kMaxStaged tokens are read in place instead).  No atomics — the error word is a plain store of the same value by every
// thread that meets a bad token — and no scratch.
#include "ldm_kernels.h"
#include "ldm_refine_core.h"

namespace ldm {

namespace {

namespace R = ldm_refine;

struct StagedTokens {
  const int32_t* toks;
  __device__ __forceinline__ int32_t operator()(int s) const { return toks[s]; }
};

struct DirectTokens {
  const void* seq;
  int seq_i64, C;
  int64_t row_off;
  int32_t* err;
  __device__ __forceinline__ int32_t operator()(int s) const {
    const int32_t t = R::checked_token(R::load_token(seq, seq_i64, row_off + s), C);
    if (t < 0) *err = R::kErrToken;
    return t;
  }
};

template <bool STAGED>
__global__ __launch_bounds__(R::kBlock) void refinement_prior_k(const void* __restrict__ seq, int seq_i64, int B_seq, int S, int C,
                                                                const float* __restrict__ table, float weight,
                                                                float* __restrict__ out, int mis, unsigned n_chunk,
                                                                int32_t* __restrict__ err) {
  __shared__ int32_t toks[STAGED ? R::kMaxStaged : 1];
  const int64_t b = blockIdx.x / n_chunk, k = blockIdx.x % n_chunk;
  if (!R::chunk_live(k, b, mis, S, C)) return;  // (the whole workgroup: nobody waits at the barrier below)
  const int64_t row_off = R::seq_row(b, B_seq) * S;
  float* slab = out + b * R::slab_size(S, C);
  if (STAGED) {
    for (int s = threadIdx.x; s < S; s += R::kBlock) {
      const int32_t t = R::checked_token(R::load_token(seq, seq_i64, row_off + s), C);
      if (t < 0) *err = R::kErrToken;
      toks[s] = t;
    }
    __syncthreads();
    R::thread_work((int)threadIdx.x, k, b, mis, S, C, table, weight, slab, StagedTokens{toks});
  } else {
    R::thread_work((int)threadIdx.x, k, b, mis, S, C, table, weight, slab, DirectTokens{seq, seq_i64, C, row_off, err});
  }
}

}  // namespace

void launch_refinement_prior(const void* seq, int seq_i64, int B_seq, int B, int S, int C, const float* table, float weight,
                             float* out, int32_t* err, hipStream_t st) {
  const unsigned n_chunk = (unsigned)R::chunks_per_layout(S, C);
  const dim3 grid((unsigned)B * n_chunk), block(R::kBlock);
  const int mis = R::misalign_of(out);
  if (S <= R::kMaxStaged)
    hipLaunchKernelGGL(refinement_prior_k<true>, grid, block, 0, st, seq, seq_i64, B_seq, S, C, table, weight, out, mis, n_chunk,
                       err);
  else
    hipLaunchKernelGGL(refinement_prior_k<false>, grid, block, 0, st, seq, seq_i64, B_seq, S, C, table, weight, out, mis,
                       n_chunk, err);
}

}  // namespace ldm
