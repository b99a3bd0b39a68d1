// Exact-mode (fp32) MFMA GEMMs for the denoiser's five Linear classes (QKV, attn-out, FFN1, FFN2, vocab head):
//     C[M,N] = epilogue(A[M,K] · W[N,K]^T + bias[N])         (torch.nn.Linear convention, "NT")
// Reference call sites: torch.nn.MultiheadAttention in/out projections
// (trainer/models/transformer_utils.py:140-142,197-204), linear1/linear2 (l.145-147,208-209),
// head Linear (trainer/models/common/nn_lib.py:186-189).
//
// gfx950 design notes
//  * 64-lane wavefronts; a 256-thread workgroup = 4 waves in a 2x2 grid, each wave owns a 64x64
//    sub-tile = 2x2 MFMA 32x32 accumulators (64 accumulator VGPRs).
//  * exact mode: v_mfma_f32_32x32x2_f32 (bit-exact fmaf chain, 157 TF peak).  Lane l supplies
//    A[i=l&31][k=l>>5]; we let each lane read 4 consecutive k (one ds_read_b128) and feed 4 MFMAs,
//    i.e. MFMA j of a group contracts k = {k0+j, k0+4+j} — a permutation of the K order that is
//    applied to A and W alike, so the product is unchanged.
//  * operands arrive by LDS-DMA into unpadded, XOR-swizzled images (see gemm_f32_tile).
//  * workgroup -> tile mapping is XCD-aware: the 8 XCDs have private L2s and the dispatcher places
//    block b on XCD b%8, so consecutive tile ids (same A row-panel, neighbouring W panels) are
//    remapped onto the same XCD.
#include "ldm_kernels.h"

namespace ldm {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr float kLoScale = kSplitLoScale;

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  // bijective for any nwg (cdna guide §5 "XCD swizzle must be bijective")
  const int xcd = bid & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ---------------------------------------------------------------- shared epilogue
struct EpiArgs {
  const float* bias;
  const float* res;
  float* C32;
  __half* C16;
  __half* C16lo;
  int M, N, ldres, ldc32, ldc16, relu;
  float out_scale = 1.0f;  // split mode: undoes the weight tensor's power-of-two pre-scale (applied to the accumulators)
};

template <int MI = 2>
__device__ __forceinline__ void epilogue_store(const EpiArgs& e, const f32x16 (&acc)[MI][2], int m_base, int n_base,
                                               int lane) {
  const int col_in = lane & 31;
  const int row_hi = (lane >> 5) * 4;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int n = n_base + ni * 32 + col_in;
      if (n >= e.N) continue;
      const float bv = e.bias ? e.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m_base + mi * 32 + (r & 3) + 8 * (r >> 2) + row_hi;
        if (m >= e.M) continue;
        float v = acc[mi][ni][r] + bv;
        if (e.relu) v = fmaxf(v, 0.f);
        if (e.res) v += e.res[(size_t)m * e.ldres + n];
        if (e.C32) e.C32[(size_t)m * e.ldc32 + n] = v;
        if (e.C16) {
          const __half h = __float2half_rn(v);
          e.C16[(size_t)m * e.ldc16 + n] = h;
          if (e.C16lo) e.C16lo[(size_t)m * e.ldc16 + n] = __float2half_rn((v - __half2float(h)) * kLoScale);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- exact fp32
constexpr int F32_BK = 16;

// Operands by LDS-DMA (global_load_lds_dwordx4): no staging registers, no ds_write, no VGPR round trip.  One wave
// instruction fills 1 KiB of LDS linearly, and WHICH (row, 16-byte k segment) lands in a slot is the lane's choice of
// global address, so the swizzle is free: slot(r, s) = 4 r + (s ^ ((r >> 1) & 3)) serves a fragment
// ds_read_b128 in two passes without padding (32 KB of LDS per workgroup).  The XOR with (r >> 2) & 3 is conflict-free
// under gfx950's 16-lane service groups (tests/test_lds_swizzle.py) and was measured: 0.5 % SLOWER in the timed loop, FFN1 and
// in_proj 2-4 % slower run alone (profiles/r03_call29_30_gemm32_swizzle_ab.txt): the LDS is far from saturated by
// this kernel (12 fragment reads per 32 MFMAs of 64 cycles), so the reads' pace is not what limits it.
// Persistent over tiles: the grid is min(tiles, 4 per CU) workgroups and workgroup w walks tiles w, w + grid, ... (the
// same XCD: grid is a multiple of 8); a workgroup that moves on leaves its 64 epilogue stores to drain from L2 under the
// next main loop and pays the launch / first-load ramp once.  tools/microbench/gemm32.hip on the four shapes of a layer
// (M = 32 000): register-staged, one workgroup per tile 414 / 161 / 507 / 527 us -> 334 / 155 / 446 / 475 us, bit-identical
// (profiles/r03_gemm32_microbench.txt).
// MI = 2: 128 x 128 tile (each wave 64 x 64), the one instantiation.  Measured and removed: 64-row tiles (MI = 1), two per
// workgroup, for the one-round GEMMs (whole job within the spread, profiles/r03_call31_gemm32_bm64_ab.txt) and 128 x 160 tiles
// for N = 464 (4 % faster run alone, 0.5 % slower in the two-lane timed loop, profiles/r03_call26_gemm32_wide_ab.txt).
template <int MI>
__global__ __launch_bounds__(256, 4) void gemm_f32_tile(const float* __restrict__ A, const float* __restrict__ W,
                                                        int lda, int ldw, int K, int tiles_n, int n_tiles, EpiArgs e) {
  constexpr int BM = 64 * MI;
  constexpr int kImgA = BM * F32_BK * 4, kImgW = 128 * F32_BK * 4;  // bytes
  __shared__ __attribute__((aligned(1024))) char L[2][kImgA + kImgW];  // [buffer][A image | W image]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 31, hi = lane >> 5;
  const int nk = K / F32_BK;
  const unsigned lds0 = (unsigned)(size_t)&L[0][0];
  // fragment read offsets (bytes inside a [rows x 16] operand image): row base + swizzled segment of k group 0 / 1
  const int xr = (frow >> 1) & 3;
  const unsigned fa0 = (unsigned)((wm * 32 * MI + frow) * 64 + 16 * (hi ^ xr)), fa1 = fa0 ^ 32u;
  const unsigned fb0 = (unsigned)(kImgA + (wn * 64 + frow) * 64 + 16 * (hi ^ xr)), fb1 = fb0 ^ 32u;
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int tile = xcd_remap(t, n_tiles);
    const int m0 = (tile / tiles_n) * BM;
    const int n0 = (tile % tiles_n) * 128;
    const float* At = A + (size_t)m0 * lda;
    const float* Wt = W + (size_t)n0 * ldw;
    // DMA source offsets (bytes from the tile's first row) of this wave's instructions: LDS slot 64 i + lane <- (row,
    // segment); A image: instructions w (+ 4 for MI = 2), W image: w and w + 4.  Rows past M / N are clamped to the last
    // one: their products are never stored.
    unsigned va[2], vw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = wave + 4 * j, r = 16 * i + (lane >> 2), sg = (lane & 3) ^ ((r >> 1) & 3);
      va[j] = (unsigned)((min(r, e.M - 1 - m0) * lda + sg * 4) * 4);
      vw[j] = (unsigned)((min(r, e.N - 1 - n0) * ldw + sg * 4) * 4);
    }
    auto dma = [&](int kt, int buf) {
      const char* ga = reinterpret_cast<const char*>(At + kt * F32_BK);
      const char* gw = reinterpret_cast<const char*>(Wt + kt * F32_BK);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned la = lds0 + (unsigned)(buf * (kImgA + kImgW)) + (unsigned)((wave + 4 * j) * 1024);
        if (j < MI)
          asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(va[j]), "s"(ga), "s"(la) : "memory");
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(vw[j]), "s"(gw), "s"(la + kImgA)
                     : "memory");
      }
    };
    f32x16 acc[MI][2];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    // (the previous tile's last iteration ended with a barrier: both buffers are free)
    dma(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // hipcc does not count the DMA in its vmcnt bookkeeping
    __syncthreads();
    auto mfmas = [&](int buf) {
      const char* lb = &L[buf][0];
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        f32x4 a[MI], b[2];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = *reinterpret_cast<const f32x4*>(lb + (kg ? fa1 : fa0) + mi * 32 * 64);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b[ni] = *reinterpret_cast<const f32x4*>(lb + (kg ? fb1 : fb0) + ni * 32 * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][j], b[ni][j], acc[mi][ni], 0, 0, 0);
      }
    };
    for (int kt = 0; kt < nk; kt += 2) {  // (two iterations per trip: the buffer index is static)
      if (kt + 1 < nk) dma(kt + 1, 1);
      mfmas(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (kt + 1 < nk) {
        if (kt + 2 < nk) dma(kt + 2, 0);
        mfmas(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
    epilogue_store<MI>(e, acc, m0 + wm * 32 * MI, n0 + wn * 64, lane);
  }
}

void launch_gemm(const GemmArgs& g, hipStream_t st) {
  const int tiles_m = (g.M + 127) / 128;
  const int tiles_n = (g.N + 127) / 128;
  EpiArgs e{g.bias, g.res, g.C32, g.C16, g.C16lo, g.M, g.N, g.ldres, g.ldc32, g.ldc16, g.relu};
  e.out_scale = g.out_scale > 0.f ? g.out_scale : 1.0f;
  static const int resident = [] {  // as many workgroups as the chip holds at once
    int dev = 0, cus = 256, per_cu = 4;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)gemm_f32_tile<2>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    return (per_cu * cus) & ~7;  // (a multiple of 8: tile t stays on XCD t % 8)
  }();  // 32 KB of LDS, < 100 VGPRs: 5 per CU
  const int n_tiles = tiles_m * tiles_n;
  hipLaunchKernelGGL(gemm_f32_tile<2>, dim3(n_tiles < resident ? n_tiles : resident), dim3(256), 0, st, (const float*)g.A,
                     (const float*)g.W, g.lda, g.ldw, g.K, tiles_n, n_tiles, e);
}

}  // namespace ldm
