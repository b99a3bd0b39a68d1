// Row kernels for gfx950: token+positional embedding gather, (Ada)LayerNorm, dtype casts and the
// load-time tables.  One 64-lane wavefront per row, float4 (16 B/lane) coalesced reads, wave-level
// DPP/shuffle reductions — no LDS, no cross-wave traffic.
//
// Reference semantics:
//   embedding     trainer/models/common/nn_lib.py:204,220 + ElementPositionalEmbedding 112-127
//   AdaLayerNorm  trainer/models/transformer_utils.py:72-83  (LN without affine, eps 1e-5)
//   LayerNorm     torch.nn.LayerNorm(d, eps=1e-5) (transformer_utils.py:156, nn_lib.py:186-189)
#include "ldm_kernels.h"
#include "ldm_variant_core.h"

namespace ldm {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr float kLoScale = kSplitLoScale;  // split mode: lo = (x - fp16(x)) * kSplitLoScale (ldm_kernels.h)

// NV = float4 per lane (D <= 256*NV)
template <int NV>
__global__ __launch_bounds__(256) void ln_rows(LnArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int nvec = a.D >> 2;
  float4 v[NV];
  if (a.tokens) {
    const int tok = a.tokens[row];
    const float4* e = reinterpret_cast<const float4*>(a.emb + (size_t)tok * a.D);
    const float4* p = reinterpret_cast<const float4*>(a.pos + (size_t)(row % a.S) * a.D);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 64 + lane;
      if (c < nvec) {
        float4 x = e[c], y = p[c];
        v[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
      } else {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  } else {
    const float4* x = reinterpret_cast<const float4*>(a.x + (size_t)row * a.D);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 64 + lane;
      v[i] = (c < nvec) ? x[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float inv_d = 1.0f / (float)a.D;
  const float mean = wave_sum(s) * inv_d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 64 + lane;
    if (c < nvec) {
      float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float var = wave_sum(q) * inv_d;  // biased variance
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
  if (a.stats_out && lane == 0) a.stats_out[row] = make_float2(mean, rstd);
  if (a.raw) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 64 + lane;
      if (c < nvec) reinterpret_cast<float4*>(a.y32 + (size_t)row * a.D)[c] = v[i];
    }
    return;
  }
  const float4* p0 = reinterpret_cast<const float4*>(a.p0);
  const float4* p1 = reinterpret_cast<const float4*>(a.p1);
  if (a.t_rows) {  // per-layout timesteps: the AdaLN rows of this row's layout (uniform over the wavefront: one row per wave)
    const float* ss = a.ada_tab + (size_t)a.t_rows[row / a.S] * a.t_stride + a.layer_off;
    p0 = reinterpret_cast<const float4*>(ss);
    p1 = reinterpret_cast<const float4*>(ss + a.D);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 64 + lane;
    if (c >= nvec) continue;
    float4 g = p0[c], b = p1[c];
    float4 y;
    if (a.ada) {
      y.x = (v[i].x - mean) * rstd * (1.0f + g.x) + b.x;
      y.y = (v[i].y - mean) * rstd * (1.0f + g.y) + b.y;
      y.z = (v[i].z - mean) * rstd * (1.0f + g.z) + b.z;
      y.w = (v[i].w - mean) * rstd * (1.0f + g.w) + b.w;
    } else {
      y.x = (v[i].x - mean) * rstd * g.x + b.x;
      y.y = (v[i].y - mean) * rstd * g.y + b.y;
      y.z = (v[i].z - mean) * rstd * g.z + b.z;
      y.w = (v[i].w - mean) * rstd * g.w + b.w;
    }
    if (a.y32) reinterpret_cast<float4*>(a.y32 + (size_t)row * a.D)[c] = y;
    if (a.y16) {
      __half2 h0 = __floats2half2_rn(y.x, y.y), h1 = __floats2half2_rn(y.z, y.w);
      uint2 pk;
      pk.x = *reinterpret_cast<unsigned*>(&h0);
      pk.y = *reinterpret_cast<unsigned*>(&h1);
      reinterpret_cast<uint2*>(a.y16 + (size_t)row * a.ld16)[c] = pk;
      if (a.y16lo) {
        float2 f0 = __half22float2(h0), f1 = __half22float2(h1);
        __half2 l0 = __floats2half2_rn((y.x - f0.x) * kLoScale, (y.y - f0.y) * kLoScale);
        __half2 l1 = __floats2half2_rn((y.z - f1.x) * kLoScale, (y.w - f1.y) * kLoScale);
        pk.x = *reinterpret_cast<unsigned*>(&l0);
        pk.y = *reinterpret_cast<unsigned*>(&l1);
        reinterpret_cast<uint2*>(a.y16lo + (size_t)row * a.ld16)[c] = pk;
      }
    }
  }
}

void launch_layernorm(const LnArgs& a, hipStream_t st) {
  const int blocks = (a.M + 3) / 4;
  if (a.D <= 256) {
    hipLaunchKernelGGL(ln_rows<1>, dim3(blocks), dim3(256), 0, st, a);
  } else if (a.D <= 512) {
    hipLaunchKernelGGL(ln_rows<2>, dim3(blocks), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(ln_rows<4>, dim3(blocks), dim3(256), 0, st, a);
  }
}

// ------------------------------------------------------------------ instance norm over a layout's rows (AdaInsNorm)
// transformer_utils.py:86-100: InstanceNorm1d(D) on x^T — per (layout, channel) mean and biased variance over the layout's S rows, eps
// 1e-5, no affine — then the AdaLN row: y = x_hat * (1 + scale) + shift.  LnArgs as ln_rows takes them (ada = 1; stats_out / raw unused).
// One workgroup of kInGroups x kInCols threads per layout: thread (g, tx) owns channels tx, tx + kInCols, ... and rows g, g + kInGroups, ...
// of them, so a wavefront reads 64 consecutive floats of one row.  Two passes in a fixed order, no atomics, any S: each thread adds its
// rows top to bottom in float64, the kInGroups partial sums of a channel meet in LDS and every thread of the channel adds them g = 0 first
// (sum -> mean, then the squared distances to that mean -> variance).  The third pass normalises the thread's own rows, so x may be y32.
// A layout of equal rows: the float64 sums of S equal floats are exact, mean == x, and y is `shift` exactly.
constexpr int kInCols = 256, kInGroups = 4;

__device__ __forceinline__ float in_load(const LnArgs& a, const int32_t* tok, int row0, int s, int c) {
  if (tok) return a.emb[(size_t)tok[s] * a.D + c] + a.pos[(size_t)s * a.D + c];
  return a.x[(size_t)(row0 + s) * a.D + c];
}

__global__ __launch_bounds__(kInCols * kInGroups) void in_rows(LnArgs a) {
  extern __shared__ double in_part[];   // [2][kInGroups][D]: partial sums, partial squared distances
  const int b = blockIdx.x, tx = threadIdx.x % kInCols, g = threadIdx.x / kInCols;
  const int S = a.S, D = a.D, row0 = b * S;
  if (row0 + S > a.M) return;   // (uniform over the workgroup; the launcher's grid is M / S)
  const int32_t* tok = a.tokens ? a.tokens + row0 : nullptr;
  double* part_sum = in_part;
  double* part_sq = in_part + (size_t)kInGroups * D;
  for (int c = tx; c < D; c += kInCols) {
    double acc = 0.0;
#pragma unroll 4
    for (int s = g; s < S; s += kInGroups) acc += (double)in_load(a, tok, row0, s, c);
    part_sum[g * D + c] = acc;
  }
  __syncthreads();
  const double inv_s = 1.0 / (double)S;
  for (int c = tx; c < D; c += kInCols) {
    const double mean = (((part_sum[c] + part_sum[D + c]) + part_sum[2 * D + c]) + part_sum[3 * D + c]) / (double)S;
    double acc = 0.0;
#pragma unroll 4
    for (int s = g; s < S; s += kInGroups) {
      const double d = (double)in_load(a, tok, row0, s, c) - mean;
      acc += d * d;
    }
    part_sq[g * D + c] = acc;
  }
  __syncthreads();
  const float* ss = a.p0;
  const float* sh = a.p1;
  if (a.t_rows) {  // per-layout timesteps: the AdaLN rows of this workgroup's layout
    ss = a.ada_tab + (size_t)a.t_rows[b] * a.t_stride + a.layer_off;
    sh = ss + D;
  }
  for (int c = tx; c < D; c += kInCols) {
    const float mean = (float)((((part_sum[c] + part_sum[D + c]) + part_sum[2 * D + c]) + part_sum[3 * D + c]) / (double)S);
    const float var = (float)((((part_sq[c] + part_sq[D + c]) + part_sq[2 * D + c]) + part_sq[3 * D + c]) * inv_s);   // biased variance
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const float mul = 1.0f + ss[c], add = sh[c];
    for (int s = g; s < S; s += kInGroups) {
      const float y = (in_load(a, tok, row0, s, c) - mean) * rstd * mul + add;
      const size_t row = (size_t)(row0 + s);
      if (a.y32) a.y32[row * D + c] = y;
      if (a.y16) {
        const __half h = __float2half_rn(y);
        a.y16[row * a.ld16 + c] = h;
        if (a.y16lo) a.y16lo[row * a.ld16 + c] = __float2half_rn((y - __half2float(h)) * kLoScale);
      }
    }
  }
}
static_assert(kInGroups == 4, "in_rows adds a channel's four partial sums by name");

void launch_instancenorm(const LnArgs& a, hipStream_t st) {
  const int layouts = a.M / a.S;   // (M = layouts * S: the denoiser's rows are whole layouts)
  const size_t lds = (size_t)2 * kInGroups * a.D * sizeof(double);   // 29 KiB at d_model 464, 64 KiB at the 1024 ldm_create admits
  hipLaunchKernelGGL(in_rows, dim3(layouts), dim3(kInCols * kInGroups), lds, st, a);
}

// ------------------------------------------------------------------ casts
__global__ __launch_bounds__(256) void cast_f32_f16(const float* __restrict__ src, __half* __restrict__ dst,
                                                    __half* __restrict__ dstlo, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (; i < n; i += stride) {
    const float x = src[i] * scale;  // (scale: an exact power of two — the split mode's weight pre-scale — or 1)
    const __half h = __float2half_rn(x);
    dst[i] = h;
    if (dstlo) dstlo[i] = __float2half_rn((x - __half2float(h)) * kLoScale);
  }
}

void launch_f32_to_f16(const float* src, __half* dst, __half* dstlo, int64_t n, hipStream_t st, float scale) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(cast_f32_f16, dim3(blocks), dim3(256), 0, st, src, dst, dstlo, n, scale);
}

// ------------------------------------------------------------------ load-time tables
// out[t][layer][j] = b[j] + sum_d W[j][d] * silu(emb[t][d])   — one wave per (t, j)
__global__ __launch_bounds__(256) void adaln_table_k(const float* __restrict__ emb, const float* __restrict__ w,
                                                     const float* __restrict__ b, float* __restrict__ out, int T,
                                                     int D, int L, int layer) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int two_d = 2 * D;
  if (idx >= T * two_d) return;
  const int t = idx / two_d, j = idx % two_d;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float e = emb[(size_t)t * D + d];
    const float sl = e / (1.0f + expf(-e));  // SiLU
    s += w[(size_t)j * D + d] * sl;
  }
  s = wave_sum(s);
  if (lane == 0) out[((size_t)t * L + layer) * two_d + j] = s + b[j];
}

void launch_adaln_table(const float* emb, const float* w, const float* b, float* out, int T, int D, int L, int layer,
                        hipStream_t st) {
  const int n = T * 2 * D;
  hipLaunchKernelGGL(adaln_table_k, dim3((n + 3) / 4), dim3(256), 0, st, emb, w, b, out, T, D, L, layer);
}

// timestep_type *_abs: the [T][D] sinusoid of SinusoidalPosEmb (ldm_variant_core.h) — one thread per (t, k), k < D / 2: the sine and the
// cosine of one argument
__global__ __launch_bounds__(256) void sinus_table_k(float* __restrict__ out, int T, int D) {
  const int half = D >> 1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * half) return;
  const int t = i / half, k = i % half;
  float s, c;
  ldm_variant::sinusoid_pair(t, T, k, half, &s, &c);
  out[(size_t)t * D + k] = s;
  out[(size_t)t * D + half + k] = c;
}

void launch_sinus_table(float* out, int T, int D, hipStream_t st) {
  const int n = T * (D >> 1);
  hipLaunchKernelGGL(sinus_table_k, dim3((n + 255) / 256), dim3(256), 0, st, out, T, D);
}

// timestep_type None: out[t][layer][j] = (j < D ? w[j] - 1 : b[j - D]) at every t
__global__ __launch_bounds__(256) void adaln_const_table_k(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ out,
                                                           int T, int D, int L, int layer) {
  const int two_d = 2 * D;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * two_d) return;
  const int t = i / two_d, j = i % two_d;
  out[((size_t)t * L + layer) * two_d + j] = ldm_variant::const_row_entry(w, b, D, j);
}

void launch_adaln_const_table(const float* w, const float* b, float* out, int T, int D, int L, int layer, hipStream_t st) {
  const int n = T * 2 * D;
  hipLaunchKernelGGL(adaln_const_table_k, dim3((n + 255) / 256), dim3(256), 0, st, w, b, out, T, D, L, layer);
}

__global__ __launch_bounds__(256) void pos_table_k(const float* __restrict__ elem, const float* __restrict__ attr,
                                                   float* __restrict__ pos, int E, int A, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * A * D) return;
  const int s = i / D, d = i % D;
  pos[i] = elem[(size_t)(s / A) * D + d] + attr[(size_t)(s % A) * D + d];
}

void launch_pos_table(const float* elem, const float* attr, float* pos, int E, int A, int D, hipStream_t st) {
  const int n = E * A * D;
  hipLaunchKernelGGL(pos_table_k, dim3((n + 255) / 256), dim3(256), 0, st, elem, attr, pos, E, A, D);
}

// Lane phase offset: one wave spins for `us` microseconds on the constant 100 MHz s_memrealtime counter.
__global__ void delay_k(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
void launch_delay_us(int us, hipStream_t st) {
  hipLaunchKernelGGL(delay_k, dim3(1), dim3(64), 0, st, (unsigned long long)us * 100ull);
}

}  // namespace ldm
