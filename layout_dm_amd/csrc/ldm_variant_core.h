// Load-time arithmetic of the denoiser variants — the timestep_type choices of the reference's Block
// (trainer/models/transformer_utils.py:124-156) beyond the learned AdaLayerNorm embedding.  ONE source, compiled for the device
// (kernels_norm.hip sinus_table_k / adaln_const_table_k) and for the host (tests/cpu_variant_check.cpp).
//
// *_abs: SinusoidalPosEmb (transformer_utils.py:34-49) in place of nn.Embedding(T, D).  The reference evaluates, in float32,
//     x    = t / T * 4000                        (a Long timestep divided by the float num_steps, times the float rescale_steps)
//     f_k  = exp(k * -(ln 1e4 / (half - 1)))     k = 0 .. half - 1, half = D / 2; the Python double is a float32 scalar to the multiply
//     a    = x * f_k
//     emb  = sin(a) | cos(a)                     [T][D]: sines in the first half of a row, cosines in the second
// Here every step is evaluated in float64 and rounded to float32 where the reference rounds: a quotient or product of two float32
// values rounded once from float64 IS the float32 operation, and exp / sin / cos rounded from float64 are the correctly rounded
// float32 functions up to the float64 routine's own last-bit error.  (torch's float32 exp is not correctly rounded: the reference's
// own table differs from this one by up to one ulp of f_k times x, tests/test_denoiser_variants.py.)
//
// timestep_type None: norm1 is nn.LayerNorm(D) with an affine.  Served by the AdaLN table, constant in t:
//     x_hat * w + b  ==  x_hat * (1 + scale) + shift   with   scale = w - 1, shift = b
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LDM_VR_HD __host__ __device__ __forceinline__
#else
#define LDM_VR_HD inline
#endif

namespace ldm_variant {

constexpr double kLn1e4 = 9.210340371976184;   // math.log(10000), the float64 the reference computes on the host
constexpr double kRescaleSteps = 4000.0;       // SinusoidalPosEmb rescale_steps

LDM_VR_HD bool sinusoid_args_ok(int T, int D) { return T >= 1 && D >= 4 && !(D & 1); }   // half - 1 >= 1

// x of timestep t
LDM_VR_HD float sinusoid_x(int t, int T) {
  const float q = (float)((double)(float)t / (double)(float)T);
  return (float)((double)q * kRescaleSteps);
}

// f_k
LDM_VR_HD float sinusoid_freq(int k, int half) {
  const float c = (float)(-(kLn1e4 / (double)(half - 1)));
  const float e = (float)((double)(float)k * (double)c);
  return (float)exp((double)e);
}

// a = x * f_k: the argument of entry (t, k) and of entry (t, half + k)
LDM_VR_HD float sinusoid_arg(int t, int T, int k, int half) { return (float)((double)sinusoid_x(t, T) * (double)sinusoid_freq(k, half)); }

// entries (t, k) and (t, half + k) of the [T][D] table
LDM_VR_HD void sinusoid_pair(int t, int T, int k, int half, float* s, float* c) {
  const double a = (double)sinusoid_arg(t, T, k, half);
  *s = (float)sin(a);
  *c = (float)cos(a);
}

// timestep_type None: entry j of a [2 D] AdaLN row from nn.LayerNorm's weight / bias
LDM_VR_HD float const_row_entry(const float* w, const float* b, int D, int j) { return j < D ? w[j] - 1.0f : b[j - D]; }

}  // namespace ldm_variant
