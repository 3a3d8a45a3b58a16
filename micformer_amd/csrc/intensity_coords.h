// intensity_coords.h -- the index, weight and random-number arithmetic of the intensity augmentation
// (include/micformer_intensity.h): the reflect index of the blur, its radius and normalised weights, and the counter-based
// normal draw of the noise.  In the style of elastic_coords.h: every function is __host__ __device__ and plain C++, so a host
// program calls the very code volume_intensity.hip runs (tests/intensity_index_main.cpp does).  Every index that leaves
// reflect_index lies in [0, n) whatever its arguments; the radius lies in [0, kMaxRadius] whatever sigma is.
#pragma once
#include <math.h>
#include <stdint.h>

#include "affine_coords.h"

namespace micf_intensity {

constexpr int kMaxRadius = 8;                  // int(4 * 2.0 + 0.5): sigma is clamped to [0.1, 2.0]
constexpr int kTaps = 2 * kMaxRadius + 1;      // a weight table is centred on element kMaxRadius
constexpr float kSigmaMin = 0.1f, kSigmaMax = 2.0f;

// scipy.ndimage's "reflect" (d c b a | a b c d | d c b a): the period is 2 n, repeated as often as needed, so an axis shorter
// than the radius is legal.  n < 1 is treated as 1.
MICF_HD int reflect_index(int i, int n) {
  if (n <= 1) return 0;
  const int p = 2 * n;                         // (n <= 2048 in the library; no overflow below 2^30)
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// sigma as the kernels use it: 0 (no blur) for sigma <= 0, NaN for NaN (it then reaches every voxel of the channel through the
// centre weight), else clamped to [kSigmaMin, kSigmaMax].
MICF_HD float clamp_sigma(float sigma) {
  if (sigma != sigma) return sigma;
  if (!(sigma > 0.0f)) return 0.0f;
  return sigma < kSigmaMin ? kSigmaMin : (sigma > kSigmaMax ? kSigmaMax : sigma);
}

// radius int(4 sigma + 0.5) of a clamped sigma, in float64 as scipy computes it (in float32 the sum can round up to the next
// integer); 0 for 0 and NaN.
MICF_HD int blur_radius(float clamped) {
  if (!(clamped > 0.0f)) return 0;
  const int r = (int)(4.0 * (double)clamped + 0.5);
  return r < 0 ? 0 : (r > kMaxRadius ? kMaxRadius : r);
}

// w[kMaxRadius + k] = exp(-k^2 / (2 sigma^2)) / sum for |k| <= radius, 0 beyond; float64 until the final rounding.  -> the radius.
MICF_HD int blur_weights(float clamped, float* w) {
  const int r = blur_radius(clamped);
  for (int j = 0; j < kTaps; ++j) w[j] = 0.0f;
  if (clamped != clamped) {
    w[kMaxRadius] = clamped;
    return 0;
  }
  if (!(clamped > 0.0f)) {
    w[kMaxRadius] = 1.0f;
    return 0;
  }
  const double s2 = (double)clamped * (double)clamped;
  double e[kMaxRadius + 1], sum = 0.0;
  for (int k = 0; k <= r; ++k) e[k] = exp(-0.5 * (double)(k * k) / s2);
  for (int k = -r; k <= r; ++k) sum += e[k < 0 ? -k : k];              // ascending k, as scipy's _gaussian_kernel1d sums it
  for (int k = -r; k <= r; ++k) w[kMaxRadius + k] = (float)(e[k < 0 ? -k : k] / sum);
  return r;
}

MICF_HD uint64_t mix64(uint64_t z) {           // splitmix64 finaliser (misc.hip's)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// key of (sample seed, channel); word of voxel i under it
MICF_HD uint64_t noise_key(int64_t seed, int c) { return mix64((uint64_t)seed ^ mix64((uint64_t)c)); }
MICF_HD uint64_t noise_word(uint64_t key, uint64_t i) { return mix64(key + i); }

// u1 = ((h >> 40) + 0.5) 2^-24 and u2 = ((h & 0xFFFFFF) + 0.5) 2^-24.  k + 0.5 is exact in float32 below k = 2^23 and rounds to
// even from there on (u = 1 for the last k), so normal() does not take ln u1 from the rounded value.
MICF_HD float uniform_hi(uint64_t h) { return ((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.0f); }
MICF_HD float uniform_lo(uint64_t h) { return ((float)(uint32_t)(h & 0xFFFFFFull) + 0.5f) * (1.0f / 16777216.0f); }

// ln u1 from the exact integers: above k = 2^23 the complement 1 - u1 = ((2^24 - 1 - k) + 0.5) 2^-24 is exact instead
MICF_HD float log_uniform_hi(uint64_t h) {
  const uint32_t k = (uint32_t)(h >> 40);
  if (k < (1u << 23)) return logf(((float)k + 0.5f) * (1.0f / 16777216.0f));
  return log1pf(-(((float)(16777215u - k) + 0.5f) * (1.0f / 16777216.0f)));
}

// Box-Muller: sqrt(-2 ln u1) cos(2 pi u2), |z| <= 5.9
MICF_HD float normal(uint64_t h) { return sqrtf(-2.0f * log_uniform_hi(h)) * cosf(6.2831855f * uniform_lo(h)); }

}  // namespace micf_intensity
