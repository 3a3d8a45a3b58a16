// lowres_coords.h -- the index, weight and prefilter-start arithmetic of the low-resolution simulation
// (include/micformer_lowres.h): the clamp of a target extent, the nearest-neighbour gather index of the downsample, the tap base
// and the cubic B-spline weights of the upsample, and the closed-form start, end and edge extension of the B-spline prefilter.
// In the style of intensity_coords.h: every function is __host__ __device__ and plain C++, so a host program calls the very code
// volume_lowres.hip runs (tests/lowres_index_main.cpp does).  All index arithmetic is integer: n <= 2048, so (2 o + 1) n < 2^24.
// Whatever its arguments, gather_index lies in [0, n) and tap_floor in [-1, t - 1]: the four taps tap_floor - 1 .. tap_floor + 2 lie
// in [-2, t + 1], the coefficient array extended by kExt entries on either side.
#pragma once
#include <math.h>
#include <stdint.h>

#include "affine_coords.h"

namespace micf_lowres {

constexpr int kExt = 2;                         // coefficients kept beyond either end of an axis: indices -2 .. t + 1
constexpr float kPole = -0.26794919243112270f;  // z = sqrt(3) - 2, the pole of the cubic B-spline prefilter
constexpr float kFirst = 4.7320508075688773f;   // 6 / (1 - z): the causal sum of 6 x a constant
constexpr float kLast = 0.28867513459481288f;   // -z / (1 - z^2) = z / (z^2 - 1)

// a target extent as the kernels use it: into [1, n] (n < 1 is treated as 1)
MICF_HD int clamp_target(int t, int n) {
  if (n < 1) n = 1;
  return t < 1 ? 1 : (t > n ? n : t);
}

// nearest downsample n -> t (t already clamped): floor((o + 1/2) n / t - 1/2 + 1/2), half-pixel centres, ties upward
MICF_HD int gather_index(int o, int n, int t) {
  if (n < 1) n = 1;
  t = clamp_target(t, n);
  if (o < 0) o = 0;
  if (o > t - 1) o = t - 1;
  const int g = ((2 * o + 1) * n) / (2 * t);
  return g > n - 1 ? n - 1 : g;
}

// upsample t -> n: output o reads at s = (o + 1/2) t / n - 1/2 = ((2 o + 1) t - n) / (2 n).  -> floor(s), in [-1, t - 1];
// frac = s - floor(s) in [0, 1): an exact remainder over 2 n, rounded once
MICF_HD int tap_floor(int o, int n, int t, float* frac) {
  if (n < 1) n = 1;
  t = clamp_target(t, n);
  if (o < 0) o = 0;
  if (o > n - 1) o = n - 1;
  const int num = (2 * o + 1) * t - n, den = 2 * n;       // num in (-n, (2 n - 1) t - n]
  int fl = num >= 0 ? num / den : -((-num + den - 1) / den);
  const int rem = num - fl * den;                         // in [0, den)
  *frac = (float)rem / (float)den;
  if (fl < -1) fl = -1;
  if (fl > t - 1) fl = t - 1;
  return fl;
}

// the four cubic B-spline weights of taps floor - 1 .. floor + 2 at fraction f: (1/6, 4/6, 1/6, 0) at f = 0
MICF_HD void cubic_weights(float f, float* w) {
  const float g = 1.0f - f, f2 = f * f, g2 = g * g;
  w[0] = g2 * g * (1.0f / 6.0f);
  w[1] = (4.0f - 6.0f * f2 + 3.0f * f2 * f) * (1.0f / 6.0f);
  w[2] = (4.0f - 6.0f * g2 + 3.0f * g2 * g) * (1.0f / 6.0f);
  w[3] = f2 * f * (1.0f / 6.0f);
}

// The prefilter of a line s[0 .. t) extended by its edge values to infinity, gain 6:
//   causal      p[0] = kFirst s[0] (the closed-form sum over the constant extension), p[k] = 6 s[k] + z p[k - 1]
//   anticausal  c[t - 1] = s[t - 1] + kLast (p[t - 1] - kFirst s[t - 1]) (closed form again), c[k] = z (c[k + 1] - p[k])
//   extension   c[-j] = s[0] + (c[0] - s[0]) z^j and c[t - 1 + j] = s[t - 1] + (c[t - 1] - s[t - 1]) z^j: the coefficients of
//               the constant part of the extended signal decay to the constant itself
MICF_HD float causal_first(float s0) { return kFirst * s0; }
MICF_HD float causal_next(float p, float s) { return fmaf(kPole, p, 6.0f * s); }
MICF_HD float anticausal_last(float p_last, float s_last) { return fmaf(kLast, p_last - kFirst * s_last, s_last); }
MICF_HD float anticausal_next(float c_next, float p) { return kPole * (c_next - p); }
MICF_HD float extend1(float c_edge, float s_edge) { return fmaf(c_edge - s_edge, kPole, s_edge); }
MICF_HD float extend2(float c_edge, float s_edge) { return fmaf(c_edge - s_edge, kPole * kPole, s_edge); }

}  // namespace micf_lowres
