// elastic_coords.h -- the control-grid arithmetic of the loader's elastic resample (include/micformer_elastic.h): output voxel ->
// control cell and fraction -> tap addresses and weights of the displacement field's interpolation, per axis.  In the style of
// affine_coords.h: every function is __host__ __device__ and plain C++, so a host program calls the very code volume_elastic.hip
// runs (tests/elastic_index_main.cpp does), and every multiply-add is an explicit fmaf.  The cell and the fraction's numerator
// are integers, so the cell is exact and the fraction carries one rounding (two where out - 1 exceeds 2^24); every tap address
// that leaves these functions lies in [0, g), whatever the inputs.
#pragma once
#include "affine_coords.h"

#if defined(__clang__)
#define MICF_UNROLL _Pragma("unroll")
#define MICF_ROLLED _Pragma("unroll 1")
#else
#define MICF_UNROLL
#define MICF_ROLLED
#endif

namespace micf_elastic {

// Control position of output voxel o on an axis of `out` voxels under a grid of g >= 2 points whose first and last point sit on
// the centres of the first and last voxel: p = o (g - 1) / (out - 1) = k + t with k in [0, g - 1] and t in [0, 1); out == 1: p = 0.
// The last voxel lands on the last control point: k = g - 1, t = 0.  An o outside [0, out) is clamped first.
struct Cell { int k; float t; };

MICF_HD Cell control_cell(int o, int out, int g) {
  Cell c{0, 0.0f};
  if (out <= 1 || g < 2) return c;
  o = o < 0 ? 0 : (o < out ? o : out - 1);
  const long long num = (long long)o * (g - 1), den = (long long)out - 1;        // (o < 2^31, g <= 512: no overflow)
  c.k = (int)(num / den);
  c.t = (float)(num % den) / (float)den;
  return c;
}

// The taps of one axis: kTaps addresses from `first` on, each clamped to [0, g - 1], and their weights.
//   linear  2 taps, k and k + 1, weights (1 - t, t): interpolates the control values
//   cubic   4 taps, k - 1 ... k + 2, the uniform cubic B-spline ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6:
//           approximates them, C2
template <int kTaps>
struct AxisTaps {
  int first, g;
  float w[kTaps];
  MICF_HD int address(int j) const {
    const int a = first + j;
    return a < 0 ? 0 : (a < g ? a : g - 1);
  }
  MICF_HD float weight(int j) const {                              // w[j] by selects: a rolled loop's j indexes no array
    float r = w[0];
    MICF_UNROLL
    for (int i = 1; i < kTaps; ++i) r = j == i ? w[i] : r;
    return r;
  }
};

MICF_HD AxisTaps<2> linear_taps(const Cell& c, int g) {
  AxisTaps<2> a;
  a.first = c.k;
  a.g = g;
  a.w[0] = 1.0f - c.t;
  a.w[1] = c.t;
  return a;
}

MICF_HD AxisTaps<4> cubic_taps(const Cell& c, int g) {
  AxisTaps<4> a;
  const float t = c.t, u = 1.0f - t, sixth = 1.0f / 6.0f;
  a.first = c.k - 1;
  a.g = g;
  a.w[0] = u * u * u * sixth;
  a.w[1] = fmaf(t * t, fmaf(0.5f, t, -1.0f), 2.0f / 3.0f);                        // t^3 / 2 - t^2 + 2 / 3
  a.w[2] = fmaf(t, fmaf(t, fmaf(-0.5f, t, 0.5f), 0.5f), sixth);                   // -t^3 / 2 + t^2 / 2 + t / 2 + 1 / 6
  a.w[3] = t * t * t * sixth;
  return a;
}

// One component of the field (gd x gh x gw floats at f) interpolated at the three axes' taps: separable, x innermost, one fmaf per
// tap and per finished row and plane.  The planes are a rolled loop (at most kTaps^2 taps in flight, 16 of the cubic's 64); the
// rows and taps of a plane unroll, so their weights are registers.
template <int kTaps>
MICF_HD float interpolate(const float* f, const AxisTaps<kTaps>& tz, const AxisTaps<kTaps>& ty, const AxisTaps<kTaps>& tx) {
  float acc = 0.0f;
  MICF_ROLLED
  for (int jz = 0; jz < kTaps; ++jz) {
    const float* slab = f + (long long)tz.address(jz) * ty.g * tx.g;
    float plane = 0.0f;
    MICF_UNROLL
    for (int jy = 0; jy < kTaps; ++jy) {
      const float* row = slab + (long long)ty.address(jy) * tx.g;
      float r = 0.0f;
      MICF_UNROLL
      for (int jx = 0; jx < kTaps; ++jx) r = fmaf(tx.w[jx], row[tx.address(jx)], r);
      plane = fmaf(ty.w[jy], r, plane);
    }
    acc = fmaf(tz.weight(jz), plane, acc);
  }
  return acc;
}

}  // namespace micf_elastic
