// affine_coords.h -- the coordinate arithmetic of the loader's affine resample (include/micformer_affine.h): output voxel ->
// normalised coordinate -> source coordinate -> tap indices, F.affine_grid + F.grid_sample(align_corners=False) per axis.
// Every function is __host__ __device__ and plain C++ (no HIP header needed), so a host program calls the very code
// volume_affine.hip runs (tests/affine_index_main.cpp does).  Every multiply-add is an explicit fmaf: host and device round alike,
// whatever the compiler's contraction setting.  Every index that leaves these functions lies in [0, extent): a coordinate is
// clamped in float BEFORE the conversion to int (clampf, which sends NaN to the lower bound), so no value, NaN and +-inf
// included, reaches the conversion outside [-1, extent].
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MICF_HD __host__ __device__ inline
#else
#define MICF_HD inline
#endif

namespace micf_affine {

// centre of output voxel o on an axis of `out` voxels, in [-1, 1]: ((2 o + 1) / out) - 1  (2 o + 1 is exact, two roundings)
MICF_HD float norm_coord(int o, int out) { return (float)(2 * o + 1) / (float)out - 1.0f; }

// one row of the 3 x 4 map applied to (nx, ny, nz, 1): three fused multiply-adds, innermost first
MICF_HD float map_row(const float* r, float nx, float ny, float nz) { return fmaf(r[0], nx, fmaf(r[1], ny, fmaf(r[2], nz, r[3]))); }

MICF_HD bool finite(float x) { return fabsf(x) <= 3.402823466e38f; }      // false for NaN and +-inf

// x into [lo, hi] by two comparisons: NaN fails the first and becomes lo
MICF_HD float clampf(float x, float lo, float hi) {
  x = x > lo ? x : lo;
  return x < hi ? x : hi;
}

// normalised source coordinate s -> index on an axis of `extent` elements: ((s + 1) * extent - 1) / 2
MICF_HD float source_index(float s, int extent) { return fmaf(s + 1.0f, (float)extent, -1.0f) * 0.5f; }

// The two taps of the linear interpolation at index i.  i0, i1: addresses, always in [0, extent).  w0, w1: their weights.
// in0, in1: whether the tap lies inside the array (always true under "border"); a tap outside contributes 0.
struct LinearTaps { int i0, i1; float w0, w1; bool in0, in1; };

MICF_HD LinearTaps linear_taps(float i, int extent, bool border) {
  LinearTaps t;
  const float last = (float)(extent - 1);
  if (border) {
    const float c = clampf(i, 0.0f, last);                   // in [0, extent - 1]
    const float f = floorf(c);
    const int k = (int)f;
    t.i0 = k;
    t.i1 = k + 1 < extent ? k + 1 : extent - 1;                    // (weight 0 where it was clamped: c == extent - 1)
    t.w1 = c - f;
    t.in0 = t.in1 = true;
  } else {
    const float c = clampf(i, -1.0f, (float)extent);         // in [-1, extent]: beyond either end both taps are outside
    const float f = floorf(c);
    const int k = (int)f;                                          // in [-1, extent]
    t.in0 = k >= 0 && k < extent;
    t.in1 = k + 1 >= 0 && k + 1 < extent;
    t.i0 = k < 0 ? 0 : (k < extent ? k : extent - 1);
    t.i1 = k + 1 < extent ? k + 1 : extent - 1;                    // (k + 1 >= 0 always)
    t.w1 = c - f;
  }
  t.w0 = 1.0f - t.w1;
  return t;
}

// The nearest element at index i: round half to even (rintf under the default rounding mode, as grid_sample's nearbyint).
// -> the address, always in [0, extent); `inside` tells whether the rounded index lay in the array (always true under "border").
MICF_HD int nearest_tap(float i, int extent, bool border, bool& inside) {
  if (border) {
    inside = true;
    return (int)rintf(clampf(i, 0.0f, (float)(extent - 1)));   // clamp and round commute: the bounds are integers
  }
  const int k = (int)rintf(clampf(i, -1.0f, (float)extent));   // in [-1, extent]
  inside = k >= 0 && k < extent;
  return k < 0 ? 0 : (k < extent ? k : extent - 1);
}

}  // namespace micf_affine
