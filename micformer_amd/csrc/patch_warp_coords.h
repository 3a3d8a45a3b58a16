// patch_warp_coords.h -- the coordinate arithmetic that the warped patch crop (include/micformer_patch_warp.h) adds to
// affine_coords.h and elastic_coords.h: the origin add that turns a normalised PATCH coordinate into a scan index, the label's
// outside rule, and the displacement field collapsed over z and y for one control cell of a row.  In the style of patches_coords.h:
// every function is __host__ __device__ and plain C++, so a host program calls the very code volume_patch_warp.hip runs
// (tests/patch_warp_index_main.cpp does), and every multiply-add is an explicit fmaf.  The control cell of a patch voxel is
// elastic_coords.h's control_cell(o, P, g) unchanged: the field's corner points sit on the centres of the patch's first and last
// voxel.  Every address that leaves these functions lies inside its array, whatever the inputs.
#pragma once
#include "elastic_coords.h"

namespace micf_patch_warp {

// Scan index on one axis of the normalised patch coordinate s, for a patch of P voxels whose window starts at scan voxel o:
// o + ((s + 1) P - 1) / 2.  source_index is affine_coords.h's (one fmaf and an exact halving); the add rounds once.  With P a power
// of two and s the centre of patch voxel x the result is o + x exactly.  o is an origin of the locate step: |o| <= 2048.
MICF_HD float scan_index(int o, float s, int P) { return (float)o + micf_affine::source_index(s, P); }

// The label's address on one axis: round half to even, and whether the ROUNDED index lies in the scan.  The patch sampler's own
// rule: outside is outside in both padding modes (the class is then pad_class), so the index is never clamped into the scan first.
// -> the address, always in [0, L).
MICF_HD int label_tap(float i, int L, bool& inside) { return micf_affine::nearest_tap(i, L, false, inside); }

// The field's taps of one row of patch voxels (fixed z and y taps) and one control cell on x, collapsed over z and y: col[c][j] is
// component c at x address ax.address(j), summed over the kTaps^2 (z, y) taps with one fmaf per tap, y inside z.  The displacement
// at a voxel of the cell is then sum_j wx[j] col[c][j] (displacement below): the x weights are the only part that changes from
// voxel to voxel inside a cell, so a thread that owns a run of x recomputes col only where the run enters another cell.
// f: [3][gd][gh][gw] floats.  Every address is clamped by AxisTaps::address.
template <int kTaps>
MICF_HD void field_columns(const float* f, const micf_elastic::AxisTaps<kTaps>& tz, const micf_elastic::AxisTaps<kTaps>& ty,
                           const micf_elastic::AxisTaps<kTaps>& ax, float (&col)[3][kTaps]) {
  const long long plane = (long long)tz.g * ty.g * ax.g;
  MICF_UNROLL
  for (int c = 0; c < 3; ++c) {
    MICF_UNROLL
    for (int j = 0; j < kTaps; ++j) col[c][j] = 0.0f;
  }
  MICF_UNROLL
  for (int jz = 0; jz < kTaps; ++jz) {
    MICF_UNROLL
    for (int c = 0; c < 3; ++c) {
      const float* slab = f + c * plane + (long long)tz.address(jz) * ty.g * ax.g;
      float part[kTaps];
      MICF_UNROLL
      for (int j = 0; j < kTaps; ++j) part[j] = 0.0f;
      MICF_UNROLL
      for (int jy = 0; jy < kTaps; ++jy) {
        const float* row = slab + (long long)ty.address(jy) * ax.g;
        MICF_UNROLL
        for (int j = 0; j < kTaps; ++j) part[j] = fmaf(ty.w[jy], row[ax.address(j)], part[j]);
      }
      MICF_UNROLL
      for (int j = 0; j < kTaps; ++j) col[c][j] = fmaf(tz.w[jz], part[j], col[c][j]);
    }
  }
}

// component c of the displacement at a voxel whose x taps are tx, from the columns of its cell
template <int kTaps>
MICF_HD float displacement(const float (&col)[3][kTaps], int c, const micf_elastic::AxisTaps<kTaps>& tx) {
  float r = 0.0f;
  MICF_UNROLL
  for (int j = 0; j < kTaps; ++j) r = fmaf(tx.w[j], col[c][j], r);
  return r;
}

}  // namespace micf_patch_warp
