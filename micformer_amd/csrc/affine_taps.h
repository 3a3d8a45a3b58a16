// affine_taps.h -- what volume_affine.hip's and volume_elastic.hip's resample kernels do with a normalised source coordinate once
// they have it (include/micformer_affine.h from "s" on): the index per axis of an array, the 8 trilinear taps normalised before
// they are weighted, the nearest label tap + value lookup, the stores and the crop extents.  Moved here from volume_affine.hip
// with its arithmetic unchanged.  Unnamed namespace: each including file gets its own copy.
#pragma once
#include "volume_normalise_stats.h"
#include "affine_coords.h"

namespace {

using micf_affine::LinearTaps;

struct AxisIndex { float z, y, x; };

// index of the normalised source coordinate (sx, sy, sz) in an array of shape (d, h, w)
__device__ __forceinline__ AxisIndex source_indices(const Vol3& v, float sx, float sy, float sz) {
  return AxisIndex{micf_affine::source_index(sz, v.d), micf_affine::source_index(sy, v.h), micf_affine::source_index(sx, v.w)};
}

// separable trilinear sum over the 8 taps, w fastest (trilinear()'s order); a tap outside the array counts 0
template <bool F32>
__device__ __forceinline__ float affine_trilinear(const Vol3& v, const NormAny& nm, const AxisIndex& i, bool border) {
  const LinearTaps tz = micf_affine::linear_taps(i.z, v.d, border);
  const LinearTaps ty = micf_affine::linear_taps(i.y, v.h, border);
  const LinearTaps tx = micf_affine::linear_taps(i.x, v.w, border);
  const int64_t r00 = ((int64_t)tz.i0 * v.h + ty.i0) * v.w, r01 = ((int64_t)tz.i0 * v.h + ty.i1) * v.w;
  const int64_t r10 = ((int64_t)tz.i1 * v.h + ty.i0) * v.w, r11 = ((int64_t)tz.i1 * v.h + ty.i1) * v.w;
  const bool i00 = tz.in0 && ty.in0, i01 = tz.in0 && ty.in1, i10 = tz.in1 && ty.in0, i11 = tz.in1 && ty.in1;
  const float a00 = i00 && tx.in0 ? tap<F32>(v.p, r00 + tx.i0, nm) : 0.0f, b00 = i00 && tx.in1 ? tap<F32>(v.p, r00 + tx.i1, nm) : 0.0f;
  const float a01 = i01 && tx.in0 ? tap<F32>(v.p, r01 + tx.i0, nm) : 0.0f, b01 = i01 && tx.in1 ? tap<F32>(v.p, r01 + tx.i1, nm) : 0.0f;
  const float a10 = i10 && tx.in0 ? tap<F32>(v.p, r10 + tx.i0, nm) : 0.0f, b10 = i10 && tx.in1 ? tap<F32>(v.p, r10 + tx.i1, nm) : 0.0f;
  const float a11 = i11 && tx.in0 ? tap<F32>(v.p, r11 + tx.i0, nm) : 0.0f, b11 = i11 && tx.in1 ? tap<F32>(v.p, r11 + tx.i1, nm) : 0.0f;
  const float t00 = a00 * tx.w0 + b00 * tx.w1, t01 = a01 * tx.w0 + b01 * tx.w1;
  const float t10 = a10 * tx.w0 + b10 * tx.w1, t11 = a11 * tx.w0 + b11 * tx.w1;
  const float u0 = t00 * ty.w0 + t01 * ty.w1, u1 = t10 * ty.w0 + t11 * ty.w1;
  return u0 * tz.w0 + u1 * tz.w1;
}

// One output voxel v = (z, y, x) of the block's sample, from the source coordinates of CT + label (cx, cy, cz) and of MR
// (mx, my, mz): both image planes, the crop extents, the class.  img points at the sample's first element, label_map at that of
// the chunk's first sample.
__device__ __forceinline__ void resample_voxel(const ResizeArgs& a, const SampleDesc& sd, const NormAny& nct, const NormAny& nmr,
                                               bool ct32, bool mr32, bool bd, float cx, float cy, float cz, float mx, float my,
                                               float mz, int v, int z, int y, int x, int D, int H, int W, int V, Extents& ext,
                                               __half* img, uint8_t* label_map) {
  const bool cok = micf_affine::finite(cx) && micf_affine::finite(cy) && micf_affine::finite(cz);
  const bool mok = micf_affine::finite(mx) && micf_affine::finite(my) && micf_affine::finite(mz);
  float c0 = 0.0f, c1 = 0.0f;
  if (cok) {
    const AxisIndex i = source_indices(sd.ct, cx, cy, cz);
    c0 = ct32 ? affine_trilinear<true>(sd.ct, nct, i, bd) : affine_trilinear<false>(sd.ct, nct, i, bd);
  }
  if (mok) {
    const AxisIndex i = source_indices(sd.mr, mx, my, mz);
    c1 = mr32 ? affine_trilinear<true>(sd.mr, nmr, i, bd) : affine_trilinear<false>(sd.mr, nmr, i, bd);
  }
  img[v] = __float2half_rn(c0);
  img[(size_t)V + v] = __float2half_rn(c1);
  if (c0 != 0.0f || c1 != 0.0f) ext.see(z, y, x, D, H, W);       // (true for NaN, as numpy's `!= 0`)
  if (label_map) {
    const Vol3& lv = sd.lab;
    int val = 0;                                               // outside the array, or a non-finite coordinate: raw label 0
    if (cok) {
      const AxisIndex i = source_indices(lv, cx, cy, cz);
      bool inz, iny, inx;
      const int sz = micf_affine::nearest_tap(i.z, lv.d, bd, inz), sy = micf_affine::nearest_tap(i.y, lv.h, bd, iny),
                sx = micf_affine::nearest_tap(i.x, lv.w, bd, inx);
      if (inz && iny && inx) val = raw_label(lv, ((int64_t)sz * lv.h + sy) * lv.w + sx);
    }
    label_map[(size_t)blockIdx.y * V + v] = (uint8_t)label_class(a, val);
  }
}

}  // namespace
