// volume_affine.hip -- the volume loader with an affine map in its resample pass (include/micformer_affine.h): every output voxel
// reads the raw CT / MR / label arrays at theta . (its normalised coordinate), F.affine_grid + F.grid_sample(align_corners=False),
// with the normalisation of volume_normalise.hip applied to each tap.  The coordinate, clamp and index arithmetic is
// affine_coords.h's (host-callable); everything else but the resample kernel -- the statistics passes, the per-channel normaliser,
// the crop extents and label lookup, the host sequence (run_stats_loader) -- is volume_normalise_stats.h's and
// volume_loader_common.h's.
//
// Launch plan of micf_volume_loader_affine (batched over the samples, 8 per launch, no host round trip):
//   0 zero, 1-4 the statistics passes the two modes need and their finish: volume_normalise.hip's plan, unchanged (the statistics
//     are the whole raw volume's, whatever the map)
//   5 resample   resize_kernel's shape: grid (blocks, samples of the chunk), one thread per output voxel, x fastest so the fp16 and
//                uint8 stores coalesce; the sample's 12 or 24 floats of theta read once per block into LDS; per voxel one
//                normalised coordinate, one source coordinate per map, and per array the three indices, the 8 taps normalised in
//                registers (NormAny: every mode in one launch), the nearest label tap + value lookup; the crop extents reduced by
//                resize_kernel's Extents
//   6 crop       loader_crop_kernel on the records: extents -> crop_indexes
// Everything that crosses threads is an integer count, sum or maximum, or is merged in a fixed order: bit-identical from run to run.
#include "volume_normalise_stats.h"
#include "affine_coords.h"
#include "../../include/micformer_affine.h"

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

// ---- 5. resample ------------------------------------------------------------------------------------------------------------------
// grid (blocks, samples of the chunk); recs / theta / image / label_map point at the chunk's first sample.  theta: per sample
// 12 floats, or 24 (per_modality: CT and label read map 0, MR map 1).
__global__ __launch_bounds__(kThreads) void affine_resample_kernel(ResizeArgs a, int D, int H, int W, SampleRec* recs,
                                                                   const float* theta, int per_modality, int border,
                                                                   __half* image, uint8_t* label_map) {
  __shared__ uint32_t s_ext[6];
  __shared__ float s_theta[24];
  const SampleDesc& sd = a.s[blockIdx.y];
  const int tid = threadIdx.x;
  const int V = D * H * W;
  SampleRec* rec = NormWords::sample(recs);
  const bool ct32 = sd.ct.dtype == MICF_LOADER_F32, mr32 = sd.mr.dtype == MICF_LOADER_F32;
  const NormAny nct = NormWords::norm(rec, 0, ct32), nmr = NormWords::norm(rec, 1, mr32);
  __half* img = image + (size_t)blockIdx.y * 2 * V;
  const int nth = per_modality ? 24 : 12;
  if (tid < 6) s_ext[tid] = 0;
  if (tid < 24) s_theta[tid] = theta[(size_t)blockIdx.y * nth + (tid < nth ? tid : tid - 12)];   // (one map: both halves hold it)
  __syncthreads();
  const float* tc = s_theta;
  const float* tm = s_theta + 12;
  const bool bd = border != 0;
  Extents ext;
  for (int v = blockIdx.x * kThreads + tid; v < V; v += gridDim.x * kThreads) {
    const int x = v % W, t = v / W, y = t % H, z = t / H;
    const float nx = micf_affine::norm_coord(x, W), ny = micf_affine::norm_coord(y, H), nz = micf_affine::norm_coord(z, D);
    const float cx = micf_affine::map_row(tc, nx, ny, nz), cy = micf_affine::map_row(tc + 4, nx, ny, nz),
                cz = micf_affine::map_row(tc + 8, nx, ny, nz);
    const float mx = micf_affine::map_row(tm, nx, ny, nz), my = micf_affine::map_row(tm + 4, nx, ny, nz),
                mz = micf_affine::map_row(tm + 8, nx, ny, nz);
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
  ext.flush(s_ext, rec->ext);
}

}  // namespace

extern "C" int64_t micf_volume_loader_affine_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_volume_loader_affine(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                         int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high,
                                         void* workspace, int64_t workspace_bytes, void* image, uint8_t* label_map,
                                         int32_t* crop_indexes, double* stats, const float* affine, int affine_per_modality,
                                         int padding_mode, micf_stream_t stream) {
  if (!affine || (reinterpret_cast<uintptr_t>(affine) & 3)) return MICF_EINVAL;
  if (affine_per_modality != 0 && affine_per_modality != 1) return MICF_EINVAL;
  if (padding_mode != MICF_PAD_ZEROS && padding_mode != MICF_PAD_BORDER) return MICF_EINVAL;
  int rc = check_norm_args(ct_mode, mr_mode, p_low, p_high, stats);
  if (rc != MICF_OK) return rc;
  rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes, B > 0 ? layout(B).total : 0,
                  image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  const int nth = affine_per_modality ? 24 : 12;
  return run_stats_loader(samples, B, D, H, W, label_values, num_label_values, Modes{{ct_mode, mr_mode}}, p_low, p_high, workspace,
                          image, label_map, crop_indexes, stats, s, false,
                          [&](const ResizeArgs& ra, const WsView& c, int b0, dim3 grid, __half* img0, uint8_t* lab0) {
                            hipLaunchKernelGGL(affine_resample_kernel, grid, dim3(kThreads), 0, s, ra, D, H, W, c.recs,
                                               affine + (size_t)b0 * nth, affine_per_modality, padding_mode, img0, lab0);
                          });
}
