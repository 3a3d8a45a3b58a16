// volume_affine.hip -- the volume loader with an affine map in its resample pass (include/micformer_affine.h): every output voxel
// reads the raw CT / MR / label arrays at theta . (its normalised coordinate), F.affine_grid + F.grid_sample(align_corners=False),
// with the normalisation of volume_normalise.hip applied to each tap.  The coordinate, clamp and index arithmetic is
// affine_coords.h's (host-callable); what happens to a source coordinate (taps, label, stores, extents) is affine_taps.h's, shared
// with volume_elastic.hip; everything else but the resample kernel -- the statistics passes, the per-channel normaliser, the host
// sequence (run_stats_loader) -- is volume_normalise_stats.h's and volume_loader_common.h's.
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
#include "affine_taps.h"
#include "../../include/micformer_affine.h"

namespace {

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
    resample_voxel(a, sd, nct, nmr, ct32, mr32, bd, cx, cy, cz, mx, my, mz, v, z, y, x, D, H, W, V, ext, img, label_map);
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
