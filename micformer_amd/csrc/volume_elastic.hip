// volume_elastic.hip -- the volume loader with a displacement field, and optionally an affine map, in its resample pass
// (include/micformer_elastic.h): every output voxel's normalised coordinate n is moved by the field interpolated on its control grid,
// u, and the raw CT / MR / label arrays are read at theta . (n + u, 1).  The control-cell, fraction and weight arithmetic is
// elastic_coords.h's and the map's is affine_coords.h's (both host-callable); what happens to a source coordinate (taps, label,
// stores, extents) is affine_taps.h's, shared with volume_affine.hip; the statistics passes, the normaliser and the host sequence
// (run_stats_loader) are volume_normalise_stats.h's and volume_loader_common.h's.
//
// Launch plan of micf_volume_loader_elastic: volume_affine.hip's, with its step 5 replaced by
//   5 resample   elastic_resample_kernel, affine_resample_kernel's shape: grid (blocks, samples of the chunk), one thread per output
//                voxel, x fastest; theta (or the identity, when the call has no map) once per block into LDS; per voxel n, the
//                control cell and fraction of each axis in integers, u from 8 (linear) or 64 (cubic) control points per component
//                -- the cubic's as a rolled loop over its four planes, 16 taps each -- then one source coordinate per map and
//                affine_taps.h's resample_voxel
//
// The field is read through the caches, not staged in LDS.  Why: one path serves every grid from 2^3 to the dense 128^3 (25 MB per
// sample, which no LDS holds), so there is no size threshold with a second kernel behind it to test and to keep bit-equal.  On the
// coarse grids where staging could pay, the 64 x-adjacent voxels of a wave lie in one or two control cells: their tap loads carry at
// most two distinct addresses per instruction, all in the one or two cache lines a 7-point row occupies, and the whole 4 KB field
// stays resident in each CU's vector L1.  What staging would save is the address arithmetic of those loads, not memory traffic.
// Everything that crosses threads is an integer maximum: bit-identical from run to run.
#include "affine_taps.h"
#include "elastic_coords.h"
#include "../../include/micformer_elastic.h"

namespace {

constexpr int kMaxGrid = 512;

struct Displacement { float x, y, z; };

// u at output voxel (z, y, x): the three components of the sample's field, each gd * gh * gw floats, x first
template <int kTaps, class T>
__device__ __forceinline__ Displacement displacement_at(const float* field, int gd, int gh, int gw, const T& tz, const T& ty,
                                                        const T& tx) {
  const size_t plane = (size_t)gd * gh * gw;
  return Displacement{micf_elastic::interpolate<kTaps>(field, tz, ty, tx), micf_elastic::interpolate<kTaps>(field + plane, tz, ty, tx),
                      micf_elastic::interpolate<kTaps>(field + 2 * plane, tz, ty, tx)};
}

// ---- 5. resample ------------------------------------------------------------------------------------------------------------------
// grid (blocks, samples of the chunk); recs / theta / field / image / label_map point at the chunk's first sample.  theta: NULL
// (the identity), or per sample 12 floats, or 24 (per_modality: CT and label read map 0, MR map 1).  field: per sample
// [3][gd][gh][gw].
__global__ __launch_bounds__(kThreads) void elastic_resample_kernel(ResizeArgs a, int D, int H, int W, SampleRec* recs,
                                                                    const float* theta, int per_modality, int border,
                                                                    const float* field, int gd, int gh, int gw, int cubic,
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
  const float* fld = field + (size_t)blockIdx.y * 3 * gd * gh * gw;
  const int nth = per_modality ? 24 : 12;
  if (tid < 6) s_ext[tid] = 0;
  if (tid < 24) {
    const int e = tid < 12 ? tid : tid - 12;                       // element of a [3][4] map
    s_theta[tid] = theta ? theta[(size_t)blockIdx.y * nth + (tid < nth ? tid : tid - 12)] : (e % 5 == 0 ? 1.0f : 0.0f);
  }
  __syncthreads();
  const float* tc = s_theta;
  const float* tm = s_theta + 12;
  const bool bd = border != 0;
  Extents ext;
  for (int v = blockIdx.x * kThreads + tid; v < V; v += gridDim.x * kThreads) {
    const int x = v % W, t = v / W, y = t % H, z = t / H;
    const micf_elastic::Cell kz = micf_elastic::control_cell(z, D, gd), ky = micf_elastic::control_cell(y, H, gh),
                             kx = micf_elastic::control_cell(x, W, gw);
    const Displacement u = cubic ? displacement_at<4>(fld, gd, gh, gw, micf_elastic::cubic_taps(kz, gd),
                                                      micf_elastic::cubic_taps(ky, gh), micf_elastic::cubic_taps(kx, gw))
                                 : displacement_at<2>(fld, gd, gh, gw, micf_elastic::linear_taps(kz, gd),
                                                      micf_elastic::linear_taps(ky, gh), micf_elastic::linear_taps(kx, gw));
    const float nx = micf_affine::norm_coord(x, W) + u.x, ny = micf_affine::norm_coord(y, H) + u.y,
                nz = micf_affine::norm_coord(z, D) + u.z;
    const float cx = micf_affine::map_row(tc, nx, ny, nz), cy = micf_affine::map_row(tc + 4, nx, ny, nz),
                cz = micf_affine::map_row(tc + 8, nx, ny, nz);
    const float mx = micf_affine::map_row(tm, nx, ny, nz), my = micf_affine::map_row(tm + 4, nx, ny, nz),
                mz = micf_affine::map_row(tm + 8, nx, ny, nz);
    resample_voxel(a, sd, nct, nmr, ct32, mr32, bd, cx, cy, cz, mx, my, mz, v, z, y, x, D, H, W, V, ext, img, label_map);
  }
  ext.flush(s_ext, rec->ext);
}

}  // namespace

extern "C" int64_t micf_volume_loader_elastic_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_volume_loader_elastic(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                          int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high,
                                          void* workspace, int64_t workspace_bytes, void* image, uint8_t* label_map,
                                          int32_t* crop_indexes, double* stats, const float* affine, int affine_per_modality,
                                          int padding_mode, const float* displacement, int gd, int gh, int gw,
                                          int field_interpolation, micf_stream_t stream) {
  if (!displacement || (reinterpret_cast<uintptr_t>(displacement) & 3)) return MICF_EINVAL;
  if (gd < 2 || gh < 2 || gw < 2) return MICF_EINVAL;
  if (field_interpolation != MICF_FIELD_LINEAR && field_interpolation != MICF_FIELD_CUBIC) return MICF_EINVAL;
  if (reinterpret_cast<uintptr_t>(affine) & 3) return MICF_EINVAL;
  if (affine_per_modality != 0 && affine_per_modality != 1) return MICF_EINVAL;
  if (padding_mode != MICF_PAD_ZEROS && padding_mode != MICF_PAD_BORDER) return MICF_EINVAL;
  int rc = check_norm_args(ct_mode, mr_mode, p_low, p_high, stats);
  if (rc != MICF_OK) return rc;
  rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes, B > 0 ? layout(B).total : 0,
                  image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;
  if (gd > kMaxGrid || gh > kMaxGrid || gw > kMaxGrid) return MICF_EUNSUPPORTED;

  hipStream_t s = (hipStream_t)stream;
  const int nth = affine_per_modality ? 24 : 12;
  const size_t per_sample = (size_t)3 * gd * gh * gw;
  return run_stats_loader(samples, B, D, H, W, label_values, num_label_values, Modes{{ct_mode, mr_mode}}, p_low, p_high, workspace,
                          image, label_map, crop_indexes, stats, s, false,
                          [&](const ResizeArgs& ra, const WsView& c, int b0, dim3 grid, __half* img0, uint8_t* lab0) {
                            hipLaunchKernelGGL(elastic_resample_kernel, grid, dim3(kThreads), 0, s, ra, D, H, W, c.recs,
                                               affine ? affine + (size_t)b0 * nth : nullptr, affine_per_modality, padding_mode,
                                               displacement + (size_t)b0 * per_sample, gd, gh, gw,
                                               (int)(field_interpolation == MICF_FIELD_CUBIC), img0, lab0);
                          });
}
