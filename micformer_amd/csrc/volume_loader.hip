// volume_loader.hip -- on-device head of the reference's input pipeline (include/micformer_loader.h): raw CT / MR volumes and the
// CT label of a sample -> float16 image [2, D, H, W], uint8 class map [D, H, W], crop_indexes [3, 2], restated line by line from
// MMWHS_noCrop_Augment.__getitem__ (MMWHS.py:308-405) and normalize (image_utils.py:48-55).
//
// Launch plan of micf_volume_loader (batched over the samples, 8 per launch, no host round trip):
//   0 zero       loader_zero_kernel: the workspace words (all of them are running maxima that start at 0)
//   1 minmax     the one full read of every raw image volume: 128-bit loads, wave + block reduction, two integer atomicMax per block
//                on order-preserving keys (max of key, max of ~key), so the result does not depend on arrival order
//   2 resize     resize_kernel<LoaderWords>, one thread per output voxel: 8 trilinear taps of CT and of MR read in the raw dtype and
//                normalised in registers (one IEEE divide per tap, as the reference normalises before it resizes), fp16 stores; the
//                nearest label gather + value lookup; the extents of the non-zero voxels reduced per block, six integer atomicMax
//                per block
//   3 finish     loader_crop_kernel: extents -> crop_indexes (max(0, min - 1), max + 1), (0, 0) where the image is all zero
// Everything that crosses threads is an integer maximum: the outputs are bit-identical from run to run.
#include "volume_loader_common.h"

namespace {

// ---- 1. min / max of every raw image volume (minmax_body) ----------------------------------------------------------------------
// grid (blocks, volumes).  keys: [sample][kWsWords] words, volume 2 s + c at words 2 c, 2 c + 1 of sample s.
__global__ __launch_bounds__(kThreads) void loader_minmax_kernel(MinMaxArgs a, uint32_t* keys) {
  __shared__ uint32_t s_red[2 * kWaves];
  minmax_body(a.v[blockIdx.y], keys + (size_t)(blockIdx.y >> 1) * kWsWords + 2 * (blockIdx.y & 1), s_red);
}

}  // namespace

extern "C" int64_t micf_volume_loader_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return align256((int64_t)B * kWsWords * 4);
}

extern "C" int micf_volume_loader(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                  int num_label_values, void* workspace, int64_t workspace_bytes, void* image, uint8_t* label_map,
                                  int32_t* crop_indexes, micf_stream_t stream) {
  const int rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes,
                            B > 0 ? align256((int64_t)B * kWsWords * 4) : 0, image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const int64_t V = (int64_t)D * H * W;
  launch_zero(s, ws, (int64_t)B * kWsWords);
  MinMaxArgs ma;
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  for_each_chunk(samples, B, ma, ra, [&](int b0, int nb, unsigned mblocks) {
    uint32_t* wsc = ws + (size_t)b0 * kWsWords;
    hipLaunchKernelGGL(loader_minmax_kernel, dim3(mblocks, (unsigned)(2 * nb)), dim3(kThreads), 0, s, ma, wsc);
    hipLaunchKernelGGL(resize_kernel<LoaderWords>, dim3(resize_blocks(V), (unsigned)nb), dim3(kThreads), 0, s, ra, D, H, W, wsc,
                       static_cast<__half*>(image) + (size_t)b0 * 2 * V, label_map ? label_map + (size_t)b0 * V : nullptr);
  });
  launch_crop(s, ws + 4, kWsWords, B, D, H, W, crop_indexes);
  MICF_RETURN_LAUNCH();
}
