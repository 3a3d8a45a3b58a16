// volume_normalise.hip -- the volume loader with a normalisation per channel (include/micformer_normalise.h): min-max as
// volume_loader.hip, z-score over the non-zero voxels (image_utils.py zscore_normalise) or min-max after a clip to two percentiles
// of the positive voxels (image_utils.py irm_min_max_preprocess).  The kernels and the host sequence (run_stats_loader) are
// volume_loader_common.h's and volume_normalise_stats.h's; this file has the plan, the entry point and its resize step.
//
// Launch plan of micf_volume_loader_norm (batched over the samples, 8 per launch, no host round trip; which statistics kernels
// run is fixed by the two modes and the dtypes, all host-known):
//   0 zero       loader_zero_kernel: the loader-format words, the records and the histograms
//   1 minmax     min-max channels: volume_loader.hip's pass (integer atomicMax on keys)
//   2 moments    z-score channels, one read.  int16: count, sum x, sum x^2 as integers, wave + block reduction, three 64-bit integer
//                atomicAdd per block.  float32: every thread sums d = x - c and d^2 in float64 about its own first non-zero element c
//                (no cancellation against the mean), turns that into (n, mean, M2), and the triples are merged (Chan's update) along
//                a fixed tree: lanes, waves, then one partial per block; the partition of a volume depends on that volume alone
//   3 hist/scan  percentile channels, one read per digit of the key (11 + 11 + 10 bits; the int16 key sits in the top 16, so two
//                digits do): a most-significant-digit-first radix select of up to four ranks (k_low, k_low + 1, k_high, k_high + 1)
//                together.  hist: histogram of the digit over the positive voxels whose higher digits equal a rank's prefix, in LDS
//                (integer ds_add), one flush per block (integer atomicAdd).  scan: one block per volume finds each rank's bin,
//                extends its prefix, reduces its rank to the rank inside the bin, clears the histograms; ranks with equal prefixes
//                share one histogram.  The first scan also totals the positives (n) and derives the ranks from it
//   4 finish     one wave per volume: the float32 partial moments merged in a fixed order; mean / std, low / high (numpy's linear
//                interpolation in float64), min / max -> the channel's two float32 constants and the optional float64 `stats`
//   5 resize     volume_loader_common.h's kernel with the per-channel normaliser below.  A min-max channel must carry the bits
//                micf_volume_loader gives it, and those depend on how the compiler contracts the trilinear sums of that kernel
//                instance; so where a call has a min-max channel, resize_kernel<LoaderWords> -- the loader's own instance, on a
//                loader-format block of words at the head of the workspace -- writes the image, the label map and (for a
//                (minmax, minmax) call with `stats`) the crop extents, and the instance below then writes the plane of the other
//                channel and the crop extents of the pair; calls without a min-max channel run the instance below alone
//   6 crop       loader_crop_kernel: extents -> crop_indexes, from the loader-format words of a (minmax, minmax) call, else the records
// Everything that crosses threads is an integer count, sum or maximum, or is merged in a fixed order: bit-identical from run to run.
#include "volume_normalise_stats.h"

extern "C" int64_t micf_volume_loader_norm_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_volume_loader_norm(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                       int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high, void* workspace,
                                       int64_t workspace_bytes, void* image, uint8_t* label_map, int32_t* crop_indexes,
                                       double* stats, micf_stream_t stream) {
  int rc = check_norm_args(ct_mode, mr_mode, p_low, p_high, stats);
  if (rc != MICF_OK) return rc;
  rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes, B > 0 ? layout(B).total : 0,
                  image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  const bool any_minmax = ct_mode == MICF_NORM_MINMAX || mr_mode == MICF_NORM_MINMAX;
  const bool both_minmax = ct_mode == MICF_NORM_MINMAX && mr_mode == MICF_NORM_MINMAX;
  return run_stats_loader(
      samples, B, D, H, W, label_values, num_label_values, Modes{{ct_mode, mr_mode}}, p_low, p_high, workspace, image, label_map,
      crop_indexes, stats, s, both_minmax,
      [&](const ResizeArgs& ra, const WsView& c, int, dim3 grid, __half* img0, uint8_t* lab0) {
        if (any_minmax) hipLaunchKernelGGL(resize_kernel<LoaderWords>, grid, dim3(kThreads), 0, s, ra, D, H, W, c.words, img0, lab0);
        if (!both_minmax)
          hipLaunchKernelGGL(resize_kernel<NormWords>, grid, dim3(kThreads), 0, s, ra, D, H, W, c.recs, img0,
                             any_minmax ? nullptr : lab0);
      });
}
