// volume_normalise.hip -- the volume loader with a normalisation per channel (include/micformer_normalise.h): min-max as
// volume_loader.hip, z-score over the non-zero voxels (image_utils.py zscore_normalise) or min-max after a clip to two percentiles
// of the positive voxels (image_utils.py irm_min_max_preprocess).  The resize + label + crop pass, the min / max pass and the
// argument checks are volume_loader_common.h's, shared with volume_loader.hip; the statistics kernels (steps 0-4 below), their
// records and the per-channel normaliser of the resize are volume_normalise_stats.h's, shared with volume_affine.hip.
//
// Launch plan of micf_volume_loader_norm (batched over the samples, 8 per launch, no host round trip; which statistics kernels
// run is fixed by the two modes and the dtypes, all host-known):
//   0 zero       the records and the histograms
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
//   6 crop       extents -> crop_indexes
// Everything that crosses threads is an integer count, sum or maximum, or is merged in a fixed order: bit-identical from run to run.
#include "volume_normalise_stats.h"

namespace {

// ---- 6. crop_indexes --------------------------------------------------------------------------------------------------------------
// words != NULL: the extents are the loader-format ones (a call with two min-max channels)
__global__ void norm_crop_kernel(const uint32_t* words, const SampleRec* recs, int B, int D, int H, int W, int32_t* crop) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 3) return;
  crop_body(words ? words + (size_t)(i / 3) * kWsWords + 4 : recs[i / 3].ext, i % 3, D, H, W, crop + i * 2);
}

}  // namespace

extern "C" int64_t micf_volume_loader_norm_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_volume_loader_norm(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                       int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high, void* workspace,
                                       int64_t workspace_bytes, void* image, uint8_t* label_map, int32_t* crop_indexes,
                                       double* stats, micf_stream_t stream) {
  if (!valid_mode(ct_mode) || !valid_mode(mr_mode)) return MICF_EINVAL;
  if (!(0.0 <= p_low && p_low < p_high && p_high <= 100.0)) return MICF_EINVAL;      // (false for NaN)
  if (reinterpret_cast<uintptr_t>(stats) & 7) return MICF_EINVAL;
  const int rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes,
                            B > 0 ? layout(B).total : 0, image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  const Layout L = layout(B);
  char* ws = static_cast<char*>(workspace);
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  SampleRec* recs = reinterpret_cast<SampleRec*>(ws + L.recs);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
  Mom* partials = reinterpret_cast<Mom*>(ws + L.partials);
  const int64_t V = (int64_t)D * H * W;
  const Modes md{{ct_mode, mr_mode}};
  const int64_t zb = (L.zero_words + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(norm_zero_kernel, dim3((unsigned)(zb < 1024 ? zb : 1024)), dim3(kThreads), 0, s,
                     reinterpret_cast<uint32_t*>(ws), L.zero_words);
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  const unsigned rblocks = resize_blocks(V);
  const bool any_minmax = ct_mode == MICF_NORM_MINMAX || mr_mode == MICF_NORM_MINMAX;
  const bool both_minmax = ct_mode == MICF_NORM_MINMAX && mr_mode == MICF_NORM_MINMAX;
  for (int b0 = 0; b0 < B; b0 += kChunk) {
    const int nb = B - b0 < kChunk ? B - b0 : kChunk;
    MinMaxArgs ma;
    const unsigned blocks = pass_blocks(fill_chunk(samples, b0, nb, ma, ra));
    SampleRec* rc0 = recs + b0;
    uint32_t* h0 = hist + (size_t)b0 * 2 * kRanks * kBins;
    Mom* p0 = partials + (size_t)b0 * 2 * kMaxPartials;
    uint32_t* w0 = words + (size_t)b0 * kWsWords;
    __half* img0 = static_cast<__half*>(image) + (size_t)b0 * 2 * V;
    uint8_t* lab0 = label_map ? label_map + (size_t)b0 * V : nullptr;
    launch_statistics(s, ma, md, nb, blocks, p_low, p_high, w0, rc0, h0, p0, stats ? stats + (size_t)b0 * 4 : nullptr);
    const dim3 rgrid(rblocks, (unsigned)nb);
    if (any_minmax) hipLaunchKernelGGL(resize_kernel<LoaderWords>, rgrid, dim3(kThreads), 0, s, ra, D, H, W, w0, img0, lab0);
    if (!both_minmax)
      hipLaunchKernelGGL(resize_kernel<NormWords>, rgrid, dim3(kThreads), 0, s, ra, D, H, W, rc0, img0, any_minmax ? nullptr : lab0);
  }
  hipLaunchKernelGGL(norm_crop_kernel, dim3((unsigned)((B * 3 + 63) / 64)), dim3(64), 0, s, both_minmax ? words : nullptr, recs, B,
                     D, H, W, crop_indexes);
  MICF_RETURN_LAUNCH();
}
