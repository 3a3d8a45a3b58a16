/*
 * micformer_normalise.h -- C-ABI of the volume loader with a choice of intensity normalisation per channel: the loader of
 * micformer_loader.h (same samples, same outputs, same limits) with the reference's other two normalisations next to min-max,
 * zscore_normalise and irm_min_max_preprocess (dataset/image_utils.py).  Conventions are those of micformer_hip.h: device
 * pointers owned by the caller, a caller-provided workspace sized by a pure query, the stream passed explicitly, no allocation or
 * synchronisation inside, 0 or a negative MICF_E* code with argument errors caught before any launch.
 * Kernels: micformer_amd/csrc/volume_normalise.hip; rules: DESIGN.md "Volume loader".
 *
 * The normaliser of a channel (ct_mode for channel 0, mr_mode for channel 1), applied to every raw element x before the trilinear
 * weighting, in float32 with one IEEE divide per element; its two constants are float64 statistics of the whole raw volume,
 * rounded to float32 once:
 *   MICF_NORM_MINMAX      (x - min) / (max - min), exactly as micf_volume_loader (same arithmetic, same bits).
 *   MICF_NORM_ZSCORE      x != 0 ? (x - mean) / std : 0, mean and population std (sqrt(mean((x - mean)^2))) over the elements with
 *                         x != 0 (-0.0f counts as zero).  int16: exact integer sums.  float32: float64 sums over a fixed
 *                         partition of the volume, merged in a fixed order.
 *   MICF_NORM_PERCENTILE  (clamp(x, low, high) - low) / (high - low) with low, high = numpy.percentile(x[x > 0], [p_low, p_high])
 *                         under numpy's default "linear" rule: virtual index h = (n - 1) * (p / 100), k = floor(h), t = h - k, value
 *                         v[k] + (v[k + 1] - v[k]) * t in float64 (formed from the upper end, v[k + 1] - (v[k + 1] - v[k]) * (1 - t),
 *                         when t >= 0.5, as numpy does); the order statistics come from a radix select, exactly.
 * Edge rules (what the reference's functions return where they return something):
 *   z-score of an all-zero volume: all zeros.  z-score of a constant non-zero value: NaN at the non-zero elements, 0 at the zeros.
 *   percentile with high == low (one positive element is such a case): NaN everywhere.  Percentile with no positive element:
 *   NaN everywhere (the reference raises).  NaN or inf in the input: unspecified.
 * One deviation joins the loader's two: zscore_normalise writes its float result back into the input array, which truncates it
 * to integers for an int16 array; that is NOT reproduced, an int16 volume is z-scored as if converted to float32 first.
 * Every value that crosses threads is an integer count, an integer sum or an integer maximum, or is combined in a fixed order:
 * the outputs are bit-identical from run to run and do not depend on the other samples of the batch.
 */
#ifndef MICFORMER_NORMALISE_H
#define MICFORMER_NORMALISE_H

#include "micformer_loader.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_NORM_MINMAX 0
#define MICF_NORM_ZSCORE 1
#define MICF_NORM_PERCENTILE 2

/* Workspace bytes of micf_volume_loader_norm for B samples (pure; < 0 for B <= 0): per (sample, channel) the statistics record,
 * the histograms of the select and the partial moments. */
int64_t micf_volume_loader_norm_workspace(int B);

/* The arguments of micf_volume_loader with the same meaning, and: ct_mode / mr_mode one of MICF_NORM_*, the same for every sample
 * of the call; 0 <= p_low < p_high <= 100 (read by the percentile mode only, checked always); stats NULL or device memory for
 * float64 [B, 2, 2], per (sample, channel) the normaliser's two statistics: (min, max), (mean, std) or (low, high).
 * Launches, fixed by the arguments (so the call can be captured in a graph): zeroing of the workspace; per chunk of 8 samples
 * the statistics passes its modes need (min / max; moments; histogram + scan for each digit of the select, two digits for a chunk
 * whose percentile volumes are all int16, else three), the finish of the statistics, the resize + label + crop pass (for a call
 * with a min-max channel two launches: the loader's own kernel instance writes that channel's plane, so that it carries the
 * loader's bits, then the per-channel instance writes the other plane and the crop extents); the crop finish. */
int micf_volume_loader_norm(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                            int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high, void* workspace,
                            int64_t workspace_bytes, void* image, uint8_t* label_map, int32_t* crop_indexes, double* stats,
                            micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_NORMALISE_H */
