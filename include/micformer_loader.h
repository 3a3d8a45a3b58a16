/*
 * micformer_loader.h -- C-ABI of the on-device volume loader of libmicformer_hip.so: the head of the reference's input pipeline,
 * everything MMWHS_noCrop_Augment.__getitem__ does between "the raw CT / MR / label arrays are in memory" and the float16
 * (2, D, H, W) image + label of one sample (MMWHS.py:308-405, image_utils.py:48-55).  Conventions are those of micformer_hip.h:
 * device pointers owned by the caller, a caller-provided workspace sized by a pure query, the stream passed explicitly, no
 * allocation or synchronisation inside, 0 or a negative MICF_E* code with argument errors caught before any launch.
 * Kernels: micformer_amd/csrc/volume_loader.hip; rules: DESIGN.md "Volume loader".
 *
 * Per sample, each array with its OWN shape (d, h, w), contiguous, w fastest:
 *   1 min-max normalise each image volume over the whole volume, (x - min) / (max - min), one IEEE fp32 divide per element.
 *     int16: x - min and max - min are formed in int32 (the reference's int16 arithmetic wraps once the range exceeds 32767; the
 *     wrap is NOT reproduced).  A constant volume gives 0 / 0 = NaN everywhere, as the reference does.  NaN inputs: unspecified.
 *   2 trilinear resize (align_corners = false) of each normalised volume to (D, H, W), taps normalised before weighting;
 *     float16 output, channel 0 = CT, channel 1 = MR, slot b of image [B, 2, D, H, W].
 *   3 nearest resize of the CT label + value lookup -> uint8 class map [B, D, H, W]: 0 where the label is 0, k where it equals
 *     label_values[k - 1], 255 where it is any other value (the reference's 8 bool planes have no plane set there).
 *   4 crop_indexes int32 [B, 3, 2]: per axis (max(0, min - 1), max + 1) over the output voxels where the resized (fp32) CT or MR
 *     value is non-zero; (0, 0) on every axis when there is none (the reference raises there).
 * Limits (else MICF_EUNSUPPORTED): every source extent <= 2048, source voxels per array < 2^31, D * H * W <= 512^3.
 */
#ifndef MICFORMER_LOADER_H
#define MICFORMER_LOADER_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_LOADER_I16 0 /* int16: images and labels */
#define MICF_LOADER_F32 1 /* float32: images only */
#define MICF_LOADER_I32 2 /* int32: labels only */

#define MICF_LOADER_MAX_LABEL_VALUES 254

/* One sample.  The pointers are device memory aligned to their element size; `label` is NULL when the call has no label_map. */
typedef struct micf_loader_sample {
  const void* ct;
  const void* mr;
  const void* label;
  int32_t ct_shape[3], mr_shape[3], label_shape[3]; /* (d, h, w) */
  int32_t ct_dtype, mr_dtype, label_dtype;          /* MICF_LOADER_* */
} micf_loader_sample;

/* Workspace bytes of micf_volume_loader for B samples (pure; < 0 for B <= 0): the min / max keys and the crop extents. */
int64_t micf_volume_loader_workspace(int B);

/* `samples` (B entries) and `label_values` (num_label_values entries, distinct, non-zero, at most MICF_LOADER_MAX_LABEL_VALUES)
 * are HOST memory, read during the call only.  label_map NULL = no labels (then every samples[b].label must be NULL too, and with
 * a label_map none may be).  The workspace needs 256-byte alignment.  Launches: zeroing of the workspace, the min / max pass over the raw image
 * volumes, the resize + label + crop pass, the crop finish -- for the whole batch, in chunks of 8 samples. */
int micf_volume_loader(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                       int num_label_values, void* workspace, int64_t workspace_bytes, void* image, uint8_t* label_map,
                       int32_t* crop_indexes, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_LOADER_H */
