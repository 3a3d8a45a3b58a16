/*
 * micformer_restore.h -- C-ABI of the on-device volume restore of libmicformer_hip.so: the inverse of micformer_loader.h.  The
 * [B, K, D, H, W] float32 logits of the network grid go back to each sample's OWN (d, h, w) grid as a label volume in one fused pass:
 * trilinear upsample of the K class planes + argmax over K + class -> label value.  The upsampled [K, d, h, w] tensor is never
 * written.  Conventions are those of micformer_hip.h: device pointers owned by the caller, a caller-provided workspace sized by a
 * pure query, the stream passed explicitly, no allocation or synchronisation inside, 0 or a negative MICF_E* code with argument
 * errors caught before any launch.  Kernels: micformer_amd/csrc/volume_restore.hip; rules: DESIGN.md "Volume restore".
 *
 * Per output voxel (z, y, x) of sample b, logits contiguous with W fastest:
 *   1 per axis, in float32 exactly as torch.nn.functional.interpolate(mode="trilinear", align_corners=False) (the rule the
 *     reference's loader applies in the other direction, MMWHS.py:332):  scale = float(D) / d;
 *     src = max(scale * (o + 0.5f) - 0.5f, 0);  i0 = int(src);  i1 = i0 + (i0 < D - 1);  l1 = src - i0;  l0 = 1 - l1.
 *   2 the eight-tap weighted sum of every class plane (only the order of that sum is this library's own), of
 *     MICF_RESTORE_LOGITS: the logits as they are, or
 *     MICF_RESTORE_PROBS:  softmax over K, evaluated ONCE per voxel of the (D, H, W) grid into the workspace by a pre-pass.
 *   3 argmax over K, the lowest class index winning an exact tie (as torch.argmax on the CPU).  NaN logits: unspecified.
 *   4 the store: MICF_RESTORE_U8 the class index itself; MICF_RESTORE_I16 / _I32 class 0 -> 0, class k -> label_values[k - 1].
 * No atomics: the outputs are bit-identical from run to run.
 * Limits (else MICF_EUNSUPPORTED): 1 <= K <= 32, every output extent <= 2048, output voxels per sample < 2^31, D * H * W <= 512^3.
 */
#ifndef MICFORMER_RESTORE_H
#define MICFORMER_RESTORE_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_RESTORE_U8 0  /* uint8 class map, no lookup: label_values NULL, num_label_values 0 */
#define MICF_RESTORE_I16 1 /* int16 label values (every label value must fit) */
#define MICF_RESTORE_I32 2 /* int32 label values */

#define MICF_RESTORE_LOGITS 0
#define MICF_RESTORE_PROBS 1

#define MICF_RESTORE_MAX_CLASSES 32

/* One sample: `out` is device memory of out_shape[0] * out_shape[1] * out_shape[2] elements of the call's out_dtype, aligned to it. */
typedef struct micf_restore_sample {
  void* out;
  int32_t out_shape[3]; /* (d, h, w) */
} micf_restore_sample;

/* Workspace bytes of micf_volume_restore (pure): 0 for MICF_RESTORE_LOGITS, B * K * D * H * W floats for MICF_RESTORE_PROBS (the
 * softmax at the low-resolution grid); < 0 for bad arguments (MICF_EINVAL, or MICF_EUNSUPPORTED beyond the limits above). */
int64_t micf_volume_restore_workspace(int B, int K, int D, int H, int W, int interpoland);

/* `samples` (B entries) and `label_values` (num_label_values == K - 1 entries, or NULL with 0 for MICF_RESTORE_U8) are HOST memory,
 * read during the call only.  The workspace (4-byte aligned) may be NULL when the query returns 0.  Launches, all on `stream`: for
 * MICF_RESTORE_PROBS the softmax pre-pass over the whole batch, then the fused pass in chunks of 8 samples. */
int micf_volume_restore(const float* logits, int B, int K, int D, int H, int W, const micf_restore_sample* samples, int out_dtype,
                        int interpoland, const int32_t* label_values, int num_label_values, void* workspace,
                        int64_t workspace_bytes, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_RESTORE_H */
