/*
 * micformer_metrics.h -- C-ABI of the surface / overlap evaluation metrics of libmicformer_hip.so: HD95 (percentile Hausdorff
 * distance) and mean IoU, restated from MONAI 1.1's HausdorffDistanceMetric / MeanIoU (the reference's test notebook scores with
 * them).  Conventions are those of micformer_hip.h: device pointers owned by the caller, a caller-provided workspace sized by a
 * pure query, the stream passed explicitly, no allocation or synchronisation inside, 0 or a negative MICF_E* code with argument
 * errors caught before any launch.  Kernels: micformer_amd/csrc/surface_metrics.hip; rules: DESIGN.md "Surface metrics".
 *
 * Inputs (both tensors in the same form):
 *   MICF_FORM_LABEL   uint8 class maps [B, D, H, W]; a voxel is in class c if its label equals c (labels >= K are in no class)
 *   MICF_FORM_ONEHOT  float32 planes [B, K, D, H, W]; a voxel is in class c if plane[b, c] == 1.0f
 * Classes first_class .. K-1 are scored (first_class 1 = MONAI's include_background=False); out is float32 [B, K - first_class].
 * Limits (else MICF_EUNSUPPORTED): K <= 32, every spatial extent <= 1024, min(D, H) <= 512.
 */
#ifndef MICFORMER_METRICS_H
#define MICFORMER_METRICS_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_FORM_LABEL 0
#define MICF_FORM_ONEHOT 1

/* Workspace bytes of micf_hausdorff_distance (pure; < 0 for an invalid shape).  Dominated by two int32 distance fields per (b, c)
 * and four uint32 class-bit masks per voxel: about (8 K + 16) bytes per voxel and sample. */
int64_t micf_surface_metrics_workspace(int B, int K, int D, int H, int W);

/* Percentile Hausdorff distance per (b, c), in voxel units.  percentile 0 = the maximum (MONAI's `percentile=None`); otherwise
 * numpy's linear percentile of the exact edge-to-edge distances, 0 < percentile <= 100.  directed != 0 scores pred -> gt only.
 * nan where both edge sets are empty, +inf where exactly one is. */
int micf_hausdorff_distance(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W, int first_class,
                            double percentile, int directed, void* workspace, int64_t workspace_bytes, float* out,
                            micf_stream_t stream);

/* Workspace bytes of micf_mean_iou (pure; < 0 for an invalid shape). */
int64_t micf_mean_iou_workspace(int B, int K, int D, int H, int W);

/* IoU = |P & G| / |P | G| per (b, c) from exact integer counts.  ignore_empty != 0: nan where |G| = 0; otherwise 1.0 where the union
 * is empty. */
int micf_mean_iou(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W, int first_class, int ignore_empty,
                  void* workspace, int64_t workspace_bytes, float* out, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_METRICS_H */
