/*
 * micformer_surface.h -- C-ABI of the surface distances in physical units of libmicformer_hip.so: percentile Hausdorff distance,
 * average (symmetric) surface distance and surface Dice at a tolerance, on a grid with a voxel spacing per sample.  Conventions
 * are those of micformer_hip.h: device pointers owned by the caller, a caller-provided workspace sized by a pure query, the
 * stream passed explicitly, no allocation or synchronisation inside, 0 or a negative MICF_E* code with argument errors caught
 * before any launch.  Kernels: micformer_amd/csrc/surface_distance.hip; rules: DESIGN.md "Surface distances in millimetres".
 *
 * Inputs (both tensors in the same form):
 *   MICF_FORM_LABEL       uint8 class maps [B, D, H, W]                      (micformer_metrics.h)
 *   MICF_FORM_ONEHOT      float32 planes [B, K, D, H, W]                     (micformer_metrics.h)
 *   MICF_FORM_VALUES_I16  int16 label volumes [B, D, H, W]: a voxel is in class k >= 1 if it equals label_values[k - 1], every
 *   MICF_FORM_VALUES_I32  int32 ...                         other value (0 included) is class 0
 * Classes first_class .. K-1 are scored; Kc = K - first_class below.
 * Limits (else MICF_EUNSUPPORTED): K <= 32, every spatial extent <= 1024, min(D, H) <= 512, B <= MICF_SURFACE_MAX_BATCH, every
 * spacing within [2^-256, 2^256].
 */
#ifndef MICFORMER_SURFACE_H
#define MICFORMER_SURFACE_H

#include "micformer_metrics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_FORM_VALUES_I16 2
#define MICF_FORM_VALUES_I32 3

#define MICF_SURFACE_MAX_PERCENTILES 4
#define MICF_SURFACE_MAX_BATCH 64

/* Workspace bytes of micf_surface_distance (pure; < 0 for an invalid shape): about (8 K + 18) bytes per voxel and sample. */
int64_t micf_surface_distance_workspace(int B, int K, int D, int H, int W);

/* Surface distances per (b, c) with the edge sets of micf_hausdorff_distance and, per sample b, the spacing
 * (s_z, s_y, s_x) = spacing[3 b .. 3 b + 2] (host, float64, each > 0 and finite).  The distance of a source edge voxel is
 * sqrt(min over the target edge voxels of ((s_z dz)^2 + (s_y dy)^2) + (s_x dx)^2), evaluated in float64 in that order.
 *   label_values      host, num_label_values = K - 1 distinct non-zero values for the two VALUES forms; NULL / 0 otherwise
 *   percentiles       host, num_percentiles in 1..MICF_SURFACE_MAX_PERCENTILES values in [0, 100]; 0 = the maximum, otherwise
 *                     numpy's linear percentile
 *   thresholds        host, Kc tolerances >= 0 in the spacing's unit (class first_class first), or NULL: no surface Dice
 * All host arrays are read before the call returns.  With P = num_percentiles, out is float32, C-contiguous sections in this order:
 *   hd           [B][Kc][P]   max of both directions' percentile distance; nan where both edge sets are empty, +inf where one is
 *   hd_directed  [B][Kc][P]   pred -> gt only, same rules
 *   asd          [B][Kc][2]   mean distance pred -> gt, gt -> pred; nan where the source set is empty, else +inf where the target is
 *   assd         [B][Kc]      (sum of both directions' distances) / (both edge counts); nan / +inf as hd
 *   nsd          [B][Kc]      (distances <= threshold, both directions) / (both edge counts); nan where both sets are empty, 0
 *                             where one is.  Not written when thresholds is NULL.
 * i.e. B * Kc * (2 P + 4) floats.  Every value is bit-identical from run to run. */
int micf_surface_distance(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W, int first_class,
                          const int32_t* label_values, int num_label_values, const double* spacing, const double* percentiles,
                          int num_percentiles, const double* thresholds, void* workspace, int64_t workspace_bytes, float* out,
                          micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_SURFACE_H */
