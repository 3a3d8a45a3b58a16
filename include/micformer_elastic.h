/*
 * micformer_elastic.h -- C-ABI of the volume loader with a displacement field (and optionally an affine map) in its resample
 * pass: the loader of micformer_affine.h (same samples, normalisations, statistics, padding modes and limits) whose output voxel
 * is first moved by a smooth non-rigid deformation: elastic augmentation on a coarse random control grid, or the dense field of a
 * registration network.  Deformation and map are composed in the one pass that reads the raw scan: the image is interpolated
 * once and the label sees one nearest-neighbour rounding.  Conventions are those of micformer_hip.h.  Kernel:
 * micformer_amd/csrc/volume_elastic.hip, control-grid arithmetic: micformer_amd/csrc/elastic_coords.h; rules: DESIGN.md "Volume
 * loader".
 *
 * The field: float32 [B][3][gd][gh][gw], components in (x, y, z) order (x along W, as F.grid_sample's last dimension), in
 * NORMALISED OUTPUT coordinates (2 = the whole axis), on a control grid whose corner points sit on the centres of the first and
 * last output voxel of each axis (align_corners=True with respect to the output grid).  For output voxel (z, y, x) of (D, H, W):
 *     n = ((2 x + 1) / W - 1, (2 y + 1) / H - 1, (2 z + 1) / D - 1)                                   (micformer_affine.h's)
 *     u = the field interpolated at the control position p = o (g - 1) / (out - 1) per axis            (out == 1: p = 0)
 *     s = theta . (n + u, 1)                                                     (theta = the identity when no map is given)
 * and everything after s is micformer_affine.h's word for word: the source index per array, the trilinear image taps normalised
 * before they are weighted, the nearest (half-to-even) label tap and value lookup, MICF_PAD_ZEROS / MICF_PAD_BORDER, crop_indexes,
 * the statistics of the whole raw volume whatever the field and the map, and a non-finite s giving image 0 and class 0.
 * The deformation lives in the common output frame and is applied BEFORE the map: with a map per modality, CT, label and MR see
 * the same deformation and then each its own map.
 *   MICF_FIELD_LINEAR  trilinear over the 8 control points of the cell k = floor(p): interpolates the control values; with
 *                      g == out on every axis it is one vector per output voxel.  F.interpolate(field, size=(D, H, W),
 *                      mode="trilinear", align_corners=True).
 *   MICF_FIELD_CUBIC   the uniform cubic B-spline over the 4 x 4 x 4 control points k - 1 ... k + 2, indices clamped to
 *                      [0, g - 1], weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 of t = p - k: approximates
 *                      the control values (does not interpolate them) and is C2, so a coarse random grid gives a deformation
 *                      without kinks at the control planes.  scipy.ndimage.map_coordinates(order=3, mode="nearest",
 *                      prefilter=False).
 * k and the numerator of t are computed in integers (k = o (g - 1) / (out - 1), r = o (g - 1) % (out - 1), t = (float) r /
 * (float) (out - 1)): the cell is exact and t carries one rounding.  u is a separable sum, x innermost, one fused multiply-add per
 * tap; a control point is weighted even where its weight is 0, so a NaN or inf entry reaches every voxel whose taps include it.
 * Every control-point address lies in [0, g) whatever the inputs, and s is clamped as micformer_affine.h says: no field produces
 * an address outside the field or the arrays.  float32 throughout; for |u| <= 0.25 and a map with row sums <= 1.5 the source
 * index is within extent * 2^-19 of its exact value (the affine arithmetic's extent * 2^-20, plus the rounding of n + u and
 * those of u through the map).
 * Outputs are bit-identical from run to run and do not depend on the other samples of the batch; no float atomics, no host round
 * trip, no scratch.  With an all-zero field the outputs are micf_volume_loader_affine's bit for bit (n + 0 = n).
 */
#ifndef MICFORMER_ELASTIC_H
#define MICFORMER_ELASTIC_H

#include "micformer_affine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_FIELD_LINEAR 0
#define MICF_FIELD_CUBIC 1

/* Workspace bytes of micf_volume_loader_elastic for B samples (pure; < 0 for B <= 0). */
int64_t micf_volume_loader_elastic_workspace(int B);

/* The arguments of micf_volume_loader_affine in the same order and with the same meaning, except that affine may be NULL (the
 * identity for every sample and modality; affine_per_modality must still be 0 or 1), and: displacement, device memory, float32
 * [B][3][gd][gh][gw], read on the device when the kernel runs; field_interpolation one of MICF_FIELD_*.
 * MICF_EINVAL before any launch for a NULL or misaligned field, a grid extent below 2, an unknown interpolation or any of
 * micf_volume_loader_affine's conditions (a misaligned non-NULL map among them); MICF_EUNSUPPORTED for a grid extent above 512.
 * Launches, fixed by the arguments (so the call can be captured in a graph, and a replay picks up new contents of `displacement`
 * and `affine`): those of micf_volume_loader_affine -- the zeroing, the statistics passes, per chunk of 8 samples ONE resample
 * launch, the crop finish. */
int micf_volume_loader_elastic(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                               int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high, void* workspace,
                               int64_t workspace_bytes, void* image, uint8_t* label_map, int32_t* crop_indexes, double* stats,
                               const float* affine, int affine_per_modality, int padding_mode, const float* displacement, int gd,
                               int gh, int gw, int field_interpolation, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_ELASTIC_H */
