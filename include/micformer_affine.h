/*
 * micformer_affine.h -- C-ABI of the volume loader with an affine map in its resample pass: the loader of micformer_normalise.h
 * (same samples, same normalisations, same statistics, same limits) whose output voxel reads the raw volumes at an affinely
 * mapped place: rotate / zoom / translate augmentation, a re-orientation (a signed permutation) or a registration of one
 * modality, in the one pass that reads the raw scan.  Nothing intermediate is written and the image is interpolated once.
 * Conventions are those of micformer_hip.h.  Kernels: micformer_amd/csrc/volume_affine.hip, coordinate arithmetic:
 * micformer_amd/csrc/affine_coords.h; rules: DESIGN.md "Volume loader".
 *
 * The map is F.affine_grid + F.grid_sample(align_corners=False): theta, float32 [3][4] per sample (or per sample and modality),
 * acts on the normalised OUTPUT coordinate and gives the normalised SOURCE coordinate (nothing is inverted; (x, y, z) order, x
 * along W).  For output voxel (z, y, x) of (D, H, W):
 *     n = ((2 x + 1) / W - 1, (2 y + 1) / H - 1, (2 z + 1) / D - 1)          s = theta . (n, 1)
 * and for a source array of shape (d, h, w) the index on an axis of `extent` elements is i = ((s + 1) * extent - 1) / 2.  One map
 * serves arrays of different shapes (CT, MR and label of a sample may all differ), because it lives in normalised coordinates.
 * float32 throughout, each multiply-add fused; the index is within extent * 2^-20 of its exact value for |s| <= a few units.
 *   Image   trilinear over the 8 taps around i, each tap normalised (micformer_normalise.h) before it is weighted, float16 result.
 *           MICF_PAD_ZEROS: a tap outside the array contributes 0.  MICF_PAD_BORDER: i is clamped to [0, extent - 1] first.
 *   Label   nearest = round-half-to-even of i, then the loader's value lookup (0 / k / 255).  MICF_PAD_ZEROS: outside the array
 *           the raw label counts as 0, i.e. class 0.  MICF_PAD_BORDER: the rounded index is clamped.  NOTE: with the identity map
 *           this is NOT micf_volume_loader's label, which is F.interpolate(mode="nearest") = floor(o * in / out); only the image
 *           agrees with the plain loader under the identity map, and only under MICF_PAD_BORDER.
 *   crop_indexes   the loader's rule on the resampled float32 values.
 *   A non-finite s on any axis gives image 0 and class 0 in both modes.  A finite s, however large, is clamped in float before any
 *   conversion to int: no map produces an address outside the arrays.
 * The statistics of the normalisers do not depend on the map: they are the whole raw volume's, computed by the passes of
 * micf_volume_loader_norm (same bits in `stats`).  A min-max channel is normalised by the same arithmetic as in the loader, but
 * its trilinear sum is this kernel's own: its bits are not pinned to micf_volume_loader's.
 * Outputs are bit-identical from run to run and do not depend on the other samples of the batch: integer counts, sums and maxima
 * or a fixed merge order across threads, no float atomics, no host round trip, no scratch.
 */
#ifndef MICFORMER_AFFINE_H
#define MICFORMER_AFFINE_H

#include "micformer_normalise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_PAD_ZEROS 0
#define MICF_PAD_BORDER 1

/* Workspace bytes of micf_volume_loader_affine for B samples (pure; < 0 for B <= 0). */
int64_t micf_volume_loader_affine_workspace(int B);

/* The arguments of micf_volume_loader_norm with the same meaning, and: affine, device memory, float32 [B][3][4]
 * (affine_per_modality 0: one map per sample for CT, MR and label) or [B][2][3][4] (affine_per_modality 1: map 0 for CT and the
 * CT label, map 1 for MR), read on the device when the kernels run; padding_mode one of MICF_PAD_*.  MICF_EINVAL for a NULL or
 * misaligned map, an unknown padding mode or a flag other than 0 / 1, before any launch.
 * Launches, fixed by the arguments (so the call can be captured in a graph, and a replay picks up new contents of `affine`): the
 * zeroing and the statistics passes of micf_volume_loader_norm; per chunk of 8 samples ONE resample launch for both channels, the
 * label and the crop extents, whatever the modes; the crop finish. */
int micf_volume_loader_affine(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                              int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high, void* workspace,
                              int64_t workspace_bytes, void* image, uint8_t* label_map, int32_t* crop_indexes, double* stats,
                              const float* affine, int affine_per_modality, int padding_mode, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_AFFINE_H */
