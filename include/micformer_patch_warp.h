/*
 * micformer_patch_warp.h -- C-ABI of the patch sampler's crop THROUGH a map: micformer_patches.h's patch (same samples, indexes,
 * draws, locate step, padding modes, pad_class and limits) cut straight from the raw scan through an affine map and / or a
 * displacement field on the patch grid -- rotation, zoom and elastic deformation OF A PATCH.  One interpolation of the image and
 * one rounding of the label; nothing intermediate is written, and nothing is padded that the scan could have filled (a rotated
 * patch's corners read the scan where it has data).  Conventions are those of micformer_patches.h.  Kernel:
 * micformer_amd/csrc/volume_patch_warp.hip; coordinate arithmetic: csrc/affine_coords.h, csrc/elastic_coords.h,
 * csrc/patch_warp_coords.h; rules: DESIGN.md "Patch sampler".
 *
 * The origin o and `picked` come from the draws exactly as in micformer_patches.h (rules 1-4): the locate step is unchanged, a
 * forced patch is still centred on its drawn foreground voxel, and the warp turns about the patch centre.  For patch voxel
 * (z, y, x) of (Pd, Ph, Pw), on a scan of extent L per axis:
 *     n = ((2 x + 1) / Pw - 1, (2 y + 1) / Ph - 1, (2 z + 1) / Pd - 1)       micformer_affine.h's n on the PATCH grid
 *     u = the field interpolated at the voxel                                micformer_elastic.h's rule on the patch grid: control
 *                                                                            position p = o (g - 1) / (P - 1) per axis; 0 without a field
 *     s = theta . (n + u, 1)                                                 the identity without a map
 *     i_axis = (float) o_axis + ((s_axis + 1) P_axis - 1) / 2               one fmaf, an exact halving, one rounded add
 * theta is F.affine_grid's map in NORMALISED PATCH coordinates, float32 [B][3][4], or [B][2][3][4] with affine_per_modality = 1:
 * map 0 for CT and its label, map 1 for MR.  The field is float32 [B][3][gd][gh][gw], components (x, y, z), in normalised patch
 * units, its corner points on the centres of the patch's first and last voxel, MICF_FIELD_LINEAR or MICF_FIELD_CUBIC
 * (micformer_elastic.h's taps and weights); it is applied BEFORE the map, and CT, label and MR see the same deformation.  u is a
 * separable sum with one fused multiply-add per tap: y inside z per x tap, then the x taps; a control point is weighted even
 * where its weight is 0, so a NaN or inf entry reaches every voxel whose taps include it.
 *   image   the trilinear sum over the 8 taps around i, each tap normalised first with the statistics of the scan's index (the
 *           per-element function of micformer_normalise.h, as micf_patch_sample), rounded with fp16 round-to-nearest.
 *           MICF_PATCH_PAD_ZEROS: a tap outside the scan counts 0.  MICF_PATCH_PAD_BORDER: i is clamped to [0, L - 1] first.
 *   label   the nearest tap (round half to even), then the loader's class.  Where the ROUNDED index lies outside the scan on any
 *           axis the class is pad_class, in BOTH padding modes: the patch sampler's own rule, not the affine loader's class 0.
 *   A non-finite s on any axis gives image 0 and pad_class.  A finite s, however large, is clamped in float before any conversion
 *   to int: no map or field produces an address outside the arrays or the field.
 * float32 throughout.  With EPS = 2^-20, an index is within P EPS + (L + P) 2^-24 voxels of its exact value for a map with row sums
 * <= 1.5 (micformer_affine.h's bound on the patch grid plus the rounding of the origin add), and within 2 P EPS + (L + P) 2^-24 with
 * a field of |u| <= 0.25 (micformer_elastic.h's bound likewise).
 * Identity map (or none) with power-of-two patch extents: every quantity above is exact and i = o + x, so for finite image data
 * the outputs are micf_patch_sample's bit for bit, in both padding modes.  An all-zero field: the map-only call bit for bit.
 * Outputs are bit-identical from run to run and do not depend on the other samples of the batch; no float atomics, no host round
 * trip, no workspace, no scratch.
 */
#ifndef MICFORMER_PATCH_WARP_H
#define MICFORMER_PATCH_WARP_H

#include "micformer_elastic.h"
#include "micformer_patches.h"

#ifdef __cplusplus
extern "C" {
#endif

/* micf_patch_sample's arguments in the same order and with the same meaning, then: affine, device float32 [B][3][4] or
 * [B][2][3][4] (affine_per_modality 0 / 1), NULL = the identity; displacement, device float32 [B][3][gd][gh][gw], NULL = no field
 * (gd, gh, gw and field_interpolation are then ignored); field_interpolation one of MICF_FIELD_*.  Both are read on the device when
 * the kernel runs.  image needs 16-byte alignment where Pw % 8 == 0, 8-byte where Pw % 4 == 0; label_map 8- and 4-byte.
 * MICF_EINVAL before any launch for any of micf_patch_sample's conditions, a misaligned map or field, an affine_per_modality other
 * than 0 / 1, an unknown interpolation or a grid extent below 2; MICF_EUNSUPPORTED for a grid extent above 512.
 * Launches per chunk of 8 samples: micf_patch_sample's locate, unchanged, and ONE warp-crop launch, grid (blocks, samples), that
 * writes both image planes and the label.  Nothing returns to the host: a captured call reads new draws, maps and fields from the
 * same tensors at every replay. */
int micf_patch_sample_warped(const micf_loader_sample* samples, int B, void* const* indexes, const int64_t* index_bytes,
                             const int32_t* label_values, int num_label_values, const float* draws, int Pd, int Ph, int Pw,
                             int padding_mode, int pad_class, int clamp, void* image, uint8_t* label_map, int32_t* origins,
                             int32_t* picked, const float* affine, int affine_per_modality, const float* displacement, int gd,
                             int gh, int gw, int field_interpolation, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_PATCH_WARP_H */
