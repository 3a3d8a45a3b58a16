/*
 * micformer_components.h -- C-ABI of the on-device connected components of libmicformer_hip.so: the clean-up step between
 * micformer_restore.h (a label volume on the scan's grid) and micformer_metrics.h (its score).  A label volume is split into the
 * connected components of its classes, and either the components themselves are returned (labels, sizes) or the volume is
 * filtered: keep the largest component of every class (MONAI's KeepLargestConnectedComponent) or drop the small ones
 * (RemoveSmallObjects).  Conventions are those of micformer_hip.h: device pointers owned by the caller, a caller-provided
 * workspace sized by a pure query, the stream passed explicitly, no allocation or synchronisation inside, 0 or a negative
 * MICF_E* code with argument errors caught before any launch.  Kernels: micformer_amd/csrc/volume_components.hip; rules and the
 * termination argument of the union-find: DESIGN.md "Connected components".
 *
 * Input: per sample one volume of its own shape (d, h, w), contiguous, w fastest, as
 *   MICF_COMPONENTS_U8   a uint8 class map: value k in 1..K-1 is class k (label_values NULL, num_label_values 0), or
 *   MICF_COMPONENTS_I16 / _I32  a label volume: value label_values[k - 1] is class k (num_label_values == K - 1 distinct non-zero
 *                        values, as micformer_restore.h writes them).
 * Value 0 is background.  Any other value that names no class belongs to no component and is written through unchanged.
 *
 * Rules:
 *   - two voxels are connected iff they hold the same class and are neighbours: connectivity 6 (faces), 18 (+ edges) or
 *     26 (+ corners).  All classes are labelled in one pass over the multi-valued map (MONAI's independent=True).
 *   - a component's ROOT is the smallest linear index (z * h + y) * w + x among its voxels, its LABEL is root + 1 (int32);
 *     background and unclassed voxels have label 0.  (scipy.ndimage.label numbers components in the same order.)
 *   - a component's SIZE is its voxel count (int32).
 *   - MICF_COMPONENTS_KEEP_LARGEST: of every class in class_mask (bit k = class k, k in 1..K-1) the component of the greatest size
 *     stays, the lowest root winning an exact tie (argmax of bincount); every other voxel of that class becomes 0.
 *   - MICF_COMPONENTS_REMOVE_SMALL: every component of a class in class_mask with size < min_size becomes 0.
 *   - classes outside class_mask pass through; the output has the input's dtype and shape; out == in is allowed.
 * Atomics: the union-find links with integer atomicMin, the sizes are integer atomic adds (one per tile and component), the
 * selection is one 64-bit integer atomicMax per root.  Integer minima, sums and maxima do not depend on the order of arrival, so
 * every output is bit-identical from run to run.  The launch sequence is fixed (it does not depend on the data): a call can be
 * captured in a HIP graph.
 * Limits (else MICF_EUNSUPPORTED): 2 <= K <= 32, every extent <= 2048, voxels per sample < 2^31 - 1.
 */
#ifndef MICFORMER_COMPONENTS_H
#define MICFORMER_COMPONENTS_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_COMPONENTS_U8 0
#define MICF_COMPONENTS_I16 1
#define MICF_COMPONENTS_I32 2

#define MICF_COMPONENTS_KEEP_LARGEST 0
#define MICF_COMPONENTS_REMOVE_SMALL 1

#define MICF_COMPONENTS_MAX_CLASSES 32

/* One sample (a HOST array of B of these, read during the call only).  `in` is device memory of shape[0] * shape[1] * shape[2]
 * elements of the call's in_dtype, aligned to it.  `out`: micf_connected_components writes int32 labels (4-byte aligned),
 * micf_filter_components the filtered volume in in_dtype (out == in allowed). */
typedef struct micf_component_sample {
  const void* in;
  void* out;
  int32_t shape[3]; /* (d, h, w) */
} micf_component_sample;

/* Workspace bytes of either call below (pure; the sum over the samples of: the parent links, 4 bytes per voxel, the sizes,
 * 4 bytes per voxel, and 256 bytes of per-class selection, each rounded up to 256 bytes); < 0 for bad arguments (MICF_EINVAL:
 * NULL, B <= 0, an extent <= 0; MICF_EUNSUPPORTED beyond the limits above). */
int64_t micf_components_workspace(const micf_component_sample* samples, int B);

/* Per voxel the label of its component into samples[b].out (int32) and, when `sizes` is not NULL, the size of its component
 * (0 off-component) into sizes[b] (a HOST array of B device pointers to int32 volumes).  The workspace must be 256-byte aligned. */
int micf_connected_components(const micf_component_sample* samples, int B, int in_dtype, int K, const int32_t* label_values,
                              int num_label_values, int connectivity, int32_t* const* sizes, void* workspace,
                              int64_t workspace_bytes, micf_stream_t stream);

/* The filtered volume into samples[b].out.  class_mask: bits 1..K-1 only, not 0.  min_size >= 1 (read by MICF_COMPONENTS_REMOVE_SMALL
 * only, checked always). */
int micf_filter_components(const micf_component_sample* samples, int B, int in_dtype, int K, const int32_t* label_values,
                           int num_label_values, int connectivity, int64_t class_mask, int mode, int min_size, void* workspace,
                           int64_t workspace_bytes, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_COMPONENTS_H */
