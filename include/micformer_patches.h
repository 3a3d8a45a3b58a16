/*
 * micformer_patches.h -- C-ABI of the on-device patch sampler of libmicformer_hip.so: native-resolution crops of a registered
 * CT / MR pair (and its CT label), a share of them centred on a foreground voxel -- the rule of nnU-Net's
 * DataLoader3D.generate_train_batch (dataset_loading.py:297-412) restated below.  Parity with nnU-Net is UNPINNED: its code is
 * not run anywhere in this project's tests; the statement below is the specification and tests/patches_ref.py (numpy) its referee.
 * Conventions are those of micformer_loader.h: micf_loader_sample descriptors in host memory, device buffers owned by the caller
 * and sized by pure queries, the stream passed explicitly, no allocation or synchronisation inside, 0 or a negative MICF_E* code
 * with argument errors caught before any launch.  The one addition to micf_loader_sample's rules: the arrays of a sample must have
 * the SAME shape (a patch of a registered pair has one origin), else MICF_EINVAL.
 * Kernels: micformer_amd/csrc/volume_patches.hip; index arithmetic: csrc/patches_coords.h; rules: DESIGN.md "Patch sampler".
 *
 * The index of a scan (micf_patch_index, computed once and reused while the scan stays resident) holds
 *   - the normaliser statistics of both channels: exactly what micf_volume_loader_norm computes and returns in `stats`;
 *   - the voxel count of every class: uint32 [256] at byte 256, class 0, 1..K, then "other" (class 255) at K + 1, exact;
 *   - for a labelled scan the count of each class 1..K in every segment, uint16 [K][R] at byte 1536, R the number of segments rounded
 *     up to a multiple of 4 (the padding holds zeros).  A segment is a run of MICF_PATCH_SEGMENT consecutive voxels in flat
 *     (z, y, x) order.
 * The float64 statistics of channel c lie at byte 112 c + 96 (two values).
 *
 * The rule, per sample b; L the scan extent on an axis, P the patch extent:
 *   1 bounds   need = max(P - L, 0), lb = -ceil(need / 2), ub = L + floor(need / 2) + need mod 2 - P  (odd need: lb = ub - 1).
 *   2 draws[b] = (force, u_class, u_voxel, u_z, u_y, u_x), float32.  index(u, n) = min(int64(double(u) * double(n)), n - 1),
 *              0 for u < 0 or NaN, n - 1 for u >= 1.
 *   3 forced   when force >= 0.5, the sample has a label and a class 1..K has a voxel: the class is the j-th PRESENT class in
 *              ascending order, j = index(u_class, classes present); the voxel is the r-th of that class in flat scan order,
 *              r = index(u_voxel, voxels of the class), exactly; the origin per axis is v - P / 2 (integer division) clamped to
 *              [lb, ub] (MICF_PATCH_CLAMP_BOTH) or from below only (MICF_PATCH_CLAMP_LOWER: the window may run past the far end).
 *   4 random   otherwise (a forced sample without foreground included): origin = lb + index(u_axis, ub - lb + 1) per axis.
 *   5 image    float16 [B, 2, Pd, Ph, Pw]: inside the scan fp16_rn(normalise(x)) with micformer_normalise.h's per-element function
 *              and whole-volume statistics, no interpolation; outside 0.0 (MICF_PATCH_PAD_ZEROS) or the nearest scan voxel
 *              (MICF_PATCH_PAD_BORDER).
 *   6 label    uint8 [B, Pd, Ph, Pw]: the loader's class of the raw value inside the scan, pad_class outside in both padding modes.
 *   origins int32 [B, 3]: where the window starts in the scan (may be negative).  picked int32 [B, 4]: (class, z, y, x) of the
 *   chosen voxel, (0, -1, -1, -1) for a random crop.
 * Sampling is uniform over ALL voxels of the class; nnU-Net draws from at most 10 000 pre-sampled locations per class.
 * Limits (else MICF_EUNSUPPORTED): every extent <= 2048, fewer than 2^31 voxels per scan, Pd * Ph * Pw <= 512^3.
 * Every value that crosses threads is an integer: the outputs are bit-identical from run to run and do not depend on the other
 * samples of the batch.
 */
#ifndef MICFORMER_PATCHES_H
#define MICFORMER_PATCHES_H

#include "micformer_normalise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_PATCH_SEGMENT 2048 /* voxels per segment: 256 threads x 8 voxels, a count fits 16 bits (csrc/patches_coords.h) */

#define MICF_PATCH_PAD_ZEROS 0
#define MICF_PATCH_PAD_BORDER 1

#define MICF_PATCH_CLAMP_BOTH 0
#define MICF_PATCH_CLAMP_LOWER 1

/* Bytes of the index of one scan of `voxels` voxels (pure; < 0 for voxels <= 0 or a bad num_label_values; a multiple of 256). */
int64_t micf_patch_index_bytes(int64_t voxels, int num_label_values, int has_label);

/* Workspace bytes of micf_patch_index for B scans (pure; < 0 for B <= 0): micf_volume_loader_norm's. */
int64_t micf_patch_index_workspace(int B);

/* Builds the index of B scans.  `samples`, `label_values` (distinct, non-zero), `indexes` (B device pointers, 256-byte aligned)
 * and `index_bytes` (B sizes, each at least micf_patch_index_bytes of its scan) are HOST memory, read during the call only.
 * Every sample has a label or none has.  ct_mode / mr_mode / p_low / p_high as micf_volume_loader_norm.  The workspace needs
 * 256-byte alignment.  Launches: zeroing of the workspace; per chunk of 8 scans the statistics passes of the two modes, the copy
 * of the records into the indexes, and (labelled scans) the counting pass: one LDS histogram per segment, the segment's counts
 * stored, one integer atomicAdd per class and workgroup on the class counts. */
int micf_patch_index(const micf_loader_sample* samples, int B, const int32_t* label_values, int num_label_values, int ct_mode,
                     int mr_mode, double p_low, double p_high, void* workspace, int64_t workspace_bytes, void* const* indexes,
                     const int64_t* index_bytes, micf_stream_t stream);

/* Cuts one patch per sample.  `samples`, `label_values`, `indexes`, `index_bytes` as above (the indexes built by micf_patch_index
 * from the same scans, label values and modes: the caller's promise, not checked on the device).  draws: device float32 [B, 6].
 * image: device float16 [B, 2, Pd, Ph, Pw], 16-byte aligned; label_map: device uint8 [B, Pd, Ph, Pw], 8-byte aligned, NULL = no
 * labels (then every samples[b].label must be NULL too, and with a label_map none may be); origins: device int32 [B, 3]; picked:
 * device int32 [B, 4].  padding_mode MICF_PATCH_PAD_*, pad_class 0..255, clamp MICF_PATCH_CLAMP_*.
 * Launches per chunk of 8 samples: locate (one workgroup per sample: class and rank from the draws and the class counts, an
 * integer prefix over the class's segment counts, the voxel inside one segment by ballot / popcount; writes origins and picked)
 * and crop (grid (blocks, samples), reads origins from device memory).  Nothing returns to the host: a captured call reads new
 * draws from the same tensor at every replay. */
int micf_patch_sample(const micf_loader_sample* samples, int B, void* const* indexes, const int64_t* index_bytes,
                      const int32_t* label_values, int num_label_values, const float* draws, int Pd, int Ph, int Pw,
                      int padding_mode, int pad_class, int clamp, void* image, uint8_t* label_map, int32_t* origins,
                      int32_t* picked, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_PATCHES_H */
