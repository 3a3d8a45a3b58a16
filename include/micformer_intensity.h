/*
 * micformer_intensity.h -- C-ABI of the on-device intensity augmentation: the intensity half of nnU-Net's "moreDA" chain
 * (batchgenerators' GaussianNoiseTransform, GaussianBlurTransform, BrightnessMultiplicativeTransform,
 * ContrastAugmentationTransform, GammaTransform) on a batch of volumes that is already on the device, e.g. the image of
 * micformer_loader.h.  Conventions are those of micformer_hip.h.  Kernels: micformer_amd/csrc/volume_intensity.hip; index, weight
 * and random-number arithmetic: micformer_amd/csrc/intensity_coords.h; rules: DESIGN.md "Volume loader".
 *
 * image: [B][C][D][H][W], float32 or float16, contiguous, C in 1..4.  The output has the same shape and dtype and may be the
 * input (in place).  Every (sample, channel) pair (b, c) is processed on its own.
 * params: device float32 [B][C][8], read on the device when the kernels run:
 *     {sigma, noise_std, brightness, contrast, gamma, gamma_mode, retain_stats, reserved = 0}
 * seeds: device int64 [B], the noise key of each sample.  A captured graph picks up new contents of both at every replay.
 *
 * The chain, in batchgenerators' order, in float32; a step that is off is an exact no-op, so with every step off the output is
 * the input bit for bit:
 *  1 noise     (noise_std > 0)  x += noise_std z(b, c, i), i the linear voxel index in the channel:
 *              h = mix64(mix64(seed_b ^ mix64(c)) + i) with the splitmix64 finaliser,
 *              u1 = ((h >> 40) + 0.5) 2^-24, u2 = ((h & 0xFFFFFF) + 0.5) 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2).
 *              The key depends on the voxel alone: the noise of a reflected halo position is recomputed.
 *  2 blur      (sigma > 0)  scipy.ndimage.gaussian_filter(x, sigma, order=0, mode="reflect", truncate=4.0): per axis the
 *              radius r = int(4 sigma + 0.5), weights exp(-k^2 / (2 sigma^2)) normalised by their sum, boundary "reflect"
 *              (d c b a | a b c d | d c b a) repeated as often as needed, so an axis shorter than r is legal.  sigma is 0 or in
 *              [0.1, 2.0] (r <= 8); the device clamps a positive value into that range.
 *  3 brightness               x *= brightness  (> 0; 1 = off)
 *  4 contrast  (contrast != 1, > 0)  mn, lo, hi = mean, min, max of the channel at this point;
 *              x = clip((x - mn) contrast + mn, lo, hi)
 *  5 gamma     (gamma_mode 0 off, 1 plain, 2 inverted)  inverted: x = -x.  retain_stats: m0, s0 = mean, population std.
 *              lo = min, rng = max - lo, x = ((x - lo) / (rng + 1e-7))^gamma rng + lo.
 *              retain_stats: x = (x - mean(x)) / (std(x) + 1e-8) s0 + m0.  inverted: x = -x again.  rng = 0 gives a finite result.
 *  6 store     rounded to the output dtype once, here.
 * The steps after the blur are monotone per channel for positive brightness and contrast, so every min and max after the blur
 * follows from the blurred channel's by the same float32 expressions; the sums are passes of their own.
 *
 * No address depends on a voxel value or, beyond the clamps, on params: NaN and inf voxels and parameters propagate as values
 * within their (sample, channel).  Outputs are bit-identical from run to run and do not depend on the other samples of the batch:
 * no float atomics, every sum is float64 in a fixed order (a partial per block, then a fixed tree).  No host round trip; the
 * launches are fixed by the shape arguments, on the one stream: the call can be captured in a graph.
 */
#ifndef MICFORMER_INTENSITY_H
#define MICFORMER_INTENSITY_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_INTENSITY_F32 0
#define MICF_INTENSITY_F16 1

#define MICF_INTENSITY_MAX_CHANNELS 4
#define MICF_INTENSITY_MAX_EXTENT 2048
#define MICF_INTENSITY_MAX_VOLUMES 65535 /* B * C */

/* Workspace bytes of micf_intensity_augment: a float32 copy of the batch (B C D H W 4 bytes) plus the per-block partial sums and
 * the per-channel records.  Pure; < 0 on arguments the call itself would refuse. */
int64_t micf_intensity_augment_workspace(int B, int C, int D, int H, int W);

/* in, out: device, dtype one of MICF_INTENSITY_*, aligned to their element; out may equal in, and must not overlap it otherwise.
 * params: device float32 [B][C][8]; seeds: device int64 [B]; workspace: device, 256-byte aligned, workspace_bytes at least the
 * query's value.  stats: NULL, or device float64 [B][C][8] that receives {mean, min, max after the blur; m0, s0; mean, std after
 * the power law; 0} (the four in the middle are 0 unless the gamma step runs with retain_stats).
 * MICF_EINVAL before any launch for a NULL or misaligned pointer, an unknown dtype, a non-positive extent or a short workspace;
 * MICF_EUNSUPPORTED for C > 4, an extent above 2048 or B * C above 65535.
 * Launches, fixed by (B, C, D, H, W): noise + blur along W and H (one LDS tile per block), blur along D + partials of sum, min
 * and max, their fixed-order finish, the partial moments before and after the power law, their finish, the pointwise chain and
 * the store. */
int micf_intensity_augment(const void* in, void* out, int dtype, int B, int C, int D, int H, int W, const float* params,
                           const int64_t* seeds, void* workspace, int64_t workspace_bytes, double* stats, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_INTENSITY_H */
