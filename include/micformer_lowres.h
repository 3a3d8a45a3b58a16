/*
 * micformer_lowres.h -- C-ABI of the on-device low-resolution simulation: batchgenerators' SimulateLowResolutionTransform as
 * nnU-Net's "moreDA" chain configures it (order_downsample = 0, order_upsample = 3, skimage resize with mode="edge" and no
 * anti-aliasing, i.e. scipy.ndimage.zoom(..., mode="nearest", grid_mode=True)) on a batch of volumes that is already on the device.
 * Conventions are those of micformer_hip.h.  Kernels: micformer_amd/csrc/volume_lowres.hip; index, weight and prefilter-start
 * arithmetic: micformer_amd/csrc/lowres_coords.h; rules: DESIGN.md "Low-resolution simulation".
 *
 * image: [B][C][D][H][W], float32 or float16, contiguous, C in 1..4.  The output has the same shape and dtype and may be the
 * input (in place).  Every (sample, channel) pair (b, c) is processed on its own.
 * target: device int32 [B][C][3], the low-resolution extents (td, th, tw) of every channel, read on the device when the kernels
 * run; each value is clamped into [1, n] of its axis there.  A captured graph picks up new contents at every replay.
 *
 * Per channel x of extents n = (D, H, W) with target t:
 *  0 off         t == n on all three axes: the output is the input bit for bit (a copy, or nothing at all in place).
 *  1 downsample  low[o] = x[min(((2 o + 1) n) / (2 t), n - 1)] per axis, in integer arithmetic: nearest neighbour at half-pixel
 *                centres, ties upward.  (scipy's order 0 agrees except at exact ties, where its float64 product lands below.)
 *  2 prefilter   c = the interpolating cubic B-spline coefficients (pole sqrt(3) - 2, gain 6) of `low` extended by its edge values
 *                to infinity, along each of the three axes.  The recursions start from the closed-form sums of the constant
 *                extension; the coefficients of the extension itself are kept two entries beyond either end of an axis.
 *  3 upsample    output voxel o reads at s = (o + 1/2) t / n - 1/2 per axis: taps floor(s) - 1 .. floor(s) + 2 of the extended
 *                coefficients (indices -2 .. t + 1 occur) with the four cubic B-spline weights of s - floor(s).  An axis with
 *                t == n still goes through prefilter and weights (1/6, 4/6, 1/6, 0): it reproduces its samples up to rounding.
 *  4 store       float32 arithmetic throughout, rounded to the output dtype once, here.  Cubic overshoot is kept: no clip.
 * Other interpolation orders and boundary modes are not offered.
 *
 * No address depends on a voxel value or, beyond the clamp, on target: NaN and inf voxels propagate as values within their
 * (sample, channel).  Outputs are bit-identical from run to run and do not depend on the other samples of the batch: no atomics.
 * No host round trip; the launches are fixed by the shape arguments, on the one stream: the call can be captured in a graph.
 */
#ifndef MICFORMER_LOWRES_H
#define MICFORMER_LOWRES_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MICF_LOWRES_F32 0
#define MICF_LOWRES_F16 1

#define MICF_LOWRES_MAX_CHANNELS 4
#define MICF_LOWRES_MAX_EXTENT 2048
#define MICF_LOWRES_MAX_VOLUMES 65535 /* B * C */

/* Workspace bytes of micf_lowres_simulate: the float32 coefficients of every channel with two entries beyond either end of every
 * axis, sized for the worst case t = n (B C (D + 4) (H + 4) (W + 4) 4 bytes).  Pure; < 0 on arguments the call itself would
 * refuse. */
int64_t micf_lowres_workspace(int B, int C, int D, int H, int W);

/* in, out: device, dtype one of MICF_LOWRES_*, aligned to their element; out may equal in, and must not overlap it otherwise.
 * target: device int32 [B][C][3] in (d, h, w) order; workspace: device, 256-byte aligned, workspace_bytes at least the query's
 * value.
 * MICF_EINVAL before any launch for a NULL or misaligned pointer, an unknown dtype, a non-positive extent or a short workspace;
 * MICF_EUNSUPPORTED for C > 4, an extent above 2048 or B * C above 65535.
 * Launches, fixed by (B, C, D, H, W): the gather fused with the prefilter along W (lines staged in LDS), the prefilter along H,
 * the prefilter along D (one column per thread, lanes across W), the separable upsample of one output tile per block (four taps
 * along D, then H, then W) and the store (16 bytes per lane where W and the pointers allow).  A channel that is off leaves the
 * first three at once and is copied by the fourth, or left alone where out == in. */
int micf_lowres_simulate(const void* in, void* out, int dtype, int B, int C, int D, int H, int W, const int32_t* target,
                         void* workspace, int64_t workspace_bytes, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_LOWRES_H */
