/*
 * micformer_blend.h -- C-ABI of the weighted accumulate of sliding-window inference with mode="gaussian" (the counterpart of
 * monai.inferers.sliding_window_inference(mode="gaussian"); micformer_amd/inference.py, micformer_amd/blend.py).  Conventions are
 * those of micformer_hip.h.  Kernel: micformer_amd/csrc/sliding_window.hip; rules: DESIGN.md "Sliding-window inference".
 *
 * The importance map of a window of (rd, rh, rw) voxels is separable.  The HOST builds three tap vectors g0 | g1 | g2 (float32,
 * g_i[j] = exp(-(j - (n_i - 1) / 2)^2 / (2 sigma_i^2)), sigma_i = sigma_scale_i * n_i) and floor = max(min of their outer product,
 * 1e-3); the device evaluates the weight of window voxel (z, y, x) as
 *     w = max((g0[z] * g1[y]) * g2[x], floor)              two float32 multiplies in that order, nothing fused,
 * which is bit for bit the host's map  max((g0[:, None] * g1[None, :])[:, :, None] * g2, floor).
 * For every voxel v of window i and every class k:   out[b, k, v] = fma(w, pred[i, k, v], out[b, k, v]);  wsum[b, v] += w.
 * No float atomics and a fixed order: the windows of a call are applied one launch each in index order, calls run in stream order,
 * and a voxel's term is the same single-rounding fma whichever launch shape (16-byte or scalar rows) serves it.  out / wsum are
 * therefore bit-identical from run to run and for every split of the same window sequence into calls.
 * micf_sw_normalize(out, wsum, ...) of micformer_hip.h finishes: out / wsum.
 */
#ifndef MICFORMER_BLEND_H
#define MICFORMER_BLEND_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pred [n,K,rd,rh,rw] weighted into out [B,K,D,H,W] and wsum [B,D,H,W] at coords (HOST int32 [n,4] = b,z0,y0,x0, read during
 * the call); taps: DEVICE float32 [rd+rh+rw] = g0|g1|g2; n <= 64, any K >= 1.  MICF_EINVAL as micf_sw_accumulate_batch.
 * Also MICF_EINVAL: NULL taps, floor <= 0 or NaN; MICF_EUNSUPPORTED: rd * rh * rw >= 2^31.  All before the first launch. */
int micf_sw_blend_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K,
                             int D, int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_BLEND_H */
