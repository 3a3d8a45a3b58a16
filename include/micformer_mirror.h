/*
 * micformer_mirror.h -- C-ABI of test-time mirroring for sliding-window inference (nnU-Net's default at prediction time;
 * micformer_amd/inference.py mirror_axes=, micformer_amd/mirror.py).  Conventions and error codes are those of micformer_blend.h /
 * micformer_hip.h.  Kernels: micformer_amd/csrc/sliding_window.hip; rules: DESIGN.md "Sliding-window inference".
 *
 * A flip code f is a 3-bit mask: bit 0 reverses D, bit 1 H, bit 2 W.  M_f maps a window index (z, y, x) of a (rd, rh, rw) window to
 * (f&1 ? rd-1-z : z, f&2 ? rh-1-y : y, f&4 ? rw-1-x : x); it is its own inverse.  An item is (b, z0, y0, x0, f): a window origin and
 * the flip it is predicted under.  Both flips of an item are index arithmetic inside passes the path runs anyway:
 *   crop        win[i, c, z, y, x]  = vol[b, c, o + M_f(z, y, x)]                          a pure copy
 *   accumulate  out[b, k, o + v]    = fma(w(v), pred[i, k, M_f(v)], out[b, k, o + v]);     wsum[b, o + v] += w(v)
 * with w(v) = max((g0[z] * g1[y]) * g2[x], floor) at the UN-mirrored v (the map of micformer_blend.h; it is bit-symmetric under
 * every flip) or w = 1 without taps.  No float atomics: the items of a call are applied one launch each in list order, so a voxel
 * receives its terms in item order whatever the split of the item list into calls; with taps and f = 0 the result is bit-equal to
 * micf_sw_blend_accumulate, and the crop with f = 0 to micf_sw_window_batch.  micf_sw_normalize(out, wsum, ...) finishes.
 */
#ifndef MICFORMER_MIRROR_H
#define MICFORMER_MIRROR_H

#include "micformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vol [B,C,D,H,W] -> win [n,C,rd,rh,rw] at coords (HOST int32 [n,5] = b,z0,y0,x0,f, read during the call), ONE launch; n <= 64.
 * MICF_EINVAL: a NULL pointer, n outside 1..64, f outside 0..7, a window that leaves the volume, a non-positive extent;
 * MICF_EUNSUPPORTED: rd * rh * rw >= 2^31.  All before the launch. */
int micf_sw_mirror_window_batch(const float* vol, float* win, const int32_t* coords, int n, int B, int C, int D, int H, int W,
                                int rd, int rh, int rw, micf_stream_t stream);

/* pred [n,K,rd,rh,rw] weighted into out [B,K,D,H,W] and wsum [B,D,H,W] at coords (as above), one launch per item in list order.
 * taps: DEVICE float32 [rd+rh+rw] = g0|g1|g2 with floor > 0, or NULL for w = 1 (floor is then ignored).  Errors as above, and
 * MICF_EINVAL for floor <= 0 or NaN with taps.  All before the first launch. */
int micf_sw_mirror_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K, int D,
                              int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MICFORMER_MIRROR_H */
