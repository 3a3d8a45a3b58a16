// sw_blend.hip -- the weighted accumulate of sliding-window inference with mode="gaussian" (include/micformer_blend.h).
//
// Store-and-sum form, no float atomics: one launch per window, each a plain read-modify-write of the window's own region of the
// volume accumulator.  A window never overlaps itself and the launches of a call run in stream order, so every voxel receives its
// terms in window-index order, each as the one expression blend_term() below -- whether the running sum came from the previous
// launch through HBM or not.  Memory-bound: per window K * roi floats of prediction read once, (K + 1) * roi floats of accumulator
// read and written once; rows along x move as 16-byte accesses when x0, rw, W and the three base pointers allow it, as dwords
// otherwise (same arithmetic, same bits).  The separable weight of a voxel is rebuilt from three taps held in registers and is
// worked out once per voxel (with the wsum update), not once per class.
#include "common.h"
#include "sw_rows.h"
#include "../../include/micformer_blend.h"

namespace {

constexpr int kBlendMax = 64;          // windows per call (kSwMax of misc.hip)
constexpr int kBlendThreads = 256;
constexpr int kBlendBlocks = 2048;     // grid cap; the rest is grid-strided (128^3 in 16-byte pieces is exactly 2048 x 256 items)

using micf_sw::Row;          // a row piece of VEC floats, and blend_term(): the ONE accumulate expression (sw_rows.h)
using micf_sw::aligned16;
using micf_sw::blend_term;

// pred: this window's [K, rd, rh, rw]; out / wsum: the window's sample, [K, D, H, W] / [D, H, W]; plane = D * H * W.
// One item = VEC consecutive x of one (z, y) row, all K classes; items = rd * rh * (rw / VEC) < 2^31.
template <int VEC>
__global__ void __launch_bounds__(kBlendThreads) sw_blend_window_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                                        float* __restrict__ wsum, const float* __restrict__ taps,
                                                                        float floor, int K, int64_t plane, int H, int W, int rd,
                                                                        int rh, int rw, int z0, int y0, int x0, uint32_t items) {
  const uint32_t qw = (uint32_t)(rw / VEC);
  const int64_t win = (int64_t)rd * rh * rw;
  for (uint64_t it = (uint64_t)blockIdx.x * kBlendThreads + threadIdx.x; it < items; it += (uint64_t)gridDim.x * kBlendThreads) {
    const uint32_t i = (uint32_t)it;
    const int x = (int)(i % qw) * VEC;
    const uint32_t row = i / qw;
    const int y = (int)(row % (uint32_t)rh), z = (int)(row / (uint32_t)rh);
    const float gzy = taps[z] * taps[rd + y];
    Row<VEC> w;
#pragma unroll
    for (int j = 0; j < VEC; ++j) w.v[j] = fmaxf(gzy * taps[rd + rh + x + j], floor);
    const int64_t v = ((int64_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
    Row<VEC> s;
    s.load(wsum + v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) s.v[j] = s.v[j] + w.v[j];
    s.store(wsum + v);
    const float* p = pred + ((int64_t)z * rh + y) * rw + x;
    float* o = out + v;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      Row<VEC> a, b;
      a.load(o + (int64_t)k * plane);
      b.load(p + (int64_t)k * win);
#pragma unroll
      for (int j = 0; j < VEC; ++j) a.v[j] = blend_term(a.v[j], w.v[j], b.v[j]);
      a.store(o + (int64_t)k * plane);
    }
  }
}

}  // namespace

extern "C" int micf_sw_blend_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K, int D,
                                        int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream) {
  if (!pred || !out || !wsum || !coords || !taps || !(floor > 0.f) || n <= 0 || n > kBlendMax || B <= 0 || K <= 0 || rd <= 0 ||
      rh <= 0 || rw <= 0 || D <= 0 || H <= 0 || W <= 0)
    return MICF_EINVAL;
  for (int i = 0; i < n; ++i) {
    const int32_t b = coords[4 * i], z0 = coords[4 * i + 1], y0 = coords[4 * i + 2], x0 = coords[4 * i + 3];
    if (b < 0 || b >= B || z0 < 0 || y0 < 0 || x0 < 0 || (int64_t)z0 + rd > D || (int64_t)y0 + rh > H || (int64_t)x0 + rw > W)
      return MICF_EINVAL;
  }
  const int64_t win = (int64_t)rd * rh * rw, plane = (int64_t)D * H * W;
  if (win > INT32_MAX) return MICF_EUNSUPPORTED;
  const bool wide = rw % 4 == 0 && W % 4 == 0 && aligned16(pred) && aligned16(out) && aligned16(wsum);
  for (int i = 0; i < n; ++i) {
    const int32_t b = coords[4 * i], z0 = coords[4 * i + 1], y0 = coords[4 * i + 2], x0 = coords[4 * i + 3];
    const float* p = pred + (int64_t)i * K * win;
    float* o = out + (int64_t)b * K * plane;
    float* ws = wsum + (int64_t)b * plane;
    const bool vec = wide && x0 % 4 == 0;
    const uint32_t items = (uint32_t)(vec ? win / 4 : win);
    const uint32_t need = (items + kBlendThreads - 1) / kBlendThreads;
    const dim3 grid(need < (uint32_t)kBlendBlocks ? need : (uint32_t)kBlendBlocks);
    if (vec)
      hipLaunchKernelGGL(sw_blend_window_kernel<4>, grid, dim3(kBlendThreads), 0, (hipStream_t)stream, p, o, ws, taps, floor, K, plane,
                         H, W, rd, rh, rw, z0, y0, x0, items);
    else
      hipLaunchKernelGGL(sw_blend_window_kernel<1>, grid, dim3(kBlendThreads), 0, (hipStream_t)stream, p, o, ws, taps, floor, K, plane,
                         H, W, rd, rh, rw, z0, y0, x0, items);
    if (hipGetLastError() != hipSuccess) return MICF_ELAUNCH;
  }
  return MICF_OK;
}
