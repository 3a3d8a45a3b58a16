// sw_mirror.hip -- test-time mirroring for sliding-window inference (include/micformer_mirror.h): the crop of a window under a
// flip and the accumulate of its prediction flipped back, both as index arithmetic in passes the path runs anyway.
//
// An item is (b, z0, y0, x0, f); bit a of f reverses axis a of the window (0 = D, 1 = H, 2 = W).  Flips along D and H only pick
// another row; a flip along W reads the row piece at rw - VEC - x and reverses it in registers, so a wave still touches one
// contiguous run of memory per access on both sides (consecutive lanes hold consecutive 16-byte pieces, ascending on the side that
// is written, descending on the side that is read).  Rows move as 16-byte accesses when x0, rw, W and the base pointers allow it, as
// dwords otherwise: the choice is per item and the bits are the same.  Memory-bound movers, no LDS: the crop moves 2 * C * roi
// floats, the accumulate reads K * roi floats of prediction and reads and writes (K + 1) * roi floats of accumulator per item.
//
// The accumulate is the store-and-sum form of sw_blend.hip: one launch per item in list order, each a plain read-modify-write of
// the window's own region, every term the one expression blend_term() of sw_rows.h.  The weight belongs to the UN-mirrored voxel
// and is worked out once per voxel with the wsum update; without taps it is 1.
#include "common.h"
#include "sw_rows.h"
#include "../../include/micformer_mirror.h"

namespace {

using micf_sw::Row;
using micf_sw::aligned16;
using micf_sw::blend_term;

constexpr int kMirrorMax = 64;         // items per call (kSwMax of misc.hip)
constexpr int kMirrorThreads = 256;
constexpr int kMirrorBlocks = 2048;    // grid cap; the rest is grid-strided (128^3 in 16-byte pieces is exactly 2048 x 256 items)

struct MirrorItems {
  int b[kMirrorMax], z[kMirrorMax], y[kMirrorMax], x[kMirrorMax];
  unsigned char flip[kMirrorMax], vec[kMirrorMax];
};

// the un-mirrored piece (z, y, x .. x + VEC) of a window -> where its mirror image starts: (mz, my, mx), read ascending from mx and
// then reversed when bit 2 is set
template <int VEC>
__device__ __forceinline__ void mirror_piece(int flip, int rd, int rh, int rw, int z, int y, int x, int& mz, int& my, int& mx) {
  mz = (flip & 1) ? rd - 1 - z : z;
  my = (flip & 2) ? rh - 1 - y : y;
  mx = (flip & 4) ? rw - VEC - x : x;
}

// src: the item's sample [C, D, H, W]; dst: the item's window [C, rd, rh, rw].  One piece = VEC consecutive x of one (z, y) row of
// the WINDOW, all C channels; pieces = rd * rh * (rw / VEC) < 2^31.
template <int VEC>
__device__ __forceinline__ void crop_item(const float* __restrict__ src, float* __restrict__ dst, int C, int64_t plane, int H, int W,
                                          int rd, int rh, int rw, int z0, int y0, int x0, int flip) {
  const uint32_t qw = (uint32_t)(rw / VEC);
  const uint32_t pieces = (uint32_t)rd * (uint32_t)rh * qw;
  const int64_t win = (int64_t)rd * rh * rw;
  for (uint64_t it = (uint64_t)blockIdx.x * kMirrorThreads + threadIdx.x; it < pieces; it += (uint64_t)gridDim.x * kMirrorThreads) {
    const uint32_t i = (uint32_t)it;
    const int x = (int)(i % qw) * VEC;
    const uint32_t row = i / qw;
    const int y = (int)(row % (uint32_t)rh), z = (int)(row / (uint32_t)rh);
    int mz, my, mx;
    mirror_piece<VEC>(flip, rd, rh, rw, z, y, x, mz, my, mx);
    const float* s = src + ((int64_t)(z0 + mz) * H + (y0 + my)) * W + (x0 + mx);
    float* d = dst + ((int64_t)z * rh + y) * rw + x;
#pragma unroll 2
    for (int c = 0; c < C; ++c) {
      Row<VEC> r;
      r.load(s + (int64_t)c * plane);
      if (flip & 4) r.reverse();
      r.store(d + (int64_t)c * win);
    }
  }
}

// blockIdx.y = the item; its row form is uniform over the block
__global__ void __launch_bounds__(kMirrorThreads) sw_mirror_window_kernel(const float* __restrict__ vol, float* __restrict__ win,
                                                                          MirrorItems c, int C, int64_t plane, int H, int W, int rd,
                                                                          int rh, int rw) {
  const int n = blockIdx.y;
  const float* src = vol + (int64_t)c.b[n] * C * plane;
  float* dst = win + (int64_t)n * C * ((int64_t)rd * rh * rw);
  if (c.vec[n])
    crop_item<4>(src, dst, C, plane, H, W, rd, rh, rw, c.z[n], c.y[n], c.x[n], c.flip[n]);
  else
    crop_item<1>(src, dst, C, plane, H, W, rd, rh, rw, c.z[n], c.y[n], c.x[n], c.flip[n]);
}

// pred: this item's [K, rd, rh, rw]; out / wsum: the item's sample, [K, D, H, W] / [D, H, W]; plane = D * H * W.
// One piece = VEC consecutive x of one (z, y) row of the VOLUME side, all K classes; pieces = rd * rh * (rw / VEC) < 2^31.
template <int VEC, bool TAPS>
__global__ void __launch_bounds__(kMirrorThreads) sw_mirror_accumulate_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                                              float* __restrict__ wsum, const float* __restrict__ taps,
                                                                              float floor, int K, int64_t plane, int H, int W, int rd,
                                                                              int rh, int rw, int z0, int y0, int x0, int flip,
                                                                              uint32_t pieces) {
  const uint32_t qw = (uint32_t)(rw / VEC);
  const int64_t win = (int64_t)rd * rh * rw;
  for (uint64_t it = (uint64_t)blockIdx.x * kMirrorThreads + threadIdx.x; it < pieces; it += (uint64_t)gridDim.x * kMirrorThreads) {
    const uint32_t i = (uint32_t)it;
    const int x = (int)(i % qw) * VEC;
    const uint32_t row = i / qw;
    const int y = (int)(row % (uint32_t)rh), z = (int)(row / (uint32_t)rh);
    Row<VEC> w;
    if (TAPS) {
      const float gzy = taps[z] * taps[rd + y];
#pragma unroll
      for (int j = 0; j < VEC; ++j) w.v[j] = fmaxf(gzy * taps[rd + rh + x + j], floor);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) w.v[j] = 1.f;
    }
    const int64_t v = ((int64_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
    Row<VEC> s;
    s.load(wsum + v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) s.v[j] = s.v[j] + w.v[j];
    s.store(wsum + v);
    int mz, my, mx;
    mirror_piece<VEC>(flip, rd, rh, rw, z, y, x, mz, my, mx);
    const float* p = pred + ((int64_t)mz * rh + my) * rw + mx;
    float* o = out + v;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      Row<VEC> a, b;
      a.load(o + (int64_t)k * plane);
      b.load(p + (int64_t)k * win);
      if (flip & 4) b.reverse();
#pragma unroll
      for (int j = 0; j < VEC; ++j) a.v[j] = blend_term(a.v[j], w.v[j], b.v[j]);
      a.store(o + (int64_t)k * plane);
    }
  }
}

// the argument checks the two entry points share; MICF_OK, MICF_EINVAL or MICF_EUNSUPPORTED
int check_items(const int32_t* coords, int n, int B, int C, int D, int H, int W, int rd, int rh, int rw) {
  if (!coords || n <= 0 || n > kMirrorMax || B <= 0 || C <= 0 || rd <= 0 || rh <= 0 || rw <= 0 || D <= 0 || H <= 0 || W <= 0)
    return MICF_EINVAL;
  for (int i = 0; i < n; ++i) {
    const int32_t b = coords[5 * i], z0 = coords[5 * i + 1], y0 = coords[5 * i + 2], x0 = coords[5 * i + 3], f = coords[5 * i + 4];
    if (b < 0 || b >= B || z0 < 0 || y0 < 0 || x0 < 0 || (int64_t)z0 + rd > D || (int64_t)y0 + rh > H || (int64_t)x0 + rw > W ||
        f < 0 || f > 7)
      return MICF_EINVAL;
  }
  const int64_t rows = (int64_t)rd * rh;
  if (rows > INT32_MAX || rows * rw > INT32_MAX) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

uint32_t blocks_for(uint32_t pieces) {
  const uint32_t need = (pieces + kMirrorThreads - 1) / kMirrorThreads;
  return need < (uint32_t)kMirrorBlocks ? need : (uint32_t)kMirrorBlocks;
}

}  // namespace

extern "C" int micf_sw_mirror_window_batch(const float* vol, float* win, const int32_t* coords, int n, int B, int C, int D, int H, int W,
                                           int rd, int rh, int rw, micf_stream_t stream) {
  if (!vol || !win) return MICF_EINVAL;
  if (const int rc = check_items(coords, n, B, C, D, H, W, rd, rh, rw)) return rc;
  const int64_t roi = (int64_t)rd * rh * rw;
  const bool wide = rw % 4 == 0 && W % 4 == 0 && aligned16(vol) && aligned16(win);
  MirrorItems c;
  bool any_dword = false;
  for (int i = 0; i < n; ++i) {
    c.b[i] = coords[5 * i]; c.z[i] = coords[5 * i + 1]; c.y[i] = coords[5 * i + 2]; c.x[i] = coords[5 * i + 3];
    c.flip[i] = (unsigned char)coords[5 * i + 4];
    c.vec[i] = wide && c.x[i] % 4 == 0;
    any_dword |= !c.vec[i];
  }
  const dim3 grid(blocks_for((uint32_t)(any_dword ? roi : roi / 4)), n);
  hipLaunchKernelGGL(sw_mirror_window_kernel, grid, dim3(kMirrorThreads), 0, (hipStream_t)stream, vol, win, c, C, (int64_t)D * H * W, H,
                     W, rd, rh, rw);
  MICF_RETURN_LAUNCH();
}

extern "C" int micf_sw_mirror_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K, int D,
                                         int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream) {
  if (!pred || !out || !wsum || (taps && !(floor > 0.f))) return MICF_EINVAL;
  if (const int rc = check_items(coords, n, B, K, D, H, W, rd, rh, rw)) return rc;
  const int64_t win = (int64_t)rd * rh * rw, plane = (int64_t)D * H * W;
  const bool wide = rw % 4 == 0 && W % 4 == 0 && aligned16(pred) && aligned16(out) && aligned16(wsum);
  for (int i = 0; i < n; ++i) {
    const int32_t b = coords[5 * i], z0 = coords[5 * i + 1], y0 = coords[5 * i + 2], x0 = coords[5 * i + 3], f = coords[5 * i + 4];
    const float* p = pred + (int64_t)i * K * win;
    float* o = out + (int64_t)b * K * plane;
    float* ws = wsum + (int64_t)b * plane;
    const bool vec = wide && x0 % 4 == 0;
    const uint32_t pieces = (uint32_t)(vec ? win / 4 : win);
    const dim3 grid(blocks_for(pieces)), block(kMirrorThreads);
    auto kernel = vec ? (taps ? sw_mirror_accumulate_kernel<4, true> : sw_mirror_accumulate_kernel<4, false>)
                      : (taps ? sw_mirror_accumulate_kernel<1, true> : sw_mirror_accumulate_kernel<1, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, p, o, ws, taps, floor, K, plane, H, W, rd, rh, rw, z0, y0, x0, f,
                       pieces);
    if (hipGetLastError() != hipSuccess) return MICF_ELAUNCH;
  }
  return MICF_OK;
}
