// sliding_window.hip -- the movers of sliding-window inference (utils.py:226-234: monai sliding_window_inference; micformer_hip.h,
// micformer_blend.h, micformer_mirror.h; micformer_amd/inference.py): crop windows of the volume, add their predictions into the
// full-volume fp32 sums, divide.  Four kernels, all memory-bound, no LDS:
//
//   crop        win[i, c, z, y, x] = vol[b, c, o + M_f(z, y, x)]: one launch for the n items of a call
//   accumulate  out[b, k, o + v] = fma(w(v), pred[i, k, M_f(v)], out[b, k, o + v]); wsum[b, o + v] += w(v): store-and-sum, one launch
//               per item in list order, each a plain read-modify-write of the window's own region (a window never overlaps itself).
//               No float atomics, and every term is the one expression blend_term(), so a voxel's sums are the same bits whichever
//               row form serves it and however the item list is cut into calls
//   accumulate, atomic   one launch for n possibly overlapping windows (constant mode, un-mirrored)
//   normalise   out[k, v] /= count[v]
//
// An item is (b, z0, y0, x0, f); bit a of f reverses axis a of the window (0 = D, 1 = H, 2 = W), M_f is that reversal.  Flips along
// D and H only pick another row; a flip along W reads the row piece at rw - VEC - x and reverses it in registers, so a wave still
// touches one contiguous run of memory per access on both sides.  Rows move as 16-byte accesses when x0, rw, W and the base
// pointers allow it, as dwords otherwise: the choice is per item and the bits are the same.  The weight w(v) = max((g0[z] * g1[y])
// * g2[x], floor) belongs to the UN-mirrored voxel and is worked out once per voxel with the wsum update; without taps it is 1.
#include "common.h"
#include "../../include/micformer_blend.h"
#include "../../include/micformer_mirror.h"

namespace {

constexpr int kItems = 64;         // items per call
constexpr int kThreads = 256;
constexpr int kBlocks = 2048;      // grid cap of the window movers; the rest is grid-strided (128^3 in 16-byte pieces is 2048 x 256)

// the ONE accumulate expression: a single rounding, independent of the compiler's contraction setting
__device__ __forceinline__ float blend_term(float acc, float w, float p) { return __builtin_fmaf(w, p, acc); }

// a row piece of VEC floats that moves as one dword or one 16-byte access
template <int VEC> struct Row;
template <> struct Row<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
  __device__ __forceinline__ void reverse() {}
};
template <> struct Row<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
  __device__ __forceinline__ void reverse() {
    const float a = v[0], b = v[1];
    v[0] = v[3]; v[1] = v[2]; v[2] = b; v[3] = a;
  }
};

struct Items {
  int b[kItems], z[kItems], y[kItems], x[kItems];
  unsigned char flip[kItems], vec[kItems];
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
  for (uint64_t it = (uint64_t)blockIdx.x * kThreads + threadIdx.x; it < pieces; it += (uint64_t)gridDim.x * kThreads) {
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
__global__ void __launch_bounds__(kThreads) sw_crop_kernel(const float* __restrict__ vol, float* __restrict__ win, Items c, int C,
                                                           int64_t plane, int H, int W, int rd, int rh, int rw) {
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
// TAPS = false: w = 1 (taps and floor unread).  FLIP = false is the form for flip code 0: `flip` is unread and the mirror vanishes.
template <int VEC, bool TAPS, bool FLIP>
__global__ void __launch_bounds__(kThreads) sw_accumulate_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                                 float* __restrict__ wsum, const float* __restrict__ taps, float floor,
                                                                 int K, int64_t plane, int H, int W, int rd, int rh, int rw, int z0,
                                                                 int y0, int x0, int flip, uint32_t pieces) {
  const uint32_t qw = (uint32_t)(rw / VEC);
  const int64_t win = (int64_t)rd * rh * rw;
  for (uint64_t it = (uint64_t)blockIdx.x * kThreads + threadIdx.x; it < pieces; it += (uint64_t)gridDim.x * kThreads) {
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
    int mz = z, my = y, mx = x;
    if (FLIP) mirror_piece<VEC>(flip, rd, rh, rw, z, y, x, mz, my, mx);
    const float* p = pred + ((int64_t)mz * rh + my) * rw + mx;
    float* o = out + v;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      Row<VEC> a, b;
      a.load(o + (int64_t)k * plane);
      b.load(p + (int64_t)k * win);
      if (FLIP && (flip & 4)) b.reverse();
#pragma unroll
      for (int j = 0; j < VEC; ++j) a.v[j] = blend_term(a.v[j], w.v[j], b.v[j]);
      a.store(o + (int64_t)k * plane);
    }
  }
}

// one launch accumulates `n` predictions (windows of a batch may overlap: fp32 atomics; the sum over <= 8 visits is
// order-independent to an ulp)
__global__ void __launch_bounds__(kThreads) sw_accumulate_batch_kernel(const float* __restrict__ pred, float* __restrict__ out,
                                                                       float* __restrict__ count, Items c, int K, int D, int H, int W,
                                                                       int rd, int rh, int rw, int64_t per) {
  const int n = blockIdx.y;
  const float* p = pred + (int64_t)n * per;
  float* o = out + (int64_t)c.b[n] * K * D * H * W;
  float* cn = count + (int64_t)c.b[n] * D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % rw); int64_t r = i / rw;
    const int y = (int)(r % rh); r /= rh;
    const int z = (int)(r % rd); const int k = (int)(r / rd);
    const int64_t v = ((int64_t)(c.z[n] + z) * H + c.y[n] + y) * W + c.x[n] + x;
    atomicAdd(o + (int64_t)k * D * H * W + v, p[i]);
    if (k == 0) atomicAdd(cn + v, 1.f);
  }
}

__global__ void __launch_bounds__(kThreads) sw_normalize_kernel(float* __restrict__ out, const float* __restrict__ count, int64_t V,
                                                                int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) out[i] /= count[i % V];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

uint32_t blocks_for(int64_t work, int64_t cap = kBlocks) {
  const int64_t need = (work + kThreads - 1) / kThreads;
  return (uint32_t)(need < cap ? need : cap);
}

// The argument checks of every entry point, and its item table.  coords: HOST int32 [n, stride], (b, z0, y0, x0) and, with a
// stride of 5, the flip code (else 0); `wide`: rw, W and the bases allow 16-byte rows, so an item with x0 % 4 == 0 takes them.
// -> MICF_OK, MICF_EINVAL, or MICF_EUNSUPPORTED for a window of >= 2^31 voxels.
int check_items(Items& c, const int32_t* coords, int stride, bool wide, int n, int B, int C, int D, int H, int W, int rd, int rh, int rw) {
  if (!coords || n <= 0 || n > kItems || B <= 0 || C <= 0 || rd <= 0 || rh <= 0 || rw <= 0 || D <= 0 || H <= 0 || W <= 0)
    return MICF_EINVAL;
  for (int i = 0; i < n; ++i) {
    const int32_t* it = coords + (int64_t)stride * i;
    const int32_t b = it[0], z0 = it[1], y0 = it[2], x0 = it[3], f = stride == 5 ? it[4] : 0;
    if (b < 0 || b >= B || z0 < 0 || y0 < 0 || x0 < 0 || (int64_t)z0 + rd > D || (int64_t)y0 + rh > H || (int64_t)x0 + rw > W ||
        f < 0 || f > 7)
      return MICF_EINVAL;
    c.b[i] = b; c.z[i] = z0; c.y[i] = y0; c.x[i] = x0;
    c.flip[i] = (unsigned char)f;
    c.vec[i] = wide && x0 % 4 == 0;
  }
  const int64_t rows = (int64_t)rd * rh;
  if (rows > INT32_MAX || rows * rw > INT32_MAX) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

int crop(const float* vol, float* win, const int32_t* coords, int stride, int n, int B, int C, int D, int H, int W, int rd, int rh,
         int rw, micf_stream_t stream) {
  if (!vol || !win) return MICF_EINVAL;
  Items c;
  const bool wide = rw % 4 == 0 && W % 4 == 0 && aligned16(vol) && aligned16(win);
  if (const int rc = check_items(c, coords, stride, wide, n, B, C, D, H, W, rd, rh, rw)) return rc;
  const int64_t roi = (int64_t)rd * rh * rw;
  bool any_dword = false;
  for (int i = 0; i < n; ++i) any_dword |= !c.vec[i];
  const dim3 grid(blocks_for(any_dword ? roi : roi / 4), n);
  hipLaunchKernelGGL(sw_crop_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, vol, win, c, C, (int64_t)D * H * W, H, W, rd, rh, rw);
  MICF_RETURN_LAUNCH();
}

template <int VEC>
auto accumulate_kernel(bool taps, bool flip) {
  return taps ? (flip ? sw_accumulate_kernel<VEC, true, true> : sw_accumulate_kernel<VEC, true, false>)
              : (flip ? sw_accumulate_kernel<VEC, false, true> : sw_accumulate_kernel<VEC, false, false>);
}

// store-and-sum: one launch per item, in list order
int accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int stride, int n, int B, int K, int D, int H, int W,
               int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream) {
  if (!pred || !out || !wsum || (taps && !(floor > 0.f))) return MICF_EINVAL;
  Items c;
  const bool wide = rw % 4 == 0 && W % 4 == 0 && aligned16(pred) && aligned16(out) && aligned16(wsum);
  if (const int rc = check_items(c, coords, stride, wide, n, B, K, D, H, W, rd, rh, rw)) return rc;
  const int64_t win = (int64_t)rd * rh * rw, plane = (int64_t)D * H * W;
  for (int i = 0; i < n; ++i) {
    const uint32_t pieces = (uint32_t)(c.vec[i] ? win / 4 : win);
    auto kernel = c.vec[i] ? accumulate_kernel<4>(taps, c.flip[i]) : accumulate_kernel<1>(taps, c.flip[i]);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(pieces)), dim3(kThreads), 0, (hipStream_t)stream, pred + (int64_t)i * K * win,
                       out + (int64_t)c.b[i] * K * plane, wsum + (int64_t)c.b[i] * plane, taps, floor, K, plane, H, W, rd, rh, rw,
                       c.z[i], c.y[i], c.x[i], (int)c.flip[i], pieces);
    if (hipGetLastError() != hipSuccess) return MICF_ELAUNCH;
  }
  return MICF_OK;
}

}  // namespace

extern "C" int micf_sw_window(const float* vol, float* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0,
                              int x0, micf_stream_t stream) {
  const int32_t at[4] = {0, z0, y0, x0};
  return crop(vol, win, at, 4, 1, 1, C, D, H, W, rd, rh, rw, stream);
}
extern "C" int micf_sw_window_batch(const float* vol, float* win, const int32_t* coords, int n, int B, int C, int D, int H, int W,
                                    int rd, int rh, int rw, micf_stream_t stream) {
  return crop(vol, win, coords, 4, n, B, C, D, H, W, rd, rh, rw, stream);
}
extern "C" int micf_sw_mirror_window_batch(const float* vol, float* win, const int32_t* coords, int n, int B, int C, int D, int H, int W,
                                           int rd, int rh, int rw, micf_stream_t stream) {
  return crop(vol, win, coords, 5, n, B, C, D, H, W, rd, rh, rw, stream);
}

extern "C" int micf_sw_accumulate(const float* pred, float* out, float* count, int K, int D, int H, int W, int rd, int rh, int rw,
                                  int z0, int y0, int x0, micf_stream_t stream) {
  const int32_t at[4] = {0, z0, y0, x0};
  return accumulate(pred, out, count, at, 4, 1, 1, K, D, H, W, rd, rh, rw, nullptr, 1.f, stream);
}
extern "C" int micf_sw_blend_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K, int D,
                                        int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream) {
  if (!taps) return MICF_EINVAL;
  return accumulate(pred, out, wsum, coords, 4, n, B, K, D, H, W, rd, rh, rw, taps, floor, stream);
}
extern "C" int micf_sw_mirror_accumulate(const float* pred, float* out, float* wsum, const int32_t* coords, int n, int B, int K, int D,
                                         int H, int W, int rd, int rh, int rw, const float* taps, float floor, micf_stream_t stream) {
  return accumulate(pred, out, wsum, coords, 5, n, B, K, D, H, W, rd, rh, rw, taps, floor, stream);
}

extern "C" int micf_sw_accumulate_batch(const float* pred, float* out, float* count, const int32_t* coords, int n, int B, int K, int D,
                                        int H, int W, int rd, int rh, int rw, micf_stream_t stream) {
  if (!pred || !out || !count) return MICF_EINVAL;
  Items c;
  if (const int rc = check_items(c, coords, 4, false, n, B, K, D, H, W, rd, rh, rw)) return rc;
  const int64_t per = (int64_t)K * rd * rh * rw;
  hipLaunchKernelGGL(sw_accumulate_batch_kernel, dim3(blocks_for(per), n), dim3(kThreads), 0, (hipStream_t)stream, pred, out, count, c,
                     K, D, H, W, rd, rh, rw, per);
  MICF_RETURN_LAUNCH();
}

extern "C" int micf_sw_normalize(float* out, const float* count, int K, int64_t V, micf_stream_t stream) {
  if (!out || !count || K <= 0 || V <= 0) return MICF_EINVAL;
  const int64_t total = (int64_t)K * V;
  // (a pass over the whole volume, not a window: it keeps the wider grid it has always had)
  hipLaunchKernelGGL(sw_normalize_kernel, dim3(blocks_for(total, 8 * kBlocks)), dim3(kThreads), 0, (hipStream_t)stream, out, count, V,
                     total);
  MICF_RETURN_LAUNCH();
}
