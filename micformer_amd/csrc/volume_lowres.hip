// volume_lowres.hip -- on-device low-resolution simulation (include/micformer_lowres.h): nearest downsample to a per-channel
// target, cubic B-spline prefilter, cubic B-spline upsample back, on a batch [B][C][D][H][W] that is already on the device.
// Index, weight and prefilter-start arithmetic: lowres_coords.h (host-callable).
//
// The coefficients of a channel with target (td, th, tw) live in the workspace as a compact float32 array
// [td + 4][th + 4][tw + 4]: index k + 2 holds coefficient k, k in -2 .. t + 1, so that no tap of the upsample clamps.
// Launch plan of micf_lowres_simulate (fixed by the shape; every kernel reads `target` on the device, a volume (b, c) never shares
// a block with another; a channel that is off leaves kernels 1-3 at once):
//   1 gather_w  `lines` <= 64 lines (od, oh) of the low volume per block: the nearest gather from `in` into LDS (lanes across W, a
//               wave per line), then one lane per line runs the two recursions along W in LDS, then the lines with their four
//               extension entries go to the workspace (lanes across W again)
//   2 axis<H>   one column (od, w) per thread, lanes across W: the recursions along H in place, rows -2, -1, th, th + 1 written
//   3 axis<D>   one column (h, w) per thread over the extended plane: the same along D
//   4 upsample  one 4 x 8 x 64 output tile per block from the <= 7 x 11 x 67 coefficients under it: 4 taps along D from registers
//               (a column per thread, lanes across W), then 4 along H and 4 along W through LDS (14 multiply-adds per voxel
//               against the 64 of a direct gather), rounded once and stored 16 bytes per lane where W and the pointer allow.
//               A channel that is off is copied (or left alone when out == in).
#include "common.h"

#include <hip/hip_fp16.h>

#include "../../include/micformer_lowres.h"
#include "lowres_coords.h"

#pragma clang fp contract(off)

namespace micf {
namespace {

namespace L = micf_lowres;

constexpr int kWave = 64;
constexpr int kLineFloats = 10240;                             // gather_w's LDS: lines x pitch floats
constexpr int kTD = 4, kTH = 8, kTW = 64;                      // upsample's output tile
constexpr int kSD = kTD + 3, kSH = kTH + 3, kSW = kTW + 3;     // the coefficients a tile reads, at most (ratio t / n <= 1)
constexpr int kSWp = kSW + 1;
constexpr int kThreads = 256;

__device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); }

struct Target { int d, h, w; bool off; };

__device__ __forceinline__ Target read_target(const int32_t* __restrict__ target, int bc, int D, int H, int W) {
  Target t;
  t.d = L::clamp_target(target[(int64_t)bc * 3 + 0], D);
  t.h = L::clamp_target(target[(int64_t)bc * 3 + 1], H);
  t.w = L::clamp_target(target[(int64_t)bc * 3 + 2], W);
  t.off = t.d == D && t.h == H && t.w == W;
  return t;
}

__host__ __device__ inline int line_pitch(int W) { return (W + 2 * L::kExt) | 1; }      // odd: a lane per line hits its own bank
__host__ inline int lines_per_block(int W) {
  const int l = kLineFloats / line_pitch(W);
  return l > kWave ? kWave : l;                                // >= 4 at W = 2048
}
__host__ __device__ inline int64_t channel_floats(int D, int H, int W) {
  return (int64_t)(D + 2 * L::kExt) * (H + 2 * L::kExt) * (W + 2 * L::kExt);
}

// The two recursions of lowres_coords.h over the n entries s[0], s[stride], ... in place, then the four extension entries.  kBatch
// values are loaded before the first of them is used and stored after the last, so that a step waits for its multiply-add and not
// for memory (one load, one step, one store at a time ran the H and D passes at the memory latency: LABNOTES).
template <int kBatch, class Index>
__device__ __forceinline__ void prefilter_line(float* s, int n, Index stride) {
  float v[kBatch];
  float p = 0.0f, s0 = 0.0f, se = 0.0f;
  for (int k0 = 0; k0 < n; k0 += kBatch) {
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 + j < n) v[j] = s[(Index)(k0 + j) * stride];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 + j < n) {
        if (k0 + j == 0) {
          s0 = v[j];
          p = L::causal_first(v[j]);
        } else {
          p = L::causal_next(p, v[j]);
        }
        if (k0 + j == n - 1) se = v[j];
        v[j] = p;
      }
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 + j < n) s[(Index)(k0 + j) * stride] = v[j];
  }
  float c = 0.0f, ce = 0.0f;
  for (int k0 = n - 1; k0 >= 0; k0 -= kBatch) {
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 - j >= 0) v[j] = s[(Index)(k0 - j) * stride];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 - j >= 0) {
        if (k0 - j == n - 1) {
          c = L::anticausal_last(v[j], se);
          ce = c;
        } else {
          c = L::anticausal_next(c, v[j]);
        }
        v[j] = c;
      }
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 - j >= 0) s[(Index)(k0 - j) * stride] = v[j];
  }
  s[-stride] = L::extend1(c, s0);
  s[-2 * stride] = L::extend2(c, s0);
  s[(Index)n * stride] = L::extend1(ce, se);
  s[(Index)(n + 1) * stride] = L::extend2(ce, se);
}

// ---- 1 gather + prefilter along W ---------------------------------------------------------------------------------------------

template <class T>
__global__ void __launch_bounds__(kThreads) lowres_gather_w_kernel(const T* __restrict__ in, float* __restrict__ coef,
                                                                   const int32_t* __restrict__ target, int D, int H, int W,
                                                                   int lines) {
  __shared__ float buf[kLineFloats];
  __shared__ int64_t src_row[kWave], dst_row[kWave];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, bc = blockIdx.y;
  const Target t = read_target(target, bc, D, H, W);
  if (t.off) return;
  const int total = t.d * t.h, first = blockIdx.x * lines;
  if (first >= total) return;
  const int pitch = line_pitch(W), pw = t.w + 2 * L::kExt;
  const int here = total - first < lines ? total - first : lines;
  if (tid < here) {
    const int od = (first + tid) / t.h, oh = (first + tid) % t.h;
    src_row[tid] = ((int64_t)L::gather_index(od, D, t.d) * H + L::gather_index(oh, H, t.h)) * W;
    dst_row[tid] = ((int64_t)(od + L::kExt) * (t.h + 2 * L::kExt) + (oh + L::kExt)) * pw;
  }
  __syncthreads();
  const T* x = in + (int64_t)bc * D * H * W;
  for (int ow = lane; ow < t.w; ow += kWave) {
    const int g = L::gather_index(ow, W, t.w);
#pragma unroll 8
    for (int l = wave; l < here; l += kThreads / kWave) buf[l * pitch + L::kExt + ow] = ld(x, src_row[l] + g);
  }
  __syncthreads();
  if (tid < here) prefilter_line<8, int>(buf + tid * pitch + L::kExt, t.w, 1);
  __syncthreads();
  float* dst = coef + (int64_t)bc * channel_floats(D, H, W);
  for (int l = wave; l < here; l += kThreads / kWave)
    for (int e = lane; e < pw; e += kWave) dst[dst_row[l] + e] = buf[l * pitch + e];
}

// ---- 2, 3 prefilter along H and along D -----------------------------------------------------------------------------------------

// kAxis 1: columns (od, w), od < td, w < tw + 4, marching along H.  kAxis 0: columns (h, w) of the extended plane, along D.
template <int kAxis>
__global__ void __launch_bounds__(kWave) lowres_axis_kernel(float* __restrict__ coef, const int32_t* __restrict__ target, int D,
                                                            int H, int W) {
  const int bc = blockIdx.y;
  const Target t = read_target(target, bc, D, H, W);
  if (t.off) return;
  const int pw = t.w + 2 * L::kExt;
  const int64_t plane = (int64_t)(t.h + 2 * L::kExt) * pw;
  const int64_t col = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t cols = kAxis == 1 ? (int64_t)t.d * pw : plane;
  if (col >= cols) return;
  const int n = kAxis == 1 ? t.h : t.d;
  const int64_t stride = kAxis == 1 ? pw : plane;
  float* s = coef + (int64_t)bc * channel_floats(D, H, W);
  if (kAxis == 1)
    s += (col / pw + L::kExt) * plane + L::kExt * (int64_t)pw + col % pw;
  else
    s += L::kExt * plane + col;
  prefilter_line<16, int64_t>(s, n, stride);
}

// ---- 4 upsample and store -------------------------------------------------------------------------------------------------------

template <class T>
struct alignas(16) Pack { T v[16 / sizeof(T)]; };

__device__ __forceinline__ float taps4(const float* w, float c0, float c1, float c2, float c3) {
  return fmaf(w[3], c3, fmaf(w[2], c2, fmaf(w[1], c1, w[0] * c0)));
}

template <class T, bool kVec>
__global__ void __launch_bounds__(kThreads) lowres_upsample_kernel(const T* in, T* out,
                                                                   const float* __restrict__ coef,
                                                                   const int32_t* __restrict__ target, int D, int H, int W,
                                                                   int tiles_h, int tiles_w) {
  constexpr int kV = 16 / (int)sizeof(T);                      // outputs per 16-byte store
  __shared__ float fa[kTD * kSH * kSWp];                       // after the taps along D; later the finished tile [32][kTW]
  __shared__ float fb[kTD * kTH * kSWp];                       // after the taps along H
  __shared__ float wts[kTD + kTH + kTW][4];
  __shared__ int base[kTD + kTH + kTW];                        // first tap of an output coordinate, relative to the tile's first
  const int tid = threadIdx.x, bc = blockIdx.y;
  const int o0w = (int)(blockIdx.x % tiles_w) * kTW, o0h = (int)(blockIdx.x / tiles_w % tiles_h) * kTH;
  const int o0d = (int)(blockIdx.x / tiles_w / tiles_h) * kTD;
  const Target t = read_target(target, bc, D, H, W);
  const int64_t vol = (int64_t)bc * D * H * W;
  const int nd = D - o0d < kTD ? D - o0d : kTD, nh = H - o0h < kTH ? H - o0h : kTH, nw = W - o0w < kTW ? W - o0w : kTW;
  if (t.off) {
    if (out == in) return;
    if (kVec) {
      for (int c = tid; c < kTD * kTH * (kTW / kV); c += kThreads) {
        const int x = c % (kTW / kV) * kV, y = c / (kTW / kV) % kTH, z = c / (kTW / kV) / kTH;
        if (z >= nd || y >= nh || x >= nw) continue;
        const int64_t i = vol + ((int64_t)(o0d + z) * H + (o0h + y)) * W + o0w + x;
        *reinterpret_cast<Pack<T>*>(out + i) = *reinterpret_cast<const Pack<T>*>(in + i);
      }
    } else {
      for (int c = tid; c < kTD * kTH * kTW; c += kThreads) {
        const int x = c % kTW, y = c / kTW % kTH, z = c / kTW / kTH;
        if (z >= nd || y >= nh || x >= nw) continue;
        const int64_t i = vol + ((int64_t)(o0d + z) * H + (o0h + y)) * W + o0w + x;
        out[i] = in[i];
      }
    }
    return;
  }
  // the coefficient range of the tile per axis, in workspace indices (coefficient k at k + 2): first = floor(s(first output)) - 1
  // + 2, last = floor(s(last output)) + 2 + 2; the count is at most tile + 3 because s advances by t / n <= 1 per output
  float f;
  const int lo_d = L::tap_floor(o0d, D, t.d, &f) + 1, lo_h = L::tap_floor(o0h, H, t.h, &f) + 1, lo_w = L::tap_floor(o0w, W, t.w, &f) + 1;
  int cd = L::tap_floor(o0d + nd - 1, D, t.d, &f) + 4 - lo_d + 1, ch = L::tap_floor(o0h + nh - 1, H, t.h, &f) + 4 - lo_h + 1;
  int cw = L::tap_floor(o0w + nw - 1, W, t.w, &f) + 4 - lo_w + 1;
  cd = cd > kSD ? kSD : cd;                                    // (never taken: the bound above)
  ch = ch > kSH ? kSH : ch;
  cw = cw > kSW ? kSW : cw;
  if (tid < kTD + kTH + kTW) {
    int o, n, tt, lo, cnt;
    if (tid < kTD) { o = o0d + tid; n = D; tt = t.d; lo = lo_d; cnt = cd; }
    else if (tid < kTD + kTH) { o = o0h + tid - kTD; n = H; tt = t.h; lo = lo_h; cnt = ch; }
    else { o = o0w + tid - kTD - kTH; n = W; tt = t.w; lo = lo_w; cnt = cw; }
    float fr;
    int b = L::tap_floor(o, n, tt, &fr) + 1 - lo;              // (an output beyond the volume clamps to the last one inside)
    b = b < 0 ? 0 : (b > cnt - 4 ? cnt - 4 : b);               // (never taken for an output inside the volume)
    base[tid] = b;
    L::cubic_weights(fr, wts[tid]);
  }
  const int pw = t.w + 2 * L::kExt;
  const int64_t plane = (int64_t)(t.h + 2 * L::kExt) * pw;
  const float* src = coef + (int64_t)bc * channel_floats(D, H, W) + lo_d * plane + (int64_t)lo_h * pw + lo_w;
  __syncthreads();
  // along D first, W last: every stage widens the field by n / t, so the narrow axes go first (7140 four-tap items per tile
  // against 10560 the other way round).  A thread takes the column of <= 7 coefficients straight from the workspace into
  // registers (lanes across W) and makes the tile's 4 outputs along D from them: the first tap is the same in the whole block
  for (int i = tid; i < kSH * kSWp; i += kThreads) {
    const int zh = i / kSWp, x = i % kSWp;
    if (zh >= ch || x >= cw) continue;
    const float* g = src + (int64_t)zh * pw + x;
    float v[kSD];
#pragma unroll
    for (int j = 0; j < kSD; ++j) v[j] = j < cd ? g[j * plane] : 0.0f;
#pragma unroll
    for (int z = 0; z < kTD; ++z) {
      const float* w = wts[z];
      float r;
      switch (__builtin_amdgcn_readfirstlane(base[z])) {       // in [0, cd - 4], cd <= 7
        case 0: r = taps4(w, v[0], v[1], v[2], v[3]); break;
        case 1: r = taps4(w, v[1], v[2], v[3], v[4]); break;
        case 2: r = taps4(w, v[2], v[3], v[4], v[5]); break;
        default: r = taps4(w, v[3], v[4], v[5], v[6]); break;
      }
      fa[(z * kSH + zh) * kSWp + x] = r;
    }
  }
  __syncthreads();
  for (int i = tid; i < kTD * kTH * kSWp; i += kThreads) {      // along H
    const int x = i % kSWp, y = i / kSWp % kTH, z = i / (kSWp * kTH);
    if (x >= cw) continue;
    const float* c = fa + (z * kSH + base[kTD + y]) * kSWp + x;
    fb[i] = taps4(wts[kTD + y], c[0], c[kSWp], c[2 * kSWp], c[3 * kSWp]);
  }
  __syncthreads();
  float* fin = fa;                                             // [kTD * kTH][kTW]
  {                                                            // along W: the thread's ow is the same for every row
    const int lane = tid % kWave, iw = kTD + kTH + lane, b = base[iw];
    const float w[4] = {wts[iw][0], wts[iw][1], wts[iw][2], wts[iw][3]};
    for (int r = tid / kWave; r < kTD * kTH; r += kThreads / kWave) {
      const float* c = fb + r * kSWp + b;
      fin[r * kTW + lane] = taps4(w, c[0], c[1], c[2], c[3]);
    }
  }
  __syncthreads();
  for (int c = tid; c < kTD * kTH * (kTW / kV); c += kThreads) {
    const int x = c % (kTW / kV) * kV, y = c / (kTW / kV) % kTH, z = c / (kTW / kV) / kTH;
    if (z >= nd || y >= nh || x >= nw) continue;
    const float* p = fin + (z * kTH + y) * kTW + x;
    const int64_t i = vol + ((int64_t)(o0d + z) * H + (o0h + y)) * W + o0w + x;
    if (kVec) {
      Pack<T> q;
#pragma unroll
      for (int j = 0; j < kV; ++j) st(q.v, j, p[j]);
      *reinterpret_cast<Pack<T>*>(out + i) = q;
    } else {
#pragma unroll
      for (int j = 0; j < kV; ++j)
        if (x + j < nw) st(out, i + j, p[j]);
    }
  }
}

int check(const void* in, void* out, int dtype, int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  if (dtype != MICF_LOWRES_F32 && dtype != MICF_LOWRES_F16) return MICF_EINVAL;
  const uintptr_t mask = dtype == MICF_LOWRES_F32 ? 3 : 1;
  if (in != nullptr && ((uintptr_t)in & mask)) return MICF_EINVAL;
  if (out != nullptr && ((uintptr_t)out & mask)) return MICF_EINVAL;
  return MICF_OK;
}

int supported(int B, int C, int D, int H, int W) {
  if (C > MICF_LOWRES_MAX_CHANNELS || D > MICF_LOWRES_MAX_EXTENT || H > MICF_LOWRES_MAX_EXTENT || W > MICF_LOWRES_MAX_EXTENT ||
      (int64_t)B * C > MICF_LOWRES_MAX_VOLUMES)
    return MICF_EUNSUPPORTED;
  return MICF_OK;
}

int64_t workspace_bytes_of(int B, int C, int D, int H, int W) {
  return ((int64_t)B * C * channel_floats(D, H, W) * 4 + 255) / 256 * 256;
}

template <class T>
int run(const T* in, T* out, int B, int C, int D, int H, int W, const int32_t* target, float* coef, hipStream_t s) {
  const int volumes = B * C, lines = lines_per_block(W);
  const int blocks_w = (int)(((int64_t)D * H + lines - 1) / lines);
  const int blocks_h = (int)(((int64_t)D * (W + 2 * L::kExt) + kWave - 1) / kWave);
  const int blocks_d = (int)(((int64_t)(H + 2 * L::kExt) * (W + 2 * L::kExt) + kWave - 1) / kWave);
  const int tiles_d = (D + kTD - 1) / kTD, tiles_h = (H + kTH - 1) / kTH, tiles_w = (W + kTW - 1) / kTW;
  constexpr int kV = 16 / (int)sizeof(T);
  const bool vec = W % kV == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  hipLaunchKernelGGL(lowres_gather_w_kernel<T>, dim3(blocks_w, volumes), dim3(kThreads), 0, s, in, coef, target, D, H, W, lines);
  hipLaunchKernelGGL(lowres_axis_kernel<1>, dim3(blocks_h, volumes), dim3(kWave), 0, s, coef, target, D, H, W);
  hipLaunchKernelGGL(lowres_axis_kernel<0>, dim3(blocks_d, volumes), dim3(kWave), 0, s, coef, target, D, H, W);
  if (vec)
    hipLaunchKernelGGL((lowres_upsample_kernel<T, true>), dim3(tiles_d * tiles_h * tiles_w, volumes), dim3(kThreads), 0, s, in, out,
                       coef, target, D, H, W, tiles_h, tiles_w);
  else
    hipLaunchKernelGGL((lowres_upsample_kernel<T, false>), dim3(tiles_d * tiles_h * tiles_w, volumes), dim3(kThreads), 0, s, in, out,
                       coef, target, D, H, W, tiles_h, tiles_w);
  MICF_RETURN_LAUNCH();
}

}  // namespace
}  // namespace micf

using namespace micf;

extern "C" int64_t micf_lowres_workspace(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  const int rc = supported(B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  return workspace_bytes_of(B, C, D, H, W);
}

extern "C" int micf_lowres_simulate(const void* in, void* out, int dtype, int B, int C, int D, int H, int W, const int32_t* target,
                                    void* workspace, int64_t workspace_bytes, micf_stream_t stream) {
  int rc = check(in, out, dtype, B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  if (in == nullptr || out == nullptr || target == nullptr || workspace == nullptr) return MICF_EINVAL;
  if (((uintptr_t)target & 3) || ((uintptr_t)workspace & 255)) return MICF_EINVAL;
  rc = supported(B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  if (workspace_bytes < workspace_bytes_of(B, C, D, H, W)) return MICF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MICF_LOWRES_F32) return run<float>((const float*)in, (float*)out, B, C, D, H, W, target, (float*)workspace, s);
  return run<__half>((const __half*)in, (__half*)out, B, C, D, H, W, target, (float*)workspace, s);
}
