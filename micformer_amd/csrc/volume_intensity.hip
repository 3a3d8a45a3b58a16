// volume_intensity.hip -- on-device intensity augmentation (include/micformer_intensity.h): noise, Gaussian blur, multiplicative
// brightness, contrast and gamma on a batch [B][C][D][H][W] that is already on the device.  Index, weight and random-number
// arithmetic: intensity_coords.h (host-callable).
//
// Launch plan of micf_intensity_augment (fixed by the shape; every kernel reads `params` / `seeds` on the device, a volume
// (b, c) never shares a block with another):
//   0 prep      one thread per volume: sigma clamped, the radius and the 17 normalised weights -> the volume's record
//   1 blur_wh   noise, then the blur along W and along H of one 16 x 64 tile of one z-slice in LDS (tile plus an 8-voxel halo,
//               reflected indices; the noise of a halo voxel is recomputed from its own index) -> float32 workspace.  Without a
//               blur the block only converts (and adds the noise).
//   2 blur_d    one (h, w) column per thread, coalesced along W, marching along D in place: a ring of 32 slices of the
//               block's columns in LDS holds the unblurred values a later output still needs (the whole column where
//               D <= 32, which covers axes shorter than the radius and their repeated reflection).  The same pass sums the
//               blurred value (and its product with the brightness) in float64 and takes min and max: one partial per block.
//   3 finish_a  one block per volume: the partials in a fixed order -> mean, min, max
//   4 moments   retain_stats volumes only: float64 sums of (v - p) and (v - p)^2 of the value before and after the power law
//               about a pivot p (the mean after the brightness; no cancellation against the mean), one partial per block
//   5 finish_c  fixed-order finish -> m0, s0, mean and std after the power law; writes `stats`
//   6 apply     the pointwise chain from the float32 workspace, rounded once to the output dtype
// Min and max after brightness and contrast are the images of the blurred channel's min and max under the same float32
// expressions (pre_gamma below is monotone for positive brightness and contrast), so only the sums need passes.
// Kept form: this separable one.  A fused single-tile 3-D form was not built: with an 8-voxel halo on three axes a tile that
// fits the LDS reads at least 5 voxels per voxel it writes.
#include "common.h"

#include <hip/hip_fp16.h>

#include <type_traits>

#include "../../include/micformer_intensity.h"
#include "intensity_coords.h"

#pragma clang fp contract(off)      // the chain's expressions round the same way in every kernel that evaluates them

namespace micf {
namespace {

namespace I = micf_intensity;

constexpr int kTH = 16, kTW = 64, kHalo = I::kMaxRadius;       // blur_wh's tile
constexpr int kCols = 64, kRing = 32;                        // blur_d's block and ring
constexpr int kThreads = 256;
constexpr int kMomentBlocks = 512, kApplyBlocks = 2048;        // upper bounds of the grid-stride grids, per volume

struct PartA { double sum, sum_b; float mn, mx; };
struct ChanRec {
  float w[I::kTaps];
  int radius, blur;
  double mean, mean_b;          // after the blur; after the brightness
  float mn, mx;                 // after the blur
  double m0, s0, m1, s1;        // before / after the power law (retain_stats)
};

struct Layout { int64_t field, part_a, part_c, recs, total; int blocks_a, blocks_c; };

__host__ int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

__host__ Layout layout(int B, int C, int D, int H, int W) {
  Layout l;
  const int64_t bc = (int64_t)B * C, hw = (int64_t)H * W, n = hw * D;
  l.blocks_a = (int)((hw + kCols - 1) / kCols);
  const int64_t want = (n + 4 * kThreads - 1) / (4 * kThreads);
  l.blocks_c = (int)(want < kMomentBlocks ? want : kMomentBlocks);
  l.field = 0;
  l.part_a = align256(bc * n * 4);
  l.part_c = l.part_a + align256(bc * l.blocks_a * (int64_t)sizeof(PartA));
  l.recs = l.part_c + align256(bc * l.blocks_c * 4 * (int64_t)sizeof(double));
  l.total = l.recs + align256(bc * (int64_t)sizeof(ChanRec));
  return l;
}

__device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld(const __half* p, int64_t i) { return __half2float(p[i]); }
__device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(__half* p, int64_t i, float v) { p[i] = __float2half_rn(v); }

// ---- the pointwise chain ------------------------------------------------------------------------------------------------------

struct Chain {
  bool bright, contrast, gamma, inv, retain;
  float b, c, g;
  float mn, lo, hi;             // contrast: the mean and the clip bounds
  float glo, rng, den;          // gamma: min, max - min, max - min + 1e-7
  float m0, s0, m1, den1;       // retain_stats
  double pivot;                 // of the moment sums
};

__device__ __forceinline__ float pre_gamma(float x, const Chain& k) {
  if (k.bright) x = x * k.b;
  if (k.contrast) {
    const float v = (x - k.mn) * k.c + k.mn;
    x = v < k.lo ? k.lo : (v > k.hi ? k.hi : v);                 // (a NaN stays a NaN)
  }
  return k.inv ? -x : x;
}

// t^gamma of t in [0, 1] as exp2(gamma log2 t) on the hardware's log and exp (1 ulp each): the product's rounding moves the
// result by t^gamma gamma |ln t| 2^-24 <= 2^-24 / e = 2.2e-8 of the range, against a tolerance of 1.7e-6; powf's extended
// precision bound the moments and the apply pass (155 us each for 8 x 2 x 128^3).  log2(0) = -inf gives 0, a NaN stays a NaN.
__device__ __forceinline__ float power(float y, const Chain& k) {
  return __builtin_amdgcn_exp2f(k.g * __builtin_amdgcn_logf((y - k.glo) / k.den)) * k.rng + k.glo;      // v_exp_f32, v_log_f32
}

__device__ Chain make_chain(const float* p, const ChanRec& r) {
  Chain k;
  k.b = p[2];
  k.c = p[3];
  k.g = p[4];
  k.bright = k.b != 1.0f;
  k.contrast = k.c != 1.0f;
  k.gamma = p[5] == 1.0f || p[5] == 2.0f;
  k.inv = false;
  k.retain = k.gamma && p[6] != 0.0f;
  k.mn = (float)r.mean_b;
  k.lo = k.bright ? r.mn * k.b : r.mn;
  k.hi = k.bright ? r.mx * k.b : r.mx;
  const float lo = pre_gamma(r.mn, k), hi = pre_gamma(r.mx, k);  // after the contrast, not yet inverted
  k.inv = k.gamma && p[5] == 2.0f;
  k.glo = k.inv ? -hi : lo;
  k.rng = (k.inv ? -lo : hi) - k.glo;
  k.den = k.rng + 1e-7f;
  k.pivot = k.inv ? -(double)k.mn : (double)k.mn;
  k.m0 = (float)r.m0;
  k.s0 = (float)r.s0;
  k.m1 = (float)r.m1;
  k.den1 = (float)r.s1 + 1e-8f;
  return k;
}

// ---- 0 prep -------------------------------------------------------------------------------------------------------------------

__global__ void intensity_prep_kernel(const float* __restrict__ params, ChanRec* __restrict__ recs, int volumes) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= volumes) return;
  const float sigma = I::clamp_sigma(params[(int64_t)v * 8]);
  float w[I::kTaps];
  const int r = I::blur_weights(sigma, w);
  for (int j = 0; j < I::kTaps; ++j) recs[v].w[j] = w[j];
  recs[v].radius = r;
  recs[v].blur = sigma != 0.0f;                                  // (NaN blurs: it reaches every voxel through the centre weight)
}

// ---- 1 noise, blur along W and H ------------------------------------------------------------------------------------------------

#ifndef MICF_UNROLL
#define MICF_UNROLL _Pragma("unroll")
#endif

// reflect_index without its division where the index is inside the axis, which all but the edge tiles' halos are
__device__ __forceinline__ int reflect_near(int i, int n) { return (unsigned)i < (unsigned)n ? i : I::reflect_index(i, n); }

// f(std::integral_constant<int, r>) for r in [0, kMaxRadius]: r is the same in every thread of a block, so a body may synchronise
template <class F>
__device__ __forceinline__ void dispatch_radius(int r, F&& f) {
  switch (r) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, I::kMaxRadius>{}); break;
  }
}

template <class T>
__global__ void __launch_bounds__(kThreads) intensity_blur_wh_kernel(const T* __restrict__ in, float* __restrict__ field,
                                                                     const float* __restrict__ params,
                                                                     const int64_t* __restrict__ seeds,
                                                                     const ChanRec* __restrict__ recs, int C, int D, int H, int W,
                                                                     int tiles_w) {
  __shared__ float tile[kTH + 2 * kHalo][kTW + 2 * kHalo];
  __shared__ float mid[kTH + 2 * kHalo][kTW];
  __shared__ float wts[I::kTaps];
  const int tid = threadIdx.x, bc = blockIdx.z, z = blockIdx.y;
  const int h0 = (int)(blockIdx.x / tiles_w) * kTH, w0 = (int)(blockIdx.x % tiles_w) * kTW;
  const ChanRec& rec = recs[bc];
  const float noise_std = params[(int64_t)bc * 8 + 1];
  const bool noisy = !(noise_std <= 0.0f);                       // (a NaN propagates)
  const uint64_t key = I::noise_key(seeds[bc / C], bc % C);
  const int64_t plane = (int64_t)z * H * W, base = (int64_t)bc * D * H * W + plane;
  auto fetch = [&](int gy, int gx) {
    const int64_t i = (int64_t)gy * W + gx;
    float v = ld(in, base + i);
    if (noisy) v = v + noise_std * I::normal(I::noise_word(key, (uint64_t)(plane + i)));
    return v;
  };
  if (!rec.blur) {
    for (int idx = tid; idx < kTH * kTW; idx += kThreads) {
      const int gy = h0 + idx / kTW, gx = w0 + idx % kTW;
      if (gy < H && gx < W) field[base + (int64_t)gy * W + gx] = fetch(gy, gx);
    }
    return;
  }
  const int r = rec.radius;                                      // in [0, kHalo] (prep)
  if (tid < I::kTaps) wts[tid] = rec.w[tid];
  for (int idx = tid; idx < (kTH + 2 * kHalo) * (kTW + 2 * kHalo); idx += kThreads) {
    const int ly = idx / (kTW + 2 * kHalo), lx = idx % (kTW + 2 * kHalo);
    if (ly < kHalo - r || ly >= kTH + kHalo + r || lx < kHalo - r || lx >= kTW + kHalo + r) continue;
    tile[ly][lx] = fetch(reflect_near(h0 + ly - kHalo, H), reflect_near(w0 + lx - kHalo, W));
  }
  __syncthreads();
  // the two blurs with the radius a compile-time constant: the weights are registers and the taps unroll
  auto blur_tile = [&](auto radius) {
    constexpr int R = decltype(radius)::value;
    float w[2 * R + 1];
    MICF_UNROLL
    for (int j = 0; j <= 2 * R; ++j) w[j] = wts[kHalo - R + j];
    for (int idx = tid; idx < (kTH + 2 * kHalo) * kTW; idx += kThreads) {
      const int ly = idx / kTW, x = idx % kTW;
      if (ly < kHalo - R || ly >= kTH + kHalo + R) continue;
      float acc = 0.0f;
      MICF_UNROLL
      for (int j = 0; j <= 2 * R; ++j) acc = fmaf(w[j], tile[ly][x + kHalo - R + j], acc);
      mid[ly][x] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < kTH * kTW; idx += kThreads) {
      const int y = idx / kTW, x = idx % kTW;
      float acc = 0.0f;
      MICF_UNROLL
      for (int j = 0; j <= 2 * R; ++j) acc = fmaf(w[j], mid[y + kHalo - R + j][x], acc);
      if (h0 + y < H && w0 + x < W) field[base + (int64_t)(h0 + y) * W + (w0 + x)] = acc;
    }
  };
  dispatch_radius(r, blur_tile);
}

// ---- 2 blur along D, partials ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kCols) intensity_blur_d_kernel(float* __restrict__ field, const float* __restrict__ params,
                                                                 const ChanRec* __restrict__ recs, PartA* __restrict__ parts,
                                                                 int D, int HW) {
  __shared__ float ring[kRing][kCols];
  __shared__ float wts[I::kTaps];
  __shared__ double red_s[kCols], red_b[kCols];
  __shared__ float red_mn[kCols], red_mx[kCols];
  const int tid = threadIdx.x, bc = blockIdx.y;
  const int hw = blockIdx.x * kCols + tid;
  const ChanRec& rec = recs[bc];
  const float b = params[(int64_t)bc * 8 + 2];
  const bool bright = b != 1.0f;
  const int r = rec.radius;
  if (tid < I::kTaps) wts[tid] = rec.w[tid];
  __syncthreads();
  double s = 0.0, sb = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  auto take = [&](float v) {
    s += (double)v;
    sb += (double)(bright ? v * b : v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  };
  if (hw < HW) {
    float* col = field + (int64_t)bc * D * HW + hw;
    if (!rec.blur) {
      for (int z = 0; z < D; ++z) take(col[(int64_t)z * HW]);
    } else {
      auto march = [&](auto radius) {                            // (the radius a compile-time constant, as in blur_wh)
        constexpr int R = decltype(radius)::value;
        float w[2 * R + 1];
        MICF_UNROLL
        for (int j = 0; j <= 2 * R; ++j) w[j] = wts[kHalo - R + j];
        int loaded = 0;
        for (int z = 0; z < D; ++z) {
          // D > 32: every tap of z reflects into [z - 8, min(z + 8, D - 1)], 17 slices of the ring's 32; D <= 32: the whole column
          const int limit = D <= kRing ? D - 1 : (z + kHalo < D - 1 ? z + kHalo : D - 1);
          for (; loaded <= limit; ++loaded) ring[loaded & (kRing - 1)][tid] = col[(int64_t)loaded * HW];
          float acc = 0.0f;
          if (z - R >= 0 && z + R < D) {
            MICF_UNROLL
            for (int j = 0; j <= 2 * R; ++j) acc = fmaf(w[j], ring[(z - R + j) & (kRing - 1)][tid], acc);
          } else {
            MICF_UNROLL
            for (int j = 0; j <= 2 * R; ++j) acc = fmaf(w[j], ring[I::reflect_index(z - R + j, D) & (kRing - 1)][tid], acc);
          }
          col[(int64_t)z * HW] = acc;
          take(acc);
        }
      };
      dispatch_radius(r, march);
    }
  }
  red_s[tid] = s;
  red_b[tid] = sb;
  red_mn[tid] = mn;
  red_mx[tid] = mx;
  __syncthreads();
  for (int o = kCols / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red_s[tid] += red_s[tid + o];
      red_b[tid] += red_b[tid + o];
      red_mn[tid] = fminf(red_mn[tid], red_mn[tid + o]);
      red_mx[tid] = fmaxf(red_mx[tid], red_mx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) parts[(int64_t)bc * gridDim.x + blockIdx.x] = PartA{red_s[0], red_b[0], red_mn[0], red_mx[0]};
}

// ---- 3 finish of the partials ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) intensity_finish_a_kernel(const PartA* __restrict__ parts, ChanRec* __restrict__ recs,
                                                                      int blocks, double voxels) {
  __shared__ double red_s[kThreads], red_b[kThreads];
  __shared__ float red_mn[kThreads], red_mx[kThreads];
  const int tid = threadIdx.x, bc = blockIdx.x;
  double s = 0.0, sb = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int j = tid; j < blocks; j += kThreads) {
    const PartA p = parts[(int64_t)bc * blocks + j];
    s += p.sum;
    sb += p.sum_b;
    mn = fminf(mn, p.mn);
    mx = fmaxf(mx, p.mx);
  }
  red_s[tid] = s;
  red_b[tid] = sb;
  red_mn[tid] = mn;
  red_mx[tid] = mx;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red_s[tid] += red_s[tid + o];
      red_b[tid] += red_b[tid + o];
      red_mn[tid] = fminf(red_mn[tid], red_mn[tid + o]);
      red_mx[tid] = fmaxf(red_mx[tid], red_mx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    recs[bc].mean = red_s[0] / voxels;
    recs[bc].mean_b = red_b[0] / voxels;
    recs[bc].mn = red_mn[0];
    recs[bc].mx = red_mx[0];
  }
}

// ---- 4 moments before and after the power law --------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) intensity_moments_kernel(const float* __restrict__ field, const float* __restrict__ params,
                                                                     const ChanRec* __restrict__ recs, double* __restrict__ parts,
                                                                     int64_t voxels) {
  __shared__ double red[4][kThreads];
  const int tid = threadIdx.x, bc = blockIdx.y;
  const Chain k = make_chain(params + (int64_t)bc * 8, recs[bc]);
  if (!k.retain) return;                                         // (uniform over the block)
  const float* x = field + (int64_t)bc * voxels;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < voxels; i += (int64_t)gridDim.x * kThreads) {
    const float y = pre_gamma(x[i], k);
    const double dy = (double)y - k.pivot, dz = (double)power(y, k) - k.pivot;
    a[0] += dy;
    a[1] += dy * dy;
    a[2] += dz;
    a[3] += dz * dz;
  }
  for (int j = 0; j < 4; ++j) red[j][tid] = a[j];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
      for (int j = 0; j < 4; ++j) red[j][tid] += red[j][tid + o];
    __syncthreads();
  }
  if (tid < 4) parts[((int64_t)bc * gridDim.x + blockIdx.x) * 4 + tid] = red[tid][0];
}

// ---- 5 their finish, `stats` ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) intensity_finish_c_kernel(const double* __restrict__ parts, const float* __restrict__ params,
                                                                      ChanRec* __restrict__ recs, double* __restrict__ stats,
                                                                      int blocks, double voxels) {
  __shared__ double red[4][kThreads];
  const int tid = threadIdx.x, bc = blockIdx.x;
  const Chain k = make_chain(params + (int64_t)bc * 8, recs[bc]);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (k.retain)
    for (int j = tid; j < blocks; j += kThreads)
      for (int q = 0; q < 4; ++q) a[q] += parts[((int64_t)bc * blocks + j) * 4 + q];
  for (int q = 0; q < 4; ++q) red[q][tid] = a[q];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o)
      for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double m0 = 0.0, s0 = 0.0, m1 = 0.0, s1 = 0.0;
    if (k.retain) {
      const double ey = red[0][0] / voxels, ez = red[2][0] / voxels;
      const double vy = red[1][0] / voxels - ey * ey, vz = red[3][0] / voxels - ez * ez;
      m0 = k.pivot + ey;
      m1 = k.pivot + ez;
      s0 = vy < 0.0 ? 0.0 : sqrt(vy);                            // (a NaN stays a NaN)
      s1 = vz < 0.0 ? 0.0 : sqrt(vz);
    }
    recs[bc].m0 = m0;
    recs[bc].s0 = s0;
    recs[bc].m1 = m1;
    recs[bc].s1 = s1;
    if (stats != nullptr) {
      double* o = stats + (int64_t)bc * 8;
      o[0] = recs[bc].mean;
      o[1] = (double)recs[bc].mn;
      o[2] = (double)recs[bc].mx;
      o[3] = m0;
      o[4] = s0;
      o[5] = m1;
      o[6] = s1;
      o[7] = 0.0;
    }
  }
}

// ---- 6 the chain and the store ---------------------------------------------------------------------------------------------------

template <class T>
__global__ void __launch_bounds__(kThreads) intensity_apply_kernel(const float* __restrict__ field, T* __restrict__ out,
                                                                   const float* __restrict__ params,
                                                                   const ChanRec* __restrict__ recs, int64_t voxels) {
  const int bc = blockIdx.y;
  const Chain k = make_chain(params + (int64_t)bc * 8, recs[bc]);
  const float* x = field + (int64_t)bc * voxels;
  T* o = out + (int64_t)bc * voxels;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < voxels; i += (int64_t)gridDim.x * kThreads) {
    float v = pre_gamma(x[i], k);
    if (k.gamma) {
      v = power(v, k);
      if (k.retain) v = (v - k.m1) / k.den1 * k.s0 + k.m0;
      if (k.inv) v = -v;
    }
    st(o, i, v);
  }
}

int check(const void* in, void* out, int dtype, int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  if (dtype != MICF_INTENSITY_F32 && dtype != MICF_INTENSITY_F16) return MICF_EINVAL;
  const uintptr_t mask = dtype == MICF_INTENSITY_F32 ? 3 : 1;
  if (in != nullptr && ((uintptr_t)in & mask)) return MICF_EINVAL;
  if (out != nullptr && ((uintptr_t)out & mask)) return MICF_EINVAL;
  return MICF_OK;
}

int supported(int B, int C, int D, int H, int W) {
  if (C > MICF_INTENSITY_MAX_CHANNELS || D > MICF_INTENSITY_MAX_EXTENT || H > MICF_INTENSITY_MAX_EXTENT ||
      W > MICF_INTENSITY_MAX_EXTENT || (int64_t)B * C > MICF_INTENSITY_MAX_VOLUMES)
    return MICF_EUNSUPPORTED;
  return MICF_OK;
}

template <class T>
int run(const T* in, T* out, int B, int C, int D, int H, int W, const float* params, const int64_t* seeds, char* ws, double* stats,
        hipStream_t s) {
  const Layout l = layout(B, C, D, H, W);
  const int volumes = B * C, hw = H * W;
  const int64_t voxels = (int64_t)hw * D;
  float* field = (float*)(ws + l.field);
  PartA* part_a = (PartA*)(ws + l.part_a);
  double* part_c = (double*)(ws + l.part_c);
  ChanRec* recs = (ChanRec*)(ws + l.recs);
  const int tiles_w = (W + kTW - 1) / kTW, tiles_h = (H + kTH - 1) / kTH;
  const int64_t want = (voxels + kThreads - 1) / kThreads;
  const int apply_blocks = (int)(want < kApplyBlocks ? want : kApplyBlocks);
  hipLaunchKernelGGL(intensity_prep_kernel, dim3((volumes + 63) / 64), dim3(64), 0, s, params, recs, volumes);
  hipLaunchKernelGGL(intensity_blur_wh_kernel<T>, dim3(tiles_w * tiles_h, D, volumes), dim3(kThreads), 0, s, in, field, params, seeds,
                     recs, C, D, H, W, tiles_w);
  hipLaunchKernelGGL(intensity_blur_d_kernel, dim3(l.blocks_a, volumes), dim3(kCols), 0, s, field, params, recs, part_a, D, hw);
  hipLaunchKernelGGL(intensity_finish_a_kernel, dim3(volumes), dim3(kThreads), 0, s, part_a, recs, l.blocks_a, (double)voxels);
  hipLaunchKernelGGL(intensity_moments_kernel, dim3(l.blocks_c, volumes), dim3(kThreads), 0, s, field, params, recs, part_c, voxels);
  hipLaunchKernelGGL(intensity_finish_c_kernel, dim3(volumes), dim3(kThreads), 0, s, part_c, params, recs, stats, l.blocks_c,
                     (double)voxels);
  hipLaunchKernelGGL(intensity_apply_kernel<T>, dim3(apply_blocks, volumes), dim3(kThreads), 0, s, field, out, params, recs, voxels);
  MICF_RETURN_LAUNCH();
}

}  // namespace
}  // namespace micf

using namespace micf;

extern "C" int64_t micf_intensity_augment_workspace(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  const int rc = supported(B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  return layout(B, C, D, H, W).total;
}

extern "C" int micf_intensity_augment(const void* in, void* out, int dtype, int B, int C, int D, int H, int W, const float* params,
                                      const int64_t* seeds, void* workspace, int64_t workspace_bytes, double* stats,
                                      micf_stream_t stream) {
  int rc = check(in, out, dtype, B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  if (in == nullptr || out == nullptr || params == nullptr || seeds == nullptr || workspace == nullptr) return MICF_EINVAL;
  if (((uintptr_t)params & 3) || ((uintptr_t)seeds & 7) || ((uintptr_t)stats & 7) || ((uintptr_t)workspace & 255)) return MICF_EINVAL;
  rc = supported(B, C, D, H, W);
  if (rc != MICF_OK) return rc;
  if (workspace_bytes < layout(B, C, D, H, W).total) return MICF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MICF_INTENSITY_F32)
    return run<float>((const float*)in, (float*)out, B, C, D, H, W, params, seeds, (char*)workspace, stats, s);
  return run<__half>((const __half*)in, (__half*)out, B, C, D, H, W, params, seeds, (char*)workspace, stats, s);
}
