// volume_loader_common.h -- what volume_loader.hip (min-max only), volume_normalise.hip (min-max / z-score / percentile clip per
// channel) and volume_affine.hip (an affine map in the resample) share: the descriptors that travel as kernel arguments, the
// order-preserving keys, the min / max pass over a raw volume, the resize + label + crop-extent pass templated on the per-channel
// normaliser and the pieces volume_affine.hip's resample reuses (crop extents, label lookup), the zero and crop kernels, and the host
// side: argument checks and the iterator over chunks of samples.  Everything lives in an unnamed namespace, so each including file
// gets its own copy; nothing uses scratch.
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"
#include "../../include/micformer_loader.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 8;                   // samples per launch (their descriptors travel as kernel arguments)
constexpr int kMaxExtent = 2048;
constexpr int64_t kMaxTarget = (int64_t)512 * 512 * 512;

typedef short short8 __attribute__((ext_vector_type(8)));

struct RawVol { const void* p; int64_t n; int dtype; int pad; };
struct MinMaxArgs { RawVol v[2 * kChunk]; };

struct Vol3 { const void* p; int d, h, w, dtype; };
struct SampleDesc { Vol3 ct, mr, lab; };
struct ResizeArgs { SampleDesc s[kChunk]; int nvals; int vals[MICF_LOADER_MAX_LABEL_VALUES]; };

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

// order-preserving keys: a < b  <=>  key(a) < key(b) as unsigned
__device__ __forceinline__ uint32_t key_i16(int x) { return (uint32_t)(x + 32768); }
__device__ __forceinline__ int unkey_i16(uint32_t k) { return (int)k - 32768; }
__device__ __forceinline__ uint32_t key_f32(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unkey_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// A raw volume as [0, head) scalar elements, then nvec aligned 16-byte vectors, then the scalar tail from tail0 on.
struct VecSpan {
  int64_t head, nvec, tail0;
  const uint4* vec;
  int nscalar;                                                   // head + tail elements: < 16
};
__device__ __forceinline__ VecSpan vec_span(const void* p, int64_t n, int es) {
  VecSpan s;
  const char* base = static_cast<const char*>(p);
  const int per = 16 / es;
  s.head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) / es;
  if (s.head > n) s.head = n;
  s.nvec = (n - s.head) / per;
  s.tail0 = s.head + s.nvec * per;
  s.vec = reinterpret_cast<const uint4*>(base + s.head * es);
  s.nscalar = (int)(s.head + (n - s.tail0));
  return s;
}

// The 16-byte vectors of a volume that fall to this thread, four loads in flight.
template <class F>
__device__ __forceinline__ void for_each_vec(const VecSpan& sp, int64_t g0, int64_t gs, F&& f) {
  int64_t i = g0;
  for (; i + 3 * gs < sp.nvec; i += 4 * gs) {
    const uint4 q0 = sp.vec[i], q1 = sp.vec[i + gs], q2 = sp.vec[i + 2 * gs], q3 = sp.vec[i + 3 * gs];
    f(q0); f(q1); f(q2); f(q3);
  }
  for (; i < sp.nvec; i += gs) f(sp.vec[i]);
}

// ---- min / max of one raw image volume: two integer atomicMax per block on keys[0] (max of key) and keys[1] (max of ~key) -------
__device__ __forceinline__ void minmax_body(const RawVol& vol, uint32_t* keys, uint32_t* s_red /* [2 * kWaves] */) {
  const int tid = threadIdx.x;
  const bool f32 = vol.dtype == MICF_LOADER_F32;
  const VecSpan sp = vec_span(vol.p, vol.n, f32 ? 4 : 2);
  const int64_t g0 = (int64_t)blockIdx.x * kThreads + tid, gs = (int64_t)gridDim.x * kThreads;
  uint32_t kmax, kmin_inv;
  if (f32) {
    const float* src = static_cast<const float*>(vol.p);
    const float first = src[0];
    float lo[4] = {first, first, first, first}, hi[4] = {first, first, first, first};
    auto take = [&](const uint4& q) {
      const float f[4] = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)};
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo[j] = fminf(lo[j], f[j]); hi[j] = fmaxf(hi[j], f[j]); }
    };
    for_each_vec(sp, g0, gs, take);
    if (blockIdx.x == 0 && tid < sp.nscalar) {
      const float x = src[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)];
      lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
    }
    kmax = key_f32(fmaxf(fmaxf(hi[0], hi[1]), fmaxf(hi[2], hi[3])));
    kmin_inv = ~key_f32(fminf(fminf(lo[0], lo[1]), fminf(lo[2], lo[3])));
  } else {
    const int16_t* src = static_cast<const int16_t*>(vol.p);
    const short first = src[0];
    short8 lo = first, hi = first;                               // packed 16-bit min / max: 4 VALU ops per 16-byte load
    auto take = [&](const uint4& q) {
      short8 h;
      __builtin_memcpy(&h, &q, 16);
      lo = __builtin_elementwise_min(lo, h);
      hi = __builtin_elementwise_max(hi, h);
    };
    for_each_vec(sp, g0, gs, take);
    int mn = lo[0], mx = hi[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) { mn = lo[j] < mn ? lo[j] : mn; mx = hi[j] > mx ? hi[j] : mx; }
    if (blockIdx.x == 0 && tid < sp.nscalar) {
      const int x = src[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)];
      mn = x < mn ? x : mn; mx = x > mx ? x : mx;
    }
    kmax = key_i16(mx);
    kmin_inv = ~key_i16(mn);
  }
  kmax = wave_umax(kmax);
  kmin_inv = wave_umax(kmin_inv);
  if ((tid & 63) == 0) { s_red[tid >> 6] = kmax; s_red[kWaves + (tid >> 6)] = kmin_inv; }
  __syncthreads();
  if (tid < 2) {
    uint32_t r = s_red[tid * kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = s_red[tid * kWaves + w] > r ? s_red[tid * kWaves + w] : r;
    atomicMax(keys + tid, r);
  }
}

// ---- resize + label + crop extents ------------------------------------------------------------------------------------------
// F.interpolate(mode="trilinear", align_corners=False) per axis, in fp32 exactly as written (no contraction into an fma: the tap
// indices are floor() of these numbers)
__device__ __forceinline__ void linear_axis(int o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  const float scale = (float)in / (float)out;
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  i0 = (int)s;
  i0 = i0 < in - 1 ? i0 : in - 1;
  i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
  l1 = s - (float)i0;
  l0 = 1.0f - l1;
}

// F.interpolate(mode="nearest")
__device__ __forceinline__ int nearest_axis(int o, int in, int out) {
#pragma clang fp contract(off)
  const float scale = (float)in / (float)out;
  const int i = (int)floorf((float)o * scale);
  return i < in - 1 ? i : in - 1;
}

// min-max normalisation constants of one volume, decoded from its two keys.  A normaliser is any type N with an overload
// `template <bool F32> float tap(const void* p, int64_t off, const N& nm)`: the normalised value of one raw element.
struct Norm { int imin; float fmin, scale; };

__device__ __forceinline__ Norm load_norm(const uint32_t* k, bool f32) {
  Norm nm;
  const uint32_t kmax = k[0], kmin = ~k[1];
  if (f32) {
    nm.imin = 0;
    nm.fmin = unkey_f32(kmin);
    nm.scale = unkey_f32(kmax) - nm.fmin;                        // fp32 subtract, as numpy on a float32 array
  } else {
    nm.imin = unkey_i16(kmin);
    nm.fmin = 0.0f;
    nm.scale = (float)(unkey_i16(kmax) - nm.imin);               // int32 subtract (<= 65535: exact in fp32)
  }
  return nm;
}

template <bool F32>
__device__ __forceinline__ float tap(const void* p, int64_t off, const Norm& nm) {
  if (F32) return (static_cast<const float*>(p)[off] - nm.fmin) / nm.scale;
  return (float)((int)static_cast<const int16_t*>(p)[off] - nm.imin) / nm.scale;
}

// separable form, outermost axis last (the order of torch's CPU kernel): w fastest
template <bool F32, class N>
__device__ __forceinline__ float trilinear(const Vol3& v, const N& nm, int z, int y, int x, int D, int H, int W) {
  int z0, z1, y0, y1, x0, x1;
  float lz0, lz1, ly0, ly1, lx0, lx1;
  linear_axis(z, v.d, D, z0, z1, lz0, lz1);
  linear_axis(y, v.h, H, y0, y1, ly0, ly1);
  linear_axis(x, v.w, W, x0, x1, lx0, lx1);
  const int64_t r00 = ((int64_t)z0 * v.h + y0) * v.w, r01 = ((int64_t)z0 * v.h + y1) * v.w;
  const int64_t r10 = ((int64_t)z1 * v.h + y0) * v.w, r11 = ((int64_t)z1 * v.h + y1) * v.w;
  const float a00 = tap<F32>(v.p, r00 + x0, nm), b00 = tap<F32>(v.p, r00 + x1, nm);
  const float a01 = tap<F32>(v.p, r01 + x0, nm), b01 = tap<F32>(v.p, r01 + x1, nm);
  const float a10 = tap<F32>(v.p, r10 + x0, nm), b10 = tap<F32>(v.p, r10 + x1, nm);
  const float a11 = tap<F32>(v.p, r11 + x0, nm), b11 = tap<F32>(v.p, r11 + x1, nm);
  const float t00 = a00 * lx0 + b00 * lx1, t01 = a01 * lx0 + b01 * lx1;
  const float t10 = a10 * lx0 + b10 * lx1, t11 = a11 * lx0 + b11 * lx1;
  const float u0 = t00 * ly0 + t01 * ly1, u1 = t10 * ly0 + t11 * ly1;
  return u0 * lz0 + u1 * lz1;
}

// The crop extents of the non-zero voxels one thread has seen: running maxima of (index + 1) and of (extent - index) on z y x,
// 0 = no non-zero voxel seen.
struct Extents {
  uint32_t ez = 0, ey = 0, ex = 0, fz = 0, fy = 0, fx = 0;
  __device__ __forceinline__ void see(int z, int y, int x, int D, int H, int W) {
    ez = max(ez, (uint32_t)(z + 1)); fz = max(fz, (uint32_t)(D - z));
    ey = max(ey, (uint32_t)(y + 1)); fy = max(fy, (uint32_t)(H - y));
    ex = max(ex, (uint32_t)(x + 1)); fx = max(fx, (uint32_t)(W - x));
  }
  // Every thread of the block calls it: wave shuffles, one LDS atomicMax per wave and word on s_ext (six words, zeroed before a
  // barrier), then the block's six global atomicMax on the sample's crop words dst.
  __device__ __forceinline__ void flush(uint32_t* s_ext, uint32_t* dst) {
    const int tid = threadIdx.x;
    ez = wave_umax(ez); ey = wave_umax(ey); ex = wave_umax(ex);
    fz = wave_umax(fz); fy = wave_umax(fy); fx = wave_umax(fx);
    if ((tid & 63) == 0) {
      atomicMax(&s_ext[0], ez); atomicMax(&s_ext[1], ey); atomicMax(&s_ext[2], ex);
      atomicMax(&s_ext[3], fz); atomicMax(&s_ext[4], fy); atomicMax(&s_ext[5], fx);
    }
    __syncthreads();
    if (tid < 6 && s_ext[tid] != 0) atomicMax(dst + tid, s_ext[tid]);
  }
};

// element `off` of a raw label volume
__device__ __forceinline__ int raw_label(const Vol3& lv, int64_t off) {
  return lv.dtype == MICF_LOADER_I32 ? static_cast<const int32_t*>(lv.p)[off] : (int)static_cast<const int16_t*>(lv.p)[off];
}

// raw label value -> class: 0 for 0, k for a.vals[k - 1], 255 elsewhere
__device__ __forceinline__ int label_class(const ResizeArgs& a, int val) {
  int cls = val == 0 ? 0 : 255;
  for (int k = 0; k < a.nvals; ++k) cls = val == a.vals[k] ? k + 1 : cls;
  return cls;
}

// micf_volume_loader's workspace: per sample ct {max key, max ~key}, mr {..}, crop {max+1 z y x, extent-min z y x}
constexpr int kWsWords = 10;
struct LoaderWords {
  typedef uint32_t Ws;
  static __device__ __forceinline__ uint32_t* sample(uint32_t* ws) { return ws + (size_t)blockIdx.y * kWsWords; }
  static __device__ __forceinline__ Norm norm(const uint32_t* wsb, int c, bool f32) { return load_norm(wsb + 2 * c, f32); }
  static __device__ __forceinline__ constexpr bool stores(const uint32_t*, int) { return true; }
  static __device__ __forceinline__ uint32_t* ext(uint32_t* wsb) { return wsb + 4; }
};

// The resize kernel, grid (blocks, samples of the chunk); ws / image / label_map point at the chunk's first sample.  A kernel
// template and not a body called from two kernels: ResizeArgs must stay the kernel's own by-value argument for the code (and
// with it the fma contraction, i.e. the bits) of volume_loader.hip's instance to stay what it has always been.  The policy P
// says where a sample's workspace lies and what it means: P::sample(ws) -> the block's sample, P::norm(wsb, c, f32) -> the
// normaliser of channel c, P::stores(wsb, c) -> whether this launch writes channel c's plane, P::ext(wsb) -> the sample's six crop
// words (running maxima of index + 1 on z y x, then of extent - index).
template <class P>
__global__ __launch_bounds__(kThreads) void resize_kernel(ResizeArgs a, int D, int H, int W, typename P::Ws* ws, __half* image,
                                                          uint8_t* label_map) {
  __shared__ uint32_t s_ext[6];
  const SampleDesc& sd = a.s[blockIdx.y];
  const int tid = threadIdx.x;
  const int V = D * H * W;
  auto* wsb = P::sample(ws);
  const bool ct32 = sd.ct.dtype == MICF_LOADER_F32, mr32 = sd.mr.dtype == MICF_LOADER_F32;
  const auto nct = P::norm(wsb, 0, ct32), nmr = P::norm(wsb, 1, mr32);
  __half* img = image + (size_t)blockIdx.y * 2 * V;
  if (tid < 6) s_ext[tid] = 0;
  __syncthreads();
  Extents ext;
  for (int v = blockIdx.x * kThreads + tid; v < V; v += gridDim.x * kThreads) {
    const int x = v % W, t = v / W, y = t % H, z = t / H;
    const float c0 = ct32 ? trilinear<true>(sd.ct, nct, z, y, x, D, H, W) : trilinear<false>(sd.ct, nct, z, y, x, D, H, W);
    const float c1 = mr32 ? trilinear<true>(sd.mr, nmr, z, y, x, D, H, W) : trilinear<false>(sd.mr, nmr, z, y, x, D, H, W);
    if (P::stores(wsb, 0)) img[v] = __float2half_rn(c0);
    if (P::stores(wsb, 1)) img[(size_t)V + v] = __float2half_rn(c1);
    if (c0 != 0.0f || c1 != 0.0f) ext.see(z, y, x, D, H, W);       // (true for NaN, as numpy's `!= 0`)
    if (label_map) {
      const Vol3& lv = sd.lab;
      const int sz = nearest_axis(z, lv.d, D), sy = nearest_axis(y, lv.h, H), sx = nearest_axis(x, lv.w, W);
      const int val = raw_label(lv, ((int64_t)sz * lv.h + sy) * lv.w + sx);
      label_map[(size_t)blockIdx.y * V + v] = (uint8_t)label_class(a, val);
    }
  }
  ext.flush(s_ext, P::ext(wsb));
}

// ---- the running maxima, counts and sums of a workspace start at 0.  A kernel, not hipMemsetAsync: captured into a graph, the memset
// node of the plain loader's few words left stale words behind at the second replay on ROCm 7.2
// (tests/test_gpu_loader.py::test_capture_and_replay_under_a_graph caught it).
__global__ void loader_zero_kernel(uint32_t* ws, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) ws[i] = 0;
}

// ---- crop_indexes (max(0, min - 1), max + 1) of every (sample, axis), (0, 0) where the image is all zero.  Sample b's six crop
// words lie at ext + b * stride: the loader format's at ws + 4, stride kWsWords; a record's at recs->ext, stride sizeof(SampleRec) / 4.
__global__ void loader_crop_kernel(const uint32_t* ext, int stride, int B, int D, int H, int W, int32_t* crop) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 3) return;
  const int ax = i % 3, extent = ax == 0 ? D : (ax == 1 ? H : W);
  const uint32_t* w = ext + (size_t)(i / 3) * stride;
  const uint32_t e = w[ax], f = w[3 + ax];
  int lo = 0, hi = 0;
  if (e != 0) {
    const int mn = extent - (int)f;
    lo = mn - 1 > 0 ? mn - 1 : 0;
    hi = (int)e;
  }
  crop[i * 2] = lo;
  crop[i * 2 + 1] = hi;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline int elem_size(int dtype) { return dtype == MICF_LOADER_I16 ? 2 : 4; }

// 0, or the error code of one source array
inline int check_volume(const void* p, const int32_t* shape, int dtype, bool is_label) {
  if (!p) return MICF_EINVAL;
  if (is_label ? (dtype != MICF_LOADER_I16 && dtype != MICF_LOADER_I32) : (dtype != MICF_LOADER_I16 && dtype != MICF_LOADER_F32))
    return MICF_EUNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(elem_size(dtype) - 1)) return MICF_EINVAL;
  if (shape[0] <= 0 || shape[1] <= 0 || shape[2] <= 0) return MICF_EINVAL;
  if (shape[0] > kMaxExtent || shape[1] > kMaxExtent || shape[2] > kMaxExtent) return MICF_EUNSUPPORTED;
  if ((int64_t)shape[0] * shape[1] * shape[2] >= (int64_t(1) << 31)) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

// Every check of a loader call but the workspace's: MICF_EINVAL before MICF_EUNSUPPORTED, nothing launched.
inline int check_call(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                      int num_label_values, const void* workspace, int64_t workspace_bytes, int64_t workspace_needed,
                      const void* image, const uint8_t* label_map, const int32_t* crop_indexes) {
  if (!samples || !workspace || !image || !crop_indexes || B <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  if (num_label_values < 0 || num_label_values > MICF_LOADER_MAX_LABEL_VALUES || (num_label_values > 0 && !label_values))
    return MICF_EINVAL;
  for (int i = 0; i < num_label_values; ++i) {
    if (label_values[i] == 0) return MICF_EINVAL;
    for (int j = 0; j < i; ++j)
      if (label_values[j] == label_values[i]) return MICF_EINVAL;
  }
  if (workspace_bytes < workspace_needed || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MICF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(image) & 1) || (reinterpret_cast<uintptr_t>(crop_indexes) & 3)) return MICF_EINVAL;
  int unsupported = 0;
  for (int b = 0; b < B; ++b) {
    const micf_loader_sample& s = samples[b];
    if ((s.label != nullptr) != (label_map != nullptr)) return MICF_EINVAL;
    const int rc[3] = {check_volume(s.ct, s.ct_shape, s.ct_dtype, false), check_volume(s.mr, s.mr_shape, s.mr_dtype, false),
                       s.label ? check_volume(s.label, s.label_shape, s.label_dtype, true) : MICF_OK};
    for (int r : rc) {
      if (r == MICF_EINVAL) return MICF_EINVAL;
      if (r == MICF_EUNSUPPORTED) unsupported = 1;
    }
  }
  if (unsupported || (int64_t)D * H * W > kMaxTarget) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

inline Vol3 vol3(const void* p, const int32_t* shape, int dtype) { return Vol3{p, shape[0], shape[1], shape[2], dtype}; }

// blocks of a pass over `bytes` of raw volume: four 16-byte loads per thread and trip, at most 1024
__host__ __device__ inline unsigned pass_blocks(int64_t bytes) {
  const int64_t mb = (bytes / 16 + 4 * kThreads - 1) / (4 * kThreads);
  return (unsigned)(mb < 1 ? 1 : (mb > 1024 ? 1024 : mb));
}

inline unsigned resize_blocks(int64_t V) {
  const int64_t vb = (V + kThreads - 1) / kThreads;
  return (unsigned)(vb < 2048 ? vb : 2048);
}

inline void fill_label_values(ResizeArgs& ra, const int32_t* label_values, int num_label_values) {
  ra.nvals = num_label_values;
  for (int i = 0; i < MICF_LOADER_MAX_LABEL_VALUES; ++i) ra.vals[i] = i < num_label_values ? label_values[i] : 0;
}

// The batch in chunks of at most kChunk samples: f(b0, nb, blocks) with ma / ra holding the descriptors of samples [b0, b0 + nb)
// (unused slots repeat the chunk's first sample and are never launched) and blocks = pass_blocks of the chunk's largest image volume.
template <class F>
inline void for_each_chunk(const micf_loader_sample* samples, int B, MinMaxArgs& ma, ResizeArgs& ra, F&& f) {
  for (int b0 = 0; b0 < B; b0 += kChunk) {
    const int nb = B - b0 < kChunk ? B - b0 : kChunk;
    int64_t most = 0;
    for (int i = 0; i < kChunk; ++i) {
      const micf_loader_sample& sm = samples[b0 + (i < nb ? i : 0)];
      ma.v[2 * i] = RawVol{sm.ct, (int64_t)sm.ct_shape[0] * sm.ct_shape[1] * sm.ct_shape[2], sm.ct_dtype, 0};
      ma.v[2 * i + 1] = RawVol{sm.mr, (int64_t)sm.mr_shape[0] * sm.mr_shape[1] * sm.mr_shape[2], sm.mr_dtype, 0};
      ra.s[i] = SampleDesc{vol3(sm.ct, sm.ct_shape, sm.ct_dtype), vol3(sm.mr, sm.mr_shape, sm.mr_dtype),
                           vol3(sm.label, sm.label_shape, sm.label_dtype)};
      for (int c = 0; c < 2; ++c) {
        const int64_t bytes = ma.v[2 * i + c].n * elem_size(ma.v[2 * i + c].dtype);
        most = bytes > most ? bytes : most;
      }
    }
    f(b0, nb, pass_blocks(most));
  }
}

inline void launch_zero(hipStream_t s, void* ws, int64_t words) {
  const int64_t zb = (words + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(loader_zero_kernel, dim3((unsigned)(zb < 1024 ? zb : 1024)), dim3(kThreads), 0, s, static_cast<uint32_t*>(ws),
                     words);
}

inline void launch_crop(hipStream_t s, const uint32_t* ext, int stride, int B, int D, int H, int W, int32_t* crop_indexes) {
  hipLaunchKernelGGL(loader_crop_kernel, dim3((unsigned)((B * 3 + 63) / 64)), dim3(64), 0, s, ext, stride, B, D, H, W, crop_indexes);
}

}  // namespace
