// volume_restore.hip -- predictions back to the grid of the scan (include/micformer_restore.h): [B, K, D, H, W] float32 logits ->
// per sample a label volume of its own shape (d, h, w), trilinear upsample + argmax over K + class -> label value in ONE pass.
// The inverse of volume_loader.hip; the upsampled [K, d, h, w] tensor is never written.
//
// Launch plan of micf_volume_restore (8 samples per launch, their descriptors travel as kernel arguments, no host round trip):
//   0 softmax    MICF_RESTORE_PROBS only: softmax over K once per voxel of the LOW-resolution grid into the workspace; the fused
//                pass then reads the workspace instead of the logits (no exp at the output resolution)
//   1 fused      a workgroup owns an output tile of 64 (x) * 4 (y) * 8 (z) voxels, a thread a column of 8 voxels along z.
//                Per class the thread walks its column and keeps the in-plane (bilinear) value of the last two source planes in
//                registers: at the usual upsampling factors 8 outputs along z touch 4 - 5 source planes, so a class costs about
//                2 loads per output voxel instead of 8.  The loads go through L1 / L2 (a wave's 64 x-neighbours read one or two
//                cache lines per instruction); there is no LDS stage -- see DESIGN.md "Volume restore" for why.
//                Running best value + its label value per voxel, strict '>' over ascending k: the lowest class wins an exact tie.
// Nothing crosses threads: no atomics, no barriers, outputs bit-identical from run to run.
#include "common.h"
#include "../../include/micformer_restore.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 64, kTY = kThreads / kTX, kTZ = 8;   // output tile of a workgroup; a wave = 64 consecutive x
constexpr int kChunk = 8;                                // samples per launch
constexpr int kMaxExtent = 2048;
constexpr int64_t kMaxSource = (int64_t)512 * 512 * 512;

struct SampleDesc {
  void* out;
  int d, h, w;
  float sz, sy, sx;      // float(D) / d, ... (IEEE fp32 divide on the host)
  int ntx, nty, ntiles;  // tiles along x, along y, in all
};
struct FusedArgs { SampleDesc s[kChunk]; int lut[MICF_RESTORE_MAX_CLASSES]; };

// F.interpolate(mode="trilinear", align_corners=False) per axis, in fp32 exactly as written (no contraction into an fma: the tap
// indices are floor() of these numbers)
__device__ __forceinline__ void linear_axis(int o, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  i0 = (int)s;
  i0 = i0 < in - 1 ? i0 : in - 1;                        // (never taken for a finite scale: keeps every tap inside the volume)
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.0f - l1;
}

// the base of a source plane is the same in every lane (it depends on the tile's z range only): say so, which also keeps the
// compiler from hoisting (plane + tap offset) out of the class loop as 64 per-lane 64-bit addresses (190 VGPRs instead of 70)
typedef const __attribute__((address_space(1))) char* global_bytes;   // (an integer -> generic pointer cast would load through flat_*)
__device__ __forceinline__ global_bytes uniform_ptr(const float* p) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (global_bytes)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float tap(global_bytes plane, uint32_t byte_offset) {
  return *(const __attribute__((address_space(1))) float*)(plane + byte_offset);
}

// ---- 0. softmax over K at the low-resolution grid: grid (blocks, samples of the chunk) -------------------------------------------
__global__ __launch_bounds__(kThreads) void restore_softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs, int K,
                                                                   int64_t V) {
  const float* in = logits + (int64_t)blockIdx.y * K * V;
  float* out = probs + (int64_t)blockIdx.y * K * V;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < V; v += (int64_t)gridDim.x * kThreads) {
    float m = in[v];
    for (int k = 1; k < K; ++k) m = fmaxf(m, in[(int64_t)k * V + v]);
    float s = 0.0f;
    for (int k = 0; k < K; ++k) s += expf(in[(int64_t)k * V + v] - m);
    for (int k = 0; k < K; ++k) out[(int64_t)k * V + v] = expf(in[(int64_t)k * V + v] - m) / s;
  }
}

// ---- 1. upsample + argmax + label: grid (tiles, samples of the chunk); src points at the chunk's first sample -------------------
template <typename OutT>
__global__ __launch_bounds__(kThreads) void restore_fused_kernel(FusedArgs a, const float* __restrict__ src, int K, int D, int H, int W) {
  const SampleDesc& sd = a.s[blockIdx.y];
  if ((int)blockIdx.x >= sd.ntiles) return;
  const int tx = (int)blockIdx.x % sd.ntx, tr = (int)blockIdx.x / sd.ntx, ty = tr % sd.nty, tz = tr / sd.nty;
  const int x = tx * kTX + (threadIdx.x & (kTX - 1)), y = ty * kTY + (threadIdx.x / kTX), z0 = tz * kTZ;
  const bool live = x < sd.w && y < sd.h;
  // threads and column ends beyond the volume compute the clamped voxel (the same taps as a neighbour) and store nothing
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  linear_axis(y < sd.h ? y : sd.h - 1, H, sd.sy, y0, y1, ly0, ly1);
  linear_axis(x < sd.w ? x : sd.w - 1, W, sd.sx, x0, x1, lx0, lx1);
  // byte offsets of the four in-plane taps (H * W <= 2^27 elements, so they fit unsigned 32-bit), added to the scalar base of
  // a plane at the load: hipcc emits one v_lshl_add_u64 (scalar base + per-lane offset) and one global_load_dword per tap, and
  // what stays in registers across the class loop is these four offsets, not an address per (plane, tap)
  const uint32_t o00 = 4u * (uint32_t)(y0 * W + x0), o01 = 4u * (uint32_t)(y0 * W + x1);
  const uint32_t o10 = 4u * (uint32_t)(y1 * W + x0), o11 = 4u * (uint32_t)(y1 * W + x1);
  int zi0[kTZ], zi1[kTZ];
  float zl0[kTZ], zl1[kTZ], best[kTZ];
  int lab[kTZ];
#pragma unroll
  for (int j = 0; j < kTZ; ++j) {
    linear_axis(z0 + j < sd.d ? z0 + j : sd.d - 1, D, sd.sz, zi0[j], zi1[j], zl0[j], zl1[j]);
    best[j] = -INFINITY;
    lab[j] = a.lut[0];
  }
  const int64_t HW = (int64_t)H * W;
  const float* cls = src + (int64_t)blockIdx.y * K * D * HW;
  for (int k = 0; k < K; ++k, cls += (int64_t)D * HW) {
    const int lv = a.lut[k];
    int pa = -1, pb = -1;                                // the two source planes whose in-plane value is held, pb the newer
    float va = 0.0f, vb = 0.0f;
    auto plane = [&](int p) -> float {
      if (p == pb) return vb;
      if (p == pa) return va;
      const global_bytes q = uniform_ptr(cls + (int64_t)p * HW);
      const float v = (tap(q, o00) * lx0 + tap(q, o01) * lx1) * ly0 + (tap(q, o10) * lx0 + tap(q, o11) * lx1) * ly1;
      pa = pb; va = vb;
      pb = p; vb = v;
      return v;
    };
#pragma unroll
    for (int j = 0; j < kTZ; ++j) {
      const float t0 = plane(zi0[j]);
      const float t1 = plane(zi1[j]);
      const float v = t0 * zl0[j] + t1 * zl1[j];
      if (v > best[j]) { best[j] = v; lab[j] = lv; }
    }
  }
  if (!live) return;
  OutT* out = static_cast<OutT*>(sd.out) + ((int64_t)z0 * sd.h + y) * sd.w + x;
  const int64_t plane_stride = (int64_t)sd.h * sd.w;
#pragma unroll
  for (int j = 0; j < kTZ; ++j)
    if (z0 + j < sd.d) out[j * plane_stride] = (OutT)lab[j];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int elem_size(int dtype) { return dtype == MICF_RESTORE_U8 ? 1 : (dtype == MICF_RESTORE_I16 ? 2 : 4); }

// 0, or the error code of the source geometry
int check_source(int B, int K, int D, int H, int W, int interpoland) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return MICF_EINVAL;
  if (interpoland != MICF_RESTORE_LOGITS && interpoland != MICF_RESTORE_PROBS) return MICF_EINVAL;
  if (K < 1 || K > MICF_RESTORE_MAX_CLASSES) return MICF_EUNSUPPORTED;
  if ((int64_t)D * H * W > kMaxSource) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

}  // namespace

extern "C" int64_t micf_volume_restore_workspace(int B, int K, int D, int H, int W, int interpoland) {
  const int rc = check_source(B, K, D, H, W, interpoland);
  if (rc != MICF_OK) return rc;
  return interpoland == MICF_RESTORE_PROBS ? (int64_t)B * K * D * H * W * (int64_t)sizeof(float) : 0;
}

extern "C" int micf_volume_restore(const float* logits, int B, int K, int D, int H, int W, const micf_restore_sample* samples,
                                   int out_dtype, int interpoland, const int32_t* label_values, int num_label_values,
                                   void* workspace, int64_t workspace_bytes, micf_stream_t stream) {
  if (!logits || !samples || (reinterpret_cast<uintptr_t>(logits) & 3)) return MICF_EINVAL;
  if (out_dtype != MICF_RESTORE_U8 && out_dtype != MICF_RESTORE_I16 && out_dtype != MICF_RESTORE_I32) return MICF_EINVAL;
  const int rc = check_source(B, K, D, H, W, interpoland);
  if (rc == MICF_EINVAL) return rc;
  int unsupported = rc == MICF_EUNSUPPORTED;
  if (!unsupported) {                                    // (the label table and the workspace are sized by a supported K)
    if (out_dtype == MICF_RESTORE_U8) {
      if (label_values || num_label_values != 0) return MICF_EINVAL;
    } else {
      if (!label_values || num_label_values != K - 1) return MICF_EINVAL;
      if (out_dtype == MICF_RESTORE_I16)
        for (int i = 0; i < num_label_values; ++i)
          if (label_values[i] < -32768 || label_values[i] > 32767) return MICF_EINVAL;
    }
    const int64_t need = micf_volume_restore_workspace(B, K, D, H, W, interpoland);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3))) return MICF_EINVAL;
  }
  for (int b = 0; b < B; ++b) {
    const micf_restore_sample& s = samples[b];
    if (!s.out || (reinterpret_cast<uintptr_t>(s.out) & (uintptr_t)(elem_size(out_dtype) - 1))) return MICF_EINVAL;
    if (s.out_shape[0] <= 0 || s.out_shape[1] <= 0 || s.out_shape[2] <= 0) return MICF_EINVAL;
    if (s.out_shape[0] > kMaxExtent || s.out_shape[1] > kMaxExtent || s.out_shape[2] > kMaxExtent) unsupported = 1;
    else if ((int64_t)s.out_shape[0] * s.out_shape[1] * s.out_shape[2] >= (int64_t(1) << 31)) unsupported = 1;
  }
  if (unsupported) return MICF_EUNSUPPORTED;

  hipStream_t s = (hipStream_t)stream;
  const int64_t V = (int64_t)D * H * W;
  const float* src = interpoland == MICF_RESTORE_PROBS ? static_cast<const float*>(workspace) : logits;
  FusedArgs fa;
  for (int k = 0; k < MICF_RESTORE_MAX_CLASSES; ++k)
    fa.lut[k] = out_dtype == MICF_RESTORE_U8 ? k : (k >= 1 && k < K ? label_values[k - 1] : 0);
  const int64_t sb = (V + kThreads - 1) / kThreads;
  const unsigned sblocks = (unsigned)(sb < 2048 ? sb : 2048);
  for (int b0 = 0; b0 < B; b0 += kChunk) {
    const int nb = B - b0 < kChunk ? B - b0 : kChunk;
    int most = 0;
    for (int i = 0; i < kChunk; ++i) {
      const micf_restore_sample& sm = samples[b0 + (i < nb ? i : 0)];            // (unused slots repeat the first: never launched)
      SampleDesc& sd = fa.s[i];
      sd.out = sm.out;
      sd.d = sm.out_shape[0]; sd.h = sm.out_shape[1]; sd.w = sm.out_shape[2];
      sd.sz = (float)D / (float)sd.d; sd.sy = (float)H / (float)sd.h; sd.sx = (float)W / (float)sd.w;
      sd.ntx = (sd.w + kTX - 1) / kTX;
      sd.nty = (sd.h + kTY - 1) / kTY;
      sd.ntiles = sd.ntx * sd.nty * ((sd.d + kTZ - 1) / kTZ);                   // <= 32 * 512 * 256
      most = sd.ntiles > most ? sd.ntiles : most;
    }
    const int64_t off = (int64_t)b0 * K * V;
    if (interpoland == MICF_RESTORE_PROBS)
      hipLaunchKernelGGL(restore_softmax_kernel, dim3(sblocks, (unsigned)nb), dim3(kThreads), 0, s, logits + off,
                         static_cast<float*>(workspace) + off, K, V);
    const dim3 grid((unsigned)most, (unsigned)nb), block(kThreads);
    if (out_dtype == MICF_RESTORE_U8)
      hipLaunchKernelGGL(restore_fused_kernel<uint8_t>, grid, block, 0, s, fa, src + off, K, D, H, W);
    else if (out_dtype == MICF_RESTORE_I16)
      hipLaunchKernelGGL(restore_fused_kernel<int16_t>, grid, block, 0, s, fa, src + off, K, D, H, W);
    else
      hipLaunchKernelGGL(restore_fused_kernel<int32_t>, grid, block, 0, s, fa, src + off, K, D, H, W);
  }
  MICF_RETURN_LAUNCH();
}
