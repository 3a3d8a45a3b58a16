// volume_affine.hip -- the volume loader with an affine map in its resample pass (include/micformer_affine.h): every output voxel
// reads the raw CT / MR / label arrays at theta . (its normalised coordinate), F.affine_grid + F.grid_sample(align_corners=False),
// with the normalisation of volume_normalise.hip applied to each tap.  The coordinate, clamp and index arithmetic is
// affine_coords.h's (host-callable); the statistics passes, the records and the per-channel normaliser are
// volume_normalise_stats.h's, shared with volume_normalise.hip.
//
// Launch plan of micf_volume_loader_affine (batched over the samples, 8 per launch, no host round trip):
//   0 zero, 1-4 the statistics passes the two modes need and their finish: volume_normalise.hip's plan, unchanged (the statistics
//     are the whole raw volume's, whatever the map)
//   5 resample   resize_kernel's shape: grid (blocks, samples of the chunk), one thread per output voxel, x fastest so the fp16 and
//                uint8 stores coalesce; the sample's 12 or 24 floats of theta read once per block into LDS; per voxel one
//                normalised coordinate, one source coordinate per map, and per array the three indices, the 8 taps normalised in
//                registers (NormAny: every mode in one launch), the nearest label tap + value lookup; the crop extents reduced as
//                in resize_kernel
//   6 crop       extents -> crop_indexes
// Everything that crosses threads is an integer count, sum or maximum, or is merged in a fixed order: bit-identical from run to run.
#include "volume_normalise_stats.h"
#include "affine_coords.h"
#include "../../include/micformer_affine.h"

namespace {

using micf_affine::LinearTaps;

struct AxisIndex { float z, y, x; };

// index of the normalised source coordinate (sx, sy, sz) in an array of shape (d, h, w)
__device__ __forceinline__ AxisIndex source_indices(const Vol3& v, float sx, float sy, float sz) {
  return AxisIndex{micf_affine::source_index(sz, v.d), micf_affine::source_index(sy, v.h), micf_affine::source_index(sx, v.w)};
}

// separable trilinear sum over the 8 taps, w fastest (trilinear()'s order); a tap outside the array counts 0
template <bool F32>
__device__ __forceinline__ float affine_trilinear(const Vol3& v, const NormAny& nm, const AxisIndex& i, bool border) {
  const LinearTaps tz = micf_affine::linear_taps(i.z, v.d, border);
  const LinearTaps ty = micf_affine::linear_taps(i.y, v.h, border);
  const LinearTaps tx = micf_affine::linear_taps(i.x, v.w, border);
  const int64_t r00 = ((int64_t)tz.i0 * v.h + ty.i0) * v.w, r01 = ((int64_t)tz.i0 * v.h + ty.i1) * v.w;
  const int64_t r10 = ((int64_t)tz.i1 * v.h + ty.i0) * v.w, r11 = ((int64_t)tz.i1 * v.h + ty.i1) * v.w;
  const bool i00 = tz.in0 && ty.in0, i01 = tz.in0 && ty.in1, i10 = tz.in1 && ty.in0, i11 = tz.in1 && ty.in1;
  const float a00 = i00 && tx.in0 ? tap<F32>(v.p, r00 + tx.i0, nm) : 0.0f, b00 = i00 && tx.in1 ? tap<F32>(v.p, r00 + tx.i1, nm) : 0.0f;
  const float a01 = i01 && tx.in0 ? tap<F32>(v.p, r01 + tx.i0, nm) : 0.0f, b01 = i01 && tx.in1 ? tap<F32>(v.p, r01 + tx.i1, nm) : 0.0f;
  const float a10 = i10 && tx.in0 ? tap<F32>(v.p, r10 + tx.i0, nm) : 0.0f, b10 = i10 && tx.in1 ? tap<F32>(v.p, r10 + tx.i1, nm) : 0.0f;
  const float a11 = i11 && tx.in0 ? tap<F32>(v.p, r11 + tx.i0, nm) : 0.0f, b11 = i11 && tx.in1 ? tap<F32>(v.p, r11 + tx.i1, nm) : 0.0f;
  const float t00 = a00 * tx.w0 + b00 * tx.w1, t01 = a01 * tx.w0 + b01 * tx.w1;
  const float t10 = a10 * tx.w0 + b10 * tx.w1, t11 = a11 * tx.w0 + b11 * tx.w1;
  const float u0 = t00 * ty.w0 + t01 * ty.w1, u1 = t10 * ty.w0 + t11 * ty.w1;
  return u0 * tz.w0 + u1 * tz.w1;
}

// ---- 5. resample ------------------------------------------------------------------------------------------------------------------
// grid (blocks, samples of the chunk); recs / theta / image / label_map point at the chunk's first sample.  theta: per sample
// 12 floats, or 24 (per_modality: CT and label read map 0, MR map 1).
__global__ __launch_bounds__(kThreads) void affine_resample_kernel(ResizeArgs a, int D, int H, int W, SampleRec* recs,
                                                                   const float* theta, int per_modality, int border,
                                                                   __half* image, uint8_t* label_map) {
  __shared__ uint32_t s_ext[6];
  __shared__ float s_theta[24];
  const SampleDesc& sd = a.s[blockIdx.y];
  const int tid = threadIdx.x;
  const int V = D * H * W;
  SampleRec* rec = NormWords::sample(recs);
  const bool ct32 = sd.ct.dtype == MICF_LOADER_F32, mr32 = sd.mr.dtype == MICF_LOADER_F32;
  const NormAny nct = NormWords::norm(rec, 0, ct32), nmr = NormWords::norm(rec, 1, mr32);
  __half* img = image + (size_t)blockIdx.y * 2 * V;
  const int nth = per_modality ? 24 : 12;
  if (tid < 6) s_ext[tid] = 0;
  if (tid < 24) s_theta[tid] = theta[(size_t)blockIdx.y * nth + (tid < nth ? tid : tid - 12)];   // (one map: both halves hold it)
  __syncthreads();
  const float* tc = s_theta;
  const float* tm = s_theta + 12;
  const bool bd = border != 0;
  uint32_t ez = 0, ey = 0, ex = 0, fz = 0, fy = 0, fx = 0;
  for (int v = blockIdx.x * kThreads + tid; v < V; v += gridDim.x * kThreads) {
    const int x = v % W, t = v / W, y = t % H, z = t / H;
    const float nx = micf_affine::norm_coord(x, W), ny = micf_affine::norm_coord(y, H), nz = micf_affine::norm_coord(z, D);
    const float cx = micf_affine::map_row(tc, nx, ny, nz), cy = micf_affine::map_row(tc + 4, nx, ny, nz),
                cz = micf_affine::map_row(tc + 8, nx, ny, nz);
    const float mx = micf_affine::map_row(tm, nx, ny, nz), my = micf_affine::map_row(tm + 4, nx, ny, nz),
                mz = micf_affine::map_row(tm + 8, nx, ny, nz);
    const bool cok = micf_affine::finite(cx) && micf_affine::finite(cy) && micf_affine::finite(cz);
    const bool mok = micf_affine::finite(mx) && micf_affine::finite(my) && micf_affine::finite(mz);
    float c0 = 0.0f, c1 = 0.0f;
    if (cok) {
      const AxisIndex i = source_indices(sd.ct, cx, cy, cz);
      c0 = ct32 ? affine_trilinear<true>(sd.ct, nct, i, bd) : affine_trilinear<false>(sd.ct, nct, i, bd);
    }
    if (mok) {
      const AxisIndex i = source_indices(sd.mr, mx, my, mz);
      c1 = mr32 ? affine_trilinear<true>(sd.mr, nmr, i, bd) : affine_trilinear<false>(sd.mr, nmr, i, bd);
    }
    img[v] = __float2half_rn(c0);
    img[(size_t)V + v] = __float2half_rn(c1);
    if (c0 != 0.0f || c1 != 0.0f) {                              // (true for NaN, as numpy's `!= 0`)
      ez = max(ez, (uint32_t)(z + 1)); fz = max(fz, (uint32_t)(D - z));
      ey = max(ey, (uint32_t)(y + 1)); fy = max(fy, (uint32_t)(H - y));
      ex = max(ex, (uint32_t)(x + 1)); fx = max(fx, (uint32_t)(W - x));
    }
    if (label_map) {
      const Vol3& lv = sd.lab;
      int val = 0;                                               // outside the array, or a non-finite coordinate: raw label 0
      if (cok) {
        const AxisIndex i = source_indices(lv, cx, cy, cz);
        bool inz, iny, inx;
        const int sz = micf_affine::nearest_tap(i.z, lv.d, bd, inz), sy = micf_affine::nearest_tap(i.y, lv.h, bd, iny),
                  sx = micf_affine::nearest_tap(i.x, lv.w, bd, inx);
        if (inz && iny && inx) {
          const int64_t off = ((int64_t)sz * lv.h + sy) * lv.w + sx;
          val = lv.dtype == MICF_LOADER_I32 ? static_cast<const int32_t*>(lv.p)[off] : (int)static_cast<const int16_t*>(lv.p)[off];
        }
      }
      int cls = val == 0 ? 0 : 255;
      for (int k = 0; k < a.nvals; ++k) cls = val == a.vals[k] ? k + 1 : cls;
      label_map[(size_t)blockIdx.y * V + v] = (uint8_t)cls;
    }
  }
  ez = wave_umax(ez); ey = wave_umax(ey); ex = wave_umax(ex);
  fz = wave_umax(fz); fy = wave_umax(fy); fx = wave_umax(fx);
  if ((tid & 63) == 0) {
    atomicMax(&s_ext[0], ez); atomicMax(&s_ext[1], ey); atomicMax(&s_ext[2], ex);
    atomicMax(&s_ext[3], fz); atomicMax(&s_ext[4], fy); atomicMax(&s_ext[5], fx);
  }
  __syncthreads();
  if (tid < 6 && s_ext[tid] != 0) atomicMax(rec->ext + tid, s_ext[tid]);
}

// ---- 6. crop_indexes --------------------------------------------------------------------------------------------------------------
__global__ void affine_crop_kernel(const SampleRec* recs, int B, int D, int H, int W, int32_t* crop) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 3) return;
  crop_body(recs[i / 3].ext, i % 3, D, H, W, crop + i * 2);
}

}  // namespace

extern "C" int64_t micf_volume_loader_affine_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_volume_loader_affine(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                                         int num_label_values, int ct_mode, int mr_mode, double p_low, double p_high,
                                         void* workspace, int64_t workspace_bytes, void* image, uint8_t* label_map,
                                         int32_t* crop_indexes, double* stats, const float* affine, int affine_per_modality,
                                         int padding_mode, micf_stream_t stream) {
  if (!affine || (reinterpret_cast<uintptr_t>(affine) & 3)) return MICF_EINVAL;
  if (affine_per_modality != 0 && affine_per_modality != 1) return MICF_EINVAL;
  if (padding_mode != MICF_PAD_ZEROS && padding_mode != MICF_PAD_BORDER) return MICF_EINVAL;
  if (!valid_mode(ct_mode) || !valid_mode(mr_mode)) return MICF_EINVAL;
  if (!(0.0 <= p_low && p_low < p_high && p_high <= 100.0)) return MICF_EINVAL;      // (false for NaN)
  if (reinterpret_cast<uintptr_t>(stats) & 7) return MICF_EINVAL;
  const int rc = check_call(samples, B, D, H, W, label_values, num_label_values, workspace, workspace_bytes,
                            B > 0 ? layout(B).total : 0, image, label_map, crop_indexes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  const Layout L = layout(B);
  char* ws = static_cast<char*>(workspace);
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  SampleRec* recs = reinterpret_cast<SampleRec*>(ws + L.recs);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
  Mom* partials = reinterpret_cast<Mom*>(ws + L.partials);
  const int64_t V = (int64_t)D * H * W;
  const Modes md{{ct_mode, mr_mode}};
  const int64_t zb = (L.zero_words + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(norm_zero_kernel, dim3((unsigned)(zb < 1024 ? zb : 1024)), dim3(kThreads), 0, s,
                     reinterpret_cast<uint32_t*>(ws), L.zero_words);
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  const unsigned rblocks = resize_blocks(V);
  const int nth = affine_per_modality ? 24 : 12;
  for (int b0 = 0; b0 < B; b0 += kChunk) {
    const int nb = B - b0 < kChunk ? B - b0 : kChunk;
    MinMaxArgs ma;
    const unsigned blocks = pass_blocks(fill_chunk(samples, b0, nb, ma, ra));
    SampleRec* rc0 = recs + b0;
    launch_statistics(s, ma, md, nb, blocks, p_low, p_high, words + (size_t)b0 * kWsWords, rc0,
                      hist + (size_t)b0 * 2 * kRanks * kBins, partials + (size_t)b0 * 2 * kMaxPartials,
                      stats ? stats + (size_t)b0 * 4 : nullptr);
    hipLaunchKernelGGL(affine_resample_kernel, dim3(rblocks, (unsigned)nb), dim3(kThreads), 0, s, ra, D, H, W, rc0,
                       affine + (size_t)b0 * nth, affine_per_modality, padding_mode,
                       static_cast<__half*>(image) + (size_t)b0 * 2 * V, label_map ? label_map + (size_t)b0 * V : nullptr);
  }
  hipLaunchKernelGGL(affine_crop_kernel, dim3((unsigned)((B * 3 + 63) / 64)), dim3(64), 0, s, recs, B, D, H, W, crop_indexes);
  MICF_RETURN_LAUNCH();
}
