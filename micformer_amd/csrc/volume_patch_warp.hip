// volume_patch_warp.hip -- the patch sampler's crop THROUGH a map (include/micformer_patch_warp.h): every patch voxel's normalised
// patch coordinate n is moved by a displacement field interpolated on the patch grid, u, mapped by theta, s = theta . (n + u, 1),
// turned into a scan index by the origin add, i = o + ((s + 1) P - 1) / 2, and the raw CT / MR / label arrays are read there: the
// image interpolated once, the label rounded once, nothing intermediate written and nothing padded that the scan could have filled.
// The locate step is patch_locate.h's kernel, the one volume_patches.hip launches; the shared argument checks and the chunk driver
// that launches it are patch_sample_common.h's (check_sample_call, sample_chunks); here are this entry's own checks, the warp
// kernel and its launch.  The map's arithmetic is affine_coords.h's, the control grid's elastic_coords.h's, the origin add, the
// label's outside rule and the field's columns patch_warp_coords.h's (all host-callable); the 8 normalised taps are affine_taps.h's
// affine_trilinear with the statistics of the scan's index.
//
// Launch plan of micf_patch_sample_warped, per chunk of 8 samples:
//   1 locate     patch_locate_kernel, unchanged: writes origins and picked
//   2 warp-crop  patch_warp_kernel<kPer, kTaps>, grid (blocks, samples): reads origins from device memory; theta (or the identity)
//                once per block into LDS.  A thread owns kPer consecutive x outputs of one (z, y) row -- 8 (Pw % 8 == 0: one 16-byte
//                store per image plane, one 8-byte store of classes), 4 (Pw % 4 == 0: 8 and 4 bytes) or 1 (any Pw).  Without a field
//                (kTaps 0) the y- and z-dependent inner two fmafs of every map row are computed once per row and the x one per
//                voxel: map_row's own nesting, so the bits are map_row's.  With a field (kTaps 2 linear, 4 cubic) the z and y taps
//                are the row's, and the field collapsed over them (3 x kTaps columns) is recomputed only where the run enters
//                another control cell on x: on a coarse grid once per thread, on the dense grid at every voxel.
//                The taps are plain global loads of the raw arrays, 8 per image channel and voxel plus the label's one; the
//                source is not staged in LDS.
// Every index is clamped in float before it becomes an int (affine_coords.h), so no map or field forms an address outside the
// arrays or the field.  Nothing crosses threads but theta through LDS: bit-identical from run to run, independent of the other
// samples.  No scratch, no workspace, no atomics.
#include "affine_taps.h"
#include "patch_sample_common.h"
#include "patch_warp_coords.h"
#include "../../include/micformer_patch_warp.h"

namespace {

namespace pw = micf_patch_warp;

constexpr int kMaxGrid = 512;

template <int kTaps>
__device__ __forceinline__ micf_elastic::AxisTaps<kTaps> axis_taps(const micf_elastic::Cell& c, int g) {
  if constexpr (kTaps == 4) return micf_elastic::cubic_taps(c, g);
  else return micf_elastic::linear_taps(c, g);
}

__device__ __forceinline__ float warp_image(const Vol3& v, bool f32, const NormAny& nm, const AxisIndex& i, bool bd) {
  return f32 ? affine_trilinear<true>(v, nm, i, bd) : affine_trilinear<false>(v, nm, i, bd);
}

// grid (blocks, samples of the chunk); origins / theta / field / image / label_map point at the chunk's first sample.  theta: NULL
// (the identity), or per sample 12 floats, or 24 (per_modality: CT and label read map 0, MR map 1).  field (kTaps != 0): per
// sample [3][gd][gh][gw].
template <int kPer, int kTaps>
__global__ __launch_bounds__(kThreads) void patch_warp_kernel(ResizeArgs a, IndexArgs ia, const int32_t* origins, int Pd, int Ph, int Pw,
                                                              const float* theta, int per_modality, const float* field, int gd, int gh,
                                                              int gw, int border, int pad_class, __half* image, uint8_t* label_map) {
  __shared__ float s_theta[24];
  constexpr int kT = kTaps ? kTaps : 2;
  const SampleDesc& sd = a.s[blockIdx.y];
  const SampleRec* rec = reinterpret_cast<const SampleRec*>(ia.idx[blockIdx.y]);
  const bool ct32 = sd.ct.dtype == MICF_LOADER_F32, mr32 = sd.mr.dtype == MICF_LOADER_F32;
  const NormAny nct = NormWords::norm(rec, 0, ct32), nmr = NormWords::norm(rec, 1, mr32);
  const int d = sd.ct.d, h = sd.ct.h, w = sd.ct.w;
  const int oz = origins[blockIdx.y * 3], oy = origins[blockIdx.y * 3 + 1], ox = origins[blockIdx.y * 3 + 2];
  const int V = Pd * Ph * Pw, tid = threadIdx.x;
  __half* img = image + (size_t)blockIdx.y * 2 * V;
  uint8_t* lab = label_map ? label_map + (size_t)blockIdx.y * V : nullptr;
  const float* fld = kTaps ? field + (size_t)blockIdx.y * 3 * gd * gh * gw : nullptr;
  const int nth = per_modality ? 24 : 12;
  if (tid < 24) {
    const int e = tid < 12 ? tid : tid - 12;                       // element of a [3][4] map
    s_theta[tid] = theta ? theta[(size_t)blockIdx.y * nth + (tid < nth ? tid : tid - 12)] : (e % 5 == 0 ? 1.0f : 0.0f);
  }
  __syncthreads();
  const float* tc = s_theta;
  const float* tm = s_theta + 12;
  const bool bd = border != 0, two = per_modality != 0;
  const int groups = Pw / kPer, items = Pd * Ph * groups;
  for (int item = blockIdx.x * kThreads + tid; item < items; item += gridDim.x * kThreads) {
    const int xg = item % groups, row = item / groups, y = row % Ph, z = row / Ph;
    const float nz = micf_affine::norm_coord(z, Pd), ny = micf_affine::norm_coord(y, Ph);
    float inc[3] = {}, inm[3] = {};                                // map_row's inner two fmafs, per row (no field)
    micf_elastic::AxisTaps<kT> tz, ty;
    float col[3][kT];
    int cell = -1;
    if constexpr (kTaps == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        inc[r] = fmaf(tc[4 * r + 1], ny, fmaf(tc[4 * r + 2], nz, tc[4 * r + 3]));
        inm[r] = fmaf(tm[4 * r + 1], ny, fmaf(tm[4 * r + 2], nz, tm[4 * r + 3]));
      }
    } else {
      tz = axis_taps<kT>(micf_elastic::control_cell(z, Pd, gd), gd);
      ty = axis_taps<kT>(micf_elastic::control_cell(y, Ph, gh), gh);
    }
    uint32_t h0[kPer > 1 ? kPer / 2 : 1] = {}, h1[kPer > 1 ? kPer / 2 : 1] = {}, cl[kPer > 4 ? 2 : 1] = {};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = xg * kPer + j;
      const float nx = micf_affine::norm_coord(x, Pw);
      float cx, cy, cz, mx, my, mz;
      if constexpr (kTaps == 0) {
        cx = fmaf(tc[0], nx, inc[0]); cy = fmaf(tc[4], nx, inc[1]); cz = fmaf(tc[8], nx, inc[2]);
        mx = fmaf(tm[0], nx, inm[0]); my = fmaf(tm[4], nx, inm[1]); mz = fmaf(tm[8], nx, inm[2]);
      } else {
        const micf_elastic::Cell kx = micf_elastic::control_cell(x, Pw, gw);
        const micf_elastic::AxisTaps<kT> tx = axis_taps<kT>(kx, gw);
        if (kx.k != cell) {                                        // the run enters another control cell
          pw::field_columns<kT>(fld, tz, ty, tx, col);
          cell = kx.k;
        }
        const float px = nx + pw::displacement<kT>(col, 0, tx), py = ny + pw::displacement<kT>(col, 1, tx),
                    pz = nz + pw::displacement<kT>(col, 2, tx);
        cx = micf_affine::map_row(tc, px, py, pz); cy = micf_affine::map_row(tc + 4, px, py, pz);
        cz = micf_affine::map_row(tc + 8, px, py, pz);
        mx = micf_affine::map_row(tm, px, py, pz); my = micf_affine::map_row(tm + 4, px, py, pz);
        mz = micf_affine::map_row(tm + 8, px, py, pz);
      }
      const bool cok = micf_affine::finite(cx) && micf_affine::finite(cy) && micf_affine::finite(cz);
      const bool mok = micf_affine::finite(mx) && micf_affine::finite(my) && micf_affine::finite(mz);
      float c0 = 0.0f, c1 = 0.0f;
      int c = pad_class;                                           // outside the scan, or a non-finite coordinate
      AxisIndex ic{0.0f, 0.0f, 0.0f};
      if (cok) {
        ic = AxisIndex{pw::scan_index(oz, cz, Pd), pw::scan_index(oy, cy, Ph), pw::scan_index(ox, cx, Pw)};
        c0 = warp_image(sd.ct, ct32, nct, ic, bd);
        if (lab) {
          bool inz, iny, inx;
          const int sz = pw::label_tap(ic.z, d, inz), sy = pw::label_tap(ic.y, h, iny), sx = pw::label_tap(ic.x, w, inx);
          if (inz && iny && inx) c = label_class(a, raw_label(sd.lab, ((int64_t)sz * h + sy) * w + sx));
        }
      }
      if (mok) {
        const AxisIndex im = two ? AxisIndex{pw::scan_index(oz, mz, Pd), pw::scan_index(oy, my, Ph), pw::scan_index(ox, mx, Pw)} : ic;
        c1 = warp_image(sd.mr, mr32, nmr, im, bd);
      }
      h0[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c0)) << (16 * (j & 1));
      h1[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c1)) << (16 * (j & 1));
      cl[j / 4] |= (uint32_t)c << (8 * (j & 3));
    }
    const int o = row * Pw + xg * kPer;
    if constexpr (kPer == 8) {
      *reinterpret_cast<uint4*>(img + o) = make_uint4(h0[0], h0[1], h0[2], h0[3]);
      *reinterpret_cast<uint4*>(img + (size_t)V + o) = make_uint4(h1[0], h1[1], h1[2], h1[3]);
      if (lab) *reinterpret_cast<uint2*>(lab + o) = make_uint2(cl[0], cl[1]);
    } else if constexpr (kPer == 4) {
      *reinterpret_cast<uint2*>(img + o) = make_uint2(h0[0], h0[1]);
      *reinterpret_cast<uint2*>(img + (size_t)V + o) = make_uint2(h1[0], h1[1]);
      if (lab) *reinterpret_cast<uint32_t*>(lab + o) = cl[0];
    } else {
      img[o] = __ushort_as_half((unsigned short)h0[0]);
      img[(size_t)V + o] = __ushort_as_half((unsigned short)h1[0]);
      if (lab) lab[o] = (uint8_t)cl[0];
    }
  }
}

}  // namespace

extern "C" int micf_patch_sample_warped(const micf_loader_sample* samples, int B, void* const* indexes, const int64_t* index_bytes,
                                        const int32_t* label_values, int num_label_values, const float* draws, int Pd, int Ph, int Pw,
                                        int padding_mode, int pad_class, int clamp, void* image, uint8_t* label_map, int32_t* origins,
                                        int32_t* picked, const float* affine, int affine_per_modality, const float* displacement,
                                        int gd, int gh, int gw, int field_interpolation, micf_stream_t stream) {
  // this entry's own MICF_EINVAL checks, then the shared ones, then its own MICF_EUNSUPPORTED limit
  if ((reinterpret_cast<uintptr_t>(affine) & 3) || (reinterpret_cast<uintptr_t>(displacement) & 3)) return MICF_EINVAL;
  if (affine_per_modality != 0 && affine_per_modality != 1) return MICF_EINVAL;
  if (displacement) {
    if (field_interpolation != MICF_FIELD_LINEAR && field_interpolation != MICF_FIELD_CUBIC) return MICF_EINVAL;
    if (gd < 2 || gh < 2 || gw < 2) return MICF_EINVAL;
  }
  const SampleCall c{samples, B, indexes, index_bytes, label_values, num_label_values, draws, Pd, Ph, Pw, padding_mode, pad_class, clamp,
                     image, label_map, origins, picked};
  const int per = Pw % 8 == 0 ? 8 : (Pw % 4 == 0 ? 4 : 1);
  const int rc = check_sample_call(c, per);
  if (rc != MICF_OK) return rc;
  if (displacement && (gd > kMaxGrid || gh > kMaxGrid || gw > kMaxGrid)) return MICF_EUNSUPPORTED;

  hipStream_t s = (hipStream_t)stream;
  const int nth = affine_per_modality ? 24 : 12;
  const int taps = !displacement ? 0 : (field_interpolation == MICF_FIELD_CUBIC ? 4 : 2);
  const size_t per_field = displacement ? (size_t)3 * gd * gh * gw : 0;
  const int border = padding_mode == MICF_PATCH_PAD_BORDER ? 1 : 0;
  sample_chunks(c, per, s, [&](dim3 grid, const ResizeArgs& ra, const IndexArgs& ia, const int32_t* org, __half* img0, uint8_t* lab0,
                               int b0) {
    const float* th0 = affine ? affine + (size_t)b0 * nth : nullptr;
    const float* fl0 = displacement ? displacement + (size_t)b0 * per_field : nullptr;
    const auto launch = [&](auto kper, auto ktaps) {
      hipLaunchKernelGGL((patch_warp_kernel<decltype(kper)::value, decltype(ktaps)::value>), grid, dim3(kThreads), 0, s, ra, ia, org,
                         Pd, Ph, Pw, th0, affine_per_modality, fl0, gd, gh, gw, border, pad_class, img0, lab0);
    };
    const auto with_taps = [&](auto kper) {
      if (taps == 0) launch(kper, Int<0>{});
      else if (taps == 2) launch(kper, Int<2>{});
      else launch(kper, Int<4>{});
    };
    if (per == 8) with_taps(Int<8>{});
    else if (per == 4) with_taps(Int<4>{});
    else with_taps(Int<1>{});
  });
  MICF_RETURN_LAUNCH();
}
