// volume_patches.hip -- the on-device patch sampler (include/micformer_patches.h): the index of a scan (normaliser statistics,
// class counts, per-segment class counts) and native-resolution crops of it, a share of them centred on a foreground voxel drawn
// uniformly from ALL voxels of a class.  The statistics passes, the per-element normaliser and the label lookup are
// volume_normalise_stats.h's and volume_loader_common.h's; the index arithmetic is patches_coords.h's (host-testable).
//
// Launch plan of micf_patch_index (batched over the scans, 8 per launch, no host round trip):
//   0 zero       loader_zero_kernel over the statistics workspace
//   1 statistics launch_statistics: exactly micf_volume_loader_norm's passes and finish for the two modes
//   2 init       patch_index_init_kernel, one workgroup per scan: the scan's statistics record -> the head of its index, the
//                class counts zeroed
//   3 count      patch_count_kernel (labelled scans), grid (blocks, scans): a workgroup takes whole segments; per segment one LDS
//                histogram of 256 bins (integer ds_add), the counts of classes 1..K stored as uint16 [K][padded segments] (each segment
//                is written by exactly one workgroup), the workgroup's totals added to the class counts with one integer atomicAdd
//                per class at the end
// Launch plan of micf_patch_sample, per chunk of 8 samples:
//   1 locate     patch_locate_kernel, one workgroup per sample, no workgroup waits on another: every thread reads the draws and
//                the class counts and picks class and rank (the same loads, so the decision is uniform); thread t sums the strip
//                of the class's segment counts that falls to it (8-byte loads of four counts, ceil(vectors / 256) of them: as
//                many trips as that), one integer prefix over the 256 sums finds the strip; the workgroup walks that strip 256
//                segments per trip with a prefix per trip and finds the segment and the rank inside it; the workgroup
//                then reads that segment's 2048 labels in 8 rounds, a ballot + popcount per wave and round gives 32 ordered
//                counts, and the lane whose match has the wanted number of matches below it writes origins and picked.  An index
//                that does not fit its scan (the rank is never found) falls back to the random crop: no address depends on it.
//   2 crop       patch_crop_kernel<kPer>, grid (blocks, samples), the only bandwidth path: reads origins from device memory; a thread
//                makes 8 consecutive output voxels of a row (Pw % 8 == 0: one 16-byte store per channel, one 8-byte store of
//                classes) or one voxel (any Pw).  Source rows start at an arbitrary element offset: where the 8 positions
//                lie inside one row of int16 arrays, each array is read with two aligned 16-byte loads and shifted by the byte
//                offset (select + v_alignbit; 64 against 87 us at 8 x 128^3 under the kernel trace); elsewhere -- float32
//                arrays, groups that cross the scan's border or touch the array's last bytes -- per element, every index
//                clamped into the scan before it is used.
// Everything that crosses threads is an integer: bit-identical from run to run, independent of the other samples.  No scratch.
// The locate kernel, the view of an index buffer and the host-side checks of the scans live in patch_locate.h; the argument checks
// of micf_patch_sample and the chunk driver with the locate launch, which micf_patch_sample_warped (volume_patch_warp.hip) shares,
// in patch_sample_common.h (check_sample_call, sample_chunks).  norm_i16, the normaliser of an element already in a register, is
// volume_normalise_stats.h's, where tap<false> is the load followed by it.
#include "patch_sample_common.h"

namespace {

// ---- index: 2 init --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void patch_index_init_kernel(IndexArgs ia, const SampleRec* recs) {
  char* idx = ia.idx[blockIdx.x];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(recs + blockIdx.x);
  const int tid = threadIdx.x;
  if (tid < (int)(sizeof(SampleRec) / 4)) reinterpret_cast<uint32_t*>(idx)[tid] = src[tid];
  index_counts(idx)[tid] = 0;                                    // (kCountsBytes = 4 * kThreads)
}

// ---- index: 3 count -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void patch_count_kernel(ResizeArgs a, IndexArgs ia) {
  __shared__ uint32_t s_h[kThreads];
  const Vol3& lv = a.s[blockIdx.y].lab;
  const int64_t V = (int64_t)lv.d * lv.h * lv.w, nseg = pc::num_segments(V), row = pc::padded_segments(V);
  char* idx = ia.idx[blockIdx.y];
  uint16_t* segs = index_segments(idx);
  const int K = a.nvals, tid = threadIdx.x;
  uint32_t total = 0;                                            // of bin `tid` over this workgroup's segments
  for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
    s_h[tid] = 0;
    __syncthreads();
    const int64_t base = s * pc::kSegment;
    // a thread takes kRounds consecutive voxels and adds each run of equal classes once: labels come in runs, so most threads
    // issue one ds_add and not kRounds
    const int64_t v0 = base + (int64_t)tid * kRounds;
    int cur = -1;
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < kRounds; ++j) {
      if (v0 + j < V) {
        const int c = label_class(a, raw_label(lv, v0 + j));
        const int bin = c == 255 ? K + 1 : c;
        if (bin != cur && run) atomicAdd(&s_h[cur], run);
        run = bin == cur ? run + 1 : 1;
        cur = bin;
      }
    }
    if (run) atomicAdd(&s_h[cur], run);
    __syncthreads();
    const uint32_t n = s_h[tid];
    total += n;
    if (tid >= 1 && tid <= K) {
      segs[(int64_t)(tid - 1) * row + s] = (uint16_t)n;
      if (s == nseg - 1)                                         // (the row's padding, by the workgroup of the last segment)
        for (int64_t q = nseg; q < row; ++q) segs[(int64_t)(tid - 1) * row + q] = 0;
    }
    __syncthreads();                                             // (the bins are read before the next trip clears them)
  }
  if (tid <= K + 1 && total) atomicAdd(index_counts(idx) + tid, total);
}

// ---- sample: 2 crop -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float norm_tap(const Vol3& v, bool f32, int64_t off, const NormAny& nm) {
  return f32 ? tap<true>(v.p, off, nm) : tap<false>(v.p, off, nm);
}

// Elements [off, off + 8) of an int16 volume of n elements through two aligned 16-byte loads and a shift by the byte offset of
// the first element; false (nothing loaded) where the two vectors do not lie inside the volume.
__device__ __forceinline__ bool shifted8_i16(const void* p, int64_t n, int64_t off, uint32_t (&out)[4]) {
  const uintptr_t first = reinterpret_cast<uintptr_t>(p), at = first + (uintptr_t)off * 2, lo = at & ~(uintptr_t)15;
  if (lo < first || lo + 32 > first + (uintptr_t)n * 2) return false;
  const uint4 q0 = *reinterpret_cast<const uint4*>(lo), q1 = *reinterpret_cast<const uint4*>(lo + 16);
  const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  const int ws = (int)(at & 15) >> 2, bits = (int)(at & 3) * 8;
  uint32_t t[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) t[j] = ws == 0 ? w[j] : (ws == 1 ? w[j + 1] : (ws == 2 ? w[j + 2] : w[j + 3]));
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = __funnelshift_r(t[j], t[j + 1], bits);
  return true;
}
__device__ __forceinline__ int unpack_i16(const uint32_t (&v)[4], int j) {
  return (int)(int16_t)((v[j / 2] >> (16 * (j & 1))) & 0xFFFFu);
}

// grid (blocks, samples of the chunk); origins / image / label_map point at the chunk's first sample; kPer 8 or 1 outputs per thread
template <int kPer>
__global__ __launch_bounds__(kThreads) void patch_crop_kernel(ResizeArgs a, IndexArgs ia, const int32_t* origins, int Pd, int Ph, int Pw,
                                                              int border, int pad_class, __half* image, uint8_t* label_map) {
  const SampleDesc& sd = a.s[blockIdx.y];
  const SampleRec* rec = reinterpret_cast<const SampleRec*>(ia.idx[blockIdx.y]);
  const bool ct32 = sd.ct.dtype == MICF_LOADER_F32, mr32 = sd.mr.dtype == MICF_LOADER_F32;
  const NormAny nct = NormWords::norm(rec, 0, ct32), nmr = NormWords::norm(rec, 1, mr32);
  const int d = sd.ct.d, h = sd.ct.h, w = sd.ct.w;
  const int oz = origins[blockIdx.y * 3], oy = origins[blockIdx.y * 3 + 1], ox = origins[blockIdx.y * 3 + 2];
  const int V = Pd * Ph * Pw;
  __half* img = image + (size_t)blockIdx.y * 2 * V;
  uint8_t* lab = label_map ? label_map + (size_t)blockIdx.y * V : nullptr;
  const int groups = Pw / kPer, items = Pd * Ph * groups;
  for (int item = blockIdx.x * kThreads + threadIdx.x; item < items; item += gridDim.x * kThreads) {
    const int xg = item % groups, row = item / groups, y = row % Ph, z = row / Ph;
    const int sz = oz + z, sy = oy + y;
    const bool in_zy = pc::inside(sz, d) && pc::inside(sy, h);
    const int64_t rowoff = ((int64_t)pc::clamp_index(sz, d) * h + pc::clamp_index(sy, h)) * w;
    uint32_t h0[kPer > 1 ? kPer / 2 : 1] = {}, h1[kPer > 1 ? kPer / 2 : 1] = {}, cl[kPer > 4 ? 2 : 1] = {};
    const auto put = [&](int j, float c0, float c1, int c) {
      h0[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c0)) << (16 * (j & 1));
      h1[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c1)) << (16 * (j & 1));
      cl[j / 4] |= (uint32_t)c << (8 * (j & 3));
    };
    const int sx0 = ox + xg * kPer;
    uint32_t r0[4], r1[4], rl[4];
    // the 8 positions lie in one source row: two vector loads per array
    if (kPer == 8 && sx0 >= 0 && sx0 + kPer <= w && (in_zy || border) && !ct32 && !mr32 && (!lab || sd.lab.dtype == MICF_LOADER_I16) &&
        shifted8_i16(sd.ct.p, (int64_t)d * h * w, rowoff + sx0, r0) && shifted8_i16(sd.mr.p, (int64_t)d * h * w, rowoff + sx0, r1) &&
        (!lab || !in_zy || shifted8_i16(sd.lab.p, (int64_t)d * h * w, rowoff + sx0, rl))) {
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        put(j, norm_i16(unpack_i16(r0, j), nct), norm_i16(unpack_i16(r1, j), nmr),
            (lab && in_zy) ? label_class(a, unpack_i16(rl, j)) : pad_class);
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int sx = sx0 + j;
        const bool in = in_zy && pc::inside(sx, w);
        const int64_t off = rowoff + pc::clamp_index(sx, w);
        float c0 = 0.0f, c1 = 0.0f;
        if (in || border) {
          c0 = norm_tap(sd.ct, ct32, off, nct);
          c1 = norm_tap(sd.mr, mr32, off, nmr);
        }
        put(j, c0, c1, lab && in ? label_class(a, raw_label(sd.lab, off)) : pad_class);
      }
    }
    const int o = row * Pw + xg * kPer;
    if constexpr (kPer == 8) {
      *reinterpret_cast<uint4*>(img + o) = make_uint4(h0[0], h0[1], h0[2], h0[3]);
      *reinterpret_cast<uint4*>(img + (size_t)V + o) = make_uint4(h1[0], h1[1], h1[2], h1[3]);
      if (lab) *reinterpret_cast<uint2*>(lab + o) = make_uint2(cl[0], cl[1]);
    } else {
      img[o] = __ushort_as_half((unsigned short)h0[0]);
      img[(size_t)V + o] = __ushort_as_half((unsigned short)h1[0]);
      if (lab) lab[o] = (uint8_t)cl[0];
    }
  }
}

}  // namespace

extern "C" int64_t micf_patch_index_bytes(int64_t voxels, int num_label_values, int has_label) {
  if (voxels <= 0 || num_label_values < 0 || num_label_values > MICF_LOADER_MAX_LABEL_VALUES) return MICF_EINVAL;
  return pc::index_bytes(voxels, num_label_values, has_label != 0);
}

extern "C" int64_t micf_patch_index_workspace(int B) {
  if (B <= 0) return MICF_EINVAL;
  return layout(B).total;
}

extern "C" int micf_patch_index(const micf_loader_sample* samples, int B, const int32_t* label_values, int num_label_values,
                                int ct_mode, int mr_mode, double p_low, double p_high, void* workspace, int64_t workspace_bytes,
                                void* const* indexes, const int64_t* index_bytes, micf_stream_t stream) {
  if (!samples || !workspace || !indexes || !index_bytes || B <= 0) return MICF_EINVAL;
  int rc = check_norm_args(ct_mode, mr_mode, p_low, p_high, nullptr);
  if (rc != MICF_OK) return rc;
  rc = check_label_values(label_values, num_label_values);
  if (rc != MICF_OK) return rc;
  const Layout L = layout(B);
  if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MICF_EINVAL;
  const bool has_label = samples[0].label != nullptr;
  rc = check_scans(samples, B, has_label, num_label_values, indexes, index_bytes);
  if (rc != MICF_OK) return rc;

  hipStream_t s = (hipStream_t)stream;
  const WsView ws = ws_view(workspace, L, nullptr);
  const Modes md{{ct_mode, mr_mode}};
  launch_zero(s, workspace, L.zero_words);
  MinMaxArgs ma;
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  for_each_chunk(samples, B, ma, ra, [&](int b0, int nb, unsigned blocks) {
    const WsView c = ws.chunk(b0);
    launch_statistics(s, ma, md, nb, blocks, p_low, p_high, c);
    IndexArgs ia;
    fill_indexes(ia, indexes, b0, nb);
    hipLaunchKernelGGL(patch_index_init_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, ia, c.recs);
    if (has_label) {
      int64_t most = 1;
      for (int i = 0; i < nb; ++i) {
        const int64_t n = pc::num_segments(ma.v[2 * i].n);
        most = n > most ? n : most;
      }
      hipLaunchKernelGGL(patch_count_kernel, dim3((unsigned)(most < 4096 ? most : 4096), (unsigned)nb), dim3(kThreads), 0, s, ra, ia);
    }
  });
  MICF_RETURN_LAUNCH();
}

extern "C" int micf_patch_sample(const micf_loader_sample* samples, int B, void* const* indexes, const int64_t* index_bytes,
                                 const int32_t* label_values, int num_label_values, const float* draws, int Pd, int Ph, int Pw,
                                 int padding_mode, int pad_class, int clamp, void* image, uint8_t* label_map, int32_t* origins,
                                 int32_t* picked, micf_stream_t stream) {
  const SampleCall c{samples, B, indexes, index_bytes, label_values, num_label_values, draws, Pd, Ph, Pw, padding_mode, pad_class, clamp,
                     image, label_map, origins, picked};
  const int per = Pw % 8 == 0 ? 8 : 1;
  const int rc = check_sample_call(c, per);
  if (rc != MICF_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int border = padding_mode == MICF_PATCH_PAD_BORDER ? 1 : 0;
  sample_chunks(c, per, s, [&](dim3 grid, const ResizeArgs& ra, const IndexArgs& ia, const int32_t* org, __half* img0, uint8_t* lab0, int) {
    const auto launch = [&](auto kper) {
      hipLaunchKernelGGL(patch_crop_kernel<decltype(kper)::value>, grid, dim3(kThreads), 0, s, ra, ia, org, Pd, Ph, Pw, border, pad_class,
                         img0, lab0);
    };
    if (per == 8) launch(Int<8>{});
    else launch(Int<1>{});
  });
  MICF_RETURN_LAUNCH();
}
