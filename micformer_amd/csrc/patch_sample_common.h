// patch_sample_common.h -- the host path that micf_patch_sample (volume_patches.hip) and micf_patch_sample_warped
// (volume_patch_warp.hip) share around patch_locate.h's kernel: SampleCall, the arguments the two entries have in common;
// check_sample_call, their checks; sample_chunks, the chunk driver that launches the locate kernel and hands every chunk to the
// entry's own crop launch.  Unnamed namespace, as patch_locate.h.
#pragma once
#include <type_traits>
#include "patch_locate.h"

namespace {

template <int N>
using Int = std::integral_constant<int, N>;                      // a template argument chosen at run time, handed to a generic lambda

// The leading arguments of both entries, in their order.
struct SampleCall {
  const micf_loader_sample* samples; int B; void* const* indexes; const int64_t* index_bytes;
  const int32_t* label_values; int num_label_values; const float* draws; int Pd, Ph, Pw, padding_mode, pad_class, clamp;
  void* image; uint8_t* label_map; int32_t *origins, *picked;
};

// Every check of these arguments, MICF_EINVAL before MICF_EUNSUPPORTED.  per: outputs per thread of the crop kernel that will run
// (8, 4 or 1); its stores want image aligned to 2 * per bytes and label_map to per bytes.
inline int check_sample_call(const SampleCall& c, int per) {
  if (!c.samples || !c.indexes || !c.index_bytes || !c.draws || !c.image || !c.origins || !c.picked || c.B <= 0 || c.Pd <= 0 ||
      c.Ph <= 0 || c.Pw <= 0)
    return MICF_EINVAL;
  if (c.padding_mode != MICF_PATCH_PAD_ZEROS && c.padding_mode != MICF_PATCH_PAD_BORDER) return MICF_EINVAL;
  if (c.clamp != MICF_PATCH_CLAMP_BOTH && c.clamp != MICF_PATCH_CLAMP_LOWER) return MICF_EINVAL;
  if (c.pad_class < 0 || c.pad_class > 255) return MICF_EINVAL;
  int rc = check_label_values(c.label_values, c.num_label_values);
  if (rc != MICF_OK) return rc;
  const auto off = [](const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) != 0; };
  if (off(c.image, 2 * per) || off(c.label_map, per) || off(c.draws, 4) || off(c.origins, 4) || off(c.picked, 4)) return MICF_EINVAL;
  rc = check_scans(c.samples, c.B, c.label_map != nullptr, c.num_label_values, c.indexes, c.index_bytes);
  if (rc != MICF_OK) return rc;
  if ((int64_t)c.Pd * c.Ph > kMaxTarget || (int64_t)c.Pd * c.Ph * c.Pw > kMaxTarget) return MICF_EUNSUPPORTED;
  return MICF_OK;
}

// The batch in chunks of kChunk samples: per chunk the locate launch, then crop(grid, ra, ia, origins, image, label_map, b0) --
// the entry's crop launch for the chunk that starts at sample b0, a thread per `per` outputs; the three pointers are the chunk's.
template <class F>
inline void sample_chunks(const SampleCall& c, int per, hipStream_t s, F&& crop) {
  const int64_t V = (int64_t)c.Pd * c.Ph * c.Pw;
  MinMaxArgs ma;
  ResizeArgs ra;
  fill_label_values(ra, c.label_values, c.num_label_values);
  for_each_chunk(c.samples, c.B, ma, ra, [&](int b0, int nb, unsigned) {
    IndexArgs ia;
    fill_indexes(ia, c.indexes, b0, nb);
    int32_t* org = c.origins + (size_t)b0 * 3;
    hipLaunchKernelGGL(patch_locate_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, ra, ia, c.draws + (size_t)b0 * 6, c.Pd, c.Ph,
                       c.Pw, c.label_map ? 1 : 0, c.clamp == MICF_PATCH_CLAMP_LOWER ? 1 : 0, org, c.picked + (size_t)b0 * 4);
    crop(dim3(resize_blocks(V / per), (unsigned)nb), ra, ia, org, static_cast<__half*>(c.image) + (size_t)b0 * 2 * V,
         c.label_map ? c.label_map + (size_t)b0 * V : nullptr, b0);
  });
}

}  // namespace
