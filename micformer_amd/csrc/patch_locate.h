// patch_locate.h -- the locate step of the patch sampler and what goes with it, shared by volume_patches.hip (the plain crop) and
// volume_patch_warp.hip (the crop through a map): the view of an index buffer, the workgroup prefix, patch_locate_kernel, and the
// host-side checks of the samples and their indexes.  Moved here from volume_patches.hip with its text unchanged.  Unnamed
// namespace: each including file gets its own copy of the kernel, so both entry points launch the very same code and a draw gives
// the same origin and pick through either.  The launch itself, and everything else the two `sample` entries share, is
// patch_sample_common.h's.
#pragma once
#include "volume_normalise_stats.h"
#include "patches_coords.h"
#include "../../include/micformer_patches.h"

namespace {

namespace pc = micf_patches;

static_assert(pc::kSegment == MICF_PATCH_SEGMENT, "the header's segment length is patches_coords.h's");
static_assert(pc::kSegment % kThreads == 0 && pc::kSegment <= 65535, "a segment is whole rounds of the workgroup, a count fits 16 bits");
static_assert(sizeof(SampleRec) == pc::kHeaderBytes, "the index starts with the scan's statistics record");
static_assert(MICF_LOADER_MAX_LABEL_VALUES + 2 <= kThreads, "one histogram bin per thread");
constexpr int kRounds = pc::kSegment / kThreads;

struct IndexArgs { char* idx[kChunk]; };

__device__ __forceinline__ uint32_t* index_counts(char* idx) { return reinterpret_cast<uint32_t*>(idx + pc::kHeaderBytes); }
__device__ __forceinline__ uint16_t* index_segments(char* idx) { return reinterpret_cast<uint16_t*>(idx + pc::kSegmentsOffset); }

// ---- sample: 1 locate -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void write_random(const float* u, const Vol3& v, int Pd, int Ph, int Pw, int32_t* origin, int32_t* pick) {
  origin[0] = pc::random_origin(u[3], v.d, Pd);
  origin[1] = pc::random_origin(u[4], v.h, Ph);
  origin[2] = pc::random_origin(u[5], v.w, Pw);
  pick[0] = 0; pick[1] = -1; pick[2] = -1; pick[3] = -1;
}

// Exclusive prefix of v over the workgroup's threads and the total; every thread calls it; s_wave [kWaves] is free to overwrite.
__device__ __forceinline__ void block_scan(uint32_t v, uint32_t* s_wave, uint32_t& excl, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  excl = inc - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    excl += w < wave ? s_wave[w] : 0;
    total += s_wave[w];
  }
}

// grid (samples of the chunk); draws / origins / picked point at the chunk's first sample
__global__ __launch_bounds__(kThreads) void patch_locate_kernel(ResizeArgs a, IndexArgs ia, const float* draws, int Pd, int Ph, int Pw,
                                                                int has_label, int lower_only, int32_t* origins, int32_t* picked) {
  __shared__ uint32_t s_wave[kWaves], s_cnt[kRounds * kWaves], s_rem;
  __shared__ long long s_seg, s_lo, s_hi;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SampleDesc& sd = a.s[b];
  const float* u = draws + (size_t)b * 6;
  int32_t* origin = origins + (size_t)b * 3;
  int32_t* pick = picked + (size_t)b * 4;
  const int K = a.nvals;
  char* idx = ia.idx[b];
  int cls = 0;
  uint32_t rank = 0;
  if (has_label && u[0] >= 0.5f) {                               // (false for NaN)
    const uint32_t* counts = index_counts(idx);
    int present = 0;
    for (int k = 1; k <= K; ++k) present += counts[k] != 0;
    if (present) {
      const int j = (int)pc::draw_index(u[1], present);
      int seen = 0;
      for (int k = 1; k <= K; ++k) {
        if (counts[k] != 0) {
          cls = seen == j ? k : cls;
          ++seen;
        }
      }
      rank = (uint32_t)pc::draw_index(u[2], (int64_t)counts[cls]);
    }
  }
  if (cls == 0) {                                                // uniform: every thread read the same words
    if (tid == 0) write_random(u, sd.ct, Pd, Ph, Pw, origin, pick);
    return;
  }
  const Vol3& lv = sd.lab;
  const int64_t V = (int64_t)lv.d * lv.h * lv.w, row = pc::padded_segments(V);
  const uint16_t* seg = index_segments(idx) + (int64_t)(cls - 1) * row;
  if (tid == 0) {
    s_seg = -1;
    s_lo = 0;
    s_hi = 0;
  }
  // a. every thread sums its strip of the row: 8-byte vectors of four counts, four loads in flight
  int64_t lo, hi;
  pc::segment_strip(row, tid, kThreads, lo, hi);
  const uint2* vec = reinterpret_cast<const uint2*>(seg);
  auto sum4 = [](const uint2& q) { return (q.x & 0xFFFFu) + (q.x >> 16) + (q.y & 0xFFFFu) + (q.y >> 16); };
  uint32_t sum = 0;
  {
    int64_t i = lo / pc::kRowAlign;
    const int64_t end = hi / pc::kRowAlign;
    for (; i + 3 < end; i += 4) {
      const uint2 q0 = vec[i], q1 = vec[i + 1], q2 = vec[i + 2], q3 = vec[i + 3];
      sum += sum4(q0) + sum4(q1) + sum4(q2) + sum4(q3);
    }
    for (; i < end; ++i) sum += sum4(vec[i]);
  }
  uint32_t excl, total;
  block_scan(sum, s_wave, excl, total);
  if (rank >= excl && rank - excl < sum) {                       // exactly one thread: its strip holds the rank
    s_lo = lo;
    s_hi = hi;
    s_rem = rank - excl;
  }
  __syncthreads();
  // b. the workgroup walks that strip, 256 segments per trip, with a prefix per trip
  const int64_t strip_lo = s_lo, strip_hi = s_hi;
  const uint32_t want = s_rem;
  uint32_t carry = 0;
  for (int64_t s0 = strip_lo; s0 < strip_hi; s0 += kThreads) {
    const int64_t sg = s0 + tid;
    const uint32_t c = sg < strip_hi ? seg[sg] : 0;
    __syncthreads();                                             // (the previous trip's s_wave has been read)
    block_scan(c, s_wave, excl, total);
    if (want >= carry + excl && want - (carry + excl) < c) {
      s_seg = sg;
      s_rem = want - (carry + excl);
    }
    carry += total;
  }
  __syncthreads();
  const int64_t found = s_seg;
  if (found < 0) {                                               // the index is not this scan's: no address is formed from it
    if (tid == 0) write_random(u, sd.ct, Pd, Ph, Pw, origin, pick);
    return;
  }
  const uint32_t rem = s_rem;
  const int64_t base = found * pc::kSegment;
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const int64_t v = base + j * kThreads + tid;
    const bool match = v < V && label_class(a, raw_label(lv, v)) == cls;
    const unsigned long long m = __ballot(match);
    if (lane == 0) s_cnt[j * kWaves + wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  int group = -1;
  uint32_t within = 0, run = 0;
#pragma unroll
  for (int g = 0; g < kRounds * kWaves; ++g) {                   // (round-major, wave-minor: flat voxel order)
    const uint32_t c = s_cnt[g];
    if (group < 0 && rem - run < c) {
      group = g;
      within = rem - run;
    }
    run += group < 0 ? c : 0;
  }
  if (group < 0) {                                               // (the segment's labels no longer hold the count the index recorded)
    if (tid == 0) write_random(u, sd.ct, Pd, Ph, Pw, origin, pick);
    return;
  }
  const int64_t v = base + (group / kWaves) * kThreads + tid;
  const bool match = v < V && label_class(a, raw_label(lv, v)) == cls;
  const unsigned long long m = __ballot(match);
  const unsigned long long below = lane == 0 ? 0ull : (m & (~0ull >> (64 - lane)));
  if (wave == group % kWaves && match && (uint32_t)__popcll(below) == within) {
    int z, y, x;
    pc::unflatten(v, lv.h, lv.w, z, y, x);
    origin[0] = pc::centred_origin(z, lv.d, Pd, lower_only != 0);
    origin[1] = pc::centred_origin(y, lv.h, Ph, lower_only != 0);
    origin[2] = pc::centred_origin(x, lv.w, Pw, lower_only != 0);
    pick[0] = cls; pick[1] = z; pick[2] = y; pick[3] = x;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline int check_label_values(const int32_t* label_values, int num_label_values) {
  if (num_label_values < 0 || num_label_values > MICF_LOADER_MAX_LABEL_VALUES || (num_label_values > 0 && !label_values))
    return MICF_EINVAL;
  for (int i = 0; i < num_label_values; ++i) {
    if (label_values[i] == 0) return MICF_EINVAL;
    for (int j = 0; j < i; ++j)
      if (label_values[j] == label_values[i]) return MICF_EINVAL;
  }
  return MICF_OK;
}

// The samples and their index buffers: MICF_EINVAL before MICF_EUNSUPPORTED.  has_label: what every sample must agree with.
inline int check_scans(const micf_loader_sample* samples, int B, bool has_label, int num_label_values, void* const* indexes,
                       const int64_t* index_bytes) {
  int unsupported = 0;
  for (int b = 0; b < B; ++b) {
    const micf_loader_sample& s = samples[b];
    if ((s.label != nullptr) != has_label) return MICF_EINVAL;
    const int rc[3] = {check_volume(s.ct, s.ct_shape, s.ct_dtype, false), check_volume(s.mr, s.mr_shape, s.mr_dtype, false),
                       s.label ? check_volume(s.label, s.label_shape, s.label_dtype, true) : MICF_OK};
    for (int r : rc) {
      if (r == MICF_EINVAL) return MICF_EINVAL;
      if (r == MICF_EUNSUPPORTED) unsupported = 1;
    }
    for (int ax = 0; ax < 3; ++ax)
      if (s.ct_shape[ax] != s.mr_shape[ax] || (s.label && s.ct_shape[ax] != s.label_shape[ax])) return MICF_EINVAL;
    if (!indexes[b] || (reinterpret_cast<uintptr_t>(indexes[b]) & 255)) return MICF_EINVAL;
    const int64_t voxels = (int64_t)s.ct_shape[0] * s.ct_shape[1] * s.ct_shape[2];
    if (index_bytes[b] < pc::index_bytes(voxels, num_label_values, has_label)) return MICF_EINVAL;
  }
  return unsupported ? MICF_EUNSUPPORTED : MICF_OK;
}

inline void fill_indexes(IndexArgs& ia, void* const* indexes, int b0, int nb) {
  for (int i = 0; i < kChunk; ++i) ia.idx[i] = static_cast<char*>(indexes[b0 + (i < nb ? i : 0)]);
}

}  // namespace
