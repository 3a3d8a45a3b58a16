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
//   2 crop       patch_crop_kernel, grid (blocks, samples), the only bandwidth path: reads origins from device memory; a thread
//                makes 8 consecutive output voxels of a row (Pw % 8 == 0: one 16-byte store per channel, one 8-byte store of
//                classes) or one voxel (any Pw).  Source rows start at an arbitrary element offset: where the 8 positions
//                lie inside one row of int16 arrays, each array is read with two aligned 16-byte loads and shifted by the byte
//                offset (select + v_alignbit; 64 against 87 us at 8 x 128^3 under the kernel trace); elsewhere -- float32
//                arrays, groups that cross the scan's border or touch the array's last bytes -- per element, every index
//                clamped into the scan before it is used.
// Everything that crosses threads is an integer: bit-identical from run to run, independent of the other samples.  No scratch.
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

// ---- sample: 2 crop -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float norm_tap(const Vol3& v, bool f32, int64_t off, const NormAny& nm) {
  return f32 ? tap<true>(v.p, off, nm) : tap<false>(v.p, off, nm);
}

// The normalised value of one raw int16 element: tap<false>'s arithmetic on a value already in a register.
__device__ __forceinline__ float norm_i16(int x, const NormAny& nm) {
  if (nm.mode == MICF_NORM_MINMAX) return (float)(x - nm.mm.imin) / nm.mm.scale;
  const float f = (float)x;
  if (nm.mode == MICF_NORM_ZSCORE) return f != 0.0f ? (f - nm.a) / nm.b : 0.0f;
  return (fminf(fmaxf(f, nm.a), nm.b) - nm.a) / nm.scale;
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

// grid (blocks, samples of the chunk); origins / image / label_map point at the chunk's first sample
template <bool kVec>
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
  constexpr int kPer = kVec ? 8 : 1;
  const int groups = Pw / kPer, items = Pd * Ph * groups;
  for (int item = blockIdx.x * kThreads + threadIdx.x; item < items; item += gridDim.x * kThreads) {
    const int xg = item % groups, row = item / groups, y = row % Ph, z = row / Ph;
    const int sz = oz + z, sy = oy + y;
    const bool in_zy = pc::inside(sz, d) && pc::inside(sy, h);
    const int64_t rowoff = ((int64_t)pc::clamp_index(sz, d) * h + pc::clamp_index(sy, h)) * w;
    uint32_t h0[kVec ? 4 : 1] = {}, h1[kVec ? 4 : 1] = {}, cl[kVec ? 2 : 1] = {};
    if (kVec) {                                                  // the 8 positions lie in one source row: two vector loads per array
      const int sx0 = ox + xg * kPer;
      uint32_t r0[4], r1[4], rl[4];
      if (sx0 >= 0 && sx0 + kPer <= w && (in_zy || border) && !ct32 && !mr32 && (!lab || sd.lab.dtype == MICF_LOADER_I16) &&
          shifted8_i16(sd.ct.p, (int64_t)d * h * w, rowoff + sx0, r0) && shifted8_i16(sd.mr.p, (int64_t)d * h * w, rowoff + sx0, r1) &&
          (!lab || !in_zy || shifted8_i16(sd.lab.p, (int64_t)d * h * w, rowoff + sx0, rl))) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const float c0 = norm_i16(unpack_i16(r0, j), nct), c1 = norm_i16(unpack_i16(r1, j), nmr);
          const int c = (lab && in_zy) ? label_class(a, unpack_i16(rl, j)) : pad_class;
          h0[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c0)) << (16 * (j & 1));
          h1[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c1)) << (16 * (j & 1));
          cl[j / 4] |= (uint32_t)c << (8 * (j & 3));
        }
        const int o = row * Pw + xg * kPer;
        *reinterpret_cast<uint4*>(img + o) = make_uint4(h0[0], h0[1], h0[2], h0[3]);
        *reinterpret_cast<uint4*>(img + (size_t)V + o) = make_uint4(h1[0], h1[1], h1[2], h1[3]);
        if (lab) *reinterpret_cast<uint2*>(lab + o) = make_uint2(cl[0], cl[1]);
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int sx = ox + xg * kPer + j;
      const bool in = in_zy && pc::inside(sx, w);
      const int64_t off = rowoff + pc::clamp_index(sx, w);
      float c0 = 0.0f, c1 = 0.0f;
      if (in || border) {
        c0 = norm_tap(sd.ct, ct32, off, nct);
        c1 = norm_tap(sd.mr, mr32, off, nmr);
      }
      int c = pad_class;
      if (lab && in) c = label_class(a, raw_label(sd.lab, off));
      h0[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c0)) << (16 * (j & 1));
      h1[j / 2] |= (uint32_t)__half_as_ushort(__float2half_rn(c1)) << (16 * (j & 1));
      cl[j / 4] |= (uint32_t)c << (8 * (j & 3));
    }
    const int o = row * Pw + xg * kPer;
    if (kVec) {
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
  if (!samples || !indexes || !index_bytes || !draws || !image || !origins || !picked || B <= 0 || Pd <= 0 || Ph <= 0 || Pw <= 0)
    return MICF_EINVAL;
  if (padding_mode != MICF_PATCH_PAD_ZEROS && padding_mode != MICF_PATCH_PAD_BORDER) return MICF_EINVAL;
  if (clamp != MICF_PATCH_CLAMP_BOTH && clamp != MICF_PATCH_CLAMP_LOWER) return MICF_EINVAL;
  if (pad_class < 0 || pad_class > 255) return MICF_EINVAL;
  int rc = check_label_values(label_values, num_label_values);
  if (rc != MICF_OK) return rc;
  const bool vec = Pw % 8 == 0;
  if (reinterpret_cast<uintptr_t>(image) & (vec ? 15 : 1)) return MICF_EINVAL;
  if (vec && (reinterpret_cast<uintptr_t>(label_map) & 7)) return MICF_EINVAL;
  if ((reinterpret_cast<uintptr_t>(draws) & 3) || (reinterpret_cast<uintptr_t>(origins) & 3) || (reinterpret_cast<uintptr_t>(picked) & 3))
    return MICF_EINVAL;
  rc = check_scans(samples, B, label_map != nullptr, num_label_values, indexes, index_bytes);
  if (rc != MICF_OK) return rc;
  if ((int64_t)Pd * Ph > kMaxTarget || (int64_t)Pd * Ph * Pw > kMaxTarget) return MICF_EUNSUPPORTED;

  hipStream_t s = (hipStream_t)stream;
  const int64_t V = (int64_t)Pd * Ph * Pw;
  MinMaxArgs ma;
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  for_each_chunk(samples, B, ma, ra, [&](int b0, int nb, unsigned) {
    IndexArgs ia;
    fill_indexes(ia, indexes, b0, nb);
    hipLaunchKernelGGL(patch_locate_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, ra, ia, draws + (size_t)b0 * 6, Pd, Ph, Pw,
                       label_map ? 1 : 0, clamp == MICF_PATCH_CLAMP_LOWER ? 1 : 0, origins + (size_t)b0 * 3, picked + (size_t)b0 * 4);
    __half* img0 = static_cast<__half*>(image) + (size_t)b0 * 2 * V;
    uint8_t* lab0 = label_map ? label_map + (size_t)b0 * V : nullptr;
    const dim3 grid(resize_blocks(vec ? V / 8 : V), (unsigned)nb);
    if (vec)
      hipLaunchKernelGGL(patch_crop_kernel<true>, grid, dim3(kThreads), 0, s, ra, ia, origins + (size_t)b0 * 3, Pd, Ph, Pw,
                         padding_mode == MICF_PATCH_PAD_BORDER ? 1 : 0, pad_class, img0, lab0);
    else
      hipLaunchKernelGGL(patch_crop_kernel<false>, grid, dim3(kThreads), 0, s, ra, ia, origins + (size_t)b0 * 3, Pd, Ph, Pw,
                         padding_mode == MICF_PATCH_PAD_BORDER ? 1 : 0, pad_class, img0, lab0);
  });
  MICF_RETURN_LAUNCH();
}
