// patches_coords.h -- the index arithmetic of the patch sampler (include/micformer_patches.h): origin bounds of a window on an
// axis, a uniform draw -> an index, the clamp of a foreground-centred origin, flat voxel <-> (z, y, x), the segment bookkeeping of
// the index and the layout of an index buffer.  In the style of affine_coords.h: every function is __host__ __device__ and plain
// C++ (no HIP header needed), so a host program calls the very code volume_patches.hip runs (tests/patches_index_main.cpp does).
// Everything is integer arithmetic but draw_index, whose one float64 product is exact enough by construction: u has 24
// significant bits and n fewer than 2^31, so u * n is exact in float64 and the truncation is the floor.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MICF_PHD __host__ __device__ inline
#else
#define MICF_PHD inline
#endif

namespace micf_patches {

// Voxels per segment of the index: a run of kSegment consecutive voxels in flat (z, y, x) order.  2048 = 256 threads x 8 voxels:
// the counting pass takes a segment per workgroup trip with one LDS histogram and no cross-workgroup traffic, the locate step
// resolves a rank inside one segment in 8 ballot rounds of its 256 threads, a count fits 16 bits (the index holds 2 bytes per
// class and segment: 0.65 MB for a 363 x 512 x 512 scan with 7 classes, one row of 93 KB read per forced patch), and the 46 464
// segment counts of a class of such a scan are summed by one workgroup in 46 8-byte loads (184 counts) per thread.
constexpr int kSegment = 2048;

constexpr int64_t kHeaderBytes = 256;       // the statistics record of the scan (csrc/volume_normalise_stats.h SampleRec)
constexpr int64_t kCountsBytes = 1024;      // uint32 [256]: voxels of class 0, 1..K, then "other" at K + 1
constexpr int64_t kSegmentsOffset = kHeaderBytes + kCountsBytes + 256;   // (256 bytes reserved)

// need = max(P - L, 0); lb = -ceil(need / 2); ub = L + floor(need / 2) + need mod 2 - P.  For odd need lb = ub - 1.
MICF_PHD int origin_lb(int L, int P) {
  const int need = P > L ? P - L : 0;
  return -((need + 1) / 2);
}
MICF_PHD int origin_ub(int L, int P) {
  const int need = P > L ? P - L : 0;
  return L + need / 2 + need % 2 - P;
}

// min(int64(double(u) * double(n)), n - 1); 0 for u < 0 or NaN, n - 1 for u >= 1.  n >= 1.
MICF_PHD int64_t draw_index(float u, int64_t n) {
  if (!(u >= 0.0f)) return 0;               // (true for NaN)
  if (u >= 1.0f) return n - 1;
  const int64_t k = (int64_t)((double)u * (double)n);
  return k < n - 1 ? k : n - 1;
}

// origin of a random crop on an axis
MICF_PHD int random_origin(float u, int L, int P) {
  const int lb = origin_lb(L, P), ub = origin_ub(L, P);
  return lb + (int)draw_index(u, (int64_t)(ub - lb + 1));
}

// origin of a crop centred on voxel v of an axis: v - P / 2 clamped to [lb, ub], or below only (clamp_lower_only)
MICF_PHD int centred_origin(int v, int L, int P, bool lower_only) {
  const int lb = origin_lb(L, P), ub = origin_ub(L, P);
  int o = v - P / 2;
  o = o > lb ? o : lb;
  if (!lower_only) o = o < ub ? o : ub;
  return o;
}

// window position o + i on an axis -> the scan index it reads (clamped into [0, L): the nearest voxel) and whether it is inside
MICF_PHD int clamp_index(int s, int L) { return s < 0 ? 0 : (s < L ? s : L - 1); }
MICF_PHD bool inside(int s, int L) { return s >= 0 && s < L; }

// flat voxel -> (z, y, x)
MICF_PHD void unflatten(int64_t v, int h, int w, int& z, int& y, int& x) {
  x = (int)(v % w);
  const int64_t t = v / w;
  y = (int)(t % h);
  z = (int)(t / h);
}

// segments of a scan of `voxels` voxels, and the voxels of segment s (the last one may be short)
MICF_PHD int64_t num_segments(int64_t voxels) { return (voxels + kSegment - 1) / kSegment; }
MICF_PHD int segment_voxels(int64_t s, int64_t voxels) {
  const int64_t left = voxels - s * kSegment;
  return (int)(left < kSegment ? (left > 0 ? left : 0) : kSegment);
}

// A class's row of segment counts is padded with zeros to a multiple of kRowAlign entries, so that every row starts on an 8-byte
// boundary and is read as whole 8-byte vectors of 4 counts.
constexpr int kRowAlign = 4;
MICF_PHD int64_t padded_segments(int64_t voxels) { return (num_segments(voxels) + kRowAlign - 1) / kRowAlign * kRowAlign; }

// The contiguous strip [lo, hi) of a padded row that thread t of `threads` sums in the locate step: whole vectors,
// ceil(vectors / threads) each; the last threads' strips may be empty.
MICF_PHD void segment_strip(int64_t padded, int t, int threads, int64_t& lo, int64_t& hi) {
  const int64_t vectors = padded / kRowAlign, per = (vectors + threads - 1) / threads * kRowAlign;
  lo = (int64_t)t * per;
  lo = lo < padded ? lo : padded;
  hi = lo + per < padded ? lo + per : padded;
}

// bytes of the index of one scan: header, class counts, then (labelled scans) uint16 [K][padded segments], rounded up to 256
MICF_PHD int64_t index_bytes(int64_t voxels, int num_label_values, bool has_label) {
  int64_t n = kSegmentsOffset;
  if (has_label) n += (int64_t)num_label_values * padded_segments(voxels) * 2;
  return (n + 255) & ~(int64_t)255;
}

}  // namespace micf_patches
