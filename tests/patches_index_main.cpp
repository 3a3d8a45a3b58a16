// Stand-alone host check of micformer_amd/csrc/patches_coords.h: the very origin, index and segment functions
// csrc/volume_patches.hip runs.  It prints one line per result -- the origin bounds and origins at extents 1 .. 2048, draw_index at
// counts 1 and 2^31 - 1 for u = 0, 0x3f7fffff (the float below 1), 1, -1 and NaN, the segment bookkeeping at voxel counts that the
// segment length does and does not divide -- and tests/test_patches_cpu.py compares every line with tests/patches_ref.py.  The
// last block runs the locate step's strip walk over real arrays of segment counts, so an address outside them is the address
// sanitizer's to report.  tests/test_patches_cpu.py compiles this with the host compiler under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../micformer_amd/csrc/patches_coords.h"

namespace P = micf_patches;

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

int main() {
  const int extents[] = {1, 2, 3, 16, 127, 128, 129, 2047, 2048};
  const uint32_t us[] = {0x00000000u, 0x3f7fffffu, 0x3f800000u, 0xbf800000u, 0x7fc00000u, 0x3f000000u, 0x3eaaaaabu};
  std::printf("segment %d\n", P::kSegment);
  for (int L : extents)
    for (int Pe : extents) {
      std::printf("bounds %d %d %d %d\n", L, Pe, P::origin_lb(L, Pe), P::origin_ub(L, Pe));
      for (uint32_t u : us) std::printf("random %u %d %d %d\n", u, L, Pe, P::random_origin(from_bits(u), L, Pe));
      const int vs[] = {0, L / 2, L - 1};
      for (int v : vs)
        for (int lower = 0; lower < 2; ++lower) {
          const int o = P::centred_origin(v, L, Pe, lower != 0);
          std::printf("centred %d %d %d %d %d\n", v, L, Pe, lower, o);
          // the voxel lies inside its window, and every position of the window clamps into the scan
          if (!(o <= v && v < o + Pe)) return 2;
          for (int i = 0; i < Pe; ++i) {
            const int c = P::clamp_index(o + i, L);
            if (c < 0 || c >= L || (P::inside(o + i, L) && c != o + i)) return 3;
          }
        }
    }
  const int64_t counts[] = {1, 2, 7, 2048, 2147483647LL};
  for (int64_t n : counts)
    for (uint32_t u : us) std::printf("index %u %lld %lld\n", u, (long long)n, (long long)P::draw_index(from_bits(u), n));
  const int64_t voxels[] = {1, 2047, 2048, 2049, 5000, 95158272LL, 2147483647LL};
  for (int64_t V : voxels) {
    const int64_t nseg = P::num_segments(V), row = P::padded_segments(V);
    if (row < nseg || row >= nseg + P::kRowAlign || row % P::kRowAlign) return 7;
    int64_t covered = 0, expect_lo = 0;
    for (int t = 0; t < 256; ++t) {
      int64_t lo, hi;
      P::segment_strip(row, t, 256, lo, hi);
      if (lo > hi || (lo < row && lo != expect_lo) || lo % P::kRowAlign || hi % P::kRowAlign) return 4;
      covered += hi - lo;
      expect_lo = hi;
    }
    if (covered != row) return 5;
    std::printf("segments %lld %lld %d %d %lld %lld\n", (long long)V, (long long)nseg, P::segment_voxels(nseg - 1, V),
                P::segment_voxels(0, V), (long long)P::index_bytes(V, 7, true), (long long)P::index_bytes(V, 7, false));
  }
  {
    int z, y, x;
    const int64_t vs[] = {0, 1, 2047, 2048, 2147483646LL};
    for (int64_t v : vs) {
      P::unflatten(v, 2048, 2048, z, y, x);
      std::printf("unflatten %lld %d %d %d\n", (long long)v, z, y, x);
    }
  }
  // the locate step on the host: per-segment counts of a labelled volume whose size the segment length does not divide, the 256
  // strips, the prefix, the walk; every rank must come back as the voxel a linear scan finds
  {
    const int64_t V = (int64_t)600 * P::kSegment + 777;          // 601 segments in a row of 604: strips of 4, the last threads' strips empty
    std::vector<uint8_t> cls((size_t)V);
    for (int64_t i = 0; i < V; ++i)                              // a multiplicative hash of the index: about 1 % of the voxels
      cls[(size_t)i] = (((uint32_t)i * 2654435761u) >> 24) < 3 ? 1 : 0;
    const int64_t nseg = P::num_segments(V), row = P::padded_segments(V);
    std::vector<uint16_t> seg((size_t)row, 0);
    std::vector<int64_t> where;
    for (int64_t s = 0; s < nseg; ++s) {
      uint32_t n = 0;
      for (int i = 0; i < P::segment_voxels(s, V); ++i) n += cls[(size_t)(s * P::kSegment + i)];
      seg[(size_t)s] = (uint16_t)n;
    }
    for (int64_t i = 0; i < V; ++i)
      if (cls[(size_t)i]) where.push_back(i);
    const int64_t n = (int64_t)where.size();
    const int64_t ranks[] = {0, 1, n / 3, n / 2, n - 2, n - 1};
    for (int64_t r : ranks) {
      uint32_t excl = 0;
      int64_t found = -1;
      for (int t = 0; t < 256 && found < 0; ++t) {
        int64_t lo, hi;
        P::segment_strip(row, t, 256, lo, hi);
        uint32_t sum = 0;
        for (int64_t s = lo; s < hi; ++s) sum += seg[(size_t)s];
        if ((uint32_t)r >= excl && (uint32_t)r - excl < sum) {
          uint32_t run = excl;
          for (int64_t s = lo; s < hi; ++s) {
            if ((uint32_t)r - run < seg[(size_t)s]) {
              uint32_t left = (uint32_t)r - run;
              for (int i = 0; i < P::segment_voxels(s, V); ++i) {
                if (cls[(size_t)(s * P::kSegment + i)] && left-- == 0) {
                  found = s * P::kSegment + i;
                  break;
                }
              }
              break;
            }
            run += seg[(size_t)s];
          }
        }
        excl += sum;
      }
      if (found != where[(size_t)r]) return 6;
      std::printf("locate %lld %lld %lld\n", (long long)V, (long long)r, (long long)found);
    }
  }
  std::printf("patches_coords: done\n");
  return 0;
}
