// Stand-alone host check of micformer_amd/csrc/affine_coords.h: the very coordinate-to-tap functions csrc/volume_affine.hip runs,
// fed NaN, +-inf, +-1e30, values around the array's two edges and the extents 1 and 2048, directly and through the whole chain
// from a map row.  Every returned index must lie in [0, extent); exits non-zero otherwise.  tests/test_affine_cpu.py compiles
// this with the host compiler under -fsanitize=address,undefined (a float-to-int conversion out of range is reported there) and
// runs it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../micformer_amd/csrc/affine_coords.h"

namespace A = micf_affine;

static int failures = 0;

static void expect(bool ok, const char* what, float v, int extent, int border) {
  if (!ok) {
    std::fprintf(stderr, "FAIL %s: value %g extent %d border %d\n", what, (double)v, extent, border);
    ++failures;
  }
}

static void check_index(float i, int extent) {
  for (int border = 0; border < 2; ++border) {
    const A::LinearTaps t = A::linear_taps(i, extent, border != 0);
    expect(t.i0 >= 0 && t.i0 < extent && t.i1 >= 0 && t.i1 < extent, "linear tap out of range", i, extent, border);
    expect(t.w1 >= 0.0f && t.w1 <= 1.0f && t.w0 >= 0.0f && t.w0 <= 1.0f, "linear weight out of [0, 1]", i, extent, border);
    if (border) expect(t.in0 && t.in1, "border tap flagged outside", i, extent, border);
    bool inside = false;
    const int k = A::nearest_tap(i, extent, border != 0, inside);
    expect(k >= 0 && k < extent, "nearest tap out of range", i, extent, border);
    if (border) expect(inside, "border nearest flagged outside", i, extent, border);
    if (!border && !(i >= -0.5f && i <= (float)extent - 0.5f)) expect(!inside, "outside index flagged inside", i, extent, border);
    if (!border && !(i > -1.0f && i < (float)extent)) expect(!t.in0 || t.w0 == 0.0f, "far tap carries weight", i, extent, border);
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float big[] = {nan, -nan, inf, -inf, 1e30f, -1e30f, 3.4e38f, -3.4e38f, 2147483648.0f, -2147483904.0f, 4294967296.0f, 0.0f, -0.0f};
  const int extents[] = {1, 2, 3, 29, 37, 512, 2047, 2048};
  for (int extent : extents) {
    std::vector<float> v(big, big + sizeof(big) / sizeof(big[0]));
    const float edges[] = {-1.0f, -0.5f, 0.0f, 0.5f, (float)extent - 1.5f, (float)extent - 1.0f, (float)extent - 0.5f, (float)extent,
                           (float)extent + 0.5f};
    for (float e : edges) {
      v.push_back(e);
      v.push_back(std::nextafterf(e, inf));
      v.push_back(std::nextafterf(e, -inf));
      v.push_back(e + 1e-3f);
      v.push_back(e - 1e-3f);
    }
    for (float i : v) check_index(i, extent);
    // the whole chain: a map row holding each special value in each place, at the corners and the centre of a 3-voxel grid
    for (float s : big) {
      for (int place = 0; place < 4; ++place) {
        float row[4] = {1.0f, 0.0f, 0.0f, 0.0f};
        row[place] = s;
        for (int o = 0; o < 3; ++o) {
          const float n = A::norm_coord(o, 3);
          const float sc = A::map_row(row, n, -n, n);
          if (!A::finite(s) && place == 3) expect(!A::finite(sc), "non-finite map gave a finite coordinate", sc, extent, 0);
          check_index(A::source_index(sc, extent), extent);
        }
      }
    }
  }
  // identity: voxel o of an extent maps onto index o of the same extent
  for (int o = 0; o < 37; ++o) {
    const float i = A::source_index(A::norm_coord(o, 37), 37);
    expect(std::fabs(i - (float)o) <= 37.0f / 1048576.0f, "identity index off by more than extent * 2^-20", i, 37, 0);
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::puts("affine_coords: every index in range");
  return 0;
}
