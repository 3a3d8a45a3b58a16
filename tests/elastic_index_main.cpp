// Stand-alone host check of micformer_amd/csrc/elastic_coords.h: the very control-cell, fraction, weight and address functions
// csrc/volume_elastic.hip runs, swept over out in {1, 2, 3, 24, 511, 512} x g in {2, 3, 7, 511, 512} x every output voxel o (and
// o = -1, o = out, which the functions clamp) in both interpolation modes.  Every tap address must lie in [0, g), every weight in
// [0, 1], the weights of an axis must sum to 1 within 4 * 2^-23, t must lie in [0, 1), the cell must be floor(o (g - 1) / (out - 1))
// and the last voxel must land on the last control point with weight 1; interpolate() is run over a real g^3 array at the corners
// of the sweep, so an address outside it is the address sanitizer's to report.  Exits non-zero on a failure.
// tests/test_elastic_cpu.py compiles this with the host compiler under -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../micformer_amd/csrc/elastic_coords.h"

namespace E = micf_elastic;

static int failures = 0;

static void expect(bool ok, const char* what, int o, int out, int g, int cubic) {
  if (!ok) {
    if (failures < 20) std::fprintf(stderr, "FAIL %s: o %d out %d g %d cubic %d\n", what, o, out, g, cubic);
    ++failures;
  }
}

template <int kTaps>
static void check_taps(const E::AxisTaps<kTaps>& a, const E::Cell& c, int o, int out, int g, int cubic) {
  float sum = 0.0f;
  for (int j = -2; j < kTaps + 2; ++j) {                       // (beyond the taps too: address() clamps whatever j)
    const int addr = a.address(j);
    expect(addr >= 0 && addr < g, "tap address out of [0, g)", o, out, g, cubic);
  }
  for (int j = 0; j < kTaps; ++j) {
    expect(a.w[j] >= 0.0f && a.w[j] <= 1.0f, "weight out of [0, 1]", o, out, g, cubic);
    expect(a.weight(j) == a.w[j], "weight(j) is not w[j]", o, out, g, cubic);
    sum += a.w[j];
  }
  expect(std::fabs(sum - 1.0f) <= 4.0f / 8388608.0f, "weights do not sum to 1 within 4 * 2^-23", o, out, g, cubic);
  const int want = c.k - (cubic ? 1 : 0);
  expect(a.address(0) == (want < 0 ? 0 : want), "first tap is not the cell's", o, out, g, cubic);
}

int main() {
  const int outs[] = {1, 2, 3, 24, 511, 512}, grids[] = {2, 3, 7, 511, 512};
  long long cells = 0;
  for (int out : outs) {
    for (int g : grids) {
      for (int o = -1; o <= out; ++o) {
        const E::Cell c = E::control_cell(o, out, g);
        const int oc = o < 0 ? 0 : (o < out ? o : out - 1);
        expect(c.t >= 0.0f && c.t < 1.0f, "t out of [0, 1)", o, out, g, 0);
        expect(c.k >= 0 && c.k <= g - 1, "cell out of [0, g - 1]", o, out, g, 0);
        if (out > 1) {
          expect(c.k == (int)(((long long)oc * (g - 1)) / (out - 1)), "cell is not floor(o (g - 1) / (out - 1))", o, out, g, 0);
          const double p = (double)oc * (g - 1) / (out - 1);
          expect(std::fabs((double)c.k + (double)c.t - p) <= 1.0 / 16777216.0, "k + t is not the control position", o, out, g, 0);
        } else {
          expect(c.k == 0 && c.t == 0.0f, "out == 1 is not p = 0", o, out, g, 0);
        }
        if (oc == out - 1 && out > 1) expect(c.k == g - 1 && c.t == 0.0f, "last voxel not on the last control point", o, out, g, 0);
        const E::AxisTaps<2> lin = E::linear_taps(c, g);
        const E::AxisTaps<4> cub = E::cubic_taps(c, g);
        check_taps(lin, c, o, out, g, 0);
        check_taps(cub, c, o, out, g, 1);
        if (oc == out - 1 && out > 1) expect(lin.w[0] == 1.0f && lin.address(0) == g - 1, "last voxel's linear weight", o, out, g, 0);
        ++cells;
      }
    }
  }
  // interpolate() over real arrays: every address it forms is dereferenced
  for (int g : {2, 3, 7}) {
    std::vector<float> f((size_t)g * g * g);
    for (size_t i = 0; i < f.size(); ++i) f[i] = 0.25f;
    for (int out : {1, 2, 3, 24}) {
      for (int o = 0; o < out; ++o) {
        const E::Cell c = E::control_cell(o, out, g), c0 = E::control_cell(0, out, g), c1 = E::control_cell(out - 1, out, g);
        const float a = E::interpolate<2>(f.data(), E::linear_taps(c, g), E::linear_taps(c0, g), E::linear_taps(c1, g));
        const float b = E::interpolate<4>(f.data(), E::cubic_taps(c1, g), E::cubic_taps(c, g), E::cubic_taps(c0, g));
        expect(std::fabs(a - 0.25f) <= 1e-6f && std::fabs(b - 0.25f) <= 1e-6f, "a constant field is not reproduced", o, out, g, 2);
      }
    }
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("elastic_coords: every tap in range over %lld cells\n", cells);
  return 0;
}
