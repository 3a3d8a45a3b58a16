// Stand-alone host check of micformer_amd/csrc/lowres_coords.h: the very clamp, gather-index, tap and weight functions and the
// prefilter steps csrc/volume_lowres.hip runs.  Every extent n in 1..70 is swept against every target 1..n and against targets out
// of range (0, negative, n + 5, which must act as 1 and n): every gather index reads a real array of n elements and must equal
// the integer rule restated here; every tap of every output reads a real array of t + 4 coefficients (an index outside either is
// the address sanitizer's to report); the fraction lies in [0, 1) and reproduces s = (o + 1/2) t / n - 1/2; the four weights are
// non-negative and sum to 1 within 4 * 2^-23.  Then the prefilter steps run on a line of every length 1..70 the way the kernels
// chain them, and the coefficients must interpolate the line: (c[k - 1] + 4 c[k] + c[k + 1]) / 6 = s[k] with the extension entries
// standing beyond the ends, and a constant line must give itself.  Exits non-zero on a failure.  Compiled by the test with the
// host compiler under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../micformer_amd/csrc/lowres_coords.h"

namespace L = micf_lowres;

static int failures = 0;

static void expect(bool ok, const char* what, double a, double b) {
  if (!ok) {
    if (failures < 20) std::fprintf(stderr, "FAIL %s: %g %g\n", what, a, b);
    ++failures;
  }
}

static void sweep(int n, int target, long long* gathers, long long* taps) {
  const int t = L::clamp_target(target, n);
  expect(t >= 1 && t <= n && (target < 1 ? t == 1 : (target > n ? t == n : t == target)), "clamp_target", target, n);
  std::vector<int> data(n);
  for (int i = 0; i < n; ++i) data[i] = 100 + i;
  for (int o = 0; o < t; ++o) {
    const int g = L::gather_index(o, n, target);
    long long want = ((2LL * o + 1) * n) / (2LL * t);
    if (want > n - 1) want = n - 1;
    expect(g >= 0 && g < n, "gather index out of [0, n)", o, n);
    if (g >= 0 && g < n) expect(data[g] == 100 + (int)want, "gather index is not the integer rule", o, n);
    ++*gathers;
  }
  std::vector<float> coef(t + 2 * L::kExt);
  for (int i = 0; i < t + 2 * L::kExt; ++i) coef[i] = 1.0f;
  for (int o = 0; o < n; ++o) {
    float f = -1.0f, w[4];
    const int fl = L::tap_floor(o, n, target, &f);
    expect(fl >= -1 && fl <= t - 1, "tap floor out of [-1, t - 1]", o, fl);
    expect(f >= 0.0f && f < 1.0f, "fraction out of [0, 1)", o, f);
    const double s = (o + 0.5) * t / n - 0.5;
    expect(std::fabs((double)fl + (double)f - s) <= 1e-6, "floor + fraction is not s", fl + f, s);
    L::cubic_weights(f, w);
    float sum = 0.0f, through = 0.0f;
    for (int j = 0; j < 4; ++j) {
      expect(w[j] >= 0.0f && w[j] <= 4.0f / 6.0f + 1e-6f, "weight out of range", o, w[j]);
      sum += w[j];
      through += w[j] * coef[fl - 1 + j + L::kExt];         // a real array of t + 4 coefficients
      ++*taps;
    }
    expect(std::fabs(sum - 1.0f) <= 4.0f / 8388608.0f && std::fabs(through - 1.0f) <= 4.0f / 8388608.0f,
           "weights do not sum to 1 within 4 * 2^-23", o, sum);
  }
  float f0;
  expect(L::tap_floor(-3, n, target, &f0) == L::tap_floor(0, n, target, &f0), "an output below 0 is not clamped", n, target);
  expect(L::tap_floor(n + 9, n, target, &f0) == L::tap_floor(n - 1, n, target, &f0), "an output above n - 1 is not clamped", n, target);
  expect(L::gather_index(-2, n, target) == L::gather_index(0, n, target) && L::gather_index(t + 7, n, target) == L::gather_index(t - 1, n, target),
         "a low-resolution position out of range is not clamped", n, target);
}

// the kernels' chain of the prefilter steps on s[0 .. t) -> c[-2 .. t + 1] (stored at + 2)
static std::vector<float> prefilter(const std::vector<float>& s) {
  const int t = (int)s.size();
  std::vector<float> c(t + 2 * L::kExt), p(t);
  p[0] = L::causal_first(s[0]);
  for (int k = 1; k < t; ++k) p[k] = L::causal_next(p[k - 1], s[k]);
  c[L::kExt + t - 1] = L::anticausal_last(p[t - 1], s[t - 1]);
  for (int k = t - 2; k >= 0; --k) c[L::kExt + k] = L::anticausal_next(c[L::kExt + k + 1], p[k]);
  c[1] = L::extend1(c[L::kExt], s[0]);
  c[0] = L::extend2(c[L::kExt], s[0]);
  c[L::kExt + t] = L::extend1(c[L::kExt + t - 1], s[t - 1]);
  c[L::kExt + t + 1] = L::extend2(c[L::kExt + t - 1], s[t - 1]);
  return c;
}

int main() {
  long long gathers = 0, taps = 0, lines = 0;
  for (int n = 1; n <= 70; ++n) {
    for (int t = 1; t <= n; ++t) sweep(n, t, &gathers, &taps);
    for (int t : {0, -1, -1000000, n + 5}) sweep(n, t, &gathers, &taps);
  }
  float f;
  expect(L::clamp_target(3, 0) == 1 && L::gather_index(0, 0, 0) == 0 && L::tap_floor(0, -4, 2, &f) == 0, "a non-positive extent is not treated as 1", 0, 0);
  {                                                              // the largest extent: no overflow
    const int n = 2048;
    for (int t : {1, 2, 1024, 1365, 2047, 2048}) sweep(n, t, &gathers, &taps);
    expect(L::tap_floor(n - 1, n, n, &f) == n - 1 && f == 0.0f && L::tap_floor(0, n, 1, &f) == -1, "taps at 2048", f, 0);
  }
  unsigned state = 12345u;
  for (int t = 1; t <= 70; ++t) {
    std::vector<float> s(t), flat(t, 0.75f);
    for (int k = 0; k < t; ++k) {
      state = state * 1664525u + 1013904223u;
      s[k] = (float)(state >> 8) / 16777216.0f * 2.0f - 1.0f;
    }
    const std::vector<float> c = prefilter(s), cf = prefilter(flat);
    for (int k = 0; k < t; ++k) {
      const float back = (c[L::kExt + k - 1] + 4.0f * c[L::kExt + k] + c[L::kExt + k + 1]) / 6.0f;
      expect(std::fabs(back - s[k]) <= 2e-6f, "coefficients do not interpolate the line", t, k);
    }
    // the extension: one step beyond either end the interpolation condition holds with the edge value
    expect(std::fabs((c[0] + 4.0f * c[1] + c[2]) / 6.0f - s[0]) <= 2e-6f, "extension below", t, 0);
    expect(std::fabs((c[t + 1] + 4.0f * c[t + 2] + c[t + 3]) / 6.0f - s[t - 1]) <= 2e-6f, "extension above", t, 0);
    for (int k = 0; k < t + 2 * L::kExt; ++k) expect(std::fabs(cf[k] - 0.75f) <= 2e-7f, "a constant line is not its own coefficients", t, k);
    ++lines;
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("lowres_coords: every index in range over %lld gather indices and %lld taps, %lld lines\n", gathers, taps, lines);
  return 0;
}
