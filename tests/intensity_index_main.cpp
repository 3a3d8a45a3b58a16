// Stand-alone host check of micformer_amd/csrc/intensity_coords.h: the very reflect-index, radius, weight and random-number
// functions csrc/volume_intensity.hip runs.  The reflect index is swept over extents 1..40 x offsets -16..56 against the mirrored
// sequence built step by step, and every index is used to read a real array of that extent (an index outside it is the address
// sanitizer's to report).  The weights are swept over sigma in [0.1, 2.0] and over values outside it (0, negative, 5, inf, NaN):
// the radius must be int(4 sigma + 0.5) of the clamped sigma and at most 8, the weights symmetric, zero beyond the radius and of
// sum 1 within 4 * 2^-23.  Then 4 096 hash words with their two uniforms (as float32 bit patterns) and the bits of the normal draw
// are printed for tests/test_intensity_cpu.py, which compares words and uniforms with the numpy referee bit for bit.  Exits non-zero
// on a failure.  Compiled by the test with the host compiler under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../micformer_amd/csrc/intensity_coords.h"

namespace I = micf_intensity;

static int failures = 0;

static void expect(bool ok, const char* what, double a, double b) {
  if (!ok) {
    if (failures < 20) std::fprintf(stderr, "FAIL %s: %g %g\n", what, a, b);
    ++failures;
  }
}

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  long long indices = 0;
  for (int n = 1; n <= 40; ++n) {
    std::vector<int> data(n);
    for (int i = 0; i < n; ++i) data[i] = 100 + i;
    // the mirrored sequence: walk outwards from 0, bouncing at both ends with the edge element repeated
    for (int off = -16; off <= 56; ++off) {
      int want = 0, dir = 1;                                     // i = -1 mirrors 0, -2 mirrors 1, ...: the walk of -i - 1 steps
      for (int step = 0; step < (off < 0 ? -off - 1 : off); ++step) {
        if (want + dir < 0 || want + dir >= n) dir = -dir; else want += dir;
      }
      const int got = I::reflect_index(off, n);
      expect(got >= 0 && got < n, "reflect index out of [0, n)", off, n);
      if (got >= 0 && got < n) expect(data[got] == 100 + want, "reflect index is not the mirrored element", off, n);
      ++indices;
    }
  }
  expect(I::reflect_index(5, 0) == 0 && I::reflect_index(-3, -2) == 0, "a non-positive extent is not treated as 1", 0, 0);

  long long sigmas = 0;
  float w[I::kTaps];
  for (int s = 0; s <= 1900; ++s) {
    const float sigma = 0.1f + 0.001f * (float)s;
    const float c = I::clamp_sigma(sigma);
    expect(c >= I::kSigmaMin && c <= I::kSigmaMax, "clamped sigma out of range", sigma, c);
    const int r = I::blur_weights(c, w);
    expect(r == (int)(4.0 * (double)c + 0.5) && r >= 0 && r <= I::kMaxRadius, "radius", sigma, r);
    expect(r == I::blur_radius(c), "blur_weights and blur_radius disagree", sigma, r);
    float sum = 0.0f;
    for (int j = 0; j < I::kTaps; ++j) {
      const int k = j - I::kMaxRadius;
      expect(w[j] == w[I::kTaps - 1 - j], "weights not symmetric", sigma, j);
      expect((k < -r || k > r) ? w[j] == 0.0f : (w[j] > 0.0f && w[j] <= 1.0f), "weight out of range", sigma, j);
      sum += w[j];
    }
    expect(std::fabs(sum - 1.0f) <= 4.0f / 8388608.0f, "weights do not sum to 1 within 4 * 2^-23", sigma, sum);
    ++sigmas;
  }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  expect(I::clamp_sigma(0.0f) == 0.0f && I::clamp_sigma(-1.0f) == 0.0f && I::clamp_sigma(-inf) == 0.0f, "sigma <= 0 is not off", 0, 0);
  expect(I::clamp_sigma(5.0f) == 2.0f && I::clamp_sigma(inf) == 2.0f && I::clamp_sigma(1e-3f) == 0.1f, "sigma not clamped", 0, 0);
  expect(std::isnan(I::clamp_sigma(nan)) && I::blur_radius(nan) == 0 && I::blur_radius(0.0f) == 0, "NaN sigma", 0, 0);
  expect(I::blur_weights(nan, w) == 0 && std::isnan(w[I::kMaxRadius]) && w[0] == 0.0f, "NaN sigma's weights", 0, 0);
  expect(I::blur_weights(0.0f, w) == 0 && w[I::kMaxRadius] == 1.0f, "sigma 0 is not the identity", 0, 0);
  expect(I::blur_radius(0.125f) == 1 && I::blur_radius(std::nextafterf(0.125f, 0.0f)) == 0, "radius at the rounding boundary", 0, 0);
  expect(I::blur_radius(2.0f) == 8 && I::blur_radius(100.0f) == 8, "radius above the clamp", 0, 0);

  const uint64_t key = I::noise_key((int64_t)0x123456789ABCDEF0ll, 1);
  for (int i = 0; i < 4096; ++i) {
    const uint64_t h = I::noise_word(key, (uint64_t)i);
    const float z = I::normal(h);
    expect(std::isfinite(z) && std::fabs(z) < 6.0f, "normal draw", i, z);
    std::printf("word %016llx %08x %08x %08x\n", (unsigned long long)h, bits(I::uniform_hi(h)), bits(I::uniform_lo(h)), bits(z));
  }
  // the ends of u1: the last k rounds to u = 1, and normal() stays finite and non-zero there
  const uint64_t top = 0xFFFFFFull << 40;
  expect(I::uniform_hi(top) == 1.0f && I::log_uniform_hi(top) < 0.0f && std::isfinite(I::log_uniform_hi(0)), "ends of u1", 0, 0);
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("intensity_coords: every index in range over %lld indices, %lld sigmas\n", indices, sigmas);
  return 0;
}
