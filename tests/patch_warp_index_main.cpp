// Stand-alone host check of the coordinate code csrc/volume_patch_warp.hip runs: micformer_amd/csrc/patch_warp_coords.h (origin add,
// label tap, field columns) on top of affine_coords.h (map, clamp, taps) and elastic_coords.h (control cells, weights).  For NaN,
// +-inf, +-1e30, +-FLT_MAX and ordinary coordinates, origins at both bounds of patches_coords.h, P from 1 to 2048 and scans from 1
// to 2048 voxels it forms the index, the two image taps in both padding modes and the label tap, READS a real array of the scan's
// length at every address (an address outside it is the address sanitizer's to report, a float -> int conversion out of range the
// undefined-behaviour sanitizer's) and prints one line per result; then it interpolates real displacement fields, a NaN control
// point among them, through field_columns with the run's cell cache as the kernel keeps it.  tests/test_patch_warp_cpu.py compiles
// this with the host compiler under -fsanitize=address,undefined and compares every line with tests/patch_warp_ref.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../micformer_amd/csrc/patch_warp_coords.h"
#include "../micformer_amd/csrc/patches_coords.h"

namespace W = micf_patch_warp;
namespace E = micf_elastic;
namespace A = micf_affine;
namespace P = micf_patches;

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

template <int kTaps>
static E::AxisTaps<kTaps> axis_taps(const E::Cell& c, int g) {
  if constexpr (kTaps == 4) return E::cubic_taps(c, g);
  else return E::linear_taps(c, g);
}

// one row of Pw voxels through the cell cache, as patch_warp_kernel walks it; prints u of every voxel
template <int kTaps>
static int field_row(const std::vector<float>& f, int gd, int gh, int gw, int z, int y, int Pd, int Ph, int Pw, int per) {
  const E::AxisTaps<kTaps> tz = axis_taps<kTaps>(E::control_cell(z, Pd, gd), gd), ty = axis_taps<kTaps>(E::control_cell(y, Ph, gh), gh);
  int recomputed = 0;
  for (int x0 = 0; x0 < Pw; x0 += per) {
    float col[3][kTaps];
    int cell = -1;
    for (int x = x0; x < x0 + per && x < Pw; ++x) {
      const E::Cell kx = E::control_cell(x, Pw, gw);
      const E::AxisTaps<kTaps> tx = axis_taps<kTaps>(kx, gw);
      if (kx.k != cell) {
        W::field_columns<kTaps>(f.data(), tz, ty, tx, col);
        cell = kx.k;
        ++recomputed;
      }
      float u[3];
      for (int c = 0; c < 3; ++c) {
        u[c] = W::displacement<kTaps>(col, c, tx);
        // the loader's own order of the same sum (elastic_coords.h): equal up to rounding, NaN where this is NaN
        const float v = E::interpolate<kTaps>(f.data() + (size_t)c * gd * gh * gw, tz, ty, tx);
        if ((u[c] != u[c]) != (v != v)) return -1;
        if (u[c] == u[c] && !(u[c] - v <= 1e-6f && v - u[c] <= 1e-6f)) return -1;
      }
      std::printf("field %d %d %d %d %d %d %d %d %d %d %u %u %u\n", kTaps, gd, gh, gw, Pd, Ph, Pw, z, y, x, bits(u[0]), bits(u[1]),
                  bits(u[2]));
    }
  }
  return recomputed;
}

int main() {
  const uint32_t ss[] = {0x7fc00000u, 0x7f800000u, 0xff800000u, 0x7149f2cau /* 1e30 */, 0xf149f2cau, 0x7f7fffffu, 0xff7fffffu,
                         0x00000000u, 0x80000000u, 0x3f800000u, 0xbf800000u, 0x3f7fffffu, 0xbf7fffffu, 0x3e99999au /* 0.3 */,
                         0xbf333333u /* -0.7 */, 0x40000000u /* 2 */, 0xc0400000u /* -3 */, 0x3f000000u, 0x00000001u};
  const int extents[] = {1, 2, 3, 5, 16, 29, 127, 128, 2047, 2048};
  for (int L : extents) {
    std::vector<int16_t> scan((size_t)L);
    for (int i = 0; i < L; ++i) scan[(size_t)i] = (int16_t)(i % 251);
    for (int Pe : extents) {
      const int origins[] = {P::origin_lb(L, Pe), P::origin_ub(L, Pe)};
      for (int o : origins)
        for (uint32_t sb : ss) {
          const float s = from_bits(sb);
          const int fin = A::finite(s) ? 1 : 0;
          // (the kernel forms an index from a finite s only; a non-finite one must still be harmless here)
          const float i = W::scan_index(o, s, Pe);
          bool in;
          const int k = W::label_tap(i, L, in);
          const A::LinearTaps tz = A::linear_taps(i, L, false), tb = A::linear_taps(i, L, true);
          const int addr[] = {k, tz.i0, tz.i1, tb.i0, tb.i1};
          long sum = 0;
          for (int a : addr) {
            if (a < 0 || a >= L) return 2;
            sum += scan[(size_t)a];                              // a real read: the address sanitizer's to judge
          }
          if (sum < 0) return 3;
          if (!(tz.w1 >= 0.0f && tz.w1 < 1.0f) || !(tb.w1 >= 0.0f && tb.w1 < 1.0f) || !tb.in0 || !tb.in1) return 4;
          std::printf("index %u %d %d %d %d %u %d %d %d %d %d %d %u %d %d %u\n", sb, o, Pe, L, fin, bits(i), k, in ? 1 : 0, tz.i0, tz.i1,
                      tz.in0 ? 1 : 0, tz.in1 ? 1 : 0, bits(tz.w1), tb.i0, tb.i1, bits(tb.w1));
        }
    }
  }
  // a whole row of every P from 1 to 2048 through the identity: i = o + x up to the bound, every address inside
  for (int Pe = 1; Pe <= 2048; ++Pe) {
    const int L = 37, o = Pe % 2 ? P::origin_lb(L, Pe) : P::origin_ub(L, Pe);
    double worst = 0.0;
    for (int x = 0; x < Pe; ++x) {
      const float i = W::scan_index(o, A::norm_coord(x, Pe), Pe);
      const double e = (double)i - (double)(o + x);
      worst = (e < 0 ? -e : e) > worst ? (e < 0 ? -e : e) : worst;
      bool in;
      const int k = W::label_tap(i, L, in);
      if (k < 0 || k >= L) return 5;
    }
    if ((Pe & (Pe - 1)) == 0 && worst != 0.0) return 6;           // a power of two: exact
    std::printf("row %d %d %.9g\n", Pe, o, worst);
  }
  // the field: a coarse grid, a dense one (g == P) and the smallest, with a NaN control point in the first
  {
    struct Case { int gd, gh, gw, Pd, Ph, Pw, per, nan_at; };
    const Case cases[] = {{5, 4, 6, 9, 11, 32, 8, 37}, {2, 2, 2, 3, 1, 13, 1, -1}, {3, 5, 12, 3, 5, 12, 4, -1}, {7, 7, 7, 4, 2, 2048, 8, -1}};
    for (const Case& c : cases) {
      std::vector<float> f((size_t)3 * c.gd * c.gh * c.gw);
      for (size_t i = 0; i < f.size(); ++i) f[i] = (float)((int)((i * 2654435761u) >> 20 & 1023) - 512) / 4096.0f;   // in +-0.125
      if (c.nan_at >= 0) f[(size_t)c.nan_at] = from_bits(0x7fc00000u);
      for (int z = 0; z < c.Pd; ++z)
        for (int y = 0; y < c.Ph; ++y) {
          const int r2 = field_row<2>(f, c.gd, c.gh, c.gw, z, y, c.Pd, c.Ph, c.Pw, c.per);
          const int r4 = field_row<4>(f, c.gd, c.gh, c.gw, z, y, c.Pd, c.Ph, c.Pw, c.per);
          if (r2 < 0 || r4 < 0) return 7;
          std::printf("recomputed %d %d %d %d %d\n", c.gw, c.Pw, c.per, r2, r4);
        }
    }
  }
  std::printf("patch_warp_coords: done\n");
  return 0;
}
