// Stand-alone host check of micformer_amd/csrc/conv3_wgrad_plan.h: the very work split csrc/conv3_wgradx.hip runs.  Swept over
// B in {1, 2, 3}, D in {1 .. 9, 16, 32}, H, W in {1 .. 20, 32} with W >= 4, Cin in {8, 48, 52, 96, 192, 384} and 1, 2, 4 or 12 items:
//   * the workgroup ids of an item map one-to-one onto (slab, part); every d range lies in [0, D], is non-empty and no shorter than
//     kMinRange planes unless D is; every footprint starts inside the plane;
//   * every token (b, d, h, w) is the centre of exactly one (workgroup, step, lane slot) of each slab (counted in a real array of
//     B * D * H * W entries: an index outside it is the address sanitizer's to report);
//   * every plane a step reads is a zero plane (-1 or D) or a plane of the workgroup's own sample;
//   * every workspace slab and every 16-float bias row has exactly one writer and lies inside workspace_floats().
// Then the grids of the three benched shapes are printed for tests/test_conv3_wgrad_plan_cpu.py: at least kWgTarget workgroups, or
// as many as the kMinRange rule allows.  Exits non-zero on a failure.  Compiled by the test with the host compiler under
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../micformer_amd/csrc/conv3_wgrad_plan.h"

namespace P = micf_wgrad;

static long long failures = 0;

static void expect(bool ok, const char* what, const P::Plan& p, long long a, long long b) {
  if (!ok) {
    if (failures < 20)
      std::fprintf(stderr, "FAIL %s: %lld %lld  (B %d D %d H %d W %d Cin %d items %d: tw %d nranges %d parts %d slabs %d)\n", what, a, b,
                   p.B, p.D, p.H, p.W, p.Cin, p.items, p.tw, p.nranges, p.parts, p.slabs);
    ++failures;
  }
}

// tokens covered once, planes read: depends on the shape and on nranges only (not on the slab, the item or the XCD order)
static long long check_cover(const P::Plan& p) {
  const int64_t DHW = (int64_t)p.D * p.H * p.W, T = DHW * p.B;
  std::vector<int> count((size_t)T, 0);
  long long steps = 0;
  for (int lin = 0; lin < P::grid_x(p); ++lin) {
    const P::Unit u = P::decode(p, lin);
    if (u.slab != 0) continue;
    for (int d = u.d0; d < u.d1; ++d, ++steps) {
      for (int slot = 0; slot < 64; ++slot) {
        const int64_t t = P::slot_token(p, u, d, slot);
        if (t >= 0) ++count[(size_t)t];
      }
      for (int plane = d - 1; plane <= d + 1; ++plane) {
        if (P::zero_plane(p, plane)) {
          expect(plane == -1 || plane == p.D, "zero plane", p, plane, d);
          continue;
        }
        // (slot 0 is never masked; within a plane every slot shares its sample: h < H and w < W, or the slot is masked)
        const int64_t t = P::slot_token(p, u, plane, 0);
        expect(plane >= 0 && plane < p.D && t >= u.b * DHW && t < (u.b + 1) * DHW, "plane of another sample", p, t, u.b);
      }
    }
  }
  for (int64_t t = 0; t < T; ++t)
    if (count[(size_t)t] != 1) expect(false, "token not covered once", p, t, count[(size_t)t]);
  return steps;
}

static void check_plan(const P::Plan& p, std::set<int>& covered) {
  const int L = P::grid_x(p);
  expect(p.th * p.tw == 64 && (p.tw == 16 || p.tw == 8), "footprint", p, p.th, p.tw);
  expect(p.slabs * P::kSlabChannels >= p.Cin && (p.slabs - 1) * P::kSlabChannels < p.Cin, "slabs", p, p.slabs, p.Cin);
  expect(p.parts == p.B * p.tiles_h * p.tiles_w * p.nranges, "parts", p, p.parts, p.nranges);
  expect(p.nranges >= 1 && (p.nranges == 1 || p.nranges * P::kMinRange <= p.D), "nranges", p, p.nranges, p.D);
  const int64_t before = (int64_t)p.items * p.slabs * p.B * p.tiles_h * p.tiles_w;
  // the split over d comes second: none while (item, slab, sample, footprint) already fill the target, no more than needed otherwise
  if (before >= P::kWgTarget) expect(p.nranges == 1, "needless d split", p, p.nranges, before);
  else expect(before * (p.nranges - 1) < P::kWgTarget, "d split past the target", p, p.nranges, before);
  std::vector<char> seen((size_t)L, 0);
  const int shortest = p.D < P::kMinRange ? p.D : P::kMinRange;
  for (int lin = 0; lin < L; ++lin) {
    const P::Unit u = P::decode(p, lin);
    expect(u.slab >= 0 && u.slab < p.slabs && u.part >= 0 && u.part < p.parts, "unit out of range", p, u.slab, u.part);
    if (u.slab < 0 || u.slab >= p.slabs || u.part < 0 || u.part >= p.parts) continue;
    const size_t k = (size_t)u.slab * p.parts + u.part;
    expect(!seen[k], "unit twice", p, u.slab, u.part);
    seen[k] = 1;
    expect(u.b >= 0 && u.b < p.B && u.h0 >= 0 && u.h0 < p.H && u.w0 >= 0 && u.w0 < p.W && u.h0 % p.th == 0 && u.w0 % p.tw == 0, "footprint origin", p, u.h0, u.w0);
    expect(0 <= u.d0 && u.d0 < u.d1 && u.d1 <= p.D, "d range", p, u.d0, u.d1);
    expect(u.d1 - u.d0 >= shortest, "short d range", p, u.d0, u.d1);
  }
  // workspace: slab (item, slab, part) is written by the one workgroup decode() gives that (slab, part) in item's grid row
  const int64_t total = P::workspace_floats(p);
  const int64_t nslab = (int64_t)p.items * p.slabs * p.parts;
  std::vector<char> slab_seen((size_t)nslab, 0), bias_seen((size_t)p.items * p.parts, 0);
  for (int item = 0; item < p.items; ++item)
    for (int slab = 0; slab < p.slabs; ++slab)
      for (int part = 0; part < p.parts; ++part) {
        const int64_t off = P::slab_offset(p, item, slab, part);
        expect(off >= 0 && off % P::kSlabFloats == 0 && off / P::kSlabFloats < nslab, "slab offset", p, off, nslab);
        if (off < 0 || off % P::kSlabFloats || off / P::kSlabFloats >= nslab) continue;
        expect(!slab_seen[(size_t)(off / P::kSlabFloats)], "slab written twice", p, off, 0);
        slab_seen[(size_t)(off / P::kSlabFloats)] = 1;
        expect(off + P::kSlabFloats <= total, "slab past the workspace", p, off, total);
      }
  for (int item = 0; item < p.items; ++item)
    for (int part = 0; part < p.parts; ++part) {
      const int64_t off = P::bias_offset(p, item, part) - nslab * P::kSlabFloats;
      expect(off >= 0 && off % 16 == 0 && off / 16 < (int64_t)p.items * p.parts, "bias offset", p, off, 0);
      if (off < 0 || off % 16 || off / 16 >= (int64_t)p.items * p.parts) continue;
      expect(!bias_seen[(size_t)(off / 16)], "bias row written twice", p, off, 0);
      bias_seen[(size_t)(off / 16)] = 1;
      expect(P::bias_offset(p, item, part) + 16 <= total, "bias row past the workspace", p, off, total);
    }
  if (covered.insert(p.nranges).second) check_cover(p);
}

int main() {
  const int Ds[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 32};
  const int Cins[] = {8, 48, 52, 96, 192, 384};
  const int Items[] = {1, 2, 4, 12};
  std::vector<int> ext;
  for (int i = 1; i <= 20; ++i) ext.push_back(i);
  ext.push_back(32);
  long long plans = 0, covers = 0;
  for (int B = 1; B <= 3; ++B)
    for (int D : Ds)
      for (int H : ext)
        for (int W : ext) {
          if (W < 4) continue;
          std::set<int> covered;                       // the values of nranges whose token cover was walked for this shape
          for (int Cin : Cins)
            for (int items : Items) {
              check_plan(P::make_plan(B, D, H, W, Cin, items), covered);
              ++plans;
            }
          covers += (long long)covered.size();
        }
  // the benched shapes with the item counts the flushes hand over
  struct Case { int B, D, H, W, Cin, items; };
  const Case benched[] = {{2, 32, 32, 32, 96, 2}, {2, 32, 32, 32, 96, 4}, {2, 16, 16, 16, 192, 4}, {2, 8, 8, 8, 384, 12}, {2, 8, 8, 8, 384, 4}};
  for (const Case& c : benched) {
    const P::Plan p = P::make_plan(c.B, c.D, c.H, c.W, c.Cin, c.items);
    const long long wgs = (long long)P::grid_x(p) * p.items;
    const int most = p.D / P::kMinRange > 1 ? p.D / P::kMinRange : 1;
    std::printf("benched %d %d %d %d Cin %d items %d: grid %d x %d = %lld workgroups, tw %d, %d d ranges of %d planes, workspace %lld floats\n",
                c.B, c.D, c.H, c.W, c.Cin, c.items, P::grid_x(p), p.items, wgs, p.tw, p.nranges, p.D / p.nranges, (long long)P::workspace_floats(p));
    expect(wgs >= P::kWgTarget || p.nranges == most, "benched shape under the target", p, wgs, p.nranges);
  }
  if (failures) {
    std::fprintf(stderr, "%lld failures\n", failures);
    return 1;
  }
  std::printf("%lld plans, %lld token covers: every token once, every plane in its sample, every slab one writer\n", plans, covers);
  return 0;
}
