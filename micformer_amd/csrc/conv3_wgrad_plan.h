// conv3_wgrad_plan.h -- the work split of the offset convolution's weight gradient (conv3_wgradx.hip), written once:
// footprints and d ranges, the workgroup -> (slab, sample, footprint, d range) map with its XCD-contiguous order, the token a
// lane slot of a plane step stands for, and the workspace size and slab offsets.  In the style of intensity_coords.h /
// elastic_coords.h: every function is __host__ __device__ and plain C++, so a host program walks the very map the kernels run
// (tests/conv3_wgrad_plan_main.cpp does, under the address and undefined-behaviour sanitizers).
//
// A workgroup owns one channel slab (48 input channels x 27 taps) of one item, an (h, w) footprint of th x tw = 64 tokens of one
// sample and a contiguous range [d0, d1) of its d planes.  It marches the range one plane per step with the three halo planes
// d - 1, d, d + 1 in an LDS ring, so a step fetches ONE new plane of (th + 2) x (tw + 2) voxel rows; planes -1 and D are zeros
// and a range never crosses a sample.  A range that starts inside a sample primes two planes, so no range is shorter than
// kMinRange planes unless D is: the split over d is taken only after (item, slab, sample, footprint) and only up to kWgTarget
// workgroups (two per CU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MICF_WGP_HD __host__ __device__ inline
#else
#define MICF_WGP_HD inline
#endif

namespace micf_wgrad {

constexpr int kSlabChannels = 48;                        // channels per slab (3 channel tiles of 16)
constexpr int kPairs = 27 * (kSlabChannels / 16);        // 81 (tap, channel tile) pairs per slab
constexpr int kTilesPerWave = (kPairs + 3) / 4;          // 21 accumulator tiles in each of the 4 waves
constexpr int kSlabFloats = 4 * kTilesPerWave * 256;     // partial slab of one workgroup in the workspace (84 chunks of 16 x 16)
constexpr int kMaxItems = 12;                            // layers of one shape per launch
constexpr int kWgTarget = 512;                           // two workgroups on each of the 256 CUs
constexpr int kMinRange = 4;                             // shortest d range (planes) the split over d produces

struct Plan {
  int B, D, H, W, Cin, items;
  int tw, th, tiles_h, tiles_w;     // footprint extents (th * tw = 64) and footprints per plane
  int slabs, nranges;               // channel slabs; d ranges per (sample, footprint)
  int parts;                        // partial slabs per (item, slab) = B * tiles_h * tiles_w * nranges
  int xcd_order;                    // 1: consecutive units of the map run on one XCD
};

struct Unit { int slab, part, b, h0, w0, d0, d1; };

// W >= 4, Cin >= 1, 1 <= items <= kMaxItems (the launcher checks).  W < 12 takes 8-wide footprints (W = 4: half of each masked).
MICF_WGP_HD Plan make_plan(int B, int D, int H, int W, int Cin, int items) {
  Plan p;
  p.B = B; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.items = items;
  p.tw = W >= 12 ? 16 : 8;
  p.th = 64 / p.tw;
  p.tiles_h = (H + p.th - 1) / p.th;
  p.tiles_w = (W + p.tw - 1) / p.tw;
  p.slabs = (Cin + kSlabChannels - 1) / kSlabChannels;
  const int64_t units = (int64_t)items * p.slabs * B * p.tiles_h * p.tiles_w;    // workgroups before any split over d
  int64_t want = (kWgTarget + units - 1) / units;
  const int most = D / kMinRange > 1 ? D / kMinRange : 1;
  p.nranges = (int)(want < most ? want : most);
  p.parts = B * p.tiles_h * p.tiles_w * p.nranges;
  p.xcd_order = ((int64_t)p.slabs * p.parts) % 8 == 0 ? 1 : 0;
  return p;
}

MICF_WGP_HD int range_begin(const Plan& p, int r) { return (int)((int64_t)r * p.D / p.nranges); }   // balanced: every range >= D / nranges

// workgroups of one item (gridDim.x); the items are gridDim.y
MICF_WGP_HD int grid_x(const Plan& p) { return p.slabs * p.parts; }

// Workgroup `lin` of an item.  The hardware deals workgroups to the 8 XCDs round-robin by linear id; with xcd_order the units one
// XCD receives are consecutive in the map (slab fastest: the slabs of a part read the same dy; then the d ranges and the
// footprints of a sample, whose halos overlap), so what neighbours share hits that XCD's L2.
MICF_WGP_HD Unit decode(const Plan& p, int lin) {
  const int L = p.slabs * p.parts;
  const int logical = p.xcd_order ? (lin % 8) * (L / 8) + lin / 8 : lin;
  Unit u;
  u.slab = logical % p.slabs;
  u.part = logical / p.slabs;
  int q = u.part;
  const int r = q % p.nranges; q /= p.nranges;
  u.w0 = (q % p.tiles_w) * p.tw; q /= p.tiles_w;
  u.h0 = (q % p.tiles_h) * p.th;
  u.b = q / p.tiles_h;
  u.d0 = range_begin(p, r);
  u.d1 = range_begin(p, r + 1);
  return u;
}

// A step at plane d reads planes d - 1, d, d + 1 of the unit's own sample; these two are zeros, never memory.
MICF_WGP_HD bool zero_plane(const Plan& p, int d) { return d < 0 || d >= p.D; }

// token (channels-last row) at the centre of lane slot `slot` (= lh * tw + lw, 0 .. 63) of the step at plane d, or -1 (masked)
MICF_WGP_HD int64_t slot_token(const Plan& p, const Unit& u, int d, int slot) {
  const int h = u.h0 + slot / p.tw, w = u.w0 + slot % p.tw;
  if (h >= p.H || w >= p.W) return -1;
  return (((int64_t)u.b * p.D + d) * p.H + h) * p.W + w;
}

// workspace: [item][slab][part][kSlabFloats] partial slabs, then [item][part][16] column sums of dy (written by slab 0)
MICF_WGP_HD int64_t slab_offset(const Plan& p, int item, int slab, int part) {
  return (((int64_t)item * p.slabs + slab) * p.parts + part) * kSlabFloats;
}
MICF_WGP_HD int64_t bias_offset(const Plan& p, int item, int part) {
  return (int64_t)p.items * p.slabs * p.parts * kSlabFloats + ((int64_t)item * p.parts + part) * 16;
}
MICF_WGP_HD int64_t workspace_floats(const Plan& p) {
  return (int64_t)p.items * p.parts * ((int64_t)p.slabs * kSlabFloats + 16);
}

}  // namespace micf_wgrad
