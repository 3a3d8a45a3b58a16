// surface_distance.hip -- on-device surface distances in physical units (include/micformer_surface.h): percentile Hausdorff
// distance, average (symmetric) surface distance and surface Dice on a grid with a voxel spacing per sample.  Rules: DESIGN.md
// "Surface distances in millimetres".  Deterministic: the nearest target is found on integer offsets and float64 candidate
// values, every distance is re-evaluated from its integer offsets (dz, dy, dx) by one formula, sums are 128-bit fixed-point
// integers, counts and histograms are integers, and order statistics come from a radix select over the float64 bit pattern.
//
// Launch plan of micf_surface_distance (batched over (b, c, direction), no host round trip, the same launches for any data):
//   0 remap      label-valued int16 / int32 volumes -> uint8 class maps (the two VALUES forms only)
//   1-4          classify, box, edges, edt_w of surface_common.h, unchanged: the edge sets are those of micf_hausdorff_distance,
//                and the field holds |dx|^2 along W
//   5 edt_mid    lower envelope along the shorter of D / H on float64 values (s_m dm)^2 + (s_x dx)^2; the stack in LDS holds
//                (|dx| << 10 | position); the field then packs |dx| | |dm| << 10
//   6 search     at every source edge voxel: outward search along the last axis, candidates valued by the full formula, exit
//                once (s_l j)^2 >= best; the winning offset j is stored in bits 19..29 of the voxel's own field word (readers
//                of the low bits mask them off), so a distance is two loads and no distance is ever stored
//   7 scan x 7   pass 0: fixed-point sum of d, count of d <= tau, max; passes 0..5: one 11-bit digit of the radix select per
//                (slot, percentile), each followed by `choose` (one workgroup per query picks the digit); pass 6: the rank's
//                successor (count of keys <= the selected key, smallest key above it)
//   8 finish     sqrt, numpy's lerp, the divisions, nan / inf rules, float32 stores
// Direction 0 is pred -> gt (distance to the gt edges), direction 1 gt -> pred.
#include "../../include/micformer_surface.h"
#include "surface_common.h"

#include <cmath>

namespace {

constexpr int kMaxBatch = MICF_SURFACE_MAX_BATCH;
constexpr int kMaxPct = MICF_SURFACE_MAX_PERCENTILES;
constexpr int kDigit = 11, kBins = 1 << kDigit, kPasses = 6;      // 9 + 5 x 11 bits = the 64 bits of a key
constexpr int kOffMask = (1 << 19) - 1;                          // |dx| (10 bits) | |dm| << 10 (9 bits)
constexpr int kJShift = 19, kJBias = 1024, kJMask = 2047;        // the winning last-axis offset, biased, in bits 19..29

struct Samples {                     // per sample, by value in the kernel arguments (2 KiB)
  double s[kMaxBatch][3];            // spacing z, y, x
  double fix[kMaxBatch];             // 2^k: d * fix < 2^31, the integer part of the fixed-point sum's high word
};
struct Query {
  double pct[kMaxPct];
  double tau[32];                    // per scored class (index c - first)
  int npct, has_tau;
};
struct Lut {
  int32_t v[31];
  int n;
};

struct Layout {
  int64_t lab_p, lab_g;              // uint8 [B][V]: class maps of the two VALUES forms
  int64_t pm, gm, pe, ge;            // uint32 class-bit masks [B][V]: membership pred / gt, edges pred / gt
  int64_t zero_begin;
  int64_t counts;                    // u64 [B][K][3]
  int64_t ecount;                    // u64 [B][K][2]: pred edges, gt edges
  int64_t proj;                      // u32 [B][D + H + W]
  int64_t acc;                       // u64 [B][K][2][4]: sum low, sum high, count of d <= tau, largest key
  int64_t sel;                       // u64 [B][K][2][kMaxPct][4]: key prefix, remaining rank, count of keys <= the selected key
  int64_t hist;                      // u32 [B][K][2][kMaxPct][kBins]
  int64_t zero_end;
  int64_t above;                     // u64 [B][K][2][kMaxPct]: the smallest key above the selected one (starts at all ones)
  int64_t above_end;
  int64_t boxes;                     // int [B][K][6]
  int64_t field;                     // int [B][K][2][V]
  int64_t total;
};

Layout layout(int B, int K, int D, int H, int W) {
  Layout L;
  const int64_t V = (int64_t)D * H * W, Q = (int64_t)B * K * 2 * kMaxPct;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o = align256(o + bytes); return r; };
  L.lab_p = take(B * V);
  L.lab_g = take(B * V);
  L.pm = take(4 * B * V);
  L.gm = take(4 * B * V);
  L.pe = take(4 * B * V);
  L.ge = take(4 * B * V);
  L.zero_begin = o;
  L.counts = take(8 * (int64_t)B * K * 3);
  L.ecount = take(8 * (int64_t)B * K * 2);
  L.proj = take(4 * (int64_t)B * (D + H + W));
  L.acc = take(8 * (int64_t)B * K * 2 * 4);
  L.sel = take(8 * Q * 4);
  L.hist = take(4 * Q * kBins);
  L.zero_end = o;
  L.above = take(8 * Q);
  L.above_end = o;
  L.boxes = take(4 * (int64_t)B * K * 6);
  L.field = take(4 * (int64_t)B * K * 2 * V);
  L.total = o;
  return L;
}

// ---- float64 arithmetic in the prescribed order: never contracted into an fma ----------------------------------------------
__device__ __forceinline__ double wsq(double s, int d) {
#pragma clang fp contract(off)
  const double t = s * (double)d;
  return t * t;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

struct Geo {
  double sz, sy, sx;
  int mid_is_h;
};
// ((s_z dz)^2 + (s_y dy)^2) + (s_x dx)^2 of the packed in-plane offsets `e` and the last-axis offset dl
__device__ __forceinline__ double dist2(const Geo& g, int dl, int e) {
  const int dx = e & 1023, dm = (e >> 10) & 511;
  const int dz = g.mid_is_h ? dl : dm, dy = g.mid_is_h ? dm : dl;
  return add_rn(add_rn(wsq(g.sz, dz), wsq(g.sy, dy)), wsq(g.sx, dx));
}

// ---- 0. label values -> class map ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void sd_remap_kernel(const T* pred, const T* gt, int64_t n, Lut lut, uint8_t* lp,
                                                            uint8_t* lg) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const int a = (int)pred[i], b = (int)gt[i];
    int ka = 0, kb = 0;
    for (int j = 0; j < lut.n; ++j) {
      ka = a == lut.v[j] ? j + 1 : ka;
      kb = b == lut.v[j] ? j + 1 : kb;
    }
    lp[i] = (uint8_t)ka;
    lg[i] = (uint8_t)kb;
  }
}

// ---- 5. weighted lower envelope along the shorter of D / H -----------------------------------------------------------------
// The last position at which parabola i is not above parabola u > i (w2 = s_m^2), clamped to [-1, 1024].  A rounding error
// here can only move a boundary between two parabolas whose values there agree to the last bits.
__device__ __forceinline__ int sepw(double w2, int i, double gi, int u, double gu) {
  const double x = floor((w2 * (double)(u * u - i * i) + (gu - gi)) / (2.0 * w2 * (double)(u - i)));
  return x < -1.0 ? -1 : (x > 1024.0 ? 1024 : (int)x);
}
__device__ __forceinline__ double pval(double sm, int d, double g) { return add_rn(wsq(sm, d), g); }

__global__ __launch_bounds__(64) void sd_edt_mid_kernel(const int* boxes, const unsigned long long* ecount, int first, int Kc,
                                                        int K, int D, int H, int W, int mid_is_h, Samples sp, int* field) {
  extern __shared__ uint32_t s_stk[];
  const Slot S = slot_of(blockIdx.z, first, Kc);
  if (ecount[((int64_t)S.b * K + S.c) * 2 + (1 - S.dir)] == 0) return;
  const int* bx = boxes + ((int64_t)S.b * K + S.c) * 6;
  const int o = blockIdx.y;                                      // coordinate along the other (non-W, non-envelope) axis
  const int o0 = mid_is_h ? bx[0] : bx[2], o1 = mid_is_h ? bx[1] : bx[3];
  const int m0 = mid_is_h ? bx[2] : bx[0], m1 = mid_is_h ? bx[3] : bx[1];
  if (o < o0 || o > o1) return;
  const int xs = bx[4] + 64 * (int)blockIdx.x;
  if (xs > bx[5]) return;
  const int lane = threadIdx.x, x = xs + lane;
  const bool active = x <= bx[5];
  const int64_t V = (int64_t)D * H * W;
  const int64_t smid = mid_is_h ? W : (int64_t)H * W, soth = mid_is_h ? (int64_t)H * W : W;
  int* p = field + (((int64_t)S.b * K + S.c) * 2 + S.dir) * V + o * soth + m0 * smid + x;
  const int m = m1 - m0 + 1;
  const double sm = sp.s[S.b][mid_is_h ? 1 : 0], sx = sp.s[S.b][2], w2 = sm * sm;
  uint32_t* stk = s_stk + lane;
  int q = -1, ts = 0, tdx = 0;                                   // stack top index, its position and |dx|
  double tg = 0.0;                                               // (s_x |dx|)^2 of the top
  constexpr int kPre = 8;
  for (int u0 = 0; u0 < m; u0 += kPre) {
    int gv[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) gv[j] = (active && u0 + j < m) ? p[(int64_t)(u0 + j) * smid] : kInf;
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
      const int u = u0 + j;
      if (gv[j] >= kInf) continue;
      const int dx = (int)__dsqrt_rn((double)gv[j]);            // edt_w left |dx|^2, a perfect square: the root is exact
      const double g = wsq(sx, dx);
      while (q >= 0) {
        int r = 0;
        if (q > 0) {
          const uint32_t e = stk[(q - 1) * 64];
          r = sepw(w2, (int)(e & 1023u), wsq(sx, (int)(e >> 10)), ts, tg) + 1;
        }
        if (pval(sm, r - ts, tg) > pval(sm, r - u, g)) {
          --q;
          if (q >= 0) {
            const uint32_t e = stk[q * 64];
            ts = (int)(e & 1023u);
            tdx = (int)(e >> 10);
            tg = wsq(sx, tdx);
          }
        } else {
          break;
        }
      }
      if (q < 0) {
        q = 0;
        ts = u;
        tdx = dx;
        tg = g;
        stk[0] = ((uint32_t)dx << 10) | (uint32_t)u;
      } else if (sepw(w2, ts, tg, u, g) + 1 < m) {
        ++q;
        ts = u;
        tdx = dx;
        tg = g;
        stk[q * 64] = ((uint32_t)dx << 10) | (uint32_t)u;
      }
    }
  }
  if (!active) return;
  for (int u = m - 1; u >= 0; --u) {
    int val = kInf;
    if (q >= 0) {
      while (q > 0) {
        const uint32_t e = stk[(q - 1) * 64];
        const int s1 = (int)(e & 1023u), d1 = (int)(e >> 10);
        const double g1 = wsq(sx, d1);
        if (pval(sm, u - s1, g1) <= pval(sm, u - ts, tg)) {
          --q;
          ts = s1;
          tdx = d1;
          tg = g1;
        } else {
          break;
        }
      }
      val = tdx | ((u > ts ? u - ts : ts - u) << 10);
    }
    p[(int64_t)u * smid] = val;
  }
}

// ---- 6. last axis at the source edge voxels: the winning offset goes into the voxel's own field word ----------------------
__global__ __launch_bounds__(kThreads) void sd_search_kernel(const uint32_t* pe, const uint32_t* ge, const int* boxes,
                                                             const unsigned long long* ecount, int first, int Kc, int K, int D,
                                                             int H, int W, int mid_is_h, Samples sp, int* field) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t V = (int64_t)D * H * W, HW = (int64_t)H * W;
  const uint32_t keep = (Kc + first >= 32 ? ~0u : ((1u << (Kc + first)) - 1)) & ~((1u << first) - 1);
  const Geo geo = {sp.s[b][0], sp.s[b][1], sp.s[b][2], mid_is_h};
  const double sl = mid_is_h ? geo.sz : geo.sy;
  const int64_t stl = mid_is_h ? HW : W;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + tid; v < V; v += stride) {
    const uint32_t e[2] = {pe[(int64_t)b * V + v] & keep, ge[(int64_t)b * V + v] & keep};
    if (!(e[0] | e[1])) continue;
    const int z = (int)(v / HW), y = (int)((v / W) % H);
    const int l = mid_is_h ? z : y;
    for (int dir = 0; dir < 2; ++dir) {
      uint32_t bits = e[dir];
      while (bits) {
        const int c = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const int64_t bc = (int64_t)b * K + c;
        if (ecount[bc * 2 + (1 - dir)] == 0) continue;          // no target: +inf, decided by the finish
        const int* bx = boxes + bc * 6;
        const int l0 = mid_is_h ? bx[0] : bx[2], l1 = mid_is_h ? bx[1] : bx[3];
        int* f = field + (bc * 2 + dir) * V + v;
        const int own = f[0] & (kInf | kOffMask);
        double best = __builtin_inf();
        int bj = 0;
        if (!(own & kInf)) best = dist2(geo, 0, own);
        for (int j = 1;; ++j) {
          if (wsq(sl, j) >= best) break;                         // every candidate at offset j is at least (s_l j)^2
          const bool lo = l - j >= l0, hi = l + j <= l1;
          if (!lo && !hi) break;
          if (lo) {
            const int t = f[-(int64_t)j * stl];
            const double cand = (t & kInf) ? __builtin_inf() : dist2(geo, j, t);
            if (cand < best) { best = cand; bj = -j; }
          }
          if (hi) {
            const int t = f[(int64_t)j * stl];
            const double cand = (t & kInf) ? __builtin_inf() : dist2(geo, j, t);
            if (cand < best) { best = cand; bj = j; }
          }
        }
        f[0] = own | ((bj + kJBias) << kJShift);                 // the low bits other threads read stay as they are
      }
    }
  }
}

// ---- 7. scans over the source edge voxels ---------------------------------------------------------------------------------
// One add per distinct bin among the lanes that arrive together (the high digits of a slot's keys are nearly all equal).
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, bool on, uint32_t idx) {
  const int lane = threadIdx.x & 63;
  while (on) {
    const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
    const bool same = idx == lead;
    const unsigned long long m = __ballot(same);
    if (same) {
      if (lane == __ffsll((long long)m) - 1) atomicAdd(&hist[lead], (uint32_t)__popcll(m));
      on = false;
    }
  }
}

// (hi, lo) += x, a 128-bit integer held in two words that are updated by separate atomics: the carry out of the low word is
// seen by exactly one adder, which hands it to the high word.  Integer addition commutes, so the total is order-independent.
__device__ __forceinline__ void add128(unsigned long long* lo, unsigned long long* hi, unsigned long long xlo,
                                       unsigned long long xhi) {
  const unsigned long long old = atomicAdd(lo, xlo);
  atomicAdd(hi, xhi + (old > ~xlo ? 1ull : 0ull));
}

__global__ __launch_bounds__(kThreads) void sd_scan_kernel(const uint32_t* pe, const uint32_t* ge,
                                                           const unsigned long long* ecount, int first, int Kc, int K, int D,
                                                           int H, int W, int mid_is_h, int pass, Samples sp, Query qy,
                                                           const int* field, unsigned long long* acc, uint32_t* hist,
                                                           unsigned long long* sel, unsigned long long* above) {
  __shared__ unsigned long long s_lo[64], s_hi[64], s_within[64], s_max[64];     // per (class, direction) slot
  __shared__ unsigned long long s_le[64 * kMaxPct], s_above[64 * kMaxPct];       // per (slot, percentile)
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < 64) s_lo[tid] = s_hi[tid] = s_within[tid] = s_max[tid] = 0;
  for (int i = tid; i < 64 * kMaxPct; i += kThreads) {
    s_le[i] = 0;
    s_above[i] = ~0ull;
  }
  __syncthreads();
  const int64_t V = (int64_t)D * H * W, HW = (int64_t)H * W;
  const uint32_t keep = (Kc + first >= 32 ? ~0u : ((1u << (Kc + first)) - 1)) & ~((1u << first) - 1);
  const Geo geo = {sp.s[b][0], sp.s[b][1], sp.s[b][2], mid_is_h};
  const double fix = sp.fix[b];
  const int64_t stl = mid_is_h ? HW : W;
  const int shift = 55 - kDigit * pass;                          // of this pass's digit (passes 0..5)
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + tid; v < V; v += stride) {
    const uint32_t e[2] = {pe[(int64_t)b * V + v] & keep, ge[(int64_t)b * V + v] & keep};
    if (!(e[0] | e[1])) continue;
    for (int dir = 0; dir < 2; ++dir) {
      uint32_t bits = e[dir];
      while (bits) {
        const int c = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const int64_t bc = (int64_t)b * K + c;
        if (ecount[bc * 2 + (1 - dir)] == 0) continue;
        const int* f = field + (bc * 2 + dir) * V + v;
        const int own = f[0];
        const int bj = ((own >> kJShift) & kJMask) - kJBias;
        const int t = bj ? f[(int64_t)bj * stl] : own;
        const double d2 = dist2(geo, bj < 0 ? -bj : bj, t & kOffMask);
        const unsigned long long key = (unsigned long long)__double_as_longlong(d2);      // d2 >= 0: the bits order as the values
        const int slot = (c - first) * 2 + dir;
        if (pass == 0) {
          const double d = __dsqrt_rn(d2);
          const double th = d * fix;                             // < 2^31; fix is a power of two
          const unsigned long long xhi = (unsigned long long)th;
          const unsigned long long xlo = (unsigned long long)((th - (double)xhi) * 18446744073709551616.0);
          add128(&s_lo[slot], &s_hi[slot], xlo, xhi);
          if (qy.has_tau && d <= qy.tau[c - first]) atomicAdd(&s_within[slot], 1ull);
          atomicMax(&s_max[slot], key);
        }
        for (int p = 0; p < qy.npct; ++p) {
          const int64_t q = (bc * 2 + dir) * kMaxPct + p;
          if (pass < kPasses) {
            const bool match = pass == 0 || (key >> (shift + kDigit)) == sel[q * 4];
            wave_hist_add(hist, match, (uint32_t)(q * kBins + (int64_t)((key >> shift) & (kBins - 1))));
          } else if (key <= sel[q * 4]) {
            atomicAdd(&s_le[slot * kMaxPct + p], 1ull);
          } else {
            atomicMin(&s_above[slot * kMaxPct + p], key);
          }
        }
      }
    }
  }
  __syncthreads();
  if (pass == 0 && tid < Kc * 2) {
    unsigned long long* A = acc + (((int64_t)b * K + first + tid / 2) * 2 + (tid & 1)) * 4;
    if (s_lo[tid] | s_hi[tid]) add128(&A[0], &A[1], s_lo[tid], s_hi[tid]);
    if (s_within[tid]) atomicAdd(&A[2], s_within[tid]);
    if (s_max[tid]) atomicMax(&A[3], s_max[tid]);
  }
  if (pass == kPasses) {
    for (int i = tid; i < Kc * 2 * kMaxPct; i += kThreads) {
      const int slot = i / kMaxPct, p = i % kMaxPct;
      const int64_t q = (((int64_t)b * K + first + slot / 2) * 2 + (slot & 1)) * kMaxPct + p;
      if (s_le[i]) atomicAdd(&sel[q * 4 + 2], s_le[i]);
      if (s_above[i] != ~0ull) atomicMin(&above[q], s_above[i]);
    }
  }
}

// The 0-based rank numpy's linear percentile starts from (the largest element for percentile 0, as MONAI's `percentile=None`).
__device__ __forceinline__ int64_t lower_rank(int64_t n, double percentile) {
  if (percentile == 0.0 || n == 1) return n - 1;
  const double vi = (double)(n - 1) * (percentile / 100.0);
  return vi >= (double)(n - 1) ? n - 1 : (int64_t)floor(vi);
}

// One workgroup per (slot, percentile): the digit whose bin holds the remaining rank; clears the histogram for the next pass.
__global__ __launch_bounds__(kThreads) void sd_choose_kernel(const unsigned long long* ecount, int first, int Kc, int K, int pass,
                                                             Query qy, uint32_t* hist, unsigned long long* sel) {
  __shared__ unsigned long long s_pre[kThreads];
  const int tid = threadIdx.x;
  const int p = blockIdx.x % qy.npct;
  const Slot S = slot_of(blockIdx.x / qy.npct, first, Kc);
  const int64_t bc = (int64_t)S.b * K + S.c;
  const int64_t n = (int64_t)ecount[bc * 2 + S.dir];
  if (n == 0 || ecount[bc * 2 + (1 - S.dir)] == 0) return;      // nothing was counted: the histogram is still clear
  const int64_t q = (bc * 2 + S.dir) * kMaxPct + p;
  const unsigned long long rank = pass == 0 ? (unsigned long long)lower_rank(n, qy.pct[p]) : sel[q * 4 + 1];
  constexpr int kSeg = kBins / kThreads;
  uint32_t* h = hist + q * kBins + tid * kSeg;
  uint32_t mine[kSeg];
  unsigned long long sum = 0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) {
    mine[i] = h[i];
    h[i] = 0;
    sum += mine[i];
  }
  s_pre[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < kThreads; ++t) {
      const unsigned long long s = s_pre[t];
      s_pre[t] = run;
      run += s;
    }
  }
  __syncthreads();
  unsigned long long run = s_pre[tid];
  if (rank >= run && rank < run + sum) {                         // exactly one thread
#pragma unroll
    for (int i = 0; i < kSeg; ++i) {
      if (rank >= run && rank < run + mine[i]) {
        sel[q * 4] = pass == 0 ? (unsigned long long)(tid * kSeg + i) : ((sel[q * 4] << kDigit) | (unsigned long long)(tid * kSeg + i));
        sel[q * 4 + 1] = rank - run;
      }
      run += mine[i];
    }
  }
}

// ---- 8. finish -------------------------------------------------------------------------------------------------------------
__device__ double directed_value(const unsigned long long* acc, const unsigned long long* sel, unsigned long long above,
                                 int64_t n, double percentile) {
  const double dmax = __dsqrt_rn(__longlong_as_double((long long)acc[3]));
  if (percentile == 0.0 || n == 1) return dmax;
  const double vi = (double)(n - 1) * (percentile / 100.0);
  if (vi >= (double)(n - 1)) return dmax;
  const double lo = floor(vi);
  const double t = vi - lo;
  const unsigned long long k0 = sel[0], k1 = sel[2] > (unsigned long long)lo + 1 ? k0 : above;
  const double a = __dsqrt_rn(__longlong_as_double((long long)k0)), bb = __dsqrt_rn(__longlong_as_double((long long)k1));
  const double diff = bb - a;
  return t >= 0.5 ? bb - diff * (1.0 - t) : a + diff * t;
}

__global__ __launch_bounds__(64) void sd_finish_kernel(const unsigned long long* ecount, const unsigned long long* acc,
                                                       const unsigned long long* sel, const unsigned long long* above, int B,
                                                       int first, int Kc, int K, Samples sp, Query qy, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * Kc) return;
  const int b = i / Kc, c = first + i % Kc, P = qy.npct;
  const int64_t bc = (int64_t)b * K + c, BK = (int64_t)B * Kc;
  const int64_t n[2] = {(int64_t)ecount[bc * 2 + 0], (int64_t)ecount[bc * 2 + 1]};
  const bool both_empty = n[0] == 0 && n[1] == 0, one_empty = !both_empty && (n[0] == 0 || n[1] == 0);
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  float* hd = out + (int64_t)i * P;
  float* hdd = out + BK * P + (int64_t)i * P;
  float* asd = out + 2 * BK * P + (int64_t)i * 2;
  float* assd = out + 2 * BK * P + 2 * BK + i;
  float* nsd = out + 2 * BK * P + 3 * BK + i;
  for (int p = 0; p < P; ++p) {
    double u = both_empty ? nan : inf, d0 = u;
    if (!both_empty && !one_empty) {
      const int64_t q0 = (bc * 2 + 0) * kMaxPct + p, q1 = (bc * 2 + 1) * kMaxPct + p;
      d0 = directed_value(acc + (bc * 2 + 0) * 4, sel + q0 * 4, above[q0], n[0], qy.pct[p]);
      u = fmax(d0, directed_value(acc + (bc * 2 + 1) * 4, sel + q1 * 4, above[q1], n[1], qy.pct[p]));
    }
    hd[p] = (float)u;
    hdd[p] = (float)d0;
  }
  double sum[2] = {0.0, 0.0};
  for (int dir = 0; dir < 2; ++dir) {
    const unsigned long long* A = acc + (bc * 2 + dir) * 4;
    sum[dir] = ((double)A[1] + (double)A[0] / 18446744073709551616.0) / sp.fix[b];      // A[1] . A[0] in units of 1 / fix
    asd[dir] = (float)(n[dir] == 0 ? nan : (n[1 - dir] == 0 ? inf : sum[dir] / (double)n[dir]));
  }
  const double total = (double)(n[0] + n[1]);
  *assd = (float)(both_empty ? nan : (one_empty ? inf : (sum[0] + sum[1]) / total));
  if (qy.has_tau) {
    const unsigned long long within = acc[(bc * 2 + 0) * 4 + 2] + acc[(bc * 2 + 1) * 4 + 2];
    *nsd = (float)(both_empty ? nan : (one_empty ? 0.0 : (double)within / total));
  }
}

}  // namespace

extern "C" int64_t micf_surface_distance_workspace(int B, int K, int D, int H, int W) {
  if (!shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (!shape_supported(K, D, H, W) || B > kMaxBatch) return MICF_EUNSUPPORTED;
  return layout(B, K, D, H, W).total;
}

extern "C" int micf_surface_distance(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W, int first_class,
                                     const int32_t* label_values, int num_label_values, const double* spacing,
                                     const double* percentiles, int num_percentiles, const double* thresholds, void* workspace,
                                     int64_t workspace_bytes, float* out, micf_stream_t stream) {
  if (!pred || !gt || !spacing || !percentiles || !workspace || !out || !shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (form < MICF_FORM_LABEL || form > MICF_FORM_VALUES_I32) return MICF_EINVAL;
  if (first_class < 0 || first_class >= K) return MICF_EINVAL;
  if (num_percentiles < 1 || num_percentiles > kMaxPct) return MICF_EINVAL;
  if (!shape_supported(K, D, H, W) || B > kMaxBatch) return MICF_EUNSUPPORTED;        // (before the arrays sized by B and K are read)
  const bool values = form == MICF_FORM_VALUES_I16 || form == MICF_FORM_VALUES_I32;
  const int Kc = K - first_class;
  Query qy = {};
  qy.npct = num_percentiles;
  for (int p = 0; p < num_percentiles; ++p) {
    if (!(percentiles[p] >= 0.0 && percentiles[p] <= 100.0)) return MICF_EINVAL;
    qy.pct[p] = percentiles[p];
  }
  qy.has_tau = thresholds ? 1 : 0;
  for (int c = 0; thresholds && c < Kc; ++c) {
    if (!(thresholds[c] >= 0.0)) return MICF_EINVAL;                                  // (false for nan)
    qy.tau[c] = thresholds[c];
  }
  Lut lut = {};
  if (values) {
    if (!label_values || num_label_values != K - 1) return MICF_EINVAL;
    for (int i = 0; i < num_label_values; ++i) {
      if (label_values[i] == 0) return MICF_EINVAL;
      if (form == MICF_FORM_VALUES_I16 && (label_values[i] < -32768 || label_values[i] > 32767)) return MICF_EINVAL;
      for (int j = 0; j < i; ++j)
        if (label_values[j] == label_values[i]) return MICF_EINVAL;
      lut.v[i] = label_values[i];
    }
    lut.n = num_label_values;
  } else if (label_values || num_label_values != 0) {
    return MICF_EINVAL;
  }
  Samples sp = {};
  bool out_of_range = false;
  const int ext[3] = {D, H, W};
  for (int b = 0; b < B; ++b) {
    double diag2 = 0.0;
    for (int a = 0; a < 3; ++a) {
      const double s = spacing[3 * b + a];
      if (!(s > 0.0) || !std::isfinite(s)) return MICF_EINVAL;
      if (s < std::ldexp(1.0, -256) || s > std::ldexp(1.0, 256)) out_of_range = true;
      sp.s[b][a] = s;
      diag2 += (s * (ext[a] - 1)) * (s * (ext[a] - 1));
    }
    // no distance exceeds the box diagonal < 2^(e + 1): d * 2^(30 - e) < 2^31, and the sum of 2^30 of them stays below 2^61
    const int e = diag2 > 0.0 && !out_of_range ? std::ilogb(std::sqrt(diag2)) : 0;
    sp.fix[b] = std::ldexp(1.0, 30 - e);
  }
  if (out_of_range) return MICF_EUNSUPPORTED;
  const Layout L = layout(B, K, D, H, W);
  if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MICF_EINVAL;

  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  uint32_t *pm = (uint32_t*)(ws + L.pm), *gm = (uint32_t*)(ws + L.gm), *pe = (uint32_t*)(ws + L.pe), *ge = (uint32_t*)(ws + L.ge);
  auto* counts = (unsigned long long*)(ws + L.counts);
  auto* ecount = (unsigned long long*)(ws + L.ecount);
  auto* acc = (unsigned long long*)(ws + L.acc);
  auto* sel = (unsigned long long*)(ws + L.sel);
  auto* above = (unsigned long long*)(ws + L.above);
  uint32_t *proj = (uint32_t*)(ws + L.proj), *hist = (uint32_t*)(ws + L.hist);
  int* boxes = (int*)(ws + L.boxes);
  int* field = (int*)(ws + L.field);
  const int64_t V = (int64_t)D * H * W;
  const int mid_is_h = H <= D ? 1 : 0;
  const int lmid = mid_is_h ? H : D, loth = mid_is_h ? D : H;
  const int64_t vb = (V + kThreads - 1) / kThreads;

  if (hipMemsetAsync(ws + L.zero_begin, 0, L.zero_end - L.zero_begin, s) != hipSuccess) return MICF_ELAUNCH;
  if (hipMemsetAsync(ws + L.above, 0xff, L.above_end - L.above, s) != hipSuccess) return MICF_ELAUNCH;
  if (values) {
    uint8_t *lp = (uint8_t*)(ws + L.lab_p), *lg = (uint8_t*)(ws + L.lab_g);
    const int64_t rb = (B * V + kThreads - 1) / kThreads;
    const dim3 rgrid((unsigned)(rb < 2048 ? rb : 2048));
    if (form == MICF_FORM_VALUES_I16)
      hipLaunchKernelGGL(sd_remap_kernel<int16_t>, rgrid, dim3(kThreads), 0, s, static_cast<const int16_t*>(pred),
                         static_cast<const int16_t*>(gt), B * V, lut, lp, lg);
    else
      hipLaunchKernelGGL(sd_remap_kernel<int32_t>, rgrid, dim3(kThreads), 0, s, static_cast<const int32_t*>(pred),
                         static_cast<const int32_t*>(gt), B * V, lut, lp, lg);
    pred = lp;
    gt = lg;
  }
  int rc = classify(pred, gt, form == MICF_FORM_ONEHOT, true, B, K, D, H, W, pm, gm, counts, proj, s);
  if (rc) return rc;
  hipLaunchKernelGGL(surf_box_kernel, dim3(B), dim3(128), 0, s, proj, K, D, H, W, boxes);
  const int eblocks = (int)(vb < 2048 ? vb : 2048);
  hipLaunchKernelGGL(surf_edges_kernel, dim3(eblocks, B), dim3(kThreads), 0, s, pm, gm, boxes, K, D, H, W, pe, ge, ecount);
  const unsigned slots = (unsigned)(B * Kc * 2);
  hipLaunchKernelGGL(surf_edt_w_kernel, dim3((unsigned)(((int64_t)D * H + 3) / 4), slots), dim3(kThreads), 0, s, pe, ge, boxes,
                     ecount, first_class, Kc, K, D, H, W, field);
  const size_t lds_mid = (size_t)64 * lmid * sizeof(uint32_t);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sd_edt_mid_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(kMaxMid * 64 * sizeof(uint32_t)));
  hipLaunchKernelGGL(sd_edt_mid_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)loth, slots), dim3(64), lds_mid, s, boxes,
                     ecount, first_class, Kc, K, D, H, W, mid_is_h, sp, field);
  const int lblocks = (int)(vb < 1024 ? vb : 1024);
  hipLaunchKernelGGL(sd_search_kernel, dim3(lblocks, B), dim3(kThreads), 0, s, pe, ge, boxes, ecount, first_class, Kc, K, D, H, W,
                     mid_is_h, sp, field);
  for (int pass = 0; pass <= kPasses; ++pass) {
    hipLaunchKernelGGL(sd_scan_kernel, dim3(lblocks, B), dim3(kThreads), 0, s, pe, ge, ecount, first_class, Kc, K, D, H, W,
                       mid_is_h, pass, sp, qy, field, acc, hist, sel, above);
    if (pass < kPasses)
      hipLaunchKernelGGL(sd_choose_kernel, dim3(slots * (unsigned)num_percentiles), dim3(kThreads), 0, s, ecount, first_class, Kc,
                         K, pass, qy, hist, sel);
  }
  hipLaunchKernelGGL(sd_finish_kernel, dim3((unsigned)((B * Kc + 63) / 64)), dim3(64), 0, s, ecount, acc, sel, above, B,
                     first_class, Kc, K, sp, qy, out);
  MICF_RETURN_LAUNCH();
}
