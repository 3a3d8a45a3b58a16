// surface_common.h -- steps 1-4 of the surface metrics' launch plan (classify, box, edges, the EDT pass along W) and the shape
// limits, shared by surface_metrics.hip (voxel-unit HD / IoU) and surface_distance.hip (spaced HD / ASD / NSD).  Both see the
// same edge sets because both run these kernels.  Included inside no namespace; everything here has internal linkage.
#pragma once
#include "common.h"
#include "../../include/micformer_metrics.h"

namespace {

constexpr int kInf = 1 << 30;        // "no target on this line"; finite squared distances stay below 2^22
constexpr int kMaxDim = 1024;        // per spatial axis (the envelope stack packs a position in 10 bits)
constexpr int kMaxMid = 512;         // the envelope axis: 64 lines x 512 entries x 4 B = 128 KiB of LDS
constexpr int kThreads = 256;

int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

bool shape_ok(int B, int K, int D, int H, int W) { return B > 0 && K > 0 && D > 0 && H > 0 && W > 0; }
bool shape_supported(int K, int D, int H, int W) {
  return K <= 32 && D <= kMaxDim && H <= kMaxDim && W <= kMaxDim && (D < H ? D : H) <= kMaxMid;
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// ---- 1. classify: masks, counts, projections ------------------------------------------------------------------------------
template <bool ONEHOT, bool FULL>
__global__ __launch_bounds__(kThreads) void surf_classify_kernel(const void* pred, const void* gt, int K, int D, int H, int W,
                                                                 int rows_per_block, uint32_t* pm, uint32_t* gm,
                                                                 unsigned long long* counts, uint32_t* proj) {
  __shared__ uint32_t s_cnt[3 * 32];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int64_t V = (int64_t)D * H * W;
  if (tid < 96) s_cnt[tid] = 0;
  __syncthreads();
  uint32_t cp = 0, cg = 0, ci = 0;           // lane c: this wave's counts of class c
  uint32_t xo[kMaxDim / kThreads] = {0, 0, 0, 0};
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  for (int64_t r = r0; r < r0 + rows_per_block && r < (int64_t)D * H; ++r) {
    const int z = (int)(r / H), y = (int)(r % H);
    uint32_t row_or = 0;
    for (int x0 = 0; x0 < W; x0 += kThreads) {
      const int x = x0 + tid;
      uint32_t pmask = 0, gmask = 0;
      if (x < W) {
        const int64_t v = r * W + x;
        if (ONEHOT) {
          const float* P = static_cast<const float*>(pred) + (int64_t)b * K * V + v;
          const float* G = static_cast<const float*>(gt) + (int64_t)b * K * V + v;
          for (int c = 0; c < K; ++c) {
            pmask |= (P[c * V] == 1.0f ? 1u : 0u) << c;
            gmask |= (G[c * V] == 1.0f ? 1u : 0u) << c;
          }
        } else {
          const int lp = static_cast<const uint8_t*>(pred)[(int64_t)b * V + v];
          const int lg = static_cast<const uint8_t*>(gt)[(int64_t)b * V + v];
          pmask = lp < K ? 1u << lp : 0u;
          gmask = lg < K ? 1u << lg : 0u;
        }
        if (FULL) {
          pm[(int64_t)b * V + v] = pmask;
          gm[(int64_t)b * V + v] = gmask;
        }
      }
      const uint32_t im = pmask & gmask;
      for (int c = 0; c < K; ++c) {
        const uint32_t np = (uint32_t)__popcll(__ballot((pmask >> c) & 1u));
        const uint32_t ng = (uint32_t)__popcll(__ballot((gmask >> c) & 1u));
        const uint32_t ni = (uint32_t)__popcll(__ballot((im >> c) & 1u));
        if (lane == c) { cp += np; cg += ng; ci += ni; }
      }
      if (FULL) {
        const uint32_t u = pmask | gmask;
        row_or |= u;
#pragma unroll
        for (int j = 0; j < kMaxDim / kThreads; ++j)
          if (j == x0 / kThreads) xo[j] |= u;
      }
    }
    if (FULL) {
      row_or = wave_or(row_or);
      if (lane == 0 && row_or) {
        atomicOr(&proj[(int64_t)b * (D + H + W) + z], row_or);
        atomicOr(&proj[(int64_t)b * (D + H + W) + D + y], row_or);
      }
    }
  }
  if (FULL) {
#pragma unroll
    for (int j = 0; j < kMaxDim / kThreads; ++j) {
      const int x = j * kThreads + tid;
      if (x < W && xo[j]) atomicOr(&proj[(int64_t)b * (D + H + W) + D + H + x], xo[j]);
    }
  }
  if (lane < K) {
    atomicAdd(&s_cnt[lane], cp);
    atomicAdd(&s_cnt[32 + lane], cg);
    atomicAdd(&s_cnt[64 + lane], ci);
  }
  __syncthreads();
  if (tid < K) {
    unsigned long long* C = counts + ((int64_t)b * K + tid) * 3;
    if (s_cnt[tid]) atomicAdd(&C[0], (unsigned long long)s_cnt[tid]);
    if (s_cnt[32 + tid]) atomicAdd(&C[1], (unsigned long long)s_cnt[32 + tid]);
    if (s_cnt[64 + tid]) atomicAdd(&C[2], (unsigned long long)s_cnt[64 + tid]);
  }
}

// ---- 2. union boxes from the projections ----------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void surf_box_kernel(const uint32_t* proj, int K, int D, int H, int W, int* boxes) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (t >= 3 * K) return;
  const int c = t / 3, a = t % 3;
  const int n = a == 0 ? D : (a == 1 ? H : W);
  const uint32_t* p = proj + (int64_t)b * (D + H + W) + (a == 0 ? 0 : (a == 1 ? D : D + H));
  int lo = 0, hi = -1;
  for (int i = 0; i < n; ++i)
    if ((p[i] >> c) & 1u) { lo = i; break; }
  for (int i = n - 1; i >= 0; --i)
    if ((p[i] >> c) & 1u) { hi = i; break; }
  boxes[((int64_t)b * K + c) * 6 + 2 * a] = lo;
  boxes[((int64_t)b * K + c) * 6 + 2 * a + 1] = hi;
}

// ---- 3. edges ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t edge_bits(const uint32_t* m, int64_t v, int z, int y, int x, int D, int H, int W,
                                              uint32_t cz, uint32_t cy, uint32_t cx) {
  const uint32_t c = m[v];
  if (!c) return 0;
  const int64_t HW = (int64_t)H * W;
  const uint32_t zm = z > 0 ? m[v - HW] : 0u, zp = z < D - 1 ? m[v + HW] : 0u;
  const uint32_t ym = y > 0 ? m[v - W] : 0u, yp = y < H - 1 ? m[v + W] : 0u;
  const uint32_t xm = x > 0 ? m[v - 1] : 0u, xp = x < W - 1 ? m[v + 1] : 0u;
  return c & ((~(zm & zp) & cz) | (~(ym & yp) & cy) | (~(xm & xp) & cx));
}

__global__ __launch_bounds__(kThreads) void surf_edges_kernel(const uint32_t* pm, const uint32_t* gm, const int* boxes, int K, int D,
                                                              int H, int W, uint32_t* pe, uint32_t* ge,
                                                              unsigned long long* ecount) {
  __shared__ uint32_t s_consult[3];
  __shared__ uint32_t s_cnt[2 * 32];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) {
    // bit c of s_consult[a]: class c's box is more than one voxel thick along axis a (MONAI squeezes the others away)
    for (int a = 0; a < 3; ++a) {
      bool thick = false;
      if (lane < K) {
        const int* bx = boxes + ((int64_t)b * K + lane) * 6;
        thick = bx[2 * a + 1] > bx[2 * a];
      }
      const uint32_t m = (uint32_t)__ballot(thick);
      if (lane == 0) s_consult[a] = m;
    }
    s_cnt[lane] = 0;
  }
  __syncthreads();
  const uint32_t cz = s_consult[0], cy = s_consult[1], cx = s_consult[2];
  const int64_t V = (int64_t)D * H * W;
  const uint32_t* P = pm + (int64_t)b * V;
  const uint32_t* G = gm + (int64_t)b * V;
  uint32_t np_ = 0, ng_ = 0;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < V; base += stride) {
    const int64_t v = base + tid;
    uint32_t ep = 0, eg = 0;
    if (v < V) {
      const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((int64_t)H * W));
      ep = edge_bits(P, v, z, y, x, D, H, W, cz, cy, cx);
      eg = edge_bits(G, v, z, y, x, D, H, W, cz, cy, cx);
      pe[(int64_t)b * V + v] = ep;
      ge[(int64_t)b * V + v] = eg;
    }
    if (__ballot((ep | eg) != 0u)) {
      for (int c = 0; c < K; ++c) {
        const uint32_t a = (uint32_t)__popcll(__ballot((ep >> c) & 1u));
        const uint32_t g = (uint32_t)__popcll(__ballot((eg >> c) & 1u));
        if (lane == c) { np_ += a; ng_ += g; }
      }
    }
  }
  if (lane < K) {
    atomicAdd(&s_cnt[lane], np_);
    atomicAdd(&s_cnt[32 + lane], ng_);
  }
  __syncthreads();
  if (tid < K) {
    if (s_cnt[tid]) atomicAdd(&ecount[((int64_t)b * K + tid) * 2 + 0], (unsigned long long)s_cnt[tid]);
    if (s_cnt[32 + tid]) atomicAdd(&ecount[((int64_t)b * K + tid) * 2 + 1], (unsigned long long)s_cnt[32 + tid]);
  }
}

// (b, c, direction) of a slot index over the scored classes
struct Slot {
  int b, c, dir;
};
__device__ __forceinline__ Slot slot_of(int s, int first, int Kc) {
  Slot r;
  r.dir = s & 1;
  const int bc = s >> 1;
  r.b = bc / Kc;
  r.c = first + bc % Kc;
  return r;
}

// ---- 4. EDT along W: one wave per row of the box, two scans over the row's ballots --------------------------------------
__global__ __launch_bounds__(kThreads) void surf_edt_w_kernel(const uint32_t* pe, const uint32_t* ge, const int* boxes,
                                                              const unsigned long long* ecount, int first, int Kc, int K, int D,
                                                              int H, int W, int* field) {
  const Slot S = slot_of(blockIdx.y, first, Kc);
  const int* bx = boxes + ((int64_t)S.b * K + S.c) * 6;
  if (ecount[((int64_t)S.b * K + S.c) * 2 + (1 - S.dir)] == 0) return;     // no target edges: the finish needs no field
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + wave;
  if (row >= (int64_t)D * H) return;
  const int z = (int)(row / H), y = (int)(row % H);
  if (z < bx[0] || z > bx[1] || y < bx[2] || y > bx[3]) return;
  const int x0 = bx[4], x1 = bx[5];
  const int64_t V = (int64_t)D * H * W;
  const uint32_t* T = (S.dir == 0 ? ge : pe) + (int64_t)S.b * V + row * W;
  int* F = field + (((int64_t)S.b * K + S.c) * 2 + S.dir) * V + row * W;
  const uint32_t bit = 1u << S.c;
  const int n = x1 - x0 + 1, nch = (n + 63) >> 6;
  unsigned long long ball[kMaxDim / 64];
#pragma unroll
  for (int k = 0; k < kMaxDim / 64; ++k) {
    ball[k] = 0;
    if (k < nch) {
      const int x = x0 + 64 * k + lane;
      ball[k] = __ballot(x <= x1 && (T[x] & bit));
    }
  }
  int next_after[kMaxDim / 64];          // first target position (relative) in the chunks after k
  int nxt = kInf;
#pragma unroll
  for (int k = kMaxDim / 64 - 1; k >= 0; --k) {
    next_after[k] = nxt;
    if (ball[k]) nxt = 64 * k + __ffsll((long long)ball[k]) - 1;
  }
  int last = -kInf;                      // last target position (relative) in the chunks before k
  const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
  const unsigned long long ge_ = ~0ull << lane;
#pragma unroll
  for (int k = 0; k < kMaxDim / 64; ++k) {
    if (k < nch) {
      const int xr = 64 * k + lane;
      const unsigned long long lm = ball[k] & le, rm = ball[k] & ge_;
      const int left = lm ? 64 * k + 63 - __clzll((long long)lm) : last;
      const int right = rm ? 64 * k + __ffsll((long long)rm) - 1 : next_after[k];
      int d = kInf;
      if (left > -kInf) d = (xr - left) * (xr - left);
      if (right < kInf) d = min(d, (right - xr) * (right - xr));
      if (xr < n) F[x0 + xr] = d;
      if (ball[k]) last = 64 * k + 63 - __clzll((long long)ball[k]);
    }
  }
}

int classify(const void* pred, const void* gt, int onehot, bool full, int B, int K, int D, int H, int W, uint32_t* pm,
             uint32_t* gm, unsigned long long* counts, uint32_t* proj, hipStream_t s) {
  const int64_t rows = (int64_t)D * H;
  int64_t rpb = (rows * B + 4095) / 4096;
  if (rpb < 1) rpb = 1;
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)B);
  if (onehot) {
    if (full) hipLaunchKernelGGL((surf_classify_kernel<true, true>), grid, dim3(kThreads), 0, s, pred, gt, K, D, H, W, (int)rpb, pm, gm, counts, proj);
    else hipLaunchKernelGGL((surf_classify_kernel<true, false>), grid, dim3(kThreads), 0, s, pred, gt, K, D, H, W, (int)rpb, pm, gm, counts, proj);
  } else {
    if (full) hipLaunchKernelGGL((surf_classify_kernel<false, true>), grid, dim3(kThreads), 0, s, pred, gt, K, D, H, W, (int)rpb, pm, gm, counts, proj);
    else hipLaunchKernelGGL((surf_classify_kernel<false, false>), grid, dim3(kThreads), 0, s, pred, gt, K, D, H, W, (int)rpb, pm, gm, counts, proj);
  }
  return hipGetLastError() == hipSuccess ? MICF_OK : MICF_ELAUNCH;
}

}  // namespace
