// surface_metrics.hip -- on-device HD95 / mean IoU (include/micformer_metrics.h), restated from MONAI 1.1's
// compute_hausdorff_distance / compute_iou.  Exact and deterministic: every distance is an integer squared distance, order
// statistics come from integer histograms, and the only float arithmetic (sqrt, numpy's lerp) runs once per (b, c) in double.
//
// Launch plan of micf_hausdorff_distance (all batched over (b, c, direction), no host round trip):
//   1 classify   pred / gt -> per-voxel class-bit masks, |P| |G| |P&G| per (b, c), OR-projections of the union on the 3 axes
//   2 box        the union box of every (b, c) from the projections
//   3 edges      per-voxel edge bits (6-neighbour erosion; axes where the box is 1 voxel thick are not consulted) + edge counts
//   4 edt_w      squared distance to the nearest target edge along W (two scans per row, one wave per row)
//   5 edt_mid    lower envelope of parabolas along the shorter of D / H (Meijster), stacks in LDS, 64 lines adjacent in W
//   6 edt_last   at every source edge voxel: min over the last axis (outward search with early exit) -> integer histogram
//   7 finalize   ranks -> sqrt -> numpy's lerp in double, nan / inf rules, undirected max, float32 store
// Direction 0 is pred -> gt (distance to the gt edges), direction 1 gt -> pred.  Steps 1-4 live in surface_common.h, which
// surface_distance.hip (the spaced metrics) includes too.
#include "surface_common.h"

namespace {

constexpr int kLdsHist = 8192;       // LDS histogram entries of the last pass, shared by the (class, direction) slots

struct Layout {
  int64_t pm, gm, pe, ge;            // uint32 class-bit masks [B][V]: membership pred / gt, edges pred / gt
  int64_t zero_begin;
  int64_t counts;                    // u64 [B][K][3]: |P|, |G|, |P&G|
  int64_t ecount;                    // u64 [B][K][2]: pred edges, gt edges
  int64_t proj;                      // u32 [B][D + H + W]: OR of the union's class bits over each slice
  int64_t gmax;                      // u32 [B][K][2]: the largest squared distance per direction
  int64_t hist;                      // u32 [B][K][2][nh]
  int64_t zero_end;
  int64_t boxes;                     // int [B][K][6]: z0 z1 y0 y1 x0 x1 (inclusive; z1 < z0 when empty)
  int64_t field;                     // int [B][K][2][V]: squared distance to the direction's target edges (box region only)
  int64_t total;
  int64_t nh;
};

Layout layout(int B, int K, int D, int H, int W) {
  Layout L;
  const int64_t V = (int64_t)D * H * W;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o = align256(o + bytes); return r; };
  L.nh = (int64_t)(D - 1) * (D - 1) + (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1) + 1;
  L.pm = take(4 * B * V);
  L.gm = take(4 * B * V);
  L.pe = take(4 * B * V);
  L.ge = take(4 * B * V);
  L.zero_begin = o;
  L.counts = take(8 * (int64_t)B * K * 3);
  L.ecount = take(8 * (int64_t)B * K * 2);
  L.proj = take(4 * (int64_t)B * (D + H + W));
  L.gmax = take(4 * (int64_t)B * K * 2);
  L.hist = take(4 * (int64_t)B * K * 2 * L.nh);
  L.zero_end = o;
  L.boxes = take(4 * (int64_t)B * K * 6);
  L.field = take(4 * (int64_t)B * K * 2 * V);
  L.total = o;
  return L;
}

__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ---- 5. EDT along the envelope axis (Meijster / Felzenszwalb-Huttenlocher, integer separators) ---------------------------
// One wave = 64 lines adjacent in W; lane l's stack lives at LDS [k * 64 + l] (bank = lane: conflict-free for any k).  A stack
// entry packs (g << 10) | position; g < 2^21 (a squared distance along W) so the pack fits 32 bits.
__device__ __forceinline__ int sep(int i, int gi, int u, int gu) { return floor_div(u * u - i * i + gu - gi, 2 * (u - i)); }

__global__ __launch_bounds__(64) void surf_edt_mid_kernel(const int* boxes, const unsigned long long* ecount, int first, int Kc,
                                                          int K, int D, int H, int W, int mid_is_h, int* field) {
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
  uint32_t* stk = s_stk + lane;
  int q = -1, ts = 0, tg = 0;                                    // stack top index and its (position, g)
  constexpr int kPre = 8;
  for (int u0 = 0; u0 < m; u0 += kPre) {
    int gv[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) gv[j] = (active && u0 + j < m) ? p[(int64_t)(u0 + j) * smid] : kInf;
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
      const int u = u0 + j, g = gv[j];
      if (g >= kInf) continue;
      while (q >= 0) {
        int r = 0;
        if (q > 0) {
          const uint32_t e = stk[(q - 1) * 64];
          r = sep((int)(e & 1023u), (int)(e >> 10), ts, tg) + 1;
        }
        if ((r - ts) * (r - ts) + tg > (r - u) * (r - u) + g) {
          --q;
          if (q >= 0) {
            const uint32_t e = stk[q * 64];
            ts = (int)(e & 1023u);
            tg = (int)(e >> 10);
          }
        } else {
          break;
        }
      }
      if (q < 0) {
        q = 0;
        ts = u;
        tg = g;
        stk[0] = ((uint32_t)g << 10) | (uint32_t)u;
      } else if (sep(ts, tg, u, g) + 1 < m) {
        ++q;
        ts = u;
        tg = g;
        stk[q * 64] = ((uint32_t)g << 10) | (uint32_t)u;
      }
    }
  }
  if (!active) return;
  for (int u = m - 1; u >= 0; --u) {
    int val = kInf;
    if (q >= 0) {
      while (q > 0) {
        const uint32_t e = stk[(q - 1) * 64];
        const int s1 = (int)(e & 1023u), g1 = (int)(e >> 10);
        if ((u - s1) * (u - s1) + g1 <= (u - ts) * (u - ts) + tg) {
          --q;
          ts = s1;
          tg = g1;
        } else {
          break;
        }
      }
      val = (u - ts) * (u - ts) + tg;
    }
    p[(int64_t)u * smid] = val;
  }
}

// ---- 6. last axis at the source edge voxels -> histograms ----------------------------------------------------------------
__device__ __forceinline__ int search_last(const int* f, int l, int l0, int l1, int64_t s) {
  int best = f[0];
  for (int j = 1;; ++j) {
    if (j * j >= best) break;
    const bool lo = l - j >= l0, hi = l + j <= l1;
    if (!lo && !hi) break;
    if (lo) best = min(best, f[-(int64_t)j * s] + j * j);
    if (hi) best = min(best, f[(int64_t)j * s] + j * j);
  }
  return best;
}

__global__ __launch_bounds__(kThreads) void surf_edt_last_kernel(const uint32_t* pe, const uint32_t* ge, const int* boxes,
                                                                 const unsigned long long* ecount, int first, int Kc, int K, int D,
                                                                 int H, int W, int mid_is_h, int nbl, int64_t nh,
                                                                 const int* field, uint32_t* hist, uint32_t* gmax) {
  extern __shared__ uint32_t s_h[];                 // [Kc][2][nbl] small squared distances, then [Kc][2] maxima
  const int b = blockIdx.y, tid = threadIdx.x;
  uint32_t* s_max = s_h + (int64_t)Kc * 2 * nbl;
  for (int i = tid; i < Kc * 2 * nbl + Kc * 2; i += kThreads) s_h[i] = 0;
  __syncthreads();
  const int64_t V = (int64_t)D * H * W, HW = (int64_t)H * W;
  const uint32_t keep = (Kc + first >= 32 ? ~0u : ((1u << (Kc + first)) - 1)) & ~((1u << first) - 1);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + tid; v < V; v += stride) {
    const uint32_t e[2] = {pe[(int64_t)b * V + v] & keep, ge[(int64_t)b * V + v] & keep};
    if (!(e[0] | e[1])) continue;
    const int z = (int)(v / HW), y = (int)((v / W) % H);
    const int l = mid_is_h ? z : y;
    const int64_t sl = mid_is_h ? HW : W;
    for (int dir = 0; dir < 2; ++dir) {
      uint32_t bits = e[dir];
      while (bits) {
        const int c = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const int64_t bc = (int64_t)b * K + c;
        if (ecount[bc * 2 + (1 - dir)] == 0) continue;          // no target: +inf, decided by the finish
        const int* bx = boxes + bc * 6;
        const int l0 = mid_is_h ? bx[0] : bx[2], l1 = mid_is_h ? bx[1] : bx[3];
        const int sq = search_last(field + (bc * 2 + dir) * V + v, l, l0, l1, sl);
        if ((int64_t)sq >= nh) continue;                         // (unreachable with a target: keeps every store in bounds)
        const int slot = (c - first) * 2 + dir;
        if (sq < nbl) atomicAdd(&s_h[slot * nbl + sq], 1u);
        else atomicAdd(&hist[(bc * 2 + dir) * nh + sq], 1u);
        atomicMax(&s_max[slot], (uint32_t)sq);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < Kc * 2 * nbl; i += kThreads) {
    const uint32_t n = s_h[i];
    if (n) {
      const int slot = i / nbl, sq = i % nbl;
      const int64_t bc = (int64_t)b * K + first + slot / 2;
      atomicAdd(&hist[(bc * 2 + (slot & 1)) * nh + sq], n);
    }
  }
  for (int i = tid; i < Kc * 2; i += kThreads)
    if (s_max[i]) atomicMax(&gmax[((int64_t)b * K + first + i / 2) * 2 + (i & 1)], s_max[i]);
}

// ---- 7. finalize ---------------------------------------------------------------------------------------------------------
// The squared distance of rank r (0-based, ascending) in hist[0..nbins): each thread sums one contiguous segment, a block
// scan finds the segment that holds the rank, its thread walks it.
__device__ int64_t rank_value(const uint32_t* hist, int64_t nbins, int64_t r0, int64_t r1, int64_t* out1) {
  __shared__ unsigned long long s_pre[kThreads];
  __shared__ int64_t s_res[2];
  const int tid = threadIdx.x;
  const int64_t seg = (nbins + kThreads - 1) / kThreads;
  const int64_t a = tid * seg, e = min(a + seg, nbins);
  unsigned long long sum = 0;
  for (int64_t i = a; i < e; ++i) sum += hist[i];
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
  const unsigned long long pre = s_pre[tid];
  const int64_t rk[2] = {r0, r1};
  for (int k = 0; k < 2; ++k) {
    if ((unsigned long long)rk[k] >= pre && (unsigned long long)rk[k] < pre + sum) {
      unsigned long long run = pre;
      for (int64_t i = a; i < e; ++i) {
        run += hist[i];
        if ((unsigned long long)rk[k] < run) { s_res[k] = i; break; }
      }
    }
  }
  __syncthreads();
  const int64_t v0 = s_res[0];
  *out1 = s_res[1];
  __syncthreads();
  return v0;
}

// numpy's linear percentile of the n sorted distances sqrt(sq) (numpy.lib._function_base_impl._quantile / _lerp)
__device__ double directed_value(const uint32_t* hist, uint32_t gmax, int64_t n, double percentile) {
  if (percentile == 0.0 || n == 1) return __dsqrt_rn((double)gmax);
  const double vi = (double)(n - 1) * (percentile / 100.0);
  if (vi >= (double)(n - 1)) return __dsqrt_rn((double)gmax);
  const double lo = floor(vi);
  const double t = vi - lo;
  int64_t v1 = 0;
  const int64_t v0 = rank_value(hist, (int64_t)gmax + 1, (int64_t)lo, (int64_t)lo + 1, &v1);
  const double a = __dsqrt_rn((double)v0), bb = __dsqrt_rn((double)v1);
  const double diff = bb - a;
  return t >= 0.5 ? bb - diff * (1.0 - t) : a + diff * t;
}

__global__ __launch_bounds__(kThreads) void surf_finalize_kernel(const unsigned long long* ecount, const uint32_t* hist,
                                                                 const uint32_t* gmax, int first, int Kc, int K, int64_t nh,
                                                                 double percentile, int directed, float* out) {
  const int b = blockIdx.x / Kc, c = first + blockIdx.x % Kc;
  const int64_t bc = (int64_t)b * K + c;
  const int64_t n0 = (int64_t)ecount[bc * 2 + 0], n1 = (int64_t)ecount[bc * 2 + 1];
  double res;
  if (n0 == 0 && n1 == 0) {
    res = __builtin_nan("");
  } else if (n0 == 0 || n1 == 0) {
    res = __builtin_inf();
  } else {
    res = directed_value(hist + (bc * 2 + 0) * nh, gmax[bc * 2 + 0], n0, percentile);
    if (!directed) res = fmax(res, directed_value(hist + (bc * 2 + 1) * nh, gmax[bc * 2 + 1], n1, percentile));
  }
  if (threadIdx.x == 0) out[(int64_t)b * Kc + (c - first)] = (float)res;
}

__global__ __launch_bounds__(64) void surf_iou_kernel(const unsigned long long* counts, int first, int Kc, int K, int n,
                                                      int ignore_empty, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int b = i / Kc, c = first + i % Kc;
  const unsigned long long* C = counts + ((int64_t)b * K + c) * 3;
  const unsigned long long P = C[0], G = C[1], I = C[2], U = P + G - I;
  float r;
  if (ignore_empty && G == 0) r = __builtin_nanf("");
  else if (U == 0) r = 1.0f;
  else r = (float)((double)I / (double)U);      // exact for U < 2^27: one rounding of the true quotient
  out[i] = r;
}


bool percentile_ok(double p) { return p >= 0.0 && p <= 100.0; }     // (false for nan)

}  // namespace

extern "C" int64_t micf_surface_metrics_workspace(int B, int K, int D, int H, int W) {
  if (!shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (!shape_supported(K, D, H, W)) return MICF_EUNSUPPORTED;
  return layout(B, K, D, H, W).total;
}

extern "C" int64_t micf_mean_iou_workspace(int B, int K, int D, int H, int W) {
  if (!shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (K > 32) return MICF_EUNSUPPORTED;
  return align256(8 * (int64_t)B * K * 3);
}

extern "C" int micf_hausdorff_distance(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W,
                                       int first_class, double percentile, int directed, void* workspace,
                                       int64_t workspace_bytes, float* out, micf_stream_t stream) {
  if (!pred || !gt || !workspace || !out || !shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (form != MICF_FORM_LABEL && form != MICF_FORM_ONEHOT) return MICF_EINVAL;
  if (first_class < 0 || first_class >= K || !percentile_ok(percentile)) return MICF_EINVAL;
  if (!shape_supported(K, D, H, W)) return MICF_EUNSUPPORTED;
  const Layout L = layout(B, K, D, H, W);
  if (workspace_bytes < L.total || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MICF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  uint32_t *pm = (uint32_t*)(ws + L.pm), *gm = (uint32_t*)(ws + L.gm), *pe = (uint32_t*)(ws + L.pe), *ge = (uint32_t*)(ws + L.ge);
  auto* counts = (unsigned long long*)(ws + L.counts);
  auto* ecount = (unsigned long long*)(ws + L.ecount);
  uint32_t *proj = (uint32_t*)(ws + L.proj), *gmax = (uint32_t*)(ws + L.gmax), *hist = (uint32_t*)(ws + L.hist);
  int* boxes = (int*)(ws + L.boxes);
  int* field = (int*)(ws + L.field);
  const int Kc = K - first_class;
  const int64_t V = (int64_t)D * H * W;
  const int mid_is_h = H <= D ? 1 : 0;
  const int lmid = mid_is_h ? H : D, loth = mid_is_h ? D : H;

  if (hipMemsetAsync(ws + L.zero_begin, 0, L.zero_end - L.zero_begin, s) != hipSuccess) return MICF_ELAUNCH;
  int rc = classify(pred, gt, form == MICF_FORM_ONEHOT, true, B, K, D, H, W, pm, gm, counts, proj, s);
  if (rc) return rc;
  hipLaunchKernelGGL(surf_box_kernel, dim3(B), dim3(128), 0, s, proj, K, D, H, W, boxes);
  int64_t vb = (V + kThreads - 1) / kThreads;
  const int eblocks = (int)(vb < 2048 ? vb : 2048);
  hipLaunchKernelGGL(surf_edges_kernel, dim3(eblocks, B), dim3(kThreads), 0, s, pm, gm, boxes, K, D, H, W, pe, ge, ecount);
  const unsigned slots = (unsigned)(B * Kc * 2);
  hipLaunchKernelGGL(surf_edt_w_kernel, dim3((unsigned)(((int64_t)D * H + 3) / 4), slots), dim3(kThreads), 0, s, pe, ge, boxes,
                     ecount, first_class, Kc, K, D, H, W, field);
  const size_t lds_mid = (size_t)64 * lmid * sizeof(uint32_t);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&surf_edt_mid_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(kMaxMid * 64 * sizeof(uint32_t)));
  hipLaunchKernelGGL(surf_edt_mid_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)loth, slots), dim3(64), lds_mid, s, boxes,
                     ecount, first_class, Kc, K, D, H, W, mid_is_h, field);
  const int nbl = kLdsHist / (2 * Kc);
  const size_t lds_last = ((size_t)Kc * 2 * nbl + Kc * 2) * sizeof(uint32_t);
  const int lblocks = (int)(vb < 1024 ? vb : 1024);
  hipLaunchKernelGGL(surf_edt_last_kernel, dim3(lblocks, B), dim3(kThreads), lds_last, s, pe, ge, boxes, ecount, first_class, Kc,
                     K, D, H, W, mid_is_h, nbl, L.nh, field, hist, gmax);
  hipLaunchKernelGGL(surf_finalize_kernel, dim3((unsigned)(B * Kc)), dim3(kThreads), 0, s, ecount, hist, gmax, first_class, Kc, K,
                     L.nh, percentile, directed ? 1 : 0, out);
  MICF_RETURN_LAUNCH();
}

extern "C" int micf_mean_iou(const void* pred, const void* gt, int form, int B, int K, int D, int H, int W, int first_class,
                             int ignore_empty, void* workspace, int64_t workspace_bytes, float* out, micf_stream_t stream) {
  if (!pred || !gt || !workspace || !out || !shape_ok(B, K, D, H, W)) return MICF_EINVAL;
  if (form != MICF_FORM_LABEL && form != MICF_FORM_ONEHOT) return MICF_EINVAL;
  if (first_class < 0 || first_class >= K) return MICF_EINVAL;
  if (K > 32) return MICF_EUNSUPPORTED;
  const int64_t need = align256(8 * (int64_t)B * K * 3);
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MICF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  auto* counts = static_cast<unsigned long long*>(workspace);
  if (hipMemsetAsync(counts, 0, 8 * (size_t)B * K * 3, s) != hipSuccess) return MICF_ELAUNCH;
  int rc = classify(pred, gt, form == MICF_FORM_ONEHOT, false, B, K, D, H, W, nullptr, nullptr, counts, nullptr, s);
  if (rc) return rc;
  const int Kc = K - first_class, n = B * Kc;
  hipLaunchKernelGGL(surf_iou_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, counts, first_class, Kc, K, n,
                     ignore_empty ? 1 : 0, out);
  MICF_RETURN_LAUNCH();
}
