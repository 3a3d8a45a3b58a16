// conv3_wgradx.hip -- weight gradient of the 3x3x3 / pad 1 convolution with 16 output channels (conv_offset[0], MS.py:314)
// on the matrix cores, with the WHOLE gradient slab of a workgroup resident in accumulator registers.
//
//   dW[n][c][tap] = sum_t dy[t, n] * in[t + off(tap), c]                 in = [x1 | x2], n < 16
//
// MFMA rows i = 16 input channels, columns j = the 16 dy channels, k = tokens.  A workgroup owns a slab of 48 input channels x
// 27 taps = 81 (tap, channel tile) pairs -> 21 accumulator tiles (84 registers) in each of its 4 waves, an (h, w) footprint of 64
// tokens of one sample and a contiguous range of its d planes (conv3_wgrad_plan.h holds that split and is shared with the host).
// It MARCHES the range: the halo planes d - 1, d, d + 1 of the footprint sit in an LDS ring of three, a step commits the one new
// plane d + 1 ((TH + 2) x (TW + 2) voxel rows of the slab's 48 channels) over the slot of plane d - 2, and two register sets run
// ahead of the ring (planes d + 2 and d + 3 are in flight under the MFMAs of step d).  Planes -1 and D are zeros, a range never
// crosses a sample, a range that starts inside a sample primes two planes.  What a thread moves of every plane is the same, so its
// source addresses and LDS offsets are worked out once, before the march.  A tap is an offset on the centre voxel's address:
// in-plane part fixed, plane part = the ring slot of d + kd - 1, which is wave-uniform and changes per step.
//   * bf16 mode (the benched one, conv3_wgradx_b16_kernel): x and dy are rounded to bf16 (RNE) at the LDS write, token-major, and the
//     fragments -- 8 tokens of one channel per lane -- are read with the transposing ds_read_b64_tr_b16; dbias sums the unrounded dy.
//   * fp32 mode (the parity mode, conv3_wgradx_kernel): MFMA 16x16x4 fp32, voxel stride 52 floats, one 4-byte LDS read per MFMA.
// Partial slabs go to a workspace with coalesced 16-byte stores (the float4 of a lane re-ordered so that the 16 of one quad of dy
// channels are contiguous) and conv3_wgradx_reduce_kernel sums them in a fixed order and adds them into [N][Cin][27].
#include <cstdlib>
#include <mutex>

#include "common.h"
#include "conv3_wgrad_plan.h"
#include "gemm_dma.h"

namespace micf {

namespace wgp = micf_wgrad;

constexpr int wCS = wgp::kSlabChannels; // channels per slab (3 channel tiles)
constexpr int wDS = 20;                 // fp32 mode: LDS stride of a dy row (floats): the four lane groups' tokens are 80 floats = 16 banks apart
constexpr int wXS = 52;                 // fp32 mode: LDS voxel stride (floats): 4 * 52 = 208 = 16 (mod 64) -> the four k lanes hit disjoint banks
constexpr int wPairs = wgp::kPairs;     // 81 (tap, channel tile) pairs per slab
constexpr int wTPW = wgp::kTilesPerWave;   // 21 accumulator tiles per wave
constexpr int wRSB = 104;               // bf16 mode: bytes per halo voxel row: 48 bf16 + 8 pad (26 dwords: the 4 token rows of a read are bank-disjoint)
constexpr int wDYB = 40;                // bf16 mode: bytes per dy token row: 16 bf16 + 8 pad

constexpr int kWgxItems = wgp::kMaxItems;   // layers of one shape per launch (blockIdx.y): the two modalities' offset convs of every
                                            // depth slot a flush hands over (6 items at the six-slot stages)
struct WgxArgs {
  const float* dy[kWgxItems];           // channels-last [T, 16]
  const float* x1[kWgxItems]; const float* x2[kWgxItems];
  int c1, c2;
  float* ws;                            // wgp::slab_offset / wgp::bias_offset
  int want_bias;
  wgp::Plan plan;
};

typedef short s16x4x __attribute__((ext_vector_type(4)));
typedef unsigned u32x2w __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bf16x8 tr_pair(unsigned a0, unsigned a1) {
  const s16x4x lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4x*)(uintptr_t)a0);
  const s16x4x hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4x*)(uintptr_t)a1);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// LDS of one workgroup: the ring of 3 planes, then the dy rows of the step's 64 tokens
template <int TW, bool BF16>
constexpr int wgx_lds_bytes() {
  constexpr int PL = (64 / TW + 2) * (TW + 2);
  return BF16 ? 3 * PL * wRSB + 64 * wDYB : (int)sizeof(float) * (3 * PL * wXS + 64 * wDS);
}

// TW: footprint extent along w (16 or 8).  Footprint = 64/TW (h) x TW (w) = 64 tokens per plane.
template <int TW, bool BF16>
__device__ __forceinline__ void wgx_march(const WgxArgs& a, char* smem) {
  constexpr int TH = 64 / TW, HH = TH + 2, HW = TW + 2;
  constexpr int PL = HH * HW;                                          // voxel rows of one halo plane
  constexpr int ROWB = BF16 ? wRSB : wXS * (int)sizeof(float);         // bytes per voxel row
  constexpr int PLB = PL * ROWB;
  constexpr int NQ = PL * (wCS / 4);                                   // float4 of one plane
  constexpr int NB = (NQ + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lr = lane >> 4;
  const wgp::Unit un = wgp::decode(a.plan, blockIdx.x);
  const int item = blockIdx.y;
  const float* __restrict__ a_dy = a.dy[item];
  const float* __restrict__ a_x1 = a.x1[item];
  const float* __restrict__ a_x2 = a.x2[item];
  const int D = a.plan.D, H = a.plan.H, W = a.plan.W, Cin = a.c1 + a.c2;
  const int cbase = un.slab * wCS, h0 = un.h0, w0 = un.w0;
  const int64_t tok0 = (int64_t)un.b * D * H * W;                      // first token of the sample
  const unsigned xh = (unsigned)(uintptr_t)smem, dyl = xh + 3 * PLB;

  f32x4 acc[wTPW];
#pragma unroll
  for (int p = 0; p < wTPW; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (tap, channel tile) p of this wave: the in-plane part of its offset from the centre voxel (bytes).  Its plane kd is one of
  // two per wave: pairs run tap-major, so the wave's 21 pairs cross at most one multiple of 27.
  int offs[wTPW];
#pragma unroll
  for (int p = 0; p < wTPW; ++p) {
    const int pair = min(wave * wTPW + p, wPairs - 1);                  // the 3 surplus tiles of wave 3 recompute the last pair
    const int tap = pair / (wCS / 16), ct = pair % (wCS / 16);          // (never read back): no branch in the MFMA stream
    const int kh = (tap / 3) % 3, kw = tap % 3;
    offs[p] = ((kh - 1) * HW + (kw - 1)) * ROWB + ct * (BF16 ? 32 : 64);
  }
  const int kd_a = (wave * wTPW) / 27, kd_b = min(kd_a + 1, 2);
  const int kd_split = 27 * (kd_a + 1) - wave * wTPW;                   // pairs p < kd_split lie in plane kd_a, the others in kd_b

  // bf16: token t = 8 lr + 4 r + (li >> 2) of k-step ks (32 tokens = 32 / TW rows): its centre voxel row in a plane / its dy row
  unsigned abase[2][2], bbase[2][2];
  if constexpr (BF16) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int t = 8 * lr + 4 * r + (li >> 2);
        const int lh = ks * (32 / TW) + t / TW, lw = t % TW;
        abase[ks][r] = xh + (unsigned)(((lh + 1) * HW + lw + 1) * ROWB + 8 * (li & 3));
        bbase[ks][r] = dyl + (unsigned)((32 * ks + t) * wDYB + 8 * (li & 3));
      }
  }
  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);                         // column sums of dy (channels 4 (tid & 3) ..) over this thread's tokens

  // What thread tid moves of EVERY plane is fixed for the whole march, so its addresses are worked out once: float4 u is voxel row
  // hv = idx / 12 of the plane, channels cbase + 4 (idx % 12) .., idx = 256 u + tid.
  const float* fsrc[NB];                                               // its address in plane 0 of the sample; nullptr: zeros (h / w border, c >= Cin, idx >= NQ)
  int fstride[NB];                                                     // floats from one plane to the next in its source (x1 or x2)
  unsigned fdst[NB];                                                   // its byte offset in a ring slot
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int idx = u * 256 + tid;
    const int hv = idx / (wCS / 4), g = idx % (wCS / 4);
    const int yy = h0 + hv / HW - 1, ww = w0 + hv % HW - 1;
    const int c = cbase + 4 * g;
    const bool first = c < a.c1;
    const int cw = first ? a.c1 : a.c2;
    const bool ok = idx < NQ && (unsigned)yy < (unsigned)H && (unsigned)ww < (unsigned)W && c < Cin;
    fsrc[u] = ok ? (first ? a_x1 + c : a_x2 + (c - a.c1)) + (tok0 + (int64_t)yy * W + ww) * cw : nullptr;
    fstride[u] = H * W * cw;
    fdst[u] = (unsigned)(hv * ROWB + (BF16 ? 8 : 16) * g);
  }
  // plane dd of the footprint's halo -> registers (zeros for the planes -1 and D)
  auto fetch = [&](int dd, float4 (&v)[NB]) {
    const bool plane = (unsigned)dd < (unsigned)D;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (plane && fsrc[u]) v[u] = *reinterpret_cast<const float4*>(fsrc[u] + (int64_t)dd * fstride[u]);
    }
  };
  auto commit = [&](int slot, const float4 (&v)[NB]) {
    char* base = smem + slot * PLB;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (u * 256 + tid < NQ) {
        if constexpr (BF16) *reinterpret_cast<u32x2w*>(base + fdst[u]) = u32x2w{pack_bf16(v[u].x, v[u].y), pack_bf16(v[u].z, v[u].w)};
        else *reinterpret_cast<float4*>(base + fdst[u]) = v[u];
      }
    }
  };
  // dy of the 64 tokens of plane dd: thread tid holds channels 4 (tid & 3) .. of tile-local token tid >> 2 (= lh * TW + lw)
  const float* dsrc = nullptr;
  {
    const int tk = tid >> 2, yy = h0 + tk / TW, ww = w0 + tk % TW;
    if (yy < H && ww < W) dsrc = a_dy + (tok0 + (int64_t)yy * W + ww) * 16 + 4 * (tid & 3);
  }
  const int dstride = H * W * 16;
  auto fetch_dy = [&](int dd) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (dsrc) r = *reinterpret_cast<const float4*>(dsrc + (int64_t)dd * dstride);
    return r;
  };

  // ---- prime the ring with planes d0 - 1 and d0 (slot of plane d = d mod 3).  Two register sets run ahead of the ring: at step d
  // one holds plane d + 1 and dy(d), which the step commits, the other plane d + 2 and dy(d + 1), still in flight; the set just
  // committed is refilled with plane d + 3 and dy(d + 2).  All four fetches of the prologue are issued before the first wait.
  float4 va[NB], vb[NB], dya, dyb = make_float4(0.f, 0.f, 0.f, 0.f);
  int sc = un.d0 % 3;                                                  // slot of the centre plane d
  {
    float4 p0[NB], p1[NB];
    fetch(un.d0 - 1, p0);
    fetch(un.d0, p1);
    fetch(un.d0 + 1, va);
    dya = fetch_dy(un.d0);
    if (un.d0 + 1 < un.d1) {
      fetch(un.d0 + 2, vb);
      dyb = fetch_dy(un.d0 + 1);
    }
    commit(sc == 0 ? 2 : sc - 1, p0);
    commit(sc, p1);
  }
  auto step = [&](int d, float4 (&v)[NB], float4& vdy) {
    const int sp = sc == 0 ? 2 : sc - 1, sn = sc == 2 ? 0 : sc + 1;     // slots of planes d - 1 and d + 1
    __syncthreads();                                                   // step d - 1 fully consumed: slot sn (plane d - 2) and the dy rows are free
    commit(sn, v);
    if constexpr (BF16) *reinterpret_cast<u32x2w*>(smem + 3 * PLB + (tid >> 2) * wDYB + 8 * (tid & 3)) = u32x2w{pack_bf16(vdy.x, vdy.y), pack_bf16(vdy.z, vdy.w)};
    else *reinterpret_cast<float4*>(smem + 3 * PLB + ((tid >> 2) * wDS + 4 * (tid & 3)) * (int)sizeof(float)) = vdy;
    bs.x += vdy.x; bs.y += vdy.y; bs.z += vdy.z; bs.w += vdy.w;
    __syncthreads();
    // The set just committed is refilled under the MFMAs for the step after the next.  The MFMA phase itself issues no global
    // load (dy fragments come from LDS): loads return in order, one issued there would wait for the planes in flight.
    if (d + 2 < un.d1) {
      fetch(d + 3, v);
      vdy = fetch_dy(d + 2);
    }
    const int plane_a = (kd_a == 0 ? sp : kd_a == 1 ? sc : sn) * PLB, plane_b = (kd_b == 1 ? sc : sn) * PLB;   // ring slots of d + kd - 1

    if constexpr (BF16) {
      // 2 k-steps x 21 pairs in 6 batches of 7: the fragments of batch i + 1 are read while the MFMAs of batch i run (two
      // register sets; LDS reads return in order, so a batch waits only for its own)
      constexpr int G = 7, NBAT = 2 * (wTPW / G);
      static_assert(wTPW % G == 0 && NBAT % 2 == 0, "batches of G pairs, two sets");
      auto read_batch = [&](int bi, bf16x8 (&f)[G]) {
        const int ks = bi / (wTPW / G), p0 = (bi % (wTPW / G)) * G;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int o = offs[p0 + i] + (p0 + i < kd_split ? plane_a : plane_b);
          f[i] = tr_pair(abase[ks][0] + o, abase[ks][1] + o);
        }
      };
      const bf16x8 bb[2] = {tr_pair(bbase[0][0], bbase[0][1]), tr_pair(bbase[1][0], bbase[1][1])};
      auto mfma_batch = [&](int bi, const bf16x8 (&f)[G]) {
        const int ks = bi / (wTPW / G), p0 = (bi % (wTPW / G)) * G;
#pragma unroll
        for (int i = 0; i < G; ++i) acc[p0 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[i], bb[ks], acc[p0 + i], 0, 0, 0);
      };
      bf16x8 f0[G], f1[G];
      read_batch(0, f0);
#pragma unroll
      for (int bi = 0; bi < NBAT; bi += 2) {
        read_batch(bi + 1, f1);
        mfma_batch(bi, f0);
        if (bi + 2 < NBAT) read_batch(bi + 2, f0);
        mfma_batch(bi + 1, f1);
      }
    } else {
      constexpr int CH = 16 / TW;
      const float* Xs = reinterpret_cast<const float*>(smem);
      const float* Dys = reinterpret_cast<const float*>(smem + 3 * PLB);
      // dy fragment of a 16-token group (k-permutation: in step s lane group lr supplies token j = 4*lr + s of the group)
      auto load_dy = [&](int g, float (&bv)[4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) bv[s] = g < 4 ? Dys[(g * 16 + 4 * lr + s) * wDS + li] : 0.f;
      };
      float bv[4], bn[4];
      load_dy(0, bv);
      // ---- 4 token groups of 16 tokens
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {
        load_dy(g + 1, bn);
        int vox[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int j = 4 * lr + s;
          const int lh = g * CH + j / TW, lw = j % TW;
          vox[s] = ((lh + 1) * HW + lw + 1) * wXS + li;                // centre voxel of the token in a plane, + channel li
        }
        // s outer / pair inner: consecutive MFMAs hit different accumulators (no back-to-back dependency on one tile)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
          for (int p = 0; p < wTPW; ++p) {
            const int o = (offs[p] + (p < kd_split ? plane_a : plane_b)) >> 2;
            acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(Xs[vox[s] + o], bv[s], acc[p], 0, 0, 0);
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) bv[s] = bn[s];
      }
    }
    sc = sn;
  };
  for (int d = un.d0; d < un.d1; d += 2) {
    step(d, va, dya);
    if (d + 1 < un.d1) step(d + 1, vb, dyb);
  }
  // ---- partial slab -> workspace: chunk (wave*TPW + p) of 64 float4, lane (n = li, channel quad lr) at n-quad major position:
  // 16-byte stores, 1 KiB per wave instruction
  float* out = a.ws + wgp::slab_offset(a.plan, item, un.slab, un.part);
  const int pos = (li >> 2) * 16 + lr * 4 + (li & 3);
#pragma unroll
  for (int p = 0; p < wTPW; ++p)
    *reinterpret_cast<float4*>(out + ((wave * wTPW + p) * 64 + pos) * 4) = make_float4(acc[p][0], acc[p][1], acc[p][2], acc[p][3]);
  if (a.want_bias && un.slab == 0) {                                   // column sums of dy: over the lanes of one channel quad, then the waves
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) {
      bs.x += __shfl_xor(bs.x, m, 64); bs.y += __shfl_xor(bs.y, m, 64); bs.z += __shfl_xor(bs.z, m, 64); bs.w += __shfl_xor(bs.w, m, 64);
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    if (lane < 4) *reinterpret_cast<float4*>(red + (wave * 4 + lane) * 4) = bs;
    __syncthreads();
    if (tid < 16) a.ws[wgp::bias_offset(a.plan, item, un.part) + tid] = red[tid] + red[16 + tid] + red[32 + tid] + red[48 + tid];
  }
}

template <int TW>
__global__ void __launch_bounds__(256) conv3_wgradx_kernel(WgxArgs a) {
  extern __shared__ __attribute__((aligned(16))) char wgx_smem[];
  wgx_march<TW, false>(a, wgx_smem);
}

template <int TW>
__global__ void __launch_bounds__(256, 2) conv3_wgradx_b16_kernel(WgxArgs a) {   // two workgroups per CU: at most 256 registers
  extern __shared__ __attribute__((aligned(16))) char wgx_smem[];
  wgx_march<TW, true>(a, wgx_smem);
}

// dw[n][c][tap] += sum over the parts' partial slabs;  dbias[n] += sum of the parts' column sums.  No atomics, one owner per
// element and a fixed order of summation (part 0, 1, 2, ... in one thread): two runs are bit-identical.
// A block owns, of one (item, slab, channel tile), a quad of dy channels: per (part, tap) 16 consecutive float4 of the slab (the
// marching kernel stores them n-quad major), 27 x 16 = 432 columns, one per thread.  A thread streams its column over the parts
// with up to 16 independent 16-byte loads in flight and no exchange with any other thread; the sums are then turned through LDS
// into the block's [4 n][16 c][27 taps] -- per n one contiguous run of 432 floats of dw -- which is read, added and written back
// in address order.
struct WgxOut { float* dw[kWgxItems]; float* dbias[kWgxItems]; };
constexpr int kReduceThreads = 448;                                    // 7 waves: 432 columns
__global__ void __launch_bounds__(kReduceThreads) conv3_wgradx_reduce_kernel(const float* __restrict__ ws, WgxOut o, int want_bias, wgp::Plan plan) {
  __shared__ float4 red[27][16];
  const int tid = threadIdx.x;
  const int item = blockIdx.y;
  int q = blockIdx.x;
  const int nq = q % 4; q /= 4;
  const int ct = q % (wCS / 16);
  const int slab = q / (wCS / 16);
  const int parts = plan.parts, Cin = plan.Cin;
  if (tid < 27 * 16) {
    const int tap = tid >> 4, col = tid & 15;
    constexpr int64_t STEP = wgp::kSlabFloats / 4;                     // float4 between the slabs of consecutive parts
    const float4* __restrict__ src = reinterpret_cast<const float4*>(ws + wgp::slab_offset(plan, item, slab, 0)) + ((tap * (wCS / 16) + ct) * 64 + nq * 16 + col);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int part = 0;
#pragma unroll 1
    for (; part + 16 <= parts; part += 16) {
      float4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = src[(part + u) * STEP];
#pragma unroll
      for (int u = 0; u < 16; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
#pragma unroll 1
    for (; part + 8 <= parts; part += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(part + u) * STEP];
#pragma unroll
      for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
    for (; part < parts; ++part) {
      const float4 v = src[part * STEP];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    red[tap][col] = acc;
  }
  __syncthreads();
  float* __restrict__ dw = o.dw[item];
  const int c0 = slab * wCS + ct * 16;                                  // first of the block's 16 channels
  const float* redf = reinterpret_cast<const float*>(&red[0][0]);
  for (int e = tid; e < 4 * 16 * 27; e += kReduceThreads) {             // e = (j * 16 + cc) * 27 + tap: address order within the run of n = 4 nq + j
    const int j = e / (16 * 27), rem = e % (16 * 27);
    const int cc = rem / 27, tap = rem % 27;
    if (c0 + cc < Cin) dw[((int64_t)(nq * 4 + j) * Cin + c0 + cc) * 27 + tap] += redf[((tap * 16) + (cc >> 2) * 4 + j) * 4 + (cc & 3)];
  }
  float* __restrict__ dbias = o.dbias[item];
  if (want_bias && dbias && slab == 0 && ct == 0 && tid < 64) {         // dbias of the block's n quad: lane = n x 16 part slices
    const float* __restrict__ b = ws + wgp::bias_offset(plan, item, 0) + nq * 4 + (tid & 3);
    float s = 0.f;
    for (int part = tid >> 2; part < parts; part += 16) s += b[(int64_t)part * 16];
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    if (tid < 4) dbias[nq * 4 + tid] += s;
  }
}

int64_t conv3_wgradx_workspace(int B, int D, int H, int W, int N, int c1, int c2, int items) {
  if (N != 16 || W < 4 || (c1 & 3) || (c2 & 3) || c1 + c2 <= 0 || items < 1 || items > kWgxItems) return 0;   // (W = 4: masked 8-wide footprints)
  return wgp::workspace_floats(wgp::make_plan(B, D, H, W, c1 + c2, items));
}

// MICF_EUNSUPPORTED when the shape / workspace is outside what this kernel covers (caller falls back).
// n items of ONE shape per launch (blockIdx.y): dy / x1 / x2 / dw / dbias per item.
int conv3_wgradx_items(const float* const* dy, const float* const* x1, const float* const* x2, float* const* dw, float* const* dbias,
                       int n, int c1, int c2, int B, int D, int H, int W, int N, float* ws, int64_t ws_floats, hipStream_t stream,
                       int dtype) {
  const int64_t need = conv3_wgradx_workspace(B, D, H, W, N, c1, c2, n);
  if (need == 0 || !ws || ws_floats < need || !aligned16(ws)) return MICF_EUNSUPPORTED;
  WgxArgs a{};
  WgxOut o{};
  a.plan = wgp::make_plan(B, D, H, W, c1 + c2, n);
  const wgp::Plan& p = a.plan;
  const int cmax = c1 > c2 ? c1 : c2;
  if ((int64_t)p.slabs * p.parts > 0x7fffffffll || (int64_t)H * W * (cmax > 16 ? cmax : 16) > 0x7fffffffll) return MICF_EUNSUPPORTED;   // (plane strides are ints)
  bool any_bias = false;
  for (int i = 0; i < n; ++i) {
    if (!dy[i] || !x1[i] || !dw[i] || !aligned16(dy[i]) || !aligned16(x1[i]) || (x2 && x2[i] && !aligned16(x2[i]))) return MICF_EUNSUPPORTED;
    a.dy[i] = dy[i]; a.x1[i] = x1[i]; a.x2[i] = (x2 && x2[i]) ? x2[i] : x1[i];
    o.dw[i] = dw[i]; o.dbias[i] = dbias ? dbias[i] : nullptr;
    any_bias = any_bias || o.dbias[i];
  }
  a.c1 = c1; a.c2 = c2;
  a.ws = ws; a.want_bias = any_bias ? 1 : 0;
  static std::once_flag attr_once;       // > 64 KiB of dynamic LDS needs the opt-in once per process
  std::call_once(attr_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_wgradx_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_wgradx_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
  });
  const dim3 grid(wgp::grid_x(p), n);
  const bool b16 = dtype == MICF_DTYPE_BF16;
  if (p.tw == 16) {
    if (b16) hipLaunchKernelGGL((conv3_wgradx_b16_kernel<16>), grid, dim3(256), (wgx_lds_bytes<16, true>()), stream, a);
    else hipLaunchKernelGGL((conv3_wgradx_kernel<16>), grid, dim3(256), (wgx_lds_bytes<16, false>()), stream, a);
  } else {
    if (b16) hipLaunchKernelGGL((conv3_wgradx_b16_kernel<8>), grid, dim3(256), (wgx_lds_bytes<8, true>()), stream, a);
    else hipLaunchKernelGGL((conv3_wgradx_kernel<8>), grid, dim3(256), (wgx_lds_bytes<8, false>()), stream, a);
  }
  if (hipGetLastError() != hipSuccess) return MICF_ELAUNCH;
  hipLaunchKernelGGL(conv3_wgradx_reduce_kernel, dim3(p.slabs * (wCS / 16) * 4, n), dim3(kReduceThreads), 0, stream, ws, o, a.want_bias, p);
  return hipGetLastError() == hipSuccess ? MICF_OK : MICF_ELAUNCH;
}

int conv3_wgradx(const float* dy, const float* x1, int c1, const float* x2, int c2, float* dw, float* dbias, int B, int D, int H,
                 int W, int N, float* ws, int64_t ws_floats, hipStream_t stream, int dtype) {
  return conv3_wgradx_items(&dy, &x1, &x2, &dw, &dbias, 1, c1, c2, B, D, H, W, N, ws, ws_floats, stream, dtype);
}

}  // namespace micf
