// volume_normalise_stats.h -- the statistics passes of the loader's normalisations (min / max, moments, radix select, finish) and the
// per-channel normaliser of the resize, and the host side that volume_normalise.hip and volume_affine.hip share: their common
// argument checks, the view of the workspace and the driver of a call (run_stats_loader), which each of the two hands its own
// resample step.  volume_normalise.hip has the launch plan and the rules.  Unnamed namespace: each including file gets its own copy.
#pragma once
#include "volume_loader_common.h"
#include "../../include/micformer_normalise.h"

namespace {

constexpr int kBins = 2048;                 // 11-bit digits: 8 KB of LDS per histogram, four histograms (one per rank) per block
constexpr int kRanks = 4;
constexpr int kMaxPartials = 1024;          // = the most blocks of a pass (pass_blocks)
constexpr uint32_t kKeyZero = 0x80000000u;  // key of +0.0f and of int16 0 << 16: the positive voxels are the keys above it

// digit `pass` of a 32-bit key: bits [shift, shift + width)
__host__ __device__ constexpr int digit_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int digit_width(int pass) { return pass == 2 ? 10 : 11; }

struct ChanRec {                            // one per (sample, channel)
  uint32_t keys[2];                         // min-max: max key, max ~key, copied by the finish from the loader-format words
  uint32_t prefix[kRanks], rank[kRanks], slot[kRanks];   // select: digits found so far, rank inside them, histogram the rank reads
  unsigned long long n;                     // z-score int16: voxels != 0; percentile: voxels > 0
  unsigned long long sum, sumsq;            // z-score int16 (sum is a two's-complement int64)
  float a, b;                               // what the resize reads: (mean, std) or (low, high) rounded to fp32
  int mode, pad;                            // MICF_NORM_* of the channel
  double stat[2];
};
struct SampleRec { ChanRec c[2]; uint32_t ext[6]; uint32_t pad[2]; };
struct Mom { double n, mean, m2; };         // count, mean, sum of squared deviations

// [loader-format words: B x kWsWords][records][histograms][partial moments]
struct Layout { int64_t recs, hist, partials, total, zero_words; };
Layout layout(int B) {
  Layout L;
  L.recs = align256((int64_t)B * kWsWords * 4);
  L.hist = L.recs + align256((int64_t)B * sizeof(SampleRec));
  L.partials = L.hist + (int64_t)B * 2 * kRanks * kBins * 4;
  L.total = align256(L.partials + (int64_t)B * 2 * kMaxPartials * sizeof(Mom));
  L.zero_words = L.partials / 4;
  return L;
}

struct Modes { int m[2]; };

// ---- 0. zero: loader_zero_kernel (volume_loader_common.h) over L.zero_words ------------------------------------------------------

// ---- 1. min / max ---------------------------------------------------------------------------------------------------------------
// grid (blocks, volumes of the chunk) for every statistics kernel; volume y is channel y & 1 of sample y >> 1.
__global__ __launch_bounds__(kThreads) void norm_minmax_kernel(MinMaxArgs a, Modes md, uint32_t* words) {
  __shared__ uint32_t s_red[2 * kWaves];
  if (md.m[blockIdx.y & 1] != MICF_NORM_MINMAX) return;
  minmax_body(a.v[blockIdx.y], words + (size_t)(blockIdx.y >> 1) * kWsWords + 2 * (blockIdx.y & 1), s_red);
}

// ---- 2. moments -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Mom merge(const Mom& a, const Mom& b) {
  const double n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
  Mom r{n, a.mean + d * f, a.m2 + b.m2 + d * d * (a.n * f)};
  if (b.n == 0.0) r = a;
  if (a.n == 0.0) r = b;
  return r;
}

__device__ __forceinline__ Mom wave_merge(Mom m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Mom t;
    t.n = __shfl_down(m.n, o, 64);
    t.mean = __shfl_down(m.mean, o, 64);
    t.m2 = __shfl_down(m.m2, o, 64);
    m = merge(m, t);                                             // (lane 0's tree is complete; the other lanes' values are unused)
  }
  return m;
}

__device__ __forceinline__ unsigned long long wave_add64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void norm_moments_kernel(MinMaxArgs a, Modes md, SampleRec* recs, Mom* partials) {
  __shared__ unsigned long long s_int[3 * kWaves];
  __shared__ Mom s_mom[kWaves];
  if (md.m[blockIdx.y & 1] != MICF_NORM_ZSCORE) return;
  const RawVol& vol = a.v[blockIdx.y];
  const bool f32 = vol.dtype == MICF_LOADER_F32;
  const int es = f32 ? 4 : 2;
  const unsigned nblk = pass_blocks(vol.n * es);                 // of this volume alone: its partition does not depend on the batch
  if (blockIdx.x >= nblk) return;
  const int tid = threadIdx.x;
  const VecSpan sp = vec_span(vol.p, vol.n, es);
  const int64_t g0 = (int64_t)blockIdx.x * kThreads + tid, gs = (int64_t)nblk * kThreads;
  if (f32) {
    const float* src = static_cast<const float*>(vol.p);
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    uint32_t cnt = 0;
    auto take = [&](float x) {
      if (x != 0.0f) {                                           // (-0.0f is zero)
        if (cnt == 0) c = (double)x;
        const double d = (double)x - c;
        s1 += d;
        s2 = fma(d, d, s2);
        ++cnt;
      }
    };
    for_each_vec(sp, g0, gs, [&](const uint4& q) {
      take(__uint_as_float(q.x)); take(__uint_as_float(q.y)); take(__uint_as_float(q.z)); take(__uint_as_float(q.w));
    });
    if (blockIdx.x == 0 && tid < sp.nscalar) take(src[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)]);
    Mom m{0.0, 0.0, 0.0};
    if (cnt) {
      const double n = (double)cnt, mu = s1 / n;
      m = Mom{n, c + mu, fmax(s2 - s1 * mu, 0.0)};
    }
    m = wave_merge(m);
    if ((tid & 63) == 0) s_mom[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      Mom r = s_mom[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) r = merge(r, s_mom[w]);
      partials[(size_t)blockIdx.y * kMaxPartials + blockIdx.x] = r;
    }
  } else {
    const int16_t* src = static_cast<const int16_t*>(vol.p);
    unsigned long long cnt = 0, s2 = 0;
    long long s1 = 0;
    auto take = [&](int x) {
      cnt += x != 0;
      s1 += x;
      s2 += (unsigned long long)((long long)x * x);
    };
    for_each_vec(sp, g0, gs, [&](const uint4& q) {
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) { take((int)(int16_t)(w[j] & 0xFFFFu)); take((int)(int16_t)(w[j] >> 16)); }
    });
    if (blockIdx.x == 0 && tid < sp.nscalar) take((int)src[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)]);
    cnt = wave_add64(cnt);
    const unsigned long long u1 = wave_add64((unsigned long long)s1);
    s2 = wave_add64(s2);
    if ((tid & 63) == 0) { s_int[tid >> 6] = cnt; s_int[kWaves + (tid >> 6)] = u1; s_int[2 * kWaves + (tid >> 6)] = s2; }
    __syncthreads();
    if (tid < 3) {
      unsigned long long r = s_int[tid * kWaves];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) r += s_int[tid * kWaves + w];
      ChanRec& rec = recs[blockIdx.y >> 1].c[blockIdx.y & 1];
      atomicAdd(tid == 0 ? &rec.n : (tid == 1 ? &rec.sum : &rec.sumsq), r);
    }
  }
}

// ---- 3. radix select --------------------------------------------------------------------------------------------------------------
// hist: [volume][kRanks][kBins] counts.  Pass 0 fills histogram 0 alone (every rank has the empty prefix).
__global__ __launch_bounds__(kThreads) void norm_hist_kernel(MinMaxArgs a, Modes md, int pass, const SampleRec* recs,
                                                             uint32_t* hist) {
  __shared__ uint32_t s_h[kRanks * kBins];
  if (md.m[blockIdx.y & 1] != MICF_NORM_PERCENTILE) return;
  const RawVol& vol = a.v[blockIdx.y];
  const bool f32 = vol.dtype == MICF_LOADER_F32;
  if (pass == 2 && !f32) return;                                 // an int16 key has no third digit
  const int es = f32 ? 4 : 2;
  const unsigned nblk = pass_blocks(vol.n * es);
  if (blockIdx.x >= nblk) return;
  const int tid = threadIdx.x;
  const ChanRec& rec = recs[blockIdx.y >> 1].c[blockIdx.y & 1];
  const int used = pass == 0 ? kBins : kRanks * kBins;
  for (int i = tid; i < used; i += kThreads) s_h[i] = 0;
  uint32_t pre[kRanks];
  bool own[kRanks];
#pragma unroll
  for (int r = 0; r < kRanks; ++r) {
    pre[r] = rec.prefix[r];
    own[r] = pass > 0 && rec.slot[r] == (uint32_t)r;             // the first of the ranks that share a prefix counts for all of them
  }
  __syncthreads();
  const int shift = digit_shift(pass), up = shift + digit_width(pass);
  const uint32_t mask = (1u << digit_width(pass)) - 1;
  auto add = [&](uint32_t key) {
    if (key > kKeyZero) {
      if (pass == 0) {
        atomicAdd(&s_h[key >> 21], 1u);
      } else {
        const uint32_t top = key >> up, d = (key >> shift) & mask;
#pragma unroll
        for (int r = 0; r < kRanks; ++r)
          if (own[r] && top == pre[r]) atomicAdd(&s_h[r * kBins + d], 1u);
      }
    }
  };
  const VecSpan sp = vec_span(vol.p, vol.n, es);
  const int64_t g0 = (int64_t)blockIdx.x * kThreads + tid, gs = (int64_t)nblk * kThreads;
  if (f32) {
    for_each_vec(sp, g0, gs, [&](const uint4& q) {
      add(key_f32(__uint_as_float(q.x))); add(key_f32(__uint_as_float(q.y)));
      add(key_f32(__uint_as_float(q.z))); add(key_f32(__uint_as_float(q.w)));
    });
    if (blockIdx.x == 0 && tid < sp.nscalar)
      add(key_f32(static_cast<const float*>(vol.p)[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)]));
  } else {
    for_each_vec(sp, g0, gs, [&](const uint4& q) {
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        add(key_i16((int)(int16_t)(w[j] & 0xFFFFu)) << 16);
        add(key_i16((int)(int16_t)(w[j] >> 16)) << 16);
      }
    });
    if (blockIdx.x == 0 && tid < sp.nscalar)
      add(key_i16((int)static_cast<const int16_t*>(vol.p)[tid < sp.head ? tid : sp.tail0 + (tid - sp.head)]) << 16);
  }
  __syncthreads();
  uint32_t* g = hist + (size_t)blockIdx.y * kRanks * kBins;
  for (int i = tid; i < used; i += kThreads)
    if (s_h[i]) atomicAdd(g + i, s_h[i]);
}

// numpy's "linear" method: the two order statistics of percentile p among n sorted values and the weight of the upper one
__device__ __forceinline__ void virtual_index(int64_t n, double p, int64_t& k0, int64_t& k1, double& t) {
#pragma clang fp contract(off)
  const double h = (double)(n - 1) * (p / 100.0);
  if (h >= (double)(n - 1)) {
    k0 = k1 = n - 1;
    t = 0.0;
  } else {
    const double fl = floor(h);
    k0 = (int64_t)fl;
    k1 = k0 + 1;
    t = h - fl;
  }
}

// grid (volumes of the chunk).  After pass p the prefix of a rank is its key >> digit_shift(p).
__global__ __launch_bounds__(kThreads) void norm_scan_kernel(MinMaxArgs a, Modes md, int pass, double p_low, double p_high,
                                                             SampleRec* recs, uint32_t* hist) {
  __shared__ uint32_t s_wave[kWaves], s_new[2 * kRanks];
  if (md.m[blockIdx.x & 1] != MICF_NORM_PERCENTILE) return;
  if (pass == 2 && a.v[blockIdx.x].dtype != MICF_LOADER_F32) return;
  constexpr int kSeg = kBins / kThreads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ChanRec& rec = recs[blockIdx.x >> 1].c[blockIdx.x & 1];
  uint32_t* h = hist + (size_t)blockIdx.x * kRanks * kBins;
  uint32_t rank[kRanks], slot[kRanks], pre[kRanks];
#pragma unroll
  for (int r = 0; r < kRanks; ++r) {
    rank[r] = rec.rank[r];
    slot[r] = pass == 0 ? 0 : rec.slot[r];
    pre[r] = pass == 0 ? 0 : rec.prefix[r];
  }
  if (tid < 2 * kRanks) s_new[tid] = 0;
  uint32_t mine[kSeg], sum = 0, excl = 0, n = 0;
  for (int r = 0; r < kRanks; ++r) {
    if (r == 0 || pass > 0) {                                    // (pass 0: one histogram serves the four ranks)
      sum = 0;
#pragma unroll
      for (int i = 0; i < kSeg; ++i) {
        mine[i] = h[slot[r] * kBins + tid * kSeg + i];
        sum += mine[i];
      }
      uint32_t inc = sum;                                        // inclusive scan over the lanes, then over the waves
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
      }
      __syncthreads();                                           // (the previous round's s_wave has been read)
      if (lane == 63) s_wave[wave] = inc;
      __syncthreads();
      uint32_t base = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        base += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
      }
      excl = base + inc - sum;
      if (pass == 0) {                                           // the count of positive voxels, and from it the four ranks
        n = total;
        int64_t k0 = 0, k1 = 0;
        double t;
        if (n) virtual_index((int64_t)n, p_low, k0, k1, t);
        rank[0] = (uint32_t)k0; rank[1] = (uint32_t)k1;
        k0 = k1 = 0;
        if (n) virtual_index((int64_t)n, p_high, k0, k1, t);
        rank[2] = (uint32_t)k0; rank[3] = (uint32_t)k1;
      }
    }
    if (rank[r] >= excl && rank[r] - excl < sum) {               // exactly one thread (none when the volume has no positive voxel)
      uint32_t run = excl;
#pragma unroll
      for (int i = 0; i < kSeg; ++i) {
        if (rank[r] >= run && rank[r] - run < mine[i]) {
          s_new[r] = (uint32_t)(tid * kSeg + i);
          s_new[kRanks + r] = rank[r] - run;
        }
        run += mine[i];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kRanks * kBins; i += kThreads) h[i] = 0;  // clear for the next pass (and for the next call's zeroing-free reuse)
  if (tid == 0) {
    uint32_t np[kRanks];
    for (int r = 0; r < kRanks; ++r) {
      np[r] = (pre[r] << digit_width(pass)) | s_new[r];
      uint32_t sl = (uint32_t)r;
      for (int q = r - 1; q >= 0; --q)
        if (np[q] == np[r]) sl = (uint32_t)q;
      rec.prefix[r] = np[r];
      rec.rank[r] = s_new[kRanks + r];
      rec.slot[r] = sl;
    }
    if (pass == 0) rec.n = n;
  }
}

// ---- 4. finish ------------------------------------------------------------------------------------------------------------------
// numpy's _lerp
__device__ __forceinline__ double lerp(double a, double b, double t) {
#pragma clang fp contract(off)
  const double diff = b - a;
  return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

// grid (volumes of the chunk), one wave each.  stats: [sample of the chunk][2][2] or NULL.
__global__ __launch_bounds__(64) void norm_finish_kernel(MinMaxArgs a, Modes md, double p_low, double p_high,
                                                         const uint32_t* words, SampleRec* recs, const Mom* partials,
                                                         double* stats) {
  const RawVol& vol = a.v[blockIdx.x];
  const bool f32 = vol.dtype == MICF_LOADER_F32;
  const int mode = md.m[blockIdx.x & 1], lane = threadIdx.x;
  ChanRec& rec = recs[blockIdx.x >> 1].c[blockIdx.x & 1];
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double s0 = nan, s1 = nan;
  if (mode == MICF_NORM_ZSCORE && f32) {
    const int nblk = (int)pass_blocks(vol.n * 4);
    const Mom* P = partials + (size_t)blockIdx.x * kMaxPartials;
    Mom m{0.0, 0.0, 0.0};
    for (int i = lane; i < nblk; i += 64) m = merge(m, P[i]);
    m = wave_merge(m);
    if (m.n > 0.0) {
      s0 = m.mean;
      s1 = __dsqrt_rn(m.m2 / m.n);
    }
  }
  if (lane != 0) return;
  if (mode == MICF_NORM_MINMAX) {
    const uint32_t* k = words + (size_t)(blockIdx.x >> 1) * kWsWords + 2 * (blockIdx.x & 1);
    rec.keys[0] = k[0];
    rec.keys[1] = k[1];
    const uint32_t kmax = k[0], kmin = ~k[1];
    s0 = f32 ? (double)unkey_f32(kmin) : (double)unkey_i16(kmin);
    s1 = f32 ? (double)unkey_f32(kmax) : (double)unkey_i16(kmax);
  } else if (mode == MICF_NORM_ZSCORE && !f32) {
    // n sumsq - sum^2 >= 0 in 128 bits (n < 2^31, sumsq < 2^61, |sum| < 2^46), exactly; variance = that / n^2
    const unsigned long long n = rec.n, sq = rec.sumsq;
    const long long sm = (long long)rec.sum;
    if (n) {
      const unsigned long long as = (unsigned long long)(sm < 0 ? -sm : sm);
      const unsigned long long alo = n * sq, ahi = __umul64hi(n, sq), blo = as * as, bhi = __umul64hi(as, as);
      const unsigned long long lo = alo - blo, hi = ahi - bhi - (alo < blo ? 1ull : 0ull);
      const double num = (double)hi * 18446744073709551616.0 + (double)lo;
      s0 = (double)sm / (double)n;
      s1 = __dsqrt_rn(num / (double)n / (double)n);
    }
  } else if (mode == MICF_NORM_PERCENTILE) {
    const int64_t n = (int64_t)rec.n;
    if (n) {
      double v[kRanks];
#pragma unroll
      for (int r = 0; r < kRanks; ++r)                          // (an int16 select stops after two digits: prefix = key >> 10)
        v[r] = f32 ? (double)unkey_f32(rec.prefix[r]) : (double)unkey_i16(rec.prefix[r] >> 6);
      int64_t k0, k1;
      double t;
      virtual_index(n, p_low, k0, k1, t);
      s0 = lerp(v[0], v[1], t);
      virtual_index(n, p_high, k0, k1, t);
      s1 = lerp(v[2], v[3], t);
    }
  }
  rec.stat[0] = s0;
  rec.stat[1] = s1;
  rec.a = (float)s0;
  rec.b = (float)s1;
  rec.mode = mode;
  if (stats) {
    stats[(size_t)blockIdx.x * 2] = s0;
    stats[(size_t)blockIdx.x * 2 + 1] = s1;
  }
}

// ---- 5. resize --------------------------------------------------------------------------------------------------------------------
// The normaliser of one channel: one raw element -> its normalised fp32 value (micformer_normalise.h has the three rules).
struct NormAny { int mode; Norm mm; float a, b, scale; };

// the z-score and percentile-clip rules on a value already in fp32
__device__ __forceinline__ float norm_f32(float x, const NormAny& nm) {
  if (nm.mode == MICF_NORM_ZSCORE) return x != 0.0f ? (x - nm.a) / nm.b : 0.0f;
  return (fminf(fmaxf(x, nm.a), nm.b) - nm.a) / nm.scale;             // numpy.clip = minimum(maximum(x, low), high)
}

// one raw int16 element already in a register (the patch crop unpacks eight of them from two vector loads)
__device__ __forceinline__ float norm_i16(int x, const NormAny& nm) {
  if (nm.mode == MICF_NORM_MINMAX) return (float)(x - nm.mm.imin) / nm.mm.scale;     // tap<false>(.., Norm)'s expression
  return norm_f32((float)x, nm);
}

template <bool F32>
__device__ __forceinline__ float tap(const void* p, int64_t off, const NormAny& nm) {
  if constexpr (!F32) return norm_i16((int)static_cast<const int16_t*>(p)[off], nm);
  else if (nm.mode == MICF_NORM_MINMAX) return tap<true>(p, off, nm.mm);     // (feeds the crop extents only: see the launch plan)
  else return norm_f32(static_cast<const float*>(p)[off], nm);
}

struct NormWords {
  typedef SampleRec Ws;
  static __device__ __forceinline__ SampleRec* sample(SampleRec* recs) { return recs + blockIdx.y; }
  static __device__ __forceinline__ NormAny norm(const SampleRec* rec, int c, bool f32) {
    const ChanRec& ch = rec->c[c];
    NormAny nm;
    nm.mode = ch.mode;
    nm.mm = load_norm(ch.keys, f32);
    nm.a = ch.a;
    nm.b = ch.b;
    nm.scale = ch.b - ch.a;                                        // fp32 subtract, as numpy on the clipped float32 array
    return nm;
  }
  static __device__ __forceinline__ bool stores(const SampleRec* rec, int c) { return rec->c[c].mode != MICF_NORM_MINMAX; }
  static __device__ __forceinline__ uint32_t* ext(SampleRec* rec) { return rec->ext; }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline bool valid_mode(int m) { return m == MICF_NORM_MINMAX || m == MICF_NORM_ZSCORE || m == MICF_NORM_PERCENTILE; }

// What micf_volume_loader_norm and micf_volume_loader_affine check in front of check_call.
inline int check_norm_args(int ct_mode, int mr_mode, double p_low, double p_high, const double* stats) {
  if (!valid_mode(ct_mode) || !valid_mode(mr_mode)) return MICF_EINVAL;
  if (!(0.0 <= p_low && p_low < p_high && p_high <= 100.0)) return MICF_EINVAL;      // (false for NaN)
  if (reinterpret_cast<uintptr_t>(stats) & 7) return MICF_EINVAL;
  return MICF_OK;
}

// The workspace as layout(B) carves it, and the call's optional `stats`; chunk(b0): the same from sample b0 on.
struct WsView {
  uint32_t* words;
  SampleRec* recs;
  uint32_t* hist;
  Mom* partials;
  double* stats;
  WsView chunk(int b0) const {
    return WsView{words + (size_t)b0 * kWsWords, recs + b0, hist + (size_t)b0 * 2 * kRanks * kBins,
                  partials + (size_t)b0 * 2 * kMaxPartials, stats ? stats + (size_t)b0 * 4 : nullptr};
  }
};
inline WsView ws_view(void* workspace, const Layout& L, double* stats) {
  char* ws = static_cast<char*>(workspace);
  return WsView{reinterpret_cast<uint32_t*>(ws), reinterpret_cast<SampleRec*>(ws + L.recs), reinterpret_cast<uint32_t*>(ws + L.hist),
                reinterpret_cast<Mom*>(ws + L.partials), stats};
}

// The statistics launches of one chunk of `nb` samples (steps 1-4 of the launch plan) on the chunk's view of the workspace.
inline void launch_statistics(hipStream_t s, const MinMaxArgs& ma, const Modes& md, int nb, unsigned blocks, double p_low,
                              double p_high, const WsView& c) {
  const dim3 grid(blocks, (unsigned)(2 * nb)), vols((unsigned)(2 * nb));
  const bool any_minmax = md.m[0] == MICF_NORM_MINMAX || md.m[1] == MICF_NORM_MINMAX;
  const bool any_zscore = md.m[0] == MICF_NORM_ZSCORE || md.m[1] == MICF_NORM_ZSCORE;
  const bool any_pct = md.m[0] == MICF_NORM_PERCENTILE || md.m[1] == MICF_NORM_PERCENTILE;
  if (any_minmax) hipLaunchKernelGGL(norm_minmax_kernel, grid, dim3(kThreads), 0, s, ma, md, c.words);
  if (any_zscore) hipLaunchKernelGGL(norm_moments_kernel, grid, dim3(kThreads), 0, s, ma, md, c.recs, c.partials);
  if (any_pct) {
    bool third = false;                                        // a float32 volume among the chunk's percentile channels?
    for (int v = 0; v < 2 * nb; ++v) third |= md.m[v & 1] == MICF_NORM_PERCENTILE && ma.v[v].dtype == MICF_LOADER_F32;
    for (int pass = 0; pass < (third ? 3 : 2); ++pass) {
      hipLaunchKernelGGL(norm_hist_kernel, grid, dim3(kThreads), 0, s, ma, md, pass, c.recs, c.hist);
      hipLaunchKernelGGL(norm_scan_kernel, vols, dim3(kThreads), 0, s, ma, md, pass, p_low, p_high, c.recs, c.hist);
    }
  }
  hipLaunchKernelGGL(norm_finish_kernel, vols, dim3(64), 0, s, ma, md, p_low, p_high, c.words, c.recs, c.partials, c.stats);
}

// micf_volume_loader_norm and micf_volume_loader_affine after their checks: zero, then per chunk the statistics passes and the
// entry's own resample(ra, c, b0, grid, image0, label0) -- c, image0 and label0 the chunk's, grid (blocks, samples of the chunk) --
// then the crop finish on the loader-format words (words_ext) or on the records.
template <class R>
inline int run_stats_loader(const micf_loader_sample* samples, int B, int D, int H, int W, const int32_t* label_values,
                            int num_label_values, const Modes& md, double p_low, double p_high, void* workspace, void* image,
                            uint8_t* label_map, int32_t* crop_indexes, double* stats, hipStream_t s, bool words_ext, R&& resample) {
  const Layout L = layout(B);
  const WsView ws = ws_view(workspace, L, stats);
  const int64_t V = (int64_t)D * H * W;
  launch_zero(s, workspace, L.zero_words);
  MinMaxArgs ma;
  ResizeArgs ra;
  fill_label_values(ra, label_values, num_label_values);
  for_each_chunk(samples, B, ma, ra, [&](int b0, int nb, unsigned blocks) {
    const WsView c = ws.chunk(b0);
    launch_statistics(s, ma, md, nb, blocks, p_low, p_high, c);
    resample(ra, c, b0, dim3(resize_blocks(V), (unsigned)nb), static_cast<__half*>(image) + (size_t)b0 * 2 * V,
             label_map ? label_map + (size_t)b0 * V : nullptr);
  });
  if (words_ext) launch_crop(s, ws.words + 4, kWsWords, B, D, H, W, crop_indexes);
  else launch_crop(s, ws.recs->ext, (int)(sizeof(SampleRec) / 4), B, D, H, W, crop_indexes);
  MICF_RETURN_LAUNCH();
}

}  // namespace
