// volume_components.hip -- connected components of a label volume (include/micformer_components.h): per-voxel labels and sizes,
// keep-largest-per-class and remove-small filters, all on the device, in a launch sequence that does not depend on the data.
//
// Union-find over `parent` (int32 per voxel, workspace).  Invariant: parent[i] <= i for every classed voxel, -1 for the others;
// a link only ever decreases (atomicMin), a find walks strictly downward, so every loop ends without waiting for another
// thread (DESIGN.md "Connected components" has the argument).  The root of a component is its smallest linear index.
//
// Launch plan, per chunk of 8 samples (descriptors travel as kernel arguments; a workgroup owns a tile of 64 (x) * 8 (y) * 8 (z)
// voxels, a wave a row of 64 x):
//   1 local    value -> class into LDS; runs of equal class along a row from one wave64 ballot; union-find of the tile in LDS
//              over the links that the run structure does not already imply; parent[i] = global index of the tile-local root
//   2 merge    voxels on tile faces join their neighbours of the same value across the face: find with relaxed agent-scope atomic
//              loads (other XCDs link the same chains in this launch), link with atomicMin
//   3 flatten  per tile: voxels counted per local root in LDS, then per (tile, local root) one find, ONE atomic add of the count
//              into size[root], and the local root's link shortened to the root (so root(i) == parent[parent[i]] afterwards)
//   4 select   KEEP_LARGEST only: per root one 64-bit atomicMax of (size << 32 | ~root) into its class's slot
//   5 output   labels (+ sizes), or the filtered volume
#include "common.h"
#include "../../include/micformer_components.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTX = 64, kTY = 8, kTZ = 8;                 // tile of a workgroup; a wave = 64 consecutive x
constexpr int kRows = kTY * kTZ, kTileVox = kTX * kRows, kWaves = kThreads / 64, kRowsPerWave = kRows / kWaves;
constexpr int kChunk = 8;                                 // samples per launch
constexpr int kMaxExtent = 2048;
constexpr int64_t kMaxVoxels = ((int64_t)1 << 31) - 1;    // exclusive: root + 1 must fit int32
constexpr int kOutLabels = 2;                             // output kernel modes beyond MICF_COMPONENTS_KEEP_LARGEST / _REMOVE_SMALL

struct SampleDesc {
  const void* in;
  void* out;
  int32_t* sizes_out;
  int* parent;
  int* size;
  unsigned long long* best;   // [32] per class: size << 32 | ~root of the component to keep
  int d, h, w;
  int ntx, nty, ntiles;
};
struct Args {
  SampleDesc s[kChunk];
  int lut[MICF_COMPONENTS_MAX_CLASSES];   // lut[k] = value of class k (k >= 1)
  int K;
};

template <typename T>
__device__ __forceinline__ int class_of(const Args& a, T v) {
  if (v == 0) return 0;
  if constexpr (sizeof(T) == 1) {
    return (int)v < a.K ? (int)v : 0;
  } else {
    int c = 0;
    for (int k = 1; k < a.K; ++k) c = a.lut[k] == (int)v ? k : c;
    return c;
  }
}

// The links of voxel (z, y, x) of value c to the 13 neighbours that precede it in linear order, less those that the others imply.
// Within a pair of rows (the voxel's and one of the four preceding neighbour rows) with neighbours n(x-1), n(x), n(x+1):
//   n(x) == c:  link to n(x) alone (n(x +- 1) hang on n(x) by a row link), and not even that when v(x-1) == n(x-1) == c (the
//               pair one step to the left is linked, and both rows continue a run);
//   otherwise:  link to n(x-1) unless v(x-1) == c (which links to it itself), and to n(x+1) unless v(x+1) == c.
// Why the skipped link v(x)-n(x) is implied (v(x-1) == n(x-1) == v(x) == n(x) == c), by induction along the run to the left: the
// same row pair handles the pair at x-1, which either links v(x-1)-n(x-1) itself or skips it for the same reason one step further
// left.  The chain ends at the first x' where v(x'-1) or n(x'-1) is not c -- the start of one of the two runs, or "no voxel" past
// the edge of the tile (local phase) or of the volume (merge) -- and there the link v(x')-n(x') is made.  Both rows are runs from
// x' to x, so v(x) -row- v(x') - n(x') -row- n(x).  In the merge the chain may run through several tiles along x: rowok depends on
// the rows alone, so every lane of the chain takes the same row pair in whichever tile it lies; the row links inside a tile come
// from the local phase, those across an x-face from lane 0 (xedge), which like lane 63 takes all four rows, the diagonal
// neighbours of an x-face voxel lying in another tile whatever the rows.  The two one-sided skips are direct: v(x-1) == c links
// n(x-1) by its own n(x) case, v(x+1) == c likewise.
// get(z, y, x) is the value there, or something that equals no c where there is no voxel; rowok(q) lets the caller skip rows.
template <typename V, typename Get, typename RowOk, typename Link>
__device__ __forceinline__ void for_each_link(int z, int y, int x, V c, int conn, bool xedge, Get get, RowOk rowok, Link link) {
  const V vl = get(z, y, x - 1), vr = get(z, y, x + 1);
  if (xedge && vl == c) link(z, y, x - 1);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dz = q == 0 ? 0 : -1, dy = q == 0 ? -1 : q - 2;   // (0,-1) (-1,-1) (-1,0) (-1,1)
    const bool diag = q == 1 || q == 3;
    if (diag && conn == 6) continue;
    if (!rowok(q)) continue;
    const bool wide = conn == 26 || (conn == 18 && !diag);
    const int nz = z + dz, ny = y + dy;
    if (get(nz, ny, x) == c) {
      if (!(vl == c && get(nz, ny, x - 1) == c)) link(nz, ny, x);
    } else if (wide) {
      if (vl != c && get(nz, ny, x - 1) == c) link(nz, ny, x - 1);
      if (vr != c && get(nz, ny, x + 1) == c) link(nz, ny, x + 1);
    }
  }
}

// ---- union-find.  find: parent[i] < i unless i is a root, so the walk ends.  unite: every retry continues from a value that the
// atomicMin returned and that is smaller than the node it was applied to: max(a, b) decreases strictly, nothing waits.
template <typename Load>
__device__ __forceinline__ int uf_find(int i, Load load) {
  int p;
  while ((p = load(i)) != i) i = p;
  return i;
}
template <typename Load, typename Min>
__device__ __forceinline__ void uf_unite(int a, int b, Load load, Min amin) {
  a = uf_find(a, load);
  b = uf_find(b, load);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = amin(a, b);                            // parent[a] = min(parent[a], b), b < a
    if (old == a) break;                                   // a was a root and now hangs on b
    a = uf_find(old, load);                                // a had been linked to old (< a) meanwhile: old and b remain to be joined
    b = uf_find(b, load);
  }
}

__device__ __forceinline__ void tile_origin(const SampleDesc& sd, int& x0, int& y0, int& z0) {
  const int tx = (int)blockIdx.x % sd.ntx, tr = (int)blockIdx.x / sd.ntx;
  x0 = tx * kTX; y0 = (tr % sd.nty) * kTY; z0 = (tr / sd.nty) * kTZ;
}

// ---- 1. local: grid (tiles, samples of the chunk) ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void components_local_kernel(Args a, int conn) {
  const SampleDesc& sd = a.s[blockIdx.y];
  if ((int)blockIdx.x >= sd.ntiles) return;
  __shared__ int lab[kTileVox];
  __shared__ uint8_t cls[kTileVox];
  if (blockIdx.x == 0 && threadIdx.x < MICF_COMPONENTS_MAX_CLASSES) sd.best[threadIdx.x] = 0ull;
  int x0, y0, z0;
  tile_origin(sd, x0, y0, z0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T* in = static_cast<const T*>(sd.in);
  const int x = x0 + lane;
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, z = z0 + (r >> 3), y = y0 + (r & 7);
    const bool inb = z < sd.d && y < sd.h && x < sd.w;
    const int c = inb ? class_of<T>(a, in[((int64_t)z * sd.h + y) * sd.w + x]) : 0;
    // the start of the lane's run of equal class: the highest lane <= this one that does not continue its left neighbour
    const int lc = __shfl_up(c, 1, 64);
    const unsigned long long starts = ~__ballot(lane > 0 && lc == c);
    const int start = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));
    cls[r * kTX + lane] = (uint8_t)c;
    lab[r * kTX + lane] = r * kTX + start;
  }
  __syncthreads();
  auto load = [&](int i) { return __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  auto amin = [&](int i, int v) { return atomicMin(&lab[i], v); };
  auto get = [&](int lz, int ly, int lx) -> int {
    return ((unsigned)lz < (unsigned)kTZ && (unsigned)ly < (unsigned)kTY && (unsigned)lx < (unsigned)kTX) ? (int)cls[(lz * kTY + ly) * kTX + lx] : -1;
  };
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, l = r * kTX + lane;
    const int c = cls[l];
    if (c == 0) continue;
    for_each_link(r >> 3, r & 7, lane, c, conn, false, get, [](int) { return true; },
                  [&](int lz, int ly, int lx) { uf_unite(l, (lz * kTY + ly) * kTX + lx, load, amin); });
  }
  __syncthreads();
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, l = r * kTX + lane, z = z0 + (r >> 3), y = y0 + (r & 7);
    if (!(z < sd.d && y < sd.h && x < sd.w)) continue;
    const int64_t idx = ((int64_t)z * sd.h + y) * sd.w + x;
    if (cls[l] == 0) { sd.parent[idx] = -1; continue; }
    const int root = uf_find(l, load);
    const int rr = root / kTX;
    sd.parent[idx] = (int)(((int64_t)(z0 + (rr >> 3)) * sd.h + y0 + (rr & 7)) * sd.w + x0 + (root & 63));
    if (root == l) sd.size[idx] = 0;                       // only local roots can become roots: the only sizes ever added to
  }
}

// ---- 2. merge across tile faces: grid (tiles, samples of the chunk) ----------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void components_merge_kernel(Args a, int conn) {
  const SampleDesc& sd = a.s[blockIdx.y];
  if ((int)blockIdx.x >= sd.ntiles) return;
  int x0, y0, z0;
  tile_origin(sd, x0, y0, z0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T* in = static_cast<const T*>(sd.in);
  int* parent = sd.parent;
  const int d = sd.d, h = sd.h, w = sd.w;
  const int x = x0 + lane;
  if (x >= w) return;
  // links are read while workgroups on other XCDs write them: agent-scope loads (L2, never this CU's L1), writes by atomicMin only
  auto load = [&](int i) { return __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto amin = [&](int i, int v) { return atomicMin(&parent[i], v); };
  constexpr long long kNone = 1ll << 40;                   // equals no voxel's value
  auto get = [&](int z, int y, int xx) -> long long {
    return ((unsigned)z < (unsigned)d && (unsigned)y < (unsigned)h && (unsigned)xx < (unsigned)w) ? (long long)in[((int64_t)z * h + y) * w + xx] : kNone;
  };
  const bool xface = lane == 0 || lane == kTX - 1;
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, lz = r >> 3, ly = r & 7, z = z0 + lz, y = y0 + ly;
    if (z >= d || y >= h) continue;
    if (!(xface || lz == 0 || ly == 0 || ly == kTY - 1)) continue;
    const int idx = (int)(((int64_t)z * h + y) * w + x);
    if (load(idx) < 0) continue;                           // background or a value that names no class
    const long long c = in[idx];
    for_each_link(z, y, x, c, conn, true, get,
                  [&](int q) { return xface || (q == 0 ? ly == 0 : (lz == 0 || (q == 1 && ly == 0) || (q == 3 && ly == kTY - 1))); },
                  [&](int nz, int ny, int nx) {
                    if ((nx >> 6) != (x >> 6) || (ny >> 3) != (y >> 3) || (nz >> 3) != (z >> 3))      // else joined in LDS already
                      uf_unite(idx, (int)(((int64_t)nz * h + ny) * w + nx), load, amin);
                  });
  }
}

// ---- 3. flatten + sizes: grid (tiles, samples of the chunk).  A separate launch: the links are final, plain loads ------------------
__global__ __launch_bounds__(kThreads) void components_flatten_kernel(Args a) {
  const SampleDesc& sd = a.s[blockIdx.y];
  if ((int)blockIdx.x >= sd.ntiles) return;
  __shared__ int cnt[kTileVox];
  int x0, y0, z0;
  tile_origin(sd, x0, y0, z0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d = sd.d, h = sd.h, w = sd.w, x = x0 + lane;
  int* parent = sd.parent;
  for (int i = threadIdx.x; i < kTileVox; i += kThreads) cnt[i] = 0;
  __syncthreads();
  // a voxel counts at the slot of its link when that lies in this tile (its local root, or for a local root that was merged
  // under another one of this tile, that one: the same component), at its own slot otherwise (a local root linked elsewhere)
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, z = z0 + (r >> 3), y = y0 + (r & 7);
    if (z >= d || y >= h || x >= w) continue;
    const int p = parent[((int64_t)z * h + y) * w + x];
    if (p < 0) continue;
    const unsigned px = (unsigned)p % (unsigned)w, pr = (unsigned)p / (unsigned)w, py = pr % (unsigned)h, pz = pr / (unsigned)h;
    const unsigned lx = px - (unsigned)x0, ly = py - (unsigned)y0, lz = pz - (unsigned)z0;
    const int slot = (lx < (unsigned)kTX && ly < (unsigned)kTY && lz < (unsigned)kTZ) ? (int)((lz * kTY + ly) * kTX + lx) : r * kTX + lane;
    atomicAdd(&cnt[slot], 1);
  }
  __syncthreads();
  // one find and one atomic add per (tile, occupied slot); every occupied slot is a local root, whose link may be shortened
  // while other workgroups walk through it: they read the old link or the root, both of them ancestors
  for (int j = 0; j < kRowsPerWave; ++j) {
    const int r = wv + kWaves * j, n = cnt[r * kTX + lane];
    if (n == 0) continue;
    const int idx = (int)(((int64_t)(z0 + (r >> 3)) * h + y0 + (r & 7)) * w + x);
    const int g = uf_find(idx, [&](int i) { return parent[i]; });
    atomicAdd(&sd.size[g], n);
    if (g != idx) parent[idx] = g;
  }
}

// ---- 4. select: grid (blocks, samples of the chunk) --------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void components_select_kernel(Args a, unsigned mask) {
  const SampleDesc& sd = a.s[blockIdx.y];
  const int V = sd.d * sd.h * sd.w;
  const T* in = static_cast<const T*>(sd.in);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < V; i += (int64_t)gridDim.x * kThreads) {
    if (sd.parent[i] != (int)i) continue;
    const int c = class_of<T>(a, in[i]);
    if ((mask >> c) & 1u) atomicMax(&sd.best[c], ((unsigned long long)(unsigned)sd.size[i] << 32) | (unsigned)~(unsigned)i);
  }
}

// ---- 5. output: grid (blocks, samples of the chunk) --------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void components_output_kernel(Args a, unsigned mask, int min_size) {
  const SampleDesc& sd = a.s[blockIdx.y];
  const int V = sd.d * sd.h * sd.w;
  const T* in = static_cast<const T*>(sd.in);
  const int* parent = sd.parent;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < V; i += (int64_t)gridDim.x * kThreads) {
    const int p = parent[i];
    if constexpr (MODE == kOutLabels) {
      const int root = p < 0 ? -1 : parent[p];
      static_cast<int32_t*>(sd.out)[i] = root + 1;
      if (sd.sizes_out) sd.sizes_out[i] = p < 0 ? 0 : sd.size[root];
    } else {
      T v = in[i];
      if (p >= 0) {
        const int c = class_of<T>(a, v);
        if ((mask >> c) & 1u) {
          const int root = parent[p];
          const bool keep = MODE == MICF_COMPONENTS_KEEP_LARGEST ? (unsigned)~(unsigned)sd.best[c] == (unsigned)root : sd.size[root] >= min_size;
          if (!keep) v = 0;
        }
      }
      static_cast<T*>(sd.out)[i] = v;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int elem_size(int dtype) { return dtype == MICF_COMPONENTS_U8 ? 1 : (dtype == MICF_COMPONENTS_I16 ? 2 : 4); }
int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }

// bytes of one sample's workspace, or the error code of its shape
int64_t sample_bytes(const micf_component_sample& s) {
  if (s.shape[0] <= 0 || s.shape[1] <= 0 || s.shape[2] <= 0) return MICF_EINVAL;
  if (s.shape[0] > kMaxExtent || s.shape[1] > kMaxExtent || s.shape[2] > kMaxExtent) return MICF_EUNSUPPORTED;
  const int64_t V = (int64_t)s.shape[0] * s.shape[1] * s.shape[2];
  if (V >= kMaxVoxels) return MICF_EUNSUPPORTED;
  return 2 * align256(V * 4) + 256;
}

int64_t workspace_bytes_of(const micf_component_sample* samples, int B) {
  if (!samples || B <= 0) return MICF_EINVAL;
  int64_t total = 0;
  int unsupported = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = sample_bytes(samples[b]);
    if (n == MICF_EINVAL) return MICF_EINVAL;
    if (n < 0) unsupported = 1;
    else total += n;
  }
  return unsupported ? (int64_t)MICF_EUNSUPPORTED : total;
}

template <typename T>
void launch_all(const Args& a, int nb, int most, int64_t most_voxels, int conn, int mode, unsigned mask, int min_size, hipStream_t s) {
  const dim3 tiles((unsigned)most, (unsigned)nb), block(kThreads);
  const int64_t vb = (most_voxels + kThreads - 1) / kThreads;
  const dim3 flat((unsigned)(vb < 16384 ? vb : 16384), (unsigned)nb);
  hipLaunchKernelGGL(components_local_kernel<T>, tiles, block, 0, s, a, conn);
  hipLaunchKernelGGL(components_merge_kernel<T>, tiles, block, 0, s, a, conn);
  hipLaunchKernelGGL(components_flatten_kernel, tiles, block, 0, s, a);
  if (mode == MICF_COMPONENTS_KEEP_LARGEST) {
    hipLaunchKernelGGL(components_select_kernel<T>, flat, block, 0, s, a, mask);
    hipLaunchKernelGGL((components_output_kernel<T, MICF_COMPONENTS_KEEP_LARGEST>), flat, block, 0, s, a, mask, min_size);
  } else if (mode == MICF_COMPONENTS_REMOVE_SMALL) {
    hipLaunchKernelGGL((components_output_kernel<T, MICF_COMPONENTS_REMOVE_SMALL>), flat, block, 0, s, a, mask, min_size);
  } else {
    hipLaunchKernelGGL((components_output_kernel<T, kOutLabels>), flat, block, 0, s, a, mask, min_size);
  }
}

int run(const micf_component_sample* samples, int B, int in_dtype, int K, const int32_t* label_values, int num_label_values,
        int connectivity, int32_t* const* sizes, int mode, int64_t class_mask, int min_size, void* workspace, int64_t workspace_bytes,
        micf_stream_t stream) {
  if (!samples || B <= 0) return MICF_EINVAL;
  if (in_dtype != MICF_COMPONENTS_U8 && in_dtype != MICF_COMPONENTS_I16 && in_dtype != MICF_COMPONENTS_I32) return MICF_EINVAL;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return MICF_EINVAL;
  if (mode != kOutLabels) {
    if (mode != MICF_COMPONENTS_KEEP_LARGEST && mode != MICF_COMPONENTS_REMOVE_SMALL) return MICF_EINVAL;
    if (min_size < 1) return MICF_EINVAL;
  }
  int unsupported = K < 2 || K > MICF_COMPONENTS_MAX_CLASSES;
  if (!unsupported) {                                    // (the label table and the class mask are sized by a supported K)
    if (in_dtype == MICF_COMPONENTS_U8) {
      if (label_values || num_label_values != 0) return MICF_EINVAL;
    } else {
      if (!label_values || num_label_values != K - 1) return MICF_EINVAL;
      for (int i = 0; i < num_label_values; ++i) {
        if (label_values[i] == 0) return MICF_EINVAL;
        if (in_dtype == MICF_COMPONENTS_I16 && (label_values[i] < -32768 || label_values[i] > 32767)) return MICF_EINVAL;
        for (int j = 0; j < i; ++j)
          if (label_values[j] == label_values[i]) return MICF_EINVAL;
      }
    }
    if (mode != kOutLabels && (class_mask == 0 || (class_mask & ~((((int64_t)1 << K) - 1) & ~(int64_t)1)))) return MICF_EINVAL;
  }
  const int out_elem = mode == kOutLabels ? 4 : elem_size(in_dtype);
  for (int b = 0; b < B; ++b) {
    const micf_component_sample& sm = samples[b];
    if (!sm.in || (reinterpret_cast<uintptr_t>(sm.in) & (uintptr_t)(elem_size(in_dtype) - 1))) return MICF_EINVAL;
    if (!sm.out || (reinterpret_cast<uintptr_t>(sm.out) & (uintptr_t)(out_elem - 1))) return MICF_EINVAL;
    if (sizes && (!sizes[b] || (reinterpret_cast<uintptr_t>(sizes[b]) & 3))) return MICF_EINVAL;
  }
  const int64_t need = workspace_bytes_of(samples, B);
  if (need == MICF_EINVAL) return MICF_EINVAL;
  if (need < 0 || unsupported) return MICF_EUNSUPPORTED;
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255)) return MICF_EINVAL;

  hipStream_t s = (hipStream_t)stream;
  Args a;
  a.K = K;
  for (int k = 0; k < MICF_COMPONENTS_MAX_CLASSES; ++k)
    a.lut[k] = in_dtype == MICF_COMPONENTS_U8 ? k : (k >= 1 && k < K ? label_values[k - 1] : 0);
  char* ws = static_cast<char*>(workspace);
  for (int b0 = 0; b0 < B; b0 += kChunk) {
    const int nb = B - b0 < kChunk ? B - b0 : kChunk;
    int most = 0;
    int64_t most_voxels = 0;
    for (int i = 0; i < kChunk; ++i) {
      SampleDesc& sd = a.s[i];
      if (i >= nb) { sd = a.s[0]; continue; }            // (unused slots repeat the first: never launched)
      const micf_component_sample& sm = samples[b0 + i];
      const int64_t V = (int64_t)sm.shape[0] * sm.shape[1] * sm.shape[2];
      sd.in = sm.in;
      sd.out = sm.out;
      sd.sizes_out = sizes ? sizes[b0 + i] : nullptr;
      sd.parent = reinterpret_cast<int*>(ws);
      sd.size = reinterpret_cast<int*>(ws + align256(V * 4));
      sd.best = reinterpret_cast<unsigned long long*>(ws + 2 * align256(V * 4));
      ws += 2 * align256(V * 4) + 256;
      sd.d = sm.shape[0]; sd.h = sm.shape[1]; sd.w = sm.shape[2];
      sd.ntx = (sd.w + kTX - 1) / kTX;
      sd.nty = (sd.h + kTY - 1) / kTY;
      sd.ntiles = sd.ntx * sd.nty * ((sd.d + kTZ - 1) / kTZ);                    // <= 32 * 256 * 256
      most = sd.ntiles > most ? sd.ntiles : most;
      most_voxels = V > most_voxels ? V : most_voxels;
    }
    const unsigned mask = (unsigned)class_mask;
    if (in_dtype == MICF_COMPONENTS_U8) launch_all<uint8_t>(a, nb, most, most_voxels, connectivity, mode, mask, min_size, s);
    else if (in_dtype == MICF_COMPONENTS_I16) launch_all<int16_t>(a, nb, most, most_voxels, connectivity, mode, mask, min_size, s);
    else launch_all<int32_t>(a, nb, most, most_voxels, connectivity, mode, mask, min_size, s);
  }
  MICF_RETURN_LAUNCH();
}

}  // namespace

extern "C" int64_t micf_components_workspace(const micf_component_sample* samples, int B) { return workspace_bytes_of(samples, B); }

extern "C" int micf_connected_components(const micf_component_sample* samples, int B, int in_dtype, int K, const int32_t* label_values,
                                         int num_label_values, int connectivity, int32_t* const* sizes, void* workspace,
                                         int64_t workspace_bytes, micf_stream_t stream) {
  return run(samples, B, in_dtype, K, label_values, num_label_values, connectivity, sizes, kOutLabels, 0, 1, workspace, workspace_bytes,
             stream);
}

extern "C" int micf_filter_components(const micf_component_sample* samples, int B, int in_dtype, int K, const int32_t* label_values,
                                      int num_label_values, int connectivity, int64_t class_mask, int mode, int min_size,
                                      void* workspace, int64_t workspace_bytes, micf_stream_t stream) {
  if (mode != MICF_COMPONENTS_KEEP_LARGEST && mode != MICF_COMPONENTS_REMOVE_SMALL) return MICF_EINVAL;
  return run(samples, B, in_dtype, K, label_values, num_label_values, connectivity, nullptr, mode, class_mask, min_size, workspace,
             workspace_bytes, stream);
}
