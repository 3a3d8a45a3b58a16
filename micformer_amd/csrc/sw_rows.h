// sw_rows.h -- what the store-and-sum kernels of sliding-window inference share (sw_blend.hip, sw_mirror.hip): a row piece of VEC
// floats that moves as one dword or one 16-byte access, and the ONE accumulate expression.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace micf_sw {

// the ONE accumulate expression: a single rounding, independent of the compiler's contraction setting
__device__ __forceinline__ float blend_term(float acc, float w, float p) { return __builtin_fmaf(w, p, acc); }

template <int VEC> struct Row;
template <> struct Row<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
  __device__ __forceinline__ void reverse() {}
};
template <> struct Row<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
  __device__ __forceinline__ void reverse() {
    const float a = v[0], b = v[1];
    v[0] = v[3]; v[1] = v[2]; v[2] = b; v[3] = a;
  }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace micf_sw
