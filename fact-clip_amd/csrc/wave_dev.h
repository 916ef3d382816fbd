// Wave-level device pieces that several kernel files used to spell out for themselves: the accumulator
// type of v_mfma_f32_32x32x2_f32 and its row map, the 64-lane sum / max, and the write-through (sc1)
// accesses of partials that another workgroup reads inside the same launch.
#pragma once
#include <hip/hip_runtime.h>

namespace fx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}
// accumulator element r of a lane: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------ write-through (sc1) accesses
// (cache-policy operand 16 = sc1 on gfx950: L1 bypassed, stores written through)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ float4 ldc4(const float* base, long long idx) {
  const v4f v = __builtin_amdgcn_raw_buffer_load_b128(rsrc(base), (int)(idx * 4), 0, 16);
  return make_float4(v[0], v[1], v[2], v[3]);
}
// (the b32 forms move 32-bit integers: the float's bits, not its value)
__device__ __forceinline__ float ldc1(const float* base, long long idx) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc(base), (int)(idx * 4), 0, 16));
}
__device__ __forceinline__ void stc1(float* base, long long idx, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc(base), (int)(idx * 4), 0, 16);
}
__device__ __forceinline__ void stc4(float* base, long long idx, float4 v) {
  v4f x = {v.x, v.y, v.z, v.w};
  __builtin_amdgcn_raw_buffer_store_b128(x, rsrc(base), (int)(idx * 4), 0, 16);
}

}  // namespace fx
