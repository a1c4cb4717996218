// Device-only helpers that two or more kernel sources share (included by common.hpp).  A helper belongs here when it has at least
// two users and depends on no file-local constant; every one is force-inlined, so moving a body here changes no kernel.  One copy of
// a formula is what lets a forward kernel and its gradient, compiled from different files, agree on it to the last bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mt {

// ---- sigmoid / swish: the one formula of every kernel that evaluates either, forward or backward
// v_rcp_f32 (1 ulp) instead of the 10-instruction IEEE division: the swish kernels are VALU-bound
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float swishf_(float x) { return x * sigmoidf_(x); }
__device__ __forceinline__ float dswishf_(float u) { const float s = sigmoidf_(u); return s * (1.0f + u * (1.0f - s)); }

// ---- float4 one-liners
__device__ __forceinline__ float4 f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return f4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return f4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return f4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- activations.  ACT: 0 none, 1 swish [EfficientNet], 2 relu [Xception]
template <int ACT>
__device__ __forceinline__ float4 act4(float4 u) {
  if (ACT == 1) return f4(swishf_(u.x), swishf_(u.y), swishf_(u.z), swishf_(u.w));
  if (ACT == 2) return f4(fmaxf(u.x, 0.f), fmaxf(u.y, 0.f), fmaxf(u.z, 0.f), fmaxf(u.w, 0.f));
  return u;
}
template <int ACT>
__device__ __forceinline__ float4 dact4(float4 u) {     // derivative of the activation at pre-activation u
  if (ACT == 1) return f4(dswishf_(u.x), dswishf_(u.y), dswishf_(u.z), dswishf_(u.w));
  if (ACT == 2) return f4(u.x > 0.f ? 1.f : 0.f, u.y > 0.f ? 1.f : 0.f, u.z > 0.f ? 1.f : 0.f, u.w > 0.f ? 1.f : 0.f);
  return f4(1.f, 1.f, 1.f, 1.f);
}
// the activation of the per-channel affine z * sc + sh (BatchNorm folded into scale / shift, applied while loading the raw z)
template <int ACT>
__device__ __forceinline__ float4 act_affine4(float4 z, float4 sc, float4 sh) { return act4<ACT>(fma4(z, sc, sh)); }

// ---- reductions over the 64 lanes of a wavefront (xor butterfly: every lane ends with the same value, in a fixed order) ...
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// ... and over a block of WAVES wavefronts through red[WAVES] (LDS), the wavefronts' values combined in wavefront order
template <int WAVES>
__device__ __forceinline__ float block_reduce(float v, float* red, int wave, int lane, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();                                   // red may still be read from the previous reduction
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// row of a wavefront's 32 x 32 v_mfma_f32_32x32x2_f32 accumulator tile that register r of a lane in half hf (= lane >> 5) holds
// (its column is lane & 31)
__device__ __forceinline__ int mfma_slot_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// squeeze-excite: loads `count` consecutive floats of src into the [rows][CS+1] slab image (LDS), eight loads in flight per thread
// of a 256-thread block, then the LDS writes
__device__ __forceinline__ void se_load_slab(float* slab, const float* __restrict__ src, int count, int CS, int tid) {
  const int pitch = CS + 1;
  const float inv_cs = 1.0f / (float)CS;
  for (int e0 = tid; e0 < count; e0 += 256 * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[min(e0 + 256 * u, count - 1)];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 256 * u;
      const int r = (int)(((float)e + 0.5f) * inv_cs);          // e / CS, exact for e < 2^16
      if (e < count) slab[r * pitch + (e - r * CS)] = v[u];
    }
  }
}

}  // namespace mt
