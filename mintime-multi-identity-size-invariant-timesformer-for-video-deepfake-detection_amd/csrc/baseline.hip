// The Baseline model's head (reference models/baseline.py:15-37: AdaptiveAvgPool2d(1) -> Linear(dim, mlp) -> Linear(mlp, 1)) as
// rank-1 algebra.  With one class and nothing between the two Linears the head is one vector:
//   v = W1^T w2 [C],  c0 = w2 . b1 + b2,  logit_i = mean_p(f_i[p, :]) . v + c0
// so the features are read once and no GEMM runs (hidden = pooled W1^T + b1 is never formed).  The backward, for g_i = dL/dlogit_i:
//   s = sum_i g_i,  u = sum_i g_i pooled_i [C],  db2 = s,  db1 = w2 s,  dW1 = w2 (x) u,  dW2[j] = W1[j, :] . u + b1[j] s,
//   dfeat_i[p, c] = g_i v[c] / hw.
// Every sum runs in a fixed order and no kernel issues an atomic: the results are the same bits run after run.
#include "../../include/mintime_hip.h"
#include "common.hpp"

using namespace mt;

namespace {

constexpr int kChunk = 256;    // channels per block of the pooling kernel
constexpr int kSlab = 32;      // crops per partial sum of the backward reduction

// vc[c] = sum_j W1[j][c] w2[j] (c < C);  vc[C] = sum_j b1[j] w2[j] + b2.  Block = 64 columns x 16 groups of consecutive rows j (the
// lanes read 64 consecutive floats of a row of W1); the group sums are added in group order.  (4 groups: 52 us per call at C = 1280,
// m = 512 -- too few wavefronts, each a long chain of dependent loads.)
constexpr int kPrepGroups = 16;
__global__ __launch_bounds__(64 * kPrepGroups) void prep_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                                const float* __restrict__ w2, const float* __restrict__ b2,
                                                                float* __restrict__ vc, int C, int m) {
  __shared__ float part[kPrepGroups][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int per = (m + kPrepGroups - 1) / kPrepGroups, j0 = min(m, grp * per), j1 = min(m, j0 + per);
  float acc = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int j = j0; j < j1; ++j) acc = fmaf(w1[(int64_t)j * C + c], w2[j], acc);
  } else if (c == C) {
    for (int j = j0; j < j1; ++j) acc = fmaf(b1[j], w2[j], acc);
  }
  part[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && c <= C) {
    float r = part[0][lane];
    for (int k = 1; k < kPrepGroups; ++k) r += part[k][lane];
    if (c == C) r += b2[0];
    vc[c] = r;
  }
}

// Block (chunk s of 256 channels, crop i): pooled = mean over the hw pixels, part[i][s] = pooled . v over the chunk.
// LAYOUT 0 (NHWC, x[i][p][c]): lane = 4 channels (one float4), wave = pixels p = wave, wave + 4, ...; the four wave sums in order.
// LAYOUT 1 (NCHW, x[i][c][p]): wave = 64 of the chunk's channels one after the other, lanes = pixels (a coalesced row of hw floats).
template <int LAYOUT>
__global__ __launch_bounds__(256) void pool_dot_kernel(const float* __restrict__ x, const float* __restrict__ vc, float* __restrict__ pooled,
                                                       float* __restrict__ part, int C, int hw, int S) {
  __shared__ float4 red4[4][64];
  __shared__ float sum[kChunk];
  __shared__ float wred[4];
  const int s = blockIdx.x, i = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int cbase = s * kChunk;
  const float* xi = x + (int64_t)i * hw * C;
  if (LAYOUT == 0) {
    const int c = cbase + lane * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
#pragma unroll 4
      for (int p = wave; p < hw; p += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xi + (int64_t)p * C + c);
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
    red4[wave][lane] = acc;
    __syncthreads();
    const float* r = reinterpret_cast<const float*>(&red4[0][0]);      // [4][256]: channel t of the chunk at r[g * 256 + t]
    sum[t] = ((r[t] + r[256 + t]) + r[512 + t]) + r[768 + t];
  } else {
    for (int k = 0; k < 64; ++k) {
      const int cl = wave * 64 + k, c = cbase + cl;
      float a = 0.f;
      if (c < C)
        for (int p = lane; p < hw; p += 64) a += xi[(int64_t)c * hw + p];
      a = wave_sum(a);
      if (lane == 0) sum[cl] = a;
    }
  }
  __syncthreads();
  const int c = cbase + t;
  float d = 0.f;
  if (c < C) {
    const float pv = sum[t] / (float)hw;
    if (pooled) pooled[(int64_t)i * C + c] = pv;
    d = pv * vc[c];
  }
  d = wave_sum(d);
  if (lane == 0) wred[wave] = d;
  __syncthreads();
  if (t == 0) part[(int64_t)i * S + s] = ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

// logits[i] = (sum over chunks s of part[i][s], in chunk order) + c0
__global__ __launch_bounds__(256) void logits_kernel(const float* __restrict__ part, const float* __restrict__ vc, float* __restrict__ logits,
                                                     int n, int S, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* pi = part + (int64_t)i * S;
  float a = pi[0];
  for (int s = 1; s < S; ++s) a += pi[s];
  logits[i] = a + vc[C];
}

// ws[slab][c] = sum_{i in slab} g_i pooled[i][c] (c < C), ws[slab][C] = sum_{i in slab} g_i; crops in increasing order.
__global__ __launch_bounds__(256) void slab_kernel(const float* __restrict__ g, const float* __restrict__ pooled, float* __restrict__ ws,
                                                   int n, int C, int ld) {
  const int c = blockIdx.x * 256 + threadIdx.x, slab = blockIdx.y;
  if (c > C) return;
  const int i0 = slab * kSlab, i1 = min(n, i0 + kSlab);
  float a = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int i = i0; i < i1; ++i) a = fmaf(g[i], pooled[(int64_t)i * C + c], a);
  } else {
    for (int i = i0; i < i1; ++i) a += g[i];
  }
  ws[(int64_t)slab * ld + c] = a;
}

// u[c] = the slabs' partial sums added in slab order (the second pass when n > kSlab)
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ ws, float* __restrict__ u, int nslab, int C, int ld) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > C) return;
  float a = ws[c];
  for (int sl = 1; sl < nslab; ++sl) a += ws[(int64_t)sl * ld + c];
  u[c] = a;
}

// One wavefront per row j of W1: dW1[j][:] = w2[j] u, dW2[j] = W1[j][:] . u + b1[j] s, db1[j] = w2[j] s, db2 = s (u[C] = s).
__global__ __launch_bounds__(256) void params_kernel(const float* __restrict__ u, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, float* __restrict__ dw1, float* __restrict__ db1,
                                                     float* __restrict__ dw2, float* __restrict__ db2, int C, int m) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;                    // uniform per wavefront
  const float s = u[C], w2j = w2[j];
  float d = 0.f;
  for (int c = lane * 4; c < C; c += 256) {
    const float4 uu = *reinterpret_cast<const float4*>(u + c);
    if (dw2) {
      const float4 w = *reinterpret_cast<const float4*>(w1 + (int64_t)j * C + c);
      d = fmaf(w.x, uu.x, d);
      d = fmaf(w.y, uu.y, d);
      d = fmaf(w.z, uu.z, d);
      d = fmaf(w.w, uu.w, d);
    }
    if (dw1) *reinterpret_cast<float4*>(dw1 + (int64_t)j * C + c) = make_float4(w2j * uu.x, w2j * uu.y, w2j * uu.z, w2j * uu.w);
  }
  if (dw2) {
    d = wave_sum(d);
    if (lane == 0) dw2[j] = d + b1[j] * s;
  }
  if (lane == 0) {
    if (db1) db1[j] = w2j * s;
    if (db2 && j == 0) db2[0] = s;
  }
}

// dx[i] = g_i v / hw broadcast over the crop's pixels, in the input's layout (4 consecutive elements per thread; C % 4 == 0).
template <int LAYOUT>
__global__ __launch_bounds__(256) void dfeat_kernel(const float* __restrict__ g, const float* __restrict__ vc, float* __restrict__ dx, int C,
                                                    int hw) {
  const int i = blockIdx.y;
  const int per = C * hw;
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k >= per) return;
  const float gi = g[i], fhw = (float)hw;
  float4 o;
  if (LAYOUT == 0) {
    const float4 v = *reinterpret_cast<const float4*>(vc + k % C);
    o = make_float4(gi * v.x / fhw, gi * v.y / fhw, gi * v.z / fhw, gi * v.w / fhw);
  } else {
    o = make_float4(gi * vc[k / hw] / fhw, gi * vc[(k + 1) / hw] / fhw, gi * vc[(k + 2) / hw] / fhw, gi * vc[(k + 3) / hw] / fhw);
  }
  *reinterpret_cast<float4*>(dx + (int64_t)i * per + k) = o;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(const char* what, int layout, int n, int hw, int C, int m) {
  if (layout != 0 && layout != 1) return fail(MT_ERR_ARG, "%s: layout must be 0 (NHWC) or 1 (NCHW), got %d", what, layout);
  if (n <= 0 || hw <= 0 || C <= 0 || m <= 0) return fail(MT_ERR_ARG, "%s: empty shape (n %d, hw %d, C %d, m %d)", what, n, hw, C, m);
  if (C % 4) return fail(MT_ERR_UNSUPPORTED, "%s: C %% 4 == 0 expected (float4 loads over channels), got C = %d", what, C);
  if (n > 65535) return fail(MT_ERR_UNSUPPORTED, "%s: at most 65535 crops per call, got %d", what, n);
  if ((int64_t)C * hw > 0x7fffffffLL) return fail(MT_ERR_UNSUPPORTED, "%s: one crop's C * hw must stay below 2^31 elements", what);
  return 0;
}

}  // namespace

extern "C" int mt_baseline_head_fwd(const float* x, int layout, int n, int hw, int C, int m, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float* vc, float* pooled, float* part, float* logits, void* stream) {
  if (int rc = check_shape("mt_baseline_head_fwd", layout, n, hw, C, m)) return rc;
  if (!x || !w1 || !b1 || !w2 || !b2 || !vc || !part || !logits) return fail(MT_ERR_ARG, "mt_baseline_head_fwd: null pointer");
  if (!aligned16(x) || !aligned16(vc))
    return fail(MT_ERR_UNSUPPORTED, "mt_baseline_head_fwd: x and vc must be 16-byte aligned (float4 loads)");
  const hipStream_t st = (hipStream_t)stream;
  const int S = (C + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(prep_kernel, dim3((C + 1 + 63) / 64), dim3(64 * kPrepGroups), 0, st, w1, b1, w2, b2, vc, C, m);
  if (layout == 0)
    hipLaunchKernelGGL(pool_dot_kernel<0>, dim3(S, n), dim3(256), 0, st, x, vc, pooled, part, C, hw, S);
  else
    hipLaunchKernelGGL(pool_dot_kernel<1>, dim3(S, n), dim3(256), 0, st, x, vc, pooled, part, C, hw, S);
  hipLaunchKernelGGL(logits_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, vc, logits, n, S, C);
  return check_launch("mt_baseline_head_fwd");
}

extern "C" int mt_baseline_head_bwd(const float* dlogits, const float* pooled, const float* vc, int n, int hw, int C, int m, const float* w1,
                                    const float* b1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dx, int layout,
                                    float* work, void* stream) {
  if (int rc = check_shape("mt_baseline_head_bwd", layout, n, hw, C, m)) return rc;
  if (!dlogits || !vc) return fail(MT_ERR_ARG, "mt_baseline_head_bwd: null pointer");
  const bool params = dw1 || db1 || dw2 || db2;
  if (params && (!pooled || !work || !w2 || (dw2 && (!w1 || !b1))))
    return fail(MT_ERR_ARG, "mt_baseline_head_bwd: parameter gradients need pooled, work, w2 (and w1, b1 for dW2)");
  if (!aligned16(vc) || (dx && !aligned16(dx)) || (work && !aligned16(work)) || (dw1 && !aligned16(dw1)) || (dw2 && !aligned16(w1)))
    return fail(MT_ERR_UNSUPPORTED, "mt_baseline_head_bwd: vc, dx, work, dW1 and W1 must be 16-byte aligned (float4 accesses)");
  const hipStream_t st = (hipStream_t)stream;
  if (params) {
    const int ld = C + 4;                              // (C + 1) rounded up to a multiple of 4: every row starts 16-byte aligned
    const int nslab = (n + kSlab - 1) / kSlab;
    float* u = work + (int64_t)nslab * ld;
    const dim3 cgrid((C + 1 + 255) / 256);
    if (nslab == 1) {
      hipLaunchKernelGGL(slab_kernel, dim3(cgrid.x, 1), dim3(256), 0, st, dlogits, pooled, u, n, C, ld);
    } else {
      hipLaunchKernelGGL(slab_kernel, dim3(cgrid.x, nslab), dim3(256), 0, st, dlogits, pooled, work, n, C, ld);
      hipLaunchKernelGGL(slab_sum_kernel, cgrid, dim3(256), 0, st, work, u, nslab, C, ld);
    }
    hipLaunchKernelGGL(params_kernel, dim3((m + 3) / 4), dim3(256), 0, st, u, w1, b1, w2, dw1, db1, dw2, db2, C, m);
  }
  if (dx) {
    const dim3 grid((C * hw / 4 + 255) / 256, n);
    if (layout == 0)
      hipLaunchKernelGGL(dfeat_kernel<0>, grid, dim3(256), 0, st, dlogits, vc, dx, C, hw);
    else
      hipLaunchKernelGGL(dfeat_kernel<1>, grid, dim3(256), 0, st, dlogits, vc, dx, C, hw);
  }
  return check_launch("mt_baseline_head_bwd");
}
