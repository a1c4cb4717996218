// Data gradient of SlowFast's stem convolutions, down to the 3 clip channels: the gradient with respect to the input clips.
//   slow stem (1,7,7) stride (1,2,2) pad (0,3,3), 64 -> 3;  fast stem (5,7,7) stride (1,2,2) pad (2,3,3), 8 -> 3.
// dz [N][T][Ho][Wo] rows of K floats (pitch ld), wt the host-repacked weight [kt*K][160] (below), dx [N][T][H][W][4], written.
//
//   dx[n,t,h,w,c] = sum_{dt,kh,kw,co} dz[n, t+pt-dt, (h+3-kh)/2, (w+3-kw)/2, co] * w[co,c,dt,kh,kw]     (even h+3-kh, w+3-kw only)
//
// Gather form, one writer per element, no atomics, every sum in a fixed order: the same bits every run.  mt_conv3d_dgrad would fill 4
// of its 64 tile columns here and run the 3 of 4 taps the stride skips; this kernel turns the product round:
//   P[z-pixel, 147 = 49 taps * 3] = A[z-pixel, Kc] . Wt[Kc, 147]       on v_mfma_f32_32x32x2_f32 (147 of 160 columns used)
// with Kc = 64 (slow) or 5 * 8 = 40 (fast: the five temporal taps of one input frame t are five z-frames t+2-dt of the same pixel,
// gathered as extra contraction rows; frames outside the clip are zeros).  Row k = dt*K + co of Wt holds w[co][c][dt][kh][kw] at column
// (kh*7 + kw)*3 + c; columns 147..159 are zero.  A lane reads its pixel's row as float4 pieces (contraction step 4j+e <-> row
// 8j + 4*half + e, so the two halves of a wavefront read adjacent pieces); Wt is read from global memory (40 KB, cache-resident).
//
// One block owns one input frame (n, t), a strip of 29 column pairs and a run of row pairs.  Input row pair (2q, 2q+1) needs z-rows
// q-1 .. q+2 (kh = 5|6, 3|4, 1|2, 0) and column pair p likewise needs z-columns p-1 .. p+2: a strip is 32 z-pixels wide (one MFMA
// tile, 29 + 3 halo).  Per step the four wavefronts form P of four consecutive z-rows (32 pixels x 160 columns each: five
// accumulators) into an LDS ring of 8 row slots (149 floats per pixel: odd pitch), then the block emits the four row pairs that became
// complete as a col2im gather (9..16 taps per element) and stores whole float4 pixels (c = 3 written as 0).  A run re-computes
// the 3 z-rows around it.  Useful multiply-adds = N*T*Ho*Wo*Kc*147.
#include "../../include/mintime_hip.h"
#include "common.hpp"
#include <stdint.h>
#include <algorithm>

namespace {
using namespace mt;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TAPS = 147;                  // 7 * 7 * 3
constexpr int NCOL = 160;                  // columns of Wt (five 32-wide MFMA tiles)
constexpr int PS = 149;                    // LDS floats per z-pixel
constexpr int ZC = 32;                     // z-pixels per strip (one MFMA tile)
constexpr int STRIP = ZC - 3;              // column pairs per strip
constexpr int RING = 8;                    // z-row slots
constexpr int MINROWS = 16;                // a frame is cut into at most ceil(Ho / MINROWS) runs (3 z-rows are re-computed per run)

struct Args {
  const float* dz; const float* wt; float* dx;
  int64_t ld;
  int N, T, H, W, Ho, Wo, strips, chunks, qrows;
};

template <int KT>
__global__ __launch_bounds__(256) void sf_stem_dgrad_kernel(Args p) {
  constexpr int NJ = KT == 1 ? 8 : 5;      // 8-float pieces of a z-pixel's contraction row (Kc = 8 NJ)
  extern __shared__ __attribute__((aligned(16))) float P[];          // [RING][ZC][PS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, cl = lane & 31;
  int64_t b = blockIdx.x;
  const int strip = (int)(b % p.strips);
  b /= p.strips;
  const int chunk = (int)(b % p.chunks);
  const int64_t nt = b / p.chunks;         // n * T + t
  const int t = (int)(nt % p.T);
  const int64_t n = nt / p.T;
  const int q0 = chunk * p.qrows, q1 = min(q0 + p.qrows, p.Ho);      // row pairs [q0, q1)
  const int rb = q0 - 1;                   // first z-row of the run: local row lr = z-row - rb
  const int pc0 = strip * STRIP, pend = min(pc0 + STRIP, p.Wo);      // column pairs [pc0, pend); z-column of pixel j = pc0 - 1 + j
  const int zcl = min(max(pc0 - 1 + cl, 0), p.Wo - 1);               // clamped: pixels off the grid repeat an edge pixel, never gathered
  const int nsteps = (q1 - rb + 1) / 4 + 1;                          // until local pair 4s-2 passes q1 - 1 - rb

  for (int s = 0; s < nsteps; ++s) {
    const int r = rb + 4 * s + wave;       // this wavefront's z-row
    if (r >= 0 && r < p.Ho) {
      float4 a[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (KT == 1) {
          a[j] = *reinterpret_cast<const float4*>(p.dz + ((nt * p.Ho + r) * p.Wo + zcl) * p.ld + 8 * j + 4 * half);
        } else {
          const int tz = t + KT / 2 - j;   // temporal tap dt = j
          a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (tz >= 0 && tz < p.T)
            a[j] = *reinterpret_cast<const float4*>(p.dz + (((n * p.T + tz) * p.Ho + r) * p.Wo + zcl) * p.ld + 4 * half);
        }
      }
      f32x16 acc[5];
#pragma unroll
      for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float av[4] = {a[j].x, a[j].y, a[j].z, a[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* wrow = p.wt + (8 * j + 4 * half + e) * NCOL + cl;
#pragma unroll
          for (int c = 0; c < 5; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], wrow[32 * c], acc[c], 0, 0, 0);
        }
      }
      float* Ps = P + ((4 * s + wave) & (RING - 1)) * (ZC * PS);
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int col = 32 * c + cl;
        if (col < TAPS) {
#pragma unroll
          for (int i = 0; i < 16; ++i) Ps[((i & 3) + 8 * (i >> 2) + 4 * half) * PS + col] = acc[c][i];   // acc[c][i] = P[pixel][col]
        }
      }
    }
    __syncthreads();
    // local row pairs 4s-2 .. 4s+1 are complete: 8 input rows of up to 2 * STRIP pixels
    for (int idx = tid; idx < 8 * 2 * STRIP; idx += 256) {
      const int lrow = idx / (2 * STRIP), wl = idx - lrow * (2 * STRIP);
      const int lq = 4 * s - 2 + (lrow >> 1), rh = lrow & 1;
      const int q = rb + lq, pp = pc0 + (wl >> 1), rw = wl & 1;
      const int h = 2 * q + rh, w = 2 * pp + rw;
      if (lq < 1 || q >= q1 || h >= p.H || pp >= pend || w >= p.W) continue;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      for (int kh = 1 - rh; kh < 7; kh += 2) {
        const int zr = (h + 3 - kh) >> 1;
        if (zr < 0 || zr >= p.Ho) continue;
        const float* Pr = P + ((zr - rb) & (RING - 1)) * (ZC * PS);
        for (int kw = 1 - rw; kw < 7; kw += 2) {
          const int zc = (w + 3 - kw) >> 1;
          if (zc < 0 || zc >= p.Wo) continue;
          const float* e = Pr + (zc - pc0 + 1) * PS + (kh * 7 + kw) * 3;
          a0 += e[0]; a1 += e[1]; a2 += e[2];
        }
      }
      *reinterpret_cast<float4*>(p.dx + (((nt * p.H + h) * p.W) + w) * 4) = make_float4(a0, a1, a2, 0.f);
    }
    __syncthreads();                       // the slots of local rows 4s-4 .. 4s-1 are free for rows 4s+4 .. 4s+7
  }
}

}  // namespace

extern "C" int mt_sf_stem_dgrad(const float* dz, int64_t ldz, const float* wt, float* dx, int N, int T, int H, int W, int kt, int K,
                                void* stream) {
  if (!((kt == 1 && K == 64) || (kt == 5 && K == 8)))
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_stem_dgrad: (kt, K) = (%d, %d) is neither the slow stem (1, 64) nor the fast stem (5, 8)", kt, K);
  if (!dz || !wt || !dx || N <= 0 || T <= 0 || H <= 0 || W <= 0) return fail(MT_ERR_ARG, "mt_sf_stem_dgrad: null pointer or empty shape");
  if ((ldz & 3) || ldz < K || (((uintptr_t)dz | (uintptr_t)dx) & 15) || ((uintptr_t)wt & 3))
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_stem_dgrad: ldz %% 4 == 0, ldz >= K, dz and dx 16-byte aligned");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int strips = (Wo + STRIP - 1) / STRIP;
  const int64_t base = (int64_t)N * T * strips;
  // runs per frame: enough blocks to fill the chip at small N*T, never more than ceil(Ho / MINROWS): runs of about MINROWS row pairs
  // (12 at Ho = 35, 16 at Ho = 128) when frames are few, whole frames once N*T*strips passes 1024
  int chunks = (int)std::max<int64_t>(1, std::min<int64_t>((Ho + MINROWS - 1) / MINROWS, 1024 / base));
  const int qrows = (Ho + chunks - 1) / chunks;
  chunks = (Ho + qrows - 1) / qrows;
  if (base * chunks >= ((int64_t)1 << 31)) return fail(MT_ERR_UNSUPPORTED, "mt_sf_stem_dgrad: too many blocks");
  Args a{dz, wt, dx, ldz, N, T, H, W, Ho, Wo, strips, chunks, qrows};
  const size_t smem = (size_t)RING * ZC * PS * sizeof(float);        // 152576 bytes: one block per CU
  const dim3 grid((unsigned)(base * chunks)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (kt == 1) {
    if (ensure_dynamic_lds((const void*)sf_stem_dgrad_kernel<1>, smem) != hipSuccess)
      return fail(MT_ERR_LAUNCH, "mt_sf_stem_dgrad: LDS attribute");
    hipLaunchKernelGGL(sf_stem_dgrad_kernel<1>, grid, block, smem, st, a);
  } else {
    if (ensure_dynamic_lds((const void*)sf_stem_dgrad_kernel<5>, smem) != hipSuccess)
      return fail(MT_ERR_LAUNCH, "mt_sf_stem_dgrad: LDS attribute");
    hipLaunchKernelGGL(sf_stem_dgrad_kernel<5>, grid, block, smem, st, a);
  }
  return check_launch("mt_sf_stem_dgrad");
}
