// Data gradient of the stems' dense 3x3 stride-2 convolution, 32 -> 3 channels: the gradient with respect to the crops.  Replaces
// torch autograd through _conv_stem (reference efficientnet_pytorch/model.py:173,276, TF-"SAME" static padding) and through
// Xception's conv1 (reference xception.py:161-170, no padding).  du, z [N*Ho*Wo, 32], kabc [3][32] (the operand is formed on load,
// dz = ka*du + kb*z + kc: the BatchNorm backward of the stem's norm), w [32,3,3,3] torch layout, dx [N,H,W,3] fp32, overwritten.
//
//   dx[n,ih,iw,ci] = sum_{kh,kw} sum_co dz[n,oh,ow,co] * w[co,ci,kh,kw]   over the taps with ih+pb-kh = 2 oh, iw+pb-kw = 2 ow
//
// HBM-bound: 256 B read per output pixel (du + z), 12 B written per input pixel -- 0.98 GB for 256 crops of 224^2 -- against
// 2048 flops per output pixel on the matrix pipe.  Gather form, one writer per element, no atomics: the same bits every run.
//
// One block walks a run of consecutive output rows of one image.  Per output row each wavefront takes 32 pixels and forms
//   P[pixel, 27 taps] = dz[pixel, 32] . W[32, 27]      (16 steps of v_mfma_f32_32x32x2_f32, tap = (kh*3 + kw)*3 + ci)
// with both operands in registers: a lane's 16 weights are loop-invariant, and a lane reads its pixel's du / z as four 16-byte
// pieces (the contraction index is permuted so that the two halves of a wavefront read adjacent pieces: step 4j+e <-> channel
// 8j + 4*half + e).  P goes to one of two LDS row slots.  With t = ih + pb, the input row pair (2q, 2q+1) needs the output rows
// q (kh = 0 and kh = 1) and q-1 (kh = 2) only, so after the row q has landed the block emits both input rows as a col2im gather
// from the two slots (at most 4 LDS reads per element) and stores them as whole rows (16-byte stores where 3 W % 4 == 0).  The next
// row's du / z are in flight through the LDS write and the gather.  A run re-computes the one row above it (1 / ROWS more reads).
// Taps that fall outside the output grid read nothing: with no padding and even H or W the last input row / column comes out 0.
// Algorithmic bytes = N*Ho*Wo*32*4*2 + N*H*W*3*4.
#include "common.hpp"
#include <stdint.h>

namespace {
using namespace mt;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CO = 32;
constexpr int MAXW = 512;                  // as the forward (stem_fwd.hip)
constexpr int PP = 28;                     // LDS floats per output pixel: 27 taps + 1 (a half-wavefront's 28 stores hit 28 banks)

struct DgradArgs {
  const float* du; const float* z; const float* kabc; const float* w; float* dx;
  int N, H, W, Ho, Wo, pad0, Q, rows, chunks;      // Q = input row pairs per image, rows = pairs per block, chunks = blocks per image
};

template <int V>                            // V = floats per store (4: every dx row starts on a 16-byte boundary and 3 W % 4 == 0)
__global__ __launch_bounds__(256, 4) void stem_dgrad_kernel(DgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // [2][Wo][PP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, cl = lane & 31;
  const int n = blockIdx.x / p.chunks, chunk = blockIdx.x - n * p.chunks;
  const int q0 = chunk * p.rows, q1 = min(q0 + p.rows, p.Q);
  const int slot_f = p.Wo * PP;

  // B operand (lane = tap cl, contraction index = half) and the BatchNorm-backward coefficients of this lane's 16 channels
  // (kc's share of P is the same for every pixel, sum_co kc[co] w[co, tap]: the accumulators start from it)
  float wr[16], ka[16], kb[16], pc = 0.f;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const int co = 8 * (ks >> 2) + 4 * half + (ks & 3);
    float v = 0.f;
    if (cl < 27) {
      const int ci = cl % 3, kk = cl / 3, kw = kk % 3, kh = kk / 3;
      v = p.w[((co * 3 + ci) * 3 + kh) * 3 + kw];                   // torch layout [co][ci][kh][kw]
    }
    wr[ks] = v;
    ka[ks] = p.kabc[co]; kb[ks] = p.kabc[CO + co];
    pc = fmaf(p.kabc[2 * CO + co], v, pc);
  }
  pc += __shfl_xor(pc, 32);

  // the output rows this block forms: [qa, qb) -- its own and the one above its first
  const int qa = max(q0 - 1, 0), qb = min(q1, p.Ho);
  const int nspan = (p.Wo + 127) >> 7;
  const int steps = (qb - qa) * nspan;       // (row, 128-pixel span) pairs, in order
  float4 a_du[4], a_z[4];
  auto fetch = [&](int step) {               // clamped pixel: lanes past the row load the last pixel again (their results are dropped)
    const int q = qa + step / nspan, span = step - (q - qa) * nspan;
    const int px = min(span * 128 + wave * 32 + cl, p.Wo - 1);
    const int64_t off = (((int64_t)n * p.Ho + q) * p.Wo + px) * CO + 4 * half;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a_du[j] = *reinterpret_cast<const float4*>(p.du + off + 8 * j);
      a_z[j] = *reinterpret_cast<const float4*>(p.z + off + 8 * j);
    }
  };
  int step = 0;
  if (steps > 0) fetch(0);

  const int rowf = p.W * 3;
  for (int q = q0 - 1; q < q1; ++q) {
    if (q >= qa && q < qb) {
      float* P = smem + (q & 1) * slot_f;
      for (int span = 0; span < nspan; ++span, ++step) {
        const int base = span * 128 + wave * 32;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = pc;
        if (base < p.Wo) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d[4] = {a_du[j].x, a_du[j].y, a_du[j].z, a_du[j].w}, zz[4] = {a_z[j].x, a_z[j].y, a_z[j].z, a_z[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int ks = 4 * j + e;
              const float dz = fmaf(ka[ks], d[e], kb[ks] * zz[e]);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz, wr[ks], acc, 0, 0, 0);
            }
          }
        }
        if (step + 1 < steps) fetch(step + 1);                       // uniform; in flight through the LDS write and the gather
        if (base < p.Wo && cl < PP) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int px = base + (r & 3) + 8 * (r >> 2) + 4 * half;  // acc[r] = P[pixel px][tap cl]
            if (px < p.Wo) P[px * PP + cl] = acc[r];
          }
        }
      }
    }
    lds_barrier();
    if (q >= q0) {
      const float* Pq = smem + (q & 1) * slot_f;                     // output row q (taps kh = 0, 1)
      const float* Pm = smem + ((q + 1) & 1) * slot_f;               // output row q - 1 (tap kh = 2)
      const bool vq = q < p.Ho, vm = q >= 1 && q - 1 < p.Ho;
#pragma unroll
      for (int odd = 0; odd < 2; ++odd) {
        const int ih = 2 * q + odd - p.pad0;
        if (ih < 0 || ih >= p.H) continue;                           // uniform
        float* out = p.dx + ((int64_t)n * p.H + ih) * rowf;
        for (int e0 = tid * V; e0 < rowf; e0 += 256 * V) {
          float v[V];
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const int e = e0 + k, iw = e / 3, ci = e - 3 * iw;
            const int s = iw + p.pad0, o = s >> 1;
            // columns: s even -> (kw 0, ow o) and (kw 2, ow o - 1); s odd -> (kw 1, ow o)
            const int kw0 = (s & 1) ? 1 : 0;
            const bool c0 = o < p.Wo, c1 = !(s & 1) && o >= 1 && o - 1 < p.Wo;
            const int i0 = o * PP + kw0 * 3 + ci, i1 = (o - 1) * PP + 6 + ci;
            float acc = 0.f;
            if (odd) {
              if (vq && c0) acc = Pq[i0 + 9];
              if (vq && c1) acc += Pq[i1 + 9];
            } else {
              if (vq && c0) acc = Pq[i0];
              if (vq && c1) acc += Pq[i1];
              if (vm && c0) acc += Pm[i0 + 18];
              if (vm && c1) acc += Pm[i1 + 18];
            }
            v[k] = acc;
          }
          if constexpr (V == 4) *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
          else out[e0] = v[0];
        }
      }
    }
    lds_barrier();                           // the slot of row q - 1 is free for row q + 1
  }
}

}  // namespace

static int stem_conv_dgrad(const float* du, const float* z, const float* kabc, const float* w, float* dx, int N, int H, int W, bool valid,
                           void* stream) {
  const char* name = valid ? "mt_stem_conv_dgrad_valid" : "mt_stem_conv_dgrad";
  if (!du || !z || !kabc || !w || !dx) return fail(MT_ERR_ARG, "%s: null pointer", name);
  if (N <= 0 || H <= 0 || W <= 0 || W > MAXW || (int64_t)N * H > (1 << 30))
    return fail(MT_ERR_ARG, "%s: crops of 1..%d columns, N*H < 2^30", name, MAXW);
  if (valid && (H < 3 || W < 3)) return fail(MT_ERR_ARG, "%s: crops of at least 3 x 3", name);
  if (((uintptr_t)du | (uintptr_t)z) & 15) return fail(MT_ERR_ARG, "%s: du and z must be 16-byte aligned", name);
  // the forward's geometry (stem_fwd.hip)
  const int Ho = valid ? (H - 3) / 2 + 1 : (H + 1) / 2, Wo = valid ? (W - 3) / 2 + 1 : (W + 1) / 2;
  const int padt_h = valid ? 0 : max((Ho - 1) * 2 + 3 - H, 0), padt_w = valid ? 0 : max((Wo - 1) * 2 + 3 - W, 0);
  if (padt_h / 2 != padt_w / 2) return fail(MT_ERR_UNSUPPORTED, "%s: H and W must need the same leading padding", name);
  const int pad0 = padt_h / 2;
  const int Q = ((H - 1 + pad0) >> 1) + 1;                           // pairs (2q, 2q+1) of padded input rows
  // blocks per image: enough blocks to fill the chip at small N, runs of at least 8 pairs (each run re-reads one output row)
  int chunks = 2048 / N;
  chunks = max(1, min(chunks, (Q + 7) / 8));
  const int rows = (Q + chunks - 1) / chunks;
  chunks = (Q + rows - 1) / rows;
  if ((int64_t)N * chunks >= ((int64_t)1 << 31)) return fail(MT_ERR_ARG, "%s: too many crops", name);
  DgradArgs a{du, z, kabc, w, dx, N, H, W, Ho, Wo, pad0, Q, rows, chunks};
  const size_t smem = (size_t)2 * Wo * PP * sizeof(float);           // <= 2 * 256 * 28 * 4 = 57344 bytes
  const dim3 grid((unsigned)(N * chunks)), block(256);
  if ((W * 3) % 4 == 0 && ((uintptr_t)dx & 15) == 0) {
    if (ensure_dynamic_lds((const void*)stem_dgrad_kernel<4>, smem) != hipSuccess) return fail(MT_ERR_LAUNCH, "%s: LDS attribute", name);
    hipLaunchKernelGGL(stem_dgrad_kernel<4>, grid, block, smem, (hipStream_t)stream, a);
  } else {
    if (ensure_dynamic_lds((const void*)stem_dgrad_kernel<1>, smem) != hipSuccess) return fail(MT_ERR_LAUNCH, "%s: LDS attribute", name);
    hipLaunchKernelGGL(stem_dgrad_kernel<1>, grid, block, smem, (hipStream_t)stream, a);
  }
  return check_launch(name);
}

extern "C" int mt_stem_conv_dgrad(const float* du, const float* z, const float* kabc, const float* w, float* dx, int N, int H, int W,
                                  void* stream) {
  return stem_conv_dgrad(du, z, kabc, w, dx, N, H, W, false, stream);
}

extern "C" int mt_stem_conv_dgrad_valid(const float* du, const float* z, const float* kabc, const float* w, float* dx, int N, int H, int W,
                                        void* stream) {
  return stem_conv_dgrad(du, z, kabc, w, dx, N, H, W, true, stream);
}
