// SlowFast clip ingest with the reference's spatial steps (utils.py:166-186): UniformTemporalSubsample, /255, Normalize,
// ShortSideScale (bilinear, align_corners=False, no antialiasing), CenterCropVideo, PackPathway -- one launch for both pathways, and
// its exact adjoint as a gather.  mt_sf_ingest / mt_sf_ingest_bwd (slowfast.hip) are the same pair without the two spatial steps.
//
// The host describes the resize per axis, for the rows and columns of the CROP WINDOW only (window index d <-> resized index
// top + d or left + d):
//   forward  taps:    idx [2][n] (int32: i0 then i1, source indices) and lam [n] (fp32);  value = (1 - lam) x[i0] + lam x[i1]
//   backward sources: start [n_in + 1], out [nnz] (int32: window index), wt [nnz] (fp32: 1 - lam for an i0 reference, lam for an
//                     i1 reference), CSR by source index, window index ascending, i0 before i1
// Both are made from one table (slowfast.py: axis_taps / axis_sources), so the two kernels use the same taps and the same weights.
//
// Forward: one thread per output pixel; each of the four taps is normalised first and the lerp follows, columns then rows:
//   out = h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11),   v = (u / 255 - 0.45) / 0.225
// Backward: one thread per source pixel, summing   wt_h[r] wt_w[c] dout[b][j][r][c]   over the output frames j that selected the
// frame (ascending), the window rows r that reference the source row and the window columns c that reference the source column, in
// list order.  One writer per element, no atomics: the same bits every run; an element nothing references gets exact 0.
//
// Every index read from a table is clamped to its range before it addresses memory.
#include "../../include/mintime_hip.h"
#include "common.hpp"
#include <stdint.h>

namespace {
using namespace mt;

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

template <typename TS>
__global__ __launch_bounds__(256) void ingest_resize_kernel(const TS* __restrict__ src, int64_t sb, int64_t sf, int64_t sh, int64_t sw,
                                                            int64_t sc, const int* __restrict__ fidx, int Tsplit, int Hs, int Ws,
                                                            const int* __restrict__ hidx, const float* __restrict__ hlam,
                                                            const int* __restrict__ widx, const float* __restrict__ wlam, int Ho, int Wo,
                                                            int normalize, float* __restrict__ out, float* __restrict__ out2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Ho * Wo) return;
  const int j = blockIdx.y, Tout = gridDim.y, b = blockIdx.z;
  const int ho = p / Wo, wo = p - ho * Wo;
  const int r0 = clampi(hidx[ho], Hs), r1 = clampi(hidx[Ho + ho], Hs), c0 = clampi(widx[wo], Ws), c1 = clampi(widx[Wo + wo], Ws);
  const float h1 = hlam[ho], h0 = 1.0f - h1, w1 = wlam[wo], w0 = 1.0f - w1;
  const TS* s = src + b * sb + (int64_t)fidx[j] * sf;
  const TS* s00 = s + r0 * sh + c0 * sw;
  const TS* s01 = s + r0 * sh + c1 * sw;
  const TS* s10 = s + r1 * sh + c0 * sw;
  const TS* s11 = s + r1 * sh + c1 * sw;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float t00 = (float)s00[c * sc], t01 = (float)s01[c * sc], t10 = (float)s10[c * sc], t11 = (float)s11[c * sc];
    if (normalize) {
      t00 = (t00 / 255.0f - 0.45f) / 0.225f;
      t01 = (t01 / 255.0f - 0.45f) / 0.225f;
      t10 = (t10 / 255.0f - 0.45f) / 0.225f;
      t11 = (t11 / 255.0f - 0.45f) / 0.225f;
    }
    v[c] = h0 * (w0 * t00 + w1 * t01) + h1 * (w0 * t10 + w1 * t11);
  }
  const int64_t hw = (int64_t)Ho * Wo;
  float* o = j < Tsplit ? out + (((int64_t)b * Tsplit + j) * hw + p) * 4
                        : out2 + (((int64_t)b * (Tout - Tsplit) + (j - Tsplit)) * hw + p) * 4;
  *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], 0.f);
}

__global__ __launch_bounds__(256) void ingest_resize_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dout2,
                                                                const int* __restrict__ fstart, const int* __restrict__ jlist, int Tout,
                                                                int Tsplit, int Hs, int Ws, const int* __restrict__ hstart,
                                                                const int* __restrict__ hout, const float* __restrict__ hwt,
                                                                const int* __restrict__ wstart, const int* __restrict__ wout,
                                                                const float* __restrict__ wwt, int Ho, int Wo, float k, int normalize,
                                                                float* __restrict__ dsrc, int64_t sb, int64_t sf, int64_t sh, int64_t sw,
                                                                int64_t sc) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Hs * Ws) return;
  const int f = blockIdx.y, b = blockIdx.z;
  const int hs = p / Ws, ws = p - hs * Ws;
  const int ra = hstart[hs], rb = hstart[hs + 1], ca = wstart[ws], cb = wstart[ws + 1];
  const int64_t hw = (int64_t)Ho * Wo;
  float a[3] = {0.f, 0.f, 0.f};
  if (ra < rb && ca < cb)
    for (int m = fstart[f]; m < fstart[f + 1]; ++m) {
      const int j = jlist[m];
      const float* d = j < Tsplit ? dout + ((int64_t)b * Tsplit + j) * hw * 4
                                  : dout2 + ((int64_t)b * (Tout - Tsplit) + (j - Tsplit)) * hw * 4;
      for (int r = ra; r < rb; ++r) {
        const float wr = hwt[r];
        const float* row = d + (int64_t)clampi(hout[r], Ho) * Wo * 4;
        for (int c = ca; c < cb; ++c) {
          const float w = wr * wwt[c];
          const float4 g = *reinterpret_cast<const float4*>(row + (int64_t)clampi(wout[c], Wo) * 4);
          a[0] += w * g.x; a[1] += w * g.y; a[2] += w * g.z;
        }
      }
    }
  float* o = dsrc + b * sb + f * sf + hs * sh + ws * sw;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * sc] = normalize ? a[c] * k : a[c];
}

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
constexpr int64_t kMaxPixels = ((int64_t)1 << 31) - 256;      // a block's pixel index (blockIdx.x * 256 + threadIdx.x) stays an int

// the crop window [top, top + Ho) x [left, left + Wo) lies inside the resized Hr x Wr frame
bool window_ok(int Hr, int Wr, int top, int left, int Ho, int Wo) {
  return Hr > 0 && Wr > 0 && Ho > 0 && Wo > 0 && top >= 0 && left >= 0 && (int64_t)top + Ho <= Hr && (int64_t)left + Wo <= Wr;
}

}  // namespace

extern "C" int mt_sf_ingest_resize(const void* src, int is_u8, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc, const int* fidx,
                                   int Tout, int Tsplit, int B, int Hs, int Ws, const int* hidx, const float* hlam, const int* widx,
                                   const float* wlam, int Hr, int Wr, int top, int left, int Ho, int Wo, int normalize, float* out,
                                   float* out2, void* stream) {
  if (!src || !fidx || !hidx || !hlam || !widx || !wlam || !out || Tout <= 0 || B <= 0 || Hs <= 0 || Ws <= 0 || Tsplit <= 0 ||
      Tsplit > Tout || (Tsplit < Tout && !out2))
    return fail(MT_ERR_ARG, "mt_sf_ingest_resize: null pointer or empty shape");
  if (!window_ok(Hr, Wr, top, left, Ho, Wo))
    return fail(MT_ERR_ARG, "mt_sf_ingest_resize: crop window %d+%d x %d+%d outside the resized %d x %d frame", top, Ho, left, Wo, Hr, Wr);
  if (((uintptr_t)out | (uintptr_t)(out2 ? out2 : out)) & 15)
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest_resize: outputs must be 16-byte aligned");
  if (Tout > 65535 || B > 65535 || (int64_t)Ho * Wo > kMaxPixels)
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest_resize: more than 65535 frames or clips, or a window of 2^31 pixels");
  const dim3 grid(blocks((int64_t)Ho * Wo), Tout, B);
  const hipStream_t st = (hipStream_t)stream;
  if (is_u8)
    hipLaunchKernelGGL(ingest_resize_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)src, sb, sf, sh, sw, sc, fidx, Tsplit, Hs, Ws,
                       hidx, hlam, widx, wlam, Ho, Wo, normalize, out, out2);
  else
    hipLaunchKernelGGL(ingest_resize_kernel<float>, grid, dim3(256), 0, st, (const float*)src, sb, sf, sh, sw, sc, fidx, Tsplit, Hs, Ws,
                       hidx, hlam, widx, wlam, Ho, Wo, normalize, out, out2);
  return check_launch("mt_sf_ingest_resize");
}

extern "C" int mt_sf_ingest_resize_bwd(const float* dout, const float* dout2, const int* fstart, const int* jlist, int F, int Tout,
                                       int Tsplit, int B, int Hs, int Ws, const int* hstart, const int* hout, const float* hwt,
                                       const int* wstart, const int* wout, const float* wwt, int Hr, int Wr, int top, int left, int Ho,
                                       int Wo, int normalize, float* dsrc, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc,
                                       void* stream) {
  if (!dout || !fstart || !jlist || !hstart || !hout || !hwt || !wstart || !wout || !wwt || !dsrc || F <= 0 || Tout <= 0 || B <= 0 ||
      Hs <= 0 || Ws <= 0 || Tsplit <= 0 || Tsplit > Tout || (Tsplit < Tout && !dout2))
    return fail(MT_ERR_ARG, "mt_sf_ingest_resize_bwd: null pointer or empty shape");
  if (!window_ok(Hr, Wr, top, left, Ho, Wo))
    return fail(MT_ERR_ARG, "mt_sf_ingest_resize_bwd: crop window %d+%d x %d+%d outside the resized %d x %d frame", top, Ho, left, Wo, Hr,
                Wr);
  if (((uintptr_t)dout | (uintptr_t)(dout2 ? dout2 : dout)) & 15)
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest_resize_bwd: dout and dout2 must be 16-byte aligned");
  if (F > 65535 || B > 65535 || (int64_t)Hs * Ws > kMaxPixels)
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest_resize_bwd: more than 65535 frames or clips, or a frame of 2^31 pixels");
  const float k = (float)(1.0 / (255.0 * 0.225));
  hipLaunchKernelGGL(ingest_resize_bwd_kernel, dim3(blocks((int64_t)Hs * Ws), F, B), dim3(256), 0, (hipStream_t)stream, dout, dout2, fstart,
                     jlist, Tout, Tsplit, Hs, Ws, hstart, hout, hwt, wstart, wout, wwt, Ho, Wo, k, normalize, dsrc, sb, sf, sh, sw, sc);
  return check_launch("mt_sf_ingest_resize_bwd");
}
