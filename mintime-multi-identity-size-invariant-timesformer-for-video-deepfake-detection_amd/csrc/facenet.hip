// FaceNet InceptionResnetV1 (inference): the kernels of the face embedder in front of the identity clustering (csrc/identity.hip).
//   mt_conv2d_fwd         Conv2d as an implicit GEMM on v_mfma_f32_32x32x2_f32 with the whole block tail in the epilogue:
//                           y = act(conv + bias)                       (res NULL)
//                           y = act(res + res_scale * (conv + bias))   (the Inception-ResNet blocks)
//   mt_face_ingest        uint8 / fp32 crops, any element strides -> [T][H][W][4] fp32 rows, (u - 127.5) / 128 or passthrough
//   mt_maxpool2d_fwd      MaxPool2d(3, 2) over pitched rows (writes its slice of a concatenation buffer)
//   mt_avgpool_rows       AdaptiveAvgPool2d(1): the mean of each face's rows, in row order
//   mt_l2_normalize_rows  x / max(||x||, eps)
// Activations are channels-last rows with a row pitch, weights are [K][kh][kw][C] (BatchNorm folded by the host).  One block of
// mt_conv2d_fwd owns a 64 x 64 output tile and walks the WHOLE reduction (tap-major, channel-minor, 32 per step) by itself: there is
// no split of the reduction and no atomic, so the order of every sum depends on the layer's geometry alone and never on how many
// faces share the launch.  Against csrc/conv3d.hip's forward: the epilogue carries bias / residual / ReLU, rows are decoded once per
// thread in 32-bit arithmetic, the tap walk is incremental (no division in the loop), eight threads read 128 contiguous bytes of a
// row, and the next step's global loads are in flight under the current step's MFMAs (LDS is double-buffered, one barrier a step).
#include "../../include/mintime_hip.h"
#include "common.hpp"

using namespace mt;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 32;   // block tile (4 wavefronts, 32 x 32 each) and K step (16 MFMAs of K = 2)
constexpr int LS = BM + 2;                 // LDS row stride: the 8 k-groups of a wavefront's writes fall on 4 bank groups

struct Geo {
  int M, HoWo, Wo, H, W, C, K, KD, kw, sh, sw, ph, pw, act;
  float res_scale;
  int64_t ldx, ldy, ldr;
};

// where output row m reads: first input row of its face, top-left tap position (may be negative: padding)
struct RowSrc {
  int64_t base;
  int hi0, wi0;
  bool ok;
};

__device__ __forceinline__ RowSrc row_src(const Geo& g, int m) {
  RowSrc r;
  r.ok = m < g.M;
  const unsigned mm = r.ok ? (unsigned)m : 0u, n = mm / (unsigned)g.HoWo, rem = mm - n * (unsigned)g.HoWo;
  const unsigned ho = rem / (unsigned)g.Wo, wo = rem - ho * (unsigned)g.Wo;
  r.base = (int64_t)n * g.H * g.W;
  r.hi0 = (int)ho * g.sh - g.ph;
  r.wi0 = (int)wo * g.sw - g.pw;
  return r;
}

// four consecutive input channels ci.. that tap (b, c) of the row reads; zero for padding, rows past M and k past the reduction
__device__ __forceinline__ float4 gather(const Geo& g, const float* __restrict__ x, const RowSrc& r, int b, int c, int ci, bool kin) {
  const int hi = r.hi0 + b, wi = r.wi0 + c;
  if (!kin || !r.ok || hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return f4(0.f, 0.f, 0.f, 0.f);
  return ld4(x + (r.base + (int64_t)hi * g.W + wi) * g.ldx + ci);
}

__device__ __forceinline__ void put4(float (*S)[LS], int k, int col, float4 v) {
  S[k + 0][col] = v.x; S[k + 1][col] = v.y; S[k + 2][col] = v.z; S[k + 3][col] = v.w;
}

__global__ __launch_bounds__(256) void conv2d_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ res, float* __restrict__ y) {
  __shared__ float As[2][BK][LS], Bs[2][BK][LS];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int ar = t >> 3, ag = t & 7;           // rows / columns ar and ar + 32, k group ag (4 consecutive k)
  const RowSrc r0 = row_src(g, m0 + ar), r1 = row_src(g, m0 + ar + 32);
  const bool c0 = n0 + ar < g.K, c1 = n0 + ar + 32 < g.K;
  const float* w0 = w + (int64_t)(c0 ? n0 + ar : 0) * g.KD;
  const float* w1 = w + (int64_t)(c1 ? n0 + ar + 32 : 0) * g.KD;
  // (tap row b, tap column c, channel ci) of this thread's k, advanced by BK a step
  int k = ag * 4;
  int tap = k / g.C, ci = k - tap * g.C, b = tap / g.kw, c = tap - b * g.kw;
  const float4 zero = f4(0.f, 0.f, 0.f, 0.f);
  float4 a0, a1, b0, b1;
  {
    const bool kin = k < g.KD;
    a0 = gather(g, x, r0, b, c, ci, kin);
    a1 = gather(g, x, r1, b, c, ci, kin);
    b0 = kin && c0 ? ld4(w0 + k) : zero;
    b1 = kin && c1 ? ld4(w1 + k) : zero;
  }
  put4(As[0], ag * 4, ar, a0); put4(As[0], ag * 4, ar + 32, a1);
  put4(Bs[0], ag * 4, ar, b0); put4(Bs[0], ag * 4, ar + 32, b1);
  __syncthreads();
  f32x16 acc = {};
  const int r = lane & 31, h = lane >> 5;
  int cur = 0;
  for (int k0 = 0; k0 < g.KD; k0 += BK) {
    const bool more = k0 + BK < g.KD;
    if (more) {                                // the next step's operands: loads in flight under this step's MFMAs
      k += BK;
      ci += BK;
      while (ci >= g.C) {
        ci -= g.C;
        if (++c == g.kw) { c = 0; ++b; }
      }
      const bool kin = k < g.KD;
      a0 = gather(g, x, r0, b, c, ci, kin);
      a1 = gather(g, x, r1, b, c, ci, kin);
      b0 = kin && c0 ? ld4(w0 + k) : zero;
      b1 = kin && c1 ? ld4(w1 + k) : zero;
    }
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[cur][2 * kk + h][wm * 32 + r], Bs[cur][2 * kk + h][wn * 32 + r], acc, 0, 0, 0);
    if (more) {
      put4(As[cur ^ 1], ag * 4, ar, a0); put4(As[cur ^ 1], ag * 4, ar + 32, a1);
      put4(Bs[cur ^ 1], ag * 4, ar, b0); put4(Bs[cur ^ 1], ag * 4, ar + 32, b1);
    }
    __syncthreads();
    cur ^= 1;
  }
  const int col = n0 + wn * 32 + r;
  if (col < g.K) {
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = m0 + wm * 32 + mfma_slot_row(i, h);
      if (row < g.M) {
        float v = acc[i] + bv;
        if (res) v = res[(int64_t)row * g.ldr + col] + g.res_scale * v;
        if (g.act) v = fmaxf(v, 0.f);
        y[(int64_t)row * g.ldy + col] = v;
      }
    }
  }
}

// one thread per pixel: three source elements -> one float4
template <typename TS>
__global__ __launch_bounds__(256) void ingest_kernel(const TS* __restrict__ src, int64_t st, int64_t sh, int64_t sw, int64_t sc, int64_t pixels,
                                                     int H, int W, int standardize, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const int64_t hw = (int64_t)H * W, n = p / hw, rem = p - n * hw, hh = rem / W, ww = rem - hh * W;
  const TS* s = src + n * st + hh * sh + ww * sw;
  float v0 = (float)s[0], v1 = (float)s[sc], v2 = (float)s[2 * sc];
  if (standardize) {
    v0 = (v0 - 127.5f) * 0.0078125f; v1 = (v1 - 127.5f) * 0.0078125f; v2 = (v2 - 127.5f) * 0.0078125f;      // / 128, exact
  }
  st4(out + p * 4, f4(v0, v1, v2, 0.f));
}

// one thread per (output row, 4 channels)
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int H, int W,
                                                      int Ho, int Wo, int C4, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const int64_t row = i / C4, how = (int64_t)Ho * Wo, n = row / how, rem = row - n * how;
  const int ho = (int)(rem / Wo), wo = (int)(rem - (int64_t)ho * Wo);
  const float* p = x + ((n * H + 2 * ho) * W + 2 * wo) * ldx + c;
  float4 m = ld4(p);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float4 v = ld4(p + ((int64_t)a * W + b) * ldx);
      m = f4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
    }
  st4(y + row * ldy + c, m);
}

// one thread per (face, channel): the rows of a face in ascending order, then one division
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int rows, int C,
                                                      int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t n = i / C;
  const int c = (int)(i - n * C);
  const float* p = x + n * rows * ldx + c;
  float s = 0.f;
  for (int q = 0; q < rows; ++q) s += p[(int64_t)q * ldx];
  y[n * ldy + c] = s / (float)rows;
}

// one wavefront per row
__global__ __launch_bounds__(256) void l2norm_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int64_t rows, int D,
                                                     float eps) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* p = x + row * ldx;
  float s = 0.f;
  for (int j = lane; j < D; j += 64) s = fmaf(p[j], p[j], s);
  s = wave_sum(s);
  const float d = fmaxf(sqrtf(s), eps);
  for (int j = lane; j < D; j += 64) y[row * ldy + j] = p[j] / d;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mt_conv2d_fwd(const mt_conv2d_desc* d, const float* x, const float* w, const float* bias, const float* res, float* y,
                             void* stream) {
  const char* what = "mt_conv2d_fwd";
  if (!d) return fail(MT_ERR_ARG, "%s: null descriptor", what);
  if (!x || !w || !y) return fail(MT_ERR_ARG, "%s: null pointer", what);
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kh <= 0 || d->kw <= 0 || d->sh <= 0 || d->sw <= 0 || d->ph < 0 ||
      d->pw < 0)
    return fail(MT_ERR_ARG, "%s: empty or negative shape", what);
  if (d->Ho <= 0 || d->Wo <= 0 || d->Ho != (d->H + 2 * d->ph - d->kh) / d->sh + 1 || d->Wo != (d->W + 2 * d->pw - d->kw) / d->sw + 1 ||
      d->H + 2 * d->ph < d->kh || d->W + 2 * d->pw < d->kw)
    return fail(MT_ERR_ARG, "%s: output grid %dx%d does not match the input, kernel, stride and padding", what, d->Ho, d->Wo);
  if (d->act != 0 && d->act != 1) return fail(MT_ERR_ARG, "%s: act is 0 (none) or 1 (ReLU)", what);
  if ((d->C & 3) || (d->K & 3) || (d->ldx & 3) || (d->ldy & 3) || d->ldx < d->C || d->ldy < d->K || (res && ((d->ldr & 3) || d->ldr < d->K)))
    return fail(MT_ERR_UNSUPPORTED, "%s: C, K and the row pitches must be multiples of 4, pitches >= widths", what);
  if (!al16(x) || !al16(w) || ((uintptr_t)y & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)res & 3))
    return fail(MT_ERR_UNSUPPORTED, "%s: x and w must be 16-byte aligned", what);
  const int64_t M = (int64_t)d->N * d->Ho * d->Wo, KD = (int64_t)d->kh * d->kw * d->C;
  if (M > 0x7fffffff - BM || (int64_t)d->N * d->H * d->W > 0x7fffffff || KD > (1 << 24))
    return fail(MT_ERR_UNSUPPORTED, "%s: more than 2^31 rows or a reduction longer than 2^24", what);
  Geo g;
  g.M = (int)M; g.HoWo = d->Ho * d->Wo; g.Wo = d->Wo; g.H = d->H; g.W = d->W; g.C = d->C; g.K = d->K; g.KD = (int)KD; g.kw = d->kw;
  g.sh = d->sh; g.sw = d->sw; g.ph = d->ph; g.pw = d->pw; g.act = d->act; g.res_scale = d->res_scale;
  g.ldx = d->ldx; g.ldy = d->ldy; g.ldr = d->ldr;
  const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((d->K + BN - 1) / BN));
  hipLaunchKernelGGL(conv2d_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, x, w, bias, res, y);
  return check_launch(what);
}

extern "C" int mt_face_ingest(const void* src, int is_u8, int64_t st, int64_t sh, int64_t sw, int64_t sc, int T, int H, int W, int standardize,
                              float* out, void* stream) {
  if (!src || !out) return fail(MT_ERR_ARG, "mt_face_ingest: null pointer");
  if (T <= 0 || H <= 0 || W <= 0) return fail(MT_ERR_ARG, "mt_face_ingest: empty shape");
  if (st < 0 || sh < 0 || sw < 0 || sc < 0) return fail(MT_ERR_UNSUPPORTED, "mt_face_ingest: negative strides");
  if (!al16(out) || (!is_u8 && ((uintptr_t)src & 3))) return fail(MT_ERR_UNSUPPORTED, "mt_face_ingest: out must be 16-byte aligned");
  const int64_t pixels = (int64_t)T * H * W;
  if (pixels > ((int64_t)1 << 37)) return fail(MT_ERR_UNSUPPORTED, "mt_face_ingest: too many pixels");
  const dim3 grid((unsigned)((pixels + 255) / 256));
  if (is_u8)
    hipLaunchKernelGGL(ingest_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, st, sh, sw, sc, pixels, H, W,
                       standardize, out);
  else
    hipLaunchKernelGGL(ingest_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, st, sh, sw, sc, pixels, H, W,
                       standardize, out);
  return check_launch("mt_face_ingest");
}

extern "C" int mt_maxpool2d_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, int N, int H, int W, int C, int k, int s, int p,
                                void* stream) {
  if (!x || !y) return fail(MT_ERR_ARG, "mt_maxpool2d_fwd: null pointer");
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(MT_ERR_ARG, "mt_maxpool2d_fwd: empty shape");
  if (k != 3 || s != 2 || p != 0) return fail(MT_ERR_UNSUPPORTED, "mt_maxpool2d_fwd: only kernel 3, stride 2, padding 0");
  if (H < 3 || W < 3) return fail(MT_ERR_ARG, "mt_maxpool2d_fwd: the input is smaller than the window");
  if ((C & 3) || (ldx & 3) || (ldy & 3) || ldx < C || ldy < C || !al16(x) || !al16(y))
    return fail(MT_ERR_UNSUPPORTED, "mt_maxpool2d_fwd: C and the pitches must be multiples of 4, x and y 16-byte aligned");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
  if (total > ((int64_t)1 << 37)) return fail(MT_ERR_UNSUPPORTED, "mt_maxpool2d_fwd: too many elements");
  hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, H, W, Ho, Wo,
                     C / 4, total);
  return check_launch("mt_maxpool2d_fwd");
}

extern "C" int mt_avgpool_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int N, int rows, int C, void* stream) {
  if (!x || !y) return fail(MT_ERR_ARG, "mt_avgpool_rows: null pointer");
  if (N <= 0 || rows <= 0 || C <= 0 || ldx < C || ldy < C) return fail(MT_ERR_ARG, "mt_avgpool_rows: empty shape or a pitch below the width");
  const int64_t total = (int64_t)N * C;
  hipLaunchKernelGGL(avgpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, rows, C, total);
  return check_launch("mt_avgpool_rows");
}

extern "C" int mt_l2_normalize_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int D, float eps, void* stream) {
  if (!x || !y) return fail(MT_ERR_ARG, "mt_l2_normalize_rows: null pointer");
  if (rows <= 0 || D <= 0 || ldx < D || ldy < D || rows > ((int64_t)1 << 32))
    return fail(MT_ERR_ARG, "mt_l2_normalize_rows: empty shape or a pitch below the width");
  hipLaunchKernelGGL(l2norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, rows, D, eps);
  return check_launch("mt_l2_normalize_rows");
}
