// SlowFast R50 (pytorchvideo slowfast_r50, reference train.py:143-147, `--model 2`): everything around the 3-D convolutions
// (conv3d.hip).  BatchNorm3d + ReLU + residual, the stems' MaxPool3d, the head (window AvgPool3d, dropout, proj, output mean) and the
// clip ingest (utils.py:166-186).  All tensors are channels-last rows with an explicit row pitch, so that a pathway's channel slice of
// a concatenated tensor is addressed in place.  No kernel issues an atomic; every sum runs in a fixed order.
#include "../../include/mintime_hip.h"
#include "common.hpp"

using namespace mt;

namespace mt {
int colsum_stats(const float* part, int64_t rows, int cols, double* mid, double* stats, hipStream_t st);
int64_t colsum_mid_floats(int64_t rows, int cols);
}

namespace {

// ---- BatchNorm + ReLU (+ residual) ----------------------------------------------------------------------------------------------
// y = relu(z * scale + shift + r), r = res * rscale + rshift (rscale given: the shortcut's own BatchNorm), res (identity), or 0
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ res, int64_t ldr,
                                                          const float* __restrict__ rscale, const float* __restrict__ rshift,
                                                          float* __restrict__ y, int64_t ldy, int64_t rows, int C) {
  const int CQ = C >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * CQ) return;
  const int64_t r = i / CQ;
  const int c = (int)(i - r * CQ) * 4;
  const float4 v = *reinterpret_cast<const float4*>(z + r * ldz + c);
  const float4 s = *reinterpret_cast<const float4*>(scale + c), b = *reinterpret_cast<const float4*>(shift + c);
  float4 o = make_float4(fmaf(v.x, s.x, b.x), fmaf(v.y, s.y, b.y), fmaf(v.z, s.z, b.z), fmaf(v.w, s.w, b.w));
  if (res) {
    float4 q = *reinterpret_cast<const float4*>(res + r * ldr + c);
    if (rscale) {
      const float4 rs = *reinterpret_cast<const float4*>(rscale + c), rb = *reinterpret_cast<const float4*>(rshift + c);
      q = make_float4(fmaf(q.x, rs.x, rb.x), fmaf(q.y, rs.y, rb.y), fmaf(q.z, rs.z, rb.z), fmaf(q.w, rs.w, rb.w));
    }
    o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
  }
  *reinterpret_cast<float4*>(y + r * ldy + c) =
      make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
}

// du = g * mask, mask = (z * scale + shift > 0) when scale is given, (m > 0) when m is given, else 1
__device__ __forceinline__ float masked(float g, const float* z, const float* scale, const float* shift, const float* m, int64_t r,
                                        int64_t ldz, int64_t ldm, int c) {
  if (scale) return fmaf(z[r * ldz + c], scale[c], shift[c]) > 0.f ? g : 0.f;
  if (m) return m[r * ldm + c] > 0.f ? g : 0.f;
  return g;
}

constexpr int kStatCols = 64, kStatRowsPerBlock = 256;

// part[blk][0][c] = sum du, part[blk][1][c] = sum du * (z - mean) * invstd over the block's rows (block = 64 channels x 4 row lanes)
__global__ __launch_bounds__(256) void bn_relu_bwd_stats_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ z,
                                                                int64_t ldz, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ m, int64_t ldm, const float* __restrict__ mi,
                                                                float* __restrict__ part, int64_t rows, int C) {
  __shared__ float red[4][2][kStatCols];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.y * kStatCols + cl;
  const int64_t r0 = (int64_t)blockIdx.x * kStatRowsPerBlock, r1 = min(rows, r0 + kStatRowsPerBlock);
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float mean = mi[c], istd = mi[C + c];
    for (int64_t r = r0 + rg; r < r1; r += 4) {
      const float du = masked(g[r * ldg + c], z, scale, shift, m, r, ldz, ldm, c);
      s1 += du;
      s2 = fmaf(du, (z[r * ldz + c] - mean) * istd, s2);
    }
  }
  red[rg][0][cl] = s1;
  red[rg][1][cl] = s2;
  __syncthreads();
  if (rg < 2 && c < C)
    part[((int64_t)blockIdx.x * 2 + rg) * C + c] = ((red[0][rg][cl] + red[1][rg][cl]) + red[2][rg][cl]) + red[3][rg][cl];
}

// out = ka * du + kb * z + kc (kabc given: the BatchNorm adjoint of mt_bn_bwd_finalize) or du; accumulate adds to out
__global__ __launch_bounds__(256) void bn_relu_bwd_apply_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ z,
                                                                int64_t ldz, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ m, int64_t ldm, const float* __restrict__ kabc,
                                                                float* __restrict__ out, int64_t ldo, int accumulate, int64_t rows, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const int64_t r = i / C;
  const int c = (int)(i - r * C);
  float v = masked(g[r * ldg + c], z, scale, shift, m, r, ldz, ldm, c);
  if (kabc) v = fmaf(kabc[c], v, fmaf(kabc[C + c], z[r * ldz + c], kabc[2 * C + c]));
  float* o = out + r * ldo + c;
  *o = accumulate ? *o + v : v;
}

// ---- stem MaxPool3d((1,3,3), (1,2,2), (0,1,1)) over relu(z * scale + shift) --------------------------------------------------------
// out row (n, t, ho, wo): the first maximum in (kh, kw) order, as torch's max_pool3d; arg = h * W + w of that input (int32)
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ out, int64_t ldo,
                                                          int* __restrict__ arg, int64_t NT, int H, int W, int Ho, int Wo, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= NT * Ho * Wo * C) return;
  const int c = (int)(i % C);
  int64_t r = i / C;
  const int wo = (int)(r % Wo), ho = (int)((r / Wo) % Ho);
  const int64_t nt = r / ((int64_t)Wo * Ho);
  const float s = scale[c], b = shift[c];
  float best = -INFINITY;
  int bi = 0;
  for (int dh = 0; dh < 3; ++dh) {
    const int h = ho * 2 - 1 + dh;
    if (h < 0 || h >= H) continue;
    for (int dw = 0; dw < 3; ++dw) {
      const int w = wo * 2 - 1 + dw;
      if (w < 0 || w >= W) continue;
      const float v = fmaxf(fmaf(z[((nt * H + h) * W + w) * C + c], s, b), 0.f);
      if (v > best) { best = v; bi = h * W + w; }
    }
  }
  out[r * ldo + c] = best;
  arg[r * C + c] = bi;
}

// din[n, t, h, w, c] = sum of dout over the windows whose recorded maximum is this element (a gather: one writer per element)
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dout, int64_t ldd, const int* __restrict__ arg,
                                                          float* __restrict__ din, int64_t NT, int H, int W, int Ho, int Wo, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= NT * H * W * C) return;
  const int c = (int)(i % C);
  const int64_t r = i / C;
  const int w = (int)(r % W), h = (int)((r / W) % H);
  const int64_t nt = r / ((int64_t)W * H);
  const int me = h * W + w;
  float a = 0.f;
  for (int ho = max(0, h / 2); ho <= min(Ho - 1, (h + 1) / 2); ++ho)
    for (int wo = max(0, w / 2); wo <= min(Wo - 1, (w + 1) / 2); ++wo) {
      if (ho * 2 - 1 > h || ho * 2 + 1 < h || wo * 2 - 1 > w || wo * 2 + 1 < w) continue;
      const int64_t o = (nt * Ho + ho) * Wo + wo;
      if (arg[o * C + c] == me) a += dout[o * ldd + c];
    }
  din[i] = a;
}

// ---- head ---------------------------------------------------------------------------------------------------------------------
// d[b][p][coff + c] = mult[b][p][coff + c] * mean of feat over window p (AvgPool3d, stride 1, no padding); p = (pt, ph, pw) row-major
__global__ __launch_bounds__(256) void head_pool_kernel(const float* __restrict__ feat, int64_t ldf, const float* __restrict__ mult,
                                                        float* __restrict__ d, int B, int T, int H, int W, int C, int kt, int kh, int kw,
                                                        int Pt, int Ph, int Pw, int coff, int CT) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int P = Pt * Ph * Pw;
  if (i >= (int64_t)B * P * C) return;
  const int c = (int)(i % C);
  const int p = (int)((i / C) % P), b = (int)(i / ((int64_t)C * P));
  const int pw = p % Pw, ph = (p / Pw) % Ph, pt = p / (Pw * Ph);
  float a = 0.f;
  for (int t = pt; t < pt + kt; ++t)
    for (int h = ph; h < ph + kh; ++h)
      for (int w = pw; w < pw + kw; ++w) a += feat[((((int64_t)b * T + t) * H + h) * W + w) * ldf + c];
  const int64_t o = ((int64_t)b * P + p) * CT + coff + c;
  const float v = a / (float)(kt * kh * kw);
  d[o] = mult ? v * mult[o] : v;
}

// logits[b][j] = bias[j] + (1 / P) sum_p sum_c W[j][c] d[b][p][c]: one wavefront per (b, j)
__global__ __launch_bounds__(256) void head_proj_kernel(const float* __restrict__ d, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ logits, int B, int P, int CT, int J) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (int64_t)B * J) return;
  const int b = (int)(idx / J), j = (int)(idx % J);
  float tot = 0.f;
  for (int p = 0; p < P; ++p) {
    const float* dp = d + ((int64_t)b * P + p) * CT;
    float a = 0.f;
    for (int c = lane; c < CT; c += 64) a = fmaf(w[(int64_t)j * CT + c], dp[c], a);
    tot += wave_sum(a);
  }
  if (lane == 0) logits[idx] = (bias ? bias[j] : 0.f) + tot / (float)P;
}

// dW[j][c] = (1 / P) sum_b g[b][j] sum_p d[b][p][c] (accumulated); db[j] = sum_b g[b][j] (accumulated, column c == CT)
__global__ __launch_bounds__(256) void head_params_kernel(const float* __restrict__ g, const float* __restrict__ d, float* __restrict__ dw,
                                                          float* __restrict__ db, int B, int P, int CT, int J) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)J * (CT + 1)) return;
  const int j = (int)(i / (CT + 1)), c = (int)(i % (CT + 1));
  float a = 0.f;
  if (c < CT) {
    if (!dw) return;
    for (int b = 0; b < B; ++b) {
      float s = 0.f;
      for (int p = 0; p < P; ++p) s += d[((int64_t)b * P + p) * CT + c];
      a = fmaf(g[(int64_t)b * J + j], s, a);
    }
    dw[(int64_t)j * CT + c] += a / (float)P;
  } else {
    if (!db) return;
    for (int b = 0; b < B; ++b) a += g[(int64_t)b * J + j];
    db[j] += a;
  }
}

// dpool[b][p][c] = mult[b][p][c] (1 / P) sum_j g[b][j] W[j][c]
__global__ __launch_bounds__(256) void head_dpool_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ mult,
                                                         float* __restrict__ dpool, int B, int P, int CT, int J) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * CT) return;
  const int b = (int)(i / CT), c = (int)(i % CT);
  float a = 0.f;
  for (int j = 0; j < J; ++j) a = fmaf(g[(int64_t)b * J + j], w[(int64_t)j * CT + c], a);
  a /= (float)P;
  for (int p = 0; p < P; ++p) {
    const int64_t o = ((int64_t)b * P + p) * CT + c;
    dpool[o] = mult ? a * mult[o] : a;
  }
}

// dfeat[b, t, h, w, c] = sum over the windows p that hold (t, h, w) of dpool[b][p][coff + c] / window volume (a gather)
__global__ __launch_bounds__(256) void head_dfeat_kernel(const float* __restrict__ dpool, float* __restrict__ dfeat, int64_t ldf, int B, int T,
                                                         int H, int W, int C, int kt, int kh, int kw, int Pt, int Ph, int Pw, int coff,
                                                         int CT) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * T * H * W * C) return;
  const int c = (int)(i % C);
  const int64_t r = i / C;
  const int w = (int)(r % W), h = (int)((r / W) % H), t = (int)((r / ((int64_t)W * H)) % T);
  const int b = (int)(r / ((int64_t)W * H * T));
  const int P = Pt * Ph * Pw;
  float a = 0.f;
  for (int pt = max(0, t - kt + 1); pt <= min(Pt - 1, t); ++pt)
    for (int ph = max(0, h - kh + 1); ph <= min(Ph - 1, h); ++ph)
      for (int pw = max(0, w - kw + 1); pw <= min(Pw - 1, w); ++pw)
        a += dpool[((int64_t)b * P + (pt * Ph + ph) * Pw + pw) * CT + coff + c];
  dfeat[r * ldf + c] = a / (float)(kt * kh * kw);
}

// ---- ingest ---------------------------------------------------------------------------------------------------------------------
// Frame j of the Tout listed in fidx: v(src[b][fidx[j]][h][w][c]) for c < 3 and 0 for c = 3, as one float4, into out[b][j] (j < Tsplit)
// or out2[b][j - Tsplit]; v = (u / 255 - 0.45) / 0.225 when normalize (the reference's fp32 arithmetic), else the value as it is.
// Element strides of src (b, f, h, w, c) are given.  Both pathways of a clip batch come from one launch.
template <typename TS>
__global__ __launch_bounds__(256) void ingest_kernel(const TS* __restrict__ src, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc,
                                                     const int* __restrict__ fidx, int Tout, int Tsplit, int B, int H, int W, int normalize,
                                                     float* __restrict__ out, float* __restrict__ out2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * Tout * H * W) return;
  const int64_t hw = (int64_t)H * W;
  const int64_t p = i % hw;
  const int w = (int)(p % W), h = (int)(p / W), j = (int)((i / hw) % Tout);
  const int b = (int)(i / (hw * Tout));
  const TS* s = src + b * sb + (int64_t)fidx[j] * sf + h * sh + w * sw;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float u = (float)s[c * sc];
    v[c] = normalize ? (u / 255.0f - 0.45f) / 0.225f : u;
  }
  float* o = j < Tsplit ? out + (((int64_t)b * Tsplit + j) * hw + p) * 4
                        : out2 + (((int64_t)b * (Tout - Tsplit) + (j - Tsplit)) * hw + p) * 4;
  *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], 0.f);
}

// The ingest's adjoint: dsrc[b][f][h][w][c] = k * sum of dout_j[b][.][h][w][c] over the output frames j that selected f, in the order
// jlist[start[f] .. start[f+1]) lists them (ascending j); a frame nobody selected gets 0.  One thread per source pixel: a gather.
__global__ __launch_bounds__(256) void ingest_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dout2,
                                                         const int* __restrict__ start, const int* __restrict__ jlist, int F, int Tout,
                                                         int Tsplit, int B, int H, int W, float k, int normalize, float* __restrict__ dsrc,
                                                         int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * F * H * W) return;
  const int64_t hw = (int64_t)H * W;
  const int64_t p = i % hw;
  const int w = (int)(p % W), h = (int)(p / W), f = (int)((i / hw) % F);
  const int b = (int)(i / (hw * F));
  float a[3] = {0.f, 0.f, 0.f};
  for (int m = start[f]; m < start[f + 1]; ++m) {
    const int j = jlist[m];
    const float* s = j < Tsplit ? dout + (((int64_t)b * Tsplit + j) * hw + p) * 4
                                : dout2 + (((int64_t)b * (Tout - Tsplit) + (j - Tsplit)) * hw + p) * 4;
    const float4 v = *reinterpret_cast<const float4*>(s);
    a[0] += v.x; a[1] += v.y; a[2] += v.z;
  }
  float* o = dsrc + b * sb + f * sf + h * sh + w * sw;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * sc] = normalize ? a[c] * k : a[c];
}

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int mt_sf_bn_relu_fwd(const float* z, int64_t ldz, const float* scale, const float* shift, const float* res, int64_t ldr,
                                 const float* rscale, const float* rshift, float* y, int64_t ldy, int64_t rows, int C, void* stream) {
  if (!z || !scale || !shift || !y || rows <= 0 || C <= 0) return fail(MT_ERR_ARG, "mt_sf_bn_relu_fwd: null pointer or empty shape");
  if ((C & 3) || (ldz & 3) || (ldy & 3) || (res && (ldr & 3)) || (((uintptr_t)z | (uintptr_t)y | (uintptr_t)(res ? res : z)) & 15))
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_bn_relu_fwd: C, pitches and pointers must allow float4 accesses");
  if ((rscale == nullptr) != (rshift == nullptr) || (rscale && !res)) return fail(MT_ERR_ARG, "mt_sf_bn_relu_fwd: rscale/rshift need res");
  hipLaunchKernelGGL(bn_relu_fwd_kernel, dim3(blocks(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, z, ldz, scale, shift, res, ldr,
                     rscale, rshift, y, ldy, rows, C);
  return check_launch("mt_sf_bn_relu_fwd");
}

extern "C" int64_t mt_sf_bn_bwd_part_floats(int64_t rows, int C) {
  const int64_t nb = (rows + kStatRowsPerBlock - 1) / kStatRowsPerBlock;
  return ((nb * 2 * C + 3) & ~(int64_t)3) + colsum_mid_floats(nb, 2 * C);
}

extern "C" int mt_sf_bn_relu_bwd_stats(const float* g, int64_t ldg, const float* z, int64_t ldz, const float* scale, const float* shift,
                                       const float* m, int64_t ldm, const float* mean_invstd, float* part, double* stats, int64_t rows, int C,
                                       void* stream) {
  if (!g || !z || !mean_invstd || !part || !stats || rows <= 0 || C <= 0) return fail(MT_ERR_ARG, "mt_sf_bn_relu_bwd_stats: null pointer");
  if ((scale == nullptr) != (shift == nullptr)) return fail(MT_ERR_ARG, "mt_sf_bn_relu_bwd_stats: scale and shift go together");
  const int64_t nb = (rows + kStatRowsPerBlock - 1) / kStatRowsPerBlock;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_relu_bwd_stats_kernel, dim3((unsigned)nb, (C + kStatCols - 1) / kStatCols), dim3(256), 0, st, g, ldg, z, ldz, scale,
                     shift, m, ldm, mean_invstd, part, rows, C);
  colsum_stats(part, nb, 2 * C, reinterpret_cast<double*>(part + ((nb * 2 * C + 3) & ~(int64_t)3)), stats, st);
  return check_launch("mt_sf_bn_relu_bwd_stats");
}

extern "C" int mt_sf_bn_relu_bwd_apply(const float* g, int64_t ldg, const float* z, int64_t ldz, const float* scale, const float* shift,
                                       const float* m, int64_t ldm, const float* kabc, float* out, int64_t ldo, int accumulate, int64_t rows,
                                       int C, void* stream) {
  if (!g || !out || (kabc && !z) || (scale && (!z || !shift)) || rows <= 0 || C <= 0)
    return fail(MT_ERR_ARG, "mt_sf_bn_relu_bwd_apply: null pointer");
  hipLaunchKernelGGL(bn_relu_bwd_apply_kernel, dim3(blocks(rows * C)), dim3(256), 0, (hipStream_t)stream, g, ldg, z, ldz, scale, shift, m,
                     ldm, kabc, out, ldo, accumulate, rows, C);
  return check_launch("mt_sf_bn_relu_bwd_apply");
}

extern "C" int mt_sf_maxpool_fwd(const float* z, const float* scale, const float* shift, float* out, int64_t ldo, int* arg, int64_t NT, int H,
                                 int W, int C, void* stream) {
  if (!z || !scale || !shift || !out || !arg || NT <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(MT_ERR_ARG, "mt_sf_maxpool_fwd: bad args");
  if ((int64_t)H * W > INT32_MAX) return fail(MT_ERR_UNSUPPORTED, "mt_sf_maxpool_fwd: plane too large");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks(NT * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, z, scale, shift, out, ldo, arg,
                     NT, H, W, Ho, Wo, C);
  return check_launch("mt_sf_maxpool_fwd");
}

extern "C" int mt_sf_maxpool_bwd(const float* dout, int64_t ldd, const int* arg, float* din, int64_t NT, int H, int W, int C, void* stream) {
  if (!dout || !arg || !din || NT <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(MT_ERR_ARG, "mt_sf_maxpool_bwd: bad args");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks(NT * H * W * C)), dim3(256), 0, (hipStream_t)stream, dout, ldd, arg, din, NT, H, W, Ho,
                     Wo, C);
  return check_launch("mt_sf_maxpool_bwd");
}

extern "C" int mt_sf_head_pool(const float* feat, int64_t ldf, const float* mult, float* d, int B, int T, int H, int W, int C, int kt,
                               int kh, int kw, int coff, int CT, void* stream) {
  if (!feat || !d || kt > T || kh > H || kw > W || kt <= 0 || kh <= 0 || kw <= 0 || coff + C > CT)
    return fail(MT_ERR_ARG, "mt_sf_head_pool: bad args");
  const int Pt = T - kt + 1, Ph = H - kh + 1, Pw = W - kw + 1;
  hipLaunchKernelGGL(head_pool_kernel, dim3(blocks((int64_t)B * Pt * Ph * Pw * C)), dim3(256), 0, (hipStream_t)stream, feat, ldf, mult, d, B,
                     T, H, W, C, kt, kh, kw, Pt, Ph, Pw, coff, CT);
  return check_launch("mt_sf_head_pool");
}

extern "C" int mt_sf_head_proj(const float* d, const float* w, const float* bias, float* logits, int B, int P, int CT, int J, void* stream) {
  if (!d || !w || !logits || B <= 0 || P <= 0 || CT <= 0 || J <= 0) return fail(MT_ERR_ARG, "mt_sf_head_proj: bad args");
  hipLaunchKernelGGL(head_proj_kernel, dim3(blocks((int64_t)B * J * 64)), dim3(256), 0, (hipStream_t)stream, d, w, bias, logits, B, P, CT, J);
  return check_launch("mt_sf_head_proj");
}

extern "C" int mt_sf_head_bwd(const float* g, const float* d, const float* w, const float* mult, float* dw, float* db, float* dpool, int B,
                              int P, int CT, int J, void* stream) {
  if (!g || B <= 0 || P <= 0 || CT <= 0 || J <= 0 || ((dw || dpool) && (!d || !w))) return fail(MT_ERR_ARG, "mt_sf_head_bwd: bad args");
  const hipStream_t st = (hipStream_t)stream;
  if (dw || db) hipLaunchKernelGGL(head_params_kernel, dim3(blocks((int64_t)J * (CT + 1))), dim3(256), 0, st, g, d, dw, db, B, P, CT, J);
  if (dpool) hipLaunchKernelGGL(head_dpool_kernel, dim3(blocks((int64_t)B * CT)), dim3(256), 0, st, g, w, mult, dpool, B, P, CT, J);
  return check_launch("mt_sf_head_bwd");
}

extern "C" int mt_sf_head_dfeat(const float* dpool, float* dfeat, int64_t ldf, int B, int T, int H, int W, int C, int kt, int kh, int kw,
                                int coff, int CT, void* stream) {
  if (!dpool || !dfeat || kt > T || kh > H || kw > W || kt <= 0 || kh <= 0 || kw <= 0 || coff + C > CT)
    return fail(MT_ERR_ARG, "mt_sf_head_dfeat: bad args");
  hipLaunchKernelGGL(head_dfeat_kernel, dim3(blocks((int64_t)B * T * H * W * C)), dim3(256), 0, (hipStream_t)stream, dpool, dfeat, ldf, B, T,
                     H, W, C, kt, kh, kw, T - kt + 1, H - kh + 1, W - kw + 1, coff, CT);
  return check_launch("mt_sf_head_dfeat");
}

extern "C" int mt_sf_ingest(const void* src, int is_u8, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc, const int* fidx, int Tout,
                            int Tsplit, int B, int H, int W, int normalize, float* out, float* out2, void* stream) {
  if (!src || !fidx || !out || Tout <= 0 || B <= 0 || H <= 0 || W <= 0 || Tsplit <= 0 || Tsplit > Tout || (Tsplit < Tout && !out2))
    return fail(MT_ERR_ARG, "mt_sf_ingest: bad args");
  if (((uintptr_t)out | (uintptr_t)(out2 ? out2 : out)) & 15) return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest: outputs must be 16-byte aligned");
  const dim3 grid(blocks((int64_t)B * Tout * H * W));
  const hipStream_t st = (hipStream_t)stream;
  if (is_u8)
    hipLaunchKernelGGL(ingest_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)src, sb, sf, sh, sw, sc, fidx, Tout, Tsplit, B, H, W,
                       normalize, out, out2);
  else
    hipLaunchKernelGGL(ingest_kernel<float>, grid, dim3(256), 0, st, (const float*)src, sb, sf, sh, sw, sc, fidx, Tout, Tsplit, B, H, W,
                       normalize, out, out2);
  return check_launch("mt_sf_ingest");
}

extern "C" int mt_sf_ingest_bwd(const float* dout, const float* dout2, const int* start, const int* jlist, int F, int Tout, int Tsplit, int B,
                                int H, int W, int normalize, float* dsrc, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc,
                                void* stream) {
  if (!dout || !start || !jlist || !dsrc || F <= 0 || Tout <= 0 || B <= 0 || H <= 0 || W <= 0 || Tsplit <= 0 || Tsplit > Tout ||
      (Tsplit < Tout && !dout2))
    return fail(MT_ERR_ARG, "mt_sf_ingest_bwd: bad args");
  if (((uintptr_t)dout | (uintptr_t)(dout2 ? dout2 : dout)) & 15)
    return fail(MT_ERR_UNSUPPORTED, "mt_sf_ingest_bwd: dout and dout2 must be 16-byte aligned");
  const float k = (float)(1.0 / (255.0 * 0.225));
  hipLaunchKernelGGL(ingest_bwd_kernel, dim3(blocks((int64_t)B * F * H * W)), dim3(256), 0, (hipStream_t)stream, dout, dout2, start, jlist, F,
                     Tout, Tsplit, B, H, W, k, normalize, dsrc, sb, sf, sh, sw, sc);
  return check_launch("mt_sf_ingest_bwd");
}
