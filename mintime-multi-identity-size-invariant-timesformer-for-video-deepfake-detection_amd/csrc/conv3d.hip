// Implicit-GEMM 3-D convolution on v_mfma_f32_32x32x2_f32 (SlowFast R50: every Conv3d of pytorchvideo's slowfast_r50).
// Activations are channels-last rows ([N][T][H][W] rows of C floats, any row pitch), weights are K-contiguous:
//   forward  y[m][co]  = sum_{tap, ci} pro(x[in(m, tap)][ci]) * wp[co][tap][ci]              (wp = w.permute(0, 2, 3, 4, 1))
//   dgrad    dx[r][ci] = sum_{tap, co} dy[out(r, tap)][co] * wt[tap][co][ci]                  (wt = w.permute(2, 3, 4, 0, 1))
//   wgrad    dw[co][tap][ci] = sum_m dy[m][co] * pro(x[in(m, tap)][ci])
// where in(m, tap) is the input row the tap reads for output row m (zero outside the volume) and out(r, tap) the output row that
// read input row r through that tap (a gather: no row when the stride does not divide, so strided data gradients need no atomics).
// pro(v) = max(v * scale[ci] + shift[ci], 0) when scale is given (BatchNorm + ReLU of the producer folded into the loads; padding
// stays zero, as in the module where the padding is applied after the activation), else v.
// Every sum runs in a fixed order and no kernel issues an atomic: the results are the same bits run after run.
#include "../../include/mintime_hip.h"
#include "common.hpp"

using namespace mt;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 16;   // block tile (4 wavefronts, 32 x 32 each) and K step (8 MFMAs of K = 2)
constexpr int LP = 4;                      // LDS row padding

struct Geo {
  int N, T, H, W, C, To, Ho, Wo, K, kt, kh, kw, st, sh, sw, pt, ph, pw;
  int64_t ldx, ldy;
};

__device__ __forceinline__ float4 pro4(float4 v, const float* scale, const float* shift, int ci) {
  const float4 s = *reinterpret_cast<const float4*>(scale + ci), b = *reinterpret_cast<const float4*>(shift + ci);
  return make_float4(fmaxf(fmaf(v.x, s.x, b.x), 0.f), fmaxf(fmaf(v.y, s.y, b.y), 0.f), fmaxf(fmaf(v.z, s.z, b.z), 0.f),
                     fmaxf(fmaf(v.w, s.w, b.w), 0.f));
}

// output row m -> (n, t, h, w) of the output grid
struct Pos { int n, t, h, w; };
__device__ __forceinline__ Pos decode(int64_t m, int T, int H, int W) {
  Pos p;
  p.w = (int)(m % W); m /= W;
  p.h = (int)(m % H); m /= H;
  p.t = (int)(m % T);
  p.n = (int)(m / T);
  return p;
}

// four consecutive input channels ci.. of the row that tap `tap` of output position o reads (zero outside the volume)
template <bool PRO>
__device__ __forceinline__ float4 gather_x(const Geo& g, const float* __restrict__ x, const float* scale, const float* shift, Pos o,
                                           int tap, int ci) {
  const int khw = g.kh * g.kw, a = tap / khw, rem = tap - a * khw, b = rem / g.kw, c = rem - b * g.kw;
  const int ti = o.t * g.st - g.pt + a, hi = o.h * g.sh - g.ph + b, wi = o.w * g.sw - g.pw + c;
  if (ti < 0 || ti >= g.T || hi < 0 || hi >= g.H || wi < 0 || wi >= g.W) return make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t row = (((int64_t)o.n * g.T + ti) * g.H + hi) * g.W + wi;
  float4 v = *reinterpret_cast<const float4*>(x + row * g.ldx + ci);
  if (PRO) v = pro4(v, scale, shift, ci);
  return v;
}

// one K step of the block: the 4 wavefronts each multiply their 32 x 32 slice of As x Bs
__device__ __forceinline__ void mma_step(const float (*As)[BM + LP], const float (*Bs)[BN + LP], int lane, int wm, int wn, f32x16& acc) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < BK / 2; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * kk + h][wm * 32 + r], Bs[2 * kk + h][wn * 32 + r], acc, 0, 0, 0);
}

// ---- forward: M = N*To*Ho*Wo output rows, N = K output channels, reduction over taps * C --------------------------------------
template <bool PRO>
__global__ __launch_bounds__(256) void fwd_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ scale,
                                                  const float* __restrict__ shift, const float* __restrict__ wp, float* __restrict__ y,
                                                  int accumulate, float* __restrict__ part) {
  __shared__ float As[BK][BM + LP], Bs[BK][BN + LP];
  __shared__ float red[2][2][BN];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
  const int64_t M = (int64_t)g.N * g.To * g.Ho * g.Wo;
  const int KD = g.kt * g.kh * g.kw * g.C;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int ar = t >> 2, ag = t & 3;           // A: row, group of 4 k
  const bool arow = m0 + ar < M;
  const Pos ao = decode(arow ? m0 + ar : 0, g.To, g.Ho, g.Wo);
  const bool bcol = n0 + ar < g.K;             // B: column (output channel) ar, group ag
  const float* wrow = wp + (int64_t)(bcol ? n0 + ar : 0) * KD;
  f32x16 acc = {};
  for (int k0 = 0; k0 < KD; k0 += BK) {
    const int k = k0 + ag * 4;
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    if (k < KD) {
      if (arow) {
        const int tap = k / g.C;
        av = gather_x<PRO>(g, x, scale, shift, ao, tap, k - tap * g.C);
      }
      if (bcol) bv = *reinterpret_cast<const float4*>(wrow + k);
    }
    __syncthreads();
    As[ag * 4 + 0][ar] = av.x; As[ag * 4 + 1][ar] = av.y; As[ag * 4 + 2][ar] = av.z; As[ag * 4 + 3][ar] = av.w;
    Bs[ag * 4 + 0][ar] = bv.x; Bs[ag * 4 + 1][ar] = bv.y; Bs[ag * 4 + 2][ar] = bv.z; Bs[ag * 4 + 3][ar] = bv.w;
    __syncthreads();
    mma_step(As, Bs, lane, wm, wn, acc);
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col < g.K) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t row = m0 + wm * 32 + mfma_slot_row(i, lane >> 5);
      if (row < M) {
        float* p = y + row * g.ldy + col;
        *p = accumulate ? *p + acc[i] : acc[i];
      }
    }
  }
  if (part) {                                  // BatchNorm sums of this block's 64 rows (rows past M hold exact zeros)
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s += acc[i]; q = fmaf(acc[i], acc[i], q); }
    s += __shfl_xor(s, 32, 64);
    q += __shfl_xor(q, 32, 64);
    if (lane < 32) { red[wm][0][wn * 32 + lane] = s; red[wm][1][wn * 32 + lane] = q; }
    __syncthreads();
    if (t < 2 * BN) {
      const int w = t >> 6, c = t & 63;
      if (n0 + c < g.K) part[((int64_t)blockIdx.x * 2 + w) * g.K + n0 + c] = red[0][w][c] + red[1][w][c];
    }
  }
}

// ---- data gradient: M = N*T*H*W input rows, N = C input channels, reduction over taps * K ---------------------------------------
__global__ __launch_bounds__(256) void dgrad_kernel(Geo g, const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx,
                                                    int accumulate) {
  __shared__ float As[BK][BM + LP], Bs[BK][BN + LP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
  const int64_t M = (int64_t)g.N * g.T * g.H * g.W;
  const int KD = g.kt * g.kh * g.kw * g.K;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int ar = t >> 2, ag = t & 3;           // A: input row, group of 4 (tap, co)
  const bool arow = m0 + ar < M;
  const Pos ai = decode(arow ? m0 + ar : 0, g.T, g.H, g.W);
  const int bk = t >> 4, bn = (t & 15) * 4;    // B: k row, 4 input channels
  const int khw = g.kh * g.kw;
  f32x16 acc = {};
  for (int k0 = 0; k0 < KD; k0 += BK) {
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    const int k = k0 + ag * 4;
    if (arow && k < KD) {
      const int tap = k / g.K, co = k - tap * g.K;
      const int a = tap / khw, rem = tap - a * khw, b = rem / g.kw, c = rem - b * g.kw;
      const int tt = ai.t + g.pt - a, hh = ai.h + g.ph - b, ww = ai.w + g.pw - c;
      if (tt >= 0 && hh >= 0 && ww >= 0 && tt % g.st == 0 && hh % g.sh == 0 && ww % g.sw == 0) {
        const int to = tt / g.st, ho = hh / g.sh, wo = ww / g.sw;
        if (to < g.To && ho < g.Ho && wo < g.Wo) {
          const int64_t row = (((int64_t)ai.n * g.To + to) * g.Ho + ho) * g.Wo + wo;
          av = *reinterpret_cast<const float4*>(dy + row * g.ldy + co);
        }
      }
    }
    if (k0 + bk < KD && n0 + bn < g.C) bv = *reinterpret_cast<const float4*>(wt + (int64_t)(k0 + bk) * g.C + n0 + bn);
    __syncthreads();
    As[ag * 4 + 0][ar] = av.x; As[ag * 4 + 1][ar] = av.y; As[ag * 4 + 2][ar] = av.z; As[ag * 4 + 3][ar] = av.w;
    *reinterpret_cast<float4*>(&Bs[bk][bn]) = bv;
    __syncthreads();
    mma_step(As, Bs, lane, wm, wn, acc);
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col < g.C) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t row = m0 + wm * 32 + mfma_slot_row(i, lane >> 5);
      if (row < M) {
        float* p = dx + row * g.ldx + col;
        *p = accumulate ? *p + acc[i] : acc[i];
      }
    }
  }
}

// ---- weight gradient: M = K output channels, N = taps * C, reduction over the output rows of split blockIdx.z --------------------
template <bool PRO>
__global__ __launch_bounds__(256) void wgrad_kernel(Geo g, const float* __restrict__ x, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, const float* __restrict__ dy, float* __restrict__ out,
                                                    int64_t rows_per_split) {
  __shared__ float As[BK][BM + LP], Bs[BK][BN + LP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv & 1, wn = wv >> 1;
  const int64_t R = (int64_t)g.N * g.To * g.Ho * g.Wo;
  const int KD = g.kt * g.kh * g.kw * g.C;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int64_t r0 = (int64_t)blockIdx.z * rows_per_split, r1 = min(R, r0 + rows_per_split);
  const int lr = t >> 4, lc = (t & 15) * 4;    // both operands: reduction row lr, 4 consecutive columns
  const bool acol = m0 + lc < g.K;
  const int kk = n0 + lc;
  const bool bcol = kk < KD;
  const int tap = bcol ? kk / g.C : 0, ci = kk - tap * g.C;
  f32x16 acc = {};
  for (int64_t rb = r0; rb < r1; rb += BK) {
    const int64_t r = rb + lr;
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
    if (r < r1) {
      if (acol) av = *reinterpret_cast<const float4*>(dy + r * g.ldy + m0 + lc);
      if (bcol) bv = gather_x<PRO>(g, x, scale, shift, decode(r, g.To, g.Ho, g.Wo), tap, ci);
    }
    __syncthreads();
    *reinterpret_cast<float4*>(&As[lr][lc]) = av;
    *reinterpret_cast<float4*>(&Bs[lr][lc]) = bv;
    __syncthreads();
    mma_step(As, Bs, lane, wm, wn, acc);
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col < KD) {
    float* o = out + (int64_t)blockIdx.z * g.K * KD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = m0 + wm * 32 + mfma_slot_row(i, lane >> 5);
      if (row < g.K) o[(int64_t)row * KD + col] = acc[i];
    }
  }
}

// dw[i] = sum over the splits of ws[s][i], in split order
__global__ __launch_bounds__(256) void split_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = ws[i];
  for (int s = 1; s < splits; ++s) a += ws[(int64_t)s * n + i];
  dw[i] = a;
}

Geo geo(const mt_conv3d_desc* d) {
  return Geo{d->N, d->T, d->H, d->W, d->C, d->To, d->Ho, d->Wo, d->K, d->kt, d->kh, d->kw, d->st, d->sh, d->sw, d->pt, d->ph, d->pw,
             d->ldx, d->ldy};
}

int check_desc(const char* what, const mt_conv3d_desc* d) {
  if (!d) return fail(MT_ERR_ARG, "%s: null descriptor", what);
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->K <= 0 || d->kt <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->st <= 0 || d->sh <= 0 || d->sw <= 0 || d->pt < 0 || d->ph < 0 || d->pw < 0)
    return fail(MT_ERR_ARG, "%s: empty or negative shape", what);
  if (d->To != (d->T + 2 * d->pt - d->kt) / d->st + 1 || d->Ho != (d->H + 2 * d->ph - d->kh) / d->sh + 1 ||
      d->Wo != (d->W + 2 * d->pw - d->kw) / d->sw + 1 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0)
    return fail(MT_ERR_ARG, "%s: output grid %dx%dx%d does not match the input, kernel, stride and padding", what, d->To, d->Ho, d->Wo);
  if ((d->C & 3) || (d->K & 3) || (d->ldx & 3) || (d->ldy & 3) || d->ldx < d->C || d->ldy < d->K)
    return fail(MT_ERR_UNSUPPORTED, "%s: C, K and the row pitches must be multiples of 4 (float4 accesses), pitches >= widths", what);
  if ((int64_t)d->kt * d->kh * d->kw * (d->C > d->K ? d->C : d->K) > (1 << 24))
    return fail(MT_ERR_UNSUPPORTED, "%s: reduction length too large", what);
  if ((int64_t)d->N * d->T * d->H * d->W > ((int64_t)1 << 37) || (int64_t)d->N * d->To * d->Ho * d->Wo > ((int64_t)1 << 37))
    return fail(MT_ERR_UNSUPPORTED, "%s: too many rows", what);
  return 0;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr int kReduceGroups = 8;      // column sums of the statistics partials: 32 columns x 8 row groups per block
constexpr int kReduceChunk = 512;     // partial rows per first-level chunk

// out[c][j] = sum over rows i in chunk c of in[i][j] (fp64, fixed order): block = 32 columns x 8 groups, group g takes rows g, g + 8, ..
template <typename TI>
__global__ __launch_bounds__(256) void colsum_kernel(const TI* __restrict__ in, int64_t rows, int cols, int chunk, double* __restrict__ out) {
  __shared__ double red[kReduceGroups][32];
  const int cl = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + cl;
  const int64_t i0 = (int64_t)blockIdx.y * chunk, i1 = min(rows, i0 + chunk);
  double a = 0.0;
  if (j < cols)
    for (int64_t i = i0 + grp; i < i1; i += kReduceGroups) a += (double)in[i * cols + j];
  red[grp][cl] = a;
  __syncthreads();
  if (grp == 0 && j < cols) {
    double r = red[0][cl];
    for (int q = 1; q < kReduceGroups; ++q) r += red[q][cl];
    out[(int64_t)blockIdx.y * cols + j] = r;
  }
}

}  // namespace

namespace mt {
// stats [2][cols/2] (fp64, written) = the column sums of part [rows][cols] (fp32), in a fixed order; `mid` holds
// ceil(rows / kReduceChunk) * cols doubles when rows > kReduceChunk.
int colsum_stats(const float* part, int64_t rows, int cols, double* mid, double* stats, hipStream_t st) {
  const dim3 gx((cols + 31) / 32);
  if (rows <= kReduceChunk) {
    hipLaunchKernelGGL(colsum_kernel<float>, dim3(gx.x, 1), dim3(256), 0, st, part, rows, cols, (int)rows, stats);
  } else {
    const int64_t nc = (rows + kReduceChunk - 1) / kReduceChunk;
    hipLaunchKernelGGL(colsum_kernel<float>, dim3(gx.x, (unsigned)nc), dim3(256), 0, st, part, rows, cols, kReduceChunk, mid);
    hipLaunchKernelGGL(colsum_kernel<double>, dim3(gx.x, 1), dim3(256), 0, st, (const double*)mid, nc, cols, (int)nc, stats);
  }
  return 0;
}
int64_t colsum_mid_floats(int64_t rows, int cols) {
  return rows <= kReduceChunk ? 0 : 2 * ((rows + kReduceChunk - 1) / kReduceChunk) * cols;
}
}  // namespace mt

extern "C" int64_t mt_conv3d_part_floats(const mt_conv3d_desc* d) {
  if (!d) return 0;
  const int64_t M = (int64_t)d->N * d->To * d->Ho * d->Wo, nb = (M + BM - 1) / BM;
  const int64_t part = nb * 2 * d->K;
  return ((part + 3) & ~(int64_t)3) + colsum_mid_floats(nb, 2 * d->K);
}

extern "C" int mt_conv3d_fwd(const mt_conv3d_desc* d, const float* x, const float* scale, const float* shift, const float* w, float* y,
                             int accumulate, float* part, double* stats, void* stream) {
  if (int rc = check_desc("mt_conv3d_fwd", d)) return rc;
  if (!x || !w || !y) return fail(MT_ERR_ARG, "mt_conv3d_fwd: null pointer");
  if ((scale == nullptr) != (shift == nullptr)) return fail(MT_ERR_ARG, "mt_conv3d_fwd: scale and shift go together");
  if ((part == nullptr) != (stats == nullptr)) return fail(MT_ERR_ARG, "mt_conv3d_fwd: part and stats go together");
  if (stats && accumulate) return fail(MT_ERR_ARG, "mt_conv3d_fwd: statistics of an accumulated output are not supported");
  if (!al16(x) || !al16(w) || (scale && (!al16(scale) || !al16(shift))))
    return fail(MT_ERR_UNSUPPORTED, "mt_conv3d_fwd: x, w, scale and shift must be 16-byte aligned");
  const Geo g = geo(d);
  const int64_t M = (int64_t)g.N * g.To * g.Ho * g.Wo, nb = (M + BM - 1) / BM;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nb, (g.K + BN - 1) / BN);
  if (scale)
    hipLaunchKernelGGL(fwd_kernel<true>, grid, dim3(256), 0, st, g, x, scale, shift, w, y, accumulate, part);
  else
    hipLaunchKernelGGL(fwd_kernel<false>, grid, dim3(256), 0, st, g, x, scale, shift, w, y, accumulate, part);
  if (stats) {
    const int64_t pf = (nb * 2 * g.K + 3) & ~(int64_t)3;
    colsum_stats(part, nb, 2 * g.K, reinterpret_cast<double*>(part + pf), stats, st);
  }
  return check_launch("mt_conv3d_fwd");
}

extern "C" int mt_conv3d_dgrad(const mt_conv3d_desc* d, const float* dy, const float* wt, float* dx, int accumulate, void* stream) {
  if (int rc = check_desc("mt_conv3d_dgrad", d)) return rc;
  if (!dy || !wt || !dx) return fail(MT_ERR_ARG, "mt_conv3d_dgrad: null pointer");
  if (!al16(dy) || !al16(wt)) return fail(MT_ERR_UNSUPPORTED, "mt_conv3d_dgrad: dy and wt must be 16-byte aligned");
  const Geo g = geo(d);
  const int64_t M = (int64_t)g.N * g.T * g.H * g.W;
  hipLaunchKernelGGL(dgrad_kernel, dim3((unsigned)((M + BM - 1) / BM), (g.C + BN - 1) / BN), dim3(256), 0, (hipStream_t)stream, g, dy,
                     wt, dx, accumulate);
  return check_launch("mt_conv3d_dgrad");
}

extern "C" int mt_conv3d_wgrad_splits(const mt_conv3d_desc* d) {
  if (!d) return 1;
  const int64_t R = (int64_t)d->N * d->To * d->Ho * d->Wo;
  const int64_t KD = (int64_t)d->kt * d->kh * d->kw * d->C;
  const int64_t tiles = ((d->K + BM - 1) / BM) * ((KD + BN - 1) / BN);
  int64_t s = (2048 + tiles - 1) / tiles;                 // about 2048 blocks
  const int64_t by_rows = (R + 8 * BK - 1) / (8 * BK);     // at least 8 K steps per block
  const int64_t by_ws = ((int64_t)64 << 20) / ((int64_t)d->K * KD);   // workspace at most 256 MB
  if (s > by_rows) s = by_rows;
  if (s > by_ws) s = by_ws;
  if (s > 4096) s = 4096;
  return s < 1 ? 1 : (int)s;
}

extern "C" int mt_conv3d_wgrad(const mt_conv3d_desc* d, const float* x, const float* scale, const float* shift, const float* dy, float* dw,
                               float* ws, int splits, void* stream) {
  if (int rc = check_desc("mt_conv3d_wgrad", d)) return rc;
  if (!x || !dy || !dw || splits < 1 || (splits > 1 && !ws)) return fail(MT_ERR_ARG, "mt_conv3d_wgrad: null pointer or bad split count");
  if ((scale == nullptr) != (shift == nullptr)) return fail(MT_ERR_ARG, "mt_conv3d_wgrad: scale and shift go together");
  if (!al16(x) || !al16(dy) || (scale && (!al16(scale) || !al16(shift))))
    return fail(MT_ERR_UNSUPPORTED, "mt_conv3d_wgrad: x, dy, scale and shift must be 16-byte aligned");
  const Geo g = geo(d);
  const int64_t R = (int64_t)g.N * g.To * g.Ho * g.Wo;
  const int KD = g.kt * g.kh * g.kw * g.C;
  const int64_t per = ((R + splits - 1) / splits + BK - 1) / BK * BK;
  const int nsplit = (int)((R + per - 1) / per);
  float* out = nsplit > 1 ? ws : dw;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((g.K + BM - 1) / BM, (KD + BN - 1) / BN, nsplit);
  if (scale)
    hipLaunchKernelGGL(wgrad_kernel<true>, grid, dim3(256), 0, st, g, x, scale, shift, dy, out, per);
  else
    hipLaunchKernelGGL(wgrad_kernel<false>, grid, dim3(256), 0, st, g, x, scale, shift, dy, out, per);
  if (nsplit > 1) {
    const int64_t n = (int64_t)g.K * KD;
    hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, dw, n, nsplit);
  }
  return check_launch("mt_conv3d_wgrad");
}
