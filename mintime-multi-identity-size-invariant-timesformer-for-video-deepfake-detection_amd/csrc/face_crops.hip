// Face crops for the embedder, kept on the device: what the reference does on the host between the detector and InceptionResnetV1,
// one face at a time -- the crop rule (predict.py:103-140, preprocessing/extract_crops.py:75-113) and preprocess_images
// (preprocessing/utils.py:32-34): torchvision Resize([128, 128]) of a PIL image, i.e. Pillow's antialiased 8-bit bilinear resize.
//   mt_face_rects      detector boxes -> source windows.  The rule, per face, in integers: double and truncate the four coordinates;
//                      pad each side by a third of the box (floor); take the padding of the longer padded span down by half the
//                      difference so the window is square; clamp the near ends at 0 and cut the far ends at the frame; if the cut left
//                      the window off square, trim the longer side by half the difference at both ends, or by one row (the first) /
//                      one column (the last) when the sides are one apart.  Empty windows, negative far ends (where the reference's
//                      slice would wrap around), sides above 4096 and frame indices outside the batch are marked invalid and counted.
//   mt_crop_resize_u8  windows of any size -> [T][OH][OW][3] uint8, byte for byte what Image.resize((OW, OH), BILINEAR) returns:
//                      per axis a triangle filter of support max(in / out, 1) around (i + 0.5) in / out, weights normalised in
//                      double, rounded to 22 fractional bits; a horizontal pass into uint8, then a vertical pass over that.
// Pillow's C is compiled without contraction, hipcc fuses a * b + c by default: one fused `center - support` moves a window bound
// or a coefficient, and a byte with it.  Contraction is off for this whole file.
// One block = (band of output rows, face).  The grid cannot depend on the windows (they exist only on the device), so a block sizes
// its own work: it walks its band in sub-bands whose horizontal-pass rows fit a fixed LDS tile, and a single output row whose
// taps do not fit (a long side squeezed into very few rows) is accumulated over several fills of the tile.  The intermediate never
// goes to memory.  include/mintime_hip.h states both rules in full.
#include "common.hpp"
#include <stdint.h>

#pragma clang fp contract(off)

namespace {
using namespace mt;

constexpr int FC_THREADS = 256;
constexpr int FC_BANDS = 8;                              // grid.x: bands of ceil(OH / 8) output rows
constexpr int FC_MAX_OUT = 256, FC_MAX_SIDE = 4096;
constexpr int FC_BAND_ROWS = FC_MAX_OUT / FC_BANDS;
constexpr int FC_KY = 2048;                              // vertical coefficients held at a time (ints)
constexpr int FC_TILE_BYTES = 24 * 1024;                 // horizontal-pass tile; smaller when the x table is large
constexpr int FC_DYN_LDS_MAX = 50 * 1024;                // x table + tile; the static arrays below take 12.5 KB more
constexpr int FC_HALF = 1 << 21;
constexpr int64_t FC_COORD_MAX = 1 << 29;
enum { FC_OK = 0, FC_SKIP = 1, FC_BAD = 2 };

struct Axis {
  double scale, fs;
  int in, ksize;
};
__host__ __device__ inline Axis axis_of(int in, int out) {
  Axis a;
  a.in = in;
  a.scale = (double)in / (double)out;
  a.fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.ksize = 2 * (int)ceil(a.fs) + 1;
  return a;
}
__device__ __forceinline__ double axis_center(const Axis& a, int i) { return ((double)i + 0.5) * a.scale; }
__device__ __forceinline__ void axis_bounds(const Axis& a, int i, int& first, int& n) {
  const double c = axis_center(a, i);
  int lo = (int)(c - a.fs + 0.5), hi = (int)(c + a.fs + 0.5);
  lo = lo < 0 ? 0 : lo;
  hi = hi > a.in ? a.in : hi;
  first = lo;
  n = hi - lo;
}
// (Pillow's C multiplies by 1.0 / filterscale where this divides by fs; the integer coefficients of the two forms were compared for
// every input side 1..4096 at outputs 1, 2, 3, 96, 128, 160, 256 and none differs: profiles/face_crops.txt)
__device__ __forceinline__ double axis_weight(const Axis& a, double center, int pos) {      // pos = source index
  double x = ((double)pos - center + 0.5) / a.fs;
  x = x < 0.0 ? -x : x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
__device__ double axis_weight_sum(const Axis& a, int i, int first, int n) {                 // in index order
  const double c = axis_center(a, i);
  double s = 0.0;
  for (int j = 0; j < n; ++j) s += axis_weight(a, c, first + j);
  return s;
}
__device__ __forceinline__ int axis_coeff(const Axis& a, int i, int pos, double sum) {
  double w = axis_weight(a, axis_center(a, i), pos);
  if (sum != 0.0) w = w / sum;
  return (int)(w * 4194304.0 + 0.5);
}
__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> 22;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ int64_t floor_div3(int64_t a) { return a / 3 - ((a % 3 != 0 && a < 0) ? 1 : 0); }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(FC_THREADS) void face_rects_kernel(const float* __restrict__ boxes, const int* __restrict__ frame_index, int T,
                                                                int N, int H, int W, int* __restrict__ rects,
                                                                unsigned char* __restrict__ valid, int* __restrict__ err) {
  const int t = blockIdx.x * FC_THREADS + threadIdx.x;
  if (t >= T) return;
  int64_t c[4];
  bool ok = frame_index[t] >= 0 && frame_index[t] < N;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float v = boxes[4 * t + q] * 2.0f;
    const bool fin = fabsf(v) <= (float)FC_COORD_MAX;            // false for NaN and infinities
    ok = ok && fin;
    c[q] = fin ? (int64_t)v : 0;                                 // conversion truncates toward zero
  }
  const int64_t xlo = c[0], ylo = c[1], xhi = c[2], yhi = c[3];
  int64_t ph = floor_div3(yhi - ylo), pw = floor_div3(xhi - xlo);
  const int64_t sh = (yhi + ph) - max64(ylo - ph, 0), sw = (xhi + pw) - max64(xlo - pw, 0);
  if (sh > sw) ph -= (sh - sw) / 2; else pw -= (sw - sh) / 2;    // non-negative differences: / truncates as int() does
  int64_t y0 = max64(ylo - ph, 0), y1 = yhi + ph, x0 = max64(xlo - pw, 0), x1 = xhi + pw;
  ok = ok && y1 >= 0 && x1 >= 0;
  y1 = min64(y1, H);
  x1 = min64(x1, W);
  int64_t h = y1 - y0, w = x1 - x0;
  ok = ok && h > 0 && w > 0;
  if (h > w) {
    const int64_t d = (h - w) / 2;
    if (d > 0) { y0 += d; h -= 2 * d; } else { y0 += 1; h -= 1; }
  } else if (h < w) {
    const int64_t d = (w - h) / 2;
    if (d > 0) { x0 += d; w -= 2 * d; } else { w -= 1; }
  }
  ok = ok && h <= FC_MAX_SIDE && w <= FC_MAX_SIDE;
  rects[4 * t + 0] = ok ? (int)x0 : 0;
  rects[4 * t + 1] = ok ? (int)y0 : 0;
  rects[4 * t + 2] = ok ? (int)w : 0;
  rects[4 * t + 3] = ok ? (int)h : 0;
  valid[t] = ok ? 1 : 0;
  if (!ok && err) atomicAdd(err, 1);
}

struct Window {
  const unsigned char* base;      // first byte of the window's first row
  int64_t pitch;                  // bytes between rows
  int w, h;
};

// the window of face t, checked against the source it is cut from: nothing below reads outside [src, src + src_bytes)
__device__ int window_of(const unsigned char* src, int64_t src_bytes, int N, int H, int W, const int* rects, const int* frame_index,
                         const unsigned char* valid, const int64_t* crops, int t, Window& s) {
  s.base = src;
  s.pitch = 0;
  s.w = s.h = 1;
  if (crops) {
    const int64_t off = crops[4 * t], pitch = crops[4 * t + 1], w = crops[4 * t + 2], h = crops[4 * t + 3];
    if (w < 1 || h < 1 || w > FC_MAX_SIDE || h > FC_MAX_SIDE || pitch < 3 * w || pitch > src_bytes || off < 0 || off > src_bytes) return FC_BAD;
    if ((h - 1) * pitch + 3 * w > src_bytes - off) return FC_BAD;
    s.base = src + off;
    s.pitch = pitch;
    s.w = (int)w;
    s.h = (int)h;
    return FC_OK;
  }
  if (!valid[t]) return FC_SKIP;
  const int f = frame_index[t], x0 = rects[4 * t], y0 = rects[4 * t + 1], w = rects[4 * t + 2], h = rects[4 * t + 3];
  if (f < 0 || f >= N || w < 1 || h < 1 || w > FC_MAX_SIDE || h > FC_MAX_SIDE || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return FC_BAD;
  s.base = src + (((int64_t)f * H + y0) * W + x0) * 3;
  s.pitch = (int64_t)W * 3;
  s.w = w;
  s.h = h;
  return FC_OK;
}

extern __shared__ int fc_dyn[];

// the horizontal pass of `rows` rows of 3-byte pixels starting at `p0` (row pitch `pitch` bytes) into q0 (row pitch q_pitch bytes):
// thread <-> (row, output column), three accumulators
__device__ __forceinline__ void horizontal_pass(const unsigned char* p0, int64_t pitch, int rows, unsigned char* q0, int64_t q_pitch, int OW,
                                                const int* kx, int ksx, const int* xfirst, const int* xcnt, int tid) {
  int row = tid / OW, ox = tid - row * OW;
  const int dq = FC_THREADS / OW, dr = FC_THREADS - dq * OW;
  while (row < rows) {
    const unsigned char* p = p0 + (int64_t)row * pitch + xfirst[ox] * 3;
    const int* k = kx + ox * ksx;
    const int n = xcnt[ox];
    int a0 = FC_HALF, a1 = FC_HALF, a2 = FC_HALF;
    for (int j = 0; j < n; ++j) {
      const int kk = k[j];
      a0 += (int)p[3 * j] * kk;
      a1 += (int)p[3 * j + 1] * kk;
      a2 += (int)p[3 * j + 2] * kk;
    }
    unsigned char* q = q0 + (int64_t)row * q_pitch + ox * 3;
    q[0] = clip8(a0);
    q[1] = clip8(a1);
    q[2] = clip8(a2);
    row += dq;
    ox += dr;
    if (ox >= OW) { ox -= OW; ++row; }
  }
}

__global__ __launch_bounds__(FC_THREADS) void crop_resize_kernel(const unsigned char* __restrict__ src, int64_t src_bytes, int N, int H, int W,
                                                                 const int* __restrict__ rects, const int* __restrict__ frame_index,
                                                                 const unsigned char* __restrict__ valid, const int64_t* __restrict__ crops,
                                                                 int OH, int OW, int kx_ints, int tile_bytes,
                                                                 unsigned char* __restrict__ out, int* __restrict__ err) {
  __shared__ int kyc[FC_KY];
  __shared__ int xfirst[FC_MAX_OUT], xcnt[FC_MAX_OUT];
  __shared__ double xsum[FC_MAX_OUT];
  __shared__ int yfirst[FC_BAND_ROWS], ycnt[FC_BAND_ROWS];
  __shared__ double ysum[FC_BAND_ROWS];
  int* kx = fc_dyn;
  unsigned char* tile = reinterpret_cast<unsigned char*>(fc_dyn + kx_ints);

  const int tid = threadIdx.x, t = blockIdx.y;
  const int band_rows = (OH + FC_BANDS - 1) / FC_BANDS;
  const int r0 = blockIdx.x * band_rows, r1 = min(r0 + band_rows, OH);
  if (r0 >= r1) return;                                  // uniform: no barrier has been reached
  const int OW3 = OW * 3;
  unsigned char* dst = out + (int64_t)t * OH * OW3;

  Window s;
  int state = window_of(src, src_bytes, N, H, W, rects, frame_index, valid, crops, t, s);
  const Axis ax = axis_of(s.w, OW), ay = axis_of(s.h, OH);
  const int ksx = ax.ksize, ksy = ay.ksize;
  if (state == FC_OK && (int64_t)OW * ksx > kx_ints) state = FC_BAD;      // wider than the bound the x table was sized for
  if (state != FC_OK) {                                  // uniform
    for (int e = tid; e < (r1 - r0) * OW3; e += FC_THREADS) dst[(int64_t)r0 * OW3 + e] = 0;
    if (state == FC_BAD && err && blockIdx.x == 0 && tid == 0) atomicOr(err + 1, 1);
    return;
  }

  // bounds and weight sums of every output column, and of this band's rows (taken by the other end of the block)
  for (int i = tid; i < OW; i += FC_THREADS) {
    int first, n;
    axis_bounds(ax, i, first, n);
    xfirst[i] = first;
    xcnt[i] = n;
    xsum[i] = axis_weight_sum(ax, i, first, n);
  }
  {
    const int i = FC_THREADS - 1 - tid;
    if (i < r1 - r0) {
      int first, n;
      axis_bounds(ay, r0 + i, first, n);
      yfirst[i] = first;
      ycnt[i] = n;
      ysum[i] = axis_weight_sum(ay, r0 + i, first, n);
    }
  }
  __syncthreads();
  for (int e = tid; e < OW * ksx; e += FC_THREADS) {
    const int i = e / ksx, j = e - i * ksx;
    kx[e] = j < xcnt[i] ? axis_coeff(ax, i, xfirst[i] + j, xsum[i]) : 0;
  }
  __syncthreads();

  if (s.h > 100 * s.w && OH < s.h) {
    // Image.resize's own exception: a strip over 100 times as tall as wide is shortened first.  w <= 40, so one thread per byte of
    // a source row; the band's intermediate rows [r1 - r0][w][3] (at most 3840 bytes) go in the tile.
    const int W3 = s.w * 3;
    for (int row = r0; row < r1; ++row) {
      const int first = yfirst[row - r0], n = ycnt[row - r0];
      const double sum = ysum[row - r0];
      int acc = FC_HALF;
      for (int c0 = 0; c0 < n; c0 += FC_KY) {
        const int m = min(FC_KY, n - c0);
        for (int e = tid; e < m; e += FC_THREADS) kyc[e] = axis_coeff(ay, row, first + c0 + e, sum);
        __syncthreads();
        if (tid < W3) {
          const unsigned char* p = s.base + (int64_t)(first + c0) * s.pitch + tid;
          for (int y = 0; y < m; ++y) acc += (int)p[(int64_t)y * s.pitch] * kyc[y];
        }
        __syncthreads();
      }
      if (tid < W3) tile[(row - r0) * W3 + tid] = clip8(acc);
    }
    __syncthreads();
    horizontal_pass(tile, W3, r1 - r0, dst + (int64_t)r0 * OW3, OW3, OW, kx, ksx, xfirst, xcnt, tid);
    return;
  }

  const int cap = tile_bytes / OW3;                      // rows of the horizontal pass the tile holds (>= 1)
  for (int a = r0; a < r1;) {
    // sub-band [a, b): as many output rows as have their source rows in the tile and their coefficients in kyc
    const int s0 = yfirst[a - r0];
    int b = a + 1;
    while (b < r1 && yfirst[b - r0] + ycnt[b - r0] - s0 <= cap && (b + 1 - a) * ksy <= FC_KY) ++b;
    const int s1 = yfirst[b - 1 - r0] + ycnt[b - 1 - r0];    // first and first + count never fall from one row to the next
    if (s1 - s0 <= cap && ksy <= FC_KY) {
      for (int e = tid; e < (b - a) * ksy; e += FC_THREADS) {
        const int rr = e / ksy, j = e - rr * ksy, i = a + rr - r0;
        kyc[e] = j < ycnt[i] ? axis_coeff(ay, a + rr, yfirst[i] + j, ysum[i]) : 0;
      }
      horizontal_pass(s.base + (int64_t)s0 * s.pitch, s.pitch, s1 - s0, tile, OW3, OW, kx, ksx, xfirst, xcnt, tid);
      __syncthreads();
      int rr = tid / OW3, jj = tid - rr * OW3;
      const int dq = FC_THREADS / OW3, dr = FC_THREADS - dq * OW3;
      while (rr < b - a) {
        const int i = a + rr - r0, n = ycnt[i];
        const unsigned char* p = tile + (yfirst[i] - s0) * OW3 + jj;
        const int* k = kyc + rr * ksy;
        int acc = FC_HALF;
        for (int y = 0; y < n; ++y) acc += (int)p[y * OW3] * k[y];
        dst[(int64_t)(a + rr) * OW3 + jj] = clip8(acc);
        rr += dq;
        jj += dr;
        if (jj >= OW3) { jj -= OW3; ++rr; }
      }
      __syncthreads();
    } else {
      // one output row whose source rows do not fit: fill the tile several times, sums kept in registers (OW3 <= 768 = 3 a thread)
      const int chunk = min(cap, FC_KY);
      const double sum = ysum[a - r0];
      int acc[3] = {FC_HALF, FC_HALF, FC_HALF};
      for (int c0 = s0; c0 < s1; c0 += chunk) {
        const int m = min(chunk, s1 - c0);
        for (int e = tid; e < m; e += FC_THREADS) kyc[e] = axis_coeff(ay, a, c0 + e, sum);
        horizontal_pass(s.base + (int64_t)c0 * s.pitch, s.pitch, m, tile, OW3, OW, kx, ksx, xfirst, xcnt, tid);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int jj = tid + q * FC_THREADS;
          if (jj < OW3)
            for (int y = 0; y < m; ++y) acc[q] += (int)tile[y * OW3 + jj] * kyc[y];
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int jj = tid + q * FC_THREADS;
        if (jj < OW3) dst[(int64_t)a * OW3 + jj] = clip8(acc[q]);
      }
    }
    a = b;
  }
}

}  // namespace

extern "C" int mt_face_rects(const float* boxes, const int* frame_index, int T, int N, int H, int W, int* rects, unsigned char* valid,
                             int* err, void* stream) {
  if (T < 0 || N < 1 || H < 1 || W < 1) return fail(MT_ERR_ARG, "mt_face_rects: T = %d, N = %d, H = %d, W = %d", T, N, H, W);
  if (T == 0) return 0;
  if (!boxes || !frame_index || !rects || !valid) return fail(MT_ERR_ARG, "mt_face_rects: null pointer");
  hipLaunchKernelGGL(face_rects_kernel, dim3((T + FC_THREADS - 1) / FC_THREADS), dim3(FC_THREADS), 0, (hipStream_t)stream, boxes, frame_index,
                     T, N, H, W, rects, valid, err);
  return check_launch("mt_face_rects");
}

extern "C" int mt_crop_resize_u8(const unsigned char* src, int64_t src_bytes, int N, int H, int W, const int* rects, const int* frame_index,
                                 const unsigned char* valid, const int64_t* crops, int T, int max_w, int OH, int OW, unsigned char* out,
                                 int* err, void* stream) {
  if (T < 0 || src_bytes < 0) return fail(MT_ERR_ARG, "mt_crop_resize_u8: T = %d, src_bytes = %lld", T, (long long)src_bytes);
  if (OH < 1 || OW < 1 || OH > FC_MAX_OUT || OW > FC_MAX_OUT)
    return fail(MT_ERR_UNSUPPORTED, "mt_crop_resize_u8: output %d x %d; sides of 1..%d are built", OH, OW, FC_MAX_OUT);
  if (max_w < 1 || max_w > FC_MAX_SIDE)
    return fail(MT_ERR_UNSUPPORTED, "mt_crop_resize_u8: max_w = %d; window sides of 1..%d are built", max_w, FC_MAX_SIDE);
  if (T > 65535) return fail(MT_ERR_UNSUPPORTED, "mt_crop_resize_u8: %d faces in one launch; at most 65535 (grid.y)", T);
  if (!crops) {
    if (N < 1 || H < 1 || W < 1) return fail(MT_ERR_ARG, "mt_crop_resize_u8: frames N = %d, H = %d, W = %d", N, H, W);
    if ((int64_t)N * H * W * 3 > src_bytes) return fail(MT_ERR_ARG, "mt_crop_resize_u8: %d frames of %d x %d exceed src_bytes", N, H, W);
    if (T > 0 && (!rects || !frame_index || !valid)) return fail(MT_ERR_ARG, "mt_crop_resize_u8: null pointer");
  }
  if (T == 0) return 0;
  if (!src || !out) return fail(MT_ERR_ARG, "mt_crop_resize_u8: null pointer");
  const int kx_ints = OW * axis_of(max_w, OW).ksize;     // never smaller than the table of a narrower window
  int tile_bytes = FC_DYN_LDS_MAX - kx_ints * 4;
  if (tile_bytes > FC_TILE_BYTES) tile_bytes = FC_TILE_BYTES;
  const size_t dyn = (size_t)kx_ints * 4 + tile_bytes;
  if (ensure_dynamic_lds(reinterpret_cast<const void*>(crop_resize_kernel), dyn) != hipSuccess)
    return fail(MT_ERR_LAUNCH, "mt_crop_resize_u8: %zu bytes of dynamic LDS refused", dyn);
  hipLaunchKernelGGL(crop_resize_kernel, dim3(FC_BANDS, T), dim3(FC_THREADS), dyn, (hipStream_t)stream, src, src_bytes, N, H, W, rects,
                     frame_index, valid, crops, OH, OW, kx_ints, tile_bytes, out, err);
  return check_launch("mt_crop_resize_u8");
}
