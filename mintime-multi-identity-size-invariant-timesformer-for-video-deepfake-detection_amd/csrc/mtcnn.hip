// MTCNN face detector (the reference's FacenetDetector: preprocessing/face_detector.py:38-56 builds facenet_pytorch's MTCNN and
// calls .detect(frames, landmarks=False)), kept on the device from the decoded frames to the boxes.  include/mintime_hip.h states
// the algorithm and every entry point in full; DESIGN.md section 3.14 has the decisions.
//   mt_mtcnn_pnet        one pyramid level: area resample + normalise a tile of the frame into LDS, conv1 + PReLU + ceil-mode pool,
//                        conv2 + PReLU, conv3 + PReLU, both heads, softmax, the >= threshold test and the candidate append, with
//                        nothing but the candidates written to memory (the maps and the level only on request, for the tests)
//   mt_mtcnn_nms         greedy NMS of ragged segments, one wavefront per segment: sort by (score desc, key asc), sweep, compact
//   mt_mtcnn_boxes       refine / bbreg / rerec / pad, one thread per box, every operation rounded on its own
//   mt_mtcnn_crop        pad windows -> [rows][S][S][4] fp32, area resampled and normalised (the input rows of mt_conv2d_fwd)
//   mt_mtcnn_prelu_pool  PReLU + ceil-mode MaxPool(k, s) of channels-last rows (k = 1: PReLU alone)
//   mt_mtcnn_score       two-way softmax of the stacked head rows, the strict threshold test, the regression values
//   mt_mtcnn_finalize    per-image lists -> one compact list (Detections)
// A record is 12 floats: x1 y1 x2 y2 score reg[4] key(int32) 0 0.  key = level << 24 | (y Wm + x) names the P-Net map position a
// box came from; it is the tie-break of every NMS order (deviation (a)), so no result depends on the order of the appends.
// Contraction is off for the whole file: torch rounds a * b + c twice, hipcc would fuse it, and one fused refine moves a truncated
// coordinate.  The convolutions ask for their fused multiply-adds by name (fmaf).
#include "common.hpp"
#include <stdint.h>

#pragma clang fp contract(off)

namespace {
using namespace mt;

constexpr int REC = 12;
enum { R_X1 = 0, R_Y1 = 1, R_X2 = 2, R_Y2 = 3, R_SCORE = 4, R_REG = 5, R_KEY = 9 };
enum { ERR_LEVEL_LIST = 1, ERR_MAX = 31 };

constexpr int PN_THREADS = 256;
constexpr int PN_T = 16;                      // map positions per tile side
constexpr int PN_IN = 2 * PN_T + 10;          // 42: level pixels a tile reads per side (receptive field 12, stride 2)
constexpr int PN_P = PN_T + 4;                // 20: pooled positions
constexpr int PN_C2 = PN_T + 2;               // 18: conv2 positions
// packed P-Net weights (mtcnn_engine.pack_pnet): every filter as [ky][kx][ci][co], so the co weights of one input value are adjacent
constexpr int PW_W1 = 0, PW_B1 = 270, PW_A1 = 280, PW_W2 = 290, PW_B2 = 1730, PW_A2 = 1746, PW_W3 = 1762, PW_B3 = 6370, PW_A3 = 6402,
              PW_W4 = 6434, PW_B4 = 6626, PW_FLOATS = 6632;
constexpr int NMS_MAX = 1024;
constexpr int FIN_MAX_IMAGES = 4096;

__device__ __forceinline__ float prelu(float v, float a) { return v > 0.0f ? v : a * v; }

// torch.softmax over two channels, channel 1: exp(l1 - max) / (exp(l0 - max) + exp(l1 - max))
__device__ __forceinline__ float softmax2(float l0, float l1) {
  const float m = fmaxf(l0, l1);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m);
  return __fdiv_rn(e1, e0 + e1);
}

// area_resize: output cell i of `out` averages source indices floor(i in / out) .. ceil((i + 1) in / out) - 1
__device__ __forceinline__ void area_span(int i, int in, int out, int& first, int& end) {
  first = (int)(((int64_t)i * in) / out);
  end = (int)((((int64_t)i + 1) * in + out - 1) / out);
}

// one resampled, normalised pixel: integer sums (exact), one division, (v - 127.5) * 0.0078125
__device__ __forceinline__ void area_pixel(const unsigned char* __restrict__ img, int64_t pitch, int y0, int y1, int x0, int x1, float* v) {
  int s0 = 0, s1 = 0, s2 = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* p = img + (int64_t)y * pitch + (int64_t)x0 * 3;
    for (int x = x0; x < x1; ++x, p += 3) {
      s0 += p[0];
      s1 += p[1];
      s2 += p[2];
    }
  }
  const float cnt = (float)((y1 - y0) * (x1 - x0));
  v[0] = (__fdiv_rn((float)s0, cnt) - 127.5f) * 0.0078125f;
  v[1] = (__fdiv_rn((float)s1, cnt) - 127.5f) * 0.0078125f;
  v[2] = (__fdiv_rn((float)s2, cnt) - 127.5f) * 0.0078125f;
}

__global__ __launch_bounds__(PN_THREADS) void pnet_kernel(const unsigned char* __restrict__ frames, int H, int W, int Hs, int Ws, int Hm,
                                                          int Wm, float scale, int level, int levels, const float* __restrict__ wt,
                                                          float thr, float* __restrict__ rec, int* __restrict__ counts, int cap,
                                                          int* __restrict__ err, float* __restrict__ dbg_level,
                                                          float* __restrict__ dbg_maps) {
  __shared__ float s_in[3][PN_IN][PN_IN + 1];
  __shared__ float s_p[10][PN_P][PN_P + 1];
  __shared__ float s_c2[16][PN_C2][PN_C2 + 1];
  __shared__ int s_cnt, s_base;

  const int tid = threadIdx.x, n = blockIdx.y;
  const int tx_n = (Wm + PN_T - 1) / PN_T;
  const int ty0 = (blockIdx.x / tx_n) * PN_T, tx0 = (blockIdx.x % tx_n) * PN_T;
  const unsigned char* img = frames + (int64_t)n * H * W * 3;
  if (tid == 0) s_cnt = 0;

  // the level's pixels under this tile, resampled from the frame
  for (int e = tid; e < PN_IN * PN_IN; e += PN_THREADS) {
    const int iy = e / PN_IN, ix = e - iy * PN_IN;
    const int gy = 2 * ty0 + iy, gx = 2 * tx0 + ix;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (gy < Hs && gx < Ws) {
      int y0, y1, x0, x1;
      area_span(gy, H, Hs, y0, y1);
      area_span(gx, W, Ws, x0, x1);
      area_pixel(img, (int64_t)W * 3, y0, y1, x0, x1, v);
      if (dbg_level) {
        float* d = dbg_level + (((int64_t)n * Hs + gy) * Ws + gx) * 3;      // tiles overlap: the same value from each
        d[0] = v[0];
        d[1] = v[1];
        d[2] = v[2];
      }
    }
    s_in[0][iy][ix] = v[0];
    s_in[1][iy][ix] = v[1];
    s_in[2][iy][ix] = v[2];
  }
  __syncthreads();

  // conv1 (3 -> 10, k3) + PReLU + MaxPool(2, 2, ceil_mode): a window at the level's edge holds the conv1 outputs that exist
  const int c1h = Hs - 2, c1w = Ws - 2;
  for (int e = tid; e < PN_P * PN_P; e += PN_THREADS) {
    const int py = e / PN_P, px = e - py * PN_P;
    float m[10];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 10; ++c) m[c] = 0.0f;
    for (int d = 0; d < 4; ++d) {
      const int dy = d >> 1, dx = d & 1;
      if (2 * (ty0 + py) + dy >= c1h || 2 * (tx0 + px) + dx >= c1w) continue;
      float acc[10];
#pragma unroll
      for (int c = 0; c < 10; ++c) acc[c] = wt[PW_B1 + c];
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float x = s_in[ci][2 * py + dy + ky][2 * px + dx + kx];
#pragma unroll
          for (int c = 0; c < 10; ++c) acc[c] = fmaf(x, wt[PW_W1 + (tap * 3 + ci) * 10 + c], acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 10; ++c) {
        const float v = prelu(acc[c], wt[PW_A1 + c]);
        m[c] = any ? fmaxf(m[c], v) : v;
      }
      any = true;
    }
#pragma unroll
    for (int c = 0; c < 10; ++c) s_p[c][py][px] = m[c];
  }
  __syncthreads();

  // conv2 (10 -> 16, k3) + PReLU
  for (int e = tid; e < PN_C2 * PN_C2; e += PN_THREADS) {
    const int y = e / PN_C2, x = e - y * PN_C2;
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = wt[PW_B2 + c];
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int ci = 0; ci < 10; ++ci) {
        const float v = s_p[ci][y + ky][x + kx];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, wt[PW_W2 + (tap * 10 + ci) * 16 + c], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) s_c2[c][y][x] = prelu(acc[c], wt[PW_A2 + c]);
  }
  __syncthreads();

  // conv3 (16 -> 32, k3) + PReLU and the heads, one map position a thread, in registers
  const int y = tid / PN_T, x = tid - y * PN_T;
  float acc[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) acc[c] = wt[PW_B3 + c];
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
    for (int ci = 0; ci < 16; ++ci) {
      const float v = s_c2[ci][y + ky][x + kx];
#pragma unroll
      for (int c = 0; c < 32; ++c) acc[c] = fmaf(v, wt[PW_W3 + (tap * 16 + ci) * 32 + c], acc[c]);
    }
  }
  float o[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) o[j] = wt[PW_B4 + j];
#pragma unroll
  for (int ci = 0; ci < 32; ++ci) {
    const float v = prelu(acc[ci], wt[PW_A3 + ci]);
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = fmaf(v, wt[PW_W4 + ci * 6 + j], o[j]);
  }
  const float prob = softmax2(o[0], o[1]);
  const int gy = ty0 + y, gx = tx0 + x;
  const bool inside = gy < Hm && gx < Wm;
  if (inside && dbg_maps) {
    float* d = dbg_maps + (int64_t)n * 5 * Hm * Wm + (int64_t)gy * Wm + gx;
    d[0] = prob;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[(int64_t)(j + 1) * Hm * Wm] = o[2 + j];
  }

  // candidates: one LDS counter per block, one global add per block
  const bool hit = inside && prob >= thr;
  int slot = 0;
  if (hit) slot = atomicAdd(&s_cnt, 1);
  __syncthreads();
  const int seg = n * levels + level;
  if (tid == 0) s_base = s_cnt > 0 ? atomicAdd(&counts[seg], s_cnt) : 0;
  __syncthreads();
  if (hit) {
    const int at = s_base + slot;
    if (at < cap) {
      float* r = rec + ((int64_t)seg * cap + at) * REC;
      r[R_X1] = floorf(__fdiv_rn((float)(2 * gx + 1), scale));
      r[R_Y1] = floorf(__fdiv_rn((float)(2 * gy + 1), scale));
      r[R_X2] = floorf(__fdiv_rn((float)(2 * gx + 12), scale));
      r[R_Y2] = floorf(__fdiv_rn((float)(2 * gy + 12), scale));
      r[R_SCORE] = prob;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[R_REG + j] = o[2 + j];
      r[R_KEY] = __int_as_float((level << 24) | (gy * Wm + gx));
      r[10] = 0.0f;
      r[11] = 0.0f;
    } else {
      atomicOr(err, ERR_LEVEL_LIST);
    }
  }
}

__device__ __forceinline__ int seg_count(const int* counts, int seg, int cap) {
  const int c = counts[seg];
  return c < 0 ? 0 : (c > cap ? cap : c);
}

// one wavefront per segment
__global__ __launch_bounds__(64) void nms_kernel(const float* __restrict__ rec_in, const int* __restrict__ count_in, int cap_in, int group,
                                                 int form, float thr, float* __restrict__ rec_out, int* __restrict__ count_out,
                                                 int cap_out, int* __restrict__ picks, int* __restrict__ err, int err_bit) {
  __shared__ unsigned long long s_key[NMS_MAX];
  __shared__ short s_idx[NMS_MAX], s_keep[NMS_MAX];
  __shared__ float s_box[4][NMS_MAX], s_area[NMS_MAX];
  __shared__ unsigned char s_dead[NMS_MAX];
  __shared__ int s_alive, s_base;

  const int lane = threadIdx.x, seg = blockIdx.x;
  const int n = seg_count(count_in, seg, cap_in);
  const float* in = rec_in + (int64_t)seg * cap_in * REC;
  int P = 1;
  while (P < n) P <<= 1;
  if (lane == 0) s_alive = 0;
  for (int i = lane; i < P; i += 64) {
    unsigned long long k = ~0ull;
    if (i < n) {
      const float sc = in[i * REC + R_SCORE];
      if (sc >= 0.0f)                                     // a dropped row carries -1; NaN is dropped too
        k = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(sc)) << 32) | (unsigned)__float_as_int(in[i * REC + R_KEY]);
    }
    s_key[i] = k;
    s_idx[i] = (short)i;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < P; i += 64) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long a = s_key[i], b = s_key[p];
          if ((a > b) == ((i & k) == 0)) {
            s_key[i] = b;
            s_key[p] = a;
            const short t = s_idx[i];
            s_idx[i] = s_idx[p];
            s_idx[p] = t;
          }
        }
      }
      __syncthreads();
    }
  int mine = 0;
  for (int i = lane; i < n; i += 64) mine += s_key[i] != ~0ull;
  if (mine) atomicAdd(&s_alive, mine);
  __syncthreads();
  const int m = s_alive;
  for (int i = lane; i < m; i += 64) {
    const float* r = in + (int)s_idx[i] * REC;
    const float x1 = r[R_X1], y1 = r[R_Y1], x2 = r[R_X2], y2 = r[R_Y2];
    s_box[0][i] = x1;
    s_box[1][i] = y1;
    s_box[2][i] = x2;
    s_box[3][i] = y2;
    s_area[i] = form ? __fmul_rn(x2 - x1 + 1.0f, y2 - y1 + 1.0f) : __fmul_rn(x2 - x1, y2 - y1);
    s_dead[i] = 0;
  }
  __syncthreads();
  int kept = 0;
  const float one = form ? 1.0f : 0.0f;
  for (int i = 0; i < m; ++i) {
    if (s_dead[i]) continue;                              // the same in every lane
    if (lane == 0) s_keep[kept] = (short)i;
    ++kept;
    const float x1 = s_box[0][i], y1 = s_box[1][i], x2 = s_box[2][i], y2 = s_box[3][i], a = s_area[i];
    for (int j = i + 1 + lane; j < m; j += 64) {
      if (s_dead[j]) continue;
      const float w = fmaxf(0.0f, fminf(x2, s_box[2][j]) - fmaxf(x1, s_box[0][j]) + one);
      const float h = fmaxf(0.0f, fminf(y2, s_box[3][j]) - fmaxf(y1, s_box[1][j]) + one);
      const float inter = __fmul_rn(w, h);
      const float den = form ? fminf(a, s_area[j]) : a + s_area[j] - inter;
      if (__fdiv_rn(inter, den) > thr) s_dead[j] = 1;
    }
    __syncthreads();
  }
  if (lane == 0) {
    if (group > 1) {
      s_base = kept > 0 ? atomicAdd(&count_out[seg / group], kept) : 0;
    } else {
      s_base = 0;
      count_out[seg] = kept;
    }
  }
  __syncthreads();
  const int base = s_base;
  float* out = rec_out + (int64_t)(seg / group) * cap_out * REC;
  bool over = false;
  for (int t = lane; t < kept; t += 64) {
    const int src = s_idx[s_keep[t]];
    if (base + t < cap_out) {
#pragma unroll
      for (int q = 0; q < REC; ++q) out[(int64_t)(base + t) * REC + q] = in[src * REC + q];
    } else {
      over = true;
    }
  }
  if (over && err) atomicOr(err, err_bit);
  if (picks)
    for (int t = lane; t < cap_in; t += 64) picks[(int64_t)seg * cap_in + t] = t < kept ? (int)s_idx[s_keep[t]] : -1;
}

__global__ __launch_bounds__(256) void boxes_kernel(float* __restrict__ rec, const int* __restrict__ counts, int segs, int cap, int mode, int H,
                                                    int W, int* __restrict__ win) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)segs * cap) return;
  const int seg = (int)(t / cap), i = (int)(t - (int64_t)seg * cap);
  if (i >= seg_count(counts, seg, cap)) {
    if (win) *reinterpret_cast<int4*>(win + 4 * t) = make_int4(0, 0, 0, 0);
    return;
  }
  float* r = rec + t * REC;
  float x1 = r[R_X1], y1 = r[R_Y1], x2 = r[R_X2], y2 = r[R_Y2];
  if (mode != 0) {
    float w = x2 - x1, h = y2 - y1;
    if (mode != 1) {                                      // bbreg measures inclusive pixels
      w = w + 1.0f;
      h = h + 1.0f;
    }
    x1 = x1 + r[R_REG + 0] * w;
    y1 = y1 + r[R_REG + 1] * h;
    x2 = x2 + r[R_REG + 2] * w;
    y2 = y2 + r[R_REG + 3] * h;
    if (mode != 3) {                                      // rerec
      h = y2 - y1;
      w = x2 - x1;
      const float l = fmaxf(w, h);
      x1 = x1 + w * 0.5f - l * 0.5f;
      y1 = y1 + h * 0.5f - l * 0.5f;
      x2 = x1 + l;
      y2 = y1 + l;
    }
    r[R_X1] = x1;
    r[R_Y1] = y1;
    r[R_X2] = x2;
    r[R_Y2] = y2;
  }
  if (win) {
    const float lim = 1073741824.0f;                      // conversions below stay defined; frames are far smaller
    int x = (int)fminf(fmaxf(x1, -lim), lim), y = (int)fminf(fmaxf(y1, -lim), lim);
    int ex = (int)fminf(fmaxf(x2, -lim), lim), ey = (int)fminf(fmaxf(y2, -lim), lim);
    if (!(x1 == x1)) x = 0;
    if (!(y1 == y1)) y = 0;
    if (!(x2 == x2)) ex = 0;
    if (!(y2 == y2)) ey = 0;
    x = x < 1 ? 1 : x;
    y = y < 1 ? 1 : y;
    ex = ex > W ? W : ex;
    ey = ey > H ? H : ey;
    *reinterpret_cast<int4*>(win + 4 * t) = make_int4(x, y, ex, ey);
  }
}

// a window that holds no pixel (deviation (c)), or one that does not lie in the frame (never produced by boxes_kernel)
__device__ __forceinline__ bool window_ok(int4 w, int H, int W) {
  return w.x >= 1 && w.y >= 1 && w.z <= W && w.w <= H && w.w > w.y - 1 && w.z > w.x - 1;
}

__global__ __launch_bounds__(256) void crop_kernel(const unsigned char* __restrict__ frames, int H, int W, const int* __restrict__ win,
                                                   const int* __restrict__ counts, int cap, int S, float* __restrict__ out) {
  const int row = blockIdx.x, seg = blockIdx.y;
  const int64_t t = (int64_t)seg * cap + row;
  float4* dst = reinterpret_cast<float4*>(out) + t * S * S;
  int4 w = make_int4(1, 1, 0, 0);
  if (row < seg_count(counts, seg, cap)) w = *reinterpret_cast<const int4*>(win + 4 * t);
  if (!window_ok(w, H, W)) {
    for (int e = threadIdx.x; e < S * S; e += 256) dst[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const int wy = w.y - 1, wx = w.x - 1, wh = w.w - wy, ww = w.z - wx;
  const unsigned char* img = frames + ((int64_t)seg * H + wy) * W * 3 + (int64_t)wx * 3;
  for (int e = threadIdx.x; e < S * S; e += 256) {
    const int oy = e / S, ox = e - oy * S;
    int y0, y1, x0, x1;
    area_span(oy, wh, S, y0, y1);
    area_span(ox, ww, S, x0, x1);
    float v[3];
    area_pixel(img, (int64_t)W * 3, y0, y1, x0, x1, v);
    dst[e] = make_float4(v[0], v[1], v[2], 0.0f);
  }
}

__global__ __launch_bounds__(256) void prelu_pool_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ slope,
                                                         int64_t total, int H, int W, int C4, int Ho, int Wo, int k, int s,
                                                         const int* __restrict__ counts, int cap) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c4 = (int)(t % C4);
  int64_t q = t / C4;
  const int ox = (int)(q % Wo);
  q /= Wo;
  const int oy = (int)(q % Ho);
  const int64_t n = q / Ho;
  if (counts && (int)(n % cap) >= seg_count(counts, (int)(n / cap), cap)) return;
  const float4 a = reinterpret_cast<const float4*>(slope)[c4];
  const float4* src = reinterpret_cast<const float4*>(x) + n * H * W * C4 + c4;
  float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  bool any = false;
  for (int dy = 0; dy < k; ++dy) {
    const int iy = oy * s + dy;
    if (iy >= H) break;
    for (int dx = 0; dx < k; ++dx) {
      const int ix = ox * s + dx;
      if (ix >= W) break;
      const float4 v = src[((int64_t)iy * W + ix) * C4];
      const float4 p = make_float4(prelu(v.x, a.x), prelu(v.y, a.y), prelu(v.z, a.z), prelu(v.w, a.w));
      m = any ? make_float4(fmaxf(m.x, p.x), fmaxf(m.y, p.y), fmaxf(m.z, p.z), fmaxf(m.w, p.w)) : p;
      any = true;
    }
  }
  reinterpret_cast<float4*>(y)[t] = m;
}

__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ head, int ldh, float* __restrict__ rec,
                                                    const int* __restrict__ win, const int* __restrict__ counts, int segs, int cap, int H,
                                                    int W, float thr) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)segs * cap) return;
  const int seg = (int)(t / cap), i = (int)(t - (int64_t)seg * cap);
  if (i >= seg_count(counts, seg, cap)) return;
  const float* h = head + t * ldh;
  float* r = rec + t * REC;
  const float p = softmax2(h[0], h[1]);
  const bool ok = window_ok(*reinterpret_cast<const int4*>(win + 4 * t), H, W);
  r[R_SCORE] = (ok && p > thr) ? p : -1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[R_REG + j] = h[2 + j];
}

__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ rec, const int* __restrict__ counts, int N, int cap,
                                                       int max_faces, float* __restrict__ boxes, float* __restrict__ probs,
                                                       int* __restrict__ frame_index, int* __restrict__ count,
                                                       int* __restrict__ image_counts, int* __restrict__ err, int err_bit) {
  __shared__ int s_off[FIN_MAX_IMAGES + 1];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int at = 0;
    for (int n = 0; n < N; ++n) {
      s_off[n] = at;
      at += seg_count(counts, n, cap);
    }
    s_off[N] = at;
    if (at > max_faces) atomicOr(err, err_bit);
    *count = at < max_faces ? at : max_faces;
  }
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    const int lo = s_off[n] < max_faces ? s_off[n] : max_faces, hi = s_off[n + 1] < max_faces ? s_off[n + 1] : max_faces;
    image_counts[n] = hi - lo;
  }
  for (int64_t t = tid; t < (int64_t)N * cap; t += 256) {
    const int n = (int)(t / cap), i = (int)(t - (int64_t)n * cap);
    const int d = s_off[n] + i;
    if (i >= s_off[n + 1] - s_off[n] || d >= max_faces) continue;
    const float* r = rec + t * REC;
    boxes[4 * d + 0] = r[R_X1];
    boxes[4 * d + 1] = r[R_Y1];
    boxes[4 * d + 2] = r[R_X2];
    boxes[4 * d + 3] = r[R_Y2];
    probs[d] = r[R_SCORE];
    frame_index[d] = n;
  }
  for (int d = s_off[N] + tid; d < max_faces; d += 256) {
    boxes[4 * d + 0] = boxes[4 * d + 1] = boxes[4 * d + 2] = boxes[4 * d + 3] = 0.0f;
    probs[d] = 0.0f;
    frame_index[d] = -1;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int pnet_map(int s) { return (s - 2 + 1) / 2 - 4; }      // conv1, ceil-mode pool, conv2, conv3

}  // namespace

extern "C" int mt_mtcnn_pnet(const unsigned char* frames, int N, int H, int W, int Hs, int Ws, float scale, int level, int levels,
                             const float* weights, float thr, float* rec, int* counts, int cap, int* err, float* dbg_level,
                             float* dbg_maps, void* stream) {
  const char* what = "mt_mtcnn_pnet";
  if (N < 1 || H < 1 || W < 1 || Hs < 12 || Ws < 12 || cap < 1 || levels < 1 || level < 0 || level >= levels || !(scale > 0.0f))
    return fail(MT_ERR_ARG, "%s: N = %d, frame %d x %d, level %d x %d (at least 12 x 12), scale %g, level %d of %d, cap %d", what, N, H, W,
                Hs, Ws, (double)scale, level, levels, cap);
  if (!frames || !weights || !rec || !counts || !err) return fail(MT_ERR_ARG, "%s: null pointer", what);
  const int Hm = pnet_map(Hs), Wm = pnet_map(Ws);
  if (levels > 127 || (int64_t)Hm * Wm >= (1 << 24) || N > 65535 || (int64_t)N * levels > 0x7fffffff / cap || H > (1 << 20) || W > (1 << 20) ||
      Hs > (1 << 20) || Ws > (1 << 20))
    return fail(MT_ERR_UNSUPPORTED, "%s: at most 127 levels, 2^24 map positions, 65535 frames and 2^31 candidate slots", what);
  const int tiles = ((Hm + PN_T - 1) / PN_T) * ((Wm + PN_T - 1) / PN_T);
  hipLaunchKernelGGL(pnet_kernel, dim3(tiles, N), dim3(PN_THREADS), 0, (hipStream_t)stream, frames, H, W, Hs, Ws, Hm, Wm, scale, level, levels,
                     weights, thr, rec, counts, cap, err, dbg_level, dbg_maps);
  return check_launch(what);
}

extern "C" int mt_mtcnn_nms(const float* rec_in, const int* count_in, int segs, int cap_in, int group, int form, float thr, float* rec_out,
                            int* count_out, int cap_out, int* picks, int* err, int err_bit, void* stream) {
  const char* what = "mt_mtcnn_nms";
  if (segs < 0 || cap_in < 1 || cap_out < 1 || group < 1 || (form != 0 && form != 1) || !(thr >= 0.0f) || err_bit < 0 || err_bit > ERR_MAX)
    return fail(MT_ERR_ARG, "%s: segs = %d, cap_in = %d, cap_out = %d, group = %d, form = %d, thr = %g", what, segs, cap_in, cap_out, group,
                form, (double)thr);
  if (cap_in > NMS_MAX) return fail(MT_ERR_UNSUPPORTED, "%s: segments of up to %d boxes are built; cap_in = %d", what, NMS_MAX, cap_in);
  if (segs == 0) return 0;
  if (segs % group) return fail(MT_ERR_ARG, "%s: %d segments do not divide into groups of %d", what, segs, group);
  if (!rec_in || !count_in || !rec_out || !count_out || rec_in == rec_out || (err_bit && !err)) return fail(MT_ERR_ARG, "%s: null or aliased pointer", what);
  hipLaunchKernelGGL(nms_kernel, dim3(segs), dim3(64), 0, (hipStream_t)stream, rec_in, count_in, cap_in, group, form, thr, rec_out, count_out,
                     cap_out, picks, err, err_bit);
  return check_launch(what);
}

extern "C" int mt_mtcnn_boxes(float* rec, const int* counts, int segs, int cap, int mode, int H, int W, int* win, void* stream) {
  const char* what = "mt_mtcnn_boxes";
  if (segs < 0 || cap < 1 || mode < 0 || mode > 3 || H < 1 || W < 1 || (int64_t)segs * cap > 0x7fffffff)
    return fail(MT_ERR_ARG, "%s: segs = %d, cap = %d, mode = %d, frame %d x %d", what, segs, cap, mode, H, W);
  if (segs == 0) return 0;
  if (!rec || !counts || (mode == 0 && !win) || !al16(win)) return fail(MT_ERR_ARG, "%s: null or misaligned pointer", what);
  const int64_t total = (int64_t)segs * cap;
  hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, counts, segs, cap, mode, H, W,
                     win);
  return check_launch(what);
}

extern "C" int mt_mtcnn_crop(const unsigned char* frames, int N, int H, int W, const int* win, const int* counts, int cap, int S, float* out,
                             void* stream) {
  const char* what = "mt_mtcnn_crop";
  if (N < 1 || H < 1 || W < 1 || cap < 1 || S < 1 || S > 256 || H > (1 << 20) || W > (1 << 20))
    return fail(MT_ERR_ARG, "%s: N = %d, frame %d x %d, cap = %d, S = %d", what, N, H, W, cap, S);
  if (N > 65535) return fail(MT_ERR_UNSUPPORTED, "%s: %d frames in one launch; at most 65535 (grid.y)", what, N);
  if (!frames || !win || !counts || !out || !al16(win) || !al16(out)) return fail(MT_ERR_ARG, "%s: null or misaligned pointer", what);
  hipLaunchKernelGGL(crop_kernel, dim3(cap, N), dim3(256), 0, (hipStream_t)stream, frames, H, W, win, counts, cap, S, out);
  return check_launch(what);
}

extern "C" int mt_mtcnn_prelu_pool(const float* x, float* y, const float* slope, int64_t rows, int H, int W, int C, int k, int s,
                                   const int* counts, int cap, void* stream) {
  const char* what = "mt_mtcnn_prelu_pool";
  if (rows < 0 || H < 1 || W < 1 || C < 1 || k < 1 || k > 3 || s < 1 || (k == 1 && s != 1) || k > H || k > W || (counts && cap < 1))
    return fail(MT_ERR_ARG, "%s: rows = %lld, %d x %d x %d, k = %d, s = %d", what, (long long)rows, H, W, C, k, s);
  if (C & 3) return fail(MT_ERR_UNSUPPORTED, "%s: C = %d is not a multiple of 4", what, C);
  if (rows == 0) return 0;
  if (!x || !y || !slope || x == y || !al16(x) || !al16(y) || !al16(slope)) return fail(MT_ERR_ARG, "%s: null, aliased or misaligned pointer", what);
  int Ho = (H - k + s - 1) / s + 1, Wo = (W - k + s - 1) / s + 1;      // ceil_mode; the last window starts inside the input
  if ((Ho - 1) * s >= H) --Ho;
  if ((Wo - 1) * s >= W) --Wo;
  const int64_t total = rows * Ho * Wo * (C / 4);
  if (total > (int64_t)0x7fffffff * 256) return fail(MT_ERR_UNSUPPORTED, "%s: too many elements", what);
  hipLaunchKernelGGL(prelu_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, slope, total, H, W, C / 4,
                     Ho, Wo, k, s, counts, cap);
  return check_launch(what);
}

extern "C" int mt_mtcnn_score(const float* head, int ldh, float* rec, const int* win, const int* counts, int segs, int cap, int H, int W,
                              float thr, void* stream) {
  const char* what = "mt_mtcnn_score";
  if (segs < 0 || cap < 1 || ldh < 6 || H < 1 || W < 1 || (int64_t)segs * cap > 0x7fffffff)
    return fail(MT_ERR_ARG, "%s: segs = %d, cap = %d, ldh = %d, frame %d x %d", what, segs, cap, ldh, H, W);
  if (segs == 0) return 0;
  if (!head || !rec || !win || !counts || !al16(win)) return fail(MT_ERR_ARG, "%s: null or misaligned pointer", what);
  const int64_t total = (int64_t)segs * cap;
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, head, ldh, rec, win, counts, segs,
                     cap, H, W, thr);
  return check_launch(what);
}

extern "C" int mt_mtcnn_finalize(const float* rec, const int* counts, int N, int cap, int max_faces, float* boxes, float* probs,
                                 int* frame_index, int* count, int* image_counts, int* err, int err_bit, void* stream) {
  const char* what = "mt_mtcnn_finalize";
  if (N < 1 || cap < 1 || max_faces < 1 || err_bit < 1 || err_bit > ERR_MAX)
    return fail(MT_ERR_ARG, "%s: N = %d, cap = %d, max_faces = %d", what, N, cap, max_faces);
  if (N > FIN_MAX_IMAGES) return fail(MT_ERR_UNSUPPORTED, "%s: %d frames; at most %d", what, N, FIN_MAX_IMAGES);
  if (!rec || !counts || !boxes || !probs || !frame_index || !count || !image_counts || !err) return fail(MT_ERR_ARG, "%s: null pointer", what);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rec, counts, N, cap, max_faces, boxes, probs, frame_index,
                     count, image_counts, err, err_bit);
  return check_launch(what);
}
