// Next-row f5: the epoch metrics of the reference's step bodies, kept on the device.  The reference copies the logits to the host
// every step and loops over them there (check_correct, utils.py:32-57; train.py:367-374, :434-441, test.py:267-277), then hands every
// stored prediction to sklearn's roc_curve / auc / f1_score at the end of a test run (test.py:280-283).  Here one small launch per
// step accumulates the counters and appends the (logit, label) pairs to a store in device memory; the AUC is an exact all-pairs
// count over that store at the end of the epoch.  Nothing in this file reads back to the host.
//
// Predicted class: 1 iff logit > 0.  The reference's rule is round(fp32 sigmoid(logit)), which is 1 iff sigmoid > 0.5 (round sends
// the tie at 0.5 to 0).  The two differ only for 0 < logit <~ 1.2e-7, where fp32 sigmoid returns exactly 0.5 and the reference
// predicts 0 (5e-8 -> 0, 1.1e-7 -> 1 there; 1 for both here).  logit == 0 is 0 under both rules; a NaN logit compares false: 0.
// AUC: ranks the logits, not fp32 sigmoid(logit) as the reference does; the rankings differ only where distinct logits collapse to
// one sigmoid value (saturation from about |logit| > 16.6, or neighbours closer than an ulp of the sigmoid).
//
// Every counter is an integer and the loss sums are fp64 additions in call order by one thread: the state is the same bits run
// after run, with or without deterministic mode.  No atomics: launches on one stream are serialised, so the state has one writer.
#include "common.hpp"
#include <stdint.h>
#include <math.h>

namespace {
using namespace mt;

// counts_i64 slots (mintime_hip.h)
enum { C_SEEN = 0, C_TP, C_FP, C_TN, C_FN, C_STEPS, C_STORED, C_OVERFLOW, C_SLOTS };
constexpr int MC_CLASSES = 9;                          // test.py:219
constexpr int UPD_VALUES = 4 + MC_CLASSES;             // tp, fp, tn, fn, then the error table

__global__ __launch_bounds__(256) void metrics_update_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ loss, const float* __restrict__ mc,
                                                             long long* __restrict__ counts, double* __restrict__ loss_sums,
                                                             long long* __restrict__ mc_errors, float* __restrict__ store_x,
                                                             unsigned char* __restrict__ store_y, long long capacity, int n) {
  __shared__ int red[4][UPD_VALUES];
  // the append position lives in the state: read by every thread BEFORE the barrier below, written by thread 0 after it
  const long long base = counts[C_STORED];
  int v[UPD_VALUES];
#pragma unroll
  for (int k = 0; k < UPD_VALUES; ++k) v[k] = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float xi = x[i];
    const bool yi = y[i] != 0.f, pi = xi > 0.f;        // NaN > 0 is false: predicted 0
    v[0] += pi && yi;
    v[1] += pi && !yi;
    v[2] += !pi && !yi;
    v[3] += !pi && yi;
    if (mc) {
      const float c = mc[i];                            // NaN fails every comparison: skipped, like the math.isnan guard
      const bool counted = (pi != yi) && c >= 0.f && c <= (float)(MC_CLASSES - 1) && c == truncf(c);
      const int ci = counted ? (int)c : -1;
#pragma unroll
      for (int k = 0; k < MC_CLASSES; ++k) v[4 + k] += ci == k;
    }
    const long long pos = base + i;
    if (pos < capacity) {
      store_x[pos] = xi;
      store_y[pos] = yi ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < UPD_VALUES; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[C_SEEN] += n;
    counts[C_TP] += red[0][0] + red[1][0] + red[2][0] + red[3][0];
    counts[C_FP] += red[0][1] + red[1][1] + red[2][1] + red[3][1];
    counts[C_TN] += red[0][2] + red[1][2] + red[2][2] + red[3][2];
    counts[C_FN] += red[0][3] + red[1][3] + red[2][3] + red[3][3];
    counts[C_STEPS] += 1;
    const long long end = base + n;
    counts[C_STORED] = end < capacity ? end : capacity;   // base <= capacity always: the store fills up to its last slot, then stops
    if (end > capacity) counts[C_OVERFLOW] = 1;
    if (loss) {
      const double l = (double)loss[0];
      loss_sums[0] += l;
      loss_sums[1] += rint(l * 100.0) / 100.0;          // Python's round(loss.item(), 2): halves to the even integer
    }
    if (mc)
      for (int k = 0; k < MC_CLASSES; ++k) mc_errors[k] += red[0][4 + k] + red[1][4 + k] + red[2][4 + k] + red[3][4 + k];
  }
}

// All-pairs count.  Thread i owns sample i; the block walks every j through LDS tiles.  A pair counts only for y_i = 1, y_j = 0 and
// two non-NaN scores, so the label is folded into the staged score: a tile entry is x_j when y_j = 0 and NaN otherwise, and the
// owner's score is x_i when y_i = 1 and NaN otherwise.  A comparison with NaN is false, so the inner loop is two compares and two
// adds per pair with no branch.  Every lane reads the same LDS address (a broadcast: no bank conflict), 16 bytes at a time.
constexpr int AUC_BLOCK = 256, AUC_TILE = 1024;
constexpr int AUC_PARTIAL = 4;                         // gt, eq, n_pos, n_neg per block

__global__ __launch_bounds__(AUC_BLOCK) void metrics_auc_pairs_kernel(const float* __restrict__ sx, const unsigned char* __restrict__ sy,
                                                                      int n, unsigned long long* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float tile[AUC_TILE];
  __shared__ unsigned long long red[AUC_BLOCK / 64][AUC_PARTIAL];
  const float nan = __int_as_float(0x7fc00000);
  const int i = blockIdx.x * AUC_BLOCK + threadIdx.x;
  float xi = nan;
  unsigned pos = 0, neg = 0;
  if (i < n) {
    const float s = sx[i];
    const bool valid = s == s, yi = sy[i] != 0;
    pos = valid && yi;
    neg = valid && !yi;
    if (pos) xi = s;
  }
  unsigned gt = 0, eq = 0;                               // at most n <= 2^24 each
  for (int j0 = 0; j0 < n; j0 += AUC_TILE) {
    __syncthreads();                                     // the previous tile has been read by every wavefront
#pragma unroll
    for (int k = 0; k < AUC_TILE / AUC_BLOCK; ++k) {
      const int t = k * AUC_BLOCK + threadIdx.x, j = j0 + t;
      float s = nan;
      if (j < n && sy[j] == 0) s = sx[j];               // a NaN score stays NaN
      tile[t] = s;
    }
    __syncthreads();
    const int left = n - j0, lim = left < AUC_TILE ? ((left + 3) & ~3) : AUC_TILE;     // entries past n hold NaN
    for (int t = 0; t < lim; t += 4) {
      const float4 s = *reinterpret_cast<const float4*>(tile + t);
      gt += xi > s.x; eq += xi == s.x;
      gt += xi > s.y; eq += xi == s.y;
      gt += xi > s.z; eq += xi == s.z;
      gt += xi > s.w; eq += xi == s.w;
    }
  }
  unsigned long long v[AUC_PARTIAL] = {gt, eq, pos, neg};    // widened here: a block's sum can pass 2^32
#pragma unroll
  for (int k = 0; k < AUC_PARTIAL; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < AUC_PARTIAL) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < AUC_BLOCK / 64; ++w) s += red[w][threadIdx.x];
    partials[(size_t)blockIdx.x * AUC_PARTIAL + threadIdx.x] = s;
  }
}

// second pass: the block partials in index order (integers: any order gives the same sum; this one is simply fixed)
__global__ __launch_bounds__(64) void metrics_auc_sum_kernel(const unsigned long long* __restrict__ partials, int blocks,
                                                             unsigned long long* __restrict__ out) {
  if (threadIdx.x < AUC_PARTIAL) {
    unsigned long long s = 0;
    for (int b = 0; b < blocks; ++b) s += partials[(size_t)b * AUC_PARTIAL + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

}  // namespace

extern "C" int mt_metrics_update(const float* logits, const float* labels, const float* loss, const float* mc_labels, int64_t* counts,
                                 double* loss_sums, int64_t* mc_errors, float* store_scores, unsigned char* store_labels,
                                 int64_t capacity, int n, void* stream) {
  if (!logits || !labels || !counts || n <= 0) return fail(MT_ERR_ARG, "mt_metrics_update: null pointer / empty batch");
  if (capacity < 0 || (capacity > 0 && (!store_scores || !store_labels)))
    return fail(MT_ERR_ARG, "mt_metrics_update: capacity %lld without a sample store", (long long)capacity);
  if ((loss && !loss_sums) || (mc_labels && !mc_errors)) return fail(MT_ERR_ARG, "mt_metrics_update: loss / class labels without their state");
  hipLaunchKernelGGL(metrics_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels, loss, mc_labels,
                     reinterpret_cast<long long*>(counts), loss_sums, reinterpret_cast<long long*>(mc_errors), store_scores,
                     store_labels, (long long)capacity, n);
  return check_launch("mt_metrics_update");
}

extern "C" int mt_metrics_auc(const float* store_scores, const unsigned char* store_labels, int64_t n, uint64_t* partials, uint64_t* out,
                              void* stream) {
  if (!out || n < 0) return fail(MT_ERR_ARG, "mt_metrics_auc: null output / negative n");
  if (n > ((int64_t)1 << 24)) return fail(MT_ERR_UNSUPPORTED, "mt_metrics_auc: n = %lld above 2^24", (long long)n);
  if (n == 0) {
    if (hipMemsetAsync(out, 0, AUC_PARTIAL * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess)
      return fail(MT_ERR_LAUNCH, "mt_metrics_auc: memset failed");
    return 0;
  }
  if (!store_scores || !store_labels || !partials) return fail(MT_ERR_ARG, "mt_metrics_auc: null pointer");
  const int blocks = (int)((n + AUC_BLOCK - 1) / AUC_BLOCK);
  hipLaunchKernelGGL(metrics_auc_pairs_kernel, dim3(blocks), dim3(AUC_BLOCK), 0, (hipStream_t)stream, store_scores, store_labels,
                     (int)n, reinterpret_cast<unsigned long long*>(partials));
  hipLaunchKernelGGL(metrics_auc_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(partials), blocks, reinterpret_cast<unsigned long long*>(out));
  return check_launch("mt_metrics_auc");
}
