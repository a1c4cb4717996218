// Dispatch of the split-operand GEMM main loop (gemm_split.hpp): fp32 operands split exactly into three bf16 pieces, six
// piece products per fp32 product on the bf16 matrix pipe, fp32 accumulators.  mt_gemm (gemm.hip) asks try_launch_split()
// first; problems it does not take (most operand prologues, tiny or K % 8 != 0 shapes) go on to the fp32-MFMA kernels.
#include "gemm_split_dispatch.hpp"
#include <atomic>
#include <mutex>

using namespace mt;

namespace {

// 0 = fp32 MFMA everywhere, 1 = split-operand bf16x6 where eligible.  Process-wide; MT_GEMM_SPLIT sets the initial value.
int g_mode = -1;
int mode() {
  if (g_mode < 0) g_mode = env_int("MT_GEMM_SPLIT", 1) != 0;
  return g_mode;
}

// Arithmetic tier of the bf16-pipe contractions (include/mintime_hip.h: mt_gemm_set_precision).  Process-wide, read at dispatch time
// by try_launch_split() below and by mt_gemm_planes; MT_MATMUL_PRECISION sets the initial value.
std::atomic<int> g_precision{MT_PRECISION_HIGHEST};
std::once_flag g_precision_once;                  // the environment is read once, by whichever thread asks first
std::atomic<bool> g_precision_env_bad{false};     // an unknown MT_MATMUL_PRECISION, reported by the first mt_gemm_get_precision()
char g_precision_env[64] = {0};                   // (written inside the call_once only)

}  // namespace

namespace mt {
int matmul_precision() {
  std::call_once(g_precision_once, [] {
    const char* e = getenv("MT_MATMUL_PRECISION");
    if (e && !strcmp(e, "high")) g_precision.store(MT_PRECISION_HIGH);
    else if (e && *e && strcmp(e, "highest")) {
      snprintf(g_precision_env, sizeof(g_precision_env), "%s", e);
      g_precision_env_bad.store(true);
    }
  });
  return g_precision.load(std::memory_order_relaxed);
}
}  // namespace mt

extern "C" int mt_gemm_set_precision(int level) {
  if (level != MT_PRECISION_HIGHEST && level != MT_PRECISION_HIGH)
    return fail(MT_ERR_ARG, "mt_gemm_set_precision: unknown level %d (MT_PRECISION_HIGHEST = 0, MT_PRECISION_HIGH = 1)", level);
  (void)matmul_precision();                       // the environment's initial value never overwrites an explicit setting
  return g_precision.exchange(level);
}

extern "C" int mt_gemm_get_precision(void) {
  const int level = matmul_precision();
  if (g_precision_env_bad.exchange(false)) {
    (void)fail(MT_ERR_ARG, "MT_MATMUL_PRECISION=%s is not one of highest, high: keeping highest", g_precision_env);
  }
  return level;
}

extern "C" int mt_gemm_set_split(int on) {
  const int prev = mode();
  g_mode = on != 0;
  return prev;
}

extern "C" int mt_gemm_get_split(void) { return mode(); }

namespace {
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ src, __bf16* __restrict__ planes, int64_t n) {
  const int64_t n8 = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const float4 u = reinterpret_cast<const float4*>(src)[2 * i], v = reinterpret_cast<const float4*>(src)[2 * i + 1];
    const float lo[4] = {u.x, u.y, u.z, u.w}, hi[4] = {v.x, v.y, v.z, v.w};
    bf16x8_t x0, x1, x2;
    split_bf16<true>(lo, hi, x0, x1, x2);
    reinterpret_cast<bf16x8_t*>(planes)[i] = x0;
    reinterpret_cast<bf16x8_t*>(planes + n)[i] = x1;
    reinterpret_cast<bf16x8_t*>(planes + 2 * n)[i] = x2;
  }
}
}  // namespace

extern "C" int mt_split_planes(const float* src, void* planes, int64_t n, void* stream) {
  if (!src || !planes) return fail(MT_ERR_ARG, "mt_split_planes: null pointer");
  if (n <= 0 || (n & 7) || ((uintptr_t)src & 15) || ((uintptr_t)planes & 15))
    return fail(MT_ERR_ARG, "mt_split_planes: n must be a positive multiple of 8, pointers 16-byte aligned");
  const int64_t n8 = n >> 3;
  const unsigned blocks = (unsigned)((n8 + 255) / 256 < 2048 ? (n8 + 255) / 256 : 2048);
  hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, reinterpret_cast<__bf16*>(planes), n);
  return check_launch("mt_split_planes");
}

namespace mt {

// Returns 1 when the problem is not eligible (caller falls back), 0 on success, < 0 on error.
int try_launch_split(const mt_gemm_desc* d, GemmArgs a, hipStream_t s) {
  if (!mode()) return 1;
  if (matmul_precision() == MT_PRECISION_HIGH) return launch_split_high(d, a, s);
  return split_dispatch::launch_split_tier<true>(d, a, s);
}

}  // namespace mt
