// Launch of the plane-operand GEMM loop (gemm_planes.hpp), templated on the pieces read per operand so that each arithmetic tier's
// instances compile in a translation unit of their own: NP = 3 in gemm_planes.hip (MT_PRECISION_HIGHEST, six products), NP = 2 in
// gemm_planes_high.hip (MT_PRECISION_HIGH, three products).  mt_gemm_planes prepares the same arguments and grid for both.
#pragma once
#include "../../include/mintime_hip.h"
#include "common.hpp"
#include "gemm_planes.hpp"

// Ring depth of the two-piece loop.  A stage is 16 KB instead of 24 KB, so a ring of three takes the LDS of the six-product loop's ring
// of two (48 KB) and leaves residency where it was.  Measured in-step (profiles/precision_high_step.txt, config 3, B = 32): training step
// 37.01 ms with three stages against 38.14 / 38.26 ms with two, eval forward 11.70 against 12.08 / 12.21 ms.  The persistent form keeps
// its ring of two (gemm_planes.hpp: the next tile's first stage rides in the free slot).  MINW stays: the balanced instances need
// 160-194 VGPRs, a third wave per SIMD would leave 168.
#ifndef MT_PLANES_HIGH_STAGES
#define MT_PLANES_HIGH_STAGES 3
#endif

namespace mt {

template <int NP, bool AKM, bool BKM, int EPI, int BAL, bool CPL, int SK = 0>
int launch_planes(const GemmArgs& a, dim3 grid, hipStream_t s) {
  constexpr int ST = (NP == 2 && SK != 2) ? MT_PLANES_HIGH_STAGES : 2;
  auto k = gemm_planes_kernel<2, 2, 2, 2, AKM, BKM, EPI, ST, BAL == BAL_PAIR ? 2 : 3, BAL, CPL, SK, NP>;
  constexpr size_t lds = (size_t)ST * NP * (128 + 128) * 32;
  {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(k), lds);
    if (e != hipSuccess) return fail(MT_ERR_LAUNCH, "mt_gemm_planes: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
  return check_launch("mt_gemm_planes");
}

// every form mt_gemm_planes reaches.  skm: 0 = one block per tile, 1 = stream-K, 2 = persistent blocks (gemm_planes.hpp SKM)
template <int NP>
int launch_planes_form(int op, int epi, bool cpl, int skm, const GemmArgs& a, dim3 grid, hipStream_t s) {
  if (op == MT_OP_TN && epi == MT_EPI_ATOMIC) return launch_planes<NP, true, true, EPI_ATOMIC, BAL_NONE, false, 0>(a, grid, s);
  if (skm == 2 && !cpl) {
    if (op == MT_OP_NT && epi == MT_EPI_STORE) return launch_planes<NP, false, false, EPI_STORE, BAL_PAIR, false, 2>(a, grid, s);
    if (op == MT_OP_NT && epi == MT_EPI_BIAS_RES) return launch_planes<NP, false, false, EPI_BIAS_RES, BAL_PAIR, false, 2>(a, grid, s);
    if (op == MT_OP_NN && epi == MT_EPI_STORE) return launch_planes<NP, false, true, EPI_STORE, BAL_PAIR, false, 2>(a, grid, s);
  }
  if (skm == 0 || skm == 1) {
#define PL_COMBO(OP, BKM_, EPI_, CPL_)                                                               \
  if (op == OP && epi == EPI_ && cpl == CPL_)                                                        \
    return skm ? launch_planes<NP, false, BKM_, EPI_, BAL_PAIR, CPL_, 1>(a, grid, s)                 \
               : launch_planes<NP, false, BKM_, EPI_, BAL_PAIR, CPL_, 0>(a, grid, s);
    PL_COMBO(MT_OP_NT, false, EPI_STORE, false)
    PL_COMBO(MT_OP_NT, false, EPI_BIAS_RES, false)
    PL_COMBO(MT_OP_NT, false, EPI_STATS, false)
    PL_COMBO(MT_OP_NT, false, EPI_GEGLU, false)
    PL_COMBO(MT_OP_NT, false, EPI_GEGLU, true)
    PL_COMBO(MT_OP_NN, true, EPI_STORE, false)
    PL_COMBO(MT_OP_NN, true, EPI_BIAS_RES, false)
    PL_COMBO(MT_OP_NN, true, EPI_GEGLU_BWD, false)
    PL_COMBO(MT_OP_NN, true, EPI_GEGLU_BWD, true)
#undef PL_COMBO
  }
  return fail(MT_ERR_UNSUPPORTED, "mt_gemm_planes: unsupported op / epilogue %d / %d", op, epi);
}

// gemm_planes_high.hip: launch_planes_form<2>
int launch_planes_high(int op, int epi, bool cpl, int skm, const GemmArgs& a, dim3 grid, hipStream_t s);

}  // namespace mt
