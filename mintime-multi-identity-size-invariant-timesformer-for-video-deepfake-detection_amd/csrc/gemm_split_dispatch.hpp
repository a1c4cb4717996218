// Dispatch of the split-operand GEMM main loop (gemm_split.hpp), templated on the arithmetic tier so that each tier's instances
// compile in a translation unit of their own: X6 = true (gemm_split.hip) accumulates the six leading piece products
// (MT_PRECISION_HIGHEST), X6 = false (gemm_split_high.hip) the three of MT_PRECISION_HIGH, a0 b0 + a0 b1 + a1 b0, from two planes
// per operand.  Same eligibility rules, tiles, grids and split-K ranges for both.
#pragma once
#include "../../include/mintime_hip.h"
#include "common.hpp"
#include "gemm_split.hpp"
#include "gemm_geometry.hpp"
#include "det.hpp"
#include <stdio.h>
#include <string.h>

namespace mt {
namespace split_dispatch {

enum { S_BIG = 0, S_MID = 1, S_COUNT };      // 128 x 128 (4 waves of 64 x 64), 128 x 64 (64 x 32)
struct Var { int bm, bn; };
constexpr Var kVar[S_COUNT] = {{128, 128}, {128, 64}};

template <bool X6, int WM, int WN, int TM, int TN, int AL, int BL, int EPI, int MINW, bool BAL, int PRO = PRO_NONE, bool BPL = false>
int launch_one(const GemmArgs& a, dim3 grid, hipStream_t s) {
  auto k = gemm_split_kernel<WM, WN, TM, TN, AL, BL, EPI, MINW, X6, 2, BAL, PRO, BPL>;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  size_t lds = BPL ? (size_t)(6 * BM + 9 * BN) * 32 : (size_t)2 * (X6 ? 3 : 2) * (BM + BN) * 32;      // two stages of three (two) planes per operand
  if (PRO == PRO_BN_SWISH_GATE) lds += (size_t)(2 + (BM - 1) / a.hw + 2) * a.K * 4;      // scale, shift, gate rows of the images a row tile touches
  if (PRO == PRO_BN_BWD && AL == LAYOUT_KCONTIG) lds += (size_t)3 * a.K * 4;             // ka, kb, kc
  if (lds > 160 * 1024) return 1;      // not this way: the caller falls back to the fp32 kernels
  {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(k), lds);
    if (e != hipSuccess) return fail(MT_ERR_LAUNCH, "mt_gemm(split): cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k, grid, dim3(WM * WN * 64), lds, s, a);
  return check_launch("mt_gemm(split)");
}

template <bool X6, int AL, int BL, int EPI, int PRO = PRO_NONE>
int launch_variant(int v, const GemmArgs& a, dim3 grid, hipStream_t s) {
  // Balanced accumulators (gemm_split.hpp: BAL) wherever a result feeds further contractions (activations, data gradients): the
  // bf16 pipe's rounding bias is only a problem when it adds up coherently through depth.  Weight gradients (TN) are leaves --
  // their error goes no further than lr x bias into the next step's weights -- and take the single-accumulator loop
  // (max / rms error equal to the fp32 pipe's, 6-8 % faster, 146 instead of 206 VGPRs).
  if constexpr (AL == LAYOUT_KMAJOR && BL == LAYOUT_KMAJOR) {
    return v == S_BIG ? launch_one<X6, 2, 2, 2, 2, AL, BL, EPI, 2, false, PRO>(a, grid, s)
                      : launch_one<X6, 2, 2, 2, 1, AL, BL, EPI, 3, false, PRO>(a, grid, s);
  } else {
    // (the B-planes variant is a six-product loop: at tier high the call goes on to the normal instance)
    if constexpr (X6 && AL == LAYOUT_KCONTIG && BL == LAYOUT_KCONTIG && EPI != EPI_STATS && PRO == PRO_NONE) {
      // weight pre-split into bf16 planes (mt_split_planes): B by DMA, 128 x 128 tiles only.  Bit-identical to the in-kernel split.
      // Round 2: 7-12 % slower (hipcc's vmcnt for the staged A tile also drained the DMA of the same step).  Round 3: the A loads
      // are inline asm under one counted wait per step (no compiler-inserted vmcnt left in the loop, checked in the ISA) -- and the
      // variant now runs EQUAL to the in-kernel split, not faster (profiles/r03_split_planes_manual_waits.txt:
      // QKV 154.7 / 153.6 us, FF2 203.8 / 201.2, FF1 data gradient 353.5 / 352.0, 4096^3 747 / 780), with two or with three A
      // register sets in flight: the loop is limited by its matrix + LDS issue, not by operand delivery.  Stays opt-in
      // (MT_SPLIT_PLANES=1; read per call: tests toggle it).
      const bool planes_on = env_int("MT_SPLIT_PLANES", 0) != 0;
      if (planes_on && a.b_planes && (a.K % 16) == 0 && a.k_chunk == 0 && (a.ldb % 8) == 0 && a.b_map.gin == 0 && (v == S_BIG || EPI == EPI_GEGLU_BWD))
        return launch_one<X6, 2, 2, 2, 2, AL, BL, EPI, 2, true, PRO_NONE, true>(a, grid, s);
    }
    if constexpr (EPI != EPI_GEGLU) {      // (GEGLU needs the 128-column tile: launch_split_tier gives it S_BIG)
      if (v == S_MID) return launch_one<X6, 2, 2, 2, 1, AL, BL, EPI, 3, true, PRO>(a, grid, s);
    }
    return launch_one<X6, 2, 2, 2, 2, AL, BL, EPI, 2, true, PRO>(a, grid, s);
  }
}

// The body of try_launch_split() behind its mode check.  Returns 1 when the problem is not eligible (caller falls back), 0 on
// success, < 0 on error.
template <bool X6>
int launch_split_tier(const mt_gemm_desc* d, GemmArgs a, hipStream_t s) {
  if (d->b_prologue != MT_BPRO_NONE) return 1;
  if (d->K % 8 || d->M < 128 || d->N < 64) return 1;     // K % 16 == 8: the last k-tile is half zeros (gemm_split.hpp k_tail)
  if (d->prologue == MT_PRO_BN_SWISH_GATE) {
    // MBConv project convolution (forward): the operand transform rides in the staging registers (gemm_split.hpp PRO)
    if (d->op != MT_OP_NT || d->M < 4096 || d->K < 256 || (d->K % 16)) return 1;
    if (d->epilogue != MT_EPI_STATS && d->epilogue != MT_EPI_STORE) return 1;
    // tile width by padding waste: 128 columns unless 64-wide tiles waste fewer padded columns
    const int pad128 = (d->N + 127) / 128 * 128, pad64 = (d->N + 63) / 64 * 64;
    const int v = pad64 < pad128 ? S_MID : S_BIG;
    const TileGrid tg = tile_grid(d->M, d->N, kVar[v].bm, kVar[v].bn, (int64_t)kVar[v].bn * d->K * 4);
    dim3 grid(tg.grid_x, 1, 1);
    a.group_n = tg.group_n; a.k_chunk = 0; a.trace = nullptr;
    constexpr int KC = LAYOUT_KCONTIG;
    if (d->epilogue == MT_EPI_STATS)
      return v == S_BIG ? launch_one<X6, 2, 2, 2, 2, KC, KC, EPI_STATS, 2, true, PRO_BN_SWISH_GATE>(a, grid, s)
                        : launch_one<X6, 2, 2, 2, 1, KC, KC, EPI_STATS, 3, true, PRO_BN_SWISH_GATE>(a, grid, s);
    return v == S_BIG ? launch_one<X6, 2, 2, 2, 2, KC, KC, EPI_STORE, 2, true, PRO_BN_SWISH_GATE>(a, grid, s)
                      : launch_one<X6, 2, 2, 2, 1, KC, KC, EPI_STORE, 3, true, PRO_BN_SWISH_GATE>(a, grid, s);
  }
  // BatchNorm-backward operand prologue (data gradients NN, weight gradients TN with a plain second operand): VALU work in the
  // staging registers like the split itself.  Long contractions only (the Xception pointwise convolutions, EfficientNet's
  // expand convolutions from stage 5 on and its head; the weight gradients' K is the row count).
  const bool bn_bwd = d->prologue == MT_PRO_BN_BWD;
  if (bn_bwd) {
    static const int on = env_int("MT_SPLIT_BN_BWD", 1);
    if (!on || d->a_map.gin != 0) return 1;
    const bool nn = d->op == MT_OP_NN && (d->epilogue == MT_EPI_STORE || d->epilogue == MT_EPI_BIAS_RES);
    const bool tn = d->op == MT_OP_TN && d->epilogue == MT_EPI_ATOMIC;
    if (!nn && !tn) return 1;
  } else if (d->prologue != MT_PRO_NONE) return 1;
  // short contractions stay on the fp32 pipe: the matrix time they could save is small next to their epilogue, and the bf16 pipe's
  // residual rounding bias (gemm_split.hpp) is then kept out of the extractors' long chains of small-K convolutions
  static const int min_k = env_int("MT_SPLIT_MIN_K", 512);
  if (d->K < min_k) return 1;
  if (d->epilogue == MT_EPI_STATS && d->M < 4096) return 1;
  if (d->epilogue == MT_EPI_GEGLU && (d->n_half & 63)) return 1;
  // a handful of tiles: the fp32 kernels' small tiles fill the chip better -- unless it is a weight gradient over very many rows,
  // whose K-ranges supply the blocks
  if ((int64_t)d->M * d->N < (1 << 18) && !(d->op == MT_OP_TN && d->K >= 8192 && (int64_t)d->M * d->N >= (1 << 15))) return 1;
  // 128 x 128 tiles; 128 x 64 for the GEGLU-backward epilogue and for narrow outputs
  const int v = d->epilogue == MT_EPI_GEGLU_BWD || d->N < 128 ? S_MID : S_BIG;
  const TileGrid tg = tile_grid(d->M, d->N, kVar[v].bm, kVar[v].bn, (int64_t)kVar[v].bn * d->K * 4);
  dim3 grid(tg.grid_x, 1, 1);
  a.group_n = tg.group_n;
  a.k_chunk = 0;
  a.trace = nullptr;
  if (d->op == MT_OP_TN || d->epilogue == MT_EPI_ATOMIC) {
    // blocks per weight-gradient launch.  Round 2: 2048 (16-49 K-ranges, whose fp32-atomic partial sums were as much HBM-side
    // traffic as the operands).  With the K-range-major XCD mapping the step time is flat from 384 to 2048 (53.7-54.2 ms); 640
    // keeps 8-40 ranges: partial-sum traffic 104 -> ~48 MB per launch (family total ~1.45x the algorithmic bytes).
    static const int target = env_int("MT_WGRAD_BLOCKS", 640);   // tuning knob
    static const int xcd_k_on = env_int("MT_WGRAD_XCD_K", 1);
    const bool tn = d->op == MT_OP_TN;
    const bool xcd_k = tn && xcd_k_on && d->split_k <= 0 && d->K >= 8 * 256 && d->a_map.gin == 0 && d->b_map.gin == 0;
    const SplitK sk = split_k_ranges(d->K, tg.m_tiles * tg.n_tiles, d->split_k, tn ? target : 0, 16, xcd_k ? K_XCD_CAPPED : K_PLAIN);
    a.k_chunk = sk.k_chunk;
    a.xcd_k = sk.xcd_k;
    grid.y = sk.grid_y;
    if (xcd_k) {       // one block per tile and range
      a.group_n = 0;
      grid.x = tg.m_tiles * tg.n_tiles;
    }
    if (d->epilogue == MT_EPI_ATOMIC)
      if (int rc = det_gemm_setup(a.C, a.ldc, a.det_slab, d->M, d->N, sk.ranges, a.c_map.gin != 0, s)) return rc;
  }

  if (bn_bwd) {
    if (d->op == MT_OP_TN) return launch_variant<X6, LAYOUT_KMAJOR, LAYOUT_KMAJOR, EPI_ATOMIC, PRO_BN_BWD>(v, a, grid, s);
    if (d->epilogue == MT_EPI_BIAS_RES) return launch_variant<X6, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_BIAS_RES, PRO_BN_BWD>(v, a, grid, s);
    return launch_variant<X6, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_STORE, PRO_BN_BWD>(v, a, grid, s);
  }
#define SPLIT_COMBO(OP, AL, BL, EPI)                                 \
  if (d->op == OP && d->epilogue == EPI) return launch_variant<X6, AL, BL, EPI>(v, a, grid, s);
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_STORE)
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_BIAS_RES)
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_GEGLU)
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_ATOMIC)
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_STATS)
  SPLIT_COMBO(MT_OP_NT, LAYOUT_KCONTIG, LAYOUT_KCONTIG, EPI_GEGLU_BWD)   // data gradient over a transposed weight (tsf_backward.py)
  SPLIT_COMBO(MT_OP_NN, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_STORE)
  SPLIT_COMBO(MT_OP_NN, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_ACCUM)
  SPLIT_COMBO(MT_OP_NN, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_GEGLU_BWD)
  SPLIT_COMBO(MT_OP_NN, LAYOUT_KCONTIG, LAYOUT_KMAJOR, EPI_ATOMIC)
  SPLIT_COMBO(MT_OP_TN, LAYOUT_KMAJOR, LAYOUT_KMAJOR, EPI_ATOMIC)
#undef SPLIT_COMBO
  return 1;
}

}  // namespace split_dispatch

// gemm_split_high.hip: launch_split_tier<false>
int launch_split_high(const mt_gemm_desc* d, GemmArgs a, hipStream_t s);

}  // namespace mt
