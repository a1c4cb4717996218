// MT_PRECISION_HIGH instances of the plane-operand GEMM loop (gemm_planes_launch.hpp): two planes read per operand, three piece
// products per fp32 product.
#include "gemm_planes_launch.hpp"

namespace mt {

int launch_planes_high(int op, int epi, bool cpl, int skm, const GemmArgs& a, dim3 grid, hipStream_t s) {
  return launch_planes_form<2>(op, epi, cpl, skm, a, grid, s);
}

}  // namespace mt
