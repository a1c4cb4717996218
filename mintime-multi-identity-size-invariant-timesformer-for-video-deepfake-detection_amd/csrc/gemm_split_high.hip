// MT_PRECISION_HIGH instances of the split-operand GEMM loop (gemm_split_dispatch.hpp): three piece products per fp32 product.
#include "gemm_split_dispatch.hpp"

namespace mt {

int launch_split_high(const mt_gemm_desc* d, GemmArgs a, hipStream_t s) { return split_dispatch::launch_split_tier<false>(d, a, s); }

}  // namespace mt
