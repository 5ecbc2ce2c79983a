// x^p of the GeM pooling, shared by its forward (mdx_pool.hip) and its backward (mdx_train.hip).
#pragma once
#include "mdx_common.h"

namespace mdx {

// x^p for x >= eps > 0.  Exact products for the exponents that occur untrained
// (p = 1, 2, 3, layers/pooling.py:38); exp2(p*log2 x) through the hardware
// transcendental units otherwise (relative error ~1e-6; tests/test_gpu_kernels.py::test_pool_l2n_golden, rtol 1e-5).
template <int MODE>
__device__ __forceinline__ float pow_pos(float x, float p)
{
    if (MODE == 1) return x;
    if (MODE == 2) return x * x;
    if (MODE == 3) return x * x * x;
    return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x));
}

}  // namespace mdx
