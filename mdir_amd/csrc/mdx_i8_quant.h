// The MDX_I8 quantisation of one fp32 row (include/mdx.h states it) as every kernel that makes codes evaluates it: the index build
// and mdx_quantize_i8 (mdx_retile_kernel.h) and the list storage of the inverted file (mdx_lists_i8.hip).  One definition, so the
// codes and scales of one row are the same bits wherever they are made.
#pragma once
#include "mdx_common.h"

namespace mdx {

constexpr int64_t I8_MAX_DPAD = 133120;        // largest multiple of 64 with 127^2 * d_pad < 2^31 (exact int32 accumulation)

__device__ __forceinline__ float i8_inv(float a) { return __fdiv_rn(127.0f, a); }
__device__ __forceinline__ float i8_scale(float a) { return __fdiv_rn(a, 127.0f); }
__device__ __forceinline__ uint32_t i8_code(float x, float a, float inv)      // the code's byte
{
    if (a == 0.f) return 0u;
    const float y = fminf(fmaxf(rintf(__fmul_rn(x, inv)), -127.f), 127.f);
    return (uint32_t)(uint8_t)(int8_t)(int)y;
}

}  // namespace mdx
