// The exact fp32 chain as the shortlist kernel (mdx_rescore.hip, rescore_kernel) and the join kernels (mdx_join.hip,
// exact_kernel) run it: rows read in place from row-major memory, k ascending, __builtin_fmaf from +0, continued over zeros to
// round_up(d, 64) as the fp32 MFMA kernels of an index do -- the bits of mdx_scores on an fp32 index of the same rows.  The two
// kernels keep their own tile geometry and share these device functions.
#pragma once
#include "mdx_common.h"

namespace mdx {

typedef float f32x4 __attribute__((ext_vector_type(4)));     // the same types under the same names as in mdx_scores_kernel.h
typedef int i32x4 __attribute__((ext_vector_type(4)));       // and mdx_scores_i8_kernel.h

// floats k .. k + 3 of row `id` of rows [., d] at ld (zeros beyond d; nothing is read for id < 0).  vec: ld % 4 == 0 and a
// 16-byte aligned base, so that a piece inside the row is one 16-byte load
__device__ __forceinline__ f32x4 row_piece(const float *rows, int64_t id, int64_t ld, int64_t d, int64_t k, bool vec)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (id < 0) return v;
    const float *p = rows + id * ld;
    if (vec && k + 4 <= d) return *(const f32x4 *)(p + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k + e < d ? p[k + e] : 0.f;
    return v;
}

// where the chain ends, the stages of kc elements that cover it, and the elements of the stage at k0 (a multiple of 64)
__device__ __forceinline__ int64_t chain_pad(int64_t d) { return (d + 63) / 64 * 64; }
__device__ __forceinline__ int64_t chain_stages(int64_t d_pad, int kc) { return (d_pad + kc - 1) / kc; }
__device__ __forceinline__ int chain_kend(int64_t d_pad, int64_t k0, int kc) { return (int)(d_pad - k0 < kc ? d_pad - k0 : kc); }

// four links of one chain, k ascending: acc + x[0] y[0] + x[1] y[1] + x[2] y[2] + x[3] y[3], one fma each.  The loop over a
// stage stays in each kernel: written once as a function of two LDS rows it changes rescore_kernel's register allocation.
__device__ __forceinline__ float chain_step4(float acc, f32x4 x, f32x4 y)
{
    acc = __builtin_fmaf(x[0], y[0], acc);
    acc = __builtin_fmaf(x[1], y[1], acc);
    acc = __builtin_fmaf(x[2], y[2], acc);
    return __builtin_fmaf(x[3], y[3], acc);
}

// the next fp32 value above a finite x
__device__ __forceinline__ float next_up(float x)
{
    if (x == 0.f) return __uint_as_float(1u);
    const uint32_t u = __float_as_uint(x);
    return __uint_as_float(x > 0.f ? u + 1 : u - 1);
}

// the smallest fp32 value >= v (v >= 0); +inf beyond the range
__device__ __forceinline__ float up_f32(double v)
{
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

}  // namespace mdx
