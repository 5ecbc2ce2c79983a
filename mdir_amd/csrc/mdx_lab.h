// The RGB <-> Lab device code shared by the photometric pre-processing kernels (mdx_clahe.hip, mdx_photometric.hip): OpenCV 4's
// RGB2Lab_f / Lab2RGB_f (color_lab.cpp; sRGB gamma, D65) restated with exact transfer functions where OpenCV interpolates spline
// tables, and the reference's round trip through its normalised space (functional.py:24-48).  PARITY UNPINNED against OpenCV
// itself; pinned against oracle.rgb_to_lab / oracle.lab_to_rgb, the same restatement in numpy.
#pragma once
#include "mdx_common.h"

// Every product and sum below is rounded on its own, as in OpenCV's scalar code (and in the numpy restatement): hipcc's
// default contraction would fuse a*b + c*d into an fma and move the interpolation's exact .5 ties (HIP's __fmul_rn /
// __fadd_rn are plain operators inlined from a header compiled WITH contraction, so they do not stop it: the helpers below do).
// The pragma is this header's own: whoever includes it gets the helpers compiled without contraction, whatever its own setting.
#pragma clang fp contract(off)

namespace mdx {

// defined HERE, under the pragma (the HIP header versions are inlined with the contraction flags of their own scope)
__device__ __forceinline__ float mul_(float a, float b) { return a * b; }
__device__ __forceinline__ float add_(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_(float a, float b) { return a - b; }
__device__ __forceinline__ float div_(float a, float b) { return a / b; }

struct Lab { float L, a, b; };

__device__ __forceinline__ float srgb_to_linear(float c)
{
    return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + (float)(16.0 / 116.0); }

// RGB2Lab_f with the sRGB -> linear step looked up (lin[v] = srgb_to_linear(v / 255), the same call on the same 256 inputs)
__device__ __forceinline__ Lab rgb8_to_lab_lut(const float *lin, uint8_t r8, uint8_t g8, uint8_t b8)
{
    const float r = lin[r8], g = lin[g8], b = lin[b8];
    constexpr float m00 = (float)(0.412453 / 0.950456), m01 = (float)(0.357580 / 0.950456), m02 = (float)(0.180423 / 0.950456);
    constexpr float m10 = 0.212671f, m11 = 0.715160f, m12 = 0.072169f;
    constexpr float m20 = (float)(0.019334 / 1.088754), m21 = (float)(0.119193 / 1.088754), m22 = (float)(0.950227 / 1.088754);
    const float x = add_(add_(mul_(r, m00), mul_(g, m01)), mul_(b, m02));
    const float y = add_(add_(mul_(r, m10), mul_(g, m11)), mul_(b, m12));
    const float z = add_(add_(mul_(r, m20), mul_(g, m21)), mul_(b, m22));
    const float fx = lab_f(x), fy = lab_f(y), fz = lab_f(z);
    Lab o;
    o.L = y > 0.008856f ? sub_(mul_(116.0f, fy), 16.0f) : mul_(903.3f, y);
    o.a = mul_(500.0f, sub_(fx, fy));
    o.b = mul_(200.0f, sub_(fy, fz));
    return o;
}

struct LabNorm { float mean[3], std[3]; };

// linear -> sRGB on the OUTPUT side: c^(1/2.4) through the hardware's exp2 / log2 (a few ulp; nothing is truncated after it --
// the value goes straight into (x - mean) / std -- and OpenCV itself interpolates a spline table here).  The INPUT side keeps
// powf: its result is truncated to the uint8 lightness CLAHE sees, and it is evaluated 256 times per workgroup, not per pixel.
__device__ __forceinline__ float linear_to_srgb_fast(float c)
{
    return c <= 0.0031308f ? c * 12.92f : 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(c) * (float)(1.0 / 2.4)) - 0.055f;
}

// one pixel with its new lightness L (already back on the 0..100 scale): the chroma's round trip, Lab -> RGB -> (x - mean) / std
__device__ __forceinline__ void lab_finish_pixel(float L, float2 chroma, const LabNorm &nrm, float (&o)[3])
{
    // back through the reference's normalised space: spc = (lab + [0,128,128]) / [100,255,255]; spc[0] = the new lightness;
    // lab' = spc * [100,255,255] - [0,128,128]   (float32 steps as written there)
    const float a = sub_(mul_(div_(add_(chroma.x, 128.0f), 255.0f), 255.0f), 128.0f);
    const float b = sub_(mul_(div_(add_(chroma.y, 128.0f), 255.0f), 255.0f), 128.0f);
    // Lab2RGB_f
    constexpr float lthresh = (float)(0.008856 * 903.3), fthresh = (float)(7.787 * 0.008856 + 16.0 / 116.0);
    float fy, yy;
    if (L <= lthresh) {
        yy = div_(L, 903.3f);
        fy = add_(mul_(7.787f, yy), (float)(16.0 / 116.0));
    } else {
        fy = div_(add_(L, 16.0f), 116.0f);
        yy = mul_(mul_(fy, fy), fy);
    }
    const float fx = add_(div_(a, 500.0f), fy), fz = sub_(fy, div_(b, 200.0f));
    const float xx = fx <= fthresh ? div_(sub_(fx, (float)(16.0 / 116.0)), 7.787f) : mul_(mul_(fx, fx), fx);
    const float zz = fz <= fthresh ? div_(sub_(fz, (float)(16.0 / 116.0)), 7.787f) : mul_(mul_(fz, fz), fz);
    constexpr float k00 = (float)(3.240479 * 0.950456), k01 = -1.53715f, k02 = (float)(-0.498535 * 1.088754);
    constexpr float k10 = (float)(-0.969256 * 0.950456), k11 = 1.875991f, k12 = (float)(0.041556 * 1.088754);
    constexpr float k20 = (float)(0.055648 * 0.950456), k21 = -0.204043f, k22 = (float)(1.057311 * 1.088754);
    float c[3];
    c[0] = add_(add_(mul_(xx, k00), mul_(yy, k01)), mul_(zz, k02));
    c[1] = add_(add_(mul_(xx, k10), mul_(yy, k11)), mul_(zz, k12));
    c[2] = add_(add_(mul_(xx, k20), mul_(yy, k21)), mul_(zz, k22));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float s = linear_to_srgb_fast(fminf(fmaxf(c[ch], 0.0f), 1.0f));
        o[ch] = div_(sub_(s, nrm.mean[ch]), nrm.std[ch]);         // totensor (no scaling of a float image) | normalize
    }
}

}  // namespace mdx
