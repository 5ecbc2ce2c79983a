// U-Net epilogue (include/mdx_unet.h): conv bias / inference batch-norm + ReLU / LeakyReLU of a convolution output in one pass, written
// into a channel slice of a wider tensor -- the half of a skip connection's concat buffer the producer owns -- so that no torch.cat
// runs.  mdx_bn_act's structure (mdx_trunk.hip): one workgroup per run of one (image, channel) plane, the per-channel constants
// computed once per plane, 16-byte accesses where the planes allow them.  HBM-bound: one read and one write per element.
#include "mdx_common.h"

namespace mdx {

struct IntoArgs {
    const float *mean, *var, *weight, *bias;
    float eps, slope;
};

constexpr int INTO_UNR = 4;

struct alignas(16) IntoPack { float e[4]; };

template <int ACT> __device__ __forceinline__ float into_elem(float v, float mean, float scale, float shift, float slope)
{
    const float y = fmaf(v - mean, scale, shift);
    if (ACT == MDX_ACT_RELU) return y < 0.0f ? 0.0f : y;          // NaN and -0 pass
    if (ACT == MDX_ACT_LEAKY) return y > 0.0f ? y : y * slope;    // NaN takes the product: NaN
    return y;
}

// x and out are NOT __restrict__: out == x is the in-place form.  A thread loads all of its elements before its first store and
// no other thread touches them, so the in-place form reads nothing that was already written.
template <bool VECTOR, int ACT>
__global__ __launch_bounds__(256) void bn_act_into_kernel(const float *x, float *out, int64_t plane0, unsigned hw_vec, unsigned C,
                                                          int64_t hw, int64_t out_batch_stride, IntoArgs a)
{
    const int64_t plane = plane0 + blockIdx.y;
    const int64_t n = plane / C;
    const int c = (int)(plane - n * C);
    const float mean = a.mean ? a.mean[c] : 0.0f;
    const float invstd = a.var ? 1.0f / sqrtf(a.var[c] + a.eps) : 1.0f;
    const float scale = a.weight ? invstd * a.weight[c] : invstd;
    const float shift = a.bias ? a.bias[c] : 0.0f;
    const float *src = x + plane * hw;
    float *dst = out + n * out_batch_stride + (int64_t)c * hw;
    const unsigned i0 = blockIdx.x * (256 * INTO_UNR) + threadIdx.x;
    if (VECTOR) {
        IntoPack v[INTO_UNR];
#pragma unroll
        for (int u = 0; u < INTO_UNR; ++u) {
            const unsigned i = i0 + u * 256;
            if (i < hw_vec) v[u] = ((const IntoPack *)src)[i];
        }
#pragma unroll
        for (int u = 0; u < INTO_UNR; ++u) {
            const unsigned i = i0 + u * 256;
            if (i >= hw_vec) continue;
            IntoPack o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o.e[e] = into_elem<ACT>(v[u].e[e], mean, scale, shift, a.slope);
            ((IntoPack *)dst)[i] = o;
        }
    } else {
        float v[INTO_UNR];
#pragma unroll
        for (int u = 0; u < INTO_UNR; ++u) {
            const unsigned i = i0 + u * 256;
            if (i < hw_vec) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < INTO_UNR; ++u) {
            const unsigned i = i0 + u * 256;
            if (i < hw_vec) dst[i] = into_elem<ACT>(v[u], mean, scale, shift, a.slope);
        }
    }
}

template <bool VECTOR>
static void launch_bn_act_into(const float *x, float *out, int64_t planes, unsigned hw_vec, unsigned C, int64_t hw,
                               int64_t out_batch_stride, const IntoArgs &a, int act, hipStream_t s)
{
    const unsigned gx = (unsigned)ceil_div((int64_t)hw_vec, (int64_t)(256 * INTO_UNR));
    for (int64_t p0 = 0; p0 < planes; p0 += 65535) {
        const unsigned gy = (unsigned)((planes - p0) < 65535 ? (planes - p0) : 65535);
        const dim3 grid(gx, gy);
        if (act == MDX_ACT_RELU)
            hipLaunchKernelGGL((bn_act_into_kernel<VECTOR, MDX_ACT_RELU>), grid, dim3(256), 0, s, x, out, p0, hw_vec, C, hw, out_batch_stride, a);
        else if (act == MDX_ACT_LEAKY)
            hipLaunchKernelGGL((bn_act_into_kernel<VECTOR, MDX_ACT_LEAKY>), grid, dim3(256), 0, s, x, out, p0, hw_vec, C, hw, out_batch_stride, a);
        else
            hipLaunchKernelGGL((bn_act_into_kernel<VECTOR, MDX_ACT_NONE>), grid, dim3(256), 0, s, x, out, p0, hw_vec, C, hw, out_batch_stride, a);
    }
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_bn_act_into(const float *x, float *out, int64_t N, int64_t C, int64_t HW, int64_t out_batch_stride, const float *mean,
                               const float *var, const float *weight, const float *bias, float eps, int act, float slope, void *stream)
{
    const char *who = "mdx_bn_act_into";
    MDX_CHECK_ARG(x && out, "%s: NULL x or out", who);
    MDX_CHECK_ARG((mean == nullptr) == (var == nullptr), "%s: mean and var must both be given or both be NULL", who);
    MDX_CHECK_ARG(N > 0 && C > 0 && HW > 0, "%s: N=%lld C=%lld HW=%lld must be positive", who, (long long)N, (long long)C, (long long)HW);
    MDX_CHECK_ARG(C < (1ll << 31) && HW < (1ll << 31), "%s: C or HW too large", who);
    MDX_CHECK_ARG(eps >= 0.0f, "%s: eps=%g must be >= 0", who, (double)eps);
    MDX_CHECK_ARG(act == MDX_ACT_NONE || act == MDX_ACT_RELU || act == MDX_ACT_LEAKY, "%s: act=%d (0 none, 1 ReLU, 2 LeakyReLU)", who, act);
    MDX_CHECK_ARG(act != MDX_ACT_LEAKY || (slope - slope == 0.0f), "%s: slope=%g must be finite", who, (double)slope);
    const int64_t slice = C * HW;
    MDX_CHECK_ARG(out_batch_stride >= slice, "%s: out_batch_stride=%lld is below C*HW=%lld", who, (long long)out_batch_stride,
                  (long long)slice);
    // the extents below are products: N * out_batch_stride <= 2^60 elements keeps them, in bytes, inside int64 / uintptr_t
    MDX_CHECK_ARG(N <= ((int64_t)1 << 60) / out_batch_stride, "%s: N=%lld images of out_batch_stride=%lld are too large", who,
                  (long long)N, (long long)out_batch_stride);
    const bool in_place = (const float *)out == x && out_batch_stride == slice;
    if (!in_place) {
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)(N * slice) * sizeof(float);
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((N - 1) * out_batch_stride + slice) * sizeof(float);
        MDX_CHECK_ARG(x1 <= o0 || o1 <= x0, "%s: x and out overlap (only out == x with out_batch_stride == C*HW may)", who);
    }
    const IntoArgs a{mean, var, weight, bias, eps, act == MDX_ACT_LEAKY ? slope : 0.0f};
    const bool vec = (HW % 4 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)out & 15) == 0) && (N == 1 || out_batch_stride % 4 == 0);
    if (vec) launch_bn_act_into<true>(x, out, N * C, (unsigned)(HW / 4), (unsigned)C, HW, out_batch_stride, a, act, (hipStream_t)stream);
    else     launch_bn_act_into<false>(x, out, N * C, (unsigned)HW, (unsigned)C, HW, out_batch_stride, a, act, (hipStream_t)stream);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}
