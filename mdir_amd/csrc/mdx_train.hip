// The trainable descriptor tail (include/mdx_train.h): backward of the global pooling (GeM / MAC / SPoC) and of the row L2
// normalisation, the contrastive and the triplet loss with their gradients.  Everything is a streaming or launch-bound kernel; every
// sum runs in a fixed order (no float atomics), so a call returns the same bits on every run.
//
// Replaces what torch's autograd does for LF.gem / LF.mac / LF.spoc / LF.l2n (mdir/external/cirtorch/layers/functional.py:11-22,
// :130-131) and LF.contrastive_loss / LF.triplet_loss (:141-173) in the reference's training loop (cirtorch/examples/train.py:350-364).
#include <math.h>

#include "mdx_common.h"
#include "mdx_pow.h"

namespace mdx {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// four elements of a plane: a 16-byte access on the 16-byte grid, the same access at dword alignment off it (mdx_pool.hip, pool_wide)
__device__ __forceinline__ float4 load4(const float *p, bool aligned)
{
    if (aligned) return *(const float4 *)p;
    const f32x4u v = *(const f32x4u *)p;
    return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void store4(float *p, bool aligned, float4 v)
{
    if (aligned) {
        *(float4 *)p = v;
    } else {
        f32x4u u;
        u.x = v.x; u.y = v.y; u.z = v.z; u.w = v.w;
        *(f32x4u *)p = u;
    }
}

constexpr float LN2 = 0.69314718055994530942f;

// xc^p and xc^p log2(xc) of one element; x^(p-1) for the gradient
template <int MODE>
__device__ __forceinline__ void gem_terms(float x, float p, float eps, float &xp, float &xpl)
{
    const float xc = x < eps ? eps : x;
    const float l = __builtin_amdgcn_logf(xc);
    xp = MODE == 0 ? __builtin_amdgcn_exp2f(p * l) : pow_pos<MODE>(xc, p);
    xpl = xp * l;
}

template <int MODE>
__device__ __forceinline__ float gem_grad(float x, float pm1, float eps, float coef)
{
    if (x < eps) return 0.0f;                 // the clamp's gradient: 0 below eps, 1 at and above it (x == eps passes)
    if (MODE == 1) return coef;
    return coef * pow_pos<MODE == 0 ? 0 : MODE - 1>(x, pm1);
}

// the better of two (value, index) candidates of the MAC backward: the larger value, on a tie the smaller index
__device__ __forceinline__ void arg_better(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// one wave per (image, channel) plane, as pool_kernel of mdx_pool.hip; `parts` [planes]: the planes' parts of grad_p (GEM)
template <int KIND, int MODE>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float *__restrict__ feat, const float *__restrict__ pooled,
                                                       const float *__restrict__ grad_pooled, int64_t planes, int HW, float p, float eps,
                                                       float *__restrict__ grad_feat, float *__restrict__ parts)
{
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const float *src = feat + plane * HW;
    float *dst = grad_feat + plane * HW;
    const bool wide = (HW & 3) == 0;
    const bool src16 = ((uintptr_t)src & 15) == 0, dst16 = ((uintptr_t)dst & 15) == 0;
    const int n4 = HW >> 2;
    const float g = grad_pooled[plane];

    if (KIND == MDX_POOL_SPOC) {
        const float v = g / (float)HW;
        if (wide) {
            for (int i = lane; i < n4; i += 64) store4(dst + 4 * i, dst16, make_float4(v, v, v, v));
        } else {
            for (int i = lane; i < HW; i += 64) dst[i] = v;
        }
        return;
    }

    if (KIND == MDX_POOL_MAC) {
        // a lane meets its elements in ascending index, so `>` keeps its first maximum; NaN never wins and the index stays inside
        float best = -INFINITY;
        int at = 0x7FFFFFFF;
        if (wide) {
            for (int i = lane; i < n4; i += 64) {
                const float4 v = load4(src + 4 * i, src16);
                if (v.x > best) { best = v.x; at = 4 * i; }
                if (v.y > best) { best = v.y; at = 4 * i + 1; }
                if (v.z > best) { best = v.z; at = 4 * i + 2; }
                if (v.w > best) { best = v.w; at = 4 * i + 3; }
            }
        } else {
            for (int i = lane; i < HW; i += 64) {
                const float v = src[i];
                if (v > best) { best = v; at = i; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) arg_better(best, at, __shfl_xor(best, o, 64), __shfl_xor(at, o, 64));
        if (at >= HW) at = 0;                   // no element compared greater than -inf (a plane of NaN / -inf): element 0
        if (wide) {
            for (int i = lane; i < n4; i += 64)
                store4(dst + 4 * i, dst16, make_float4(at == 4 * i ? g : 0.0f, at == 4 * i + 1 ? g : 0.0f, at == 4 * i + 2 ? g : 0.0f,
                                                       at == 4 * i + 3 ? g : 0.0f));
        } else {
            for (int i = lane; i < HW; i += 64) dst[i] = at == i ? g : 0.0f;
        }
        return;
    }

    // GEM.  Pass 1: s0 = sum xc^p in the forward's order (so m is the forward's mean), s1 = sum xc^p log2 xc
    float s0 = 0.0f, s1 = 0.0f;
    if (wide) {
        for (int i = lane; i < n4; i += 64) {
            const float4 v = load4(src + 4 * i, src16);
            float a, b, c, d, la, lb, lc, ld;
            gem_terms<MODE>(v.x, p, eps, a, la);
            gem_terms<MODE>(v.y, p, eps, b, lb);
            gem_terms<MODE>(v.z, p, eps, c, lc);
            gem_terms<MODE>(v.w, p, eps, d, ld);
            s0 += (a + b) + (c + d);
            s1 += (la + lb) + (lc + ld);
        }
    } else {
        for (int i = lane; i < HW; i += 64) {
            float a, la;
            gem_terms<MODE>(src[i], p, eps, a, la);
            s0 += a;
            s1 += la;
        }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    const float y = pooled[plane];
    const float m = s0 / (float)HW;
    const float ml = s1 * LN2 / (float)HW;                      // mean_hw(xc^p ln xc)
    if (lane == 0) parts[plane] = g * y * (ml / (p * m) - logf(m) / (p * p));
    // y^(1-p): exact forms for the exponents that occur untrained
    const float ypow = MODE == 1 ? 1.0f : MODE == 2 ? 1.0f / y : MODE == 3 ? 1.0f / (y * y) : powf(y, 1.0f - p);
    const float coef = g * ypow / (float)HW;
    const float pm1 = p - 1.0f;
    // pass 2: the plane again (from the cache), the gradient out
    if (wide) {
        for (int i = lane; i < n4; i += 64) {
            const float4 v = load4(src + 4 * i, src16);
            store4(dst + 4 * i, dst16, make_float4(gem_grad<MODE>(v.x, pm1, eps, coef), gem_grad<MODE>(v.y, pm1, eps, coef),
                                                   gem_grad<MODE>(v.z, pm1, eps, coef), gem_grad<MODE>(v.w, pm1, eps, coef)));
        }
    } else {
        for (int i = lane; i < HW; i += 64) dst[i] = gem_grad<MODE>(src[i], pm1, eps, coef);
    }
}

// one workgroup: out[0] = the sum of parts[0 .. n): thread t adds the parts t, t + 1024, ... in that order, the wave a fixed butterfly,
// thread 0 the 16 wave sums in wave order
__global__ __launch_bounds__(1024) void sum_parts_kernel(const float *__restrict__ parts, int64_t n, float *__restrict__ out)
{
    __shared__ float part[16];
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int64_t i = tid; i < n; i += 1024) s += parts[i];
    s = wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += part[w];
        out[0] = tot;
    }
}

// one wave: out[0] = parts[0] + parts[1] + ... in index order (every lane carries the same running sum)
__global__ __launch_bounds__(64) void sum_in_order_kernel(const float *__restrict__ parts, int64_t n, float *__restrict__ out)
{
    const int lane = threadIdx.x;
    float tot = 0.0f;
    for (int64_t base = 0; base < n; base += 64) {
        const float v = base + lane < n ? parts[base + lane] : 0.0f;
        const int count = n - base < 64 ? (int)(n - base) : 64;
        for (int i = 0; i < count; ++i) tot += __shfl(v, i, 64);
    }
    if (lane == 0) out[0] = tot;
}

// sum over the 256 threads of a workgroup in the order of l2n_rows_kernel (mdx_pool.hip); `part` [4] may be reused at once
__device__ __forceinline__ float block_sum(float v, float *part)
{
    v = wave_sum(v);
    __syncthreads();                            // `part` of the previous sum has been read by everybody
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// one workgroup per row
__global__ __launch_bounds__(256) void l2n_rows_bwd_kernel(const float *x, const float *grad_out, int64_t D, float eps, float *grad_x)
{
    __shared__ float part[4];
    const float *row = x + (int64_t)blockIdx.x * D;
    const float *g = grad_out + (int64_t)blockIdx.x * D;
    float *o = grad_x + (int64_t)blockIdx.x * D;
    const int tid = threadIdx.x;
    float ss = 0.0f, dot = 0.0f;
    for (int64_t k = tid; k < D; k += 256) {
        const float v = row[k];
        ss += v * v;
        dot += g[k] * v;
    }
    ss = block_sum(ss, part);
    dot = block_sum(dot, part);
    const float n = sqrtf(ss);
    const float den = n + eps;
    const float c = n > 0.0f ? dot / (n * den * den) : 0.0f;     // the norm's subgradient at 0 is 0
    for (int64_t k = tid; k < D; k += 256) o[k] = g[k] / den - row[k] * c;
}

// x [D, N]: element k of column c is x[k * N + c].  One workgroup per tuple; thread t owns the elements t, t + 256, ... of every
// column, so the query's gradient (in grad_x, read back by the thread that wrote it) accumulates over the pairs in column order
__global__ __launch_bounds__(256) void contrastive_kernel(const float *__restrict__ x, const float *__restrict__ label, int64_t D, int64_t N,
                                                          int64_t S, float margin, float eps, float *__restrict__ grad_x,
                                                          float *__restrict__ parts)
{
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * S;
    float loss = 0.0f;
    for (int64_t k = tid; k < D; k += 256) grad_x[k * N + q] = 0.0f;
    for (int64_t j = 1; j < S; ++j) {
        float ss = 0.0f;
        for (int64_t k = tid; k < D; k += 256) {
            const float d = x[k * N + q] - x[k * N + q + j] + eps;
            ss += d * d;
        }
        const float dist = sqrtf(block_sum(ss, part));
        const float l = label[q + j];
        const float slack = fmaxf(margin - dist, 0.0f);
        loss += 0.5f * l * (dist * dist) + 0.5f * (1.0f - l) * (slack * slack);
        const float coef = l - (1.0f - l) * slack / dist;
        for (int64_t k = tid; k < D; k += 256) {
            const float gr = coef * (x[k * N + q] - x[k * N + q + j] + eps);
            grad_x[k * N + q] += gr;
            grad_x[k * N + q + j] = -gr;
        }
    }
    if (tid == 0) parts[blockIdx.x] = loss;
}

// the same layout; the tuple's positive is its first label-1 column, every label-0 column is a negative
__global__ __launch_bounds__(256) void triplet_kernel(const float *__restrict__ x, const float *__restrict__ label, int64_t D, int64_t N, int64_t S,
                                                      float margin, float *__restrict__ grad_x, float *__restrict__ parts)
{
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * S;
    int64_t pos = 1;
    for (int64_t j = S - 1; j >= 1; --j)
        if (label[q + j] == 1.0f) pos = j;
    float sp = 0.0f;
    for (int64_t k = tid; k < D; k += 256) {
        const float d = x[k * N + q] - x[k * N + q + pos];
        sp += d * d;
        grad_x[k * N + q] = 0.0f;
        grad_x[k * N + q + pos] = 0.0f;
    }
    const float dist_pos = block_sum(sp, part);
    float loss = 0.0f;
    for (int64_t j = 1; j < S; ++j) {
        if (j == pos) continue;
        const bool negative = label[q + j] == 0.0f;                    // (uniform; any other label: no term, gradient 0)
        float sn = 0.0f;
        for (int64_t k = tid; k < D; k += 256) {
            const float d = x[k * N + q] - x[k * N + q + j];
            sn += d * d;
        }
        const float arg = dist_pos - block_sum(sn, part) + margin;
        const bool active = negative && arg >= 0.0f;                    // the clamp passes the gradient at equality
        if (active) loss += arg;
        for (int64_t k = tid; k < D; k += 256) {
            const float xq = x[k * N + q];
            const float gp = 2.0f * (xq - x[k * N + q + pos]), gn = 2.0f * (xq - x[k * N + q + j]);
            if (active) {
                grad_x[k * N + q] += gp - gn;
                grad_x[k * N + q + pos] -= gp;
            }
            grad_x[k * N + q + j] = active ? gn : 0.0f;
        }
    }
    if (tid == 0) parts[blockIdx.x] = loss;
}

template <int KIND>
static void launch_pool_bwd(int mode, const float *feat, const float *pooled, const float *gy, int64_t planes, int HW, float p, float eps,
                            float *gx, float *parts, hipStream_t s)
{
    const dim3 grid((unsigned)ceil_div(planes, 4)), blk(256);
    switch (mode) {
        case 1: hipLaunchKernelGGL((pool_bwd_kernel<KIND, 1>), grid, blk, 0, s, feat, pooled, gy, planes, HW, p, eps, gx, parts); break;
        case 2: hipLaunchKernelGGL((pool_bwd_kernel<KIND, 2>), grid, blk, 0, s, feat, pooled, gy, planes, HW, p, eps, gx, parts); break;
        case 3: hipLaunchKernelGGL((pool_bwd_kernel<KIND, 3>), grid, blk, 0, s, feat, pooled, gy, planes, HW, p, eps, gx, parts); break;
        default: hipLaunchKernelGGL((pool_bwd_kernel<KIND, 0>), grid, blk, 0, s, feat, pooled, gy, planes, HW, p, eps, gx, parts); break;
    }
}

// the checks the two losses share; S out
static int tuple_args(const char *who, const float *x, const float *label, int64_t D, int64_t N, int64_t nq, int64_t min_s, const float *loss,
                      const float *grad_x, void *workspace, int64_t workspace_bytes, int64_t *S)
{
    MDX_CHECK_ARG(x && label && loss && grad_x, "%s: NULL pointer", who);
    MDX_CHECK_ARG(D >= 1 && N >= 1 && nq >= 1, "%s: D=%lld N=%lld nq=%lld must be >= 1", who, (long long)D, (long long)N, (long long)nq);
    MDX_CHECK_ARG(nq < (1ll << 31), "%s: nq=%lld must be < 2^31", who, (long long)nq);
    MDX_CHECK_ARG(N % nq == 0, "%s: N=%lld is not a multiple of nq=%lld", who, (long long)N, (long long)nq);
    *S = N / nq;
    MDX_CHECK_ARG(*S >= min_s, "%s: tuples of S=%lld columns, at least %lld needed", who, (long long)*S, (long long)min_s);
    MDX_CHECK_ARG(D <= INT64_MAX / N, "%s: D * N overflows", who);
    MDX_CHECK_WORKSPACE(who, workspace, workspace_bytes, mdx_tuple_loss_workspace(nq));
    return MDX_OK;
}

}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_pool_bwd_workspace(int B, int C)
{
    if (B <= 0 || C <= 0) return 0;
    return round_up((int64_t)B * C * 4, 256);
}

int mdx_pool_bwd(const float *feat, const float *pooled, const float *grad_pooled, int B, int C, int H, int W, int kind, float p,
                 float pool_eps, float *grad_feat, float *grad_p, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(feat && pooled && grad_pooled && grad_feat, "mdx_pool_bwd: NULL pointer");
    MDX_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "mdx_pool_bwd: bad shape [%d,%d,%d,%d]", B, C, H, W);
    MDX_CHECK_ARG((int64_t)H * W < (1ll << 31), "mdx_pool_bwd: H*W too large");
    const int64_t planes = (int64_t)B * C;
    const int HW = H * W;
    const uintptr_t f0 = (uintptr_t)feat, g0 = (uintptr_t)grad_feat, bytes = (uintptr_t)planes * HW * 4;
    MDX_CHECK_ARG(f0 + bytes <= g0 || g0 + bytes <= f0, "mdx_pool_bwd: grad_feat overlaps feat");
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case MDX_POOL_GEM: {
            MDX_CHECK_ARG(p > 0.0f && pool_eps > 0.0f, "mdx_pool_bwd: gem needs p > 0 and eps > 0");
            MDX_CHECK_ARG(grad_p, "mdx_pool_bwd: NULL pointer (grad_p)");
            MDX_CHECK_WORKSPACE("mdx_pool_bwd", workspace, workspace_bytes, mdx_pool_bwd_workspace(B, C));
            const int mode = p == 1.0f ? 1 : p == 2.0f ? 2 : p == 3.0f ? 3 : 0;
            launch_pool_bwd<MDX_POOL_GEM>(mode, feat, pooled, grad_pooled, planes, HW, p, pool_eps, grad_feat, (float *)workspace, s);
            hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(1024), 0, s, (const float *)workspace, planes, grad_p);
            break;
        }
        case MDX_POOL_MAC: launch_pool_bwd<MDX_POOL_MAC>(1, feat, pooled, grad_pooled, planes, HW, 1.0f, 0.0f, grad_feat, nullptr, s); break;
        case MDX_POOL_SPOC: launch_pool_bwd<MDX_POOL_SPOC>(1, feat, pooled, grad_pooled, planes, HW, 1.0f, 0.0f, grad_feat, nullptr, s); break;
        default: MDX_CHECK_ARG(false, "mdx_pool_bwd: unknown pooling kind %d", kind);
    }
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_l2n_rows_bwd(const float *x, const float *grad_out, int64_t R, int64_t D, float eps, float *grad_x, void *stream)
{
    MDX_CHECK_ARG(x && grad_out && grad_x, "mdx_l2n_rows_bwd: NULL pointer");
    MDX_CHECK_ARG(R > 0 && D > 0 && R < (1ll << 31), "mdx_l2n_rows_bwd: R=%lld D=%lld", (long long)R, (long long)D);
    MDX_CHECK_ARG(eps >= 0.0f, "mdx_l2n_rows_bwd: eps=%g", (double)eps);
    hipLaunchKernelGGL(l2n_rows_bwd_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, x, grad_out, D, eps, grad_x);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_tuple_loss_workspace(int64_t nq)
{
    if (nq < 1 || nq >= (1ll << 31)) return 0;
    return round_up(nq * 4, 256);
}

int mdx_contrastive_loss(const float *x, const float *label, int64_t D, int64_t N, int64_t nq, float margin, float eps, float *loss,
                         float *grad_x, void *workspace, int64_t workspace_bytes, void *stream)
{
    int64_t S;
    const int rc = tuple_args("mdx_contrastive_loss", x, label, D, N, nq, 2, loss, grad_x, workspace, workspace_bytes, &S);
    if (rc != MDX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(contrastive_kernel, dim3((unsigned)nq), dim3(256), 0, s, x, label, D, N, S, margin, eps, grad_x, (float *)workspace);
    hipLaunchKernelGGL(sum_in_order_kernel, dim3(1), dim3(64), 0, s, (const float *)workspace, nq, loss);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_triplet_loss(const float *x, const float *label, int64_t D, int64_t N, int64_t nq, float margin, float *loss, float *grad_x,
                     void *workspace, int64_t workspace_bytes, void *stream)
{
    int64_t S;
    const int rc = tuple_args("mdx_triplet_loss", x, label, D, N, nq, 3, loss, grad_x, workspace, workspace_bytes, &S);
    if (rc != MDX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(triplet_kernel, dim3((unsigned)nq), dim3(256), 0, s, x, label, D, N, S, margin, grad_x, (float *)workspace);
    hipLaunchKernelGGL(sum_in_order_kernel, dim3(1), dim3(64), 0, s, (const float *)workspace, nq, loss);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
