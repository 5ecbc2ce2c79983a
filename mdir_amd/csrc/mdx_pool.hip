// Descriptor tail: global pooling (GeM / MAC / SPoC), L2 normalisation, multi-scale
// aggregation.  All HBM- (really launch-) bound streaming reductions: one wave per
// (image, channel) plane with 16-B loads, wavefront shuffles for the reduction.
//
// Replaces LF.gem / LF.mac / LF.spoc / LF.l2n (mdir/external/cirtorch/layers/
// functional.py:11-22,130-131) as used by ImageRetrievalNet.forward
// (cirtorch/networks/imageretrievalnet.py:108-112) and
// CirMultiscaleAggregation.aggregate_tensor (mdir/components/data/wrapper.py:109-119).
#include <math.h>

#include <hip/hip_fp16.h>

#include "mdx_common.h"
#include "mdx_pow.h"

namespace mdx {

// (pow_pos, the x^p of GeM: mdx_pow.h, shared with the backward in mdx_train.hip)

template <int KIND, int MODE>
__device__ __forceinline__ float pool_elem(float x, float p, float eps)
{
    if (KIND == MDX_POOL_GEM) return pow_pos<MODE>(x < eps ? eps : x, p);       // `clamp(min=eps)`: a NaN stays NaN (fmaxf would return eps)
    return x;
}

// The maximum keeps NaN out (fmaxf returns the operand that is a number) where the reference's max pooling returns NaN for a
// plane that holds one: a lane remembers that it saw a NaN, the wave ORs the flags at the end (include/mdx.h, "Non-finite
// values").
__device__ __forceinline__ float max_or_nan(float wave_maximum, bool lane_saw_nan)
{
    return __any(lane_saw_nan) ? __builtin_nanf("") : wave_maximum;
}

// a lane's part of a plane read in pieces of four elements (16 bytes of fp32, 8 of fp16; a half converts exactly): the order
// of the sum is the same for every vector type, so fp16 maps pool to the bits of their fp32 copies (mdx_pool_l2n_f16)
template <int KIND, int MODE, typename V4, typename T>
__device__ __forceinline__ float pool_pieces(const T *__restrict__ src, int HW, float p, float eps, int lane, float acc,
                                             bool &saw_nan)
{
    const V4 *s4 = (const V4 *)src;
    const int n4 = HW >> 2;
    for (int i = lane; i < n4; i += 64) {
        const V4 v = s4[i];
        const float a = pool_elem<KIND, MODE>((float)v.x, p, eps), b = pool_elem<KIND, MODE>((float)v.y, p, eps);
        const float c = pool_elem<KIND, MODE>((float)v.z, p, eps), d = pool_elem<KIND, MODE>((float)v.w, p, eps);
        if (KIND == MDX_POOL_MAC) {
            acc = fmaxf(acc, fmaxf(fmaxf(a, b), fmaxf(c, d)));
            saw_nan |= (a != a) | (b != b) | (c != c) | (d != d);
        } else {
            acc += (a + b) + (c + d);
        }
    }
    return acc;
}

// the four-element pieces of a wide plane: fp32 in 16-byte loads (at dword alignment off the 16-byte grid), fp16 in 8-byte
// loads (at 2-byte alignment off the 8-byte grid)
template <int KIND, int MODE>
__device__ __forceinline__ float pool_wide(const float *__restrict__ src, int HW, float p, float eps, int lane, float acc, bool &saw_nan)
{
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
    if (((uintptr_t)src & 15) == 0) return pool_pieces<KIND, MODE, float4>(src, HW, p, eps, lane, acc, saw_nan);
    return pool_pieces<KIND, MODE, f32x4u>(src, HW, p, eps, lane, acc, saw_nan);
}

template <int KIND, int MODE>
__device__ __forceinline__ float pool_wide(const __half *__restrict__ src, int HW, float p, float eps, int lane, float acc, bool &saw_nan)
{
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4), aligned(8)));
    typedef _Float16 f16x4u __attribute__((ext_vector_type(4), aligned(2)));
    if (((uintptr_t)src & 7) == 0) return pool_pieces<KIND, MODE, f16x4>(src, HW, p, eps, lane, acc, saw_nan);
    return pool_pieces<KIND, MODE, f16x4u>(src, HW, p, eps, lane, acc, saw_nan);
}

__device__ __forceinline__ float pool_load(float v) { return v; }
__device__ __forceinline__ float pool_load(__half v) { return __half2float(v); }

// one wave reduces one (image, channel) plane; every lane returns the pooled value
template <int KIND, int MODE, typename T>
__device__ __forceinline__ float pool_plane(const T *__restrict__ src, bool wide, int HW, float p, float inv_p, float eps,
                                            int lane)
{
    float acc = KIND == MDX_POOL_MAC ? -INFINITY : 0.0f;
    bool saw_nan = false;
    if (wide) {
        // H*W % 4 == 0.  The plane of a sliced feature map starts at any multiple of its element size; the summation order
        // (hence every bit of the result) must not depend on where the caller's tensor lies, so a plane off the grid of
        // its loads is read in the same pieces through the same loads at element alignment
        acc = pool_wide<KIND, MODE>(src, HW, p, eps, lane, acc, saw_nan);
    } else {
        for (int i = lane; i < HW; i += 64) {
            const float a = pool_elem<KIND, MODE>(pool_load(src[i]), p, eps);
            if (KIND == MDX_POOL_MAC) {
                acc = fmaxf(acc, a);
                saw_nan |= a != a;
            } else {
                acc += a;
            }
        }
    }
    acc = KIND == MDX_POOL_MAC ? max_or_nan(wave_max(acc), saw_nan) : wave_sum(acc);
    float r = acc;
    if (KIND != MDX_POOL_MAC) r = acc / (float)HW;
    if (KIND == MDX_POOL_GEM && MODE != 1) r = powf(r, inv_p);
    return r;
}

template <int KIND, int MODE, typename T>
__global__ __launch_bounds__(256) void pool_kernel(const T *__restrict__ feat, int64_t planes,
                                                   int HW, float p, float inv_p, float eps,
                                                   float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const bool wide = (HW & 3) == 0;
    const float r = pool_plane<KIND, MODE>(feat + plane * HW, wide, HW, p, inv_p, eps, lane);
    if (lane == 0) out[plane] = r;
}

// The S feature maps of an image pyramid ([B,C,H_s,W_s] each) pooled by ONE launch: plane index -> (scale, image,
// channel); out [S,B,C].  Same per-plane arithmetic as pool_kernel.
template <typename T>
struct PoolMaps {
    const T *feat[8];
    int hw[8];
    int64_t first[9];           // first plane of scale s; first[S] = all planes
};

template <int KIND, int MODE, typename T>
__global__ __launch_bounds__(256) void pool_multi_kernel(PoolMaps<T> maps, int S, float p, float inv_p, float eps,
                                                         float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= maps.first[S]) return;
    int s = 0;
    while (s + 1 < S && plane >= maps.first[s + 1]) ++s;
    const T *feat = maps.feat[s];
    const int HW = maps.hw[s];
    const bool wide = (HW & 3) == 0;
    const float r = pool_plane<KIND, MODE>(feat + (plane - maps.first[s]) * HW, wide, HW, p, inv_p, eps, lane);
    if (lane == 0) out[plane] = r;
}

// (A single-launch form of pool + L2N -- the workgroup that finishes an image last normalises it, hand-off through
// write-through stores, an arrival ticket and an agent-scope acquire -- was built, is bit-identical, and is SLOWER:
// 29 us against 12 us (batch 1) / 20 us (batch 4) for these two launches on a 2048 x 24 x 32 map:
// the hand-off through memory costs more than the kernel boundary it removes, as the MI355X
// guide's section 5.6 predicts.  In the history: git show 47a9fe2:tools/attic/pool_l2n_fused.hip.)

// one workgroup per row: x = (x + bias) / (||x + bias|| + eps)
__global__ __launch_bounds__(256) void l2n_rows_kernel(float *__restrict__ x, int64_t D,
                                                       const float *__restrict__ bias, float eps)
{
    __shared__ float part[4];
    float *row = x + (int64_t)blockIdx.x * D;
    const int tid = threadIdx.x;
    float ss = 0.0f;
    for (int64_t k = tid; k < D; k += 256) {
        float v = row[k];
        if (bias) v += bias[k];
        ss += v * v;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    const float den = sqrtf((part[0] + part[1]) + (part[2] + part[3])) + eps;
    for (int64_t k = tid; k < D; k += 256) {
        float v = row[k];
        if (bias) v += bias[k];
        row[k] = v / den;
    }
}

struct ScalePtrs { const float *p[8]; };

// single workgroup: power mean over scales, then plain L2 normalisation (no eps)
__global__ __launch_bounds__(1024) void ms_aggregate_kernel(ScalePtrs sp, int S, int64_t D, float msp,
                                                            float inv_msp, float *__restrict__ out)
{
    __shared__ float part[16];
    const int tid = threadIdx.x;
    float ss = 0.0f;
    for (int64_t k = tid; k < D; k += 1024) {
        float a = 0.0f;
        for (int s = 0; s < S; ++s) a += (msp == 1.0f) ? sp.p[s][k] : powf(sp.p[s][k], msp);
        a = a / (float)S;
        if (msp != 1.0f) a = powf(a, inv_msp);
        out[k] = a;
        ss += a * a;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += part[w];
    const float nrm = sqrtf(tot);
    for (int64_t k = tid; k < D; k += 1024) out[k] = out[k] / nrm;
}

// batched form: scale s is a [B,D] row-major matrix; one workgroup per image
__global__ __launch_bounds__(1024) void ms_aggregate_batch_kernel(ScalePtrs sp, int S, int64_t D, float msp, float inv_msp,
                                                                  float *__restrict__ out)
{
    __shared__ float part[16];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float *dst = out + b * D;
    float ss = 0.0f;
    for (int64_t k = tid; k < D; k += 1024) {
        float a = 0.0f;
        for (int s = 0; s < S; ++s) a += (msp == 1.0f) ? sp.p[s][b * D + k] : powf(sp.p[s][b * D + k], msp);
        a = a / (float)S;
        if (msp != 1.0f) a = powf(a, inv_msp);
        dst[k] = a;
        ss += a * a;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += part[w];
    const float nrm = sqrtf(tot);
    for (int64_t k = tid; k < D; k += 1024) dst[k] = dst[k] / nrm;
}

// pooled [S,B,D] -> out [B,D]: L2N of every scale's row (eps added to the norm), power mean over the scales, plain
// renormalisation -- l2n_rows_kernel x S and ms_aggregate_batch_kernel in one launch, one workgroup per image.  The
// sums run in the order of those two kernels (the norms over 256 threads, the rest over 1024), so the result is
// bit-identical to the separate launches.
__global__ __launch_bounds__(1024) void l2n_aggregate_kernel(const float *__restrict__ pooled, int S, int64_t B, int64_t D,
                                                             float eps, float msp, float inv_msp, float *__restrict__ out)
{
    __shared__ float npart[8][4];
    __shared__ float part[16];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < 256) {
        for (int s = 0; s < S; ++s) {
            const float *row = pooled + ((int64_t)s * B + b) * D;
            float ss = 0.0f;
            for (int64_t k = tid; k < D; k += 256) {
                const float v = row[k];
                ss += v * v;
            }
            ss = wave_sum(ss);
            if ((tid & 63) == 0) npart[s][tid >> 6] = ss;
        }
    }
    __syncthreads();
    float den[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
        den[s] = s < S ? sqrtf((npart[s][0] + npart[s][1]) + (npart[s][2] + npart[s][3])) + eps : 1.0f;
    float *dst = out + b * D;
    float ss = 0.0f;
    for (int64_t k = tid; k < D; k += 1024) {
        float a = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (s < S) {
                const float v = pooled[((int64_t)s * B + b) * D + k] / den[s];
                a += (msp == 1.0f) ? v : powf(v, msp);
            }
        a = a / (float)S;
        if (msp != 1.0f) a = powf(a, inv_msp);
        dst[k] = a;
        ss += a * a;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += part[w];
    const float nrm = sqrtf(tot);
    for (int64_t k = tid; k < D; k += 1024) dst[k] = dst[k] / nrm;
}

template <int KIND, typename T>
static void launch_pool_multi(int mode, const PoolMaps<T> &maps, int S, float p, float eps, float *out, hipStream_t s)
{
    const dim3 grid((unsigned)ceil_div(maps.first[S], 4)), blk(256);
    const float inv_p = 1.0f / p;
    switch (mode) {
        case 1: hipLaunchKernelGGL((pool_multi_kernel<KIND, 1, T>), grid, blk, 0, s, maps, S, p, inv_p, eps, out); break;
        case 2: hipLaunchKernelGGL((pool_multi_kernel<KIND, 2, T>), grid, blk, 0, s, maps, S, p, inv_p, eps, out); break;
        case 3: hipLaunchKernelGGL((pool_multi_kernel<KIND, 3, T>), grid, blk, 0, s, maps, S, p, inv_p, eps, out); break;
        default: hipLaunchKernelGGL((pool_multi_kernel<KIND, 0, T>), grid, blk, 0, s, maps, S, p, inv_p, eps, out); break;
    }
}

template <int KIND, typename T>
static void launch_pool(int mode, const T *feat, int64_t planes, int HW, float p, float eps,
                        float *out, hipStream_t s)
{
    const dim3 grid((unsigned)ceil_div(planes, 4)), blk(256);
    const float inv_p = 1.0f / p;
    switch (mode) {
        case 1: hipLaunchKernelGGL((pool_kernel<KIND, 1, T>), grid, blk, 0, s, feat, planes, HW, p, inv_p, eps, out); break;
        case 2: hipLaunchKernelGGL((pool_kernel<KIND, 2, T>), grid, blk, 0, s, feat, planes, HW, p, inv_p, eps, out); break;
        case 3: hipLaunchKernelGGL((pool_kernel<KIND, 3, T>), grid, blk, 0, s, feat, planes, HW, p, inv_p, eps, out); break;
        default: hipLaunchKernelGGL((pool_kernel<KIND, 0, T>), grid, blk, 0, s, feat, planes, HW, p, inv_p, eps, out); break;
    }
}

}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_l2n_rows(float *x, int64_t R, int64_t D, const float *bias, float eps, void *stream)
{
    MDX_CHECK_ARG(x, "mdx_l2n_rows: NULL pointer");
    MDX_CHECK_ARG(R > 0 && D > 0 && R < (1ll << 31), "mdx_l2n_rows: R=%lld D=%lld", (long long)R,
                  (long long)D);
    hipLaunchKernelGGL(l2n_rows_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, x, D,
                       bias, eps);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

// mdx_pool_l2n / mdx_pool_l2n_f16 (`who`): T = the element of the maps
extern "C++" {
template <typename T>
static int pool_l2n(const char *who, const T *feat, int B, int C, int H, int W, int kind, float p, float pool_eps, float l2n_eps, float *out,
                    void *stream)
{
    MDX_CHECK_ARG(feat && out, "%s: NULL pointer", who);
    MDX_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape [%d,%d,%d,%d]", who, B, C, H, W);
    MDX_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: H*W too large", who);
    hipStream_t s = (hipStream_t)stream;
    const int64_t planes = (int64_t)B * C;
    const int HW = H * W;
    switch (kind) {
        case MDX_POOL_GEM: {
            MDX_CHECK_ARG(p > 0.0f && pool_eps > 0.0f, "%s: gem needs p > 0 and eps > 0", who);
            const int mode = p == 1.0f ? 1 : p == 2.0f ? 2 : p == 3.0f ? 3 : 0;
            launch_pool<MDX_POOL_GEM>(mode, feat, planes, HW, p, pool_eps, out, s);
            break;
        }
        case MDX_POOL_MAC: launch_pool<MDX_POOL_MAC>(1, feat, planes, HW, 1.0f, 0.0f, out, s); break;
        case MDX_POOL_SPOC: launch_pool<MDX_POOL_SPOC>(1, feat, planes, HW, 1.0f, 0.0f, out, s); break;
        default: MDX_CHECK_ARG(false, "%s: unknown pooling kind %d", who, kind);
    }
    MDX_LAUNCH_CHECK();
    if (l2n_eps >= 0.0f) return mdx_l2n_rows(out, B, C, nullptr, l2n_eps, stream);
    return MDX_OK;
}
}   // extern "C++"

int mdx_pool_l2n(const float *feat, int B, int C, int H, int W, int kind, float p, float pool_eps,
                 float l2n_eps, float *out, void *stream)
{
    return pool_l2n("mdx_pool_l2n", feat, B, C, H, W, kind, p, pool_eps, l2n_eps, out, stream);
}

int mdx_pool_l2n_f16(const __half *feat, int B, int C, int H, int W, int kind, float p, float pool_eps,
                     float l2n_eps, float *out, void *stream)
{
    return pool_l2n("mdx_pool_l2n_f16", feat, B, C, H, W, kind, p, pool_eps, l2n_eps, out, stream);
}

// ---------------------------------------------------------------------------
// R-MAC (cirtorch/layers/functional.py:26-72): maxima over the whole map and over a grid of square regions, each
// L2-normalised over the channels (eps added to the norm), summed in region order.  The grid is the caller's (the reference
// computes it in float32 tensor arithmetic; the host restates that, mdir_amd/layers.py).
// Launch 1: one wave per (image, channel) plane -- the plane is read ONCE into registers (lane = column block), every region's
// maximum is a masked wave reduction: regmax[b][r][c].  Launch 2: one workgroup per image walks the regions in order: norm over
// the channels (workgroup reduction), v += max / (norm + eps).
// ---------------------------------------------------------------------------
constexpr int RMAC_MAX_REGIONS = 64;
struct RmacGrid { int i0[RMAC_MAX_REGIONS], j0[RMAC_MAX_REGIONS], h[RMAC_MAX_REGIONS], w[RMAC_MAX_REGIONS]; int n; };

// (also `roipool` of functional.py:75-121: KIND = the regional pooling -- max, mean or GeM over every region)
extern "C++" {
template <int KIND, int MODE>
__global__ __launch_bounds__(256) void roi_pool_kernel(const float *__restrict__ feat, int64_t planes, int C, int H, int W, RmacGrid grid,
                                                       float pw, float inv_p, float eps, float *__restrict__ regions_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const float *p = feat + plane * (int64_t)H * W;
    const int64_t b = plane / C, c = plane % C;
    for (int r = 0; r < grid.n; ++r) {
        const int i0 = grid.i0[r], j0 = grid.j0[r], rh = grid.h[r], rw = grid.w[r];
        float acc = KIND == MDX_POOL_MAC ? -INFINITY : 0.0f;
        bool saw_nan = false;
        for (int e = lane; e < rh * rw; e += 64) {           // (the map is L2-resident after region 0)
            const float v = pool_elem<KIND, MODE>(p[(i0 + e / rw) * W + j0 + e % rw], pw, eps);
            acc = KIND == MDX_POOL_MAC ? fmaxf(acc, v) : acc + v;
            if (KIND == MDX_POOL_MAC) saw_nan |= v != v;
        }
        acc = KIND == MDX_POOL_MAC ? max_or_nan(wave_max(acc), saw_nan) : wave_sum(acc);
        if (KIND != MDX_POOL_MAC) acc = acc / (float)(rh * rw);
        if (KIND == MDX_POOL_GEM && MODE != 1) acc = powf(acc, inv_p);
        if (lane == 0) regions_out[(b * grid.n + r) * C + c] = acc;
    }
}

static int fill_grid(RmacGrid *grid, const int32_t *regions, int nregions, int H, int W, const char *who)
{
    grid->n = nregions;
    for (int r = 0; r < nregions; ++r) {
        grid->i0[r] = regions[4 * r]; grid->j0[r] = regions[4 * r + 1]; grid->h[r] = regions[4 * r + 2]; grid->w[r] = regions[4 * r + 3];
        MDX_CHECK_ARG(grid->i0[r] >= 0 && grid->j0[r] >= 0 && grid->h[r] > 0 && grid->w[r] > 0 && grid->i0[r] + grid->h[r] <= H && grid->j0[r] + grid->w[r] <= W,
                      "%s: region %d = (%d, %d, %d, %d) outside the %d x %d map", who, r, grid->i0[r], grid->j0[r], grid->h[r], grid->w[r], H, W);
    }
    return MDX_OK;
}

template <int KIND>
static void launch_roi(int mode, const float *feat, int64_t planes, int C, int H, int W, const RmacGrid &grid, float p, float eps, float *out,
                       hipStream_t s)
{
    const dim3 g((unsigned)ceil_div(planes, (int64_t)4)), b(256);
    const float inv_p = 1.0f / p;
    switch (mode) {
        case 1: hipLaunchKernelGGL((roi_pool_kernel<KIND, 1>), g, b, 0, s, feat, planes, C, H, W, grid, p, inv_p, eps, out); break;
        case 2: hipLaunchKernelGGL((roi_pool_kernel<KIND, 2>), g, b, 0, s, feat, planes, C, H, W, grid, p, inv_p, eps, out); break;
        case 3: hipLaunchKernelGGL((roi_pool_kernel<KIND, 3>), g, b, 0, s, feat, planes, C, H, W, grid, p, inv_p, eps, out); break;
        default: hipLaunchKernelGGL((roi_pool_kernel<KIND, 0>), g, b, 0, s, feat, planes, C, H, W, grid, p, inv_p, eps, out); break;
    }
}
}   // extern "C++"

int mdx_roipool(const float *feat, int B, int C, int H, int W, const int32_t *regions, int nregions, int kind, float p, float pool_eps,
                float *out, void *stream)
{
    MDX_CHECK_ARG(feat && regions && out, "mdx_roipool: NULL pointer");
    MDX_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "mdx_roipool: bad shape [%d,%d,%d,%d]", B, C, H, W);
    MDX_CHECK_ARG(nregions >= 1 && nregions <= RMAC_MAX_REGIONS, "mdx_roipool: %d regions, 1..%d supported", nregions, RMAC_MAX_REGIONS);
    RmacGrid grid;
    int rc = fill_grid(&grid, regions, nregions, H, W, "mdx_roipool");
    if (rc != MDX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t planes = (int64_t)B * C;
    switch (kind) {
        case MDX_POOL_GEM: {
            MDX_CHECK_ARG(p > 0.0f && pool_eps > 0.0f, "mdx_roipool: gem needs p > 0 and eps > 0");
            launch_roi<MDX_POOL_GEM>(p == 1.0f ? 1 : p == 2.0f ? 2 : p == 3.0f ? 3 : 0, feat, planes, C, H, W, grid, p, pool_eps, out, s);
            break;
        }
        case MDX_POOL_MAC: launch_roi<MDX_POOL_MAC>(1, feat, planes, C, H, W, grid, 1.0f, 0.0f, out, s); break;
        case MDX_POOL_SPOC: launch_roi<MDX_POOL_SPOC>(1, feat, planes, C, H, W, grid, 1.0f, 0.0f, out, s); break;
        default: MDX_CHECK_ARG(false, "mdx_roipool: unknown pooling kind %d", kind);
    }
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

// eps < 0: the region vectors are summed as they are (Rpool's `o.sum(1)`, pooling.py:91)
__global__ __launch_bounds__(256) void rmac_sum_kernel(const float *__restrict__ regmax, int C, int nreg, float eps, float *__restrict__ out)
{
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const float *m = regmax + (int64_t)blockIdx.x * nreg * C;
    float *o = out + (int64_t)blockIdx.x * C;
    for (int r = 0; r < nreg; ++r) {
        float den = 1.0f;
        if (eps >= 0.0f) {                     // (uniform)
            float ss = 0.0f;
            for (int k = tid; k < C; k += 256) ss += m[r * (int64_t)C + k] * m[r * (int64_t)C + k];
            ss = wave_sum(ss);
            __syncthreads();                   // `part` of the previous region has been read by everybody
            if ((tid & 63) == 0) part[tid >> 6] = ss;
            __syncthreads();
            den = sqrtf((part[0] + part[1]) + (part[2] + part[3])) + eps;
        }
        for (int k = tid; k < C; k += 256) {
            const float v = m[r * (int64_t)C + k] / den;
            o[k] = r == 0 ? v : o[k] + v;       // a thread owns its channels: no hazard between regions
        }
    }
}

int mdx_region_sum(const float *vecs, int B, int nregions, int C, float l2n_eps, float *out, void *stream)
{
    MDX_CHECK_ARG(vecs && out, "mdx_region_sum: NULL pointer");
    MDX_CHECK_ARG(B > 0 && C > 0 && nregions >= 1, "mdx_region_sum: bad shape [%d,%d,%d]", B, nregions, C);
    hipLaunchKernelGGL(rmac_sum_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, vecs, C, nregions, l2n_eps, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_rmac_workspace(int B, int C, int nregions)
{
    if (B <= 0 || C <= 0 || nregions <= 0) return 0;
    return (int64_t)B * nregions * C * 4;
}

int mdx_rmac(const float *feat, int B, int C, int H, int W, const int32_t *regions, int nregions, float eps, void *workspace,
             int64_t workspace_bytes, float *out, void *stream)
{
    MDX_CHECK_ARG(feat && regions && out, "mdx_rmac: NULL pointer");
    MDX_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "mdx_rmac: bad shape [%d,%d,%d,%d]", B, C, H, W);
    MDX_CHECK_ARG(nregions >= 1 && nregions <= RMAC_MAX_REGIONS, "mdx_rmac: %d regions, 1..%d supported", nregions, RMAC_MAX_REGIONS);
    MDX_CHECK_ARG(eps >= 0.0f, "mdx_rmac: eps=%g", (double)eps);
    const int64_t need = mdx_rmac_workspace(B, C, nregions);
    MDX_CHECK_WORKSPACE("mdx_rmac", workspace, workspace_bytes, need);
    RmacGrid grid;
    int rc = fill_grid(&grid, regions, nregions, H, W, "mdx_rmac");
    if (rc != MDX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t planes = (int64_t)B * C;
    launch_roi<MDX_POOL_MAC>(1, feat, planes, C, H, W, grid, 1.0f, 0.0f, (float *)workspace, s);
    hipLaunchKernelGGL(rmac_sum_kernel, dim3((unsigned)B), dim3(256), 0, s, (const float *)workspace, C, nregions, eps, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

// mdx_pool_multi / mdx_pool_multi_f16 (`who`): T = the element of the maps
extern "C++" {
template <typename T>
static int pool_multi(const char *who, const T *const *feats, int S, int B, int C, const int *H, const int *W, int kind, float p,
                      float pool_eps, float *pooled, void *stream)
{
    MDX_CHECK_ARG(feats && H && W && pooled, "%s: NULL pointer", who);
    MDX_CHECK_ARG(S >= 1 && S <= 8, "%s: S=%d not in 1..8", who, S);
    MDX_CHECK_ARG(B > 0 && C > 0, "%s: bad batch/channels [%d,%d]", who, B, C);
    PoolMaps<T> maps;
    maps.first[0] = 0;
    for (int s = 0; s < 8; ++s) {
        maps.feat[s] = s < S ? feats[s] : nullptr;
        maps.hw[s] = 0;
        if (s < S) {
            MDX_CHECK_ARG(feats[s], "%s: map %d is NULL", who, s);
            MDX_CHECK_ARG(H[s] > 0 && W[s] > 0 && (int64_t)H[s] * W[s] < (1ll << 31), "%s: bad map size %d x %d", who, H[s], W[s]);
            maps.hw[s] = H[s] * W[s];
        }
        maps.first[s + 1] = maps.first[s] + (s < S ? (int64_t)B * C : 0);
    }
    hipStream_t st = (hipStream_t)stream;
    switch (kind) {
        case MDX_POOL_GEM: {
            MDX_CHECK_ARG(p > 0.0f && pool_eps > 0.0f, "%s: gem needs p > 0 and eps > 0", who);
            const int mode = p == 1.0f ? 1 : p == 2.0f ? 2 : p == 3.0f ? 3 : 0;
            launch_pool_multi<MDX_POOL_GEM>(mode, maps, S, p, pool_eps, pooled, st);
            break;
        }
        case MDX_POOL_MAC: launch_pool_multi<MDX_POOL_MAC>(1, maps, S, 1.0f, 0.0f, pooled, st); break;
        case MDX_POOL_SPOC: launch_pool_multi<MDX_POOL_SPOC>(1, maps, S, 1.0f, 0.0f, pooled, st); break;
        default: MDX_CHECK_ARG(false, "%s: unknown pooling kind %d", who, kind);
    }
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}
}   // extern "C++"

int mdx_pool_multi(const float *const *feats, int S, int B, int C, const int *H, const int *W, int kind, float p,
                   float pool_eps, float *pooled, void *stream)
{
    return pool_multi("mdx_pool_multi", feats, S, B, C, H, W, kind, p, pool_eps, pooled, stream);
}

int mdx_pool_multi_f16(const __half *const *feats, int S, int B, int C, const int *H, const int *W, int kind, float p,
                       float pool_eps, float *pooled, void *stream)
{
    return pool_multi("mdx_pool_multi_f16", feats, S, B, C, H, W, kind, p, pool_eps, pooled, stream);
}

int mdx_l2n_aggregate(const float *pooled, int S, int64_t B, int64_t D, float l2n_eps, float msp, float *out,
                      void *stream)
{
    MDX_CHECK_ARG(pooled && out, "mdx_l2n_aggregate: NULL pointer");
    MDX_CHECK_ARG(S >= 1 && S <= 8, "mdx_l2n_aggregate: S=%d not in 1..8", S);
    MDX_CHECK_ARG(D > 0 && B > 0 && B < (1ll << 31), "mdx_l2n_aggregate: B=%lld D=%lld", (long long)B, (long long)D);
    MDX_CHECK_ARG(msp > 0.0f && l2n_eps >= 0.0f, "mdx_l2n_aggregate: msp=%g eps=%g", (double)msp, (double)l2n_eps);
    hipLaunchKernelGGL(l2n_aggregate_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, pooled, S, B, D, l2n_eps,
                       msp, 1.0f / msp, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_ms_aggregate_batch(const float *const *scale_mats, int S, int64_t B, int64_t D, float msp, float *out,
                           void *stream)
{
    MDX_CHECK_ARG(scale_mats && out, "mdx_ms_aggregate_batch: NULL pointer");
    MDX_CHECK_ARG(S >= 1 && S <= 8, "mdx_ms_aggregate_batch: S=%d not in 1..8", S);
    MDX_CHECK_ARG(D > 0 && B > 0 && B < (1ll << 31), "mdx_ms_aggregate_batch: B=%lld D=%lld", (long long)B, (long long)D);
    ScalePtrs sp;
    for (int s = 0; s < 8; ++s) {
        sp.p[s] = s < S ? scale_mats[s] : nullptr;
        MDX_CHECK_ARG(s >= S || sp.p[s], "mdx_ms_aggregate_batch: scale %d is NULL", s);
    }
    hipLaunchKernelGGL(ms_aggregate_batch_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, sp, S, D, msp,
                       1.0f / msp, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_ms_aggregate(const float *const *scale_vecs, int S, int64_t D, float msp, float *out,
                     void *stream)
{
    MDX_CHECK_ARG(scale_vecs && out, "mdx_ms_aggregate: NULL pointer");
    MDX_CHECK_ARG(S >= 1 && S <= 8, "mdx_ms_aggregate: S=%d not in 1..8", S);
    MDX_CHECK_ARG(D > 0, "mdx_ms_aggregate: D=%lld", (long long)D);
    ScalePtrs sp;
    for (int s = 0; s < 8; ++s) {
        sp.p[s] = s < S ? scale_vecs[s] : nullptr;
        MDX_CHECK_ARG(s >= S || sp.p[s], "mdx_ms_aggregate: scale %d is NULL", s);
    }
    hipLaunchKernelGGL(ms_aggregate_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sp, S, D, msp,
                       1.0f / msp, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
