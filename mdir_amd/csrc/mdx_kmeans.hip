// Spherical k-means beside the similarity (include/mdx_kmeans.h): the best centroid of every row of a score block, the sum of every
// cluster's rows in a fixed order, and the normalisation of the sums.  All three are streaming kernels bound by HBM; there are no
// float atomics, so a call returns the same bits on every run.
#include <math.h>

#include "mdx_common.h"

namespace mdx {

constexpr int SEG = MDX_KMEANS_SEGMENT;
constexpr int SLICE = 1024;                     // dimensions per workgroup of the segment sums: 256 threads x 4
constexpr int WAVE_ROW_MAX_K = 1024;            // up to here one wave reads a row of scores (16 columns per lane and less)

// ------------------------------------------------------------------------------------------------------------------ argmax

// the running best of a lane: columns arrive in ascending order, so `<` on the order key keeps the first of equal scores
__device__ __forceinline__ void arg_first(uint32_t &bk, uint32_t &bi, float v, uint32_t i)
{
    const uint32_t k = desc_key(v);
    if (k < bk) {
        bk = k;
        bi = i;
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

// minimum of (key << 32 | id) over the wave: the smaller key, on a tie the smaller id
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = shfl_xor_u64(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// (key << 32 | id) of the best of the columns first, first + step, ... of one row; a row on the 16-byte grid is read four columns
// at a time (a thread's quads ascend, then its share of the K % 4 tail, whose ids are larger still)
__device__ __forceinline__ uint64_t row_best(const float *__restrict__ src, int K, int first, int step)
{
    uint32_t bk = 0xFFFFFFFFu, bi = 0xFFFFFFFFu;            // a NaN (key 0xFFFFFFFF) never replaces this: an all-NaN row keeps id -1
    if (((uintptr_t)src & 15) == 0) {
        const int n4 = K >> 2;
        for (int i = first; i < n4; i += step) {
            const float4 v = *(const float4 *)(src + 4 * i);
            arg_first(bk, bi, v.x, 4 * i);
            arg_first(bk, bi, v.y, 4 * i + 1);
            arg_first(bk, bi, v.z, 4 * i + 2);
            arg_first(bk, bi, v.w, 4 * i + 3);
        }
        for (int i = 4 * n4 + first; i < K; i += step) arg_first(bk, bi, src[i], i);
    } else {
        for (int i = first; i < K; i += step) arg_first(bk, bi, src[i], i);
    }
    return ((uint64_t)bk << 32) | bi;
}

__device__ __forceinline__ void put_best(const float *__restrict__ src, uint64_t packed, int64_t row, int64_t *__restrict__ labels,
                                         float *__restrict__ best)
{
    uint32_t id = (uint32_t)packed;
    if (id == 0xFFFFFFFFu) id = 0;                          // nothing but NaN: the first column, as the ranking has it
    if (labels) labels[row] = id;
    if (best) best[row] = src[id];
}

// one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void argmax_wave_kernel(const float *__restrict__ scores, int64_t m, int K, int64_t ld,
                                                          int64_t *__restrict__ labels, float *__restrict__ best)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const float *src = scores + row * ld;
    const uint64_t p = wave_min_u64(row_best(src, K, lane, 64));
    if (lane == 0) put_best(src, p, row, labels, best);
}

// one workgroup per row
__global__ __launch_bounds__(256) void argmax_block_kernel(const float *__restrict__ scores, int K, int64_t ld, int64_t *__restrict__ labels,
                                                           float *__restrict__ best)
{
    __shared__ uint64_t part[4];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float *src = scores + row * ld;
    const uint64_t p = wave_min_u64(row_best(src, K, tid, 256));
    if ((tid & 63) == 0) part[tid >> 6] = p;
    __syncthreads();
    if (tid == 0) {
        uint64_t b = part[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) b = part[w] < b ? part[w] : b;
        put_best(src, b, row, labels, best);
    }
}

// ------------------------------------------------------------------------------------------------------------------ sums

__device__ __forceinline__ int64_t clamp_offset(int64_t o, int64_t n) { return o < 0 ? 0 : o > n ? n : o; }

// the members cluster c has after clamping, and its segments
__device__ __forceinline__ int64_t cluster_segments(const int64_t *__restrict__ offsets, int64_t c, int64_t n)
{
    const int64_t lo = clamp_offset(offsets[c], n), hi = clamp_offset(offsets[c + 1], n);
    return hi > lo ? (hi - lo + SEG - 1) / SEG : 0;
}

// one workgroup: segbase[c] = the number of segments of the clusters before c, segbase[K] = all of them.  Thread t owns a run of
// ceil(K / 1024) clusters; the 1024 run totals are scanned in LDS
__global__ __launch_bounds__(1024) void segbase_kernel(const int64_t *__restrict__ offsets, int64_t K, int64_t n, int64_t *__restrict__ segbase)
{
    __shared__ int64_t sh[1024];
    const int t = threadIdx.x;
    const int64_t per = (K + 1023) / 1024;
    const int64_t c0 = t * per < K ? t * per : K, c1 = c0 + per < K ? c0 + per : K;
    int64_t local = 0;
    for (int64_t c = c0; c < c1; ++c) local += cluster_segments(offsets, c, n);
    sh[t] = local;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    int64_t run = sh[t] - local;
    for (int64_t c = c0; c < c1; ++c) {
        segbase[c] = run;
        run += cluster_segments(offsets, c, n);
    }
    if (t == 1023) segbase[K] = sh[1023];
}

// acc = acc + x over the members, in order, for `count` dimensions dim0, dim0 + step, ... of one thread (dword loads).  A skipped member
// adds +0, which leaves every acc as it is (acc starts from +0 and is never -0)
template <int MAXC>
__device__ __forceinline__ void chain_dwords(const float *__restrict__ rows, int64_t ld, const int64_t *ids, int members, int64_t dim0, int step,
                                             int count, float *__restrict__ out)
{
    float acc[MAXC];
#pragma unroll
    for (int e = 0; e < MAXC; ++e) acc[e] = 0.0f;
#pragma unroll 4
    for (int j = 0; j < members; ++j) {
        const int64_t id = ids[j];
#pragma unroll
        for (int e = 0; e < MAXC; ++e) {
            const float v = (id >= 0 && e < count) ? rows[id * ld + dim0 + (int64_t)e * step] : 0.0f;
            acc[e] = acc[e] + v;
        }
    }
#pragma unroll
    for (int e = 0; e < MAXC; ++e)
        if (e < count) out[dim0 + (int64_t)e * step] = acc[e];
}

// one workgroup per (segment, slice of SLICE dimensions).  VEC: rows on the 16-byte grid and ld % 4 == 0 -- a thread owns the dimensions
// 4 t .. 4 t + 3 of the slice; otherwise t, t + 256, t + 512, t + 768
template <bool VEC>
__global__ __launch_bounds__(256) void segment_sums_kernel(const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld,
                                                           const int64_t *__restrict__ members, const int64_t *__restrict__ offsets,
                                                           const int64_t *__restrict__ segbase, int64_t K, int slices, int64_t bound,
                                                           float *__restrict__ partials, int64_t dpad)
{
    __shared__ int64_t ids[SEG];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x / slices;
    const int slice = blockIdx.x % slices;
    const int64_t all = segbase[K];
    if (g >= (all < bound ? all : bound)) return;           // (the whole workgroup) the segment does not exist
    // the cluster of segment g: the last c with segbase[c] <= g (segbase[0] = 0 <= g < segbase[K])
    int64_t lo = 0, hi = K;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (segbase[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t start = clamp_offset(offsets[lo], n) + (g - segbase[lo]) * SEG;
    const int64_t stop = clamp_offset(offsets[lo + 1], n);
    const int count = (int)(stop - start < SEG ? stop - start : SEG);         // 1 .. SEG: start < stop <= n, because the segment exists
    for (int j = tid; j < count; j += 256) {
        const int64_t id = members[start + j];
        ids[j] = (id >= 0 && id < n) ? id : -1;
    }
    __syncthreads();
    float *out = partials + g * dpad;
    if (VEC) {
        const int64_t d0 = (int64_t)slice * SLICE + 4 * tid;
        if (d0 + 4 <= d) {
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
            for (int j = 0; j < count; ++j) {
                const int64_t id = ids[j];
                const float4 v = id >= 0 ? *(const float4 *)(rows + id * ld + d0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                acc.x = acc.x + v.x;
                acc.y = acc.y + v.y;
                acc.z = acc.z + v.z;
                acc.w = acc.w + v.w;
            }
            *(float4 *)(out + d0) = acc;                     // the workspace lies on the 16-byte grid and dpad % 4 == 0
        } else if (d0 < d) {
            chain_dwords<3>(rows, ld, ids, count, d0, 1, (int)(d - d0), out);
        }
    } else {
        const int64_t d0 = (int64_t)slice * SLICE + tid;
        if (d0 < d) {
            const int64_t left = (d - d0 + 255) / 256;
            chain_dwords<4>(rows, ld, ids, count, d0, 256, (int)(left < 4 ? left : 4), out);
        }
    }
}

// one thread per (cluster, dimension): the chain over the cluster's partials in segment order
__global__ __launch_bounds__(256) void cluster_sums_kernel(const float *__restrict__ partials, int64_t dpad, const int64_t *__restrict__ segbase,
                                                           int64_t bound, int64_t d, int dslices, float *__restrict__ sums)
{
    const int64_t c = blockIdx.x / dslices;
    const int64_t dim = (int64_t)(blockIdx.x % dslices) * 256 + threadIdx.x;
    if (dim >= d) return;
    const int64_t s0 = segbase[c];
    const int64_t s1 = segbase[c + 1] < bound ? segbase[c + 1] : bound;
    float acc = 0.0f;
#pragma unroll 4
    for (int64_t s = s0; s < s1; ++s) acc = acc + partials[s * dpad + dim];
    sums[c * d + dim] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ finish

// one workgroup per row: c = s / (||s|| + eps); an all-zero row takes the previous centroid (zeros without one)
__global__ __launch_bounds__(256) void finish_kernel(const float *sums, int64_t d, float eps, const float *previous, float *centroids)
{
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const float *s = sums + (int64_t)blockIdx.x * d;
    float *o = centroids + (int64_t)blockIdx.x * d;
    float ss = 0.0f;
    int nonzero = 0;
    for (int64_t k = tid; k < d; k += 256) {
        const float v = s[k];
        ss = __fmaf_rn(v, v, ss);
        nonzero |= v != 0.0f;                               // (a NaN counts as not zero)
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    nonzero = __syncthreads_or(nonzero);
    if (!nonzero) {
        const float *prev = previous ? previous + (int64_t)blockIdx.x * d : nullptr;
        for (int64_t k = tid; k < d; k += 256) o[k] = prev ? prev[k] : 0.0f;
        return;
    }
    const float den = sqrtf((part[0] + part[1]) + (part[2] + part[3])) + eps;
    for (int64_t k = tid; k < d; k += 256) o[k] = s[k] / den;
}

constexpr int64_t LIMIT = 1ll << 31;

// the segments the grid of mdx_kmeans_sums is sized by
static inline int64_t segment_bound(int64_t n, int64_t K) { return ceil_div(n, SEG) + K; }

static inline bool sums_sizes_ok(int64_t n, int64_t K, int64_t d)
{
    if (n < 1 || K < 1 || d < 1 || n >= LIMIT || K >= LIMIT || d >= LIMIT) return false;
    return segment_bound(n, K) * ceil_div(d, SLICE) < LIMIT && K * ceil_div(d, 256) < LIMIT;
}

}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_kmeans_argmax(const float *scores, int64_t m, int64_t K, int64_t ld, int64_t *labels, float *best, void *stream)
{
    MDX_CHECK_ARG(scores && (labels || best), "mdx_kmeans_argmax: NULL pointer");
    MDX_CHECK_ARG(m >= 1 && K >= 1 && m < LIMIT && K < LIMIT, "mdx_kmeans_argmax: m=%lld K=%lld must be in [1, 2^31)", (long long)m, (long long)K);
    MDX_CHECK_ARG(ld >= K, "mdx_kmeans_argmax: ld=%lld < K=%lld", (long long)ld, (long long)K);
    MDX_CHECK_ARG(ld <= INT64_MAX / m, "mdx_kmeans_argmax: m * ld overflows");
    hipStream_t s = (hipStream_t)stream;
    if (K <= WAVE_ROW_MAX_K)
        hipLaunchKernelGGL(argmax_wave_kernel, dim3((unsigned)ceil_div(m, 4)), dim3(256), 0, s, scores, m, (int)K, ld, labels, best);
    else
        hipLaunchKernelGGL(argmax_block_kernel, dim3((unsigned)m), dim3(256), 0, s, scores, (int)K, ld, labels, best);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_kmeans_sums_workspace(int64_t n, int64_t K, int64_t d)
{
    if (!sums_sizes_ok(n, K, d)) return 0;
    return round_up(8 * (K + 1), 256) + round_up(4 * segment_bound(n, K) * round_up(d, 4), 256);
}

int mdx_kmeans_sums(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, const int64_t *offsets, int64_t K,
                    float *sums, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(rows && members && offsets && sums, "mdx_kmeans_sums: NULL pointer");
    MDX_CHECK_ARG(n >= 1 && d >= 1 && K >= 1, "mdx_kmeans_sums: n=%lld d=%lld K=%lld must be >= 1", (long long)n, (long long)d, (long long)K);
    MDX_CHECK_ARG(sums_sizes_ok(n, K, d), "mdx_kmeans_sums: n=%lld d=%lld K=%lld too large (a size or a launch of 2^31 or more)", (long long)n,
                  (long long)d, (long long)K);
    MDX_CHECK_ARG(ld >= d, "mdx_kmeans_sums: ld=%lld < d=%lld", (long long)ld, (long long)d);
    MDX_CHECK_ARG(ld <= INT64_MAX / n, "mdx_kmeans_sums: n * ld overflows");
    MDX_CHECK_WORKSPACE("mdx_kmeans_sums", workspace, workspace_bytes, mdx_kmeans_sums_workspace(n, K, d));
    hipStream_t s = (hipStream_t)stream;
    int64_t *segbase = (int64_t *)workspace;
    float *partials = (float *)((char *)workspace + round_up(8 * (K + 1), 256));
    const int64_t bound = segment_bound(n, K), dpad = round_up(d, 4);
    const int slices = (int)ceil_div(d, SLICE), dslices = (int)ceil_div(d, 256);
    hipLaunchKernelGGL(segbase_kernel, dim3(1), dim3(1024), 0, s, offsets, K, n, segbase);
    const dim3 grid((unsigned)(bound * slices)), blk(256);
    if (((uintptr_t)rows & 15) == 0 && (ld & 3) == 0)
        hipLaunchKernelGGL(segment_sums_kernel<true>, grid, blk, 0, s, rows, n, d, ld, members, offsets, (const int64_t *)segbase, K, slices, bound,
                           partials, dpad);
    else
        hipLaunchKernelGGL(segment_sums_kernel<false>, grid, blk, 0, s, rows, n, d, ld, members, offsets, (const int64_t *)segbase, K, slices, bound,
                           partials, dpad);
    hipLaunchKernelGGL(cluster_sums_kernel, dim3((unsigned)(K * dslices)), blk, 0, s, (const float *)partials, dpad, (const int64_t *)segbase, bound, d,
                       dslices, sums);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_kmeans_finish(const float *sums, int64_t K, int64_t d, float eps, const float *previous, float *centroids, void *stream)
{
    MDX_CHECK_ARG(sums && centroids, "mdx_kmeans_finish: NULL pointer");
    MDX_CHECK_ARG(K >= 1 && d >= 1 && K < LIMIT && d < LIMIT, "mdx_kmeans_finish: K=%lld d=%lld must be in [1, 2^31)", (long long)K, (long long)d);
    MDX_CHECK_ARG(eps >= 0.0f, "mdx_kmeans_finish: eps=%g", (double)eps);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, sums, d, eps, previous, centroids);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
