// Re-ranking: the weighted gather-and-normalise of neighbour rows behind alpha-weighted query expansion (alpha-QE) and
// database-side augmentation (DBA) of the GeM paper's protocol (Radenovic, Tolias, Chum, "Fine-tuning CNN image retrieval
// with no human annotation", TPAMI 2018).  The top-k that feeds it is mdx_topk; the similarity is mdx_scores_rowmajor.
//
// One wave per output row.  The row's d accumulators live in registers: lane l owns the 16-byte column slots
// l, l + 64, .. of a block of 256 * NV columns (NV = 8: 32 VGPRs at d = 2048).  The wave walks its neighbours in j order,
// reading each neighbour row as coalesced dwordx4 lane slices, the next row's loads issued before the current row's FMAs.
// Rows that cannot be read 16 bytes at a time (d % 4 != 0, an ld that is not a multiple of 4, a pointer that is not
// 16-byte aligned) take the dword path, which gives every lane the SAME columns and so the same bits.  The weights are
// computed once per (q, j) by lane j % 64 and broadcast with v_readlane; the norm is a per-lane sum in slot order and a
// fixed butterfly across the wave.  d > 256 * 8 runs the column blocks one after another, storing the unscaled sums and
// rescaling them once the norm is known.
#include <math.h>

#include "mdx_common.h"

namespace mdx {

constexpr int AGG_WAVES = 4;                  // waves (output rows) per workgroup

// w_j of include/mdx.h: s ** alpha for s > 0 (alpha == 0 -> 1), 0 otherwise (NaN included)
__device__ __forceinline__ float knn_weight(float s, float alpha)
{
    if (!(s > 0.0f)) return 0.0f;
    return alpha == 0.0f ? 1.0f : powf(s, alpha);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A buffer resource over one row of d floats: loads past its end return zeros and stores past it are dropped, so the
// lanes of the last slots need no branches.  Built from wave-uniform scalars only (readfirstlane), which keeps the
// descriptor in SGPRs.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float *row, int64_t d)
{
    const uint64_t a = (uint64_t)(uintptr_t)row;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)(((uint64_t)hi << 32) | lo), (short)0,
                                             (int)(d * (int64_t)sizeof(float)), 0x00020000);
}

// slot = the four columns c .. c + 3 (c in floats); VEC: one dwordx4, else four dwords (d % 4 != 0 or an unaligned row)
template <bool VEC>
__device__ __forceinline__ float4 load_slot(__amdgpu_buffer_rsrc_t r, int c)
{
    if (VEC) {
        const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, 4 * c, 0, 0);
        return make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
    }
    return make_float4(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * c, 0, 0)),
                       __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * c + 4, 0, 0)),
                       __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * c + 8, 0, 0)),
                       __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4 * c + 12, 0, 0)));
}

template <bool VEC>
__device__ __forceinline__ void store_slot(__amdgpu_buffer_rsrc_t r, int c, float4 v)
{
    if (VEC) {
        u32x4 u;
        u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y); u.z = __float_as_uint(v.z); u.w = __float_as_uint(v.w);
        __builtin_amdgcn_raw_buffer_store_b128(u, r, 4 * c, 0, 0);
        return;
    }
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.x), r, 4 * c, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.y), r, 4 * c + 4, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.z), r, 4 * c + 8, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.w), r, 4 * c + 12, 0, 0);
}

__device__ __forceinline__ void fma4(float4 &acc, float w, float4 x)
{
    acc.x = fmaf(w, x.x, acc.x);
    acc.y = fmaf(w, x.y, acc.y);
    acc.z = fmaf(w, x.z, acc.z);
    acc.w = fmaf(w, x.w, acc.w);
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ float readlanef(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---------------------------------------------------------------------------------------------------------------------
// out[q] = l2n(self[q] + sum_j w(s[q, j]) * rows[ids[q, j]]), j ascending, one fmaf per element and neighbour
// ---------------------------------------------------------------------------------------------------------------------
template <int NV, bool VEC>
__global__ __launch_bounds__(64 * AGG_WAVES) void knn_aggregate_kernel(
    const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld, const int64_t *__restrict__ ids,
    const float *__restrict__ sims, int64_t nq, int64_t k, const float *__restrict__ self_rows, int64_t ld_self,
    float alpha, float eps, float *__restrict__ out, int64_t ld_out)
{
    constexpr int BLOCK = 256 * NV;          // columns per pass: NV 16-byte slots per lane
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * AGG_WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;                     // whole waves only
    const int64_t *qids = ids + q * k;
    const float *qsims = sims + q * k;
    const auto orow = row_rsrc(out + q * ld_out, d);
    const auto srow = row_rsrc(self_rows ? self_rows + q * ld_self : out, self_rows ? d : 0);   // 0 bytes: reads zeros
    float ssq = 0.0f;

    for (int c0 = 0; c0 < d; c0 += BLOCK) {
        const int c = c0 + 4 * lane;         // this lane's first column; slot v is c + 256 v
        float4 acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = load_slot<VEC>(srow, c + 256 * v);

        for (int64_t jb = 0; jb < k; jb += 64) {
            // this chunk's ids and weights, one (q, j) per lane; a neighbour outside [0, n) is never read
            const int64_t j = jb + lane;
            int64_t id = -1;
            float w = 0.0f;
            if (j < k) {
                id = qids[j];
                w = knn_weight(qsims[j], alpha);
            }
            uint64_t todo = __ballot(id >= 0 && id < n);
            if (!todo) continue;
            int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            float wcur = readlanef(w, src);
            auto r = row_rsrc(rows + readlane64(id, src) * ld, d);
            float4 cur[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) cur[v] = load_slot<VEC>(r, c + 256 * v);
            for (;;) {
                const bool more = todo != 0;
                float4 nxt[NV];
                float wnxt = 0.0f;
                if (more) {                   // wave-uniform: the next neighbour's loads go out before this one's FMAs
                    src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    wnxt = readlanef(w, src);
                    r = row_rsrc(rows + readlane64(id, src) * ld, d);
#pragma unroll
                    for (int v = 0; v < NV; ++v) nxt[v] = load_slot<VEC>(r, c + 256 * v);
                }
#pragma unroll
                for (int v = 0; v < NV; ++v) fma4(acc[v], wcur, cur[v]);
                if (!more) break;
#pragma unroll
                for (int v = 0; v < NV; ++v) cur[v] = nxt[v];
                wcur = wnxt;
            }
        }

#pragma unroll
        for (int v = 0; v < NV; ++v) {
            ssq = fmaf(acc[v].x, acc[v].x, ssq);
            ssq = fmaf(acc[v].y, acc[v].y, ssq);
            ssq = fmaf(acc[v].z, acc[v].z, ssq);
            ssq = fmaf(acc[v].w, acc[v].w, ssq);
        }
        if (d <= BLOCK) {
            // the only pass (slots past d hold zeros; their stores fall outside the row's resource and are dropped)
            const float den = sqrtf(wave_sum(ssq)) + eps;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                float4 o = acc[v];
                o.x /= den; o.y /= den; o.z /= den; o.w /= den;
                store_slot<VEC>(orow, c + 256 * v, o);
            }
            return;
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) store_slot<VEC>(orow, c + 256 * v, acc[v]);
    }

    // d > BLOCK: every lane rescales exactly the slots it stored (same lane, same addresses: program order suffices)
    const float den = sqrtf(wave_sum(ssq)) + eps;
    for (int c0 = 0; c0 < d; c0 += BLOCK) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = c0 + 4 * lane + 256 * v;
            float4 o = load_slot<VEC>(orow, c);
            o.x /= den; o.y /= den; o.z /= den; o.w /= den;
            store_slot<VEC>(orow, c, o);
        }
    }
}

template <int NV>
static void launch_aggregate(bool vec, dim3 grid, hipStream_t s, const float *rows, int64_t n, int64_t d, int64_t ld,
                             const int64_t *ids, const float *sims, int64_t nq, int64_t k, const float *self_rows,
                             int64_t ld_self, float alpha, float eps, float *out, int64_t ld_out)
{
    if (vec)
        hipLaunchKernelGGL((knn_aggregate_kernel<NV, true>), grid, dim3(64 * AGG_WAVES), 0, s, rows, n, d, ld, ids, sims, nq,
                           k, self_rows, ld_self, alpha, eps, out, ld_out);
    else
        hipLaunchKernelGGL((knn_aggregate_kernel<NV, false>), grid, dim3(64 * AGG_WAVES), 0, s, rows, n, d, ld, ids, sims, nq,
                           k, self_rows, ld_self, alpha, eps, out, ld_out);
}

// [a, a + bytes) and [b, b + bytes_b) share a byte
static bool overlaps(const void *a, int64_t bytes_a, const void *b, int64_t bytes_b)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_knn_aggregate(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *ids, const float *sims, int64_t nq,
                      int64_t k, const float *self_rows, int64_t ld_self, float alpha, float l2n_eps, float *out, int64_t ld_out,
                      void *stream)
{
    MDX_CHECK_ARG(rows && ids && sims && out, "mdx_knn_aggregate: NULL pointer (rows, ids, sims and out are required)");
    MDX_CHECK_ARG(n >= 1 && d >= 1 && nq >= 1 && k >= 1, "mdx_knn_aggregate: n=%lld d=%lld nq=%lld k=%lld (each must be >= 1)",
                  (long long)n, (long long)d, (long long)nq, (long long)k);
    MDX_CHECK_ARG(ld >= d && ld_out >= d && (!self_rows || ld_self >= d),
                  "mdx_knn_aggregate: ld=%lld ld_self=%lld ld_out=%lld must be >= d=%lld", (long long)ld, (long long)ld_self,
                  (long long)ld_out, (long long)d);
    MDX_CHECK_ARG(isfinite(alpha) && alpha >= 0.0f, "mdx_knn_aggregate: alpha=%g must be finite and >= 0", (double)alpha);
    MDX_CHECK_ARG(isfinite(l2n_eps) && l2n_eps >= 0.0f, "mdx_knn_aggregate: eps=%g must be finite and >= 0", (double)l2n_eps);
    MDX_CHECK_ARG(nq <= (int64_t)0x7FFFFFFF * AGG_WAVES, "mdx_knn_aggregate: nq=%lld too large", (long long)nq);
    MDX_CHECK_ARG(d <= (1 << 28), "mdx_knn_aggregate: d=%lld too large (a row is addressed with 32-bit byte offsets)", (long long)d);
    const int64_t out_bytes = ((nq - 1) * ld_out + d) * (int64_t)sizeof(float);
    MDX_CHECK_ARG(!overlaps(out, out_bytes, rows, ((n - 1) * ld + d) * (int64_t)sizeof(float)),
                  "mdx_knn_aggregate: out overlaps rows (the neighbour rows are read while outputs are written)");
    MDX_CHECK_ARG(!self_rows || !overlaps(out, out_bytes, self_rows, ((nq - 1) * ld_self + d) * (int64_t)sizeof(float)),
                  "mdx_knn_aggregate: out overlaps self_rows");

    const bool vec = d % 4 == 0 && ld % 4 == 0 && ld_out % 4 == 0 && aligned16(rows) && aligned16(out) &&
                     (!self_rows || (ld_self % 4 == 0 && aligned16(self_rows)));
    const dim3 grid((unsigned)ceil_div(nq, AGG_WAVES));
    hipStream_t s = (hipStream_t)stream;
    if (d <= 256)
        launch_aggregate<1>(vec, grid, s, rows, n, d, ld, ids, sims, nq, k, self_rows, ld_self, alpha, l2n_eps, out, ld_out);
    else if (d <= 512)
        launch_aggregate<2>(vec, grid, s, rows, n, d, ld, ids, sims, nq, k, self_rows, ld_self, alpha, l2n_eps, out, ld_out);
    else if (d <= 1024)
        launch_aggregate<4>(vec, grid, s, rows, n, d, ld, ids, sims, nq, k, self_rows, ld_self, alpha, l2n_eps, out, ld_out);
    else
        launch_aggregate<8>(vec, grid, s, rows, n, d, ld, ids, sims, nq, k, self_rows, ld_self, alpha, l2n_eps, out, ld_out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
