// int8 refinement of per-query shortlists (include/mdx_refine.h, mdx_refine_i8): the MDX_I8 scores of a shortlist of ids against codes
// kept in list order, found through `where`, then the per-query sort of mdx_rescore.
//
//   refine_kernel    one workgroup of four waves per (query, 64 shortlist entries); a wave takes 16 entries, four at a time.  A
//                    candidate's row is gathered whole into registers: lane l loads the 16 bytes k = 1024 j + 16 l .. of it, and the
//                    loads of all four candidates are issued before the first is consumed.  The query's codes for the lane's k
//                    slices stay in registers (NS slices of 1024 k, d_pad <= 1024 NS; NS = 0: rows of more than 4096 columns, whose
//                    query pieces are loaded again slice by slice).  Four byte products per v_dot4 (__builtin_amdgcn_sdot4), the
//                    int32 partial sums added across the wave by shuffles: integers, so no order changes a bit.
//   rescore_sort     mdx_shortlist_sort.h, as mdx_rescore launches it.
#include "mdx_exact.h"
#include "mdx_i8_quant.h"
#include "mdx_shortlist_sort.h"

namespace mdx {
namespace {

constexpr int RF_TC = 64;                   // shortlist entries per workgroup
constexpr int RF_PER_WAVE = RF_TC / 4;      // entries per wave
constexpr int RF_FLIGHT = 4;                // candidates whose rows a wave has in flight
constexpr int RF_SLICE = 1024;              // k per wave-instruction: 16 bytes per lane
constexpr int RF_MAX_NS = 4;                // slices of the query a lane keeps in registers
constexpr int64_t RF_LIMIT = 1ll << 31;

// bytes k .. k + 15 of the codes of query q (zeros beyond d).  vec: d % 16 == 0 and a 16-byte aligned base, so that a piece inside the
// row is one 16-byte load (as query_piece of mdx_lists_i8.hip)
__device__ __forceinline__ i32x4 refine_query_piece(const int8_t *qcodes, int64_t q, int64_t d, int64_t k, bool vec)
{
    i32x4 w = {0, 0, 0, 0};
    if (k >= d) return w;
    const int8_t *p = qcodes + q * d + k;
    if (vec && k + 16 <= d) return *(const i32x4 *)p;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (k + e < d) w[e >> 2] |= (int)((uint32_t)(uint8_t)p[e] << (8 * (e & 3)));
    return w;
}

// acc + the 16 byte products of two pieces
__device__ __forceinline__ int dot16(i32x4 a, i32x4 b, int acc)
{
#pragma unroll
    for (int v = 0; v < 4; ++v) acc = __builtin_amdgcn_sdot4(a[v], b[v], acc, false);
    return acc;
}

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NS>
__global__ __launch_bounds__(256) void refine_kernel(const int8_t *__restrict__ codes, const float *__restrict__ scales, int64_t m,
                                                     int64_t d, int64_t d_pad, const int64_t *__restrict__ where, int64_t n,
                                                     const int8_t *__restrict__ qcodes, const float *__restrict__ qscales,
                                                     const int64_t *__restrict__ ids, int64_t S, int64_t tiles, bool qvec,
                                                     float *__restrict__ out)
{
    __shared__ int64_t pos[RF_TC];              // the position of the entry's row, -1 without one
    const int64_t q = (int64_t)blockIdx.x / tiles, c0 = ((int64_t)blockIdx.x % tiles) * RF_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < RF_TC) {
        const int64_t j = c0 + tid;
        const int64_t id = j < S ? ids[q * S + j] : -1;
        int64_t p = -1;
        if (id >= 0 && id < n) {                // an id outside [0, n) dereferences neither where nor codes
            const int64_t w = where[id];
            if (w >= 0 && w < m) p = w;
        }
        pos[tid] = p;
    }
    __syncthreads();
    const int64_t kl = 16 * lane;
    i32x4 qr[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) qr[s] = refine_query_piece(qcodes, q, d, (int64_t)RF_SLICE * s + kl, qvec);
    const float sq = qscales[q];

    for (int g = 0; g < RF_PER_WAVE / RF_FLIGHT; ++g) {
        const int e0 = wave * RF_PER_WAVE + g * RF_FLIGHT;
        if (c0 + e0 >= S) break;                                  // wave-uniform: no entry is left
        int64_t p[RF_FLIGHT];
#pragma unroll
        for (int c = 0; c < RF_FLIGHT; ++c) {                     // the same value in every lane: kept in scalar registers
            const int64_t v = pos[e0 + c];
            const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
            p[c] = (int64_t)(((uint64_t)hi << 32) | lo);
        }
        const int64_t mine = lane < RF_FLIGHT ? pos[e0 + lane] : -1;
        const float sc = mine >= 0 ? scales[mine] : __builtin_nanf("");
        int acc[RF_FLIGHT] = {0, 0, 0, 0};
        if (NS > 0) {
            i32x4 a[RF_FLIGHT][NS > 0 ? NS : 1];
#pragma unroll
            for (int c = 0; c < RF_FLIGHT; ++c)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int64_t k = (int64_t)RF_SLICE * s + kl;  // a piece that starts below d_pad ends at or below it
                    a[c][s] = (p[c] >= 0 && k < d_pad) ? *(const i32x4 *)(codes + p[c] * d_pad + k) : (i32x4){0, 0, 0, 0};
                }
#pragma unroll
            for (int c = 0; c < RF_FLIGHT; ++c)
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[c] = dot16(a[c][s], qr[s], acc[c]);
        } else {
            for (int64_t k = kl; k < d_pad; k += RF_SLICE) {
                const i32x4 qv = refine_query_piece(qcodes, q, d, k, qvec);
                i32x4 a[RF_FLIGHT];
#pragma unroll
                for (int c = 0; c < RF_FLIGHT; ++c)
                    a[c] = p[c] >= 0 ? *(const i32x4 *)(codes + p[c] * d_pad + k) : (i32x4){0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < RF_FLIGHT; ++c) acc[c] = dot16(a[c], qv, acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < RF_FLIGHT; ++c) acc[c] = wave_sum_i32(acc[c]);
        const int sum = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
        if (lane < RF_FLIGHT && c0 + e0 + lane < S)
            out[q * S + c0 + e0 + lane] = mine >= 0 ? __fmul_rn((float)sum, __fmul_rn(sc, sq)) : __builtin_nanf("");
    }
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_refine_i8_workspace(int64_t nq, int64_t S)
{
    if (nq < 1 || S < 1 || S > MDX_RESCORE_MAX_K) return 0;
    return round_up(nq * S * 4, 256);
}

int mdx_refine_i8(const int8_t *codes, const float *scales, int64_t m, int64_t d, const int64_t *where, int64_t n, const int8_t *qcodes,
                  const float *qscales, int64_t nq, const int64_t *ids, int64_t S, int64_t *out_ids, float *out_scores, void *workspace,
                  int64_t workspace_bytes, void *stream)
{
    const char *who = "mdx_refine_i8";
    MDX_CHECK_ARG(codes && scales && where && qcodes && qscales && ids && out_ids && out_scores, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && m >= 1 && d >= 1 && nq >= 1 && S >= 1, "%s: n=%lld m=%lld d=%lld nq=%lld S=%lld must be >= 1", who, (long long)n,
                  (long long)m, (long long)d, (long long)nq, (long long)S);
    MDX_CHECK_ARG(S <= MDX_RESCORE_MAX_K, "%s: S=%lld > %d", who, (long long)S, MDX_RESCORE_MAX_K);
    MDX_CHECK_ARG(d <= I8_MAX_DPAD, "%s: d=%lld too large (127^2 * round_up(d, 64) must stay below 2^31; d <= %lld)", who, (long long)d,
                  (long long)I8_MAX_DPAD);
    MDX_CHECK_ARG(n < RF_LIMIT && m < RF_LIMIT && nq < RF_LIMIT, "%s: n=%lld m=%lld nq=%lld must be below 2^31", who, (long long)n,
                  (long long)m, (long long)nq);
    const int64_t tiles = ceil_div(S, (int64_t)RF_TC);
    MDX_CHECK_ARG(nq * tiles < RF_LIMIT, "%s: nq=%lld S=%lld too large for one launch", who, (long long)nq, (long long)S);
    MDX_CHECK_ARG(((uintptr_t)codes & 15) == 0, "%s: codes must be 16-byte aligned", who);
    MDX_CHECK_WORKSPACE(who, workspace, workspace_bytes, mdx_refine_i8_workspace(nq, S));
    hipStream_t s = (hipStream_t)stream;
    float *sc = (float *)workspace;
    const int64_t d_pad = round_up(d, 64);
    const bool qvec = d % 16 == 0 && ((uintptr_t)qcodes & 15) == 0;    // 16-byte pieces at 16-byte addresses
    const dim3 grid((unsigned)(nq * tiles)), block(256);
#define MDX_REFINE_LAUNCH(NS)                                                                                                            \
    hipLaunchKernelGGL(refine_kernel<NS>, grid, block, 0, s, codes, scales, m, d, d_pad, where, n, qcodes, qscales, ids, S, tiles, qvec, sc)
    if (d_pad <= RF_SLICE) MDX_REFINE_LAUNCH(1);
    else if (d_pad <= 2 * RF_SLICE) MDX_REFINE_LAUNCH(2);
    else if (d_pad <= RF_MAX_NS * RF_SLICE) MDX_REFINE_LAUNCH(4);
    else MDX_REFINE_LAUNCH(0);
#undef MDX_REFINE_LAUNCH
    int P = 1;
    while (P < S) P <<= 1;
    hipLaunchKernelGGL(rescore_sort_kernel, dim3((unsigned)nq), dim3(SORT_THREADS), 0, s, (const float *)sc, ids, S, P, out_ids, out_scores);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
