// The per-query sort of a scored shortlist, shared by mdx_rescore.hip (mdx_rescore) and mdx_refine.hip (mdx_refine_i8): one workgroup
// per query, a bitonic sort of up to MDX_RESCORE_MAX_K (desc_key, id, position) triples in LDS.  Both files launch it as the second
// of their two launches, on the unsorted scores their first launch left in the workspace.
#pragma once
#include "mdx_common.h"

namespace mdx {
namespace {

constexpr int SORT_THREADS = 1024;

// ascending (desc_key, id, position): key = desc_key << 32 | position, pads = ~0
__device__ __forceinline__ bool sort_before(uint64_t a, uint64_t b, const int64_t *sid)
{
    if ((a >> 32) != (b >> 32)) return (a >> 32) < (b >> 32);
    if (a == ~0ull || b == ~0ull) return a < b;
    const int64_t ia = sid[a & 0xFFFFFFFFu], ib = sid[b & 0xFFFFFFFFu];
    if (ia != ib) return ia < ib;
    return a < b;
}

__global__ __launch_bounds__(SORT_THREADS) void rescore_sort_kernel(const float *__restrict__ sc, const int64_t *ids, int64_t K, int P,
                                                                     int64_t *out_ids, float *out_scores)
{
    __shared__ uint64_t key[MDX_RESCORE_MAX_K];
    __shared__ int64_t sid[MDX_RESCORE_MAX_K];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += SORT_THREADS) {
        if (i < K) {
            key[i] = ((uint64_t)desc_key(sc[q * K + i]) << 32) | (uint32_t)i;
            sid[i] = ids[q * K + i];
        } else {
            key[i] = ~0ull;
        }
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += SORT_THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = key[lo], b = key[hi];
                if (sort_before(b, a, sid) == up) {
                    key[lo] = b;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < K; i += SORT_THREADS) {     // all of the query's ids are in LDS: out_ids may be ids
        const uint32_t p = (uint32_t)(key[i] & 0xFFFFFFFFu);
        out_ids[q * K + i] = sid[p];
        out_scores[q * K + i] = sc[q * K + p];
    }
}

}  // namespace
}  // namespace mdx
