// The overlap of two sets of top-K lists (include/mdx_overlap.h): per query and depth, how many ids of the head of a[q] occur in the
// head of b[q].  One workgroup per query: the head of b[q] goes into an open-addressing table in LDS (32-bit keys, linear probing, at
// most half full) with the position of every id, the head of a[q] is looked up, and a hit at positions (i, j) counts for every depth
// above max(i, j).  Integers only; the only atomics are on LDS.
#include "mdx_common.h"

namespace mdx {

constexpr int OVERLAP_THREADS = 256;
constexpr int OVERLAP_SLOTS = 2 * MDX_OVERLAP_MAX_K;          // the largest table: half full at MDX_OVERLAP_MAX_K keys
constexpr uint32_t OVERLAP_EMPTY = 0xFFFFFFFFu;               // no key: keys are ids below 2^31

struct OverlapDepths {
    int32_t d[MDX_OVERLAP_MAX_DEPTHS];
};

// ids outside [0, 2^31) are padding
__device__ __forceinline__ bool overlap_key(int64_t id, uint32_t *key)
{
    *key = (uint32_t)id;
    return id >= 0 && id < ((int64_t)1 << 31);
}

__device__ __forceinline__ uint32_t overlap_slot(uint32_t key, int shift) { return (key * 2654435761u) >> shift; }

// slots = 1 << (32 - shift) <= OVERLAP_SLOTS and >= 2 * nb, so a probe sequence always meets an empty slot
__global__ __launch_bounds__(OVERLAP_THREADS) void topk_overlap_kernel(const int64_t *__restrict__ a, int ka, const int64_t *__restrict__ b,
                                                                       int kb, OverlapDepths dep, int T, int shift, int32_t *__restrict__ out)
{
    __shared__ uint32_t keys[OVERLAP_SLOTS];
    __shared__ uint16_t where[OVERLAP_SLOTS];
    __shared__ int32_t total[MDX_OVERLAP_MAX_DEPTHS];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t slots = 1u << (32 - shift), mask = slots - 1;
    const int deepest = dep.d[T - 1];
    const int na = deepest < ka ? deepest : ka, nb = deepest < kb ? deepest : kb;
    for (uint32_t s = tid; s < slots; s += OVERLAP_THREADS) keys[s] = OVERLAP_EMPTY;
    if (tid < MDX_OVERLAP_MAX_DEPTHS) total[tid] = 0;
    __syncthreads();
    const int64_t *rb = b + q * kb;
    for (int j = tid; j < nb; j += OVERLAP_THREADS) {
        uint32_t key;
        if (!overlap_key(rb[j], &key)) continue;
        uint32_t s = overlap_slot(key, shift);
        for (;;) {
            const uint32_t old = atomicCAS(&keys[s], OVERLAP_EMPTY, key);
            if (old == OVERLAP_EMPTY) { where[s] = (uint16_t)j; break; }
            if (old == key) break;                                 // a repeated id (outside the contract): the first to arrive stays
            s = (s + 1) & mask;
        }
    }
    __syncthreads();
    int32_t cnt[MDX_OVERLAP_MAX_DEPTHS];
#pragma unroll
    for (int t = 0; t < MDX_OVERLAP_MAX_DEPTHS; ++t) cnt[t] = 0;
    const int64_t *ra = a + q * ka;
    for (int i = tid; i < na; i += OVERLAP_THREADS) {
        uint32_t key;
        if (!overlap_key(ra[i], &key)) continue;
        uint32_t s = overlap_slot(key, shift);
        for (;;) {
            const uint32_t have = keys[s];
            if (have == OVERLAP_EMPTY) break;
            if (have == key) {
                const int j = where[s];
                const int m = i > j ? i : j;
#pragma unroll
                for (int t = 0; t < MDX_OVERLAP_MAX_DEPTHS; ++t) cnt[t] += (t < T && m < dep.d[t]) ? 1 : 0;
                break;
            }
            s = (s + 1) & mask;
        }
    }
#pragma unroll
    for (int t = 0; t < MDX_OVERLAP_MAX_DEPTHS; ++t) {
        int32_t v = cnt[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((tid & 63) == 0 && v) atomicAdd(&total[t], v);
    }
    __syncthreads();
    if (tid < T) out[q * T + tid] = total[tid];
}

}  // namespace mdx

using namespace mdx;

extern "C" int mdx_topk_overlap(const int64_t *a, int64_t ka, const int64_t *b, int64_t kb, int64_t nq, const int32_t *depths, int64_t T,
                                int32_t *out, void *stream)
{
    const char *who = "mdx_topk_overlap";
    MDX_CHECK_ARG(a && b && depths && out, "%s: NULL a, b, depths or out", who);
    MDX_CHECK_ARG(nq >= 1 && nq < ((int64_t)1 << 31), "%s: nq=%lld must be in [1, 2^31)", who, (long long)nq);
    MDX_CHECK_ARG(ka >= 1 && ka <= MDX_OVERLAP_MAX_K && kb >= 1 && kb <= MDX_OVERLAP_MAX_K, "%s: ka=%lld and kb=%lld must be in [1, %d]", who,
                  (long long)ka, (long long)kb, MDX_OVERLAP_MAX_K);
    MDX_CHECK_ARG(T >= 1 && T <= MDX_OVERLAP_MAX_DEPTHS, "%s: T=%lld depths, between 1 and %d", who, (long long)T, MDX_OVERLAP_MAX_DEPTHS);
    OverlapDepths dep;
    for (int t = 0; t < MDX_OVERLAP_MAX_DEPTHS; ++t) dep.d[t] = 0;
    for (int t = 0; t < (int)T; ++t) {
        MDX_CHECK_ARG(depths[t] >= 1 && (t == 0 || depths[t] >= depths[t - 1]), "%s: depths must be positive and ascending (depths[%d]=%d)",
                      who, t, (int)depths[t]);
        dep.d[t] = depths[t];
    }
    MDX_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 7) == 0 && ((uintptr_t)out & 3) == 0, "%s: a and b must be 8-byte aligned, out 4-byte", who);
    const int64_t nb = dep.d[T - 1] < kb ? dep.d[T - 1] : kb;
    int log2 = 6;                                                      // at least 64 slots
    while (((int64_t)1 << log2) < 2 * nb) ++log2;                      // <= 13: 2 * nb <= OVERLAP_SLOTS
    hipLaunchKernelGGL(topk_overlap_kernel, dim3((unsigned)nq), dim3(OVERLAP_THREADS), 0, (hipStream_t)stream, a, (int)ka, b, (int)kb, dep,
                       (int)T, 32 - log2, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}
