// The plan of the inverted file (include/mdx_ivf.h) as the kernels that read it see it: its sections, the clamping of the offsets,
// the checks every call makes of the sizes it shares with the plan, and the second launch of a scan (NaN / -1 beyond a query's
// count).  Shared by mdx_ivf.hip (the plan itself, the fp32 scan, the selection) and mdx_lists_i8.hip (the int8 scan of the same work
// items).  Everything sits in an anonymous namespace: each of the two files gets its own copy.
#pragma once
#include "mdx_common.h"

namespace mdx {
namespace {

constexpr int G = MDX_IVF_QUERY_GROUP;
constexpr int TC = MDX_IVF_TILE;            // members per tile: one per lane
constexpr int64_t LIMIT = 1ll << 31;

// the sections of the plan (include/mdx_ivf.h)
struct Plan {
    int64_t *base, *count, *first, *item, *entry;
    unsigned long long *cursor;
};

static inline int64_t plan_bytes_of(int64_t nq, int64_t nprobe, int64_t K)
{
    return 2 * round_up(8 * nq * nprobe, 256) + round_up(8 * nq, 256) + 2 * round_up(8 * (K + 1), 256) + round_up(16 * K, 256);
}

static inline Plan carve(const void *plan, int64_t nq, int64_t nprobe, int64_t K)
{
    char *p = (char *)plan;
    Plan v;
    v.base = (int64_t *)p;
    p += round_up(8 * nq * nprobe, 256);
    v.count = (int64_t *)p;
    p += round_up(8 * nq, 256);
    v.first = (int64_t *)p;
    p += round_up(8 * (K + 1), 256);
    v.item = (int64_t *)p;
    p += round_up(8 * (K + 1), 256);
    v.entry = (int64_t *)p;
    p += round_up(8 * nq * nprobe, 256);
    v.cursor = (unsigned long long *)p;
    return v;
}

__device__ __forceinline__ int64_t clamp_to(int64_t o, int64_t hi) { return o < 0 ? 0 : o > hi ? hi : o; }

// the members list l has after clamping its offsets to [0, m]
__device__ __forceinline__ int64_t list_size(const int64_t *__restrict__ offsets, int64_t l, int64_t m)
{
    const int64_t lo = clamp_to(offsets[l], m), hi = clamp_to(offsets[l + 1], m);
    return hi > lo ? hi - lo : 0;
}

// the columns at or beyond a query's count: NaN / -1.  One workgroup per (query, 1024 columns)
__global__ __launch_bounds__(256) void ivf_pad_kernel(const int64_t *__restrict__ count, int64_t cap, int64_t blocks,
                                                      float *__restrict__ cand_scores, int64_t *__restrict__ cand_ids)
{
    const int64_t q = (int64_t)blockIdx.x / blocks, c0 = ((int64_t)blockIdx.x % blocks) * 1024;
    const int64_t have = clamp_to(count[q], cap);
    const int64_t c1 = c0 + 1024 < cap ? c0 + 1024 : cap;
    for (int64_t c = (c0 > have ? c0 : have) + threadIdx.x; c < c1; c += 256) {
        cand_scores[q * cap + c] = __builtin_nanf("");
        cand_ids[q * cap + c] = -1;
    }
}

// the sizes every call shares, and the plan
static int check_plan(const char *who, int64_t nq, int64_t nprobe, int64_t K, const void *plan, int64_t plan_bytes)
{
    MDX_CHECK_ARG(nq >= 1 && nprobe >= 1 && K >= 1, "%s: nq=%lld nprobe=%lld K=%lld must be >= 1", who, (long long)nq, (long long)nprobe,
                  (long long)K);
    MDX_CHECK_ARG(nq < LIMIT && K < LIMIT && nprobe <= K && nq * nprobe < LIMIT,
                  "%s: nq=%lld nprobe=%lld K=%lld too large (nprobe > K, or a size or nq nprobe of 2^31 or more)", who, (long long)nq,
                  (long long)nprobe, (long long)K);
    MDX_CHECK_WORKSPACE(who, plan, plan_bytes, plan_bytes_of(nq, nprobe, K));
    return MDX_OK;
}

static int check_cap(const char *who, int64_t nq, int64_t cap)
{
    MDX_CHECK_ARG(cap >= 1 && cap < LIMIT, "%s: cap=%lld must be in [1, 2^31)", who, (long long)cap);
    MDX_CHECK_ARG(nq * ceil_div(cap, 1024) < LIMIT, "%s: nq=%lld cap=%lld too large for one launch", who, (long long)nq, (long long)cap);
    return MDX_OK;
}

}  // namespace
}  // namespace mdx
