// The plan of the inverted file (include/mdx_ivf.h) as the kernels that read it see it: its sections, the list of a work item and
// the slots of its entries, the checks every call makes of the sizes it shares with the plan, and the second launch of a scan
// (NaN / -1 beyond a query's count).  Shared by mdx_ivf.hip (the plan itself, the fp32 scan, the selection), mdx_lists_i8.hip (the
// int8 scan of the same work items) and mdx_lists_pq.hip (the query-major ADC scan).  Everything sits in an anonymous namespace: each
// file gets its own copy.
#pragma once
#include "mdx_common.h"
#include "mdx_lists_clamp.h"

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

// the list of work item g of a list-major scan: the last l with item[l] <= g
__device__ __forceinline__ int64_t item_list(const int64_t *__restrict__ item, int64_t K, int64_t g)
{
    int64_t lo = 0, hi = K;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (item[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// threads 0 .. G - 1: the query of entry e0 + tid (-1 without one) and the column of tile t's first member in its candidate row
__device__ __forceinline__ void item_slots(int tid, int64_t t, int64_t e0, int ne, const int64_t *__restrict__ entry,
                                           const int64_t *__restrict__ base, int64_t nq, int64_t nprobe, int64_t *qidx, int64_t *qcol)
{
    if (tid >= G) return;
    int64_t qi = -1, col = -1;
    if (tid < ne) {
        const int64_t e = entry[e0 + tid];
        if (e >= 0 && e < nq * nprobe && base[e] >= 0) {
            qi = e / nprobe;
            col = base[e] + t * TC;
        }
    }
    qidx[tid] = qi;
    qcol[tid] = col;
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

// the second launch of every scan
static inline void launch_pad(const Plan &v, int64_t nq, int64_t cap, float *cand_scores, int64_t *cand_ids, hipStream_t s)
{
    const int64_t blocks = ceil_div(cap, 1024);
    hipLaunchKernelGGL(ivf_pad_kernel, dim3((unsigned)(nq * blocks)), dim3(256), 0, s, (const int64_t *)v.count, cap, blocks, cand_scores,
                       cand_ids);
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
