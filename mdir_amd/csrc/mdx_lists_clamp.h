// The offsets of a list-ordered structure as every kernel reads them: clamped to [0, m], so that offsets which lie outside the
// structure or do not ascend give empty lists and never an address outside it.  Included by mdx_ivf_plan.h (the plan and the scans)
// and by mdx_lists_edit.hip (the merge and the compaction).
#pragma once
#include "mdx_common.h"

namespace mdx {
namespace {

__device__ __forceinline__ int64_t clamp_to(int64_t o, int64_t hi) { return o < 0 ? 0 : o > hi ? hi : o; }

// where list l starts after clamping its offsets to [0, m], and the members it has
__device__ __forceinline__ void list_extent(const int64_t *__restrict__ offsets, int64_t l, int64_t m, int64_t &start, int64_t &size)
{
    const int64_t lo = clamp_to(offsets[l], m), hi = clamp_to(offsets[l + 1], m);
    start = lo;
    size = hi > lo ? hi - lo : 0;
}

__device__ __forceinline__ int64_t list_size(const int64_t *__restrict__ offsets, int64_t l, int64_t m)
{
    int64_t start, size;
    list_extent(offsets, l, m, start, size);
    return size;
}

}  // namespace
}  // namespace mdx
