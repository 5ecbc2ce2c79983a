// Editing the lists of the inverted file (include/mdx_lists_edit.h): the merge of two list-ordered structures and the compaction of
// one.  Both are one gather pass over opaque payload rows and their member ids, after a small launch that writes the new offsets.
//
//   merge     a thread owns one piece (16, 4 or 1 bytes) of one destination row: it finds the row's list by a binary search of
//             out_offsets, then its source row in a or b.  Pieces are numbered row-major over the destination, so a wave writes a
//             contiguous run where out_ld == width.
//   compact   a thread owns one piece of one source row; kept[p] is where the row goes.  What stays keeps its order, so the writes
//             of a wave ascend with its reads.
#include <initializer_list>

#include "mdx_lists_clamp.h"

namespace mdx {
namespace {

constexpr int THREADS = 256;
constexpr int SPAN = MDX_LISTS_EDIT_SPAN;   // pieces a workgroup moves at a time
constexpr int PER_THREAD = SPAN / THREADS;  // loads in flight per thread
constexpr int64_t LIMIT = 1ll << 31;

static_assert(SPAN % THREADS == 0 && PER_THREAD >= 1, "a span is a whole number of pieces per thread");

template <int W> struct Piece;
template <> struct Piece<16> { typedef int type __attribute__((ext_vector_type(4))); };
template <> struct Piece<4> { typedef uint32_t type; };
template <> struct Piece<1> { typedef uint8_t type; };

// ------------------------------------------------------------------------------------------------------------------ merge

__global__ __launch_bounds__(THREADS) void merge_offsets_kernel(const int64_t *__restrict__ a_offsets, int64_t ma,
                                                                const int64_t *__restrict__ b_offsets, int64_t mb, int64_t K,
                                                                int64_t *__restrict__ out_offsets)
{
    const int64_t l = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (l <= K) out_offsets[l] = clamp_to(a_offsets[l], ma) + clamp_to(b_offsets[l], mb);
}

// One piece of destination row p = t / ppr.  false: nothing covers p (or its source would lie outside a and b), nothing is loaded.
template <int W>
__device__ __forceinline__ bool merge_source(const uint8_t *__restrict__ a_rows, int64_t a_ld, const int64_t *__restrict__ a_members,
                                             const int64_t *__restrict__ a_offsets, int64_t ma, const uint8_t *__restrict__ b_rows,
                                             int64_t b_ld, const int64_t *__restrict__ b_members, const int64_t *__restrict__ b_offsets,
                                             int64_t mb, int64_t K, const int64_t *__restrict__ out_offsets, int64_t p, int64_t j,
                                             typename Piece<W>::type &v, int64_t &id)
{
    // the list of p: the first l in [0, K) with out_offsets[l + 1] > p
    int64_t lo = 0, hi = K;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (out_offsets[mid + 1] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= K) return false;                                    // at or beyond the last offset
    const int64_t i = p - out_offsets[lo];
    if (i < 0) return false;                                      // offsets that do not ascend
    int64_t a0, an, b0, bn;
    list_extent(a_offsets, lo, ma, a0, an);
    list_extent(b_offsets, lo, mb, b0, bn);
    const uint8_t *row;
    if (i < an) {                                                 // a0 + i < a0 + an <= ma
        row = a_rows + (a0 + i) * a_ld;
        id = a_members[a0 + i];
    } else if (i - an < bn) {                                     // b0 + i - an < b0 + bn <= mb
        row = b_rows + (b0 + i - an) * b_ld;
        id = b_members[b0 + i - an];
    } else {
        return false;
    }
    v = *(const typename Piece<W>::type *)(row + j * W);
    return true;
}

template <int W>
__global__ __launch_bounds__(THREADS) void lists_merge_kernel(const uint8_t *__restrict__ a_rows, int64_t a_ld,
                                                              const int64_t *__restrict__ a_members, const int64_t *__restrict__ a_offsets,
                                                              int64_t ma, const uint8_t *__restrict__ b_rows, int64_t b_ld,
                                                              const int64_t *__restrict__ b_members, const int64_t *__restrict__ b_offsets,
                                                              int64_t mb, int64_t K, int64_t ppr, const int64_t *__restrict__ out_offsets,
                                                              uint8_t *__restrict__ out_rows, int64_t out_ld,
                                                              int64_t *__restrict__ out_members)
{
    typedef typename Piece<W>::type T;
    const int64_t total = (ma + mb) * ppr;
    for (int64_t t0 = (int64_t)blockIdx.x * SPAN + threadIdx.x; t0 < total; t0 += (int64_t)gridDim.x * SPAN) {
        T v[PER_THREAD];
        int64_t id[PER_THREAD], p[PER_THREAD], j[PER_THREAD];
        bool have[PER_THREAD];
#pragma unroll
        for (int u = 0; u < PER_THREAD; ++u) {
            const int64_t t = t0 + u * THREADS;
            have[u] = false;
            if (t < total) {
                p[u] = t / ppr;
                j[u] = t - p[u] * ppr;
                have[u] = merge_source<W>(a_rows, a_ld, a_members, a_offsets, ma, b_rows, b_ld, b_members, b_offsets, mb, K, out_offsets,
                                          p[u], j[u], v[u], id[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < PER_THREAD; ++u) {
            if (!have[u]) continue;
            *(T *)(out_rows + p[u] * out_ld + j[u] * W) = v[u];  // p < ma + mb, j W < width <= out_ld
            if (j[u] == 0) out_members[p[u]] = id[u];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ compact

__global__ __launch_bounds__(THREADS) void compact_offsets_kernel(const int64_t *__restrict__ offsets, int64_t m, int64_t K,
                                                                  const int64_t *__restrict__ kept, int64_t mo,
                                                                  int64_t *__restrict__ out_offsets)
{
    const int64_t l = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (l <= K) out_offsets[l] = clamp_to(kept[clamp_to(offsets[l], m)], mo);
}

template <int W>
__global__ __launch_bounds__(THREADS) void lists_compact_kernel(const uint8_t *__restrict__ rows, int64_t ld,
                                                                const int64_t *__restrict__ members, int64_t m, int64_t ppr,
                                                                const int64_t *__restrict__ kept, int64_t mo,
                                                                uint8_t *__restrict__ out_rows, int64_t out_ld,
                                                                int64_t *__restrict__ out_members)
{
    typedef typename Piece<W>::type T;
    const int64_t total = m * ppr;
    for (int64_t t0 = (int64_t)blockIdx.x * SPAN + threadIdx.x; t0 < total; t0 += (int64_t)gridDim.x * SPAN) {
        T v[PER_THREAD];
        int64_t id[PER_THREAD], to[PER_THREAD], j[PER_THREAD];
        bool have[PER_THREAD];
#pragma unroll
        for (int u = 0; u < PER_THREAD; ++u) {
            const int64_t t = t0 + u * THREADS;
            have[u] = false;
            if (t < total) {
                const int64_t p = t / ppr;                        // < m
                j[u] = t - p * ppr;
                to[u] = kept[p];
                have[u] = kept[p + 1] > to[u] && to[u] >= 0 && to[u] < mo;
                if (have[u]) {
                    v[u] = *(const T *)(rows + p * ld + j[u] * W);
                    id[u] = members[p];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PER_THREAD; ++u) {
            if (!have[u]) continue;
            *(T *)(out_rows + to[u] * out_ld + j[u] * W) = v[u];
            if (j[u] == 0) out_members[to[u]] = id[u];
        }
    }
}

// 16, 4 or 1: the widest piece that width, every stride and every base are multiples of
static int piece_width(int64_t width, std::initializer_list<int64_t> strides, std::initializer_list<const void *> bases)
{
    uintptr_t all = (uintptr_t)width;
    for (int64_t s : strides) all |= (uintptr_t)s;
    for (const void *b : bases) all |= (uintptr_t)b;
    return all % 16 == 0 ? 16 : all % 4 == 0 ? 4 : 1;
}

static unsigned groups_of(int64_t pieces)
{
    const int64_t spans = ceil_div(pieces, SPAN);
    return (unsigned)(spans < MDX_LISTS_EDIT_GROUPS ? spans : MDX_LISTS_EDIT_GROUPS);
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_lists_merge(const uint8_t *a_rows, int64_t a_ld, const int64_t *a_members, const int64_t *a_offsets, int64_t ma,
                    const uint8_t *b_rows, int64_t b_ld, const int64_t *b_members, const int64_t *b_offsets, int64_t mb, int64_t K,
                    int64_t width, uint8_t *out_rows, int64_t out_ld, int64_t *out_members, int64_t *out_offsets, void *stream)
{
    const char *who = "mdx_lists_merge";
    MDX_CHECK_ARG(a_rows && a_members && a_offsets && b_rows && b_members && b_offsets && out_rows && out_members && out_offsets,
                  "%s: NULL pointer", who);
    MDX_CHECK_ARG(ma >= 0 && mb >= 0 && ma < LIMIT && mb < LIMIT && ma + mb >= 1 && ma + mb < LIMIT,
                  "%s: ma=%lld mb=%lld must be >= 0 and ma + mb in [1, 2^31)", who, (long long)ma, (long long)mb);
    MDX_CHECK_ARG(K >= 1 && K < LIMIT && width >= 1 && width < LIMIT, "%s: K=%lld width=%lld must be in [1, 2^31)", who, (long long)K,
                  (long long)width);
    MDX_CHECK_ARG(a_ld >= width && b_ld >= width && out_ld >= width && a_ld < LIMIT && b_ld < LIMIT && out_ld < LIMIT,
                  "%s: a_ld=%lld b_ld=%lld out_ld=%lld must be in [width=%lld, 2^31)", who, (long long)a_ld, (long long)b_ld,
                  (long long)out_ld, (long long)width);
    const void *ins[] = {a_rows, a_members, a_offsets, b_rows, b_members, b_offsets}, *outs[] = {out_rows, out_members, out_offsets};
    for (const void *o : outs)
        for (const void *i : ins) MDX_CHECK_ARG(o != i, "%s: an output pointer equals an input pointer", who);
    MDX_CHECK_ARG(outs[0] != outs[1] && outs[0] != outs[2] && outs[1] != outs[2], "%s: two output pointers are equal", who);
    // a structure of no rows is never read: its stride and base do not narrow the pieces
    const int W = piece_width(width, {ma ? a_ld : 0, mb ? b_ld : 0, out_ld}, {ma ? a_rows : nullptr, mb ? b_rows : nullptr, out_rows});
    const int64_t ppr = width / W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(merge_offsets_kernel, dim3((unsigned)ceil_div(K + 1, THREADS)), dim3(THREADS), 0, s, a_offsets, ma, b_offsets, mb, K,
                       out_offsets);
    const dim3 grid(groups_of((ma + mb) * ppr));
#define MDX_MERGE_LAUNCH(w)                                                                                                              \
    hipLaunchKernelGGL(lists_merge_kernel<w>, grid, dim3(THREADS), 0, s, a_rows, a_ld, a_members, a_offsets, ma, b_rows, b_ld, b_members, \
                       b_offsets, mb, K, ppr, (const int64_t *)out_offsets, out_rows, out_ld, out_members)
    if (W == 16)
        MDX_MERGE_LAUNCH(16);
    else if (W == 4)
        MDX_MERGE_LAUNCH(4);
    else
        MDX_MERGE_LAUNCH(1);
#undef MDX_MERGE_LAUNCH
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_lists_compact(const uint8_t *rows, int64_t ld, const int64_t *members, const int64_t *offsets, int64_t m, int64_t K, int64_t width,
                      const int64_t *kept, int64_t mo, uint8_t *out_rows, int64_t out_ld, int64_t *out_members, int64_t *out_offsets,
                      void *stream)
{
    const char *who = "mdx_lists_compact";
    MDX_CHECK_ARG(rows && members && offsets && kept && out_rows && out_members && out_offsets, "%s: NULL pointer", who);
    MDX_CHECK_ARG(m >= 1 && m < LIMIT && mo >= 1 && mo < LIMIT, "%s: m=%lld mo=%lld must be in [1, 2^31)", who, (long long)m, (long long)mo);
    MDX_CHECK_ARG(K >= 1 && K < LIMIT && width >= 1 && width < LIMIT, "%s: K=%lld width=%lld must be in [1, 2^31)", who, (long long)K,
                  (long long)width);
    MDX_CHECK_ARG(ld >= width && out_ld >= width && ld < LIMIT && out_ld < LIMIT, "%s: ld=%lld out_ld=%lld must be in [width=%lld, 2^31)", who,
                  (long long)ld, (long long)out_ld, (long long)width);
    const void *ins[] = {rows, members, offsets, kept}, *outs[] = {out_rows, out_members, out_offsets};
    for (const void *o : outs)
        for (const void *i : ins) MDX_CHECK_ARG(o != i, "%s: an output pointer equals an input pointer", who);
    MDX_CHECK_ARG(outs[0] != outs[1] && outs[0] != outs[2] && outs[1] != outs[2], "%s: two output pointers are equal", who);
    const int W = piece_width(width, {ld, out_ld}, {rows, out_rows});
    const int64_t ppr = width / W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(compact_offsets_kernel, dim3((unsigned)ceil_div(K + 1, THREADS)), dim3(THREADS), 0, s, offsets, m, K, kept, mo,
                       out_offsets);
    const dim3 grid(groups_of(m * ppr));
#define MDX_COMPACT_LAUNCH(w) \
    hipLaunchKernelGGL(lists_compact_kernel<w>, grid, dim3(THREADS), 0, s, rows, ld, members, m, ppr, kept, mo, out_rows, out_ld, out_members)
    if (W == 16)
        MDX_COMPACT_LAUNCH(16);
    else if (W == 4)
        MDX_COMPACT_LAUNCH(4);
    else
        MDX_COMPACT_LAUNCH(1);
#undef MDX_COMPACT_LAUNCH
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
