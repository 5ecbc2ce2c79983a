// The reverse-edge merge of kNN lists (include/mdx_knn_reverse.h): where row i lists j and j does not list i, (i, score) is offered to
// j, and every row keeps the first k of its own entries and its offers.
//
//   reverse_count_kernel   eight lanes per edge (i, r): the tests of offer_of_edge, row j read in 64-byte steps, then one integer atomic
//                          add on counts[j] by the first of them.
//   reverse_fill_kernel    the same tests; the slot is offsets[j] + an integer atomic ticket on cursor[j]; one 8-byte store per offer.
//   reverse_merge_kernel   one wave (a workgroup of 64) per row: the row's valid entries as a sorted list of (order key << 32 | id)
//                          words in LDS, its offers streamed 64 at a time, filtered against the current k-th entry, and merged by
//                          rank counting -- the rank of an element in the union is its rank in its own list plus the number of
//                          elements of the other list before it; all words are distinct, so the ranks are a permutation and the
//                          arrival order of the offers changes nothing.
#include "mdx_common.h"

namespace mdx {
namespace {

constexpr int KR_MAX_K = MDX_KNN_REVERSE_MAX_K;
constexpr int KR_THREADS = 256;
constexpr int KR_GROUP = 8;                 // lanes that share an edge in the count and fill passes
constexpr int KR_TILE = 64;                 // offers per step of the merge: one per lane
constexpr int64_t KR_LIMIT = 1ll << 31;

// ascending (desc_key, id): ids lie in [0, 2^31), so the words of distinct ids differ
__device__ __forceinline__ uint64_t pair_word(float s, uint32_t id) { return ((uint64_t)desc_key(s) << 32) | id; }

// Edge e = (i, r) of the lists, in the hands of the KR_GROUP lanes sub = 0 .. KR_GROUP - 1 of one aligned lane group: true, in every
// lane of the group, when (i, scores[e]) is an offer to j = ids[e] that can enter row j.  Row j is read once, lane sub taking every
// KR_GROUP-th id, so that a step of the group reads 64 contiguous bytes (one thread walking a row alone pulls a cache line per id and
// lane; measured at N = 1 004 993, k = 50: 39 ms a pass).  Nothing is dereferenced through an id outside [0, n).
__device__ __forceinline__ bool offer_of_edge(const int64_t *__restrict__ ids, const float *__restrict__ scores, int64_t n, int k,
                                              int64_t e, int sub, int64_t *target, uint2 *offer)
{
    const int64_t i = e / k, j = ids[e];
    if (j < 0 || j >= n || j == i) return false;                // the same in every lane of the group
    const float s = scores[e];
    const int64_t *row = ids + j * k;
    int valid = 0, member = 0;
    for (int c = sub; c < k; c += KR_GROUP) {
        const int64_t v = row[c];
        valid += (v >= 0 && v < n) ? 1 : 0;
        member |= v == i ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < KR_GROUP; o <<= 1) {                    // integers: the order of the sum changes nothing
        valid += __shfl_xor(valid, o, 64);
        member |= __shfl_xor(member, o, 64);
    }
    if (member) return false;
    // a row without padding: its k-th own entry is its last, and an offer that does not precede it cannot be among the first k
    if (valid == k && !(pair_word(s, (uint32_t)i) < pair_word(scores[j * k + k - 1], (uint32_t)row[k - 1]))) return false;
    *target = j;
    *offer = make_uint2(__float_as_uint(s), (uint32_t)i);
    return true;
}

__global__ __launch_bounds__(KR_THREADS) void reverse_count_kernel(const int64_t *__restrict__ ids, const float *__restrict__ scores,
                                                                   int64_t n, int k, int64_t edges, int32_t *__restrict__ counts)
{
    const int64_t e = ((int64_t)blockIdx.x * KR_THREADS + threadIdx.x) / KR_GROUP;
    const int sub = threadIdx.x % KR_GROUP;
    if (e >= edges) return;                                     // whole groups: KR_THREADS is a multiple of KR_GROUP
    int64_t j;
    uint2 offer;
    if (offer_of_edge(ids, scores, n, k, e, sub, &j, &offer) && sub == 0) atomicAdd(&counts[j], 1);
}

__global__ __launch_bounds__(KR_THREADS) void reverse_fill_kernel(const int64_t *__restrict__ ids, const float *__restrict__ scores,
                                                                  int64_t n, int k, int64_t edges, const int64_t *__restrict__ offsets,
                                                                  int32_t *__restrict__ cursor, uint2 *__restrict__ offers,
                                                                  int64_t capacity)
{
    const int64_t e = ((int64_t)blockIdx.x * KR_THREADS + threadIdx.x) / KR_GROUP;
    const int sub = threadIdx.x % KR_GROUP;
    if (e >= edges) return;
    int64_t j;
    uint2 offer;
    if (!offer_of_edge(ids, scores, n, k, e, sub, &j, &offer) || sub != 0) return;
    const int64_t slot = offsets[j] + (int64_t)atomicAdd(&cursor[j], 1);
    if (slot >= 0 && slot < capacity) offers[slot] = offer;       // never at or beyond the capacity, whatever offsets holds
}

__global__ __launch_bounds__(KR_TILE) void reverse_merge_kernel(const int64_t *__restrict__ ids, const float *__restrict__ scores,
                                                                int64_t n, int k, const int64_t *__restrict__ offsets,
                                                                const uint2 *__restrict__ offers, int64_t capacity,
                                                                int64_t *__restrict__ out_ids, float *__restrict__ out_scores,
                                                                int32_t *__restrict__ gained)
{
    __shared__ uint64_t word[2][KR_MAX_K];      // the current list, ascending, and the one being built
    __shared__ uint32_t bits[2][KR_MAX_K];      // the score of every entry as it came in
    __shared__ uint32_t offered[2][KR_MAX_K];   // 1: the entry came from an offer
    __shared__ uint64_t tword[KR_TILE];         // the offers of a tile that passed the filter
    __shared__ uint32_t tbits[KR_TILE];
    const int64_t j = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;

    // the row's valid entries, compacted in their order: an id outside [0, n) is padding wherever it stands
    uint64_t w[2] = {0, 0};
    uint32_t b[2] = {0, 0};
    bool ok[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        if (p < k) {
            const int64_t id = ids[j * k + p];
            if (id >= 0 && id < n) {
                const float s = scores[j * k + p];
                ok[h] = true, w[h] = pair_word(s, (uint32_t)id), b[h] = __float_as_uint(s);
            }
        }
    }
    const uint64_t b0 = __ballot(ok[0]), b1 = __ballot(ok[1]);
    const int n0 = __popcll(b0);
    int m = n0 + __popcll(b1);                  // entries of the current list, <= k
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (ok[h]) {
            const int pos = h == 0 ? __popcll(b0 & below) : n0 + __popcll(b1 & below);
            word[0][pos] = w[h], bits[0][pos] = b[h], offered[0][pos] = 0;
        }
    __syncthreads();

    int cur = 0;
    int64_t lo = offsets[j], hi = offsets[j + 1];
    lo = lo < 0 ? 0 : lo > capacity ? capacity : lo;            // the segment, inside the buffer whatever offsets holds
    hi = hi < lo ? lo : hi > capacity ? capacity : hi;
    for (int64_t t0 = lo; t0 < hi; t0 += KR_TILE) {
        bool have = t0 + lane < hi;
        uint64_t ow = 0;
        uint32_t ob = 0;
        if (have) {
            const uint2 o = offers[t0 + lane];
            ow = pair_word(__uint_as_float(o.x), o.y), ob = o.x;
            if (m == k && !(ow < word[cur][k - 1])) have = false;       // cannot be among the first k any more
        }
        const uint64_t pass = __ballot(have);
        const int tn = __popcll(pass);
        if (tn == 0) continue;                  // the same in every lane; no LDS was written
        if (have) {
            const int pos = __popcll(pass & below);
            tword[pos] = ow, tbits[pos] = ob;
        }
        __syncthreads();
        const int nxt = cur ^ 1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < m) {
                const uint64_t a = word[cur][p];
                int r = p;
                for (int t = 0; t < tn; ++t) r += tword[t] < a ? 1 : 0;
                if (r < k) word[nxt][r] = a, bits[nxt][r] = bits[cur][p], offered[nxt][r] = offered[cur][p];
            }
        }
        if (lane < tn) {
            const uint64_t a = tword[lane];
            int r = 0;
            for (int t = 0; t < tn; ++t) r += tword[t] < a ? 1 : 0;
            for (int p = 0; p < m; ++p) r += word[cur][p] < a ? 1 : 0;
            if (r < k) word[nxt][r] = a, bits[nxt][r] = tbits[lane], offered[nxt][r] = 1;
        }
        m = m + tn < k ? m + tn : k;
        cur = nxt;
        __syncthreads();
    }

    int g = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        if (p < k) {
            const bool filled = p < m;
            out_ids[j * k + p] = filled ? (int64_t)(uint32_t)word[cur][p] : -1;
            out_scores[j * k + p] = filled ? __uint_as_float(bits[cur][p]) : __builtin_nanf("");
            g += filled ? (int)(offered[cur][p] & 1u) : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
    if (lane == 0) gained[j] = g;
}

// the checks the three calls share; who: the entry point
int check_lists(const char *who, const int64_t *ids, const float *scores, int64_t n, int64_t k)
{
    MDX_CHECK_ARG(ids && scores, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && k >= 1, "%s: n=%lld k=%lld must be >= 1", who, (long long)n, (long long)k);
    MDX_CHECK_ARG(k <= KR_MAX_K, "%s: k=%lld > %d", who, (long long)k, KR_MAX_K);
    MDX_CHECK_ARG(n < KR_LIMIT, "%s: n=%lld must be below 2^31", who, (long long)n);
    MDX_CHECK_ARG(n * k < KR_LIMIT, "%s: n=%lld k=%lld: n * k must be below 2^31", who, (long long)n, (long long)k);
    MDX_CHECK_ARG(((uintptr_t)ids & 7) == 0, "%s: ids must be 8-byte aligned", who);
    MDX_CHECK_ARG(((uintptr_t)scores & 3) == 0, "%s: scores must be 4-byte aligned", who);
    return MDX_OK;
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_knn_reverse_count(const int64_t *ids, const float *scores, int64_t n, int64_t k, int32_t *counts, void *stream)
{
    const char *who = "mdx_knn_reverse_count";
    MDX_CHECK_ARG(counts, "%s: NULL pointer", who);
    if (int rc = check_lists(who, ids, scores, n, k)) return rc;
    MDX_CHECK_ARG(((uintptr_t)counts & 3) == 0, "%s: counts must be 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    MDX_HIP(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), s));
    const int64_t edges = n * k;
    hipLaunchKernelGGL(reverse_count_kernel, dim3((unsigned)ceil_div(edges * KR_GROUP, (int64_t)KR_THREADS)), dim3(KR_THREADS), 0, s, ids, scores, n,
                       (int)k, edges, counts);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_knn_reverse_fill(const int64_t *ids, const float *scores, int64_t n, int64_t k, const int64_t *offsets, int32_t *cursor,
                         void *offers, int64_t capacity, void *stream)
{
    const char *who = "mdx_knn_reverse_fill";
    MDX_CHECK_ARG(offsets && cursor && offers, "%s: NULL pointer", who);
    if (int rc = check_lists(who, ids, scores, n, k)) return rc;
    MDX_CHECK_ARG(capacity >= 1, "%s: capacity=%lld must be >= 1", who, (long long)capacity);
    MDX_CHECK_ARG(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)offers & 7) == 0, "%s: offsets and offers must be 8-byte aligned", who);
    MDX_CHECK_ARG(((uintptr_t)cursor & 3) == 0, "%s: cursor must be 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    MDX_HIP(hipMemsetAsync(cursor, 0, (size_t)n * sizeof(int32_t), s));
    const int64_t edges = n * k;
    hipLaunchKernelGGL(reverse_fill_kernel, dim3((unsigned)ceil_div(edges * KR_GROUP, (int64_t)KR_THREADS)), dim3(KR_THREADS), 0, s, ids, scores, n,
                       (int)k, edges, offsets, cursor, (uint2 *)offers, capacity);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_knn_reverse_merge(const int64_t *ids, const float *scores, int64_t n, int64_t k, const int64_t *offsets, const void *offers,
                          int64_t capacity, int64_t *out_ids, float *out_scores, int32_t *gained, void *stream)
{
    const char *who = "mdx_knn_reverse_merge";
    MDX_CHECK_ARG(offsets && offers && out_ids && out_scores && gained, "%s: NULL pointer", who);
    if (int rc = check_lists(who, ids, scores, n, k)) return rc;
    MDX_CHECK_ARG(capacity >= 1, "%s: capacity=%lld must be >= 1", who, (long long)capacity);
    MDX_CHECK_ARG(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)offers & 7) == 0 && ((uintptr_t)out_ids & 7) == 0,
                  "%s: offsets, offers and out_ids must be 8-byte aligned", who);
    MDX_CHECK_ARG(((uintptr_t)out_scores & 3) == 0 && ((uintptr_t)gained & 3) == 0, "%s: out_scores and gained must be 4-byte aligned", who);
    hipLaunchKernelGGL(reverse_merge_kernel, dim3((unsigned)n), dim3(KR_TILE), 0, (hipStream_t)stream, ids, scores, n, (int)k, offsets,
                       (const uint2 *)offers, capacity, out_ids, out_scores, gained);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
