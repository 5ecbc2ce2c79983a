// The inverted file (include/mdx_ivf.h): the plan of a batch of probes, the list-major exact scan and the per-query selection.
//
//   plan      four small launches: per query the prefix of its probes' list sizes, per list the entries (query, probe) that probe
//             it (count, scan, fill with integer atomics) and the prefix over work items.
//   scan      one workgroup per (tile of 64 members of a list, group of up to 8 entries).  The loader, the stage arithmetic and the
//             four-link chain step are those of mdx_exact.h, the padded tile is rescore_kernel's (mdx_rescore.hip): the rows go to LDS
//             once per stage and serve the whole group, wave w runs the chains of entries w and w + 4.
//   select    one workgroup per query: everything into LDS up to 4096 candidates, a radix select over (order key, id) above that,
//             then a bitonic sort of the chosen pairs.
//
// The sections of the plan, the list search and the slot fill of a work item, the checks of the shared sizes and the pad launch of
// the scan are in mdx_ivf_plan.h, which the int8 scan of the same work items (mdx_lists_i8.hip) includes too.
#include "mdx_exact.h"
#include "mdx_ivf_plan.h"

namespace mdx {
namespace {

constexpr int KC = 256;                   // k per stage: one 1-KiB piece of every row
constexpr int LD = KC + 4;                  // floats per LDS row: lane r reads row r with ds_read_b128, banks 4r .. 4r+3 (mod 64)
constexpr int ROWS_PER_WAVE = TC / 4;
constexpr int QPW = G / 4;                  // entries per wave
constexpr int SEL_THREADS = 1024;
constexpr int SEL_MAX = MDX_RESCORE_MAX_K;

static_assert(TC == 64 && G % 4 == 0 && G <= 64, "one member per lane, the entries dealt to four waves");

// ------------------------------------------------------------------------------------------------------------------ plan

__global__ __launch_bounds__(256) void plan_zero_kernel(unsigned long long *cursor, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) cursor[i] = 0;
}

// one thread per query: the prefix of its probes' list sizes, one count per valid probe
__global__ __launch_bounds__(256) void plan_query_kernel(const int64_t *__restrict__ probes, int64_t nq, int64_t nprobe,
                                                         const int64_t *__restrict__ offsets, int64_t K, int64_t m, int64_t cap,
                                                         int64_t *__restrict__ base, int64_t *__restrict__ count, unsigned long long *counts)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int64_t run = 0;
    for (int64_t p = 0; p < nprobe; ++p) {
        const int64_t l = probes[q * nprobe + p];
        if (l < 0 || l >= K) {
            base[q * nprobe + p] = -1;
            continue;
        }
        base[q * nprobe + p] = run;
        run += list_size(offsets, l, m);
        atomicAdd(&counts[l], 1ull);
    }
    count[q] = run < cap ? run : cap;
}

// one workgroup: first[l] = the entries of the lists before l, item[l] = their work items.  Thread t owns a run of ceil(K / 1024)
// lists; the 1024 run totals are scanned in LDS (segbase_kernel of mdx_kmeans.hip, for two sums at once)
__global__ __launch_bounds__(1024) void plan_scan_kernel(const int64_t *__restrict__ offsets, int64_t K, int64_t m,
                                                         const unsigned long long *__restrict__ counts, int64_t *__restrict__ first,
                                                         int64_t *__restrict__ item)
{
    __shared__ int64_t she[1024], shi[1024];
    const int t = threadIdx.x;
    const int64_t per = (K + 1023) / 1024;
    const int64_t c0 = t * per < K ? t * per : K, c1 = c0 + per < K ? c0 + per : K;
    auto items_of = [&](int64_t l) {
        const int64_t e = (int64_t)counts[l];
        return ((list_size(offsets, l, m) + TC - 1) / TC) * ((e + G - 1) / G);
    };
    int64_t le = 0, li = 0;
    for (int64_t l = c0; l < c1; ++l) {
        le += (int64_t)counts[l];
        li += items_of(l);
    }
    she[t] = le;
    shi[t] = li;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t ve = t >= o ? she[t - o] : 0, vi = t >= o ? shi[t - o] : 0;
        __syncthreads();
        she[t] += ve;
        shi[t] += vi;
        __syncthreads();
    }
    int64_t re = she[t] - le, ri = shi[t] - li;
    for (int64_t l = c0; l < c1; ++l) {
        first[l] = re;
        item[l] = ri;
        re += (int64_t)counts[l];
        ri += items_of(l);
    }
    if (t == 1023) {
        first[K] = she[1023];
        item[K] = shi[1023];
    }
}

// one thread per (query, probe): its place among the entries of its list
__global__ __launch_bounds__(256) void plan_fill_kernel(const int64_t *__restrict__ probes, int64_t entries, int64_t K,
                                                        const int64_t *__restrict__ first, unsigned long long *cursor,
                                                        int64_t *__restrict__ entry)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const int64_t l = probes[e];
    if (l < 0 || l >= K) return;
    const int64_t pos = first[l] + (int64_t)atomicAdd(&cursor[l], 1ull);
    if (pos >= 0 && pos < entries) entry[pos] = e;
}

// ------------------------------------------------------------------------------------------------------------------ scan

// element k of query q (x_q = q - center, one fp32 subtraction), 0 beyond d or without a query
__device__ __forceinline__ float query_elem(const float *queries, int64_t nq, int64_t d, int qlayout, const float *center, int64_t q,
                                            int64_t k)
{
    if (q < 0 || k >= d) return 0.f;
    const float x = qlayout == MDX_ROW_MAJOR ? queries[q * d + k] : queries[k * nq + q];
    return center ? x - center[k] : x;
}

__global__ __launch_bounds__(256) void ivf_scan_kernel(const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld,
                                                       const int64_t *__restrict__ members, int64_t m,
                                                       const int64_t *__restrict__ offsets, int64_t K,
                                                       const float *__restrict__ queries, int64_t nq, int qlayout,
                                                       const float *__restrict__ center, int64_t nprobe,
                                                       const int64_t *__restrict__ base, const int64_t *__restrict__ first,
                                                       const int64_t *__restrict__ item, const int64_t *__restrict__ entry, int64_t cap,
                                                       bool vec, float *__restrict__ cand_scores, int64_t *__restrict__ cand_ids)
{
    __shared__ __attribute__((aligned(16))) float tile[TC * LD];
    __shared__ __attribute__((aligned(16))) float qs[G * KC];
    __shared__ int64_t rid[TC], gid[TC];        // the member's row, -1 where there is nothing to read; the member id as given
    __shared__ int64_t qidx[G], qcol[G];        // the entry's query, -1 without one; the column of the tile's first member
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // everything up to the first barrier is uniform over the workgroup: it leaves as a whole
    if (g >= item[K]) return;                                   // the item does not exist
    const int64_t l = item_list(item, K, g), local = g - item[l];
    int64_t start, size;
    list_extent(offsets, l, m, start, size);
    const int64_t tiles = (size + TC - 1) / TC;
    if (item[l] < 0 || local < 0 || tiles < 1) return;
    const int64_t t = local % tiles, grp = local / tiles;       // consecutive workgroups share the tile's rows
    const int64_t entries = nq * nprobe;
    const int64_t f0 = clamp_to(first[l], entries), f1 = clamp_to(first[l + 1], entries);
    const int64_t e0 = f0 + grp * G;
    if (e0 >= f1) return;
    const int ne = (int)(f1 - e0 < G ? f1 - e0 : G);
    const int in_tile = (int)(size - t * TC < TC ? size - t * TC : TC);
    if (tid < TC) {
        const int64_t id = tid < in_tile ? members[start + t * TC + tid] : -1;
        gid[tid] = id;
        rid[tid] = (tid < in_tile && id >= 0 && id < n) ? id : -1;      // an id outside [0, n) is never dereferenced
    }
    item_slots(tid, t, e0, ne, entry, base, nq, nprobe, qidx, qcol);
    __syncthreads();
    const int64_t d_pad = chain_pad(d), stages = chain_stages(d_pad, KC);
    int64_t my_ids[ROWS_PER_WAVE], my_q[G];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) my_ids[r] = rid[wave * ROWS_PER_WAVE + r];
#pragma unroll
    for (int j = 0; j < G; ++j) my_q[j] = qidx[j];

    f32x4 reg[ROWS_PER_WAVE];
    float qreg[G];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) reg[r] = row_piece(rows, my_ids[r], ld, d, k0 + 4 * lane, vec);
#pragma unroll
        for (int j = 0; j < G; ++j) qreg[j] = query_elem(queries, nq, d, qlayout, center, my_q[j], k0 + tid);
    };
    auto put = [&]() {
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) *(f32x4 *)(tile + (wave * ROWS_PER_WAVE + r) * LD + 4 * lane) = reg[r];
#pragma unroll
        for (int j = 0; j < G; ++j) qs[j * KC + tid] = qreg[j];
    };

    float acc[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) acc[i] = 0.f;
    fetch(0);
    put();
    __syncthreads();
    for (int64_t s = 0; s < stages; ++s) {
        const int64_t k0 = s * KC;
        if (s + 1 < stages) fetch(k0 + KC);                       // in flight during the chains
        if (wave < ne) {
            const int kend = chain_kend(d_pad, k0, KC);
            const float *x = tile + lane * LD;
            for (int kk = 0; kk < kend; kk += 4) {
                const f32x4 xv = *(const f32x4 *)(x + kk);
#pragma unroll
                for (int i = 0; i < QPW; ++i) {
                    const f32x4 qv = *(const f32x4 *)(qs + (wave + 4 * i) * KC + kk);
                    acc[i] = chain_step4(acc[i], qv, xv);
                }
            }
        }
        if (s + 1 < stages) {
            __syncthreads();                                      // the chains are done with the tile
            put();
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
        const int slot = wave + 4 * i;
        if (slot >= ne || qidx[slot] < 0 || lane >= in_tile) continue;
        const int64_t col = qcol[slot] + lane;
        if (col >= cap) continue;                                 // beyond the candidate row: the candidate does not exist
        cand_scores[qidx[slot] * cap + col] = rid[lane] >= 0 ? acc[i] : __builtin_nanf("");
        cand_ids[qidx[slot] * cap + col] = gid[lane];
    }
}

// ------------------------------------------------------------------------------------------------------------------ select

__device__ __forceinline__ uint64_t id_key(int64_t id) { return (uint64_t)id ^ (1ull << 63); }     // ascending as signed ids

// (order key, id) of pair a before that of pair b
__device__ __forceinline__ bool pair_before(float sa, int64_t ia, float sb, int64_t ib)
{
    const uint32_t ka = desc_key(sa), kb = desc_key(sb);
    return ka != kb ? ka < kb : ia < ib;
}

// thread 0: the bin in which the `need`-th smallest of the histogram lies; need becomes its rank inside that bin
__device__ __forceinline__ void pick_bin(const uint32_t *hist, int64_t *need, uint32_t *bin, uint32_t *in_bin)
{
    int64_t cum = 0;
    int b = 0;
    for (; b < 255; ++b) {
        if (cum + hist[b] >= *need) break;
        cum += hist[b];
    }
    *need -= cum;
    *bin = (uint32_t)b;
    *in_bin = hist[b];
}

__global__ __launch_bounds__(SEL_THREADS) void ivf_select_kernel(const float *__restrict__ cand_scores, const int64_t *__restrict__ cand_ids,
                                                                  int64_t cap, const int64_t *__restrict__ count, int64_t k,
                                                                  int64_t *__restrict__ out_ids, float *__restrict__ out_scores)
{
    __shared__ float ssc[SEL_MAX];
    __shared__ int64_t sid[SEL_MAX];
    __shared__ uint32_t hist[256];
    __shared__ int64_t need_s;
    __shared__ uint32_t bin_s, in_bin_s, taken_s, equal_s;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const float *sc = cand_scores + q * cap;
    const int64_t *ids = cand_ids + q * cap;
    const int64_t have = clamp_to(count[q], cap);
    int total;
    if (have <= SEL_MAX) {
        total = (int)have;
        for (int i = tid; i < total; i += SEL_THREADS) {
            ssc[i] = sc[i];
            sid[i] = ids[i];
        }
    } else {
        // the order key of position k (k <= SEL_MAX < have): four passes of 8 bits, the most significant first
        uint32_t prefix = 0, mask = 0;
        if (tid == 0) need_s = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < have; i += SEL_THREADS) {
                const uint32_t key = desc_key(sc[i]);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int64_t need = need_s;
                pick_bin(hist, &need, &bin_s, &in_bin_s);
                need_s = need;
            }
            __syncthreads();
            prefix |= bin_s << shift;
            mask |= 255u << shift;
        }
        const uint32_t T = prefix;                   // need_s of the in_bin_s candidates with this key are wanted
        // more of them than wanted: the id of the last one taken, eight passes over the ids of that key
        const bool all = (int64_t)in_bin_s <= need_s;
        uint64_t iprefix = 0, imask = 0;
        if (!all) {
            for (int shift = 56; shift >= 0; shift -= 8) {
                __syncthreads();
                if (tid < 256) hist[tid] = 0;
                __syncthreads();
                for (int64_t i = tid; i < have; i += SEL_THREADS) {
                    if (desc_key(sc[i]) != T) continue;
                    const uint64_t ik = id_key(ids[i]);
                    if ((ik & imask) == iprefix) atomicAdd(&hist[(ik >> shift) & 255u], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    int64_t need = need_s;
                    pick_bin(hist, &need, &bin_s, &in_bin_s);
                    need_s = need;
                }
                __syncthreads();
                iprefix |= (uint64_t)bin_s << shift;
                imask |= 255ull << shift;
            }
        }
        // collect: smaller keys, key T with smaller ids, and need_s of the pairs (T, that id) -- equal pairs of one row
        __syncthreads();
        if (tid == 0) taken_s = equal_s = 0;
        __syncthreads();
        const int64_t need_equal = need_s;
        for (int64_t i = tid; i < have; i += SEL_THREADS) {
            const float s = sc[i];
            const uint32_t key = desc_key(s);
            if (key > T) continue;
            const int64_t id = ids[i];
            if (key == T && !all) {
                const uint64_t ik = id_key(id);
                if (ik > iprefix) continue;
                if (ik == iprefix && (int64_t)atomicAdd(&equal_s, 1u) >= need_equal) continue;
            }
            const uint32_t pos = atomicAdd(&taken_s, 1u);
            if (pos < (uint32_t)SEL_MAX) {
                ssc[pos] = s;
                sid[pos] = id;
            }
        }
        __syncthreads();
        total = (int)(taken_s < (uint32_t)SEL_MAX ? taken_s : (uint32_t)SEL_MAX);
    }
    int P = 2;
    while (P < total) P <<= 1;
    for (int i = total + tid; i < P; i += SEL_THREADS) {      // pads sort behind every pair
        ssc[i] = __builtin_nanf("");
        sid[i] = INT64_MAX;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += SEL_THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const float sa = ssc[lo], sb = ssc[hi];
                const int64_t ia = sid[lo], ib = sid[hi];
                if (pair_before(sb, ib, sa, ia) == up) {
                    ssc[lo] = sb;
                    ssc[hi] = sa;
                    sid[lo] = ib;
                    sid[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (int64_t i = tid; i < k; i += SEL_THREADS) {
        out_ids[q * k + i] = i < total ? sid[i] : -1;
        out_scores[q * k + i] = i < total ? ssc[i] : __builtin_nanf("");
    }
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_ivf_plan_workspace(int64_t nq, int64_t nprobe, int64_t K)
{
    if (nq < 1 || nprobe < 1 || K < 1 || nq >= LIMIT || K >= LIMIT || nprobe > K || nq * nprobe >= LIMIT) return 0;
    return plan_bytes_of(nq, nprobe, K);
}

int mdx_ivf_plan(const int64_t *probes, int64_t nq, int64_t nprobe, const int64_t *offsets, int64_t K, int64_t m, int64_t cap,
                 void *plan, int64_t plan_bytes, void *stream)
{
    const char *who = "mdx_ivf_plan";
    MDX_CHECK_ARG(probes && offsets, "%s: NULL pointer", who);
    MDX_CHECK_ARG(m >= 1 && m < LIMIT, "%s: m=%lld must be in [1, 2^31)", who, (long long)m);
    if (int rc = check_plan(who, nq, nprobe, K, plan, plan_bytes)) return rc;
    if (int rc = check_cap(who, nq, cap)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Plan v = carve(plan, nq, nprobe, K);
    hipLaunchKernelGGL(plan_zero_kernel, dim3((unsigned)ceil_div(2 * K, 256)), dim3(256), 0, s, v.cursor, 2 * K);
    hipLaunchKernelGGL(plan_query_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, s, probes, nq, nprobe, offsets, K, m, cap, v.base,
                       v.count, v.cursor);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, s, offsets, K, m, (const unsigned long long *)v.cursor, v.first, v.item);
    hipLaunchKernelGGL(plan_fill_kernel, dim3((unsigned)ceil_div(nq * nprobe, 256)), dim3(256), 0, s, probes, nq * nprobe, K,
                       (const int64_t *)v.first, v.cursor + K, v.entry);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_ivf_scan(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, int64_t m, const int64_t *offsets,
                 int64_t K, const float *queries, int64_t nq, int qlayout, const float *center, int64_t nprobe, const void *plan,
                 int64_t plan_bytes, int64_t cap, int64_t items, float *cand_scores, int64_t *cand_ids, void *stream)
{
    const char *who = "mdx_ivf_scan";
    MDX_CHECK_ARG(rows && members && offsets && queries && cand_scores && cand_ids, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && d >= 1 && m >= 1 && n < LIMIT && d < LIMIT && m < LIMIT, "%s: n=%lld d=%lld m=%lld must be in [1, 2^31)", who,
                  (long long)n, (long long)d, (long long)m);
    MDX_CHECK_ARG(ld >= d, "%s: ld=%lld < d=%lld", who, (long long)ld, (long long)d);
    MDX_CHECK_ARG(ld <= INT64_MAX / n, "%s: n * ld overflows", who);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "%s: qlayout %d", who, qlayout);
    MDX_CHECK_ARG(items >= 1 && items < LIMIT, "%s: items=%lld must be in [1, 2^31)", who, (long long)items);
    if (int rc = check_plan(who, nq, nprobe, K, plan, plan_bytes)) return rc;
    if (int rc = check_cap(who, nq, cap)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Plan v = carve(plan, nq, nprobe, K);
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;       // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)items), dim3(256), 0, s, rows, n, d, ld, members, m, offsets, K, queries, nq, qlayout,
                       center, nprobe, (const int64_t *)v.base, (const int64_t *)v.first, (const int64_t *)v.item, (const int64_t *)v.entry,
                       cap, vec, cand_scores, cand_ids);
    launch_pad(v, nq, cap, cand_scores, cand_ids, s);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_ivf_select(const float *cand_scores, const int64_t *cand_ids, int64_t nq, int64_t cap, int64_t nprobe, int64_t K,
                   const void *plan, int64_t plan_bytes, int64_t k, int64_t *out_ids, float *out_scores, void *stream)
{
    const char *who = "mdx_ivf_select";
    MDX_CHECK_ARG(cand_scores && cand_ids && out_ids && out_scores, "%s: NULL pointer", who);
    MDX_CHECK_ARG(k >= 1 && k <= MDX_RESCORE_MAX_K, "%s: k=%lld must be in [1, %d]", who, (long long)k, MDX_RESCORE_MAX_K);
    if (int rc = check_plan(who, nq, nprobe, K, plan, plan_bytes)) return rc;
    if (int rc = check_cap(who, nq, cap)) return rc;
    const Plan v = carve(plan, nq, nprobe, K);
    hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)nq), dim3(SEL_THREADS), 0, (hipStream_t)stream, cand_scores, cand_ids, cap,
                       (const int64_t *)v.count, k, out_ids, out_scores);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
