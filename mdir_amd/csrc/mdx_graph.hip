// The graph index (include/mdx_graph.h): beam search over a fixed-degree neighbour graph, and the detour counts of its build.
//
//   graph_search_kernel    one workgroup per query.  The centred query stays in LDS; the beam is the head of a sort buffer of P words,
//                          word = desc_key << 32 | id << 1 | unexpanded.  A round (a chunk of the seeds, or the graph rows of a step's
//                          parents) filters its candidates through a table of rows already scored, runs one chain per lane on the
//                          survivors (graph_score_f32: the chain of mdx_exact.h, the bits of mdx_scores), sorts beam and survivors
//                          together and drops the copies of an id, which the sort has made adjacent.  The table only saves chains
//                          (the proof is in the header); the adjacency test is what keeps duplicates out of the beam.
//   graph_detours_kernel   one workgroup per row: the row's list in an LDS table id -> rank, the lists of its neighbours streamed
//                          through it.  Integers only.
#include "mdx_exact.h"

namespace mdx {
namespace {

constexpr int GS_THREADS = 256;
constexpr uint32_t GS_EMPTY = 0xFFFFFFFFu;        // no key: keys are ids below 2^31
constexpr uint64_t GS_PAD = ~0ull;                // sorts after every word of a row (ids stay below 2^31 - 1)
constexpr int GS_PROBES = 32;                     // an insert that finds no free slot this soon is given up
constexpr int GS_MISC = 16;                       // ints: 0 survivors, 1 keys in the table, 2 parents, 4..7 wave totals, 8..15 the parents

// element k of query q (x_q = q - center, one fp32 subtraction), 0 beyond d: mdx_rescore's
__device__ __forceinline__ float graph_query_elem(const float *queries, int64_t nq, int64_t d, int qlayout, const float *center, int64_t q,
                                                  int64_t k)
{
    if (k >= d) return 0.f;
    const float x = qlayout == MDX_ROW_MAJOR ? queries[q * d + k] : queries[k * nq + q];
    return center ? x - center[k] : x;
}

// the score of a key of desc_key (a chain's score is never -0); the NaN key gives the quiet NaN
__device__ __forceinline__ float key_score(uint32_t key)
{
    if (key == 0xFFFFFFFFu) return __builtin_nanf("");
    uint32_t u = ~key;
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}

// The scoring step: the exact chain of row `id` (0 <= id < n) against the query in LDS (d_pad floats, zeros beyond d).  One lane, one
// chain; the row is read in place.  A scorer on other codes replaces this function and nothing else.
__device__ __forceinline__ float graph_score_f32(const float *__restrict__ rows, int64_t id, int64_t ld, int64_t d, int64_t d_pad, bool vec,
                                                 const float *qs)
{
    const float *p = rows + id * ld;
    float acc = 0.f;
    int64_t k = 0;
    if (vec) {
        for (; k + 16 <= d; k += 16) {                             // four pieces in flight ahead of their links
            const f32x4 x0 = *(const f32x4 *)(p + k), x1 = *(const f32x4 *)(p + k + 4);
            const f32x4 x2 = *(const f32x4 *)(p + k + 8), x3 = *(const f32x4 *)(p + k + 12);
            acc = chain_step4(acc, *(const f32x4 *)(qs + k), x0);
            acc = chain_step4(acc, *(const f32x4 *)(qs + k + 4), x1);
            acc = chain_step4(acc, *(const f32x4 *)(qs + k + 8), x2);
            acc = chain_step4(acc, *(const f32x4 *)(qs + k + 12), x3);
        }
    }
    for (; k < d_pad; k += 4) acc = chain_step4(acc, *(const f32x4 *)(qs + k), row_piece(rows, id, ld, d, k, vec));
    return acc;
}

// true: `key` was not in the table (and is now, if a slot was free within GS_PROBES)
__device__ __forceinline__ bool table_insert(uint32_t *table, uint32_t mask, int shift, uint32_t key, int32_t *held)
{
    uint32_t s = (key * 2654435761u) >> shift;
    for (int p = 0; p < GS_PROBES; ++p) {
        const uint32_t old = atomicCAS(&table[s], GS_EMPTY, key);
        if (old == GS_EMPTY) {
            atomicAdd(held, 1);
            return true;
        }
        if (old == key) return false;
        s = (s + 1) & mask;
    }
    return true;
}

// P: a power of two >= L + W * R and >= 2; the dynamic LDS is laid out as the header says
__global__ __launch_bounds__(GS_THREADS) void graph_search_kernel(const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld,
                                                                  const int32_t *__restrict__ graph, int R,
                                                                  const float *__restrict__ queries, int64_t nq, int qlayout,
                                                                  const float *__restrict__ center, const int64_t *__restrict__ seeds,
                                                                  int S, int k, int L, int W, int64_t T, int table_bits, int P, bool vec,
                                                                  int64_t *__restrict__ ids, float *__restrict__ scores,
                                                                  int32_t *__restrict__ steps_out, int32_t *__restrict__ scored_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char graph_lds[];
    const int64_t q = blockIdx.x, d_pad = chain_pad(d);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int C = P - L;                                           // candidates of one round, >= W * R
    const uint32_t slots = 1u << table_bits, mask = slots - 1;
    const int shift = 32 - table_bits;
    float *qs = (float *)graph_lds;
    uint64_t *word = (uint64_t *)(graph_lds + 4 * d_pad);
    int32_t *cid = (int32_t *)(word + P);                          // the round's candidates as they come
    int32_t *sid = cid + C;                                        // those that are scored
    uint32_t *table = (uint32_t *)(sid + C);
    int32_t *misc = (int32_t *)(table + slots);

    for (int64_t kk = tid; kk < d_pad; kk += GS_THREADS) qs[kk] = graph_query_elem(queries, nq, d, qlayout, center, q, kk);
    for (int i = tid; i < P; i += GS_THREADS) word[i] = GS_PAD;
    for (uint32_t s = tid; s < slots; s += GS_THREADS) table[s] = GS_EMPTY;
    if (tid < GS_MISC) misc[tid] = 0;
    __syncthreads();

    int32_t scored = 0;
    // one round: cid[0 .. nc) -> the beam.  Called by all threads, after a barrier that follows the writes of cid.
    auto round = [&](int nc) {
        // one thread reads the count and the barrier hands its decision to all: no wave can see the count after another wave's
        // inserts of this round, which start behind this barrier
        if (__syncthreads_or(tid == 0 && (uint32_t)misc[1] > slots / 2)) {
            for (uint32_t s = tid; s < slots; s += GS_THREADS) table[s] = GS_EMPTY;
            if (tid == 0) misc[1] = 0;
            __syncthreads();
        }
        for (int c = tid; c < nc; c += GS_THREADS) {
            const int32_t id = cid[c];
            if (id < 0 || (int64_t)id >= n) continue;
            if (table_insert(table, mask, shift, (uint32_t)id, &misc[1])) sid[atomicAdd(&misc[0], 1)] = id;
        }
        __syncthreads();
        const int ns = misc[0];
        for (int c = tid; c < ns; c += GS_THREADS) {
            const int32_t id = sid[c];
            const float s = graph_score_f32(rows, id, ld, d, d_pad, vec, qs);
            word[L + c] = ((uint64_t)desc_key(s) << 32) | ((uint32_t)id << 1) | 1u;
        }
        for (int c = ns + tid; c < C; c += GS_THREADS) word[L + c] = GS_PAD;
        __syncthreads();
        if (tid == 0) misc[0] = 0;
        scored += ns;
        if (ns == 0) return;
        // ascending (desc_key, id, unexpanded): the copies of an id are adjacent, the expanded one first
        for (int size = 2; size <= P; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = tid; i < P / 2; i += GS_THREADS) {
                    const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const uint64_t a = word[lo], b = word[hi];
                    if ((b < a) == up) {
                        word[lo] = b;
                        word[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        // thread t owns words 4 t .. 4 t + 3 (P <= 1024): drop every word whose id is its predecessor's
        uint64_t w[4];
        bool keep[4];
        int mine = 0, dup = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * tid + e;
            w[e] = i < P ? word[i] : GS_PAD;
            const uint64_t before = (i > 0 && i < P) ? word[i - 1] : GS_PAD;
            const bool copy = i > 0 && w[e] != GS_PAD && (w[e] >> 1) == (before >> 1);
            keep[e] = w[e] != GS_PAD && !copy;
            dup |= copy;
            mine += keep[e];
        }
        if (!__syncthreads_or(dup)) return;
        const int incl = (int)wave_inclusive_sum((uint32_t)mine);
        if (lane == 63) misc[4 + wave] = incl;
        __syncthreads();
        int pos = incl - mine;
        for (int v = 0; v < wave; ++v) pos += misc[4 + v];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * tid + e < P) word[4 * tid + e] = GS_PAD;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (keep[e]) word[pos++] = w[e];
        __syncthreads();
    };

    for (int base = 0; base < S; base += C) {
        const int nc = S - base < C ? S - base : C;
        for (int c = tid; c < nc; c += GS_THREADS) {
            const int64_t id = seeds[q * S + base + c];
            cid[c] = (id >= 0 && id < n) ? (int32_t)id : -1;
        }
        __syncthreads();
        round(nc);
    }

    int32_t steps = 0;
    while ((int64_t)steps < T) {
        if (wave == 0) {                                           // the first W unexpanded entries, in beam order
            int found = 0;
            for (int b = 0; b < L && found < W; b += 64) {
                const int i = b + lane;
                const uint64_t w = i < L ? word[i] : GS_PAD;
                const bool open = w != GS_PAD && (w & 1);
                const uint64_t m = __ballot(open);
                const int at = found + __popcll(m & ((1ull << lane) - 1));
                if (open && at < W) {
                    misc[8 + at] = (int32_t)((uint32_t)w >> 1);
                    word[i] = w & ~1ull;
                }
                found += __popcll(m);
            }
            if (lane == 0) misc[2] = found < W ? found : W;
        }
        __syncthreads();
        const int np = misc[2];
        if (np == 0) break;
        ++steps;
        for (int c = tid; c < np * R; c += GS_THREADS) cid[c] = graph[(int64_t)misc[8 + c / R] * R + c % R];
        __syncthreads();
        round(np * R);
    }

    for (int i = tid; i < k; i += GS_THREADS) {
        const uint64_t w = word[i];
        ids[q * k + i] = w == GS_PAD ? -1 : (int64_t)((uint32_t)w >> 1);
        scores[q * k + i] = w == GS_PAD ? __builtin_nanf("") : key_score((uint32_t)(w >> 32));
    }
    if (tid == 0) {
        steps_out[q] = steps;
        scored_out[q] = scored;
    }
}

constexpr int GD_THREADS = 256;
constexpr int GD_SLOTS = 2 * MDX_GRAPH_MAX_K0;                     // at most half full

__device__ __forceinline__ uint32_t detour_slot(uint32_t key) { return (key * 2654435761u) >> 24; }
static_assert(GD_SLOTS == 256, "detour_slot keeps 8 bits");

__global__ __launch_bounds__(GD_THREADS) void graph_detours_kernel(const int64_t *__restrict__ lists, int64_t n, int K0,
                                                                   int32_t *__restrict__ detours)
{
    __shared__ uint32_t keys[GD_SLOTS];
    __shared__ uint8_t where[GD_SLOTS];
    __shared__ int32_t count[MDX_GRAPH_MAX_K0];
    __shared__ int64_t mine[MDX_GRAPH_MAX_K0];
    const int64_t i = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    keys[tid] = GS_EMPTY;
    if (tid < MDX_GRAPH_MAX_K0) {
        const int64_t id = tid < K0 ? lists[i * K0 + tid] : -1;
        mine[tid] = (id >= 0 && id < n) ? id : -1;                 // an id outside [0, n) is never dereferenced
        count[tid] = 0;
    }
    __syncthreads();
    if (tid < K0 && mine[tid] >= 0) {
        const uint32_t key = (uint32_t)mine[tid];
        uint32_t s = detour_slot(key);
        for (;;) {
            const uint32_t old = atomicCAS(&keys[s], GS_EMPTY, key);
            if (old == GS_EMPTY) { where[s] = (uint8_t)tid; break; }
            if (old == key) break;                                 // a repeated id (outside the contract): the first to arrive stays
            s = (s + 1) & (GD_SLOTS - 1);
        }
    }
    __syncthreads();
    for (int t = wave; t < K0; t += GD_THREADS / 64) {             // wave-uniform
        const int64_t a = mine[t];
        if (a < 0) continue;
        for (int r = lane; r < K0; r += 64) {
            const int64_t b = lists[a * K0 + r];
            if (b < 0 || b >= n) continue;
            const uint32_t key = (uint32_t)b;
            uint32_t s = detour_slot(key);
            for (;;) {
                const uint32_t have = keys[s];
                if (have == GS_EMPTY) break;
                if (have == key) {
                    const int j = where[s];
                    if (t < j && r < j) atomicAdd(&count[j], 1);
                    break;
                }
                s = (s + 1) & (GD_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    if (tid < K0) detours[i * K0 + tid] = mine[tid] >= 0 ? count[tid] : K0;
}

int64_t graph_search_lds(int64_t d, int64_t L, int64_t P, int table_bits)
{
    return 4 * round_up(d, 64) + 8 * P + 8 * (P - L) + 4 * ((int64_t)1 << table_bits) + 4 * GS_MISC;
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_graph_search(const float *rows, int64_t n, int64_t d, int64_t ld, const int32_t *graph, int64_t R, const float *queries, int64_t nq,
                     int qlayout, const float *center, const int64_t *seeds, int64_t S, int64_t k, int64_t L, int64_t W, int64_t T,
                     int table_bits, int64_t *ids, float *scores, int32_t *steps, int32_t *scored, void *stream)
{
    const char *who = "mdx_graph_search";
    const int64_t top = (int64_t)1 << 31;
    MDX_CHECK_ARG(rows && graph && queries && seeds && ids && scores && steps && scored, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && n < top && nq >= 1 && nq < top, "%s: n=%lld and nq=%lld must be in [1, 2^31)", who, (long long)n, (long long)nq);
    MDX_CHECK_ARG(d >= 1 && d <= MDX_GRAPH_MAX_D, "%s: d=%lld must be in [1, %d]", who, (long long)d, MDX_GRAPH_MAX_D);
    MDX_CHECK_ARG(ld >= d, "%s: ld=%lld < d=%lld", who, (long long)ld, (long long)d);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "%s: qlayout %d", who, qlayout);
    MDX_CHECK_ARG(R >= 1 && R <= MDX_GRAPH_MAX_DEGREE, "%s: R=%lld must be in [1, %d]", who, (long long)R, MDX_GRAPH_MAX_DEGREE);
    MDX_CHECK_ARG(S >= 1 && S <= MDX_GRAPH_MAX_SEEDS, "%s: S=%lld must be in [1, %d]", who, (long long)S, MDX_GRAPH_MAX_SEEDS);
    MDX_CHECK_ARG(L >= 1 && L <= MDX_GRAPH_MAX_BEAM, "%s: L=%lld must be in [1, %d]", who, (long long)L, MDX_GRAPH_MAX_BEAM);
    MDX_CHECK_ARG(k >= 1 && k <= L, "%s: k=%lld must be in [1, L=%lld]", who, (long long)k, (long long)L);
    MDX_CHECK_ARG(W >= 1 && W <= MDX_GRAPH_MAX_WIDTH, "%s: W=%lld must be in [1, %d]", who, (long long)W, MDX_GRAPH_MAX_WIDTH);
    static_assert(MDX_GRAPH_MAX_WIDTH * MDX_GRAPH_MAX_DEGREE == MDX_GRAPH_MAX_CANDIDATES, "W * R <= MDX_GRAPH_MAX_CANDIDATES follows");
    MDX_CHECK_ARG(T >= 1, "%s: T=%lld must be >= 1", who, (long long)T);
    MDX_CHECK_ARG(table_bits == 0 || (table_bits >= 8 && table_bits <= 14), "%s: table_bits=%d must be 0 or in [8, 14]", who, table_bits);
    MDX_CHECK_ARG((((uintptr_t)seeds | (uintptr_t)ids) & 7) == 0, "%s: seeds and ids must be 8-byte aligned", who);
    MDX_CHECK_ARG((((uintptr_t)rows | (uintptr_t)graph | (uintptr_t)queries | (uintptr_t)center | (uintptr_t)scores | (uintptr_t)steps |
                    (uintptr_t)scored) & 3) == 0,
                  "%s: rows, graph, queries, center, scores, steps and scored must be 4-byte aligned", who);
    int64_t P = 2;
    while (P < L + W * R) P <<= 1;                                     // <= 1024
    if (table_bits == 0) {
        table_bits = 8;
        while (table_bits < 13 && ((int64_t)1 << table_bits) < 8 * (L + W * R)) ++table_bits;
    }
    // more than 64 KiB of dynamic LDS needs an opt-in per kernel and device: done once, not on every launch (as mdx_lists_pq.hip)
    static bool opted[64];
    int dev = 0;
    MDX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !opted[dev]) {
        MDX_HIP(hipFuncSetAttribute((const void *)graph_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)graph_search_lds(MDX_GRAPH_MAX_D, 1, 1024, 14)));
        if (dev >= 0 && dev < 64) opted[dev] = true;
    }
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;       // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(graph_search_kernel, dim3((unsigned)nq), dim3(GS_THREADS), (unsigned)graph_search_lds(d, L, P, table_bits),
                       (hipStream_t)stream, rows, n, d, ld, graph, (int)R, queries, nq, qlayout, center, seeds, (int)S, (int)k, (int)L, (int)W,
                       T, table_bits, (int)P, vec, ids, scores, steps, scored);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_graph_detours(const int64_t *lists, int64_t n, int64_t K0, int32_t *detours, void *stream)
{
    const char *who = "mdx_graph_detours";
    MDX_CHECK_ARG(lists && detours, "%s: NULL lists or detours", who);
    MDX_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "%s: n=%lld must be in [1, 2^31)", who, (long long)n);
    MDX_CHECK_ARG(K0 >= 1 && K0 <= MDX_GRAPH_MAX_K0, "%s: K0=%lld must be in [1, %d]", who, (long long)K0, MDX_GRAPH_MAX_K0);
    MDX_CHECK_ARG(((uintptr_t)lists & 7) == 0 && ((uintptr_t)detours & 3) == 0, "%s: lists must be 8-byte aligned, detours 4-byte", who);
    hipLaunchKernelGGL(graph_detours_kernel, dim3((unsigned)n), dim3(GD_THREADS), 0, (hipStream_t)stream, lists, n, (int)K0, detours);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
