// Near-duplicate groups: the connected components of the exact self-join (include/mdx.h, "near-duplicate groups").
//
//   groups_init_kernel    parent[t][i] = i, status = 0.
//   union_pairs_kernel    one workgroup per 64 candidates (i << 32 | j) of the join kernel: exact_kernel's tile plan (mdx_join.hip) --
//                         the row pieces of both ends staged in LDS 128 k at a time, wave 0 running the chains of mdx_exact.h, lane =
//                         candidate -- and then, instead of a score, unite(i, j) in every level whose threshold the chain reaches.
//                         Before anything is staged wave 0 drops the pairs whose ends already share a root in the level of the
//                         largest threshold (the skip rule of include/mdx.h); a workgroup with nothing left exits.
//   union_dense_kernel    the exact route: one workgroup per row of an fp32 score block, coalesced reads, unite on the hits above the
//                         diagonal.
//   labels_kernel         a launch of its own, after every union: labels[t][i] = the root of i in level t.
//
// The forest and unite are mdx_unionfind.h.  Memory: a CU's L1 is not refreshed by another CU's stores, so inside the union kernels
// EVERY access to parent is an agent-scope relaxed atomic (loads that bypass L1, compare-and-swap and min at the L2 / memory side);
// no plain load of parent exists there, and a failed compare-and-swap goes on from the value it returned.  Relaxed is enough: each
// word is used on its own (a stale parent is still an ancestor), nothing is handed off through it, and the label pass is ordered
// behind the unions by the stream.  Nothing waits on another workgroup.
#include "mdx_exact.h"
#include "mdx_unionfind.h"

namespace mdx {
namespace {

constexpr int G_MAX_T = MDX_GROUPS_MAX_T;
constexpr int G_TC = 64;               // pairs per workgroup: one per lane of wave 0 (exact_kernel's EX_TC)
constexpr int G_KC = 128;              // k per stage (EX_KC)
constexpr int G_LD = G_KC + 4;
constexpr int G_FLAG_RANGE = 2;        // bit 1 of the status flags: a pair named a row >= n

struct Taus {
    float v[G_MAX_T];
};

// parent inside a kernel that also writes it
struct AgentMem {
    static __host__ __device__ __forceinline__ int32_t load(int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __host__ __device__ __forceinline__ int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
    static __host__ __device__ __forceinline__ void store_min(int32_t *p, int32_t v)
    {
        (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// parent in the label pass: nobody writes it any more
struct PlainMem {
    static __host__ __device__ __forceinline__ int32_t load(int32_t *p) { return *p; }
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// one lane adds a workgroup's counters and flags to status (words that are zero are left alone)
__device__ __forceinline__ void report(int64_t *status, uint32_t chains, uint32_t edges, uint32_t hooks, uint32_t flags)
{
    unsigned long long *s = (unsigned long long *)status;
    if (chains) atomicAdd(s + 0, (unsigned long long)chains);
    if (edges) atomicAdd(s + 1, (unsigned long long)edges);
    if (hooks) atomicAdd(s + 2, (unsigned long long)hooks);
    if (flags) atomicOr(s + 3, (unsigned long long)flags);
}

__global__ __launch_bounds__(256) void groups_init_kernel(int32_t *__restrict__ parent, int64_t total, int64_t n, int64_t *__restrict__ status)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) parent[e] = (int32_t)(e % n);
    if (blockIdx.x == 0 && threadIdx.x < 4) status[threadIdx.x] = 0;
}

// unite(i, j) in every level whose threshold s reaches; the number of hooks made
__device__ __forceinline__ uint32_t unite_levels(int32_t *parent, int64_t n, const Taus &taus, int T, float s, int32_t i, int32_t j, int &flags)
{
    uint32_t hooks = 0;
    for (int t = 0; t < T; ++t)
        if (s >= taus.v[t]) hooks += (uint32_t)uf_unite<AgentMem>(parent + (int64_t)t * n, i, j, n + 1, flags);
    return hooks;
}

// tmax: the level of the largest threshold (the skip rule reads it).  vec: ld % 4 == 0 and a 16-byte aligned base
__global__ __launch_bounds__(256) void union_pairs_kernel(const float *__restrict__ rows, int64_t ld, int64_t d, const uint64_t *__restrict__ pairs,
                                                          int64_t P, Taus taus, int T, int tmax, int32_t *parent, int64_t n,
                                                          int64_t *status, bool vec)
{
    __shared__ __attribute__((aligned(16))) float ta[G_TC * G_LD];
    __shared__ __attribute__((aligned(16))) float tb[G_TC * G_LD];
    __shared__ int32_t live_i[G_TC], live_j[G_TC];               // the ends of the pairs that are staged; -1: dropped
    const int64_t c0 = (int64_t)blockIdx.x * G_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    int flags = 0;
    int32_t mi = -1, mj = -1;                                    // of wave 0: lane's pair, if it is staged
    if (wave == 0) {
        const int64_t p = c0 + lane;
        if (p < P) {
            const uint64_t kk = pairs[p];
            const int64_t i = (int64_t)(kk >> 32), j = (int64_t)(kk & 0xFFFFFFFFu);
            if (i >= n || j >= n) {
                flags |= G_FLAG_RANGE;
            } else if (i != j) {
                // the skip rule: ends that share a root in the level of the largest threshold are joined by edges of EVERY level
                int32_t *top = parent + (int64_t)tmax * n;
                const int32_t ri = uf_find<AgentMem>(top, (int32_t)i, n + 1, flags);
                const int32_t rj = uf_find<AgentMem>(top, (int32_t)j, n + 1, flags);
                if (ri != rj || (flags & MDX_UF_GAVE_UP)) {
                    mi = (int32_t)i;
                    mj = (int32_t)j;
                }
            }
        }
        live_i[lane] = mi;
        live_j[lane] = mj;
    }
    if (!__syncthreads_or(mi >= 0)) {                            // nothing to stage (the barrier also publishes live_i / live_j)
        if (wave == 0) {
            const uint32_t f = wave_or_u32((uint32_t)flags);
            if (lane == 0) report(status, 0, 0, 0, f);
        }
        return;
    }
    // wave w stages pairs 16 w .. 16 w + 15: two rows per wave-instruction (32 lanes x 16 B = one 512-B piece)
    int64_t ia[8], ib[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int c = wave * 16 + 2 * u + half;
        ia[u] = live_i[c];
        ib[u] = live_j[c];
    }
    const int64_t d_pad = chain_pad(d), stages = chain_stages(d_pad, G_KC);
    f32x4 ra_[8], rb_[8];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ra_[u] = row_piece(rows, ia[u], ld, d, k0 + 4 * l32, vec);
            rb_[u] = row_piece(rows, ib[u], ld, d, k0 + 4 * l32, vec);
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = wave * 16 + 2 * u + half;
            *(f32x4 *)(ta + c * G_LD + 4 * l32) = ra_[u];
            *(f32x4 *)(tb + c * G_LD + 4 * l32) = rb_[u];
        }
    };
    float acc = 0.f;
    fetch(0);
    put();
    __syncthreads();
    for (int64_t s = 0; s < stages; ++s) {
        const int64_t k0 = s * G_KC;
        if (s + 1 < stages) fetch(k0 + G_KC);
        if (wave == 0) {
            const int kend = chain_kend(d_pad, k0, G_KC);
            const float *x = ta + lane * G_LD, *y = tb + lane * G_LD;
            for (int kk = 0; kk < kend; kk += 4) {
                const f32x4 xv = *(const f32x4 *)(x + kk);
                const f32x4 yv = *(const f32x4 *)(y + kk);
                acc = chain_step4(acc, xv, yv);
            }
        }
        if (s + 1 < stages) {
            __syncthreads();
            put();
            __syncthreads();
        }
    }
    if (wave != 0) return;
    uint32_t hooks = 0, edge = 0;
    if (mi >= 0) {
        hooks = unite_levels(parent, n, taus, T, acc, mi, mj, flags);
        edge = acc >= taus.v[0] ? 1u : 0u;                       // a NaN chain is an edge of no level
        for (int t = 1; t < T; ++t) edge |= acc >= taus.v[t] ? 1u : 0u;
    }
    const uint32_t chains = (uint32_t)__popcll(__ballot(mi >= 0)), edges = (uint32_t)__popcll(__ballot(edge != 0));
    hooks = wave_sum_u32(hooks);
    const uint32_t f = wave_or_u32((uint32_t)flags);
    if (lane == 0) report(status, chains, edges, hooks, f);
}

// row r of scores [m, ncols] at ld is row row_base + r, column c is row col_base + c; tmin: the smallest threshold
__global__ __launch_bounds__(256) void union_dense_kernel(const float *__restrict__ sc, int64_t ncols, int64_t ld, int64_t row_base, int64_t col_base,
                                                          Taus taus, int T, float tmin, int32_t *parent, int64_t n, int64_t *status)
{
    __shared__ uint32_t part[4][3];
    const int64_t r = blockIdx.x, i = row_base + r;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t edges = 0, hooks = 0;
    int flags = 0;
    for (int64_t c = tid; c < ncols; c += 256) {
        const float s = sc[r * ld + c];
        const int64_t j = col_base + c;
        if (j > i && s >= tmin) {
            ++edges;
            hooks += unite_levels(parent, n, taus, T, s, (int32_t)i, (int32_t)j, flags);
        }
    }
    edges = wave_sum_u32(edges);
    hooks = wave_sum_u32(hooks);
    const uint32_t f = wave_or_u32((uint32_t)flags);
    if (lane == 0) {
        part[wave][0] = edges;
        part[wave][1] = hooks;
        part[wave][2] = f;
    }
    __syncthreads();
    if (tid == 0)
        report(status, 0, part[0][0] + part[1][0] + part[2][0] + part[3][0], part[0][1] + part[1][1] + part[2][1] + part[3][1],
               part[0][2] | part[1][2] | part[2][2] | part[3][2]);
}

__global__ __launch_bounds__(256) void labels_kernel(const int32_t *__restrict__ parent, int64_t total, int64_t n, int64_t *__restrict__ labels)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t t = e / n;
    labels[e] = (int64_t)uf_root<PlainMem>(parent + t * n, (int32_t)(e - t * n), n + 1);
}

// the checks that the two unions share; fills taus, *tmax (the level of the largest threshold) and *tmin (the smallest one)
int union_args(const char *who, const float *taus_host, int64_t T, const void *parent, int64_t n, const void *status, Taus *taus, int *tmax,
               float *tmin)
{
    MDX_CHECK_ARG(taus_host && parent && status, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && n < (1ll << 31), "%s: n=%lld must be in [1, 2^31)", who, (long long)n);
    MDX_CHECK_ARG(T >= 1 && T <= G_MAX_T, "%s: T=%lld thresholds, between 1 and MDX_GROUPS_MAX_T = %d", who, (long long)T, G_MAX_T);
    *tmax = 0;
    *tmin = taus_host[0];
    for (int t = 0; t < G_MAX_T; ++t) {
        taus->v[t] = t < T ? taus_host[t] : __builtin_inff();
        if (t >= T) continue;
        MDX_CHECK_ARG(__builtin_isfinite(taus_host[t]), "%s: thresholds must be finite (taus[%d])", who, t);
        if (taus_host[t] > taus_host[*tmax]) *tmax = t;
        if (taus_host[t] < *tmin) *tmin = taus_host[t];
    }
    return MDX_OK;
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_groups_init(int32_t *parent, int64_t T, int64_t n, int64_t *status, void *stream)
{
    MDX_CHECK_ARG(parent && status, "mdx_groups_init: NULL pointer");
    MDX_CHECK_ARG(n >= 1 && n < (1ll << 31), "mdx_groups_init: n=%lld must be in [1, 2^31)", (long long)n);
    MDX_CHECK_ARG(T >= 1 && T <= G_MAX_T, "mdx_groups_init: T=%lld levels, between 1 and MDX_GROUPS_MAX_T = %d", (long long)T, G_MAX_T);
    const int64_t total = T * n;
    hipLaunchKernelGGL(groups_init_kernel, dim3((unsigned)ceil_div(total, (int64_t)256)), dim3(256), 0, (hipStream_t)stream, parent, total, n, status);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_groups_union_pairs(const float *rows, int64_t ld, int64_t d, const uint64_t *pairs, int64_t P, const float *taus, int64_t T,
                           int32_t *parent, int64_t n, int64_t *status, void *stream)
{
    const char *who = "mdx_groups_union_pairs";
    MDX_CHECK_ARG(rows && pairs, "%s: NULL pointer", who);
    Taus tv;
    int tmax = 0;
    float tmin = 0.f;
    if (const int rc = union_args(who, taus, T, parent, n, status, &tv, &tmax, &tmin)) return rc;
    MDX_CHECK_ARG(d >= 1 && P >= 1, "%s: d=%lld P=%lld must be >= 1", who, (long long)d, (long long)P);
    MDX_CHECK_ARG(P < (1ll << 31), "%s: P=%lld >= 2^31", who, (long long)P);
    MDX_CHECK_ARG(ld >= d, "%s: ld=%lld < d=%lld", who, (long long)ld, (long long)d);
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;
    hipLaunchKernelGGL(union_pairs_kernel, dim3((unsigned)ceil_div(P, (int64_t)G_TC)), dim3(256), 0, (hipStream_t)stream, rows, ld, d, pairs, P, tv,
                       (int)T, tmax, parent, n, status, vec);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_groups_union_dense(const float *scores, int64_t m, int64_t ncols, int64_t ld, int64_t row_base, int64_t col_base, const float *taus,
                           int64_t T, int32_t *parent, int64_t n, int64_t *status, void *stream)
{
    const char *who = "mdx_groups_union_dense";
    MDX_CHECK_ARG(scores, "%s: NULL pointer", who);
    Taus tv;
    int tmax = 0;
    float tmin = 0.f;
    if (const int rc = union_args(who, taus, T, parent, n, status, &tv, &tmax, &tmin)) return rc;
    MDX_CHECK_ARG(m >= 1 && ncols >= 1, "%s: m=%lld ncols=%lld must be >= 1", who, (long long)m, (long long)ncols);
    MDX_CHECK_ARG(ld >= ncols, "%s: ld=%lld < ncols=%lld", who, (long long)ld, (long long)ncols);
    MDX_CHECK_ARG(row_base >= 0 && col_base >= 0, "%s: row_base=%lld / col_base=%lld < 0", who, (long long)row_base, (long long)col_base);
    MDX_CHECK_ARG(m <= n && row_base <= n - m && ncols <= n && col_base <= n - ncols,
                  "%s: rows [%lld, +%lld) or columns [%lld, +%lld) outside the n=%lld rows of the forest", who, (long long)row_base, (long long)m,
                  (long long)col_base, (long long)ncols, (long long)n);
    hipLaunchKernelGGL(union_dense_kernel, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream, scores, ncols, ld, row_base, col_base, tv, (int)T,
                       tmin, parent, n, status);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_groups_labels(const int32_t *parent, int64_t T, int64_t n, int64_t *labels, void *stream)
{
    MDX_CHECK_ARG(parent && labels, "mdx_groups_labels: NULL pointer");
    MDX_CHECK_ARG((const void *)parent != (const void *)labels, "mdx_groups_labels: labels must be a buffer of its own, not parent");
    MDX_CHECK_ARG(n >= 1 && n < (1ll << 31), "mdx_groups_labels: n=%lld must be in [1, 2^31)", (long long)n);
    MDX_CHECK_ARG(T >= 1 && T <= G_MAX_T, "mdx_groups_labels: T=%lld levels, between 1 and MDX_GROUPS_MAX_T = %d", (long long)T, G_MAX_T);
    const int64_t total = T * n;
    hipLaunchKernelGGL(labels_kernel, dim3((unsigned)ceil_div(total, (int64_t)256)), dim3(256), 0, (hipStream_t)stream, parent, total, n, labels);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
