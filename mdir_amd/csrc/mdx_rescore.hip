// Exact rescoring of per-query shortlists and its certificate (include/mdx.h, mdx_rescore / mdx_index_i8_bounds /
// mdx_rescore_certify).
//
//   rescore_kernel   one workgroup per (query, tile of 64 candidates).  The 64 rows are gathered whole, 1 KiB of one row
//                    per wave-instruction (no piece crosses a row), into a padded LDS tile; the next stage's pieces are in
//                    flight in registers while wave 0 runs the chains (lane = candidate, the query chunk broadcast from
//                    LDS).  The row loader, the stage arithmetic and the four-link chain step are those of mdx_exact.h, shared
//                    with exact_kernel of mdx_join.hip: the bits are those of mdx_scores on an fp32 index of the same rows.
//   rescore_sort     one workgroup per query: bitonic sort of up to 4096 (desc_key, id) pairs in LDS (mdx_shortlist_sort.h, shared
//                    with mdx_refine.hip).
//   certify_kernel   one workgroup per query: ||x_q||_1, the query's int8 scale, U_q and the certified depth.
//   i8 bounds        a reduction over the codes and scales of an MDX_I8 shard (vector atomics of order-free max / min / or).
#include "mdx_exact.h"
#include "mdx_shortlist_sort.h"

namespace mdx {
namespace {

constexpr int RS_TC = 64;              // candidates per workgroup: one per lane of wave 0
constexpr int RS_KC = 256;             // k per stage: one 1-KiB piece of every row
constexpr int RS_LD = RS_KC + 4;       // floats per LDS row: lane r reads row r with ds_read_b128, banks 4r .. 4r+3 (mod 64)
constexpr int RS_ROWS_PER_WAVE = RS_TC / 4;

// element k of query q (x_q = q - center, one fp32 subtraction), 0 beyond d
__device__ __forceinline__ float query_elem(const float *queries, int64_t nq, int64_t d, int qlayout, const float *center,
                                            int64_t q, int64_t k)
{
    if (k >= d) return 0.f;
    const float x = qlayout == MDX_ROW_MAJOR ? queries[q * d + k] : queries[k * nq + q];
    return center ? x - center[k] : x;
}

__global__ __launch_bounds__(256) void rescore_kernel(const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld,
                                                      const float *__restrict__ queries, int64_t nq, int qlayout,
                                                      const float *__restrict__ center, const int64_t *__restrict__ ids, int64_t K,
                                                      int64_t tiles, bool vec, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float tile[RS_TC * RS_LD];
    __shared__ __attribute__((aligned(16))) float qs[RS_KC];
    __shared__ int64_t rid[RS_TC];
    const int64_t q = (int64_t)blockIdx.x / tiles, c0 = ((int64_t)blockIdx.x % tiles) * RS_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < RS_TC) {
        const int64_t j = c0 + tid;
        const int64_t id = j < K ? ids[q * K + j] : -1;
        rid[tid] = (id >= 0 && id < n) ? id : -1;        // an id outside [0, n) is never dereferenced
    }
    __syncthreads();
    const int64_t d_pad = chain_pad(d), stages = chain_stages(d_pad, RS_KC);
    int64_t my_ids[RS_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < RS_ROWS_PER_WAVE; ++r) my_ids[r] = rid[wave * RS_ROWS_PER_WAVE + r];

    f32x4 reg[RS_ROWS_PER_WAVE];
    float qreg;
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int r = 0; r < RS_ROWS_PER_WAVE; ++r) reg[r] = row_piece(rows, my_ids[r], ld, d, k0 + 4 * lane, vec);
        qreg = query_elem(queries, nq, d, qlayout, center, q, k0 + tid);
    };
    auto put = [&]() {
#pragma unroll
        for (int r = 0; r < RS_ROWS_PER_WAVE; ++r)
            *(f32x4 *)(tile + (wave * RS_ROWS_PER_WAVE + r) * RS_LD + 4 * lane) = reg[r];
        qs[tid] = qreg;
    };

    float acc = 0.f;
    fetch(0);
    put();
    __syncthreads();
    for (int64_t s = 0; s < stages; ++s) {
        const int64_t k0 = s * RS_KC;
        if (s + 1 < stages) fetch(k0 + RS_KC);                    // in flight during the chains
        if (wave == 0) {
            const int kend = chain_kend(d_pad, k0, RS_KC);
            const float *x = tile + lane * RS_LD;
            for (int kk = 0; kk < kend; kk += 4) {
                const f32x4 xv = *(const f32x4 *)(x + kk);
                const f32x4 qv = *(const f32x4 *)(qs + kk);
                acc = chain_step4(acc, qv, xv);
            }
        }
        if (s + 1 < stages) {
            __syncthreads();                                      // the chains are done with the tile
            put();
            __syncthreads();
        }
    }
    if (wave == 0 && c0 + lane < K) out[q * K + c0 + lane] = rid[lane] >= 0 ? acc : __builtin_nanf("");
}

// ---------------------------------------------------------------- the int8 shard's bounds

constexpr double TINY_SCALE = 0x1p-106;     // > fl(2^-100 / 127): every row with 0 < a < 2^-100 has a scale below it

__global__ __launch_bounds__(64) void i8_bounds_init_kernel(mdx_i8_bounds *b)
{
    if (threadIdx.x == 0) {
        b->s_max = 0.0;
        b->s_min = __builtin_inf();
        b->l_max = 0.0;
        b->flag = 0;
        b->reserved = 0;
    }
}

// one wave per row tile (16 rows x KB tiles of 64 k): lane (g, j) sums |code| of row j over k groups g, the 4 groups add up
__global__ __launch_bounds__(256) void i8_bounds_kernel(const i32x4 *__restrict__ tiles, const float *__restrict__ scales, int64_t n,
                                                        int64_t RT, int64_t KB, mdx_i8_bounds *b)
{
    const int64_t rt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 15;
    if (rt >= RT) return;                                        // wave-uniform
    uint32_t sum = 0;
    for (int64_t kb = 0; kb < KB; ++kb) {
        const i32x4 w = tiles[(rt * KB + kb) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = (int)(int8_t)(uint8_t)((uint32_t)w[e >> 2] >> (8 * (e & 3)));
            sum += (uint32_t)(c < 0 ? -c : c);
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const int64_t row = rt * 16 + j;
    double smax = 0.0, smin = __builtin_inf(), lmax = 0.0;
    int flag = 0;
    if (lane < 16 && row < n) {
        const float sc = scales[row];
        if (!__builtin_isfinite(sc) || (sc > 0.f && (double)sc < TINY_SCALE)) {
            flag = 1;
        } else {
            smax = sc;
            if (sc > 0.f) smin = sc;
            lmax = (double)sc * (double)sum;                     // exact: 24-bit scale times an integer < 2^25
        }
    }
    smax = wave_max_d(smax);
    smin = wave_min_d(smin);
    lmax = wave_max_d(lmax);
    const bool any = __any(flag);
    if (lane == 0) {
        // non-negative doubles order as their bit patterns: order-free integer max / min
        atomicMax((unsigned long long *)&b->s_max, (unsigned long long)__double_as_longlong(smax));
        atomicMin((unsigned long long *)&b->s_min, (unsigned long long)__double_as_longlong(smin));
        atomicMax((unsigned long long *)&b->l_max, (unsigned long long)__double_as_longlong(lmax));
        if (any) atomicOr(&b->flag, 1);
    }
}

// ---------------------------------------------------------------- the certificate

constexpr int CERT_THREADS = 256;

__global__ __launch_bounds__(CERT_THREADS) void certify_kernel(const float *__restrict__ scores, int64_t K, const float *__restrict__ t,
                                                               const float *__restrict__ queries, int64_t nq, int64_t d, int qlayout,
                                                               const float *__restrict__ center, const mdx_i8_bounds *__restrict__ b,
                                                               int64_t n, float *__restrict__ upper, int32_t *__restrict__ depth)
{
    __shared__ double part[CERT_THREADS];
    __shared__ float amax[CERT_THREADS];
    __shared__ int bad[CERT_THREADS];
    __shared__ float u_shared;
    __shared__ int void_shared;
    __shared__ int64_t first[CERT_THREADS];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    // ||x_q||_1 (float64, per-thread partials over k = tid + 256 i, then a fixed tree), a = max |x_q,k|, non-finite values
    double l1 = 0.0;
    float a = 0.f;
    int nonfinite = 0;
    for (int64_t k = tid; k < d; k += CERT_THREADS) {
        const float x = query_elem(queries, nq, d, qlayout, center, q, k);
        if (!__builtin_isfinite(x)) nonfinite = 1;
        l1 += (double)fabsf(x);
        a = fmaxf(a, fabsf(x));
    }
    part[tid] = l1;
    amax[tid] = a;
    bad[tid] = nonfinite;
    __syncthreads();
    for (int o = CERT_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            part[tid] += part[tid + o];
            amax[tid] = fmaxf(amax[tid], amax[tid + o]);
            bad[tid] |= bad[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int voided = 0;
        double u = -__builtin_inf();
        if (K < n) {
            const double xl1 = part[0];
            const float aq = amax[0];
            const float scale_q = __fdiv_rn(aq, 127.0f);                // the query's scale in the int8 path
            const double tq = (double)t[q];
            const double smax = b->s_max, lmax = b->l_max;
            const double e = 0.5 + 0x1p-15, ud = (double)d * 0x1p-24;
            const double gamma = ud / (1.0 - ud);
            const double big = 127.0 * smax * (1.0 + 0x1p-22) * xl1;     // >= sum_k |x_i,k x_q,k| of every row
            voided = b->flag || bad[0] || (aq > 0.f && (double)aq < 0x1p-100) || tq != tq || ud >= 0.5 ||
                     b->s_min * (double)scale_q < 0x1p-126 || !(big < 0x1p126);
            if (!voided) {
                const double terms[5] = {0x1p-22 * fabs(tq), smax * e * xl1, lmax * (double)scale_q * e, gamma * big,
                                         (double)d * 0x1p-149};
                double sum = tq, mag = fabs(tq);
                for (int i = 0; i < 5; ++i) {
                    sum += terms[i];
                    mag += terms[i];
                }
                // float64 rounding: every operation above errs by at most 2^-53 of the magnitudes summed, and ||x_q||_1 by
                // at most d 2^-53 of itself; (d + 16) 2^-52 of everything covers all of it
                u = sum + mag * ((double)d + 16.0) * 0x1p-52;
                if (!__builtin_isfinite(u)) voided = 1;
            }
        }
        float uf = (float)u;                                             // round to nearest, then up if it went down
        if ((double)uf < u) uf = next_up(uf);
        u_shared = uf;
        void_shared = voided;
    }
    __syncthreads();
    const float uf = u_shared;
    // depth = the first position whose score is not > U_q (the scores are sorted: larger first, NaN last)
    int64_t f = K;
    if (K < n && !void_shared) {
        for (int64_t i = tid; i < K; i += CERT_THREADS)
            if (!(scores[q * K + i] > uf)) { f = i; break; }
    }
    first[tid] = f;
    __syncthreads();
    for (int o = CERT_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) first[tid] = first[tid] < first[tid + o] ? first[tid] : first[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        upper[q] = uf;
        depth[q] = void_shared ? 0 : (int32_t)first[0];
    }
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_rescore_workspace(int64_t nq, int64_t K, int64_t d)
{
    if (nq < 1 || K < 1 || K > MDX_RESCORE_MAX_K || d < 1) return 0;
    return round_up(nq * K * 4, 256);
}

int mdx_rescore(const float *rows, int64_t n, int64_t d, int64_t ld, const float *queries, int64_t nq, int qlayout,
                const float *center, const int64_t *ids, int64_t K, int64_t *out_ids, float *out_scores, void *workspace,
                int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(rows && queries && ids && out_ids && out_scores, "mdx_rescore: NULL pointer");
    MDX_CHECK_ARG(n >= 1 && d >= 1 && nq >= 1 && K >= 1, "mdx_rescore: n=%lld d=%lld nq=%lld K=%lld must be >= 1", (long long)n,
                  (long long)d, (long long)nq, (long long)K);
    MDX_CHECK_ARG(K <= MDX_RESCORE_MAX_K, "mdx_rescore: K=%lld > %d", (long long)K, MDX_RESCORE_MAX_K);
    MDX_CHECK_ARG(ld >= d, "mdx_rescore: ld=%lld < d=%lld", (long long)ld, (long long)d);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "mdx_rescore: qlayout %d", qlayout);
    const int64_t tiles = ceil_div(K, (int64_t)RS_TC);
    MDX_CHECK_ARG(nq * tiles < (1ll << 31), "mdx_rescore: nq=%lld too large for one launch", (long long)nq);
    const int64_t need = mdx_rescore_workspace(nq, K, d);
    MDX_CHECK_WORKSPACE("mdx_rescore", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float *sc = (float *)workspace;
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;       // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(rescore_kernel, dim3((unsigned)(nq * tiles)), dim3(256), 0, s, rows, n, d, ld, queries, nq, qlayout, center, ids,
                       K, tiles, vec, sc);
    int P = 1;
    while (P < K) P <<= 1;
    hipLaunchKernelGGL(rescore_sort_kernel, dim3((unsigned)nq), dim3(SORT_THREADS), 0, s, (const float *)sc, ids, K, P, out_ids, out_scores);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_index_i8_bounds(const mdx_index *index, mdx_i8_bounds *bounds, void *stream)
{
    MDX_CHECK_ARG(index && bounds, "mdx_index_i8_bounds: NULL pointer");
    const void *tiles = nullptr;
    const float *scales = nullptr;
    int64_t n = 0, RT = 0, KB = 0;
    MDX_CHECK_ARG(i8_view(index, &tiles, &scales, &n, &RT, &KB), "mdx_index_i8_bounds: an int8 shard is needed");
    MDX_CHECK_ARG(ceil_div(RT, (int64_t)4) < (1ll << 31), "mdx_index_i8_bounds: shard too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(i8_bounds_init_kernel, dim3(1), dim3(64), 0, s, bounds);
    hipLaunchKernelGGL(i8_bounds_kernel, dim3((unsigned)ceil_div(RT, (int64_t)4)), dim3(256), 0, s, (const i32x4 *)tiles, scales, n, RT,
                       KB, bounds);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_rescore_certify(const float *scores, int64_t nq, int64_t K, const float *t, const float *queries, int64_t d, int qlayout,
                        const float *center, const mdx_i8_bounds *bounds, int64_t n, float *upper, int32_t *depth, void *stream)
{
    MDX_CHECK_ARG(scores && t && queries && bounds && upper && depth, "mdx_rescore_certify: NULL pointer");
    MDX_CHECK_ARG(nq >= 1 && K >= 1 && d >= 1 && n >= 1, "mdx_rescore_certify: nq=%lld K=%lld d=%lld n=%lld must be >= 1",
                  (long long)nq, (long long)K, (long long)d, (long long)n);
    MDX_CHECK_ARG(K <= MDX_RESCORE_MAX_K && K <= n, "mdx_rescore_certify: K=%lld must be <= min(n=%lld, %d)", (long long)K,
                  (long long)n, MDX_RESCORE_MAX_K);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "mdx_rescore_certify: qlayout %d", qlayout);
    MDX_CHECK_ARG(nq < (1ll << 31), "mdx_rescore_certify: nq=%lld too large for one launch", (long long)nq);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(certify_kernel, dim3((unsigned)nq), dim3(CERT_THREADS), 0, s, scores, K, t, queries, nq, d, qlayout, center, bounds,
                       n, upper, depth);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
