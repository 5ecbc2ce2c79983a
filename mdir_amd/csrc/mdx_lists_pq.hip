// Product-quantised lists of the inverted file (include/mdx_lists_pq.h): the look-up table of a batch of queries and the scan over
// byte codes.
//
//   lut       one workgroup per (subspace m, group of LQ queries): thread j owns codeword (m, j), reads it once and runs the exact
//             chain against the LQ sub-vectors, which are staged in LDS LKC elements at a time and broadcast.
//   scan      query-major: nq * splits workgroups of eight waves.  A workgroup copies its query's table (M KiB) to LDS and walks the
//             probes s, s + splits, ... of its query, one wave per probe in turn, lane = member: the member's codes come 16 (4, 1) at
//             a time from global memory, every code is one LDS read at table[m][code], the additions run in m order.
#include "mdx_exact.h"
#include "mdx_ivf_plan.h"

namespace mdx {
namespace {

constexpr int LQ = MDX_PQ_LUT_QUERIES;      // queries that share the registers of a codeword
constexpr int LKC = 256;                    // k per stage of the sub-vectors
constexpr int CW = MDX_PQ_CODEWORDS;
constexpr int SCAN_THREADS = 512, SCAN_WAVES = SCAN_THREADS / WAVE;
constexpr int TABLE_BYTES_MAX = MDX_PQ_MAX_M * CW * 4;

static_assert(CW == 256, "a code is one byte, a codeword one thread of the table kernel");

// ------------------------------------------------------------------------------------------------------------------ lut

// element k of query q (x_q = q - center, one fp32 subtraction), as query_elem of mdx_ivf.hip
__device__ __forceinline__ float lut_query_elem(const float *queries, int64_t nq, int64_t d, int qlayout, const float *center, int64_t q,
                                                int64_t k)
{
    const float x = qlayout == MDX_ROW_MAJOR ? queries[q * d + k] : queries[k * nq + q];
    return center ? x - center[k] : x;
}

__global__ __launch_bounds__(256) void pq_lut_kernel(const float *__restrict__ codewords, int64_t M, int64_t dsub,
                                                     const float *__restrict__ queries, int64_t nq, int qlayout,
                                                     const float *__restrict__ center, bool vec, float *__restrict__ lut)
{
    __shared__ __attribute__((aligned(16))) float xs[LQ][LKC];
    const int64_t m = (int64_t)blockIdx.x % M, q0 = ((int64_t)blockIdx.x / M) * LQ;
    const int tid = threadIdx.x;
    const int64_t d = M * dsub, word = m * CW + tid;
    float acc[LQ];
#pragma unroll
    for (int r = 0; r < LQ; ++r) acc[r] = 0.f;
    for (int64_t k0 = 0; k0 < dsub; k0 += LKC) {
        const int kend = (int)(dsub - k0 < LKC ? dsub - k0 : LKC);
        if (k0) __syncthreads();                                  // the chains are done with the stage before
        for (int i = tid; i < LQ * LKC; i += 256) {
            const int r = i / LKC, k = i % LKC;
            xs[r][k] = (q0 + r < nq && k < kend) ? lut_query_elem(queries, nq, d, qlayout, center, q0 + r, m * dsub + k0 + k) : 0.f;
        }
        __syncthreads();
        // four links at a time; beyond dsub both factors are zero: fmaf(0, 0, acc), which the padding below repeats
        for (int k = 0; k < kend; k += 4) {
            const f32x4 c = row_piece(codewords, word, dsub, dsub, k0 + k, vec);
#pragma unroll
            for (int r = 0; r < LQ; ++r) acc[r] = chain_step4(acc[r], *(const f32x4 *)&xs[r][k], c);
        }
    }
    const bool padded = dsub % 64 != 0;                           // the chain of an index goes on over zeros to round_up(dsub, 64)
#pragma unroll
    for (int r = 0; r < LQ; ++r) {
        if (q0 + r >= nq) break;
        lut[((q0 + r) * M + m) * CW + tid] = padded ? __builtin_fmaf(0.f, 0.f, acc[r]) : acc[r];
    }
}

// ------------------------------------------------------------------------------------------------------------------ scan

// acc + table[m][code[m]] for m = 0 .. M - 1 in that order, the codes read W bytes at a time (the bytes M .. of the last piece are
// loaded -- they lie inside the row's stride -- and not used)
template <int W>
__device__ __forceinline__ float adc_chain(const float *table, const uint8_t *row, int M, float acc)
{
    constexpr int NW = W >= 4 ? W / 4 : 1;
    for (int m0 = 0; m0 < M; m0 += W) {
        uint32_t w[NW];
        if constexpr (W == 16) {
            const i32x4 v = *(const i32x4 *)(row + m0);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (uint32_t)v[e];
        } else if constexpr (W == 4) {
            w[0] = *(const uint32_t *)(row + m0);
        } else {
            w[0] = row[m0];
        }
        const float *t = table + m0 * CW;
        if (M - m0 >= W) {
            float x[W];
#pragma unroll
            for (int e = 0; e < W; ++e) x[e] = t[e * CW + ((w[e >> 2] >> (8 * (e & 3))) & 255u)];
#pragma unroll
            for (int e = 0; e < W; ++e) acc = __fadd_rn(acc, x[e]);
        } else {
            for (int e = 0; e < M - m0; ++e) acc = __fadd_rn(acc, t[e * CW + ((w[e >> 2] >> (8 * (e & 3))) & 255u)]);
        }
    }
    return acc;
}

__global__ __launch_bounds__(SCAN_THREADS) void lists_pq_scan_kernel(const uint8_t *__restrict__ codes, int64_t m, int M, int64_t ldc,
                                                                     int width, const int64_t *__restrict__ members, int64_t n,
                                                                     const int64_t *__restrict__ offsets, int64_t K,
                                                                     const float *__restrict__ lut, bool lvec,
                                                                     const float *__restrict__ coarse, const int64_t *__restrict__ probes,
                                                                     int64_t nq, int64_t nprobe, int64_t splits,
                                                                     const int64_t *__restrict__ base, int64_t cap,
                                                                     float *__restrict__ cand_scores, int64_t *__restrict__ cand_ids)
{
    extern __shared__ __attribute__((aligned(16))) float table[];       // [M][256]
    const int64_t q = (int64_t)blockIdx.x / splits, s = (int64_t)blockIdx.x % splits;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (q >= nq) return;                                          // uniform over the workgroup
    const float *src = lut + q * M * CW;
    for (int i = tid; i < M * (CW / 4); i += SCAN_THREADS) {
        f32x4 v;
        if (lvec) {
            v = ((const f32x4 *)src)[i];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = src[4 * i + e];
        }
        ((f32x4 *)table)[i] = v;
    }
    __syncthreads();
    for (int64_t p = s + splits * wave; p < nprobe; p += splits * SCAN_WAVES) {      // wave-uniform
        const int64_t e = q * nprobe + p;
        const int64_t l = probes[e], b = base[e];
        if (l < 0 || l >= K || b < 0) continue;                   // a probe outside the lists, or one the plan marks invalid
        int64_t start, size;
        list_extent(offsets, l, m, start, size);
        const float c0 = coarse[e];
        for (int64_t i = lane; i < size; i += WAVE) {
            const int64_t col = b + i;
            if (col >= cap) break;                                // beyond the candidate row: the candidate does not exist
            const int64_t pos = start + i;                        // < start + size <= m
            const uint8_t *row = codes + pos * ldc;
            const float acc = width == 16 ? adc_chain<16>(table, row, M, c0) : width == 4 ? adc_chain<4>(table, row, M, c0)
                                                                                         : adc_chain<1>(table, row, M, c0);
            const int64_t id = members[pos];
            cand_scores[q * cap + col] = (id >= 0 && id < n) ? acc : __builtin_nanf("");
            cand_ids[q * cap + col] = id;
        }
    }
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_pq_lut(const float *codewords, int64_t M, int64_t dsub, const float *queries, int64_t nq, int qlayout, const float *center,
               float *lut, void *stream)
{
    const char *who = "mdx_pq_lut";
    MDX_CHECK_ARG(codewords && queries && lut, "%s: NULL pointer", who);
    MDX_CHECK_ARG(M >= 1 && M <= MDX_PQ_MAX_M, "%s: M=%lld must be in [1, %d]", who, (long long)M, MDX_PQ_MAX_M);
    MDX_CHECK_ARG(dsub >= 1 && nq >= 1, "%s: dsub=%lld nq=%lld must be >= 1", who, (long long)dsub, (long long)nq);
    MDX_CHECK_ARG(dsub < LIMIT && M * dsub < LIMIT && nq < LIMIT && M * ceil_div(nq, LQ) < LIMIT,
                  "%s: M=%lld dsub=%lld nq=%lld too large (M dsub, nq or M ceil(nq / %d) of 2^31 or more)", who, (long long)M,
                  (long long)dsub, (long long)nq, LQ);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "%s: qlayout %d", who, qlayout);
    const bool vec = dsub % 4 == 0 && ((uintptr_t)codewords & 15) == 0;   // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)(M * ceil_div(nq, LQ))), dim3(256), 0, (hipStream_t)stream, codewords, M, dsub, queries,
                       nq, qlayout, center, vec, lut);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_lists_pq_scan(const uint8_t *codes, int64_t m, int64_t M, int64_t ldc, const int64_t *members, int64_t n, const int64_t *offsets,
                      int64_t K, const float *lut, const float *coarse, const int64_t *probes, int64_t nq, int64_t nprobe,
                      const void *plan, int64_t plan_bytes, int64_t cap, float *cand_scores, int64_t *cand_ids, void *stream)
{
    const char *who = "mdx_lists_pq_scan";
    MDX_CHECK_ARG(codes && members && offsets && lut && coarse && probes && cand_scores && cand_ids, "%s: NULL pointer", who);
    MDX_CHECK_ARG(M >= 1 && M <= MDX_PQ_MAX_M, "%s: M=%lld must be in [1, %d]", who, (long long)M, MDX_PQ_MAX_M);
    MDX_CHECK_ARG(m >= 1 && n >= 1 && m < LIMIT && n < LIMIT, "%s: m=%lld n=%lld must be in [1, 2^31)", who, (long long)m, (long long)n);
    MDX_CHECK_ARG(ldc >= M && ldc < LIMIT, "%s: ldc=%lld must be in [M=%lld, 2^31)", who, (long long)ldc, (long long)M);
    if (int rc = check_plan(who, nq, nprobe, K, plan, plan_bytes)) return rc;
    if (int rc = check_cap(who, nq, cap)) return rc;
    const int64_t want = ceil_div(MDX_PQ_SCAN_GROUPS, nq), splits = want < nprobe ? want : nprobe;     // >= 1
    MDX_CHECK_ARG(nq * splits < LIMIT, "%s: nq=%lld too large for one launch", who, (long long)nq);
    hipStream_t s = (hipStream_t)stream;
    // more than 64 KiB of dynamic LDS needs an opt-in per kernel and device: done once, not on every launch (as mdx_index.hip)
    static bool opted[64];
    int dev = 0;
    MDX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !opted[dev]) {
        MDX_HIP(hipFuncSetAttribute((const void *)lists_pq_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TABLE_BYTES_MAX));
        if (dev >= 0 && dev < 64) opted[dev] = true;
    }
    const Plan v = carve(plan, nq, nprobe, K);
    const int width = (ldc % 16 == 0 && ((uintptr_t)codes & 15) == 0) ? 16 : (ldc % 4 == 0 && ((uintptr_t)codes & 3) == 0) ? 4 : 1;
    const bool lvec = ((uintptr_t)lut & 15) == 0;
    hipLaunchKernelGGL(lists_pq_scan_kernel, dim3((unsigned)(nq * splits)), dim3(SCAN_THREADS), (size_t)(M * CW * 4), s, codes, m, (int)M, ldc,
                       width, members, n, offsets, K, lut, lvec, coarse, probes, nq, nprobe, splits, (const int64_t *)v.base, cap, cand_scores,
                       cand_ids);
    launch_pad(v, nq, cap, cand_scores, cand_ids, s);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
