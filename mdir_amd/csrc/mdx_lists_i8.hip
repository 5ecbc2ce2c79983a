// int8 list storage of the inverted file (include/mdx_lists_i8.h): the codes of the rows in list order, their bounds, and the first
// stage of a search on v_mfma_i32_16x16x64_i8.
//
//   encode    one wave per position p: the absmax of row members[p], then 16 codes per lane and store (the arithmetic of
//             mdx_i8_quant.h, the row loader of mdx_exact.h).
//   bounds    one wave per 16 positions: sum |code| per row, the maxima / minimum / flag of i8_bounds_kernel (mdx_rescore.hip) by the
//             same order-free atomics.
//   scan      one workgroup per work item of the plan (mdx_ivf_plan.h): a tile of 64 members of a list and a group of up to 8
//             entries.  Wave w owns members 16 w .. 16 w + 15: the A operand is loaded straight from the contiguous code tile, lane
//             (g, j) the 16 bytes k = 64 kb + 16 g .. of member j; the B operand is the group's query codes from LDS, rows 8 .. 15
//             zero.  acc[i] of lane (g, c) is member 4 g + i against query slot c.
#include <type_traits>

#include "mdx_exact.h"
#include "mdx_i8_quant.h"
#include "mdx_ivf_plan.h"

namespace mdx {
namespace {

constexpr int QKC = 1024;                   // k per stage of the query codes: 16 MFMAs per wave
constexpr int QKB = QKC / 64;
constexpr int QLD = QKC + 16;               // bytes per LDS row: lanes j = 0 .. 15 of a ds_read_b128 hit banks 4 j .. 4 j + 3
constexpr int QPW = G / 4;                  // query rows a wave brings in per stage
constexpr double TINY_SCALE = 0x1p-106;     // as in mdx_rescore.hip: every row with 0 < a < 2^-100 has a scale below it

static_assert(TC == 64 && G % 4 == 0 && G <= 16, "four waves of 16 members, the entries in the 16 columns of one MFMA");

// ------------------------------------------------------------------------------------------------------------------ encode

__global__ __launch_bounds__(256) void lists_encode_kernel(const float *__restrict__ rows, int64_t n, int64_t d, int64_t ld,
                                                           const int64_t *__restrict__ members, int64_t m, int64_t d_pad, bool vec,
                                                           i32x4 *__restrict__ codes, float *__restrict__ scales)
{
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= m) return;                                           // wave-uniform
    const int64_t given = members[p];
    const int64_t id = (given >= 0 && given < n) ? given : -1;   // an id outside [0, n) is never dereferenced: row_piece reads nothing
    float a = 0.f;
    for (int64_t k = 4 * lane; k < d; k += 256) {
        const f32x4 v = row_piece(rows, id, ld, d, k, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaxf(a, fabsf(v[e]));
    }
    a = wave_max(a);
    const float inv = i8_inv(a);
    i32x4 *out = codes + p * (d_pad / 16);
    for (int64_t k0 = 16 * lane; k0 < d_pad; k0 += 1024) {
        i32x4 w = {0, 0, 0, 0};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const f32x4 x = row_piece(rows, id, ld, d, k0 + 4 * v, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[v] |= (int)(i8_code(x[e], a, inv) << (8 * e));
        }
        out[k0 / 16] = w;
    }
    if (lane == 0) scales[p] = id >= 0 ? i8_scale(a) : __builtin_nanf("");
}

// ------------------------------------------------------------------------------------------------------------------ bounds

__global__ __launch_bounds__(64) void lists_bounds_init_kernel(mdx_i8_bounds *b)
{
    if (threadIdx.x == 0) {
        b->s_max = 0.0;
        b->s_min = __builtin_inf();
        b->l_max = 0.0;
        b->flag = 0;
        b->reserved = 0;
    }
}

__global__ __launch_bounds__(256) void lists_bounds_kernel(const i32x4 *__restrict__ codes, const float *__restrict__ scales, int64_t m,
                                                           int64_t d_pad, mdx_i8_bounds *b)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const int lane = threadIdx.x & 63;
    if (p0 >= m) return;                                          // wave-uniform
    const int64_t p1 = p0 + 16 < m ? p0 + 16 : m;
    double smax = 0.0, smin = __builtin_inf(), lmax = 0.0;
    int flag = 0;
    for (int64_t p = p0; p < p1; ++p) {
        const i32x4 *row = codes + p * (d_pad / 16);
        uint32_t sum = 0;
        for (int64_t k0 = 16 * lane; k0 < d_pad; k0 += 1024) {
            const i32x4 w = row[k0 / 16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = (int)(int8_t)(uint8_t)((uint32_t)w[e >> 2] >> (8 * (e & 3)));
                sum += (uint32_t)(c < 0 ? -c : c);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);      // integers: every lane holds the row's sum
        const float sc = scales[p];
        if (!__builtin_isfinite(sc) || (sc > 0.f && (double)sc < TINY_SCALE)) {
            flag = 1;
        } else {
            smax = fmax(smax, (double)sc);
            if (sc > 0.f) smin = fmin(smin, (double)sc);
            lmax = fmax(lmax, (double)sc * (double)sum);         // exact: 24-bit scale times an integer < 2^25
        }
    }
    if (lane == 0) {
        // non-negative doubles order as their bit patterns: order-free integer max / min
        atomicMax((unsigned long long *)&b->s_max, (unsigned long long)__double_as_longlong(smax));
        atomicMin((unsigned long long *)&b->s_min, (unsigned long long)__double_as_longlong(smin));
        atomicMax((unsigned long long *)&b->l_max, (unsigned long long)__double_as_longlong(lmax));
        if (flag) atomicOr(&b->flag, 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ scan

// bytes k .. k + 15 of the codes of query q (zeros beyond d; nothing is read without a query).  vec: d % 16 == 0 and a 16-byte
// aligned base, so that a piece inside the row is one 16-byte load
__device__ __forceinline__ i32x4 query_piece(const int8_t *qcodes, int64_t q, int64_t d, int64_t k, bool vec)
{
    i32x4 w = {0, 0, 0, 0};
    if (q < 0 || k >= d) return w;
    const int8_t *p = qcodes + q * d + k;
    if (vec && k + 16 <= d) return *(const i32x4 *)p;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (k + e < d) w[e >> 2] |= (int)((uint32_t)(uint8_t)p[e] << (8 * (e & 3)));
    return w;
}

__global__ __launch_bounds__(256) void lists_scan_kernel(const int8_t *__restrict__ codes, const float *__restrict__ scales, int64_t m,
                                                         int64_t d, const int64_t *__restrict__ members,
                                                         const int64_t *__restrict__ offsets, int64_t K,
                                                         const int8_t *__restrict__ qcodes, const float *__restrict__ qscales, int64_t nq,
                                                         int64_t nprobe, const int64_t *__restrict__ base,
                                                         const int64_t *__restrict__ first, const int64_t *__restrict__ item,
                                                         const int64_t *__restrict__ entry, int64_t cap, bool qvec,
                                                         float *__restrict__ cand_scores, int64_t *__restrict__ cand_ids)
{
    __shared__ __attribute__((aligned(16))) int8_t qs[16 * QLD];
    __shared__ int64_t gid[TC];                 // the member id as given
    __shared__ float msc[TC];                   // the member's scale (NaN for an id the encoder refused)
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
    const int64_t t = local % tiles, grp = local / tiles;       // consecutive workgroups share the tile's codes
    const int64_t entries = nq * nprobe;
    const int64_t f0 = clamp_to(first[l], entries), f1 = clamp_to(first[l + 1], entries);
    const int64_t e0 = f0 + grp * G;
    if (e0 >= f1) return;
    const int ne = (int)(f1 - e0 < G ? f1 - e0 : G);
    const int in_tile = (int)(size - t * TC < TC ? size - t * TC : TC);
    const int64_t pos0 = start + t * TC;                        // pos0 + in_tile <= start + size <= m
    if (tid < TC) {
        gid[tid] = tid < in_tile ? members[pos0 + tid] : -1;
        msc[tid] = tid < in_tile ? scales[pos0 + tid] : __builtin_nanf("");
    }
    item_slots(tid, t, e0, ne, entry, base, nq, nprobe, qidx, qcol);
    // rows G .. 15 of the B operand are zero for good: one 16-byte piece per thread and row
    for (int r = G + wave; r < 16; r += 4) *(i32x4 *)(qs + r * QLD + 16 * lane) = (i32x4){0, 0, 0, 0};
    __syncthreads();
    const int64_t d_pad = chain_pad(d), stages = (d_pad + QKC - 1) / QKC;
    int64_t my_q[QPW];
#pragma unroll
    for (int i = 0; i < QPW; ++i) my_q[i] = qidx[wave + 4 * i];

    i32x4 qreg[QPW];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < QPW; ++i) qreg[i] = query_piece(qcodes, my_q[i], d, k0 + 16 * lane, qvec);
    };
    auto put = [&]() {
#pragma unroll
        for (int i = 0; i < QPW; ++i) *(i32x4 *)(qs + (wave + 4 * i) * QLD + 16 * lane) = qreg[i];
    };

    const int j = lane & 15, kg = lane >> 4;
    const bool active = wave * 16 < in_tile;                    // wave-uniform: the wave has members
    // a lane whose member does not exist (beyond the tile's end) reads the tile's first member instead -- memory that is there --
    // and its sums are never written: no load of the stage hangs on a per-lane condition
    const bool mine = wave * 16 + j < in_tile;
    const i32x4 *arow = (const i32x4 *)(codes + (pos0 + (mine ? wave * 16 + j : 0)) * d_pad) + kg;
    const int8_t *brow = qs + j * QLD + 16 * kg;
    i32x4 acc = {0, 0, 0, 0};
    // one stage: all of its loads first (16 KiB per wave in flight), then its MFMAs.  FULL: 16 k-blocks, no condition at all
    auto stage = [&](const i32x4 *ap, int nkb, auto full) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full)::value;
        i32x4 a[QKB];
#pragma unroll
        for (int kb = 0; kb < QKB; ++kb)
            if (FULL || kb < nkb) a[kb] = ap[kb * 4];
#pragma unroll
        for (int kb = 0; kb < QKB; ++kb)
            if (FULL || kb < nkb) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[kb], *(const i32x4 *)(brow + 64 * kb), acc, 0, 0, 0);
    };
    fetch(0);
    put();
    __syncthreads();
    for (int64_t s = 0; s < stages; ++s) {
        const int64_t k0 = s * QKC;
        if (s + 1 < stages) fetch(k0 + QKC);                      // in flight during the MFMAs
        if (active) {
            const int nkb = (int)(d_pad - k0 < QKC ? (d_pad - k0) / 64 : QKB);
            const i32x4 *ap = arow + (k0 / 64) * 4;
            if (nkb == QKB) stage(ap, nkb, std::true_type{}); else stage(ap, nkb, std::false_type{});
        }
        if (s + 1 < stages) {
            __syncthreads();                                      // the MFMAs are done with the query stage
            put();
            __syncthreads();
        }
    }
    // lane (kg, j): members 16 wave + 4 kg + i against query slot j
    if (!active || j >= ne || qidx[j] < 0) return;
    const int64_t q = qidx[j];
    const float sq = qscales[q];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wave * 16 + 4 * kg + i;
        if (r >= in_tile) continue;
        const int64_t col = qcol[j] + r;
        if (col >= cap) continue;                                 // beyond the candidate row: the candidate does not exist
        cand_scores[q * cap + col] = __fmul_rn((float)acc[i], __fmul_rn(msc[r], sq));
        cand_ids[q * cap + col] = gid[r];
    }
}

static int check_codes(const char *who, const void *codes, int64_t m, int64_t d)
{
    MDX_CHECK_ARG(m >= 1 && d >= 1 && m < LIMIT, "%s: m=%lld d=%lld must be >= 1 and m below 2^31", who, (long long)m, (long long)d);
    MDX_CHECK_ARG(d <= I8_MAX_DPAD, "%s: d=%lld too large (127^2 * round_up(d, 64) must stay below 2^31; d <= %lld)", who, (long long)d,
                  (long long)I8_MAX_DPAD);
    MDX_CHECK_ARG(((uintptr_t)codes & 15) == 0, "%s: codes must be 16-byte aligned", who);
    return MDX_OK;
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_lists_i8_encode(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, int64_t m, int8_t *codes,
                        float *scales, void *stream)
{
    const char *who = "mdx_lists_i8_encode";
    MDX_CHECK_ARG(rows && members && codes && scales, "%s: NULL pointer", who);
    MDX_CHECK_ARG(n >= 1 && n < LIMIT, "%s: n=%lld must be in [1, 2^31)", who, (long long)n);
    if (int rc = check_codes(who, codes, m, d)) return rc;
    MDX_CHECK_ARG(ld >= d, "%s: ld=%lld < d=%lld", who, (long long)ld, (long long)d);
    MDX_CHECK_ARG(ld <= INT64_MAX / n, "%s: n * ld overflows", who);
    const bool vec = ld % 4 == 0 && ((uintptr_t)rows & 15) == 0;       // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(lists_encode_kernel, dim3((unsigned)ceil_div(m, 4)), dim3(256), 0, (hipStream_t)stream, rows, n, d, ld, members, m,
                       round_up(d, 64), vec, (i32x4 *)codes, scales);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_lists_i8_bounds(const int8_t *codes, const float *scales, int64_t m, int64_t d, mdx_i8_bounds *bounds, void *stream)
{
    const char *who = "mdx_lists_i8_bounds";
    MDX_CHECK_ARG(codes && scales && bounds, "%s: NULL pointer", who);
    if (int rc = check_codes(who, codes, m, d)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lists_bounds_init_kernel, dim3(1), dim3(64), 0, s, bounds);
    hipLaunchKernelGGL(lists_bounds_kernel, dim3((unsigned)ceil_div(m, 64)), dim3(256), 0, s, (const i32x4 *)codes, scales, m, round_up(d, 64),
                       bounds);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_lists_i8_scan(const int8_t *codes, const float *scales, int64_t m, int64_t d, const int64_t *members, const int64_t *offsets,
                      int64_t K, const int8_t *qcodes, const float *qscales, int64_t nq, int64_t nprobe, const void *plan,
                      int64_t plan_bytes, int64_t cap, int64_t items, float *cand_scores, int64_t *cand_ids, void *stream)
{
    const char *who = "mdx_lists_i8_scan";
    MDX_CHECK_ARG(codes && scales && members && offsets && qcodes && qscales && cand_scores && cand_ids, "%s: NULL pointer", who);
    if (int rc = check_codes(who, codes, m, d)) return rc;
    MDX_CHECK_ARG(items >= 1 && items < LIMIT, "%s: items=%lld must be in [1, 2^31)", who, (long long)items);
    if (int rc = check_plan(who, nq, nprobe, K, plan, plan_bytes)) return rc;
    if (int rc = check_cap(who, nq, cap)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Plan v = carve(plan, nq, nprobe, K);
    const bool qvec = d % 16 == 0 && ((uintptr_t)qcodes & 15) == 0;    // 16-byte pieces at 16-byte addresses
    hipLaunchKernelGGL(lists_scan_kernel, dim3((unsigned)items), dim3(256), 0, s, codes, scales, m, d, members, offsets, K, qcodes, qscales, nq,
                       nprobe, (const int64_t *)v.base, (const int64_t *)v.first, (const int64_t *)v.item, (const int64_t *)v.entry, cap, qvec,
                       cand_scores, cand_ids);
    launch_pad(v, nq, cap, cand_scores, cand_ids, s);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
