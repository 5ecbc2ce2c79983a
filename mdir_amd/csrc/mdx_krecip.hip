// k-reciprocal re-ranking (Zhong, Zheng, Cao, Li, "Re-ranking person re-identification with k-reciprocal encoding", CVPR 2017)
// in its database-side form: reciprocal sets of the database's kNN lists, sparse codes of every database row (raw, then locally
// expanded), and the Jaccard min-sum of a query's code against the codes of its first-stage shortlist.  The contract is in
// include/mdx_krecip.h, with the prototypes (include/mdx.h, section "k-reciprocal re-ranking", only points there).
//
// mdx_krecip_sets          one wave per row i: lane e takes L_i[e] = j (its first copy only), scans L_j for the first copy of i,
//                          and the two sets R(i, k) and R(i, h) are compacted in list order by ballot prefixes.
// mdx_krecip_raw_offsets   one 64-thread workgroup per row: R(i, k) to LDS; per member c the intersection |R(i, k) & R(c, h)| by a
// mdx_krecip_raw_fill      ballot; the accepted sets appended at positions from a serial prefix; a bitonic sort of the ids in LDS;
//                          the distinct ids compacted by ballot.  The count pass stores the count (then one single-workgroup scan
//                          turns the counts into offsets in place); the fill pass finds s_ij in L_i or recomputes the exact chain,
//                          one pair per lane, sums the weights serially in id order and stores w / t.
// mdx_krecip_expand_*      one 64-thread workgroup per row: the raw rows of the first k2 list entries gathered into LDS as 64-bit
//                          keys (column << 32 | gather position; the gather is in list order, so equal columns sort in list order)
//                          beside their values, a bitonic sort, one lane per distinct column walks its run: a serial fp32 sum.
// mdx_krecip_rerank        one workgroup of 1024 threads per query, the query's code built and kept sorted in LDS (the same device
//                          functions as the database side), then one wave per shortlist entry streams V'_g from the CSR, binary-
//                          searches the query's columns and sums the minima: per-lane partials over the positions lane, lane + 64,
//                          ..., then the butterfly of wave_sum -- a fixed order.  The values go to the workspace; out = s - 3 and
//                          the scatter are launches of their own, as in the truncated diffusion.
// Nothing here uses a float atomic, and no workgroup waits for another.
#include <math.h>

#include "mdx_exact.h"

namespace mdx {

constexpr uint32_t KR_NONE = 0x7FFFFFFFu;                              // no id (n < 2^31): sorts last, never a member
constexpr int KR_MAX_K = MDX_KRECIP_MAX_K1;
constexpr int KR_MAX_CAND = KR_MAX_K + KR_MAX_K * (KR_MAX_K / 2);      // k + k h candidates of one raw code at most
constexpr int KR_MAX_NNZ = MDX_KRECIP_MAX_NNZ;
constexpr int KR_Q_THREADS = 1024;
static_assert(KR_MAX_K <= 64, "one lane per list entry");
static_assert((KR_MAX_NNZ & (KR_MAX_NNZ - 1)) == 0, "the sort pads to a power of two");

__host__ __device__ inline int kr_pow2(int x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

__host__ __device__ inline int64_t kr_half(int64_t k) { return (k + 1) / 2; }
__host__ __device__ inline int64_t kr_code_cap(int64_t k) { return k + k * kr_half(k); }
__host__ __device__ inline int64_t kr_qe_cap(int64_t k, int64_t k2)
{
    const int64_t c = (k2 < k ? k2 : k) * kr_code_cap(k);
    return c < KR_MAX_NNZ ? c : KR_MAX_NNZ;
}

// ascending bitonic sort of keys[0, P) (P a power of two, the same in every thread) by the whole workgroup
template <typename T>
__device__ void kr_bitonic(T *keys, int P)
{
    const int t = threadIdx.x, nt = blockDim.x;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = t; i < P / 2; i += nt) {
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const T a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    }
    __syncthreads();
}

// The candidates of R*: A[0, na) (a set of the database or R(q); KR_NONE entries are no members) and every R(c, h), c in A, with
// 3 |A & R(c, h)| >= 2 |R(c, h)| > 0, sorted ascending in cand[0, pow2(total)).  Every thread of the workgroup calls it; acc and
// pos are LDS scratch of 64 and 65 ints.  Returns the padded length.
__device__ int kr_candidates(const uint32_t *A, int na, const int32_t *__restrict__ rh, const int32_t *__restrict__ rh_counts,
                             int64_t n, int h, uint32_t *cand, int *acc, int *pos)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int e = wave; e < na; e += nw) {                            // wave-uniform
        const uint32_t c = A[e];
        int hc = 0;
        if (c < (uint64_t)n) {
            hc = rh_counts[c];
            hc = hc < 0 ? 0 : (hc > h ? h : hc);
        }
        bool in = false;
        if (lane < hc) {
            const int32_t m = rh[(int64_t)c * h + lane];
            if (m >= 0 && m < n)
                for (int a = 0; a < na; ++a)
                    if (A[a] == (uint32_t)m) {
                        in = true;
                        break;
                    }
        }
        const int inter = __builtin_popcountll(__ballot(in));
        if (lane == 0) acc[e] = (hc > 0 && 3 * inter >= 2 * hc) ? hc : 0;
    }
    for (int e = threadIdx.x; e < na; e += blockDim.x) cand[e] = A[e];
    __syncthreads();
    if (threadIdx.x == 0) {
        int p = na;
        for (int e = 0; e < na; ++e) {
            pos[e] = p;
            p += acc[e];
        }
        pos[64] = p;
    }
    __syncthreads();
    for (int e = wave; e < na; e += nw) {
        if (lane < acc[e]) {
            const int32_t m = rh[(int64_t)A[e] * h + lane];
            cand[pos[e] + lane] = (m >= 0 && m < n) ? (uint32_t)m : KR_NONE;
        }
    }
    const int total = pos[64];
    const int P = kr_pow2(total);
    for (int e = total + threadIdx.x; e < P; e += blockDim.x) cand[e] = KR_NONE;
    kr_bitonic(cand, P);
    return P;
}

// the distinct ids of sorted[0, P) to outc, ascending; one wave calls it (all 64 lanes) and every lane gets the count
__device__ int kr_unique(const uint32_t *sorted, int P, uint32_t *outc)
{
    const int lane = threadIdx.x & 63;
    int count = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int p = p0 + lane;
        uint32_t v = KR_NONE;
        bool head = false;
        if (p < P) {
            v = sorted[p];
            head = v != KR_NONE && (p == 0 || sorted[p - 1] != v);
        }
        const uint64_t mask = __ballot(head);
        if (head) outc[count + __builtin_popcountll(mask & ((1ull << lane) - 1))] = v;
        count += __builtin_popcountll(mask);
    }
    return count;
}

__device__ __forceinline__ float kr_weight(float s) { return s != s ? 0.0f : expf(fmaf(2.0f, s, -2.0f)); }

// the exact chain of rows i and j (mdx_exact.h: k ascending from +0, continued over zeros to round_up(d, 64))
__device__ float kr_chain(const float *__restrict__ rows, int64_t ld, int64_t d, int64_t i, int64_t j, bool vec)
{
    float acc = 0.0f;
    for (int64_t k = 0; k < d; k += 4) acc = chain_step4(acc, row_piece(rows, i, ld, d, k, vec), row_piece(rows, j, ld, d, k, vec));
    if (d != chain_pad(d)) acc = __builtin_fmaf(0.0f, 0.0f, acc);
    return acc;
}

// ------------------------------------------------------------------------------------------------------ reciprocal sets

__global__ __launch_bounds__(256) void krecip_sets_kernel(const int64_t *__restrict__ ids, int64_t n, int k, int h,
                                                          int32_t *__restrict__ rk, int32_t *__restrict__ rk_counts,
                                                          int32_t *__restrict__ rh, int32_t *__restrict__ rh_counts)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                              // whole waves only
    const int64_t *li = ids + i * k;
    int64_t j = -1;
    int tpos = -1;
    if (lane < k) {
        j = li[lane];
        bool first = true;                                           // a repeated id: only its first copy
        for (int t = 0; t < lane; ++t)
            if (li[t] == j) {
                first = false;
                break;
            }
        if (first && j >= 0 && j < n) {
            const int64_t *lj = ids + j * k;
            for (int t = 0; t < k; ++t)
                if (lj[t] == i) {
                    tpos = t;
                    break;
                }
        }
    }
    const bool keepk = tpos >= 0, keeph = tpos >= 0 && tpos < h && lane < h;
    const uint64_t mk = __ballot(keepk), mh = __ballot(keeph), below = (1ull << lane) - 1;
    const int ck = __builtin_popcountll(mk), ch = __builtin_popcountll(mh);
    if (keepk) rk[i * k + __builtin_popcountll(mk & below)] = (int32_t)j;
    if (keeph) rh[i * h + __builtin_popcountll(mh & below)] = (int32_t)j;
    if (lane >= ck && lane < k) rk[i * k + lane] = -1;               // defined padding
    if (lane >= ch && lane < h) rh[i * h + lane] = -1;
    if (lane == 0) {
        rk_counts[i] = ck;
        rh_counts[i] = ch;
    }
}

// ------------------------------------------------------------------------------------------------------------ raw codes

// counts in offsets[0, n) -> exclusive offsets in place, the total in offsets[n]; one workgroup, every thread a contiguous run
__global__ __launch_bounds__(1024) void krecip_scan_kernel(int64_t *offsets, int64_t n)
{
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += offsets[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int w = 0; w < 1024; ++w) {
            const int64_t v = part[w];
            part[w] = run;
            run += v;
        }
        offsets[n] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t v = offsets[i];
        offsets[i] = run;
        run += v;
    }
}

// bytes of dynamic LDS of krecip_raw_kernel: cand u32 [pow2(cap)], uq u32 [cap], wq f32 [cap], A u32 [64], acc [64], pos [65], t
__host__ __device__ inline int64_t kr_raw_lds(int64_t k) { return 4 * (kr_pow2((int)kr_code_cap(k)) + 2 * kr_code_cap(k) + 64 + 64 + 65 + 3); }

template <bool FILL>
__global__ __launch_bounds__(64) void krecip_raw_kernel(const float *__restrict__ rows, int64_t ld, int64_t d, bool vec,
                                                        const int64_t *__restrict__ ids, const float *__restrict__ sims, int64_t n,
                                                        int k, int h, const int32_t *__restrict__ rk,
                                                        const int32_t *__restrict__ rk_counts, const int32_t *__restrict__ rh,
                                                        const int32_t *__restrict__ rh_counts, int64_t *offsets,
                                                        int32_t *__restrict__ cols, float *__restrict__ vals, int64_t nnz)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int cap = (int)kr_code_cap(k), lane = threadIdx.x;
    uint32_t *cand = (uint32_t *)lds, *uq = cand + kr_pow2(cap), *A = uq + cap + cap;
    float *wq = (float *)(uq + cap), *tsum = (float *)(A + 64 + 64 + 65);
    int *acc = (int *)(A + 64), *pos = acc + 64;
    const int64_t i = blockIdx.x;
    int na = rk_counts[i];
    na = na < 0 ? 0 : (na > k ? k : na);
    if (lane < na) {
        const int32_t c = rk[i * k + lane];
        A[lane] = (c >= 0 && c < n) ? (uint32_t)c : KR_NONE;
    }
    __syncthreads();
    const int P = kr_candidates(A, na, rh, rh_counts, n, h, cand, acc, pos);
    const int cnt = kr_unique(cand, P, uq);
    if (!FILL) {
        if (lane == 0) offsets[i] = cnt;
        return;
    }
    __syncthreads();
    const int64_t *li = ids + i * k;
    for (int e = lane; e < cnt; e += 64) {
        const int64_t j = uq[e];
        float s = 0.0f;
        int t = 0;
        for (; t < k; ++t)
            if (li[t] == j) break;
        s = t < k ? sims[i * k + t] : kr_chain(rows, ld, d, i, j, vec);
        wq[e] = kr_weight(s);
    }
    __syncthreads();
    if (lane == 0) {
        float t = 0.0f;
        for (int e = 0; e < cnt; ++e) t += wq[e];                    // fp32 sequential sum in ascending-id order
        *tsum = t;
    }
    __syncthreads();
    const float t = *tsum;
    const int64_t lo = offsets[i], room = offsets[i + 1] - lo;
    for (int e = lane; e < cnt; e += 64) {
        if (lo < 0 || e >= room || lo + e >= nnz) break;             // offsets of another call: nothing outside [0, nnz)
        cols[lo + e] = (int32_t)uq[e];
        vals[lo + e] = t > 0.0f ? wq[e] / t : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------- expanded codes

// The merge of up to `terms` sorted CSR rows, shared by the database side and the query: keys[0, total) hold
// column << 32 | gather position, gv the values at the gather positions.  Sorts, then wave 0 walks the distinct columns in
// ascending order: column and sum / c to (oc, ov)[0, count), each guarded by `room`.  Every thread calls it; returns the count
// in wave 0 (other waves get 0).
template <bool FILL, typename CT>
__device__ int kr_merge(uint64_t *keys, const float *gv, int total, float c, CT *oc, float *ov, int64_t room)
{
    const int P = kr_pow2(total);
    for (int e = total + threadIdx.x; e < P; e += blockDim.x) keys[e] = ~0ull;
    kr_bitonic(keys, P);
    if (threadIdx.x >= 64) return 0;
    const int lane = threadIdx.x;
    int count = 0;
    for (int p0 = 0; p0 < total; p0 += 64) {
        const int p = p0 + lane;
        uint32_t col = 0;
        bool head = false;
        if (p < total) {
            col = (uint32_t)(keys[p] >> 32);
            head = p == 0 || (uint32_t)(keys[p - 1] >> 32) != col;
        }
        const uint64_t mask = __ballot(head);
        if (FILL && head) {
            float s = gv[(uint32_t)keys[p]];                         // the run is in list order: a sequential fp32 sum
            for (int x = p + 1; x < total && (uint32_t)(keys[x] >> 32) == col; ++x) s += gv[(uint32_t)keys[x]];
            const int64_t at = count + __builtin_popcountll(mask & ((1ull << lane) - 1));
            if (at < room) {
                oc[at] = (CT)col;
                ov[at] = s / c;
            }
        }
        count += __builtin_popcountll(mask);
    }
    return count;
}

__device__ __forceinline__ int64_t kr_clamp(int64_t x, int64_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// bytes of dynamic LDS of krecip_expand_kernel: keys u64 [pow2(cap)], gv f32 [cap], base int [65], c
__host__ __device__ inline int64_t kr_expand_lds(int64_t k, int64_t k2)
{
    return 8 * kr_pow2((int)kr_qe_cap(k, k2)) + 4 * (kr_qe_cap(k, k2) + 65 + 1);
}

template <bool FILL>
__global__ __launch_bounds__(64) void krecip_expand_kernel(const int64_t *__restrict__ ids, int64_t n, int k, int kk,
                                                           const int64_t *__restrict__ raw_offsets,
                                                           const int32_t *__restrict__ raw_cols,
                                                           const float *__restrict__ raw_vals, int64_t raw_nnz, int64_t *offsets,
                                                           int32_t *__restrict__ cols, float *__restrict__ vals, int64_t nnz)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int cap = (int)kr_qe_cap(k, kk), lane = threadIdx.x;
    uint64_t *keys = (uint64_t *)lds;
    float *gv = (float *)(keys + kr_pow2(cap));
    int *base = (int *)(gv + cap), *present = base + 65;
    const int64_t i = blockIdx.x;
    const int64_t *li = ids + i * k;
    if (lane == 0) {
        int p = 0, c = 0;
        for (int t = 0; t < kk; ++t) {
            const int64_t g = li[t];
            bool ok = g >= 0 && g < n;
            for (int u = 0; ok && u < t; ++u) ok = li[u] != g;       // a repeated id: only its first copy
            int64_t len = 0;
            if (ok) {
                ++c;
                len = kr_clamp(raw_offsets[g + 1], raw_nnz) - kr_clamp(raw_offsets[g], raw_nnz);
                len = len < 0 ? 0 : (len > cap - p ? cap - p : len);
            }
            base[t] = p;
            p += (int)len;
        }
        base[kk] = p;
        *present = c;
    }
    __syncthreads();
    for (int t = 0; t < kk; ++t) {
        const int len = base[t + 1] - base[t];
        if (len == 0) continue;
        const int64_t lo = kr_clamp(raw_offsets[li[t]], raw_nnz);
        for (int e = lane; e < len; e += 64) {
            const int x = base[t] + e;
            keys[x] = (uint64_t)(uint32_t)raw_cols[lo + e] << 32 | (uint32_t)x;
            if (FILL) gv[x] = raw_vals[lo + e];
        }
    }
    const int total = base[kk];
    int64_t lo = 0, room = 0;
    if (FILL) {
        lo = offsets[i];
        room = offsets[i + 1] - lo;
        if (lo < 0 || lo > nnz) room = 0;
        if (room > nnz - lo) room = nnz - lo;
    }
    const int cnt = kr_merge<FILL>(keys, gv, total, (float)*present, cols + lo, vals + lo, room);
    if (!FILL && lane == 0) offsets[i] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------- query

// dynamic LDS of krecip_rerank_kernel, in 4-byte words: keys u64 [4096] | gv [4096] | cand / qc [4096] | qv [4096] | uq [2112] |
// wq [2112] | A [64] | acc [64] | pos [65] | scalars [8]
constexpr int KR_Q_LDS = 4 * (2 * KR_MAX_NNZ + 3 * KR_MAX_NNZ + 2 * KR_MAX_CAND + 64 + 64 + 65 + 8);

__global__ __launch_bounds__(KR_Q_THREADS) void krecip_rerank_kernel(
    const int32_t *__restrict__ rh, const int32_t *__restrict__ rh_counts, const float *__restrict__ kth, int64_t n, int k, int h,
    int kk, const int64_t *__restrict__ raw_offsets, const int32_t *__restrict__ raw_cols, const float *__restrict__ raw_vals,
    int64_t raw_nnz, const int64_t *__restrict__ qe_offsets, const int32_t *__restrict__ qe_cols,
    const float *__restrict__ qe_vals, int64_t qe_nnz, const float *scores, int64_t ld_scores,
    const int64_t *__restrict__ top_ids, int r, float lam, char *__restrict__ ws, int64_t ws_stride)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint64_t *keys = (uint64_t *)lds;
    float *gv = (float *)(keys + KR_MAX_NNZ);
    uint32_t *cand = (uint32_t *)(gv + KR_MAX_NNZ), *qc = cand;      // the candidates are dead when the code is stored
    float *qv = (float *)(cand + KR_MAX_NNZ);
    uint32_t *uq = (uint32_t *)(qv + KR_MAX_NNZ);
    float *wq = (float *)(uq + KR_MAX_CAND);
    uint32_t *A = (uint32_t *)(wq + KR_MAX_CAND);
    int *acc = (int *)(A + 64), *pos = acc + 64, *sc = pos + 65;      // sc: 0 na, 1 nu, 2 total, 3 present, 4 nqv; 5 t (float)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t q = blockIdx.x;
    const int64_t *tq = top_ids + q * r;
    const float *sq = scores + q * ld_scores;
    float *F = (float *)(ws + q * ws_stride);
    const int cap = (int)kr_qe_cap(k, kk);

    // R(q): the entries g of the first min(k, r) of T_q with s_qg >= the k-th score of g's own list (q would enter it)
    if (wave == 0) {
        const int kn = k < r ? k : r;
        bool keep = false;
        int64_t g = -1;
        if (lane < kn) {
            g = tq[lane];
            bool ok = g >= 0 && g < n;
            for (int u = 0; ok && u < lane; ++u) ok = tq[u] != g;
            keep = ok && sq[g] >= kth[g];                            // fp32 compare: NaN is false
        }
        const uint64_t mask = __ballot(keep);
        if (keep) A[__builtin_popcountll(mask & ((1ull << lane) - 1))] = (uint32_t)g;
        if (lane == 0) sc[0] = __builtin_popcountll(mask);
    }
    __syncthreads();
    const int na = sc[0];
    const int P = kr_candidates(A, na, rh, rh_counts, n, h, cand, acc, pos);
    if (wave == 0) {
        const int nu = kr_unique(cand, P, uq);
        if (lane == 0) sc[1] = nu;
    }
    __syncthreads();
    const int nu = sc[1];
    for (int e = t; e < nu; e += KR_Q_THREADS) wq[e] = kr_weight(sq[uq[e]]);
    __syncthreads();
    if (t == 0) {
        float s = 0.0f;
        for (int e = 0; e < nu; ++e) s += wq[e];                     // fp32 sequential sum in ascending-id order
        ((float *)sc)[5] = s;
        // the gather plan: V_q first, then the raw codes of the best k2 - 1 rows in list order
        int p = nu < cap ? nu : cap, c = 1;
        pos[0] = p;
        for (int u = 0; u + 1 < kk; ++u) {
            int64_t len = 0;
            if (u < r) {
                const int64_t g = tq[u];
                bool ok = g >= 0 && g < n;
                for (int v = 0; ok && v < u; ++v) ok = tq[v] != g;
                if (ok) {
                    ++c;
                    len = kr_clamp(raw_offsets[g + 1], raw_nnz) - kr_clamp(raw_offsets[g], raw_nnz);
                    len = len < 0 ? 0 : (len > cap - p ? cap - p : len);
                }
            }
            p += (int)len;
            pos[u + 1] = p;
        }
        sc[2] = p;
        sc[3] = c;
    }
    __syncthreads();
    const float tsum = ((float *)sc)[5];
    for (int e = t; e < pos[0]; e += KR_Q_THREADS) {
        keys[e] = (uint64_t)uq[e] << 32 | (uint32_t)e;
        gv[e] = tsum > 0.0f ? wq[e] / tsum : 0.0f;
    }
    for (int u = 0; u + 1 < kk; ++u) {
        const int len = pos[u + 1] - pos[u];
        if (len == 0) continue;
        const int64_t lo = kr_clamp(raw_offsets[tq[u]], raw_nnz);
        for (int e = t; e < len; e += KR_Q_THREADS) {
            const int x = pos[u] + e;
            keys[x] = (uint64_t)(uint32_t)raw_cols[lo + e] << 32 | (uint32_t)x;
            gv[x] = raw_vals[lo + e];
        }
    }
    __syncthreads();
    const int nqv0 = kr_merge<true>(keys, gv, sc[2], (float)sc[3], qc, qv, (int64_t)KR_MAX_NNZ);
    if (t == 0) sc[4] = nqv0;
    __syncthreads();
    const int nqv = sc[4];

    // one wave per shortlist entry: m = sum_j min(V'_q[j], V'_g[j]) over the columns of V'_g
    for (int a = wave; a < r; a += KR_Q_THREADS / 64) {
        const int64_t g = tq[a];
        float val = 0.0f;
        if (g >= 0 && g < n) {                                       // wave-uniform
            const int64_t lo = kr_clamp(qe_offsets[g], qe_nnz), hi = kr_clamp(qe_offsets[g + 1], qe_nnz);
            float part = 0.0f;
            for (int64_t e = lo + lane; e < hi; e += 64) {
                const uint32_t col = (uint32_t)qe_cols[e];
                int b = 0, len = nqv;
                while (len > 0) {
                    const int half = len >> 1;
                    if (qc[b + half] < col) {
                        b += half + 1;
                        len -= half + 1;
                    } else {
                        len = half;
                    }
                }
                if (b < nqv && qc[b] == col) part += fminf(qv[b], qe_vals[e]);
            }
            const float m = wave_sum(part);
            const float s = sq[g];
            val = fmaf(1.0f - lam, m / (2.0f - m), lam * (0.5f * (1.0f + s)));
        }
        if (lane == 0) F[a] = val;
    }
}

// out[q, j] = scores[q, j] - 3, 4096 entries of one row per workgroup (VEC: 16-byte aligned rows, float4)
template <bool VEC>
__global__ __launch_bounds__(256) void krecip_base_kernel(const float *scores, int64_t ld_scores, float *out, int64_t ld_out,
                                                          int64_t n, int64_t nblk)
{
    const int64_t q = blockIdx.x / nblk, j0 = (blockIdx.x - q * nblk) * (int64_t)4096;
    const float *s = scores + q * ld_scores;
    float *o = out + q * ld_out;
    if (VEC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t j = j0 + (u * 256 + threadIdx.x) * 4;
            if (j + 4 <= n) {
                float4 v = *(const float4 *)(s + j);
                v.x -= 3.0f; v.y -= 3.0f; v.z -= 3.0f; v.w -= 3.0f;
                *(float4 *)(o + j) = v;
            } else {
                for (; j < n; ++j) o[j] = s[j] - 3.0f;
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int64_t j = j0 + u * 256 + threadIdx.x;
            if (j < n) o[j] = s[j] - 3.0f;
        }
    }
}

// out[q, t_a] = the value of shortlist entry a (the copies of a repeated id hold the same bits)
__global__ __launch_bounds__(256) void krecip_scatter_kernel(const char *__restrict__ ws, int64_t ws_stride, int64_t r,
                                                             const int64_t *__restrict__ top_ids, int64_t n, int64_t nq, float *out,
                                                             int64_t ld_out)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= nq * r) return;
    const int64_t q = x / r, a = x - q * r;
    const int64_t id = top_ids[x];
    if (id >= 0 && id < n) out[q * ld_out + id] = ((const float *)(ws + q * ws_stride))[a];
}

static bool kr_overlaps(const void *a, int64_t bytes_a, const void *b, int64_t bytes_b)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

static int64_t kr_ws_stride(int64_t r) { return round_up(r * (int64_t)sizeof(float), 256); }

}  // namespace mdx

using namespace mdx;

// n and k of every call: the lists are [n, k], cols are int32
#define KR_CHECK_NK(who)                                                                                                    \
    do {                                                                                                                    \
        MDX_CHECK_ARG(n >= 1 && k >= 1, "%s: n=%lld k=%lld (each must be >= 1)", who, (long long)n, (long long)k);         \
        MDX_CHECK_ARG(n < (1ll << 31), "%s: n=%lld must be < 2^31 (columns are int32)", who, (long long)n);                \
        MDX_CHECK_ARG(k <= MDX_KRECIP_MAX_K1, "%s: k=%lld > MDX_KRECIP_MAX_K1 = %d", who, (long long)k, MDX_KRECIP_MAX_K1); \
    } while (0)

#define KR_CHECK_K2(who)                                                                                                     \
    do {                                                                                                                     \
        MDX_CHECK_ARG(k2 >= 1 && k2 <= k, "%s: k2=%lld must be in [1, k] = [1, %lld]", who, (long long)k2, (long long)k);   \
        MDX_CHECK_ARG(k2 * kr_code_cap(k) <= MDX_KRECIP_MAX_NNZ,                                                            \
                      "%s: k2 * k * (1 + ceil(k / 2)) = %lld > MDX_KRECIP_MAX_NNZ = %d (k=%lld k2=%lld)", who,              \
                      (long long)(k2 * kr_code_cap(k)), MDX_KRECIP_MAX_NNZ, (long long)k, (long long)k2);                   \
    } while (0)

extern "C" {

int mdx_krecip_sets(const int64_t *ids, int64_t n, int64_t k, int32_t *rk, int32_t *rk_counts, int32_t *rh, int32_t *rh_counts,
                    void *stream)
{
    MDX_CHECK_ARG(ids && rk && rk_counts && rh && rh_counts,
                  "mdx_krecip_sets: NULL pointer (ids, rk, rk_counts, rh and rh_counts are required)");
    KR_CHECK_NK("mdx_krecip_sets");
    hipLaunchKernelGGL(krecip_sets_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream, ids, n, (int)k,
                       (int)kr_half(k), rk, rk_counts, rh, rh_counts);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_krecip_raw_offsets(int64_t n, int64_t k, const int32_t *rk, const int32_t *rk_counts, const int32_t *rh,
                           const int32_t *rh_counts, int64_t *offsets, void *stream)
{
    MDX_CHECK_ARG(rk && rk_counts && rh && rh_counts && offsets,
                  "mdx_krecip_raw_offsets: NULL pointer (rk, rk_counts, rh, rh_counts and offsets are required)");
    KR_CHECK_NK("mdx_krecip_raw_offsets");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(krecip_raw_kernel<false>, dim3((unsigned)n), dim3(64), (unsigned)kr_raw_lds(k), s, (const float *)nullptr,
                       (int64_t)0, (int64_t)0, false, (const int64_t *)nullptr, (const float *)nullptr, n, (int)k, (int)kr_half(k),
                       rk, rk_counts, rh, rh_counts, offsets, (int32_t *)nullptr, (float *)nullptr, (int64_t)0);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(krecip_scan_kernel, dim3(1), dim3(1024), 0, s, offsets, n);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_krecip_raw_fill(const float *rows, int64_t ld, int64_t d, const int64_t *ids, const float *sims, int64_t n, int64_t k,
                        const int32_t *rk, const int32_t *rk_counts, const int32_t *rh, const int32_t *rh_counts,
                        const int64_t *offsets, int32_t *cols, float *vals, int64_t nnz, void *stream)
{
    MDX_CHECK_ARG(rows && ids && sims && rk && rk_counts && rh && rh_counts && offsets && (nnz == 0 || (cols && vals)),
                  "mdx_krecip_raw_fill: NULL pointer (rows, ids, sims, rk, rk_counts, rh, rh_counts and offsets are required, "
                  "cols and vals unless nnz == 0)");
    KR_CHECK_NK("mdx_krecip_raw_fill");
    MDX_CHECK_ARG(d >= 1 && ld >= d, "mdx_krecip_raw_fill: d=%lld ld=%lld (d >= 1 and ld >= d)", (long long)d, (long long)ld);
    MDX_CHECK_ARG(nnz >= 0, "mdx_krecip_raw_fill: nnz=%lld must be >= 0", (long long)nnz);
    if (nnz == 0) return MDX_OK;
    const bool vec = ((uintptr_t)rows & 15) == 0 && ld % 4 == 0;
    hipLaunchKernelGGL(krecip_raw_kernel<true>, dim3((unsigned)n), dim3(64), (unsigned)kr_raw_lds(k), (hipStream_t)stream, rows, ld,
                       d, vec, ids, sims, n, (int)k, (int)kr_half(k), rk, rk_counts, rh, rh_counts, (int64_t *)offsets, cols, vals,
                       nnz);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_krecip_expand_offsets(const int64_t *ids, int64_t n, int64_t k, int64_t k2, const int64_t *raw_offsets,
                              const int32_t *raw_cols, int64_t raw_nnz, int64_t *offsets, void *stream)
{
    MDX_CHECK_ARG(ids && raw_offsets && offsets && (raw_nnz == 0 || raw_cols),
                  "mdx_krecip_expand_offsets: NULL pointer (ids, raw_offsets and offsets are required, raw_cols unless "
                  "raw_nnz == 0)");
    KR_CHECK_NK("mdx_krecip_expand_offsets");
    KR_CHECK_K2("mdx_krecip_expand_offsets");
    MDX_CHECK_ARG(raw_nnz >= 0, "mdx_krecip_expand_offsets: raw_nnz=%lld must be >= 0", (long long)raw_nnz);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(krecip_expand_kernel<false>, dim3((unsigned)n), dim3(64), (unsigned)kr_expand_lds(k, k2), s, ids, n, (int)k,
                       (int)k2, raw_offsets, raw_cols, (const float *)nullptr, raw_nnz, offsets, (int32_t *)nullptr,
                       (float *)nullptr, (int64_t)0);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(krecip_scan_kernel, dim3(1), dim3(1024), 0, s, offsets, n);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_krecip_expand_fill(const int64_t *ids, int64_t n, int64_t k, int64_t k2, const int64_t *raw_offsets,
                           const int32_t *raw_cols, const float *raw_vals, int64_t raw_nnz, const int64_t *offsets, int32_t *cols,
                           float *vals, int64_t nnz, void *stream)
{
    MDX_CHECK_ARG(ids && raw_offsets && offsets && (raw_nnz == 0 || (raw_cols && raw_vals)) && (nnz == 0 || (cols && vals)),
                  "mdx_krecip_expand_fill: NULL pointer (ids, raw_offsets and offsets are required, raw_cols and raw_vals unless "
                  "raw_nnz == 0, cols and vals unless nnz == 0)");
    KR_CHECK_NK("mdx_krecip_expand_fill");
    KR_CHECK_K2("mdx_krecip_expand_fill");
    MDX_CHECK_ARG(raw_nnz >= 0 && nnz >= 0, "mdx_krecip_expand_fill: raw_nnz=%lld nnz=%lld (each must be >= 0)",
                  (long long)raw_nnz, (long long)nnz);
    if (nnz == 0) return MDX_OK;
    hipLaunchKernelGGL(krecip_expand_kernel<true>, dim3((unsigned)n), dim3(64), (unsigned)kr_expand_lds(k, k2),
                       (hipStream_t)stream, ids, n, (int)k, (int)k2, raw_offsets, raw_cols, raw_vals, raw_nnz, (int64_t *)offsets,
                       cols, vals, nnz);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_krecip_rerank_workspace(int64_t nq, int64_t r)
{
    if (nq < 1 || nq >= (1ll << 31) || r < 1 || r > MDX_KRECIP_MAX_R) return 0;
    return nq * kr_ws_stride(r);
}

int mdx_krecip_rerank(const int32_t *rh, const int32_t *rh_counts, const float *kth, int64_t n, int64_t k, int64_t k2,
                      const int64_t *raw_offsets, const int32_t *raw_cols, const float *raw_vals, int64_t raw_nnz,
                      const int64_t *qe_offsets, const int32_t *qe_cols, const float *qe_vals, int64_t qe_nnz, const float *scores,
                      int64_t ld_scores, const int64_t *top_ids, int64_t nq, int64_t r, float lam, float *out, int64_t ld_out,
                      void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(rh && rh_counts && kth && raw_offsets && qe_offsets && scores && top_ids && out && workspace &&
                      (raw_nnz == 0 || (raw_cols && raw_vals)) && (qe_nnz == 0 || (qe_cols && qe_vals)),
                  "mdx_krecip_rerank: NULL pointer (rh, rh_counts, kth, raw_offsets, qe_offsets, scores, top_ids, out and "
                  "workspace are required, the columns and values of a CSR unless its nnz == 0)");
    KR_CHECK_NK("mdx_krecip_rerank");
    KR_CHECK_K2("mdx_krecip_rerank");
    MDX_CHECK_ARG(nq >= 1 && r >= 1, "mdx_krecip_rerank: nq=%lld r=%lld (each must be >= 1)", (long long)nq, (long long)r);
    MDX_CHECK_ARG(r <= MDX_KRECIP_MAX_R && r <= n, "mdx_krecip_rerank: r=%lld must be <= MDX_KRECIP_MAX_R = %d and <= n=%lld",
                  (long long)r, MDX_KRECIP_MAX_R, (long long)n);
    MDX_CHECK_ARG(nq * ceil_div(n, 4096) < (1ll << 31), "mdx_krecip_rerank: nq=%lld too large for n=%lld (split the queries)",
                  (long long)nq, (long long)n);
    MDX_CHECK_ARG(nq * r < (1ll << 39), "mdx_krecip_rerank: nq * r = %lld too large (split the queries)", (long long)(nq * r));
    MDX_CHECK_ARG(raw_nnz >= 0 && qe_nnz >= 0, "mdx_krecip_rerank: raw_nnz=%lld qe_nnz=%lld (each must be >= 0)",
                  (long long)raw_nnz, (long long)qe_nnz);
    MDX_CHECK_ARG(ld_scores >= n && ld_out >= n, "mdx_krecip_rerank: ld_scores=%lld ld_out=%lld must be >= n=%lld",
                  (long long)ld_scores, (long long)ld_out, (long long)n);
    MDX_CHECK_ARG(isfinite(lam) && lam >= 0.0f && lam <= 1.0f, "mdx_krecip_rerank: lam=%g must be in [0, 1]", (double)lam);
    const int64_t span = ((nq - 1) * ld_out + n) * (int64_t)sizeof(float);
    MDX_CHECK_ARG((out == scores && ld_out == ld_scores) ||
                      !kr_overlaps(out, span, scores, ((nq - 1) * ld_scores + n) * (int64_t)sizeof(float)),
                  "mdx_krecip_rerank: out overlaps scores (only out == scores with the same stride is allowed)");
    const int64_t need = mdx_krecip_rerank_workspace(nq, r);
    MDX_CHECK_WORKSPACE("mdx_krecip_rerank", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    auto solve = krecip_rerank_kernel;
    MDX_HIP(hipFuncSetAttribute((const void *)solve, hipFuncAttributeMaxDynamicSharedMemorySize, KR_Q_LDS));
    hipLaunchKernelGGL(solve, dim3((unsigned)nq), dim3(KR_Q_THREADS), (unsigned)KR_Q_LDS, s, rh, rh_counts, kth, n, (int)k,
                       (int)kr_half(k), (int)k2, raw_offsets, raw_cols, raw_vals, raw_nnz, qe_offsets, qe_cols, qe_vals, qe_nnz,
                       scores, ld_scores, top_ids, (int)r, lam, (char *)workspace, kr_ws_stride(r));
    MDX_LAUNCH_CHECK();
    const int64_t nblk = ceil_div(n, 4096);
    const bool vec = (((uintptr_t)scores | (uintptr_t)out) & 15) == 0 && ld_scores % 4 == 0 && ld_out % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(krecip_base_kernel<true>, dim3((unsigned)(nq * nblk)), dim3(256), 0, s, scores, ld_scores, out, ld_out,
                           n, nblk);
    else
        hipLaunchKernelGGL(krecip_base_kernel<false>, dim3((unsigned)(nq * nblk)), dim3(256), 0, s, scores, ld_scores, out, ld_out,
                           n, nblk);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(krecip_scatter_kernel, dim3((unsigned)ceil_div(nq * r, 256)), dim3(256), 0, s, (const char *)workspace,
                       kr_ws_stride(r), r, top_ids, n, nq, out, ld_out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
