// Exact range search, self-join and kNN join, pruned on the int8 shard (include/mdx.h, "exact range search and self-join",
// "exact kNN join").
//
//   join_stats_kernel     one wave per row: ||x||_1 (float64), max |x|, finiteness and ||c||_1 of the row's int8 codes ->
//                         the four per-row factors {scale, q, r, w} of the pruning bound, rounded up to fp32.
//   join_kernel           one workgroup per (I, J) block of 128 x 128 rows of two int8 shards A and B: both operands are
//                         staged in LDS a 64-k chunk at a time (double buffer, one barrier per chunk), every wave multiplies
//                         64 x 64 rows on v_mfma_i32_16x16x64_i8 (exact int32 sums), and the epilogue forms the MDX_I8 score
//                         of each pair and tests it against tau - beta_ij.  Candidates leave through a wave prefix sum, ONE
//                         global atomic per wave that has any, and 8-byte stores; the count runs on past the capacity.
//   knn_bound_kernel      the exact kNN join (include/mdx.h, "exact kNN join"): the same block body, one workgroup per 128 rows of A and
//                         slice of the J blocks; per row the k largest lower bounds l_ij of the exact chain stay in LDS, fed through
//                         an LDS queue; knn_select_kernel takes the k-th largest of a row's slices.  join_kernel<., ROWS> then reads
//                         its threshold per row, and knn_dense_kernel writes the first k of every row's sorted candidates.
//   exact_kernel          one workgroup per 64 sorted candidates: the A and B row pieces are staged in LDS 128 k at a time
//                         and wave 0 runs the chains of mdx_rescore (lane = candidate): the row loader, the stage arithmetic
//                         and the four-link chain step are those of mdx_exact.h, shared with rescore_kernel.
//   select_count/_write   the dense threshold compaction of an fp32 score matrix (one workgroup per row, ordered).
//   the final order       one stable radix sort of (row, desc_key(score)) keys whose input is in (row, id) order, then a
//                         gather and a binary search per row for the CSR offsets.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "mdx_exact.h"

namespace mdx {
namespace {

constexpr int JB_TILES = 8;                     // row tiles (of 16 rows) per block side: 128 rows
constexpr int JB_ROWS = JB_TILES * 16;
constexpr int J_GROUP = 16;                     // I blocks that run side by side over the J blocks (L2 reuse of both operands)
constexpr double E_Q = 0.5 + 0x1p-15;           // E of the MDX_I8 bound
constexpr float TINY = 0x1p-149f;               // floor of the factors: inf * factor is never NaN

// ---------------------------------------------------------------- per-row factors

__global__ __launch_bounds__(256) void join_stats_kernel(const i32x4 *__restrict__ tiles, const float *__restrict__ scales, int64_t n,
                                                         int64_t KB, const float *__restrict__ rows, int64_t ld, int64_t d,
                                                         f32x4 *__restrict__ stats)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;                                        // wave-uniform
    double l1 = 0.0;
    float a = 0.f;
    int bad = 0;
    for (int64_t k = lane; k < d; k += 64) {
        const float x = rows[row * ld + k];
        bad |= !__builtin_isfinite(x);
        l1 += (double)fabsf(x);
        a = fmaxf(a, fabsf(x));
    }
    // ||c||_1 from the row's codes: tile (row / 16, kb), lane (g, row % 16) holds 16 codes of k group g
    const int64_t rt = row >> 4;
    const int j = (int)(row & 15);
    uint32_t c1 = 0;
    for (int64_t kb = lane >> 2; kb < KB; kb += 16) {
        const i32x4 w = tiles[(rt * KB + kb) * 64 + (lane & 3) * 16 + j];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = (int)(int8_t)(uint8_t)((uint32_t)w[e >> 2] >> (8 * (e & 3)));
            c1 += (uint32_t)(c < 0 ? -c : c);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l1 += __shfl_xor(l1, o, 64);
        a = fmaxf(a, __shfl_xor(a, o, 64));
        bad |= __shfl_xor(bad, o, 64);
        c1 += __shfl_xor(c1, o, 64);
    }
    if (lane != 0) return;
    const float sc = scales[row];
    // a zero row (a == 0) scores exactly 0; any other row needs a scale in [2^-106, 2^40] -- a nonzero row whose scale rounded
    // to 0 (a subnormal max |x|) has scale c = 0 and an error of x itself, which no scale-proportional term covers
    const bool covered = !bad && (a == 0.f || (sc >= 0x1p-106f && sc <= 0x1p40f));
    f32x4 st;
    st[0] = sc;
    if (covered) {
        const double ud = (double)d * 0x1p-24, gamma = ud / (1.0 - ud);
        // float64 rounding: ||x||_1 errs by at most d 2^-53 of itself, every other operation by 2^-53: (1 + (d + 16) 2^-52) covers it
        const double slack = 1.0 + ((double)d + 16.0) * 0x1p-52;
        st[1] = fmaxf(up_f32(E_Q * l1 * slack), TINY);                                   // q = E ||x||_1
        st[2] = fmaxf(up_f32(E_Q * (double)sc * (double)c1 * slack), TINY);              // r = E scale ||c||_1
        st[3] = fmaxf(up_f32(((double)sc + gamma * (double)a / E_Q) * slack), TINY);     // w = scale + gamma_d max|x| / E
    } else {
        st[1] = st[2] = st[3] = __builtin_inff();
    }
    stats[row] = st;
}

// ---------------------------------------------------------------- the join kernel

// beta of x in the query role and y in the database role, rounded up (include/mdx.h): b >= beta + 2^-150
__device__ __forceinline__ float beta_up(f32x4 x, f32x4 y, float c0)
{
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(x[1], y[3]), __fmul_rn(y[2], fmaxf(x[0], TINY))), c0);
    return __fmul_rn(s, 1.0f + 0x1p-20f);
}

// The block body of the join and the kNN bound kernel: acc = the int32 code products of the 128 rows of A block I against the 128
// rows of B block J; wave (wa, wb) holds its 64 x 64 corner as 4 x 4 MFMA tiles.  16 x 64 tiles of both shards are staged in LDS a
// 64-k chunk at a time (double buffer, one barrier per chunk).  On entry every wave has left both buffers (a fresh workgroup, or
// a barrier since the last call); on exit a wave may still read the last buffer.
__device__ __forceinline__ void block_mma(i32x4 (*lds)[2 * JB_TILES * 64], const i32x4 *__restrict__ a, const i32x4 *__restrict__ b,
                                          int64_t I, int64_t J, int KB, i32x4 (&acc)[4][4])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;                     // the wave's 64 x 64 corner of the block
    // stage loads: thread t moves pieces t, t + 256, t + 512, t + 768 of the 16 tiles (A 0..7, B 8..15) of a chunk
    const i32x4 *src[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = tid + 256 * u, t = p >> 6;
        const int64_t rt = t < JB_TILES ? I * JB_TILES + t : J * JB_TILES + (t - JB_TILES);
        src[u] = (t < JB_TILES ? a : b) + rt * KB * 64 + (p & 63);
    }
    i32x4 reg[4];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int u = 0; u < 4; ++u) reg[u] = src[u][(int64_t)kb * 64];
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int u = 0; u < 4; ++u) lds[buf][tid + 256 * u] = reg[u];
    };
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = (i32x4){0, 0, 0, 0};

    fetch(0);
    put(0);
    __syncthreads();
    for (int kb = 0; kb < KB; ++kb) {
        const bool more = kb + 1 < KB;
        if (more) fetch(kb + 1);                                 // in flight during the MFMAs
        const i32x4 *s = lds[kb & 1];
        i32x4 av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = s[(wa * 4 + r) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = s[(JB_TILES + wb * 4 + c) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[r], bv[c], acc[r][c], 0, 0, 0);
        if (more) {
            put((kb + 1) & 1);                                   // every wave left this buffer before the last barrier
            __syncthreads();
        }
    }
}

// the MDX_I8 score of a pair from its code product and the rounded-up bound b of include/mdx.h (+inf: the pair is not covered)
__device__ __forceinline__ void pair_bound(int acc, f32x4 xs, f32x4 ys, float c0, float &sc, float &bnd)
{
    const float prod = __fmul_rn(ys[0], xs[0]);                              // scale_B * scale_A, as MDX_I8
    sc = __fmul_rn((float)acc, prod);
    bnd = fminf(beta_up(xs, ys, c0), beta_up(ys, xs, c0));
    if (xs[0] > 0.f && ys[0] > 0.f && prod < 0x1p-126f) bnd = __builtin_inff();     // the product may have underflowed
}

// a: the A shard's tiles, b: B's (== a for the self-join).  A blocks [I0, I1) in groups of GS (<= J_GROUP) that sweep every J
// block -- or, symmetric, one group of J_GROUP blocks from I0 against J >= I0.  out: (i << 32 | j) of every candidate, i, j
// global rows of A and B.  ROWS: the threshold of A row i is taus[i - 128 I0] (any fp32 value: -inf or NaN keeps every pair).
template <bool SYM, bool ROWS>
__global__ __launch_bounds__(256, 2) void join_kernel(const i32x4 *__restrict__ a, const f32x4 *__restrict__ sa, int64_t na,
                                                      const i32x4 *__restrict__ b, const f32x4 *__restrict__ sb, int64_t nb, int KB,
                                                      int64_t I0, int64_t I1, int64_t NJ, int GS, float tau, const float *__restrict__ taus,
                                                      float c0, uint64_t *__restrict__ out, int64_t capacity,
                                                      unsigned long long *__restrict__ count)
{
    static_assert(!(SYM && ROWS), "per-row thresholds: the non-symmetric join only");
    __shared__ i32x4 lds[2][2 * JB_TILES * 64];             // [buffer][A tiles, then B tiles][lane]: 2 x 16 KiB
    int64_t I, J;
    const int64_t bid = blockIdx.x;
    if constexpr (SYM) {                                         // J >= I0; I = I0 + (0 .. J_GROUP-1), J >= I
        I = I0 + bid % J_GROUP;
        J = I0 + bid / J_GROUP;
        if (I >= I1 || J < I) return;
    } else {                                                     // groups of GS I blocks sweep every J block
        const int64_t g = bid / (GS * NJ), w = bid % (GS * NJ);
        I = I0 + g * GS + w % GS;
        J = w / GS;
        if (I >= I1) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;                     // the wave's 64 x 64 corner of the block

    i32x4 acc[4][4];
    block_mma(lds, a, b, I, J, KB, acc);

    // Epilogue: lane (g, col) holds rows 4 g .. 4 g + 3 of A tile r against row col of B tile c
    const int g4 = 4 * (lane >> 4), col = lane & 15;
    int64_t jrow[4];
    f32x4 ys[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        jrow[c] = (J * JB_TILES + wb * 4 + c) * 16 + col;
        ys[c] = jrow[c] < nb ? sb[jrow[c]] : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    uint64_t mask = 0;                                           // bit (r * 4 + e) * 4 + c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t irow = (I * JB_TILES + wa * 4 + r) * 16 + g4 + e;
            if (irow >= na) continue;
            const f32x4 xs = sa[irow];
            const float t = ROWS ? taus[irow - I0 * JB_ROWS] : tau;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (jrow[c] >= nb || (SYM && jrow[c] <= irow)) continue;
                float sc, bnd;
                pair_bound(acc[r][c][e], xs, ys[c], c0, sc, bnd);
                const float lhs = __fadd_rn(__fadd_rn(sc, __fmul_rn(fabsf(sc), 0x1p-21f)), bnd);
                if (!(lhs < t)) mask |= 1ull << ((r * 4 + e) * 4 + c);      // a NaN score is a candidate
            }
        }
    }
    const uint32_t mine = (uint32_t)__popcll(mask);
    if (!__any(mine != 0)) return;
    const uint32_t incl = wave_inclusive_sum(mine);
    const uint32_t total = __shfl(incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 63) base = atomicAdd(count, (unsigned long long)total);
    base = __shfl(base, 63, 64);
    int64_t pos = (int64_t)base + (incl - mine);
    while (mask) {
        const int bit = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int r = bit >> 4, e = (bit >> 2) & 3, c = bit & 3;
        const int64_t irow = (I * JB_TILES + wa * 4 + r) * 16 + g4 + e;
        if (pos < capacity) out[pos] = ((uint64_t)irow << 32) | (uint64_t)jrow[c];
        ++pos;
    }
}

// ---------------------------------------------------------------- the kNN bound kernel

constexpr int KNN_MAX_K = 64;                   // MDX_KNN_JOIN_MAX_K: 128 lists of 64 fp32 = 32 KiB of LDS beside 32 KiB of staging
constexpr int KNN_LD = KNN_MAX_K + 1;           // list stride: thread t walks list t, 65 t + c hits 32 banks for 32 lanes
constexpr int KNN_QCAP = 1024;                  // queue entries: one (r, e) step of a whole block (4 waves x 64 lanes x 4 tiles)
constexpr int KNN_MAX_SLICES = 64;              // one lane per list in knn_select_kernel

// l_ij of include/mdx.h ("exact kNN join"): fl(fl(s - fl(2^-21 |s|)) - b) <= chain_ij, or -inf where the pair gives no lower bound
// (b infinite, a NaN score, l not finite); -0 is returned as +0, so that equal values are equal bits
__device__ __forceinline__ float knn_lower(int acc, f32x4 xs, f32x4 ys, float c0)
{
    float sc, bnd;
    pair_bound(acc, xs, ys, c0, sc, bnd);
    const float l = __fsub_rn(__fsub_rn(sc, __fmul_rn(fabsf(sc), 0x1p-21f)), bnd);
    return __builtin_isfinite(l) ? (l == 0.f ? 0.f : l) : -__builtin_inff();
}

// One workgroup per (A block I, slice sl of the J blocks): it sweeps J in [sl NJ / S, (sl + 1) NJ / S) and keeps, per A row, the k
// largest l_ij seen (top, unsorted, thread t < 128 owns row t) and their minimum theta (-inf until the list is full).  Per J block
// the values above theta go through an LDS queue (wave prefix sum, one LDS atomic per wave) and are merged after a barrier; a
// block that overflows the queue (the first ones do) is redone in 16 steps of at most KNN_QCAP values.  Workgroups of one group
// of GS A blocks and one slice are neighbours in the grid and walk J in the same order (L2 reuse of both operands).
// lists [S, m, k]: every list sorted descending, -inf beyond the values it holds.
__global__ __launch_bounds__(256, 2) void knn_bound_kernel(const i32x4 *__restrict__ a, const f32x4 *__restrict__ sa, int64_t na,
                                                           const i32x4 *__restrict__ b, const f32x4 *__restrict__ sb, int64_t nb, int KB,
                                                           int64_t I0, int64_t I1, int64_t NJ, int GS, int S, int k, float c0,
                                                           float *__restrict__ lists, int64_t m)
{
    __shared__ i32x4 lds[2][2 * JB_TILES * 64];             // 32 KiB of staging
    __shared__ float top[JB_ROWS * KNN_LD];                      // 32.5 KiB: the k largest of each row
    __shared__ f32x4 sx[JB_ROWS];                             // the factors of the A rows (zeros beyond the shard)
    __shared__ float theta[JB_ROWS];
    __shared__ float qval[KNN_QCAP];
    __shared__ uint32_t qrow[KNN_QCAP];
    __shared__ uint32_t qn[2];                                   // the queue length, by phase parity: the idle one is zero
    const int64_t bid = blockIdx.x;
    const int64_t g = bid / ((int64_t)GS * S), w = bid % ((int64_t)GS * S);
    const int64_t I = I0 + g * GS + w % GS;
    const int sl = (int)(w / GS);
    if (I >= I1) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave >> 1, wb = wave & 1;
    const int g4 = 4 * (lane >> 4), col = lane & 15;
    const float ninf = -__builtin_inff();

    if (tid < JB_ROWS) {
        theta[tid] = ninf;
        sx[tid] = I * JB_ROWS + tid < na ? sa[I * JB_ROWS + tid] : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (tid < 2) qn[tid] = 0;
    int cnt = 0, amin = 0;                                       // of thread tid < 128: its list's length and the slot of its minimum
    float th = ninf;
    __syncthreads();

    auto rescan = [&]() {
        th = top[tid * KNN_LD];
        amin = 0;
        for (int c = 1; c < k; ++c) {
            const float x = top[tid * KNN_LD + c];
            if (x < th) {
                th = x;
                amin = c;
            }
        }
    };
    auto merge = [&](uint32_t n) {                               // the queue into the lists: each entry by the thread of its row
        if (tid >= JB_ROWS) return;
        for (uint32_t q = 0; q < n; ++q) {
            if (qrow[q] != (uint32_t)tid) continue;
            const float v = qval[q];
            if (cnt < k) {
                top[tid * KNN_LD + cnt++] = v;
                if (cnt == k) rescan();
            } else if (v > th) {                                 // theta may have risen since the value was queued
                top[tid * KNN_LD + amin] = v;
                rescan();
            }
        }
        theta[tid] = th;
    };

    int ph = 0;
    const int64_t j_lo = sl * NJ / S, j_hi = (sl + 1) * NJ / S;
    for (int64_t J = j_lo; J < j_hi; ++J) {
        i32x4 acc[4][4];
        block_mma(lds, a, b, I, J, KB, acc);

        int64_t jrow[4];
        f32x4 ys[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            jrow[c] = (J * JB_TILES + wb * 4 + c) * 16 + col;
            ys[c] = jrow[c] < nb ? sb[jrow[c]] : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        uint64_t mask = 0;                                       // bit (r * 4 + e) * 4 + c: l above the row's theta as it was
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = (wa * 4 + r) * 16 + g4 + e;
                if (I * JB_ROWS + row >= na) continue;
                const float t = theta[row];
                const f32x4 xs = sx[row];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (jrow[c] >= nb) continue;
                    if (knn_lower(acc[r][c][e], xs, ys[c], c0) > t) mask |= 1ull << ((r * 4 + e) * 4 + c);
                }
            }
        }
        // steps [lo, hi) of (r, e) into the queue of phase p; a position beyond the queue is counted and dropped
        auto push = [&](int lo, int hi, int p) {
            const uint64_t mm = hi - lo == 16 ? mask : mask & (((1ull << (4 * (hi - lo))) - 1) << (4 * lo));
            const uint32_t mine = (uint32_t)__popcll(mm);
            if (!__any(mine != 0)) return;                       // wave-uniform
            const uint32_t incl = wave_inclusive_sum(mine);
            const uint32_t total = __shfl(incl, 63, 64);
            uint32_t base = 0;
            if (lane == 63) base = atomicAdd(&qn[p], total);
            base = __shfl(base, 63, 64);
            uint32_t pos = base + (incl - mine);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((mm >> ((r * 4 + e) * 4 + c)) & 1) {
                            if (pos < KNN_QCAP) {
                                const int row = (wa * 4 + r) * 16 + g4 + e;
                                qrow[pos] = (uint32_t)row;
                                qval[pos] = knn_lower(acc[r][c][e], sx[row], ys[c], c0);
                            }
                            ++pos;
                        }
        };
        // after a phase: merge what it queued, clear the idle counter (last read before the previous such barrier), swap
        auto settle = [&](uint32_t n, bool fits) {
            if (fits) merge(n < KNN_QCAP ? n : KNN_QCAP);
            if (tid == 0) qn[ph ^ 1] = 0;
            __syncthreads();
            ph ^= 1;
        };
        push(0, 16, ph);
        __syncthreads();                                         // the queue is whole; every wave has left the staging buffers
        uint32_t n = qn[ph];
        if (n == 0) continue;                                    // uniform: nothing was queued, no list changed
        if (n <= KNN_QCAP) {
            settle(n, true);
            continue;
        }
        settle(n, false);
        for (int step = 0; step < 16; ++step) {
            push(step, step + 1, ph);
            __syncthreads();
            n = qn[ph];
            settle(n, n != 0);                                   // always: the next step adds to a counter nobody still reads
        }
    }

    // the lists leave sorted: larger first, -inf behind what a list holds
    const int64_t irow = I * JB_ROWS + tid;
    if (tid < JB_ROWS && irow < na) {
        float *l = top + tid * KNN_LD;
        for (int i = 1; i < cnt; ++i) {
            const float v = l[i];
            int j = i;
            for (; j > 0 && l[j - 1] < v; --j) l[j] = l[j - 1];
            l[j] = v;
        }
        float *dst = lists + ((int64_t)sl * m + (irow - I0 * JB_ROWS)) * k;
        for (int c = 0; c < k; ++c) dst[c] = c < cnt ? l[c] : ninf;
    }
}

// t[row] = the k-th largest of the union of the row's S sorted lists (one wave per row, lane = list: k pops of the largest head)
__global__ __launch_bounds__(256) void knn_select_kernel(const float *__restrict__ lists, int64_t m, int S, int k, float *__restrict__ t)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= m) return;                                        // wave-uniform
    const float ninf = -__builtin_inff();
    const float *l = lists + ((int64_t)lane * m + row) * k;
    int ptr = 0;
    float head = lane < S ? l[0] : ninf, kth = ninf;
    for (int i = 0; i < k; ++i) {
        kth = wave_max(head);
        const uint64_t who = __ballot(head == kth);
        if (lane == __builtin_ctzll(who)) {
            ++ptr;
            head = lane < S && ptr < k ? l[ptr] : ninf;
        }
    }
    if (lane == 0) t[row] = kth;
}

// ---------------------------------------------------------------- exact stage

constexpr int EX_TC = 64;              // candidates per workgroup: one per lane of wave 0
constexpr int EX_KC = 128;             // k per stage
constexpr int EX_LD = EX_KC + 4;

// sorted candidates (i << 32 | j) -> key (i - m_lo) << 32 | desc_key(chain) for a hit, ~0 otherwise; idx = position.  ALL (the kNN
// join): no threshold, every candidate is kept, a NaN chain too (desc_key ranks it last in its row)
template <bool ALL>
__global__ __launch_bounds__(256) void exact_kernel(const float *__restrict__ ra, int64_t lda, const float *__restrict__ rb, int64_t ldb, int64_t d,
                                                    const uint64_t *__restrict__ cand, int64_t P, float tau, int64_t m_lo, bool vec,
                                                    float *__restrict__ score, uint64_t *__restrict__ key, int32_t *__restrict__ idx)
{
    __shared__ __attribute__((aligned(16))) float ta[EX_TC * EX_LD];
    __shared__ __attribute__((aligned(16))) float tb[EX_TC * EX_LD];
    const int64_t c0 = (int64_t)blockIdx.x * EX_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    // wave w stages candidates 16 w .. 16 w + 15: two rows per wave-instruction (32 lanes x 16 B = one 512-B piece)
    int64_t ia[8], ib[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t p = c0 + wave * 16 + 2 * u + half;
        const uint64_t kk = p < P ? cand[p] : ~0ull;
        ia[u] = p < P ? (int64_t)(kk >> 32) : -1;
        ib[u] = p < P ? (int64_t)(kk & 0xFFFFFFFFu) : -1;
    }
    const int64_t d_pad = chain_pad(d), stages = chain_stages(d_pad, EX_KC);
    f32x4 ra_[8], rb_[8];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ra_[u] = row_piece(ra, ia[u], lda, d, k0 + 4 * l32, vec);
            rb_[u] = row_piece(rb, ib[u], ldb, d, k0 + 4 * l32, vec);
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = wave * 16 + 2 * u + half;
            *(f32x4 *)(ta + c * EX_LD + 4 * l32) = ra_[u];
            *(f32x4 *)(tb + c * EX_LD + 4 * l32) = rb_[u];
        }
    };
    float acc = 0.f;
    fetch(0);
    put();
    __syncthreads();
    for (int64_t s = 0; s < stages; ++s) {
        const int64_t k0 = s * EX_KC;
        if (s + 1 < stages) fetch(k0 + EX_KC);
        if (wave == 0) {
            const int kend = chain_kend(d_pad, k0, EX_KC);
            const float *x = ta + lane * EX_LD, *y = tb + lane * EX_LD;
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
    const int64_t p = c0 + lane;
    if (wave == 0 && p < P) {
        const uint64_t kk = cand[p];
        const bool hit = ALL || acc >= tau;                      // NaN: never a hit of a threshold
        score[p] = acc;
        key[p] = hit ? ((uint64_t)((int64_t)(kk >> 32) - m_lo) << 32) | desc_key(acc) : ~0ull;
        idx[p] = (int32_t)p;
    }
}

// ---------------------------------------------------------------- dense compaction

// hits of row r of scores [m, n] at ld: s >= tau and (diag < 0 or j > diag + r)
__device__ __forceinline__ bool dense_hit(float s, int64_t j, int64_t r, int64_t diag, float tau)
{
    return s >= tau && (diag < 0 || j > diag + r);
}

__global__ __launch_bounds__(256) void select_count_kernel(const float *__restrict__ sc, int64_t n, int64_t ld, int64_t diag, float tau,
                                                           int64_t *__restrict__ counts)
{
    __shared__ int64_t part[4];
    const int64_t r = blockIdx.x;
    int64_t c = 0;
    for (int64_t j = threadIdx.x; j < n; j += 256) c += dense_hit(sc[r * ld + j], j, r, diag, tau);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[r] = part[0] + part[1] + part[2] + part[3];
}

// row r's hits in ascending j at offsets[r]: key (r << 32 | desc_key), idx = position, the ids and scores beside
__global__ __launch_bounds__(256) void select_write_kernel(const float *__restrict__ sc, int64_t n, int64_t ld, int64_t diag, float tau,
                                                           const int64_t *__restrict__ offsets, int64_t m, int64_t capacity,
                                                           uint64_t *__restrict__ key, int32_t *__restrict__ idx, int64_t *__restrict__ ids,
                                                           float *__restrict__ vals)
{
    __shared__ uint32_t wsum[4];
    if (offsets[m] > capacity) return;                           // the caller retries with the size offsets[m]
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t pos = offsets[r];
    for (int64_t j0 = 0; j0 < n; j0 += 256) {
        const int64_t j = j0 + tid;
        const float s = j < n ? sc[r * ld + j] : 0.f;
        const bool hit = j < n && dense_hit(s, j, r, diag, tau);
        const uint32_t incl = wave_inclusive_sum(hit ? 1u : 0u);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (hit) {
            const int64_t p = pos + before + incl - 1;
            key[p] = ((uint64_t)r << 32) | desc_key(s);
            idx[p] = (int32_t)p;
            ids[p] = j;
            vals[p] = s;
        }
        pos += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the final order

__global__ __launch_bounds__(256) void fill_kernel(uint64_t *__restrict__ key, int32_t *__restrict__ idx, int64_t P)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < P) {
        key[p] = ~0ull;
        idx[p] = (int32_t)p;
    }
}

// out[p] = the hit at sorted position p (j from the candidate key or from ids_in; score from vals)
__global__ __launch_bounds__(256) void gather_kernel(const uint64_t *__restrict__ key, const int32_t *__restrict__ idx, int64_t P,
                                                     const uint64_t *__restrict__ cand, const int64_t *__restrict__ ids_in,
                                                     const float *__restrict__ vals, int64_t *__restrict__ out_ids, float *__restrict__ out_scores)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || key[p] == ~0ull) return;
    const int32_t q = idx[p];
    out_ids[p] = cand ? (int64_t)(cand[q] & 0xFFFFFFFFu) : ids_in[q];
    out_scores[p] = vals[q];
}

// offsets[r] = the first sorted position whose row is >= r (non-hits, key ~0, sort last)
__global__ __launch_bounds__(256) void offsets_kernel(const uint64_t *__restrict__ key, int64_t P, int64_t m, int64_t *__restrict__ offsets)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > m) return;
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(key[mid] >> 32) < r && key[mid] != ~0ull) lo = mid + 1;
        else hi = mid;
    }
    offsets[r] = lo;
}

// the first k of every row's sorted candidates into dense [m, k]; id -1 / NaN where a row has fewer; counts[r] = its candidates
__global__ __launch_bounds__(256) void knn_dense_kernel(const int32_t *__restrict__ idx, const uint64_t *__restrict__ cand,
                                                        const float *__restrict__ vals, const int64_t *__restrict__ offsets, int64_t m, int64_t k,
                                                        int64_t *__restrict__ ids, float *__restrict__ scores, int32_t *__restrict__ counts)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * k) return;
    const int64_t r = e / k, c = e % k;
    const int64_t lo = offsets[r], have = offsets[r + 1] - lo;
    if (c == 0) counts[r] = (int32_t)have;
    if (c < have) {
        const int32_t q = idx[lo + c];
        ids[e] = (int64_t)(cand[q] & 0xFFFFFFFFu);
        scores[e] = vals[q];
    } else {
        ids[e] = -1;
        scores[e] = __builtin_nanf("");
    }
}

int key_bits(int64_t m)                 // bits of the row field that keep ~0 (non-hits) above every row < m
{
    int b = 1;
    while (b < 32 && (1ll << b) - 1 <= m) ++b;
    return 32 + b;
}

struct Carve {
    char *p;
    int64_t used = 0;
    template <class T> T *take(int64_t count)
    {
        T *r = (T *)(p ? p + used : nullptr);
        used += round_up(count * (int64_t)sizeof(T), 256);
        return r;
    }
};

// the stable sort of (key, idx) over P items: temp bytes (query with tmp == nullptr)
size_t sort_bytes(int64_t P, int end_bit)
{
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int32_t *)nullptr,
                                             (int32_t *)nullptr, (int)P, 0, end_bit, (hipStream_t)0);
    return t;
}

size_t cand_sort_bytes(int64_t P, int end_bit)
{
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)P, 0, end_bit, (hipStream_t)0);
    return t;
}

size_t scan_bytes(int64_t m)
{
    size_t t = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const int64_t *)nullptr, (int64_t *)nullptr, (int)(m + 1), (hipStream_t)0);
    return t;
}

// the workspace of the two resolves: the sorted candidates, their chains, the (key, idx) pairs before and after the sort, and
// `extra` int64 words behind them (the kNN join's offsets; none for extra == 0)
struct ResolveWs {
    uint64_t *cs, *key, *key2;
    float *score;
    int32_t *idx, *idx2;
    void *tmp;
    size_t tmp_bytes;
    int64_t *offsets;
};

void resolve_layout(int64_t P, int64_t m, int64_t extra, Carve &cv, ResolveWs &w)
{
    w.cs = cv.take<uint64_t>(P);
    w.score = cv.take<float>(P);
    w.key = cv.take<uint64_t>(P);
    w.idx = cv.take<int32_t>(P);
    w.key2 = cv.take<uint64_t>(P);
    w.idx2 = cv.take<int32_t>(P);
    w.tmp_bytes = std::max(sort_bytes(P, key_bits(m)), cand_sort_bytes(P, 64));
    w.tmp = cv.take<char>((int64_t)w.tmp_bytes);
    w.offsets = extra ? cv.take<int64_t>(extra) : nullptr;
}

struct SelectWs {
    int64_t *counts, *ids;
    uint64_t *key, *key2;
    int32_t *idx, *idx2;
    float *vals;
    void *tmp;
    size_t tmp_bytes;
};

void select_layout(int64_t m, int64_t capacity, Carve &cv, SelectWs &w)
{
    const int64_t P = capacity > 0 ? capacity : 1;
    w.counts = cv.take<int64_t>(m + 1);
    w.key = cv.take<uint64_t>(P);
    w.idx = cv.take<int32_t>(P);
    w.key2 = cv.take<uint64_t>(P);
    w.idx2 = cv.take<int32_t>(P);
    w.ids = cv.take<int64_t>(P);
    w.vals = cv.take<float>(P);
    w.tmp_bytes = std::max(sort_bytes(P, key_bits(m)), scan_bytes(m));
    w.tmp = cv.take<char>((int64_t)w.tmp_bytes);
}

constexpr int64_t J_MAX_ITEMS = (1ll << 31) - 1;     // hipcub item counts and the int32 positions of the sort

__global__ __launch_bounds__(256) void center_kernel(const float *__restrict__ src, int64_t n, int64_t d, int layout,
                                                     const float *__restrict__ center, float *__restrict__ out)
{
    const int64_t total = n * d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / d, k = e % d;
        const float x = layout == MDX_ROW_MAJOR ? src[e] : src[k * n + row];
        out[e] = center ? x - center[k] : x;
    }
}

// the shards, sizes and launch geometry that the candidate and bound sweeps share
struct JoinArgs {
    const void *ta, *tb;
    int64_t na, nb, d, I0, I1, NJ, gs, blocks;
    int KB;
    float c0;
};

int join_args(const char *who, const mdx_index *a, const mdx_index *b, int64_t a_lo, int64_t a_hi, JoinArgs *g)
{
    const float *sca = nullptr, *scb = nullptr;
    int64_t rta = 0, kba = 0, rtb = 0, kbb = 0, db = 0;
    MDX_CHECK_ARG(i8_view(a, &g->ta, &sca, &g->na, &rta, &kba) && i8_view(b, &g->tb, &scb, &g->nb, &rtb, &kbb),
                  "%s: int8 shards are needed (an fp16 or fp32 one has no bound)", who);
    (void)mdx_index_info(a, nullptr, &g->d, nullptr, nullptr);
    (void)mdx_index_info(b, nullptr, &db, nullptr, nullptr);
    MDX_CHECK_ARG(g->d == db, "%s: dimensions %lld and %lld differ", who, (long long)g->d, (long long)db);
    MDX_CHECK_ARG(g->na < (1ll << 31) && g->nb < (1ll << 31), "%s: n >= 2^31", who);
    MDX_CHECK_ARG(a_lo >= 0 && a_lo < a_hi && a_hi <= g->na && a_lo % JB_ROWS == 0,
                  "%s: rows [%lld, %lld) of A: 0 <= lo < hi <= n=%lld and lo a multiple of %d", who, (long long)a_lo, (long long)a_hi,
                  (long long)g->na, JB_ROWS);
    g->I0 = a_lo / JB_ROWS;
    g->I1 = ceil_div(a_hi, (int64_t)JB_ROWS);
    g->NJ = ceil_div(g->nb, (int64_t)JB_ROWS);
    g->KB = (int)kba;
    g->c0 = (float)((double)(g->d + 2) * 0x1p-149);             // exact: a multiple of 2^-149 below 2^-126
    return MDX_OK;
}

// the grid of a non-symmetric sweep: the A blocks in groups of g->gs (<= J_GROUP) side by side, `per` workgroups (J blocks or
// slices) for each
int sweep_grid(const char *who, JoinArgs *g, int64_t per)
{
    g->gs = std::min(g->I1 - g->I0, (int64_t)J_GROUP);          // a range search of <= 128 queries is one block row
    g->blocks = ceil_div(g->I1 - g->I0, g->gs) * g->gs * per;
    MDX_CHECK_ARG(g->blocks < (1ll << 31), "%s: too many blocks for one launch", who);
    return MDX_OK;
}

// bytes of the resolve layout for P candidates of m rows with `extra` words behind it (0: the size is not defined)
int64_t resolve_bytes(int64_t P, int64_t m, int64_t extra)
{
    if (P < 1 || m < 1 || P > J_MAX_ITEMS || m > J_MAX_ITEMS) return 0;
    Carve cv{nullptr};
    ResolveWs w;
    resolve_layout(P, m, extra, cv, w);
    return cv.used + 256;
}

// What mdx_join_resolve and mdx_knn_resolve share, in the name `who` of the entry point: the checks of the operands and of the
// workspace, the carve (with `extra` words, as who's size function counts them), the candidates in (i, j) order (the chains then
// run row-grouped, and the stable sort breaks ties by ascending j), their chains (all: no threshold, every candidate is kept)
// and the stable (row, desc_key) sort.  It leaves the sorted keys and positions in w.key2 / w.idx2.
// The callers check their pointers and their own argument (k, tau) first, so among several invalid arguments that one is
// reported before P, m, d, lda / ldb and m_lo; when each entry point carried its own copy of these checks, k came after the
// two checks of P and m and tau came last.  The status is MDX_ERR_INVALID either way.
int resolve_front(const char *who, const float *rows_a, int64_t lda, const float *rows_b, int64_t ldb, int64_t d, const uint64_t *pairs,
                  int64_t P, float tau, bool all, int64_t m_lo, int64_t m, int64_t extra, void *workspace, int64_t workspace_bytes,
                  hipStream_t s, ResolveWs &w)
{
    MDX_CHECK_ARG(P >= 1 && m >= 1 && d >= 1, "%s: P=%lld m=%lld d=%lld must be >= 1", who, (long long)P, (long long)m, (long long)d);
    MDX_CHECK_ARG(P <= J_MAX_ITEMS && m <= J_MAX_ITEMS, "%s: P=%lld or m=%lld >= 2^31", who, (long long)P, (long long)m);
    MDX_CHECK_ARG(lda >= d && ldb >= d, "%s: lda=%lld / ldb=%lld < d=%lld", who, (long long)lda, (long long)ldb, (long long)d);
    MDX_CHECK_ARG(m_lo >= 0, "%s: m_lo=%lld < 0", who, (long long)m_lo);
    const int64_t need = resolve_bytes(P, m, extra);
    MDX_CHECK_WORKSPACE(who, workspace, workspace_bytes, need);
    Carve cv{(char *)round_up((int64_t)(uintptr_t)workspace, 256)};     // the + 256 of the size covers the alignment
    resolve_layout(P, m, extra, cv, w);
    MDX_HIP(hipcub::DeviceRadixSort::SortKeys(w.tmp, w.tmp_bytes, pairs, w.cs, (int)P, 0, 64, s));
    const bool vec = lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)rows_a & 15) == 0 && ((uintptr_t)rows_b & 15) == 0;
    const dim3 grid((unsigned)ceil_div(P, (int64_t)EX_TC));
    if (all)
        hipLaunchKernelGGL(exact_kernel<true>, grid, dim3(256), 0, s, rows_a, lda, rows_b, ldb, d, (const uint64_t *)w.cs, P, 0.f, m_lo, vec,
                           w.score, w.key, w.idx);
    else
        hipLaunchKernelGGL(exact_kernel<false>, grid, dim3(256), 0, s, rows_a, lda, rows_b, ldb, d, (const uint64_t *)w.cs, P, tau, m_lo, vec,
                           w.score, w.key, w.idx);
    MDX_HIP(hipcub::DeviceRadixSort::SortPairs(w.tmp, w.tmp_bytes, (const uint64_t *)w.key, w.key2, (const int32_t *)w.idx, w.idx2, (int)P, 0,
                                               key_bits(m), s));
    return MDX_OK;
}

}  // namespace
}  // namespace mdx

using namespace mdx;

extern "C" {

int mdx_center_rows(const float *src, int64_t n, int64_t d, int layout, const float *center, float *out, void *stream)
{
    MDX_CHECK_ARG(src && out, "mdx_center_rows: NULL pointer");
    MDX_CHECK_ARG(n >= 1 && d >= 1, "mdx_center_rows: n=%lld d=%lld must be >= 1", (long long)n, (long long)d);
    MDX_CHECK_ARG(layout == MDX_DIM_MAJOR || layout == MDX_ROW_MAJOR, "mdx_center_rows: layout %d", layout);
    const int64_t blocks = std::min(ceil_div(n * d, (int64_t)256), (int64_t)65536);
    hipLaunchKernelGGL(center_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, n, d, layout, center, out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_join_stats(const mdx_index *index, const float *rows, int64_t ld, float *stats, void *stream)
{
    MDX_CHECK_ARG(index && rows && stats, "mdx_join_stats: NULL pointer");
    MDX_CHECK_ARG(((uintptr_t)stats & 15) == 0, "mdx_join_stats: stats must be 16-byte aligned (one {p, q, r, w} per 16-byte word)");
    const void *tiles = nullptr;
    const float *scales = nullptr;
    int64_t n = 0, RT = 0, KB = 0, d = 0;
    MDX_CHECK_ARG(i8_view(index, &tiles, &scales, &n, &RT, &KB), "mdx_join_stats: an int8 shard is needed (an fp16 or fp32 one has no bound)");
    MDX_CHECK_ARG(mdx_index_info(index, nullptr, &d, nullptr, nullptr) == MDX_OK, "mdx_join_stats: index info");
    MDX_CHECK_ARG(ld >= d, "mdx_join_stats: ld=%lld < d=%lld", (long long)ld, (long long)d);
    MDX_CHECK_ARG(ceil_div(n, (int64_t)4) < (1ll << 31), "mdx_join_stats: shard too large for one launch");
    hipLaunchKernelGGL(join_stats_kernel, dim3((unsigned)ceil_div(n, (int64_t)4)), dim3(256), 0, (hipStream_t)stream, (const i32x4 *)tiles,
                       scales, n, KB, rows, ld, d, (f32x4 *)stats);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_join_candidates(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo, int64_t a_hi,
                        int symmetric, float tau, uint64_t *pairs, int64_t capacity, int64_t *count, void *stream)
{
    MDX_CHECK_ARG(a && stats_a && b && stats_b && pairs && count, "mdx_join_candidates: NULL pointer");
    MDX_CHECK_ARG((((uintptr_t)stats_a | (uintptr_t)stats_b) & 15) == 0, "mdx_join_candidates: stats_a / stats_b must be 16-byte aligned");
    MDX_CHECK_ARG(__builtin_isfinite(tau), "mdx_join_candidates: tau must be finite");
    MDX_CHECK_ARG(capacity >= 0, "mdx_join_candidates: capacity=%lld < 0", (long long)capacity);
    MDX_CHECK_ARG(!symmetric || a == b, "mdx_join_candidates: the self-join needs a == b");
    JoinArgs g;
    if (const int rc = join_args("mdx_join_candidates", a, b, a_lo, a_hi, &g)) return rc;
    hipStream_t s = (hipStream_t)stream;
    MDX_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    if (symmetric) {
        for (int64_t i = g.I0; i < g.I1; i += J_GROUP) {         // one launch per group of J_GROUP I blocks: J >= i only
            const int64_t blocks = J_GROUP * (g.NJ - i);
            MDX_CHECK_ARG(blocks < (1ll << 31), "mdx_join_candidates: too many blocks for one launch");
            hipLaunchKernelGGL((join_kernel<true, false>), dim3((unsigned)blocks), dim3(256), 0, s, (const i32x4 *)g.ta, (const f32x4 *)stats_a, a_hi,
                               (const i32x4 *)g.tb, (const f32x4 *)stats_b, g.nb, g.KB, i, std::min(i + J_GROUP, g.I1), g.NJ, J_GROUP, tau,
                               (const float *)nullptr, g.c0, pairs, capacity, (unsigned long long *)count);
        }
    } else {
        if (const int rc = sweep_grid("mdx_join_candidates", &g, g.NJ)) return rc;
        hipLaunchKernelGGL((join_kernel<false, false>), dim3((unsigned)g.blocks), dim3(256), 0, s, (const i32x4 *)g.ta, (const f32x4 *)stats_a, a_hi,
                           (const i32x4 *)g.tb, (const f32x4 *)stats_b, g.nb, g.KB, g.I0, g.I1, g.NJ, (int)g.gs, tau, (const float *)nullptr, g.c0,
                           pairs, capacity, (unsigned long long *)count);
    }
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

// the compute units of the current device (256 where there is none to ask: a size function called on a host without a GPU)
int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
        (void)hipGetLastError();
        return 256;
    }
    return cus;
}

// slices of the J blocks per A block: 0 = as many as bring a chunk to the two workgroups per CU that the kernel's LDS allows on
// the current device; never more than the J blocks (every slice sweeps at least one).  Every slicing gives the same bits.
int knn_slices(int64_t m, int64_t nb, int64_t slices)
{
    const int64_t rb = ceil_div(m, (int64_t)JB_ROWS), NJ = ceil_div(nb, (int64_t)JB_ROWS);
    int64_t s = slices > 0 ? slices : ceil_div((int64_t)2 * device_cus(), rb);
    return (int)std::max((int64_t)1, std::min(std::min(s, (int64_t)KNN_MAX_SLICES), NJ));
}

int64_t mdx_knn_bounds_workspace(int64_t m, int64_t k, int64_t nb, int64_t slices)
{
    if (m < 1 || nb < 1 || k < 1 || k > KNN_MAX_K || k > nb || slices < 0 || slices > KNN_MAX_SLICES || m > J_MAX_ITEMS || nb > J_MAX_ITEMS)
        return 0;
    return round_up((int64_t)knn_slices(m, nb, slices) * m * k * (int64_t)sizeof(float), 256);
}

int mdx_knn_bounds(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo, int64_t a_hi, int64_t k,
                   int64_t slices, float *t, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(a && stats_a && b && stats_b && t, "mdx_knn_bounds: NULL pointer");
    MDX_CHECK_ARG((((uintptr_t)stats_a | (uintptr_t)stats_b) & 15) == 0, "mdx_knn_bounds: stats_a / stats_b must be 16-byte aligned");
    MDX_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "mdx_knn_bounds: k=%lld must be in [1, MDX_KNN_JOIN_MAX_K = %d]", (long long)k, KNN_MAX_K);
    MDX_CHECK_ARG(slices >= 0 && slices <= KNN_MAX_SLICES, "mdx_knn_bounds: slices=%lld must be 0 (automatic) or in [1, %d]", (long long)slices,
                  KNN_MAX_SLICES);
    JoinArgs g;
    if (const int rc = join_args("mdx_knn_bounds", a, b, a_lo, a_hi, &g)) return rc;
    MDX_CHECK_ARG(k <= g.nb, "mdx_knn_bounds: k=%lld > the %lld rows of B", (long long)k, (long long)g.nb);
    const int64_t m = a_hi - a_lo, need = mdx_knn_bounds_workspace(m, k, g.nb, slices);
    MDX_CHECK_WORKSPACE("mdx_knn_bounds", workspace, workspace_bytes, need);
    const int S = knn_slices(m, g.nb, slices);
    if (const int rc = sweep_grid("mdx_knn_bounds", &g, S)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(knn_bound_kernel, dim3((unsigned)g.blocks), dim3(256), 0, s, (const i32x4 *)g.ta, (const f32x4 *)stats_a, a_hi,
                       (const i32x4 *)g.tb, (const f32x4 *)stats_b, g.nb, g.KB, g.I0, g.I1, g.NJ, (int)g.gs, S, (int)k, g.c0,
                       (float *)workspace, m);
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)ceil_div(m, (int64_t)4)), dim3(256), 0, s, (const float *)workspace, m, S, (int)k, t);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_join_candidates_rows(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo, int64_t a_hi,
                             const float *tau, uint64_t *pairs, int64_t capacity, int64_t *count, void *stream)
{
    MDX_CHECK_ARG(a && stats_a && b && stats_b && tau && pairs && count, "mdx_join_candidates_rows: NULL pointer");
    MDX_CHECK_ARG((((uintptr_t)stats_a | (uintptr_t)stats_b) & 15) == 0, "mdx_join_candidates_rows: stats_a / stats_b must be 16-byte aligned");
    MDX_CHECK_ARG(capacity >= 0, "mdx_join_candidates_rows: capacity=%lld < 0", (long long)capacity);
    JoinArgs g;
    if (const int rc = join_args("mdx_join_candidates_rows", a, b, a_lo, a_hi, &g)) return rc;
    if (const int rc = sweep_grid("mdx_join_candidates_rows", &g, g.NJ)) return rc;
    hipStream_t s = (hipStream_t)stream;
    MDX_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL((join_kernel<false, true>), dim3((unsigned)g.blocks), dim3(256), 0, s, (const i32x4 *)g.ta, (const f32x4 *)stats_a, a_hi,
                       (const i32x4 *)g.tb, (const f32x4 *)stats_b, g.nb, g.KB, g.I0, g.I1, g.NJ, (int)g.gs, 0.f, tau, g.c0, pairs, capacity,
                       (unsigned long long *)count);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_knn_resolve_workspace(int64_t P, int64_t m) { return resolve_bytes(P, m, m + 1); }     // the offsets on top

int mdx_knn_resolve(const float *rows_a, int64_t lda, const float *rows_b, int64_t ldb, int64_t d, const uint64_t *pairs, int64_t P,
                    int64_t m_lo, int64_t m, int64_t k, int64_t *ids, float *scores, int32_t *counts, void *workspace, int64_t workspace_bytes,
                    void *stream)
{
    MDX_CHECK_ARG(rows_a && rows_b && pairs && ids && scores && counts, "mdx_knn_resolve: NULL pointer");
    MDX_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "mdx_knn_resolve: k=%lld must be in [1, MDX_KNN_JOIN_MAX_K = %d]", (long long)k, KNN_MAX_K);
    hipStream_t s = (hipStream_t)stream;
    ResolveWs w;
    if (const int rc = resolve_front("mdx_knn_resolve", rows_a, lda, rows_b, ldb, d, pairs, P, 0.f, true, m_lo, m, m + 1, workspace,
                                     workspace_bytes, s, w))
        return rc;
    // the CSR of the sorted candidates, then the first k of every row
    hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)ceil_div(m + 1, (int64_t)256)), dim3(256), 0, s, (const uint64_t *)w.key2, P, m, w.offsets);
    hipLaunchKernelGGL(knn_dense_kernel, dim3((unsigned)ceil_div(m * k, (int64_t)256)), dim3(256), 0, s, (const int32_t *)w.idx2,
                       (const uint64_t *)w.cs, (const float *)w.score, (const int64_t *)w.offsets, m, k, ids, scores, counts);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_join_resolve_workspace(int64_t P, int64_t m) { return resolve_bytes(P, m, 0); }

int mdx_join_resolve(const float *rows_a, int64_t lda, const float *rows_b, int64_t ldb, int64_t d, const uint64_t *pairs, int64_t P,
                     float tau, int64_t m_lo, int64_t m, int64_t *offsets, int64_t *ids, float *scores, void *workspace, int64_t workspace_bytes,
                     void *stream)
{
    MDX_CHECK_ARG(rows_a && rows_b && pairs && offsets && ids && scores, "mdx_join_resolve: NULL pointer");
    MDX_CHECK_ARG(__builtin_isfinite(tau), "mdx_join_resolve: tau must be finite");
    hipStream_t s = (hipStream_t)stream;
    ResolveWs w;
    if (const int rc = resolve_front("mdx_join_resolve", rows_a, lda, rows_b, ldb, d, pairs, P, tau, false, m_lo, m, 0, workspace,
                                     workspace_bytes, s, w))
        return rc;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)ceil_div(P, (int64_t)256)), dim3(256), 0, s, (const uint64_t *)w.key2, (const int32_t *)w.idx2,
                       P, (const uint64_t *)w.cs, (const int64_t *)nullptr, (const float *)w.score, ids, scores);
    hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)ceil_div(m + 1, (int64_t)256)), dim3(256), 0, s, (const uint64_t *)w.key2, P, m, offsets);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_range_select_workspace(int64_t m, int64_t capacity)
{
    if (m < 1 || capacity < 0 || m > J_MAX_ITEMS || capacity > J_MAX_ITEMS) return 0;
    Carve cv{nullptr};
    SelectWs w;
    select_layout(m, capacity, cv, w);
    return cv.used + 256;
}

int mdx_range_select(const float *scores, int64_t m, int64_t n, int64_t ld, float tau, int64_t diag, int64_t *offsets, int64_t *ids,
                     float *out_scores, int64_t capacity, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(scores && offsets && ids && out_scores, "mdx_range_select: NULL pointer");
    MDX_CHECK_ARG(m >= 1 && n >= 1, "mdx_range_select: m=%lld n=%lld must be >= 1", (long long)m, (long long)n);
    MDX_CHECK_ARG(m <= J_MAX_ITEMS && capacity <= J_MAX_ITEMS, "mdx_range_select: m=%lld or capacity=%lld >= 2^31", (long long)m,
                  (long long)capacity);
    MDX_CHECK_ARG(ld >= n, "mdx_range_select: ld=%lld < n=%lld", (long long)ld, (long long)n);
    MDX_CHECK_ARG(capacity >= 0, "mdx_range_select: capacity=%lld < 0", (long long)capacity);
    MDX_CHECK_ARG(__builtin_isfinite(tau), "mdx_range_select: tau must be finite");
    const int64_t need = mdx_range_select_workspace(m, capacity);
    MDX_CHECK_WORKSPACE("mdx_range_select", workspace, workspace_bytes, need);
    Carve cv{(char *)round_up((int64_t)(uintptr_t)workspace, 256)};
    SelectWs w;
    select_layout(m, capacity, cv, w);
    const int64_t P = capacity > 0 ? capacity : 1;
    hipStream_t s = (hipStream_t)stream;
    MDX_HIP(hipMemsetAsync(w.counts + m, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)m), dim3(256), 0, s, scores, n, ld, diag, tau, w.counts);
    MDX_HIP(hipcub::DeviceScan::ExclusiveSum(w.tmp, w.tmp_bytes, (const int64_t *)w.counts, offsets, (int)(m + 1), s));
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)ceil_div(P, (int64_t)256)), dim3(256), 0, s, w.key, w.idx, P);
    hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)m), dim3(256), 0, s, scores, n, ld, diag, tau, (const int64_t *)offsets, m, capacity,
                       w.key, w.idx, w.ids, w.vals);
    MDX_HIP(hipcub::DeviceRadixSort::SortPairs(w.tmp, w.tmp_bytes, (const uint64_t *)w.key, w.key2, (const int32_t *)w.idx, w.idx2, (int)P, 0,
                                               key_bits(m), s));
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)ceil_div(P, (int64_t)256)), dim3(256), 0, s, (const uint64_t *)w.key2, (const int32_t *)w.idx2, P,
                       (const uint64_t *)nullptr, (const int64_t *)w.ids, (const float *)w.vals, ids, out_scores);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
