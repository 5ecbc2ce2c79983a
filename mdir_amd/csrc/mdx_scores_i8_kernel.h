// Register-streaming similarity for the int8 shard (MDX_I8, include/mdx.h): the sibling of scores_f16_stream_kernel
// (mdx_scores_stream_kernel.h) on v_mfma_i32_16x16x64_i8.
//
// Same shape as the fp16 kernel -- every wave streams its own row tiles global -> VGPR with non-temporal 16-B loads, PF
// chunks ahead; the query tiles of the next PF chunks sit in a two-stage LDS ring; the accumulators leave through an LDS
// transpose -- with three differences:
//   * a tile is 16 rows x 64 k of int8 (1 KiB); lane (g, j) holds row j, k 64 kb + 16 g + e in byte e (e = 0..15), which is
//     the A / B operand of one v_mfma_i32_16x16x64_i8.  Shard and query tiles use the same k map and the int32 sums are
//     exact, so no lane map or summation order can change a bit;
//   * NC (chunks of 64 k) need not be a multiple of PF: the k range is padded to 64 only (the query tiles and their scales
//     must fit in mdx_scores_workspace, which a pad to 256 would not for d <= 64).  Loads past the last chunk are clamped to
//     it and the last stage issues the MFMAs of its valid chunks only;
//   * the epilogue converts the int32 accumulators to fp32 and applies the two scales: (float)acc * (scale_i * scale_q).
#pragma once
#include <type_traits>

#include "mdx_scores_stream_kernel.h"

namespace mdx {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// db: the int8 shard's tiles; NC = tiles per row tile = chunks of 64 k (any NC >= 1); db_scale: one fp32 scale per row.
// qtiles: [query tile][NC] KiB tiles of int8 queries, q_scale: one scale per query row, both advanced to the launch's first
// query tile.  One workgroup per row block of STREAM_CW * R row tiles; blockIdx.y = pass over groups of QT query tiles.
template <int QT, int R, int WGS>
__global__ __launch_bounds__(STREAM_CW * 64, WGS) void scores_i8_stream_kernel(const f32x4 *__restrict__ db, const float *__restrict__ db_scale,
                                                                              const f32x4 *__restrict__ qtiles, const float *__restrict__ q_scale,
                                                                              float *__restrict__ out, int64_t n, int NC, int nq_valid)
{
    constexpr int PF = STREAM_PF, CW = STREAM_CW;
    constexpr int STAGE_TILES = PF * QT;                            // [chunk of the stage][query tile]
    constexpr int PER_WAVE = (STAGE_TILES + CW - 1) / CW;           // query tiles of a stage this wave brings in (uneven: the last tile again)
    extern __shared__ __attribute__((aligned(16))) f32x4 ring[];   // [2][STAGE_TILES][64]; the output staging afterwards

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NIT = (NC + PF - 1) / PF;
    const int last_chunks = NC - (NIT - 1) * PF;                    // valid chunks of the last stage: 1 .. PF
    const int64_t rt_wg = row_block_of(blockIdx.x, gridDim.x) * CW * R;       // first row tile of the workgroup (XCD-contiguous order)
    qtiles += (int64_t)blockIdx.y * QT * NC * 64;
    q_scale += (int64_t)blockIdx.y * QT * TILE_ROWS;
    out += (int64_t)blockIdx.y * QT * TILE_ROWS * n;

    // query stage s (chunks PF*s .. PF*s+PF-1, clamped to NC-1) -> ring slot s & 1: this wave's tiles, through registers
    const f32x4 *qsrc[PER_WAVE];
    int qdst[PER_WAVE], qchunk[PER_WAVE];
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
        const int i = (wave + t * CW) < STAGE_TILES ? (wave + t * CW) : (STAGE_TILES - 1);
        const int g = i / QT, q = i % QT;
        qdst[t] = i * 64 + lane;
        qchunk[t] = g;
        qsrc[t] = qtiles + (int64_t)q * NC * 64 + lane;
    }
    f32x4 qreg[PER_WAVE];
    auto load_queries = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < PER_WAVE; ++t) {
            const int c = s * PF + qchunk[t];
            qreg[t] = qsrc[t][(int64_t)(c < NC ? c : NC - 1) * 64];
        }
    };
    auto store_queries = [&](int s) __attribute__((always_inline)) {
        f32x4 *slot = ring + (s & 1) * (STAGE_TILES * 64);
#pragma unroll
        for (int t = 0; t < PER_WAVE; ++t) slot[qdst[t]] = qreg[t];
    };

    i32x4 acc[R][QT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < QT; ++q) acc[r][q] = (i32x4){0, 0, 0, 0};

    const f32x4 *dbp = db + (rt_wg + wave * R) * (int64_t)NC * 64 + lane;     // this wave's R row tiles: NC KiB each, back to back
    f32x4 raw[PF][R];
    auto fetch = [&](int j, int c) __attribute__((always_inline)) {            // chunk c (clamped) of the wave's row tiles -> slot j
        const int cc = c < NC ? c : NC - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) raw[j][r] = __builtin_nontemporal_load(dbp + ((int64_t)r * NC + cc) * 64);
    };
    load_queries(0);                            // first, so that the wait for them leaves the shard loads below in flight
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PF; ++j) {
        fetch(j, j);
        __builtin_amdgcn_sched_barrier(0);
    }
    store_queries(0);
    __builtin_amdgcn_sched_barrier(0);

    auto body = [&](int it, auto more) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more)::value;
        // B_it: every wave has written its part of stage `it` (and waited for the writes), and every wave has left stage
        // it-1, whose slot this iteration's writes go to
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE) load_queries(it + 1);
        __builtin_amdgcn_sched_barrier(0);      // the scheduler otherwise sinks every load of the iteration to its end
        const f32x4 *qs = ring + (it & 1) * (STAGE_TILES * 64) + lane;
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            if (MORE || j < last_chunks) {      // uniform: only the last stage may hold clamped (repeated) chunks
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const i32x4 a = __builtin_bit_cast(i32x4, qs[(j * QT + q) * 64]);
#pragma unroll
                    for (int r = 0; r < R; ++r)     // waits (counted vmcnt) for this chunk's loads only
                        acc[r][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, __builtin_bit_cast(i32x4, raw[j][r]), acc[r][q], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (MORE) fetch(j, (it + 1) * PF + j);                // the slot's MFMAs are issued: refill it at once
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (MORE) store_queries(it + 1);
    };
    for (int it = 0; it + 1 < NIT; ++it) body(it, std::true_type{});
    body(NIT - 1, std::false_type{});

    // Epilogue: (float)acc through the LDS transpose (as the fp16 kernel), then both scales on the way out -- every query row
    // of the workgroup's rows leaves as one contiguous run
    constexpr int ROWS = CW * R * TILE_ROWS;
    constexpr int LDW = ROWS + 4;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    float *stage = (float *)ring;
    {
        const int qrow = 4 * (lane >> 4), col = lane & 15;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < QT; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    stage[(q * 16 + qrow + i) * LDW + (wave * R + r) * TILE_ROWS + col] = (float)acc[r][q][i];   // round to nearest even
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int64_t row0 = rt_wg * TILE_ROWS;
    const int rows_valid = (int)((n - row0) < ROWS ? (n - row0) : ROWS);
    const int left = nq_valid - (int)blockIdx.y * QT * TILE_ROWS;
    const int nq_here = left < QT * TILE_ROWS ? left : QT * TILE_ROWS;
    for (int e = tid; e < nq_here * ROWS; e += CW * 64) {
        const int qi = e / ROWS, rr = e % ROWS;
        if (rr < rows_valid)
            store_score<false>(out + (int64_t)qi * n + row0 + rr, __fmul_rn(stage[qi * LDW + rr], __fmul_rn(db_scale[row0 + rr], q_scale[qi])));
    }
}

}  // namespace mdx
