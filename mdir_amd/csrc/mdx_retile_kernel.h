// The re-tiling and int8 quantisation kernels of mdx_index.hip (the index build, the queries of every call, mdx_quantize_i8).
#pragma once
#include "mdx_i8_quant.h"
#include "mdx_scores_i8_kernel.h"

namespace mdx {

// ---------------------------------------------------------------------------
// Re-tiling: an fp32 matrix [rows, k] in either layout of the API -> fragment-order tiles (the index build, the queries
// of every call, the whitening matrix).  Rows >= n and k >= d read 0; `center[k]` (or nothing) is subtracted on the way.
//   fp32 tile = 16 rows x 16 k: lane (g, j), element t = (row j, k 16 kb + 4 t + g)
//   fp16 tile = 16 rows x 32 k: lane (g, j), element e = (row j, k 32 kb + 8 g + e), round-to-nearest-even
// Round 1-3 let every lane fetch its own elements from the source: a wave-load was 16 pieces of 16 B (row-major sources)
// or 4 pieces of 64 B (dimension-major) -- the build of the 8.2 GB shard ran at 0.86 TB/s read + write (19 ms; rocprofv3,
// profiles/r04_summary.md).  Here a workgroup reads a block of the source in whole 1-KiB runs (64 lanes x 16 B along the
// contiguous direction), parks it in LDS and every wave assembles tiles from there; the row stride of the LDS block makes the
// 64 lanes of an assembling read hit 64 different banks.  The tiles leave as before, one coalesced KiB per wave-store.
//   ROWMAJOR  (element (row, k) at src[row * d + k]):  block = 16 rows x 256 k
//   otherwise (element (row, k) at src[k * n + row]):  block = 32 k x 256 rows (two fp32 k blocks or one fp16 k block)
// ---------------------------------------------------------------------------
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a 16-byte load at dword alignment (any n, d)
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool F16, bool ROWMAJOR>
__global__ __launch_bounds__(256) void retile_block_kernel(const float *__restrict__ src, int64_t n, int64_t d, const float *__restrict__ center,
                                                           f32x4 *__restrict__ tiles, int64_t RT, int64_t KB, uint32_t *__restrict__ absmax,
                                                           unsigned inner)
{
    // block id -> (bx, by) = (row tile, k span) or (row span, k block); the index that walks ALONG the source's contiguous
    // direction is the fast one: consecutive blocks read adjacent KiB of the same lines
    const unsigned bx = ROWMAJOR ? blockIdx.x / inner : blockIdx.x % inner, by = ROWMAJOR ? blockIdx.x % inner : blockIdx.x / inner;
    constexpr int TK = F16 ? 32 : 16;                       // k per tile
    constexpr int KBS = (!ROWMAJOR && !F16) ? 2 : 1;        // dimension-major fp32: two k blocks per block, so that a row tile's two tiles leave as one 2-KiB run
    constexpr int LINES = ROWMAJOR ? 16 : TK * KBS;         // 1-KiB runs of the source per block: rows, or k rows
    constexpr int LD = ROWMAJOR ? 260 : (F16 ? 258 : 272);  // floats per line in LDS (bank spread of the assembling reads)
    __shared__ __attribute__((aligned(16))) float blk[LINES * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    uint32_t best = 0;
    // ---- the block, in runs of 1 KiB: line `l`, floats 4 * lane .. 4 * lane + 3
    const int64_t line0 = ROWMAJOR ? (int64_t)bx * 16 : (int64_t)by * TK * KBS;      // first row / first k
    const int64_t col0 = (ROWMAJOR ? (int64_t)by : (int64_t)bx) * 256 + 4 * lane;   // first k / first row of this lane
    const int64_t nlines = ROWMAJOR ? n : d, ncols = ROWMAJOR ? d : n;
    const int64_t ld_src = ncols;
    float cen[4] = {0.f, 0.f, 0.f, 0.f};
    if (ROWMAJOR && center) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cen[e] = col0 + e < d ? center[col0 + e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < LINES / 4; ++i) {
        const int l = wave * (LINES / 4) + i;
        const int64_t line = line0 + l;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (line < nlines) {
            const float *p = src + line * ld_src + col0;
            if (col0 + 3 < ncols) {
                const f32x4u v = *(const f32x4u *)p;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = v[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = col0 + e < ncols ? p[e] : 0.f;
            }
            if (center) {
                const float ck = ROWMAJOR ? 0.f : center[line];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col0 + e < ncols) x[e] -= ROWMAJOR ? cen[e] : ck;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t u = __float_as_uint(x[e]) & 0x7FFFFFFFu;
            if (u < 0x7F800000u && u > best) best = u;
        }
        *(f32x2 *)&blk[l * LD + 4 * lane] = (f32x2){x[0], x[1]};
        *(f32x2 *)&blk[l * LD + 4 * lane + 2] = (f32x2){x[2], x[3]};
    }
    __syncthreads();
    // ---- tiles: 16 (fp16: 8) of them per block, 4 (2) per wave
    constexpr int TILES = ROWMAJOR ? 256 / TK : 16 * KBS;       // dimension-major: tile tl = (row tile tl / KBS, k block tl % KBS)
#pragma unroll
    for (int i = 0; i < TILES / 4; ++i) {
        const int tl = wave * (TILES / 4) + i;                          // tile of the block: along k (ROWMAJOR) or along rows
        const int rl = ROWMAJOR ? 0 : tl / KBS, kl = ROWMAJOR ? 0 : tl % KBS;       // dimension-major: row tile and k block inside the block
        const int64_t rt = ROWMAJOR ? (int64_t)bx : (int64_t)bx * 16 + rl;
        const int64_t kb = ROWMAJOR ? (int64_t)by * TILES + tl : (int64_t)by * KBS + kl;
        if (rt >= RT || kb >= KB) continue;
        f32x4 out;
        if constexpr (F16) {
            f16x8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (_Float16)(ROWMAJOR ? blk[j * LD + tl * 32 + 8 * g + e] : blk[(8 * g + e) * LD + rl * 16 + j]);
            out = __builtin_bit_cast(f32x4, h);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) out[t] = ROWMAJOR ? blk[j * LD + tl * 16 + 4 * t + g] : blk[(kl * 16 + 4 * t + g) * LD + rl * 16 + j];
        }
        tiles[(rt * KB + kb) * 64 + lane] = out;
    }
    if (absmax) {               // the shard's largest finite magnitude (index build only): the scale of MDX_F32_SPLIT2
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)best, o, 64);
            best = other > best ? other : best;
        }
        // one device-wide atomic per wave would be 2 M of them on ONE address for a 1 M x 2048 shard (~10 ns each: 20 of the
        // build's 23 ms); a wave first looks at the cell -- a stale, smaller value only costs an atomic that changes nothing
        if (lane == 0 && best > *(volatile uint32_t *)absmax) atomicMax(absmax, best);
    }
}

// ---------------------------------------------------------------------------
// The int8 form of the re-tiling (MDX_I8, include/mdx.h states the quantisation).  A row's codes need its absmax first, so it
// takes three launches: i8_absmax_kernel (a = max_k |x_k| per row, into the scale array), retile_i8_kernel (codes, reading a)
// and i8_scale_kernel (a -> a / 127 in place).  mdx_quantize_i8 is the same three steps with row-major codes out.
//   int8 tile = 16 rows x 64 k: lane (g, j), byte e = (row j, k 64 kb + 16 g + e)
// ---------------------------------------------------------------------------
// I8_MAX_DPAD, i8_inv, i8_scale and i8_code: mdx_i8_quant.h, shared with mdx_lists_i8.hip
// element (row, k) of the source, center[k] subtracted
template <bool ROWMAJOR>
__device__ __forceinline__ float i8_src(const float *src, int64_t n, int64_t d, const float *center, int64_t row, int64_t k)
{
    const float x = ROWMAJOR ? src[row * d + k] : src[k * n + row];
    return center ? x - center[k] : x;
}

// a of rows 0 .. rows_pad-1 (0 for rows >= n).  Row-major: a wave per row; dimension-major: a thread per row (coalesced along rows)
template <bool ROWMAJOR>
__global__ __launch_bounds__(256) void i8_absmax_kernel(const float *__restrict__ src, int64_t n, int64_t d, const float *__restrict__ center,
                                                        float *__restrict__ amax, int64_t rows_pad)
{
    if constexpr (ROWMAJOR) {
        const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        if (row >= rows_pad) return;
        float m = 0.f;
        if (row < n)
            for (int64_t k = lane; k < d; k += 64) m = fmaxf(m, fabsf(i8_src<true>(src, n, d, center, row, k)));
        m = wave_max(m);
        if (lane == 0) amax[row] = m;
    } else {
        const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (row >= rows_pad) return;
        float m = 0.f;
        if (row < n)
            for (int64_t k = 0; k < d; ++k) m = fmaxf(m, fabsf(i8_src<false>(src, n, d, center, row, k)));
        amax[row] = m;
    }
}

// one wave per tile (rt, kb) of RT x KB; every lane assembles its 16 bytes
template <bool ROWMAJOR>
__global__ __launch_bounds__(256) void retile_i8_kernel(const float *__restrict__ src, int64_t n, int64_t d, const float *__restrict__ center,
                                                        const float *__restrict__ amax, i32x4 *__restrict__ tiles, int64_t RT, int64_t KB)
{
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= RT * KB) return;
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int64_t row = (tile / KB) * TILE_ROWS + j, k0 = (tile % KB) * 64 + 16 * g;
    i32x4 w = {0, 0, 0, 0};
    if (row < n) {
        const float a = amax[row], inv = i8_inv(a);
        float x[16];
        if (ROWMAJOR && !center && k0 + 16 <= d) {
            const f32x4u *p = (const f32x4u *)(src + row * d + k0);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const f32x4u t = p[v];
#pragma unroll
                for (int e = 0; e < 4; ++e) x[4 * v + e] = t[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = k0 + e < d ? i8_src<ROWMAJOR>(src, n, d, center, row, k0 + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) w[e >> 2] |= (int)(i8_code(x[e], a, inv) << (8 * (e & 3)));
    }
    tiles[tile * 64 + lane] = w;
}

__global__ __launch_bounds__(256) void i8_scale_kernel(float *__restrict__ amax, int64_t rows)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row < rows) amax[row] = i8_scale(amax[row]);
}

// mdx_quantize_i8: codes [n, d] row-major, one byte per thread (consecutive threads: consecutive k of a row)
template <bool ROWMAJOR>
__global__ __launch_bounds__(256) void quantize_i8_kernel(const float *__restrict__ src, int64_t n, int64_t d, const float *__restrict__ amax,
                                                          int8_t *__restrict__ codes)
{
    const int64_t total = n * d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / d, k = e % d;
        const float a = amax[row];
        codes[e] = (int8_t)(uint8_t)i8_code(i8_src<ROWMAJOR>(src, n, d, nullptr, row, k), a, i8_inv(a));
    }
}

}  // namespace mdx
