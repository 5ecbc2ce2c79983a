// Database shard ("index") in MFMA-fragment order + the similarity kernel.
//
// Replaces `scores = np.dot(vecs.T, qvecs)` (mdir/components/optim/score/
// cirscore.py:69) and, with the whitening matrix as the "database", the projection
// of CirtorchWhiten.postprocess (mdir/components/data/wrapper.py:193-195).
//
// Data layout: rows are grouped in tiles of 16, the dimension in blocks
// of 16; tile (rt, kb) is 1 KiB = 64 lanes x float4, stored at ((rt*KB)+kb)*1024 B.
// Lane l = 16*g + j holds, in element t (0..3), value (row 16*rt+j, k 16*kb+4*t+g).
// One wave-wide 16-B load therefore fetches one fully coalesced KiB and element t
// of every lane is exactly the B (or A) operand of v_mfma_f32_16x16x4_f32 number t
// of that k-block, with k ascending inside each MFMA and across MFMAs -- so every
// score is the k = 0..D-1 fused-multiply-add chain stated in oracle/chain.c.
#include <stdarg.h>

#include <type_traits>

#include "mdx_common.h"
#include "mdx_scores_kernel.h"
#include "mdx_scores_split_kernel.h"
#include "mdx_scores_stream_kernel.h"
#include "mdx_scores_i8_kernel.h"
#include "mdx_retile_kernel.h"

namespace mdx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------------------
// The launch plan of a similarity call: which kernel instantiation a group of queries takes, and how nq queries are cut
// into groups.  Everything below is host code; the kernels are in the *_kernel.h files.
// ---------------------------------------------------------------------------

// Loader/consumer kernel (4 MFMA waves + 4 LDS-DMA loader waves), chunks of 2 tiles along k,
// ring of 3 stages.  R = 2 row tiles per consumer (128-row workgroups, (QT+8)*6 KiB of LDS)
// for shards of >= 32 768 rows; R = 1 (64-row workgroups) below, so that small shards still
// spread over the CUs -- measured crossover (round 2; the harness is in the history at commit 47a9fe2).
constexpr int64_t R2_MIN_RT = 2048;            // row tiles from which R = 2 (fp32, fp16 and int8 shards, the row-major route)
constexpr int LC_KC = 2, LC_NSTAGE = 3;
#ifndef MDX_SCORES_PIPE_DEFAULT
#define MDX_SCORES_PIPE_DEFAULT 1      // profiles/r05_scores_schedule.md: -1.0 ... -1.2 % (bit-equal); MDX_SCORES_PIPE=0 keeps the round-4 schedule
#endif

// Split-precision launches (mdx_scores_split_kernel.h): 8 consumer waves x R row tiles + 4 loader waves, one workgroup
// per CU, ring of 3 stages of (3 QT + 16 R) KiB.  Up to SPLIT_QT query tiles per workgroup; more queries = more passes (grid.y).
// R = 2 (256-row workgroups) from 65 536 rows; below, 128-row workgroups, so that the shard still spreads over the CUs.
constexpr int SPLIT_CW = 8, SPLIT_NSTAGE = 3, SPLIT_QT = 5;
constexpr int64_t SPLIT_R2_MIN_RT = 4096;

// f(std::integral_constant<int, N>) for N = qt, or MAX for every qt outside 1 .. MAX - 1: a run-time tile count as a template argument
template <int MAX, typename F>
static int with_qt(int qt, F &&f)
{
    if constexpr (MAX > 1) {
        if (qt >= 1 && qt < MAX) return with_qt<MAX - 1>(qt, f);
    }
    return f(std::integral_constant<int, MAX>{});
}

// Launches Kern.  > 64 KiB of dynamic LDS needs an opt-in per kernel and device: done once (the flags are Kern's), not on every launch
template <auto Kern, typename... Args>
static int launch(dim3 grid, dim3 block, int lds, hipStream_t s, Args... args)
{
    static bool opted[64];
    int dev = 0;
    MDX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !opted[dev]) {
        MDX_HIP(hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        if (dev >= 0 && dev < 64) opted[dev] = true;
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
    return MDX_OK;
}

// what the launches of one call share: the tiles (or, ld != 0, the row-major matrix read where it lies), their geometry, the stream
struct Shard { const f32x4 *tiles; int64_t n, RT; int KB; hipStream_t s; int64_t ld; };

// where a launch puts its scores: rows == nullptr: the plain [nq, n] matrix `out`; else query q's run goes to rows[q] + col0
// (device array of nq row pointers: mdx_scores_p2p)
struct Route { float *const *rows; int64_t col0; };

// One launch's share of the queries: `passes` runs (grid.y) of `tiles` query tiles each, from query tile `first` of the call on
struct QGroup {
    int64_t first;      // first query tile
    int tiles;          // query tiles per workgroup
    int nq_valid;       // queries that exist in the passes * tiles tiles
    int tail;           // of them, in the last tile: 1 .. 16
    int passes;         // > 1: full groups of the same size behind each other (only the call's last tile can be partial)
    int64_t q0() const { return first * TILE_ROWS; }
};
constexpr int64_t MAX_PASSES = 32768;          // grid.y < 65 536

// Cuts nq queries into groups of at most max_qt query tiles and hands each to launch_one(const QGroup &): the full groups first --
// pass_grid: up to MAX_PASSES of them per launch, so that many queries against a small database still fill the chip (20 000
// rows are 313 workgroups per group); else one by one -- then the rest
template <typename F>
static int for_query_groups(int64_t nq, int max_qt, bool pass_grid, F &&launch_one)
{
    const int64_t QT_total = ceil_div(nq, TILE_ROWS), full = QT_total / max_qt, step = pass_grid ? MAX_PASSES : 1;
    auto group = [&](int64_t first, int tiles, int64_t passes) -> int {
        const int64_t room = passes * tiles * TILE_ROWS, left = nq - first * TILE_ROWS;
        const int nq_valid = (int)(left < room ? left : room);
        int rc = launch_one(QGroup{first, tiles, nq_valid, nq_valid - (int)(passes * tiles - 1) * TILE_ROWS, (int)passes});
        if (rc != MDX_OK) return rc;
        MDX_LAUNCH_CHECK();
        return MDX_OK;
    };
    for (int64_t g0 = 0; g0 < full; g0 += step) {
        int rc = group(g0 * max_qt, max_qt, (full - g0) < step ? (full - g0) : step);
        if (rc != MDX_OK) return rc;
    }
    return full * max_qt < QT_total ? group(full * max_qt, (int)(QT_total - full * max_qt), 1) : MDX_OK;
}

// The ring kernel on fp32 or fp16 tiles (MM), QT full query tiles + QR leftover tiles (<= 8 queries on v_mfma_f32_4x4x1).  Three
// forms of it: the routed epilogue, the pipelined consumer (PIPE, 128-row workgroups on fp32 tiles) and the plain one
template <int QT, int R, typename MM, int QR = 0, bool RM = false>
static int launch_scores_lc(const Shard &sh, const f32x4 *qt, float *out, int nq_valid, int passes, Route route)
{
    constexpr int lds = LC_NSTAGE * (QT + QR + 4 * R) * LC_KC * 1024;
    const dim3 grid((unsigned)ceil_div(sh.RT, (int64_t)4 * R), (unsigned)passes), block(512);
    if constexpr (MM::STEPS == 4 && !RM) {
        if (route.rows)             // routed epilogue (the shipped schedule of each shape: PIPE for 128-row workgroups)
            return launch<scores_lc_kernel<QT, R, LC_KC, LC_NSTAGE, 2, MM, QR, 4, false, (R == 2 ? 1 : 0), 4, true>>(
                grid, block, lds, sh.s, sh.tiles, qt, out, sh.n, sh.KB, nq_valid, sh.ld, route.rows, route.col0);
    }
    if (route.rows) {
        set_error("routed scores need an fp32 tiled shard");
        return MDX_ERR_INVALID;
    }
    if constexpr (MM::STEPS == 4 && !RM && R == 2) {
        // the pipelined consumer (PIPE): MDX_SCORES_PIPE=0/1 picks the form per launch (A/B in one process: tools/chain_power_probe.py)
        const char *e = getenv("MDX_SCORES_PIPE");
        if (e ? e[0] == '1' : MDX_SCORES_PIPE_DEFAULT)
            return launch<scores_lc_kernel<QT, R, LC_KC, LC_NSTAGE, 2, MM, QR, 4, RM, 1>>(
                grid, block, lds, sh.s, sh.tiles, qt, out, sh.n, sh.KB, nq_valid, sh.ld, (float *const *)nullptr, (int64_t)0);
    }
    return launch<scores_lc_kernel<QT, R, LC_KC, LC_NSTAGE, 2, MM, QR, 4, RM>>(      // 2 = non-temporal database stream
        grid, block, lds, sh.s, sh.tiles, qt, out, sh.n, sh.KB, nq_valid, sh.ld, (float *const *)nullptr, (int64_t)0);
}

// fp16 shards whose k range is a whole number of four-chunk stages (d_pad % 128 == 0: every descriptor size of the path) take the
// register-streaming kernel (mdx_scores_stream_kernel.h; bit-identical to the ring kernel, 6-10 % faster at 1 M x 2048);
// MDX_F16_RING=1 keeps the ring kernel (A/B, tests)
static bool f16_streams(int KB)
{
    static const bool ring_only = getenv("MDX_F16_RING") != nullptr;
    return !ring_only && KB % STREAM_PF == 0;
}

// the register-streaming kernels: fp16 tiles, or (I8) int8 tiles with the row scales of both sides
template <int QT, int R, bool I8>
static int launch_stream(const Shard &sh, const float *db_scale, const f32x4 *qt, const float *q_scale, float *out, int nq_valid, int passes)
{
    constexpr int WGS = QT <= 5 ? 3 : 2;
    constexpr int lds = stream_lds_bytes<QT, R>();
    const dim3 grid((unsigned)ceil_div(sh.RT, (int64_t)STREAM_CW * R), (unsigned)passes), block(STREAM_CW * 64);
    if constexpr (I8)
        return launch<scores_i8_stream_kernel<QT, R, WGS>>(grid, block, lds, sh.s, sh.tiles, db_scale, qt, q_scale, out, sh.n, sh.KB, nq_valid);
    else
        return launch<scores_f16_stream_kernel<QT, R, WGS>>(grid, block, lds, sh.s, sh.tiles, qt, out, sh.n, sh.KB, nq_valid);
}

// QT query tiles against an fp32 or fp16 shard, R row tiles per consumer wave
template <int QT, int R>
static int launch_tiles(bool f16, const Shard &sh, const f32x4 *q, float *out, int nq_valid, int passes, Route route)
{
    if (!f16) return launch_scores_lc<QT, R, MmaF32>(sh, q, out, nq_valid, passes, route);
    if (f16_streams(sh.KB) && !route.rows) return launch_stream<QT, R, false>(sh, nullptr, q, nullptr, out, nq_valid, passes);
    return launch_scores_lc<QT, R, MmaF16>(sh, q, out, nq_valid, passes, route);
}

// One query group against a tiled fp32 / fp16 shard (r2: 128-row workgroups).  leftover_mfma: a last tile of <= 8 queries goes to
// v_mfma_f32_4x4x1 beside tiles - 1 full tiles on the 16x16x4 MFMA (fp32 shards with 128-row workgroups)
static int launch_group(const QGroup &g, bool r2, bool f16, bool leftover_mfma, const Shard &sh, const f32x4 *q, float *out, Route route)
{
    if (leftover_mfma && r2 && !f16 && g.passes == 1 && g.tiles >= 2 && g.tail <= 8)
        return with_qt<MAX_QT - 1>(g.tiles - 1, [&](auto qt) {
            return launch_scores_lc<decltype(qt)::value, 2, MmaF32, 1>(sh, q, out, g.nq_valid, 1, route);
        });
    return with_qt<MAX_QT>(g.tiles, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        return r2 ? launch_tiles<QT, 2>(f16, sh, q, out, g.nq_valid, g.passes, route) : launch_tiles<QT, 1>(f16, sh, q, out, g.nq_valid, g.passes, route);
    });
}

// The same kernels on a row-major database read where it lies (RM = true; mdx_scores_rowmajor)
static int launch_group_rowmajor(const QGroup &g, bool r2, const Shard &sh, const f32x4 *q, float *out)
{
    const Route plain{nullptr, 0};
    if (r2 && g.tiles >= 2 && g.tail <= 8)
        return with_qt<MAX_QT - 1>(g.tiles - 1, [&](auto qt) {
            return launch_scores_lc<decltype(qt)::value, 2, MmaF32, 1, true>(sh, q, out, g.nq_valid, 1, plain);
        });
    return with_qt<MAX_QT>(g.tiles, [&](auto qt) {
        constexpr int QT = decltype(qt)::value;
        return r2 ? launch_scores_lc<QT, 2, MmaF32, 0, true>(sh, q, out, g.nq_valid, 1, plain)
                  : launch_scores_lc<QT, 1, MmaF32, 0, true>(sh, q, out, g.nq_valid, 1, plain);
    });
}

// the split-precision kernels: three bf16 pieces, or (TWO) two fp16 pieces with the block scales of both sides
template <int QT, int R, bool TWO>
static int launch_split(const QGroup &g, const Shard &sh, const u32x4 *qp, float *out, int QT_total, int nq, float db_scale, const uint32_t *q_cell)
{
    constexpr int lds = SPLIT_NSTAGE * ((TWO ? 2 : 3) * QT + 2 * SPLIT_CW * R) * 1024;
    const dim3 grid((unsigned)ceil_div(sh.RT, (int64_t)SPLIT_CW * R), (unsigned)g.passes), block(SPLIT_CW * 64 + 256);
    if constexpr (TWO)
        return launch<scores_split2_kernel<QT, R, SPLIT_NSTAGE, SPLIT_CW>>(grid, block, lds, sh.s, sh.tiles, qp, out, sh.n, sh.KB, QT_total,
                                                                          (int)g.first, nq, db_scale, q_cell);
    else
        return launch<scores_split3_kernel<QT, R, SPLIT_NSTAGE, SPLIT_CW>>(grid, block, lds, sh.s, sh.tiles, qp, out, sh.n, sh.KB, QT_total,
                                                                          (int)g.first, nq);
}

}  // namespace mdx

using namespace mdx;

struct mdx_index {
    f32x4 *tiles;
    int64_t n, d, d_pad, RT, RT_pad, KB, row_offset;
    int64_t bytes;
    int storage;        // MDX_F32 / MDX_F16 / MDX_I8
    float *scales;      // MDX_I8: one scale per padded row, behind the tiles (nullptr otherwise)
    bool owns;          // tiles came from hipMalloc here (mdx_index_create*) and are freed on destroy; false: the caller's memory
    uint32_t max_bits;  // fp32 shards: bit pattern of the largest finite |x| (read back once at creation): the scale of MDX_F32_SPLIT2
};

bool mdx::i8_view(const mdx_index *ix, const void **tiles, const float **scales, int64_t *n, int64_t *rt, int64_t *kb)
{
    if (!ix || ix->storage != MDX_I8) return false;
    *tiles = ix->tiles;
    *scales = ix->scales;
    *n = ix->n;
    *rt = ix->RT;
    *kb = ix->KB;
    return true;
}

extern "C" {

int mdx_abi_version(void) { return MDX_ABI_VERSION; }

int mdx_capture_recover(void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(s, &g);       // an invalidated capture ends with an error and no graph
        if (g) (void)hipGraphDestroy(g);
    }
    (void)hipGetLastError();                    // the sticky (non-fatal) error of the failed capture
    (void)hipGetLastError();
    return MDX_OK;
}
const char *mdx_last_error(void) { return mdx::g_err; }

// MDX_I8: tiles of 16 rows x 64 k (KB of them per row tile) and the scales of the RT * 16 rows, in three launches
static int retile_i8(const float *src, int64_t n, int64_t d, bool rowmajor, const float *center, f32x4 *tiles, int64_t RT, int64_t KB,
                     float *scales, hipStream_t s)
{
    const int64_t rows = RT * TILE_ROWS;
    MDX_CHECK_ARG(ceil_div(RT * KB, (int64_t)4) < (1ll << 31) && ceil_div(rows, (int64_t)4) < (1ll << 31), "matrix too large to re-tile in one launch");
    const dim3 block(256), grid_abs((unsigned)(rowmajor ? ceil_div(rows, (int64_t)4) : ceil_div(rows, (int64_t)256)));
    const dim3 grid_tiles((unsigned)ceil_div(RT * KB, (int64_t)4)), grid_rows((unsigned)ceil_div(rows, (int64_t)256));
    i32x4 *t = (i32x4 *)tiles;
    if (rowmajor) {
        hipLaunchKernelGGL(i8_absmax_kernel<true>, grid_abs, block, 0, s, src, n, d, center, scales, rows);
        hipLaunchKernelGGL(retile_i8_kernel<true>, grid_tiles, block, 0, s, src, n, d, center, (const float *)scales, t, RT, KB);
    } else {
        hipLaunchKernelGGL(i8_absmax_kernel<false>, grid_abs, block, 0, s, src, n, d, center, scales, rows);
        hipLaunchKernelGGL(retile_i8_kernel<false>, grid_tiles, block, 0, s, src, n, d, center, (const float *)scales, t, RT, KB);
    }
    hipLaunchKernelGGL(i8_scale_kernel, grid_rows, block, 0, s, scales, rows);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

static int retile(const float *src, int64_t n, int64_t d, int layout, const float *center,
                  f32x4 *tiles, int64_t RT, int64_t KB, hipStream_t s, int storage = MDX_F32, uint32_t *absmax = nullptr,
                  float *scales = nullptr)
{
    const bool rowmajor = layout != MDX_DIM_MAJOR, f16 = storage == MDX_F16;
    if (storage == MDX_I8) return retile_i8(src, n, d, rowmajor, center, tiles, RT, KB, scales, s);
    // blocks: 16 rows x 256 k (row-major) or 32 k x 256 rows (dimension-major: two fp32 k blocks or one fp16 k block)
    const int64_t gx = rowmajor ? RT : ceil_div(RT, (int64_t)16);
    const int64_t gy = rowmajor ? ceil_div(KB * (f16 ? 32 : 16), (int64_t)256) : (f16 ? KB : ceil_div(KB, (int64_t)2));
    MDX_CHECK_ARG(gx * gy < (1ll << 31), "matrix too large to re-tile in one launch");
    const dim3 grid((unsigned)(gx * gy)), block(256);
    const unsigned inner = (unsigned)(rowmajor ? gy : gx);
    if (f16 && rowmajor)       hipLaunchKernelGGL((retile_block_kernel<true, true>), grid, block, 0, s, src, n, d, center, tiles, RT, KB, absmax, inner);
    else if (f16)              hipLaunchKernelGGL((retile_block_kernel<true, false>), grid, block, 0, s, src, n, d, center, tiles, RT, KB, absmax, inner);
    else if (rowmajor)         hipLaunchKernelGGL((retile_block_kernel<false, true>), grid, block, 0, s, src, n, d, center, tiles, RT, KB, absmax, inner);
    else                       hipLaunchKernelGGL((retile_block_kernel<false, false>), grid, block, 0, s, src, n, d, center, tiles, RT, KB, absmax, inner);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_index_create(mdx_index **out, const float *src, int64_t n, int64_t d, int layout,
                     int64_t row_offset, void *stream)
{
    return mdx_index_create_ex(out, src, n, d, layout, row_offset, MDX_F32, stream);
}

static void index_geometry(mdx_index *ix, int64_t n, int64_t d, int storage)
{
    ix->n = n;
    ix->d = d;
    ix->storage = storage;
    ix->d_pad = round_up(d, 64);                                  // 4 fp32, 2 fp16 or 1 int8 k-blocks
    ix->KB = ix->d_pad / (storage == MDX_F16 ? 32 : storage == MDX_I8 ? 64 : TILE_K);
    ix->RT = ceil_div(n, TILE_ROWS);
    // every wave of every workgroup has a tile to read: 8 row tiles per workgroup, 16 for the split-precision kernel (fp32 shards)
    ix->RT_pad = round_up(ix->RT, storage == MDX_F32 ? 16 : 8);
    ix->bytes = ix->RT_pad * ix->KB * 1024 + (storage == MDX_I8 ? ix->RT_pad * TILE_ROWS * 4 : 0);    // int8: + the row scales
    ix->max_bits = 0;
    ix->scales = nullptr;
}

int64_t mdx_index_bytes(int64_t n, int64_t d, int storage)
{
    if (n <= 0 || d <= 0 || (storage != MDX_F32 && storage != MDX_F16 && storage != MDX_I8)) return 0;
    if (storage == MDX_I8 && round_up(d, 64) > I8_MAX_DPAD) return 0;
    mdx_index g;
    index_geometry(&g, n, d, storage);
    return g.bytes + 256;                                          // + one word behind the tiles: the |x| maximum
}

int mdx_index_create_ex(mdx_index **out, const float *src, int64_t n, int64_t d, int layout,
                        int64_t row_offset, int storage, void *stream)
{
    return mdx_index_create_in(out, src, n, d, layout, row_offset, storage, nullptr, 0, stream);
}

int mdx_index_create_in(mdx_index **out, const float *src, int64_t n, int64_t d, int layout, int64_t row_offset, int storage,
                        void *memory, int64_t memory_bytes, void *stream)
{
    MDX_CHECK_ARG(out && src, "mdx_index_create: NULL pointer");
    MDX_CHECK_ARG(storage == MDX_F32 || storage == MDX_F16 || storage == MDX_I8, "mdx_index_create: storage %d", storage);
    MDX_CHECK_ARG(n > 0 && d > 0, "mdx_index_create: n=%lld d=%lld must be positive",
                  (long long)n, (long long)d);
    MDX_CHECK_ARG(storage != MDX_I8 || round_up(d, 64) <= I8_MAX_DPAD,
                  "mdx_index_create: d=%lld too large for an int8 shard (127^2 * round_up(d, 64) must stay below 2^31; d <= %lld)",
                  (long long)d, (long long)I8_MAX_DPAD);
    MDX_CHECK_ARG(layout == MDX_DIM_MAJOR || layout == MDX_ROW_MAJOR, "mdx_index_create: layout %d",
                  layout);
    mdx_index *ix = new mdx_index();
    index_geometry(ix, n, d, storage);
    ix->row_offset = row_offset;
    ix->owns = memory == nullptr;
    if (memory) {
        if (memory_bytes < ix->bytes + 256 || ((uintptr_t)memory & 255)) {
            set_error("mdx_index_create_in: %lld bytes at a 256-byte boundary needed (mdx_index_bytes), got %lld at %p", (long long)ix->bytes + 256,
                      (long long)memory_bytes, memory);
            delete ix;
            return MDX_ERR_WORKSPACE;
        }
        ix->tiles = (f32x4 *)memory;
    } else {
        hipError_t e = hipMalloc((void **)&ix->tiles, (size_t)ix->bytes + 256);
        if (e != hipSuccess) {
            set_error("mdx_index_create: hipMalloc(%lld bytes) failed: %s", (long long)ix->bytes,
                      hipGetErrorString(e));
            delete ix;
            return MDX_ERR_NOMEM;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t *cell = storage == MDX_F32 ? (uint32_t *)((char *)ix->tiles + ix->bytes) : nullptr;
    if (cell && hipMemsetAsync(cell, 0, 4, s) != hipSuccess) cell = nullptr;
    if (storage == MDX_I8) ix->scales = (float *)((char *)ix->tiles + ix->RT_pad * ix->KB * 1024);
    int rc = retile(src, n, d, layout, nullptr, ix->tiles, ix->RT_pad, ix->KB, s, storage, cell, ix->scales);
    if (rc == MDX_OK && cell) {
        // index creation is the call of this path that may synchronise: the maximum comes back with the build
        if (hipMemcpyAsync(&ix->max_bits, cell, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            set_error("mdx_index_create: reading the shard's maximum failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MDX_ERR_RUNTIME;
        }
    }
    if (rc != MDX_OK) {
        (void)hipStreamSynchronize(s);
        if (ix->owns) (void)hipFree(ix->tiles);
        delete ix;
        return rc;
    }
    // index creation is the one call of the ranking path that may synchronise: settle here how the sort ranks inside a
    // wave on this device (mdx_rank.hip), so that the enqueue-only ranking calls -- also captured ones -- find the answer
    (void)probe_lds_order(s);
    *out = ix;
    return MDX_OK;
}

int mdx_index_destroy(mdx_index *ix)
{
    if (!ix) return MDX_OK;
    const hipError_t e = ix->owns ? hipFree(ix->tiles) : hipSuccess;
    delete ix;
    if (e != hipSuccess) {
        set_error("mdx_index_destroy: hipFree failed: %s", hipGetErrorString(e));
        return MDX_ERR_RUNTIME;
    }
    return MDX_OK;
}

int mdx_index_info(const mdx_index *ix, int64_t *n, int64_t *d, int64_t *row_offset,
                   int64_t *device_bytes)
{
    MDX_CHECK_ARG(ix, "mdx_index_info: NULL index");
    if (n) *n = ix->n;
    if (d) *d = ix->d;
    if (row_offset) *row_offset = ix->row_offset;
    if (device_bytes) *device_bytes = ix->bytes;
    return MDX_OK;
}

int64_t mdx_scores_workspace(int64_t nq, int64_t d)
{
    if (nq <= 0 || d <= 0) return 0;
    return round_up(nq, TILE_ROWS) * round_up(d, 64) * 4;   // fp32 tiles; an fp16 shard uses half of it, an int8 one a quarter + the scales
}

static const char *storage_name(int storage) { return storage == MDX_F16 ? "fp16" : storage == MDX_I8 ? "int8" : "fp32"; }

int mdx_quantize_i8(const float *src, int64_t n, int64_t d, int layout, int8_t *codes, float *scales, void *stream)
{
    MDX_CHECK_ARG(src && codes && scales, "mdx_quantize_i8: NULL pointer");
    MDX_CHECK_ARG(n > 0 && d > 0, "mdx_quantize_i8: n=%lld d=%lld must be positive", (long long)n, (long long)d);
    MDX_CHECK_ARG(round_up(d, 64) <= I8_MAX_DPAD, "mdx_quantize_i8: d=%lld too large (127^2 * round_up(d, 64) must stay below 2^31; d <= %lld)",
                  (long long)d, (long long)I8_MAX_DPAD);
    MDX_CHECK_ARG(layout == MDX_DIM_MAJOR || layout == MDX_ROW_MAJOR, "mdx_quantize_i8: layout %d", layout);
    MDX_CHECK_ARG(ceil_div(n, (int64_t)4) < (1ll << 31), "mdx_quantize_i8: n=%lld too large for one launch", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    const bool rowmajor = layout == MDX_ROW_MAJOR;
    const int64_t blocks = ceil_div(n * d, (int64_t)256);
    const dim3 block(256), grid_q((unsigned)(blocks < 65536 ? blocks : 65536)), grid_rows((unsigned)ceil_div(n, (int64_t)256));
    if (rowmajor) {
        hipLaunchKernelGGL(i8_absmax_kernel<true>, dim3((unsigned)ceil_div(n, (int64_t)4)), block, 0, s, src, n, d, (const float *)nullptr, scales, n);
        hipLaunchKernelGGL(quantize_i8_kernel<true>, grid_q, block, 0, s, src, n, d, (const float *)scales, codes);
    } else {
        hipLaunchKernelGGL(i8_absmax_kernel<false>, grid_rows, block, 0, s, src, n, d, (const float *)nullptr, scales, n);
        hipLaunchKernelGGL(quantize_i8_kernel<false>, grid_q, block, 0, s, src, n, d, (const float *)scales, codes);
    }
    hipLaunchKernelGGL(i8_scale_kernel, grid_rows, block, 0, s, scales, n);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

static int scores_impl(const mdx_index *ix, const float *queries, int64_t nq, int qlayout, const float *center, float *scores,
                       Route route, void *workspace, int64_t workspace_bytes, void *stream);

int mdx_scores(const mdx_index *ix, const float *queries, int64_t nq, int qlayout,
               const float *center, float *scores, void *workspace, int64_t workspace_bytes,
               void *stream)
{
    MDX_CHECK_ARG(ix && queries && scores, "mdx_scores: NULL pointer");
    return scores_impl(ix, queries, nq, qlayout, center, scores, Route{nullptr, 0}, workspace, workspace_bytes, stream);
}

int mdx_scores_p2p(const mdx_index *ix, const float *queries, int64_t nq, int qlayout, const float *center, mdx_p2p *p2p,
                   void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(ix && queries && p2p, "mdx_scores_p2p: NULL pointer");
    MDX_CHECK_ARG(ix->storage == MDX_F32, "mdx_scores_p2p: an fp32 shard is needed (this one is stored as %s)", storage_name(ix->storage));
    MDX_CHECK_ARG(nq > 0 && nq <= MAX_QT * TILE_ROWS, "mdx_scores_p2p: nq=%lld, 1..%d supported", (long long)nq, MAX_QT * TILE_ROWS);
    float *const *rows = nullptr;
    if (!p2p_route(p2p, nq, &rows)) {
        set_error("mdx_scores_p2p: the exchange is not connected or was created for another number of queries");
        return MDX_ERR_INVALID;
    }
    return scores_impl(ix, queries, nq, qlayout, center, nullptr, Route{rows, ix->row_offset}, workspace, workspace_bytes, stream);
}

static int scores_impl(const mdx_index *ix, const float *queries, int64_t nq, int qlayout, const float *center, float *scores,
                       Route route, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(nq > 0, "mdx_scores: nq=%lld must be positive", (long long)nq);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "mdx_scores: qlayout %d",
                  qlayout);
    MDX_CHECK_WORKSPACE("mdx_scores", workspace, workspace_bytes, mdx_scores_workspace(nq, ix->d));
    const Shard sh{ix->tiles, ix->n, ix->RT, (int)ix->KB, (hipStream_t)stream, 0};
    f32x4 *qtiles = (f32x4 *)workspace;
    const int64_t QT_total = ceil_div(nq, TILE_ROWS);
    const bool r2 = ix->RT >= R2_MIN_RT;              // >= 32 768 rows: 128-row workgroups
    if (ix->storage == MDX_I8) {
        // int8 query tiles (QT_total * KB KiB), then one scale per padded query: round_up(nq, 16) * (d_pad + 4) bytes <= need
        float *q_scale = (float *)((char *)workspace + QT_total * ix->KB * 1024);
        int rc = retile(queries, nq, ix->d, qlayout, center, qtiles, QT_total, ix->KB, sh.s, MDX_I8, nullptr, q_scale);
        if (rc != MDX_OK) return rc;
        return for_query_groups(nq, MAX_QT, true, [&](const QGroup &g) {
            const f32x4 *qp = qtiles + g.first * ix->KB * 64;
            const float *qs = q_scale + g.q0();
            float *op = scores + g.q0() * ix->n;
            return with_qt<MAX_QT>(g.tiles, [&](auto qt) {
                constexpr int QT = decltype(qt)::value;
                return r2 ? launch_stream<QT, 2, true>(sh, ix->scales, qp, qs, op, g.nq_valid, g.passes)
                          : launch_stream<QT, 1, true>(sh, ix->scales, qp, qs, op, g.nq_valid, g.passes);
            });
        });
    }
    int rc = retile(queries, nq, ix->d, qlayout, center, qtiles, QT_total, ix->KB, sh.s, ix->storage);
    if (rc != MDX_OK) return rc;

    static const bool no_pass_grid = getenv("MDX_NO_PASS_GRID") != nullptr, no_query_split = getenv("MDX_NO_QUERY_SPLIT") != nullptr,
                      no_leftover = getenv("MDX_NO_LEFTOVER_MFMA") != nullptr;
    if (!r2 && QT_total > 1 && QT_total <= MAX_QT && ceil_div(ix->RT, (int64_t)4) * QT_total <= 1024 && ix->storage == MDX_F32 &&
        !no_query_split) {
        // few queries against a small shard (rOxford5k alone: 70 x 4 993): 64-row workgroups taking all
        // query tiles are only RT/4 = 79 workgroups, each a 5-tile-long MFMA chain.  Give every workgroup
        // ONE query tile instead (grid.y = tile): 5x the workgroups, a fifth of the chain each.
        rc = launch_scores_lc<1, 1, MmaF32>(sh, qtiles, scores, (int)nq, (int)QT_total, route);
        if (rc != MDX_OK) return rc;
        MDX_LAUNCH_CHECK();
        return MDX_OK;
    }
    return for_query_groups(nq, MAX_QT, !no_pass_grid && !route.rows, [&](const QGroup &g) {
        return launch_group(g, r2, ix->storage == MDX_F16, !no_leftover, sh, qtiles + g.first * ix->KB * 64,
                            route.rows ? nullptr : scores + g.q0() * ix->n, route);
    });
}

int mdx_scores_rowmajor(const float *db, int64_t n, int64_t d, const float *queries, int64_t nq, int qlayout, const float *center,
                        float *scores, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(db && queries && scores, "mdx_scores_rowmajor: NULL pointer");
    MDX_CHECK_ARG(n > 0 && nq > 0, "mdx_scores_rowmajor: n=%lld nq=%lld must be positive", (long long)n, (long long)nq);
    // 16-byte LDS-DMA pieces are served from any 4-byte-aligned address (tools/align_probe.py: bit-exact at every offset)
    MDX_CHECK_ARG(d >= 4 && d % 4 == 0 && ((uintptr_t)db & 3) == 0,
                  "mdx_scores_rowmajor: d=%lld must be a multiple of 4 (rows are read in pieces of four values) and the matrix 4-byte aligned; "
                  "build an index for other shapes", (long long)d);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "mdx_scores_rowmajor: qlayout %d", qlayout);
    MDX_CHECK_WORKSPACE("mdx_scores_rowmajor", workspace, workspace_bytes, mdx_scores_workspace(nq, d));
    f32x4 *qtiles = (f32x4 *)workspace;
    const int64_t QT_total = ceil_div(nq, TILE_ROWS), KB = round_up(d, 64) / TILE_K;
    const Shard sh{(const f32x4 *)db, n, ceil_div(n, TILE_ROWS), (int)KB, (hipStream_t)stream, d};
    int rc = retile(queries, nq, d, qlayout, center, qtiles, QT_total, KB, sh.s, MDX_F32);
    if (rc != MDX_OK) return rc;
    const bool r2 = sh.RT >= R2_MIN_RT;               // >= 32 768 rows: 128-row workgroups
    return for_query_groups(nq, MAX_QT, false, [&](const QGroup &g) {
        return launch_group_rowmajor(g, r2, sh, qtiles + g.first * KB * 64, scores + g.q0() * n);
    });
}

int64_t mdx_scores_workspace_ex(int64_t nq, int64_t d, int compute)
{
    if (nq <= 0 || d <= 0) return 0;
    if (compute == MDX_F32_SPLIT3) return round_up(nq, TILE_ROWS) * round_up(d, 64) * 6;      // three bf16 pieces per element
    if (compute == MDX_F32_SPLIT2) return round_up(nq, TILE_ROWS) * round_up(d, 64) * 4 + 256;    // two fp16 pieces + the queries' |q| maximum
    return mdx_scores_workspace(nq, d);
}

int mdx_scores_ex(const mdx_index *ix, const float *queries, int64_t nq, int qlayout, const float *center, float *scores,
                  void *workspace, int64_t workspace_bytes, int compute, void *stream)
{
    if (compute == MDX_F32_CHAIN) return mdx_scores(ix, queries, nq, qlayout, center, scores, workspace, workspace_bytes, stream);
    MDX_CHECK_ARG(compute == MDX_F32_SPLIT3 || compute == MDX_F32_SPLIT2, "mdx_scores_ex: compute mode %d", compute);
    MDX_CHECK_ARG(ix && queries && scores, "mdx_scores_ex: NULL pointer");
    MDX_CHECK_ARG(ix->storage == MDX_F32, "mdx_scores_ex: the split-precision modes multiply an fp32 shard (this one is stored as %s)",
                  storage_name(ix->storage));
    MDX_CHECK_ARG(nq > 0 && nq < (1 << 20), "mdx_scores_ex: nq=%lld", (long long)nq);
    MDX_CHECK_ARG(qlayout == MDX_DIM_MAJOR || qlayout == MDX_ROW_MAJOR, "mdx_scores_ex: qlayout %d", qlayout);
    const int64_t need = mdx_scores_workspace_ex(nq, ix->d, compute);
    MDX_CHECK_WORKSPACE("mdx_scores_ex", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    u32x4 *qp = (u32x4 *)workspace;
    const int64_t QT_total = ceil_div(nq, TILE_ROWS), NC = ix->KB / 2;
    const int64_t rs = qlayout == MDX_DIM_MAJOR ? 1 : ix->d, ks = qlayout == MDX_DIM_MAJOR ? nq : 1;
    const bool two = compute == MDX_F32_SPLIT2;
    uint32_t *q_cell = two ? (uint32_t *)((char *)workspace + need - 256) : nullptr;
    const float db_scale = two ? split2_scale(ix->max_bits) : 1.0f;
    if (two) {
        // the queries' largest |q - center| stays on the device: a reduction, then the re-tiling and the kernel's epilogue read it
        MDX_HIP(hipMemsetAsync(q_cell, 0, 4, s));
        const int64_t total = nq * ix->d;
        hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)(ceil_div(total, (int64_t)1024) < 1024 ? ceil_div(total, (int64_t)1024) : 1024)), dim3(256), 0, s,
                           queries, rs, ks, nq, ix->d, center, q_cell);
        hipLaunchKernelGGL(retile_split2_kernel, dim3((unsigned)ceil_div(QT_total * NC, (int64_t)4)), dim3(256), 0, s, queries, rs, ks, nq, ix->d,
                           center, (const uint32_t *)q_cell, qp, QT_total, NC);
    } else {
        hipLaunchKernelGGL(retile_split3_kernel, dim3((unsigned)ceil_div(QT_total * NC, (int64_t)4)), dim3(256), 0, s, queries, rs, ks, nq, ix->d,
                           center, qp, QT_total, NC);
    }
    MDX_LAUNCH_CHECK();
    const Shard sh{ix->tiles, ix->n, ix->RT, (int)ix->KB, s, 0};
    const bool r2 = ix->RT >= SPLIT_R2_MIN_RT;
    // the kernels find a group's pieces and scores themselves, from the call's pointers and the group's first tile
    return for_query_groups(nq, SPLIT_QT, true, [&](const QGroup &g) {
        return with_qt<SPLIT_QT>(g.tiles, [&](auto qt) {
            constexpr int QT = decltype(qt)::value;
            if (two)
                return r2 ? launch_split<QT, 2, true>(g, sh, qp, scores, (int)QT_total, (int)nq, db_scale, q_cell)
                          : launch_split<QT, 1, true>(g, sh, qp, scores, (int)QT_total, (int)nq, db_scale, q_cell);
            return r2 ? launch_split<QT, 2, false>(g, sh, qp, scores, (int)QT_total, (int)nq, db_scale, q_cell)
                      : launch_split<QT, 1, false>(g, sh, qp, scores, (int)QT_total, (int)nq, db_scale, q_cell);
        });
    });
}

}  // extern "C"
