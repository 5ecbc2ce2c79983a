// Diffusion re-ranking on a mutual kNN graph of the database (Iscen, Tolias, Avrithis, Furon, Chum, "Efficient diffusion
// on region manifolds", CVPR 2017): the graph build from per-row top-k lists and the conjugate-gradient solve of
// (I - alpha S) f = y for a block of queries.  The contract is in include/mdx.h.
//
// mdx_knn_graph, two launches:
//   1. one wave per row i: lane e takes the edge L_i[e] = j (its first copy only), scans L_j for the first copy of i
//      (mutual test), keeps the weight
//      max(s, 0) ** gamma of the similarity recorded in the list of min(i, j), compacts the kept edges in L_i order with a
//      ballot prefix, and sums the degree as an fp32 sequential sum in that order (v_readlane walk, wave-uniform);
//   2. one thread per stored entry: S_ij = w_ij * (r_lo * r_hi), r = 1 / sqrt(d + 1e-12) from the workspace.
// mdx_diffusion: the work arrays F, R, P, AP are node-major [n, nqp] (nqp = nq rounded up to 4), so one edge gathers one
// contiguous row of nqp floats; lane l of a wave owns the columns 4l .. 4l + 3 (one dwordx4).  Per CG step:
//   spmm      AP = P - alpha * S P (one wave per graph row, eight edge rows in flight), fused with the p . Ap partials;
//   reduce    per column, the partials summed in a fixed order -> a_c = rr_c / pAp_c;
//   update    F += a P, R -= a AP, fused with the r . r partials;
//   reduce    -> beta_c = rr'_c / rr_c, the step count and the device-side stop;
//   direction P = R + beta P (not after the last step).
// The partials use a fixed partition of the rows (PART rows per workgroup, independent of nq) and are summed in one fixed
// order, so every output is bit-identical from run to run and a column's bits do not depend on the other columns of the
// launch.  No float atomics.  Nothing is read back to the host and the launch sequence depends on iters only.
// mdx_diffusion_truncated: each query's CG on the subgraph induced by its top-R first-stage rows, one workgroup of 1024
// threads per query, every vector in LDS:
//   (a) the R ids with their local positions as 64-bit keys (id << 32 | position), bitonic-sorted in LDS; an edge's
//       membership is a binary search; a repeated id is a node at its first position only, an id outside [0, n) is none;
//   (b) one wave per local row: the row's ELL entries in order, the in-set edges compacted by ballot into the per-query
//       workspace as (local column, w), stored edge-major [k][R] (lane l of a wave reads row a + l: one coalesced load per
//       edge slot), the degree an fp32 sequential sum in edge order; then S = w * (r_a * r_b) in place;
//   (c) CG with r, f, p, Ap in LDS, one thread per row (rows t, t + 1024, ...), the row's SpMV an fp32 fma chain in edge
//       order with the edges streamed from the workspace (L2 / MALL resident);
//   (d) the dot products: per-thread fma partials over the thread's rows, a butterfly inside each wave, the 16 wave sums in
//       wave order: fixed, so a query's bits do not depend on the other queries;
//   (e) f [nq, R] to the workspace.  Two output launches: out = s - 3 over [nq, n], then the positive f scattered to t_a.
#include <math.h>

#include "mdx_common.h"

namespace mdx {

constexpr int DIF_WAVES = 4;                          // waves per workgroup
constexpr int DIF_ROWS_PER_WAVE = 8;                  // consecutive graph rows per wave
constexpr int DIF_PART = DIF_WAVES * DIF_ROWS_PER_WAVE;   // rows per partition (one partial per column)
constexpr int DIF_GATHER = 8;                         // edge rows in flight per wave
constexpr int DIF_MAX_NQ = 256;                       // 64 lanes x float4
constexpr int DIF_REDUCE = 256;                       // threads per column in the reductions

enum { ST_RR = 0, ST_YY, ST_A, ST_BETA, ST_ACTIVE, ST_STEPS, ST_COUNT };   // per-column state, DIF_MAX_NQ words each

__device__ __forceinline__ float graph_weight(float s, float gamma) { return powf(fmaxf(s, 0.0f), gamma); }

__device__ __forceinline__ float readlane_f(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ void fma4(float4 &acc, float w, float4 x)
{
    acc.x = fmaf(w, x.x, acc.x);
    acc.y = fmaf(w, x.y, acc.y);
    acc.z = fmaf(w, x.z, acc.z);
    acc.w = fmaf(w, x.w, acc.w);
}

// ------------------------------------------------------------------------------------------------------ graph build

__global__ __launch_bounds__(64 * DIF_WAVES) void knn_graph_edges_kernel(
    const int64_t *__restrict__ ids, const float *__restrict__ sims, int64_t n, int64_t k, float gamma,
    int32_t *__restrict__ cols, float *__restrict__ vals, int32_t *__restrict__ counts, float *__restrict__ rinv)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * DIF_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                   // whole waves only
    const int64_t *li = ids + i * k;
    const float *si = sims + i * k;
    int64_t count = 0;
    float deg = 0.0f;
    for (int64_t eb = 0; eb < k; eb += 64) {
        const int64_t e = eb + lane;
        bool keep = false;
        int64_t j = -1;
        float w = 0.0f;
        if (e < k) {
            j = li[e];
            int64_t first = e;                            // a repeated id: only its first copy in L_i is an edge
            for (int64_t t = 0; t < e; ++t) {
                if (li[t] == j) {
                    first = t;
                    break;
                }
            }
            if (first == e && j >= 0 && j < n && j != i) {
                const int64_t *lj = ids + j * k;
                for (int64_t t = 0; t < k; ++t) {
                    if (lj[t] == i) {                     // mutual: the similarity of the list of min(i, j)
                        keep = true;
                        w = graph_weight(i < j ? si[e] : sims[j * k + t], gamma);
                        break;
                    }
                }
            }
        }
        uint64_t mask = __ballot(keep);
        if (keep) {
            const int64_t pos = count + __builtin_popcountll(mask & ((1ull << lane) - 1));
            cols[i * k + pos] = (int32_t)j;
            vals[i * k + pos] = w;
        }
        count += __builtin_popcountll(mask);
        while (mask) {                                    // the degree: fp32 sequential sum in L_i order
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            deg += readlane_f(w, src);
        }
    }
    for (int64_t e = count + lane; e < k; e += 64) {      // defined padding: no edge
        cols[i * k + e] = -1;
        vals[i * k + e] = 0.0f;
    }
    if (lane == 0) {
        counts[i] = (int32_t)count;
        rinv[i] = 1.0f / sqrtf(deg + 1e-12f);
    }
}

__global__ __launch_bounds__(256) void knn_graph_normalise_kernel(const int32_t *__restrict__ cols, float *__restrict__ vals,
                                                                 const int32_t *__restrict__ counts,
                                                                 const float *__restrict__ rinv, int64_t n, int64_t k)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n * k) return;
    const int64_t i = x / k, e = x - i * k;
    if (e >= counts[i]) return;
    const int64_t j = cols[x];
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    vals[x] = vals[x] * (rinv[lo] * rinv[hi]);            // fixed operand order: S is exactly symmetric
}

// ---------------------------------------------------------------------------------------------------------- solve

struct DifWs {
    float *F, *R, *P, *AP;                                // [n, nqp] node-major
    float *part;                                          // [DIF_MAX_NQ][nparts] column-major partials
    float *st;                                            // [ST_COUNT][DIF_MAX_NQ]
};

static int64_t dif_nparts(int64_t n) { return ceil_div(n, DIF_PART); }

// byte layout of the workspace (ws == nullptr: size only)
static int64_t dif_carve(DifWs *ws, char *base, int64_t n, int64_t nq)
{
    const int64_t nqp = round_up(nq, 4);
    const int64_t block = round_up(n * nqp * (int64_t)sizeof(float), 256);
    const int64_t part = round_up(DIF_MAX_NQ * dif_nparts(n) * (int64_t)sizeof(float), 256);
    const int64_t st = round_up(ST_COUNT * DIF_MAX_NQ * (int64_t)sizeof(float), 256);
    if (ws) {
        ws->F = (float *)base;
        ws->R = (float *)(base + block);
        ws->P = (float *)(base + 2 * block);
        ws->AP = (float *)(base + 3 * block);
        ws->part = (float *)(base + 4 * block);
        ws->st = (float *)(base + 4 * block + part);
    }
    return 4 * block + part + st;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *(const float4 *)p; }
__device__ __forceinline__ void st4(float *p, float4 v) { *(float4 *)p = v; }

// the four per-column partials of a lane, summed over the workgroup's waves in wave order, stored column-major
__device__ __forceinline__ void write_partials(float4 mine, float *part, int64_t nparts, int64_t nqp)
{
    __shared__ float4 red[DIF_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    red[wave][lane] = mine;
    __syncthreads();
    if (wave == 0 && 4 * lane < nqp) {
        float4 s = red[0][lane];
#pragma unroll
        for (int w = 1; w < DIF_WAVES; ++w) {
            const float4 o = red[w][lane];
            s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
        }
        const int64_t c = 4 * lane, p = blockIdx.x;
        part[(c + 0) * nparts + p] = s.x;
        part[(c + 1) * nparts + p] = s.y;
        part[(c + 2) * nparts + p] = s.z;
        part[(c + 3) * nparts + p] = s.w;
    }
}

// y_j = max(s, 0) ** gamma for the seeds of column c (one thread per column: a repeated id keeps its last value)
__global__ __launch_bounds__(256) void diffusion_seed_kernel(const int64_t *__restrict__ seed_ids,
                                                             const float *__restrict__ seed_sims, int64_t n, int64_t nq,
                                                             int64_t nqp, int64_t kq, float gamma, float *__restrict__ R,
                                                             float *__restrict__ P)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nq) return;
    for (int64_t t = 0; t < kq; ++t) {
        const int64_t j = seed_ids[c * kq + t];
        if (j < 0 || j >= n) continue;
        const float y = graph_weight(seed_sims[c * kq + t], gamma);
        R[j * nqp + c] = y;
        P[j * nqp + c] = y;
    }
}

// AP = P - alpha * S P, and the p . Ap partials of this partition
__global__ __launch_bounds__(64 * DIF_WAVES) void diffusion_spmm_kernel(
    const int32_t *__restrict__ cols, const float *__restrict__ vals, const int32_t *__restrict__ counts, int64_t n,
    int64_t k, const float *__restrict__ P, float *__restrict__ AP, int64_t nqp, float alpha, float *__restrict__ part,
    int64_t nparts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = 4 * lane < nqp;
    const int64_t c = on ? 4 * lane : 0;
    const int64_t row0 = (int64_t)blockIdx.x * DIF_PART + wave * DIF_ROWS_PER_WAVE;
    float4 dot = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int r = 0; r < DIF_ROWS_PER_WAVE; ++r) {
        const int64_t i = row0 + r;
        if (i >= n) break;                                // wave-uniform
        int64_t cnt = counts[i];
        cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int64_t eb = 0; eb < cnt; eb += 64) {
            // this chunk's (col, val), one edge per lane; a column outside [0, n) is no edge and is never read
            const int64_t e = eb + lane;
            int32_t col = -1;
            float val = 0.0f;
            if (e < cnt) {
                col = cols[i * k + e];
                val = vals[i * k + e];
            }
            const int m = (int)(cnt - eb < 64 ? cnt - eb : 64);
            for (int b = 0; b < m; b += DIF_GATHER) {
                float4 g[DIF_GATHER];
                bool ok[DIF_GATHER];
#pragma unroll
                for (int t = 0; t < DIF_GATHER; ++t) {    // all gathers of the batch before any FMA
                    const int j = b + t < m ? __builtin_amdgcn_readlane(col, b + t) : -1;
                    ok[t] = j >= 0 && j < n;
                    g[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (ok[t] && on) g[t] = ld4(P + (int64_t)j * nqp + c);
                }
#pragma unroll
                for (int t = 0; t < DIF_GATHER; ++t)      // edge order: the row's fixed fma chain
                    if (ok[t]) fma4(acc, readlane_f(val, b + t), g[t]);
            }
        }
        if (on) {
            const float4 p = ld4(P + i * nqp + c);
            float4 ap;
            ap.x = fmaf(-alpha, acc.x, p.x);
            ap.y = fmaf(-alpha, acc.y, p.y);
            ap.z = fmaf(-alpha, acc.z, p.z);
            ap.w = fmaf(-alpha, acc.w, p.w);
            st4(AP + i * nqp + c, ap);
            dot.x = fmaf(p.x, ap.x, dot.x);
            dot.y = fmaf(p.y, ap.y, dot.y);
            dot.z = fmaf(p.z, ap.z, dot.z);
            dot.w = fmaf(p.w, ap.w, dot.w);
        }
    }
    write_partials(dot, part, nparts, nqp);
}

// INIT: only the r . r partials (of the seeded R); else F += a P, R -= a AP, then the r . r partials
template <bool INIT>
__global__ __launch_bounds__(64 * DIF_WAVES) void diffusion_update_kernel(float *__restrict__ F, float *__restrict__ R,
                                                                          const float *__restrict__ P,
                                                                          const float *__restrict__ AP, int64_t n,
                                                                          int64_t nqp, const float *__restrict__ st,
                                                                          float *__restrict__ part, int64_t nparts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = 4 * lane < nqp;
    const int64_t c = on ? 4 * lane : 0;
    const int64_t row0 = (int64_t)blockIdx.x * DIF_PART + wave * DIF_ROWS_PER_WAVE;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!INIT && on) a = ld4(st + ST_A * DIF_MAX_NQ + c);
    float4 rr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (on) {
#pragma unroll 4
        for (int r = 0; r < DIF_ROWS_PER_WAVE; ++r) {
            const int64_t i = row0 + r;
            if (i >= n) break;
            float4 rv = ld4(R + i * nqp + c);
            if (!INIT) {
                float4 f = ld4(F + i * nqp + c);
                const float4 p = ld4(P + i * nqp + c), ap = ld4(AP + i * nqp + c);
                f.x = fmaf(a.x, p.x, f.x); f.y = fmaf(a.y, p.y, f.y); f.z = fmaf(a.z, p.z, f.z); f.w = fmaf(a.w, p.w, f.w);
                rv.x = fmaf(-a.x, ap.x, rv.x); rv.y = fmaf(-a.y, ap.y, rv.y);
                rv.z = fmaf(-a.z, ap.z, rv.z); rv.w = fmaf(-a.w, ap.w, rv.w);
                st4(F + i * nqp + c, f);
                st4(R + i * nqp + c, rv);
            }
            rr.x = fmaf(rv.x, rv.x, rr.x); rr.y = fmaf(rv.y, rv.y, rr.y);
            rr.z = fmaf(rv.z, rv.z, rr.z); rr.w = fmaf(rv.w, rv.w, rr.w);
        }
    }
    write_partials(rr, part, nparts, nqp);
}

// P = R + beta P (beta = 0 for a stopped column)
__global__ __launch_bounds__(256) void diffusion_direction_kernel(const float *__restrict__ R, float *__restrict__ P,
                                                                  int64_t n, int64_t nqp, const float *__restrict__ st)
{
    const int64_t x = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= n * nqp) return;
    const int64_t c = x % nqp;                            // nqp % 4 == 0: the four columns of one row
    const float4 b = ld4(st + ST_BETA * DIF_MAX_NQ + c);
    const float4 r = ld4(R + x);
    float4 p = ld4(P + x);
    p.x = fmaf(b.x, p.x, r.x); p.y = fmaf(b.y, p.y, r.y); p.z = fmaf(b.z, p.z, r.z); p.w = fmaf(b.w, p.w, r.w);
    st4(P + x, p);
}

enum { RED_INIT = 0, RED_PAP = 1, RED_RR = 2 };

// one workgroup per column: the partials in a fixed order (strided per thread, then a fixed LDS tree), then the scalar
// recurrences of CG on that column's state
__global__ __launch_bounds__(DIF_REDUCE) void diffusion_reduce_kernel(const float *__restrict__ part, int64_t nparts,
                                                                      float *__restrict__ st, int mode, float tol2)
{
    __shared__ float buf[DIF_REDUCE];
    const int c = blockIdx.x, t = threadIdx.x;
    const float *pc = part + (int64_t)c * nparts;
    float s = 0.0f;
    for (int64_t p = t; p < nparts; p += DIF_REDUCE) s += pc[p];
    buf[t] = s;
    __syncthreads();
    for (int h = DIF_REDUCE / 2; h > 0; h >>= 1) {
        if (t < h) buf[t] += buf[t + h];
        __syncthreads();
    }
    if (t != 0) return;
    const float total = buf[0];
    float *rr = st + ST_RR * DIF_MAX_NQ + c, *yy = st + ST_YY * DIF_MAX_NQ + c, *a = st + ST_A * DIF_MAX_NQ + c;
    float *beta = st + ST_BETA * DIF_MAX_NQ + c;
    int *active = (int *)(st + ST_ACTIVE * DIF_MAX_NQ) + c, *steps = (int *)(st + ST_STEPS * DIF_MAX_NQ) + c;
    if (mode == RED_INIT) {
        *rr = total;
        *yy = total;
        *a = 0.0f;
        *beta = 0.0f;
        *steps = 0;
        *active = total > 0.0f && !(total <= tol2 * total);
    } else if (mode == RED_PAP) {
        const bool go = *active && total > 0.0f && isfinite(total);   // A is SPD: p . Ap > 0 unless p == 0
        *a = go ? *rr / total : 0.0f;
        if (!go) *active = 0;
    } else {
        if (*active) {
            *steps += 1;
            *beta = total / *rr;
            *rr = total;
            if (total <= tol2 * *yy) *active = 0;
        }
        if (!*active) *beta = 0.0f;
    }
}

// out[c, j] = F[j, c] if > 0, else scores[c, j] - 3: a 64 x 64 tile transposed through LDS; the per-column residual and
// step count from block (0, 0)
__global__ __launch_bounds__(256) void diffusion_final_kernel(const float *__restrict__ F, int64_t n, int64_t nq,
                                                              int64_t nqp, const float *scores, int64_t ld_scores, float *out,
                                                              int64_t ld_out, const float *__restrict__ st,
                                                              float *__restrict__ residual, int32_t *__restrict__ steps)
{
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    for (int x = t; x < 64 * 64; x += 256) {
        const int jj = x >> 6, cc = x & 63;
        const int64_t j = j0 + jj, c = c0 + cc;
        tile[cc][jj] = (j < n && c < nq) ? F[j * nqp + c] : 0.0f;
    }
    __syncthreads();
    for (int x = t; x < 64 * 64; x += 256) {
        const int cc = x >> 6, jj = x & 63;
        const int64_t j = j0 + jj, c = c0 + cc;
        if (j >= n || c >= nq) continue;
        const float f = tile[cc][jj];
        const float s = scores[c * ld_scores + j];        // read before the write: out may be scores
        out[c * ld_out + j] = f > 0.0f ? f : s - 3.0f;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int64_t c = t; c < nq; c += 256) {
            const float yy = st[ST_YY * DIF_MAX_NQ + c], rr = st[ST_RR * DIF_MAX_NQ + c];
            if (residual) residual[c] = yy > 0.0f ? sqrtf(rr / yy) : 0.0f;
            if (steps) steps[c] = ((const int *)(st + ST_STEPS * DIF_MAX_NQ))[c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- truncated solve

constexpr int TRD_THREADS = 1024;                                 // one workgroup per query
constexpr int TRD_WAVES = TRD_THREADS / 64;
constexpr int TRD_ROWS = MDX_DIFFUSION_MAX_R / TRD_THREADS;       // local rows per thread at most
constexpr int TRD_GATHER = 8;                                     // edges in flight per thread in the SpMV
constexpr uint32_t TRD_NONE = 0x7FFFFFFFu;                        // key id of a non-node (no column equals it: n < 2^31)
static_assert(MDX_DIFFUSION_MAX_R % TRD_THREADS == 0, "rows per thread");

__host__ __device__ inline int64_t trd_round(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

__host__ __device__ inline int64_t trd_pow2(int64_t r)
{
    int64_t p = 1;
    while (p < r) p <<= 1;
    return p;
}

// bytes of dynamic LDS: keys [P] u64, then rinv, f, r, p, ap [round_up(R, 4)] fp32, then the 2 x 16 wave sums
__host__ __device__ inline int64_t trd_lds(int64_t r) { return 8 * trd_pow2(r) + 5 * 4 * trd_round(r, 4) + 2 * TRD_WAVES * 4; }

// per query: edges int2 [k][R] (local column, w then S), edge counts int32 [R], f fp32 [R]
__host__ __device__ inline int64_t trd_edges_bytes(int64_t k, int64_t r) { return trd_round(k * r * 8, 256); }
__host__ __device__ inline int64_t trd_query_bytes(int64_t k, int64_t r) { return trd_edges_bytes(k, r) + 2 * trd_round(r * 4, 256); }

// the sum of v over the workgroup, the same bits in every thread: a butterfly in the wave, then the wave sums in order
__device__ __forceinline__ float trd_block_sum(float v, float *red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < TRD_WAVES; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(TRD_THREADS) void diffusion_truncated_solve_kernel(
    const int32_t *__restrict__ cols, const float *__restrict__ wts, const int32_t *__restrict__ counts, int64_t n, int64_t k,
    const int64_t *__restrict__ top_ids, const float *__restrict__ top_sims, int r, int64_t kq, float gamma, float alpha,
    int64_t iters, float tol2, char *__restrict__ ws, float *__restrict__ residual, int32_t *__restrict__ steps_out)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t q = blockIdx.x;
    const int P = (int)trd_pow2(r), rp = (int)trd_round(r, 4);
    uint64_t *keys = (uint64_t *)lds;
    float *rinv = (float *)(lds + 8 * P), *fv = rinv + rp, *rv = fv + rp, *pv = rv + rp, *apv = pv + rp;
    float *red = apv + rp;
    int *node = (int *)apv;                                       // until the CG starts: 1 = a node, 0 = none
    const int64_t *ids = top_ids + q * r;
    char *wq = ws + q * trd_query_bytes(k, r);
    int2 *edges = (int2 *)wq;
    int32_t *ecount = (int32_t *)(wq + trd_edges_bytes(k, r));
    float *F = (float *)(wq + trd_edges_bytes(k, r) + trd_round((int64_t)r * 4, 256));

    // (a) keys and the bitonic sort (the keys are distinct: the order is fixed)
    for (int i = t; i < P; i += TRD_THREADS) {
        uint32_t id = TRD_NONE;
        if (i < r) {
            const int64_t g = ids[i];
            if (g >= 0 && g < n) id = (uint32_t)g;
        }
        keys[i] = (uint64_t)id << 32 | (uint32_t)i;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = t; i < P / 2; i += TRD_THREADS) {
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < P; i += TRD_THREADS) {
        const uint64_t key = keys[i];
        const uint32_t pos = (uint32_t)key, id = (uint32_t)(key >> 32);
        if (pos < (uint32_t)r) node[pos] = id != TRD_NONE && (i == 0 || (uint32_t)(keys[i - 1] >> 32) != id);
    }
    __syncthreads();

    // (b) the in-set edges of every node's ELL row, in row order; the degree; r = 1 / sqrt(d + 1e-12)
    for (int a = wave; a < r; a += TRD_WAVES) {
        int64_t cnt = 0, i = 0;
        if (node[a]) {
            i = ids[a];
            cnt = counts[i];
            cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
        }
        int c = 0;
        float deg = 0.0f;
        for (int64_t eb = 0; eb < cnt; eb += 64) {
            const int64_t e = eb + lane;
            int b = -1;
            float w = 0.0f;
            if (e < cnt) {
                const int64_t j = cols[i * k + e];
                if (j >= 0 && j < n) {                            // lower bound of (j, 0) among the keys
                    const uint64_t want = (uint64_t)j << 32;
                    int lo = 0, len = P;
                    while (len > 0) {
                        const int half = len >> 1;
                        if (keys[lo + half] < want) {
                            lo += half + 1;
                            len -= half + 1;
                        } else {
                            len = half;
                        }
                    }
                    if (lo < P && (uint32_t)(keys[lo] >> 32) == (uint32_t)j) b = (int)(uint32_t)keys[lo];
                }
                if (b >= 0) w = wts[i * k + e];
            }
            uint64_t mask = __ballot(b >= 0);
            if (b >= 0) {
                const int pos = c + __builtin_popcountll(mask & ((1ull << lane) - 1));
                edges[(int64_t)pos * r + a] = make_int2(b, __float_as_int(w));
            }
            c += __builtin_popcountll(mask);
            while (mask) {                                        // fp32 sequential sum in edge order
                const int src = __builtin_ctzll(mask);
                mask &= mask - 1;
                deg += readlane_f(w, src);
            }
        }
        if (lane == 0) {
            ecount[a] = c;
            rinv[a] = 1.0f / sqrtf(deg + 1e-12f);
        }
    }
    __syncthreads();

    // S = w * (r_a * r_b) (the product of the two r is commutative: S is exactly symmetric, and with R = N it is
    // mdx_knn_graph's S bit for bit); f = 0, r = p = y; y . y
    const int kseed = (int)(kq < r ? kq : r);
    int rc[TRD_ROWS];
    float part = 0.0f;
#pragma unroll
    for (int u = 0; u < TRD_ROWS; ++u) {
        const int a = t + u * TRD_THREADS;
        rc[u] = 0;
        if (a >= r) continue;
        const int c = ecount[a];
        rc[u] = c;
        const float ra = rinv[a];
        for (int e = 0; e < c; ++e) {
            int2 ed = edges[(int64_t)e * r + a];
            ed.y = __float_as_int(__int_as_float(ed.y) * (ra * rinv[ed.x]));
            edges[(int64_t)e * r + a] = ed;
        }
        const float y = a < kseed && node[a] ? graph_weight(top_sims[q * r + a], gamma) : 0.0f;
        fv[a] = 0.0f;
        rv[a] = y;
        pv[a] = y;
        part = fmaf(y, y, part);
    }
    __syncthreads();                                              // node[] (apv) is read above: ap is written below
    const float yy = trd_block_sum(part, red + TRD_WAVES);
    float rr = yy;
    int steps = 0;
    bool active = yy > 0.0f && !(yy <= tol2 * yy);

    // (c) CG: the recurrence and the stop rule of mdx_diffusion; a stopped query's later steps there change nothing
    for (int64_t it = 0; it < iters && active; ++it) {
        float dot = 0.0f;
#pragma unroll
        for (int u = 0; u < TRD_ROWS; ++u) {
            const int a = t + u * TRD_THREADS;
            if (a >= r) continue;
            const int c = rc[u];
            float acc = 0.0f;
            for (int e0 = 0; e0 < c; e0 += TRD_GATHER) {
                int2 ed[TRD_GATHER];
#pragma unroll
                for (int g = 0; g < TRD_GATHER; ++g)             // the batch's loads before any FMA
                    ed[g] = e0 + g < c ? edges[(int64_t)(e0 + g) * r + a] : make_int2(0, 0);
#pragma unroll
                for (int g = 0; g < TRD_GATHER; ++g)             // edge order: the row's fixed fma chain
                    if (e0 + g < c) acc = fmaf(__int_as_float(ed[g].y), pv[ed[g].x], acc);
            }
            const float p = pv[a], ap = fmaf(-alpha, acc, p);
            apv[a] = ap;
            dot = fmaf(p, ap, dot);
        }
        const float pap = trd_block_sum(dot, red);
        if (!(pap > 0.0f && isfinite(pap))) break;                // A is SPD: p . Ap > 0 unless p == 0
        const float step = rr / pap;
        part = 0.0f;
#pragma unroll
        for (int u = 0; u < TRD_ROWS; ++u) {
            const int a = t + u * TRD_THREADS;
            if (a >= r) continue;
            fv[a] = fmaf(step, pv[a], fv[a]);
            const float x = fmaf(-step, apv[a], rv[a]);
            rv[a] = x;
            part = fmaf(x, x, part);
        }
        const float rrn = trd_block_sum(part, red + TRD_WAVES);
        ++steps;
        const float beta = rrn / rr;
        rr = rrn;
        if (rrn <= tol2 * yy) active = false;
        if (active && it + 1 < iters) {
#pragma unroll
            for (int u = 0; u < TRD_ROWS; ++u) {
                const int a = t + u * TRD_THREADS;
                if (a < r) pv[a] = fmaf(beta, pv[a], rv[a]);
            }
            __syncthreads();                                      // the next SpMV reads every row's p
        }
    }

    // (e) f of this thread's rows; the residual and the step count
#pragma unroll
    for (int u = 0; u < TRD_ROWS; ++u) {
        const int a = t + u * TRD_THREADS;
        if (a < r) F[a] = fv[a];
    }
    if (t == 0) {
        if (residual) residual[q] = yy > 0.0f ? sqrtf(rr / yy) : 0.0f;
        if (steps_out) steps_out[q] = steps;
    }
}

// out[q, j] = scores[q, j] - 3, 4096 entries of one row per workgroup (VEC: 16-byte aligned rows, float4)
template <bool VEC>
__global__ __launch_bounds__(256) void diffusion_truncated_base_kernel(const float *scores, int64_t ld_scores, float *out,
                                                                       int64_t ld_out, int64_t n, int64_t nblk)
{
    const int64_t q = blockIdx.x / nblk, j0 = (blockIdx.x - q * nblk) * (int64_t)4096;
    const float *s = scores + q * ld_scores;
    float *o = out + q * ld_out;
    if (VEC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int64_t j = j0 + (u * 256 + threadIdx.x) * 4;
            if (j + 4 <= n) {
                float4 v = ld4(s + j);
                v.x -= 3.0f; v.y -= 3.0f; v.z -= 3.0f; v.w -= 3.0f;
                st4(o + j, v);
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

// out[q, t_a] = f_a where f_a > 0 (a non-node keeps f = 0 and is never written)
__global__ __launch_bounds__(256) void diffusion_truncated_scatter_kernel(const char *__restrict__ ws, int64_t k, int64_t r,
                                                                          const int64_t *__restrict__ top_ids, int64_t n,
                                                                          int64_t nq, float *out, int64_t ld_out)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= nq * r) return;
    const int64_t q = x / r, a = x - q * r;
    const float *F = (const float *)(ws + q * trd_query_bytes(k, r) + trd_edges_bytes(k, r) + trd_round(r * 4, 256));
    const float f = F[a];
    const int64_t id = top_ids[x];
    if (f > 0.0f && id >= 0 && id < n) out[q * ld_out + id] = f;
}

static bool overlaps(const void *a, int64_t bytes_a, const void *b, int64_t bytes_b)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_knn_graph_workspace(int64_t n)
{
    if (n <= 0) return 0;
    return round_up(n * (int64_t)sizeof(float), 256);
}

int mdx_knn_graph(const int64_t *ids, const float *sims, int64_t n, int64_t k, float gamma, int32_t *cols, float *vals,
                  int32_t *counts, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(ids && sims && cols && vals && counts && workspace,
                  "mdx_knn_graph: NULL pointer (ids, sims, cols, vals, counts and workspace are required)");
    MDX_CHECK_ARG(n >= 1 && k >= 1, "mdx_knn_graph: n=%lld k=%lld (each must be >= 1)", (long long)n, (long long)k);
    MDX_CHECK_ARG(n < (1ll << 31), "mdx_knn_graph: n=%lld must be < 2^31 (cols are int32)", (long long)n);
    MDX_CHECK_ARG(k <= (1ll << 20), "mdx_knn_graph: k=%lld too large", (long long)k);
    MDX_CHECK_ARG(isfinite(gamma) && gamma >= 0.0f, "mdx_knn_graph: gamma=%g must be finite and >= 0", (double)gamma);
    const int64_t need = mdx_knn_graph_workspace(n);
    MDX_CHECK_WORKSPACE("mdx_knn_graph", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float *rinv = (float *)workspace;
    hipLaunchKernelGGL(knn_graph_edges_kernel, dim3((unsigned)ceil_div(n, DIF_WAVES)), dim3(64 * DIF_WAVES), 0, s, ids, sims,
                       n, k, gamma, cols, vals, counts, rinv);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_graph_normalise_kernel, dim3((unsigned)ceil_div(n * k, 256)), dim3(256), 0, s, cols, vals, counts,
                       rinv, n, k);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_diffusion_workspace(int64_t n, int64_t nq)
{
    if (n <= 0 || nq <= 0 || nq > DIF_MAX_NQ) return 0;
    return dif_carve(nullptr, nullptr, n, nq);
}

int mdx_diffusion(const int32_t *cols, const float *vals, const int32_t *counts, int64_t n, int64_t k, const float *scores,
                  int64_t ld_scores, const int64_t *seed_ids, const float *seed_sims, int64_t nq, int64_t kq, float gamma,
                  float alpha, int64_t iters, float tol, float *out, int64_t ld_out, float *residual, int32_t *steps,
                  void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(cols && vals && counts && scores && seed_ids && seed_sims && out && workspace,
                  "mdx_diffusion: NULL pointer (cols, vals, counts, scores, seed_ids, seed_sims, out and workspace are "
                  "required)");
    MDX_CHECK_ARG(n >= 1 && k >= 1 && nq >= 1 && kq >= 1, "mdx_diffusion: n=%lld k=%lld nq=%lld kq=%lld (each must be >= 1)",
                  (long long)n, (long long)k, (long long)nq, (long long)kq);
    MDX_CHECK_ARG(nq <= DIF_MAX_NQ, "mdx_diffusion: nq=%lld > %d per call (split the queries)", (long long)nq, DIF_MAX_NQ);
    MDX_CHECK_ARG(n < (1ll << 31), "mdx_diffusion: n=%lld must be < 2^31 (cols are int32)", (long long)n);
    MDX_CHECK_ARG(k <= (1ll << 20) && kq <= (1ll << 20), "mdx_diffusion: k=%lld or kq=%lld too large", (long long)k,
                  (long long)kq);
    MDX_CHECK_ARG(ld_scores >= n && ld_out >= n, "mdx_diffusion: ld_scores=%lld ld_out=%lld must be >= n=%lld",
                  (long long)ld_scores, (long long)ld_out, (long long)n);
    MDX_CHECK_ARG(isfinite(gamma) && gamma >= 0.0f, "mdx_diffusion: gamma=%g must be finite and >= 0", (double)gamma);
    MDX_CHECK_ARG(alpha >= 0.0f && alpha < 1.0f, "mdx_diffusion: alpha=%g must be in [0, 1)", (double)alpha);
    MDX_CHECK_ARG(iters >= 1, "mdx_diffusion: iters=%lld must be >= 1", (long long)iters);
    MDX_CHECK_ARG(isfinite(tol) && tol >= 0.0f, "mdx_diffusion: tol=%g must be finite and >= 0", (double)tol);
    const int64_t span = ((nq - 1) * ld_out + n) * (int64_t)sizeof(float);
    MDX_CHECK_ARG((out == scores && ld_out == ld_scores) ||
                      !overlaps(out, span, scores, ((nq - 1) * ld_scores + n) * (int64_t)sizeof(float)),
                  "mdx_diffusion: out overlaps scores (only out == scores with the same stride is allowed)");
    const int64_t need = dif_carve(nullptr, nullptr, n, nq);
    MDX_CHECK_WORKSPACE("mdx_diffusion", workspace, workspace_bytes, need);
    DifWs ws;
    dif_carve(&ws, (char *)workspace, n, nq);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nqp = round_up(nq, 4), nparts = dif_nparts(n);
    const float tol2 = tol * tol;
    const dim3 parts((unsigned)nparts), wg(64 * DIF_WAVES), cols_grid((unsigned)nq), red(DIF_REDUCE);

    // f = 0, r = p = y
    MDX_HIP(hipMemsetAsync(ws.F, 0, (size_t)(3 * ((char *)ws.R - (char *)ws.F)), s));   // F, R, P are adjacent
    MDX_HIP(hipMemsetAsync(ws.st, 0, ST_COUNT * DIF_MAX_NQ * sizeof(float), s));        // padding columns: a = beta = 0
    hipLaunchKernelGGL(diffusion_seed_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, s, seed_ids, seed_sims, n, nq,
                       nqp, kq, gamma, ws.R, ws.P);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(diffusion_update_kernel<true>, parts, wg, 0, s, ws.F, ws.R, ws.P, ws.AP, n, nqp, ws.st, ws.part,
                       nparts);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(diffusion_reduce_kernel, cols_grid, red, 0, s, ws.part, nparts, ws.st, (int)RED_INIT, tol2);
    MDX_LAUNCH_CHECK();
    for (int64_t it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(diffusion_spmm_kernel, parts, wg, 0, s, cols, vals, counts, n, k, ws.P, ws.AP, nqp, alpha,
                           ws.part, nparts);
        MDX_LAUNCH_CHECK();
        hipLaunchKernelGGL(diffusion_reduce_kernel, cols_grid, red, 0, s, ws.part, nparts, ws.st, (int)RED_PAP, tol2);
        MDX_LAUNCH_CHECK();
        hipLaunchKernelGGL(diffusion_update_kernel<false>, parts, wg, 0, s, ws.F, ws.R, ws.P, ws.AP, n, nqp, ws.st, ws.part,
                           nparts);
        MDX_LAUNCH_CHECK();
        hipLaunchKernelGGL(diffusion_reduce_kernel, cols_grid, red, 0, s, ws.part, nparts, ws.st, (int)RED_RR, tol2);
        MDX_LAUNCH_CHECK();
        if (it + 1 < iters) {
            hipLaunchKernelGGL(diffusion_direction_kernel, dim3((unsigned)ceil_div(n * nqp / 4, 256)), dim3(256), 0, s, ws.R,
                               ws.P, n, nqp, ws.st);
            MDX_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(diffusion_final_kernel, dim3((unsigned)ceil_div(n, 64), (unsigned)ceil_div(nq, 64)), dim3(256), 0, s,
                       ws.F, n, nq, nqp, scores, ld_scores, out, ld_out, ws.st, residual, steps);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_knn_graph_weights(const int64_t *ids, const float *sims, int64_t n, int64_t k, float gamma, int32_t *cols, float *w,
                          int32_t *counts, void *workspace, int64_t workspace_bytes, void *stream)
{
    MDX_CHECK_ARG(ids && sims && cols && w && counts && workspace,
                  "mdx_knn_graph_weights: NULL pointer (ids, sims, cols, w, counts and workspace are required)");
    MDX_CHECK_ARG(n >= 1 && k >= 1, "mdx_knn_graph_weights: n=%lld k=%lld (each must be >= 1)", (long long)n, (long long)k);
    MDX_CHECK_ARG(n < (1ll << 31), "mdx_knn_graph_weights: n=%lld must be < 2^31 (cols are int32)", (long long)n);
    MDX_CHECK_ARG(k <= (1ll << 20), "mdx_knn_graph_weights: k=%lld too large", (long long)k);
    MDX_CHECK_ARG(isfinite(gamma) && gamma >= 0.0f, "mdx_knn_graph_weights: gamma=%g must be finite and >= 0", (double)gamma);
    const int64_t need = mdx_knn_graph_workspace(n);
    MDX_CHECK_WORKSPACE("mdx_knn_graph_weights", workspace, workspace_bytes, need);
    hipLaunchKernelGGL(knn_graph_edges_kernel, dim3((unsigned)ceil_div(n, DIF_WAVES)), dim3(64 * DIF_WAVES), 0,
                       (hipStream_t)stream, ids, sims, n, k, gamma, cols, w, counts, (float *)workspace);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int64_t mdx_diffusion_truncated_workspace(int64_t n, int64_t k, int64_t nq, int64_t r)
{
    if (n < 1 || k < 1 || k > (1ll << 20) || nq < 1 || nq >= (1ll << 31) || r < 1 || r > MDX_DIFFUSION_MAX_R || r > n)
        return 0;
    return nq * trd_query_bytes(k, r);
}

int mdx_diffusion_truncated(const int32_t *cols, const float *w, const int32_t *counts, int64_t n, int64_t k,
                            const float *scores, int64_t ld_scores, const int64_t *top_ids, const float *top_sims, int64_t nq,
                            int64_t r, int64_t kq, float gamma, float alpha, int64_t iters, float tol, float *out,
                            int64_t ld_out, float *residual, int32_t *steps, void *workspace, int64_t workspace_bytes,
                            void *stream)
{
    MDX_CHECK_ARG(cols && w && counts && scores && top_ids && top_sims && out && workspace,
                  "mdx_diffusion_truncated: NULL pointer (cols, w, counts, scores, top_ids, top_sims, out and workspace are "
                  "required)");
    MDX_CHECK_ARG(n >= 1 && k >= 1 && nq >= 1 && r >= 1 && kq >= 1,
                  "mdx_diffusion_truncated: n=%lld k=%lld nq=%lld r=%lld kq=%lld (each must be >= 1)", (long long)n,
                  (long long)k, (long long)nq, (long long)r, (long long)kq);
    MDX_CHECK_ARG(r <= MDX_DIFFUSION_MAX_R && r <= n, "mdx_diffusion_truncated: r=%lld must be <= %d and <= n=%lld",
                  (long long)r, MDX_DIFFUSION_MAX_R, (long long)n);
    MDX_CHECK_ARG(n < (1ll << 31), "mdx_diffusion_truncated: n=%lld must be < 2^31 (cols are int32)", (long long)n);
    MDX_CHECK_ARG(k <= (1ll << 20), "mdx_diffusion_truncated: k=%lld too large", (long long)k);
    MDX_CHECK_ARG(nq * ceil_div(n, 4096) < (1ll << 31), "mdx_diffusion_truncated: nq=%lld too large for n=%lld (split the queries)",
                  (long long)nq, (long long)n);
    MDX_CHECK_ARG(ld_scores >= n && ld_out >= n, "mdx_diffusion_truncated: ld_scores=%lld ld_out=%lld must be >= n=%lld",
                  (long long)ld_scores, (long long)ld_out, (long long)n);
    MDX_CHECK_ARG(isfinite(gamma) && gamma >= 0.0f, "mdx_diffusion_truncated: gamma=%g must be finite and >= 0", (double)gamma);
    MDX_CHECK_ARG(alpha >= 0.0f && alpha < 1.0f, "mdx_diffusion_truncated: alpha=%g must be in [0, 1)", (double)alpha);
    MDX_CHECK_ARG(iters >= 1, "mdx_diffusion_truncated: iters=%lld must be >= 1", (long long)iters);
    MDX_CHECK_ARG(isfinite(tol) && tol >= 0.0f, "mdx_diffusion_truncated: tol=%g must be finite and >= 0", (double)tol);
    const int64_t span = ((nq - 1) * ld_out + n) * (int64_t)sizeof(float);
    MDX_CHECK_ARG((out == scores && ld_out == ld_scores) ||
                      !overlaps(out, span, scores, ((nq - 1) * ld_scores + n) * (int64_t)sizeof(float)),
                  "mdx_diffusion_truncated: out overlaps scores (only out == scores with the same stride is allowed)");
    const int64_t need = mdx_diffusion_truncated_workspace(n, k, nq, r);
    MDX_CHECK_WORKSPACE("mdx_diffusion_truncated", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int64_t lds = trd_lds(r);
    auto solve = diffusion_truncated_solve_kernel;
    MDX_HIP(hipFuncSetAttribute((const void *)solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)trd_lds(MDX_DIFFUSION_MAX_R)));
    hipLaunchKernelGGL(solve, dim3((unsigned)nq), dim3(TRD_THREADS), (unsigned)lds, s, cols, w, counts, n, k, top_ids, top_sims,
                       (int)r, kq, gamma, alpha, iters, tol * tol, (char *)workspace, residual, steps);
    MDX_LAUNCH_CHECK();
    const int64_t nblk = ceil_div(n, 4096);
    const bool vec = (((uintptr_t)scores | (uintptr_t)out) & 15) == 0 && ld_scores % 4 == 0 && ld_out % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(diffusion_truncated_base_kernel<true>, dim3((unsigned)(nq * nblk)), dim3(256), 0, s, scores, ld_scores,
                           out, ld_out, n, nblk);
    else
        hipLaunchKernelGGL(diffusion_truncated_base_kernel<false>, dim3((unsigned)(nq * nblk)), dim3(256), 0, s, scores,
                           ld_scores, out, ld_out, n, nblk);
    MDX_LAUNCH_CHECK();
    hipLaunchKernelGGL(diffusion_truncated_scatter_kernel, dim3((unsigned)ceil_div(nq * r, 256)), dim3(256), 0, s,
                       (const char *)workspace, k, r, top_ids, n, nq, out, ld_out);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
