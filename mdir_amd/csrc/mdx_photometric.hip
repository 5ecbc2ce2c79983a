// Histogram matching and gamma equalisation of the Lab lightness on the device, beside CLAHE.
//
// Replaces the `match_histogram` and `gamma_equalize` transforms of the scenarios -- photometric_transforms.py:50-97 ->
// functional.image_histogram_matching / image_gamma_matching (functional.py:55-102): on what `pil2np` makes of the image
//     spc = (cv2.cvtColor(img, COLOR_RGB2LAB) + [0,128,128]) / [100,255,255]
//     spc[:,:,0] = channel_histogram_matching(spc[:,:,0], histogram)      or      channel_gamma_matching(spc[:,:,0], target)
//     img = cv2.cvtColor(spc*[100,255,255] - [0,128,128], COLOR_LAB2RGB)
// followed by `totensor | normalize`.  The colour conversions are mdx_lab.h's (shared with mdx_clahe.hip, PARITY UNPINNED against
// OpenCV); the middle line is numpy / scipy arithmetic (np.histogram, np.cumsum, np.interp; scipy.optimize.newton's secant) and is
// restated here -- in float64 without contraction, so that counts, fp and the mapped lightness can be compared bit for bit.
// include/mdx_photometric.h states the contract, the workspace and the launches:
//   stats   Lab once per pixel: x = L / 100 and the chroma to the workspace; the 256-bin histogram (LDS, then one integer atomic per
//           workgroup and non-empty bin) or log2(x)
//   solve   (gamma) one workgroup per image: the mean, the secant iteration, the fallback, the clip -> gamma
//   apply   fp and its slopes rebuilt in LDS per workgroup (or gamma read), x -> x', Lab -> RGB, normalise
// The launch boundaries are the grid-wide dependencies (every count before any pixel is mapped).
#include "mdx_lab.h"

// np.interp's and scipy's formulas round every operation on its own: no fma anywhere below
#pragma clang fp contract(off)

namespace mdx {

// np.linspace(start, stop, num): arange(num) * ((stop - start) / (num - 1)) + start, the last element set to stop
constexpr double PH_EDGE_START = -0.00196078431372549, PH_EDGE_STOP = 1.0019607843137255;
constexpr double PH_EDGE_STEP = (PH_EDGE_STOP - PH_EDGE_START) / 256.0;
constexpr double PH_CENTRE_STEP = 1.0 / 255.0;

__host__ __device__ __forceinline__ double ph_edge(int k) { return k == 256 ? PH_EDGE_STOP : (double)k * PH_EDGE_STEP + PH_EDGE_START; }
__host__ __device__ __forceinline__ double ph_centre(int k) { return k == 255 ? 1.0 : (double)k * PH_CENTRE_STEP + 0.0; }

// np.histogram(x, edges): k with edges[k] <= x < edges[k + 1] in float64, the last bin closed on the right.  The bins are 1 / 255
// wide and centred on k / 255: the rounded guess is at most one off.  (x = L / 100 lies in [0, 1.0001]: inside the edges; a value
// outside would be counted in the first or the last bin, where np.histogram drops it.)
__device__ __forceinline__ int ph_bin(float x)
{
    const double xd = (double)x;
    int k = (int)(xd * 255.0 + 0.5);
    k = k < 0 ? 0 : (k > 255 ? 255 : k);
    if (xd < ph_edge(k))
        k = k > 0 ? k - 1 : 0;
    else if (k < 255 && xd >= ph_edge(k + 1))
        k = k + 1;
    return k;
}

constexpr int PH_THREADS = 256;
constexpr int PH_STATS_PIXELS = 16 * PH_THREADS;        // per workgroup of the stats kernel
constexpr int PH_APPLY_ROUNDS = 4;                      // a workgroup of the apply kernel finishes 4 * 256 * VEC pixels
constexpr int PH_SOLVE_THREADS = 1024;

// one pass over the pixels: Lab, x and chroma to the workspace; GAMMA: log2(x) beside them, otherwise the histogram
template <bool GAMMA>
__global__ __launch_bounds__(PH_THREADS) void photometric_stats_kernel(const uint8_t *__restrict__ rgb, int64_t hw, float *__restrict__ xs,
                                                                       float *__restrict__ log2x, float2 *__restrict__ ab,
                                                                       int *__restrict__ counts)
{
    __shared__ float lin[256];
    __shared__ int hist[256];
    const int tid = threadIdx.x, img = blockIdx.y;
    lin[tid] = srgb_to_linear((float)tid / 255.0f);
    hist[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)img * hw, start = (int64_t)blockIdx.x * PH_STATS_PIXELS;
    for (int k = 0; k < PH_STATS_PIXELS / PH_THREADS; ++k) {
        const int64_t i = start + (int64_t)k * PH_THREADS + tid;
        if (i >= hw) break;
        const int64_t pix = base + i;
        const Lab v = rgb8_to_lab_lut(lin, rgb[3 * pix], rgb[3 * pix + 1], rgb[3 * pix + 2]);
        const float x = div_(v.L, 100.0f);              // (lab + [0,128,128]) / [100,255,255], lightness
        xs[pix] = x;
        ab[pix] = make_float2(v.a, v.b);
        if constexpr (GAMMA)
            log2x[pix] = log2f(x);                      // -inf for x = 0
        else
            atomicAdd(&hist[ph_bin(x)], 1);
    }
    if constexpr (!GAMMA) {
        __syncthreads();
        const int c = hist[tid];
        if (c != 0) atomicAdd(&counts[img * 256 + tid], c);         // integer: the sum does not depend on the order
    }
}

// sum of one double per thread over the workgroup, in a fixed order (butterfly inside the wave, then the waves in turn): every
// thread gets the same bits, every call the same bits
__device__ __forceinline__ double block_sum_fixed(double v, double *wave_sums)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    const int wave = threadIdx.x / WAVE, nwaves = blockDim.x / WAVE;
    __syncthreads();                                    // the previous call's readers are done
    if (threadIdx.x % WAVE == 0) wave_sums[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nwaves; ++w) s = s + wave_sums[w];
    return s;
}

// mean(x^gamma) over one plane from the stored log2(x): exp2 of the float32 product gamma * log2(x) -- gamma as the sum of two
// floats, so that its own rounding does not shift the function -- x = 0 as pow defines it; four neighbours are summed in float32,
// everything above them in float64 (the conversions to and from float64 run at a quarter of the float32 rate: per pixel they
// would cost more than the exp2).  gamma is finite.
__device__ __forceinline__ float gamma_pow_f32(float l, float g_hi, float g_lo, float zero_pow)
{
    return l == -__builtin_inff() ? zero_pow : __builtin_amdgcn_exp2f(__builtin_fmaf(g_lo, l, g_hi * l));
}

__device__ __forceinline__ double gamma_mean_pow(const float *__restrict__ l2, int64_t hw, double gamma, double *wave_sums)
{
    const float zero_pow = gamma > 0.0 ? 0.0f : (gamma == 0.0 ? 1.0f : __builtin_inff());
    const float g_hi = (float)gamma, g_lo = (float)(gamma - (double)g_hi);
    double acc = 0.0;
    if ((hw & 3) == 0) {                                // every plane then starts at a 16-byte address
        const float4 *l4 = (const float4 *)l2;
        for (int64_t i = threadIdx.x; i < hw / 4; i += PH_SOLVE_THREADS) {
            const float4 l = l4[i];
            const float e01 = gamma_pow_f32(l.x, g_hi, g_lo, zero_pow) + gamma_pow_f32(l.y, g_hi, g_lo, zero_pow);
            const float e23 = gamma_pow_f32(l.z, g_hi, g_lo, zero_pow) + gamma_pow_f32(l.w, g_hi, g_lo, zero_pow);
            acc = acc + (double)(e01 + e23);
        }
    } else {
        for (int64_t i = threadIdx.x; i < hw; i += PH_SOLVE_THREADS) acc = acc + (double)gamma_pow_f32(l2[i], g_hi, g_lo, zero_pow);
    }
    return block_sum_fixed(acc, wave_sums) / (double)hw;
}

// mean(x) over one plane, the same way (it only places the iteration's starting point)
__device__ __forceinline__ double plane_mean(const float *__restrict__ x, int64_t hw, double *wave_sums)
{
    double acc = 0.0;
    if ((hw & 3) == 0) {
        const float4 *x4 = (const float4 *)x;
        for (int64_t i = threadIdx.x; i < hw / 4; i += PH_SOLVE_THREADS) {
            const float4 v = x4[i];
            acc = acc + (double)((v.x + v.y) + (v.z + v.w));
        }
    } else {
        for (int64_t i = threadIdx.x; i < hw; i += PH_SOLVE_THREADS) acc = acc + (double)x[i];
    }
    return block_sum_fixed(acc, wave_sums) / (double)hw;
}

// one workgroup per image: scipy.optimize.newton(func, x0, tol=1e-4, maxiter=50) without a derivative (its secant branch), the
// reference's fallback and clip.  Every thread runs the same scalar steps on the same broadcast sums.
__global__ __launch_bounds__(PH_SOLVE_THREADS) void photometric_gamma_solve_kernel(const float *__restrict__ xs, const float *__restrict__ log2x,
                                                                                  int64_t hw, double target, double *__restrict__ gammas,
                                                                                  int *__restrict__ info)
{
    __shared__ double wave_sums[PH_SOLVE_THREADS / WAVE];
    const int img = blockIdx.x;
    const float *x = xs + (int64_t)img * hw, *l2 = log2x + (int64_t)img * hw;
    const double mean = plane_mean(x, hw, wave_sums);
    constexpr double tol = 1e-4, eps = 1e-4;
    constexpr int maxiter = 50;
    double p0 = log(target) / log(mean), p = 0.0;
    bool solved = false;
    int steps = 0;
    if (isfinite(p0)) {
        double p1 = p0 * (1.0 + eps);
        p1 = p1 + (p1 >= 0.0 ? eps : -eps);
        double q0 = gamma_mean_pow(l2, hw, p0, wave_sums) - target;
        double q1 = gamma_mean_pow(l2, hw, p1, wave_sums) - target;
        if (fabs(q1) < fabs(q0)) {
            double t = p0; p0 = p1; p1 = t;
            t = q0; q0 = q1; q1 = t;
        }
        for (int itr = 0; itr < maxiter; ++itr) {
            steps = itr + 1;
            if (q1 == q0) {
                if (p1 == p0) {                         // "Tolerance of p1 - p0 reached" otherwise: scipy raises, the fallback decides
                    p = (p1 + p0) / 2.0;
                    solved = true;
                }
                break;
            }
            if (fabs(q1) > fabs(q0))
                p = (-q0 / q1 * p1 + p0) / (1.0 - q0 / q1);
            else
                p = (-q1 / q0 * p0 + p1) / (1.0 - q1 / q0);
            if (!isfinite(p)) break;
            if (fabs(p - p1) <= tol) {                  // np.isclose(p, p1, rtol=0, atol=tol)
                solved = true;
                break;
            }
            p0 = p1;
            q0 = q1;
            p1 = p;
            q1 = gamma_mean_pow(l2, hw, p1, wave_sums) - target;
        }
    }
    if (!solved) {                                      // solution = 0.1 if abs(func(0.1)) < abs(func(10)) else 10
        const double f_lo = gamma_mean_pow(l2, hw, 0.1, wave_sums) - target, f_hi = gamma_mean_pow(l2, hw, 10.0, wave_sums) - target;
        p = fabs(f_lo) < fabs(f_hi) ? 0.1 : 10.0;
    }
    p = p < 0.1 ? 0.1 : (p > 10.0 ? 10.0 : p);          // np.clip(solution, 0.1, 10)
    if (threadIdx.x == 0) {
        gammas[img] = p;
        info[2 * img] = steps;
        info[2 * img + 1] = solved ? 0 : 1;
    }
}

// np.interp(v, xp, centres) for one value, xp[256] non-decreasing in LDS
__device__ __forceinline__ double interp_into_centres(double v, const double *xp)
{
    if (v < xp[0]) return ph_centre(0);
    if (v >= xp[255]) return ph_centre(255);
    int lo = 0, hi = 256;                               // the last j with xp[j] <= v: xp[j + 1] > v, so the slope's divisor is > 0
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v >= xp[mid]) lo = mid + 1; else hi = mid;
    }
    const int j = lo - 1;
    if (v == xp[j]) return ph_centre(j);
    const double slope = (ph_centre(j + 1) - ph_centre(j)) / (xp[j + 1] - xp[j]);
    return slope * (v - xp[j]) + ph_centre(j);
}

// np.interp(x, centres, fp) for one value with the slopes precomputed, as numpy precomputes them
__device__ __forceinline__ float interp_from_centres(float x, const double *fp, const double *slope)
{
    const double xd = (double)x;
    if (xd < 0.0) return (float)fp[0];
    if (xd >= 1.0) return (float)fp[255];
    int j = (int)(xd * 255.0);
    j = j > 254 ? 254 : j;
    if (xd < ph_centre(j))
        j = j - 1;                                      // xd >= 0 = centre(0): j stays >= 0
    else if (xd >= ph_centre(j + 1))
        j = j + 1;                                      // xd < 1 = centre(255): j stays <= 254
    const double c = ph_centre(j);
    if (xd == c) return (float)fp[j];
    return (float)(slope[j] * (xd - c) + fp[j]);
}

// VEC = 4: a thread finishes four consecutive pixels (W % 4 == 0, 16-byte loads and stores); VEC = 1: any width.
// GAMMA: x' = pow(x, gamma); otherwise x' = interp(x, centres, fp) with fp from the image's counts (and target_cdf, if any)
template <int VEC, bool GAMMA>
__global__ __launch_bounds__(PH_THREADS) void photometric_apply_kernel(const float *__restrict__ xs, const float2 *__restrict__ ab, int64_t hw,
                                                                       const int *__restrict__ counts, const double *__restrict__ target_cdf,
                                                                       const double *__restrict__ gammas, LabNorm nrm, double *__restrict__ fp_out,
                                                                       float *__restrict__ mapped, float *__restrict__ out)
{
    __shared__ double fp[256];
    __shared__ double slope[256];
    __shared__ double tcdf[256];
    __shared__ int scan[256];
    const int tid = threadIdx.x, img = blockIdx.y;
    double gamma = 1.0;
    if constexpr (GAMMA) {
        gamma = gammas[img];
    } else {
        scan[tid] = counts[img * 256 + tid];
        if (target_cdf) tcdf[tid] = target_cdf[tid];
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {             // inclusive prefix over the 256 bins (Hillis-Steele in LDS: 8 steps)
            const int add = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const double cdf0 = (double)scan[tid] / (double)hw;
        const double f = target_cdf ? interp_into_centres(cdf0, tcdf) : cdf0 * ph_centre(255);
        fp[tid] = f;
        if (blockIdx.x == 0) fp_out[img * 256 + tid] = f;
        __syncthreads();
        if (tid < 255) slope[tid] = (fp[tid + 1] - fp[tid]) / (ph_centre(tid + 1) - ph_centre(tid));
        __syncthreads();
    }
    const int64_t first = (int64_t)blockIdx.x * (PH_APPLY_ROUNDS * PH_THREADS * VEC);
    for (int r = 0; r < PH_APPLY_ROUNDS; ++r) {
        const int64_t i = first + ((int64_t)r * PH_THREADS + tid) * VEC;
        if (i >= hw) break;
        const int64_t pix = (int64_t)img * hw + i;
        float x[VEC], xm[VEC], o[VEC][3];
        float2 chroma[VEC];
        if constexpr (VEC == 4) {
            const float4 x4 = *(const float4 *)(xs + pix);
            const float4 c01 = *(const float4 *)(ab + pix), c23 = *(const float4 *)(ab + pix + 2);
            x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w;
            chroma[0] = make_float2(c01.x, c01.y);
            chroma[1] = make_float2(c01.z, c01.w);
            chroma[2] = make_float2(c23.x, c23.y);
            chroma[3] = make_float2(c23.z, c23.w);
        } else {
            x[0] = xs[pix];
            chroma[0] = ab[pix];
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if constexpr (GAMMA)
                xm[k] = (float)pow((double)x[k], gamma);
            else
                xm[k] = interp_from_centres(x[k], fp, slope);
            lab_finish_pixel(mul_(xm[k], 100.0f), chroma[k], nrm, o[k]);
        }
        if constexpr (VEC == 4) {
            if constexpr (!GAMMA) *(float4 *)(mapped + pix) = make_float4(xm[0], xm[1], xm[2], xm[3]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *(float4 *)(out + ((int64_t)img * 3 + ch) * hw + i) = make_float4(o[0][ch], o[1][ch], o[2][ch], o[3][ch]);
        } else {
            if constexpr (!GAMMA) mapped[pix] = xm[0];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[((int64_t)img * 3 + ch) * hw + i] = o[0][ch];
        }
    }
}

struct PhotometricWorkspace {
    float *x, *aux;
    float2 *ab;
    int *counts;
    double *fp, *gammas;
    int *info;
};

static int64_t photometric_plane_bytes(int64_t B, int64_t H, int64_t W) { return round_up(4 * B * H * W, 256); }

static bool photometric_sizes_ok(int64_t B, int64_t H, int64_t W)
{
    return B > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24) && B < 65536 && H * W < ((int64_t)1 << 31);
}

static PhotometricWorkspace photometric_carve(void *workspace, int64_t B, int64_t H, int64_t W)
{
    const int64_t plane = photometric_plane_bytes(B, H, W);
    uint8_t *p = (uint8_t *)workspace;
    PhotometricWorkspace w;
    w.x = (float *)p;
    w.aux = (float *)(p + plane);
    w.ab = (float2 *)(p + 2 * plane);
    w.counts = (int *)(p + 4 * plane);
    w.fp = (double *)(p + 4 * plane + 1024 * B);
    w.gammas = (double *)(p + 4 * plane + 3072 * B);
    w.info = (int *)(p + 4 * plane + 3072 * B + round_up(8 * B, 256));
    return w;
}

template <bool GAMMA>
static void photometric_launch_apply(const PhotometricWorkspace &w, int64_t B, int64_t H, int64_t W, const double *target_cdf, const float *mean,
                                     const float *std, float *out, hipStream_t s)
{
    LabNorm nrm;
    for (int c = 0; c < 3; ++c) {
        nrm.mean[c] = mean[c];
        nrm.std[c] = std[c];
    }
    const int64_t hw = H * W;
    // four pixels per thread where every row (and with it every plane: H * W, the workspace regions' 256-byte starts, the
    // caller's `out`) keeps 16-byte alignment
    if (W % 4 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL((photometric_apply_kernel<4, GAMMA>), dim3((unsigned)ceil_div(hw, PH_APPLY_ROUNDS * PH_THREADS * 4), (unsigned)B),
                           dim3(PH_THREADS), 0, s, (const float *)w.x, (const float2 *)w.ab, hw, (const int *)w.counts, target_cdf,
                           (const double *)w.gammas, nrm, w.fp, w.aux, out);
    else
        hipLaunchKernelGGL((photometric_apply_kernel<1, GAMMA>), dim3((unsigned)ceil_div(hw, PH_APPLY_ROUNDS * PH_THREADS), (unsigned)B),
                           dim3(PH_THREADS), 0, s, (const float *)w.x, (const float2 *)w.ab, hw, (const int *)w.counts, target_cdf,
                           (const double *)w.gammas, nrm, w.fp, w.aux, out);
}

}  // namespace mdx

using namespace mdx;

extern "C" {

int64_t mdx_photometric_workspace(int64_t B, int64_t H, int64_t W)
{
    if (!photometric_sizes_ok(B, H, W)) return 0;
    // x, x' or log2(x), chroma (two planes); counts int32 [B,256]; fp float64 [B,256]; gamma float64 [B]; solver info int32 [B,2]
    return 4 * photometric_plane_bytes(B, H, W) + 1024 * B + 2048 * B + 2 * round_up(8 * B, 256);
}

int mdx_photometric_tables(double *edges257, double *centres256)
{
    MDX_CHECK_ARG(edges257 && centres256, "mdx_photometric_tables: NULL pointer");
    for (int k = 0; k <= 256; ++k) edges257[k] = ph_edge(k);
    for (int k = 0; k < 256; ++k) centres256[k] = ph_centre(k);
    return MDX_OK;
}

int mdx_histmatch_u8_to_chw(const uint8_t *rgb, int64_t B, int64_t H, int64_t W, const double *target_cdf, const float *mean,
                            const float *std, void *workspace, int64_t workspace_bytes, float *out, void *stream)
{
    MDX_CHECK_ARG(rgb && out && mean && std, "mdx_histmatch_u8_to_chw: NULL pointer");
    MDX_CHECK_ARG(photometric_sizes_ok(B, H, W), "mdx_histmatch_u8_to_chw: bad sizes");
    MDX_CHECK_ARG(((uintptr_t)target_cdf & 7) == 0, "mdx_histmatch_u8_to_chw: target_cdf must be 8-byte aligned");
    const int64_t need = mdx_photometric_workspace(B, H, W);
    MDX_CHECK_WORKSPACE("mdx_histmatch_u8_to_chw", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const PhotometricWorkspace w = photometric_carve(workspace, B, H, W);
    const int64_t hw = H * W;
    MDX_HIP(hipMemsetAsync(w.counts, 0, (size_t)(1024 * B), s));       // in-stream, on every call: a memset node under capture
    hipLaunchKernelGGL(photometric_stats_kernel<false>, dim3((unsigned)ceil_div(hw, PH_STATS_PIXELS), (unsigned)B), dim3(PH_THREADS), 0, s, rgb,
                       hw, w.x, w.aux, w.ab, w.counts);
    photometric_launch_apply<false>(w, B, H, W, target_cdf, mean, std, out, s);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

int mdx_gamma_u8_to_chw(const uint8_t *rgb, int64_t B, int64_t H, int64_t W, double target, const float *mean, const float *std,
                        void *workspace, int64_t workspace_bytes, float *out, void *stream)
{
    MDX_CHECK_ARG(rgb && out && mean && std, "mdx_gamma_u8_to_chw: NULL pointer");
    MDX_CHECK_ARG(photometric_sizes_ok(B, H, W), "mdx_gamma_u8_to_chw: bad sizes");
    MDX_CHECK_ARG(target > 0.0 && target < 1.0, "mdx_gamma_u8_to_chw: target=%g must satisfy 0 < target < 1", target);
    const int64_t need = mdx_photometric_workspace(B, H, W);
    MDX_CHECK_WORKSPACE("mdx_gamma_u8_to_chw", workspace, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const PhotometricWorkspace w = photometric_carve(workspace, B, H, W);
    const int64_t hw = H * W;
    hipLaunchKernelGGL(photometric_stats_kernel<true>, dim3((unsigned)ceil_div(hw, PH_STATS_PIXELS), (unsigned)B), dim3(PH_THREADS), 0, s, rgb,
                       hw, w.x, w.aux, w.ab, w.counts);
    hipLaunchKernelGGL(photometric_gamma_solve_kernel, dim3((unsigned)B), dim3(PH_SOLVE_THREADS), 0, s, (const float *)w.x,
                       (const float *)w.aux, hw, target, w.gammas, w.info);
    photometric_launch_apply<true>(w, B, H, W, nullptr, mean, std, out, s);
    MDX_LAUNCH_CHECK();
    return MDX_OK;
}

}  // extern "C"
