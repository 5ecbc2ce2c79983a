/* mdx_photometric.h -- histogram matching and gamma equalisation of the Lab lightness, fused with the input conversion.  Included
 * by mdx.h (section "photometric normalisation"); include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the
 * reason given there under "exact kNN join" for mdx_knn_join.h: tests/test_cabi.py and tests/test_memguard_host.py pin the prototypes
 * of mdx.h itself and their number.  Their names are in _lib.PHOTOMETRIC_EXPORTS, their census is tests/test_photometric_host.py.
 *
 * Both conversions take uint8 RGB images [B,H,W,3] and write normalised fp32 [B,3,H,W]: the scenarios' chains
 *     pil2np | match_histogram:<eq or a name>[:lab] | totensor | normalize
 *     pil2np | gamma_equalize:<target>[:lab]        | totensor | normalize
 * of mdir/components/data/transform/photometric_transforms.py:50-97 -> functional.py:55-102.  RGB -> Lab and Lab -> RGB are the
 * device code of mdx_clahe_u8_to_chw (csrc/mdx_lab.h; PARITY UNPINNED against OpenCV, as there); what lies between them is numpy
 * and scipy arithmetic and is restated to the bit where that is possible.  Statistics are per image.
 *
 * Lightness: x = L / 100 as float32, the float32 steps of rgb2normspace; the chroma takes the round trip of mdx_clahe_u8_to_chw.
 *
 * Tables (mdx_photometric_tables, host only, no GPU needed; the device code calls the same inline functions):
 *     edges   [257] = np.linspace(-0.00196078431372549, 1.0019607843137255, 257):  k * step + start, the last one the end point
 *     centres [256] = np.linspace(0, 1, 256):                                      k * (1 / 255),    the last one 1
 *
 * Histogram matching (functional.channel_histogram_matching), everything after the lightness plane in float64, no contraction:
 *     bin      k with edges[k] <= x < edges[k + 1] compared in float64, the last bin closed on the right (np.histogram)
 *     cdf0[k]  = (double)(count[0] + ... + count[k]) / (double)(H * W)
 *     fp[k]    = cdf0[k] * centres[255]                      target_cdf == NULL, the reference's "eq"
 *              = interp(cdf0[k], target_cdf, centres)        target_cdf: DEVICE pointer to 256 float64, non-decreasing, finite
 *                                                            (the reference's np.cumsum of a histogram, unnormalised; equal
 *                                                            neighbours are legal)
 *     x'       = (float) interp((double)x, centres, fp)
 *     interp(x, xp, fp): x < xp[0] -> fp[0]; x >= xp[255] -> fp[255]; otherwise, with j the last index with xp[j] <= x,
 *              (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j]: a division, a product and a sum, each rounded on its
 *              own -- np.interp's rule and bits.
 * Gamma equalisation (functional.channel_gamma_matching): per image the gamma with mean(x^gamma) = target, by the secant iteration
 * scipy.optimize.newton runs without a derivative: p0 = log(target) / log(mean(x)), p1 = p0 * (1 + 1e-4) +- 1e-4, the pair ordered
 * by |f|, at most 50 steps, stop when |p - p1| <= 1e-4 (or f(p1) == f(p0) with p1 == p0: their midpoint).  When the iteration does
 * not stop that way, or p0 or a step is not finite: gamma = 0.1 or 10, whichever has the smaller |mean(x^gamma) - target| (10 on a
 * tie).  Then gamma is clipped to [0.1, 10] and x' = (float) pow((double)x, gamma).  The means are float64 sums in a fixed order
 * (per thread, then a fixed tree: the same bits every call) over float32 sums of four neighbouring pixels; inside the iteration
 * x^gamma is exp2(gamma * log2(x)) in float32 on the log2 the first launch stores, gamma as the sum of two floats, 0^gamma taken as
 * pow defines it -- within 1e-6 of the float64 mean, where the solver's own tolerance is 1e-4.  A plane of zeros or of ones comes
 * back as it was; nothing in the output is NaN or Inf.
 *
 * Launches: histogram matching one memset node (the counters) and two kernels, gamma three kernels; their number depends on the
 * shape alone.  No host synchronisation, no allocation, no host-to-device copy: both are legal under stream capture.  The integer
 * histogram is the only atomic; the result does not depend on the order in which workgroups arrive.
 *   stats   RGB -> Lab once per pixel: x [B,H,W] fp32 and the chroma to the workspace; histogram matching: 256 bins in LDS per
 *           workgroup, merged into counts [B,256]; gamma: log2(x)
 *   solve   (gamma) one workgroup per image runs the whole secant iteration over its plane
 *   apply   every workgroup rebuilds fp and its 255 slopes in LDS (or reads gamma); then x -> x', Lab -> RGB, (s - mean) / std;
 *           four pixels per thread when W % 4 == 0 and out is 16-byte aligned
 *
 * workspace: mdx_photometric_workspace(B, H, W) bytes of device scratch, 16-byte aligned, the same for both calls (0 for sizes the
 * calls refuse); with P = round_up(4 * B*H*W, 256), every region at a multiple of 256 bytes and readable by the caller afterwards:
 *     [0, P)              x fp32 [B,H,W]
 *     [P, 2P)             histogram matching: x' fp32 [B,H,W];  gamma: log2(x) fp32 [B,H,W]
 *     [2P, 4P)            chroma (a, b) fp32 [B,H,W,2]
 *     then  1024 * B bytes        counts int32 [B,256]
 *     then  2048 * B bytes        fp float64 [B,256]
 *     then  round_up(8 * B, 256)  gamma float64 [B]
 *     then  round_up(8 * B, 256)  int32 [B,2]: secant steps taken (0: none), and 1 where the fallback decided
 * mean, std: HOST arrays of 3 floats.  out: 4-byte aligned.  MDX_ERR_INVALID, nothing launched, for a NULL rgb, out, mean or std,
 * B, H or W < 1, B >= 65536, H or W >= 2^24, H * W >= 2^31 (the counters are 32-bit), a target_cdf that is not 8-byte aligned, a
 * target outside 0 < target < 1 (NaN included); MDX_ERR_WORKSPACE for a workspace that is NULL or too small. */
#ifndef MDX_PHOTOMETRIC_H
#define MDX_PHOTOMETRIC_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

int64_t mdx_photometric_workspace(int64_t B, int64_t H, int64_t W);
int mdx_photometric_tables(double *edges257, double *centres256);
int mdx_histmatch_u8_to_chw(const uint8_t *rgb, int64_t B, int64_t H, int64_t W, const double *target_cdf, const float *mean,
                            const float *std, void *workspace, int64_t workspace_bytes, float *out, void *stream);
int mdx_gamma_u8_to_chw(const uint8_t *rgb, int64_t B, int64_t H, int64_t W, double target, const float *mean, const float *std,
                        void *workspace, int64_t workspace_bytes, float *out, void *stream);

#endif /* MDX_PHOTOMETRIC_H */
