/* mdx_unet.h -- the epilogue of the U-Net generators (mdir_amd/unet.py): conv bias / inference batch-norm and ReLU / LeakyReLU of a
 * convolution output in one pass, written into a channel slice of a wider tensor.  Included by mdx.h (section "U-Net epilogue") after
 * mdx_knn_reverse.h; include mdx.h, not this file.  The prototype is apart from mdx.h's own for the reason given there under "exact kNN
 * join" for mdx_knn_join.h; its name is in _lib.UNET_EXPORTS and its census is tests/test_unet_host.py.
 *
 * What this is for.  A U-Net level ends in `torch.cat([x, y], dim=1)`: both halves of every skip connection are copied once more.
 * Here the producer of x and the producer of y each write their epilogue straight into their half of one [N, 2C, H, W] buffer, so the
 * concatenation is never run; and the activations a U-Net uses (LeakyReLU(0.2) beside ReLU) are ones mdx_bn_act cannot express.
 *
 * Definition.  x fp32 [N, C, HW] contiguous; for every n < N, c < C, p < HW
 *     invstd = var ? 1 / sqrtf(var[c] + eps) : 1
 *     scale  = weight ? invstd * weight[c] : invstd
 *     y      = fmaf(x[n][c][p] - (mean ? mean[c] : 0), scale, bias ? bias[c] : 0)
 *     out[n * out_batch_stride + c * HW + p] = act(y)
 *   in single IEEE fp32 operations -- the first three lines of mdx_bn_act.  Nothing is added afterwards, so a -0 stays -0 (mdx_bn_act
 *   adds the residual or +0): this is oracle_bn_act(add_zero = 0) of oracle/chain.c, and tests/unet_restatement.py in numpy.
 *     act = MDX_ACT_NONE   y
 *     act = MDX_ACT_RELU   y < 0 ? 0 : y               (torch.relu: NaN stays NaN, -0 stays -0)
 *     act = MDX_ACT_LEAKY  y > 0 ? y : y * slope       (torch's leaky_relu: one multiplication, NaN stays NaN)
 *   slope is read for MDX_ACT_LEAKY only and must then be finite.  Every element has one right value.
 * mean / var (both or neither), weight and bias are optional as in mdx_bn_act: device arrays of C floats or NULL.
 *
 * The output.  out_batch_stride >= C * HW (in elements): `out` may be the channel slice [c0, c0 + C) of a contiguous
 *   [N, Ctot, H, W] tensor, the caller passing the slice's base pointer and Ctot * HW.  Within an image only the C * HW elements of
 *   the slice are written; the out_batch_stride - C * HW elements between two images' slices are neither read nor written.
 *   Nothing is read outside the N * C * HW elements of x.
 *   out == x with out_batch_stride == C * HW is the in-place form.  Any other overlap of the bytes
 *   [x, x + N * C * HW) and [out, out + (N - 1) * out_batch_stride + C * HW) is refused (MDX_ERR_ARG).
 * Launch shape (HBM-bound: one read and one write per element).  One workgroup per run of one (image, channel) plane, the per-channel
 *   constants computed once per plane; 16-byte accesses when HW % 4 == 0 and both x and every plane start of out are 16-byte aligned
 *   (out and, for N > 1, out_batch_stride * 4 bytes), the scalar form otherwise; planes beyond 65 535 go to further launches.
 *   Enqueued on `stream`; allocates nothing and reads nothing back (legal under stream capture).
 * Refusals: NULL x or out; N, C or HW not positive; C or HW >= 2^31; eps < 0; mean without var; act outside the three values; a
 *   non-finite slope with MDX_ACT_LEAKY; out_batch_stride < C * HW; N * out_batch_stride above 2^60 elements; the overlap above.
 * Bit for bit in tests/test_gpu_unet_exact.py; the memory contract in tests/test_gpu_unet_memcontract.py. */
#ifndef MDX_UNET_H
#define MDX_UNET_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_ACT_NONE 0
#define MDX_ACT_RELU 1
#define MDX_ACT_LEAKY 2

int mdx_bn_act_into(const float *x, float *out, int64_t N, int64_t C, int64_t HW, int64_t out_batch_stride, const float *mean,
                    const float *var, const float *weight, const float *bias, float eps, int act, float slope, void *stream);

#endif /* MDX_UNET_H */
