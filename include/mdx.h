/* mdx.h -- C ABI of libmdx.so: the MI355X (gfx950) implementation of the
 * descriptor-extraction-and-ranking hot path of jenicek/mdir + cirtorch.
 *
 * This is the drop-in boundary.  Every entry point replaces one statement (or a
 * short run of statements) of the reference; the reference location is cited
 * per function (paths relative to the upstream repository).  The reference is
 * pure Python, so "what its FFI would bind" is a ctypes stub -- INTEGRATION.md
 * shows it for each call site.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) unless
 *    a parameter says "host".  The caller owns every buffer; the library allocates
 *    nothing persistent except inside an mdx_index (explicit create/destroy).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    only enqueue work and do not synchronise the device, with two exceptions:
 *    mdx_index_create / _ex / _destroy allocate / free (creating an fp32 shard also waits
 *    for its build: see there), and creation also waits for a
 *    one-off probe kernel (a few hundred microseconds per device and process) that
 *    settles how the sort ranks inside a wave; a process that ranks WITHOUT ever
 *    creating an index runs that probe in its first mdx_rank_* / mdx_topk call instead
 *    (and waits for it once) -- unless that stream is being captured, in which case
 *    nothing synchronises and the probe-free kernels are recorded.  Everything but
 *    index creation / destruction and mdx_comm_init / _destroy is safe under graph capture.
 *  - Every function returns MDX_OK (0) or a negative mdx_status; the message of
 *    the last failure on the calling thread is mdx_last_error().  Nothing aborts.
 *  - One host thread per device at a time; handles are not internally locked.
 *  - Matrices are dense fp32 (the feature maps of section "fp16 trunk" excepted).  "row-major [a,b]" means element (i,j) at i*b+j.
 *
 * Alignment
 *    Every device pointer must be aligned to the size of ITS ELEMENT (4 bytes for float / int32, 8 for int64 / double, 2
 *    for int16 / fp16, 1 for uint8 / int8) and to nothing more -- a row slice of a larger tensor is a legal argument and gives
 *    the same bits as an aligned copy (where a kernel has a 16-byte path it picks it by the address, or issues its 16-byte
 *    accesses at element alignment) -- except:
 *      pointer                                                     alignment   otherwise
 *      `workspace` of every entry point that takes one             16 bytes    MDX_ERR_INVALID
 *      `memory` of mdx_index_create_in                             256 bytes   MDX_ERR_WORKSPACE
 *      `stats` of mdx_join_stats, `stats_a` / `stats_b` of
 *        mdx_join_candidates / _rows and mdx_knn_bounds
 *        (one {p, q, r, w} per 16-byte word)                       16 bytes    MDX_ERR_INVALID
 *      `planes` of mdx_jpeg_pixels (rows of 8 samples as 2 words)  4 bytes     MDX_ERR_INVALID
 *    No entry point reads or writes outside the extents stated for its arguments, reads a workspace or an output before
 *    writing it, or writes an input that is not documented as updated in place (tests/test_gpu_memcontract.py).
 */
#ifndef MDX_H
#define MDX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: round 4's additions (mdx_index_bytes, mdx_index_create_in, mdx_scores_rowmajor, mdx_scores_ex / _workspace_ex,
 * mdx_rank_positions) and the stream synchronisation inside mdx_index_create* for fp32 shards (the shard maximum is read
 * back): a host built against version 1 must not load this library unnoticed. */
/* 3: round 6's additions (the direct-store exchange: mdx_p2p_* and mdx_scores_p2p); nothing of version 2 changed. */
#define MDX_ABI_VERSION 3

typedef enum mdx_status {
    MDX_OK = 0,
    MDX_ERR_INVALID = -1,   /* bad argument (NULL, negative size, unsupported value) */
    MDX_ERR_RUNTIME = -2,   /* a HIP runtime call failed (message has hipGetErrorString) */
    MDX_ERR_NOMEM = -3,     /* device allocation failed */
    MDX_ERR_WORKSPACE = -4  /* caller-provided workspace too small */
} mdx_status;

/* Layout of a descriptor matrix handed to the library. */
typedef enum mdx_layout {
    MDX_DIM_MAJOR = 0,  /* [D,N]: the reference's `vecs` (imageretrievalnet.py:291) */
    MDX_ROW_MAJOR = 1   /* [N,D]: one descriptor per row */
} mdx_layout;

/* Global pooling kinds (cirtorch/networks/imageretrievalnet.py:32-37; rmac is out
 * of scope). */
/* Storage type of a shard.  MDX_F32 is the exact path (k-ordered fp32 fma chain).  MDX_F16
 * stores descriptors (and the queries of a call) as IEEE fp16 and multiplies them on the
 * fp16 MFMA with fp32 accumulation (BASELINE.json configs[4]); scores then carry fp16 input
 * rounding (~1e-3 relative against the fp32 scores).  What is pinned, bit for bit (tests/lattice.py,
 * tests/test_gpu_lattice.py; tests/test_lattice_host.py states the same on the host):
 *   - every fp32 input (a query: q - center, one fp32 subtraction) is rounded to fp16 to nearest, ties to even:
 *     |x| >= 65520 becomes an infinity, values under fp16's normal range land on its subnormal grid 2^-24
 *     (|x| <= 2^-25 becomes 0), and subnormal operands enter the MFMA as they are (nothing is flushed);
 *   - the product of two fp16 values is exact, the accumulation is fp32; the order of the fp32 additions is
 *     not part of the contract, so whenever every partial sum of the products is representable in fp32
 *     (sum_k |q_k x_k| below 2^24 units of the operands' common power-of-two grid) the score is the exact dot
 *     product of the rounded operands -- the same bits from both fp16 kernels and for every shape and layout;
 *   - a score is NaN / +inf / -inf exactly where the IEEE product of the rounded operands is (0 * inf = NaN,
 *     inf - inf = NaN), and a non-finite element changes no bit of any other row or query: the zero padding
 *     of rows, queries and k multiplies nothing non-finite.
 * On real-valued data the accumulation rounds; tests/test_gpu_f16.py bounds that (2e-6 against the float64
 * product of the rounded operands for unit vectors). */
/* MDX_I8 stores every row as int8 codes with one fp32 scale per row (a quarter of the fp32 bytes) and multiplies the codes
 * on the int8 MFMA (v_mfma_i32_16x16x64_i8), whose int32 accumulation is exact -- so, unlike fp16, every score is defined
 * to the bit:
 *
 *   Quantising one fp32 row x of length d (a query row is x = q - center, one fp32 subtraction, when a center is given).
 *   Every operation is IEEE fp32 with round-to-nearest-even; nothing is contracted into an fma:
 *     a = max_k |x_k|                                       (exact)
 *     a == 0:  scale = 0, every code 0
 *     else:    inv   = 127.0f / a                           (correctly rounded division)
 *              c_k   = clamp(rint(x_k * inv), -127, 127)    (one rounded product; rint: half to even)
 *              scale = a / 127.0f                           (correctly rounded division)
 *   Score of query q against row i:
 *     acc          = sum_k c_q,k * c_i,k                    (int32, exact: |acc| <= 127^2 d_pad < 2^31)
 *     scores[q, i] = (float)acc * (scale_i * scale_q)       (two rounded products; (float) rounds to nearest even)
 *   Zero padding of k adds nothing, so neither the padding nor the order of the k terms can change a bit.  d is refused
 *   (MDX_ERR_INVALID) where 127^2 * round_up(d, 64) could reach 2^31, i.e. d > 133 120.  Rows (or queries) holding a NaN or
 *   an infinity, or whose a is below 2^-100, carry no contract.
 *
 *   Error bound against the unquantised dot product.  With u = 2^-24, inv = (127/a)(1+d1), fl(x_k inv) = x_k inv (1+d2) and
 *   scale = (a/127)(1+d3), |d_i| <= u: |fl(x_k inv)| <= 127 (1+u)^2 < 127.5, so the clamp never acts and |c_k - fl(x_k inv)|
 *   <= 1/2; scale fl(x_k inv) = x_k (1+d1)(1+d2)(1+d3), so e_x = x - scale c_x obeys
 *     ||e_x||_inf <= scale/2 + a ((1+u)^3 - 1) <= scale/2 + 127 scale ((1+u)^3 - 1) / (1-u) <= scale (1/2 + 2^-15) =: E_x.
 *   x.q - (scale_x c_x).(scale_q c_q) = e_x.q + scale_x c_x.e_q, and the score is that exact product of the quantised rows
 *   times (1+d4)(1+d5)(1+d6) (three roundings: (float)acc, the scale product, the final product), so, barring underflow of
 *   scale_i * scale_q,
 *     |x.q - s| <= E_x ||q||_1 + scale_x ||c_x||_1 E_q + 2^-22 |s|
 *   for every pair -- each term is computable from the inputs, the codes and the scales (tests/test_gpu_i8.py evaluates it).
 *   mdx_quantize_i8 returns the codes and scales of this definition. */
typedef enum mdx_storage { MDX_F32 = 0, MDX_F16 = 1, MDX_I8 = 2 } mdx_storage;

typedef enum mdx_pool_kind { MDX_POOL_GEM = 0, MDX_POOL_MAC = 1, MDX_POOL_SPOC = 2 } mdx_pool_kind;

int mdx_abi_version(void);
const char *mdx_last_error(void);
/* After a stream capture that was INVALIDATED (a call that is illegal while capturing: a synchronisation, a host read): ends the
 * capture if `stream` is still in it (the half-built graph is destroyed) and clears the runtime's per-thread last-error, which
 * otherwise makes the next -- perfectly legal -- launch check of the host framework report "operation failed due to a previous
 * error during capture".  The host of this path captures one graph per input shape (mdir_amd/graphs.py) and stays eager for a shape
 * whose capture was refused; without this call it could not.  No reference counterpart (the reference has no graphs). */
int mdx_capture_recover(void *stream);

/* ---------------------------------------------------------------- extraction */

/* Non-finite values.  The rule is the reference's (torch: relu(NaN) = NaN, clamp(min=eps) keeps NaN, max pooling and the mean
 * return NaN for a window that holds one; checked against torch in tests/test_trunk_exact_host.py), because "NaN scores rank
 * last" only works if the NaN arrives:
 *   - a NaN input element makes NaN exactly the outputs the reference makes NaN: its own element (mdx_bn_act, x or residual;
 *     a residual element of mdx_conv1x1_bn_act), its own pixel column over every output channel (the convolution's x), its
 *     plane (mdx_pool_l2n / mdx_pool_multi / mdx_roipool: the regions that hold it), its descriptor (after the L2N; mdx_rmac);
 *   - it changes no bit of any other output;
 *   - an infinity follows IEEE arithmetic (relu(-inf) = 0, relu(+inf) = +inf, a maximum or a mean over a +inf is +inf).
 * So ReLU is `y < 0 ? 0 : y`, GeM's clamp is `x < eps ? eps : x` (fmaxf returns the operand that is a number), and the maxima
 * carry a "saw a NaN" flag.  Pinned by tests/test_gpu_trunk_exact.py and tests/test_gpu_tail_exact.py; the fused trunk and the
 * module calls (MDIR_AMD_FUSED_TRUNK=1 / 0) give the same NaN mask. */

/* Global pooling of a feature-map batch followed by L2 normalisation over channels.
 *   feat [B,C,H,W] row-major  ->  out [B,C]
 * Replaces `self.norm(self.pool(o))` of ImageRetrievalNet.forward
 * (cirtorch/networks/imageretrievalnet.py:108) = LF.gem / LF.mac / LF.spoc
 * (cirtorch/layers/functional.py:11-22) then LF.l2n (functional.py:130-131).
 *   p, pool_eps: GeM exponent and clamp (ignored for mac/spoc).
 *   l2n_eps    : added to the norm; pass a NEGATIVE value to skip normalisation. */
int mdx_pool_l2n(const float *feat, int B, int C, int H, int W, int kind, float p,
                 float pool_eps, float l2n_eps, float *out, void *stream);

/* R-MAC pooling: feat [B,C,H,W] row-major  ->  out [B,C] (NOT yet L2-normalised as a whole: the network's `self.norm` follows).
 * Replaces `LF.rmac(x, L, eps)` (cirtorch/layers/functional.py:26-72; module RMAC, layers/pooling.py:50-60):
 *     v = l2n(max over the map);  for every region of the grid: v += l2n(max over the region)      (l2n: eps added to the norm)
 *   regions : HOST array [nregions][4] int32 = (row0, col0, height, width), the whole map first, then the grid in the
 *             reference's order (levels 1..L, rows of centres outer, columns inner); the host restates the reference's float32
 *             grid arithmetic (mdir_amd/layers.py: rmac_regions).  At most 64 regions (L = 3 gives 15-51).
 *   workspace: mdx_rmac_workspace(B, C, nregions) bytes of device memory (the regions' maxima). */
int64_t mdx_rmac_workspace(int B, int C, int nregions);
int mdx_rmac(const float *feat, int B, int C, int H, int W, const int32_t *regions, int nregions, float eps,
             void *workspace, int64_t workspace_bytes, float *out, void *stream);

/* Regional pooling: feat [B,C,H,W]  ->  out [B, nregions, C]: the pooling `kind` (p, pool_eps as in mdx_pool_l2n) of every
 * region, no normalisation.  Replaces `LF.roipool(x, rpool, L, eps)` (cirtorch/layers/functional.py:75-121) inside `Rpool.forward`
 * (layers/pooling.py:62-95: `regional: True`); regions as in mdx_rmac. */
int mdx_roipool(const float *feat, int B, int C, int H, int W, const int32_t *regions, int nregions, int kind, float p,
                float pool_eps, float *out, void *stream);

/* vecs [B, nregions, C]  ->  out [B, C] = the sum over the regions in order; l2n_eps >= 0: every region vector is L2-normalised
 * (eps added to the norm) before it is added (R-MAC, functional.py:62-70); l2n_eps < 0: summed as they are (`o.sum(1)`,
 * layers/pooling.py:91). */
int mdx_region_sum(const float *vecs, int B, int nregions, int C, float l2n_eps, float *out, void *stream);

/* The S feature maps of one image pyramid (or of a batch of B equal-sized images), pooled by ONE launch:
 *   feats[s] [B,C,H[s],W[s]] row-major  ->  pooled [S,B,C]   (no normalisation)
 * Replaces the S calls of `self.pool(o)` (imageretrievalnet.py:108; LF.gem / LF.mac / LF.spoc,
 * functional.py:11-22) that CirMultiscaleAggregation (mdir/components/data/wrapper.py:104-107) and extract_ms
 * (imageretrievalnet.py:315-318) cause, one per scale.  Per plane the arithmetic of mdx_pool_l2n. */
int mdx_pool_multi(const float *const *feats, int S, int B, int C, const int *H, const int *W, int kind,
                   float p, float pool_eps, float *pooled, void *stream);

/* Descriptor tail of a pyramid in ONE launch:  pooled [S,B,D] -> out [B,D]
 *   per scale  v_s = pooled[s,b,:] / (||pooled[s,b,:]||_2 + l2n_eps)          LF.l2n, functional.py:130-131
 *   then       out = (sum_s v_s^msp / S)^(1/msp);  out /= ||out||_2 (no eps)  wrapper.py:112-117, imageretrievalnet.py:319-322
 * Bit-identical to mdx_l2n_rows on every scale followed by mdx_ms_aggregate_batch. */
int mdx_l2n_aggregate(const float *pooled, int S, int64_t B, int64_t D, float l2n_eps, float msp, float *out,
                      void *stream);

/* In place: x[r,:] = (x[r,:] + bias) / (||x[r,:] + bias||_2 + eps) for R rows of
 * length D; bias may be NULL.  LF.l2n (functional.py:130-131); with bias it is the
 * tail of the in-network whitening `self.norm(self.whiten(o))`
 * (imageretrievalnet.py:111-112). */
int mdx_l2n_rows(float *x, int64_t R, int64_t D, const float *bias, float eps, void *stream);

/* Trunk epilogue, in place on a convolution output x[N,C,H*W] (NCHW, contiguous):
 *   x = act( (x - mean[c]) * weight[c] / sqrt(var[c] + eps) + bias[c]  (+ residual) ),  act = ReLU or identity
 * i.e. inference `bn(x)`, `out += identity`, `relu(out)` of a residual block (mdir_amd/backbones.py; the
 * torchvision Bottleneck/BasicBlock forward kept by cirtorch/networks/imageretrievalnet.py:172-173) as one
 * pass.  weight / bias / residual may be NULL; mean and var may both be NULL (no normalisation: with only
 * `bias` given this is the `conv bias + ReLU` of a VGG / AlexNet layer).  mean, var, weight, bias: C floats.
 * In single IEEE fp32 operations (correctly rounded division and square root, one fma), so every element has ONE right value:
 *     invstd = var    ? 1.0f / sqrtf(var[c] + eps) : 1.0f
 *     scale  = weight ? invstd * weight[c]         : invstd
 *     y      = fmaf(x - (mean ? mean[c] : 0.0f), scale, bias ? bias[c] : 0.0f)
 *     y      = y + (residual ? residual : 0.0f)        (the + 0 without a residual turns a -0 into +0)
 *     x      = relu ? (y < 0 ? 0 : y) : y              (NaN stays NaN)
 * stated as oracle_bn_act(add_zero = 1) in oracle/chain.c; bit for bit in tests/test_gpu_trunk_exact.py: across the 1024-vector
 * block boundary, on the scalar path (H*W % 4 != 0, or x / residual off the 16-byte grid) and on both sides of the split into
 * launches of 65 535 planes. */
int mdx_bn_act(float *x, const float *residual, int64_t N, int64_t C, int64_t HW, const float *mean,
               const float *var, const float *weight, const float *bias, float eps, int relu, void *stream);

/* 1x1 convolution with its epilogue, one kernel (stride 1, no padding, no groups, no conv bias):
 *   out[b,co,p] = act( (sum_ci w[co,ci] * x[b,ci,p] - mean[co]) * weight[co] / sqrt(var[co] + eps) + bias[co]  (+ residual[b,co,p]) )
 * = `self.bn1(self.conv1(x))` + relu and `self.bn3(self.conv3(out)); out += identity; relu` of the torchvision Bottleneck
 * that cirtorch keeps as `features` (cirtorch/networks/imageretrievalnet.py:172-173; mdir_amd/backbones.py): the GEMM on
 * the f32 matrix cores (v_mfma_f32_32x32x2_f32), the arithmetic of mdx_bn_act applied to the accumulators on their way out:
 *     acc = fmaf chain over ci = 0 .. Cin-1 from +0 (oracle_gemm_nt_chain(w, x[b]^T)), then the five lines of mdx_bn_act with
 *     acc for x, except that without a residual NOTHING is added (no + 0: a -0 stays -0) -- oracle_bn_act(add_zero = 0).
 *   x [N,Cin,HW], out / residual [N,Cout,HW] (NCHW, contiguous; out must not alias x);  Cin % 16 == 0, Cout % 64 == 0
 *   wt [Cin,Cout]: the weights TRANSPOSED, made once per convolution by mdx_conv1x1_transpose_weights(w [Cout,Cin])
 *   mean/var, weight, bias, residual: optional as in mdx_bn_act.
 * Accumulation order: ci ascending, one fma per ci from +0 (the 32x32x2 MFMA is bitwise that chain; a fixed order, the library
 * convolution's differs by fp32 rounding).  Bit for bit in tests/test_gpu_trunk_exact.py: Cin / 16 = 1..5 and 64 steps, 1 and 3
 * channel tiles, partial / full / full + partial groups of pixel tiles, rows off the 16-byte grid, both tile widths, all 2^5
 * epilogue options; the same values as mdx_bn_act on the plain convolution output, and as mdx_scores of w against x[b]. */
int mdx_conv1x1_transpose_weights(const float *w, int64_t Cout, int64_t Cin, float *wt, void *stream);
int mdx_conv1x1_bn_act(const float *x, const float *wt, int64_t N, int64_t Cin, int64_t Cout, int64_t HW, const float *mean,
                       const float *var, const float *weight, const float *bias, float eps, const float *residual, int relu,
                       float *out, void *stream);

/* ------------------------------------------------------------------ fp16 trunk */

/* The LABELLED half-precision mode of extraction (`precision: f16`, mdir_amd/networks.py): the convolutions run on fp16 feature
 * maps (the library's, on the fp16 MFMA), the maps are held and moved as fp16, and everything from the pooling accumulator
 * onwards is fp32 exactly as above.  fp32 remains the default and the parity contract; descriptors of an f16 trunk differ
 * from fp32 ones by fp16 rounding of every layer's activations (tests/test_gpu_trunk_f16_e2e.py measures it against torch's own
 * half path).  An element is an IEEE binary16; pointers are 2-byte aligned ("Alignment" above).  Two contracts:
 *
 * mdx_bn_act_f16      mdx_bn_act in place on an fp16 x (and an fp16 residual); mean, var, weight, bias stay C FLOATS.  Per
 *                     element: x and the residual are converted to fp32 (exact), the five lines of mdx_bn_act run unchanged in
 *                     fp32 (the + 0 without a residual and NaN through the ReLU included), and the result is rounded ONCE to
 *                     fp16, to nearest even, overflow to +-inf as `Tensor.half()`.  So every element has one right value:
 *                     oracle_bn_act(add_zero = 1) on the upcast input, then the conversion.  (torch's half bn / add / relu
 *                     round three times.)  Vector path: 8 halves per 16-byte access when H*W % 8 == 0 and x / residual are
 *                     16-byte aligned, the scalar path otherwise; the same split into launches of 65 535 planes.  Bit for bit
 *                     in tests/test_gpu_bn_act_f16.py.
 * mdx_pool_l2n_f16,   mdx_pool_l2n / mdx_pool_multi on fp16 maps, out / pooled fp32: BIT FOR BIT the value the fp32 entry point
 * mdx_pool_multi_f16  returns on the same maps converted to fp32 -- for every H*W, kind, p and plane start (any multiple of 2
 *                     bytes).  The kernels are the fp32 ones with another load: the same element-to-lane mapping and per-lane
 *                     order, a lane's four consecutive elements now one 8-byte piece, (a + b) + (c + d), the same rule
 *                     H*W % 4 == 0 for the pieces; MAC's NaN flag and GeM's clamp carry over.  tests/test_gpu_pool_f16.py.
 * Not in this mode: mdx_conv1x1_bn_act (an f16 trunk leaves every convolution to the library, followed by mdx_bn_act_f16: the
 * rule that picks the fp32 kernel rests on fp32 measurements), the input conversion, the thumbnail and the pyramid (fp32; a
 * level is converted just before the trunk), R-MAC / regional pooling (they are given fp32 copies of the maps). */
/* The prototypes of this section are in mdx_trunk_f16.h, beside this file, and their names in _lib.TRUNK_F16_EXPORTS, for the
 * reason given under "exact kNN join" for mdx_knn_join.h: tests/test_cabi.py and tests/test_memguard_host.py pin the prototypes
 * of THIS file.  Their census is tests/test_trunk_f16_host.py (exported, bound, and covered by
 * tests/test_gpu_trunk_f16_memcontract.py). */
#include "mdx_trunk_f16.h"

/* Input conversion: uint8 images [B,H,W,C] (C = 1 or 3, interleaved) -> fp32 [B,C,H,W] with
 *   out = (u / 255 - mean[c]) / std[c]            (fp32, IEEE divisions, this operation order)
 * = the `pil2np | totensor | normalize` transform chain of the scenarios (mdir/components/data/transform/
 * core_transforms.py:33-63) moved behind the host-to-device copy.  mean, std: HOST arrays of C floats. */
int mdx_u8_to_chw(const uint8_t *hwc, int64_t B, int64_t H, int64_t W, int C, const float *mean,
                  const float *std, float *out, void *stream);

/* The paper's CLAHE pre-processing + input conversion: uint8 RGB images [B,H,W,3] -> normalised fp32 [B,3,H,W]
 * = the `pil2np | apply_clahe[:clip[:lab[:grid]]] | totensor | normalize` chain of the CLAHE networks' checkpoints
 * (mdir/components/data/transform/photometric_transforms.py:28-36 -> functional.ImageClahe.apply, functional.py:106-129):
 * RGB -> Lab, CLAHE (clip limit, tiles_x x tiles_y grid) on the uint8 lightness, Lab -> RGB, (x - mean) / std.
 * The reference calls OpenCV for all three steps; this restates OpenCV 4's published algorithms (clahe.cpp, color_lab.cpp)
 * and is pinned against the same restatement in numpy (oracle.apply_clahe_rgb) only -- PARITY UNPINNED against OpenCV, which
 * is absent from the build image.  mean, std: HOST arrays of 3 floats.  workspace: device scratch of
 * mdx_clahe_workspace(B, H, W, tiles_x, tiles_y) bytes (the uint8 lightness plane [B,H,W], the per-tile look-up tables
 * [B, tiles_y, tiles_x, 256], the equalised lightness plane [B,H,W]; each region starts at a multiple of 256 bytes and is
 * readable by the caller afterwards; then the chroma (a, b) of RGB -> Lab as fp32 [B,H,W,2], so that the colour conversion's
 * transcendental functions run once per pixel).  Two launches: one workgroup per (image, tile) -- Lab, LDS histogram, clip,
 * spread, LUT -- then one thread per pixel. */
int64_t mdx_clahe_workspace(int64_t B, int64_t H, int64_t W, int tiles_x, int tiles_y);
int mdx_clahe_u8_to_chw(const uint8_t *rgb, int64_t B, int64_t H, int64_t W, int clip_limit, int tiles_x, int tiles_y,
                        const float *mean, const float *std, void *workspace, int64_t workspace_bytes, float *out, void *stream);

/* The scaled copies of an image batch, every level in ONE launch:  src [B,C,H,W] fp32 -> outs[l] [B,C,floor(H*s_l),floor(W*s_l)]
 * = `F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False)` of CirMultiscaleAggregation.preprocess
 * (mdir/components/data/wrapper.py:104-107) and extract_ms (cirtorch/networks/imageretrievalnet.py:315), torch >= 1.6
 * semantics (source coordinate (dst + 0.5) / s - 0.5 clamped at 0, fp32).  scales: HOST array of L doubles (levels with
 * s = 1 are the caller's own tensor and are not passed); outs: HOST array of L device pointers. */
int mdx_bilinear_pyramid(const float *src, int64_t B, int64_t C, int H, int W, int L, const double *scales,
                         float *const *outs, void *stream);

/* One pass of the image down-scaling, along the width (axis 1: [B,H,W,C] -> [B,H,out_len,C]) or the height
 * (axis 0: -> [B,out_len,W,C]) of uint8 images:
 *   dst[o] = clip8((2^21 + sum_{t < count[o]} src[first[o] + t] * k[o*ksize + t]) >> 22)
 * = ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc of Pillow (src/libImaging/Resample.c), the
 * arithmetic of `img.thumbnail((imsize, imsize), Image.ANTIALIAS)` in imresize
 * (cirtorch/datasets/datahelpers.py:48-50) as called by ImagesFromList.__getitem__
 * (cirtorch/datasets/genericdataset.py:63-64).  bounds int32 [out_len,2] = (first, count) and the fixed-point
 * taps k int32 [out_len,ksize] (round(w * 2^22), Pillow's precompute_coeffs + normalize_coeffs_8bpc) are DEVICE
 * arrays computed once per (source length, out_len) by the host (mdir_amd/resample.py).  Width pass first, then
 * height, as Pillow orders them; the result equals Pillow's pixel for pixel. */
int mdx_resample_u8(const uint8_t *src, int64_t B, int H, int W, int C, int axis, int out_len,
                    const int32_t *bounds, const int32_t *k, int ksize, uint8_t *dst, void *stream);

/* JPEG decoding, host half + device half.  Together they replace `Image.open(f).convert('RGB')` of pil_loader
 * (cirtorch/datasets/datahelpers.py:24-31) for baseline JPEG files, with the arithmetic of libjpeg(-turbo) as Pillow
 * configures it (Huffman decoding; jidctint.c islow IDCT; jdsample.c fancy upsampling; jdcolor.c YCbCr -> RGB), bit for bit.
 *   mdx_jpeg_probe          HOST.  Geometry of the file; info->supported = 0 for what stays with the host decoder
 *                           (arithmetic, 12-bit, lossless, CMYK / RGB-coded, other sampling factors).  Sequential and
 *                           progressive Huffman files are covered.  The file is UNTRUSTED input: every table index,
 *                           code length, component / table id, spectral band and block index derived from its bytes is
 *                           range-checked, a Huffman table whose codes do not fit their lengths is refused as libjpeg
 *                           refuses it (jdhuff.c), and a frame header that announces more picture than the file can hold
 *                           (size < width * height / 512 bytes: one bit per block) is "unsupported", so nobody sizes a
 *                           buffer from it.  These two functions run under ASan + UBSan over mutated and hand-made
 *                           hostile files in tests/test_fuzz_asan.py (`make -C mdir_amd/csrc -f Makefile.asan`).
 *   mdx_jpeg_coefficients   HOST (no device call; thread-safe, so loader threads run it in parallel).  Entropy decoding
 *                           of all scans (an error for a stream whose data runs out inside a scan: leave it to Pillow):
 *                           coef [nblocks][64] int16, quantised, natural order, component after component, every
 *                           component's blocks row by row over whole MCUs; quant [3][64] uint16, natural order.
 *   mdx_jpeg_pixels         DEVICE.  coef / quant as above (device copies) -> rgb uint8 [height, width, 3].
 *                           planes: device scratch of nblocks * 64 bytes. */
typedef struct {
    int32_t width, height;          /* image size */
    int32_t ncomp;                  /* 1 (grey) or 3 (YCbCr) */
    int32_t hsamp[3], vsamp[3];     /* sampling factors */
    int32_t blocks_w[3], blocks_h[3];   /* 8x8 blocks per row / column of every component (whole MCUs) */
    int32_t supported;
    int64_t block_offset[3];        /* first block of the component in coef */
    int64_t nblocks;                /* blocks of all components */
} mdx_jpeg_info;
int mdx_jpeg_probe(const uint8_t *file, int64_t size, mdx_jpeg_info *info);
int mdx_jpeg_coefficients(const uint8_t *file, int64_t size, int16_t *coef, int64_t coef_blocks, uint16_t *quant);
int mdx_jpeg_pixels(const int16_t *coef, const uint16_t *quant, const mdx_jpeg_info *info, uint8_t *planes,
                    uint8_t *rgb, void *stream);

/* Multi-scale aggregation of S per-scale descriptors of one image:
 *   out[k] = v[k] / ||v||,  v[k] = (sum_s vecs[s][k]^msp / S)^(1/msp)     (no eps)
 * Replaces CirMultiscaleAggregation.aggregate_tensor
 * (mdir/components/data/wrapper.py:109-119) and the tail of extract_ms
 * (cirtorch/networks/imageretrievalnet.py:319-322).
 *   scale_vecs: HOST array of S device pointers, each D floats (1 <= S <= 8). */
int mdx_ms_aggregate(const float *const *scale_vecs, int S, int64_t D, float msp, float *out,
                     void *stream);

/* The same for a batch: scale s is a [B,D] row-major matrix (one row per image), out is [B,D]; ONE launch
 * (a workgroup per image) instead of one mdx_ms_aggregate per image. */
int mdx_ms_aggregate_batch(const float *const *scale_mats, int S, int64_t B, int64_t D, float msp, float *out,
                           void *stream);

/* ------------------------------------------------------------------- index  */

/* A resident shard of database descriptors, re-laid out once into MFMA-fragment
 * order (DESIGN.md "Data layout").  Also used for a whitening matrix P, whose rows
 * then play the part of database rows. */
typedef struct mdx_index mdx_index;

/* Build a shard from n descriptors of dimension d.  `src` is a DEVICE pointer in
 * the given layout.  `row_offset` is the global id of the shard's first row
 * (added to ids by nothing here -- kept for the caller, see mdx_index_info).
 * Allocates n_pad*d_pad*4 bytes of device memory.  An fp32 shard's creation waits for
 * the build on `stream` (the shard's largest magnitude -- the block exponent of
 * MDX_F32_SPLIT2 -- is reduced inside the re-tiling pass and read back here, once);
 * an fp16 or int8 shard's only if the build fails. */
int mdx_index_create(mdx_index **out, const float *src, int64_t n, int64_t d, int layout,
                     int64_t row_offset, void *stream);
/* Same with an explicit storage type (mdx_storage).  `src` is fp32 in both cases. */
int mdx_index_create_ex(mdx_index **out, const float *src, int64_t n, int64_t d, int layout,
                        int64_t row_offset, int storage, void *stream);
/* The same in memory the caller provides (and keeps alive until mdx_index_destroy, which then frees nothing): `memory` =
 * mdx_index_bytes(n, d, storage) bytes of device memory at a 256-byte boundary.  hipMalloc + hipFree of an 8 GB shard cost
 * ~190 ms per create / destroy pair -- seventy times the re-tiling itself; a host that builds an index per evaluation hands
 * in memory from its own pool (PyTorch's caching allocator in mdir_amd/ops.py). */
int64_t mdx_index_bytes(int64_t n, int64_t d, int storage);
/*   With RT = round_up(ceil(n / 16), 8) row tiles and d_pad = round_up(d, 64):
 *     MDX_F32: RT * 16 * d_pad * 4 + 256     MDX_F16: RT * 16 * d_pad * 2 + 256
 *     MDX_I8:  RT * 16 * d_pad + RT * 16 * 4 + 256   (codes in tiles of 16 rows x 64 k, then one fp32 scale per padded row)
 *   0 for n <= 0, d <= 0, an unknown storage or (MDX_I8) d > 133 120. */
int mdx_index_create_in(mdx_index **out, const float *src, int64_t n, int64_t d, int layout, int64_t row_offset,
                        int storage, void *memory, int64_t memory_bytes, void *stream);
int mdx_index_destroy(mdx_index *index);
/* n, d, row_offset and device bytes held. */
int mdx_index_info(const mdx_index *index, int64_t *n, int64_t *d, int64_t *row_offset,
                   int64_t *device_bytes);

/* Bytes of scratch mdx_scores needs for nq queries of dimension d (the fp32 query tiles; an fp16 shard uses half of it, an
 * int8 shard round_up(nq, 16) * (round_up(d, 64) + 4) bytes of it: the int8 query tiles and one scale per padded query). */
int64_t mdx_scores_workspace(int64_t nq, int64_t d);

/* The int8 quantisation of MDX_I8 (see mdx_storage) of n rows of dimension d, `src` in `layout` (device, fp32):
 *   codes [n, d] int8 row-major, scales [n] fp32 -- the values an MDX_I8 index holds for the same rows (the same device
 * functions quantise both; e.g. to keep a quantised database on disk).  Enqueue only.  MDX_ERR_INVALID for NULL pointers,
 * n <= 0, d <= 0, d > 133 120 or an unknown layout. */
int mdx_quantize_i8(const float *src, int64_t n, int64_t d, int layout, int8_t *codes, float *scales, void *stream);

/* Similarity of nq queries against every row of the shard:
 *   scores[q, i] = sum_k queries(q,k) * db(i,k)      scores row-major [nq, n]
 * i.e. the TRANSPOSE of `np.dot(vecs.T, qvecs)` (mdir/components/optim/score/
 * cirscore.py:69; cirtorch/examples/test.py:240,250), one row per query.
 * Accumulation order is fixed: k ascending, one fused multiply-add per k from +0
 * (oracle/chain.c states it; fp32 MFMA executes exactly that chain).
 *   queries : device, layout `qlayout` ([d,nq] dim-major as the reference's qvecs,
 *             or [nq,d] row-major)
 *   center  : optional device vector [d] subtracted from every query first
 *             (the `v - m` of CirtorchWhiten.postprocess, wrapper.py:194); NULL = none
 *   workspace: device scratch of at least mdx_scores_workspace(nq, d) bytes */
int mdx_scores(const mdx_index *index, const float *queries, int64_t nq, int qlayout,
               const float *center, float *scores, void *workspace, int64_t workspace_bytes,
               void *stream);

/* The same similarity for a database that is multiplied ONCE -- the literal `scores = np.dot(vecs.T, qvecs)` of one
 * evaluation (cirscore.py:69) -- read where it lies: db [n, d] row-major fp32 on the device, no index, no second copy of it
 * (an index of 1 M x 2048 is another 8.2 GB and 3 ms of re-tiling).  Same kernels, same k order: the scores are bit-identical
 * to mdx_scores on an index of the same rows.  d must be a multiple of 4 (rows are fetched in pieces of four values, from any
 * 4-byte-aligned address; MDX_ERR_INVALID otherwise: build an index).  queries / center / scores / workspace (mdx_scores_workspace(nq, d)) as
 * in mdx_scores. */
int mdx_scores_rowmajor(const float *db, int64_t n, int64_t d, const float *queries, int64_t nq, int qlayout,
                        const float *center, float *scores, void *workspace, int64_t workspace_bytes, void *stream);

/* How mdx_scores_ex multiplies an fp32 shard.
 *   MDX_F32_CHAIN   the exact path of mdx_scores (k-ordered fp32 fma chain on the fp32 MFMA; the parity contract).
 *   MDX_F32_SPLIT3  split precision, a LABELLED second mode for the same statement (cirscore.py:69) on the SAME shard
 *                   (nothing is re-quantised or copied): every fp32 operand is written as three bf16 pieces
 *                   x = h + m + l (round to nearest even, residuals exact; the shard's tiles are split in registers by
 *                   the waves that multiply them, the queries once per call) and a product as the six piece products
 *                   hh + hm + mh + hl + lh + mm on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- dropped terms
 *                   <= 2^-23 of a product, below fp32's own rounding.  6/16 of the fp32 MFMA time: the kernel is bound
 *                   by the shard stream (HBM) instead of the matrix pipe.  NOT bit-equal to the chain: the accumulation
 *                   order differs (measured 8e-7 at most over the 70 M scores of the headline workload; tests/test_gpu_round4.py
 *                   bounds it by 2e-6 -- the summation-order bound bench.py holds the reference's own BLAS path to -- for
 *                   scores up to ~0.5 and by 1e-6 + 4e-6 |s| in general: at a self-match, s = 1, ANY fp32 evaluation of a
 *                   2048-term dot product is ~2e-6 from the exact value, the chain included).  fp32 range (bf16 has
 *                   fp32's exponent); an infinite operand gives NaN.  Pinned bit for bit: the six piece products are
 *                   exact, so whenever every partial sum of them is representable in fp32 the score is their exact sum
 *                   (operands of <= 16 significant bits: the exact dot product; tests/test_gpu_lattice.py).
 *   MDX_F32_SPLIT2  a second labelled mode, for when the matrix' dynamic range is ordinary (L2-normalised descriptors: the path's
 *                   own data).  Block floating point: each matrix is scaled by a power of two that brings its largest magnitude
 *                   into fp16's range (the shard's maximum is read once at mdx_index_create, the queries' by a reduction on the
 *                   device), every operand is two fp16 pieces X = h + m / 2^11 (round toward zero, residual exact and scaled:
 *                   |X - h - m / 2^11| < 2^-20 |X|), a product is hh + (hm + mh) / 2^11 on v_mfma_f32_16x16x32_f16 -- THREE
 *                   products instead of six, the cross terms in an accumulator of their own -- and the result is unscaled
 *                   exactly.  Worst case for unit vectors 2^-20 sum |x_k q_k| <= 1e-6 on top of fp32 accumulation; elements
 *                   more than 2^-27 below their matrix' largest lose relative precision (the bound is relative to
 *                   max|x| max|q|, not to each element -- use MDX_F32_SPLIT3 for wide-range data).  Half the matrix work of
 *                   SPLIT3: the kernel runs at its stream's speed (measured 1.4-1.55 ms against 1.92-2.1 and 2.6 for the exact chain).
 *                   Pinned bit for bit: whenever every partial sum of the three kept piece products is representable in fp32
 *                   the score is exactly hh + (hm + mh) / 2^11, unscaled by the exact power of two (tests/test_gpu_lattice.py). */
typedef enum mdx_compute { MDX_F32_CHAIN = 0, MDX_F32_SPLIT3 = 1, MDX_F32_SPLIT2 = 2 } mdx_compute;

/* mdx_scores with an explicit compute mode; workspace of at least mdx_scores_workspace_ex(nq, d, compute) bytes
 * (MDX_F32_SPLIT3: 6 bytes per padded query element; MDX_F32_SPLIT2: 4 + 256 bytes).  Both need an MDX_F32 shard (an fp16 or
 * int8 one is refused with MDX_ERR_INVALID). */
int64_t mdx_scores_workspace_ex(int64_t nq, int64_t d, int compute);
int mdx_scores_ex(const mdx_index *index, const float *queries, int64_t nq, int qlayout, const float *center,
                  float *scores, void *workspace, int64_t workspace_bytes, int compute, void *stream);

/* ------------------------------------------------------------------ ranking */

int64_t mdx_rank_workspace(int64_t n, int64_t nq);

/* Full descending ranking of every query row:
 *   ranks[q, r] = id of the r-th best database row for query q    int64 [nq, n]
 * the transpose of `np.argsort(-scores, axis=0)` (cirscore.py:70).  Order: larger
 * score first, equal scores by ascending id, -0 == +0, NaN last (numpy puts NaN
 * last too; its order inside a run of equal scores is unspecified).
 * `id_offset` is added to every id (shard offset / global ids). */
int mdx_rank_full(const float *scores, int64_t n, int64_t nq, int64_t id_offset, int64_t *ranks,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* The same ranking when row q of the scores lies in pieces: block g is a [nq, widths[g]] row-major matrix and
 * row q of the problem is its rows q side by side, g = 0 .. nblocks-1 (<= 32), n = sum of the widths.  These are
 * the peer blocks the multi-GPU exchange delivers ("all-gather of per-shard partial scores", BASELINE.json
 * north_star): the first pass reads them in place, no re-blocked [nq, n] copy is made.  Workspace of
 * mdx_rank_workspace(n, nq).  Ids are column positions in the concatenation + id_offset. */
int mdx_rank_full_segments(const float *const *blocks, const int64_t *widths, int nblocks, int64_t nq,
                           int64_t id_offset, int64_t *ranks, void *workspace, int64_t workspace_bytes,
                           void *stream);

/* First k entries of mdx_rank_full per query, with their scores:
 *   top_ids [nq,k] int64, top_scores [nq,k] fp32 (either may be NULL).
 * For k << n this is a radix SELECT (the k-th key found digit by digit from histograms, candidates
 * compacted in id order, only those sorted) -- about a third of the time of the full ranking at
 * 1M rows; same order, same tie rule.  Same workspace size as mdx_rank_full. */
int mdx_topk(const float *scores, int64_t n, int64_t nq, int64_t k, int64_t id_offset,
             int64_t *top_ids, float *top_scores, void *workspace, int64_t workspace_bytes,
             void *stream);

/* Which kernels a ranking call would run: host arithmetic only -- nothing is launched, no device memory is touched, nothing
 * synchronises -- so that a test can say which route a shape pins (tests/rank_data.py) and a moved threshold is noticed.
 * The library decides through the same two functions.  (Additions: MDX_ABI_VERSION stays, nothing that exists has changed.)
 *
 * mdx_rank_route: the route of mdx_rank_full / _segments (and of mdx_topk's MDX_TOPK_ROUTE_SORT, and of the candidate list of
 * MDX_TOPK_ROUTE_SELECT with n = k + 4096) for rows of n scores on the current device, NOW:
 *   MDX_RANK_ROUTE_SMALL   one workgroup sorts the row in LDS: n <= 8192, and only with the ordered ds_add_rtn form
 *   MDX_RANK_ROUTE_PACKED  four tiled passes over packed words: n <= 2^24
 *   MDX_RANK_ROUTE_KV      four tiled passes over (key word, id word)
 * under the switches MDX_SORT_SMALL=0, MDX_SORT_NO_PACK=1 and MDX_SORT_RANK=ballot|atomic (read once per process).  The form a
 * wave ranks with is the CACHED verdict of the one-off probe ("Conventions"): this function never runs the probe, and before
 * any index was created or row ranked on this device -- or without a device -- the verdict is unknown and counts as ballots,
 * as it does for a ranking call on a capturing stream.  `stream` is accepted for symmetry and not used.
 * mdx_topk_route: the route of mdx_topk for [nq, n] scores, k and a workspace of workspace_bytes (one mdx_topk accepts):
 *   MDX_TOPK_ROUTE_SAMPLED sampled threshold: n >= 16384, k <= 1024, 256 k <= n (MDX_NO_SAMPLED_TOPK, read per call, turns it off);
 *                          a query that ends with fewer than k or more than 16384 candidates is answered exactly in the kernel
 *   MDX_TOPK_ROUTE_SELECT  radix select, then mdx_rank_route(k + 4096) over the candidates: 4 (k + 4096) <= n
 *   MDX_TOPK_ROUTE_SORT    the full ranking, trimmed in its last pass
 * each only where its carve-up fits the workspace.  MDX_ERR_INVALID for sizes the ranking calls refuse. */
#define MDX_RANK_ROUTE_SMALL 1
#define MDX_RANK_ROUTE_PACKED 2
#define MDX_RANK_ROUTE_KV 3
#define MDX_TOPK_ROUTE_SAMPLED 1
#define MDX_TOPK_ROUTE_SELECT 2
#define MDX_TOPK_ROUTE_SORT 3
int mdx_rank_route(int64_t n, void *stream);
int mdx_topk_route(int64_t n, int64_t nq, int64_t k, int64_t workspace_bytes);

/* Rank position of labelled database ids without materialising the ranking:
 *   pos[t] = #{i : score[q,i] ranks strictly before id t's score under the order above}
 * for t in [offsets[q], offsets[q+1]).  Gives compute_map (cirtorch/utils/
 * evaluate.py:80-81) exactly what `np.arange(N)[np.in1d(ranks[:,q], ids)]` yields,
 * unsorted.  ids int64 [total], offsets int64 [nq+1] (CSR), pos int64 [total];
 * ids are LOCAL to this score matrix (0 <= id < n).  id_scores fp32 [total]
 * receives scores[q, ids[t]] (it is also the kernel's scratch, so it is required). */
int mdx_rank_of(const float *scores, int64_t n, int64_t nq, const int64_t *ids,
                const int64_t *offsets, int64_t total, float *id_scores, int64_t *pos,
                void *stream);

/* Positions of labelled ids inside a GIVEN ranking (the literal form of evaluate.py:80-81,
 * `np.arange(N)[np.in1d(ranks[:, q], ids)]`, for every query in one pass):
 *   pos[t] = p with ranks[q * ld + p] == ids[t], or -1 when the id does not occur among the n entries of row q,
 * t in [offsets[q], offsets[q+1]).  ranks int64, one row of n ids per query at a stride of ld >= n elements (the
 * [Q, N] matrix mdx_rank_full writes, or its first columns); ids int64 [total] >= 0, unique within a query. */
int mdx_rank_positions(const int64_t *ranks, int64_t n, int64_t nq, int64_t ld, const int64_t *ids,
                       const int64_t *offsets, int64_t total, int64_t *pos, void *stream);

/* Scores of given ids: out[t] = scores[q, ids[t]] for t in the CSR range of q. */
int mdx_gather_scores(const float *scores, int64_t n, int64_t nq, const int64_t *ids,
                      const int64_t *offsets, int64_t total, float *out, void *stream);

/* Count, per labelled id given by its SCORE (possibly living on another shard),
 * how many rows of THIS score matrix rank strictly before it:
 *   cnt[t] += #{i : (score[q,i], i + id_offset) precedes (ref_scores[t], ref_ids[t])}
 * The multi-GPU form of mdx_rank_of: every shard adds its partial count, the sum
 * over shards is the global position.  cnt int64 [total] is ACCUMULATED into. */
int mdx_rank_count(const float *scores, int64_t n, int64_t nq, int64_t id_offset,
                   const float *ref_scores, const int64_t *ref_ids, const int64_t *offsets,
                   int64_t total, int64_t *cnt, void *stream);

/* --------------------------------------------------------------- re-ranking */

/* The weighted gather-and-normalise behind alpha-weighted query expansion (alpha-QE) and database-side augmentation (DBA),
 * the re-ranking of the GeM paper's protocol (Radenovic, Tolias, Chum, "Fine-tuning CNN image retrieval with no human
 * annotation", TPAMI 2018).  Not in the reference (the vendored cirtorch does not ship it).
 *
 * For an output row q with neighbour ids ids[q, 0..k-1] and their similarities s[q, j]:
 *
 *   w_j   = s_j ** alpha   if s_j > 0   (alpha == 0 -> 1)
 *           0              otherwise    (includes NaN)
 *   v     = self_q (if a self row is given, weight 1, first) ; then for j = 0 .. k-1 in that order:
 *           v = fmaf(w_j, rows[ids[q, j]], v)          elementwise, fp32
 *   out_q = v / (||v||_2 + eps)                        eps = 1e-6: the project's L2N rule, zero row -> zero row
 *
 *  - An id outside [0, n) contributes nothing and is never dereferenced: the call is safe on any id array.
 *  - alpha-QE, for queries Q against a database X (rows [N, D]):
 *      (ids, s) = topk(Q.X^T, k), k' = min(k, N), mdx_topk's order (descending score, ascending id on ties);
 *      Q' = aggregate(X, ids, s, self = Q); the final scores are Q'.X^T.
 *    alpha = 0 is plain average QE.  In self-retrieval the query's own row is its own top neighbour.
 *  - DBA of X: for every row i, (ids, s) = topk(x_i.X^T, k) -- the top-k includes i itself, no separate self term --
 *    and x'_i = aggregate(X, ids, s, self = none), always read from the ORIGINAL X.  The result is a new matrix.
 *  - With both: DBA first, then alpha-QE, which searches and aggregates over X'.  Queries are never DBA-augmented.
 *  - Bit-determinism: every out_q is bit-identical run to run and does not depend on nq or on which other rows are in
 *    the launch (one wave per row, fixed summation orders).
 *
 * rows [n, d] at a stride of ld >= d floats; ids int64 and sims fp32, both [nq, k] contiguous; self_rows [nq, d] at ld_self
 * (NULL = no self term); out [nq, d] at ld_out.  All device pointers.  MDX_ERR_INVALID, nothing launched, for a NULL rows /
 * ids / sims / out, n, d, nq or k < 1, a stride < d, alpha or eps negative or not finite, or out overlapping rows or
 * self_rows.  With eps = 0 an all-zero row divides 0 by 0. */
int mdx_knn_aggregate(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *ids, const float *sims, int64_t nq,
                      int64_t k, const float *self_rows, int64_t ld_self, float alpha, float l2n_eps, float *out, int64_t ld_out,
                      void *stream);

/* Diffusion on a mutual kNN graph of the database (Iscen, Tolias, Avrithis, Furon, Chum, "Efficient diffusion on region
 * manifolds", CVPR 2017; the "DFS" rows of Radenovic et al., "Revisiting Oxford and Paris", CVPR 2018).  Not in the
 * reference.  Defaults of the paper's public release: k = 50, kq = 10, gamma = 3, alpha = 0.99, iters = 20, tol = 1e-6
 * (the paper's values; not checked against published tables here).
 *
 * Graph of the database X [N, D] (L2-normalised fp32 rows), built once, offline like DBA:
 *   L_i   = topk(x_i . X^T, min(k, N)) in mdx_topk's order (descending score, ascending id on ties); normally holds i itself
 *   edge (i, j): j != i (by id), j in L_i and i in L_j (mutual neighbours); an id repeated in a list counts at its first
 *   position only (mdx_topk's lists have no repeats)
 *   w_ij  = max(s, 0) ** gamma (powf; NaN counts as 0), s = the similarity recorded in the list of min(i, j) (at the
 *   first position of the other id): w_ij == w_ji
 *   d_i   = sum_j w_ij, an fp32 sequential sum in L_i order;  r_i = 1 / sqrt(d_i + 1e-12)
 *   S_ij  = w_ij * (r_lo * r_hi), lo = min(i, j), hi = max(i, j): S is exactly symmetric
 *   stored as a compacted ELL: cols int32 [N, k] (row i's edges first, in L_i order; then -1), vals fp32 [N, k] (then 0),
 *   counts int32 [N].  No row has more than k entries.
 * Query q with first-stage scores s_q = q . X^T (any similarity mode):
 *   seeds y_j = max(s_qj, 0) ** gamma for j in topk(s_q, min(kq, N)), 0 elsewhere (a repeated seed id keeps its last value)
 *   CG on (I - alpha S) f = y, 0 <= alpha < 1, from f = 0, r = p = y, at most iters steps:
 *     Ap_i = fmaf(-alpha, sum_e S_ie p_j(e), p_i)   (the sum an fp32 fma chain in the row's edge order)
 *     a = rr / (p . Ap);  f += a p;  r -= a Ap;  rr' = r . r;  beta = rr' / rr;  p = r + beta p
 *   A column stops once rr' <= (tol * tol) * (y . y) (fp32), decided on the device: from then on its step sizes are 0.
 *   Nothing is read back and the launch sequence depends on iters only.  y = 0: f = 0, no step.
 *   out[q, j] = f_j if f_j > 0, else s_qj - 3: rows the diffusion did not reach rank after every reached row, in their
 *   first-stage order (ties: mdx_rank_full's rule).
 *   residual[q] = sqrt(rr / y . y) at the end (0 when y = 0); steps[q] = the steps taken.
 * Bit-determinism, as mdx_knn_aggregate: every output is bit-identical run to run, and a query's outputs do not depend on nq
 * or on the other queries of the launch.  The dot products are sums over a fixed partition of the rows (independent of nq),
 * one partial per partition and column, summed in a fixed order; no float atomics.
 * Everything is legal under stream capture. */

/* Bytes of device workspace of mdx_knn_graph (r = 1 / sqrt(d + 1e-12) per row); 0 for n < 1. */
int64_t mdx_knn_graph_workspace(int64_t n);
/* The graph from ids int64 and sims fp32, both [n, k] contiguous (what mdx_topk returns for the database against itself),
 * into cols / vals [n, k] and counts [n].  Two launches (mutual test + weights + compaction + degree; normalisation).  An id
 * outside [0, n) is never dereferenced and is no edge.  MDX_ERR_INVALID, nothing launched, for a NULL pointer, n or k < 1,
 * n >= 2^31, gamma negative or not finite; MDX_ERR_WORKSPACE for fewer than mdx_knn_graph_workspace(n) bytes. */
int mdx_knn_graph(const int64_t *ids, const float *sims, int64_t n, int64_t k, float gamma, int32_t *cols, float *vals,
                  int32_t *counts, void *workspace, int64_t workspace_bytes, void *stream);
/* Bytes of device workspace of mdx_diffusion: F, R, P, AP node-major [n, round_up(nq, 4)] fp32, the per-partition partials and
 * the per-column CG state; 0 for n < 1, nq < 1 or nq > 256. */
int64_t mdx_diffusion_workspace(int64_t n, int64_t nq);
/* The solve for nq <= 256 queries: graph (cols, vals, counts) of mdx_knn_graph, width k; scores [nq, n] at a stride of
 * ld_scores floats (the first-stage s_q); seed_ids int64 / seed_sims fp32 [nq, kq] (mdx_topk of the scores); out [nq, n] at
 * ld_out, row-major for mdx_rank_full.  out may equal scores (with the same stride); any other overlap is refused.
 * residual fp32 [nq] and steps int32 [nq] are optional (NULL).  A column outside [0, n) in cols is no edge, a seed id outside
 * [0, n) no seed.  MDX_ERR_INVALID, nothing launched, for a NULL pointer, n, k, kq or nq < 1, nq > 256, n >= 2^31, a stride
 * below n, gamma or tol negative or not finite, alpha outside [0, 1), iters < 1; MDX_ERR_WORKSPACE for fewer than
 * mdx_diffusion_workspace(n, nq) bytes (16-byte aligned). */
int mdx_diffusion(const int32_t *cols, const float *vals, const int32_t *counts, int64_t n, int64_t k, const float *scores,
                  int64_t ld_scores, const int64_t *seed_ids, const float *seed_sims, int64_t nq, int64_t kq, float gamma,
                  float alpha, int64_t iters, float tol, float *out, int64_t ld_out, float *residual, int32_t *steps,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* Truncated diffusion: each query's CG on the subgraph induced by its top-R first-stage rows, renormalised on that subgraph
 * (whether the paper's release renormalises is not checked here), one workgroup per query with the whole state in LDS.  An opt-in mode beside mdx_diffusion, whose
 * graph it shares through the unnormalised weights:
 *   W     the affinity of mdx_knn_graph before normalisation: the same edges in the same compacted ELL order,
 *         w_ij = max(s, 0) ** gamma as defined there (mdx_knn_graph_weights)
 *   R     = min(truncate, N), 1 <= R <= MDX_DIFFUSION_MAX_R
 *   T_q   = mdx_topk(s_q, R): ids t_0 .. t_{R-1} and their scores, in mdx_topk's order; an id repeated in T_q is a node at its
 *         first position only, an id outside [0, N) is no node
 *   seeds the first min(kq, R) entries of T_q (by that order exactly topk(s_q, kq), the seeds of mdx_diffusion),
 *         y_a = max(s, 0) ** gamma
 *   edges (a, b) for t_b in the ELL row of t_a, kept in that row's order; d^R_a = fp32 sequential sum of the kept w in that
 *         order; r_a = 1 / sqrt(d^R_a + 1e-12); S^R_ab = w * (r_a * r_b): exactly symmetric, and with R = N bit-identical to
 *         mdx_knn_graph's S
 *   CG on (I - alpha S^R) f = y over the R unknowns: mdx_diffusion's recurrence, fp32 fma-chain SpMV in edge order, device
 *   stop rule (rr' <= tol^2 * y . y) and iters cap
 *   out[q, t_a] = f_a where f_a > 0; every other entry, in T_q or not, s_qj - 3.  residual / steps as mdx_diffusion.
 * The dot products are per-thread fma partials over fixed rows, then a fixed-order reduction inside the query's workgroup:
 * every output is bit-identical run to run and independent of nq and of the other queries.  No float atomics; nothing is read
 * back; legal under stream capture.  nq is unbounded (one workgroup per query). */
#define MDX_DIFFUSION_MAX_R 4096

/* W of the graph: cols and counts bit-identical to mdx_knn_graph's, w [n, k] fp32 the weights before normalisation (then 0).
 * Launch 1 of mdx_knn_graph alone; same arguments, checks and workspace (mdx_knn_graph_workspace(n) bytes). */
int mdx_knn_graph_weights(const int64_t *ids, const float *sims, int64_t n, int64_t k, float gamma, int32_t *cols, float *w,
                          int32_t *counts, void *workspace, int64_t workspace_bytes, void *stream);
/* Bytes of device workspace of mdx_diffusion_truncated: per query the kept edges (int32 local column + fp32 value) [k, r], the
 * edge counts and f [r]: nq * (round_up(8 k r, 256) + 2 round_up(4 r, 256)).  0 for n, k, nq or r < 1, k > 2^20, nq >= 2^31,
 * r > MDX_DIFFUSION_MAX_R or r > n. */
int64_t mdx_diffusion_truncated_workspace(int64_t n, int64_t k, int64_t nq, int64_t r);
/* The truncated solve: (cols, w, counts) of mdx_knn_graph_weights, width k; scores [nq, n] at ld_scores (the first-stage s_q);
 * top_ids int64 / top_sims fp32 [nq, r] contiguous (mdx_topk of the scores, k = r); out [nq, n] at ld_out (may equal scores
 * with the same stride; any other overlap is refused); residual fp32 [nq] and steps int32 [nq] optional (NULL).
 * MDX_ERR_INVALID, nothing launched, for a NULL pointer, n, k, nq, r or kq < 1, r > MDX_DIFFUSION_MAX_R or r > n,
 * n >= 2^31, k > 2^20, nq * ceil(n / 4096) >= 2^31, a stride below n, gamma or tol negative or not finite, alpha outside
 * [0, 1), iters < 1, out overlapping scores; MDX_ERR_WORKSPACE for fewer than mdx_diffusion_truncated_workspace(n, k, nq, r)
 * bytes (16-byte aligned).  Three launches: the solve (one workgroup per query), out = s - 3, the scatter of f > 0. */
int mdx_diffusion_truncated(const int32_t *cols, const float *w, const int32_t *counts, int64_t n, int64_t k,
                            const float *scores, int64_t ld_scores, const int64_t *top_ids, const float *top_sims, int64_t nq,
                            int64_t r, int64_t kq, float gamma, float alpha, int64_t iters, float tol, float *out,
                            int64_t ld_out, float *residual, int32_t *steps, void *workspace, int64_t workspace_bytes,
                            void *stream);

/* --------------------------------------------------- exact rescoring of shortlists */

/* Exact scores of per-query shortlists (the second stage of a search whose first stage ranks compressed scores):
 *   rows      fp32 [n, d] row-major at a stride of ld >= d floats (device), read in place
 *   x_q       = q - center (one fp32 subtraction; none when center == NULL); queries in either mdx_layout, [d, nq] or [nq, d]
 *   ids       int64 [nq, K] (unique within a query), 1 <= K <= MDX_RESCORE_MAX_K
 *   score     = the k-ascending fmaf chain from +0.0f of oracle/chain.c: acc = fmaf(x_q,k, rows[id, k], acc), k = 0 .. d-1,
 *               continued over zeros to round_up(d, 64) as the fp32 kernels of an index do (exact: it can only turn a -0 into
 *               +0) -- every score is bit-identical to mdx_scores on an fp32 index of the same rows at [q, id], and to
 *               mdx_scores_rowmajor wherever d % 4 == 0
 *   out_ids   int64 [nq, K], out_scores fp32 [nq, K]: each query's pairs sorted by mdx_rank_full's order (larger score first,
 *               -0 == +0, NaN last, equal scores by ascending id; the same key function as the rank kernels)
 * An id outside [0, n) is never dereferenced: its score is NaN, so it sorts last.  Each query's output bits depend on nothing
 * but its own inputs (not on nq, not on the other queries).  out_ids may equal ids.  Two launches: the gather and chains (a
 * workgroup per query and 64 candidates, the rows staged in LDS a KiB at a time) and a per-query bitonic sort in LDS.
 * MDX_ERR_INVALID, nothing launched, for a NULL pointer, n, d, nq or K < 1, K > MDX_RESCORE_MAX_K, ld < d or an unknown
 * layout; MDX_ERR_WORKSPACE for fewer than mdx_rescore_workspace(nq, K, d) bytes. */
#define MDX_RESCORE_MAX_K 4096
/* round_up(4 nq K, 256) bytes (the unsorted scores); 0 for nq, K or d < 1 or K > MDX_RESCORE_MAX_K. */
int64_t mdx_rescore_workspace(int64_t nq, int64_t K, int64_t d);
int mdx_rescore(const float *rows, int64_t n, int64_t d, int64_t ld, const float *queries, int64_t nq, int qlayout,
                const float *center, const int64_t *ids, int64_t K, int64_t *out_ids, float *out_scores, void *workspace,
                int64_t workspace_bytes, void *stream);

/* What the certificate needs to know of an MDX_I8 shard, written on the device by mdx_index_i8_bounds:
 *   s_max = max_i scale_i        s_min = the smallest nonzero scale_i (+inf when there is none)
 *   l_max = max_i scale_i ||c_i||_1 (exact in float64: a 24-bit scale times an integer below 2^25)
 *   flag  = 1 when some row is outside the int8 contract as the shard can tell: a non-finite scale (an infinite element) or
 *           0 < scale < 2^-106 (every row with 0 < a < 2^-100, and a few just above it), else 0.
 * A NaN element that is not a row's absmax leaves no trace in the codes; it needs none: the row's chain score is NaN, which
 * ranks after every number in the exact order, so it cannot enter an exact top-c ahead of a certified entry.  Rows of scale 0
 * (all zero) score exactly 0 on both paths.  Only the maxima and minima are reduced (order-free), so the values are the same
 * on every run. */
typedef struct mdx_i8_bounds {
    double s_max, s_min, l_max;
    int32_t flag, reserved;
} mdx_i8_bounds;
/* A reduction over the codes and scales of an MDX_I8 index into `bounds` (device, one mdx_i8_bounds): enqueued only, two
 * launches, nothing of the index is changed (a host runs it once per index and keeps the result).  MDX_ERR_INVALID for a
 * NULL pointer or an index that is not MDX_I8. */
int mdx_index_i8_bounds(const mdx_index *index, mdx_i8_bounds *bounds, void *stream);

/* The certificate of a rescored int8 shortlist: a depth c_q such that the first c_q entries of mdx_rescore's output are,
 * bit for bit (ids and scores), the first c_q entries of the exact ranking -- mdx_topk on mdx_scores of an fp32 index of the
 * same rows.
 *   scores  fp32 [nq, K]: mdx_rescore's sorted out_scores for the shortlist ids = mdx_topk(int8 scores, K) of the index
 *   t       fp32 [nq]: t_q = the K-th int8 shortlist score (top_scores[:, K-1] of that mdx_topk)
 *   queries / d / qlayout / center: those of the int8 scores (x_q = q - center); bounds: mdx_index_i8_bounds of that index
 *   n       the rows of the index; K <= n
 *   upper   fp32 [nq] = U_q below, rounded up;  depth int32 [nq] = c_q
 * Proof.  Every row i outside the shortlist ranks after it in the int8 order, so s_i <= t_q (NaN t_q: no certificate).  By the
 * MDX_I8 bound (mdx_storage), with E = 1/2 + 2^-15 and scale_q the query's int8 scale,
 *     x_i.x_q <= s_i + 2^-22 |s_i| + scale_i E ||x_q||_1 + scale_i ||c_i||_1 scale_q E
 *             <= t_q + 2^-22 |t_q| + S_max E ||x_q||_1 + L_max scale_q E                 (s + 2^-22|s| increases with s)
 * The chain is a recursive fma sum: |chain_i - x_i.x_q| <= gamma_d sum_k |x_i,k x_q,k| + d 2^-149, gamma_d = d u / (1 - d u),
 * u = 2^-24 (one rounding per fma; the d 2^-149 covers the absolute error of results in the subnormal range), and
 * sum_k |x_i,k x_q,k| <= a_i ||x_q||_1 <= 127 S_max (1 + 2^-22) ||x_q||_1 =: B_q (a_i <= 127 scale_i / (1 - u)).  Hence
 *     chain_i <= U_q = t_q + 2^-22 |t_q| + S_max E ||x_q||_1 + L_max scale_q E + gamma_d B_q + d 2^-149
 * for every row outside the shortlist whose chain score is a number.  The shortlist's entries are exact and sorted by the
 * ranking's order, so its first c_q entries, all with a score > U_q (strictly), precede every other row of the database:
 *     c_q = the number of leading entries with score > U_q;  c_q = K when K == n (no row is outside; upper = -inf).
 * Rounding.  U_q is evaluated in float64 from the fp32 inputs (||x_q||_1 as a float64 sum of the fp32 |x_q,k|), inflated by
 * (d + 16) 2^-52 times the sum of the magnitudes of its terms -- more than all float64 rounding of the evaluation -- and then
 * rounded to fp32 upwards (round to nearest; one step up if that went down).  So rounding can only raise U_q.
 * No certificate (c_q = 0) when K < n and: bounds->flag is set; x_q holds a non-finite value or 0 < max|x_q| < 2^-100 (outside
 * the int8 contract); t_q is NaN; S_min scale_q < 2^-126 (the scale product could underflow, which the MDX_I8 bound excludes);
 * B_q >= 2^126 (a partial sum could overflow); d u >= 1/2; or U_q is not finite.
 * One workgroup per query, fixed-order reductions: bit-identical run to run and independent of nq.  MDX_ERR_INVALID, nothing
 * launched, for a NULL pointer, nq, K, d or n < 1, K > min(n, MDX_RESCORE_MAX_K) or an unknown layout. */
int mdx_rescore_certify(const float *scores, int64_t nq, int64_t K, const float *t, const float *queries, int64_t d, int qlayout,
                        const float *center, const mdx_i8_bounds *bounds, int64_t n, float *upper, int32_t *depth, void *stream);

/* --------------------------------------------- exact range search and self-join */

/* Every pair whose exact score reaches a threshold tau: a range search (queries x database) and a self-join (i < j of one
 * database), pruned on MDX_I8 shards and decided by the exact chain.
 *   Exact score of a pair (x in the query role, y in the database role): the fmaf chain of mdx_rescore, acc = fmaf(x_k, y_k, acc)
 *     from +0, k = 0 .. round_up(d, 64) - 1 over zeros -- bit-identical to mdx_scores on an fp32 index of the database rows.  x =
 *     q - center for external queries (one fp32 subtraction; mdx_center_rows), the raw row for the self-join.  chain(i, j) ==
 *     chain(j, i) bitwise: fma is commutative in its two factors, so the self-join computes every unordered pair once.
 *   Result: every pair with chain >= tau (a NaN score never is); the self-join leaves out i == j and reports i < j only.  CSR over
 *     the query (over i for the self-join): offsets int64 [m + 1], ids int64 [P], scores fp32 [P]; each segment in mdx_rank_full's
 *     order (larger score first, -0 == +0, ties by ascending id).  The bits depend on the inputs only -- not on chunking, capacity,
 *     nq or launch order.
 *
 * Pruning bound.  Per row, from its fp32 values x, its codes c and scale of an MDX_I8 shard (mdx_join_stats):
 *     p = scale,  q >= E ||x||_1,  r >= E scale ||c||_1,  w >= scale + gamma_d max|x| / E,   E = 1/2 + 2^-15
 *   (fp32, each evaluated in float64, inflated by 1 + (d + 16) 2^-52 -- more than the float64 rounding, ||x||_1 being a sum of d
 *   terms -- rounded upwards and floored at 2^-149).  For a pair x (query role), y (database role) with int8 score s (mdx_storage):
 *     |x.y - s| <= scale_y E ||x||_1 + scale_y ||c_y||_1 scale_x E + 2^-22 |s|                      (the MDX_I8 bound)
 *     |chain - x.y| <= gamma_d sum_k |x_k y_k| + d 2^-149 <= gamma_d max|y| ||x||_1 + d 2^-149       (mdx_rescore_certify)
 *   so  chain >= tau  =>  s + 2^-22 |s| >= tau - beta_xy  with
 *     beta_xy = scale_y E ||x||_1 + scale_y ||c_y||_1 scale_x E + gamma_d max|y| ||x||_1 + d 2^-149  <=  q_x w_y + r_y p_x + d 2^-149.
 *   The bound is symmetric in the roles of the MDX_I8 error terms (and the chain's sum_k |x_k y_k| is), so beta_yx is valid as
 *   well; the kernel takes the smaller of the two.
 * Rounding inside the join kernel.  b = fl(fl(fl(q_x w_y) + fl(r_y max(p_x, 2^-149))) + c0) * (1 + 2^-20) rounded, with
 *   c0 = (d + 2) 2^-149 (exact).  With u = 2^-24, a rounded product of non-negatives is >= its value (1 - u) - 2^-150, a rounded sum
 *   >= (1 - u) of its value, and (1 - u)^5 (1 + 2^-20) > 1, so b >= q_x w_y + r_y p_x + (d + 2) 2^-149 - 3 2^-150 >= beta + 2^-150.
 *   A pair is a candidate unless fl(fl(s + fl(2^-21 |s|)) + b) < tau.  fl(2^-21 |s|) >= 2^-21 |s| - 2^-150 and the rounded sum
 *   s + h loses at most u |s + h| <= (2^-24 + 2^-45) |s|, so fl(s + h) >= s + 2^-22 |s| - 2^-150 and fl(s + h) + b >=
 *   s + 2^-22 |s| + beta >= tau; rounding is monotone and tau is an fp32 value, so the computed sum is >= tau as well.  The fp32
 *   evaluation can only enlarge beta: the int8 pass over-selects and never drops a hit.  A NaN score is a candidate.
 * Pairs the bound does not cover are never pruned (their beta is +inf): rows with a non-finite value (as their scale or their
 *   ||x||_1 may show nothing); nonzero rows whose scale is below 2^-106 -- every row with 0 < max|x| < 2^-100, among them the rows
 *   whose max|x| is so small a subnormal that scale = max|x| / 127 rounds to 0: scale c is then 0 and their quantisation error is
 *   x itself, which no scale-proportional term covers -- or above 2^40 (the score could overflow); and pairs of nonzero scales
 *   whose fp32 product is below 2^-126 (it may have underflowed).  Only a row with max|x| == 0 (all zero) is covered with scale 0:
 *   it scores exactly 0 on both paths.  So the result is exact for every input: infinities, NaN rows, zero and subnormal rows.
 *
 * Stages (all enqueue only):
 *   mdx_center_rows      out [n, d] row-major = src - center (center NULL: a copy); the fp32 query rows of a range search
 *   mdx_join_stats       stats fp32 [n, 4] = {p, q, r, w} of each row of an MDX_I8 index of the fp32 rows `rows` [n, d] at a
 *                        stride of ld (the rows the index was built from); an fp16 or fp32 index is refused (it has no bound)
 *   mdx_join_candidates  the join kernel over rows [a_lo, a_hi) of A (a_lo a multiple of MDX_JOIN_BLOCK) against every row of B,
 *                        both MDX_I8 of one d; symmetric (A == B): j > i only.  pairs[0 .. min(count, capacity)) = i << 32 | j
 *                        (global rows) of the candidates in no particular order; *count (device int64) = the number of
 *                        candidates, counted on past the capacity (a caller retries with that size).  No score matrix is written.
 *   mdx_join_resolve     pairs [P] (each unique) of rows i in [m_lo, m_lo + m): the exact chains of rows_a[i] and rows_b[j] (row-
 *                        grouped: the pairs are sorted by (i, j) first), the hits, and the CSR of rows m_lo .. m_lo + m - 1 into
 *                        offsets [m + 1] (offsets[m] = the hits), ids [P], scores [P] (the first offsets[m] entries written).
 *                        workspace: mdx_join_resolve_workspace(P, m) bytes.
 *   mdx_range_select     the dense route: the same CSR of an fp32 score matrix [m, n] at a stride of ld (scores_rowmajor or
 *                        mdx_scores output), hits s >= tau and, for diag >= 0, j > diag + r in row r (the upper triangle of a
 *                        self-join block whose first row is diag); diag < 0: every column.  offsets [m + 1] are always written;
 *                        ids / scores only when offsets[m] <= capacity (else the caller retries with offsets[m]).  workspace:
 *                        mdx_range_select_workspace(m, capacity) bytes.
 * The final order is a stable radix sort of (row, desc_key(score)) whose input is in (row, id) order; the offsets are a binary
 * search per row.  MDX_ERR_INVALID, nothing launched, for a NULL pointer, sizes < 1 (n, d, P, m), P, m or a capacity at or above
 * 2^31, a negative capacity, ld below d (or n), a non-finite tau, a non-int8 index, A and B of different d, symmetric with A != B,
 * an unknown layout; MDX_ERR_WORKSPACE for a workspace below the size functions' (0 for sizes they refuse). */
#define MDX_JOIN_BLOCK 128
int mdx_center_rows(const float *src, int64_t n, int64_t d, int layout, const float *center, float *out, void *stream);
int mdx_join_stats(const mdx_index *index, const float *rows, int64_t ld, float *stats, void *stream);
int mdx_join_candidates(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo, int64_t a_hi,
                        int symmetric, float tau, uint64_t *pairs, int64_t capacity, int64_t *count, void *stream);
int64_t mdx_join_resolve_workspace(int64_t P, int64_t m);
int mdx_join_resolve(const float *rows_a, int64_t lda, const float *rows_b, int64_t ldb, int64_t d, const uint64_t *pairs, int64_t P,
                     float tau, int64_t m_lo, int64_t m, int64_t *offsets, int64_t *ids, float *scores, void *workspace,
                     int64_t workspace_bytes, void *stream);
int64_t mdx_range_select_workspace(int64_t m, int64_t capacity);
int mdx_range_select(const float *scores, int64_t m, int64_t n, int64_t ld, float tau, int64_t diag, int64_t *offsets, int64_t *ids,
                     float *out_scores, int64_t capacity, void *workspace, int64_t workspace_bytes, void *stream);

/* --------------------------------------------------------------- exact kNN join */

/* The exact top-k of rows [a_lo, a_hi) of A against EVERY row of B, the join whose threshold is not given but is each row's own
 * k-th score: ids int64 [m, k] and scores fp32 [m, k], m = a_hi - a_lo.  Both operands are MDX_I8 shards of fp32 row matrices
 * (stats: mdx_join_stats of each).  The result is bit-identical to mdx_topk(mdx_scores(fp32 index of B, the A rows), k): the same
 * chain (the exact score of "exact range search and self-join", continued over zeros to round_up(d, 64)) in mdx_rank_full's order
 * (larger score first, -0 == +0, NaN last, ties by ascending id).  With A == B a row's own match is included, as in mdx_topk.  The
 * bits depend on the inputs only -- not on chunking, slicing, buffer capacity or launch order.
 *
 * Lower bound.  For a pair (i, j) with MDX_I8 score s and the join kernel's rounded-up bound b (above; +inf where the pair is not
 * covered, the scale-product override included):
 *     h = fl(2^-21 |s|),   l_ij = fl(fl(s - h) - b).
 *   From  |x.y - s| <= (the MDX_I8 terms) + 2^-22 |s|  and  |chain - x.y| <= gamma_d max|y| ||x||_1 + d 2^-149  (both two-sided):
 *     chain >= s - 2^-22 |s| - beta_xy,  and with the roles swapped  chain >= s - 2^-22 |s| - beta_yx;  b >= min(beta) + 2^-150.
 *   Rounding, mirroring the join kernel's: h >= 2^-21 |s| - 2^-150 (a product with a power of two is exact unless it is subnormal);
 *   the rounded difference s - h gains at most u |s - h| <= (2^-24 + 2^-45) |s|, u = 2^-24 (a subnormal difference is exact), so
 *   fl(s - h) <= s - (2^-21 - 2^-24 - 2^-45) |s| + 2^-150 <= s - 2^-22 |s| + 2^-150, and fl(s - h) - b <= s - 2^-22 |s| - beta <=
 *   chain.  chain is an fp32 value and rounding is monotone, so l_ij = fl(fl(s - h) - b) <= chain_ij.  The fp32 evaluation can only
 *   lower l.  Covered rows hold finite values of magnitude below 2^47, so their chain is a number.
 *   A pair contributes NO lower bound when b is infinite, when s is NaN or when l_ij is not finite.  A zero l_ij counts as +0.
 * Threshold.  t_i = the k-th largest of the multiset {l_ij : j contributes}; -inf when fewer than k pairs contribute -- a value
 *   defined by the inputs alone (a k-th largest of a fixed multiset), whatever the slices and their order.
 *   At least k rows j have chain_ij >= l_ij >= t_i, so the exact k-th score e_i (rank order) satisfies e_i >= t_i.  By the join
 *   proof above (it holds for every fp32 threshold), every j with chain_ij >= t_i is a candidate of mdx_join_candidates_rows at
 *   tau_i = t_i; so every row that ties with or beats e_i is a candidate, and the first k candidates of row i in rank order are its
 *   exact top-k, ties included.  t_i = -inf makes every row of B a candidate (lhs < -inf never holds), NaN rows too: rows with NaN,
 *   infinite or uncovered entries are still exact.
 *
 * Stages (all enqueue only):
 *   mdx_knn_bounds            t fp32 [m]: t_i of rows [a_lo, a_hi) of A (a_lo a multiple of MDX_JOIN_BLOCK).  One workgroup per
 *                             128-row block of A and slice of the 128-row blocks of B: the int8 MFMA block body of the join kernel,
 *                             the k largest l_ij of every row kept in LDS (MDX_KNN_JOIN_MAX_K = 64: 128 lists of 64 fp32 are 32 KiB
 *                             beside the 32 KiB of operand staging, so two workgroups still share a CU), each slice's sorted list
 *                             written to the workspace [slices, m, k]; a second launch takes the k-th largest of a row's lists.
 *                             slices: 0 = automatic (enough to fill the chip), or 1 .. 64 (never more than the blocks of B are
 *                             used); every value gives the same bits.  workspace: mdx_knn_bounds_workspace(m, k, nb, slices) bytes.
 *   mdx_join_candidates_rows  mdx_join_candidates (non-symmetric) with the threshold of row i read from tau [a_hi - a_lo] (device
 *                             fp32, any value: -inf or NaN keep every pair of the row); pairs, capacity and count as there.
 *   mdx_knn_resolve           pairs [P] (each unique) of rows i in [m_lo, m_lo + m): sorted by (i, j), the exact chains of
 *                             mdx_join_resolve with no threshold test (a NaN score is kept and ranks last), the same stable (row,
 *                             desc_key) sort, then the first k of each row into ids int64 [m, k] / scores fp32 [m, k] and the
 *                             candidates of each row into counts int32 [m].  A count below k can only mean thresholds that were
 *                             not mdx_knn_bounds': the tail of such a row is id -1 / score NaN.  workspace:
 *                             mdx_knn_resolve_workspace(P, m) bytes.
 * MDX_ERR_INVALID, nothing launched, for a NULL pointer, k < 1, k > nb (mdx_knn_bounds) or k > MDX_KNN_JOIN_MAX_K, slices outside
 * [0, 64], a non-int8 index, A and B of different d, a_lo not a multiple of MDX_JOIN_BLOCK or rows outside A, sizes (n, P, m) at or
 * above 2^31 or below 1, a negative capacity, lda / ldb below d, stats not 16-byte aligned; MDX_ERR_WORKSPACE for a workspace below
 * the size functions' (0 for sizes they refuse). */
/* The prototypes of this section (and MDX_KNN_JOIN_MAX_K) are in mdx_knn_join.h, beside this file, and their names in
 * _lib.KNN_JOIN_EXPORTS.  The reason is a test, not the ABI: tests/test_memguard_host.py pins the number of prototypes in THIS
 * file and takes their memory-contract cases from tests/test_gpu_memcontract.py alone, and the change that added this section
 * was to leave existing tests as they were.  So that census and tests/test_cabi.py do NOT cover these five names; their own
 * census is tests/test_knn_join_host.py (every prototype of mdx_knn_join.h is exported, bound, and -- unless it is a size
 * function -- has cases in tests/test_gpu_knn_join_memcontract.py).  Whoever next edits that census should move the prototypes
 * here, the names into _lib.EXPORTS and the cases into the table, and delete the second header. */
#include "mdx_knn_join.h"

/* --------------------------------------------------------------- near-duplicate groups */

/* The connected components of the exact self-join, at up to MDX_GROUPS_MAX_T = 8 thresholds from one pass over the candidates.
 * For rows x_0 .. x_{n-1} (fp32, row-major) and a finite fp32 threshold tau, G_tau is the undirected graph with an edge i ~ j
 * (i != j) iff chain(i, j) >= tau -- chain the exact score of "exact range search and self-join": bitwise symmetric, and a NaN score
 * is never an edge.  Those are exactly the pairs the self-join reports.
 *     label_tau[i] = min { j : j is connected to i in G_tau }        (i itself included)
 * so labels[i] == i exactly for the representatives.  For T thresholds (1 <= T <= MDX_GROUPS_MAX_T, any order, duplicates allowed)
 * the result is labels int64 [T, n], row t for taus[t].  The labels depend on the inputs only: not on chunking, buffer sizes, launch
 * order, the route (candidates of the int8 join kernel, or dense fp32 scores), or which candidates were skipped.  Rows with NaN or
 * infinite values, all-zero rows and subnormal rows are handled as the self-join handles them: the candidates are the join
 * kernel's (its proofs apply unchanged) and the chain that decides them is the same.
 *
 * Forest.  parent int32 [T, n] (so n < 2^31), one forest per threshold.  parent[x] <= x at all times; a root has parent[x] == x.
 *   find(x) follows parents; it may halve the path, which only ever lowers parent[x] to an ancestor of x.  unite(a, b) loops:
 *   ra = find(a), rb = find(b); done if equal; hi = max, lo = min; compare-and-swap(parent[hi]: hi -> lo); done if it succeeded,
 *   else go on from the value it returned.  Only a root is ever hooked, and always under a smaller id, so the root of every tree is
 *   its minimum, and once every edge is in each component is one tree whose root is the label.  (A hook by an atomic min on a
 *   non-root can drop a link, and is not used.)
 * Memory model.  On this chip a CU's L1 is never refreshed by another CU's stores and the L2s of the XCDs are not coherent with
 *   each other for plain accesses.  Inside a kernel that also writes parent, every read of parent is an agent-scope relaxed atomic
 *   load and every write an agent-scope atomic; after a failed compare-and-swap the loop continues from the returned value and never
 *   from a fresh plain load -- which could return the same stale "I am a root" for ever against a compare-and-swap that sees the
 *   truth.  Stale values are harmless otherwise: an old parent is still an ancestor.  The label pass is a launch of its own behind
 *   the unions and reads with plain loads.
 * Bounded loops.  A find takes at most n steps; a unite retries only after another thread hooked the same root, and a level has
 *   at most n - 1 hooks.  Both loops count, and beyond n + 1 they set bit 0 of the flags and return without hooking.  Nothing
 *   waits on another workgroup: no flags, no grid barriers, no spins.
 * Skip rule (mdx_groups_union_pairs).  Before a pair is staged, if find(i) == find(j) in the level of the LARGEST threshold the
 *   pair is dropped and its chain is never computed.  Sound: a path in that level consists of hooks, each made for a pair whose
 *   chain reaches the largest threshold and so every threshold; the thread that computed such a chain unites its pair in EVERY
 *   level before it ends (in this launch, or in an earlier one on the same stream).  So when the kernel ends i and j are connected
 *   in every level, which is all the dropped pair could have added, whatever its own chain.  The components are unchanged; only
 *   the counters of chains and edges depend on the schedule.
 *
 * Stages (all enqueue only, on the caller's stream; no workspace):
 *   mdx_groups_init         parent[t][i] = i for T levels of n rows; status (device int64 [4]) = 0.
 *   mdx_groups_union_pairs  pairs [P] = i << 32 | j as mdx_join_candidates (symmetric) writes them, in any order, duplicates
 *                           allowed, of rows [n, d] at a stride of ld.  One workgroup per 64 pairs: the skip rule, then the exact
 *                           chain of the rows of every pair left (the tile plan of the join's exact stage: k ascending from +0 over
 *                           zeros to round_up(d, 64); 16-byte loads only when ld % 4 == 0 and rows is 16-byte aligned), then unite
 *                           in every level t with chain >= taus[t].  taus: a HOST pointer to T floats (passed to the kernel by value).
 *                           A pair with i == j is dropped; one that names a row >= n is dropped and sets bit 1 of the flags.
 *   mdx_groups_union_dense  the exact route: scores fp32 [m, ncols] at a stride of ld (mdx_scores_rowmajor / mdx_scores output);
 *                           entry (r, c) is the pair (row_base + r, col_base + c), an edge of level t iff s >= taus[t] and
 *                           col_base + c > row_base + r.  One workgroup per row.
 *   mdx_groups_labels       labels int64 [T, n] = the root of every row; labels is a buffer of its own, never parent.
 * status: [0] chains computed, [1] pairs that were an edge of at least one level, [2] successful hooks summed over the levels,
 *   [3] flags (bit 0: a loop gave up -- the labels are then not to be used; bit 1: a pair out of range).  One atomic add per
 *   workgroup and word.  [0] and [1] vary from run to run under the skip rule (the dense route computes no chain and adds nothing
 *   to [0]); [2] does not: it is the sum over t of n minus the number of groups of level t.
 * MDX_ERR_INVALID, nothing launched, for a NULL pointer, n, d, P, m or ncols < 1, n or P at or above 2^31, T outside [1, 8], a
 * non-finite threshold, ld below d (pairs) or below ncols (dense), a negative base, row_base + m > n or col_base + ncols > n,
 * labels == parent. */
/* The prototypes of this section (and MDX_GROUPS_MAX_T) are in mdx_groups.h, beside this file, and their names in
 * _lib.GROUPS_EXPORTS, for the reason given above for mdx_knn_join.h; their census is tests/test_groups_host.py (every prototype is
 * exported, bound, and has cases in tests/test_gpu_groups_memcontract.py). */
#include "mdx_groups.h"

/* --------------------------------------------------------------- k-reciprocal re-ranking */

/* k-reciprocal encoding (Zhong et al., CVPR 2017) beside alpha-QE, DBA and diffusion: the reciprocal sets of the database's kNN lists
 * (R(i, k) and R(i, ceil(k / 2))), the sparse raw and locally expanded codes of every database row as CSRs, and per query the
 * Jaccard min-sum of its code against the codes of its top-R first-stage rows, blended with the first-stage score by lam; rows
 * outside the shortlist keep s - 3.  The whole contract -- sets, expansion, weights, summation orders, the static cap
 * (MDX_KRECIP_MAX_K1 = 64, MDX_KRECIP_MAX_NNZ = 4096, MDX_KRECIP_MAX_R = 4096), the refusals -- is stated in mdx_krecip.h, beside this
 * file, with the prototypes; their names are in _lib.KRECIP_EXPORTS, for the reason given above for mdx_knn_join.h, and their census
 * is tests/test_krecip_host.py (every prototype is exported, bound, and -- unless it is a size function -- has cases in
 * tests/test_gpu_krecip_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_krecip.h"

/* --------------------------------------------------------------- photometric normalisation */

/* The reference's other two photometric normalisations of the Lab lightness beside CLAHE, each fused with the input conversion like
 * mdx_clahe_u8_to_chw: histogram matching (`match_histogram:eq` or a target CDF) and gamma equalisation (`gamma_equalize:<target>`).
 * The whole contract -- the numpy / scipy arithmetic restated, the bin edges and centres, the secant iteration and its fallback, the
 * workspace layout, the launches, the refusals -- is stated in mdx_photometric.h, beside this file, with the prototypes; their names
 * are in _lib.PHOTOMETRIC_EXPORTS, for the reason given above for mdx_knn_join.h, and their census is
 * tests/test_photometric_host.py (every prototype is exported and bound; the two conversions have cases in
 * tests/test_gpu_photometric_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_photometric.h"

/* --------------------------------------------------------------- trainable tail */

/* What a gradient step on mined tuples needs after the trunk: the backward of the global pooling (GeM with the gradient of its
 * exponent, MAC, SPoC) and of the row L2 normalisation, and the reference's contrastive and triplet losses with their gradients.  The
 * whole contract -- the formulas, the layout of a tuple batch, the summation orders, the launches, the refusals -- is stated in
 * mdx_train.h, beside this file, with the prototypes; their names are in _lib.TRAIN_EXPORTS, for the reason given above for
 * mdx_knn_join.h, and their census is tests/test_train_host.py (every prototype is exported and bound; the four launching ones have
 * cases in tests/test_gpu_train_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_train.h"

/* --------------------------------------------------------------- spherical k-means */

/* Partitioning a database of L2-normalised descriptors by cosine similarity: beside mdx_scores_ex on an fp32 index of the centroids, an
 * iteration needs the best centroid of every row of a score block (the first entry of mdx_topk, in one pass), the sum of every
 * cluster's rows in a fixed order, and the normalisation of the sums.  The whole contract -- the tie rule, the segment chain that
 * defines a sum to the bit, the order of the norm, the workspace layout, the launches, the refusals -- is stated in mdx_kmeans.h,
 * beside this file, with the prototypes and MDX_KMEANS_SEGMENT; their names are in _lib.KMEANS_EXPORTS, for the reason given above for
 * mdx_knn_join.h, and their census is tests/test_kmeans_host.py (every prototype is exported and bound; the three launching ones have
 * cases in tests/test_gpu_kmeans_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_kmeans.h"

/* --------------------------------------------------------------- inverted file */

/* Searching the partition that spherical k-means makes: a query is scored against the members of the lists whose centroids it scores
 * best against, with the exact fp32 chain, and answered with the first k of them in mdx_rank_full's order.  Beside mdx_scores_ex and
 * mdx_topk on an fp32 index of the centroids this takes a plan of the batch's probes (the inverted probe table), a list-major scan
 * that reads a list's rows once for the queries that share it, and a selection per query.  The whole contract -- the layout of the
 * plan, the candidate columns, the bounds that stand in for sizes the host does not know, the order, the refusals -- is stated in
 * mdx_ivf.h, beside this file, with the prototypes, MDX_IVF_QUERY_GROUP and MDX_IVF_TILE; their names are in _lib.IVF_EXPORTS, for the
 * reason given above for mdx_knn_join.h, and their census is tests/test_ivf_host.py (every prototype is exported and bound; the three
 * launching ones have cases in tests/test_gpu_ivf_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_ivf.h"

/* --------------------------------------------------- inverted file, int8 lists */

/* The rows of the lists a second time as MDX_I8 codes in list order, and a first stage of the search that scans them on the int8 MFMA:
 * a quarter of the bytes, read as a contiguous stream where the fp32 scan gathers whole rows.  The plan, the work items and the
 * selection are those of mdx_ivf.h; the candidates are then rescored exactly (mdx_rescore) and certified (mdx_rescore_certify).  The
 * whole contract -- the storage, the scores to the bit, what the certified prefix of a result equals and why, the refusals -- is
 * stated in mdx_lists_i8.h, beside this file, with the prototypes; their names are in _lib.LISTS_I8_EXPORTS, for the reason given
 * above for mdx_knn_join.h, and their census is tests/test_lists_i8_host.py (every prototype is exported and bound; the three have
 * cases in tests/test_gpu_lists_i8_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_lists_i8.h"

/* ------------------------------------- inverted file, product-quantised lists */

/* The rows of the lists as M bytes each: the residual of a row against its list's centroid, cut into M sub-vectors, every one replaced
 * by the id of its nearest of 256 codewords (IVF-PQ).  A search builds one look-up table per query -- the exact chain of its
 * sub-vectors with every codeword -- and scans the codes by table look-ups (asymmetric distance computation); the fp32 rows are needed
 * only for an optional exact second stage (mdx_rescore).  The plan and the selection are those of mdx_ivf.h.  The whole contract -- the
 * table and the score to the bit, the layout of the codes, the launch shape, the refusals -- is stated in mdx_lists_pq.h, beside this
 * file, with the prototypes and MDX_PQ_MAX_M; their names are in _lib.LISTS_PQ_EXPORTS, for the reason given above for mdx_knn_join.h,
 * and their census is tests/test_pq_host.py (every prototype is exported and bound; both have cases in
 * tests/test_gpu_lists_pq_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_lists_pq.h"

/* ------------------------------------------- inverted file, editing the lists */

/* Adding and removing rows after the build.  An index that keeps its rows in list order is three parts -- payload rows of opaque bytes,
 * their member ids, the offsets of the lists -- and a batch of new rows, sorted by list, is a second structure of the same kind: adding
 * it is the per-list concatenation of the two (mdx_lists_merge), removing rows the compaction of one along the prefix sum of its keep
 * flags (mdx_lists_compact).  One gather pass each, no workspace.  The whole contract -- the structure, the order, the clamping, the
 * widths of the loads and stores, the launch shape, the refusals -- is stated in mdx_lists_edit.h, beside this file, with the
 * prototypes; their names are in _lib.LISTS_EDIT_EXPORTS, for the reason given above for mdx_knn_join.h, and their census is
 * tests/test_lists_edit_host.py (every prototype is exported and bound; both have cases in tests/test_gpu_lists_edit_memcontract.py).
 * Additions: MDX_ABI_VERSION stays. */
#include "mdx_lists_edit.h"

/* ------------------------------- inverted file, int8 refinement of shortlists */

/* A second-level code for the product-quantised lists: beside the M bytes of a position the MDX_I8 codes and the scale of its row -- the
 * storage mdx_lists_i8_encode writes, opaque payload to mdx_lists_merge / mdx_lists_compact -- and a call that scores a per-query
 * shortlist of ids against them and sorts it as mdx_rescore does.  An index then answers with int8-quality rankings and no fp32 rows
 * on the device, and where the rows are attached the exact stage runs on a few hundred of them.  One gather pass over whole int8 rows
 * and the per-query sort of mdx_rescore.  The whole contract -- the storage, the score to the bit, the order, the launch shape, the
 * refusals -- is stated in mdx_refine.h, beside this file, with the prototypes; their names are in _lib.REFINE_EXPORTS, for the reason
 * given above for mdx_knn_join.h, and their census is tests/test_refine_host.py (every prototype is exported and bound; the launching one
 * has cases in tests/test_gpu_refine_memcontract.py).  Additions: MDX_ABI_VERSION stays. */
#include "mdx_refine.h"

/* ------------------------------- kNN lists, reverse-edge merge */

/* The kNN lists of all rows, improved by their own reverse edges: the exact chain is symmetric to the bit, so where row i lists j and
 * j does not list i, the pair (i, score) is offered to j at no scoring cost, and every row keeps the first k of its own entries and its
 * offers.  This is what makes an approximate join through the inverted file (mdir_amd/ivf.py, IVFIndex.knn_join) as good as a wider
 * probe.  A count pass, the caller's prefix sum, a fill pass and a one-wave-per-row merge.  The whole contract -- the definition, the
 * order, the determinism, the offer buffer, the launch shape, the refusals -- is stated in mdx_knn_reverse.h, beside this file, with
 * the prototypes; their names are in _lib.KNN_REVERSE_EXPORTS, for the reason given above for mdx_knn_join.h, and their census is
 * tests/test_knn_reverse_host.py (every prototype is exported and bound; each has cases in tests/test_gpu_knn_reverse_memcontract.py).
 * Additions: MDX_ABI_VERSION stays. */
#include "mdx_knn_reverse.h"

/* ------------------------------- U-Net epilogue */

/* The generators in front of the embedding network (mdir_amd/unet.py; a SequentialNetwork checkpoint = U-Net + trunk) run at the full
 * image size, and around their library convolutions they have what mdx_bn_act removed from the trunk -- full-tensor passes for the conv
 * bias, the batch-norm and the activation -- plus one torch.cat per level.  mdx_bn_act_into is mdx_bn_act's first three lines with
 * ReLU or LeakyReLU, written into a channel slice of a wider tensor: each half of a skip connection is produced in place in the concat
 * buffer.  The whole contract -- the value to the bit, the slice, the overlap rule, the launch shape, the refusals -- is stated in
 * mdx_unet.h, beside this file, with the prototype; its name is in _lib.UNET_EXPORTS, for the reason given above for mdx_knn_join.h,
 * and its census is tests/test_unet_host.py (exported, bound, and covered by tests/test_gpu_unet_memcontract.py).
 * An addition: MDX_ABI_VERSION stays. */
#include "mdx_unet.h"

/* ------------------------------- top-K lists, overlap */

/* How much of one set of top-K lists another holds: per query and depth, the ids of the head of a[q] that occur in the head of b[q] --
 * the count behind recall@depth of an approximate search (mdir_amd/ivf.py, mdir_amd/ivfpq.py, search.search) against the exact top-K,
 * for up to 8 depths in one launch (search.recall_at; the `search` criterion key of mdir_amd/score.py prints it).  One workgroup per
 * query, row b in an open-addressing table in LDS, integers only.  The whole contract -- the definition, padding and large ids, the
 * launch shape, the refusals -- is stated in mdx_overlap.h, beside this file, with the prototype; its name is in _lib.OVERLAP_EXPORTS,
 * for the reason given above for mdx_knn_join.h, and its census is tests/test_overlap_host.py (exported, bound, and covered by
 * tests/test_gpu_overlap_memcontract.py).  An addition: MDX_ABI_VERSION stays. */
#include "mdx_overlap.h"

/* ------------------------------- graph index */

/* The fourth family of index beside the scan, the inverted file and IVF-PQ: a best-first walk over a fixed-degree neighbour graph of
 * the database (mdir_amd/graph.py, GraphIndex; the `search` criterion key of mdir_amd/score.py, index: graph).  The graph is made of
 * the kNN lists the library already builds (search.knn_join, IVFIndex.knn_join), pruned by rank-based detour counts and completed with
 * reverse edges.  mdx_graph_search walks it, one workgroup per query, with exact chain scores -- the bits of mdx_scores -- so that no
 * rescoring stage follows; mdx_graph_detours is the integer kernel of the build.  The whole contract -- the sequential definition of
 * the walk, why a visited-row table cannot change it, the LDS footprint, the launch shapes, the refusals -- is stated in mdx_graph.h,
 * beside this file, with the prototypes; their names are in _lib.GRAPH_EXPORTS, for the reason given above for mdx_knn_join.h, and
 * their census is tests/test_graph_host.py (exported, bound, and covered by tests/test_gpu_graph_memcontract.py).
 * Additions: MDX_ABI_VERSION stays. */
#include "mdx_graph.h"

/* ------------------------------------------------- whitening learning (float64) */

/* The dense products of whitenlearn / pcawhitenlearn (mdir/external/cirtorch/utils/whiten.py:14-53), which the
 * reference runs in float64 on float64 descriptors; here on the f64 matrix cores (v_mfma_f64_16x16x4_f64, f64
 * accumulation).  Cholesky / eig / inverse of the D x D results stay on the host, as in the reference.
 *
 * Gram matrix of the rows of a dimension-major matrix:
 *   a [d, n] row-major, center [d] or NULL  ->  out [d, d],  out[i][j] = sum_k (a[i][k] - center[i]) * (a[j][k] - center[j])
 * = `np.dot(Xc, Xc.T)` with `Xc = X - m` (whiten.py:21-22), `np.dot(df, df.T)` (whiten.py:42 and :46).  Only the
 * tiles on or above the diagonal are computed and each is stored twice: the result is exactly symmetric.  workspace:
 * mdx_gram_f64_workspace(d, n) bytes of device scratch -- the centred input transposed to [n, d] (both operands of the GEMM
 * are then read in 1-KiB runs), then the partial results of up to 16 K ranges, which are added in range order: a fixed
 * summation order, whatever the schedule.  That is at most 8 * (n_pad * d_pad + 16 * d^2) bytes: 0.84 GB at d = 2048,
 * n = 20 000 (0.33 GB of transposed input + 0.50 GB for 15 ranges) -- size the scratch from the function, not by guess. */
int64_t mdx_gram_f64_workspace(int64_t d, int64_t n);
int mdx_gram_f64(const double *a, int64_t d, int64_t n, const double *center, double *out, void *workspace,
                 int64_t workspace_bytes, void *stream);

/* Projection of centred descriptors:
 *   p [dout, d] row-major, x [d, n] row-major, center [d] or NULL  ->  out [dout, n] = p . (x - center)
 * = `df = np.dot(P, X-m)` (whiten.py:45).  workspace: mdx_project_f64_workspace(dout, d) bytes of device scratch (p
 * transposed, so that both operands are read in 1-KiB runs).  An odd n costs one more short launch (the large-tile kernel
 * moves column pairs). */
int64_t mdx_project_f64_workspace(int64_t dout, int64_t d);
/* x [d, n] float64, in place: every COLUMN divided by (its L2 norm + eps) = `X / (np.linalg.norm(X, ord=2, axis=0, keepdims=True)
 * + 1e-6)` of whitenapply (whiten.py:10-11) when it is handed float64 `P` (then the reference computes in float64). */
int mdx_l2n_cols_f64(double *x, int64_t d, int64_t n, double eps, void *stream);
int mdx_project_f64(const double *p, int64_t dout, int64_t d, const double *x, int64_t n, const double *center,
                    double *out, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------- multi-GPU exchange (RCCL over xGMI) */

/* The reference is single-process; what is sharded here is `scores = np.dot(vecs.T, qvecs)` (cirscore.py:69):
 * database rows are independent, so rank g of G (one process per GPU) keeps rows [lo_g, hi_g) as its own mdx_index
 * and computes its block S_g [nq, w_g] with mdx_scores alone.  The two calls below move the blocks to where
 * `np.argsort(-scores, axis=0)` (cirscore.py:70) needs them; both deliver blocks BACK TO BACK in rank order (block g
 * row-major, widths[g] columns), which is the form mdx_rank_full_segments reads in place.
 *
 * RCCL is bound at run time (dlopen of librccl.so.1 -- the copy the process already holds, e.g. PyTorch's); a box
 * without it gets MDX_ERR_RUNTIME from these calls and nothing else changes.  Communicator set-up follows RCCL:
 * ONE rank calls mdx_comm_unique_id and hands the MDX_COMM_ID_BYTES bytes to the others by any means (the Python
 * host uses its torch.distributed group), then EVERY rank calls mdx_comm_init with its device selected
 * (hipSetDevice); the call is collective.  Exchange calls only enqueue work on `stream`. */
typedef struct mdx_comm mdx_comm;
#define MDX_COMM_ID_BYTES 128
int mdx_comm_unique_id(void *id_host);
int mdx_comm_init(mdx_comm **out, const void *id_host, int nranks, int rank);
int mdx_comm_destroy(mdx_comm *comm);
int mdx_comm_info(const mdx_comm *comm, int *nranks, int *rank);

/* Queries [lo, hi) that rank `rank` of `nranks` ranks (sorts) under the query split: contiguous, sizes differ by <= 1. */
int mdx_query_bounds(int64_t nq, int nranks, int rank, int64_t *lo, int64_t *hi);

/* "All-gather of per-shard partial scores" (BASELINE.json north_star):
 *   local [nq, widths[rank]] on every rank  ->  all = G blocks back to back, block g = S_g [nq, widths[g]], on every rank.
 * widths: HOST array of nranks column counts (the shard sizes; the same on every rank).  Equal widths go out as one
 * ncclAllGather, unequal ones as a grouped send/receive per peer (one per xGMI link). */
int mdx_allgather_scores(mdx_comm *comm, const float *local, int64_t nq, const int64_t *widths, float *all, void *stream);

/* The query-split form (1/G of the bytes per rank; the ranking becomes G-way parallel): rank r keeps queries
 * [qlo_r, qhi_r) = mdx_query_bounds(nq, G, r) and receives their rows of every block:
 *   local [nq, widths[rank]]  ->  mine = G blocks back to back, block g = S_g[qlo_r:qhi_r, :]  ([nq_mine, widths[g]]).
 * mdx_rank_full_segments(blocks, widths, G, nq_mine, 0, ...) then yields the rankings of this rank's queries with
 * GLOBAL row ids. */
int mdx_exchange_scores(mdx_comm *comm, const float *local, int64_t nq, const int64_t *widths, float *mine, void *stream);

/* ------------------------------------------------- direct-store exchange (no collective; hipIpc + xGMI stores) */

/* The third form of the same exchange (round 6): the similarity kernel itself writes query q's run of scores into row
 * q - qlo_owner of the OWNER's receive buffer, at the columns of this shard -- over xGMI, into memory the owner has shared with
 * hipIpcGetMemHandle.  The transfer is spread over the kernel's run time, there is no collective launch, and the owner finds a
 * DENSE [nq_mine, n_total] matrix (mdx_rank_full; no peer blocks).  A step is closed by one flag per peer.  Shards the same
 * statement as above, `np.dot(vecs.T, qvecs)` (cirscore.py:69), for the query-split `np.argsort(-scores, axis=0)` (cirscore.py:70).
 *
 *   every rank, once:  mdx_p2p_create(&p, G, r, nq, n_total, handle)   (allocates 2 receive buffers of ceil(nq/G) x n_total fp32)
 *                      gather the G handles (MDX_P2P_HANDLE_BYTES each, rank order) by any means
 *                      mdx_p2p_connect(p, handles)                        (maps the peers' buffers; not a collective)
 *   every step:        mdx_scores_p2p(index, queries, nq, ..., p, ...)  once per shard (or row chunk) this rank holds
 *                      mdx_p2p_close_step(p, &mine, stream)             mine = this rank's queries x all rows, valid until the
 *                                                                       step after next is opened by any peer
 * Every rank must run the same steps with the same nq.  nq <= 128; fp32 shards (fp16 and int8 ones are refused); the shard's first global row is the index's
 * row_offset.  HARDWARE STATUS: exercised with several rank processes on ONE GPU (same-device IPC); it has not run over xGMI --
 * tools/preflight_ranks.py checks it on a multi-GPU node before bench.py uses it, and mdx_exchange_scores stays the default.
 * Needs HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC) in the environment of every rank process. */
typedef struct mdx_p2p mdx_p2p;
#define MDX_P2P_HANDLE_BYTES 64
/* handle_host: MDX_P2P_HANDLE_BYTES bytes, written.  MDX_ERR_RUNTIME with *out VALID when the buffer cannot be exported
 * (then only mdx_p2p_connect_ptrs can connect it). */
int mdx_p2p_create(mdx_p2p **out, int nranks, int rank, int64_t nq, int64_t n_total, void *handle_host);
/* handles_host: nranks x MDX_P2P_HANDLE_BYTES bytes in rank order (this rank's own entry is not read). */
int mdx_p2p_connect(mdx_p2p *p2p, const void *handles_host);
/* Ranks that live in ONE process (threads, tests): the peers' mdx_p2p_base pointers instead of handles (host array of nranks). */
int mdx_p2p_connect_ptrs(mdx_p2p *p2p, void *const *bases);
void *mdx_p2p_base(mdx_p2p *p2p);
int64_t mdx_p2p_bytes(const mdx_p2p *p2p);
/* mdx_scores with the routed epilogue: scores[q, i] goes to row q - qlo_owner(q), column row_offset(index) + i of owner(q)'s
 * receive buffer of the open step.  Same kernels, same k order, same bits as mdx_scores.  workspace: mdx_scores_workspace(nq, d). */
int mdx_scores_p2p(const mdx_index *index, const float *queries, int64_t nq, int qlayout, const float *center, mdx_p2p *p2p,
                   void *workspace, int64_t workspace_bytes, void *stream);
/* Enqueues: raise this rank's flag of the step at every peer, wait for every peer's.  *mine = device pointer to this rank's
 * [ceil(nq/G), n_total] buffer of the step (its first nq_mine rows are the queries mdx_query_bounds gives this rank). */
int mdx_p2p_close_step(mdx_p2p *p2p, float **mine, void *stream);
/* Synchronises `stream` and reads the status word: bit r set = a wait for peer r gave up after 20 s (results of that step are
 * undefined).  0 = every step so far was closed by every peer. */
int mdx_p2p_status(mdx_p2p *p2p, uint32_t *late_peers, void *stream);
int mdx_p2p_destroy(mdx_p2p *p2p);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H */
