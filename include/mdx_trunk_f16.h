/* mdx_trunk_f16.h -- the prototypes of the fp16 trunk mode of libmdx.so: the epilogue and the poolings on fp16 feature maps.
 * Included by mdx.h, which states the two contracts in its section "fp16 trunk"; include mdx.h, not this file.  Why they are
 * apart from mdx.h's own prototypes is said there (as for mdx_knn_join.h). */
#ifndef MDX_TRUNK_F16_H
#define MDX_TRUNK_F16_H

#ifndef MDX_H
#error "include mdx.h: it states the contract and includes this file"
#endif

/* An fp16 element is an IEEE binary16 in 2 bytes.  The type is HIP's (hip/hip_fp16.h defines it); it is only named here,
 * so any other caller passes pointers to its own 16-bit type. */
struct __half;
typedef struct __half __half;

int mdx_bn_act_f16(__half *x, const __half *residual, int64_t N, int64_t C, int64_t HW, const float *mean, const float *var,
                   const float *weight, const float *bias, float eps, int relu, void *stream);
int mdx_pool_l2n_f16(const __half *feat, int B, int C, int H, int W, int kind, float p, float pool_eps, float l2n_eps, float *out,
                     void *stream);
int mdx_pool_multi_f16(const __half *const *feats, int S, int B, int C, const int *H, const int *W, int kind, float p, float pool_eps,
                       float *pooled, void *stream);

#endif /* MDX_TRUNK_F16_H */
