/* mdx_train.h -- the trainable descriptor tail of libmdx.so: the backward of the global pooling and of the L2 normalisation, and the
 * two tuple losses with their gradients.  Included by mdx.h (section "trainable tail"); include mdx.h, not this file.  The prototypes
 * are apart from mdx.h's own for the reason given there under "exact kNN join" for mdx_knn_join.h; their names are in
 * _lib.TRAIN_EXPORTS and their census is tests/test_train_host.py.
 *
 * What this is for: mdir_amd/autograd.py wraps these calls into torch.autograd.Functions, so that the tail of ImageRetrievalNet
 * (pooling, L2N, in-network whitening) and the reference's ContrastiveLoss / TripletLoss (cirtorch/layers/loss.py,
 * layers/functional.py:141-173) take part in a backward pass.  The formulas are the ones torch's autograd evaluates for the
 * reference's statements (functional.py:11-22, :130-131); tests/train_restatement.py states them in float64.
 *
 * Common to every call: fp32, enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  Every sum
 * runs in a fixed order and there are no floating-point atomics: the same inputs give the same bits on every run.  Every pointer
 * needs the alignment of its element (4 bytes); a workspace 16 bytes.  Non-finite inputs carry no contract beyond staying inside
 * the buffers.
 *
 * mdx_pool_bwd.  feat [B,C,H,W], pooled [B,C] = mdx_pool_l2n(feat, ..., l2n_eps < 0), grad_pooled [B,C]  ->  grad_feat [B,C,H,W]
 *   (must not overlap feat) and, for MDX_POOL_GEM, grad_p [1].  With xc = x < eps ? eps : x, m = mean_hw(xc^p), y = m^(1/p) = pooled:
 *     GEM   grad_x = grad_y * y^(1-p) * xc^(p-1) / (H W) where x >= eps (the clamp passes the gradient at x == eps), exactly 0 where
 *           x < eps: an all-zero plane gets an all-zero gradient.
 *           grad_p = sum over the planes, in plane order, of grad_y * y * (-ln(m) / p^2 + mean_hw(xc^p ln xc) / (p m)).
 *     SPOC  grad_x = grad_y / (H W) everywhere.
 *     MAC   grad_x = grad_y at the first maximum of the plane in row-major order, 0 elsewhere (an all-zero plane: element 0).
 *   x^p is the routine of the forward (exact products for p = 1, 2, 3, the hardware exp2 / log2 units otherwise), and m is summed in
 *   the forward's order.  One wave per (image, channel) plane reads it twice (the sums, then the gradient; the second read comes from
 *   the cache) and writes it once, in 16-byte accesses where H W % 4 == 0 (at dword alignment off the 16-byte grid).  GEM: every
 *   plane's part of grad_p goes to the workspace and a second, one-workgroup launch adds the parts: thread t of 1024 adds the parts
 *   t, t + 1024, ... in that order, then a fixed butterfly.  MAC and SPOC take one launch and use neither workspace nor grad_p (both
 *   may be NULL).
 * mdx_l2n_rows_bwd.  x [R,D] (the rows BEFORE normalisation, bias already added), grad_out [R,D]  ->  grad_x [R,D] (may be grad_out).
 *   With n = ||x||:  n > 0: grad_x = grad_out / (n + eps) - x * (grad_out . x) / (n (n + eps)^2);  n == 0: grad_x = grad_out / eps
 *   (the norm's subgradient at 0 is 0).  One workgroup per row; the two sums in the order of mdx_l2n_rows.
 * mdx_contrastive_loss.  x [D,N] row-major (one descriptor per COLUMN, as the reference's `output`), label [N] fp32, nq tuples of
 *   S = N / nq columns each: column t S is the query of tuple t (label -1), the columns t S + 1 .. t S + S - 1 are its pairs with
 *   label l = 1 or 0.  Per pair, with dif = x_query - x_pair: dist = sqrt(sum_k (dif_k + eps)^2), the term is
 *   0.5 l dist^2 + 0.5 (1 - l) max(margin - dist, 0)^2, and its gradient with respect to dif_k is
 *   (l - (1 - l) max(margin - dist, 0) / dist) (dif_k + eps): added to the query's column, subtracted from the pair's.  A pair with
 *   dist == 0 is NaN in the reference and carries no contract.  loss [1] = the sum of the terms; grad_x [D,N] is written whole.
 * mdx_triplet_loss.  The same layout with S >= 3 and one label-1 column per tuple (the first one counts; the host checks that there
 *   is exactly one): loss = sum over the tuples and their label-0 columns n of max(|q - p|^2 - |q - n|^2 + margin, 0); the gradient
 *   flows where the argument is >= 0 (the clamp passes at equality): 2 (q - p) - 2 (q - n) to q, -2 (q - p) to p, 2 (q - n) to n.
 *   Both losses: one workgroup per tuple walks its columns in order (the query's gradient accumulates in column order), the terms of
 *   a tuple are added in column order, and a second one-wave launch adds the tuples' parts from the workspace IN TUPLE ORDER.
 *   The label vector is not validated on the device: labels in another layout pair other columns, inside the buffers.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer, a size < 1, H W >= 2^31,
 * R or nq >= 2^31, an unknown kind, GEM with p <= 0 or pool_eps <= 0, eps < 0 (mdx_l2n_rows_bwd), grad_feat overlapping feat, N not a
 * multiple of nq, S < 2 (contrastive) / S < 3 (triplet).  MDX_ERR_WORKSPACE for fewer bytes than the size function says, or NULL
 * (MDX_ERR_INVALID for a workspace that is not 16-byte aligned). */
#ifndef MDX_TRAIN_H
#define MDX_TRAIN_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* Bytes of device workspace of mdx_pool_bwd with MDX_POOL_GEM: one fp32 per plane, round_up(4 B C, 256); 0 for B or C < 1. */
int64_t mdx_pool_bwd_workspace(int B, int C);
int mdx_pool_bwd(const float *feat, const float *pooled, const float *grad_pooled, int B, int C, int H, int W, int kind, float p,
                 float pool_eps, float *grad_feat, float *grad_p, void *workspace, int64_t workspace_bytes, void *stream);
int mdx_l2n_rows_bwd(const float *x, const float *grad_out, int64_t R, int64_t D, float eps, float *grad_x, void *stream);
/* Bytes of device workspace of the two losses: one fp32 per tuple, round_up(4 nq, 256); 0 for nq < 1 or nq >= 2^31. */
int64_t mdx_tuple_loss_workspace(int64_t nq);
int mdx_contrastive_loss(const float *x, const float *label, int64_t D, int64_t N, int64_t nq, float margin, float eps, float *loss,
                         float *grad_x, void *workspace, int64_t workspace_bytes, void *stream);
int mdx_triplet_loss(const float *x, const float *label, int64_t D, int64_t N, int64_t nq, float margin, float *loss, float *grad_x,
                     void *workspace, int64_t workspace_bytes, void *stream);

#endif /* MDX_TRAIN_H */
