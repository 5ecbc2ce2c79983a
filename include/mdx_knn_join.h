/* mdx_knn_join.h -- the prototypes of the exact kNN join of libmdx.so.  Included by mdx.h, which states the contract, the
 * proofs, the stages and the refusals in its section "exact kNN join"; include mdx.h, not this file.  Why they are apart, and that
 * the entry-point census of tests/test_memguard_host.py therefore does not see them, is said there. */
#ifndef MDX_KNN_JOIN_H
#define MDX_KNN_JOIN_H

#ifndef MDX_H
#error "include mdx.h: it declares mdx_index and includes this file"
#endif

#define MDX_KNN_JOIN_MAX_K 64
int64_t mdx_knn_bounds_workspace(int64_t m, int64_t k, int64_t nb, int64_t slices);
int mdx_knn_bounds(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo, int64_t a_hi,
                   int64_t k, int64_t slices, float *t, void *workspace, int64_t workspace_bytes, void *stream);
int mdx_join_candidates_rows(const mdx_index *a, const float *stats_a, const mdx_index *b, const float *stats_b, int64_t a_lo,
                             int64_t a_hi, const float *tau, uint64_t *pairs, int64_t capacity, int64_t *count, void *stream);
int64_t mdx_knn_resolve_workspace(int64_t P, int64_t m);
int mdx_knn_resolve(const float *rows_a, int64_t lda, const float *rows_b, int64_t ldb, int64_t d, const uint64_t *pairs, int64_t P,
                    int64_t m_lo, int64_t m, int64_t k, int64_t *ids, float *scores, int32_t *counts, void *workspace,
                    int64_t workspace_bytes, void *stream);

#endif /* MDX_KNN_JOIN_H */
