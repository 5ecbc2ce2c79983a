/* mdx_groups.h -- the prototypes of the near-duplicate groups of libmdx.so.  Included by mdx.h, which states the contract, the
 * forest, the memory-model rule, the skip rule and the refusals in its section "near-duplicate groups"; include mdx.h, not this
 * file.  They are apart from mdx.h's own prototypes for the reason given there under "exact kNN join" for mdx_knn_join.h:
 * tests/test_cabi.py and tests/test_memguard_host.py pin the prototypes of mdx.h itself and their number, and the change that added
 * this section was to leave existing tests as they were.  Their census is tests/test_groups_host.py. */
#ifndef MDX_GROUPS_H
#define MDX_GROUPS_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_GROUPS_MAX_T 8
int mdx_groups_init(int32_t *parent, int64_t T, int64_t n, int64_t *status, void *stream);
int mdx_groups_union_pairs(const float *rows, int64_t ld, int64_t d, const uint64_t *pairs, int64_t P, const float *taus, int64_t T,
                           int32_t *parent, int64_t n, int64_t *status, void *stream);
int mdx_groups_union_dense(const float *scores, int64_t m, int64_t ncols, int64_t ld, int64_t row_base, int64_t col_base, const float *taus,
                           int64_t T, int32_t *parent, int64_t n, int64_t *status, void *stream);
int mdx_groups_labels(const int32_t *parent, int64_t T, int64_t n, int64_t *labels, void *stream);

#endif /* MDX_GROUPS_H */
