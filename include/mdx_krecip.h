/* mdx_krecip.h -- k-reciprocal re-ranking of libmdx.so: the contract and the prototypes.  Included by mdx.h (section "k-reciprocal
 * re-ranking"); include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under "exact kNN
 * join" for mdx_knn_join.h; their names are in _lib.KRECIP_EXPORTS and their census is tests/test_krecip_host.py.
 *
 * k-reciprocal encoding (Zhong, Zheng, Cao, Li, "Re-ranking person re-identification with k-reciprocal encoding", CVPR 2017) in its
 * database-side form: the codes of the database rows are built once from the database's own kNN lists; a query is encoded against
 * those lists at query time.  The database lists are NOT rebuilt with the query in them, and the paper's all-pairs form over
 * (gallery + probe)^2 is not what this is.
 *
 * Inputs and notation
 *   L_i     row i's list of mdx_topk / the exact kNN join: ids int64 / sims fp32 [N, k], k = min(k1, N), descending score, ascending
 *           id on ties.  L_i^w = its first w entries.  An id outside [0, N) is never dereferenced and is a member of nothing; a
 *           repeated id counts at its first position only.
 *   h       = ceil(k / 2)
 * Reciprocal sets.  R(i, w) = { j in L_i^w : i in L_j^w }, taken literally, kept in the order of L_i.  Row i is in its own set exactly
 *   when it is in its own list (with many identical rows it may not be).  Two widths are stored: R(i, k) and R(i, h), as ELL
 *   [N, k] / [N, h] int32 with int32 counts [N]; the entries beyond a count are -1.
 * Expansion.  R*(i) = R(i, k) U union { R(c, h) : c in R(i, k), 3 |R(i, k) & R(c, h)| >= 2 |R(c, h)| }: integer arithmetic only; an
 *   empty R(c, h) adds nothing.
 * Raw code V_i.  Support R*(i), ascending id.  w_ij = expf(fmaf(2, s_ij, -2)) (exp(-|x_i - x_j|^2) for unit rows); a NaN score
 *   gives weight 0.  s_ij is the exact chain score of rows i and j: for j in L_i it is GATHERED, sims[i, first position of j]; for
 *   every other j it is RECOMPUTED in the kernel with the chain of "exact rescoring of shortlists" (k ascending fmaf from +0,
 *   continued over zeros to round_up(d, 64)), the bits of mdx_rescore and, for d % 4 == 0, of mdx_scores_rowmajor.
 *   V_ij = w_ij / t, t the fp32 sequential sum of the w in ascending-id order; t == 0 gives an all-zero code.
 * Local query expansion.  V'_i = (1 / c) sum over t < min(k2, k), L_i[t] present, of V_{L_i[t]}; an entry is present when its id is
 *   in [0, N) and is the first copy in L_i; c is the number of present entries.  Each column is a sequential fp32 sum in list order
 *   over the codes that hold it, then one division by c.  Support: the union of the summed supports, ascending.
 * Both codes are CSRs: offsets int64 [N + 1], cols int32 ascending within a row, vals fp32.
 * Static cap.  k <= MDX_KRECIP_MAX_K1 = 64, 1 <= k2 <= k and k2 * k * (1 + ceil(k / 2)) <= MDX_KRECIP_MAX_NNZ = 4096: this bounds
 *   every support (a raw code by k + k h), so nothing can overflow at run time; parameters beyond it are MDX_ERR_INVALID before any
 *   launch.
 *
 * Query q.  Inputs: the first-stage scores s_q [N] (any similarity mode) and T_q = the ids of mdx_topk(s_q, R), R = min(truncate, N)
 *   <= MDX_KRECIP_MAX_R = 4096.  Every score of q is read from the score row: s_qg = s_q[g].
 *   N(q)   = the first min(k, R) entries of T_q (valid ids, first copies)
 *   R(q)   = { g in N(q) : s_qg >= kth[g] }, kth[g] = sims[g, k - 1]: q would enter g's list.  An fp32 compare; NaN is false.
 *   R*(q)  the expansion above with R(q) in place of R(i, k); V_q as V_i with s_q[j] as the score
 *   V'_q   = (V_q + sum over t < k2 - 1 of V_{T_q[t]}) / c: its own raw code first, then the raw codes of its best k2 - 1 rows
 *            (present as above), c = 1 + the number of present rows.  A query that is a database row meets its own row among
 *            them and is counted once more, as in alpha-QE.
 *   for every a < R, g = T_q[a] in [0, N):   m = sum_j min(V'_q[j], V'_g[j])
 *            out[q, g] = (1 - lam) * m / (2 - m) + lam * (1 + s_qg) / 2         (m / (2 - m) = 1 - d_Jaccard for codes that sum to 1)
 *            (the copies of a repeated id compute the same bits)
 *   every other entry of the row is s_qj - 3: rows outside the shortlist rank last, in first-stage order, as in truncated diffusion.
 * Determinism.  Supports, counts and offsets are integer results.  Every value is bit-identical run to run and independent of nq and
 *   of the other queries: all sums run in a fixed order (the min-sum: per-lane partials over the positions lane, lane + 64, ... of
 *   V'_g, then a fixed butterfly); no float atomics.
 * Stream capture.  Every call only enqueues; mdx_krecip_rerank reads nothing back and is legal under capture.  A caller of the two
 *   *_offsets calls reads offsets[N] (the nnz) back to size cols / vals: one read-back per CSR.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer (cols / vals of a CSR may be NULL
 * only when its nnz is 0), n, k, nq or r < 1, n >= 2^31, k > MDX_KRECIP_MAX_K1, k2 outside [1, k], the cap above, d < 1, ld < d,
 * a negative nnz, r > MDX_KRECIP_MAX_R or r > n, nq * ceil(n / 4096) >= 2^31, nq * r >= 2^39, a stride below n, lam outside [0, 1]
 * or not finite, out overlapping scores other than out == scores with the same stride.  MDX_ERR_WORKSPACE for fewer than
 * mdx_krecip_rerank_workspace(nq, r) bytes (16-byte aligned). */
#ifndef MDX_KRECIP_H
#define MDX_KRECIP_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_KRECIP_MAX_K1 64
#define MDX_KRECIP_MAX_NNZ 4096
#define MDX_KRECIP_MAX_R 4096

/* R(i, k) -> rk [n, k], rk_counts [n]; R(i, ceil(k / 2)) -> rh [n, ceil(k / 2)], rh_counts [n].  One launch, no workspace. */
int mdx_krecip_sets(const int64_t *ids, int64_t n, int64_t k, int32_t *rk, int32_t *rk_counts, int32_t *rh, int32_t *rh_counts,
                    void *stream);
/* offsets int64 [n + 1] of the raw codes from the sets of mdx_krecip_sets: the count pass and the scan, on the device. */
int mdx_krecip_raw_offsets(int64_t n, int64_t k, const int32_t *rk, const int32_t *rk_counts, const int32_t *rh,
                           const int32_t *rh_counts, int64_t *offsets, void *stream);
/* cols int32 / vals fp32 [nnz] of the raw codes, nnz = offsets[n]; rows fp32 [n, d] at a stride of ld floats, read in place.  Nothing
 * is written outside [0, nnz) whatever offsets holds. */
int mdx_krecip_raw_fill(const float *rows, int64_t ld, int64_t d, const int64_t *ids, const float *sims, int64_t n, int64_t k,
                        const int32_t *rk, const int32_t *rk_counts, const int32_t *rh, const int32_t *rh_counts,
                        const int64_t *offsets, int32_t *cols, float *vals, int64_t nnz, void *stream);
/* offsets int64 [n + 1] of the expanded codes from the raw CSR (raw_nnz = raw_offsets[n]). */
int mdx_krecip_expand_offsets(const int64_t *ids, int64_t n, int64_t k, int64_t k2, const int64_t *raw_offsets,
                              const int32_t *raw_cols, int64_t raw_nnz, int64_t *offsets, void *stream);
/* cols / vals [nnz] of the expanded codes, nnz = offsets[n]. */
int mdx_krecip_expand_fill(const int64_t *ids, int64_t n, int64_t k, int64_t k2, const int64_t *raw_offsets,
                           const int32_t *raw_cols, const float *raw_vals, int64_t raw_nnz, const int64_t *offsets, int32_t *cols,
                           float *vals, int64_t nnz, void *stream);
/* Bytes of device workspace of mdx_krecip_rerank: the values of every query's shortlist, nq * round_up(4 r, 256); 0 for nq or r < 1,
 * nq >= 2^31 or r > MDX_KRECIP_MAX_R. */
int64_t mdx_krecip_rerank_workspace(int64_t nq, int64_t r);
/* The query-time call: rh / rh_counts of mdx_krecip_sets, kth fp32 [n] = sims[:, k - 1], both CSRs, scores [nq, n] at ld_scores,
 * top_ids int64 [nq, r] contiguous (mdx_topk of the scores), out [nq, n] at ld_out (may equal scores with the same stride).  Here k2
 * counts the query's own code: k2 - 1 rows are added.  Three launches: the codes and min-sums (one workgroup per query, nq
 * unbounded), out = s - 3, the scatter. */
int mdx_krecip_rerank(const int32_t *rh, const int32_t *rh_counts, const float *kth, int64_t n, int64_t k, int64_t k2,
                      const int64_t *raw_offsets, const int32_t *raw_cols, const float *raw_vals, int64_t raw_nnz,
                      const int64_t *qe_offsets, const int32_t *qe_cols, const float *qe_vals, int64_t qe_nnz, const float *scores,
                      int64_t ld_scores, const int64_t *top_ids, int64_t nq, int64_t r, float lam, float *out, int64_t ld_out,
                      void *workspace, int64_t workspace_bytes, void *stream);

#endif /* MDX_KRECIP_H */
