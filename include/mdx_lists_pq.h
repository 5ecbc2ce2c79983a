/* mdx_lists_pq.h -- product-quantised list storage for the inverted file (IVF-PQ): the per-query look-up table and the scan over byte
 * codes (asymmetric distance computation, ADC).  Included by mdx.h (section "inverted file, product-quantised lists") after
 * mdx_lists_i8.h; include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under "exact kNN
 * join" for mdx_knn_join.h; their names are in _lib.LISTS_PQ_EXPORTS and their census is tests/test_pq_host.py.
 *
 * What this is for.  mdx_ivf_scan reads 4 d bytes of a member, mdx_lists_i8_scan round_up(d, 64).  Here a member is M bytes: its
 * residual r = row - centroid[list] is cut into M sub-vectors of dsub = d / M elements and each is replaced by the id of its nearest
 * of 256 codewords (mdir_amd/pq.py trains the codebook and encodes; it composes mdx_scores_ex, mdx_kmeans_argmax and mdx_kmeans_sums
 * and needs no kernel of its own).  The score of a member against a query is then
 *     <x_q, centroid> + sum_m <x_q sub-vector m, codeword (m, code[m])>
 * whose first term is the coarse score that chose the list and whose others are M look-ups in a table of the query.  The plan
 * (mdx_ivf_plan), the candidate rows and the selection (mdx_ivf_select) are those of mdx_ivf.h, unchanged; an exact second stage is
 * mdx_rescore on the fp32 rows, where they are kept.  mdir_amd/ivfpq.py, IVFPQIndex, puts them together; tests/pq_restatement.py
 * restates the quantiser and the search in numpy.
 *
 * Common to both calls: enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  Every pointer needs
 * the alignment of its element (1 byte for codes, 4 for fp32, 8 for int64); the plan 16 bytes.  No input makes a kernel read or write
 * outside its buffers, as in mdx_ivf.h.
 *
 * mdx_pq_lut.  codewords fp32 [M, 256, dsub] contiguous, queries fp32 in qlayout ([nq, d] MDX_ROW_MAJOR or [d, nq] MDX_DIM_MAJOR, d =
 *   M dsub), center fp32 [d] or NULL (x_q = q - center in one fp32 subtraction)  ->  lut fp32 [nq, M, 256]:
 *     lut[q, m, j] = the exact chain of sub-vector m of x_q with codeword (m, j): acc = +0, acc = fmaf(x_q[m dsub + k], c[k], acc) for
 *     k = 0 .. dsub - 1 in that order, and where dsub % 64 != 0 once more acc = fmaf(0, 0, acc), as the library's zero padding of a chain
 *     to round_up(dsub, 64) does (a -0 becomes +0) -- the bits mdx_scores gives on an fp32 index of codewords[m] for that sub-vector.
 *   One workgroup of 256 threads per (subspace, group of MDX_PQ_LUT_QUERIES queries): thread j owns codeword j and reads it once for
 *   the whole group (16-byte loads where dsub % 4 == 0 and codewords lies on the 16-byte grid, dword loads otherwise: the same bits);
 *   the group's sub-vectors are staged in LDS 256 k at a time and broadcast.
 * mdx_lists_pq_scan.  The hot kernel, query-major.  codes uint8 [m, ldc]: row p holds the M codes of member members[p] in its first M
 *   bytes, subspace 0 first (list order, as the int8 lists).  ldc >= M is the row stride in bytes; the bytes M .. ldc of a row may be
 *   read and are never interpreted.  There is no other padding: mdir_amd/ivfpq.py keeps codes [N, M] with ldc = M.  16-byte loads where
 *   ldc % 16 == 0 and codes lies on the 16-byte grid, dword loads where that holds for 4, byte loads otherwise: the same bits.
 *   lut fp32 [nq, M, 256] is mdx_pq_lut's; coarse fp32 [nq, nprobe] the values mdx_topk returned with `probes` int64 [nq, nprobe];
 *   `plan` is mdx_ivf_plan's of the same probes, offsets, m and cap.  Outputs cand_scores fp32 / cand_ids int64 [nq, cap]: the member
 *   at index i of the list of probe p of query q goes to column base[q, p] + i,
 *     cand_scores = acc after  acc = coarse[q, p];  acc = acc + lut[q, m, code[m]]  for m = 0 .. M - 1 in that order
 *   -- M plain fp32 additions, one rounding each, nothing reassociated; cand_ids = the member id as given.  A member id outside [0, n)
 *   scores NaN.  A probe outside [0, K), or one the plan marks invalid (base < 0), owns no candidates; a column at or beyond cap does
 *   not exist; offsets are clamped to [0, m].  The second launch is the pad kernel of csrc/mdx_ivf_plan.h (NaN / -1 at or beyond
 *   count[q]), so mdx_ivf_select works unchanged.
 *   Launch shape: nq * splits workgroups of 512 threads, splits = min(nprobe, ceil(MDX_PQ_SCAN_GROUPS / nq)) -- a host-side bound,
 *   nothing read back.  A workgroup copies its query's table to LDS (M KiB: two workgroups per CU up to M = 80, one above) and walks
 *   the probes s, s + splits, ... of its query, one wave per probe in turn, lane = member: the codes of a member are loaded 16 at a
 *   time, each is one LDS read at table[m][code], and the additions run in m order per lane.  The reads of one wave-instruction go to
 *   random columns of one table row, so they conflict on banks (tools/ivf_pq_bench.py measures the stage; profiles/r23_ivf_pq.md).
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer (center may be NULL); M outside
 * [1, MDX_PQ_MAX_M]; dsub, nq, nprobe, K, m, n or cap < 1; M dsub, nq, K, m, n, cap or ldc at or above 2^31; M ceil(nq /
 * MDX_PQ_LUT_QUERIES), nq nprobe, nq splits or nq ceil(cap / 1024) at or above 2^31; nprobe > K; ldc < M; a qlayout that is neither
 * MDX_DIM_MAJOR nor MDX_ROW_MAJOR; a plan that is not 16-byte aligned.  MDX_ERR_WORKSPACE for a plan of fewer bytes than
 * mdx_ivf_plan_workspace says, or NULL. */
#ifndef MDX_LISTS_PQ_H
#define MDX_LISTS_PQ_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* Sub-quantisers of a code at most (ops.PQ_MAX_M; the table of a query is M KiB of LDS), the codewords of each (a code is one byte),
 * the queries that share a codeword's registers in mdx_pq_lut, and the workgroups mdx_lists_pq_scan aims for when it splits the probes
 * of a query. */
#define MDX_PQ_MAX_M 128
#define MDX_PQ_CODEWORDS 256
#define MDX_PQ_LUT_QUERIES 8
#define MDX_PQ_SCAN_GROUPS 2048

int mdx_pq_lut(const float *codewords, int64_t M, int64_t dsub, const float *queries, int64_t nq, int qlayout, const float *center,
               float *lut, void *stream);
int mdx_lists_pq_scan(const uint8_t *codes, int64_t m, int64_t M, int64_t ldc, const int64_t *members, int64_t n, const int64_t *offsets,
                      int64_t K, const float *lut, const float *coarse, const int64_t *probes, int64_t nq, int64_t nprobe,
                      const void *plan, int64_t plan_bytes, int64_t cap, float *cand_scores, int64_t *cand_ids, void *stream);

#endif /* MDX_LISTS_PQ_H */
