/* mdx_ivf.h -- the inverted file: score only the rows of the lists a query probes.  Included by mdx.h (section "inverted file");
 * include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under "exact kNN join" for
 * mdx_knn_join.h; their names are in _lib.IVF_EXPORTS and their census is tests/test_ivf_host.py.
 *
 * What this is for: mdir_amd/ivf.py keeps the partition of a database that mdir_amd/cluster.py makes -- `members`, the row ids grouped
 * by list and ascending inside a list, and `offsets`, int64 [K + 1] -- and answers a batch of queries from the lists whose centroids
 * score best (`probes`, int64 [nq, nprobe], the ids of mdx_topk over the centroid scores).  A query's candidates are the members of
 * its probed lists, in probe order and, inside a list, in member order; their scores are the exact fp32 chain (csrc/mdx_exact.h), the
 * bits of mdx_scores on an fp32 index of the same rows; the answer is the first k candidates in mdx_rank_full's order.
 * tests/ivf_restatement.py states all of it in numpy.
 *
 * Common to every call: enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  Sizes the host
 * cannot know without a read-back are replaced by bounds it does know: `cap`, the columns of a query's candidate row (the sum of the
 * nprobe largest list sizes is enough for distinct probes), and `items`, the workgroups of the scan (below).  Every pointer needs the
 * alignment of its element (4 bytes for fp32, 8 for int64); the plan 16 bytes.  No input makes a kernel read or write outside its
 * buffers: offsets are clamped to [0, m] and a list whose clamped end lies before its start is empty; a probe outside [0, K) is
 * skipped (it owns no candidates); a member id outside [0, n) is never dereferenced and scores NaN; everything a kernel reads from the
 * plan is checked against the sizes of the call before it is used as an index.
 *
 * mdx_ivf_plan.  probes [nq, nprobe], offsets [K + 1], m members  ->  the plan, mdx_ivf_plan_workspace(nq, nprobe, K) bytes that
 *   mdx_ivf_scan and mdx_ivf_select read.  Its sections, each int64 and each starting on a multiple of 256 bytes, in this order:
 *     base    [nq, nprobe]  the first column of probe p's segment in query q's candidate row: the sum of the (clamped) sizes of the
 *                           lists of the valid probes before p; -1 for a probe outside [0, K);
 *     count   [nq]          min(cap, the sum over the valid probes): the candidates of the query.  Candidates whose column would be
 *                           cap or more do not exist;
 *     first   [K + 1]       the inverted probe table, CSR: list l is probed by the entries entry[first[l] .. first[l + 1]);
 *     item    [K + 1]       item[l] = the work items of the lists before l; list l has ceil(size / 64) tiles times
 *                           ceil(probing entries / MDX_IVF_QUERY_GROUP) groups of them; item[K] is their number;
 *     entry   [nq nprobe]   q nprobe + p of every valid probe, grouped by list.  The order inside a list is the order in which
 *                           integer atomics landed: no score and no column depends on it (a candidate's column is fixed by base and
 *                           its member index), only which queries share a workgroup;
 *     cursor  [2 K]         the counters of the count and of the fill.
 *   Four launches: zero the counters; one thread per query (prefix over its probes, one atomic per valid probe); one workgroup scans
 *   the K counts into first and item; one thread per probe fills entry.
 * mdx_ivf_scan.  The hot kernel, list-major.  One workgroup of 256 threads owns one work item: a tile of 64 members of one list and a
 *   group of up to MDX_IVF_QUERY_GROUP entries that probe it.  The tile's rows are gathered whole through `members`, 1 KiB of one row
 *   per wave-instruction, into a padded LDS tile once per stage of 256 dimensions and serve every query of the group; the next
 *   stage's pieces are in flight in registers meanwhile.  Wave w runs the chains of the group's entries w, w + 4, ...: lane = member,
 *   the query's stage broadcast from LDS, acc = fma(x_q[k], row[k], acc) from +0 with k ascending, continued over zeros to
 *   round_up(d, 64); x_q = q - center in one fp32 subtraction when center is given.  16-byte loads where ld % 4 == 0 and rows lie on
 *   the 16-byte grid, dword loads otherwise: the same bits.  It writes cand_scores [nq, cap] and cand_ids [nq, cap] (the member id
 *   as given; NaN for an id outside [0, n)); a second launch writes NaN / -1 into the columns at or beyond count[q].  The grid is
 *   `items` workgroups; a workgroup whose item does not exist leaves.  `items` must be at least item[K], which the host bounds from
 *   the tile counts of the lists (mdir_amd/ivf.py, item_bound); with fewer the candidates of the items beyond keep what the buffers
 *   held.
 * mdx_ivf_select.  cand_scores, cand_ids [nq, cap] and the plan's count  ->  out_ids int64 [nq, k], out_scores fp32 [nq, k]: per query
 *   the first min(k, count) candidates by (order key of the score, id) -- larger score first, -0 == +0, NaN last, equal keys by
 *   ascending id -- sorted; positions at or beyond count hold id -1 and NaN.  One workgroup of 1024 threads per query.  Up to
 *   MDX_RESCORE_MAX_K candidates go to LDS as they are; above that a radix select over the order key (four passes of 8 bits) finds
 *   the key of position k, and where more candidates than needed carry that key a second select over their ids (eight passes) finds
 *   the last id taken; the chosen min(k, count) pairs are collected in LDS.  A bitonic sort of the pairs by (key, id) ends both
 *   routes, so the order in which pairs were collected does not reach the result.  Scores leave with the bits they came with.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer (center may be NULL); nq, nprobe, K,
 * m, n, d, cap, items or k < 1; nprobe > K; k > MDX_RESCORE_MAX_K; nq, K, m, n, d or cap at or above 2^31, nq nprobe or items at or
 * above 2^31, nq ceil(cap / 1024) at or above 2^31; ld < d; n ld or nq cap beyond int64; a qlayout that is neither MDX_DIM_MAJOR nor
 * MDX_ROW_MAJOR; a plan that is not 16-byte aligned.  MDX_ERR_WORKSPACE for a plan of fewer bytes than mdx_ivf_plan_workspace says, or
 * NULL. */
#ifndef MDX_IVF_H
#define MDX_IVF_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* Entries (query, probe) that share one tile of a list in one workgroup of mdx_ivf_scan (ops.IVF_QUERY_GROUP mirrors it), and the
 * members of a tile (ops.IVF_TILE). */
#define MDX_IVF_QUERY_GROUP 8
#define MDX_IVF_TILE 64

/* Bytes of the plan: round_up(8 nq nprobe, 256) * 2 + round_up(8 nq, 256) + round_up(8 (K + 1), 256) * 2 + round_up(16 K, 256); 0 for
 * sizes the calls refuse. */
int64_t mdx_ivf_plan_workspace(int64_t nq, int64_t nprobe, int64_t K);
int mdx_ivf_plan(const int64_t *probes, int64_t nq, int64_t nprobe, const int64_t *offsets, int64_t K, int64_t m, int64_t cap,
                 void *plan, int64_t plan_bytes, void *stream);
int mdx_ivf_scan(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, int64_t m, const int64_t *offsets,
                 int64_t K, const float *queries, int64_t nq, int qlayout, const float *center, int64_t nprobe, const void *plan,
                 int64_t plan_bytes, int64_t cap, int64_t items, float *cand_scores, int64_t *cand_ids, void *stream);
int mdx_ivf_select(const float *cand_scores, const int64_t *cand_ids, int64_t nq, int64_t cap, int64_t nprobe, int64_t K,
                   const void *plan, int64_t plan_bytes, int64_t k, int64_t *out_ids, float *out_scores, void *stream);

#endif /* MDX_IVF_H */
