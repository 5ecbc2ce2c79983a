/* mdx_kmeans.h -- spherical k-means on the device: what one iteration needs beside the similarity itself.  Included by mdx.h (section
 * "spherical k-means"); include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under
 * "exact kNN join" for mdx_knn_join.h; their names are in _lib.KMEANS_EXPORTS and their census is tests/test_kmeans_host.py.
 *
 * What this is for: mdir_amd/cluster.py partitions a database of L2-normalised descriptors into K clusters by cosine similarity.  The
 * expensive half of an iteration, the scores of every row against the K centroids, is mdx_scores_ex on an fp32 mdx_index of the
 * centroids.  The three calls here are the rest: the best centroid of every row, the sum of every cluster's rows, and the
 * normalisation of the sums into the next centroids.  tests/kmeans_restatement.py states all three, and the loop, in numpy.
 *
 * Common to every call: fp32 rows, enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  There are
 * no floating-point atomics and every sum runs in the order stated here: the same inputs give the same bits on every run.  Every
 * pointer needs the alignment of its element (4 bytes for fp32, 8 for int64); a workspace 16 bytes.
 *
 * mdx_kmeans_argmax.  scores [m, K] row-major with leading dimension ld >= K  ->  labels int64 [m], best fp32 [m] (either may be NULL,
 *   not both).  labels[r] and best[r] are the first entry of mdx_topk(k = 1) of row r: the larger score wins, equal scores go to the
 *   smaller id, -0 == +0, NaN loses to everything; best[r] holds the bits of scores[r, labels[r]] (a -0 that wins stays -0).  A row
 *   of NaN alone gives label 0 and the NaN of column 0.  One pass over the block: for K <= 1024 one wave reads a row (four rows per
 *   workgroup), above that the four waves of a workgroup share a row; 16-byte loads where ld % 4 == 0 and the base lies on the
 *   16-byte grid, dword loads otherwise.  A lane meets its columns in ascending order and keeps the first best one; lanes, then
 *   waves, are merged by the minimum of (order key, id).  Nothing is sorted.
 * mdx_kmeans_sums.  rows [n, d] row-major with leading dimension ld >= d; members int64 [n], the row ids grouped by cluster and
 *   ascending inside a cluster; offsets int64 [K + 1], cluster c owns members[offsets[c] .. offsets[c + 1])  ->  sums [K, d],
 *   contiguous.  sums[c, :] is defined to the bit:
 *     - the members of cluster c are cut into consecutive segments of MDX_KMEANS_SEGMENT members (the last one may be shorter);
 *     - a segment's partial is, per dimension, acc = +0.0f, then acc = acc + x over its members in order;
 *     - the cluster's sum is, per dimension, acc = +0.0f, then acc = acc + partial over its segments in order.
 *   Plain IEEE fp32 additions, round to nearest even; nothing is contracted or reassociated.  An empty cluster gets +0.  A member id
 *   outside [0, n) is skipped (its segment keeps its place).  Offsets are clamped to [0, n], and a cluster whose clamped end lies
 *   before its start is empty.  members and offsets are not validated beyond that: offsets that overlap or leave rows out sum what
 *   they say, and where overlapping offsets describe more than ceil(n / MDX_KMEANS_SEGMENT) + K segments the segments beyond that
 *   number are left out of their sums -- no input makes a kernel read or write outside the buffers.
 *   Three launches.  (1) One workgroup turns the offsets into the first segment number of every cluster, int64 [K + 1] at the start
 *   of the workspace.  (2) One workgroup per (segment, slice of 1024 dimensions): the grid is the bound ceil(n / SEGMENT) + K, so
 *   nothing is read back; a workgroup finds its cluster by bisection and leaves when its segment does not exist.  A thread owns four
 *   dimensions and reads them with one 16-byte load per member where ld % 4 == 0 and the base lies on the 16-byte grid, with dword
 *   loads otherwise; the partial goes to the workspace, a matrix [segments, round_up(d, 4)].  (3) One thread per (cluster, dimension)
 *   runs the chain over the cluster's partials.  d need not be a multiple of 4.
 *   The segment length trades the partials' traffic against parallelism: at 256 members the partials of a million rows are 1/256 of
 *   the rows read plus one row per cluster, and a database of a million rows in 256 clusters still makes 8 000 workgroups for the
 *   256 compute units; a longer segment would leave clusters of a few thousand rows to one or two workgroups each.
 * mdx_kmeans_finish.  sums [K, d] contiguous, previous [K, d] contiguous or NULL  ->  centroids [K, d] contiguous (may be sums, may be
 *   previous).  Per row: c = s / (||s||_2 + eps), the L2N rule of this library (eps is added to the norm).  A row whose elements are
 *   all zero (+0 or -0) takes previous[c, :], or +0 when previous is NULL.  One workgroup of 256 threads per row.  The order of the
 *   norm's sum: thread t runs ss = fma(v, v, ss) from +0 over the elements t, t + 256, ... in that order; a wave adds its 64 values by
 *   the butterfly v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1; the four wave sums are added as (w0 + w1) + (w2 + w3).  The square
 *   root, the addition of eps and the division are IEEE fp32, correctly rounded.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer (labels and best: both NULL), a
 * size < 1, m, K, n or d at or above 2^31, a launch of 2^31 workgroups or more ((ceil(n / SEGMENT) + K) ceil(d / 1024) for the sums,
 * K ceil(d / 256) for their chain), ld < K (argmax) or ld < d (sums), eps negative or NaN.  MDX_ERR_WORKSPACE for fewer bytes
 * than mdx_kmeans_sums_workspace says, or NULL (MDX_ERR_INVALID for a workspace that is not 16-byte aligned). */
#ifndef MDX_KMEANS_H
#define MDX_KMEANS_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* Members per segment of mdx_kmeans_sums: part of the definition of its result (ops.KMEANS_SEGMENT mirrors it). */
#define MDX_KMEANS_SEGMENT 256

int mdx_kmeans_argmax(const float *scores, int64_t m, int64_t K, int64_t ld, int64_t *labels, float *best, void *stream);
/* Bytes of device workspace of mdx_kmeans_sums: round_up(8 (K + 1), 256) + round_up(4 (ceil(n / MDX_KMEANS_SEGMENT) + K) round_up(d, 4),
 * 256); 0 for sizes the call refuses. */
int64_t mdx_kmeans_sums_workspace(int64_t n, int64_t K, int64_t d);
int mdx_kmeans_sums(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, const int64_t *offsets, int64_t K,
                    float *sums, void *workspace, int64_t workspace_bytes, void *stream);
int mdx_kmeans_finish(const float *sums, int64_t K, int64_t d, float eps, const float *previous, float *centroids, void *stream);

#endif /* MDX_KMEANS_H */
