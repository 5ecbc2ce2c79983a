/* mdx_knn_reverse.h -- the reverse-edge merge of kNN lists.  Included by mdx.h (section "kNN lists, reverse-edge merge") after
 * mdx_refine.h; include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under "exact kNN
 * join" for mdx_knn_join.h; their names are in _lib.KNN_REVERSE_EXPORTS and their census is tests/test_knn_reverse_host.py.
 *
 * What this is for.  A kNN join through the inverted file (mdir_amd/ivf.py, IVFIndex.knn_join) finds, for row i, the best rows among
 * the lists i probes.  The exact chain is symmetric to the bit -- one fmaf chain over ascending k, and fmaf(a, b, c) == fmaf(b, a, c)
 * -- so where i found j but the probes of j never reached the list of i, the pair (i, score) can be offered to j without scoring
 * anything.  These three calls do that for all rows at once.  tests/knn_reverse_restatement.py restates them in numpy.
 *
 * Input.  ids int64 [n, k] and scores fp32 [n, k], both contiguous: row j is a neighbour list in mdx_rank_full's order -- larger score
 *   first, -0 == +0, NaN last, equal keys by ascending id -- whose tail may be padding, id -1.  Ids within a row are distinct.
 *   1 <= k <= MDX_KNN_REVERSE_MAX_K and n < 2^31.
 * Definition.  The edges are E = {(i, j, s) : j = ids[i, r], 0 <= j < n, j != i, s = scores[i, r]}.  The offers to j are
 *   O_j = {(i, s) : (i, j, s) in E and i not in ids[j, :]}.  Output row j is the first k entries, by (order key, id), of its own valid
 *   entries together with O_j, padded with id -1 / score NaN; gained[j] counts how many of them came from O_j.  Every output score is
 *   the bit pattern of the input entry it came from (a -0 stays -0, a NaN keeps its payload).
 *   An id outside [0, n) is never dereferenced: it is neither offered nor an offer target, and in its own row it is treated as padding
 *   wherever it stands.  A row with repeated ids, or one that is not in order, gives an unspecified but memory-safe result.  That
 *   score(i, j) == score(j, i) is the caller's premise: nothing here checks it.
 * Determinism.  A result row is the k smallest of a set of distinct (order key, id) pairs, so the order in which offers arrive in the
 *   offer buffer cannot change a byte: two runs are equal.  Only integer atomics are used, on the per-row counters.
 *
 * The three calls.  All are enqueued on `stream`, allocate nothing and read nothing back (legal under stream capture).  Between the
 * first and the second the caller turns counts into offsets: offsets int64 [n + 1], offsets[0] = 0, offsets[j + 1] = offsets[j] +
 * counts[j] (one prefix sum).
 *   mdx_knn_reverse_count   counts int32 [n], all of it written: counts[j] = the offers to j that can enter its row.  An offer that
 *             does not precede the k-th own entry of a row without padding cannot, and is dropped here; so is an edge whose source is
 *             a member of ids[j, :].  Eight lanes per edge; together they read row j of ids once, 64 contiguous bytes a step, and the
 *             first of them makes one integer atomic add on counts[j].  One counter per target row is contended only for hubs, and
 *             the drop keeps even those short.
 *   mdx_knn_reverse_fill    the same tests; the slot of an offer is offsets[j] plus an integer atomic ticket on cursor[j] (int32 [n],
 *             workspace: zeroed by the call).  An offer is 8 bytes -- the score's bits, then the source id as int32 -- written by one
 *             8-byte vector store.  offers holds `capacity` offers; n k is always enough, so nothing has to be read back to size it.
 *             The call never writes at or beyond `capacity`, whatever offsets holds.
 *   mdx_knn_reverse_merge   one wave per row.  The row's valid entries are kept, up to two per lane, as a sorted list in LDS; its
 *             segment offers[offsets[j] .. offsets[j + 1]) (clamped to [0, capacity]) is streamed 64 offers at a time; a tile is
 *             filtered against the current k-th entry and merged by rank counting.  A segment of any length works.  out_ids int64
 *             [n, k], out_scores fp32 [n, k], gained int32 [n]; the outputs do not overlap the inputs.
 * Alignment: every pointer that of its element -- 8 bytes for ids, offsets, offers and out_ids, 4 for scores, counts, cursor,
 * out_scores and gained.  No input makes a kernel read or write outside its buffers.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer; n or k < 1; k >
 * MDX_KNN_REVERSE_MAX_K; n at or above 2^31; n k at or above 2^31; a capacity < 1; a pointer below the alignment above. */
#ifndef MDX_KNN_REVERSE_H
#define MDX_KNN_REVERSE_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_KNN_REVERSE_MAX_K 128

int mdx_knn_reverse_count(const int64_t *ids, const float *scores, int64_t n, int64_t k, int32_t *counts, void *stream);
int mdx_knn_reverse_fill(const int64_t *ids, const float *scores, int64_t n, int64_t k, const int64_t *offsets, int32_t *cursor,
                         void *offers, int64_t capacity, void *stream);
int mdx_knn_reverse_merge(const int64_t *ids, const float *scores, int64_t n, int64_t k, const int64_t *offsets, const void *offers,
                          int64_t capacity, int64_t *out_ids, float *out_scores, int32_t *gained, void *stream);

#endif /* MDX_KNN_REVERSE_H */
