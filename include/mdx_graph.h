/* mdx_graph.h -- a graph index: beam search over a fixed-degree neighbour graph of the database, and the detour counts that prune a kNN
 * graph into a search graph.  Included by mdx.h (section "graph index") after mdx_overlap.h; include mdx.h, not this file.  The prototypes
 * are apart from mdx.h's own for the reason given there under "exact kNN join" for mdx_knn_join.h; their names are in _lib.GRAPH_EXPORTS
 * and their census is tests/test_graph_host.py.  tests/graph_restatement.py restates both calls in numpy; mdir_amd/graph.py (GraphIndex)
 * is the index built on them.
 *
 * ---------------------------------------------------------------------------------------------------------------- mdx_graph_search
 *
 * Input.  rows fp32 [n, d] at stride ld >= d, read in place, 1 <= n < 2^31, 1 <= d <= MDX_GRAPH_MAX_D.  graph int32 [n, R] contiguous,
 *   1 <= R <= MDX_GRAPH_MAX_DEGREE: row i holds the neighbours of row i; an entry < 0 or >= n is padding and is never dereferenced;
 *   repeats and self loops are allowed.  queries fp32 under `qlayout` (either mdx_layout), nq of them, with an optional center [d]:
 *   x_q = q - center, one fp32 subtraction, as in mdx_rescore.  seeds int64 [nq, S], 1 <= S <= MDX_GRAPH_MAX_SEEDS: invalid ids (< 0 or
 *   >= n) are ignored and repeats collapse.  The beam length L (k <= L <= MDX_GRAPH_MAX_BEAM), the parents per step W (1 <= W <=
 *   MDX_GRAPH_MAX_WIDTH, so W * R <= MDX_GRAPH_MAX_CANDIDATES = 8 * 64), the step limit T >= 1, and table_bits: 0 for a default, else 8 .. 14.
 * Score.  score(q, id) is the exact chain of mdx_rescore: the bits of mdx_scores on an fp32 index of `rows` at [q, id] (k ascending,
 *   fmaf from +0, continued over zeros to round_up(d, 64); the device functions of mdx_exact.h).  Such a score is never -0.
 * Order.  mdx_rank_full's: larger score first, -0 == +0, NaN last, equal scores by ascending id.
 * Definition (sequential; restated in tests/graph_restatement.py, graph_search).  The beam is a list of at most L distinct ids in the
 *   order, each with an `expanded` flag.  It starts as the first L of the distinct valid seeds in the order, none expanded.  One step:
 *     1. the parents are the first W unexpanded entries of the beam in beam order; if there are none, stop;
 *     2. the parents are marked expanded and `steps` grows by 1;
 *     3. the candidates are the distinct valid ids in the parents' graph rows that are not in the beam;
 *     4. they are scored;
 *     5. the beam becomes the first L of beam U candidates in the order; surviving entries keep their flag.
 *   Stop after T steps.
 * Output, all of it written: ids int64 [nq, k] and scores fp32 [nq, k], the first k of the beam, padded with -1 and NaN; steps int32 [nq];
 *   scored int32 [nq], the chains the query ran (a diagnostic).  A score that is NaN is returned as the quiet NaN 0x7FC00000; every
 *   other score has the chain's bits.  Each query's outputs depend on nothing but its own inputs.
 *
 * A visited-row table cannot change the result.  The L-th entry of the beam only ever improves under step 5, so a row that was scored
 *   and rejected or evicted can never enter again: scoring it again gives the same bits and the same rejection.  A table of rows
 *   already scored is therefore a pure optimisation.  The kernel keeps an open-addressing table of 2^table_bits 32-bit keys in LDS; a
 *   candidate found there is not scored.  The table is cleared at the start of a step when it is more than half full, and an insert
 *   that finds no free slot within 32 probes is given up (the candidate is scored and not remembered).  No table size and no clearing
 *   changes a bit of ids, scores or steps; only `scored` depends on it, and scored <= S + steps * W * R always.
 *   What is exact is the test "already in the beam, or twice among this step's candidates": the scored candidates are sorted together
 *   with the beam by (order key, id, unexpanded), copies of one id have one key and end up adjacent, and all but the first -- the
 *   expanded one, if the beam held the id -- are dropped before the first L are taken.  A duplicate never reaches the beam.
 *
 * Launch shape.  One workgroup of 256 threads per query, one launch.  Per round (the seeds in chunks, then one round per step): the
 *   candidates are filtered through the table, one lane runs the chain of one candidate on all four waves (the row read in place in
 *   16-byte pieces where ld % 4 == 0 and rows is 16-byte aligned, the centred query resident in LDS), and the beam and the scored
 *   candidates are sorted by a bitonic network of P = the smallest power of two >= L + W * R words of 64 bits.  Dynamic LDS, a function of
 *   (d, L, W * R, table_bits) and not of the maxima:   4 * round_up(d, 64)  +  8 * P  +  8 * (P - L)  +  4 * 2^table_bits  +  64 bytes
 *   -- 13.6 KiB at d = 2048, L = 64, W * R = 32 and the default table_bits, at most 112.1 KiB.  The default table_bits is the smallest in
 *   8 .. 13 with 2^table_bits >= 8 * (L + W * R).  Nothing is allocated, nothing is read back, no global atomics: the call only enqueues
 *   on `stream` and is legal under stream capture.
 * Alignment: seeds and ids 8 bytes, everything else 4.  No input makes the kernel read or write outside its buffers: of rows it reads
 *   only rows with ids in [0, n), of graph only rows of beam members.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, "mdx_graph_search" in mdx_last_error): a NULL pointer (center may be NULL); n or nq
 *   outside [1, 2^31); d outside [1, MDX_GRAPH_MAX_D]; ld < d; an unknown layout; R, S, L, W, T or k out of the ranges above;
 *   a table_bits outside {0, 8 .. 14}; a pointer below the alignment above.
 *
 * --------------------------------------------------------------------------------------------------------------- mdx_graph_detours
 *
 * A plain kNN graph is a poor search graph: its edges crowd into the nearest clump.  The rank-based pruning of CAGRA counts, for every
 * edge i -> b, the two-edge walks i -> a -> b whose edges both rank before it; edges with few such detours are kept.  Integers only.
 *
 * Input.  lists int64 [n, K0] contiguous, 1 <= n < 2^31, 1 <= K0 <= MDX_GRAPH_MAX_K0: neighbour lists, best first, the row's own id
 *   removed; an entry < 0 or >= n is padding; the valid ids of a row are distinct.
 * Definition.  detours int32 [n, K0], all of it written.  For a valid b = lists[i, j]:
 *     detours[i, j] = #{ t < j : a = lists[i, t] is valid and lists[a, r] == b for some r < j };
 *   for an invalid entry detours[i, j] = K0, which sorts after every real count.  A row with repeated ids gives an unspecified but
 *   memory-safe count for that row and for the rows that list it.
 * Launch shape.  One workgroup of 256 threads per row: the row's list goes into an open-addressing table in LDS (256 slots of 32-bit
 *   keys, at most half full, LDS compare-and-swap) with the rank of every id; each wave streams the lists of every fourth neighbour
 *   through it (K0^2 look-ups a row, n * K0^2 * 8 bytes of gathered reads: the cost of the call) and counts into LDS with integer
 *   atomics.  No global atomics, nothing allocated, nothing read back; legal under stream capture.  Alignment: lists 8, detours 4.
 * Refusals (MDX_ERR_INVALID, nothing launched, "mdx_graph_detours" in mdx_last_error): a NULL pointer; n outside [1, 2^31); K0 outside
 *   [1, MDX_GRAPH_MAX_K0]; a pointer below the alignment above. */
#ifndef MDX_GRAPH_H
#define MDX_GRAPH_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_GRAPH_MAX_D 8192
#define MDX_GRAPH_MAX_DEGREE 64
#define MDX_GRAPH_MAX_SEEDS 512
#define MDX_GRAPH_MAX_BEAM 512
#define MDX_GRAPH_MAX_WIDTH 8
#define MDX_GRAPH_MAX_CANDIDATES 512
#define MDX_GRAPH_MAX_K0 128

int mdx_graph_search(const float *rows, int64_t n, int64_t d, int64_t ld, const int32_t *graph, int64_t R, const float *queries, int64_t nq,
                     int qlayout, const float *center, const int64_t *seeds, int64_t S, int64_t k, int64_t L, int64_t W, int64_t T,
                     int table_bits, int64_t *ids, float *scores, int32_t *steps, int32_t *scored, void *stream);

int mdx_graph_detours(const int64_t *lists, int64_t n, int64_t K0, int32_t *detours, void *stream);

#endif /* MDX_GRAPH_H */
