/* mdx_overlap.h -- the overlap of two sets of top-K lists.  Included by mdx.h (section "top-K lists, overlap") after mdx_unet.h; include
 * mdx.h, not this file.  The prototype is apart from mdx.h's own for the reason given there under "exact kNN join" for mdx_knn_join.h;
 * its name is in _lib.OVERLAP_EXPORTS and its census is tests/test_overlap_host.py.
 *
 * What this is for.  An approximate search (mdir_amd/ivf.py, mdir_amd/ivfpq.py, search.search) returns a list of K ids per query; how
 * good it is, is how much of the exact list it holds: recall@depth.  That is a count of common ids per query and depth, and this call
 * is that count, for all queries and up to MDX_OVERLAP_MAX_DEPTHS depths at once.  tests/overlap_restatement.py restates it in numpy.
 *
 * Input.  a int64 [nq, ka] and b int64 [nq, kb], both contiguous: row q of each is a list of ids, best first.  The ids >= 0 of a row
 *   are distinct; -1 (any negative id) is padding and may stand anywhere.  1 <= ka, kb <= MDX_OVERLAP_MAX_K (= MDX_RESCORE_MAX_K, the
 *   limit of every search of the library).  depths: a HOST array of T int32, 1 <= T <= MDX_OVERLAP_MAX_DEPTHS, positive and ascending
 *   (depths[t] <= depths[t + 1]; equal neighbours are allowed).  It is read before the call returns.
 * Definition.  out int32 [nq, T], all of it written:
 *     out[q, t] = #{ i < min(depths[t], ka) : a[q, i] >= 0 and a[q, i] == b[q, j] for some j < min(depths[t], kb) }.
 *   An id at or above 2^31 is not compared: the kernel treats it as padding, in a and in b alike (the table keys are 32 bits), and the
 *   Python wrapper, ops.topk_overlap, refuses such lists.  A row with repeated ids gives an unspecified but memory-safe count for that
 *   row (each occurrence in a counts; which occurrence in b sets the depth is not defined).
 * Determinism.  Integer arithmetic only: the result is a count, and no order of the work can change a bit of it.
 *
 * Launch shape.  One workgroup of 256 threads per query.  The first min(depths[T - 1], kb) entries of b[q] go into an open-addressing
 *   table in LDS -- 32-bit keys, linear probing, at most half full (the smallest power of two >= 2 entries per key, at least 64
 *   slots, at most 8192: 32 KiB of keys and 16 KiB of 16-bit positions), filled with LDS compare-and-swap -- with the position j of
 *   every id beside it.  Every thread then looks up entries i of a[q]: a hit at (i, j) counts for depth t iff max(i, j) < depths[t].
 *   The per-thread counts are added across the wave by lane shuffles and across the four waves by LDS integer atomics; T threads
 *   store the row of out.  No atomics to global memory, nothing allocated, nothing read back: the call only enqueues on `stream` and
 *   is legal under stream capture.
 * Alignment: a and b 8 bytes, out 4.  No input makes the kernel read or write outside its buffers: it reads exactly the first
 *   min(depths[T - 1], ka) entries of every row of a and the first min(depths[T - 1], kb) of every row of b, and writes nq * T ints.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, "mdx_topk_overlap" in mdx_last_error): a NULL pointer; nq < 1 or nq at or above 2^31;
 * ka or kb outside [1, MDX_OVERLAP_MAX_K]; T outside [1, MDX_OVERLAP_MAX_DEPTHS]; a depth < 1 or below its predecessor; a pointer below
 * the alignment above. */
#ifndef MDX_OVERLAP_H
#define MDX_OVERLAP_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

#define MDX_OVERLAP_MAX_K 4096
#define MDX_OVERLAP_MAX_DEPTHS 8

int mdx_topk_overlap(const int64_t *a, int64_t ka, const int64_t *b, int64_t kb, int64_t nq, const int32_t *depths, int64_t T,
                     int32_t *out, void *stream);

#endif /* MDX_OVERLAP_H */
