/* mdx_refine.h -- int8 refinement of per-query shortlists on codes kept in list order.  Included by mdx.h (section "inverted file, int8
 * refinement of shortlists") after mdx_lists_edit.h; include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the
 * reason given there under "exact kNN join" for mdx_knn_join.h; their names are in _lib.REFINE_EXPORTS and their census is
 * tests/test_refine_host.py.
 *
 * What this is for.  An index of product-quantised lists (mdx_lists_pq.h; mdir_amd/ivfpq.py) ranks its candidates by ADC score, which
 * M bytes a row make coarse, and until now could only improve on that with the fp32 rows (mdx_rescore): all of the database back on the
 * device, and whole fp32 rows gathered per shortlist entry.  Here the index keeps, beside the PQ code of every position, the MDX_I8
 * quantisation of its row (mdx.h, mdx_storage) -- the storage mdx_lists_i8_encode writes, a quarter of the fp32 bytes, opaque payload to
 * mdx_lists_merge / mdx_lists_compact -- and a shortlist of ids is scored against it: mdx_refine_i8.  mdx_lists_i8_scan walks whole
 * lists through the plan; this call follows ids.  mdir_amd/ivfpq.py, IVFPQIndex(..., refine="i8"), is the caller;
 * tests/refine_restatement.py restates it in numpy.
 *
 * mdx_refine_i8.  Enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  d_pad = round_up(d, 64).
 *   codes     int8 [m, d_pad], 16-byte aligned (every row then is), scales fp32 [m]: the storage of mdx_lists_i8_encode, position p
 *             holding a row's codes, zeros in the columns d .. d_pad, and its scale
 *   where     int64 [n]: the position in [0, m) that holds id i; any value outside [0, m) means "id i is not stored"
 *   qcodes    int8 [nq, d] row-major at 1-byte alignment, qscales fp32 [nq]: mdx_quantize_i8 of the query rows x_q = q - center
 *             (mdx_center_rows, then mdx_quantize_i8)
 *   ids       int64 [nq, S], 1 <= S <= MDX_RESCORE_MAX_K
 *   score     for id in [0, n) with p = where[id] in [0, m):
 *                 (float)acc * (scales[p] * qscales[q]),    acc = sum_k qcodes[q, k] codes[p, k]  (int32, exact)
 *             two separately rounded products, nothing fused: the bits an MDX_I8 mdx_index of the rows gives mdx_scores at [q, id].
 *             For every other id NaN; neither `where` nor `codes` is dereferenced through an id outside [0, n), nor `codes` or
 *             `scales` through a position outside [0, m).
 *   out_ids   int64 [nq, S], out_scores fp32 [nq, S]: each query's pairs sorted exactly as mdx_rescore sorts its output -- by
 *             mdx_rank_full's key (larger score first, -0 == +0, NaN last), then by ascending id, then by position in the shortlist; so
 *             repeated padding ids are harmless (equal pairs, every order of them is the same bytes).  out_ids may equal ids.
 *   Each query's output bits depend on nothing but its own inputs (not on nq, not on the other queries).  Every other pointer needs the
 *   alignment of its element (4 for fp32, 8 for int64); the workspace 16 bytes.  No input makes a kernel read or write outside its
 *   buffers.
 * Launch shape.  Two launches.  The first is a gather, bound by bytes -- a query reads S (d_pad + 4) bytes from random places: a
 *   workgroup of four waves per (query, 64 shortlist entries), one wave per candidate, four candidates at a time: lane l loads the 16
 *   bytes k = 1024 j + 16 l .. + 15 of the row, and the loads of all four candidates are issued before the first is consumed.  The
 *   query's codes for a lane's k slices are loaded once per workgroup and stay in registers (d_pad / 1024 times four registers, for
 *   d_pad <= 4096; longer rows load their query pieces again slice by slice), zero-padded to d_pad, with 16-byte loads where d % 16 == 0
 *   and qcodes lies on the 16-byte grid and with byte loads otherwise: the same bits.  Four byte products per v_dot4 instruction; the
 *   per-lane int32 sums are added across the wave by shuffles -- integers, so no order can change a bit.  The unsorted scores go to
 *   the workspace.  The second launch is the per-query bitonic sort in LDS of mdx_rescore, the same kernel with the same key function.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer; n, m, d, nq or S < 1; S >
 * MDX_RESCORE_MAX_K; d > 133 120 (127^2 d_pad must stay below 2^31, as for MDX_I8); n, m or nq at or above 2^31; nq ceil(S / 64) at or
 * above 2^31; codes that are not 16-byte aligned.  MDX_ERR_WORKSPACE for a workspace of fewer bytes than mdx_refine_i8_workspace says,
 * or NULL. */
#ifndef MDX_REFINE_H
#define MDX_REFINE_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* round_up(4 nq S, 256) bytes (the unsorted scores); 0 for nq or S < 1 or S > MDX_RESCORE_MAX_K. */
int64_t mdx_refine_i8_workspace(int64_t nq, int64_t S);
int mdx_refine_i8(const int8_t *codes, const float *scales, int64_t m, int64_t d, const int64_t *where, int64_t n, const int8_t *qcodes,
                  const float *qscales, int64_t nq, const int64_t *ids, int64_t S, int64_t *out_ids, float *out_scores, void *workspace,
                  int64_t workspace_bytes, void *stream);

#endif /* MDX_REFINE_H */
