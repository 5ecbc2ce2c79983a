/* mdx_lists_i8.h -- int8 list storage for the inverted file, with exact rescoring.  Included by mdx.h (section "inverted file, int8
 * lists") after mdx_ivf.h; include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under
 * "exact kNN join" for mdx_knn_join.h; their names are in _lib.LISTS_I8_EXPORTS and their census is tests/test_lists_i8_host.py.
 *
 * What this is for.  mdx_ivf_scan (mdx_ivf.h) gathers whole fp32 rows through `members`.  Here the rows of the lists are kept a second
 * time as MDX_I8 codes (mdx.h, mdx_storage) IN LIST ORDER: position p of `codes` holds the quantisation of row members[p], so a tile
 * of a list is one contiguous run of a quarter of the bytes, and the first stage of a search multiplies it on v_mfma_i32_16x16x64_i8.
 * The plan (mdx_ivf_plan), the work items, the candidate row and the selection (mdx_ivf_select) are those of mdx_ivf.h, unchanged;
 * the second stage is mdx_rescore on the fp32 rows and its certificate mdx_rescore_certify (mdx.h).  mdir_amd/ivf.py,
 * IVFIndex(..., storage="i8"), puts them together; tests/test_lists_i8_host.py restates the search in numpy.
 *
 * Common to every call: enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture).  d_pad =
 * round_up(d, 64).  `codes` is int8 [m, d_pad] and must be 16-byte aligned (every row then is: d_pad is a multiple of 64); every other
 * pointer needs the alignment of its element (1 byte for qcodes, 4 for fp32, 8 for int64 and for mdx_i8_bounds); the plan 16 bytes.
 * No input makes a kernel read or write outside its buffers, as in mdx_ivf.h.
 *
 * mdx_lists_i8_encode.  rows fp32 [n, d] at row stride ld, members int64 [m]  ->  codes int8 [m, d_pad], scales fp32 [m]: position p
 *   holds the MDX_I8 quantisation of row members[p] -- the bits mdx_quantize_i8 gives for that row (one definition of the arithmetic,
 *   csrc/mdx_i8_quant.h) -- and zeros in the columns d .. d_pad.  One wave per position: the absmax (order-free), then 16 codes per
 *   lane and store.  `rows` is read in place, with 16-byte loads where ld % 4 == 0 and the base lies on the 16-byte grid and with
 *   dword loads otherwise: the same bits.  A member id outside [0, n) is never dereferenced: its position gets zero codes and a NaN
 *   scale, so every score against it is NaN, as in the fp32 scan.
 * mdx_lists_i8_bounds.  codes, scales  ->  the mdx_i8_bounds (mdx.h) of this storage: s_max, s_min, l_max, flag, by the same order-free
 *   reductions as mdx_index_i8_bounds (integer max / min of the bit patterns of non-negative doubles, an or): for valid members the
 *   values of an MDX_I8 mdx_index of the same rows, to the bit.  A non-finite scale (an infinite element, or a member id outside
 *   [0, n)) sets flag, as does 0 < scale < 2^-106.  Two launches.
 * mdx_lists_i8_scan.  The first stage.  qcodes int8 [nq, d] row-major and qscales fp32 [nq] are mdx_quantize_i8 of the query rows x_q
 *   = q - center (mdx_center_rows, then mdx_quantize_i8).  `plan` is mdx_ivf_plan's of the same probes, offsets, m and cap; the work
 *   items are those of mdx_ivf_scan: a tile of MDX_IVF_TILE members of one list times a group of up to MDX_IVF_QUERY_GROUP entries;
 *   `items` and `cap` have the meaning they have there, and so have the outputs cand_scores / cand_ids [nq, cap] and the second launch
 *   (NaN / -1 at or beyond count[q]).
 *     cand_scores[q, col] = (float)acc * (scale_member * scale_q),    acc = sum_k c_q,k c_member,k  (int32, exact)
 *   two separately rounded products, nothing fused: the bits an MDX_I8 mdx_index of the rows gives mdx_scores at [q, id].
 *   One workgroup of four waves per work item, each wave 16 members.  The A operand of v_mfma_i32_16x16x64_i8 comes straight from the
 *   contiguous code tile in global memory: lane (g, j) loads the 16 bytes k = 64 kb + 16 g .. + 15 of member j, the k map of
 *   csrc/mdx_scores_i8_kernel.h.  The B operand is the group's query codes, staged in LDS 1024 k at a time, zero-padded to 16 columns
 *   and to d_pad (16-byte loads where d % 16 == 0 and qcodes lies on the 16-byte grid, byte loads otherwise: the same bits).  One MFMA
 *   covers 64 k; the int32 sums are exact, so no order of the k terms can change a bit.  The scales are applied in the epilogue.
 *   Everything read from the plan is range-checked before it is used as an index, as in mdx_ivf_scan.
 *
 * The contract of the two-stage search (mdir_amd/ivf.py, IVFIndex.search on storage="i8" with shortlist=S, k <= S <=
 * MDX_RESCORE_MAX_K): select S candidates by int8 score (mdx_ivf_select), rescore them (mdx_rescore), certify (mdx_rescore_certify
 * with t_q = the S-th int8 score and the bounds of mdx_lists_i8_bounds), return the first k.
 *   The first certified[q] entries of the result are, bit for bit (ids and scores), the first entries of the fp32 search of the same
 *   index -- mdx_ivf_scan and mdx_ivf_select on the same probes.  With exact=True the whole result is.
 * Proof.  It is the proof under mdx_rescore_certify (mdx.h) with "the database" read as C_q, the union of the lists query q probes
 * (its candidates), for which the fp32 search is the exact ranking:
 *   - S_max and L_max are maxima over all rows, so they bound the scale and scale ||c||_1 of every row of the subset C_q; the MDX_I8
 *     bound and the chain bound of that proof are per pair and hold for every row of C_q as they stand;
 *   - every candidate outside the shortlist ranks after it in the int8 order of mdx_ivf_select (larger score first, NaN last), so its
 *     int8 score is <= t_q, or NaN.  An int8 score is NaN only for a member id outside [0, n) (NaN scale), whose chain score is NaN
 *     too and ranks after every number; rows of the int8 contract have a finite score;
 *   hence chain_i <= U_q for every unshortlisted candidate whose chain score is a number, and the leading entries of the rescored
 *   shortlist with score > U_q precede every other candidate in the exact order.  mdx_rescore sorts by that order (key, then id), as
 *   mdx_ivf_select does, so those entries are the first entries of the fp32 search.
 *   Where scanned[q] <= S every candidate is in the shortlist: certified[q] = S, and the row is the fp32 search's whole row -- the
 *   padding included.  The shortlist's tail is padding, id -1.  mdx_rescore (csrc/mdx_rescore.hip) never dereferences an id outside
 *   [0, n), scores it NaN and sorts by (key, id, position in the shortlist): REPEATED padding ids are harmless -- they are equal
 *   pairs, every order of them is the same bytes, and none is read.  With id -1 they would sort before a candidate whose chain score
 *   is NaN (a row holding a NaN), where mdx_ivf_select has its padding behind every candidate; so the host hands them to mdx_rescore
 *   as the id n, which sorts behind every candidate, and writes -1 back.
 *   exact=True runs the queries with certified[q] < k again through mdx_ivf_scan / mdx_ivf_select on the fp32 rows: their rows are the
 *   fp32 search's by construction, the others' first k <= certified[q] entries by the certificate.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer; n, m, d, nq, nprobe, K, cap or
 * items < 1; d > 133 120 (127^2 d_pad must stay below 2^31, as for MDX_I8); n, m, nq, K or cap at or above 2^31, nq nprobe or items
 * at or above 2^31, nq ceil(cap / 1024) at or above 2^31; nprobe > K; ld < d; n ld beyond int64; codes that are not 16-byte aligned; a
 * plan that is not 16-byte aligned.  MDX_ERR_WORKSPACE for a plan of fewer bytes than mdx_ivf_plan_workspace says, or NULL. */
#ifndef MDX_LISTS_I8_H
#define MDX_LISTS_I8_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

int mdx_lists_i8_encode(const float *rows, int64_t n, int64_t d, int64_t ld, const int64_t *members, int64_t m, int8_t *codes,
                        float *scales, void *stream);
int mdx_lists_i8_bounds(const int8_t *codes, const float *scales, int64_t m, int64_t d, mdx_i8_bounds *bounds, void *stream);
int mdx_lists_i8_scan(const int8_t *codes, const float *scales, int64_t m, int64_t d, const int64_t *members, const int64_t *offsets,
                      int64_t K, const int8_t *qcodes, const float *qscales, int64_t nq, int64_t nprobe, const void *plan,
                      int64_t plan_bytes, int64_t cap, int64_t items, float *cand_scores, int64_t *cand_ids, void *stream);

#endif /* MDX_LISTS_I8_H */
