/* mdx_lists_edit.h -- editing the lists of the inverted file after the build: the merge of two list-ordered structures (adding a
 * batch of rows) and the compaction of one (removing rows).  Included by mdx.h (section "inverted file, editing the lists") after
 * mdx_lists_pq.h; include mdx.h, not this file.  The prototypes are apart from mdx.h's own for the reason given there under "exact kNN
 * join" for mdx_knn_join.h; their names are in _lib.LISTS_EDIT_EXPORTS and their census is tests/test_lists_edit_host.py.
 *
 * What this is for.  An index that stores its rows in list order (mdir_amd/ivfpq.py: M bytes of code and an id per row) is a
 * "list-ordered structure" of three parts:
 *     rows     m payload rows of `width` bytes at a row stride of `ld` >= width bytes (a buffer of m ld bytes)
 *     members  int64 [m]: the id of the row at every position
 *     offsets  int64 [K + 1]: list l holds the positions offsets[l] .. offsets[l + 1]
 * The payload is opaque bytes: nothing here interprets it (PQ codes today; int8 codes or scales as well).  A list's members ascend in
 * id and a batch of new rows gets ids above all old ones, so the batch -- sorted by list -- is a second such structure, and adding it
 * is, per list, the concatenation of the two: mdx_lists_merge.  Removing rows keeps the order of what stays: mdx_lists_compact, driven
 * by the exclusive prefix sum of the keep flags.  tests/lists_edit_restatement.py restates both in numpy; mdir_amd/ivfpq.py
 * (IVFPQIndex.add, IVFPQIndex.remove) is the caller.
 *
 * Common to both calls: enqueued on `stream`, nothing allocated, nothing read back (legal under stream capture), no workspace and
 * no [m]-sized temporary.  Two launches each: a small one writes out_offsets, the second moves rows and members gather-wise in one pass.
 * Every pointer needs the alignment of its element (1 byte for rows, 8 for int64).  Offsets are clamped to [0, m] (m = ma, mb) as in
 * the other list headers, and a list whose clamped end lies before its clamped start is empty.  No input makes a kernel read or write
 * outside its buffers: a destination position that no list covers, or whose source would lie outside [0, m), is left unwritten, and
 * with offsets that ascend from 0 to m there is no such position.  The bytes width .. ld of an input row may be read and are
 * never interpreted; the bytes width .. out_ld of an output row are left untouched.  Loads and stores are 16-byte where `width`,
 * every stride and every base are multiples of 16, dword where that holds for 4, byte otherwise (the stride and base of a structure
 * of no rows do not count): all three give the same bits.
 * Launch shape: a thread owns one piece (16, 4 or 1 bytes) of one destination row (merge) or source row (compaction), pieces
 * numbered row-major, so consecutive lanes own consecutive pieces of consecutive rows and -- where out_ld == width -- a wave writes one
 * contiguous run.  A workgroup of 256 threads takes a span of MDX_LISTS_EDIT_SPAN pieces at a time, four per thread with the loads
 * ahead of the stores; at most MDX_LISTS_EDIT_GROUPS workgroups stride over the spans.
 *
 * mdx_lists_merge.  Structures a (ma rows) and b (mb rows) over the same K lists and of the same width; ma or mb may be 0, not both
 * (the rows and members pointers of a structure of no rows are not NULL all the same; they are never dereferenced).  Outputs:
 * out_rows [ma + mb] rows at the stride out_ld, out_members int64 [ma + mb], out_offsets int64 [K + 1]:
 *     out_offsets[l] = clamp(a_offsets[l], ma) + clamp(b_offsets[l], mb)
 *     list l of the output is list l of a followed by list l of b, rows and members moved together.
 *   A destination position p finds its list by a binary search of out_offsets (the last l with out_offsets[l] <= p < out_offsets[l +
 *   1]), its index i = p - out_offsets[l] there, and reads position a_start(l) + i of a where i < a_size(l), position b_start(l) + i -
 *   a_size(l) of b otherwise.
 * mdx_lists_compact.  One structure of m rows and `kept` int64 [m + 1], the exclusive prefix sum of the keep flags: kept[p] is the
 * number of kept positions before p, and position p is kept exactly when kept[p + 1] > kept[p].  Outputs: out_rows `mo` rows at the
 * stride out_ld, out_members int64 [mo], out_offsets int64 [K + 1]; mo is what the caller allocated, kept[m] where it knows it:
 *     position p, where kept, goes to position kept[p] (a destination outside [0, mo) is not written)
 *     out_offsets[l] = clamp(kept[clamp(offsets[l], m)], mo)
 *   The order inside a list is unchanged; positions outside every list move like the others.
 *
 * Refusals (MDX_ERR_INVALID, nothing launched, the call's name in mdx_last_error): a NULL pointer; K, width, ma + mb, m or mo < 1; a
 * negative ma or mb; a stride below width; K, width, a stride, ma + mb, m or mo at or above 2^31 (so every m ld product stays inside
 * int64); an output pointer equal to an input pointer or to another output pointer. */
#ifndef MDX_LISTS_EDIT_H
#define MDX_LISTS_EDIT_H

#ifndef MDX_H
#error "include mdx.h: it includes this file"
#endif

/* The pieces a workgroup of 256 threads moves at a time, and the workgroups a launch has at most. */
#define MDX_LISTS_EDIT_SPAN 1024
#define MDX_LISTS_EDIT_GROUPS 2048

int mdx_lists_merge(const uint8_t *a_rows, int64_t a_ld, const int64_t *a_members, const int64_t *a_offsets, int64_t ma,
                    const uint8_t *b_rows, int64_t b_ld, const int64_t *b_members, const int64_t *b_offsets, int64_t mb, int64_t K,
                    int64_t width, uint8_t *out_rows, int64_t out_ld, int64_t *out_members, int64_t *out_offsets, void *stream);
int mdx_lists_compact(const uint8_t *rows, int64_t ld, const int64_t *members, const int64_t *offsets, int64_t m, int64_t K, int64_t width,
                      const int64_t *kept, int64_t mo, uint8_t *out_rows, int64_t out_ld, int64_t *out_members, int64_t *out_offsets,
                      void *stream);

#endif /* MDX_LISTS_EDIT_H */
