"""Editing the lists of the inverted file (include/mdx_lists_edit.h; IVFPQIndex.add / .remove of mdir_amd/ivfpq.py) restated in numpy (a
helper module, imported by test_lists_edit_host.py, test_gpu_lists_edit.py and test_gpu_lists_edit_memcontract.py; no GPU).

A list-ordered structure is ``(rows, members, offsets)``: ``rows`` uint8 ``[m, width]`` (opaque payload), ``members`` int64 ``[m]``,
``offsets`` int64 ``[K + 1]``.

``merge``      per list the rows of ``a`` followed by those of ``b``; the offsets of each are clamped to its ``[0, m]``
``compact``    the positions that are kept, in their order; ``offsets`` becomes ``kept[offsets]``
``prefix``     the exclusive prefix sum ``kept`` of keep flags
``remove``     the structure without the members named by ``ids``, and how many left
"""
import numpy as np

from ivf_restatement import clamped


def merge(a_rows, a_members, a_offsets, b_rows, b_members, b_offsets):
    """(rows, members, offsets) of ``ma + mb`` rows: ``offsets[l] = clamp(a_offsets[l], ma) + clamp(b_offsets[l], mb)``, list ``l`` is
    list ``l`` of ``a`` then list ``l`` of ``b``.  (Offsets that ascend from 0 to m: every position of the result is covered.)"""
    a_rows, b_rows = np.asarray(a_rows, np.uint8), np.asarray(b_rows, np.uint8)
    a_members, b_members = np.asarray(a_members, np.int64), np.asarray(b_members, np.int64)
    ma, mb = len(a_members), len(b_members)
    (a0, an), (b0, bn) = clamped(a_offsets, ma), clamped(b_offsets, mb)
    rows, members = [np.empty((0, a_rows.shape[1]), np.uint8)], [np.empty(0, np.int64)]
    for l in range(len(an)):
        rows += [a_rows[a0[l]:a0[l] + an[l]], b_rows[b0[l]:b0[l] + bn[l]]]
        members += [a_members[a0[l]:a0[l] + an[l]], b_members[b0[l]:b0[l] + bn[l]]]
    offsets = np.clip(np.asarray(a_offsets, np.int64), 0, ma) + np.clip(np.asarray(b_offsets, np.int64), 0, mb)
    return np.concatenate(rows), np.concatenate(members), offsets


def prefix(keep):
    """int64 [m + 1]: the number of kept positions before every position, and their total."""
    kept = np.zeros(len(keep) + 1, np.int64)
    kept[1:] = np.cumsum(np.asarray(keep, bool))
    return kept


def compact(rows, members, offsets, kept):
    """(rows, members, offsets): position ``p`` stays exactly when ``kept[p + 1] > kept[p]`` and goes to ``kept[p]``; ``offsets[l] =
    kept[clamp(offsets[l], m)]``."""
    rows, members, kept = np.asarray(rows, np.uint8), np.asarray(members, np.int64), np.asarray(kept, np.int64)
    keep = kept[1:] > kept[:-1]
    return rows[keep], members[keep], kept[np.clip(np.asarray(offsets, np.int64), 0, len(members))]


def remove(rows, members, offsets, ids):
    """((rows, members, offsets), removed): the structure without the positions whose member is among ``ids``."""
    keep = ~np.isin(np.asarray(members, np.int64), np.asarray(ids, np.int64))
    return compact(rows, members, offsets, prefix(keep)), int((~keep).sum())
