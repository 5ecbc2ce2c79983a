"""The int8 refinement of shortlists (include/mdx_refine.h; mdir_amd/ivfpq.py, refine="i8") restated in numpy (a helper module, imported
by test_refine_host.py, test_gpu_refine.py, test_gpu_ivfpq_refine.py and test_gpu_refine_memcontract.py; no GPU).

Nothing here is new arithmetic: the storage is lists_i8_restatement.encode, the int8 scores are test_i8_host.quantize_np / scores_np,
the ADC shortlist is pq_restatement.search, the order is test_rescore_host.rank_order and the exact chain is oracle/chain.c (through
pq_restatement.chain, which continues it to a multiple of 64 as the library does).  What this module states is how they are put
together.

``where_of``    the inverse of ``members``
``refine``      mdx_refine_i8: per query the (ids, scores) of its shortlist, sorted
``search``      IVFPQIndex.search on a refine="i8" index with a shortlist: the refined row, or the exact row of its first ``rescore``
"""
import numpy as np

import lists_i8_restatement as LI
import pq_restatement as PR
from test_i8_host import quantize_np, scores_np
from test_rescore_host import rank_order

F32 = np.float32


def where_of(members, n):
    """int64 [n]: the position that holds id i, -1 for an id that no position holds (members outside [0, n) hold none)."""
    members = np.asarray(members, np.int64)
    where = np.full(n, -1, np.int64)
    ok = (members >= 0) & (members < n)
    where[members[ok]] = np.flatnonzero(ok)
    return where


def refine(codes, scales, d, where, qcodes, qscales, ids):
    """(ids int64 [nq, S], scores fp32 [nq, S]) of mdx_refine_i8: an id in [0, n) whose position where[id] lies in [0, m) scores as the
    int8 contract says, every other id NaN; sorted by (desc_key, id, position in the shortlist)."""
    codes, scales, where, ids = np.asarray(codes), np.asarray(scales, F32), np.asarray(where, np.int64), np.asarray(ids, np.int64)
    m, n = len(scales), len(where)
    out_ids, out_sc = np.empty(ids.shape, np.int64), np.empty(ids.shape, F32)
    for q, row in enumerate(ids):
        ok = (row >= 0) & (row < n)
        pos = np.full(len(row), -1, np.int64)
        pos[ok] = where[row[ok]]
        ok = (pos >= 0) & (pos < m)
        sc = np.full(len(row), np.nan, F32)
        with np.errstate(invalid="ignore"):
            sc[ok] = scores_np(qcodes[q:q + 1], qscales[q:q + 1], codes[pos[ok], :d], scales[pos[ok]])[0]
        out_ids[q], out_sc[q] = rank_order(sc, row)          # lexsort is stable: equal (key, id) pairs stay in shortlist order
    return out_ids, out_sc


def search(pq_codes, members, n, offsets, table, coarse, probes, fine_codes, fine_scales, queries, k, shortlist, rescore=None, center=None,
           rows=None):
    """(ids int64 [nq, k], scores fp32 [nq, k], scanned int64 [nq]) of IVFPQIndex.search(queries, k, nprobe, center=center,
    shortlist=shortlist, rescore=rescore) on a refine="i8" index: ``pq_codes``, ``members``, ``offsets`` its structure, ``n`` its id bound,
    ``fine_codes`` / ``fine_scales`` its refinement payload, ``table`` / ``coarse`` / ``probes`` of pq_restatement; ``queries`` fp32 [nq, d];
    ``rows`` fp32 [n, d] (for ``rescore``): the row of every id."""
    d = np.asarray(queries).shape[1]
    short, _, scanned = PR.search(pq_codes, members, n, offsets, table, coarse, probes, shortlist)
    qcodes, qscales = quantize_np(LI.centred(queries, center))
    ids, sc = refine(fine_codes, fine_scales, d, where_of(members, n), qcodes, qscales, np.where(short < 0, n, short))
    if rescore is not None:
        exact = PR.chain(LI.centred(queries, center), np.ascontiguousarray(rows, F32))
        for q in range(len(ids)):
            head = ids[q, :rescore]
            ok = head < n                                       # the padding n: NaN, behind every candidate
            chain_sc = np.full(rescore, np.nan, F32)
            chain_sc[ok] = exact[q, head[ok]]
            ids[q, :rescore], sc[q, :rescore] = rank_order(chain_sc, head)
    ids = np.where(ids >= n, -1, ids)
    return np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(sc[:, :k]), scanned
