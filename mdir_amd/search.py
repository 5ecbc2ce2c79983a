"""Two-stage search: a compressed first stage, an exact second stage and a certificate.

``search(index, rows, queries, k, shortlist)`` runs

    index.scores(queries)               int8 (or fp16) scores of every row       (mdx_scores)
    topk(scores, K)                     the shortlist, K = min(shortlist, N)     (mdx_topk)
    rescore(rows, queries, ids)         exact fp32 chain scores of the K rows    (mdx_rescore)
    rescore_certify(...)                int8 only: the certified depth per query (mdx_rescore_certify)

and returns the first k rescored entries per query.  For an int8 index, ``certified[q]`` is a depth up to which the result
is provably the exact fp32 top-k, bit for bit (``include/mdx.h`` states the proof).  An fp16 first stage has no
certificate.  With ``exact=True``, every query whose certified depth is below k (every query of an fp16 index) is run
again through the exact path, ``scores_rowmajor`` + ``topk``, on those queries only; then every row of the result equals
``topk(scores_rowmajor(rows, queries), k)``.
"""
from collections import namedtuple

import torch

from . import ops

SearchResult = namedtuple("SearchResult", ["ids", "scores", "certified", "fallback"])
SearchResult.__doc__ = """ids int64 [nq, k], scores fp32 [nq, k]; certified int32 [nq] (int8 index) or None (fp16);
fallback: int64 tensor of the queries re-run on the exact path (empty without ``exact``)."""


def _select(queries, qlayout, which):
    """The queries ``which`` (a 1-d index tensor) in the same layout."""
    if qlayout in ("DN", "dim_major", ops.MDX_DIM_MAJOR):
        return queries[:, which].contiguous()
    return queries[which].contiguous()


def search(index, rows, queries, k, shortlist, qlayout="ND", center=None, exact=False):
    """Top-k of ``queries`` against ``rows`` (fp32 ``[N, D]`` on the device) through an int8 or fp16 ``index`` of the same rows
    (a :class:`ops.DescriptorIndex`).  ``shortlist`` rows per query (clamped to N, at most 4096) are rescored exactly.
    Returns a :data:`SearchResult`."""
    if index.storage not in ("i8", "f16"):
        raise ValueError("search: the first stage is an int8 or fp16 index; this one is stored as %s" % index.storage)
    if rows.dim() != 2 or tuple(rows.shape) != (index.n, index.d):
        raise ValueError("rows must be the index's [%d, %d] rows, got %s" % (index.n, index.d, tuple(rows.shape)))
    for name, x in (("k", k), ("shortlist", shortlist)):
        if isinstance(x, bool) or not isinstance(x, int) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (name, x))
    n = index.n
    K = min(shortlist, n)
    if K > ops.RESCORE_MAX_K:
        raise ValueError("shortlist=%d: at most %d rows per query are rescored" % (shortlist, ops.RESCORE_MAX_K))
    if k > K:
        raise ValueError("k=%d must be <= min(shortlist, N) = %d" % (k, K))
    if exact and index.d % 4:
        raise ValueError("exact=True re-runs queries through scores_rowmajor, which needs d %% 4 == 0 (d = %d)" % index.d)
    scores = index.scores(queries, qlayout, center=center)
    top_ids, top_scores = ops.topk(scores, K)
    del scores
    ids, sc = ops.rescore(rows, queries, top_ids, qlayout, center)
    certified = None
    if index.storage == "i8":
        certified, _ = ops.rescore_certify(sc, top_scores[:, K - 1], queries, index.i8_bounds(), n, qlayout, center)
    ids, sc = ids[:, :k].contiguous(), sc[:, :k].contiguous()
    fallback = torch.empty(0, dtype=torch.int64, device=ids.device)
    if exact:
        need = torch.ones(ids.shape[0], dtype=torch.bool, device=ids.device) if certified is None else certified < k
        fallback = torch.nonzero(need).reshape(-1)
        if fallback.numel():
            sub = _select(queries, qlayout, fallback)
            fi, fs = ops.topk(ops.scores_rowmajor(rows, sub, qlayout, center), k)
            ids[fallback] = fi
            sc[fallback] = fs
    return SearchResult(ids, sc, certified, fallback)
