"""Re-ranking of the revisited Oxford/Paris protocol: alpha-weighted query expansion (alpha-QE) and database-side
augmentation (DBA), as the GeM paper defines them (Radenovic, Tolias, Chum, "Fine-tuning CNN image retrieval with no human
annotation", TPAMI 2018), and diffusion on a mutual kNN graph of the database (Iscen et al., "Efficient diffusion on region
manifolds", CVPR 2017), and k-reciprocal encoding (Zhong et al., "Re-ranking person re-identification with k-reciprocal
encoding", CVPR 2017) in its database-side form.  Not in the reference: the vendored cirtorch ships none of them.

Both are built from the library's own pieces -- the exact similarity (``mdx_scores_rowmajor`` or an index), the top-k of
``mdx_topk`` (descending score, ascending id on ties) and the weighted gather-and-normalise ``mdx_knn_aggregate``, whose
contract (weights ``s ** alpha`` for ``s > 0``, fp32 fma chain in neighbour order, L2N with eps 1e-6) is stated in
``include/mdx.h``.  Everything stays on the device; nothing falls back to the CPU.
"""
import math

import torch

from . import _lib, ivf, ops, search
from .search import KNN_MEMORY_CAP as DBA_MEMORY_CAP        # bytes of [chunk, N] scores + top-k workspace one DBA chunk may hold
from .search import _knn_bytes as _dba_bytes


def _check(k, alpha):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("k must be an integer >= 1, got %r" % (k,))
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError("alpha must be a finite number >= 0, got %r" % (alpha,))


def _similarity(vecs, queries, index, compute, out=None):
    """[nq, N] scores of row-major ``queries`` against the rows of ``vecs`` (or of ``index``, which holds the same rows)."""
    if index is None:
        if compute not in ("chain", "exact"):
            raise ValueError("compute=%r multiplies an index: pass index=DescriptorIndex(vecs, 'ND')" % (compute,))
        return ops.scores_rowmajor(vecs, queries, "ND", out=out)
    return index.scores(queries, "ND", out=out, compute=compute)


def query_expansion(qvecs, vecs, k, alpha, index=None, compute="chain"):
    """alpha-QE of ``qvecs`` ``[Q, D]`` against the database ``vecs`` ``[N, D]`` (both row-major fp32 on the device).

    ``(ids, s) = topk(Q.X^T, min(k, N))``, ``Q' = knn_aggregate(X, ids, s, alpha, self_rows=Q)``, and the returned scores
    are ``Q'.X^T``.  ``alpha = 0`` is plain average query expansion.  Both similarity passes use the same mode: with no
    ``index`` the exact chain reads ``vecs`` where it lies (``scores_rowmajor``); with an ``index`` (an fp16 shard, or the
    split3 / split2 modes through ``compute``) both passes are ``index.scores``.  The neighbour rows always come from the
    fp32 ``vecs``.  In self-retrieval (queries that are database rows, as on Tokyo) a query's own row is its own top
    neighbour and is counted once more on top of the self term, as a naive numpy implementation does.

    Returns ``(scores [Q, N], expanded queries [Q, D])``."""
    _check(k, alpha)
    if vecs.dim() != 2 or qvecs.dim() != 2 or qvecs.shape[1] != vecs.shape[1]:
        raise ValueError("qvecs [Q, D] and vecs [N, D] expected, got %s and %s" % (tuple(qvecs.shape), tuple(vecs.shape)))
    k = min(k, vecs.shape[0])
    scores = _similarity(vecs, qvecs, index, compute)
    ids, sims = ops.topk(scores, k)
    expanded = ops.knn_aggregate(vecs, ids, sims, alpha, self_rows=qvecs)
    return _similarity(vecs, expanded, index, compute, out=scores), expanded


def dba_chunk(n, k, cap=DBA_MEMORY_CAP):
    """Rows per DBA step: as many as keep the ``[chunk, N]`` scores, the top-k workspace and the neighbour lists under
    ``cap`` bytes (at least one) -- :func:`search.knn_chunk`."""
    return search.knn_chunk(n, k, cap)


def _neighbours(vecs, k, chunk, index):
    """The top-k lists of every row: exact from :func:`search.knn_join` (the exact route, or pruned on an int8 ``index`` of ``vecs``),
    or approximate from ``IVFIndex.knn_join`` where ``index`` is an :class:`ivf.IVFNeighbours` whose rows are ``vecs``."""
    if isinstance(index, ivf.IVFNeighbours):
        return index.lists_of(vecs, k)
    if index is not None and (not isinstance(index, ops.DescriptorIndex) or index.storage != "i8"):
        raise ValueError("index must be an int8 DescriptorIndex of vecs (storage='i8'), or None for the exact route")
    res = search.knn_join(index, vecs, k, chunk=chunk)
    return res.ids, res.scores


def database_augmentation(vecs, k, alpha, chunk=None, layout="ND", index=None):
    """DBA of the database ``vecs``: a NEW ``[N, D]`` row-major fp32 matrix whose row i is
    ``knn_aggregate(X, topk(x_i.X^T, min(k, N)), alpha)`` with no separate self term (the top-k includes i itself), always
    read from the original rows.  ``vecs`` is never written.

    The neighbour lists are :func:`search.knn_join`'s: the exact fp32 chain, ``chunk`` rows at a time (scores_rowmajor, topk;
    the default chunk keeps each step under ``DBA_MEMORY_CAP`` bytes, :func:`dba_chunk`), or, with ``index`` -- an int8
    ``DescriptorIndex`` of ``vecs`` -- the same lists pruned on the int8 shard; then one ``knn_aggregate``.  The result depends
    on neither the chunk nor the index.  (``index`` may also be an ``ivf.IVFNeighbours`` whose rows are ``vecs``: the lists
    are then ``IVFIndex.knn_join``'s, approximate unless every list is probed -- here, in :class:`DiffusionGraph` and in
    :class:`ReciprocalEncoding`.)  ``layout="DN"`` accepts the reference's ``[D, N]`` matrix through one transpose copy
    (an ``index`` is of the row-major rows); the result is ``[N, D]`` either way."""
    _check(k, alpha)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError("chunk must be an integer >= 1, got %r" % (chunk,))
    if layout in ("DN", "dim_major", _lib.MDX_DIM_MAJOR):
        vecs = vecs.t().contiguous()
    elif layout not in ("ND", "row_major", _lib.MDX_ROW_MAJOR):
        raise ValueError("unknown layout %r" % (layout,))
    if vecs.dim() != 2:
        raise ValueError("vecs must be 2-d, got %s" % (tuple(vecs.shape),))
    n, d = vecs.shape
    k = min(k, n)
    ids, sims = _neighbours(vecs, k, chunk, index)
    out = torch.empty((n, d), dtype=torch.float32, device=vecs.device)
    step = min(chunk or dba_chunk(n, k), n)                  # the aggregation launches of the chunked loop, unchanged
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        ops.knn_aggregate(vecs, ids[i0:i1], sims[i0:i1], alpha, out=out[i0:i1])
    return out


# ------------------------------------------------------------------------------------------------------------ diffusion

DIFFUSION_DEFAULTS = {"k": 50, "kq": 10, "gamma": 3.0, "alpha": 0.99, "iters": 20, "tol": 1e-6}   # the paper's release


def _check_int(x, what):
    if isinstance(x, bool) or not isinstance(x, int) or x < 1:
        raise ValueError("%s must be an integer >= 1, got %r" % (what, x))


def _check_real(x, what, upper=None):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0 or \
            (upper is not None and x >= upper):
        raise ValueError("%s must be a finite number >= 0%s, got %r" % (what, "" if upper is None else " and < %g" % upper, x))


class DiffusionGraph:
    """The normalised mutual kNN graph of the database ``vecs`` ``[N, D]`` that :func:`diffusion` solves on
    (``mdx_knn_graph``; definition in ``include/mdx.h``).  Built once per database, like DBA: the neighbour lists of
    :func:`search.knn_join` -- the exact fp32 chain ``chunk`` rows at a time (scores_rowmajor, topk of ``min(k, N)``), under the
    DBA memory cap for the chunk (:func:`dba_chunk`), or pruned on ``index``, an int8 ``DescriptorIndex`` of ``vecs`` -- then
    the graph kernel on the whole ``[N, k]`` lists.  The lists depend on neither the chunk nor the index.

    Attributes: ``cols`` int32 / ``vals`` fp32 ``[N, k]``, ``counts`` int32 ``[N]``, ``n``, ``k`` (``min(k, N)``),
    ``gamma``, and ``wvals`` fp32 ``[N, k]``: with ``weights=True`` the unnormalised weights that the truncated solve
    renormalises on each query's subgraph (``mdx_knn_graph_weights``, N * k * 4 more bytes), else None.
    ``layout="DN"`` accepts the reference's ``[D, N]`` matrix through one transpose copy."""

    def __init__(self, vecs, k=50, gamma=3.0, chunk=None, layout="ND", weights=False, index=None):
        _check_int(k, "k")
        _check_real(gamma, "gamma")
        if chunk is not None:
            _check_int(chunk, "chunk")
        if layout in ("DN", "dim_major", _lib.MDX_DIM_MAJOR):
            vecs = vecs.t().contiguous()
        elif layout not in ("ND", "row_major", _lib.MDX_ROW_MAJOR):
            raise ValueError("unknown layout %r" % (layout,))
        if vecs.dim() != 2:
            raise ValueError("vecs must be 2-d, got %s" % (tuple(vecs.shape),))
        n, d = vecs.shape
        k = min(k, n)
        ids, sims = _neighbours(vecs, k, chunk, index)
        self.cols, self.vals, self.counts = ops.knn_graph(ids, sims, gamma)
        self.wvals = ops.knn_graph_weights(ids, sims, gamma)[1] if weights else None     # same cols / counts
        self.n, self.k, self.gamma = n, k, float(gamma)

    def edges(self):
        """Stored (directed) edges: twice the number of mutual pairs.  Reads the counts back (synchronises)."""
        return int(self.counts.sum(dtype=torch.int64).item())

    def close(self):
        self.cols = self.vals = self.counts = self.wvals = None


def diffusion(qvecs, vecs, graph=None, kq=10, alpha=0.99, iters=20, tol=1e-6, index=None, compute="chain", scores=None,
              return_residual=False, truncate=None):
    """Diffusion scores ``[Q, N]`` of the queries ``qvecs`` ``[Q, D]`` on the database ``vecs`` ``[N, D]``
    (``mdx_diffusion``; definition in ``include/mdx.h``): seeds ``max(s, 0) ** gamma`` at the ``min(kq, N)`` best
    first-stage scores, CG on ``(I - alpha S) f = y`` for at most ``iters`` steps, then ``f`` where positive and the
    first-stage score minus 3 elsewhere, so that rows the diffusion did not reach rank last, in first-stage order.

    ``graph`` is a :class:`DiffusionGraph` of ``vecs`` (built here with its defaults when None; pass one to reuse it across
    batches); its ``gamma`` also weights the seeds.  The first-stage scores come from ``scores`` when given (never
    written), else from the similarity of ``vecs`` or ``index`` in mode ``compute`` (as :func:`query_expansion`).
    With ``return_residual``: ``(scores, residual [Q], steps [Q])``, the final ``||r|| / ||y||`` and the steps taken.

    ``truncate`` (an integer, ``kq <= truncate <= 4096``) solves each query on the subgraph of its ``R = min(truncate, N)``
    best first-stage rows instead (``mdx_diffusion_truncated``): the graph must hold ``wvals`` (``weights=True``; built so
    when None).  None: the full solve."""
    _check_int(kq, "kq")
    _check_real(alpha, "alpha", upper=1.0)
    _check_int(iters, "iters")
    _check_real(tol, "tol")
    if truncate is not None:
        _check_int(truncate, "truncate")
        if truncate > ops.DIFFUSION_MAX_R or truncate < kq:
            raise ValueError("truncate must be in [kq, %d] = [%d, %d], got %r" % (ops.DIFFUSION_MAX_R, kq, ops.DIFFUSION_MAX_R,
                                                                                   truncate))
        if graph is not None and getattr(graph, "wvals", None) is None:
            raise ValueError("truncate needs the graph's unnormalised weights: build it with DiffusionGraph(..., weights=True)")
    if vecs.dim() != 2 or qvecs.dim() != 2 or qvecs.shape[1] != vecs.shape[1]:
        raise ValueError("qvecs [Q, D] and vecs [N, D] expected, got %s and %s" % (tuple(qvecs.shape), tuple(vecs.shape)))
    n = vecs.shape[0]
    if graph is None:
        graph = DiffusionGraph(vecs, weights=truncate is not None)
    if graph.n != n:
        raise ValueError("graph has %d rows, the database %d" % (graph.n, n))
    if scores is None:
        first = _similarity(vecs, qvecs, index, compute)
        out = first                                        # ours: solved in place
    else:
        if tuple(scores.shape) != (qvecs.shape[0], n):
            raise ValueError("scores must be [%d, %d], got %s" % (qvecs.shape[0], n, tuple(scores.shape)))
        first, out = scores, None
    if truncate is not None:
        top_ids, top_sims = ops.topk(first, min(truncate, n))       # the seeds are its first min(kq, R) entries
        return ops.diffusion_truncated(graph, first, top_ids, top_sims, kq, graph.gamma, alpha, iters, tol, out=out,
                                       return_residual=return_residual)
    seed_ids, seed_sims = ops.topk(first, min(kq, n))
    return ops.diffusion(graph, first, seed_ids, seed_sims, graph.gamma, alpha, iters, tol, out=out,
                         return_residual=return_residual)


# ---------------------------------------------------------------------------------------------------------- k-reciprocal

K_RECIPROCAL_DEFAULTS = {"k1": 20, "k2": 6, "lam": 0.3, "truncate": 1000}


def _check_krecip(k1, k2):
    _check_int(k1, "k1")
    _check_int(k2, "k2")
    if k1 > ops.KRECIP_MAX_K1:
        raise ValueError("k1 must be <= %d, got %r" % (ops.KRECIP_MAX_K1, k1))
    if k2 > k1:
        raise ValueError("k2 must be <= k1 = %d, got %r" % (k1, k2))
    if k2 * k1 * (1 + (k1 + 1) // 2) > ops.KRECIP_MAX_NNZ:
        raise ValueError("k2 * k1 * (1 + ceil(k1 / 2)) = %d exceeds %d (k1=%d, k2=%d): the codes are bounded statically"
                         % (k2 * k1 * (1 + (k1 + 1) // 2), ops.KRECIP_MAX_NNZ, k1, k2))


class ReciprocalEncoding:
    """The k-reciprocal codes of the database ``vecs`` ``[N, D]`` that :func:`k_reciprocal` compares the queries with
    (definition in ``include/mdx_krecip.h``).  Built once per database, like :class:`DiffusionGraph`: the neighbour lists of
    :func:`search.knn_join` (``k = min(k1, N)``; the exact route ``chunk`` rows at a time, or pruned on ``index``, an int8
    ``DescriptorIndex`` of ``vecs``), the reciprocal sets, the raw codes and their local expansion over the first ``min(k2, k)``
    list entries.  The lists, and so every bit here, depend on neither the chunk nor the index.  Each CSR reads its nnz back once
    (synchronises).

    Attributes: ``rk`` / ``rh`` int32 ``[N, k]`` / ``[N, ceil(k / 2)]`` with ``rk_counts`` / ``rh_counts`` int32 ``[N]`` (the two
    ELLs); ``raw`` and ``expanded``, each ``(offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz])``; ``kth`` fp32 ``[N]`` (the
    k-th score of every list); ``n``, ``k`` (``min(k1, N)``), ``k1``, ``k2``.  ``layout="DN"`` accepts the reference's ``[D, N]``
    matrix through one transpose copy."""

    def __init__(self, vecs, k1=20, k2=6, chunk=None, layout="ND", index=None):
        _check_krecip(k1, k2)
        if chunk is not None:
            _check_int(chunk, "chunk")
        if layout in ("DN", "dim_major", _lib.MDX_DIM_MAJOR):
            vecs = vecs.t().contiguous()
        elif layout not in ("ND", "row_major", _lib.MDX_ROW_MAJOR):
            raise ValueError("unknown layout %r" % (layout,))
        if vecs.dim() != 2:
            raise ValueError("vecs must be 2-d, got %s" % (tuple(vecs.shape),))
        n = vecs.shape[0]
        k = min(k1, n)
        ids, sims = _neighbours(vecs, k, chunk, index)
        sets = ops.krecip_sets(ids)
        self.rk, self.rk_counts, self.rh, self.rh_counts = sets
        offsets = ops.krecip_raw_offsets(sets)
        nnz = int(offsets[n].item())
        self.raw = (offsets,) + ops.krecip_raw_fill(vecs, ids, sims, sets, offsets, nnz)
        kk = min(k2, k)
        offsets = ops.krecip_expand_offsets(ids, kk, self.raw)
        nnz = int(offsets[n].item())
        self.expanded = (offsets,) + ops.krecip_expand_fill(ids, kk, self.raw, offsets, nnz)
        self.kth = sims[:, k - 1].contiguous()
        self.n, self.k, self.k1, self.k2 = n, k, k1, k2

    def nnz(self):
        """``(raw, expanded)`` stored entries."""
        return self.raw[1].shape[0], self.expanded[1].shape[0]

    def close(self):
        self.rk = self.rk_counts = self.rh = self.rh_counts = self.raw = self.expanded = self.kth = None


def k_reciprocal(qvecs, vecs, encoding=None, lam=0.3, truncate=1000, index=None, compute="chain", scores=None):
    """k-reciprocal scores ``[Q, N]`` of the queries ``qvecs`` ``[Q, D]`` on the database ``vecs`` ``[N, D]``
    (``mdx_krecip_rerank``; definition in ``include/mdx_krecip.h``): each query is encoded against the database's lists, and the
    ``R = min(truncate, N)`` best first-stage rows get ``(1 - lam) * (1 - d_Jaccard) + lam * (1 + s) / 2``; every other row
    keeps its first-stage score minus 3, so that rows outside the shortlist rank last, in first-stage order.

    ``encoding`` is a :class:`ReciprocalEncoding` of ``vecs``; pass one to reuse it across batches.  When None, one is built here
    with its defaults on the exact route (``index`` is the index of the first-stage similarity, as in :func:`diffusion`, and is not
    handed to the neighbour join) and closed again before the call returns.  The first-stage scores come from ``scores`` when given (never written), else from the similarity of
    ``vecs`` or ``index`` in mode ``compute`` (as :func:`query_expansion`) and are then solved in place.  A query that is a
    database row finds its own row among the ``k2 - 1`` rows of its local expansion and counts it once more, as alpha-QE does.
    ``truncate`` is an integer in ``[1, 4096]``, ``lam`` a number in ``[0, 1]``."""
    _check_int(truncate, "truncate")
    if truncate > ops.KRECIP_MAX_R:
        raise ValueError("truncate must be in [1, %d], got %r" % (ops.KRECIP_MAX_R, truncate))
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not math.isfinite(lam) or not 0 <= lam <= 1:
        raise ValueError("lam must be a finite number in [0, 1], got %r" % (lam,))
    if vecs.dim() != 2 or qvecs.dim() != 2 or qvecs.shape[1] != vecs.shape[1]:
        raise ValueError("qvecs [Q, D] and vecs [N, D] expected, got %s and %s" % (tuple(qvecs.shape), tuple(vecs.shape)))
    n = vecs.shape[0]
    own = encoding is None
    if own:
        encoding = ReciprocalEncoding(vecs)
    if encoding.n != n:
        raise ValueError("encoding has %d rows, the database %d" % (encoding.n, n))
    if scores is None:
        first = _similarity(vecs, qvecs, index, compute)
        out = first                                        # ours: solved in place
    else:
        if tuple(scores.shape) != (qvecs.shape[0], n):
            raise ValueError("scores must be [%d, %d], got %s" % (qvecs.shape[0], n, tuple(scores.shape)))
        first, out = scores, None
    top_ids, _ = ops.topk(first, min(truncate, n))
    res = ops.krecip_rerank((encoding.rh, encoding.rh_counts), encoding.kth, encoding.k, min(encoding.k2, encoding.k),
                            encoding.raw, encoding.expanded, first, top_ids, float(lam), out=out)
    if own:
        encoding.close()                                   # the launches hold the stream's order; torch frees behind them
    return res
