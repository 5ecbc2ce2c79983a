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

``range_search(index, rows, queries, threshold)`` and ``self_join(index, rows, threshold)`` return EVERY pair whose exact fp32
chain score is ``>= threshold`` -- query x database row, or database row pairs i < j -- as a CSR :data:`RangeResult`.  With an
int8 ``index`` the join kernel prunes on the int8 scores with a per-pair error bound that can only over-select (the proof is in
``include/mdx.h``), and the exact chain decides every candidate; with ``index=None`` the exact route scores everything in fp32 and
compacts.  Both routes return the same bits.

``knn_join(index, rows, k)`` is the all-pairs kNN query: the exact top-k of every row against all rows (the neighbour lists of
DBA and of the diffusion graph) as a :data:`KnnResult`.  With an int8 ``index`` each chunk of rows runs bounds -> candidates ->
resolve (``include/mdx.h``, "exact kNN join"): a lower bound of every row's own k-th score from the int8 shard, the join kernel
at that per-row threshold, the exact chain on the candidates.  With ``index=None`` it is the exact route, ``scores_rowmajor`` (or
an fp32 index) + ``topk`` on chunks of rows.  Both routes return the same bits.

``duplicate_groups(index, rows, threshold)`` is what a user of ``self_join`` usually wants: not the pairs but the groups they form,
the connected components of the self-join's graph, at up to 8 thresholds from one pass of the join kernel, as a :data:`Groups`.
The candidates of each chunk go straight into a lock-free union-find on the device (``include/mdx.h``, "near-duplicate groups") and
are dropped again: N integers per threshold are kept, never a pair list.  Both routes return the same labels.

``recall_at(found_ids, exact_ids, depths)`` is how good a set of top-K lists is against another, usually the exact one: per query and
depth the share of the exact head that the found head holds, from the counts of ``ops.topk_overlap`` (``include/mdx_overlap.h``).
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops

RangeResult = namedtuple("RangeResult", ["offsets", "ids", "scores"])
RangeResult.__doc__ = """CSR over the queries (the rows i of a self-join): offsets int64 [m + 1], ids int64 [P], scores fp32 [P]; segment q
= ``ids[offsets[q]:offsets[q + 1]]``, larger score first, equal scores by ascending id."""

KnnResult = namedtuple("KnnResult", ["ids", "scores", "pruned_rows"])
KnnResult.__doc__ = """ids int64 [N, k], scores fp32 [N, k]: every row's exact top-k in rank order (its own match included);
pruned_rows: the rows whose list came from the int8 route (0 on the exact route)."""

Groups = namedtuple("Groups", ["labels", "offsets", "members", "stats"])
Groups.__doc__ = """labels int64 [N] (one threshold) or [T, N] (a sequence): the smallest row id of every row's group, so ``labels[i] == i``
exactly for the representatives.  offsets int64 [G + 1], members int64 [N]: the CSR of the groups in ascending label order, the
members of each in ascending id, singletons included -- ``members[offsets[:-1]]`` are the representatives; for a sequence of
thresholds, lists of T such tensors.  stats: ``{"chains", "edges", "hooks", "candidates"}``, the device counters of include/mdx.h
and the candidates the join kernel reported (0 on the exact route)."""

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


def _check_rows(index, rows):
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.float32 or rows.dim() != 2:
        raise ValueError("rows must be a 2-d fp32 device tensor [N, D]")
    if rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("rows must be non-empty, got %s" % (tuple(rows.shape),))
    if index is not None:
        if not isinstance(index, ops.DescriptorIndex):
            raise ValueError("index must be an int8 DescriptorIndex of rows, or None (the exact route)")
        if index.storage != "i8":
            raise ValueError("pruning needs an int8 index; this one is stored as %s (pass index=None for the exact route)" % index.storage)
        if tuple(rows.shape) != (index.n, index.d):
            raise ValueError("rows must be the index's [%d, %d] rows, got %s" % (index.n, index.d, tuple(rows.shape)))


def _join_stats(index, rows):
    """The index's join_stats for these rows, reduced once and kept on the index."""
    key = (rows.data_ptr(), tuple(rows.shape), tuple(rows.stride()))
    cached = getattr(index, "_join_stats", None)
    if cached is None or cached[0] != key:
        cached = (key, ops.join_stats(index, rows))
        index._join_stats = cached
    return cached[1]


def _candidates(a, sa, b, sb, tau, lo, hi, symmetric, capacity, remedy):
    pairs, count = ops.join_candidates(a, sa, b, sb, tau, lo, hi, symmetric, capacity)
    if count > capacity:                                   # the kernel counted on: run again at the exact size
        if count > ops._MAX_ITEMS:
            raise ValueError("%d candidates, more than one call holds (2^31 - 1): %s" % (count, remedy))
        pairs, count = ops.join_candidates(a, sa, b, sb, tau, lo, hi, symmetric, count)
    return pairs


def _concat(parts, device):
    """One CSR from consecutive row blocks' CSRs."""
    if len(parts) == 1:
        return RangeResult(*parts[0])
    offs, base = [torch.zeros(1, dtype=torch.int64, device=device)], 0
    for o, ids, _ in parts:
        offs.append(o[1:] + base)
        base += ids.numel()
    return RangeResult(torch.cat(offs), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]))


def range_search(index, rows, queries, threshold, qlayout="ND", center=None):
    """Every database row whose exact fp32 chain score against ``queries`` (minus ``center``) is ``>= threshold``, as a
    :data:`RangeResult` over the queries.  ``rows`` fp32 ``[N, D]`` on the device; ``index`` an int8 ``DescriptorIndex`` of
    ``rows`` (pruned on the int8 shard) or None (the exact route: ``scores_rowmajor``, or an fp32 index where D % 4 != 0, then
    :func:`ops.range_select`).  Both give the bits of ``mdx_scores`` on an fp32 index, filtered and in rank order."""
    _check_rows(index, rows)
    tau = ops._tau(threshold)
    x = ops.center_rows(queries, qlayout, center)             # x_q = q - center, row-major
    nq, d = x.shape
    if d != rows.shape[1]:
        raise ValueError("query dimension %d != rows dimension %d" % (d, rows.shape[1]))
    if index is None:                                         # blocks of queries: ~256 MB of fp32 scores at a time
        n = rows.shape[0]
        block = max(1, (1 << 28) // (4 * n))
        fp32 = None if d % 4 == 0 else ops.DescriptorIndex(rows, "ND")
        try:
            parts = []
            for lo in range(0, nq, block):
                sub = x[lo:min(nq, lo + block)]
                sc = ops.scores_rowmajor(rows, sub, "ND") if fp32 is None else fp32.scores(sub, "ND")
                parts.append(ops.range_select(sc, tau))
                del sc
            return _concat(parts, rows.device)
        finally:
            if fp32 is not None:
                fp32.close()
    qix = ops.DescriptorIndex(x, "ND", storage="i8")
    try:
        pairs = _candidates(qix, ops.join_stats(qix, x), index, _join_stats(index, rows), tau, 0, nq, False, max(4096, 64 * nq),
                            "search fewer queries at a time")
        return RangeResult(*ops.join_resolve(x, rows, pairs, tau, 0, nq))
    finally:
        qix.close()


def self_join(index, rows, threshold, chunk=None, max_pairs=None):
    """Every pair i < j of ``rows`` (fp32 ``[N, D]`` on the device) whose exact fp32 chain score is ``>= threshold``, as a
    :data:`RangeResult` over i.  ``index``: an int8 ``DescriptorIndex`` of ``rows`` (the join kernel prunes, the exact chain
    decides) or None (the exact route: fp32 scores of row blocks against every row, then :func:`ops.range_select`).  Memory is
    bounded by blocks of ``chunk`` rows (a multiple of 128 on the pruned route); a chunk whose candidates overflow the buffer is
    run again at their exact number.  ``max_pairs``: raise ValueError as soon as the result holds more pairs.  The bits depend
    on neither ``chunk`` nor the buffer sizes."""
    _check_rows(index, rows)
    tau = ops._tau(threshold)
    n, d = rows.shape
    for name, v in (("chunk", chunk), ("max_pairs", max_pairs)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
            raise ValueError("%s must be None or an integer >= 1, got %r" % (name, v))
    parts, total = [], 0
    if index is None:
        if chunk is None:                                     # ~256 MB of fp32 scores per block
            chunk = max(ops.JOIN_BLOCK, (1 << 28) // (4 * n) // ops.JOIN_BLOCK * ops.JOIN_BLOCK)
        fp32 = None if d % 4 == 0 else ops.DescriptorIndex(rows, "ND")
        try:
            for lo in range(0, n, chunk):
                hi = min(n, lo + chunk)
                if fp32 is None:                              # the upper triangle only: columns lo .. n-1, read in place
                    sc = ops.scores_rowmajor(rows[lo:], rows[lo:hi], "ND")
                    off, ids, vals = ops.range_select(sc, tau, diag=0)
                    parts.append((off, ids + lo, vals))
                else:
                    sc = fp32.scores(rows[lo:hi], "ND")
                    parts.append(ops.range_select(sc, tau, diag=lo))
                del sc
                total += parts[-1][1].numel()
                if max_pairs is not None and total > max_pairs:
                    raise ValueError("self_join: more than max_pairs=%d pairs at threshold %r" % (max_pairs, threshold))
        finally:
            if fp32 is not None:
                fp32.close()
        return _concat(parts, rows.device)
    # the join kernel runs groups of 16 row blocks against every later block: 2048 rows of A is one group; 32 768 rows per chunk
    # keep the candidate buffer small at the thresholds this targets and the per-chunk synchronisation rare
    chunk = 1 << 15 if chunk is None else -(-chunk // ops.JOIN_BLOCK) * ops.JOIN_BLOCK
    stats = _join_stats(index, rows)
    capacity = 1 << 20
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        pairs = _candidates(index, stats, index, stats, tau, lo, hi, True, capacity, "use a smaller chunk")
        capacity = max(capacity, pairs.numel())
        parts.append(ops.join_resolve(rows, rows, pairs, tau, lo, hi - lo))
        del pairs
        total += parts[-1][1].numel()
        if max_pairs is not None and total > max_pairs:
            raise ValueError("self_join: more than max_pairs=%d pairs at threshold %r" % (max_pairs, threshold))
    return _concat(parts, rows.device)


# ------------------------------------------------------------------------------------------------------ exact kNN join

KNN_MEMORY_CAP = 4 << 30        # bytes of [chunk, N] scores + top-k workspace one step of the exact route may hold


def _knn_bytes(n, chunk, k):
    return chunk * n * 4 + ops.rank_workspace_bytes(n, chunk) + chunk * k * 12


def knn_chunk(n, k, cap=KNN_MEMORY_CAP):
    """Rows per step of the exact route: as many as keep the ``[chunk, N]`` scores, the top-k workspace and the neighbour
    lists under ``cap`` bytes (at least one)."""
    chunk = max(1, min(n, cap // max(1, _knn_bytes(n, 1, k))))
    while chunk > 1 and _knn_bytes(n, chunk, k) > cap:
        chunk = max(1, min(chunk - 1, chunk * cap // _knn_bytes(n, chunk, k)))
    return chunk


class _ExactKnn:
    """The exact route on row ranges: ``scores_rowmajor`` where the rows lie (D % 4 == 0) or an fp32 index of the same rows
    (same kernels, same bits: include/mdx.h mdx_scores_rowmajor), then ``topk``; the score block and the top-k workspace are
    allocated once."""

    def __init__(self, rows, k, chunk):
        n, d = rows.shape
        self.rows, self.k, self.chunk = rows, k, chunk
        self.index = None if d % 4 == 0 else ops.DescriptorIndex(rows, "ND")
        self.scores = torch.empty((chunk, n), dtype=torch.float32, device=rows.device)
        self.workspace = ops._workspace(ops.rank_workspace_bytes(n, chunk), rows.device)

    def run(self, lo, hi, ids, sims):
        for i0 in range(lo, hi, self.chunk):
            i1 = min(hi, i0 + self.chunk)
            if self.index is None:
                block = ops.scores_rowmajor(self.rows, self.rows[i0:i1], "ND", out=self.scores[:i1 - i0])
            else:
                block = self.index.scores(self.rows[i0:i1], "ND", out=self.scores[:i1 - i0])
            bi, bs = ops.topk(block, self.k, workspace=self.workspace)
            ids[i0:i1] = bi
            sims[i0:i1] = bs

    def close(self):
        if self.index is not None:
            self.index.close()
        self.index = self.scores = self.workspace = None


def _check_count(x, what):
    if isinstance(x, bool) or not isinstance(x, int) or x < 1:
        raise ValueError("%s must be an integer >= 1, got %r" % (what, x))


def knn_join(index, rows, k, chunk=None, capacity=None):
    """The exact top-``min(k, N)`` of every row of ``rows`` (fp32 ``[N, D]`` on the device) against all of them, its own match
    included, as a :data:`KnnResult`: the bits of ``topk(scores of the rows against an fp32 index of them, k)``.

    ``index=None``: the exact route, ``chunk`` rows at a time (default: :func:`knn_chunk`, what fits ``KNN_MEMORY_CAP``).
    ``index``: an int8 ``DescriptorIndex`` of ``rows``; per chunk (a multiple of 128 rows, default 32 768) ``knn_bounds`` ->
    ``join_candidates_rows`` -> ``knn_resolve``.  A candidate buffer that overflows (``capacity`` pairs at first) is run again at
    the counted size.  A chunk with more than ``chunk * N / 8`` candidates is one the bound does not prune (structureless rows:
    at D = 2048 the bound is about 1.3 standard deviations of random scores) and takes the exact route instead;
    ``pruned_rows`` counts the rows that stayed on the int8 route.  The bits depend on none of this."""
    _check_rows(index, rows)
    _check_count(k, "k")
    if chunk is not None:
        _check_count(chunk, "chunk")
    if capacity is not None:
        _check_count(capacity, "capacity")
    n, d = rows.shape
    k = min(k, n)
    if index is not None and k > ops.KNN_JOIN_MAX_K:
        raise ValueError("knn_join: k=%d with an index: the int8 route keeps at most KNN_JOIN_MAX_K = %d neighbours per row "
                         "(pass index=None for the exact route)" % (k, ops.KNN_JOIN_MAX_K))
    ids = torch.empty((n, k), dtype=torch.int64, device=rows.device)
    sims = torch.empty((n, k), dtype=torch.float32, device=rows.device)
    if index is None:
        exact = _ExactKnn(rows, k, min(chunk or knn_chunk(n, k), n))
        try:
            exact.run(0, n, ids, sims)
        finally:
            exact.close()
        return KnnResult(ids, sims, 0)
    chunk = 1 << 15 if chunk is None else -(-chunk // ops.JOIN_BLOCK) * ops.JOIN_BLOCK
    stats = _join_stats(index, rows)
    capacity = capacity or 1 << 20
    exact, pruned = None, 0
    try:
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            limit = min((hi - lo) * n // 8, ops._MAX_ITEMS)      # beyond it the bound does not prune (and a call holds no more)
            t = ops.knn_bounds(index, stats, index, stats, lo, hi, k)
            pairs, count = ops.join_candidates_rows(index, stats, index, stats, t, lo, hi, min(capacity, max(limit, 1)))
            if count > limit:
                del pairs
                if exact is None:
                    exact = _ExactKnn(rows, k, min(knn_chunk(n, k), n))
                exact.run(lo, hi, ids, sims)
                continue
            if count > pairs.numel():                            # the kernel counted on: run again at the exact size
                pairs, count = ops.join_candidates_rows(index, stats, index, stats, t, lo, hi, count)
            capacity = max(capacity, pairs.numel())
            bi, bs, _ = ops.knn_resolve(rows, rows, pairs, lo, hi - lo, k)
            del pairs
            ids[lo:hi] = bi
            sims[lo:hi] = bs
            pruned += hi - lo
    finally:
        if exact is not None:
            exact.close()
    return KnnResult(ids, sims, pruned)


# ------------------------------------------------------------------------------------------------------ near-duplicate groups

def split_rows(lo, hi):
    """The two halves ``((lo, mid), (mid, hi))`` of the row range ``[lo, hi)`` of a chunk whose candidates were too many, cut at a
    multiple of ``JOIN_BLOCK`` rows from ``lo`` (itself one); None for a single block, which cannot be split."""
    blocks = -(-(hi - lo) // ops.JOIN_BLOCK)
    if blocks <= 1:
        return None
    mid = lo + blocks // 2 * ops.JOIN_BLOCK
    return (lo, mid), (mid, hi)


def _group_csr(labels):
    """(offsets, members) of one level's labels: a stable sort keeps the members of a group in ascending id."""
    vals, members = torch.sort(labels, stable=True)
    _, counts = torch.unique_consecutive(vals, return_counts=True)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets, members


def duplicate_groups(index, rows, threshold, chunk=None, max_candidates=1 << 26):
    """The groups of near-duplicates of ``rows`` (fp32 ``[N, D]`` on the device): the connected components of the graph whose edges
    are the pairs :func:`self_join` reports at ``threshold``, as a :data:`Groups`.  ``threshold``: a number, or a sequence of at most
    8 (any order, duplicates allowed) -- all of them from ONE pass of the join kernel, at the smallest.

    ``index``: an int8 ``DescriptorIndex`` of ``rows``; per chunk (a multiple of 128 rows, default 32 768, as ``self_join``)
    ``join_candidates`` -> ``groups_union_pairs``, and the candidates are dropped before the next chunk.  A chunk with more than
    ``max_candidates`` candidates is split in halves and run again; a single 128-row block runs at its counted size.  Pairs whose
    rows are already in one group are never scored, so a cluster of many identical rows costs little more than its candidates'
    listing.  ``index=None``: the exact route, the fp32 score blocks of ``self_join``'s into ``groups_union_dense``.  The labels
    depend on the rows and thresholds only."""
    _check_rows(index, rows)
    single = isinstance(threshold, (bool, int, float))
    if not single and (not isinstance(threshold, (list, tuple)) or not 1 <= len(threshold) <= ops.GROUPS_MAX_T):
        raise ValueError("threshold must be a number or a sequence of 1 to %d numbers, got %r" % (ops.GROUPS_MAX_T, threshold))
    taus = [ops._tau(t) for t in ([threshold] if single else threshold)]
    if chunk is not None:
        _check_count(chunk, "chunk")
    _check_count(max_candidates, "max_candidates")
    n, d = rows.shape
    if n > ops._MAX_ITEMS:
        raise ValueError("duplicate_groups: %d rows, the forest holds at most 2^31 - 1" % n)
    parent, status = ops.groups_init(len(taus), n, rows.device)
    candidates = 0
    if index is None:
        if chunk is None:                                     # ~256 MB of fp32 scores per block
            chunk = max(ops.JOIN_BLOCK, (1 << 28) // (4 * n) // ops.JOIN_BLOCK * ops.JOIN_BLOCK)
        fp32 = None if d % 4 == 0 else ops.DescriptorIndex(rows, "ND")
        try:
            for lo in range(0, n, chunk):
                hi = min(n, lo + chunk)
                if fp32 is None:                              # the upper triangle only: columns lo .. n-1, read in place
                    ops.groups_union_dense(ops.scores_rowmajor(rows[lo:], rows[lo:hi], "ND"), lo, lo, taus, parent, status)
                else:
                    ops.groups_union_dense(fp32.scores(rows[lo:hi], "ND"), lo, 0, taus, parent, status)
        finally:
            if fp32 is not None:
                fp32.close()
    else:
        chunk = 1 << 15 if chunk is None else -(-chunk // ops.JOIN_BLOCK) * ops.JOIN_BLOCK
        stats = _join_stats(index, rows)
        tmin, capacity = min(taus), 1 << 20
        for start in range(0, n, chunk):
            work = [(start, min(n, start + chunk))]
            while work:
                lo, hi = work.pop()
                pairs, count = ops.join_candidates(index, stats, index, stats, tmin, lo, hi, True, min(capacity, max_candidates))
                halves = split_rows(lo, hi) if count > max_candidates else None
                if halves is not None:
                    del pairs
                    work.extend(reversed(halves))
                    continue
                if count > pairs.numel():                     # the kernel counted on: run again at the exact size
                    if count > ops._MAX_ITEMS:
                        raise ValueError("%d candidates in one 128-row block, more than one call holds (2^31 - 1)" % count)
                    del pairs
                    pairs, count = ops.join_candidates(index, stats, index, stats, tmin, lo, hi, True, count)
                capacity = max(capacity, pairs.numel())
                candidates += count
                if count:
                    ops.groups_union_pairs(rows, pairs, taus, parent, status)
                del pairs
    labels = ops.groups_labels(parent)
    st = ops.groups_status(status)
    if st["flags"]:
        raise ops._lib.MdxError("duplicate_groups: the union kernels set flags %#x (1: a loop gave up, 2: a pair out of range)" % st["flags"])
    csr = [_group_csr(labels[t]) for t in range(len(taus))]
    stats = {"chains": st["chains"], "edges": st["edges"], "hooks": st["hooks"], "candidates": candidates}
    if single:
        return Groups(labels[0], csr[0][0], csr[0][1], stats)
    return Groups(labels, [c[0] for c in csr], [c[1] for c in csr], stats)


def recall_at(found_ids, exact_ids, depths):
    """Recall of the lists ``found_ids`` int64 ``[nq, ka]`` against ``exact_ids`` int64 ``[nq, kb]`` (device tensors, best first, -1
    padding) at each of ``depths`` (an integer or 1 to ``ops.OVERLAP_MAX_DEPTHS`` ascending ones): float64 ``[nq, T]`` on the host,
    ``ops.topk_overlap(found_ids, exact_ids, depths)[q, t] / min(depths[t], valid entries of exact_ids[q])`` -- the share of the
    exact head that the found head holds; NaN for a query whose exact list is all padding."""
    depths = list(depths) if isinstance(depths, (list, tuple)) else [depths]
    counts = ops.topk_overlap(found_ids, exact_ids, depths).cpu().numpy().astype("float64")
    valid = (exact_ids >= 0).sum(1).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        return counts / np.minimum(np.asarray(depths, dtype=np.int64)[None, :], valid[:, None])
