"""An inverted file (IVF) over the partition of spherical k-means: score only the rows whose centroid is among a query's best.

Every other search path of the library reads the whole database for every batch of queries; this one reads the lists a query probes.
The partition is ``cluster.kmeans``'s (or any labels), the rows stay where they are, the scores are the exact fp32 chain, and the
result is defined to the bit: with ``nprobe == lists`` it is ``ops.topk(index.scores(q), k)`` of an fp32 ``DescriptorIndex`` of the
rows, with fewer probes it is that ranking restricted to the rows of the probed lists.  ``tests/ivf_restatement.py`` states it in numpy.

``IVFIndex(rows, centroids, labels=None, chunk=None, storage="f32")``
    ``rows`` fp32 ``[N, D]`` on the device, rows contiguous at any row stride (as ``ops.rescore`` accepts); read in place, never
    copied or permuted.  ``centroids`` fp32 ``[K, D]`` on the same device, contiguous.  ``labels`` int64 ``[N]`` in ``[0, K)``: the
    list of every row; ``None`` means ``cluster.assign(centroids, rows, chunk)[0]`` (``rows`` must then be contiguous).  Explicit
    labels need not be the argmax: a row is found through the list it was put in.
    The index keeps ``order``, ``offsets`` and ``sizes`` as ``cluster._members`` builds them -- a stable sort of the labels, so the
    members of a list ascend -- and ``coarse``, an fp32 ``ops.DescriptorIndex`` of the centroids.  It reads ``sizes`` back once, at
    build time (the one synchronisation a search rests on; the range check of explicit labels and the build of the coarse index
    synchronise there too): from the sorted list sizes and tile counts it knows, for every ``nprobe``, the candidate
    capacity of a query (``capacity(nprobe)``: the sum of the ``nprobe`` largest lists) and a bound on the scan's work items
    (:func:`item_bound`), so a search reads nothing back.

    ``storage="i8"`` (``include/mdx_lists_i8.h``) also keeps ``codes`` (int8 ``[N, round_up(D, 64)]``) and ``scales`` (fp32 ``[N]``),
    the ``MDX_I8`` quantisation of the rows in list order (``ops.lists_i8_encode`` of ``order``), and ``bounds``
    (``ops.lists_i8_bounds``), all built once here.  The fp32 rows stay: the exact second stage reads them.  ``D <= 133120``.

``IVFIndex.train(rows, lists, storage="f32", **kmeans_kwargs)``
    ``cluster.kmeans(rows, lists, **kmeans_kwargs)``, then the index of ``fit.centroids`` and ``fit.labels``; the :data:`KMeans`
    result stays reachable as ``.fit``.

``index.search(queries, k, nprobe, qlayout="ND", center=None)`` -> :data:`IVFResult`
    1. ``probes`` = the ids of ``ops.topk(coarse.scores(queries, qlayout, center=center), nprobe)``.  ``center`` has the library's
       usual meaning, ``x_q = q - center`` in one fp32 subtraction, for the coarse stage and the scan alike.
    2. ``ops.ivf_plan``: per query the first column of every probe's segment in its candidate row (a prefix sum of list sizes in
       probe order) and ``scanned``, its number of candidates; per list the queries that probe it.
    3. ``ops.ivf_scan``: list-major, a tile of 64 members of a list is read once for up to ``ops.IVF_QUERY_GROUP`` queries that probe
       it.  ``scores`` are bit-identical to ``ops.DescriptorIndex(rows, "ND").scores(queries, qlayout, center)`` at the same id.
    4. ``ops.ivf_select``: the first ``k`` candidates in ``rank_full``'s order: the larger score first, ``-0 == +0``, NaN last, equal
       keys by ascending row id, whichever list a row sits in.  Where ``scanned[q] < k`` the tail is id ``-1`` and score NaN.
    ``1 <= nprobe <= K`` and ``1 <= k <= ops.RESCORE_MAX_K``.  The queries are taken ``query_chunk(nprobe)`` at a time, so that the
    candidate block stays under ``CANDIDATE_MEMORY_CAP`` bytes; the chunk changes no bit of the result.  Nothing is read back and
    nothing synchronises.  There is no CPU fallback.

``index.search(queries, k, nprobe, qlayout="ND", center=None, shortlist=None, exact=False)`` on an ``"i8"`` index -> :data:`IVFRescored`
    Steps 1 and 2 as above.  3. ``ops.lists_i8_scan`` on ``ops.quantize_i8(ops.center_rows(queries, qlayout, center))``: the same work
    items on the int8 MFMA, over the contiguous codes; the candidate scores are the bits of
    ``ops.DescriptorIndex(rows, "ND", storage="i8").scores(queries, qlayout, center)`` at the same id.
    ``shortlist=None``: the int8 ranking -- ``ops.ivf_select`` of those candidates; ``certified`` is ``None`` and ``fallback`` empty.
    ``shortlist=S`` (``k <= S <= ops.RESCORE_MAX_K``): ``ops.ivf_select`` takes ``S`` candidates by int8 score, ``ops.rescore``
    scores them with the exact chain on ``rows`` and sorts them, ``ops.rescore_certify`` (``t`` = the S-th int8 score, ``bounds``)
    gives the depth, and the first ``k`` are returned.  The first ``certified[q]`` entries are, bit for bit, the first entries of
    ``IVFIndex(rows, centroids, labels).search(queries, k, nprobe, qlayout, center)`` -- the proof is in ``include/mdx_lists_i8.h``.
    Where ``scanned[q] <= S`` every candidate was rescored: ``certified[q] = S`` and the whole row, padding included, is the fp32
    index's.  (The -1 ids that pad a shortlist go to ``ops.rescore`` as the id ``N``, which it never dereferences either, so that they
    sort behind a candidate whose chain score is NaN, where the fp32 search has its padding; they come back as -1.)
    ``exact=True`` (needs ``shortlist``): the queries with ``certified < k`` are run again through the fp32 scan of this index
    (``ops.ivf_scan`` on ``rows``) and ``fallback`` (int64, ascending) lists them; the whole result then equals the fp32 index's.  This
    is the one read-back of a search: ``nonzero`` of ``certified < k``.  ``shortlist`` and ``exact`` are a ``ValueError`` on an
    ``"f32"`` index.  ``query_chunk(nprobe, shortlist)`` counts the query codes and the shortlist's buffers as well.

``index.knn_join(k, nprobe, shortlist=None, reverse=True, chunk=None)`` -> :data:`IVFKnnResult`
    The approximate kNN join of the rows with themselves, ``k' = min(k, N)`` neighbours a row, for the database-side re-ranking
    (``rerank.database_augmentation``, ``rerank.DiffusionGraph``, ``rerank.ReciprocalEncoding``), whose exact lists
    (``search.knn_join``) cost a pass over all pairs.
    Forward stage: ``self.search(rows[lo:hi], k', nprobe, shortlist=shortlist)`` for blocks of ``chunk`` rows (a contiguous copy of the
    block where the rows are strided); ``ids``, ``scores`` and ``scanned`` are kept, the probes dropped.  The forward lists are, by
    definition and to the bit, ``index.search(rows, k', nprobe, shortlist=shortlist)``, and ``chunk`` changes nothing.  The default
    chunk is ``min(query_chunk(nprobe, shortlist), 32768)``: ``search`` then takes a block in one step, its candidate buffers stay under
    ``CANDIDATE_MEMORY_CAP``, and the ``[chunk, lists]`` coarse scores, which that cap does not count, under half a GiB at 4096 lists.
    On an ``"i8"`` index ``shortlist`` is required (a ``ValueError`` without one): every returned score is then the exact chain's bits,
    which is also what the symmetry premise of the reverse stage needs.  On an ``"f32"`` index ``shortlist`` is refused, as ``search``
    refuses it.  After the forward stage there is one read-back, ``scanned.min()``: a row that scanned fewer than ``k'`` candidates is
    a ``ValueError`` that names ``nprobe`` (the graph kernels downstream are not specified on padded lists).
    Reverse stage (``reverse=True``; ``k' <= ops.KNN_REVERSE_MAX_K``, else a ``ValueError``): ``ops.knn_reverse_merge`` of the whole
    ``[N, k']`` result -- the chain is symmetric to the bit, so where i found j and j did not find i, i is offered to j at no scoring
    cost; ``gained[j]`` counts the entries row j took from such offers.  With ``reverse=False`` ``gained`` is zeros.
    A row's own match is present whenever its own list is among its probes.  That always holds for ``labels=None`` and for
    ``IVFIndex.train``, where a row's list is the argmax of the same coarse scores its probes are the top of; explicit labels can
    break it.
    With ``nprobe == lists`` the result is ``search.knn_join(None, rows, k)`` bit for bit and ``gained`` is all zero (on an ``"i8"``
    index this needs ``shortlist >= N``).

``IVFNeighbours(index, nprobe, shortlist=None, reverse=True)``
    What the re-ranking code carries in place of an int8 ``DescriptorIndex``: ``rerank`` calls ``index.knn_join(k, nprobe, shortlist,
    reverse)`` for its neighbour lists, after checking that its ``vecs`` are the index's ``rows``.

``index.close()`` releases the coarse index.
"""
from collections import namedtuple

import torch

from . import cluster, ops

IVFResult = namedtuple("IVFResult", ["ids", "scores", "probes", "scanned"])
IVFResult.__doc__ = """ids int64 [nq, k] and scores fp32 [nq, k]: the first k candidates of every query, best first (-1 / NaN beyond
its candidates); probes int64 [nq, nprobe]: the lists it probed, best first; scanned int64 [nq]: its candidates."""

IVFRescored = namedtuple("IVFRescored", ["ids", "scores", "probes", "scanned", "certified", "fallback"])
IVFRescored.__doc__ = """ids, scores, probes, scanned as in :data:`IVFResult`; certified int64 [nq]: the leading entries that are, bit for
bit, the fp32 index's (None without a shortlist); fallback int64 [f]: the queries answered by the fp32 scan (empty unless exact=True)."""

IVFKnnResult = namedtuple("IVFKnnResult", ["ids", "scores", "scanned", "gained"])
IVFKnnResult.__doc__ = """ids int64 [N, k'] and scores fp32 [N, k'] (k' = min(k, N)): the neighbour list of every row, best first;
scanned int64 [N]: the candidates of its forward search; gained int32 [N]: the entries it took from reverse edges."""

STORAGES = ("f32", "i8")

KNN_JOIN_CHUNK = 1 << 15          # the most rows per block of knn_join by default: the [chunk, lists] coarse scores stay small

CANDIDATE_MEMORY_CAP = 4 << 30    # bytes of candidate scores and ids ([chunk, capacity] fp32 + int64) one step of search may hold


def item_bound(tiles_np, tiles_all, nq):
    """An upper bound on the work items of ``ops.ivf_scan`` for ``nq`` queries that probe distinct lists each: list l makes
    ``tiles(l) * ceil(e(l) / G)`` items for its ``e(l)`` probing queries, and ``ceil(e / G) <= (e + G - 1) / G``, so the items are at
    most ``(sum_l tiles(l) e(l) + (G - 1) * sum_{l probed} tiles(l)) / G``.  The first sum is at most ``nq * tiles_np`` (``tiles_np``:
    the tiles of the ``nprobe`` lists with the most tiles), the second at most ``min(tiles_all, nq * tiles_np)``."""
    g = ops.IVF_QUERY_GROUP
    shared = nq * tiles_np
    return max(1, (shared + (g - 1) * min(tiles_all, shared)) // g)


class InvertedLists:
    """What :class:`IVFIndex` and ``ivfpq.IVFPQIndex`` share: the partition and what follows from its list sizes, the checks of a
    search's queries, and the two ends of a search step, between which each storage puts its scan.  ``n`` is the id bound and
    ``size`` the number of positions, which only an index that removes rows tells apart."""

    _home = "rows"             # what the queries must share a device with, in the words of the messages

    def _build(self, rows, centroids, labels, chunk):
        """Checks the arguments, makes the partition (``order``, ``offsets``, ``sizes`` and what ``_set_sizes`` derives, after the one
        read-back) and the coarse index; ``(labels, sizes)``: the labels, given or assigned, and the list sizes on the device."""
        _rows_matrix(rows, "rows")
        cluster._matrix(centroids, "centroids")
        if centroids.shape[1] != rows.shape[1]:
            raise ValueError("centroids are [K, %d] and rows [N, %d]: the dimensions differ" % (centroids.shape[1], rows.shape[1]))
        n, k = rows.shape[0], centroids.shape[0]
        _labels_fit(labels, rows, "rows")
        if chunk is not None:
            cluster._count(chunk, "chunk")
        cluster._on_device(rows, "rows")
        cluster._on_device(centroids, "centroids")
        if centroids.device != rows.device:
            raise ValueError("centroids are on %s and rows on %s" % (centroids.device, rows.device))
        if labels is not None:
            _labels_in_range(labels, k, rows.device, "rows")
        else:
            labels = cluster.assign(centroids, rows, chunk)[0]
        self.rows, self.centroids, self.fit = rows, centroids, None
        self.n, self.size, self.d, self.lists = n, n, rows.shape[1], k
        self.order, self.offsets, sizes = cluster._members(labels, k)
        self._set_sizes(sizes.cpu().tolist())                                   # the one read-back
        self.coarse = ops.DescriptorIndex(centroids, "ND")
        return labels, sizes

    def _set_sizes(self, host_sizes):
        """The list sizes on the host and what follows from them for every nprobe: the candidates and the tiles of the largest lists."""
        self.host_sizes = host_sizes
        self._capacity, self._tiles = [0], [0]
        for s in sorted(host_sizes, reverse=True):
            self._capacity.append(self._capacity[-1] + s)
            self._tiles.append(self._tiles[-1] + -(-s // ops.IVF_TILE))

    def capacity(self, nprobe):
        """The most candidates a query can have with ``nprobe`` probes: the sum of the ``nprobe`` largest list sizes (at least 1)."""
        return max(1, self._capacity[nprobe])

    def items(self, nq, nprobe):
        """The workgroups ``search`` launches for a list-major scan of ``nq`` queries: :func:`item_bound` of this index."""
        return item_bound(self._tiles[nprobe], self._tiles[-1], nq)

    def _check_search(self, queries, k, nprobe, qlayout, center):
        if self.coarse is None:
            raise ValueError("the index is closed")
        if not isinstance(queries, torch.Tensor) or queries.dtype != torch.float32 or queries.dim() != 2 or queries.numel() < 1:
            raise ValueError("queries must be a non-empty fp32 2-d tensor, got %s" % (
                "%s %s" % (queries.dtype, tuple(queries.shape)) if isinstance(queries, torch.Tensor) else type(queries).__name__))
        if qlayout not in ("ND", "DN"):
            raise ValueError("qlayout %r (\"ND\" or \"DN\")" % (qlayout,))
        dq = queries.shape[1] if qlayout == "ND" else queries.shape[0]
        if dq != self.d:
            raise ValueError("queries have dimension %d and the rows %d" % (dq, self.d))
        if not queries.is_contiguous():
            raise ValueError("queries must be contiguous")
        cluster._count(k, "k")
        if k > ops.RESCORE_MAX_K:
            raise ValueError("k = %d > %d" % (k, ops.RESCORE_MAX_K))
        cluster._count(nprobe, "nprobe")
        if nprobe > self.lists:
            raise ValueError("nprobe = %d > %d lists" % (nprobe, self.lists))
        if center is not None and (not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.numel() != self.d
                                   or not center.is_contiguous()):
            raise ValueError("center must be a contiguous fp32 tensor of %d elements" % self.d)
        cluster._on_device(queries, "queries")
        if queries.device != self.device:
            raise ValueError("queries are on %s and %s on %s" % (queries.device, self._home, self.device))
        if center is not None and center.device != self.device:
            raise ValueError("center is on %s and %s on %s" % (center.device, self._home, self.device))

    def _chunked(self, step, kind, chunk, queries, qlayout, *args):
        """``step`` on the queries ``chunk`` at a time; the parts of every field back to back (a field that is None stays None)."""
        nq = queries.shape[0] if qlayout == "ND" else queries.shape[1]
        if nq <= chunk:
            return step(queries, qlayout, *args)
        parts = []
        for q0 in range(0, nq, chunk):
            block = queries[q0:q0 + chunk] if qlayout == "ND" else queries[:, q0:q0 + chunk].contiguous()
            parts.append(step(block, qlayout, *args))
        return kind(*(None if parts[0][i] is None else torch.cat([p[i] for p in parts]) for i in range(len(parts[0]))))

    def _probe(self, queries, qlayout, center, nprobe):
        """The front half of a search step: ``(probes, their coarse values, plan, cap)``.  The plan counts positions (``size``)."""
        probes, coarse = ops.topk(self.coarse.scores(queries, qlayout, center=center), nprobe)
        cap = self.capacity(nprobe)
        return probes, coarse, ops.ivf_plan(probes, self.offsets, self.size, cap), cap

    def _select(self, cand_scores, cand_ids, plan, nprobe, k):
        """The tail of a search step: ``(ids, scores)`` of the first ``k`` candidates, and ``scanned``, the plan's count of them."""
        ids, scores = ops.ivf_select(cand_scores, cand_ids, plan, nprobe, self.lists, k)
        return ids, scores, ops.ivf_plan_views(plan, ids.shape[0], nprobe, self.lists)["count"].clone()

    # The -1 ids that pad a shortlist go to its second stage as the id n (the id bound): never dereferenced, scored NaN, and behind
    # every candidate in the order of the rescored row, where the fp32 search has its padding.  They come back as -1.
    def _pad_in(self, ids):
        return torch.where(ids < 0, self.n, ids)

    def _pad_out(self, ids):
        return torch.where(ids >= self.n, -1, ids)

    def close(self):
        """Releases the coarse index."""
        if self.coarse is not None:
            self.coarse.close()
            self.coarse = None


class IVFIndex(InvertedLists):
    """The inverted file of ``rows`` over ``centroids`` -- the module docstring states the contract."""

    storage, codes, scales, bounds = "f32", None, None, None
    device = property(lambda self: self.rows.device)

    def __init__(self, rows, centroids, labels=None, chunk=None, storage="f32"):
        if storage not in STORAGES:
            raise ValueError("storage %r (\"f32\" or \"i8\")" % (storage,))
        self.labels, self.sizes = self._build(rows, centroids, labels, chunk)
        self.storage = storage
        if storage == "i8":
            self.codes, self.scales = ops.lists_i8_encode(rows, self.order)
            self.bounds = ops.lists_i8_bounds(self.codes, self.scales, self.d)

    @classmethod
    def train(cls, rows, lists, storage="f32", **kmeans_kwargs):
        """The index of ``cluster.kmeans(rows, lists, **kmeans_kwargs)``; the fit stays reachable as ``.fit``."""
        if storage not in STORAGES:
            raise ValueError("storage %r (\"f32\" or \"i8\")" % (storage,))
        fit = cluster.kmeans(rows, lists, **kmeans_kwargs)
        index = cls(rows, fit.centroids, fit.labels, storage=storage)
        index.fit = fit
        return index

    def query_chunk(self, nprobe, shortlist=None):
        """Queries per step of ``search``: as many as keep the candidate block under ``CANDIDATE_MEMORY_CAP`` bytes (at least one).  On an
        int8 index a query also holds its centred row, codes and scale (``5 d + 4`` bytes) and, with a shortlist of ``S``, the int8
        selection, the rescored pairs and the unsorted scores (``28 S``) and its depth and bound (8)."""
        per_query = 12 * self.capacity(nprobe)
        if self.storage == "i8":
            per_query += 5 * self.d + 4 + (0 if shortlist is None else 28 * shortlist + 8)
        return max(1, CANDIDATE_MEMORY_CAP // per_query)

    def _check_stages(self, k, shortlist, exact):
        cluster._count(k, "k")
        if not isinstance(exact, bool):
            raise ValueError("exact must be a bool, got %r" % (exact,))
        if self.storage != "i8":
            if shortlist is not None or exact:
                raise ValueError("shortlist and exact need an int8 index (storage=\"i8\"); this one is %s" % self.storage)
            return
        if shortlist is not None:
            cluster._count(shortlist, "shortlist")
            if not k <= shortlist <= ops.RESCORE_MAX_K:
                raise ValueError("shortlist = %d must be in [k = %d, %d]" % (shortlist, k, ops.RESCORE_MAX_K))
        elif exact:
            raise ValueError("exact=True needs a shortlist")

    def search(self, queries, k, nprobe, qlayout="ND", center=None, shortlist=None, exact=False):
        """:data:`IVFResult` (an int8 index: :data:`IVFRescored`) of the ``k`` best rows of every query among the members of its
        ``nprobe`` best lists -- the module docstring has the contract."""
        self._check_stages(k, shortlist, exact)
        self._check_search(queries, k, nprobe, qlayout, center)
        if self.storage != "i8":
            return self._chunked(self._search, IVFResult, self.query_chunk(nprobe), queries, qlayout, k, nprobe, center)
        res = self._chunked(self._search_i8, IVFRescored, self.query_chunk(nprobe, shortlist), queries, qlayout, k, nprobe, center, shortlist)
        if not exact:
            return res
        fallback = torch.nonzero(res.certified < k).reshape(-1)                 # the one read-back: how many queries run again
        if fallback.numel():
            again = queries[fallback] if qlayout == "ND" else queries[:, fallback].contiguous()
            sure = self._chunked(self._search, IVFResult, self.query_chunk(nprobe), again, qlayout, k, nprobe, center)
            res.ids.index_copy_(0, fallback, sure.ids)
            res.scores.index_copy_(0, fallback, sure.scores)
        return res._replace(fallback=fallback)

    def _search(self, queries, qlayout, k, nprobe, center):
        probes, _, plan, cap = self._probe(queries, qlayout, center, nprobe)
        cand_scores, cand_ids = ops.ivf_scan(self.rows, self.order, self.offsets, queries, plan, nprobe, cap,
                                             self.items(probes.shape[0], nprobe), qlayout, None if center is None else center.reshape(-1))
        ids, scores, scanned = self._select(cand_scores, cand_ids, plan, nprobe, k)
        return IVFResult(ids, scores, probes, scanned)

    def _search_i8(self, queries, qlayout, k, nprobe, center, shortlist):
        center = None if center is None else center.reshape(-1)
        probes, _, plan, cap = self._probe(queries, qlayout, center, nprobe)
        qcodes, qscales = ops.quantize_i8(ops.center_rows(queries, qlayout, center))
        cand_scores, cand_ids = ops.lists_i8_scan(self.codes, self.scales, self.d, self.order, self.offsets, qcodes, qscales, plan, nprobe,
                                                  cap, self.items(probes.shape[0], nprobe))
        ids, scores, scanned = self._select(cand_scores, cand_ids, plan, nprobe, k if shortlist is None else shortlist)
        none = torch.empty(0, dtype=torch.int64, device=self.rows.device)
        if shortlist is None:
            return IVFRescored(ids, scores, probes, scanned, None, none)
        del cand_scores, cand_ids
        sure_ids, sure = ops.rescore(self.rows, queries, self._pad_in(ids), qlayout, center)
        sure_ids = self._pad_out(sure_ids)
        depth, _ = ops.rescore_certify(sure, scores[:, shortlist - 1], queries, self.bounds, max(self.n, shortlist), qlayout, center)
        certified = torch.where(scanned <= shortlist, shortlist, depth.to(torch.int64))
        return IVFRescored(sure_ids[:, :k].contiguous(), sure[:, :k].contiguous(), probes, scanned, certified, none)

    def knn_join(self, k, nprobe, shortlist=None, reverse=True, chunk=None):
        """:data:`IVFKnnResult`: the ``min(k, N)`` best rows of every row among the members of its ``nprobe`` best lists, merged with
        their reverse edges -- the module docstring has the contract."""
        cluster._count(k, "k")
        k = min(k, self.n)
        if not isinstance(reverse, bool):
            raise ValueError("reverse must be a bool, got %r" % (reverse,))
        if chunk is not None:
            cluster._count(chunk, "chunk")
        if self.storage == "i8" and shortlist is None:
            raise ValueError("knn_join on an int8 index needs a shortlist: its scores are then the exact chain's, which the reverse "
                             "merge and the re-ranking rest on")
        self._check_stages(k, shortlist, False)
        if reverse and k > ops.KNN_REVERSE_MAX_K:
            raise ValueError("knn_join: k = %d > %d with reverse=True (ops.KNN_REVERSE_MAX_K)" % (k, ops.KNN_REVERSE_MAX_K))
        cluster._count(nprobe, "nprobe")
        if nprobe > self.lists:
            raise ValueError("nprobe = %d > %d lists" % (nprobe, self.lists))
        if self.coarse is None:
            raise ValueError("the index is closed")
        if chunk is None:
            chunk = min(self.query_chunk(nprobe, shortlist), KNN_JOIN_CHUNK)
        n, device = self.n, self.rows.device
        ids = torch.empty((n, k), dtype=torch.int64, device=device)
        scores = torch.empty((n, k), dtype=torch.float32, device=device)
        scanned = torch.empty((n,), dtype=torch.int64, device=device)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            res = self.search(self.rows[lo:hi].contiguous(), k, nprobe, shortlist=shortlist)
            ids[lo:hi], scores[lo:hi], scanned[lo:hi] = res.ids, res.scores, res.scanned
            del res
        least = int(scanned.min())                                              # the one read-back
        if least < k:
            raise ValueError("knn_join: a row scanned %d candidates, fewer than k = %d: nprobe = %d is too small for these lists"
                             % (least, k, nprobe))
        if not reverse:
            return IVFKnnResult(ids, scores, scanned, torch.zeros((n,), dtype=torch.int32, device=device))
        ids, scores, gained = ops.knn_reverse_merge(ids, scores)
        return IVFKnnResult(ids, scores, scanned, gained)

class IVFNeighbours:
    """An :class:`IVFIndex` with the arguments of its ``knn_join``: the handle ``rerank.database_augmentation``,
    ``rerank.DiffusionGraph`` and ``rerank.ReciprocalEncoding`` take as ``index=`` beside an int8 ``DescriptorIndex``.  The
    neighbour lists are then approximate (the module docstring says how), and the ``vecs`` of the call must be the index's ``rows``."""

    def __init__(self, index, nprobe, shortlist=None, reverse=True):
        if not isinstance(index, IVFIndex):
            raise ValueError("IVFNeighbours: index must be an IVFIndex, got %s" % type(index).__name__)
        cluster._count(nprobe, "nprobe")
        if nprobe > index.lists:
            raise ValueError("nprobe = %d > %d lists" % (nprobe, index.lists))
        if shortlist is not None:
            cluster._count(shortlist, "shortlist")
        if not isinstance(reverse, bool):
            raise ValueError("reverse must be a bool, got %r" % (reverse,))
        self.index, self.nprobe, self.shortlist, self.reverse = index, nprobe, shortlist, reverse

    def lists_of(self, vecs, k):
        """``(ids, scores)`` of ``index.knn_join(k, nprobe, shortlist, reverse)``; ``vecs`` must be the index's rows."""
        rows = self.index.rows
        if not isinstance(vecs, torch.Tensor) or vecs.data_ptr() != rows.data_ptr() or tuple(vecs.shape) != tuple(rows.shape) \
                or vecs.stride() != rows.stride():
            raise ValueError("IVFNeighbours: vecs must be the rows the index was built on (same storage, shape and strides)")
        res = self.index.knn_join(k, self.nprobe, shortlist=self.shortlist, reverse=self.reverse)
        return res.ids, res.scores


def _labels_fit(labels, vectors, what):
    """Explicit labels are an int64 tensor with one entry per vector; without them the vectors (named ``what``) must be contiguous."""
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (vectors.shape[0],):
            raise ValueError("labels must be an int64 [%d] tensor, got %s" % (
                vectors.shape[0], "%s %s" % (labels.dtype, tuple(labels.shape)) if isinstance(labels, torch.Tensor) else type(labels).__name__))
    elif not vectors.is_contiguous():
        raise ValueError("%s must be contiguous to be assigned (labels=None)" % what)


def _labels_in_range(labels, lists, device, home):
    """Explicit labels lie on ``device`` (where ``home`` is, in the words of the message) and in ``[0, lists)`` -- one read-back."""
    cluster._on_device(labels, "labels")
    if labels.device != device:
        raise ValueError("labels are on %s and %s on %s" % (labels.device, home, device))
    low, high = int(labels.min()), int(labels.max())
    if low < 0 or high >= lists:
        raise ValueError("labels must lie in [0, %d), got %d .. %d" % (lists, low, high))


def _rows_matrix(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be a non-empty fp32 [rows, D] tensor, got %s" % (
            what, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s must have contiguous rows" % what)
