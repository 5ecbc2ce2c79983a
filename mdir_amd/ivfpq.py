"""An inverted file over product-quantised residuals (IVF-PQ): M bytes per row, scanned by table look-ups.

``ivf.IVFIndex`` scores the rows of the probed lists themselves (fp32, or int8 beside the fp32 rows).  This index keeps, per row, the
``pq`` code of its residual against the centroid of its list -- ``M`` bytes -- and its id, and scores a candidate by asymmetric
distance computation (ADC): the coarse score of the list plus ``M`` entries of a table built once per query
(include/mdx_lists_pq.h).  The fp32 rows are optional: they serve an exact second stage only.  Every result is defined to the bit;
``tests/pq_restatement.py`` states the search in numpy.

``IVFPQIndex(rows, centroids, labels=None, m=64, codebook=None, keep_rows=True, chunk=None, **pq_train_kwargs)``
    ``rows``, ``centroids``, ``labels`` and ``chunk`` as for ``ivf.IVFIndex``, which builds the partition: ``order``, ``offsets``, the
    list sizes on the host, ``capacity(nprobe)`` and ``coarse``, the fp32 index of the centroids, are its.  ``D % m == 0`` and
    ``1 <= m <= ops.PQ_MAX_M``.  The residuals ``r = row - centroids[label]`` (one fp32 subtraction per element) are taken in list
    order, ``chunk`` rows at a time (default ``pq.CHUNK``).  ``codebook=None`` runs ``pq.train(residuals, m, **pq_train_kwargs)`` on all
    of them (a transient fp32 ``[N, D]`` block; ``N >= 256``); a :data:`pq.Codebook` is taken as it is.  ``codes`` uint8 ``[N, m]`` is
    ``pq.encode`` of the residuals: position ``p`` holds the code of row ``order[p]``.  With ``keep_rows=False`` the index drops its
    reference to ``rows``.  Neither the labels nor the centroids are kept: ``order`` and ``offsets`` state the former, ``coarse`` holds
    the latter.  ``nbytes()`` is what the index holds on the device: the codes, ``order``, ``offsets``, the codebook, the coarse
    index, and the rows if they are kept.

``IVFPQIndex.train(rows, lists, m=64, kmeans=None, pq=None, keep_rows=True)``
    ``cluster.kmeans(rows, lists, **kmeans)``, then the index of ``fit.centroids`` and ``fit.labels`` with ``**pq`` handed to
    ``pq.train``; the :data:`cluster.KMeans` result stays reachable as ``.fit``.

``index.search(queries, k, nprobe, qlayout="ND", center=None, shortlist=None)`` -> :data:`IVFPQResult`
    1. the coarse scores ``coarse.scores(queries, qlayout, center=center)``;
    2. ``ops.topk`` of them: ``probes`` and their values;
    3. ``ops.ivf_plan``;
    4. ``ops.pq_lut``: per query the exact chain of its sub-vectors with every codeword;
    5. ``ops.lists_pq_scan``: a candidate's score is the probe's coarse value plus the ``m`` table entries of its code, added in
       subspace order in fp32;
    6. ``ops.ivf_select``: the first ``k`` candidates in ``rank_full``'s order, padded with -1 / NaN where ``scanned[q] < k``.
    Without a shortlist that is the result: the ADC ranking.  With ``shortlist=S`` (``k <= S <= ops.RESCORE_MAX_K``; needs
    ``keep_rows=True``) the ``S`` best by ADC score are rescored with ``ops.rescore`` on the fp32 rows and the first ``k`` returned:
    every returned score is the exact chain's bits, and where ``scanned[q] <= S`` the whole row, padding included, is that of
    ``ivf.IVFIndex(rows, centroids, labels).search``.  (The padding id goes to ``ops.rescore`` as the id ``N`` and comes back as -1, as
    in ``ivf.py``.)  There is no certificate for the ADC shortlist.
    The queries are taken ``query_chunk(nprobe, shortlist)`` at a time under ``ivf.CANDIDATE_MEMORY_CAP``; a query holds its candidate
    row (12 bytes a column), its table (``m`` KiB) and, with a shortlist, ``28 S`` bytes.  The chunk changes no bit.  Nothing is read
    back and nothing synchronises.  There is no CPU fallback.

``index.close()`` releases the coarse index.
"""
from collections import namedtuple

import torch

from . import cluster, ivf, ops, pq as _pq

IVFPQResult = namedtuple("IVFPQResult", ["ids", "scores", "probes", "scanned"])
IVFPQResult.__doc__ = """ids int64 [nq, k] and scores fp32 [nq, k]: the first k candidates of every query, best first (-1 / NaN beyond
its candidates) -- ADC scores without a shortlist, exact chain scores with one; probes int64 [nq, nprobe]: the lists it probed, best
first; scanned int64 [nq]: its candidates."""


class IVFPQIndex:
    """The inverted file of the product-quantised residuals of ``rows`` over ``centroids`` -- the module docstring states the
    contract."""

    def __init__(self, rows, centroids, labels=None, m=64, codebook=None, keep_rows=True, chunk=None, **pq_train_kwargs):
        ivf._rows_matrix(rows, "rows")
        dsub = _pq._subspaces(m, rows.shape[1])
        if not isinstance(keep_rows, bool):
            raise ValueError("keep_rows must be a bool, got %r" % (keep_rows,))
        if codebook is not None:
            if pq_train_kwargs:
                raise ValueError("a codebook is given: %s would not be used" % sorted(pq_train_kwargs))
            words, m_have, dsub_have = _pq._codebook(codebook)
            if (m_have, dsub_have) != (m, dsub):
                raise ValueError("the codebook is [%d, %d, %d] and m = %d, D = %d need [%d, %d, %d]" % (
                    m_have, _pq.CODEWORDS, dsub_have, m, rows.shape[1], m, _pq.CODEWORDS, dsub))
        elif rows.shape[0] < _pq.CODEWORDS:
            raise ValueError("N = %d rows: pq.train needs at least %d" % (rows.shape[0], _pq.CODEWORDS))
        partition = ivf.IVFIndex(rows, centroids, labels, chunk)       # every other check, the lists, the capacities, the coarse index
        self.n, self.d, self.lists, self.m = partition.n, partition.d, partition.lists, m
        self.order, self.offsets, self.host_sizes = partition.order, partition.offsets, partition.host_sizes
        self._capacity, self.coarse, self.fit = partition._capacity, partition.coarse, None
        self.device = rows.device
        try:
            step = min(self.n, chunk or _pq.CHUNK)
            if codebook is None:
                residuals = torch.empty((self.n, self.d), dtype=torch.float32, device=self.device)
                for p0 in range(0, self.n, step):
                    residuals[p0:p0 + step] = self._residuals(rows, centroids, partition.labels, p0, p0 + step)
                codebook = _pq.train(residuals, m, chunk=chunk, **pq_train_kwargs)
                self.codes = _pq.encode(codebook, residuals, chunk)
                del residuals
            else:
                if words.device != self.device:
                    raise ValueError("the codebook is on %s and rows on %s" % (words.device, self.device))
                self.codes = torch.empty((self.n, m), dtype=torch.uint8, device=self.device)
                for p0 in range(0, self.n, step):
                    self.codes[p0:p0 + step] = _pq.encode(codebook, self._residuals(rows, centroids, partition.labels, p0, p0 + step))
        except BaseException:
            self.close()
            raise
        self.codebook = codebook if isinstance(codebook, _pq.Codebook) else _pq.Codebook(codebook, [], 0)
        self.rows = rows if keep_rows else None

    def _residuals(self, rows, centroids, labels, p0, p1):
        """fp32 [p1 - p0, D]: row - centroids[label] of the rows at positions p0 .. p1 of the list order."""
        ids = self.order[p0:p1]
        return rows.index_select(0, ids) - centroids.index_select(0, labels.index_select(0, ids))

    @classmethod
    def train(cls, rows, lists, m=64, kmeans=None, pq=None, keep_rows=True):
        """The index of ``cluster.kmeans(rows, lists, **kmeans)`` with ``pq.train(residuals, m, **pq)``; the fit stays reachable as
        ``.fit``."""
        ivf._rows_matrix(rows, "rows")
        _pq._subspaces(m, rows.shape[1])
        fit = cluster.kmeans(rows, lists, **(kmeans or {}))
        index = cls(rows, fit.centroids, fit.labels, m=m, keep_rows=keep_rows, **(pq or {}))
        index.fit = fit
        return index

    def nbytes(self):
        """The bytes the index holds on the device: codes, order, offsets, codebook, coarse index, and the rows if they are kept."""
        held = self.codes.numel() + 8 * self.order.numel() + 8 * self.offsets.numel() + 4 * self.codebook.codewords.numel()
        held += self.coarse.device_bytes if self.coarse is not None else 0
        if self.rows is not None:
            held += 4 * self.rows.shape[0] * (self.rows.stride(0) if self.rows.shape[0] > 1 else self.rows.shape[1])
        return held

    def capacity(self, nprobe):
        """The most candidates a query can have with ``nprobe`` probes: the sum of the ``nprobe`` largest list sizes (at least 1)."""
        return max(1, self._capacity[nprobe])

    def query_chunk(self, nprobe, shortlist=None):
        """Queries per step of ``search``: as many as keep their candidate rows (12 bytes a column), their tables (``m`` KiB each) and,
        with a shortlist of ``S``, the selection and the rescored pairs (``28 S``) under ``ivf.CANDIDATE_MEMORY_CAP`` (at least one)."""
        per_query = 12 * self.capacity(nprobe) + 4 * _pq.CODEWORDS * self.m + (0 if shortlist is None else 28 * shortlist)
        return max(1, ivf.CANDIDATE_MEMORY_CAP // per_query)

    def _check_search(self, queries, k, nprobe, qlayout, center, shortlist):
        if self.coarse is None:
            raise ValueError("the index is closed")
        cluster._count(k, "k")
        if k > ops.RESCORE_MAX_K:
            raise ValueError("k = %d > %d" % (k, ops.RESCORE_MAX_K))
        if shortlist is not None:
            cluster._count(shortlist, "shortlist")
            if not k <= shortlist <= ops.RESCORE_MAX_K:
                raise ValueError("shortlist = %d must be in [k = %d, %d]" % (shortlist, k, ops.RESCORE_MAX_K))
            if self.rows is None:
                raise ValueError("a shortlist is rescored on the fp32 rows; this index was built with keep_rows=False")
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
        cluster._count(nprobe, "nprobe")
        if nprobe > self.lists:
            raise ValueError("nprobe = %d > %d lists" % (nprobe, self.lists))
        if center is not None and (not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or center.numel() != self.d
                                   or not center.is_contiguous()):
            raise ValueError("center must be a contiguous fp32 tensor of %d elements" % self.d)
        cluster._on_device(queries, "queries")
        if queries.device != self.device:
            raise ValueError("queries are on %s and the index on %s" % (queries.device, self.device))
        if center is not None and center.device != self.device:
            raise ValueError("center is on %s and the index on %s" % (center.device, self.device))

    def search(self, queries, k, nprobe, qlayout="ND", center=None, shortlist=None):
        """:data:`IVFPQResult` of the ``k`` best rows of every query among the members of its ``nprobe`` best lists, by ADC score or,
        with a shortlist, by the exact score of the ADC shortlist -- the module docstring has the contract."""
        self._check_search(queries, k, nprobe, qlayout, center, shortlist)
        return ivf.IVFIndex._chunked(self, self._search, IVFPQResult, self.query_chunk(nprobe, shortlist), queries, qlayout, k, nprobe,
                                     center, shortlist)

    def _search(self, queries, qlayout, k, nprobe, center, shortlist):
        nq = queries.shape[0] if qlayout == "ND" else queries.shape[1]
        center = None if center is None else center.reshape(-1)
        probes, coarse = ops.topk(self.coarse.scores(queries, qlayout, center=center), nprobe)
        cap = self.capacity(nprobe)
        plan = ops.ivf_plan(probes, self.offsets, self.n, cap)
        lut = ops.pq_lut(self.codebook.codewords, queries, qlayout, center)
        cand_scores, cand_ids = ops.lists_pq_scan(self.codes, self.order, self.n, self.offsets, lut, coarse, probes, plan, cap)
        ids, scores = ops.ivf_select(cand_scores, cand_ids, plan, nprobe, self.lists, k if shortlist is None else shortlist)
        scanned = ops.ivf_plan_views(plan, nq, nprobe, self.lists)["count"].clone()
        if shortlist is None:
            return IVFPQResult(ids, scores, probes, scanned)
        del cand_scores, cand_ids, lut
        # the padding of a shortlist as the id n: not dereferenced, NaN, and behind every candidate in the order of the rescored row
        sure_ids, sure = ops.rescore(self.rows, queries, torch.where(ids < 0, self.n, ids), qlayout, center)
        sure_ids = torch.where(sure_ids >= self.n, -1, sure_ids)
        return IVFPQResult(sure_ids[:, :k].contiguous(), sure[:, :k].contiguous(), probes, scanned)

    def close(self):
        """Releases the coarse index."""
        if self.coarse is not None:
            self.coarse.close()
            self.coarse = None
