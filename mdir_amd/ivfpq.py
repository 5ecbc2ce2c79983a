"""An inverted file over product-quantised residuals (IVF-PQ): M bytes per row, scanned by table look-ups.

``ivf.IVFIndex`` scores the rows of the probed lists themselves (fp32, or int8 beside the fp32 rows).  This index keeps, per row, the
``pq`` code of its residual against the centroid of its list -- ``M`` bytes -- and its id, and scores a candidate by asymmetric
distance computation (ADC): the coarse score of the list plus ``M`` entries of a table built once per query
(include/mdx_lists_pq.h).  The fp32 rows are optional: they serve an exact second stage only.  Every result is defined to the bit;
``tests/pq_restatement.py`` states the search in numpy.

``IVFPQIndex(rows, centroids, labels=None, m=64, codebook=None, keep_rows=True, chunk=None, refine=None, **pq_train_kwargs)``
    ``rows``, ``centroids``, ``labels`` and ``chunk`` as for ``ivf.IVFIndex``; the base the two share, ``ivf.InvertedLists``, builds the
    partition: ``order``, ``offsets``, the list sizes on the host, ``capacity(nprobe)`` and ``coarse``, the fp32 index of the
    centroids, are its.  ``D % m == 0`` and
    ``1 <= m <= ops.PQ_MAX_M``.  The residuals ``r = row - centroids[label]`` (one fp32 subtraction per element) are taken in list
    order, ``chunk`` rows at a time (default ``pq.CHUNK``).  ``codebook=None`` runs ``pq.train(residuals, m, **pq_train_kwargs)`` on all
    of them (a transient fp32 ``[N, D]`` block; ``N >= 256``); a :data:`pq.Codebook` is taken as it is.  ``codes`` uint8 ``[N, m]`` is
    ``pq.encode`` of the residuals: position ``p`` holds the code of row ``order[p]``.  With ``keep_rows=False`` the index drops its
    reference to ``rows``.  The labels are not kept: ``order`` and ``offsets`` state them.  ``centroids`` stays referenced (it is the
    caller's tensor; ``coarse`` holds its own copy).  ``nbytes()`` is what the index holds on the device: the codes, ``order``,
    ``offsets``, the codebook, the coarse index, and the rows if they are kept -- the centroids are the caller's and are mirrored by
    ``coarse``, so they are not counted a second time.
    ``refine=None`` is the index described so far.  ``refine="i8"`` (``D <= 133120``; any other value is a ``ValueError``) keeps a
    second-level code beside the PQ codes (include/mdx_refine.h): ``refine_codes`` int8 ``[size, round_up(D, 64)]`` and
    ``refine_scales`` fp32 ``[size]``, ``ops.lists_i8_encode(rows, order)`` -- the ``MDX_I8`` quantisation of the row at every position
    -- and ``where`` int64 ``[n]``, the inverse of ``order`` with -1 at ids that are not live (derived: rebuilt after every change of
    ``order``, never part of ``state()``).  ``nbytes()`` counts all three: about ``N (m + round_up(D, 64) + 20)`` bytes in all.

``IVFPQIndex.train(rows, lists, m=64, kmeans=None, pq=None, keep_rows=True, refine=None)``
    ``cluster.kmeans(rows, lists, **kmeans)``, then the index of ``fit.centroids`` and ``fit.labels`` with ``**pq`` handed to
    ``pq.train``; the :data:`cluster.KMeans` result stays reachable as ``.fit``.

``index.search(queries, k, nprobe, qlayout="ND", center=None, shortlist=None, rescore=None)`` -> :data:`IVFPQResult`
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
    in ``ivf.py``.)  There is no certificate for the ADC shortlist.  ``rescore`` other than ``None`` is a ``ValueError`` on such an
    index.
    On a ``refine="i8"`` index ``shortlist=None`` is the ADC ranking as above (``rescore`` must be ``None``), and with ``shortlist=S``:
    ``rescore=None``  7. ``ops.quantize_i8(ops.center_rows(queries, qlayout, center))``: the query codes; 8. ``ops.refine_i8`` scores
        the ``S`` best by ADC score on ``refine_codes`` and sorts them; the first ``k`` are returned.  No fp32 rows are needed.  The
        padding goes in as the id ``n`` and comes back as -1, as above.
    ``rescore=R`` (``k <= R <= S``; needs the fp32 rows, kept or attached)  9. the first ``R`` of the refined row go through
        ``ops.rescore``; the first ``k`` are returned.  ``rescore=S`` is the rescoring of all of ``S`` in fp32.
    What holds, and the tests check:
    (a) every score returned with ``rescore=None`` is the bit pattern of ``DescriptorIndex(rows, "ND", storage="i8").scores(queries,
        qlayout, center)`` at ``[q, id]``;
    (b) where ``scanned[q] <= S`` the row equals the row of ``ivf.IVFIndex(rows, centroids, labels, storage="i8").search(queries, k,
        nprobe, qlayout, center)`` -- ids, score bits and padding: both are the int8 ranking of the same candidates under the same
        order, computed independently by the gather kernel here and the MFMA scan there;
    (c) with ``rescore=R`` and ``scanned[q] <= R`` the row equals the fp32 ``ivf.IVFIndex`` search's row;
    (d) every returned row is that of ``tests/refine_restatement.py`` bit for bit, whatever the query chunk.
    There is no certificate for the refined shortlist either.
    The queries are taken ``query_chunk(nprobe, shortlist)`` at a time under ``ivf.CANDIDATE_MEMORY_CAP``; a query holds its candidate
    row (12 bytes a column), its table (``m`` KiB) and, with a shortlist, ``28 S`` bytes -- on a ``refine="i8"`` index also its
    centred row, codes and scale (``5 d + 4``) and the refined pairs (``16 S``).  The chunk changes no bit.  Nothing is read back
    and nothing synchronises.  There is no CPU fallback.

``index.close()`` releases the coarse index.

After the build.  The index keeps a reference to the caller's ``centroids`` tensor (the residuals of a batch need it; ``coarse`` mirrors
it in its own layout, so ``nbytes()`` does not count it a second time) and two numbers: ``index.n``, the id bound -- one more than the
largest id ever issued -- and ``index.size``, the live rows, ``codes.shape[0]``.  They differ after a removal; the plan of a search
takes ``size`` (offsets are clamped to the number of positions), the scan and the rescore padding ``n`` (the id bound).  A list's
members ascend in id and new ids are larger than all old ones, so a batch is a small list-ordered structure of its own and adding it is
a per-list concatenation (include/mdx_lists_edit.h; ``tests/lists_edit_restatement.py`` states the merge and the compaction in numpy).

``index.add(batch, labels=None, chunk=None)`` -> ids int64 ``[B]``: ``n .. n + B - 1``
    ``batch`` fp32 ``[B, D]`` on the index's device, rows contiguous; ``labels`` as for the constructor (``None``:
    ``cluster.assign(index.centroids, batch, chunk)[0]``; explicit labels are range-checked with the one read-back the constructor
    makes too).  1. ``cluster._members(labels, lists)`` of the batch; 2. the residuals of the batch in that order, ``chunk`` rows at a
    time, by the expression of the constructor; 3. ``pq.encode`` with the index's codebook; 4. ``ops.lists_merge`` of the index's
    structure with the batch's, whose members are ``n + batch_members``; 5. one read-back of the ``lists`` list sizes, for
    ``host_sizes`` and ``capacity(.)``; 6. ``n += B`` and ``size += B``.  On any failure the index is left as it was.  Every step is
    per row and independent of the chunk, so for any split of ``rows`` into consecutive batches the constructor on the first (with
    ``codebook=`` given and ``keep_rows=False``) followed by ``add`` of the others has ``codes``, ``order``, ``offsets``, ``host_sizes``
    and ``capacity(.)`` equal to those of the constructor on all of ``rows`` with the same centroids, codebook and labels (or ``None``):
    every search result is equal bit for bit.  Every ``add`` rewrites the structure once, ``size (m + 8)`` bytes; there is no slack
    capacity inside the lists.  On a ``refine="i8"`` index the batch is also encoded with ``ops.lists_i8_encode(batch, members)`` and
    ``refine_codes`` (as uint8 ``[size, round_up(D, 64)]``) and ``refine_scales`` (as uint8 ``[size, 4]``) go through the same
    ``ops.lists_merge`` beside the PQ codes; the split-build guarantee extends to ``refine_codes``, ``refine_scales`` and ``where``
    (same codebook, ``refine="i8"`` on both sides).

``index.remove(ids)`` -> the number of rows removed
    ``ids`` int64 on the index's device, in any order; duplicates are allowed, and ids that are not live (negative, ``>= n``, already
    removed) are ignored.  1. a dead flag per id in ``[0, n)``; 2. the keep flags of ``order``; 3. their exclusive prefix
    (``torch.cumsum``); 4. one read-back of the new list sizes and the count (before the rows move, so that the result is allocated
    at its size); 5. ``ops.lists_compact``.  Ids are never reused: ``n`` is unchanged and a later ``add`` continues at ``n``.  A removal
    that would leave no row is a ``ValueError`` and changes nothing (the scan refuses ``m < 1``).  On a ``refine="i8"`` index
    ``refine_codes`` and ``refine_scales`` are compacted with the same ``kept`` and ``where`` is rebuilt.

``index.attach_rows(rows)``
    For an index that does not keep the rows: ``rows`` fp32 ``[n, D]`` on the index's device, rows contiguous, becomes ``index.rows``,
    so ``shortlist=`` works again; the rows at removed ids are never read.  ``attach_rows(None)`` drops the reference.  ``add`` and
    ``remove`` on an index that currently keeps rows are a ``ValueError`` -- ``attach_rows(None)`` first: the index never copies or grows
    the caller's tensor.

``index.state()`` -> dict of ``centroids``, ``codewords``, ``codes``, ``order``, ``offsets`` (the index's own tensors, not copies), ``n``, ``m``
``IVFPQIndex.from_state(state, device=None, rows=None)``
    The index of a state: the tensors are moved to ``device`` (``None``: where the codes are), the coarse index and the capacities are
    rebuilt from the centroids and the offsets (one read-back), ``rows`` goes to ``attach_rows``.  Its searches equal the original's bit
    for bit.  Writing to disk is the caller's: ``torch.save(index.state(), path)``.  The state of a ``refine="i8"`` index also holds
    ``refine_codes`` and ``refine_scales``; ``from_state`` checks their dtypes and shapes against ``codes`` and ``centroids``, rebuilds
    ``where`` and gives a ``refine="i8"`` index.  A state without those keys loads as a ``refine=None`` index.
"""
from collections import namedtuple

import torch

from . import cluster, ivf, ops, pq as _pq

IVFPQResult = namedtuple("IVFPQResult", ["ids", "scores", "probes", "scanned"])
IVFPQResult.__doc__ = """ids int64 [nq, k] and scores fp32 [nq, k]: the first k candidates of every query, best first (-1 / NaN beyond
its candidates) -- ADC scores without a shortlist, exact chain scores with one; probes int64 [nq, nprobe]: the lists it probed, best
first; scanned int64 [nq]: its candidates."""


REFINES = (None, "i8")


def _check_refine(refine, d):
    if refine is not None and not (isinstance(refine, str) and refine in REFINES):
        raise ValueError("refine must be None or \"i8\", got %r" % (refine,))
    if refine == "i8" and d > ops.LISTS_I8_MAX_D:
        raise ValueError("refine=\"i8\": D = %d > %d" % (d, ops.LISTS_I8_MAX_D))


class IVFPQIndex(ivf.InvertedLists):
    """The inverted file of the product-quantised residuals of ``rows`` over ``centroids`` -- the module docstring states the
    contract."""

    refine = None              # "i8": refine_codes, refine_scales and where are kept
    _home = "the index"

    def __init__(self, rows, centroids, labels=None, m=64, codebook=None, keep_rows=True, chunk=None, refine=None, **pq_train_kwargs):
        ivf._rows_matrix(rows, "rows")
        dsub = _pq._subspaces(m, rows.shape[1])
        if not isinstance(keep_rows, bool):
            raise ValueError("keep_rows must be a bool, got %r" % (keep_rows,))
        _check_refine(refine, rows.shape[1])
        if codebook is not None:
            if pq_train_kwargs:
                raise ValueError("a codebook is given: %s would not be used" % sorted(pq_train_kwargs))
            words, m_have, dsub_have = _pq._codebook(codebook)
            if (m_have, dsub_have) != (m, dsub):
                raise ValueError("the codebook is [%d, %d, %d] and m = %d, D = %d need [%d, %d, %d]" % (
                    m_have, _pq.CODEWORDS, dsub_have, m, rows.shape[1], m, _pq.CODEWORDS, dsub))
        elif rows.shape[0] < _pq.CODEWORDS:
            raise ValueError("N = %d rows: pq.train needs at least %d" % (rows.shape[0], _pq.CODEWORDS))
        labels, _ = self._build(rows, centroids, labels, chunk)         # every other check, the lists, the capacities, the coarse index
        self.m, self.device = m, rows.device
        try:
            step = min(self.n, chunk or _pq.CHUNK)
            if codebook is None:
                residuals = torch.empty((self.n, self.d), dtype=torch.float32, device=self.device)
                for p0 in range(0, self.n, step):
                    residuals[p0:p0 + step] = self._residuals(rows, centroids, labels, p0, p0 + step)
                codebook = _pq.train(residuals, m, chunk=chunk, **pq_train_kwargs)
                self.codes = _pq.encode(codebook, residuals, chunk)
                del residuals
            else:
                if words.device != self.device:
                    raise ValueError("the codebook is on %s and rows on %s" % (words.device, self.device))
                self.codes = torch.empty((self.n, m), dtype=torch.uint8, device=self.device)
                for p0 in range(0, self.n, step):
                    self.codes[p0:p0 + step] = _pq.encode(codebook, self._residuals(rows, centroids, labels, p0, p0 + step))
            if refine is not None:
                self.refine = refine
                self.refine_codes, self.refine_scales = ops.lists_i8_encode(rows, self.order)
                self.where = self._where()
        except BaseException:
            self.close()
            raise
        self.codebook = codebook if isinstance(codebook, _pq.Codebook) else _pq.Codebook(codebook, [], 0)
        self.rows = rows if keep_rows else None

    def _residuals(self, rows, centroids, labels, p0, p1, order=None):
        """fp32 [p1 - p0, D]: row - centroids[label] of the rows at positions p0 .. p1 of the list order (``order``: of a batch's)."""
        ids = (self.order if order is None else order)[p0:p1]
        return rows.index_select(0, ids) - centroids.index_select(0, labels.index_select(0, ids))

    def _where(self):
        """int64 [n]: the position of every live id in the list order, -1 at ids that are not live -- the inverse of ``order``."""
        where = torch.full((self.n,), -1, dtype=torch.int64, device=self.device)
        where.index_copy_(0, self.order, torch.arange(self.size, dtype=torch.int64, device=self.device))
        return where

    @classmethod
    def train(cls, rows, lists, m=64, kmeans=None, pq=None, keep_rows=True, refine=None):
        """The index of ``cluster.kmeans(rows, lists, **kmeans)`` with ``pq.train(residuals, m, **pq)``; the fit stays reachable as
        ``.fit``."""
        ivf._rows_matrix(rows, "rows")
        _pq._subspaces(m, rows.shape[1])
        _check_refine(refine, rows.shape[1])
        fit = cluster.kmeans(rows, lists, **(kmeans or {}))
        index = cls(rows, fit.centroids, fit.labels, m=m, keep_rows=keep_rows, refine=refine, **(pq or {}))
        index.fit = fit
        return index

    def nbytes(self):
        """The bytes the index holds on the device: codes, order, offsets, codebook, coarse index, the refinement codes, scales and
        ``where`` of a ``refine="i8"`` index, and the rows if they are kept.  The centroids are the caller's tensor and are mirrored by
        ``coarse``: they are not counted a second time."""
        held = self.codes.numel() + 8 * self.order.numel() + 8 * self.offsets.numel() + 4 * self.codebook.codewords.numel()
        held += self.coarse.device_bytes if self.coarse is not None else 0
        if self.refine is not None:
            held += self.refine_codes.numel() + 4 * self.refine_scales.numel() + 8 * self.where.numel()
        if self.rows is not None:
            held += 4 * self.rows.shape[0] * (self.rows.stride(0) if self.rows.shape[0] > 1 else self.rows.shape[1])
        return held

    def query_chunk(self, nprobe, shortlist=None):
        """Queries per step of ``search``: as many as keep their candidate rows (12 bytes a column), their tables (``m`` KiB each) and,
        with a shortlist of ``S``, the selection and the rescored pairs (``28 S``) under ``ivf.CANDIDATE_MEMORY_CAP`` (at least one).  On a
        ``refine="i8"`` index a shortlisted query also holds its centred row, codes and scale (``5 d + 4`` bytes) and the refined pairs
        with their unsorted scores (``16 S``)."""
        per_query = 12 * self.capacity(nprobe) + 4 * _pq.CODEWORDS * self.m + (0 if shortlist is None else 28 * shortlist)
        if self.refine is not None and shortlist is not None:
            per_query += 5 * self.d + 4 + 16 * shortlist
        return max(1, ivf.CANDIDATE_MEMORY_CAP // per_query)

    def _check_search(self, queries, k, nprobe, qlayout, center, shortlist, rescore=None):
        if self.coarse is None:
            raise ValueError("the index is closed")
        cluster._count(k, "k")
        if k > ops.RESCORE_MAX_K:
            raise ValueError("k = %d > %d" % (k, ops.RESCORE_MAX_K))
        if rescore is not None and self.refine is None:
            raise ValueError("rescore = %r needs an index built with refine=\"i8\"" % (rescore,))
        if shortlist is not None:
            cluster._count(shortlist, "shortlist")
            if not k <= shortlist <= ops.RESCORE_MAX_K:
                raise ValueError("shortlist = %d must be in [k = %d, %d]" % (shortlist, k, ops.RESCORE_MAX_K))
            if rescore is not None:
                cluster._count(rescore, "rescore")
                if not k <= rescore <= shortlist:
                    raise ValueError("rescore = %d must be in [k = %d, shortlist = %d]" % (rescore, k, shortlist))
            if self.rows is None and (self.refine is None or rescore is not None):
                raise ValueError("%s is rescored on the fp32 rows; this index was built with keep_rows=False" % (
                    "a shortlist" if self.refine is None else "rescore = %d of the refined shortlist" % rescore))
        elif rescore is not None:
            raise ValueError("rescore = %r needs a shortlist" % (rescore,))
        super()._check_search(queries, k, nprobe, qlayout, center)

    def search(self, queries, k, nprobe, qlayout="ND", center=None, shortlist=None, rescore=None):
        """:data:`IVFPQResult` of the ``k`` best rows of every query among the members of its ``nprobe`` best lists, by ADC score or,
        with a shortlist, by the exact score of the ADC shortlist -- on a ``refine="i8"`` index by its int8 score, and with ``rescore=R``
        by the exact score of the ``R`` best of those -- the module docstring has the contract."""
        self._check_search(queries, k, nprobe, qlayout, center, shortlist, rescore)
        return self._chunked(self._search, IVFPQResult, self.query_chunk(nprobe, shortlist), queries, qlayout, k, nprobe, center, shortlist,
                             rescore)

    def _search(self, queries, qlayout, k, nprobe, center, shortlist, rescore=None):
        center = None if center is None else center.reshape(-1)
        probes, coarse, plan, cap = self._probe(queries, qlayout, center, nprobe)     # the plan counts positions; self.n is the id bound
        lut = ops.pq_lut(self.codebook.codewords, queries, qlayout, center)
        cand_scores, cand_ids = ops.lists_pq_scan(self.codes, self.order, self.n, self.offsets, lut, coarse, probes, plan, cap)
        ids, scores, scanned = self._select(cand_scores, cand_ids, plan, nprobe, k if shortlist is None else shortlist)
        if shortlist is None:
            return IVFPQResult(ids, scores, probes, scanned)
        del cand_scores, cand_ids, lut
        ids = self._pad_in(ids)
        if self.refine is not None:
            qcodes, qscales = ops.quantize_i8(ops.center_rows(queries, qlayout, center))
            ids, fine = ops.refine_i8(self.refine_codes, self.refine_scales, self.d, self.where, qcodes, qscales, ids)
            if rescore is None:
                ids = self._pad_out(ids)
                return IVFPQResult(ids[:, :k].contiguous(), fine[:, :k].contiguous(), probes, scanned)
            ids = ids[:, :rescore].contiguous()
        sure_ids, sure = ops.rescore(self.rows, queries, ids, qlayout, center)
        sure_ids = self._pad_out(sure_ids)
        return IVFPQResult(sure_ids[:, :k].contiguous(), sure[:, :k].contiguous(), probes, scanned)

    # -------------------------------------------------------------------------------------------- after the build

    def _check_edit(self, what):
        if self.coarse is None:
            raise ValueError("the index is closed")
        if self.rows is not None:
            raise ValueError("%s on an index that keeps the fp32 rows: the index never copies or grows the caller's tensor -- "
                             "attach_rows(None) first" % what)

    def add(self, batch, labels=None, chunk=None):
        """Encodes ``batch`` (fp32 ``[B, D]``) and merges it into the lists; the ids int64 ``[B]`` it got, ``n .. n + B - 1`` -- the module
        docstring has the contract."""
        self._check_edit("add")
        ivf._rows_matrix(batch, "batch")
        b = batch.shape[0]
        if batch.shape[1] != self.d:
            raise ValueError("batch is [B, %d] and the index has D = %d" % (batch.shape[1], self.d))
        ivf._labels_fit(labels, batch, "batch")
        if chunk is not None:
            cluster._count(chunk, "chunk")
        if self.n + b >= 1 << 31:
            raise ValueError("n + B = %d + %d ids: the id bound must stay below 2^31" % (self.n, b))
        cluster._on_device(batch, "batch")
        if batch.device != self.device:
            raise ValueError("batch is on %s and the index on %s" % (batch.device, self.device))
        if labels is not None:
            ivf._labels_in_range(labels, self.lists, self.device, self._home)
        else:
            labels = cluster.assign(self.centroids, batch, chunk)[0]
        members, offsets, _ = cluster._members(labels, self.lists)
        step = min(b, chunk or _pq.CHUNK)
        codes = torch.empty((b, self.m), dtype=torch.uint8, device=self.device)
        for p0 in range(0, b, step):
            codes[p0:p0 + step] = _pq.encode(self.codebook, self._residuals(batch, self.centroids, labels, p0, p0 + step, members))
        merged = ops.lists_merge(self.codes, self.order, self.offsets, codes, members + self.n, offsets)
        if self.refine is not None:                                               # the same merge of the two other payloads, as bytes
            fine_codes, fine_scales = ops.lists_i8_encode(batch, members)
            fine = [ops.lists_merge(mine.view(torch.uint8).view(self.size, -1), self.order, self.offsets,
                                    new.view(torch.uint8).view(b, -1), members + self.n, offsets)[0]
                    for mine, new in ((self.refine_codes, fine_codes), (self.refine_scales, fine_scales))]
        host_sizes = (merged[2][1:] - merged[2][:-1]).cpu().tolist()             # the one read-back
        ids = torch.arange(self.n, self.n + b, dtype=torch.int64, device=self.device)
        self.codes, self.order, self.offsets = merged
        self._set_sizes(host_sizes)
        self.n, self.size = self.n + b, self.size + b
        if self.refine is not None:
            self.refine_codes, self.refine_scales = fine[0].view(torch.int8), fine[1].view(torch.float32).view(self.size)
            self.where = self._where()
        return ids

    def remove(self, ids):
        """Drops the live rows among ``ids`` (int64 on the device; any order, duplicates and ids that are not live are ignored) from the
        lists; the number of rows removed -- the module docstring has the contract."""
        self._check_edit("remove")
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 1:
            raise ValueError("ids must be an int64 1-d tensor, got %s" % (
                "%s %s" % (ids.dtype, tuple(ids.shape)) if isinstance(ids, torch.Tensor) else type(ids).__name__))
        cluster._on_device(ids, "ids")
        if ids.device != self.device:
            raise ValueError("ids are on %s and the index on %s" % (ids.device, self.device))
        dead = torch.zeros(self.n + 1, dtype=torch.bool, device=self.device)       # entry n takes the ids that are out of range
        dead.index_fill_(0, torch.where((ids >= 0) & (ids < self.n), ids, self.n), True)
        kept = torch.zeros(self.size + 1, dtype=torch.int64, device=self.device)
        kept[1:] = torch.cumsum(~dead.index_select(0, self.order), 0)
        ends = kept.index_select(0, self.offsets)
        *host_sizes, total = torch.cat([ends[1:] - ends[:-1], kept[-1:]]).cpu().tolist()        # the one read-back
        if total < 1:
            raise ValueError("removing these ids would leave no row in the index")
        removed = self.size - total
        if removed:
            if self.refine is not None:
                fine = [ops.lists_compact(mine.view(torch.uint8).view(self.size, -1), self.order, self.offsets, kept, total)[0]
                        for mine in (self.refine_codes, self.refine_scales)]
            self.codes, self.order, self.offsets = ops.lists_compact(self.codes, self.order, self.offsets, kept, total)
            self._set_sizes(host_sizes)
            self.size = total
            if self.refine is not None:
                self.refine_codes, self.refine_scales = fine[0].view(torch.int8), fine[1].view(torch.float32).view(total)
                self.where = self._where()
        return removed

    def attach_rows(self, rows):
        """``rows`` (fp32 ``[n, D]`` on the index's device, rows contiguous) becomes ``index.rows``, for ``shortlist=``; ``None`` drops the
        reference."""
        if rows is not None:
            ivf._rows_matrix(rows, "rows")
            if tuple(rows.shape) != (self.n, self.d):
                raise ValueError("rows are %s and the ids of the index need [n = %d, D = %d]" % (tuple(rows.shape), self.n, self.d))
            cluster._on_device(rows, "rows")
            if rows.device != self.device:
                raise ValueError("rows are on %s and the index on %s" % (rows.device, self.device))
        self.rows = rows

    def state(self):
        """The index as plain tensors and numbers: ``centroids``, ``codewords``, ``codes``, ``order``, ``offsets`` (its own tensors, not
        copies), ``n`` and ``m`` -- and ``refine_codes`` and ``refine_scales`` of a ``refine="i8"`` index -- what :meth:`from_state`
        takes."""
        state = {"centroids": self.centroids, "codewords": self.codebook.codewords, "codes": self.codes, "order": self.order,
                 "offsets": self.offsets, "n": self.n, "m": self.m}
        if self.refine is not None:
            state.update(refine_codes=self.refine_codes, refine_scales=self.refine_scales)
        return state

    @classmethod
    def from_state(cls, state, device=None, rows=None):
        """The index of ``index.state()``, its tensors moved to ``device`` (``None``: where the codes are); ``rows`` as for
        :meth:`attach_rows`."""
        names = ("centroids", "codewords", "codes", "order", "offsets", "n", "m")
        if not isinstance(state, dict) or any(name not in state for name in names):
            raise ValueError("state must be a dict of %s" % ", ".join(names))
        kinds = {"centroids": (torch.float32, 2), "codewords": (torch.float32, 3), "codes": (torch.uint8, 2), "order": (torch.int64, 1),
                 "offsets": (torch.int64, 1)}
        for name, (dtype, dims) in kinds.items():
            t = state[name]
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dims or t.numel() < 1:
                raise ValueError("state[%r] must be a non-empty %d-d %s tensor" % (name, dims, dtype))
        device = torch.device(state["codes"].device if device is None else device)
        centroids, codewords, codes, order, offsets = (state[name].to(device).contiguous() for name in kinds)
        n, m = state["n"], state["m"]
        cluster._count(n, "n")
        dsub = _pq._subspaces(m, centroids.shape[1])
        _pq._codebook(codewords)
        size, lists = codes.shape[0], centroids.shape[0]
        if tuple(codewords.shape) != (m, _pq.CODEWORDS, dsub) or codes.shape[1] != m or tuple(order.shape) != (size,) \
                or tuple(offsets.shape) != (lists + 1,) or size > n:
            raise ValueError("the state does not fit together: centroids %s, codewords %s, codes %s, order %s, offsets %s, n = %d, m = %d" % (
                tuple(centroids.shape), tuple(codewords.shape), tuple(codes.shape), tuple(order.shape), tuple(offsets.shape), n, m))
        fine = [state.get(name) for name in ("refine_codes", "refine_scales")]
        if any(t is not None for t in fine):
            d_pad = (centroids.shape[1] + 63) // 64 * 64
            for t, name, dtype, shape in zip(fine, ("refine_codes", "refine_scales"), (torch.int8, torch.float32), ((size, d_pad), (size,))):
                if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                    raise ValueError("state[%r] must be a %s tensor of shape %s beside codes %s and centroids %s" % (
                        name, dtype, list(shape), tuple(codes.shape), tuple(centroids.shape)))
            _check_refine("i8", centroids.shape[1])
        cluster._on_device(codes, "the state")
        index = cls.__new__(cls)
        if fine[0] is not None:
            index.refine, index.refine_codes, index.refine_scales = "i8", fine[0].to(device).contiguous(), fine[1].to(device).contiguous()
        index.n, index.size, index.d, index.lists, index.m = n, size, centroids.shape[1], lists, m
        index.device, index.centroids, index.fit, index.rows = device, centroids, None, None
        index.codes, index.order, index.offsets = codes, order, offsets
        if index.refine is not None:
            index.where = index._where()
        index.codebook = _pq.Codebook(codewords, [], 0)
        index._set_sizes((offsets[1:] - offsets[:-1]).cpu().tolist())              # the one read-back
        index.coarse = None
        index.attach_rows(rows)
        index.coarse = ops.DescriptorIndex(centroids, "ND")
        return index
