"""Spherical k-means on the device: partition a database of L2-normalised descriptors by cosine similarity.

``assign(centroids, rows)`` labels every row with its best centroid; ``kmeans(rows, k)`` runs Lloyd's iteration and returns a
:data:`KMeans`.  Every result is defined to the bit: two runs on the same data return the same centroids and the same labels, whatever
the schedule of the device (there are no floating-point atomics anywhere), and ``tests/kmeans_restatement.py`` states the whole loop in
numpy.  The uses are a vocabulary or a coarse partition, an even sample of a database, and the ``clusters`` that
``mining.search_hard_negatives`` asks for when a training set has no SfM models.

``assign(centroids, rows, chunk=None, compute="chain")`` -> ``(labels int64 [N], best fp32 [N])``.
    An fp32 ``DescriptorIndex`` of the centroids scores ``chunk`` rows at a time into ONE reused ``[chunk, K]`` block
    (``mdx_scores_ex``), and ``ops.kmeans_argmax`` reads each block once (``mdx_kmeans_argmax``): the larger score wins, equal scores
    go to the smaller centroid id, ``-0 == +0``, NaN last.  The default chunk keeps the block and the similarity's workspace under
    ``ASSIGN_MEMORY_CAP`` bytes (:func:`assign_chunk`).  With ``compute="chain"`` the labels and ``best`` are the bits of
    ``ops.topk(index.scores(rows), 1)``, whatever the chunk.  ``compute`` is handed to ``scores``: ``"split3"`` and ``"split2"`` are
    its labelled faster modes, whose scores lie within their stated bound of the chain's, so a row whose two best centroids are
    closer than that may take the other label.

``kmeans(rows, k, iters=20, init="sample", seed=0, train_rows=None, tol=0.0, chunk=None, compute="chain")`` -> :data:`KMeans`.
    ``rows`` fp32 ``[N, D]`` on the device, contiguous.  One CPU generator, ``torch.Generator().manual_seed(seed)``, makes every
    random choice, in this order: the training sample, then the initial centroids.
    ``train_rows=M`` fits on a sample of M rows: the first M entries of ``torch.randperm(N)`` of that generator, sorted ascending.
    Without it the training rows are all rows.  ``k > N`` or ``k > train_rows`` is a ValueError.
    ``init``: ``"sample"`` -- k distinct training rows, the first k entries of ``torch.randperm(number of training rows)`` of the
    generator, in the order drawn; a sequence of k ids of ``rows`` (of ALL rows, also with ``train_rows``); or a ``[K, D]`` fp32
    device tensor, taken as it is (a copy).  The rows are expected to be L2-normalised and are not renormalised.
    Each iteration:
      1. ``assign`` the training rows to the current centroids.
      2. Append the float64 sum of ``best`` to ``history`` (the objective; it is a torch reduction, reproducible but not part of the
         bit contract).
      3. Stop when the share of training rows whose label differs from the previous iteration's is ``<= tol`` (before the first
         update every row counts as changed; the default 0 means: no label changed), or when ``iters`` updates have been made.
      4. Members and offsets: a stable sort of the labels, so the members of a cluster ascend (as ``search._group_csr``).
      5. ``ops.kmeans_sums`` -- the segment chain of include/mdx_kmeans.h, ``ops.KMEANS_SEGMENT`` members per segment -- then
         ``ops.kmeans_finish`` with the previous centroids: ``c = s / (||s|| + eps)``, ``eps = 1e-6``; a cluster whose sum is all
         zero keeps its previous centroid.
      6. Reseed.  Let E be the number of clusters the assignment left empty.  Taken in ascending cluster id, they become the E
         training rows with the smallest ``best`` -- the worst-represented rows -- in the order of ``ops.topk(-best, E)`` (smallest
         first, equal values by ascending row id).  Each such row goes through the same ``kmeans_finish``.  The rows keep their
         labels for this update: the cluster they came from is summed with them.  ``reseeded`` counts the reseeds of the whole run.
    ``labels``, ``sizes`` and the ``best`` behind them come from a final ``assign`` of ALL rows to the returned centroids (without
    ``train_rows``, when the loop stopped on an assignment to those very centroids, that assignment is the final one).
"""
from collections import namedtuple

import torch

from . import _lib, ops

KMeans = namedtuple("KMeans", ["centroids", "labels", "sizes", "history", "iterations", "reseeded"])
KMeans.__doc__ = """centroids fp32 [K, D]; labels int64 [N]: every row's centroid; sizes int64 [K]: rows per centroid; history: the
float64 sum of every row's best score, one entry per assignment of the loop; iterations: the centroid updates made; reseeded: the
empty clusters that were given a row, over the whole run."""

ASSIGN_MEMORY_CAP = 1 << 30     # bytes of [chunk, K] scores + similarity workspace one step of assign may hold
FINISH_EPS = 1e-6               # the eps of the L2N rule, as everywhere in this library


def _count(x, what, lo=1):
    if isinstance(x, bool) or not isinstance(x, int) or x < lo:
        raise ValueError("%s must be an integer >= %d, got %r" % (what, lo, x))


def _matrix(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be a non-empty fp32 [rows, D] tensor, got %s" % (
            what, "%s %s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)


def _on_device(t, what):
    if not t.is_cuda:
        raise ValueError("%s must be a CUDA/ROCm tensor: the MI355X path has no CPU fallback" % what)


def _compute(compute):
    if compute not in _lib.COMPUTE:
        raise ValueError("compute %r (one of %s)" % (compute, sorted(_lib.COMPUTE)))
    return _lib.COMPUTE[compute]


def _assign_bytes(chunk, k, d, mode):
    return chunk * k * 4 + _lib.lib().mdx_scores_workspace_ex(chunk, d, mode)


def assign_chunk(n, k, d, compute="chain", cap=ASSIGN_MEMORY_CAP):
    """Rows per step of :func:`assign`: as many as keep the ``[chunk, K]`` score block and the similarity's workspace under ``cap``
    bytes (at least one), as ``search.knn_chunk``; by bisection, because the workspace grows in steps of a query tile."""
    mode = _compute(compute)
    lo, hi = 1, n                                           # bytes(lo) <= cap or lo == 1; the answer lies in [lo, hi]
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _assign_bytes(mid, k, d, mode) <= cap:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _check_assign(centroids, rows, chunk, compute):
    _matrix(centroids, "centroids")
    _matrix(rows, "rows")
    if centroids.shape[1] != rows.shape[1]:
        raise ValueError("centroids are [K, %d] and rows [N, %d]: the dimensions differ" % (centroids.shape[1], rows.shape[1]))
    if chunk is not None:
        _count(chunk, "chunk")
    _compute(compute)
    _on_device(centroids, "centroids")
    _on_device(rows, "rows")
    if centroids.device != rows.device:
        raise ValueError("centroids are on %s and rows on %s" % (centroids.device, rows.device))


def assign(centroids, rows, chunk=None, compute="chain"):
    """``(labels int64 [N], best fp32 [N])``: the best centroid (fp32 ``[K, D]``) of every row (fp32 ``[N, D]``, both on the device and
    contiguous) and its score -- the module docstring has the contract."""
    _check_assign(centroids, rows, chunk, compute)
    n, d = rows.shape
    k = centroids.shape[0]
    chunk = min(n, chunk or assign_chunk(n, k, d, compute))
    labels = torch.empty((n,), dtype=torch.int64, device=rows.device)
    best = torch.empty((n,), dtype=torch.float32, device=rows.device)
    block = torch.empty((chunk, k), dtype=torch.float32, device=rows.device)
    index = ops.DescriptorIndex(centroids, "ND")
    try:
        for i0 in range(0, n, chunk):
            i1 = min(n, i0 + chunk)
            scores = index.scores(rows[i0:i1], "ND", out=block[:i1 - i0], compute=compute)
            ops.kmeans_argmax(scores, out_labels=labels[i0:i1], out_best=best[i0:i1])
    finally:
        index.close()
    return labels, best


def _members(labels, k):
    """(members int64 [n], offsets int64 [k + 1], sizes int64 [k]) of the labels: a stable sort keeps a cluster's members ascending."""
    _, members = torch.sort(labels, stable=True)
    sizes = torch.bincount(labels, minlength=k)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(sizes, 0)
    return members, offsets, sizes


def _initial(rows, train, k, init, gen):
    """The first centroids, fp32 [k, D] on the device (a tensor of its own)."""
    if isinstance(init, str):
        if init != "sample":
            raise ValueError("init %r: \"sample\", a sequence of k row ids or a [K, D] tensor" % (init,))
        ids = torch.randperm(train.shape[0], generator=gen)[:k]
        return train.index_select(0, ids.to(rows.device))
    if isinstance(init, torch.Tensor) and init.dim() == 2:
        _matrix(init, "init")
        if tuple(init.shape) != (k, rows.shape[1]) or init.device != rows.device:
            raise ValueError("init must be [%d,%d] on %s, got %s on %s" % (k, rows.shape[1], rows.device, tuple(init.shape), init.device))
        return init.clone()
    try:
        ids = [int(i) for i in (init.tolist() if isinstance(init, torch.Tensor) else init)]
    except (TypeError, ValueError):
        raise ValueError("init %r: \"sample\", a sequence of k row ids or a [K, D] tensor" % (init,)) from None
    if len(ids) != k or any(i < 0 or i >= rows.shape[0] for i in ids):
        raise ValueError("init: %d ids for k = %d clusters, each in [0, %d)" % (len(ids), k, rows.shape[0]))
    return rows.index_select(0, torch.tensor(ids, dtype=torch.int64).to(rows.device))


def kmeans(rows, k, iters=20, init="sample", seed=0, train_rows=None, tol=0.0, chunk=None, compute="chain"):
    """Spherical k-means of ``rows`` (fp32 ``[N, D]`` on the device, contiguous, L2-normalised) into ``k`` clusters, as a
    :data:`KMeans` -- the module docstring states every rule."""
    _matrix(rows, "rows")
    n, d = rows.shape
    _count(k, "k")
    _count(iters, "iters", 0)
    _count(seed, "seed", 0)
    if chunk is not None:
        _count(chunk, "chunk")
    if train_rows is not None:
        _count(train_rows, "train_rows")
        if train_rows > n:
            raise ValueError("train_rows = %d > N = %d rows" % (train_rows, n))
    if k > (n if train_rows is None else train_rows):
        raise ValueError("k = %d > %s" % (k, "N = %d rows" % n if train_rows is None else "train_rows = %d" % train_rows))
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0 <= tol <= 1:
        raise ValueError("tol must be a share in [0, 1], got %r" % (tol,))
    _compute(compute)
    if isinstance(init, str) and init != "sample":
        raise ValueError("init %r: \"sample\", a sequence of k row ids or a [K, D] tensor" % (init,))
    _on_device(rows, "rows")

    gen = torch.Generator().manual_seed(seed)
    train = rows
    if train_rows is not None and train_rows < n:
        train = rows.index_select(0, torch.sort(torch.randperm(n, generator=gen)[:train_rows]).values.to(rows.device))
    elif train_rows is not None:
        torch.randperm(n, generator=gen)                    # the generator moves on as for any other M
    centroids = _initial(rows, train, k, init, gen)
    m = train.shape[0]
    history, updates, reseeded = [], 0, 0
    previous = None
    while True:
        labels, best = assign(centroids, train, chunk, compute)
        history.append(float(best.double().sum()))
        changed = m if previous is None else int((labels != previous).sum())
        if changed <= tol * m or updates == iters:
            break
        members, offsets, sizes = _members(labels, k)
        sums = ops.kmeans_sums(train, members, offsets, k)
        centroids = ops.kmeans_finish(sums, FINISH_EPS, previous=centroids)
        empty = torch.nonzero(sizes == 0).reshape(-1)
        if empty.numel():
            worst, _ = ops.topk(torch.neg(best).reshape(1, m), int(empty.numel()))
            centroids[empty] = ops.kmeans_finish(train.index_select(0, worst.reshape(-1)), FINISH_EPS)
            reseeded += int(empty.numel())
        previous = labels
        updates += 1
    if train is not rows:
        labels, best = assign(centroids, rows, chunk, compute)
    sizes = torch.bincount(labels, minlength=k)
    return KMeans(centroids, labels, sizes, history, updates, reseeded)
