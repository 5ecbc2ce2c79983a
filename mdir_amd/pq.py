"""A product quantiser on the device: M sub-vectors per vector, one byte each.

A vector of ``D = M * dsub`` elements is cut into ``M`` sub-vectors of ``dsub``; subspace ``m`` has 256 codewords, and the code of a
vector is, per subspace, the id of the nearest one: ``M`` bytes for ``4 D``.  ``mdir_amd/ivfpq.py`` stores the residuals of an inverted
file this way and scans them by table look-ups (include/mdx_lists_pq.h).  Nothing here is a kernel of its own: the host composes the
exact similarity (``ops.DescriptorIndex``), ``ops.kmeans_argmax`` and ``ops.kmeans_sums``, and every result is defined to the bit, as
in ``cluster.py``; ``tests/pq_restatement.py`` states ``train``, ``encode`` and ``decode`` in numpy.

:data:`Codebook` ``(codewords, history, iterations)``: ``codewords`` fp32 ``[M, 256, dsub]`` on the device, contiguous;
``1 <= M <= ops.PQ_MAX_M``.

The code of a vector ``v``.  For subspace ``m`` it is the first argmax over ``j`` of ``fl(chain(v_m, c_mj) + b_mj)`` with
``kmeans_argmax``'s tie rule (the smaller id wins, ``-0 == +0``, NaN loses).  ``chain`` is the library's exact fp32 chain, the bits of
``ops.DescriptorIndex(codewords[m], "ND").scores(v_m)``; ``b_mj = -0.5 * chain(c_mj, c_mj)`` is the diagonal of the same index scoring
its own codewords, times -0.5 (exact); the sum is one fp32 addition on the score block (``block.add_(bias)``).  This is the
nearest codeword in the Euclidean sense, ``argmin ||v_m - c||^2 = argmax <v_m, c> - ||c||^2 / 2``, stated through the inner product.

``encode(codebook, vectors, chunk=None)`` -> uint8 ``[T, M]``.
    ``vectors`` fp32 ``[T, D]`` on the device, contiguous.  ``chunk`` rows at a time (default :data:`CHUNK`), one subspace at a time,
    into ONE reused ``[chunk, 256]`` block.  The chunk changes no bit of the result.

``decode(codebook, codes)`` -> fp32 ``[T, D]``: the codewords of the codes side by side, a gather.

``train(vectors, m, iters=10, seed=0, train_rows=None, chunk=None)`` -> :data:`Codebook`.
    ``vectors`` fp32 ``[T, D]`` on the device, contiguous, ``T >= 256``, ``D % m == 0``.  One CPU generator,
    ``torch.Generator().manual_seed(seed)``, makes every random choice, in this order, as ``cluster.kmeans`` does:
    the training sample -- with ``train_rows`` (``>= 256``) the first ``train_rows`` entries of ``torch.randperm(T)``, sorted ascending;
    without it all rows, and nothing is drawn --, then the initial codewords: the first 256 entries of ``torch.randperm(number of
    training rows)``, in the order drawn; subspace ``m`` takes sub-vector ``m`` of those same 256 rows.
    Each iteration, for every subspace:
      1. Assign the training rows as in ``encode``.
      2. Append the float64 sum of the winning values to ``history`` (subspace 0 first; a torch reduction, not part of the bit
         contract).
      3. Stop when ``iters`` updates have been made, or when no label changed in any subspace (before the first update every label
         counts as changed).
      4. Members and offsets by a stable sort (``cluster._members``).
      5. ``ops.kmeans_sums`` on the sub-vector view of the training rows (leading dimension ``D``): the segment chain of
         include/mdx_kmeans.h, unchanged.
      6. ``codeword = sum / float(count)``, one fp32 division per element; a codeword without members keeps its previous value.
    Two runs give equal bits.
"""
from collections import namedtuple

import torch

from . import cluster, ops

Codebook = namedtuple("Codebook", ["codewords", "history", "iterations"])
Codebook.__doc__ = """codewords fp32 [M, 256, dsub]; history: the float64 sum of the winning values, one entry per assignment and
subspace; iterations: the codeword updates made."""

CODEWORDS = ops.PQ_CODEWORDS      # a code is one byte
CHUNK = 1 << 16                   # rows per step of an assignment: a 64 MiB score block


def _subspaces(m, d):
    cluster._count(m, "m")
    if m > ops.PQ_MAX_M:
        raise ValueError("m = %d sub-quantisers: m must be in [1, %d]" % (m, ops.PQ_MAX_M))
    if d % m:
        raise ValueError("D = %d is not a multiple of m = %d" % (d, m))
    return d // m


def _codebook(codebook):
    """(M, dsub) of a :data:`Codebook` (or of its codewords alone), checked."""
    words = codebook.codewords if isinstance(codebook, Codebook) else codebook
    if not isinstance(words, torch.Tensor) or words.dtype != torch.float32 or words.dim() != 3 or words.shape[1] != CODEWORDS \
            or not 1 <= words.shape[0] <= ops.PQ_MAX_M or words.shape[2] < 1 or not words.is_contiguous():
        raise ValueError("codewords must be a contiguous fp32 [M, %d, dsub] tensor with M in [1, %d], got %s" % (
            CODEWORDS, ops.PQ_MAX_M, "%s %s" % (words.dtype, tuple(words.shape)) if isinstance(words, torch.Tensor) else type(words).__name__))
    return words, words.shape[0], words.shape[2]


def _sweep(words, vectors, chunk, sink):
    """Assigns ``vectors`` to ``words`` ``chunk`` rows at a time, one subspace at a time: ``sink(m, i0, i1, labels, best)`` gets the
    labels int64 and the winning values fp32 of rows ``i0 .. i1`` in subspace ``m`` (buffers that are reused: copy out of them)."""
    t = vectors.shape[0]
    m_sub, dsub = words.shape[0], words.shape[2]
    chunk = min(t, chunk or CHUNK)
    block = torch.empty((chunk, CODEWORDS), dtype=torch.float32, device=vectors.device)
    piece = torch.empty((chunk, dsub), dtype=torch.float32, device=vectors.device)
    labels = torch.empty((chunk,), dtype=torch.int64, device=vectors.device)
    best = torch.empty((chunk,), dtype=torch.float32, device=vectors.device)
    indexes = []
    try:
        biases = []
        for m in range(m_sub):
            indexes.append(ops.DescriptorIndex(words[m], "ND"))
            # b_j = -0.5 * chain(c_j, c_j): the diagonal of the index scoring its own codewords
            biases.append(torch.diagonal(indexes[m].scores(words[m], "ND")).mul(-0.5))
        for i0 in range(0, t, chunk):
            i1 = min(t, i0 + chunk)
            for m in range(m_sub):
                piece[:i1 - i0].copy_(vectors[i0:i1, m * dsub:(m + 1) * dsub])
                scores = indexes[m].scores(piece[:i1 - i0], "ND", out=block[:i1 - i0])
                scores.add_(biases[m])
                ops.kmeans_argmax(scores, out_labels=labels[:i1 - i0], out_best=best[:i1 - i0])
                sink(m, i0, i1, labels[:i1 - i0], best[:i1 - i0])
    finally:
        for index in indexes:
            index.close()


def encode(codebook, vectors, chunk=None):
    """uint8 ``[T, M]``: the code of every row of ``vectors`` (fp32 ``[T, D]`` on the device, contiguous) -- the module docstring
    states the rule."""
    words, m_sub, dsub = _codebook(codebook)
    cluster._matrix(vectors, "vectors")
    if vectors.shape[1] != m_sub * dsub:
        raise ValueError("vectors are [T, %d] and the codebook covers M * dsub = %d * %d elements" % (vectors.shape[1], m_sub, dsub))
    if chunk is not None:
        cluster._count(chunk, "chunk")
    cluster._on_device(vectors, "vectors")
    cluster._on_device(words, "codewords")
    if words.device != vectors.device:
        raise ValueError("codewords are on %s and vectors on %s" % (words.device, vectors.device))
    codes = torch.empty((vectors.shape[0], m_sub), dtype=torch.uint8, device=vectors.device)

    def sink(m, i0, i1, labels, best):
        codes[i0:i1, m] = labels.to(torch.uint8)
    _sweep(words, vectors, chunk, sink)
    return codes


def decode(codebook, codes):
    """fp32 ``[T, D]``: per row the codewords its code names, subspace 0 first."""
    words, m_sub, dsub = _codebook(codebook)
    if not isinstance(codes, torch.Tensor) or codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] != m_sub:
        raise ValueError("codes must be a uint8 [T, %d] tensor, got %s" % (
            m_sub, "%s %s" % (codes.dtype, tuple(codes.shape)) if isinstance(codes, torch.Tensor) else type(codes).__name__))
    if codes.device != words.device:
        raise ValueError("codes are on %s and codewords on %s" % (codes.device, words.device))
    out = torch.empty((codes.shape[0], m_sub * dsub), dtype=torch.float32, device=words.device)
    for m in range(m_sub):
        out[:, m * dsub:(m + 1) * dsub] = words[m].index_select(0, codes[:, m].to(torch.int64))
    return out


def train(vectors, m, iters=10, seed=0, train_rows=None, chunk=None):
    """The :data:`Codebook` of ``m`` sub-quantisers fitted to ``vectors`` (fp32 ``[T, D]`` on the device, contiguous) by Lloyd's
    iteration in every subspace -- the module docstring states every rule."""
    cluster._matrix(vectors, "vectors")
    t, d = vectors.shape
    dsub = _subspaces(m, d)
    cluster._count(iters, "iters", 0)
    cluster._count(seed, "seed", 0)
    if chunk is not None:
        cluster._count(chunk, "chunk")
    if t < CODEWORDS:
        raise ValueError("T = %d vectors: at least %d are needed, one per codeword" % (t, CODEWORDS))
    if train_rows is not None:
        cluster._count(train_rows, "train_rows")
        if not CODEWORDS <= train_rows <= t:
            raise ValueError("train_rows = %d must be in [%d, T = %d]" % (train_rows, CODEWORDS, t))
    cluster._on_device(vectors, "vectors")

    gen = torch.Generator().manual_seed(seed)
    sample = vectors
    if train_rows is not None and train_rows < t:
        sample = vectors.index_select(0, torch.sort(torch.randperm(t, generator=gen)[:train_rows]).values.to(vectors.device))
    elif train_rows is not None:
        torch.randperm(t, generator=gen)                    # the generator moves on as for any other train_rows
    rows = sample.shape[0]
    first = sample.index_select(0, torch.randperm(rows, generator=gen)[:CODEWORDS].to(vectors.device))
    words = first.view(CODEWORDS, m, dsub).permute(1, 0, 2).contiguous()
    labels = torch.empty((m, rows), dtype=torch.int64, device=vectors.device)
    previous = None
    history, updates = [], 0
    while True:
        won = torch.zeros(m, dtype=torch.float64, device=vectors.device)

        def sink(s, i0, i1, chunk_labels, chunk_best):
            labels[s, i0:i1] = chunk_labels
            won[s] += chunk_best.double().sum()
        _sweep(words, sample, chunk, sink)
        history.extend(won.tolist())
        changed = m * rows if previous is None else int((labels != previous).sum())
        if updates == iters or changed == 0:
            break
        for s in range(m):
            members, offsets, sizes = cluster._members(labels[s], CODEWORDS)
            sums = ops.kmeans_sums(sample[:, s * dsub:(s + 1) * dsub], members, offsets, CODEWORDS)
            words[s] = torch.where((sizes > 0).unsqueeze(1), sums / sizes.to(torch.float32).unsqueeze(1), words[s])
        previous = labels.clone()
        updates += 1
    return Codebook(words, history, updates)
