"""The reverse-edge merge of kNN lists (include/mdx_knn_reverse.h; ops.knn_reverse_merge) and the approximate kNN join over the
inverted file (mdir_amd/ivf.py, IVFIndex.knn_join) restated in numpy (a helper module, imported by test_knn_reverse_host.py,
test_gpu_knn_reverse.py, test_gpu_knn_reverse_memcontract.py and test_gpu_ivf_knn.py).

The merge is the header's definition read aloud: a dict of offers, and per row a lexsort by (order key, id) of its own valid entries
together with its offers.  Nothing of the kernels' shape is in ``merge``; ``entering`` restates what the count and fill passes keep
(an offer is dropped where it cannot enter its row), for the tests of those two entry points.  ``random_lists`` and ``hub_lists``
build the inputs the GPU tests share."""
import numpy as np

import ivf_restatement as IR
from kmeans_restatement import order_key

F32 = np.float32
MAX_K = 128                     # MDX_KNN_REVERSE_MAX_K


def offers(ids, scores):
    """{j: [(i, score bits)]}: the offers to every row -- the edges (i, j) with j a valid id other than i, and i not in ids[j, :]."""
    ids, bits = np.asarray(ids, np.int64), np.ascontiguousarray(scores, F32).view(np.uint32)
    n, k = ids.shape
    member = [set(row.tolist()) for row in ids]
    out = {}
    for i in range(n):
        for r in range(k):
            j = int(ids[i, r])
            if 0 <= j < n and j != i and i not in member[j]:
                out.setdefault(j, []).append((i, int(bits[i, r])))
    return out


def merge(ids, scores):
    """(ids int64 [n, k], scores fp32 [n, k], gained int32 [n]) of the definition in include/mdx_knn_reverse.h."""
    ids, scores = np.asarray(ids, np.int64), np.ascontiguousarray(scores, F32)
    n, k = ids.shape
    assert 1 <= k <= MAX_K
    bits = scores.view(np.uint32)
    offered = offers(ids, scores)
    out_ids = np.full((n, k), -1, np.int64)
    out_bits = np.full((n, k), np.array(np.nan, F32).view(np.uint32), np.uint32)
    gained = np.zeros(n, np.int32)
    for j in range(n):
        own = [(int(ids[j, r]), int(bits[j, r]), 0) for r in range(k) if 0 <= ids[j, r] < n]
        pool = own + [(i, b, 1) for i, b in offered.get(j, [])]
        if not pool:
            continue
        pid = np.array([p[0] for p in pool], np.int64)
        pbits = np.array([p[1] for p in pool], np.uint32)
        src = np.array([p[2] for p in pool], np.int32)
        order = np.lexsort((pid, order_key(pbits.view(F32))))[:k]
        out_ids[j, :len(order)], out_bits[j, :len(order)] = pid[order], pbits[order]
        gained[j] = src[order].sum()
    return out_ids, out_bits.view(F32), gained


def entering(ids, scores):
    """(counts int32 [n], offsets int64 [n + 1], offers uint32 [total, 2]): the offers that can enter their row -- all of them where
    the row has padding (an id outside [0, n) is padding), else those that precede its last entry by (order key, id) -- as (score bits,
    source id), row after row and by ascending source inside a row."""
    ids, scores = np.asarray(ids, np.int64), np.ascontiguousarray(scores, F32)
    n, k = ids.shape
    offered = offers(ids, scores)
    counts, rows = np.zeros(n, np.int32), []
    for j in range(n):
        mine = sorted(offered.get(j, []))
        if mine and ((ids[j] >= 0) & (ids[j] < n)).all():
            last = (int(order_key(scores[j, k - 1:])[0]), int(ids[j, k - 1]))
            mine = [(i, b) for i, b in mine if (int(order_key(np.array([b], np.uint32).view(F32))[0]), i) < last]
        counts[j] = len(mine)
        rows += [(b, i) for i, b in mine]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(counts)
    return counts, offsets, np.array(rows, np.uint32).reshape(-1, 2)


def sorted_segments(offer_buffer, offsets):
    """The defined extent of an offer buffer, every segment sorted by source id (the order inside one comes from atomic tickets)."""
    buf = np.ascontiguousarray(offer_buffer).view(np.uint32).reshape(-1, 2)[:int(offsets[-1])].copy()
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        seg = buf[lo:hi]
        buf[lo:hi] = seg[np.argsort(seg[:, 1], kind="stable")]
    return buf


VALUES = np.array([np.nan, -2.0, -0.0, 0.0, 1.0, 2.0, np.inf], F32)      # what ``special=True`` draws the scores from


def random_lists(n, k, seed, share=0.6, levels=7, special=False):
    """(ids int64 [n, k], scores fp32 [n, k]): per row the first k, in the library's order, of a random ``share`` of the columns of a
    symmetric score matrix with ``levels`` distinct integer values (many ties; ``special``: NaN, the two zeros and infinity among them).
    A row with fewer candidates than k ends in -1 / NaN."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, levels, (n, n))
    a = np.triu(a) + np.triu(a, 1).T
    sym = VALUES[a % len(VALUES)] if special else a.astype(F32)
    ids, sc = np.empty((n, k), np.int64), np.empty((n, k), F32)
    for i in range(n):
        cand = np.flatnonzero(rng.random(n) < share).astype(np.int64)
        ids[i], sc[i] = IR.select(sym[i, cand], cand, k)
    return ids, sc


def hub_lists(n=3000):
    """k = 4 lists in which every row lists row 0 at the score i % 50, and row 0 lists the four low-scoring rows 1 .. 4: row 0 is
    offered n - 5 entries, with ties among them and scores equal to its own entries', and must end with (49, 99, 149, 199).  Every row
    i >= 1 also lists itself (100) and its two successors (-1, -2), so full rows receive offers that precede their last entry."""
    ids, sc = np.empty((n, 4), np.int64), np.empty((n, 4), F32)
    ids[0], sc[0] = [4, 3, 2, 1], [4, 3, 2, 1]
    for i in range(1, n):
        nxt, nxt2 = 1 + i % (n - 1), 1 + (i + 1) % (n - 1)
        ids[i], sc[i] = [i, 0, nxt, nxt2], [100, i % 50, -1, -2]
    return ids, sc


def knn_join(labels, lists, probes, scores, k, reverse=True):
    """IVFIndex.knn_join on the host: ``scores`` is the full fp32 [n, n] matrix of the rows against themselves, ``probes`` int64
    [n, nprobe] the lists every row probes.  (ids, scores, scanned, gained); the forward lists are IR.search_labels."""
    n = len(labels)
    k = min(k, n)
    ids, sc, scanned = IR.search_labels(labels, lists, probes, scores, k)
    if scanned.min() < k:
        raise ValueError("a row scanned %d candidates, fewer than k = %d" % (scanned.min(), k))
    if not reverse:
        return ids, sc, scanned, np.zeros(n, np.int32)
    ids, sc, gained = merge(ids, sc)
    return ids, sc, scanned, gained


def recall(ids, truth):
    """The share of the true neighbours (int64 [n, k]) found in ``ids``, over all rows."""
    hits = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth))
    return hits / truth.size
