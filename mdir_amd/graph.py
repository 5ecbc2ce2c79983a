"""A graph index: beam search over a pruned fixed-degree neighbour graph of the database (include/mdx_graph.h).

The fourth family beside the scan, the inverted file and IVF-PQ.  The graph is made of the neighbour lists the library already builds for
DBA, diffusion and k-reciprocal re-ranking -- ``search.knn_join`` (exact, or pruned on an int8 shard) or ``IVFIndex.knn_join`` with its
reverse-edge merge (approximate) -- pruned and completed as CAGRA does, and walked by ``ops.graph_search`` with exact chain scores: every
returned score has the bits of ``DescriptorIndex(rows, "ND").scores`` at its id, so no rescoring stage follows.  ``tests/graph_restatement.py``
restates the build and the walk in numpy.

Build, ``GraphIndex.from_lists(rows, ids, degree, entries=None, n_entries=1024, seed=0)``.  ``ids`` int64 ``[n, k]`` (a tensor, a
``search.KnnResult`` or an ``ivf.IVFKnnResult``), ``k >= 2``, ``k - 1 <= ops.GRAPH_MAX_K0``, ``degree <= ops.GRAPH_MAX_DEGREE``.
  1. ``strip_self``: per row, the entries that are valid and not the row's own id, in order, the first ``K0 = k - 1``, padded with -1.
  2. ``ops.graph_detours`` of these lists (the kernel of the build: ``n K0^2`` look-ups).
  3. Forward lists: each row's positions in the order (detours, rank), a stable sort; the first ``R = degree``.
  4. Reverse lists: for row b the sources i whose forward list holds b, in the order (rank of b in i's forward list, i); the first R.
  5. The row of the graph: the two lists interleaved, f0, r0, f1, r1, ... continuing with whichever remains; of that sequence the first
     R distinct ids that are not the row's own, padded with -1, as int32.
Steps 3 to 5 are stable sorts and gathers of torch over the ``n R`` edges; integers only, so two builds agree to the bit.
``GraphIndex.build(rows, degree=32, k0=None, neighbours=None, chunk=None, **from_lists_kwargs)`` makes the lists first, at ``k = k0 + 1``
with ``k0 = 2 * degree`` by default: ``neighbours=None`` is ``search.knn_join(None, rows, k)``, an int8 ``DescriptorIndex`` of ``rows``
the pruned route (``k <= 64``), an ``ivf.IVFNeighbours`` its ``lists_of(rows, k)`` (``k <= 128``) -- the handles of ``rerank``.

Entry rows.  ``index.entries`` int64 ``[E]`` are database ids and ``index.entry_index`` an fp32 ``DescriptorIndex`` of ``rows[entries]``;
a query's seeds are ``entries[topk(entry_index.scores(q), S)]``, one small exact scan.  ``entries=None`` takes a sample of
``min(n, n_entries)`` ids: the first of ``torch.randperm(n)`` of ``torch.Generator().manual_seed(seed)``, sorted.  A walk cannot leave a
component of the graph, so a clustered database wants an entry in every cluster: ``medoids(rows, centroids, labels=None)`` returns, per
non-empty list of a k-means partition, the member with the best exact chain score against its centroid (ties: the smaller id).

Search, ``index.search(queries, k, beam=64, width=1, seeds=8, max_steps=None, qlayout="ND", center=None)`` -> :data:`GraphResult`.
``seeds`` is a count or an explicit int64 ``[nq, S]`` tensor of ids; ``max_steps`` defaults to ``ceil(4 * beam / width)``.

Out of scope: walks on int8 or fp16 codes (the scoring step of the kernel is one device function so that such a scorer with a final
``ops.rescore`` can follow), HNSW layers, NN-descent construction, adding or removing rows, a certificate, more than one GPU.
"""
from collections import namedtuple

import torch

from . import cluster, ops, rerank

GraphResult = namedtuple("GraphResult", ["ids", "scores", "steps", "scored"])
GraphResult.__doc__ = """ids int64 [nq, k] and scores fp32 [nq, k]: the head of every query's beam, rank_full's order, padded with -1 and
NaN; steps int32 [nq]: the steps of the walk; scored int32 [nq]: the chains the query ran (a diagnostic)."""


def _ids_of(ids):
    ids = getattr(ids, "ids", ids)
    ops._kmeans_tensor(ids, torch.int64, "GraphIndex", "ids", 2)
    return ids


def strip_self(ids):
    """int64 ``[n, k - 1]``: per row of ``ids`` (int64 ``[n, k]`` on the device) the valid entries that are not the row's own id, in
    order, the first ``k - 1``, padded with -1."""
    n, k = ids.shape
    if k < 2:
        raise ValueError("strip_self: lists of k = %d hold no neighbour beside the row itself" % k)
    own = torch.arange(n, device=ids.device).unsqueeze(1)
    keep = (ids >= 0) & (ids < n) & (ids != own)
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :k - 1]
    return torch.where(torch.gather(keep, 1, order), torch.gather(ids, 1, order), ids.new_full((), -1)).contiguous()


def _compact(values, keep, width):
    """int64 ``[n, width]``: per row the kept values in order, padded with -1."""
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :width]
    out = torch.where(torch.gather(keep, 1, order), torch.gather(values, 1, order), values.new_full((), -1))
    if out.shape[1] < width:
        out = torch.cat([out, out.new_full((out.shape[0], width - out.shape[1]), -1)], dim=1)
    return out


def optimise(lists, degree, detours=None):
    """int32 ``[n, degree]``: the search graph of the neighbour lists ``lists`` (int64 ``[n, K0]``, best first, own id removed) -- steps 2
    to 5 of the module docstring."""
    n, k0 = lists.shape
    dev = lists.device
    det = ops.graph_detours(lists) if detours is None else detours
    valid = (lists >= 0) & (lists < n)
    # 3. forward: positions by (detours, rank); invalid entries have K0 detours and sort last
    pos = torch.sort(det.to(torch.int64), dim=1, stable=True).indices
    fwd = _compact(torch.gather(lists, 1, pos), torch.gather(valid, 1, pos), degree)              # valid prefix, -1 tail
    # 4. reverse: the edges (i, j, b = fwd[i, j]) flattened rank-major are in the order (j, i); a stable sort by b keeps it
    tgt = fwd.t().reshape(-1)
    src = torch.arange(n, device=dev).repeat(degree)
    live = tgt >= 0
    tgt, src = tgt[live], src[live]
    tgt, by = torch.sort(tgt, stable=True)
    src = src[by]
    starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    starts[1:] = torch.cumsum(torch.bincount(tgt, minlength=n), 0)
    place = torch.arange(tgt.numel(), device=dev) - starts[tgt]
    rev = torch.full((n, degree), -1, dtype=torch.int64, device=dev)
    fits = place < degree
    rev[tgt[fits], place[fits]] = src[fits]
    # 5. interleave (the padding of either list drops out: the other one continues), first `degree` distinct ids but the row's own
    seq = torch.stack([fwd, rev], dim=2).reshape(n, 2 * degree)
    by_id = torch.sort(seq, dim=1, stable=True)                                                    # equal ids: the earlier position first
    again = torch.zeros_like(seq, dtype=torch.bool)
    again.scatter_(1, by_id.indices[:, 1:], by_id.values[:, 1:] == by_id.values[:, :-1])
    own = torch.arange(n, device=dev).unsqueeze(1)
    return _compact(seq, (seq >= 0) & ~again & (seq != own), degree).to(torch.int32).contiguous()


def medoids(rows, centroids, labels=None):
    """int64 ``[number of non-empty lists]``: per list of the partition, in ascending list id, the member with the best exact chain score
    against its centroid (``rank_full``'s order), ties to the smaller id.  ``labels=None``: ``cluster.assign(centroids, rows)``'s;
    explicit labels are scored against their own centroid by ``ops.rescore``."""
    if labels is None:
        labels, best = cluster.assign(centroids, rows)
    else:
        ops._kmeans_tensor(labels, torch.int64, "medoids", "labels", 1)
        _, best = ops.rescore(centroids, rows, labels.reshape(-1, 1).contiguous())
        best = best.reshape(-1)
    n, lists = rows.shape[0], centroids.shape[0]
    # the order key of rank_full (desc_key of the library) on the score's bits, then the id
    u = best.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where((u << 1) & 0xFFFFFFFF == 0, torch.zeros_like(u), u)
    key = torch.where(u & 0x80000000 != 0, u, 0xFFFFFFFF - (u | 0x80000000))
    key = torch.where(best != best, torch.full_like(key, 0xFFFFFFFF), key)
    packed = key * n + torch.arange(n, device=rows.device)
    first = torch.full((lists,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=rows.device)
    first.scatter_reduce_(0, labels, packed, "amin")
    return (first[torch.bincount(labels, minlength=lists) > 0] % n).contiguous()


class GraphIndex:
    """The graph index of ``rows`` (fp32 ``[n, d]`` on the device, read in place by every search) -- the module docstring has the
    contract.  ``graph`` int32 ``[n, degree]``, ``entries`` int64 ``[E]``."""

    def __init__(self, rows, graph, entries):
        ops._kmeans_matrix(rows, "GraphIndex", "rows")
        n = rows.shape[0]
        ops._kmeans_tensor(graph, torch.int32, "GraphIndex", "graph", 2)
        ops._ivf_vector(graph, torch.int32, "GraphIndex", "graph", (n, graph.shape[1]), rows.device)
        ops._kmeans_tensor(entries, torch.int64, "GraphIndex", "entries", 1)
        ops._ivf_vector(entries, torch.int64, "GraphIndex", "entries", (entries.shape[0],), rows.device)
        if graph.shape[1] > ops.GRAPH_MAX_DEGREE or rows.shape[1] > ops.GRAPH_MAX_D:
            raise ValueError("GraphIndex: degree = %d and d = %d must be at most %d and %d" % (
                graph.shape[1], rows.shape[1], ops.GRAPH_MAX_DEGREE, ops.GRAPH_MAX_D))
        lo, hi = int(entries.min()), int(entries.max())                        # the one read-back of the build
        if lo < 0 or hi >= n:
            raise ValueError("GraphIndex: entries must be ids in [0, %d), got %d .. %d" % (n, lo, hi))
        self.rows, self.graph, self.entries = rows, graph, entries
        self.n, self.d, self.degree = n, rows.shape[1], graph.shape[1]
        self.entry_index = ops.DescriptorIndex(rows.index_select(0, entries).contiguous(), "ND")

    @staticmethod
    def _sample(n, n_entries, seed, device):
        cluster._count(n_entries, "n_entries")
        cluster._count(seed, "seed", 0)
        gen = torch.Generator().manual_seed(seed)
        return torch.sort(torch.randperm(n, generator=gen)[:min(n, n_entries)]).values.to(device)

    @classmethod
    def from_lists(cls, rows, ids, degree, entries=None, n_entries=1024, seed=0):
        ids = _ids_of(ids)
        cluster._count(degree, "degree")
        ops._kmeans_matrix(rows, "GraphIndex", "rows")
        n, k = ids.shape
        if n != rows.shape[0] or ids.device != rows.device or not ids.is_contiguous():
            raise ValueError("GraphIndex: ids must be a contiguous [%d, k] tensor on %s, got %s on %s" % (
                rows.shape[0], rows.device, tuple(ids.shape), ids.device))
        if degree > ops.GRAPH_MAX_DEGREE or not 2 <= k <= ops.GRAPH_MAX_K0 + 1:
            raise ValueError("GraphIndex: degree = %d must be at most %d and the lists' k = %d in [2, %d]" % (
                degree, ops.GRAPH_MAX_DEGREE, k, ops.GRAPH_MAX_K0 + 1))
        graph = optimise(strip_self(ids), degree)
        if entries is None:
            entries = cls._sample(n, n_entries, seed, rows.device)
        return cls(rows, graph, entries)

    @classmethod
    def build(cls, rows, degree=32, k0=None, neighbours=None, chunk=None, **from_lists_kwargs):
        cluster._count(degree, "degree")
        k0 = 2 * degree if k0 is None else k0
        cluster._count(k0, "k0")
        ids, _ = rerank._neighbours(rows, k0 + 1, chunk, neighbours)
        if ids.shape[1] < 2:
            raise ValueError("GraphIndex.build: %d rows have no neighbour lists" % rows.shape[0])
        return cls.from_lists(rows, ids, degree, **from_lists_kwargs)

    def seeds_of(self, queries, count, qlayout="ND", center=None):
        """int64 ``[nq, S]``: the ``S = min(count, E)`` best entry rows of every query, as database ids."""
        cluster._count(count, "seeds")
        if self.entry_index is None:
            raise ValueError("the index is closed")
        scores = self.entry_index.scores(queries, qlayout, center)
        top, _ = ops.topk(scores, min(count, self.entries.shape[0], ops.GRAPH_MAX_SEEDS))
        return self.entries[top].contiguous()

    def search(self, queries, k, beam=64, width=1, seeds=8, max_steps=None, qlayout="ND", center=None):
        if self.entry_index is None:
            raise ValueError("the index is closed")
        if not isinstance(seeds, torch.Tensor):
            seeds = self.seeds_of(queries, seeds, qlayout, center)
        return GraphResult(*ops.graph_search(self.rows, self.graph, queries, seeds, k, beam, width, max_steps, qlayout, center))

    def nbytes(self):
        """Bytes of the index beside the rows: the graph, the entry ids and the entry shard."""
        extra = self.entry_index.device_bytes if self.entry_index is not None else 0
        return self.graph.numel() * 4 + self.entries.numel() * 8 + extra

    def state(self):
        """``{"graph", "entries", "n", "degree"}``: what :meth:`from_state` needs beside the rows (tensors on the host)."""
        return {"graph": self.graph.cpu(), "entries": self.entries.cpu(), "n": self.n, "degree": self.degree}

    @classmethod
    def from_state(cls, state, rows, device=None):
        device = rows.device if device is None else torch.device(device)
        rows = rows.to(device)
        graph, entries = state["graph"].to(device).contiguous(), state["entries"].to(device).contiguous()
        if rows.shape[0] != state["n"] or tuple(graph.shape) != (state["n"], state["degree"]):
            raise ValueError("GraphIndex.from_state: the state holds a [%d, %d] graph, got %s for %d rows" % (
                state["n"], state["degree"], tuple(graph.shape), rows.shape[0]))
        return cls(rows, graph, entries)

    def close(self):
        if getattr(self, "entry_index", None) is not None:
            self.entry_index.close()
            self.entry_index = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
