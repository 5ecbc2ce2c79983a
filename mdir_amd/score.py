"""The retrieval score of the eval scenarios -- the orchestrator of the hot path.

Drop-in for ``mdir/components/optim/score/cirscore.py`` (``CirDatasetAp`` :16-80) and
the ``SCORES`` registry (``score/__init__.py:3-8``): same parameters, same logger
rows, same printed lines.  What changed underneath (cirscore.py:54-71):

    extract_vectors(...)            -> descriptors stay on the GPU as [N,D]
    np.dot(vecs.T, qvecs)           -> DescriptorIndex(vecs).scores(qvecs)   (mdx_scores)
    np.argsort(-scores, axis=0)     -> rank_full(scores)                     (mdx_rank_full)
    compute_map_and_print(ranks)    -> same function on the device ranking

The default ``ranking="positions"`` feeds compute_map from ``mdx_rank_of`` (identical APs --
asserted in the tests and in bench.py -- without an N-long sort; the score object exposes
nothing but the APs); ``ranking="full"`` runs the reference's dot + argsort + compute_map
sequence literally.  ``storage="f16"`` (criterion key, not in the reference) keeps the database shard in
fp16 for the fp16 MFMA -- BASELINE.json configs[4]; ``storage="i8"`` keeps it as int8 codes with one fp32 scale per row
on the int8 MFMA (a quarter of the fp32 bytes; scores defined to the bit by include/mdx.h ``MDX_I8``).  ``similarity="split3"`` (criterion key, not in the reference) takes
the LABELLED split-precision form of the dot product on the same fp32 shard (three bf16 pieces per operand on the bf16
MFMA: 0.75 of the exact kernel's time, scores within 2e-6 of it; ``"split2"``: two fp16 pieces with a scaled residual,
block floating point, 0.63 of the exact kernel's time, same bound for data of ordinary dynamic range; default ``"exact"`` =
the k-ordered fp32 chain).  ``query_expansion: {k, alpha}`` and ``database_augmentation: {k, alpha}`` (criterion keys,
not in the reference) add the re-ranking every table on the revisited protocol reports beside the raw numbers: alpha-QE of
the queries and DBA of the database (``mdir_amd/rerank.py``); with both, DBA runs first and alpha-QE searches the augmented
database.  Single-process only for now.  ``diffusion: {k, kq, gamma, alpha, iters, tol}`` (criterion key, every
sub-key optional, defaults of the paper's release) re-ranks by diffusion on a mutual kNN graph of the database
(``rerank.diffusion``), after DBA when both are set; not together with query_expansion; single-process only.  The optional
sub-key ``truncate: R`` (``kq <= R <= 4096``; no default) solves each query on the subgraph of its top-R rows instead.
``rescore: {shortlist: K}`` (criterion key, ``1 <= K <= 4096``, clamped to N; needs ``storage: i8`` or ``f16``;
single-process; not with the re-ranking keys) rescores each query's top-K rows of the compressed scores exactly
(``ops.rescore``, the fp32 chain) and ranks by the composite: the rescored top-K, then every other row in the compressed
order.  For int8 it prints the certified depth (``ops.rescore_certify``) per query: min / median / max.
``neighbours: exact | i8`` (criterion key, default ``exact``; only with ``database_augmentation``, ``diffusion`` or ``k_reciprocal``) chooses how
their neighbour lists are built: ``i8`` prunes the all-pairs top-k on a temporary int8 index of the rows (``search.knn_join``);
the lists, and so the results, are the same bits.  ``neighbours: {ivf: {lists: L, nprobe: P, storage: f32 | i8, shortlist: S, reverse:
true | false, iters: .., seed: ..}}`` builds them approximately instead: a temporary ``IVFIndex.train(vecs, L, storage=...)`` and its
``knn_join`` (``mdir_amd/ivf.py``) -- every row searches its ``P`` best lists and the lists are merged with their reverse edges.
``lists`` and ``nprobe`` are required; ``storage`` defaults to ``i8``, ``shortlist`` (int8 only) to ``min(4 k_max, 4096)`` over the
enabled keys, ``reverse`` to true; ``iters`` and ``seed`` go to ``cluster.kmeans``.  Every enabled key needs ``k <= 128``.
``k_reciprocal: {k1, k2, lam, truncate}`` (criterion key, every sub-key optional, defaults 20, 6, 0.3, 1000) re-ranks each query's
``truncate`` best rows by the Jaccard overlap of k-reciprocal codes (``rerank.k_reciprocal``), after DBA when both are set;
with ``query_expansion`` the expanded queries' scores are its first stage; not together with ``diffusion`` or ``rescore``;
single-process only; it honours ``neighbours: i8``.
``search: {index: exact | i8 | f16 | ivf | ivfpq | graph, depth: K, ...}`` (criterion key, not in the reference; ``1 <= K <= 4096``, clamped to
N; single-process only) evaluates the top-``K`` lists an index returns instead of a ranking of every row: the index is built on
``vecs``, searched with ``qvecs``, and the ``[Q, K]`` ids go through ``evaluate.compute_map_and_print_topk`` -- the AP of a top-K list
is the left-to-right partial sum of the full ranking's AP with the reference's normaliser ``len(ok)`` (NOT ``min(len(ok), K)``), so
``K = N`` reproduces the reference bit for bit; P@kappa is NaN where the list does not determine it; one more ``>>`` line prints the
label recall.  The printed and logged keys are the reference's.  Routes: ``exact`` -- ``ops.topk`` of the exact scores; ``i8`` /
``f16`` with ``shortlist`` (required) and ``exact`` (default false) -- ``search.search`` on a ``DescriptorIndex`` of that storage;
``ivf`` with ``lists`` and ``nprobe`` (required), ``storage: f32 | i8`` (default ``i8``), ``shortlist`` / ``exact`` (int8 only),
``iters`` / ``seed`` (to ``cluster.kmeans``) -- ``IVFIndex.train`` and its ``search``; ``ivfpq`` with ``lists`` and ``nprobe``
(required), ``m`` (default 64), ``refine: i8``, ``shortlist``, ``rescore``, ``iters`` / ``seed`` -- ``IVFPQIndex.train`` and its
``search`` (the index keeps the fp32 rows only where ``shortlist`` / ``rescore`` read them); ``graph`` with ``degree`` and ``beam``
(required; ``depth <= beam <= 512``, so a ``depth`` above 512 is refused on this route), ``k0`` (default ``2 * degree``), ``width``
(default 1), ``seeds`` (default 8), ``entries: sample | medoids`` (default ``sample``) with ``n_entries`` (default 1024) or, for the
medoids, ``lists`` (required) and ``iters`` of the k-means behind them, ``seed``, and ``neighbours: exact | i8 | {ivf: {...}}`` in the
grammar of the ``neighbours`` key (default ``exact``) -- ``graph.GraphIndex.build`` and its ``search``, a beam search over a pruned
kNN graph with exact chain scores.  A ``shortlist`` is at least ``depth``.
``recall: true`` (default false) also computes the exact top-``K`` -- one full scan -- and prints ``recall@K`` against it, min / mean
over the queries (``search.recall_at``, ``ops.topk_overlap``).  Not together with ``ranking: full``, ``rescore``, ``query_expansion``,
``diffusion``, ``k_reciprocal`` or a ``storage`` / ``similarity`` other than the default (the route chooses how the rows are kept);
``database_augmentation`` is allowed and runs first.  The ``dataset`` times gain the laps ``build_index`` and ``search`` in front of
``compute_score``.  ``CirDatasetAp.searched_map(vecs, qvecs)`` is the part after extraction; the index, the search's result, the
evaluation's stats and the recall stay reachable as ``last_index``, ``last_search``, ``last_stats`` and ``last_recall``.
"""
import contextlib
import gzip
import json
import lzma
import math
import os.path
from collections import OrderedDict

import numpy as np
import torch

from . import cluster, graph, ivf, ivfpq, ops, rerank
from . import search as _search
from .datasets import configdataset, get_data_root, initialize_transforms
from .evaluate import (compute_map_and_print, compute_map_and_print_composite, compute_map_and_print_from_scores,
                       compute_map_and_print_topk)
from .networks import extract_vectors_device
from .scenario import StopWatch, path_join
from .trace import range_


_TABLE_SUFFIXES = (".tsv", ".tsv.gz", ".tsv.xz", ".csv", ".csv.gz", ".csv.xz")


def _cell(value):
    """``GenericReader.str2collection`` (daan/data/file_readers.py:89-98): an empty cell is None, a cell bracketed
    on BOTH ends by [] or {} is JSON, everything else stays the string it is."""
    if not value:
        return None
    if (value[0], value[-1]) in {("[", "]"), ("{", "}")}:
        return json.loads(value)
    return value


def _read_table(path, keys=None):
    """Columns of a .tsv/.csv table (optionally .gz/.xz), as ``initialize_file_reader(path, keys=keys).get()`` returns them
    (daan/data/file_readers.py:101-135,243-252).  The reader is restated with its plain-split semantics, not ``csv``:
    the separator is a tab iff one of the last two dot-separated path pieces is "tsv" (:111), the header line is stripped
    on both sides (:115), data lines lose only their "\n" (:126), so a "\r" or a quote character stays in the cell; a key
    absent from the header is ``list.index``'s ValueError (:120), a short line an IndexError (:128).  An unreadable path is
    a ValueError as in ``GenericReader.open`` (:68-76) -- without its 1 + 8 + 27 seconds of retries."""
    base, suffix = path.rsplit(".", 1)
    if suffix in ("gz", "xz"):
        suffix = base.rsplit(".", 1)[1]
    if suffix not in ("tsv", "csv"):
        raise ValueError("Suffix '%s' is not supported ('%s')" % (suffix, path))
    assert path.endswith(_TABLE_SUFFIXES), path
    separator = "\t" if "tsv" in path.rsplit(".", 2) else ","
    fopen = lzma.open if path.endswith(".xz") else gzip.open if path.endswith(".gz") else open
    try:
        handle = fopen(path, "rb")
    except (FileNotFoundError, OSError, EOFError):
        raise ValueError("Error with path '%s' (try %s)" % (path, 1))
    with handle:
        header = next(handle).decode("utf8").strip().split(separator)
        indexes = [header.index(x) for x in keys] if keys else list(range(len(header)))
        columns = [[] for _ in indexes]
        for line in handle:
            cells = line.decode("utf8").strip("\n").split(separator)
            for column, j in zip(columns, indexes):
                column.append(_cell(cells[j]))
    return OrderedDict(zip([header[i] for i in indexes], columns))


class CirDatasetAp:
    search = last_search = last_index = last_recall = last_stats = None      # the `search` key: off; what its last run left

    def __init__(self, params):
        self.image_size = params.pop("image_size")
        self.dataset = params.pop("dataset")
        self.transforms = initialize_transforms(params.pop("transforms"), params.pop("mean_std"))
        self.ranking = params.pop("ranking", "positions")
        assert self.ranking in {"full", "positions"}, self.ranking
        # how the database shard is kept on the GPU: "f32" (the reference's arithmetic: exact k-ordered fp32 chain) or
        # "f16" (BASELINE.json configs[4]: fp16 descriptors on the fp16 MFMA, fp32 accumulation; half the HBM bytes,
        # scores within ~1e-3 relative: a looser, separately tested contract)
        # "i8" (int8 codes + one fp32 scale per row on the int8 MFMA: a quarter of the fp32 bytes, scores defined to the bit
        # by include/mdx.h MDX_I8)
        self.storage = params.pop("storage", "f32")
        assert self.storage in {"f32", "f16", "i8"}, self.storage
        # how an fp32 shard is multiplied: "exact" (default: the k-ordered fp32 fma chain, the parity contract) or "split3"
        # (labelled second mode, include/mdx.h MDX_F32_SPLIT3)
        self.similarity = params.pop("similarity", "exact")
        assert self.similarity in {"exact", "split3", "split2"}, self.similarity
        assert not (self.similarity != "exact" and self.storage != "f32"), "similarity: split3 / split2 multiply an fp32 shard"
        # re-ranking (not in the reference): alpha-QE of the queries and DBA of the database, each {k, alpha}; None = off
        self.query_expansion = _rerank_params(params.pop("query_expansion", None), "query_expansion")
        self.database_augmentation = _rerank_params(params.pop("database_augmentation", None), "database_augmentation")
        # diffusion on a mutual kNN graph of the database (not in the reference): {k, kq, gamma, alpha, iters, tol}; None = off
        self.diffusion = _diffusion_params(params.pop("diffusion", None))
        if self.diffusion and self.query_expansion:
            raise ValueError("diffusion together with query_expansion is not supported: choose one")
        # k-reciprocal re-ranking (not in the reference): {k1, k2, lam, truncate}; None = off
        self.k_reciprocal = _k_reciprocal_params(params.pop("k_reciprocal", None))
        if self.k_reciprocal and self.diffusion:
            raise ValueError("k_reciprocal together with diffusion is not supported: choose one")
        # how DBA, the diffusion graph and the k-reciprocal encoding get their neighbour lists: "exact" (fp32 scores of every pair) or "i8" (the same lists,
        # pruned on a temporary int8 index of the rows: search.knn_join)
        # or {"ivf": {...}}: approximate lists from a temporary inverted file of the rows (IVFIndex.knn_join)
        self.neighbours = params.pop("neighbours", "exact")
        depths = [p[key] for p, key in ((self.database_augmentation, "k"), (self.diffusion, "k"), (self.k_reciprocal, "k1")) if p]
        if isinstance(self.neighbours, dict):
            self.neighbours = _ivf_neighbours_params(self.neighbours, depths)
        elif isinstance(self.neighbours, bool) or self.neighbours not in ("exact", "i8"):
            raise ValueError("neighbours: 'exact' or 'i8', got %r" % (self.neighbours,))
        if self.neighbours != "exact" and not depths:
            raise ValueError("neighbours: %s builds the neighbour lists of database_augmentation / diffusion / k_reciprocal; neither is on"
                             % ("ivf" if isinstance(self.neighbours, dict) else self.neighbours))
        for key in ("database_augmentation", "diffusion"):
            if self.neighbours == "i8" and getattr(self, key) and getattr(self, key)["k"] > ops.KNN_JOIN_MAX_K:
                raise ValueError("neighbours: i8 keeps at most %d neighbours per row (KNN_JOIN_MAX_K); %s has k=%d"
                                 % (ops.KNN_JOIN_MAX_K, key, getattr(self, key)["k"]))
        # exact rescoring of a shortlist of the compressed scores (not in the reference): {shortlist: K}; None = off
        self.rescore = _rescore_params(params.pop("rescore", None))
        if self.rescore:
            if self.storage not in {"i8", "f16"}:
                raise ValueError("rescore: rescores the shortlist of an int8 or fp16 shard (storage: i8 / f16); storage is %s, "
                                 "whose scores are already exact" % self.storage)
            others = [k for k in ("query_expansion", "database_augmentation", "diffusion", "k_reciprocal") if getattr(self, k)]
            if others:
                raise ValueError("rescore together with %s is not supported" % " / ".join(others))
        # top-K lists of an index, evaluated as truncated rankings (not in the reference): {index, depth, ...}; None = off
        self.search = _search_params(params.pop("search", None))
        if self.search:
            if self.ranking == "full":
                raise ValueError("search together with ranking: full is not supported: a top-K list is not a full ranking")
            for key in ("rescore", "query_expansion", "diffusion", "k_reciprocal"):
                if getattr(self, key):
                    raise ValueError("search together with %s is not supported" % key)
            if self.storage != "f32" or self.similarity != "exact":
                raise ValueError("search together with storage: %s / similarity: %s is not supported: search: {index: ...} chooses "
                                 "how the rows are kept" % (self.storage, self.similarity))
        if isinstance(self.dataset, dict):
            assert self.dataset.keys() == {"name", "queries", "db", "imgdir"}
            imgdir = self.dataset["imgdir"]
            data = _read_table(self.dataset["db"], ["identifier"])
            self.images = [path_join(imgdir, x) for x in data["identifier"]]
            mapping = {x: i for i, x in enumerate(data["identifier"])}
            data = _read_table(self.dataset["queries"], ["query", "bbx", "ok", "junk"])
            self.qimages = [path_join(imgdir, x) for x in data["query"]]
            self.bbxs = [tuple(x) if x else None for x in data["bbx"]]
            self.gnd = [{"ok": [mapping[x] for x in ok], "junk": [mapping[x] for x in junk]}
                        for ok, junk in zip(data["ok"], data["junk"])]
            self.dataset = self.dataset["name"]
        else:
            cfg = configdataset(self.dataset, os.path.join(get_data_root(), "test"))
            self.images = [cfg["im_fname"](cfg, i) for i in range(cfg["n"])]
            self.qimages = [cfg["qim_fname"](cfg, i) for i in range(cfg["nq"])]
            self.bbxs = [tuple(cfg["gnd"][i]["bbx"]) if cfg["gnd"][i]["bbx"] else None for i in range(cfg["nq"])]
            self.gnd = cfg["gnd"]
        assert not params, params.keys()

    def __call__(self, network, device, logger):
        stopwatch = StopWatch()
        if _world_size() > 1 and (self.query_expansion or self.database_augmentation):
            raise ValueError("%s: query_expansion / database_augmentation re-rank in a single process for now; this run has "
                             "%d ranks" % (self.dataset, _world_size()))
        if _world_size() > 1 and self.diffusion:
            raise ValueError("%s: diffusion re-ranks in a single process (the graph spans the whole database); this run has "
                             "%d ranks" % (self.dataset, _world_size()))
        if _world_size() > 1 and self.k_reciprocal:
            raise ValueError("%s: k_reciprocal re-ranks in a single process (the codes span the whole database); this run has "
                             "%d ranks" % (self.dataset, _world_size()))
        if _world_size() > 1 and self.rescore:
            raise ValueError("%s: rescore runs in a single process for now; this run has %d ranks" % (self.dataset, _world_size()))
        if _world_size() > 1 and self.search:
            raise ValueError("%s: search builds and searches its index in a single process; this run has %d ranks"
                             % (self.dataset, _world_size()))
        if _world_size() > 1:
            # one process per GPU (torchrun eval.py ...): every rank extracts its slice of the
            # database, which stays resident as its shard; same rows go to the logger on every rank
            from .sharded import sharded_retrieval_map
            print(">> {}: database + query images, rank {} of {}...".format(self.dataset, *_rank_world()))
            averages, scores_per_query = sharded_retrieval_map(
                network, self.images, self.qimages, self.bbxs, self.gnd, self.dataset, self.image_size,
                self.transforms, device, lap=stopwatch.lap, storage=self.storage,
                compute="chain" if self.similarity == "exact" else self.similarity)
            self._log(logger, stopwatch, averages, scores_per_query)
            return
        print(">> {}: database images...".format(self.dataset))
        with range_("%s/extract_descriptors" % self.dataset):
            vecs = extract_vectors_device(network, self.images, self.image_size, self.transforms, device=device)
            print(">> {}: query images...".format(self.dataset))
            if self.images == self.qimages and set(self.bbxs) == {None}:
                qvecs = vecs.clone()
            else:
                qvecs = extract_vectors_device(network, self.qimages, self.image_size, self.transforms, device=device,
                                               bbxs=self.bbxs)
        stopwatch.lap("extract_descriptors")

        print(">> {}: Evaluating...".format(self.dataset))
        if self.search:
            with range_("%s/compute_score" % self.dataset):
                averages, scores_per_query = self.searched_map(vecs, qvecs, lap=stopwatch.lap)
            stopwatch.lap("compute_score")
            self._log(logger, stopwatch, averages, scores_per_query)
            return
        with range_("%s/compute_score" % self.dataset):
            # one evaluation multiplies the database once: the exact product reads `vecs` [N,D] where it lies
            # (mdx_scores_rowmajor: same kernels and bits as on an index, no 8 GB re-tiled copy); the fp16 shard and the
            # split-precision modes need their own operand formats and build an index
            if self.database_augmentation:
                with range_("database_augmentation"):               # DBA first: the queries keep their own descriptors
                    with _neighbour_index(vecs, self.neighbours) as nix:
                        vecs = rerank.database_augmentation(vecs, index=nix, **self.database_augmentation)
            direct = self.storage == "f32" and self.similarity == "exact" and vecs.shape[1] % 4 == 0
            index = None if direct else ops.DescriptorIndex(vecs, "ND", storage=self.storage)
            with range_("similarity"):
                if self.query_expansion:
                    compute = "chain" if self.similarity == "exact" else self.similarity
                    scores, _ = rerank.query_expansion(qvecs, vecs, index=index, compute=compute, **self.query_expansion)
                elif direct:
                    scores = ops.scores_rowmajor(vecs, qvecs, "ND")     # [Q,N] = (vecs.T @ qvecs).T
                else:
                    kw = {} if self.similarity == "exact" else {"compute": self.similarity}
                    scores = index.scores(qvecs, "ND", **kw)
            if self.diffusion:
                p = self.diffusion
                with range_("diffusion"):
                    truncate = p.get("truncate")
                    with _neighbour_index(vecs, self.neighbours) as nix:
                        graph = rerank.DiffusionGraph(vecs, k=p["k"], gamma=p["gamma"], weights=truncate is not None, index=nix)
                    scores = rerank.diffusion(qvecs, vecs, graph, kq=p["kq"], alpha=p["alpha"], iters=p["iters"],
                                              tol=p["tol"], scores=scores, truncate=truncate)
                    graph.close()
            if self.k_reciprocal:
                p = self.k_reciprocal
                with range_("k_reciprocal"):
                    with _neighbour_index(vecs, self.neighbours) as nix:
                        encoding = rerank.ReciprocalEncoding(vecs, k1=p["k1"], k2=p["k2"], index=nix)
                    scores = rerank.k_reciprocal(qvecs, vecs, encoding, lam=p["lam"], truncate=p["truncate"], scores=scores)
                    encoding.close()
            if self.rescore:
                averages, scores_per_query = self._rescored_map(vecs, qvecs, scores, index)
            elif self.ranking == "full":
                with range_("ranking"):
                    ranks = ops.rank_full(scores)                   # [Q,N] = argsort(-scores, axis=0).T
                averages, scores_per_query = compute_map_and_print(self.dataset, ranks.t(), self.gnd)
            else:
                averages, scores_per_query = compute_map_and_print_from_scores(self.dataset, scores, self.gnd)
        stopwatch.lap("compute_score")
        if index is not None:
            index.close()
        self._log(logger, stopwatch, averages, scores_per_query)

    def _rescored_map(self, vecs, qvecs, scores, index):
        """mAP of the composite ranking: each query's top-K of the compressed ``scores`` rescored exactly and sorted, then
        every other row in the compressed order (the shortlist is exactly the first K of ``rank_full(scores)``, so the
        positions beyond K do not move)."""
        n = scores.shape[1]
        K = min(self.rescore["shortlist"], n)
        with range_("rescore"):
            top_ids, top_scores = ops.topk(scores, K)
            ids, sc = ops.rescore(vecs, qvecs, top_ids, "ND")
        if self.storage == "i8":
            depth, _ = ops.rescore_certify(sc, top_scores[:, K - 1], qvecs, index.i8_bounds(), n, "ND")
            c = depth.cpu().numpy()
            print(">> {}: rescored top-{}, certified depth min {} / median {:g} / max {}".format(
                self.dataset, K, int(c.min()), float(np.median(c)), int(c.max())))
        if self.ranking == "full":
            with range_("ranking"):
                ranks = ops.rank_full(scores)
                ranks[:, :K] = ids
            return compute_map_and_print(self.dataset, ranks.t(), self.gnd)
        return compute_map_and_print_composite(self.dataset, scores, ids, self.gnd)

    def searched_map(self, vecs, qvecs, lap=None):
        """The ``search`` key after extraction: ``(averages, per_query)`` of the top-``depth`` lists that the chosen index returns
        for ``qvecs`` fp32 ``[Q, D]`` against ``vecs`` fp32 ``[N, D]`` (device tensors, as the existing path holds them), through
        ``compute_map_and_print_topk``.  DBA, if set, changes ``vecs`` first.  ``lap(name)`` is called, after a device
        synchronisation, when the index is built (``build_index``) and when the lists are there (``search``).  The index
        (closed on the way out, on errors too), the search's result, the evaluation's ``.stats`` and, with ``recall: true``, the
        per-query recall against the exact top-``depth`` stay reachable as ``last_index``, ``last_search``, ``last_stats`` and
        ``last_recall``."""
        p = self.search
        self.last_search = self.last_index = self.last_recall = self.last_stats = None

        def mark(name):
            if lap is not None:
                torch.cuda.synchronize(vecs.device)
                lap(name)

        if self.database_augmentation:
            with range_("database_augmentation"):
                with _neighbour_index(vecs, self.neighbours) as nix:
                    vecs = rerank.database_augmentation(vecs, index=nix, **self.database_augmentation)
        n = vecs.shape[0]
        depth = min(p["depth"], n)
        index = None
        try:
            with range_("build_index"):
                index = self.last_index = _search_index(p, vecs)
            mark("build_index")
            with range_("search"):
                res = self.last_search = _search_lists(p, index, vecs, qvecs, depth)
            mark("search")
            out = compute_map_and_print_topk(self.dataset, res.ids, self.gnd, n)
            self.last_stats = getattr(out, "stats", None)               # (None: a dataset the reference does not evaluate)
            if p["recall"]:
                with range_("recall"):
                    exact_ids, _ = ops.topk(_exact_scores(vecs, qvecs), depth)
                    self.last_recall = _search.recall_at(res.ids, exact_ids, depth)[:, 0]
                print(">> {}: recall@{} against the exact top-{}: min {:.4f} / mean {:.4f}".format(
                    self.dataset, depth, depth, float(np.min(self.last_recall)), float(np.mean(self.last_recall))))
        finally:
            if index is not None:
                index.close()
        return out

    @staticmethod
    def _log(logger, stopwatch, averages, scores_per_query):
        first_score = scores_per_query[list(scores_per_query.keys())[0]]
        logger(None, len(first_score), "dataset", stopwatch.reset(), "scalar/time")
        logger(None, len(first_score), "score_avg", averages, "scalar/score")
        assert len({len(x) for x in scores_per_query.values()}) == 1
        for i, _ in enumerate(first_score):
            logger(i, len(first_score), "score", {x: scores_per_query[x][i] for x in scores_per_query},
                   "scalar/score")


def _rerank_params(value, key):
    """``{k, alpha}`` of a re-ranking criterion key, validated (None: the key is absent)."""
    if value is None:
        return None
    if not isinstance(value, dict) or set(value) != {"k", "alpha"}:
        raise ValueError("%s: a mapping with exactly the keys k and alpha, got %r" % (key, value))
    k, alpha = value["k"], value["alpha"]
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("%s: k must be an integer >= 1, got %r" % (key, k))
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError("%s: alpha must be a finite number >= 0, got %r" % (key, alpha))
    return {"k": k, "alpha": float(alpha)}


@contextlib.contextmanager
def _neighbour_index(vecs, neighbours):
    """The index the neighbour lists are pruned on: a temporary int8 one of ``vecs`` for ``neighbours: i8`` (closed on exit),
    None for ``exact``; for ``neighbours: {ivf: ...}`` an ``IVFNeighbours`` over a temporary ``IVFIndex.train`` of ``vecs``."""
    if isinstance(neighbours, dict):
        p = neighbours["ivf"]
        index = ivf.IVFIndex.train(vecs, p["lists"], storage=p["storage"], **{key: p[key] for key in ("iters", "seed") if key in p})
        try:
            yield ivf.IVFNeighbours(index, p["nprobe"], shortlist=p["shortlist"], reverse=p["reverse"])
        finally:
            index.close()
        return
    index = ops.DescriptorIndex(vecs, "ND", storage="i8") if neighbours == "i8" else None
    try:
        yield index
    finally:
        if index is not None:
            index.close()


_IVF_NEIGHBOURS_KEYS = ("lists", "nprobe", "storage", "shortlist", "reverse", "iters", "seed")


def _ivf_neighbours_params(value, depths):
    """``{"ivf": {lists, nprobe, storage, shortlist, reverse[, iters][, seed]}}`` of the ``neighbours`` criterion key with its defaults
    filled in, validated; ``depths``: the k of every enabled re-ranking key."""
    if set(value) != {"ivf"} or not isinstance(value["ivf"], dict):
        raise ValueError("neighbours: 'exact' or 'i8', or the mapping {ivf: {lists, nprobe, ...}}, got %r" % (value,))
    given = value["ivf"]
    unknown = set(given) - set(_IVF_NEIGHBOURS_KEYS)
    if unknown:
        raise ValueError("neighbours: ivf: unknown keys %s (allowed: %s)" % (sorted(unknown, key=str), ", ".join(_IVF_NEIGHBOURS_KEYS)))
    for key in ("lists", "nprobe"):
        if key not in given:
            raise ValueError("neighbours: ivf: %s is required" % key)
    out = dict(given)
    for key in ("lists", "nprobe", "iters"):
        if key in out and (isinstance(out[key], bool) or not isinstance(out[key], int) or out[key] < 1):
            raise ValueError("neighbours: ivf: %s must be an integer >= 1, got %r" % (key, out[key]))
    if "seed" in out and (isinstance(out["seed"], bool) or not isinstance(out["seed"], int) or out["seed"] < 0):
        raise ValueError("neighbours: ivf: seed must be an integer >= 0, got %r" % (out["seed"],))
    if out["nprobe"] > out["lists"]:
        raise ValueError("neighbours: ivf: 1 <= nprobe <= lists is required, got nprobe=%d lists=%d" % (out["nprobe"], out["lists"]))
    out.setdefault("storage", "i8")
    if out["storage"] not in ivf.STORAGES:
        raise ValueError("neighbours: ivf: storage must be 'f32' or 'i8', got %r" % (out["storage"],))
    out.setdefault("reverse", True)
    if not isinstance(out["reverse"], bool):
        raise ValueError("neighbours: ivf: reverse must be true or false, got %r" % (out["reverse"],))
    deepest = max(depths) if depths else 0
    if deepest > ops.KNN_REVERSE_MAX_K:
        raise ValueError("neighbours: ivf keeps at most %d neighbours per row (KNN_REVERSE_MAX_K); an enabled key has k=%d"
                         % (ops.KNN_REVERSE_MAX_K, deepest))
    if out["storage"] == "f32":
        if out.get("shortlist") is not None:
            raise ValueError("neighbours: ivf: shortlist needs storage: i8 (the fp32 lists are scored exactly)")
        out["shortlist"] = None
    else:
        out.setdefault("shortlist", max(1, min(4 * deepest, ops.RESCORE_MAX_K)))
        x = out["shortlist"]
        if isinstance(x, bool) or not isinstance(x, int) or not max(1, deepest) <= x <= ops.RESCORE_MAX_K:
            raise ValueError("neighbours: ivf: shortlist must be an integer in [k_max, %d] = [%d, %d], got %r"
                             % (ops.RESCORE_MAX_K, max(1, deepest), ops.RESCORE_MAX_K, x))
    return {"ivf": out}


def _diffusion_params(value):
    """``{k, kq, gamma, alpha, iters, tol}`` of the ``diffusion`` criterion key, each optional (the defaults of
    ``rerank.DIFFUSION_DEFAULTS``), and ``truncate``, optional without a default (in the result only when given),
    validated (None: the key is absent)."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError("diffusion: a mapping with the optional keys k, kq, gamma, alpha, iters, tol, truncate, got %r"
                         % (value,))
    unknown = set(value) - set(rerank.DIFFUSION_DEFAULTS) - {"truncate"}
    if unknown:
        raise ValueError("diffusion: unknown keys %s (allowed: k, kq, gamma, alpha, iters, tol, truncate)" % sorted(unknown))
    out = dict(rerank.DIFFUSION_DEFAULTS, **value)
    for key in ("k", "kq", "iters"):
        x = out[key]
        if isinstance(x, bool) or not isinstance(x, int) or x < 1:
            raise ValueError("diffusion: %s must be an integer >= 1, got %r" % (key, x))
    for key, upper in (("gamma", None), ("alpha", 1.0), ("tol", None)):
        x = out[key]
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x < 0 or \
                (upper is not None and x >= upper):
            raise ValueError("diffusion: %s must be a finite number >= 0%s, got %r"
                             % (key, "" if upper is None else " and < %g" % upper, x))
        out[key] = float(x)
    if "truncate" in out:
        x = out["truncate"]
        if isinstance(x, bool) or not isinstance(x, int) or not out["kq"] <= x <= ops.DIFFUSION_MAX_R:
            raise ValueError("diffusion: truncate must be an integer in [kq, %d] = [%d, %d], got %r"
                             % (ops.DIFFUSION_MAX_R, out["kq"], ops.DIFFUSION_MAX_R, x))
    return out


def _k_reciprocal_params(value):
    """``{k1, k2, lam, truncate}`` of the ``k_reciprocal`` criterion key, each optional (the defaults of
    ``rerank.K_RECIPROCAL_DEFAULTS``), validated (None: the key is absent)."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError("k_reciprocal: a mapping with the optional keys k1, k2, lam, truncate, got %r" % (value,))
    unknown = set(value) - set(rerank.K_RECIPROCAL_DEFAULTS)
    if unknown:
        raise ValueError("k_reciprocal: unknown keys %s (allowed: k1, k2, lam, truncate)" % sorted(unknown))
    out = dict(rerank.K_RECIPROCAL_DEFAULTS, **value)
    for key in ("k1", "k2", "truncate"):
        x = out[key]
        if isinstance(x, bool) or not isinstance(x, int) or x < 1:
            raise ValueError("k_reciprocal: %s must be an integer >= 1, got %r" % (key, x))
    k1, k2 = out["k1"], out["k2"]
    if k1 > ops.KRECIP_MAX_K1 or k2 > k1 or k2 * k1 * (1 + (k1 + 1) // 2) > ops.KRECIP_MAX_NNZ:
        raise ValueError("k_reciprocal: k1 <= %d, k2 <= k1 and k2 * k1 * (1 + ceil(k1 / 2)) <= %d are required, got k1=%r k2=%r"
                         % (ops.KRECIP_MAX_K1, ops.KRECIP_MAX_NNZ, k1, k2))
    if out["truncate"] > ops.KRECIP_MAX_R:
        raise ValueError("k_reciprocal: truncate must be an integer in [1, %d], got %r" % (ops.KRECIP_MAX_R, out["truncate"]))
    x = out["lam"]
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or not 0 <= x <= 1:
        raise ValueError("k_reciprocal: lam must be a finite number in [0, 1], got %r" % (x,))
    out["lam"] = float(x)
    return out


def _rescore_params(value):
    """``{shortlist: K}`` of the ``rescore`` criterion key, validated (None: the key is absent)."""
    if value is None:
        return None
    if not isinstance(value, dict) or set(value) != {"shortlist"}:
        raise ValueError("rescore: a mapping with exactly the key shortlist, got %r" % (value,))
    x = value["shortlist"]
    if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= ops.RESCORE_MAX_K:
        raise ValueError("rescore: shortlist must be an integer in [1, %d], got %r" % (ops.RESCORE_MAX_K, x))
    return {"shortlist": x}


_SEARCH_KEYS = {
    "exact": ("index", "depth", "recall"),
    "i8": ("index", "depth", "recall", "shortlist", "exact"),
    "f16": ("index", "depth", "recall", "shortlist", "exact"),
    "ivf": ("index", "depth", "recall", "lists", "nprobe", "storage", "shortlist", "exact", "iters", "seed"),
    "ivfpq": ("index", "depth", "recall", "lists", "nprobe", "m", "refine", "shortlist", "rescore", "iters", "seed"),
    "graph": ("index", "depth", "recall", "degree", "k0", "beam", "width", "seeds", "entries", "n_entries", "lists", "iters", "seed",
              "neighbours"),
}
_GRAPH_ENTRIES = ("sample", "medoids")


def _search_params(value):
    """``{index, depth, ...}`` of the ``search`` criterion key with its defaults filled in, validated (None: the key is absent).
    The limits are those of the index classes (``ops.RESCORE_MAX_K``, ``ops.PQ_MAX_M``, ``ivf.STORAGES``, ``ivfpq.REFINES``)."""
    if value is None:
        return None
    if not isinstance(value, dict) or not isinstance(value.get("index"), str) or value["index"] not in _SEARCH_KEYS:
        raise ValueError("search: a mapping {index: %s, depth: K, ...}, got %r" % (" | ".join(_SEARCH_KEYS), value))
    kind = value["index"]
    allowed = _SEARCH_KEYS[kind]
    unknown = set(value) - set(allowed)
    if unknown:
        raise ValueError("search: index: %s: unknown keys %s (allowed: %s)" % (kind, sorted(unknown, key=str), ", ".join(allowed)))
    required = ("depth",) + {"exact": (), "i8": ("shortlist",), "f16": ("shortlist",), "graph": ("degree", "beam")}.get(kind, ("lists", "nprobe"))
    for key in required:
        if key not in value:
            raise ValueError("search: index: %s: %s is required" % (kind, key))
    out = dict(value)

    def integer(key, lo, hi=None):
        x = out[key]
        if isinstance(x, bool) or not isinstance(x, int) or x < lo or (hi is not None and x > hi):
            raise ValueError("search: %s must be an integer %s, got %r" % (key, ">= %d" % lo if hi is None else "in [%d, %d]" % (lo, hi), x))

    def boolean(key):
        out.setdefault(key, False)
        if not isinstance(out[key], bool):
            raise ValueError("search: %s must be true or false, got %r" % (key, out[key]))

    integer("depth", 1, ops.RESCORE_MAX_K)
    boolean("recall")
    for key in ("lists", "nprobe", "iters"):
        if key in out:
            integer(key, 1)
    if "seed" in out:
        integer("seed", 0)
    if "nprobe" in out and out["nprobe"] > out["lists"]:
        raise ValueError("search: 1 <= nprobe <= lists is required, got nprobe=%d lists=%d" % (out["nprobe"], out["lists"]))
    if "shortlist" in allowed:
        out.setdefault("shortlist", None)
        if out["shortlist"] is not None:
            integer("shortlist", out["depth"], ops.RESCORE_MAX_K)
    if kind == "ivf":
        out.setdefault("storage", "i8")
        if out["storage"] not in ivf.STORAGES:
            raise ValueError("search: storage must be 'f32' or 'i8', got %r" % (out["storage"],))
    if "exact" in allowed:
        boolean("exact")
        if kind == "ivf" and out["storage"] == "f32" and (out["shortlist"] is not None or out["exact"]):
            raise ValueError("search: shortlist and exact need storage: i8 (the fp32 lists are scored exactly)")
        if out["exact"] and out["shortlist"] is None:
            raise ValueError("search: exact: true needs a shortlist")
    if kind == "ivfpq":
        out.setdefault("m", 64)
        integer("m", 1, ops.PQ_MAX_M)
        out.setdefault("refine", None)
        if out["refine"] is not None and not (isinstance(out["refine"], str) and out["refine"] in ivfpq.REFINES):
            raise ValueError("search: refine must be 'i8' or absent, got %r" % (out["refine"],))
        out.setdefault("rescore", None)
        if out["rescore"] is not None:
            if out["refine"] is None or out["shortlist"] is None:
                raise ValueError("search: rescore needs refine: i8 and a shortlist")
            integer("rescore", out["depth"], out["shortlist"])
    if kind == "graph":
        if out["depth"] > ops.GRAPH_MAX_BEAM:
            raise ValueError("search: index: graph: depth = %d is above the beam limit %d (the lists are the head of the beam)"
                             % (out["depth"], ops.GRAPH_MAX_BEAM))
        integer("degree", 1, ops.GRAPH_MAX_DEGREE)
        out.setdefault("k0", 2 * out["degree"])
        integer("k0", 1, ops.GRAPH_MAX_K0)
        integer("beam", out["depth"], ops.GRAPH_MAX_BEAM)
        out.setdefault("width", 1)
        integer("width", 1, ops.GRAPH_MAX_WIDTH)
        out.setdefault("seeds", 8)
        integer("seeds", 1, ops.GRAPH_MAX_SEEDS)
        out.setdefault("entries", "sample")
        if not (isinstance(out["entries"], str) and out["entries"] in _GRAPH_ENTRIES):
            raise ValueError("search: entries must be 'sample' or 'medoids', got %r" % (out["entries"],))
        if out["entries"] == "medoids":
            if "lists" not in out:
                raise ValueError("search: index: graph: entries: medoids needs lists (the k-means behind them)")
            if "n_entries" in out:
                raise ValueError("search: n_entries goes with entries: sample (the medoids are one per non-empty list)")
        else:
            if "lists" in out or "iters" in out:
                raise ValueError("search: index: graph: lists and iters go with entries: medoids")
            out.setdefault("n_entries", 1024)
            integer("n_entries", 1)
        out.setdefault("neighbours", "exact")
        nb = out["neighbours"]
        if isinstance(nb, dict):
            out["neighbours"] = _ivf_neighbours_params(nb, [out["k0"] + 1])
        elif not (isinstance(nb, str) and nb in ("exact", "i8")):
            raise ValueError("search: neighbours: 'exact' or 'i8', or the mapping {ivf: {lists, nprobe, ...}}, got %r" % (nb,))
        elif nb == "i8" and out["k0"] + 1 > ops.KNN_JOIN_MAX_K:
            raise ValueError("search: neighbours: i8 keeps at most %d neighbours per row (KNN_JOIN_MAX_K); k0 + 1 = %d"
                             % (ops.KNN_JOIN_MAX_K, out["k0"] + 1))
    return out


def _exact_scores(vecs, qvecs):
    """fp32 ``[Q, N]``: the exact chain scores, read from ``vecs`` where it lies, or through an fp32 index where D % 4 != 0."""
    if vecs.shape[1] % 4 == 0:
        return ops.scores_rowmajor(vecs, qvecs, "ND")
    index = ops.DescriptorIndex(vecs, "ND")
    try:
        return index.scores(qvecs, "ND")
    finally:
        index.close()


def _search_index(p, vecs):
    """The index of the ``search`` key over ``vecs`` (None for ``index: exact``); the caller closes it."""
    kind = p["index"]
    if kind == "exact":
        return None
    if kind in ("i8", "f16"):
        return ops.DescriptorIndex(vecs, "ND", storage=kind)
    kmeans = {key: p[key] for key in ("iters", "seed") if key in p}
    if kind == "graph":
        entries = None
        if p["entries"] == "medoids":
            km = cluster.kmeans(vecs, p["lists"], **kmeans)
            entries = graph.medoids(vecs, km.centroids, km.labels)
        with _neighbour_index(vecs, p["neighbours"]) as nix:
            return graph.GraphIndex.build(vecs, p["degree"], p["k0"], neighbours=nix, entries=entries,
                                          n_entries=p.get("n_entries", 1024), seed=p.get("seed", 0))
    if kind == "ivf":
        return ivf.IVFIndex.train(vecs, p["lists"], storage=p["storage"], **kmeans)
    keep_rows = p["shortlist"] is not None and (p["refine"] is None or p["rescore"] is not None)
    return ivfpq.IVFPQIndex.train(vecs, p["lists"], m=p["m"], kmeans=kmeans, keep_rows=keep_rows, refine=p["refine"])


def _search_lists(p, index, vecs, qvecs, depth):
    """The result of the route's search, a named tuple whose ``ids`` are int64 ``[Q, depth]``."""
    kind = p["index"]
    if kind == "exact":
        ids, scores = ops.topk(_exact_scores(vecs, qvecs), depth)
        return _search.SearchResult(ids, scores, None, torch.empty(0, dtype=torch.int64, device=ids.device))
    if kind in ("i8", "f16"):
        return _search.search(index, vecs, qvecs, depth, p["shortlist"], exact=p["exact"])
    if kind == "ivf":
        return index.search(qvecs, depth, p["nprobe"], shortlist=p["shortlist"], exact=p["exact"])
    if kind == "graph":
        return index.search(qvecs, depth, beam=p["beam"], width=p["width"], seeds=p["seeds"])
    return index.search(qvecs, depth, p["nprobe"], shortlist=p["shortlist"], rescore=p["rescore"])


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _world_size():
    return _rank_world()[1]


SCORES = {"cirdatasetap": CirDatasetAp}


def initialize_score(params):
    return SCORES[params.pop("type")](params)
