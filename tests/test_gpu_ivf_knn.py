"""IVFIndex.knn_join (mdir_amd/ivf.py) on the device: the approximate kNN join of the rows with themselves through the inverted file,
merged with its reverse edges, and the re-ranking code on an ``IVFNeighbours`` handle.  One database for all tests -- N = 700 unit rows
without cluster structure, D = 96, 6 lists of three k-means iterations, k = 10 -- built once and never written."""
import numpy as np
import pytest

import ivf_restatement as IR
import knn_reverse_restatement as KR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
N, D, LISTS, K = 700, 96, 6, 10

_world = {}


def world():
    """rows (device), the fit, an fp32 and an int8 index of them, and the exact join; made at the first call."""
    if not _world:
        import torch
        from mdir_amd import cluster, ivf, search
        rng = np.random.default_rng(26)
        rows = rng.standard_normal((N, D)).astype(F32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(F32)
        t = torch.from_numpy(rows).to(DEV)
        fit = cluster.kmeans(t, LISTS, iters=3)
        exact = search.knn_join(None, t, K)
        _world.update(rows=t, fit=fit, f32=ivf.IVFIndex(t, fit.centroids, fit.labels), i8=ivf.IVFIndex(t, fit.centroids, fit.labels, storage="i8"),
                      exact=(host(exact.ids), host(exact.scores)))
    return _world


def host(t):
    return t.detach().cpu().numpy()


def same(res, ids, scores):
    IR.same_bits(host(res.ids), ids), IR.same_bits(host(res.scores), scores)


def test_every_list_probed_is_the_exact_join():
    w = world()
    for index, kw in ((w["f32"], {}), (w["i8"], {"shortlist": N})):
        res = index.knn_join(K, LISTS, **kw)
        same(res, *w["exact"])
        assert not host(res.gained).any() and host(res.gained).dtype == np.int32 and host(res.scanned).tolist() == [N] * N
        assert (host(res.ids)[:, 0] == np.arange(N)).all()                   # a row's own match leads its list


def test_forward_stage_is_the_search_and_the_chunk_changes_nothing():
    w = world()
    for index, kw in ((w["f32"], {}), (w["i8"], {"shortlist": 40})):
        want = index.search(w["rows"], K, 2, **kw)
        res = index.knn_join(K, 2, reverse=False, **kw)
        same(res, host(want.ids), host(want.scores))
        IR.same_bits(host(res.scanned), host(want.scanned))
        assert not host(res.gained).any()
        other = index.knn_join(K, 2, reverse=False, chunk=97, **kw)
        for a, b in zip(res, other):
            IR.same_bits(host(a), host(b))
        merged = [index.knn_join(K, 2, chunk=c, **kw) for c in (None, 97)]
        for a, b in zip(*merged):
            IR.same_bits(host(a), host(b))


def test_reverse_stage_equals_the_restatement_and_only_helps():
    from mdir_amd import ops
    w = world()
    index = w["f32"]
    forward = index.knn_join(K, 2, reverse=False)
    res = index.knn_join(K, 2)
    want = KR.merge(host(forward.ids), host(forward.scores))
    same(res, want[0], want[1])
    IR.same_bits(host(res.gained), want[2])
    IR.same_bits(host(res.scanned), host(forward.scanned))
    # the symmetry premise on the device: every returned score is the exact chain of its id, as the row itself would score it
    again_ids, again = ops.rescore(w["rows"], w["rows"], res.ids, "ND")
    same(res, host(again_ids), host(again))
    before, after = KR.recall(host(forward.ids), w["exact"][0]), KR.recall(host(res.ids), w["exact"][0])
    print("recall@%d: %.4f forward, %.4f merged; gained %d" % (K, before, after, int(host(res.gained).sum())))
    assert after >= before
    assert host(res.gained).sum() > 0
    # the int8 lists with an exhaustive shortlist give the same join
    via = w["i8"].knn_join(K, 2, shortlist=N)
    for a, b in zip(res, via):
        IR.same_bits(host(a), host(b))


def test_strided_rows():
    import torch
    from mdir_amd import ivf
    w = world()
    wide = torch.full((N, D + 4), float("nan"), device=DEV)
    wide[:, :D] = w["rows"]
    strided = wide[:, :D]
    assert not strided.is_contiguous()
    index = ivf.IVFIndex(strided, w["fit"].centroids, w["fit"].labels)
    try:
        for got, want in zip(index.knn_join(K, 2, chunk=300), w["f32"].knn_join(K, 2)):
            IR.same_bits(host(got), host(want))
    finally:
        index.close()


def test_a_row_with_fewer_candidates_than_k_is_refused():
    from mdir_amd import ivf
    w = world()
    centroids, labels = w["fit"].centroids.clone(), w["fit"].labels.clone()
    labels[labels == 5] = 0
    labels[:3] = 5                                                          # three rows in list 5 ...
    centroids[5] = w["rows"][0]                                             # ... which row 0 probes first: it is its own centroid
    index = ivf.IVFIndex(w["rows"], centroids, labels)
    try:
        with pytest.raises(ValueError, match="scanned 3 candidates, fewer than k = 10: nprobe = 1"):
            index.knn_join(K, 1)
        assert int(index.knn_join(3, 1, reverse=False).scanned.min()) == 3
    finally:
        index.close()


def test_reranking_on_a_handle_that_probes_every_list_is_the_exact_one():
    from mdir_amd import ivf, rerank
    w = world()
    rows = w["rows"]
    for handle in (ivf.IVFNeighbours(w["f32"], LISTS), ivf.IVFNeighbours(w["i8"], LISTS, shortlist=N)):
        IR.same_bits(host(rerank.database_augmentation(rows, K, 3.0, index=handle)), host(rerank.database_augmentation(rows, K, 3.0)))
        a, b = rerank.DiffusionGraph(rows, k=K), rerank.DiffusionGraph(rows, k=K, index=handle)
        assert a.edges() == b.edges() > 0
        for name in ("cols", "counts", "vals"):
            IR.same_bits(host(getattr(a, name)), host(getattr(b, name)))
        a.close(), b.close()
        a, b = rerank.ReciprocalEncoding(rows, k1=K, k2=4), rerank.ReciprocalEncoding(rows, k1=K, k2=4, index=handle)
        assert a.nnz() == b.nnz()
        for name in ("rk", "rk_counts", "rh", "rh_counts", "kth"):
            IR.same_bits(host(getattr(a, name)), host(getattr(b, name)))
        for x, y in zip(a.raw + a.expanded, b.raw + b.expanded):
            IR.same_bits(host(x), host(y))
        a.close(), b.close()
    with pytest.raises(ValueError, match="vecs must be the rows the index was built on"):
        rerank.DiffusionGraph(rows.clone(), k=K, index=ivf.IVFNeighbours(w["f32"], LISTS))
