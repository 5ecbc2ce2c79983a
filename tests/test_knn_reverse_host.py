"""The reverse-edge merge of kNN lists (include/mdx_knn_reverse.h; ops.knn_reverse_merge) and what is built on it (IVFIndex.knn_join,
IVFNeighbours, the ``neighbours: {ivf: ...}`` criterion key) on a CPU-only box: the restatement (tests/knn_reverse_restatement.py) on
hand-written cases, the census of the header, every refusal of the C ABI with nothing launched, the criterion key, and the dispatch of
the re-ranking code with fakes."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivf_restatement as IR
import knn_reverse_restatement as KR
from conftest import ROOT

NEW = ("mdx_knn_reverse_count", "mdx_knn_reverse_fill", "mdx_knn_reverse_merge")
F32 = np.float32
NAN = np.nan


# ------------------------------------------------------------------------------------------------ the restatement itself

def _merge(ids, scores):
    return KR.merge(np.array(ids, np.int64), np.array(scores, F32))


def test_restatement_on_hand_written_cases():
    # 0 lists 1 and 2; 1 lists 0; 2 lists 3; 3 lists 2.  The one edge without its reverse is 0 -> 2: row 2 is offered (0, 0.5)
    ids, sc, gained = _merge([[1, 2], [0, -1], [3, -1], [2, -1]], [[0.9, 0.5], [0.9, NAN], [0.7, NAN], [0.7, NAN]])
    assert ids.tolist() == [[1, 2], [0, -1], [3, 0], [2, -1]] and gained.tolist() == [0, 0, 1, 0]
    IR.same_bits(sc, np.array([[0.9, 0.5], [0.9, NAN], [0.7, 0.5], [0.7, NAN]], F32))
    # a full row: the offer enters only where it precedes the k-th own entry by (key, id); a tie on the score is decided by the id
    rows = [[1, 2], [0, 2], [0, 1], [0, 4], [0, 3]]
    scores = [[0.9, 0.8], [0.9, 0.1], [0.8, 0.1], [0.8, 0.2], [0.85, 0.2]]
    ids, sc, gained = _merge(rows, scores)
    # row 0 is offered (3, 0.8) and (4, 0.85): 4 takes the second place (0.85 > 0.8), 3 ties with 2 on 0.8 and loses on the id
    assert ids[0].tolist() == [1, 4] and gained.tolist() == [1, 0, 0, 0, 0]
    IR.same_bits(sc[0], np.array([0.9, 0.85], F32))
    scores[3][0] = 0.95                                                     # now (3, 0.95) leads row 0
    ids, sc, gained = _merge(rows, scores)
    assert ids[0].tolist() == [3, 1] and gained[0] == 2 - 1
    # the same tie won on the id: row 2 of three holds (5, 0.8) as its last entry, and is offered (1, 0.8)
    ids, sc, gained = _merge([[3, 4], [2, 3], [4, 5], [0, 1], [2, 0], [2, 0]],
                             [[0.5, 0.4], [0.8, 0.3], [0.9, 0.8], [0.5, 0.3], [0.9, 0.4], [0.8, 0.1]])
    assert ids[2].tolist() == [4, 1] and gained[2] == 1


def test_restatement_special_values_and_foreign_ids():
    # -0 and +0 are one key, and the bits stay; NaN sorts last but before the padding; ids -5 and n are padding in their own row,
    # no edge and no target; a self edge is no edge
    n = 5
    ids = [[0, 1, -5], [1, n, 2], [2, -1, -1], [3, 0, 1], [4, 0, -1]]
    sc = [[1.0, -0.0, 0.3], [1.0, 0.7, 0.0], [1.0, NAN, NAN], [1.0, 0.0, NAN], [1.0, NAN, NAN]]
    got_ids, got, gained = _merge(ids, sc)
    # row 0: own (0, 1.0), (1, -0.0); offers from 3 (+0.0) and 4 (NaN): key order 1.0, then the zeros by id 1 < 3; the NaN is cut
    assert got_ids[0].tolist() == [0, 1, 3] and gained[0] == 1
    IR.same_bits(got[0], np.array([1.0, -0.0, 0.0], F32))
    # row 1: own (1, 1.0), (2, 0.0) with the foreign id dropped; offers from 0 (-0.0) and 3 (NaN)
    assert got_ids[1].tolist() == [1, 0, 2] and gained[1] == 1
    IR.same_bits(got[1], np.array([1.0, -0.0, 0.0], F32))
    # row 2: own (2, 1.0); the offer from 1 (+0.0) fills its padding
    assert got_ids[2].tolist() == [2, 1, -1] and gained[2] == 1 and np.isnan(got[2, 2])
    assert got_ids[3].tolist() == [3, 0, 1] and got_ids[4].tolist() == [4, 0, -1] and gained[3:].tolist() == [0, 0]
    assert np.isnan(got[3, 2]) and np.isnan(got[4, 1])
    # k = 1 and n = 1
    ids1, _, g1 = _merge([[1], [2], [0]], [[0.5], [0.7], [0.6]])
    assert ids1.tolist() == [[2], [2], [1]] and g1.tolist() == [1, 0, 1]    # 0 <- (2, 0.6) > 0.5; 1 <- (0, 0.5) < 0.7; 2 <- (1, 0.7) > 0.6
    ids1, sc1, g1 = _merge([[0, -1]], [[1.0, NAN]])
    assert ids1.tolist() == [[0, -1]] and g1.tolist() == [0]


def test_restatement_of_the_join_on_planted_lists():
    """With every list probed the join is the exact top-k and gains nothing; with fewer probes the merge only adds true neighbours."""
    rows, truth, centres, _, _ = IR.planted(seed=3, lists=4, per=30, d=32)
    n = len(rows)
    scores = (rows.astype(np.float64) @ rows.astype(np.float64).T).astype(F32)
    scores = np.maximum(scores, scores.T)                                   # symmetric to the bit, as the chain is
    coarse = rows @ centres.T
    k = 8
    exact = np.stack([IR.select(scores[i], np.arange(n, dtype=np.int64), k)[0] for i in range(n)])
    everything = np.argsort(-coarse, axis=1, kind="stable").astype(np.int64)
    ids, sc, scanned, gained = KR.knn_join(truth, 4, everything, scores, k)
    assert (ids == exact).all() and not gained.any() and (scanned == n).all()
    # labels that move a quarter of the rows to the next list, and every row probing its own list and the next: a row that stayed
    # finds the neighbours that moved, a row that moved does not find those that stayed -- until they offer themselves.  (With one
    # probe nothing can be gained: both ends of an edge then lie in one list, and each has scanned the other.)
    labels = truth.copy()
    labels[::4] = (labels[::4] + 1) % 4
    probes = np.stack([labels, (labels + 1) % 4], axis=1)
    alone = KR.knn_join(labels, 4, labels[:, None].copy(), scores, k)
    assert not alone[3].any()
    forward = KR.knn_join(labels, 4, probes, scores, k, reverse=False)
    merged = KR.knn_join(labels, 4, probes, scores, k)
    assert not forward[3].any() and merged[3].sum() > 0
    assert KR.recall(merged[0], exact) >= KR.recall(forward[0], exact)
    with pytest.raises(ValueError, match="fewer than k"):
        KR.knn_join(np.array([0, 0, 0, 1, 1, 1, 1, 1]), 2, np.array([[0]] * 3 + [[1]] * 5), np.zeros((8, 8), F32), 4)


# ------------------------------------------------------------------------------------------------ census

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_knn_reverse.h"$', text, flags=re.M) and "kNN lists, reverse-edge merge" in text
    assert text.index('#include "mdx_refine.h"') < text.index('#include "mdx_knn_reverse.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_knn_reverse.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib, ops
    code = _declared()
    assert re.search(r"#ifndef MDX_H\s*\n#error", code)
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.KNN_REVERSE_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS)
              | set(_lib.IVF_EXPORTS) | set(_lib.LISTS_I8_EXPORTS) | set(_lib.LISTS_PQ_EXPORTS) | set(_lib.LISTS_EDIT_EXPORTS)
              | set(_lib.REFINE_EXPORTS))
    assert not declared & others and not {n for n in others if "knn_reverse" in n}
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_knn_reverse[a-z0-9_]*\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert int(re.search(r"#define MDX_KNN_REVERSE_MAX_K (\d+)", code).group(1)) == 128 == ops.KNN_REVERSE_MAX_K == KR.MAX_K
    header = open(os.path.join(ROOT, "include", "mdx_knn_reverse.h")).read()
    for word in ("Refusals", "Definition", "Determinism", "is never dereferenced", "legal under stream capture", "integer atomic",
                 "never writes at or beyond", "the caller's premise", "Alignment"):
        assert word in header, word
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_knn_reverse\.hip\b", makefile, flags=re.M) and "include/mdx_knn_reverse.h" in makefile
    assert '"mdx_knn_reverse.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "knn_reverse" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_entry_point_has_memory_contract_cases():
    from test_gpu_knn_reverse_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == set(NEW)
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_before_any_device_work():
    """Every refusal of the three calls through the C ABI with pointers that are no memory: nothing is launched (there is no device
    here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    ptr = [ctypes.c_void_p((1 << 20) + (i << 16)) for i in range(10)]
    big = 1 << 31

    def count(ids=ptr[0], scores=ptr[1], n=10, k=4, counts=ptr[2]):
        return h.mdx_knn_reverse_count(ids, scores, n, k, counts, None)

    def fill(ids=ptr[0], scores=ptr[1], n=10, k=4, offsets=ptr[3], cursor=ptr[4], offers=ptr[5], capacity=40):
        return h.mdx_knn_reverse_fill(ids, scores, n, k, offsets, cursor, offers, capacity, None)

    def merge(ids=ptr[0], scores=ptr[1], n=10, k=4, offsets=ptr[3], offers=ptr[5], capacity=40, out_ids=ptr[6], out_scores=ptr[7],
              gained=ptr[8]):
        return h.mdx_knn_reverse_merge(ids, scores, n, k, offsets, offers, capacity, out_ids, out_scores, gained, None)

    calls = {"mdx_knn_reverse_count": (count, ("ids", "scores", "counts"), {"ids": 8, "scores": 4, "counts": 4}),
             "mdx_knn_reverse_fill": (fill, ("ids", "scores", "offsets", "cursor", "offers"),
                                      {"ids": 8, "scores": 4, "offsets": 8, "cursor": 4, "offers": 8}),
             "mdx_knn_reverse_merge": (merge, ("ids", "scores", "offsets", "offers", "out_ids", "out_scores", "gained"),
                                       {"ids": 8, "scores": 4, "offsets": 8, "offers": 8, "out_ids": 8, "out_scores": 4, "gained": 4})}
    defaults = {"ids": ptr[0], "scores": ptr[1], "counts": ptr[2], "offsets": ptr[3], "cursor": ptr[4], "offers": ptr[5], "out_ids": ptr[6],
                "out_scores": ptr[7], "gained": ptr[8]}
    for name, (call, pointers, aligns) in calls.items():
        def refused(status, *words):
            msg = h.mdx_last_error()
            assert status == -1 and msg.startswith(name.encode() + b":"), (status, msg)
            for w in words:
                assert w.encode() in msg, (w, msg)
        for arg in pointers:
            refused(call(**{arg: None}), "NULL")
        for arg in ("n", "k"):
            for value in (0, -1, -big):
                refused(call(**{arg: value}), "must be >= 1")
        for k in (129, 1 << 20, big):
            refused(call(k=k), "k=%d > 128" % k)
        for n in (big, big + 5, 1 << 40):
            refused(call(n=n), "n=%d must be below 2^31" % n)
        refused(call(n=big // 128, k=128), "n * k must be below 2^31")
        refused(call(n=big - 1, k=2), "n * k must be below 2^31")
        assert call(n=big // 128 - 1, k=128, ids=None) == -1                # the largest n k gets as far as... the NULL check comes first
        if "capacity" in call.__code__.co_varnames:
            for capacity in (0, -1, -big):
                refused(call(capacity=capacity), "capacity=%d must be >= 1" % capacity)
        for arg, align in aligns.items():
            for off in {1, 2, 4} - {align, 2 * align}:
                if off % align:
                    refused(call(**{arg: ctypes.c_void_p(defaults[arg].value + off)}), arg, "aligned")


def test_python_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivf, ops
    ids, scores = torch.zeros((4, 2), dtype=torch.int64), torch.zeros((4, 2))
    for call in (lambda: ops.knn_reverse_merge(ids, scores), lambda: ops.knn_reverse_count(ids, scores),
                 lambda: ops.knn_reverse_fill(ids, scores, torch.zeros(5, dtype=torch.int64)),
                 lambda: ops.knn_reverse_apply(ids, scores, torch.zeros(5, dtype=torch.int64), torch.zeros(8, dtype=torch.int64))):
        with pytest.raises(ValueError, match="ids must be a CUDA"):
            call()

    def bare(storage, n=300, lists=3):
        index = ivf.IVFIndex.__new__(ivf.IVFIndex)
        index.rows, index.d, index.lists, index.coarse, index.n, index.storage = torch.zeros((n, 12)), 12, lists, object(), n, storage
        return index
    f32, i8 = bare("f32"), bare("i8")
    with pytest.raises(ValueError, match="knn_join on an int8 index needs a shortlist"):
        i8.knn_join(10, 2)
    with pytest.raises(ValueError, match="shortlist and exact need an int8 index"):
        f32.knn_join(10, 2, shortlist=40)
    with pytest.raises(ValueError, match="shortlist = 5 must be in \\[k = 10"):
        i8.knn_join(10, 2, shortlist=5)
    for index, kw in ((f32, {}), (i8, {"shortlist": 200})):
        with pytest.raises(ValueError, match="k = 129 > 128 with reverse=True"):
            index.knn_join(129, 2, **kw)
        for bad in (0, 4, True, 1.5):
            with pytest.raises(ValueError, match="nprobe"):
                index.knn_join(10, bad, **kw)
        for bad in (0, -1, True, 2.5):
            with pytest.raises(ValueError, match="k must be"):
                index.knn_join(bad, 2, **kw)
            with pytest.raises(ValueError, match="chunk must be"):
                index.knn_join(10, 2, chunk=bad, **kw)
        for bad in (0, 1, None, "yes"):
            with pytest.raises(ValueError, match="reverse must be a bool"):
                index.knn_join(10, 2, reverse=bad, **kw)
    # k is clamped to N before the limit: 200 neighbours of 100 rows are 100
    small = bare("f32", n=100)
    small.coarse = None
    with pytest.raises(ValueError, match="the index is closed"):            # past every check of knn_join itself
        small.knn_join(200, 2)
    with pytest.raises(ValueError, match="k = 129 > 128"):
        bare("f32", n=129).knn_join(200, 2)
    # the handle
    with pytest.raises(ValueError, match="index must be an IVFIndex"):
        ivf.IVFNeighbours(object(), 2)
    for bad in (0, 4, True):
        with pytest.raises(ValueError, match="nprobe"):
            ivf.IVFNeighbours(f32, bad)
    with pytest.raises(ValueError, match="reverse must be a bool"):
        ivf.IVFNeighbours(f32, 2, reverse=1)
    with pytest.raises(ValueError, match="shortlist must be"):
        ivf.IVFNeighbours(i8, 2, shortlist=0)


# ------------------------------------------------------------------------------------------------ the re-ranking code

def test_rerank_dispatch(monkeypatch):
    """A handle reaches index.knn_join with its own arguments; foreign vecs are refused; other objects are refused as before; None and
    a DescriptorIndex go to search.knn_join in the form they always had."""
    import torch
    from mdir_amd import ivf, rerank, search
    rows = torch.zeros((6, 8))
    seen = []

    class Stop(Exception):
        pass

    class Fake(ivf.IVFIndex):
        def __init__(self, rows):
            self.rows, self.lists, self.n = rows, 3, rows.shape[0]

        def knn_join(self, k, nprobe, shortlist=None, reverse=True, chunk=None):
            seen.append((k, nprobe, shortlist, reverse, chunk))
            raise Stop

    handle = ivf.IVFNeighbours(Fake(rows), 2, shortlist=40, reverse=False)
    with pytest.raises(Stop):
        rerank.database_augmentation(rows, 10, 3.0, index=handle)
    with pytest.raises(Stop):
        rerank.DiffusionGraph(rows, k=3, chunk=2, index=handle)
    with pytest.raises(Stop):
        rerank.ReciprocalEncoding(rows, k1=4, k2=2, index=ivf.IVFNeighbours(Fake(rows), 3))
    assert seen == [(6, 2, 40, False, None), (3, 2, 40, False, None), (4, 3, None, True, None)]
    # foreign vecs: another tensor, a slice, a strided view of the same storage
    wide = torch.zeros((6, 16))
    for vecs, index_rows in ((torch.zeros((6, 8)), rows), (rows[:5], rows), (wide[:, :8], wide[:, :8].contiguous()), (rows, wide[:, :8])):
        with pytest.raises(ValueError, match="vecs must be the rows the index was built on"):
            rerank.DiffusionGraph(vecs, k=3, index=ivf.IVFNeighbours(Fake(index_rows), 2))
    with pytest.raises(ValueError, match="vecs must be the rows"):          # the DN layout makes a transposed copy
        rerank.database_augmentation(rows.t().contiguous(), 3, 3.0, layout="DN", index=handle)
    strided = wide[:, :8]
    with pytest.raises(Stop):                                               # the same view is the same rows
        rerank.DiffusionGraph(strided, k=3, index=ivf.IVFNeighbours(Fake(strided), 2))
    for bad in (object(), Fake(rows)):                                      # the index itself is no handle
        with pytest.raises(ValueError, match="int8 DescriptorIndex"):
            rerank.database_augmentation(rows, 2, 3.0, index=bad)
        with pytest.raises(ValueError, match="int8 DescriptorIndex"):
            rerank.ReciprocalEncoding(rows, k1=4, k2=2, index=bad)
    calls = []

    def fake_join(index, vecs, k, chunk=None):
        calls.append((index, tuple(vecs.shape), k, chunk))
        raise Stop

    monkeypatch.setattr(search, "knn_join", fake_join)
    with pytest.raises(Stop):
        rerank.DiffusionGraph(rows, k=3, chunk=2)
    assert calls == [(None, (6, 8), 3, 2)]


# ------------------------------------------------------------------------------------------------ the criterion key

def _dataset(tmp_path):
    (tmp_path / "db.csv").write_text("identifier\na.jpg\nb.jpg\nc.jpg\n")
    (tmp_path / "q.tsv").write_text('query\tbbx\tok\tjunk\na.jpg\t\t["b.jpg"]\t[]\n')
    return {"name": "toy", "imgdir": "/img", "queries": str(tmp_path / "q.tsv"), "db": str(tmp_path / "db.csv")}


def _score(tmp_path, **criterion):
    from mdir_amd.score import initialize_score
    params = {"type": "cirdatasetap", "image_size": 64, "transforms": "pil2np | totensor | normalize",
              "mean_std": [[0.4] * 3, [0.2] * 3], "dataset": _dataset(tmp_path)}
    params.update(criterion)
    return initialize_score(params)


def _ivf(**sub):
    return {"ivf": dict({"lists": 16, "nprobe": 4}, **sub)}


def test_neighbours_mapping(tmp_path):
    s = _score(tmp_path, neighbours=_ivf(), diffusion={})                  # diffusion's k is 50
    assert s.neighbours == {"ivf": {"lists": 16, "nprobe": 4, "storage": "i8", "shortlist": 200, "reverse": True}}
    s = _score(tmp_path, neighbours=_ivf(), diffusion={"k": 30}, database_augmentation={"k": 100, "alpha": 1.0})
    assert s.neighbours["ivf"]["shortlist"] == 400                          # 4 x the deepest enabled key
    assert _score(tmp_path, neighbours=_ivf(), k_reciprocal={"k1": 20})  .neighbours["ivf"]["shortlist"] == 80
    s = _score(tmp_path, neighbours=_ivf(storage="f32", reverse=False, iters=5, seed=3), k_reciprocal={})
    assert s.neighbours == {"ivf": {"lists": 16, "nprobe": 4, "storage": "f32", "shortlist": None, "reverse": False, "iters": 5, "seed": 3}}
    assert _score(tmp_path, neighbours=_ivf(shortlist=128, nprobe=16), diffusion={"k": 128}).neighbours["ivf"]["shortlist"] == 128
    # refusals
    for sub, word in (({"lists": 0}, "lists must be an integer >= 1"), ({"lists": True}, "lists must be"), ({"nprobe": 0}, "nprobe must be"),
                      ({"nprobe": 17}, "1 <= nprobe <= lists"), ({"nprobe": 2.0}, "nprobe must be"), ({"storage": "f16"}, "storage must be"),
                      ({"reverse": 1}, "reverse must be"), ({"shortlist": 49}, "shortlist must be an integer in \\[k_max, 4096\\] = \\[50, 4096\\]"),
                      ({"shortlist": 4097}, "shortlist must be"), ({"shortlist": True}, "shortlist must be"),
                      ({"storage": "f32", "shortlist": 100}, "shortlist needs storage: i8"), ({"iters": 0}, "iters must be"),
                      ({"seed": -1}, "seed must be"), ({"probes": 3}, "unknown keys \\['probes'\\]")):
        with pytest.raises(ValueError, match="neighbours: ivf: " + word):
            _score(tmp_path, neighbours=_ivf(**sub), diffusion={})
    for missing in ("lists", "nprobe"):
        sub = {"lists": 16, "nprobe": 4}
        del sub[missing]
        with pytest.raises(ValueError, match="neighbours: ivf: %s is required" % missing):
            _score(tmp_path, neighbours={"ivf": sub}, diffusion={})
    with pytest.raises(ValueError, match="KNN_REVERSE_MAX_K.*k=129"):
        _score(tmp_path, neighbours=_ivf(), diffusion={"k": 129})
    with pytest.raises(ValueError, match="KNN_REVERSE_MAX_K.*k=200"):
        _score(tmp_path, neighbours=_ivf(storage="f32", reverse=False), database_augmentation={"k": 200, "alpha": 1.0}, diffusion={})
    for bad in ({}, {"ivf": 3}, {"ivf": None}, {"ivf": {}, "i8": {}}, {"pq": {"lists": 4, "nprobe": 2}}):
        with pytest.raises(ValueError, match="neighbours: 'exact' or 'i8'"):
            _score(tmp_path, neighbours=bad, diffusion={})
    with pytest.raises(ValueError, match="neighbours: ivf builds.*neither is on"):
        _score(tmp_path, neighbours=_ivf())
    with pytest.raises(ValueError, match="neighbours.*neither is on"):
        _score(tmp_path, neighbours=_ivf(), query_expansion={"k": 2, "alpha": 3.0})
    # what was refused before is refused as before
    for bad in ("f16", "int8", True, 8, None):
        with pytest.raises(ValueError, match="neighbours: 'exact' or 'i8'"):
            _score(tmp_path, neighbours=bad, diffusion={})
    assert _score(tmp_path, neighbours="i8", diffusion={"k": 64}).neighbours == "i8" and _score(tmp_path).neighbours == "exact"


def test_ivf_neighbours_overlay_parses(tmp_path):
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_diffusion_ivf_neighbours.yml")) as f:
        doc = yaml.safe_load(f)
    assert set(doc["validation"]) == {"roxford5k", "rparis6k", "247tokyo1k"}
    want = {"k": 50, "kq": 10, "gamma": 3.0, "alpha": 0.99, "iters": 20, "tol": 1e-6}
    for ds in doc["validation"]:
        crit = doc["validation"][ds]["criterion"]
        assert set(crit) == {"neighbours", "diffusion"} and crit["diffusion"] == want
        s = _score(tmp_path, **crit)
        assert s.diffusion == want
        assert s.neighbours == {"ivf": {"lists": 64, "nprobe": 8, "storage": "i8", "shortlist": 200, "reverse": True}}


def test_neighbour_index_builds_and_closes_the_inverted_file(monkeypatch):
    import torch
    from mdir_amd import ivf, score
    events = []

    class FakeIndex(ivf.IVFIndex):
        def __init__(self):
            self.lists = 16

        def close(self):
            events.append("closed")

    def train(rows, lists, storage="f32", **kw):
        events.append((tuple(rows.shape), lists, storage, kw))
        return FakeIndex()

    monkeypatch.setattr(ivf.IVFIndex, "train", staticmethod(train))
    vecs = torch.zeros((5, 4))
    with score._neighbour_index(vecs, {"ivf": {"lists": 16, "nprobe": 4, "storage": "i8", "shortlist": 200, "reverse": True, "seed": 7}}) as nix:
        assert isinstance(nix, ivf.IVFNeighbours) and (nix.nprobe, nix.shortlist, nix.reverse) == (4, 200, True)
        assert events == [((5, 4), 16, "i8", {"seed": 7})]
    assert events[-1] == "closed"
    with score._neighbour_index(vecs, "exact") as nix:
        assert nix is None
