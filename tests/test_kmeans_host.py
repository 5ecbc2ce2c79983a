"""Spherical k-means (include/mdx_kmeans.h; mdir_amd/cluster.py) on a CPU-only box: the census of include/mdx_kmeans.h, the
restatement (tests/kmeans_restatement.py) checked against exact integer sums on lattice data, every refusal of the C ABI with nothing
launched, the Python checks of the ops wrappers and of cluster.assign / cluster.kmeans, and the float64 loop on planted data."""
import ctypes
import os
import re

import numpy as np
import pytest

import kmeans_restatement as KR
from conftest import ROOT

NEW = ("mdx_kmeans_argmax", "mdx_kmeans_sums_workspace", "mdx_kmeans_sums", "mdx_kmeans_finish")
F32 = np.float32


def _declared():
    """The code of include/mdx_kmeans.h, which mdx.h includes for its section "spherical k-means"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_kmeans.h"$', text, flags=re.M) and "spherical k-means" in text
    assert text.index('#include "mdx_train.h"') < text.index('#include "mdx_kmeans.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_kmeans.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib, ops
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.KMEANS_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS))
    assert not declared & others
    assert re.search(r"int\s+mdx_kmeans_argmax\s*\(\s*const float \*scores,\s*int64_t m,\s*int64_t K,\s*int64_t ld,\s*int64_t \*labels,"
                     r"\s*float \*best,\s*void \*stream\s*\)", code)
    assert re.search(r"int64_t\s+mdx_kmeans_sums_workspace\s*\(\s*int64_t n,\s*int64_t K,\s*int64_t d\s*\)", code)
    assert re.search(r"int\s+mdx_kmeans_finish\s*\(\s*const float \*sums,\s*int64_t K,\s*int64_t d,\s*float eps,\s*const float \*previous,"
                     r"\s*float \*centroids,\s*void \*stream\s*\)", code)
    segment = int(re.search(r"#define MDX_KMEANS_SEGMENT (\d+)", code).group(1))
    assert segment == ops.KMEANS_SEGMENT == KR.SEGMENT
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert "mdx_kmeans.hip" in makefile and "include/mdx_kmeans.h" in makefile
    assert '"mdx_kmeans.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "kmeans" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_kmeans_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == {n for n in NEW if not n.endswith("_workspace")}
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_workspace_formula():
    from mdir_amd import _lib
    h = _lib.lib()
    for n, k, d in ((1, 1, 1), (255, 1, 3), (256, 2, 4), (257, 7, 5), (1000, 70, 36), (1004993, 4096, 2048)):
        want = (8 * (k + 1) + 255) // 256 * 256 + (4 * (-(-n // KR.SEGMENT) + k) * (-(-d // 4) * 4) + 255) // 256 * 256
        assert h.mdx_kmeans_sums_workspace(n, k, d) == want, (n, k, d)
    for n, k, d in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 31), (1 << 30, 1, 1 << 20)):
        assert h.mdx_kmeans_sums_workspace(n, k, d) == 0, (n, k, d)


# ------------------------------------------------------------------------------------------------ the restatement itself

def _lattice_rows(rng, n, d, amp=15):
    """Integer rows, |x| <= amp, about a third zeros and a quarter of those -0: any sum of up to 2^24 / amp of them is exact in
    fp32 in any order (the idea of tests/lattice.py)."""
    ints = rng.integers(-amp, amp + 1, size=(n, d), dtype=np.int64)
    ints[rng.random((n, d)) < 0.3] = 0
    rows = ints.astype(F32)
    rows[(rows == 0) & (rng.random((n, d)) < 0.25)] = F32(-0.0)
    return ints, rows


def test_segment_chain_equals_the_integer_sums_on_lattice_data():
    rng = np.random.default_rng(11)
    n, d, k = 1500, 7, 6
    ints, rows = _lattice_rows(rng, n, d)
    assert n * 15 < 1 << 24
    sizes = [0, 1, KR.SEGMENT - 1, KR.SEGMENT, KR.SEGMENT + 1, 2 * KR.SEGMENT + 3]
    labels = np.full(n, -1, np.int64)
    labels[rng.permutation(n)[:sum(sizes)]] = np.repeat(np.arange(k), sizes)
    members = np.concatenate([np.flatnonzero(labels == c) for c in range(k)])
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    got = KR.sums32(rows, members, offsets, k)
    want = np.stack([ints[labels == c].sum(axis=0) for c in range(k)]).astype(F32)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))     # +0 wherever the sum is 0
    # any segment length gives the same integers; ids outside [0, n) are skipped; offsets are clamped
    assert np.array_equal(KR.sums32(rows, members, offsets, k, segment=5), want)
    spoiled = np.concatenate([members[:3], [-1, n], members[3:]])
    off2 = offsets + 2
    off2[0] = -7
    assert np.array_equal(KR.sums32(rows, spoiled, off2, k), np.stack([ints[spoiled[max(a, 0):b][(spoiled[max(a, 0):b] >= 0) & (spoiled[max(a, 0):b] < n)]].sum(axis=0)
                                                                       for a, b in zip(off2[:-1], off2[1:])]).astype(F32))
    m2, o2 = KR.csr(np.where(labels < 0, 0, labels), k)
    assert np.array_equal(o2, np.concatenate([[0], np.cumsum(np.bincount(np.where(labels < 0, 0, labels), minlength=k))]))
    assert all(np.all(np.diff(m2[a:b]) > 0) for a, b in zip(o2[:-1], o2[1:]))


def test_argmax_restatement_has_the_ranking_tie_rule():
    nan, inf = F32(np.nan), F32(np.inf)
    block = np.array([[1, 3, 3, 2], [-0.0, 0.0, -1, -2], [0.0, -0.0, -1, -2], [nan, -inf, -inf, nan], [nan, nan, nan, nan],
                      [5, 5, 5, 5], [-inf, nan, 7, 7]], F32)
    labels, best = KR.argmax_first(block)
    assert labels.tolist() == [1, 0, 0, 1, 0, 0, 2]
    assert np.signbit(best[1]) and not np.signbit(best[2]) and best[3] == -inf and np.isnan(best[4]) and best[6] == 7
    from oracle import chain as OC
    rng = np.random.default_rng(3)
    scores = rng.integers(-3, 4, size=(9, 50)).astype(F32)
    scores[rng.random(scores.shape) < 0.1] = nan
    assert np.array_equal(KR.argmax_first(scores)[0], OC.rank_full(scores)[:, 0])      # the first entry of the oracle's full ranking
    special = np.array([0.0, -0.0, 1.0, -1.0, inf, -inf, nan, 1e-45, -1e-45, 3.4e38, -3.4e38], F32)
    assert KR.order_key(special).tolist() == [OC.desc_key(v) for v in special]


def test_finish_restatement():
    s = np.array([[3.0, 4.0], [0.0, -0.0], [1e-30, 0.0]])
    prev = np.array([[9.0, 9.0], [0.6, 0.8], [7.0, 7.0]])
    out = KR.finish64(s, 1e-6, prev)
    assert np.allclose(out[0], [3 / (5 + 1e-6), 4 / (5 + 1e-6)], rtol=1e-15) and np.array_equal(out[1], prev[1])
    assert np.allclose(out[2], [1e-30 / (1e-30 + 1e-6), 0.0])                # tiny is not zero: it is normalised, not replaced
    assert np.array_equal(KR.finish64(s, 1e-6)[1], [0.0, 0.0])


# ------------------------------------------------------------------------------------------------ the loop on planted data

N, D, K = 600, 32, 6


def test_loop_recovers_the_planted_partition():
    rows, truth = KR.planted(N, D, K, seed=5)
    assert rows.shape == (N, D) and rows.dtype == F32
    init_a, init_b = KR.planted_inits(truth, K)
    a = KR.kmeans64(rows, K, init_a)
    assert KR.pure(a.labels, truth, K) and a.reseeded == 0 and a.sizes.tolist() == [N // K] * K
    assert [truth[i] for i in init_a] == list(range(K)) and np.array_equal(a.labels, truth)   # cluster c grew from planted cluster c
    assert len(a.history) == a.iterations + 1 and a.history[-1] >= a.history[0]
    b = KR.kmeans64(rows, K, init_b)
    first, _, _ = KR.assign64(rows[init_b].astype(np.float64), rows)
    assert not (first == 5).any()                                            # two identical centroids: the smaller id takes every tie
    assert b.reseeded == 1 and KR.pure(b.labels, truth, K) and b.sizes.tolist() == [N // K] * K
    assert len(b.history) == b.iterations + 1
    # the oracle is only an oracle where fp32 rounding cannot change a label: the gap between a row's two best final scores
    for fit in (a, b):
        scores = np.sort(KR.assign64(fit.centroids, rows)[2], axis=1)
        assert float((scores[:, -1] - scores[:, -2]).min()) > 0.1
    print("assignments: (a) %d, (b) %d" % (len(a.history), len(b.history)))


def test_loop_stops_on_iters_and_tol():
    rows, truth = KR.planted(N, D, K, seed=5)
    init_a, _ = KR.planted_inits(truth, K)
    assert KR.kmeans64(rows, K, init_a, iters=0).iterations == 0
    assert KR.kmeans64(rows, K, init_a, iters=1).iterations == 1
    assert KR.kmeans64(rows, K, init_a, tol=1.0).iterations == 0
    half = np.sort(np.random.default_rng(0).permutation(N)[:300])
    fit = KR.kmeans64(rows, K, init_a, train_ids=half)
    assert fit.labels.shape == (N,) and KR.pure(fit.labels, truth, K)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID / MDX_ERR_WORKSPACE of the section through the C ABI with pointers that are no memory: nothing is
    launched (there is no device here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    p, q, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 22), ctypes.c_void_p(1 << 24)

    def refused(status, name, *words, code=-1):
        msg = h.mdx_last_error()
        assert status == code and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)

    def argmax(scores=p, m=3, k=5, ld=5, labels=q, best=q):
        return h.mdx_kmeans_argmax(scores, m, k, ld, labels, best, None)
    name = "mdx_kmeans_argmax"
    refused(argmax(scores=None), name, "NULL")
    refused(argmax(labels=None, best=None), name, "NULL")
    for kw in ({"m": 0}, {"k": 0, "ld": 0}, {"m": -1}, {"m": 1 << 31}, {"k": 1 << 31, "ld": 1 << 31}):
        refused(argmax(**kw), name, "must be in [1, 2^31)")
    refused(argmax(ld=4), name, "ld=4 < K=5")
    refused(argmax(m=1 << 30, k=1 << 30, ld=1 << 40), name, "overflows")

    def sums(rows=p, n=10, d=8, ld=8, members=q, offsets=q, k=3, out=q, wsp=ws, wsb=None):
        return h.mdx_kmeans_sums(rows, n, d, ld, members, offsets, k, out, wsp, h.mdx_kmeans_sums_workspace(n, k, d) if wsb is None else wsb, None)
    name = "mdx_kmeans_sums"
    for kw in ({"rows": None}, {"members": None}, {"offsets": None}, {"out": None}):
        refused(sums(**kw), name, "NULL")
    for kw in ({"n": 0}, {"d": 0, "ld": 0}, {"k": 0}, {"k": -2}):
        refused(sums(**kw), name, ">= 1")
    for kw in ({"n": 1 << 31}, {"k": 1 << 31}, {"d": 1 << 31, "ld": 1 << 31}, {"n": 1 << 30, "d": 1 << 20, "ld": 1 << 20}):
        refused(sums(**kw), name, "too large")
    refused(sums(ld=7), name, "ld=7 < d=8")
    need = h.mdx_kmeans_sums_workspace(10, 3, 8)
    assert need == 256 + 256
    refused(sums(wsb=need - 1), name, "workspace", code=-4)
    refused(sums(wsp=None), name, "workspace", code=-4)
    for off in (4, 8):
        refused(sums(wsp=ctypes.c_void_p((1 << 24) + off)), name, "16-byte aligned")

    def finish(s=p, k=3, d=8, eps=1e-6, prev=None, out=q):
        return h.mdx_kmeans_finish(s, k, d, eps, prev, out, None)
    name = "mdx_kmeans_finish"
    for kw in ({"s": None}, {"out": None}):
        refused(finish(**kw), name, "NULL")
    for kw in ({"k": 0}, {"d": 0}, {"k": 1 << 31}, {"d": -1}):
        refused(finish(**kw), name, "must be in [1, 2^31)")
    for eps in (-1e-6, float("nan")):
        refused(finish(eps=eps), name, "eps=")


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    block = torch.zeros((3, 5))
    i64 = torch.zeros(4, dtype=torch.int64)
    for call, word in ((lambda: ops.kmeans_argmax(block), "scores"), (lambda: ops.kmeans_sums(block, i64, i64, 3), "rows"),
                       (lambda: ops.kmeans_finish(block), "sums"), (lambda: ops.kmeans_argmax(None), "scores")):
        with pytest.raises(ValueError, match="%s must be a CUDA" % word):
            call()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    # kmeans_argmax
    with pytest.raises(ValueError, match="scores must be torch.float32"):
        ops.kmeans_argmax(block.double())
    with pytest.raises(ValueError, match="scores must be a non-empty 2-d"):
        ops.kmeans_argmax(block[0])
    with pytest.raises(ValueError, match="scores must be a non-empty 2-d"):
        ops.kmeans_argmax(block[:0])
    with pytest.raises(ValueError, match="scores must be a matrix with contiguous rows"):
        ops.kmeans_argmax(torch.zeros((5, 3)).t())
    with pytest.raises(ValueError, match="out_labels must be torch.int64"):
        ops.kmeans_argmax(block, out_labels=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"out_best must be a contiguous \[3\]"):
        ops.kmeans_argmax(block, out_best=torch.zeros(4))
    with pytest.raises(ValueError, match=r"out_labels must be a contiguous \[3\]"):
        ops.kmeans_argmax(block, out_labels=torch.zeros(6, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="both False"):
        ops.kmeans_argmax(block, out_labels=False, out_best=False)
    # kmeans_sums
    for k in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer >= 1"):
            ops.kmeans_sums(block, i64[:3], i64, k)
    with pytest.raises(ValueError, match="members must be torch.int64"):
        ops.kmeans_sums(block, i64[:3].int(), i64, 3)
    with pytest.raises(ValueError, match="members must be a contiguous tensor of at most n = 3 ids"):
        ops.kmeans_sums(block, i64, i64, 3)
    with pytest.raises(ValueError, match="offsets must be torch.int64"):
        ops.kmeans_sums(block, i64[:3], i64.float(), 3)
    with pytest.raises(ValueError, match=r"offsets must be a contiguous \[k \+ 1\] = \[3\]"):
        ops.kmeans_sums(block, i64[:3], i64, 2)
    with pytest.raises(ValueError, match="rows must be torch.float32"):
        ops.kmeans_sums(block.half(), i64[:3], i64, 3)
    # kmeans_finish
    with pytest.raises(ValueError, match="sums must be contiguous"):
        ops.kmeans_finish(torch.zeros((3, 8))[:, :5])
    for eps in (-1e-6, float("nan"), float("inf"), "1e-6", True):
        with pytest.raises(ValueError, match="eps must be a finite number >= 0"):
            ops.kmeans_finish(block, eps)
    with pytest.raises(ValueError, match=r"previous must be \[3,5\]"):
        ops.kmeans_finish(block, previous=torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="previous must be torch.float32"):
        ops.kmeans_finish(block, previous=block.double())


def test_cluster_refusals_need_no_gpu():
    import torch
    from mdir_amd import cluster
    rows, cents = torch.zeros((10, 4)), torch.zeros((3, 4))
    assert cluster.KMeans._fields == ("centroids", "labels", "sizes", "history", "iterations", "reseeded")
    for doc_word in ("randperm", "stable sort", "kmeans_sums", "kmeans_finish", "ops.topk(-best, E)", "keep their", "final ``assign`` of ALL rows",
                     "train_rows=M", "<= tol"):
        assert doc_word in cluster.__doc__, doc_word
    # assign
    for call, word in ((lambda: cluster.assign(cents, rows.double()), "rows must be a non-empty fp32"),
                       (lambda: cluster.assign(cents[0], rows), "centroids must be a non-empty fp32"),
                       (lambda: cluster.assign(cents[:0], rows), "centroids must be a non-empty fp32"),
                       (lambda: cluster.assign(cents, torch.zeros((10, 8))[:, :4]), "rows must be contiguous"),
                       (lambda: cluster.assign(torch.zeros((3, 5)), rows), "dimensions differ"),
                       (lambda: cluster.assign(cents, rows, chunk=0), "chunk must be an integer >= 1"),
                       (lambda: cluster.assign(cents, rows, chunk=2.5), "chunk must be an integer >= 1"),
                       (lambda: cluster.assign(cents, rows, compute="fp16"), "compute 'fp16'"),
                       (lambda: cluster.assign(cents, rows), "centroids must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            call()
    # kmeans
    for kw, word in (({"k": 11}, "k = 11 > N = 10 rows"), ({"k": 0}, "k must be an integer >= 1"), ({"k": 2.0}, "k must be an integer"),
                     ({"k": 4, "train_rows": 3}, "k = 4 > train_rows = 3"), ({"k": 3, "train_rows": 11}, "train_rows = 11 > N = 10"),
                     ({"k": 3, "train_rows": 0}, "train_rows must be an integer >= 1"), ({"k": 3, "iters": -1}, "iters must be an integer >= 0"),
                     ({"k": 3, "seed": -1}, "seed must be an integer >= 0"), ({"k": 3, "tol": -0.1}, "tol must be a share"),
                     ({"k": 3, "tol": 1.5}, "tol must be a share"), ({"k": 3, "tol": None}, "tol must be a share"),
                     ({"k": 3, "chunk": 0}, "chunk must be an integer >= 1"), ({"k": 3, "compute": "int8"}, "compute 'int8'"),
                     ({"k": 3, "init": "kmeans++"}, "init 'kmeans\\+\\+'"), ({"k": 3}, "rows must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            cluster.kmeans(rows, **kw)
    with pytest.raises(ValueError, match="rows must be a non-empty fp32"):
        cluster.kmeans(rows.half(), 3)
    with pytest.raises(ValueError, match="rows must be a non-empty fp32"):
        cluster.kmeans(rows[0], 3)
    # the initial centroids, on the host (the function moves nothing to a device the rows are not on)
    gen = torch.Generator().manual_seed(0)
    for init, word in (([0, 1], "2 ids for k = 3"), ([0, 1, 10], "each in \\[0, 10\\)"), ([0, -1, 2], "each in \\[0, 10\\)"),
                       (torch.zeros((3, 5)), "init must be \\[3,4\\]"), (torch.zeros((3, 4), dtype=torch.float64), "init must be a non-empty fp32"),
                       (7, "a sequence of k row ids"), ("first", "init 'first'")):
        with pytest.raises(ValueError, match=word):
            cluster._initial(rows, rows, 3, init, gen)
    marked = torch.arange(40, dtype=torch.float32).reshape(10, 4)
    assert torch.equal(cluster._initial(marked, marked, 3, [4, 0, 9], gen), marked[[4, 0, 9]])
    assert torch.equal(cluster._initial(marked, marked, 3, torch.tensor([2, 2, 1]), gen), marked[[2, 2, 1]])
    given = cluster._initial(marked, marked, 3, marked[:3], gen)
    assert torch.equal(given, marked[:3]) and given.data_ptr() != marked.data_ptr()
    a = cluster._initial(marked, marked, 3, "sample", torch.Generator().manual_seed(4))
    want = torch.randperm(10, generator=torch.Generator().manual_seed(4))[:3]
    assert torch.equal(a, marked[want]) and len(set(want.tolist())) == 3
    # the default chunk keeps a step of assign under the cap
    for n, k, d in ((1004993, 256, 2048), (1004993, 4096, 2048), (1000, 70, 36), (5, 3, 1)):
        chunk = cluster.assign_chunk(n, k, d)
        assert 1 <= chunk <= n and (chunk == n or cluster._assign_bytes(chunk + 1, k, d, 0) > cluster.ASSIGN_MEMORY_CAP >= cluster._assign_bytes(chunk, k, d, 0))
    assert cluster.assign_chunk(100, 3, 4, cap=1) == 1
