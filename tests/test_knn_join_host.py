"""The exact kNN join (include/mdx.h, "exact kNN join"; mdir_amd/search.py knn_join) on a CPU-only box: the C ABI and its argument
checks, the Python checks of knn_join, of the ``index=`` keyword of DBA / DiffusionGraph and of the ``neighbours`` criterion key,
and a float64 restatement of the per-pair lower bound -- shown sound against the oracle's exact chain: l_ij <= chain_ij, the
threshold t_i is at most the exact k-th score, and the candidates at t_i hold every row that ties with or beats it."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_join_host import _sets, row_factors

NEW = ("mdx_knn_bounds_workspace", "mdx_knn_bounds", "mdx_join_candidates_rows", "mdx_knn_resolve_workspace", "mdx_knn_resolve")
MAX_K = 64


# ------------------------------------------------------------------ the lower bound, restated in float64

def score_and_beta(x, y):
    """(s, beta) [m, n] in float64: the MDX_I8 score (its fp32 value) and the pruning bound of include/mdx.h, +inf where a pair
    is not covered."""
    px, qx, rx, wx, cx = row_factors(x)
    py, qy, ry, wy, cy = row_factors(y)
    d = x.shape[1]
    acc = cx.astype(np.float64) @ cy.astype(np.float64).T
    prod = py[None, :].astype(np.float32) * px[:, None].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (acc.astype(np.float32) * prod).astype(np.float64)
        b1 = qx[:, None] * wy[None, :] + ry[None, :] * px[:, None].astype(np.float64) + d * 2.0 ** -149
        b2 = qy[None, :] * wx[:, None] + rx[:, None] * py[None, :].astype(np.float64) + d * 2.0 ** -149
        beta = np.minimum(b1, b2)
    under = (px[:, None] > 0) & (py[None, :] > 0) & (prod < np.float32(2.0 ** -126))
    return s, np.where(under, np.inf, beta)


def thresholds_np(x, y, k):
    """(t [m], l [m, n], candidates [m, n] bool) of the exact kNN join in float64: l = s - 2^-22 |s| - beta where the pair
    contributes (-inf elsewhere), t = the k-th largest l of a row (-inf below k contributions), candidates at tau_i = t_i."""
    s, beta = score_and_beta(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        l = s - 2.0 ** -22 * np.abs(s) - beta
        l = np.where(np.isfinite(beta) & ~np.isnan(s) & np.isfinite(l), l, -np.inf)
        t = -np.sort(-l, axis=1)[:, k - 1]
        lhs = s + 2.0 ** -22 * np.abs(s) + beta
        cand = ~(lhs < t[:, None])
    return t, l, cand


def planted_groups(rng, n, d, group, noise):
    """Unit gaussian rows; every ``group`` of them (a random partition) is a first row and copies of it moved by ``noise`` times
    a unit gaussian direction, normalised."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30).astype(np.float32)
    group = max(1, min(group, n))
    members = rng.permutation(n)[:n // group * group].reshape(-1, group)
    for g in members:
        for j in g[1:]:
            u = rng.standard_normal(d).astype(np.float32)
            v = x[g[0]] + np.float32(noise) * (u / np.linalg.norm(u)).astype(np.float32)
            x[j] = v / np.linalg.norm(v)
    return x.astype(np.float32)


def rank_order(scores):
    """Per row, the ids in mdx_rank_full's order: larger first, -0 == +0, NaN last, ties by ascending id."""
    from test_gpu_join import desc_key
    key = desc_key(scores)
    return np.stack([np.lexsort((np.arange(scores.shape[1]), key[i])) for i in range(scores.shape[0])])


def test_restated_lower_bound_is_sound():
    from oracle import chain
    rng = np.random.default_rng(23)
    contributing, pruned, pairs = 0, 0, 0
    for trial in range(150):
        kind = ("random", "clustered", "adversarial")[trial % 3]
        n = int(rng.integers(2, 60))
        d = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 130]))
        x = _sets(rng, kind, n, d)
        exact = chain.gemm_nt_chain(x, x)
        order = rank_order(exact)
        for k in sorted({1, min(7, n), n}):
            t, l, cand = thresholds_np(x, x, k)
            fin = np.isfinite(l)
            assert (l[fin] <= exact[fin].astype(np.float64)).all(), (trial, kind, d)            # l_ij <= chain_ij
            for i in range(n):
                kth = exact[i, order[i, k - 1]]
                if not np.isnan(kth):
                    assert t[i] <= kth, (trial, i, k)                                            # t_i <= e_i
                    tie_or_beat = exact[i] >= kth
                    assert cand[i, tie_or_beat].all(), (trial, i, k)
                assert cand[i, order[i, :k]].all() and cand[i].sum() >= k                        # the exact top-k are candidates
            contributing += int(fin.sum())
            pruned += int((~cand).sum())
            pairs += cand.size
    assert contributing > pairs // 2 and pruned > 0, (contributing, pruned, pairs)


def test_restated_threshold_for_rows_outside_the_bound():
    x = np.eye(6, 8, dtype=np.float32)
    x[1, 2] = np.inf
    x[2, 3] = np.nan
    t, l, cand = thresholds_np(x, x, 2)
    assert np.isinf(l[1]).all() and np.isinf(l[2]).all() and (t[[1, 2]] == -np.inf).all()       # no pair of an uncovered row contributes
    assert cand[1].all() and cand[2].all()                                                      # t = -inf: every row a candidate
    assert np.isfinite(t[[0, 3, 4, 5]]).all()
    assert cand[:, 1].all() and cand[:, 2].all()                                                # uncovered rows are candidates of every row
    t, _, cand = thresholds_np(x, x, 5)                                                         # only 4 covered rows: fewer than k contribute
    assert (t == -np.inf).all() and cand.all()


def test_restated_bound_prunes_planted_rows():
    """The pruning figures that the device test asserts against: groups of 16 at noise 0.5, n = 4096, d = 256, k = 10."""
    rng = np.random.default_rng(4096)
    n, k = 4096, 10
    x = planted_groups(rng, n, 256, 16, 0.5)
    _, _, cand = thresholds_np(x, x, k)
    per_row = cand.sum(axis=1)
    assert (per_row >= k).all() and cand.sum() <= 4 * k * n, cand.sum() / n
    assert abs(cand.sum() / n - 16.0) < 0.5, cand.sum() / n


# ------------------------------------------------------------------ C ABI

def _declared():
    """The code of include/mdx_knn_join.h, the prototypes that mdx.h includes for its section "exact kNN join"."""
    assert re.search(r'^#include "mdx_knn_join.h"$', open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.M)
    text = open(os.path.join(ROOT, "include", "mdx_knn_join.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_knn_join_entry_points():
    from mdir_amd import _lib, ops
    code = _declared()
    assert re.search(r"#define MDX_KNN_JOIN_MAX_K (\d+)\b", code)
    assert int(re.search(r"#define MDX_KNN_JOIN_MAX_K (\d+)\b", code).group(1)) == ops.KNN_JOIN_MAX_K >= 64
    assert re.search(r"int\s+mdx_join_candidates_rows\s*\(\s*const mdx_index \*a,\s*const float \*stats_a,\s*const mdx_index \*b,"
                     r"\s*const float \*stats_b,\s*int64_t a_lo,\s*int64_t a_hi,\s*const float \*tau,\s*uint64_t \*pairs,"
                     r"\s*int64_t capacity,\s*int64_t \*count,\s*void \*stream\s*\)", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.KNN_JOIN_EXPORTS
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert "exact kNN join" in text and "l_ij = fl(fl(s - h) - b)" in text


def test_every_knn_join_entry_point_is_covered():
    """The census of include/mdx_knn_join.h, which tests/test_memguard_host.py does not see: every prototype is exported and
    bound, and is a size function or has at least two memory-contract cases, one of them the stale pre-fill of the others."""
    from mdir_amd import _lib
    from test_gpu_knn_join_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.KNN_JOIN_EXPORTS) == set(NEW) and not declared & set(_lib.EXPORTS)
    sizes = {n for n in declared if "_workspace" in n}
    assert {"mdx_" + entry for entry in COVERED} == declared - sizes and len(sizes) == 2
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_library_exports_the_knn_join_entry_points():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name)


def test_workspace_sizes():
    from mdir_amd import _lib
    h = _lib.lib()
    w = h.mdx_knn_bounds_workspace
    assert w(0, 5, 100, 0) == 0 and w(100, 0, 100, 0) == 0 and w(100, 5, 0, 0) == 0
    assert w(100, MAX_K + 1, 1000, 0) == 0 and w(100, 11, 10, 0) == 0                  # k > MAX_K, k > nb
    assert w(100, 5, 1000, -1) == 0 and w(100, 5, 1000, 65) == 0 and w(1 << 31, 5, 1000, 0) == 0
    assert w(100, 5, 1000, 1) == 2048                                                   # [1, 100, 5] fp32, rounded up to 256
    assert w(100, 5, 1000, 3) == 6144 and w(100, 5, 1000, 64) == 16128                  # never more slices than blocks of B (8)
    assert w(100, 5, 1000, 0) == 16128 and w(1 << 20, 64, 1 << 20, 0) == (1 << 20) * 64 * 4
    r = h.mdx_knn_resolve_workspace
    assert r(0, 5) == 0 and r(5, 0) == 0 and r(1 << 31, 5) == 0
    assert r(1000, 10) > h.mdx_join_resolve_workspace(1000, 10)                         # the offsets on top
    assert r(1000, 10) < r(100000, 10)


def test_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    big = 1 << 40

    def bounds(a=p, sa=p, b=p, sb=p, lo=0, hi=128, k=5, slices=0, t=p, ws=p, wsb=big):
        return h.mdx_knn_bounds(a, sa, b, sb, lo, hi, k, slices, t, ws, wsb, None)
    for kw in ({"a": None}, {"sa": None}, {"b": None}, {"sb": None}, {"t": None}):
        assert bounds(**kw) == -1 and b"NULL" in h.mdx_last_error()
    # the scalar arguments are checked before anything of the handles is read (these are not indexes)
    for k in (0, -1, MAX_K + 1):
        assert bounds(k=k) == -1 and b"MDX_KNN_JOIN_MAX_K" in h.mdx_last_error()
    for s in (-1, 65):
        assert bounds(slices=s) == -1 and b"slices" in h.mdx_last_error()
    assert bounds(sa=ctypes.c_void_p(264)) == -1 and b"16-byte" in h.mdx_last_error()

    def cand(a=p, sa=p, b=p, sb=p, lo=0, hi=128, tau=p, pairs=p, cap=10, count=p):
        return h.mdx_join_candidates_rows(a, sa, b, sb, lo, hi, tau, pairs, cap, count, None)
    for kw in ({"a": None}, {"sa": None}, {"b": None}, {"sb": None}, {"tau": None}, {"pairs": None}, {"count": None}):
        assert cand(**kw) == -1 and b"NULL" in h.mdx_last_error()
    assert cand(cap=-1) == -1 and b"capacity" in h.mdx_last_error()
    assert cand(sb=ctypes.c_void_p(264)) == -1 and b"16-byte" in h.mdx_last_error()

    def resolve(ra=p, lda=8, rb=p, ldb=8, d=8, pairs=p, P=10, m_lo=0, m=4, k=2, ids=p, sc=p, cnt=p, ws=p, wsb=big):
        return h.mdx_knn_resolve(ra, lda, rb, ldb, d, pairs, P, m_lo, m, k, ids, sc, cnt, ws, wsb, None)
    for kw in ({"ra": None}, {"rb": None}, {"pairs": None}, {"ids": None}, {"sc": None}, {"cnt": None}):
        assert resolve(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"P": 0}, {"m": 0}, {"d": 0}, {"P": -5}):
        assert resolve(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert resolve(P=1 << 31) == -1 and b"2^31" in h.mdx_last_error()
    for k in (0, MAX_K + 1):
        assert resolve(k=k) == -1 and b"MDX_KNN_JOIN_MAX_K" in h.mdx_last_error()
    assert resolve(ldb=4) == -1 and b"ldb" in h.mdx_last_error()
    assert resolve(m_lo=-1) == -1 and b"m_lo" in h.mdx_last_error()
    assert resolve(ws=None) == -4 and resolve(wsb=16) == -4
    assert resolve(ws=ctypes.c_void_p(264)) == -1 and b"aligned" in h.mdx_last_error()


# ------------------------------------------------------------------ the Python checks

class _FakeIndex:
    storage = "f16"
    n, d = 4, 8
    _h = None


def _fake_index(storage="i8", n=4, d=8):
    from mdir_amd import ops
    fake = ops.DescriptorIndex.__new__(ops.DescriptorIndex)
    fake.storage, fake.n, fake.d, fake._h = storage, n, d, None
    return fake


def test_knn_join_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops, search
    assert ops.KNN_JOIN_MAX_K == MAX_K and search.KnnResult._fields == ("ids", "scores", "pruned_rows")
    cpu = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="fp32 device tensor"):
        search.knn_join(None, cpu, 2)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rows = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="int8 DescriptorIndex"):
        search.knn_join(object(), rows, 2)
    with pytest.raises(ValueError, match="int8 index"):
        search.knn_join(_fake_index("f16"), rows, 2)
    with pytest.raises(ValueError, match=r"index's \[5, 8\] rows"):
        search.knn_join(_fake_index(n=5), rows, 2)
    for k in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="k must be"):
            search.knn_join(_fake_index(), rows, k)
        with pytest.raises(ValueError, match="k must be"):
            search.knn_join(None, rows, k)
    for chunk in (0, 1.5, True):
        with pytest.raises(ValueError, match="chunk"):
            search.knn_join(_fake_index(), rows, 2, chunk=chunk)
    wide = torch.zeros((100, 8))
    with pytest.raises(ValueError, match="KNN_JOIN_MAX_K = 64"):                         # the limit is named; k is clamped to N first
        search.knn_join(_fake_index(n=100), wide, 65)


def test_ops_checks_need_no_gpu():
    import torch
    from mdir_amd import ops
    cpu = torch.zeros((4, 4))
    for fn in (lambda a, b: ops.knn_bounds(a, cpu, b, cpu, 0, 4, 2), lambda a, b: ops.join_candidates_rows(a, cpu, b, cpu, cpu)):
        with pytest.raises(ValueError, match="open DescriptorIndex"):
            fn(_FakeIndex(), _FakeIndex())
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.knn_resolve(cpu, cpu, cpu, 0, 4, 2)


def test_rerank_index_keyword(monkeypatch):
    """``index=`` of DBA and DiffusionGraph: refused unless it is an int8 DescriptorIndex; an accepted one reaches knn_join."""
    import torch
    from mdir_amd import rerank, search
    rows = torch.zeros((4, 8))
    for bad in (object(), _fake_index("f16"), _fake_index("f32")):
        with pytest.raises(ValueError, match="int8 DescriptorIndex"):
            rerank.database_augmentation(rows, 2, 3.0, index=bad)
        with pytest.raises(ValueError, match="int8 DescriptorIndex"):
            rerank.DiffusionGraph(rows, k=2, index=bad)
    seen = []

    class Stop(Exception):
        pass

    def fake_join(index, vecs, k, chunk=None):
        seen.append((index, tuple(vecs.shape), k, chunk))
        raise Stop

    monkeypatch.setattr(search, "knn_join", fake_join)
    ix = _fake_index()
    with pytest.raises(Stop):
        rerank.database_augmentation(rows, 10, 3.0, index=ix)
    with pytest.raises(Stop):
        rerank.DiffusionGraph(rows, k=3, chunk=2, index=ix)
    with pytest.raises(Stop):
        rerank.DiffusionGraph(rows, k=3)
    assert seen == [(ix, (4, 8), 4, None), (ix, (4, 8), 3, 2), (None, (4, 8), 3, None)]


# ------------------------------------------------------------------ the criterion key

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


def test_neighbours_key(tmp_path):
    assert _score(tmp_path).neighbours == "exact"
    assert _score(tmp_path, diffusion={}).neighbours == "exact"
    assert _score(tmp_path, neighbours="exact").neighbours == "exact"
    assert _score(tmp_path, neighbours="i8", diffusion={"k": 64}).neighbours == "i8"
    assert _score(tmp_path, neighbours="i8", database_augmentation={"k": 10, "alpha": 3.0}).neighbours == "i8"
    for bad in ("f16", "int8", True, 8, None):
        with pytest.raises(ValueError, match="neighbours: 'exact' or 'i8'"):
            _score(tmp_path, neighbours=bad, diffusion={})
    with pytest.raises(ValueError, match="neighbours.*neither is on"):
        _score(tmp_path, neighbours="i8")
    with pytest.raises(ValueError, match="neighbours.*neither is on"):
        _score(tmp_path, neighbours="i8", query_expansion={"k": 2, "alpha": 3.0})
    with pytest.raises(ValueError, match="KNN_JOIN_MAX_K.*diffusion has k=65"):
        _score(tmp_path, neighbours="i8", diffusion={"k": 65})
    with pytest.raises(ValueError, match="KNN_JOIN_MAX_K.*database_augmentation has k=100"):
        _score(tmp_path, neighbours="i8", database_augmentation={"k": 100, "alpha": 1.0})


def test_i8_neighbours_overlay_parses(tmp_path):
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_diffusion_i8_neighbours.yml")) as f:
        doc = yaml.safe_load(f)
    assert set(doc["validation"]) == {"roxford5k", "rparis6k", "247tokyo1k"}
    want = {"k": 50, "kq": 10, "gamma": 3.0, "alpha": 0.99, "iters": 20, "tol": 1e-6}
    for ds in doc["validation"]:
        crit = doc["validation"][ds]["criterion"]
        assert set(crit) == {"neighbours", "diffusion"} and crit["neighbours"] == "i8" and crit["diffusion"] == want
        s = _score(tmp_path, **crit)
        assert s.neighbours == "i8" and s.diffusion == want
