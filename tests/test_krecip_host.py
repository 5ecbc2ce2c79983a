"""k-reciprocal re-ranking (include/mdx_krecip.h; mdir_amd/rerank.py ReciprocalEncoding / k_reciprocal) on a CPU-only box: the census
of include/mdx_krecip.h, every refusal of the C ABI with nothing launched and the call's name in the error, the workspace formula,
the `k_reciprocal:` criterion key with its exclusions, and the Python checks of rerank and of the ops wrappers."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ("mdx_krecip_sets", "mdx_krecip_raw_offsets", "mdx_krecip_raw_fill", "mdx_krecip_expand_offsets", "mdx_krecip_expand_fill",
       "mdx_krecip_rerank_workspace", "mdx_krecip_rerank")
MAX_K1, MAX_NNZ, MAX_R = 64, 4096, 4096


def _declared():
    """The code of include/mdx_krecip.h, which mdx.h includes for its section "k-reciprocal re-ranking"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_krecip.h"$', text, flags=re.M) and "k-reciprocal re-ranking" in text
    assert text.index('#include "mdx_groups.h"') < text.index('#include "mdx_krecip.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_krecip.h")).read(), flags=re.S)


def test_header_declares_the_krecip_entry_points():
    from mdir_amd import _lib, ops
    code = _declared()
    for name, value, mine in (("MAX_K1", MAX_K1, ops.KRECIP_MAX_K1), ("MAX_NNZ", MAX_NNZ, ops.KRECIP_MAX_NNZ), ("MAX_R", MAX_R, ops.KRECIP_MAX_R)):
        assert int(re.search(r"#define MDX_KRECIP_%s (\d+)\b" % name, code).group(1)) == value == mine
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.KRECIP_EXPORTS
    assert re.search(r"int\s+mdx_krecip_sets\s*\(\s*const int64_t \*ids,\s*int64_t n,\s*int64_t k,\s*int32_t \*rk,\s*int32_t \*rk_counts,"
                     r"\s*int32_t \*rh,\s*int32_t \*rh_counts,\s*void \*stream\s*\)", code)
    assert re.search(r"int64_t\s+mdx_krecip_rerank_workspace\s*\(\s*int64_t nq,\s*int64_t r\s*\)", code)
    text = open(os.path.join(ROOT, "include", "mdx_krecip.h")).read()
    for phrase in ("R(i, w) = { j in L_i^w : i in L_j^w }", "3 |R(i, k) & R(c, h)| >= 2 |R(c, h)|", "expf(fmaf(2, s_ij, -2))",
                   "NOT rebuilt with the query", "GATHERED", "RECOMPUTED", "no float atomics", "legal under capture"):
        assert phrase in text, phrase
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert "mdx_krecip.hip" in makefile and "include/mdx_krecip.h" in makefile


def test_every_krecip_entry_point_is_covered():
    """The census of include/mdx_krecip.h, which tests/test_memguard_host.py does not see: every prototype is exported and bound,
    kept out of the other export lists, and -- unless it is a size function -- has at least two memory-contract cases, each with
    another one as its stale pre-fill."""
    from mdir_amd import _lib
    from test_gpu_krecip_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.KRECIP_EXPORTS) == set(NEW)
    assert not declared & (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS))
    assert {"mdx_" + entry for entry in COVERED} == {d for d in declared if not d.endswith("_workspace")}
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_library_exports_the_krecip_entry_points_and_keeps_the_abi():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name) and getattr(h, name).argtypes is not None
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_workspace_formula():
    from mdir_amd import _lib
    h = _lib.lib()
    for nq, r in ((1, 1), (1, 64), (1, 65), (7, 1000), (70, 4096), (300, 100)):
        assert h.mdx_krecip_rerank_workspace(nq, r) == nq * ((4 * r + 255) // 256 * 256)
    for nq, r in ((0, 10), (-1, 10), (1 << 31, 10), (5, 0), (5, -2), (5, MAX_R + 1)):
        assert h.mdx_krecip_rerank_workspace(nq, r) == 0


def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID / MDX_ERR_WORKSPACE of the section, through the C ABI with pointers that are no memory: nothing is
    launched (there is no device here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(4096)
    big = 1 << 31
    inf, nan = float("inf"), float("nan")

    def refused(status, name, *words, code=-1):
        msg = h.mdx_last_error()
        assert status == code and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)

    def sets(ids=p, n=10, k=4, rk=p, rkc=p, rh=p, rhc=p):
        return h.mdx_krecip_sets(ids, n, k, rk, rkc, rh, rhc, None)
    for kw in ({"ids": None}, {"rk": None}, {"rkc": None}, {"rh": None}, {"rhc": None}):
        refused(sets(**kw), "mdx_krecip_sets", "NULL")
    for kw in ({"n": 0}, {"n": -1}, {"k": 0}, {"k": -3}):
        refused(sets(**kw), "mdx_krecip_sets", ">= 1")
    refused(sets(n=big), "mdx_krecip_sets", "2^31")
    refused(sets(k=MAX_K1 + 1), "mdx_krecip_sets", "MDX_KRECIP_MAX_K1")

    def raw_offsets(n=10, k=4, rk=p, rkc=p, rh=p, rhc=p, off=p):
        return h.mdx_krecip_raw_offsets(n, k, rk, rkc, rh, rhc, off, None)
    for kw in ({"rk": None}, {"rkc": None}, {"rh": None}, {"rhc": None}, {"off": None}):
        refused(raw_offsets(**kw), "mdx_krecip_raw_offsets", "NULL")
    for kw in ({"n": 0}, {"k": 0}):
        refused(raw_offsets(**kw), "mdx_krecip_raw_offsets", ">= 1")
    refused(raw_offsets(n=big), "mdx_krecip_raw_offsets", "2^31")
    refused(raw_offsets(k=65), "mdx_krecip_raw_offsets", "MDX_KRECIP_MAX_K1")

    def raw_fill(rows=p, ld=8, d=8, ids=p, sims=p, n=10, k=4, rk=p, rkc=p, rh=p, rhc=p, off=p, cols=p, vals=p, nnz=50):
        return h.mdx_krecip_raw_fill(rows, ld, d, ids, sims, n, k, rk, rkc, rh, rhc, off, cols, vals, nnz, None)
    for kw in ({"rows": None}, {"ids": None}, {"sims": None}, {"rk": None}, {"rkc": None}, {"rh": None}, {"rhc": None}, {"off": None},
               {"cols": None}, {"vals": None}):
        refused(raw_fill(**kw), "mdx_krecip_raw_fill", "NULL")
    for kw in ({"n": 0}, {"k": 0}):
        refused(raw_fill(**kw), "mdx_krecip_raw_fill", ">= 1")
    refused(raw_fill(n=big), "mdx_krecip_raw_fill", "2^31")
    refused(raw_fill(k=65), "mdx_krecip_raw_fill", "MDX_KRECIP_MAX_K1")
    for kw in ({"d": 0}, {"ld": 7}):
        refused(raw_fill(**kw), "mdx_krecip_raw_fill", "ld >= d")
    refused(raw_fill(nnz=-1), "mdx_krecip_raw_fill", "nnz=-1")

    def expand_offsets(ids=p, n=10, k=4, k2=2, ro=p, rc=p, rnnz=50, off=p):
        return h.mdx_krecip_expand_offsets(ids, n, k, k2, ro, rc, rnnz, off, None)

    def expand_fill(ids=p, n=10, k=4, k2=2, ro=p, rc=p, rv=p, rnnz=50, off=p, cols=p, vals=p, nnz=60):
        return h.mdx_krecip_expand_fill(ids, n, k, k2, ro, rc, rv, rnnz, off, cols, vals, nnz, None)
    for kw in ({"ids": None}, {"ro": None}, {"rc": None}, {"off": None}):
        refused(expand_offsets(**kw), "mdx_krecip_expand_offsets", "NULL")
    for kw in ({"ids": None}, {"ro": None}, {"rc": None}, {"rv": None}, {"off": None}, {"cols": None}, {"vals": None}):
        refused(expand_fill(**kw), "mdx_krecip_expand_fill", "NULL")
    for fn, name in ((expand_offsets, "mdx_krecip_expand_offsets"), (expand_fill, "mdx_krecip_expand_fill")):
        for kw in ({"n": 0}, {"k": 0}):
            refused(fn(**kw), name, ">= 1")
        refused(fn(n=big), name, "2^31")
        refused(fn(k=65, k2=1), name, "MDX_KRECIP_MAX_K1")
        for k2 in (0, -1, 5):
            refused(fn(k2=k2), name, "k2=", "[1, 4]")
        refused(fn(k=32, k2=8), name, "MDX_KRECIP_MAX_NNZ", "4352")         # 8 * 32 * 17
        refused(fn(k=64, k2=2), name, "MDX_KRECIP_MAX_NNZ")                 # k2 = 1 is the cap exactly
        refused(fn(rnnz=-1), name, "raw_nnz=-1")
    refused(expand_fill(nnz=-2), "mdx_krecip_expand_fill", "nnz=-2")

    def rerank(rh=p, rhc=p, kth=p, n=100, k=10, k2=4, ro=p, rc=p, rv=p, rnnz=50, eo=p, ec=p, ev=p, ennz=60, sc=p, lds=100,
               top=p, nq=3, r=20, lam=0.3, out=ctypes.c_void_p(1 << 20), ldo=100, ws=ctypes.c_void_p(1 << 24), wsb=1 << 20):
        return h.mdx_krecip_rerank(rh, rhc, kth, n, k, k2, ro, rc, rv, rnnz, eo, ec, ev, ennz, sc, lds, top, nq, r, lam, out, ldo,
                                   ws, wsb, None)
    name = "mdx_krecip_rerank"
    for kw in ({"rh": None}, {"rhc": None}, {"kth": None}, {"ro": None}, {"rc": None}, {"rv": None}, {"eo": None}, {"ec": None},
               {"ev": None}, {"sc": None}, {"top": None}, {"out": None}, {"ws": None}):
        refused(rerank(**kw), name, "NULL")
    for kw in ({"n": 0}, {"k": 0}, {"nq": 0}, {"nq": -4}, {"r": 0}, {"r": -1}):
        refused(rerank(**kw), name, ">= 1")
    refused(rerank(n=big, lds=big, ldo=big), name, "2^31")
    refused(rerank(k=65, k2=1), name, "MDX_KRECIP_MAX_K1")
    for k2 in (0, 11):
        refused(rerank(k2=k2), name, "k2=", "[1, 10]")
    refused(rerank(k=32, k2=8), name, "MDX_KRECIP_MAX_NNZ")
    refused(rerank(n=5000, lds=5000, ldo=5000, r=MAX_R + 1), name, "MDX_KRECIP_MAX_R")
    refused(rerank(r=101), name, "<= n=100")
    refused(rerank(n=1 << 30, lds=1 << 30, ldo=1 << 30, nq=1 << 14), name, "split the queries")
    refused(rerank(n=4096, lds=4096, ldo=4096, r=4096, nq=1 << 28), name, "nq * r", "split the queries")
    for kw in ({"rnnz": -1}, {"ennz": -1}):
        refused(rerank(**kw), name, "nnz")
    for kw in ({"lds": 99}, {"ldo": 99}):
        refused(rerank(**kw), name, "must be >= n=100")
    for lam in (-0.1, 1.5, inf, -inf, nan):
        refused(rerank(lam=lam), name, "lam=")
    refused(rerank(out=ctypes.c_void_p(4096 + 8)), name, "overlaps")
    assert rerank(out=p, wsb=0) == -4                                        # out == scores with the same stride is allowed
    need = h.mdx_krecip_rerank_workspace(3, 20)
    refused(rerank(wsb=need - 1), name, "workspace", code=-4)
    refused(rerank(ws=ctypes.c_void_p((1 << 24) + 8)), name, "16-byte aligned")
    # a CSR with no entries needs no columns
    refused(rerank(rc=None, rv=None, rnnz=0, ec=None, ev=None, ennz=0, wsb=0), name, "workspace", code=-4)


# ------------------------------------------------------------------ the criterion key

def test_k_reciprocal_key_is_validated():
    from mdir_amd import rerank
    from mdir_amd.score import _k_reciprocal_params
    assert rerank.K_RECIPROCAL_DEFAULTS == {"k1": 20, "k2": 6, "lam": 0.3, "truncate": 1000}
    assert _k_reciprocal_params(None) is None
    assert _k_reciprocal_params({}) == rerank.K_RECIPROCAL_DEFAULTS
    assert _k_reciprocal_params({"k1": 64, "k2": 1, "lam": 1, "truncate": 4096}) == {"k1": 64, "k2": 1, "lam": 1.0, "truncate": 4096}
    assert _k_reciprocal_params({"lam": 0}) == dict(rerank.K_RECIPROCAL_DEFAULTS, lam=0.0)
    for bad in ([], "k1", 5, True):
        with pytest.raises(ValueError, match="k_reciprocal: a mapping"):
            _k_reciprocal_params(bad)
    with pytest.raises(ValueError, match="unknown keys \\['k'\\]"):
        _k_reciprocal_params({"k": 5})
    for key in ("k1", "k2", "truncate"):
        for bad in (0, -1, 2.0, True, "3", None):
            with pytest.raises(ValueError, match="k_reciprocal: %s must be an integer >= 1" % key):
                _k_reciprocal_params({key: bad})
    for bad in ({"k1": 65}, {"k1": 5, "k2": 6}, {"k1": 32, "k2": 8}, {"k1": 64, "k2": 2}):
        with pytest.raises(ValueError, match="k_reciprocal: k1 <= 64, k2 <= k1 and"):
            _k_reciprocal_params(bad)
    with pytest.raises(ValueError, match=r"truncate must be an integer in \[1, 4096\]"):
        _k_reciprocal_params({"truncate": 4097})
    for bad in (-0.1, 1.01, float("nan"), float("inf"), True, "0.3", None):
        with pytest.raises(ValueError, match="k_reciprocal: lam"):
            _k_reciprocal_params({"lam": bad})


def _criterion(**keys):
    """CirDatasetAp on a dataset that is never read: the keys are validated before it is."""
    from mdir_amd.score import CirDatasetAp
    params = dict({"image_size": 64, "dataset": "no-such-dataset", "transforms": "pil2np | totensor | normalize",
                   "mean_std": [[0.5] * 3, [0.25] * 3]}, **keys)
    return CirDatasetAp(params)


def test_k_reciprocal_exclusions():
    with pytest.raises(ValueError, match="k_reciprocal together with diffusion is not supported"):
        _criterion(k_reciprocal={}, diffusion={})
    with pytest.raises(ValueError, match="rescore together with k_reciprocal is not supported"):
        _criterion(k_reciprocal={}, rescore={"shortlist": 10}, storage="i8")
    with pytest.raises(ValueError, match="k_reciprocal: k1"):
        _criterion(k_reciprocal={"k1": 65})
    with pytest.raises(ValueError, match="neighbours.*neither is on"):
        _criterion(neighbours="i8")
    # allowed together: the keys pass, and only the dataset is then missing
    for keys in ({"k_reciprocal": {}}, {"k_reciprocal": {"k1": 10}, "query_expansion": {"k": 3, "alpha": 3.0}},
                 {"k_reciprocal": {}, "database_augmentation": {"k": 3, "alpha": 3.0}, "neighbours": "i8"}):
        with pytest.raises(Exception) as err:
            _criterion(**keys)
        assert "k_reciprocal" not in str(err.value) and "neighbours" not in str(err.value), err.value


def test_k_reciprocal_is_single_process(monkeypatch):
    from mdir_amd import score
    obj = score.CirDatasetAp.__new__(score.CirDatasetAp)
    obj.dataset, obj.query_expansion, obj.database_augmentation, obj.diffusion, obj.rescore = "x", None, None, None, None
    obj.k_reciprocal = dict(score.rerank.K_RECIPROCAL_DEFAULTS)
    monkeypatch.setattr(score, "_rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="k_reciprocal re-ranks in a single process.*2 ranks"):
        obj(None, "cpu", None)


# ------------------------------------------------------------------ the Python checks

def test_rerank_checks_need_no_gpu():
    import torch
    from mdir_amd import rerank
    x = torch.zeros((8, 4))
    for kw, word in (({"k1": 0}, "k1"), ({"k1": True}, "k1"), ({"k1": 2.0}, "k1"), ({"k2": 0}, "k2"), ({"k1": 65}, "k1 must be <= 64"),
                     ({"k1": 5, "k2": 6}, "k2 must be <= k1"), ({"k1": 32, "k2": 8}, "exceeds 4096"), ({"chunk": 0}, "chunk"),
                     ({"layout": "XY"}, "unknown layout"), ({"index": object()}, "int8 DescriptorIndex")):
        with pytest.raises(ValueError, match=word):
            rerank.ReciprocalEncoding(x, **kw)
    with pytest.raises(ValueError, match="2-d"):
        rerank.ReciprocalEncoding(torch.zeros(8))
    enc = rerank.ReciprocalEncoding.__new__(rerank.ReciprocalEncoding)
    enc.n = 9
    q = torch.zeros((2, 4))
    for kw, word in (({"truncate": 0}, "truncate"), ({"truncate": 4097}, r"truncate must be in \[1, 4096\]"), ({"truncate": 1.5}, "truncate"),
                     ({"lam": -0.1}, "lam"), ({"lam": 1.1}, "lam"), ({"lam": float("nan")}, "lam"), ({"lam": True}, "lam")):
        with pytest.raises(ValueError, match=word):
            rerank.k_reciprocal(q, x, enc, **kw)
    with pytest.raises(ValueError, match=r"qvecs \[Q, D\] and vecs \[N, D\]"):
        rerank.k_reciprocal(torch.zeros((2, 5)), x, enc)
    with pytest.raises(ValueError, match="encoding has 9 rows, the database 8"):
        rerank.k_reciprocal(q, x, enc)
    enc.n = 8
    with pytest.raises(ValueError, match=r"scores must be \[2, 8\]"):
        rerank.k_reciprocal(q, x, enc, scores=torch.zeros((2, 7)))


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    ids = torch.zeros((6, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.krecip_sets(ids)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match="krecip_sets: ids must be"):
        ops.krecip_sets(torch.zeros((6, 65), dtype=torch.int64))
    with pytest.raises(TypeError, match="ids must be torch.int64"):
        ops.krecip_sets(ids.int())
    i32 = torch.int32
    sets = (torch.zeros((6, 4), dtype=i32), torch.zeros(6, dtype=i32), torch.zeros((6, 2), dtype=i32), torch.zeros(6, dtype=i32))
    with pytest.raises(ValueError, match="krecip_raw_offsets: sets of krecip_sets expected"):
        ops.krecip_raw_offsets(sets[:2] + (torch.zeros((6, 3), dtype=i32), sets[3]))
    off = torch.zeros(7, dtype=torch.int64)
    with pytest.raises(ValueError, match="krecip_raw_fill: sims must be"):
        ops.krecip_raw_fill(torch.zeros((6, 8)), ids, torch.zeros((6, 3)), sets, off, 0)
    with pytest.raises(ValueError, match="krecip_raw_fill: rows must be"):
        ops.krecip_raw_fill(torch.zeros((5, 8)), ids, torch.zeros((6, 4)), sets, off, 0)
    for nnz in (-1, 2.0, True):
        with pytest.raises(ValueError, match="integer nnz >= 0"):
            ops.krecip_raw_fill(torch.zeros((6, 8)), ids, torch.zeros((6, 4)), sets, off, nnz)
    raw = (off, torch.zeros(3, dtype=i32), torch.zeros(3))
    for k2 in (0, 5, True):
        with pytest.raises(ValueError, match=r"k2 must be an integer in \[1, k\] = \[1, 4\]"):
            ops.krecip_expand_offsets(ids, k2, raw)
    with pytest.raises(ValueError, match="raw CSR expected"):
        ops.krecip_expand_fill(ids, 2, (off[:6], raw[1], raw[2]), off, 0)
    big = torch.zeros((6, 32), dtype=torch.int64)
    with pytest.raises(ValueError, match="KRECIP_MAX_NNZ = 4096"):
        ops.krecip_expand_offsets(big, 8, raw)
    half, kth, s, top = (sets[2], sets[3]), torch.zeros(6), torch.zeros((2, 6)), torch.zeros((2, 3), dtype=torch.int64)
    for lam in (-0.5, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="lam"):
            ops.krecip_rerank(half, kth, 4, 2, raw, raw, s, top, lam)
    with pytest.raises(ValueError, match=r"R = 7 must be in \[1, min\(N, 4096\)\]"):
        ops.krecip_rerank(half, kth, 4, 2, raw, raw, s, torch.zeros((2, 7), dtype=torch.int64), 0.3)
    with pytest.raises(ValueError, match=r"scores must be \[nq, 6\]"):
        ops.krecip_rerank(half, kth, 4, 2, raw, raw, torch.zeros((2, 5)), top, 0.3)
    with pytest.raises(ValueError, match="rh \\[N, 2\\], rh_counts \\[N\\] and kth \\[N\\] expected"):
        ops.krecip_rerank(half, torch.zeros(5), 4, 2, raw, raw, s, top, 0.3)
