"""Near-duplicate groups (include/mdx.h, "near-duplicate groups"; mdir_amd/search.py duplicate_groups) on a CPU-only box: the
census of include/mdx_groups.h, every refusal of the C ABI with nothing launched, the Python checks of duplicate_groups and of the
ops wrappers, and the arithmetic that splits a chunk whose candidates are too many."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ("mdx_groups_init", "mdx_groups_union_pairs", "mdx_groups_union_dense", "mdx_groups_labels")
MAX_T = 8


def _declared():
    """The code of include/mdx_groups.h, the prototypes that mdx.h includes for its section "near-duplicate groups"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_groups.h"$', text, flags=re.M)
    assert text.index('#include "mdx_knn_join.h"') < text.index('#include "mdx_groups.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_groups.h")).read(), flags=re.S)


def test_header_declares_the_groups_entry_points():
    from mdir_amd import _lib, ops
    code = _declared()
    assert int(re.search(r"#define MDX_GROUPS_MAX_T (\d+)\b", code).group(1)) == ops.GROUPS_MAX_T == MAX_T
    assert re.search(r"int\s+mdx_groups_union_pairs\s*\(\s*const float \*rows,\s*int64_t ld,\s*int64_t d,\s*const uint64_t \*pairs,\s*int64_t P,"
                     r"\s*const float \*taus,\s*int64_t T,\s*int32_t \*parent,\s*int64_t n,\s*int64_t \*status,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_groups_union_dense\s*\(\s*const float \*scores,\s*int64_t m,\s*int64_t ncols,\s*int64_t ld,\s*int64_t row_base,"
                     r"\s*int64_t col_base,\s*const float \*taus,\s*int64_t T,\s*int32_t \*parent,\s*int64_t n,\s*int64_t \*status,"
                     r"\s*void \*stream\s*\)", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.GROUPS_EXPORTS
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    for phrase in ("near-duplicate groups", "label_tau[i] = min", "parent[x] <= x", "agent-scope relaxed atomic", "Skip rule"):
        assert phrase in text, phrase
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert "mdx_groups.hip" in makefile and "include/mdx_groups.h" in makefile


def test_every_groups_entry_point_is_covered():
    """The census of include/mdx_groups.h, which tests/test_memguard_host.py does not see: every prototype is exported and bound,
    kept out of EXPORTS, and has at least two memory-contract cases, each with another one as its stale pre-fill."""
    from mdir_amd import _lib
    from test_gpu_groups_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.GROUPS_EXPORTS) == set(NEW)
    assert not declared & (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS))
    assert {"mdx_" + entry for entry in COVERED} == declared
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def test_library_exports_the_groups_entry_points():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name) and getattr(h, name).argtypes is not None


def _floats(*vals):
    return (ctypes.c_float * len(vals))(*vals)


def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID of the section, through the C ABI with pointers that are no memory: nothing is launched (there is no
    device here to launch on)."""
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    big = (1 << 31)
    inf, nan = float("inf"), float("nan")

    def init(parent=p, T=2, n=10, status=p):
        return h.mdx_groups_init(parent, T, n, status, None)
    for kw in ({"parent": None}, {"status": None}):
        assert init(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for n in (0, -3, big):
        assert init(n=n) == -1 and b"2^31" in h.mdx_last_error()
    for T in (0, -1, MAX_T + 1):
        assert init(T=T) == -1 and b"MDX_GROUPS_MAX_T" in h.mdx_last_error()

    def labels(parent=p, T=2, n=10, out=ctypes.c_void_p(512)):
        return h.mdx_groups_labels(parent, T, n, out, None)
    for kw in ({"parent": None}, {"out": None}):
        assert labels(**kw) == -1 and b"NULL" in h.mdx_last_error()
    assert labels(out=p) == -1 and b"buffer of its own" in h.mdx_last_error()
    for n in (0, big):
        assert labels(n=n) == -1 and b"2^31" in h.mdx_last_error()
    for T in (0, MAX_T + 1):
        assert labels(T=T) == -1 and b"MDX_GROUPS_MAX_T" in h.mdx_last_error()

    good = _floats(0.9, 0.5)

    def pairs(rows=p, ld=8, d=8, pr=p, P=10, taus=good, T=2, parent=p, n=10, status=p):
        return h.mdx_groups_union_pairs(rows, ld, d, pr, P, taus, T, parent, n, status, None)
    for kw in ({"rows": None}, {"pr": None}, {"taus": None}, {"parent": None}, {"status": None}):
        assert pairs(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"n": 0}, {"n": -1}, {"n": big}):
        assert pairs(**kw) == -1 and b"n=" in h.mdx_last_error()
    for kw in ({"d": 0}, {"P": 0}, {"P": -5}, {"d": -1}):
        assert pairs(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert pairs(P=big) == -1 and b"P=" in h.mdx_last_error() and b"2^31" in h.mdx_last_error()
    for T in (0, -1, MAX_T + 1):
        assert pairs(T=T) == -1 and b"MDX_GROUPS_MAX_T" in h.mdx_last_error()
    for bad in (inf, -inf, nan):
        assert pairs(taus=_floats(0.9, bad)) == -1 and b"finite" in h.mdx_last_error()
        assert pairs(taus=_floats(bad), T=1) == -1 and b"finite" in h.mdx_last_error()
    assert pairs(ld=7) == -1 and b"ld=7" in h.mdx_last_error()

    def dense(sc=p, m=4, ncols=6, ld=6, rb=0, cb=0, taus=good, T=2, parent=p, n=10, status=p):
        return h.mdx_groups_union_dense(sc, m, ncols, ld, rb, cb, taus, T, parent, n, status, None)
    for kw in ({"sc": None}, {"taus": None}, {"parent": None}, {"status": None}):
        assert dense(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"n": 0}, {"n": big}):
        assert dense(**kw) == -1 and b"n=" in h.mdx_last_error()
    for kw in ({"m": 0}, {"ncols": 0}, {"m": -2}):
        assert dense(**kw) == -1 and b">= 1" in h.mdx_last_error()
    for T in (0, MAX_T + 1):
        assert dense(T=T) == -1 and b"MDX_GROUPS_MAX_T" in h.mdx_last_error()
    for bad in (inf, nan):
        assert dense(taus=_floats(bad, 0.5)) == -1 and b"finite" in h.mdx_last_error()
    assert dense(ld=5) == -1 and b"ld=5" in h.mdx_last_error()
    for kw in ({"rb": -1}, {"cb": -1}):
        assert dense(**kw) == -1 and b"< 0" in h.mdx_last_error()
    for kw in ({"rb": 7}, {"cb": 5}, {"m": 11}, {"ncols": 11, "ld": 11}, {"rb": (1 << 62)}):
        assert dense(**kw) == -1 and b"outside" in h.mdx_last_error()


# ------------------------------------------------------------------ the Python checks

def _fake_index(storage="i8", n=4, d=8):
    from mdir_amd import ops
    fake = ops.DescriptorIndex.__new__(ops.DescriptorIndex)
    fake.storage, fake.n, fake.d, fake._h = storage, n, d, None
    return fake


def test_duplicate_groups_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops, search
    assert search.Groups._fields == ("labels", "offsets", "members", "stats") and ops.GROUPS_MAX_T == MAX_T
    cpu = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="fp32 device tensor"):
        search.duplicate_groups(None, cpu, 0.9)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rows = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="int8 DescriptorIndex"):
        search.duplicate_groups(object(), rows, 0.9)
    with pytest.raises(ValueError, match="int8 index"):
        search.duplicate_groups(_fake_index("f16"), rows, 0.9)
    with pytest.raises(ValueError, match=r"index's \[5, 8\] rows"):
        search.duplicate_groups(_fake_index(n=5), rows, 0.9)
    for index in (None, _fake_index()):
        for bad in ("0.9", None, [], (), [0.9] * (MAX_T + 1), {0.9}):
            with pytest.raises(ValueError, match="threshold must be a number or a sequence"):
                search.duplicate_groups(index, rows, bad)
        for bad in (float("inf"), float("nan"), [0.9, float("nan")], [0.5, "x"], [True], 1e39):
            with pytest.raises(ValueError, match="threshold"):
                search.duplicate_groups(index, rows, bad)
        for chunk in (0, -128, 1.5, True):
            with pytest.raises(ValueError, match="chunk"):
                search.duplicate_groups(index, rows, 0.9, chunk=chunk)
        for cap in (0, -1, 2.0, None, False):
            with pytest.raises(ValueError, match="max_candidates"):
                search.duplicate_groups(index, rows, 0.9, max_candidates=cap)


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    cpu32, cpu64, cpuf = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros((4, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.groups_union_pairs(cpuf, cpu64, 0.9, cpu32, cpu64)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.groups_union_dense(cpuf, 0, 0, 0.9, cpu32, cpu64)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.groups_labels(cpu32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.groups_status(cpu64)
    for levels, n in ((0, 4), (MAX_T + 1, 4), (True, 4), (2, 0), (2, 1 << 31), (2, 4.0)):
        with pytest.raises(ValueError, match="groups_init"):
            ops.groups_init(levels, n, "cpu")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match="thresholds"):
        ops.groups_union_pairs(cpuf, cpu64, [], cpu32, cpu64)
    with pytest.raises(ValueError, match=r"3 thresholds and 4 rows for a forest of \[2, 4\]"):
        ops.groups_union_pairs(cpuf, cpu64, [0.9, 0.8, 0.7], cpu32, cpu64)
    with pytest.raises(ValueError, match=r"2 thresholds and 5 rows for a forest of \[2, 4\]"):
        ops.groups_union_pairs(torch.zeros((5, 4)), cpu64, [0.9, 0.8], cpu32, cpu64)
    with pytest.raises(ValueError, match="pairs must be a 1-d tensor of 1 to"):
        ops.groups_union_pairs(cpuf, cpu64[:0], [0.9, 0.8], cpu32, cpu64)
    with pytest.raises(TypeError, match="parent must be torch.int32"):
        ops.groups_union_pairs(cpuf, cpu64, [0.9, 0.8], cpu32.long(), cpu64)
    with pytest.raises(ValueError, match=r"status must be the int64 \[4\]"):
        ops.groups_union_pairs(cpuf, cpu64, [0.9, 0.8], cpu32, torch.zeros(3, dtype=torch.int64))
    for rb, cb in ((-1, 0), (0, -1), (True, 0), (0, 1.0)):
        with pytest.raises(ValueError, match="must be an integer >= 0"):
            ops.groups_union_dense(cpuf, rb, cb, [0.9, 0.8], cpu32, cpu64)
    for rb, cb in ((1, 0), (0, 1)):
        with pytest.raises(ValueError, match=r"for a forest of \[2, 4\]"):
            ops.groups_union_dense(cpuf, rb, cb, [0.9, 0.8], cpu32, cpu64)
    with pytest.raises(ValueError, match=r"forest of groups_init"):
        ops.groups_labels(torch.zeros(4, dtype=torch.int32))


# ------------------------------------------------------------------ splitting a chunk

def test_split_rows_arithmetic():
    """A chunk whose candidates exceed max_candidates is cut in two at a multiple of 128 rows from its (128-aligned) start; the
    halves cover it exactly, in order, and a single block is not split."""
    from mdir_amd import ops, search
    B = ops.JOIN_BLOCK
    assert B == 128
    assert search.split_rows(0, 1) is None and search.split_rows(0, B) is None and search.split_rows(5 * B, 5 * B + 7) is None
    assert search.split_rows(0, B + 1) == ((0, B), (B, B + 1))
    assert search.split_rows(0, 2 * B) == ((0, B), (B, 2 * B))
    assert search.split_rows(B, B + (1 << 15)) == ((B, B + (1 << 14)), (B + (1 << 14), B + (1 << 15)))
    assert search.split_rows(2 * B, 1000) == ((2 * B, 5 * B), (5 * B, 1000))
    for lo in (0, B, 7 * B):
        for rows in (1, 127, 128, 129, 255, 256, 257, 1000, 32768, 32769, 1004993 - 30 * 32768):
            todo, leaves = [(lo, lo + rows)], []
            while todo:                                   # split to the bottom, as a set whose every chunk is too large would be
                a, b = todo.pop()
                halves = search.split_rows(a, b)
                if halves is None:
                    leaves.append((a, b))
                    continue
                (a0, m0), (m1, b1) = halves
                assert a0 == a and b1 == b and m0 == m1 and a < m0 < b and (m0 - lo) % B == 0
                assert abs((m0 - a) - (b - m0)) <= 2 * B
                todo.extend([(m1, b1), (a0, m0)])
            assert leaves[0][0] == lo and leaves[-1][1] == lo + rows and all(x[1] == y[0] for x, y in zip(leaves, leaves[1:]))
            assert all(0 < b - a <= B and a % B == 0 for a, b in leaves)
