"""The overlap of two sets of top-K lists (include/mdx_overlap.h; ops.topk_overlap, search.recall_at), without a GPU:

  a. the numpy restatement (tests/overlap_restatement.py) on cases counted by hand;
  b. census: the prototype of include/mdx_overlap.h is exported, bound, apart from every other export tuple and covered by
     tests/test_gpu_overlap_memcontract.py;
  c. the library refuses every malformed call before any device work, and the Python wrapper needs no GPU for its checks.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import overlap_restatement as R
from conftest import ROOT

NEW = ("mdx_topk_overlap",)


# ------------------------------------------------------------------------------------------------------ a. the restatement

def test_restatement_by_hand():
    a = np.array([[5, 3, 9, -1], [1, 2, 3, 4]])
    b = np.array([[9, 5, 7], [4, 3, 2]])
    # query 0: depth 1 -> {5} & {9}; 2 -> {5, 3} & {9, 5}; 3 -> {5, 3, 9} & {9, 5, 7}; 10 -> the padding counts for nothing
    # query 1: depth 1 -> {1} & {4}; 2 -> {1, 2} & {4, 3}; 3 -> {1, 2, 3} & {4, 3, 2}; 10 -> {1, 2, 3, 4} & {4, 3, 2}
    np.testing.assert_array_equal(R.topk_overlap(a, b, [1, 2, 3, 10]), [[0, 1, 2, 2], [0, 0, 2, 3]])
    np.testing.assert_array_equal(R.recall_at(a, b, [2, 10]), [[0.5, 2 / 3], [0.0, 1.0]])
    assert R.topk_overlap(a, b, [3]).dtype == np.int32
    # ids at or above 2^31 are padding on both sides
    big = np.array([[R.TOP, R.TOP + 1]])
    np.testing.assert_array_equal(R.topk_overlap(big, big, [2]), [[1]])
    assert np.isnan(R.recall_at(a[:1], np.full((1, 3), -1), [2])).all()


@pytest.mark.parametrize("kind", R.KINDS)
def test_row_makers(kind):
    rng = np.random.default_rng(3)
    for ka, kb, high in ((1, 1, False), (63, 65, True), (1000, 64, False)):
        a, b = R.rows(kind, ka, kb, rng, high)
        assert a.shape == (ka,) and b.shape == (kb,) and a.dtype == b.dtype == np.int64
        for row in (a, b):
            valid = row[row >= 0]
            assert len(set(valid.tolist())) == len(valid) and (row[row < 0] == -1).all() and (valid <= R.TOP).all()
        if high and kind != "padding":
            assert a.max() > R.TOP - 3 * R.MAX_K
        got = int(R.topk_overlap(a[None], b[None], [max(ka, kb)])[0, 0])
        m = min(ka, kb)
        assert got == {"identical": m, "shuffled": m, "disjoint": 0, "padding": 0, "half": (m + 1) // 2,
                       "padded_tail": min(ka // 2, (kb + 1) // 3, m)}[kind]
    for ka, kb in ((1, 4096), (64, 64), (65, 1000)):
        for t in (1, 8):
            d = R.straddling(ka, kb, t)
            assert len(d) == t and d == sorted(d) and d[0] >= 1
            if t == 8:
                assert d[0] < min(ka, kb) or min(ka, kb) == 1
                assert d[-1] > max(ka, kb) and min(ka, kb) in d


# ------------------------------------------------------------------------------------------------------------- b. census

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_overlap.h"$', text, flags=re.M) and "top-K lists, overlap" in text
    assert text.index('#include "mdx_unet.h"') < text.index('#include "mdx_overlap.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_overlap.h")).read(), flags=re.S)


def test_every_overlap_entry_point_is_covered():
    """The prototype of include/mdx_overlap.h is exported and bound (apart from mdx.h's own and from every other export tuple), it is no
    size function, and it has at least two memory-contract cases, each with a larger one whose leftovers are its stale pre-fill."""
    from mdir_amd import _lib
    from test_gpu_overlap_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.OVERLAP_EXPORTS) == set(NEW)
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "OVERLAP_EXPORTS"]
    assert {"EXPORTS", "KNN_JOIN_EXPORTS", "UNET_EXPORTS", "KNN_REVERSE_EXPORTS", "IVF_EXPORTS"} <= set(others)
    for other in others:
        assert not declared & set(getattr(_lib, other)), other
    assert not {n for n in declared if "_workspace" in n}
    assert {"mdx_" + entry for entry in COVERED} == declared
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry
    mdx_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert not re.search(r"\bmdx_topk_overlap\s*\(", mdx_h)
    header = open(os.path.join(ROOT, "include", "mdx_overlap.h")).read()
    assert "#define MDX_OVERLAP_MAX_K %d" % R.MAX_K in header and "#define MDX_OVERLAP_MAX_DEPTHS %d" % R.MAX_DEPTHS in header
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_overlap\.hip\b", makefile, flags=re.M) and "include/mdx_overlap.h" in makefile
    assert '"mdx_overlap.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()


# --------------------------------------------------------------------------------------------------- c. refusals, no device

def test_library_exports_binds_and_refuses_before_any_device_work():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    fn = h.mdx_topk_overlap
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert h.mdx_abi_version() == _lib.ABI_VERSION == 3
    pa, pb, out = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    depths = lambda *d: (ctypes.c_int32 * len(d))(*d)
    err = lambda: h.mdx_last_error()
    assert fn(None, 4, pb, 4, 1, depths(1), 1, out, None) == -1 and b"mdx_topk_overlap: NULL" in err()
    assert fn(pa, 4, None, 4, 1, depths(1), 1, out, None) == -1 and b"NULL" in err()
    assert fn(pa, 4, pb, 4, 1, None, 1, out, None) == -1 and b"NULL" in err()
    assert fn(pa, 4, pb, 4, 1, depths(1), 1, None, None) == -1 and b"NULL" in err()
    assert fn(pa, 4, pb, 4, 0, depths(1), 1, out, None) == -1 and b"nq=0" in err()
    assert fn(pa, 4, pb, 4, 1 << 31, depths(1), 1, out, None) == -1 and b"nq=" in err()
    for ka, kb in ((0, 4), (4, 0), (R.MAX_K + 1, 4), (4, R.MAX_K + 1), (-1, 4)):
        assert fn(pa, ka, pb, kb, 1, depths(1), 1, out, None) == -1 and b"must be in [1, 4096]" in err()
    assert fn(pa, 4, pb, 4, 1, depths(1), 0, out, None) == -1 and b"T=0" in err()
    assert fn(pa, 4, pb, 4, 1, depths(*range(1, 10)), 9, out, None) == -1 and b"T=9" in err()
    assert fn(pa, 4, pb, 4, 1, depths(0), 1, out, None) == -1 and b"positive and ascending (depths[0]=0)" in err()
    assert fn(pa, 4, pb, 4, 1, depths(-3, 4), 2, out, None) == -1 and b"depths[0]=-3" in err()
    assert fn(pa, 4, pb, 4, 1, depths(2, 5, 4), 3, out, None) == -1 and b"depths[2]=4" in err()
    assert fn(ctypes.c_void_p(4100), 4, pb, 4, 1, depths(1), 1, out, None) == -1 and b"aligned" in err()
    assert fn(pa, 4, ctypes.c_void_p((1 << 20) + 4), 4, 1, depths(1), 1, out, None) == -1 and b"aligned" in err()
    assert fn(pa, 4, pb, 4, 1, depths(1), 1, ctypes.c_void_p((1 << 21) + 2), None) == -1 and b"aligned" in err()


def test_wrapper_checks_need_no_gpu():
    from mdir_amd import ops, search
    assert (ops.OVERLAP_MAX_K, ops.OVERLAP_MAX_DEPTHS) == (R.MAX_K, R.MAX_DEPTHS) and ops.OVERLAP_MAX_K == ops.RESCORE_MAX_K
    ids = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.topk_overlap(ids, ids, [1])
    with pytest.raises(ValueError, match="no CPU fallback"):
        search.recall_at(ids, ids, 1)
