"""Editing the lists of the inverted file (include/mdx_lists_edit.h; IVFPQIndex.add / .remove / .attach_rows / .state of
mdir_amd/ivfpq.py) on a CPU-only box: the census of include/mdx_lists_edit.h, every refusal of the C ABI with nothing launched, the
Python refusals that need no device, and the restatement (tests/lists_edit_restatement.py) checked against brute-force loops on tiny
data."""
import ctypes
import os
import re

import numpy as np
import pytest

import lists_edit_restatement as LR
from conftest import ROOT

NEW = ("mdx_lists_merge", "mdx_lists_compact")


def _declared():
    """The code of include/mdx_lists_edit.h, which mdx.h includes for its section "inverted file, editing the lists"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_lists_edit.h"$', text, flags=re.M) and "inverted file, editing the lists" in text
    assert text.index('#include "mdx_lists_pq.h"') < text.index('#include "mdx_lists_edit.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_lists_edit.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LISTS_EDIT_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS)
              | set(_lib.IVF_EXPORTS) | set(_lib.LISTS_I8_EXPORTS) | set(_lib.LISTS_PQ_EXPORTS))
    assert not declared & others and not {n for n in others if "lists_merge" in n or "lists_compact" in n}
    # the prototypes of mdx.h itself are pinned by tests/test_cabi.py: none of these is written there
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_lists_(merge|compact)[a-z0-9_]*\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert re.search(r"int\s+mdx_lists_merge\s*\(\s*const uint8_t \*a_rows,\s*int64_t a_ld,\s*const int64_t \*a_members,"
                     r"\s*const int64_t \*a_offsets,\s*int64_t ma,\s*const uint8_t \*b_rows,\s*int64_t b_ld,\s*const int64_t \*b_members,"
                     r"\s*const int64_t \*b_offsets,\s*int64_t mb,\s*int64_t K,\s*int64_t width,\s*uint8_t \*out_rows,\s*int64_t out_ld,"
                     r"\s*int64_t \*out_members,\s*int64_t \*out_offsets,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_lists_compact\s*\(\s*const uint8_t \*rows,\s*int64_t ld,\s*const int64_t \*members,\s*const int64_t \*offsets,"
                     r"\s*int64_t m,\s*int64_t K,\s*int64_t width,\s*const int64_t \*kept,\s*int64_t mo,\s*uint8_t \*out_rows,"
                     r"\s*int64_t out_ld,\s*int64_t \*out_members,\s*int64_t \*out_offsets,\s*void \*stream\s*\)", code)
    header = open(os.path.join(ROOT, "include", "mdx_lists_edit.h")).read()
    for word in ("Refusals", "never interpreted", "left untouched", "binary search", "Launch shape", "legal under stream capture",
                 "no workspace"):
        assert word in header, word
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_lists_edit\.hip\b", makefile, flags=re.M) and "include/mdx_lists_edit.h" in makefile
    assert '"mdx_lists_edit.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "lists_merge" in n or "lists_compact" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_lists_edit_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == set(NEW)
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_before_any_device_work():
    """Every MDX_ERR_INVALID of the section through the C ABI with pointers that are no memory: nothing is launched (there is no
    device here to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    ptr = [ctypes.c_void_p((1 << 20) + (i << 16)) for i in range(10)]
    big = 1 << 31

    def refused(status, name, *words):
        msg = h.mdx_last_error()
        assert status == -1 and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)

    def merge(ar=ptr[0], a_ld=None, am=ptr[1], ao=ptr[2], ma=10, br=ptr[3], b_ld=None, bm=ptr[4], bo=ptr[5], mb=7, k=4, width=8,
              out=ptr[6], out_ld=None, om=ptr[7], oo=ptr[8]):
        return h.mdx_lists_merge(ar, width if a_ld is None else a_ld, am, ao, ma, br, width if b_ld is None else b_ld, bm, bo, mb, k, width,
                                 out, width if out_ld is None else out_ld, om, oo, None)
    name = "mdx_lists_merge"
    for arg in ("ar", "am", "ao", "br", "bm", "bo", "out", "om", "oo"):
        refused(merge(**{arg: None}), name, "NULL")
    for kw in ({"ma": -1}, {"mb": -3}, {"ma": 0, "mb": 0}, {"ma": big}, {"mb": big}, {"ma": big - 1, "mb": 1}):
        refused(merge(**kw), name, "ma + mb in [1, 2^31)")
    for kw in ({"k": 0}, {"k": -2}, {"k": big}, {"width": 0}, {"width": -8}, {"width": big}):
        refused(merge(**kw), name, "must be in [1, 2^31)")
    for kw in ({"a_ld": 7}, {"b_ld": 0}, {"out_ld": 7}, {"a_ld": big}, {"b_ld": big}, {"out_ld": big}):
        refused(merge(**kw), name, "must be in [width=8, 2^31)")
    for out in ("out", "om", "oo"):
        for given in ("ar", "am", "ao", "br", "bm", "bo"):
            refused(merge(**{out: ptr[9], given: ptr[9]}), name, "an output pointer equals an input pointer")
    for one, two in (("out", "om"), ("out", "oo"), ("om", "oo")):
        refused(merge(**{one: ptr[9], two: ptr[9]}), name, "two output pointers are equal")

    def compact(rows=ptr[0], ld=None, members=ptr[1], offsets=ptr[2], m=10, k=4, width=8, kept=ptr[3], mo=5, out=ptr[6], out_ld=None,
                om=ptr[7], oo=ptr[8]):
        return h.mdx_lists_compact(rows, width if ld is None else ld, members, offsets, m, k, width, kept, mo, out,
                                   width if out_ld is None else out_ld, om, oo, None)
    name = "mdx_lists_compact"
    for arg in ("rows", "members", "offsets", "kept", "out", "om", "oo"):
        refused(compact(**{arg: None}), name, "NULL")
    for kw in ({"m": 0}, {"m": -1}, {"m": big}, {"mo": 0}, {"mo": -4}, {"mo": big}):
        refused(compact(**kw), name, "m=", "must be in [1, 2^31)")
    for kw in ({"k": 0}, {"k": big}, {"width": 0}, {"width": big}):
        refused(compact(**kw), name, "K=", "must be in [1, 2^31)")
    for kw in ({"ld": 7}, {"out_ld": 3}, {"ld": big}, {"out_ld": big}):
        refused(compact(**kw), name, "must be in [width=8, 2^31)")
    for out in ("out", "om", "oo"):
        for given in ("rows", "members", "offsets", "kept"):
            refused(compact(**{out: ptr[9], given: ptr[9]}), name, "an output pointer equals an input pointer")
    for one, two in (("out", "om"), ("out", "oo"), ("om", "oo")):
        refused(compact(**{one: ptr[9], two: ptr[9]}), name, "two output pointers are equal")


def test_python_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivfpq, ops
    rows, members, offsets = torch.zeros((10, 3), dtype=torch.uint8), torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    kept = torch.zeros(11, dtype=torch.int64)
    for call, word in ((lambda: ops.lists_merge(rows, members, offsets, rows, members, offsets), "a_rows"),
                       (lambda: ops.lists_merge(None, members, offsets, rows, members, offsets), "a_rows"),
                       (lambda: ops.lists_compact(rows, members, offsets, kept), "rows")):
        with pytest.raises(ValueError, match="%s must be a CUDA" % word):
            call()
    # the index: checks that come before any device work, on an index built without a device
    vectors, q = torch.zeros((300, 12)), torch.zeros((2, 12))

    def bare(keep_rows):
        index = ivfpq.IVFPQIndex.__new__(ivfpq.IVFPQIndex)
        index.rows, index.d, index.lists, index.coarse, index.m, index.device = vectors if keep_rows else None, 12, 3, object(), 3, q.device
        index.n = index.size = 300
        return index
    kept_rows, dropped = bare(True), bare(False)
    ids = torch.zeros(4, dtype=torch.int64)
    for call in (lambda: kept_rows.add(q), lambda: kept_rows.remove(ids)):
        with pytest.raises(ValueError, match="keeps the fp32 rows.*attach_rows\\(None\\)"):
            call()
    for args, word in (((torch.zeros((2, 8)),), "batch is \\[B, 8\\] and the index has D = 12"),
                       ((q.double(),), "batch must be a non-empty fp32"),
                       ((q, torch.zeros(3, dtype=torch.int64)), "labels must be an int64 \\[2\\] tensor"),
                       ((q, torch.zeros(2, dtype=torch.int32)), "labels must be an int64 \\[2\\] tensor"),
                       ((torch.zeros((12, 2)).t(),), "batch must have contiguous rows"),
                       ((q, None, 0), "chunk must be an integer >= 1"),
                       ((q,), "batch must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            dropped.add(*args)
    dropped.n = (1 << 31) - 2
    with pytest.raises(ValueError, match="the id bound must stay below 2\\^31"):
        dropped.add(q)
    dropped.n = 300
    for bad, word in ((ids.int(), "ids must be an int64 1-d tensor"), (ids.reshape(2, 2), "ids must be an int64 1-d tensor"),
                      ([1, 2], "ids must be an int64 1-d tensor"), (ids, "ids must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            dropped.remove(bad)
    for bad, word in ((vectors[:299], "rows are \\(299, 12\\) and the ids of the index need \\[n = 300, D = 12\\]"),
                      (vectors.double(), "rows must be a non-empty fp32"), (vectors, "rows must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            dropped.attach_rows(bad)
    assert dropped.rows is None
    kept_rows.attach_rows(None)
    assert kept_rows.rows is None
    closed = bare(False)
    closed.coarse = None
    for call in (lambda: closed.add(q), lambda: closed.remove(ids)):
        with pytest.raises(ValueError, match="the index is closed"):
            call()
    # a state that does not fit together, and one that is not on a device
    good = {"centroids": torch.zeros((3, 12)), "codewords": torch.zeros((3, 256, 4)), "codes": torch.zeros((300, 3), dtype=torch.uint8),
            "order": torch.zeros(300, dtype=torch.int64), "offsets": torch.zeros(4, dtype=torch.int64), "n": 300, "m": 3}
    with pytest.raises(ValueError, match="state must be a dict of centroids, codewords, codes, order, offsets, n, m"):
        ivfpq.IVFPQIndex.from_state({k: v for k, v in good.items() if k != "order"})
    for change, word in (({"codes": torch.zeros((300, 3))}, "state\\['codes'\\] must be a non-empty 2-d torch.uint8 tensor"),
                         ({"order": torch.zeros(299, dtype=torch.int64)}, "does not fit together"),
                         ({"offsets": torch.zeros(5, dtype=torch.int64)}, "does not fit together"),
                         ({"n": 299}, "does not fit together"), ({"m": 4}, "does not fit together"),
                         ({"m": 5}, "D = 12 is not a multiple of m = 5"), ({"n": 0}, "n must be an integer >= 1"),
                         ({}, "the state must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            ivfpq.IVFPQIndex.from_state(dict(good, **change))


# ------------------------------------------------------------------------------------------------ the restatement itself

def _random_structure(rng, lists, m, width, first_id=0):
    labels = rng.integers(0, lists, m)
    labels[labels == 2] = 0                                                 # list 2 stays empty
    members = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.zeros(lists + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(labels, minlength=lists))
    return rng.integers(0, 256, (m, width)).astype(np.uint8), members + first_id, offsets


def test_restatement_equals_a_brute_force_loop():
    rng = np.random.default_rng(6)
    for lists, ma, mb, width in ((5, 40, 23, 3), (4, 0, 9, 1), (4, 9, 0, 2), (1, 1, 1, 5)):
        a, b = _random_structure(rng, lists, ma, width), _random_structure(rng, lists, mb, width, first_id=ma)
        rows, members, offsets = LR.merge(*a, *b)
        want = []                                                          # (list, id, payload) of every row: by list, then by id
        for (r, mem, off) in (a, b):
            for l in range(lists):
                want += [(l, int(mem[p]), r[p].tolist()) for p in range(int(off[l]), int(off[l + 1]))]
        want.sort(key=lambda t: (t[0], t[1]))
        assert offsets.tolist() == (a[2] + b[2]).tolist() and offsets[0] == 0 and offsets[-1] == ma + mb == len(members)
        got = [(l, int(members[p]), rows[p].tolist()) for l in range(lists) for p in range(int(offsets[l]), int(offsets[l + 1]))]
        assert got == want and rows.dtype == np.uint8 and members.dtype == offsets.dtype == np.int64
        # offsets beyond m are clamped
        wild_a, wild_b = a[2].copy(), b[2].copy()
        wild_a[-1] += 5
        wild_b[-1] += 1 << 40
        for x, y in zip(LR.merge(a[0], a[1], wild_a, b[0], b[1], wild_b), (rows, members, offsets)):
            assert np.array_equal(x, y)
        # the compaction: a loop over the positions
        keep = rng.random(ma + mb) < 0.5
        keep[0] = True
        kept = LR.prefix(keep)
        assert kept[0] == 0 and kept[-1] == keep.sum() and all(kept[p + 1] - kept[p] == keep[p] for p in range(ma + mb))
        c_rows, c_members, c_offsets = LR.compact(rows, members, offsets, kept)
        out_rows, out_members = [None] * int(kept[-1]), [None] * int(kept[-1])
        for p in range(ma + mb):
            if kept[p + 1] > kept[p]:
                out_rows[kept[p]], out_members[kept[p]] = rows[p].tolist(), int(members[p])
        assert c_rows.tolist() == out_rows and c_members.tolist() == out_members
        assert c_offsets.tolist() == [int(keep[:o].sum()) for o in offsets]
        # remove: by id, duplicates and strangers ignored
        gone = [int(members[0]), int(members[-1]), int(members[0]), -1, ma + mb + 7]
        (r_rows, r_members, r_offsets), removed = LR.remove(rows, members, offsets, gone)
        stay = [p for p in range(ma + mb) if int(members[p]) not in gone]
        assert removed == len(set(gone) & set(members.tolist())) == ma + mb - len(stay)
        assert r_members.tolist() == members[stay].tolist() and r_rows.tolist() == rows[stay].tolist()
        assert np.diff(r_offsets).tolist() == [sum(1 for p in stay if offsets[l] <= p < offsets[l + 1]) for l in range(lists)]
