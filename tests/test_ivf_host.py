"""The inverted file (include/mdx_ivf.h; mdir_amd/ivf.py) on a CPU-only box: the census of include/mdx_ivf.h, the restatement
(tests/ivf_restatement.py) checked against a brute-force loop on lattice data, every refusal of the C ABI with nothing launched, and the
Python checks of the ops wrappers and of ivf.IVFIndex."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivf_restatement as IR
import lattice
from conftest import ROOT

NEW = ("mdx_ivf_plan_workspace", "mdx_ivf_plan", "mdx_ivf_scan", "mdx_ivf_select")
F32 = np.float32


def _declared():
    """The code of include/mdx_ivf.h, which mdx.h includes for its section "inverted file"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_ivf.h"$', text, flags=re.M) and "inverted file" in text
    assert text.index('#include "mdx_kmeans.h"') < text.index('#include "mdx_ivf.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_ivf.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib, ops
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.IVF_EXPORTS) == set(NEW)
    assert all(name.startswith("mdx_ivf_") for name in declared)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS))
    assert not declared & others and not {n for n in others if n.startswith("mdx_ivf")}
    # the prototypes of mdx.h itself are pinned by tests/test_cabi.py: none of these is written there
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_ivf_[a-z_]+\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert re.search(r"int64_t\s+mdx_ivf_plan_workspace\s*\(\s*int64_t nq,\s*int64_t nprobe,\s*int64_t K\s*\)", code)
    assert re.search(r"int\s+mdx_ivf_plan\s*\(\s*const int64_t \*probes,\s*int64_t nq,\s*int64_t nprobe,\s*const int64_t \*offsets,\s*int64_t K,"
                     r"\s*int64_t m,\s*int64_t cap,\s*void \*plan,\s*int64_t plan_bytes,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_ivf_select\s*\(\s*const float \*cand_scores,\s*const int64_t \*cand_ids,\s*int64_t nq,\s*int64_t cap,"
                     r"\s*int64_t nprobe,\s*int64_t K,\s*const void \*plan,\s*int64_t plan_bytes,\s*int64_t k,\s*int64_t \*out_ids,"
                     r"\s*float \*out_scores,\s*void \*stream\s*\)", code)
    group = int(re.search(r"#define MDX_IVF_QUERY_GROUP (\d+)", code).group(1))
    tile = int(re.search(r"#define MDX_IVF_TILE (\d+)", code).group(1))
    assert group == ops.IVF_QUERY_GROUP == IR.QUERY_GROUP and tile == ops.IVF_TILE == IR.TILE
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_ivf\.hip\b", makefile, flags=re.M) and "include/mdx_ivf.h" in makefile
    assert '"mdx_ivf.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "ivf" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_ivf_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == {n for n in NEW if not n.endswith("_workspace")}
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


def _plan_bytes(nq, nprobe, k):
    up = lambda b: (b + 255) // 256 * 256
    return 2 * up(8 * nq * nprobe) + up(8 * nq) + 2 * up(8 * (k + 1)) + up(16 * k)


def test_workspace_formula():
    from mdir_amd import _lib
    h = _lib.lib()
    for nq, nprobe, k in ((1, 1, 1), (3, 2, 6), (70, 16, 4096), (2048, 128, 1024), (9, 6, 6), (33, 31, 32)):
        assert h.mdx_ivf_plan_workspace(nq, nprobe, k) == _plan_bytes(nq, nprobe, k), (nq, nprobe, k)
    for nq, nprobe, k in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, 2, 1), (1 << 31, 1, 1), (1, 1, 1 << 31), (1 << 20, 1 << 11, 1 << 12)):
        assert h.mdx_ivf_plan_workspace(nq, nprobe, k) == 0, (nq, nprobe, k)


# ------------------------------------------------------------------------------------------------ the restatement itself

def _brute(labels, lists, probes, scores, k):
    """Python loops and sorted(): the candidates of every query and the first k by (key, id)."""
    from oracle import chain as OC
    ids_out, sc_out, scanned = [], [], []
    for q, row in enumerate(probes):
        cand = []
        for l in row:
            cand += [i for i in range(len(labels)) if labels[i] == l]
        ranked = sorted(cand, key=lambda i: (OC.desc_key(scores[q, i]), i))[:k]
        scanned.append(len(cand))
        ids_out.append(ranked + [-1] * (k - len(ranked)))
        sc_out.append([scores[q, i] for i in ranked] + [np.nan] * (k - len(ranked)))
    return np.array(ids_out, np.int64), np.array(sc_out, F32), np.array(scanned, np.int64)


def test_restatement_equals_a_brute_force_loop_on_lattice_data():
    lat = lattice.common(90, 12, 5, seed=4, amp=1)                       # amp = 1: about a hundred distinct scores, many ties
    lattice.assert_exact_in_any_order(lat.qi, lat.xi)
    scores = lattice.expected(lat.qi, lat.xi, 1.0)
    rng = np.random.default_rng(1)
    lists = 6
    labels = rng.integers(0, lists - 1, 90)                               # the last list stays empty
    for nprobe in (1, 2, lists):
        probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(5)])
        want_ids, want_sc, want_n = _brute(labels, lists, probes, scores, 7)
        ids, sc, n = IR.search_labels(labels, lists, probes, scores, 7)
        IR.same_bits(ids, want_ids), IR.same_bits(sc, want_sc), IR.same_bits(n, want_n)
        assert all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() for r in ids)
    # ties inside the answer: equal scores leave in ascending id, whatever list they come from
    ids, sc, _ = IR.search_labels(labels, lists, np.tile(np.arange(lists)[::-1], (5, 1)), scores, 30)
    assert any((np.diff(sc[q]) == 0).any() for q in range(5))
    for q in range(5):
        tied = np.flatnonzero(np.diff(sc[q]) == 0)
        assert (ids[q, tied] < ids[q, tied + 1]).all()
    # all lists probed: the first k of the oracle's full ranking
    from oracle import chain as OC
    np.testing.assert_array_equal(ids, OC.rank_full(scores)[:, :30])
    # padding, the cut at cap, probes outside [0, K), member ids outside the rows, clamped offsets
    members, offsets = IR.csr(labels, lists)
    ids, sc, n = IR.search(members, offsets, [[5, 0]], scores[:1], int((labels == 0).sum()) + 3)
    assert n[0] == (labels == 0).sum() and (ids[0, -3:] == -1).all() and np.isnan(sc[0, -3:]).all() and not np.isnan(sc[0, :-3]).any()
    assert [len(c) for c in IR.candidates(members, offsets, [[0, 1], [-1, 6], [1, 1]], cap=4)] == [4, 0, 4]
    spoiled = members.copy()
    spoiled[:2] = (-1, 90)
    got = IR.candidate_scores(scores[0], spoiled[:4])
    assert np.isnan(got[:2]).all() and np.array_equal(got[2:], scores[0, spoiled[2:4]])
    base, count, entries, items = IR.plan([[0, 7, 1], [1, 1, -1]], [-5, 3, 200, 200], 90, 1000)
    assert base.tolist() == [[0, -1, 3], [0, 87, -1]] and count.tolist() == [90, 174] and entries == [[0], [2, 3, 4], []] and items == 1 + 2


def test_item_bound_covers_the_plan():
    from mdir_amd import ivf, ops
    rng = np.random.default_rng(0)
    for lists, nq, nprobe in ((6, 9, 2), (40, 70, 5), (40, 300, 40), (7, 1, 1), (12, 64, 3)):
        sizes = rng.integers(0, 400, lists)
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        tiles = np.sort(-(-sizes // ops.IVF_TILE))[::-1]
        for trial in range(5):
            weights = rng.random(lists) ** (4 * trial)                    # from even to very skewed probing
            probes = np.stack([rng.choice(lists, nprobe, replace=False, p=weights / weights.sum()) for _ in range(nq)])
            items = IR.plan(probes, offsets, int(sizes.sum()), 1 << 30)[3]
            assert items <= ivf.item_bound(int(tiles[:nprobe].sum()), int(tiles.sum()), nq), (lists, nq, nprobe, trial)


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

    def common(call, name, need):
        """The refusals the three calls share: the sizes of the plan, the plan itself, cap."""
        for kw in ({"nq": 0}, {"nprobe": 0}, {"k": 0}, {"nq": -3}):
            refused(call(**kw), name, "must be >= 1")
        for kw in ({"nprobe": 7}, {"nq": 1 << 31}, {"k": 1 << 31}, {"nq": 1 << 20, "nprobe": 1 << 11, "k": 1 << 12}):
            refused(call(**kw), name, "too large")
        refused(call(wsb=need - 1), name, "workspace", code=-4)
        refused(call(wsp=None), name, "workspace", code=-4)
        for off in (4, 8):
            refused(call(wsp=ctypes.c_void_p((1 << 24) + off)), name, "16-byte aligned")
        for cap in (0, -1, 1 << 31):
            refused(call(cap=cap), name, "cap=")
        refused(call(nq=1 << 22, cap=1 << 20), name, "too large for one launch")

    need = h.mdx_ivf_plan_workspace(5, 2, 6)
    assert need == _plan_bytes(5, 2, 6) == 6 * 256

    def plan(probes=p, nq=5, nprobe=2, offsets=q, k=6, m=100, cap=50, wsp=ws, wsb=None):
        return h.mdx_ivf_plan(probes, nq, nprobe, offsets, k, m, cap, wsp, h.mdx_ivf_plan_workspace(nq, nprobe, k) if wsb is None else wsb, None)
    name = "mdx_ivf_plan"
    for kw in ({"probes": None}, {"offsets": None}):
        refused(plan(**kw), name, "NULL")
    for m in (0, -1, 1 << 31):
        refused(plan(m=m), name, "m=")
    common(plan, name, need)

    def scan(rows=p, n=100, d=8, ld=8, members=q, m=100, offsets=q, k=6, queries=p, nq=5, lay=1, center=None, nprobe=2, wsp=ws, wsb=None,
             cap=50, items=10, cs=q, ci=q):
        return h.mdx_ivf_scan(rows, n, d, ld, members, m, offsets, k, queries, nq, lay, center, nprobe, wsp,
                              h.mdx_ivf_plan_workspace(nq, nprobe, k) if wsb is None else wsb, cap, items, cs, ci, None)
    name = "mdx_ivf_scan"
    for kw in ({"rows": None}, {"members": None}, {"offsets": None}, {"queries": None}, {"cs": None}, {"ci": None}):
        refused(scan(**kw), name, "NULL")
    for kw in ({"n": 0}, {"d": 0, "ld": 0}, {"m": 0}, {"n": 1 << 31}, {"d": 1 << 31, "ld": 1 << 31}, {"m": 1 << 31}):
        refused(scan(**kw), name, "must be in [1, 2^31)")
    refused(scan(ld=7), name, "ld=7 < d=8")
    refused(scan(n=1 << 30, ld=1 << 40), name, "overflows")
    for lay in (2, -1):
        refused(scan(lay=lay), name, "qlayout")
    for items in (0, -1, 1 << 31):
        refused(scan(items=items), name, "items=")
    common(scan, name, need)

    def select(cs=p, ci=q, nq=5, cap=50, nprobe=2, k=6, wsp=ws, wsb=None, top=3, oi=q, osc=q):
        return h.mdx_ivf_select(cs, ci, nq, cap, nprobe, k, wsp, h.mdx_ivf_plan_workspace(nq, nprobe, k) if wsb is None else wsb, top, oi, osc, None)
    name = "mdx_ivf_select"
    for kw in ({"cs": None}, {"ci": None}, {"oi": None}, {"osc": None}):
        refused(select(**kw), name, "NULL")
    for top in (0, -1, 4097):
        refused(select(top=top), name, "k=")
    common(select, name, need)


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    rows, queries = torch.zeros((10, 4)), torch.zeros((3, 4))
    probes, offsets, members = torch.zeros((3, 2), dtype=torch.int64), torch.zeros(7, dtype=torch.int64), torch.zeros(10, dtype=torch.int64)
    plan = torch.zeros(_plan_bytes(3, 2, 6), dtype=torch.uint8)
    cs, ci = torch.zeros((3, 5)), torch.zeros((3, 5), dtype=torch.int64)
    for call, word in ((lambda: ops.ivf_plan(probes, offsets, 10, 5), "probes"),
                       (lambda: ops.ivf_scan(rows, members, offsets, queries, plan, 2, 5, 4), "rows"),
                       (lambda: ops.ivf_select(cs, ci, plan, 2, 6, 3), "cand_scores"), (lambda: ops.ivf_plan(None, offsets, 10, 5), "probes")):
        with pytest.raises(ValueError, match="%s must be a CUDA" % word):
            call()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    # ivf_plan
    with pytest.raises(ValueError, match="probes must be torch.int64"):
        ops.ivf_plan(probes.int(), offsets, 10, 5)
    with pytest.raises(ValueError, match="probes must be a non-empty 2-d"):
        ops.ivf_plan(probes[0], offsets, 10, 5)
    with pytest.raises(ValueError, match="probes must be a contiguous"):
        ops.ivf_plan(torch.zeros((2, 3), dtype=torch.int64).t(), offsets, 10, 5)
    with pytest.raises(ValueError, match="offsets must be torch.int64"):
        ops.ivf_plan(probes, offsets.float(), 10, 5)
    with pytest.raises(ValueError, match="offsets must be a contiguous"):
        ops.ivf_plan(probes, torch.zeros(14, dtype=torch.int64)[::2], 10, 5)
    with pytest.raises(ValueError, match="nprobe must be in \\[1, K\\]"):
        ops.ivf_plan(probes, offsets[:2], 10, 5)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="m must be an integer >= 1"):
            ops.ivf_plan(probes, offsets, bad, 5)
        with pytest.raises(ValueError, match="cap must be an integer >= 1"):
            ops.ivf_plan(probes, offsets, 10, bad)
    # ivf_scan
    with pytest.raises(ValueError, match="rows must be torch.float32"):
        ops.ivf_scan(rows.double(), members, offsets, queries, plan, 2, 5, 4)
    with pytest.raises(ValueError, match="rows must be a matrix with contiguous rows"):
        ops.ivf_scan(torch.zeros((4, 10)).t(), members, offsets, queries, plan, 2, 5, 4)
    with pytest.raises(ValueError, match="queries must be torch.float32"):
        ops.ivf_scan(rows, members, offsets, queries.half(), plan, 2, 5, 4)
    with pytest.raises(ValueError, match="query dimension 3 != rows dimension 4"):
        ops.ivf_scan(rows, members, offsets, queries, plan, 2, 5, 4, qlayout="DN")
    with pytest.raises(ValueError, match="unknown layout"):
        ops.ivf_scan(rows, members, offsets, queries, plan, 2, 5, 4, qlayout="NQ")
    with pytest.raises(ValueError, match="queries must be contiguous"):
        ops.ivf_scan(rows, members, offsets, torch.zeros((3, 8))[:, :4], plan, 2, 5, 4)
    with pytest.raises(ValueError, match="members must be torch.int64"):
        ops.ivf_scan(rows, members.int(), offsets, queries, plan, 2, 5, 4)
    with pytest.raises(ValueError, match="offsets must be a non-empty 1-d"):
        ops.ivf_scan(rows, members, offsets.reshape(1, 7), queries, plan, 2, 5, 4)
    for at, what in ((5, "nprobe"), (6, "cap"), (7, "items")):
        for bad in (0, 1.5, True):
            args = [rows, members, offsets, queries, plan, 2, 5, 4]
            args[at] = bad
            with pytest.raises(ValueError, match="%s must be an integer >= 1" % what):
                ops.ivf_scan(*args)
    with pytest.raises(ValueError, match="center must be a contiguous \\[4\\]"):
        ops.ivf_scan(rows, members, offsets, queries, plan, 2, 5, 4, center=torch.zeros(5))
    with pytest.raises(ValueError, match="center must be torch.float32"):
        ops.ivf_scan(rows, members, offsets, queries, plan, 2, 5, 4, center=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="plan must be torch.uint8"):
        ops.ivf_scan(rows, members, offsets, queries, plan.float(), 2, 5, 4)
    with pytest.raises(ValueError, match="nprobe must be in \\[1, K\\]"):
        ops.ivf_scan(rows, members, offsets, queries, plan, 7, 5, 4)
    # ivf_select
    with pytest.raises(ValueError, match="cand_scores must be torch.float32"):
        ops.ivf_select(cs.double(), ci, plan, 2, 6, 3)
    with pytest.raises(ValueError, match="cand_ids must be torch.int64"):
        ops.ivf_select(cs, ci.int(), plan, 2, 6, 3)
    with pytest.raises(ValueError, match="cand_ids must be a contiguous \\[3, 5\\]"):
        ops.ivf_select(cs, ci[:, :4], plan, 2, 6, 3)
    for bad in (0, 4097, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer in \\[1, 4096\\]"):
            ops.ivf_select(cs, ci, plan, 2, 6, bad)
    for at, what in ((3, "nprobe"), (4, "lists")):
        args = [cs, ci, plan, 2, 6, 3]
        args[at] = 0
        with pytest.raises(ValueError, match="%s must be an integer >= 1" % what):
            ops.ivf_select(*args)
    # the views of a plan need no device
    plan = torch.arange(_plan_bytes(3, 2, 6) // 8, dtype=torch.int64).view(torch.uint8)
    views = ops.ivf_plan_views(plan, 3, 2, 6)
    assert {k: tuple(v.shape) for k, v in views.items()} == {"base": (3, 2), "count": (3,), "first": (7,), "item": (7,), "entry": (6,)}
    assert [int(v.reshape(-1)[0]) for v in views.values()] == [0, 32, 64, 96, 128]


def test_index_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivf, ops
    rows, cents = torch.zeros((10, 4)), torch.zeros((3, 4))
    labels = torch.zeros(10, dtype=torch.int64)
    assert ivf.IVFResult._fields == ("ids", "scores", "probes", "scanned")
    for doc_word in ("cluster._members", "nprobe == lists", "rank_full", "ascending row id", "-1", "ops.RESCORE_MAX_K", "no CPU fallback",
                     "x_q = q - center", "one synchronisation", "never\n    copied or permuted", "ivf_plan", "ivf_scan", "ivf_select"):
        assert doc_word in ivf.__doc__, doc_word
    for call, word in ((lambda: ivf.IVFIndex(rows.double(), cents), "rows must be a non-empty fp32"),
                       (lambda: ivf.IVFIndex(rows[0], cents), "rows must be a non-empty fp32"),
                       (lambda: ivf.IVFIndex(torch.zeros((4, 10)).t(), cents), "rows must have contiguous rows"),
                       (lambda: ivf.IVFIndex(rows, cents[:0]), "centroids must be a non-empty fp32"),
                       (lambda: ivf.IVFIndex(rows, torch.zeros((3, 8))[:, :4]), "centroids must be contiguous"),
                       (lambda: ivf.IVFIndex(rows, torch.zeros((3, 5))), "dimensions differ"),
                       (lambda: ivf.IVFIndex(rows, cents, labels.int()), "labels must be an int64 \\[10\\]"),
                       (lambda: ivf.IVFIndex(rows, cents, labels[:9]), "labels must be an int64 \\[10\\]"),
                       (lambda: ivf.IVFIndex(rows, cents, [0] * 10), "labels must be an int64 \\[10\\]"),
                       (lambda: ivf.IVFIndex(torch.zeros((10, 8))[:, :4], cents), "rows must be contiguous to be assigned"),
                       (lambda: ivf.IVFIndex(rows, cents, chunk=0), "chunk must be an integer >= 1"),
                       (lambda: ivf.IVFIndex(rows, cents, labels), "rows must be a CUDA"),
                       (lambda: ivf.IVFIndex.train(rows, 11), "k = 11 > N = 10 rows"),
                       (lambda: ivf.IVFIndex.train(rows, 3, init="kmeans++"), "init 'kmeans\\+\\+'")):
        with pytest.raises(ValueError, match=word):
            call()
    # search: an index built without a device (the checks come before any device work)
    index = ivf.IVFIndex.__new__(ivf.IVFIndex)
    index.rows, index.d, index.lists, index.coarse = rows, 4, 3, object()
    q = torch.zeros((2, 4))
    for args, kw, word in (((q.double(), 1, 1), {}, "queries must be a non-empty fp32"), ((q[0], 1, 1), {}, "queries must be a non-empty fp32"),
                           ((q, 1, 1), {"qlayout": "NQ"}, "qlayout 'NQ'"), ((q, 1, 1), {"qlayout": "DN"}, "queries have dimension 2"),
                           ((torch.zeros((2, 8))[:, :4], 1, 1), {}, "queries must be contiguous"),
                           ((q, 0, 1), {}, "k must be an integer >= 1"), ((q, 2.0, 1), {}, "k must be an integer >= 1"),
                           ((q, ops.RESCORE_MAX_K + 1, 1), {}, "k = 4097 > 4096"), ((q, 1, 0), {}, "nprobe must be an integer >= 1"),
                           ((q, 1, True), {}, "nprobe must be an integer >= 1"), ((q, 1, 4), {}, "nprobe = 4 > 3 lists"),
                           ((q, 1, 1), {"center": torch.zeros(5)}, "center must be a contiguous fp32 tensor of 4"),
                           ((q, 1, 1), {"center": torch.zeros(4, dtype=torch.float64)}, "center must be a contiguous fp32 tensor of 4"),
                           ((q, 1, 1), {}, "queries must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            index.search(*args, **kw)
    index.coarse = None
    with pytest.raises(ValueError, match="the index is closed"):
        index.search(q, 1, 1)
    index.close()                                                         # closing twice is fine
    # what the index derives from the list sizes
    index._capacity, index._tiles = [0, 130, 195, 195], [0, 3, 5, 5]
    assert [index.capacity(p) for p in (1, 2, 3)] == [130, 195, 195]
    g = ops.IVF_QUERY_GROUP
    assert index.items(1, 1) == max(1, (3 + (g - 1) * 3) // g) and index.items(100, 2) == (500 + (g - 1) * 5) // g
    assert index.query_chunk(1) == ivf.CANDIDATE_MEMORY_CAP // (12 * 130)
    index._capacity = [0, 0]
    assert index.capacity(1) == 1


def test_both_indices_derive_the_same_capacities_from_one_set_sizes():
    """``_set_sizes`` is the base's: a bare ``IVFIndex`` and a bare ``IVFPQIndex`` given the same list sizes agree on ``_capacity``,
    ``capacity(p)`` is the sum of the ``p`` largest sizes and ``items(nq, p)`` the ``item_bound`` of the tiles of those lists."""
    from mdir_amd import ivf, ivfpq, ops
    sizes = (0, 1, 63, 64, 65, 130)
    plain, coded = ivf.IVFIndex.__new__(ivf.IVFIndex), ivfpq.IVFPQIndex.__new__(ivfpq.IVFPQIndex)
    assert type(plain)._set_sizes is type(coded)._set_sizes
    for index in (plain, coded):
        index._set_sizes(list(sizes))
        assert index.host_sizes == list(sizes)
    assert plain._capacity == coded._capacity and plain._tiles == coded._tiles
    by_size = sorted(sizes, reverse=True)
    tiles = [-(-s // ops.IVF_TILE) for s in by_size]
    for p in range(1, 7):
        for index in (plain, coded):
            assert index.capacity(p) == sum(by_size[:p])
            for nq in (1, 17, 100):
                assert index.items(nq, p) == ivf.item_bound(sum(tiles[:p]), sum(tiles), nq)
