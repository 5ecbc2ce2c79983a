"""The int8 refinement of shortlists (include/mdx_refine.h; ops.refine_i8; IVFPQIndex(..., refine="i8") of mdir_amd/ivfpq.py) on a
CPU-only box: the census of include/mdx_refine.h, every refusal of the C ABI with nothing launched, the Python refusals that need no
device, the restatement (tests/refine_restatement.py) checked against a brute-force loop on tiny data, and the properties the module
docstring of ivfpq.py promises -- (b) and (c) -- on the restatement itself."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivf_restatement as IR
import lists_i8_restatement as LI
import pq_restatement as PR
import refine_restatement as RR
from conftest import ROOT

NEW = ("mdx_refine_i8_workspace", "mdx_refine_i8")
F32 = np.float32


def _declared():
    """The code of include/mdx_refine.h, which mdx.h includes for its section "inverted file, int8 refinement of shortlists"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_refine.h"$', text, flags=re.M) and "inverted file, int8 refinement of shortlists" in text
    assert text.index('#include "mdx_lists_edit.h"') < text.index('#include "mdx_refine.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_refine.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib
    code = _declared()
    assert re.search(r"#ifndef MDX_H\s*\n#error", code)
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.REFINE_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS)
              | set(_lib.IVF_EXPORTS) | set(_lib.LISTS_I8_EXPORTS) | set(_lib.LISTS_PQ_EXPORTS) | set(_lib.LISTS_EDIT_EXPORTS))
    assert not declared & others and not {n for n in others if "refine" in n}
    # the names stay clear of what the census of every other section of the inverted file calls its own
    for name in NEW:
        assert not any(word in name for word in ("ivf", "_pq", "lists_i8", "lists_merge", "lists_compact", "kmeans")), name
    # the prototypes of mdx.h itself are pinned by tests/test_cabi.py: none of these is written there
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_refine[a-z0-9_]*\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert re.search(r"int64_t\s+mdx_refine_i8_workspace\s*\(\s*int64_t nq,\s*int64_t S\s*\)", code)
    assert re.search(r"int\s+mdx_refine_i8\s*\(\s*const int8_t \*codes,\s*const float \*scales,\s*int64_t m,\s*int64_t d,"
                     r"\s*const int64_t \*where,\s*int64_t n,\s*const int8_t \*qcodes,\s*const float \*qscales,\s*int64_t nq,"
                     r"\s*const int64_t \*ids,\s*int64_t S,\s*int64_t \*out_ids,\s*float \*out_scores,\s*void \*workspace,"
                     r"\s*int64_t workspace_bytes,\s*void \*stream\s*\)", code)
    header = open(os.path.join(ROOT, "include", "mdx_refine.h")).read()
    for word in ("Refusals", "is dereferenced through an id outside", "two separately rounded products", "Launch shape", "legal under stream capture",
                 "out_ids may equal ids", "depend on nothing but its own inputs", "MDX_ERR_WORKSPACE"):
        assert word in header, word
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_refine\.hip\b", makefile, flags=re.M) and "include/mdx_refine.h" in makefile
    assert '"mdx_refine.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "refine" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_refine_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == {"mdx_refine_i8"}              # the other prototype is a size function
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_before_any_device_work():
    """Every refusal of the section through the C ABI with pointers that are no memory: nothing is launched (there is no device here
    to launch on), and the error names the call."""
    from mdir_amd import _lib
    h = _lib.lib()
    ptr = [ctypes.c_void_p((1 << 20) + (i << 16)) for i in range(10)]
    big = 1 << 31
    name = "mdx_refine_i8"

    def refused(status, *words, code=-1):
        msg = h.mdx_last_error()
        assert status == code and msg.startswith(name.encode() + b":"), (status, msg)
        for w in words:
            assert w.encode() in msg, (w, msg)

    def call(codes=ptr[0], scales=ptr[1], m=10, d=70, where=ptr[2], n=12, qcodes=ptr[3], qscales=ptr[4], nq=3, ids=ptr[5], s=65,
             out_ids=ptr[6], out_scores=ptr[7], ws=ptr[8], ws_bytes=1 << 20):
        return h.mdx_refine_i8(codes, scales, m, d, where, n, qcodes, qscales, nq, ids, s, out_ids, out_scores, ws, ws_bytes, None)
    for arg in ("codes", "scales", "where", "qcodes", "qscales", "ids", "out_ids", "out_scores"):
        refused(call(**{arg: None}), "NULL")
    for arg in ("n", "m", "d", "nq", "s"):
        for value in (0, -1, -big):
            refused(call(**{arg: value}), "must be >= 1")
    for s in (4097, 1 << 20, big):
        refused(call(s=s), "S=%d > 4096" % s)
    for d in (133121, big, 1 << 40):
        refused(call(d=d), "d=%d too large" % d)
    assert call(d=133120, codes=None) == -1                              # the largest d gets as far as the next check
    for arg in ("n", "m", "nq"):
        for value in (big, big + 5, 1 << 40):
            refused(call(**{arg: value}), "must be below 2^31")
    refused(call(nq=big - 1, s=65), "too large for one launch")         # two tiles a query
    refused(call(nq=big // 64, s=4096), "too large for one launch")
    for off in (1, 4, 8):
        refused(call(codes=ctypes.c_void_p(ptr[0].value + off)), "codes must be 16-byte aligned")
    # the workspace: round_up(4 nq S, 256); NULL or one byte short is MDX_ERR_WORKSPACE
    assert h.mdx_refine_i8_workspace(3, 65) == 1024 and h.mdx_refine_i8_workspace(1, 1) == 256 and h.mdx_refine_i8_workspace(2, 4096) == 32768
    assert h.mdx_refine_i8_workspace(1, 64) == 256 and h.mdx_refine_i8_workspace(1, 65) == 512
    for nq, s in ((0, 5), (-1, 5), (5, 0), (5, -3), (5, 4097)):
        assert h.mdx_refine_i8_workspace(nq, s) == 0
    refused(call(ws=None), "workspace", code=-4)
    refused(call(ws_bytes=1023), "workspace 1023 B < required 1024 B", code=-4)
    refused(call(ws=ctypes.c_void_p(ptr[8].value + 8)), "workspace must be 16-byte aligned")


def test_python_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivfpq, ops
    codes, scales = torch.zeros((10, 64), dtype=torch.int8), torch.zeros(10)
    where, qcodes, qscales, ids = torch.zeros(12, dtype=torch.int64), torch.zeros((2, 12), dtype=torch.int8), torch.zeros(2), \
        torch.zeros((2, 5), dtype=torch.int64)
    for first in (codes, None):
        with pytest.raises(ValueError, match="refine_i8: codes must be a CUDA"):
            ops.refine_i8(first, scales, 12, where, qcodes, qscales, ids)
    # the index: checks that come before any device work
    vectors, cents, q = torch.zeros((300, 12)), torch.zeros((3, 12)), torch.zeros((2, 12))
    for bad in ("f16", "I8", 8, True, ""):
        with pytest.raises(ValueError, match="refine must be None or \"i8\""):
            ivfpq.IVFPQIndex(vectors, cents, m=3, refine=bad)
        with pytest.raises(ValueError, match="refine must be None or \"i8\""):
            ivfpq.IVFPQIndex.train(vectors, 3, m=3, refine=bad)
    wide = torch.zeros((2, 133121))
    for make in (lambda: ivfpq.IVFPQIndex(wide, torch.zeros((1, 133121)), m=1, refine="i8"),
                 lambda: ivfpq.IVFPQIndex.train(wide, 1, m=1, refine="i8")):
        with pytest.raises(ValueError, match="refine=\"i8\": D = 133121 > 133120"):
            make()

    def bare(refine, keep_rows=False):
        index = ivfpq.IVFPQIndex.__new__(ivfpq.IVFPQIndex)
        index.rows, index.d, index.lists, index.coarse, index.m, index.device = vectors if keep_rows else None, 12, 3, object(), 3, q.device
        index.n = index.size = 300
        if refine:
            index.refine = refine
        return index
    plain, fine, fine_rows = bare(None, True), bare("i8"), bare("i8", True)
    assert plain.refine is None and ivfpq.IVFPQIndex.refine is None
    for kw in ({"rescore": 5}, {"shortlist": 10, "rescore": 5}, {"shortlist": 10, "rescore": 0}):
        with pytest.raises(ValueError, match="needs an index built with refine=\"i8\""):
            plain.search(q, 5, 2, **kw)
    with pytest.raises(ValueError, match="queries must be a CUDA"):     # everything else on such an index is as it was
        plain.search(q, 5, 2, shortlist=10)
    for index in (fine, fine_rows):
        with pytest.raises(ValueError, match="rescore = 5 needs a shortlist"):
            index.search(q, 5, 2, rescore=5)
        for r in (4, 11):
            with pytest.raises(ValueError, match="rescore = %d must be in \\[k = 5, shortlist = 10\\]" % r):
                index.search(q, 5, 2, shortlist=10, rescore=r)
        for r in (0, -2, 2.5, True):
            with pytest.raises(ValueError, match="rescore must be an integer >= 1"):
                index.search(q, 5, 2, shortlist=10, rescore=r)
        with pytest.raises(ValueError, match="queries must be a CUDA"):  # no fp32 rows are needed without rescore
            index.search(q, 5, 2, shortlist=10)
    with pytest.raises(ValueError, match="rescore = 7 of the refined shortlist is rescored on the fp32 rows"):
        fine.search(q, 5, 2, shortlist=10, rescore=7)
    with pytest.raises(ValueError, match="queries must be a CUDA"):
        fine_rows.search(q, 5, 2, shortlist=10, rescore=7)
    for call in (lambda: fine_rows.add(q), lambda: fine_rows.remove(torch.zeros(4, dtype=torch.int64))):   # that rule is unchanged
        with pytest.raises(ValueError, match="keeps the fp32 rows.*attach_rows\\(None\\)"):
            call()
    # the state of a refine index: both tensors, of the dtypes and shapes that go with codes and centroids
    good = {"centroids": torch.zeros((3, 12)), "codewords": torch.zeros((3, 256, 4)), "codes": torch.zeros((300, 3), dtype=torch.uint8),
            "order": torch.zeros(300, dtype=torch.int64), "offsets": torch.zeros(4, dtype=torch.int64), "n": 300, "m": 3,
            "refine_codes": torch.zeros((300, 64), dtype=torch.int8), "refine_scales": torch.zeros(300)}
    for change, word in (({"refine_codes": None}, "state\\['refine_codes'\\] must be a torch.int8 tensor of shape \\[300, 64\\]"),
                         ({"refine_scales": None}, "state\\['refine_scales'\\] must be a torch.float32 tensor of shape \\[300\\]"),
                         ({"refine_codes": torch.zeros((300, 64), dtype=torch.uint8)}, "state\\['refine_codes'\\]"),
                         ({"refine_codes": torch.zeros((300, 12), dtype=torch.int8)}, "state\\['refine_codes'\\]"),
                         ({"refine_codes": torch.zeros((299, 64), dtype=torch.int8)}, "state\\['refine_codes'\\]"),
                         ({"refine_scales": torch.zeros(300, dtype=torch.float64)}, "state\\['refine_scales'\\]"),
                         ({"refine_scales": torch.zeros((300, 1))}, "state\\['refine_scales'\\]"),
                         ({}, "the state must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            ivfpq.IVFPQIndex.from_state(dict(good, **change))


# ------------------------------------------------------------------------------------------------ the restatement itself

def test_restatement_equals_a_brute_force_loop():
    from oracle import chain
    rng = np.random.default_rng(12)
    for d, m, n, nq, s in ((5, 7, 11, 3, 9), (64, 4, 4, 1, 1), (70, 20, 33, 2, 40)):
        rows = rng.standard_normal((n, d)).astype(F32)
        members = rng.permutation(n)[:m].astype(np.int64)
        members[0] = n + 3                                                    # a position whose id lies outside the rows
        rows[members[1]] = 0                                                  # a zero row: scale 0
        codes, scales = LI.encode(rows, members)
        assert codes.shape == (m, (d + 63) // 64 * 64) and np.isnan(scales[0]) and scales[1] == 0 and not codes[:, d:].any()
        where = RR.where_of(members, n)
        assert sorted(where[where >= 0].tolist()) == list(range(1, m)) and all(members[where[i]] == i for i in range(n) if where[i] >= 0)
        where[members[2]] = m                                                 # stored nowhere: three ways to say so
        where[members[3 % m]] = 1 << 40
        queries = rng.standard_normal((nq, d)).astype(F32)
        qcodes, qscales = LI.quantize_np(queries)
        ids = rng.integers(-2, n + 3, (nq, s)).astype(np.int64)
        ids[0, -1] = ids[0, 0]                                                # a repeated id
        got_ids, got = RR.refine(codes, scales, d, where, qcodes, qscales, ids)
        for q in range(nq):
            pairs = []
            for j, i in enumerate(ids[q].tolist()):
                sc = F32(np.nan)
                if 0 <= i < n and 0 <= where[i] < m:
                    acc = sum(int(qcodes[q, k]) * int(codes[where[i], k]) for k in range(d))
                    with np.errstate(invalid="ignore"):
                        sc = F32(acc) * (scales[where[i]] * qscales[q])
                pairs.append((int(chain.desc_key(sc)), i, j, sc))
            pairs.sort(key=lambda t: t[:3])
            assert got_ids[q].tolist() == [t[1] for t in pairs]
            IR.same_bits(got[q], np.array([t[3] for t in pairs], F32))
            assert np.isnan(got[q][[not (0 <= i < n and 0 <= where[i] < m) for i in got_ids[q]]]).all()
        # the scores of stored ids are the int8 index's
        full = LI.i8_scores(rows, queries)
        ok = (got_ids >= 0) & (got_ids < n)
        ok[ok] = (where[got_ids[ok]] >= 0) & (where[got_ids[ok]] < m)
        for q in range(nq):
            IR.same_bits(got[q][ok[q]], full[q][got_ids[q][ok[q]]])


def _world(lists=6, m_sub=4, seed=39):
    """LI.planted() as an IVF-PQ index with a refinement payload, on the host: everything RR.search takes."""
    rows, queries, labels, cents = LI.planted(seed=seed, lists=lists)
    n, d = rows.shape
    members, offsets = IR.csr(labels, lists)
    words = (F32(0.05) * np.random.default_rng(seed + 1).standard_normal((m_sub, 256, d // m_sub))).astype(F32)
    pq_codes = PR.encode(words, rows[members] - cents[labels[members]])
    fine_codes, fine_scales = LI.encode(rows, members)
    coarse_all = PR.chain(queries, cents)
    return dict(rows=rows, queries=queries, labels=labels, lists=lists, n=n, members=members, offsets=offsets, pq_codes=pq_codes,
                fine_codes=fine_codes, fine_scales=fine_scales, table=PR.lut(words, queries), coarse_all=coarse_all)


def _probes(w, nprobe):
    picks = [IR.select(row, np.arange(w["lists"], dtype=np.int64), nprobe) for row in w["coarse_all"]]
    return np.stack([p[0] for p in picks]), np.stack([p[1] for p in picks])


def _search(w, k, nprobe, shortlist, rescore=None):
    probes, coarse = _probes(w, nprobe)
    return RR.search(w["pq_codes"], w["members"], w["n"], w["offsets"], w["table"], coarse, probes, w["fine_codes"], w["fine_scales"],
                     w["queries"], k, shortlist, rescore, rows=w["rows"]) + (probes,)


def test_properties_b_and_c_hold_for_the_restatement():
    """(b): where scanned <= S the refined row is the int8 IVF search's row; (c): where scanned <= R the rescored row is the fp32 IVF
    search's row -- ids, score bits and padding."""
    w = _world()
    exact = PR.chain(w["queries"], w["rows"])
    seen = {"b": 0, "c": 0, "short": 0}
    for nprobe, k, s, r in ((1, 10, 80, 60), (2, 30, 120, 110), (6, 50, 323, 323), (3, 20, 400, 20), (2, 5, 40, 5)):
        ids, sc, scanned, probes = _search(w, k, nprobe, s)
        want8 = LI.search(w["labels"], w["lists"], probes, w["rows"], w["queries"], k)
        assert scanned.tolist() == want8[2].tolist()
        ids_r, sc_r, _, _ = _search(w, k, nprobe, s, r)
        want32 = IR.search_labels(w["labels"], w["lists"], probes, exact, k)
        for q in range(len(ids)):
            if scanned[q] <= s:
                IR.same_bits(ids[q], want8[0][q]), IR.same_bits(sc[q], want8[1][q])
                seen["b"] += 1
            else:
                seen["short"] += 1
            if scanned[q] <= r:
                IR.same_bits(ids_r[q], want32[0][q]), IR.same_bits(sc_r[q], want32[1][q])
                seen["c"] += 1
            # (a): every refined score is the int8 index's at its id; every rescored one the exact chain's
            have = ids[q] >= 0
            IR.same_bits(sc[q][have], LI.i8_scores(w["rows"], w["queries"])[q][ids[q][have]])
            have = ids_r[q] >= 0
            IR.same_bits(sc_r[q][have], exact[q][ids_r[q][have]])
    assert min(seen.values()) > 0, seen


def test_planted_near_duplicates_lead_the_refined_row():
    """The restatement alone, on lists_i8_restatement.planted() with every list probed and S = n: the ``copies`` near-duplicates of
    each planted query are the first ``copies`` ids of its refined row (as a set: the order among them is the int8 ranking's)."""
    planted_queries, copies, lists = 3, 5, 6
    w = _world(lists=lists)
    n, d = w["rows"].shape
    rng = np.random.default_rng(39)                                           # the draws of planted() up to the planted ids
    rng.standard_normal((len(w["queries"]), d)), rng.standard_normal((n, d))
    where = rng.permutation(n)[:planted_queries * copies].reshape(planted_queries, copies)
    cosines = w["queries"].astype(np.float64) @ w["rows"].astype(np.float64).T
    assert all(cosines[q, where[q]].min() > 0.9 > np.delete(cosines[q], where[q]).max() for q in range(planted_queries))
    ids, sc, scanned, _ = _search(w, copies + 5, lists, n)
    assert scanned.tolist() == [n] * len(ids)
    for q in range(planted_queries):
        assert sorted(ids[q, :copies].tolist()) == sorted(where[q].tolist()), (q, ids[q], where[q])
