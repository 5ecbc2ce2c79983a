"""The int8 lists of the inverted file (include/mdx_lists_i8.h; mdir_amd/ivf.py, storage="i8") on a CPU-only box: the census of
include/mdx_lists_i8.h, every refusal of the C ABI with nothing launched, the Python checks of the ops wrappers and of ivf.IVFIndex, and
the restatement (tests/lists_i8_restatement.py) checked against a brute-force loop, with the planted data of the GPU test."""
import ctypes
import os
import re

import numpy as np
import pytest

import ivf_restatement as IR
import lists_i8_restatement as LR
from conftest import ROOT

NEW = ("mdx_lists_i8_encode", "mdx_lists_i8_bounds", "mdx_lists_i8_scan")
F32 = np.float32


def _declared():
    """The code of include/mdx_lists_i8.h, which mdx.h includes for its section "inverted file, int8 lists"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_lists_i8.h"$', text, flags=re.M) and "inverted file, int8 lists" in text
    assert text.index('#include "mdx_ivf.h"') < text.index('#include "mdx_lists_i8.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_lists_i8.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LISTS_I8_EXPORTS) == set(NEW)
    assert all(name.startswith("mdx_lists_i8_") and "ivf" not in name and "kmeans" not in name for name in declared)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS)
              | set(_lib.IVF_EXPORTS))
    assert not declared & others and not {n for n in others if n.startswith("mdx_lists_i8")}
    # the prototypes of mdx.h itself are pinned by tests/test_cabi.py: none of these is written there
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_lists_i8_[a-z0-9_]+\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert re.search(r"int\s+mdx_lists_i8_encode\s*\(\s*const float \*rows,\s*int64_t n,\s*int64_t d,\s*int64_t ld,\s*const int64_t \*members,"
                     r"\s*int64_t m,\s*int8_t \*codes,\s*float \*scales,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_lists_i8_bounds\s*\(\s*const int8_t \*codes,\s*const float \*scales,\s*int64_t m,\s*int64_t d,"
                     r"\s*mdx_i8_bounds \*bounds,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_lists_i8_scan\s*\(\s*const int8_t \*codes,\s*const float \*scales,\s*int64_t m,\s*int64_t d,"
                     r"\s*const int64_t \*members,\s*const int64_t \*offsets,\s*int64_t K,\s*const int8_t \*qcodes,\s*const float \*qscales,"
                     r"\s*int64_t nq,\s*int64_t nprobe,\s*const void \*plan,\s*int64_t plan_bytes,\s*int64_t cap,\s*int64_t items,"
                     r"\s*float \*cand_scores,\s*int64_t \*cand_ids,\s*void \*stream\s*\)", code)
    for word in ("certified[q]", "Proof", "REPEATED", "Refusals", "16-byte aligned", "133 120"):
        assert word in open(os.path.join(ROOT, "include", "mdx_lists_i8.h")).read(), word
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_lists_i8\.hip\b", makefile, flags=re.M) and "include/mdx_lists_i8.h" in makefile
    assert '"mdx_lists_i8.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "lists_i8" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_lists_i8_memcontract import CASES, COVERED
    assert {"mdx_" + entry for entry in COVERED} == set(NEW)
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry


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

    def storage(call, name):
        """The refusals the three calls share: the sizes and the alignment of the codes."""
        for kw in ({"m": 0}, {"m": -2}, {"d": 0}, {"m": 1 << 31}):
            refused(call(**kw), name, "must be >= 1 and m below 2^31")
        for d in (133121, 1 << 31, 1 << 40):
            refused(call(d=d), name, "d=%d too large" % d)
        for off in (1, 4, 8):
            refused(call(codes=ctypes.c_void_p((1 << 20) + off)), name, "codes must be 16-byte aligned")

    def encode(rows=p, n=100, d=8, ld=None, members=q, m=100, codes=p, scales=q):
        return h.mdx_lists_i8_encode(rows, n, d, d if ld is None else ld, members, m, codes, scales, None)
    name = "mdx_lists_i8_encode"
    for kw in ({"rows": None}, {"members": None}, {"codes": None}, {"scales": None}):
        refused(encode(**kw), name, "NULL")
    for n in (0, -1, 1 << 31):
        refused(encode(n=n), name, "n=")
    storage(encode, name)
    refused(encode(ld=7), name, "ld=7 < d=8")
    refused(encode(n=1 << 30, ld=1 << 40), name, "overflows")
    assert encode(d=133120, ld=133119) == -1                               # the largest d passes the size check

    def bounds(codes=p, scales=q, m=100, d=8, out=q):
        return h.mdx_lists_i8_bounds(codes, scales, m, d, out, None)
    name = "mdx_lists_i8_bounds"
    for kw in ({"codes": None}, {"scales": None}, {"out": None}):
        refused(bounds(**kw), name, "NULL")
    storage(bounds, name)

    need = h.mdx_ivf_plan_workspace(5, 2, 6)

    def scan(codes=p, scales=q, m=100, d=8, members=q, offsets=q, k=6, qcodes=p, qscales=q, nq=5, nprobe=2, wsp=ws, wsb=None, cap=50,
             items=10, cs=q, ci=q):
        return h.mdx_lists_i8_scan(codes, scales, m, d, members, offsets, k, qcodes, qscales, nq, nprobe, wsp,
                                   h.mdx_ivf_plan_workspace(nq, nprobe, k) if wsb is None else wsb, cap, items, cs, ci, None)
    name = "mdx_lists_i8_scan"
    for kw in ({"codes": None}, {"scales": None}, {"members": None}, {"offsets": None}, {"qcodes": None}, {"qscales": None}, {"cs": None},
               {"ci": None}):
        refused(scan(**kw), name, "NULL")
    storage(scan, name)
    for items in (0, -1, 1 << 31):
        refused(scan(items=items), name, "items=")
    # the sizes of the plan, the plan itself and cap: as the three calls of mdx_ivf.h refuse them
    for kw in ({"nq": 0}, {"nprobe": 0}, {"k": 0}, {"nq": -3}):
        refused(scan(**kw), name, "must be >= 1")
    for kw in ({"nprobe": 7}, {"nq": 1 << 31}, {"k": 1 << 31}, {"nq": 1 << 20, "nprobe": 1 << 11, "k": 1 << 12}):
        refused(scan(**kw), name, "too large")
    refused(scan(wsb=need - 1), name, "workspace", code=-4)
    refused(scan(wsp=None), name, "workspace", code=-4)
    for off in (4, 8):
        refused(scan(wsp=ctypes.c_void_p((1 << 24) + off)), name, "16-byte aligned")
    for cap in (0, -1, 1 << 31):
        refused(scan(cap=cap), name, "cap=")
    refused(scan(nq=1 << 22, cap=1 << 20), name, "too large for one launch")


def test_ops_checks_need_no_gpu(monkeypatch):
    import torch
    from mdir_amd import ops
    rows, members, offsets = torch.zeros((10, 4)), torch.zeros(10, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)
    codes, scales = torch.zeros((10, 64), dtype=torch.int8), torch.zeros(10)
    qcodes, qscales = torch.zeros((3, 4), dtype=torch.int8), torch.zeros(3)
    up = lambda b: (b + 255) // 256 * 256
    plan = torch.zeros(2 * up(8 * 3 * 2) + up(8 * 3) + 2 * up(8 * 7) + up(16 * 6), dtype=torch.uint8)
    scan = lambda *a, **kw: ops.lists_i8_scan(*a, **kw)
    good = [codes, scales, 4, members, offsets, qcodes, qscales, plan, 2, 5, 4]
    for call, word in ((lambda: ops.lists_i8_encode(rows, members), "rows"), (lambda: ops.lists_i8_bounds(codes, scales, 4), "codes"),
                       (lambda: scan(*good), "codes"), (lambda: ops.lists_i8_encode(None, members), "rows")):
        with pytest.raises(ValueError, match="%s must be a CUDA" % word):
            call()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    # lists_i8_encode
    with pytest.raises(ValueError, match="rows must be torch.float32"):
        ops.lists_i8_encode(rows.double(), members)
    with pytest.raises(ValueError, match="rows must be a matrix with contiguous rows"):
        ops.lists_i8_encode(torch.zeros((4, 10)).t(), members)
    with pytest.raises(ValueError, match="members must be torch.int64"):
        ops.lists_i8_encode(rows, members.int())
    with pytest.raises(ValueError, match="members must be a contiguous"):
        ops.lists_i8_encode(rows, torch.zeros(20, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="d = 133121 > 133120"):
        ops.lists_i8_encode(torch.zeros((1, 133121)), members[:1])
    # lists_i8_bounds: the storage
    with pytest.raises(ValueError, match="codes must be torch.int8"):
        ops.lists_i8_bounds(codes.int(), scales, 4)
    with pytest.raises(ValueError, match="codes must be a contiguous \\[10, 64\\]"):
        ops.lists_i8_bounds(torch.zeros((10, 128), dtype=torch.int8), scales, 4)
    with pytest.raises(ValueError, match="codes must be a contiguous \\[10, 128\\]"):
        ops.lists_i8_bounds(codes, scales, 65)
    with pytest.raises(ValueError, match="scales must be torch.float32"):
        ops.lists_i8_bounds(codes, scales.double(), 4)
    with pytest.raises(ValueError, match="scales must be a contiguous \\[10\\]"):
        ops.lists_i8_bounds(codes, scales[:9], 4)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="d must be an integer >= 1"):
            ops.lists_i8_bounds(codes, scales, bad)
    with pytest.raises(ValueError, match="d = 133121 > 133120"):
        ops.lists_i8_bounds(codes, scales, 133121)

    # lists_i8_scan
    def with_(at, value):
        args = list(good)
        args[at] = value
        return args
    with pytest.raises(ValueError, match="qcodes must be torch.int8"):
        scan(*with_(5, qcodes.float()))
    with pytest.raises(ValueError, match="query dimension 5 != rows dimension 4"):
        scan(*with_(5, torch.zeros((3, 5), dtype=torch.int8)))
    with pytest.raises(ValueError, match="qcodes must be a contiguous"):
        scan(*with_(5, torch.zeros((3, 8), dtype=torch.int8)[:, :4]))
    with pytest.raises(ValueError, match="qscales must be a contiguous \\[3\\]"):
        scan(*with_(6, torch.zeros(4)))
    with pytest.raises(ValueError, match="members must be torch.int64"):
        scan(*with_(3, members.int()))
    with pytest.raises(ValueError, match="members must be a contiguous \\[10\\]"):
        scan(*with_(3, members[:9]))
    with pytest.raises(ValueError, match="offsets must be a non-empty 1-d"):
        scan(*with_(4, offsets.reshape(1, 7)))
    for at, what in ((8, "nprobe"), (9, "cap"), (10, "items")):
        for bad in (0, 1.5, True):
            with pytest.raises(ValueError, match="%s must be an integer >= 1" % what):
                scan(*with_(at, bad))
    with pytest.raises(ValueError, match="plan must be torch.uint8"):
        scan(*with_(7, plan.float()))
    with pytest.raises(ValueError, match="nprobe must be in \\[1, K\\]"):
        scan(*with_(8, 7))


def test_index_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivf, ops
    rows, cents = torch.zeros((10, 4)), torch.zeros((3, 4))
    assert ivf.IVFRescored._fields == ("ids", "scores", "probes", "scanned", "certified", "fallback")
    assert ivf.IVFResult._fields == ("ids", "scores", "probes", "scanned")
    for doc_word in ("storage=\"i8\"", "lists_i8_encode", "lists_i8_bounds", "lists_i8_scan", "ops.rescore", "ops.rescore_certify", "certified[q]",
                     "scanned[q] <= S", "exact=True", "one read-back", "include/mdx_lists_i8.h"):
        assert doc_word in ivf.__doc__, doc_word
    for bad in ("f16", "int8", None, 8):
        with pytest.raises(ValueError, match="storage .* \\(\"f32\" or \"i8\"\\)"):
            ivf.IVFIndex(rows, cents, storage=bad)
        with pytest.raises(ValueError, match="storage .* \\(\"f32\" or \"i8\"\\)"):
            ivf.IVFIndex.train(rows, 3, storage=bad)
    with pytest.raises(ValueError, match="rows must be a CUDA"):                 # a good storage gets as far as the device check
        ivf.IVFIndex(rows, cents, torch.zeros(10, dtype=torch.int64), storage="i8")
    # search: indexes built without a device (the checks come before any device work)
    q = torch.zeros((2, 4))

    def bare(storage):
        index = ivf.IVFIndex.__new__(ivf.IVFIndex)
        index.rows, index.d, index.lists, index.coarse, index.storage = rows, 4, 3, object(), storage
        return index
    f32 = bare("f32")
    for kw in ({"shortlist": 10}, {"exact": True}, {"shortlist": 10, "exact": True}):
        with pytest.raises(ValueError, match="shortlist and exact need an int8 index"):
            f32.search(q, 1, 1, **kw)
    with pytest.raises(ValueError, match="queries must be a CUDA"):              # without them an f32 index goes on as before
        f32.search(q, 1, 1)
    i8 = bare("i8")
    for args, kw, word in (((q, 5, 1), {"shortlist": 4}, "shortlist = 4 must be in \\[k = 5, 4096\\]"),
                           ((q, 5, 1), {"shortlist": ops.RESCORE_MAX_K + 1}, "shortlist = 4097 must be in \\[k = 5, 4096\\]"),
                           ((q, 5, 1), {"shortlist": 0}, "shortlist must be an integer >= 1"),
                           ((q, 5, 1), {"shortlist": 8.0}, "shortlist must be an integer >= 1"),
                           ((q, 5, 1), {"shortlist": True}, "shortlist must be an integer >= 1"),
                           ((q, 5, 1), {"exact": True}, "exact=True needs a shortlist"),
                           ((q, 5, 1), {"shortlist": 8, "exact": 1}, "exact must be a bool"),
                           ((q, 0, 1), {"shortlist": 8}, "k must be an integer >= 1"),
                           ((q, 5, 4), {"shortlist": 8}, "nprobe = 4 > 3 lists"),
                           ((q, 5, 1), {"shortlist": 5}, "queries must be a CUDA"),
                           ((q, 5, 1), {"shortlist": 4096, "exact": True}, "queries must be a CUDA")):
        with pytest.raises(ValueError, match=word):
            i8.search(*args, **kw)
    # the chunk counts the extra buffers of an int8 index
    i8._capacity, f32._capacity = [0, 130], [0, 130]
    assert f32.query_chunk(1) == ivf.CANDIDATE_MEMORY_CAP // (12 * 130)
    assert i8.query_chunk(1) == ivf.CANDIDATE_MEMORY_CAP // (12 * 130 + 5 * 4 + 4)
    assert i8.query_chunk(1, 1000) == ivf.CANDIDATE_MEMORY_CAP // (12 * 130 + 5 * 4 + 4 + 28 * 1000 + 8)


# ------------------------------------------------------------------------------------------------ the restatement itself

def _brute(labels, lists, probes, rows, queries, k, shortlist, center):
    """Python loops and sorted(): per query the candidates, the first ``shortlist`` by (key of the int8 score, id), those by (key of
    the chain score, id), and U_q against which the depth is counted."""
    from oracle import chain as OC
    from test_rescore_host import bounds_np, upper_np
    n, d = rows.shape
    xq = LR.centred(queries, center)
    s8 = LR.i8_scores(rows, queries, center)
    exact = OC.gemm_nt_chain(xq, rows)
    out = []
    for q, row in enumerate(probes):
        cand = []
        for l in row:
            cand += [i for i in range(n) if labels[i] == l]
        first = sorted(cand, key=lambda i: (OC.desc_key(s8[q, i]), i))
        if shortlist is None:
            ids = first[:k]
            out.append((ids + [-1] * (k - len(ids)), [s8[q, i] for i in ids] + [np.nan] * (k - len(ids)), len(cand), None))
            continue
        short = first[:shortlist]
        ranked = sorted(short, key=lambda i: (OC.desc_key(exact[q, i]), i))
        if len(cand) <= shortlist:
            depth = shortlist
        else:
            u = upper_np(F32([s8[q, short[-1]]]), xq[q:q + 1], bounds_np(rows), d)[0]
            depth = 0
            while not np.isnan(u) and depth < len(ranked) and float(exact[q, ranked[depth]]) > u:
                depth += 1
        ids = ranked[:k]
        out.append((ids + [-1] * (k - len(ids)), [exact[q, i] for i in ids] + [np.nan] * (k - len(ids)), len(cand), depth))
    return out


def test_restatement_equals_a_brute_force_loop_and_its_certificate_is_sound():
    from oracle import chain as OC
    rng = np.random.default_rng(2)
    certified_some = 0
    for trial in range(12):
        n, d, nq, lists = int(rng.integers(20, 120)), int(rng.integers(1, 70)), int(rng.integers(1, 6)), int(rng.integers(2, 7))
        rows = rng.standard_normal((n, d)).astype(F32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(F32)
        queries = rows[rng.integers(0, n, nq)] + F32(0.1) * rng.standard_normal((nq, d)).astype(F32)
        rows[rng.integers(0, n)] = rows[rng.integers(0, n)]                  # a duplicate row: equal scores on both stages
        rows[rng.integers(0, n)] = 0                                         # and an all-zero one
        center = (F32(0.01) * rng.standard_normal(d)).astype(F32) if trial % 2 else None
        labels = rng.integers(0, lists - 1, n)                               # the last list stays empty
        for nprobe in (1, lists):
            probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)])
            k = int(rng.integers(1, 12))
            exact = OC.gemm_nt_chain(LR.centred(queries, center), rows)
            f32_ids, f32_sc, f32_n = IR.search_labels(labels, lists, probes, exact, k)
            for shortlist in (None, k, k + int(rng.integers(1, 30))):
                ids, sc, scanned, certified = LR.search(labels, lists, probes, rows, queries, k, shortlist, center)
                want = _brute(labels, lists, probes, rows, queries, k, shortlist, center)
                IR.same_bits(ids, np.array([w[0] for w in want], np.int64)), IR.same_bits(sc, np.array([w[1] for w in want], F32))
                IR.same_bits(scanned, np.array([w[2] for w in want], np.int64)), IR.same_bits(scanned, f32_n)
                if shortlist is None:
                    assert certified is None
                    continue
                assert certified.tolist() == [w[3] for w in want]
                for q in range(nq):
                    c = min(int(certified[q]), k)
                    IR.same_bits(ids[q, :c], f32_ids[q, :c]), IR.same_bits(sc[q, :c], f32_sc[q, :c])   # the contract
                    if scanned[q] <= shortlist:
                        assert certified[q] == shortlist
                        IR.same_bits(ids[q], f32_ids[q]), IR.same_bits(sc[q], f32_sc[q])               # padding included
                    else:
                        assert certified[q] < shortlist       # the entry whose int8 score is t_q has a chain score <= U_q
                    certified_some += int(scanned[q] > shortlist and certified[q] > 0)
    assert certified_some > 20, certified_some                               # the certificate is not vacuous


def test_planted_data_certify_as_deep_as_the_gpu_test_expects():
    """The data of test_gpu_lists_i8.py's certificate tests, evaluated in numpy: n = 323, d = 64, unit rows, S = 16, all lists probed.
    U_q against all 323 rows certifies 12, 9 and 11 entries of the three planted queries -- their five near-duplicates and more."""
    rows, queries, labels, _ = LR.planted()
    lists = 6
    assert rows.shape == (323, 64) and np.allclose(np.linalg.norm(rows, axis=1), 1, atol=1e-6)
    probes = np.tile(np.arange(lists), (len(queries), 1))
    ids, sc, scanned, certified = LR.search(labels, lists, probes, rows, queries, 5, 16)
    assert scanned.tolist() == [323] * len(queries)
    assert certified[:3].tolist() == [12, 9, 11]
    exact = LR.centred(queries).astype(np.float64) @ rows.astype(np.float64).T
    for q in range(3):                                                       # the five near-duplicates lead, 0.97 and above
        assert np.sort(exact[q])[-5] > 0.96 and np.sort(exact[q])[-6] < 0.5
        assert set(ids[q].tolist()) == set(np.argsort(-exact[q])[:5].tolist())
    # k = S < scanned: nobody is certified to depth S
    _, _, _, all_of_it = LR.search(labels, lists, probes, rows, queries, 16, 16)
    assert (all_of_it < 16).all() and all_of_it.tolist() == certified.tolist()
