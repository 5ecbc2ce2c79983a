"""The product-quantised lists of the inverted file (include/mdx_lists_pq.h; mdir_amd/pq.py, mdir_amd/ivfpq.py) on a CPU-only box: the
census of include/mdx_lists_pq.h, every refusal of the C ABI with nothing launched, the Python refusals that need no device, and the
restatement (tests/pq_restatement.py) checked against brute-force loops on tiny data."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ivf_restatement as IR
import pq_restatement as PR
from conftest import ROOT

NEW = ("mdx_pq_lut", "mdx_lists_pq_scan")
F32 = np.float32


def _declared():
    """The code of include/mdx_lists_pq.h, which mdx.h includes for its section "inverted file, product-quantised lists"."""
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_lists_pq.h"$', text, flags=re.M) and "inverted file, product-quantised lists" in text
    assert text.index('#include "mdx_lists_i8.h"') < text.index('#include "mdx_lists_pq.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_lists_pq.h")).read(), flags=re.S)


def test_header_exports_and_library_agree():
    from mdir_amd import _lib, ops
    code = _declared()
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LISTS_PQ_EXPORTS) == set(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.KNN_JOIN_EXPORTS) | set(_lib.TRUNK_F16_EXPORTS) | set(_lib.GROUPS_EXPORTS)
              | set(_lib.KRECIP_EXPORTS) | set(_lib.PHOTOMETRIC_EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.KMEANS_EXPORTS)
              | set(_lib.IVF_EXPORTS) | set(_lib.LISTS_I8_EXPORTS))
    assert not declared & others and not {n for n in others if "_pq" in n}
    # the prototypes of mdx.h itself are pinned by tests/test_cabi.py: none of these is written there
    mdx_h = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert not re.search(r"\bmdx_(pq|lists_pq)_[a-z0-9_]+\s*\(", re.sub(r"/\*.*?\*/", "", mdx_h, flags=re.S))
    assert re.search(r"int\s+mdx_pq_lut\s*\(\s*const float \*codewords,\s*int64_t M,\s*int64_t dsub,\s*const float \*queries,\s*int64_t nq,"
                     r"\s*int qlayout,\s*const float \*center,\s*float \*lut,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_lists_pq_scan\s*\(\s*const uint8_t \*codes,\s*int64_t m,\s*int64_t M,\s*int64_t ldc,\s*const int64_t \*members,"
                     r"\s*int64_t n,\s*const int64_t \*offsets,\s*int64_t K,\s*const float \*lut,\s*const float \*coarse,"
                     r"\s*const int64_t \*probes,\s*int64_t nq,\s*int64_t nprobe,\s*const void \*plan,\s*int64_t plan_bytes,\s*int64_t cap,"
                     r"\s*float \*cand_scores,\s*int64_t \*cand_ids,\s*void \*stream\s*\)", code)
    header = open(os.path.join(ROOT, "include", "mdx_lists_pq.h")).read()
    for word in ("Refusals", "ldc", "never interpreted", "in that order", "Launch shape", "legal under stream capture"):
        assert word in header, word
    assert int(re.search(r"#define MDX_PQ_MAX_M (\d+)", code).group(1)) == ops.PQ_MAX_M == 128
    assert int(re.search(r"#define MDX_PQ_CODEWORDS (\d+)", code).group(1)) == ops.PQ_CODEWORDS == PR.CODEWORDS == 256
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_lists_pq\.hip\b", makefile, flags=re.M) and "include/mdx_lists_pq.h" in makefile
    assert '"mdx_lists_pq.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", mdx_h).group(1)) == 3
    _lib.build()
    h = _lib.lib()
    bound = _lib._declare(h)                                            # every name of the table resolves in the library
    for name in NEW:
        assert name in bound and hasattr(h, name) and getattr(h, name).argtypes is not None
    stray = {n for n in bound if "_pq" in n} - set(NEW)
    assert not stray, stray
    assert h.mdx_abi_version() == 3 == _lib.ABI_VERSION


def test_every_launching_entry_point_has_memory_contract_cases():
    from test_gpu_lists_pq_memcontract import CASES, COVERED
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

    def lut(words=p, m=4, dsub=8, queries=q, nq=5, lay=1, center=None, out=q):
        return h.mdx_pq_lut(words, m, dsub, queries, nq, lay, center, out, None)
    name = "mdx_pq_lut"
    for kw in ({"words": None}, {"queries": None}, {"out": None}):
        refused(lut(**kw), name, "NULL")
    for m in (0, -1, 129, 1 << 31):
        refused(lut(m=m), name, "M=%d must be in [1, 128]" % m)
    for kw in ({"dsub": 0}, {"nq": 0}, {"nq": -4}):
        refused(lut(**kw), name, "must be >= 1")
    for kw in ({"dsub": 1 << 31}, {"m": 128, "dsub": 1 << 24}, {"nq": 1 << 31}, {"m": 128, "nq": (1 << 31) - 1}):
        refused(lut(**kw), name, "too large")
    for lay in (-1, 2, 7):
        refused(lut(lay=lay), name, "qlayout %d" % lay)

    need = h.mdx_ivf_plan_workspace(5, 2, 6)

    def scan(codes=p, m=100, sub=4, ldc=None, members=q, n=100, offsets=q, k=6, table=p, coarse=q, probes=q, nq=5, nprobe=2, wsp=ws, wsb=None,
             cap=50, cs=q, ci=q):
        return h.mdx_lists_pq_scan(codes, m, sub, sub if ldc is None else ldc, members, n, offsets, k, table, coarse, probes, nq, nprobe, wsp,
                                   h.mdx_ivf_plan_workspace(nq, nprobe, k) if wsb is None else wsb, cap, cs, ci, None)
    name = "mdx_lists_pq_scan"
    for kw in ({"codes": None}, {"members": None}, {"offsets": None}, {"table": None}, {"coarse": None}, {"probes": None}, {"cs": None},
               {"ci": None}):
        refused(scan(**kw), name, "NULL")
    for sub in (0, -1, 129):
        refused(scan(sub=sub), name, "M=%d must be in [1, 128]" % sub)
    for kw in ({"m": 0}, {"n": 0}, {"m": 1 << 31}, {"n": 1 << 31}, {"n": -5}):
        refused(scan(**kw), name, "must be in [1, 2^31)")
    for ldc in (3, 0, 1 << 31):
        refused(scan(ldc=ldc), name, "ldc=%d must be in [M=4, 2^31)" % ldc)
    # the sizes of the plan, the plan itself and cap: as the calls of mdx_ivf.h refuse them
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


def test_python_refusals_need_no_gpu():
    import torch
    from mdir_amd import ivfpq, ops, pq
    assert pq.Codebook._fields == ("codewords", "history", "iterations")
    assert ivfpq.IVFPQResult._fields == ("ids", "scores", "probes", "scanned")
    vectors = torch.zeros((300, 12))
    # D % M != 0, M outside [1, 128], T < 256, a CPU tensor
    with pytest.raises(ValueError, match="D = 12 is not a multiple of m = 5"):
        pq.train(vectors, 5)
    for bad in (0, -1, 129, 2.0, True):
        with pytest.raises(ValueError, match="m must be an integer >= 1|m must be in \\[1, 128\\]"):
            pq.train(torch.zeros((300, 258)), bad)
    with pytest.raises(ValueError, match="T = 255 vectors: at least 256"):
        pq.train(vectors[:255], 3)
    with pytest.raises(ValueError, match="train_rows = 255 must be in \\[256, T = 300\\]"):
        pq.train(vectors, 3, train_rows=255)
    with pytest.raises(ValueError, match="vectors must be a CUDA"):
        pq.train(vectors, 3)
    words = torch.zeros((3, 256, 4))
    with pytest.raises(ValueError, match="vectors must be a CUDA"):
        pq.encode(pq.Codebook(words, [], 0), vectors)
    with pytest.raises(ValueError, match="codewords must be a contiguous fp32 \\[M, 256, dsub\\]"):
        pq.encode(torch.zeros((3, 255, 4)), vectors)
    with pytest.raises(ValueError, match="vectors are \\[T, 12\\] and the codebook covers M \\* dsub = 3 \\* 5"):
        pq.encode(torch.zeros((3, 256, 5)), vectors)
    with pytest.raises(ValueError, match="codes must be a uint8 \\[T, 3\\]"):
        pq.decode(words, torch.zeros((10, 4), dtype=torch.uint8))
    assert pq.decode(words, torch.zeros((10, 3), dtype=torch.uint8)).shape == (10, 12)          # a gather: runs where the tensors are
    # the index: the same refusals before the partition is built, and the device check of the partition
    cents = torch.zeros((3, 12))
    with pytest.raises(ValueError, match="D = 12 is not a multiple of m = 5"):
        ivfpq.IVFPQIndex(vectors, cents, m=5)
    with pytest.raises(ValueError, match="m must be in \\[1, 128\\]"):
        ivfpq.IVFPQIndex(torch.zeros((300, 258)), torch.zeros((3, 258)), m=129)
    with pytest.raises(ValueError, match="N = 255 rows: pq.train needs at least 256"):
        ivfpq.IVFPQIndex(vectors[:255], cents, m=3)
    with pytest.raises(ValueError, match="the codebook is \\[3, 256, 5\\]"):
        ivfpq.IVFPQIndex(vectors, cents, m=3, codebook=torch.zeros((3, 256, 5)))
    with pytest.raises(ValueError, match="rows must be a CUDA"):
        ivfpq.IVFPQIndex(vectors, cents, torch.zeros(300, dtype=torch.int64), m=3, codebook=words)
    with pytest.raises(ValueError, match="D = 12 is not a multiple of m = 5"):
        ivfpq.IVFPQIndex.train(vectors, 3, m=5)
    # search: an index built without a device (the checks come before any device work)
    q = torch.zeros((2, 12))

    def bare(keep_rows):
        index = ivfpq.IVFPQIndex.__new__(ivfpq.IVFPQIndex)
        index.rows, index.d, index.lists, index.coarse, index.m, index.device = vectors if keep_rows else None, 12, 3, object(), 3, q.device
        return index
    kept, dropped = bare(True), bare(False)
    with pytest.raises(ValueError, match="a shortlist is rescored on the fp32 rows; this index was built with keep_rows=False"):
        dropped.search(q, 5, 1, shortlist=8)
    for index in (kept, dropped):
        for args, kw, word in (((q, 5, 1), {"shortlist": 4}, "shortlist = 4 must be in \\[k = 5, 4096\\]"),
                               ((q, 5, 1), {"shortlist": ops.RESCORE_MAX_K + 1}, "shortlist = 4097 must be in \\[k = 5, 4096\\]"),
                               ((q, 5, 1), {"shortlist": 0}, "shortlist must be an integer >= 1"),
                               ((q, 5, 1), {"shortlist": True}, "shortlist must be an integer >= 1"),
                               ((q, 0, 1), {}, "k must be an integer >= 1"),
                               ((q, 4097, 1), {}, "k = 4097 > 4096"),
                               ((q, 5, 4), {}, "nprobe = 4 > 3 lists"),
                               ((q[:, :8], 5, 1), {}, "queries have dimension 8 and the rows 12"),
                               ((q, 5, 1), {"qlayout": "NN"}, "qlayout"),
                               ((q, 5, 1), {}, "queries must be a CUDA")):
            with pytest.raises(ValueError, match=word):
                index.search(*args, **kw)
    with pytest.raises(ValueError, match="queries must be a CUDA"):
        kept.search(q, 5, 1, shortlist=5)
    # the chunk counts the table of a query
    kept._capacity = [0, 130]
    assert kept.query_chunk(1) == ivf_cap() // (12 * 130 + 1024 * 3)
    assert kept.query_chunk(1, 1000) == ivf_cap() // (12 * 130 + 1024 * 3 + 28 * 1000)
    kept.coarse = None
    with pytest.raises(ValueError, match="the index is closed"):
        kept.search(q, 5, 1)
    # the ops wrappers
    for call, word in ((lambda: ops.pq_lut(words, q), "codewords"), (lambda: ops.pq_lut(None, q), "codewords"),
                       (lambda: ops.lists_pq_scan(torch.zeros((10, 3), dtype=torch.uint8), None, 10, None, None, None, None, None, 5), "codes")):
        with pytest.raises(ValueError, match="%s must be a CUDA" % word):
            call()


def ivf_cap():
    from mdir_amd import ivf
    return ivf.CANDIDATE_MEMORY_CAP


# ------------------------------------------------------------------------------------------------ the restatement itself

def _lattice(rng, shape, scale=4):
    """Multiples of 1 / scale in [-2, 2]: every product and every sum below is exact in fp32, in any order."""
    return (rng.integers(-2 * scale, 2 * scale + 1, shape) / scale).astype(F32)


def _nearest(v, words_m):
    """The first codeword at the smallest Euclidean distance from v, in exact rational arithmetic."""
    dist = [sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(v, c)) for c in words_m]
    return dist.index(min(dist))


def test_restatement_equals_a_brute_force_loop():
    rng = np.random.default_rng(4)
    for d, m_sub, t in ((6, 3, 40), (8, 2, 30), (5, 1, 25)):
        dsub = d // m_sub
        words = _lattice(rng, (m_sub, 256, dsub))
        words[:, 200] = words[:, 17]                                            # equal codewords: the smaller id wins
        vectors = _lattice(rng, (t, d))
        vectors[3] = words[:, 200].reshape(-1)                                  # a vector that is a codeword
        codes = PR.encode(words, vectors)
        assert codes.dtype == np.uint8 and codes.shape == (t, m_sub)
        want = [[_nearest(vectors[i, m * dsub:(m + 1) * dsub], words[m]) for m in range(m_sub)] for i in range(t)]
        assert codes.tolist() == want and codes[3].tolist() == [17] * m_sub
        IR.same_bits(PR.decode(words, codes), np.array([[x for m in range(m_sub) for x in words[m][want[i][m]]] for i in range(t)], F32))
        # the table: exact dot products on the lattice; the scan: python loops over probes, members and subspaces
        nq, lists, nprobe = 4, 5, 3
        queries, center = _lattice(rng, (nq, d)), _lattice(rng, (d,))
        table = PR.lut(words, queries, center)
        x = queries.astype(np.float64) - center.astype(np.float64)
        for m in range(m_sub):
            assert np.array_equal(table[:, m], (x[:, m * dsub:(m + 1) * dsub] @ words[m].astype(np.float64).T).astype(F32))
        labels = rng.integers(0, lists - 1, t)                                  # the last list stays empty
        members, offsets = IR.csr(labels, lists)
        members = members.copy()
        members[5] = t + 3                                                      # an id outside the rows: NaN
        probes = np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)])
        probes[1, 0] = lists                                                    # a probe outside the lists owns nothing
        coarse = rng.standard_normal((nq, nprobe)).astype(F32)
        noisy = table + F32(0.01) * rng.standard_normal(table.shape).astype(F32)     # off the lattice: the order of the additions counts
        ids, sc, scanned = PR.search(codes, members, t, offsets, noisy, coarse, probes, 12)
        for q in range(nq):
            cand = []
            for p in range(nprobe):
                l = int(probes[q, p])
                if not 0 <= l < lists:
                    continue
                for pos in range(int(offsets[l]), int(offsets[l + 1])):
                    acc = coarse[q, p]
                    for m in range(m_sub):
                        acc = F32(acc + noisy[q, m, codes[pos, m]])
                    cand.append((int(members[pos]), acc if members[pos] < t else F32(np.nan)))
            assert scanned[q] == len(cand)
            from oracle import chain as OC
            ranked = sorted(cand, key=lambda c: (OC.desc_key(c[1]), c[0]))[:12]
            pad = 12 - len(ranked)
            IR.same_bits(ids[q], np.array([c[0] for c in ranked] + [-1] * pad, np.int64))
            IR.same_bits(sc[q], np.array([c[1] for c in ranked] + [np.nan] * pad, F32))


def test_restated_training_equals_a_brute_force_iteration():
    """One update on lattice data: the first assignment is exact (Euclidean nearest in rationals), the means are sequential fp32 sums
    in member order (every cluster here is shorter than a segment) and one division; an emptied codeword keeps its value."""
    rng = np.random.default_rng(9)
    t, d, m_sub = 300, 6, 3
    dsub = d // m_sub
    vectors = _lattice(rng, (t, d), scale=8)
    _, first = PR.draw(t, 3)
    vectors[first[9]] = vectors[first[2]]                                       # a duplicate initial codeword: id 9 wins nothing
    words, history, updates = PR.train(vectors, m_sub, iters=1, seed=3)
    assert updates == 1 and len(history) == 2 * m_sub and words.shape == (m_sub, 256, dsub) and words.dtype == F32
    for m in range(m_sub):
        sub = vectors[:, m * dsub:(m + 1) * dsub]
        start = sub[first]
        labels = [_nearest(v, start) for v in sub]
        assert 9 not in labels
        for j in range(256):
            mine = [i for i in range(t) if labels[i] == j]
            want = start[j]
            if mine:
                acc = np.zeros(dsub, F32)
                for i in mine:
                    acc = acc + sub[i]
                want = (F32(0) + acc) / F32(len(mine))
            IR.same_bits(words[m, j], want.astype(F32))
    # the sample: sorted ids, and the generator moves on before the initial codewords are drawn
    sample, inside = PR.draw(t, 3, train_rows=280)
    assert len(sample) == 280 and (np.diff(sample) > 0).all() and len(inside) == 256 and inside.max() < 280
    assert PR.draw(t, 3, train_rows=t)[0] is None and not np.array_equal(PR.draw(t, 3, train_rows=t)[1], first)
