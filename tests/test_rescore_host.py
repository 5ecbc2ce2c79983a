"""Exact rescoring of int8 shortlists (include/mdx.h mdx_rescore / mdx_index_i8_bounds / mdx_rescore_certify) on a CPU-only
box: the C ABI and its argument checks, the criterion key and overlay, and a float64 restatement of the certificate that
tests/test_gpu_rescore.py compares the device with -- shown sound here against the oracle's exact chain."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_i8_host import quantize_np, scores_np

MAX_K = 4096
E = 0.5 + 2.0 ** -15


# ------------------------------------------------------------------ the certificate, restated in float64

def bounds_np(x):
    """(s_max, s_min, l_max, flag) of mdx_index_i8_bounds for fp32 rows ``x`` [n, d]."""
    c, s = quantize_np(x)
    s64 = s.astype(np.float64)
    bad = ~np.isfinite(s64) | ((s64 > 0) & (s64 < 2.0 ** -106))
    ok = ~bad
    l1 = np.abs(c.astype(np.int64)).sum(axis=1).astype(np.float64)
    s_max = s64[ok].max() if ok.any() else 0.0
    nz = ok & (s64 > 0)
    s_min = s64[nz].min() if nz.any() else np.inf
    l_max = (s64[ok] * l1[ok]).max() if ok.any() else 0.0
    return s_max, s_min, l_max, int(bad.any())


def upper_np(t, xq, bounds, d):
    """U_q of include/mdx.h in float64 (no inflation, no rounding to fp32); NaN where the query gets no certificate.
    ``t`` fp32 [nq], ``xq`` the centred fp32 queries [nq, d]."""
    s_max, s_min, l_max, flag = bounds
    xq = np.asarray(xq, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(xq).max(axis=1) if d else np.zeros(len(xq), np.float32)
        scale_q = (a / np.float32(127.0)).astype(np.float32).astype(np.float64)
        l1 = np.abs(xq.astype(np.float64)).sum(axis=1)
        t = np.asarray(t, np.float32).astype(np.float64)
        ud = d * 2.0 ** -24
        gamma = ud / (1 - ud)
        big = 127.0 * s_max * (1 + 2.0 ** -22) * l1
        u = t + 2.0 ** -22 * np.abs(t) + s_max * E * l1 + l_max * scale_q * E + gamma * big + d * 2.0 ** -149
    void = (flag != 0) | ~np.isfinite(xq).all(axis=1) | ((a > 0) & (a.astype(np.float64) < 2.0 ** -100)) | np.isnan(t) | \
        (s_min * scale_q < 2.0 ** -126) | ~(big < 2.0 ** 126) | (ud >= 0.5) | ~np.isfinite(u)
    return np.where(void, np.nan, u)


def depth_np(sorted_scores, upper, n):
    """Leading entries of each sorted row with score > upper (0 where upper is NaN); K where K == n."""
    nq, K = sorted_scores.shape
    if K == n:
        return np.full(nq, K, np.int64)
    out = np.zeros(nq, np.int64)
    for q in range(nq):
        if np.isnan(upper[q]):
            continue
        above = sorted_scores[q].astype(np.float64) > upper[q]
        out[q] = K if above.all() else int(np.argmin(above))
    return out


def rank_order(scores, ids):
    """``ids`` sorted by mdx_rank_full's order of their ``scores`` (desc_key, then id)."""
    from oracle import chain
    keys = np.array([chain.desc_key(v) for v in np.asarray(scores, np.float32)], np.uint64)
    order = np.lexsort((ids, keys))
    return ids[order], np.asarray(scores, np.float32)[order]


# ------------------------------------------------------------------ C ABI

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_rescore_entry_points():
    from mdir_amd import _lib, ops
    _, code = _declared()
    assert re.search(r"#define MDX_RESCORE_MAX_K 4096\b", code)
    assert re.search(r"int64_t\s+mdx_rescore_workspace\s*\(\s*int64_t nq,\s*int64_t K,\s*int64_t d\s*\)", code)
    assert re.search(r"int\s+mdx_rescore\s*\(\s*const float \*rows,\s*int64_t n,\s*int64_t d,\s*int64_t ld,\s*const float \*queries,"
                     r"\s*int64_t nq,\s*int qlayout,\s*const float \*center,\s*const int64_t \*ids,\s*int64_t K,\s*int64_t \*out_ids,"
                     r"\s*float \*out_scores,\s*void \*workspace,\s*int64_t workspace_bytes,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_index_i8_bounds\s*\(\s*const mdx_index \*index,\s*mdx_i8_bounds \*bounds,\s*void \*stream\s*\)", code)
    assert re.search(r"int\s+mdx_rescore_certify\s*\(", code)
    assert re.search(r"double s_max, s_min, l_max;\s*int32_t flag, reserved;", code)
    assert re.search(r"#define MDX_ABI_VERSION 3\b", code)
    for name in ("mdx_rescore_workspace", "mdx_rescore", "mdx_index_i8_bounds", "mdx_rescore_certify"):
        assert name in _lib.EXPORTS
    assert ops.RESCORE_MAX_K == MAX_K


def test_library_exports_the_rescore_entry_points():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in ("mdx_rescore_workspace", "mdx_rescore", "mdx_index_i8_bounds", "mdx_rescore_certify"):
        assert hasattr(h, name)


def test_rescore_workspace_size():
    from mdir_amd import _lib
    h = _lib.lib()
    for nq in (1, 7, 70, 1000):
        for K in (1, 7, 100, 1000, MAX_K):
            assert h.mdx_rescore_workspace(nq, K, 2048) == -(-4 * nq * K // 256) * 256
    assert h.mdx_rescore_workspace(0, 10, 10) == 0
    assert h.mdx_rescore_workspace(10, 0, 10) == 0
    assert h.mdx_rescore_workspace(10, MAX_K + 1, 10) == 0
    assert h.mdx_rescore_workspace(10, 10, 0) == 0


def test_rescore_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    big = 1 << 30

    def call(rows=p, n=8, d=4, ld=4, q=p, nq=2, lay=1, ids=p, K=3, oi=p, os_=p, ws=p, wsb=big):
        return h.mdx_rescore(rows, n, d, ld, q, nq, lay, None, ids, K, oi, os_, ws, wsb, None)

    for kw in ({"rows": None}, {"q": None}, {"ids": None}, {"oi": None}, {"os_": None}):
        assert call(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"n": 0}, {"d": 0}, {"nq": 0}, {"K": 0}, {"n": -3}):
        assert call(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert call(K=MAX_K + 1) == -1 and b"4096" in h.mdx_last_error()
    assert call(ld=3) == -1 and b"ld=3" in h.mdx_last_error()
    assert call(lay=7) == -1 and b"qlayout" in h.mdx_last_error()
    assert call(ws=None) == -4 and call(wsb=16) == -4


def test_bounds_and_certify_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    assert h.mdx_index_i8_bounds(None, p, None) == -1 and b"NULL" in h.mdx_last_error()

    def call(sc=p, nq=2, K=3, t=p, q=p, d=4, lay=1, b=p, n=10, up=p, dep=p):
        return h.mdx_rescore_certify(sc, nq, K, t, q, d, lay, None, b, n, up, dep, None)

    for kw in ({"sc": None}, {"t": None}, {"q": None}, {"b": None}, {"up": None}, {"dep": None}):
        assert call(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"nq": 0}, {"K": 0}, {"d": 0}, {"n": 0}):
        assert call(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert call(K=11) == -1 and b"K=11" in h.mdx_last_error()
    assert call(K=MAX_K + 1, n=1 << 20) == -1 and b"4096" in h.mdx_last_error()
    assert call(lay=2) == -1 and b"qlayout" in h.mdx_last_error()


# ------------------------------------------------------------------ criterion key and overlay

def _score(tmp_path, **criterion):
    from test_i8_host import _score as make
    return make(tmp_path, **criterion)


def test_criterion_accepts_rescore(tmp_path):
    assert _score(tmp_path, storage="i8", rescore={"shortlist": 100}).rescore == {"shortlist": 100}
    assert _score(tmp_path, storage="f16", rescore={"shortlist": MAX_K}).rescore == {"shortlist": MAX_K}
    assert _score(tmp_path, storage="i8", rescore={"shortlist": 1}, ranking="full").rescore == {"shortlist": 1}
    assert _score(tmp_path, storage="i8").rescore is None


@pytest.mark.parametrize("criterion,match", [
    ({"rescore": {"shortlist": 100}}, "storage is f32"),
    ({"storage": "f32", "rescore": {"shortlist": 100}}, "storage is f32"),
    ({"storage": "i8", "rescore": {"shortlist": 0}}, r"integer in \[1, 4096\]"),
    ({"storage": "i8", "rescore": {"shortlist": 4097}}, r"integer in \[1, 4096\]"),
    ({"storage": "i8", "rescore": {"shortlist": "100"}}, r"integer in \[1, 4096\]"),
    ({"storage": "i8", "rescore": {"shortlist": True}}, r"integer in \[1, 4096\]"),
    ({"storage": "i8", "rescore": {"shortlist": 10.0}}, r"integer in \[1, 4096\]"),
    ({"storage": "i8", "rescore": {"shortlist": 10, "k": 3}}, "exactly the key shortlist"),
    ({"storage": "i8", "rescore": 100}, "exactly the key shortlist"),
    ({"storage": "i8", "rescore": {"shortlist": 10}, "query_expansion": {"k": 2, "alpha": 3.0}}, "query_expansion"),
    ({"storage": "i8", "rescore": {"shortlist": 10}, "database_augmentation": {"k": 2, "alpha": 3.0}}, "database_augmentation"),
    ({"storage": "f16", "rescore": {"shortlist": 10}, "diffusion": {}}, "diffusion"),
])
def test_criterion_refuses_rescore(tmp_path, criterion, match):
    with pytest.raises(ValueError, match=match):
        _score(tmp_path, **criterion)


def test_rescore_refused_in_a_multi_process_run(tmp_path, monkeypatch):
    from mdir_amd import score
    s = _score(tmp_path, storage="i8", rescore={"shortlist": 10})
    monkeypatch.setattr(score, "_world_size", lambda: 2)
    with pytest.raises(ValueError, match="single process"):
        s(None, None, None)


def test_rescore_overlay_parses():
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_int8_rescore.yml")) as f:
        doc = yaml.safe_load(f)
    assert doc["validation"]["247tokyo1k"]["criterion"] == {"storage": "i8", "rescore": {"shortlist": 100}}


# ------------------------------------------------------------------ the restated certificate is sound

def _problem(rng, kind, n, d, nq):
    if kind == "random":
        x = rng.standard_normal((n, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
    elif kind == "clustered":
        centers = rng.standard_normal((3, d)).astype(np.float32)
        x = (centers[rng.integers(0, 3, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
        q = (centers[rng.integers(0, 3, nq)] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    else:                                                 # near ties: every row a hair away from one direction
        base = rng.standard_normal(d).astype(np.float32)
        x = (base[None, :] + 1e-4 * rng.standard_normal((n, d))).astype(np.float32)
        q = (base[None, :] + 1e-3 * rng.standard_normal((nq, d))).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    if n >= 4 and rng.random() < 0.3:
        x[rng.integers(0, n)] = x[rng.integers(0, n)]    # a duplicate row: equal scores go by ascending id
    return x, q


def test_restated_certificate_is_sound():
    from oracle import chain
    rng = np.random.default_rng(11)
    certified, total = 0, 0
    for trial in range(300):
        kind = ("random", "clustered", "near_tie")[trial % 3]
        n, d, nq = int(rng.integers(2, 80)), int(rng.integers(1, 48)), int(rng.integers(1, 5))
        x, q = _problem(rng, kind, n, d, nq)
        K = int(rng.integers(1, n + 1))
        cx, sx = quantize_np(x)
        cq, sq = quantize_np(q)
        s8 = scores_np(cq, sq, cx, sx)
        exact = chain.gemm_nt_chain(q, x)                  # [nq, n], the chain of every pair
        r8 = chain.rank_full(s8)
        rx = chain.rank_full(exact)
        short = r8[:, :K]
        t = s8[np.arange(nq), short[:, -1]]
        res_ids = np.empty((nq, K), np.int64)
        res_sc = np.empty((nq, K), np.float32)
        for i in range(nq):
            res_ids[i], res_sc[i] = rank_order(exact[i, short[i]], short[i])
        u = upper_np(t, q, bounds_np(x), d)
        depth = depth_np(res_sc, u, n)
        for i in range(nq):
            c = depth[i]
            np.testing.assert_array_equal(res_ids[i, :c], rx[i, :c])
            np.testing.assert_array_equal(res_sc[i, :c].view(np.uint32), exact[i, rx[i, :c]].view(np.uint32))
            total += 1
            certified += c > 0
    assert certified > total // 4, (certified, total)       # the certificate is not vacuous


def test_restated_void_rules():
    x = np.eye(6, 8, dtype=np.float32)
    q = np.ones((2, 8), np.float32) / np.float32(np.sqrt(8))
    b = bounds_np(x)
    assert b[3] == 0 and b[0] == np.float32(1) / np.float32(127)
    assert not np.isnan(upper_np(np.float32([0.3, 0.3]), q, b, 8)).any()
    assert np.isnan(upper_np(np.float32([np.nan, 0.3]), q, b, 8))[0]
    xt = x.copy()
    xt[2] = 0
    xt[2, 1] = np.float32(2.0 ** -110)                 # 0 < a < 2^-100: outside the int8 contract
    assert bounds_np(xt)[3] == 1 and np.isnan(upper_np(np.float32([0.3]), q[:1], bounds_np(xt), 8)).all()
    xi = x.copy()
    xi[3, 0] = np.inf
    assert bounds_np(xi)[3] == 1
    qn = q.copy()
    qn[1, 2] = np.nan
    assert np.isnan(upper_np(np.float32([0.3, 0.3]), qn, b, 8)).tolist() == [False, True]
    sc = np.float32([[0.9, 0.5], [0.2, 0.1]])
    assert depth_np(sc, np.array([np.nan, 0.0]), 2).tolist() == [2, 2]         # K == n: every entry
    assert depth_np(sc, np.array([0.6, 0.15]), 5).tolist() == [1, 1]
