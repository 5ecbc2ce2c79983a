"""Exact range search and self-join (include/mdx.h, "exact range search and self-join") on a CPU-only box: the C ABI and its
argument checks, the Python checks, and a float64 restatement of the pruning bound -- shown sound against the oracle's exact
chain: every pair whose chain score reaches tau passes the candidate test."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_i8_host import quantize_np

E = 0.5 + 2.0 ** -15
NEW = ("mdx_center_rows", "mdx_join_stats", "mdx_join_candidates", "mdx_join_resolve_workspace", "mdx_join_resolve",
       "mdx_range_select_workspace", "mdx_range_select")


# ------------------------------------------------------------------ the bound, restated in float64

def row_factors(x):
    """{p, q, r, w} of mdx_join_stats in float64 (no rounding up), +inf for rows the bound does not cover."""
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    c, s = quantize_np(x)
    s64 = s.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l1 = np.abs(x.astype(np.float64)).sum(axis=1)
        a = np.abs(x).max(axis=1).astype(np.float64)
        c1 = np.abs(c.astype(np.int64)).sum(axis=1).astype(np.float64)
    ud = d * 2.0 ** -24
    gamma = ud / (1 - ud)
    # only an all-zero row is covered with scale 0: a nonzero row whose scale rounded to 0 (a subnormal max|x|) is not
    covered = np.isfinite(x).all(axis=1) & ((a == 0) | ((s64 >= 2.0 ** -106) & (s64 <= 2.0 ** 40)))
    q = np.where(covered, E * l1, np.inf)
    r = np.where(covered, E * s64 * c1, np.inf)
    w = np.where(covered, s64 + gamma * a / E, np.inf)
    return s, q, r, w, c


def candidates_np(x, y, tau, symmetric=False):
    """[m, n] bool: the candidate test of include/mdx.h in float64 for rows x (query role) and y (database role)."""
    px, qx, rx, wx, cx = row_factors(x)
    py, qy, ry, wy, cy = row_factors(y)
    d = x.shape[1]
    acc = cx.astype(np.float64) @ cy.astype(np.float64).T
    prod = py[None, :].astype(np.float32) * px[:, None].astype(np.float32)          # scale_B * scale_A in fp32
    with np.errstate(invalid="ignore", over="ignore"):
        s = (acc.astype(np.float32) * prod).astype(np.float64)
        b1 = qx[:, None] * wy[None, :] + ry[None, :] * px[:, None].astype(np.float64) + d * 2.0 ** -149
        b2 = qy[None, :] * wx[:, None] + rx[:, None] * py[None, :].astype(np.float64) + d * 2.0 ** -149
        beta = np.minimum(b1, b2)
        under = (px[:, None] > 0) & (py[None, :] > 0) & (prod < np.float32(2.0 ** -126))
        beta = np.where(under, np.inf, beta)
        lhs = s + 2.0 ** -22 * np.abs(s) + beta
    cand = ~(lhs < tau)                                       # NaN: a candidate
    if symmetric:
        cand &= np.arange(y.shape[0])[None, :] > np.arange(x.shape[0])[:, None]
    return cand


def _sets(rng, kind, n, d):
    if kind == "random":
        x = rng.standard_normal((n, d)).astype(np.float32)
    elif kind == "clustered":
        c = rng.standard_normal((3, d)).astype(np.float32)
        x = (c[rng.integers(0, 3, n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    else:                                                     # adversarial: near ties, duplicates, zero and tiny rows
        base = rng.standard_normal(d).astype(np.float32)
        x = (base[None, :] + 1e-4 * rng.standard_normal((n, d))).astype(np.float32)
        if n >= 6:
            x[1] = x[0]
            x[2] = 0
            x[3] = x[4] * np.float32(2.0 ** -100)
            x[5] = x[4] * np.float32(2.0 ** -60)
        if n >= 8:
            x[6] = 0
            x[6, 0] = np.float32(2.0 ** -145)                 # a subnormal row: its scale rounds to 0
            x[7] = x[4] * np.float32(2.0 ** 40)               # a large row: products with the subnormal one are normal
    if kind == "adversarial":
        return x.astype(np.float32)                            # the scales of the awkward rows stay as they are
    norm = np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return np.where(norm > 0, x / np.maximum(norm, np.float32(1e-38)), x).astype(np.float32)


def test_restated_bound_is_sound():
    from oracle import chain
    rng = np.random.default_rng(17)
    hits, cands, pairs = 0, 0, 0
    for trial in range(240):
        kind = ("random", "clustered", "adversarial")[trial % 3]
        n = int(rng.integers(2, 60))
        d = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 130]))
        y = _sets(rng, kind, n, d)
        x = _sets(rng, kind, int(rng.integers(1, 6)), d) if trial % 2 else y
        exact = chain.gemm_nt_chain(x, y)                     # [m, n] the chain of every pair
        flat = exact[np.isfinite(exact)]
        tiny = flat[(flat > 0) & (flat < 2.0 ** -90)]
        for tau in (float(np.quantile(flat, 0.5)), float(np.quantile(flat, 0.95)), float(flat.max()), float(rng.choice(flat)),
                    float(tiny.min()) if tiny.size else 2.0 ** -99):
            tau = float(np.float32(tau))
            sym = x is y
            cand = candidates_np(x, y, tau, symmetric=sym)
            hit = exact >= np.float32(tau)
            if sym:
                hit &= np.arange(n)[None, :] > np.arange(n)[:, None]
            assert not (hit & ~cand).any(), (trial, kind, d, tau)
            hits += int(hit.sum())
            cands += int(cand.sum())
            pairs += hit.size
    assert hits > 0 and cands < pairs // 2, (hits, cands, pairs)        # the test prunes, and hits exist


def test_restated_rules_for_rows_outside_the_bound():
    x = np.eye(4, 8, dtype=np.float32)
    x[1, 2] = np.inf
    x[2, 3] = np.nan
    x[3] = 0
    x[3, 5] = np.float32(2.0 ** -110)
    _, q, r, w, _ = row_factors(x)
    assert np.isfinite(q[0]) and np.isinf(q[1:]).all() and np.isinf(r[1:]).all() and np.isinf(w[1:]).all()
    cand = candidates_np(x, x, 0.5, symmetric=True)
    assert cand[0, 1:].all() and cand[1, 2:].all()           # uncovered rows are always candidates
    z = np.zeros((2, 8), np.float32)
    assert not candidates_np(z, z, 0.5).any()                 # zero rows score exactly 0


def test_a_subnormal_row_whose_scale_rounds_to_zero_is_never_pruned():
    """x = [2^-145] quantises to scale 0 (127 / a overflows, the code clamps to 127), so its int8 scores are 0, yet
    chain(x, y) = 2^-99 for y = [2^46]: at tau = 2^-99 the pair is a hit."""
    from oracle import chain
    x = np.float32([[2.0 ** -145]])
    y = np.float32([[2.0 ** 46]])
    assert quantize_np(x)[1][0] == 0
    tau = 2.0 ** -99
    assert chain.gemm_nt_chain(x, y)[0, 0] == np.float32(tau)
    assert candidates_np(x, y, tau)[0, 0] and candidates_np(y, x, tau)[0, 0]
    both = np.concatenate([x, y, np.float32([[0.5]]), np.float32([[0.0]])])
    cand = candidates_np(both, both, tau, symmetric=True)
    assert cand[0, 1] and cand[0, 2] and cand[0, 3]                            # the subnormal row reaches the exact stage
    assert not cand[2, 3]                                                      # the zero row is still pruned (score exactly 0)
    _, q, _, _, _ = row_factors(both)
    assert np.isinf(q[0]) and np.isfinite(q[1:]).all()


def test_chain_is_symmetric_in_its_factors():
    from oracle import chain
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 100)).astype(np.float32)
    s = chain.gemm_nt_chain(x, x)
    np.testing.assert_array_equal(s.view(np.uint32), s.T.view(np.uint32))


# ------------------------------------------------------------------ C ABI

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_join_entry_points():
    from mdir_amd import _lib, ops
    code = _declared()
    assert re.search(r"#define MDX_ABI_VERSION 3\b", code)
    assert re.search(r"#define MDX_JOIN_BLOCK 128\b", code) and ops.JOIN_BLOCK == 128
    assert re.search(r"int\s+mdx_join_candidates\s*\(\s*const mdx_index \*a,\s*const float \*stats_a,\s*const mdx_index \*b,"
                     r"\s*const float \*stats_b,\s*int64_t a_lo,\s*int64_t a_hi,\s*int symmetric,\s*float tau,\s*uint64_t \*pairs,"
                     r"\s*int64_t capacity,\s*int64_t \*count,\s*void \*stream\s*\)", code)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS


def test_library_exports_the_join_entry_points():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    for name in NEW:
        assert hasattr(h, name)


def test_workspace_sizes():
    from mdir_amd import _lib
    h = _lib.lib()
    assert h.mdx_join_resolve_workspace(0, 5) == 0 and h.mdx_join_resolve_workspace(5, 0) == 0
    assert h.mdx_join_resolve_workspace(1 << 31, 5) == 0
    assert h.mdx_range_select_workspace(0, 5) == 0 and h.mdx_range_select_workspace(5, -1) == 0
    a, b = h.mdx_join_resolve_workspace(1000, 10), h.mdx_join_resolve_workspace(100000, 10)
    assert 0 < a < b and b >= 100000 * 32
    assert h.mdx_range_select_workspace(10, 0) > 0 and h.mdx_range_select_workspace(10, 1000) < h.mdx_range_select_workspace(10, 10 ** 6)


def test_refusals_before_any_device_work():
    from mdir_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(256)
    big = 1 << 40
    f32 = ctypes.c_float

    assert h.mdx_center_rows(None, 4, 4, 1, None, p, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_center_rows(p, 4, 4, 1, None, None, None) == -1
    assert h.mdx_center_rows(p, 0, 4, 1, None, p, None) == -1 and b">= 1" in h.mdx_last_error()
    assert h.mdx_center_rows(p, 4, 0, 1, None, p, None) == -1
    assert h.mdx_center_rows(p, 4, 4, 5, None, p, None) == -1 and b"layout" in h.mdx_last_error()

    assert h.mdx_join_stats(None, p, 4, p, None) == -1 and b"NULL" in h.mdx_last_error()
    assert h.mdx_join_stats(p, None, 4, p, None) == -1
    assert h.mdx_join_stats(p, p, 4, None, None) == -1

    def cand(a=p, sa=p, b=p, sb=p, lo=0, hi=128, sym=0, tau=0.5, pairs=p, cap=10, count=p):
        return h.mdx_join_candidates(a, sa, b, sb, lo, hi, sym, f32(tau), pairs, cap, count, None)
    for kw in ({"a": None}, {"sa": None}, {"b": None}, {"sb": None}, {"pairs": None}, {"count": None}):
        assert cand(**kw) == -1 and b"NULL" in h.mdx_last_error()
    # the scalar arguments are checked before anything of the handles is read (these are not indexes)
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert cand(tau=bad) == -1 and b"finite" in h.mdx_last_error()
    assert cand(cap=-1) == -1 and b"capacity" in h.mdx_last_error()
    assert cand(sym=1, b=ctypes.c_void_p(512)) == -1 and b"a == b" in h.mdx_last_error()

    def resolve(ra=p, lda=8, rb=p, ldb=8, d=8, pairs=p, P=10, tau=0.5, m_lo=0, m=4, off=p, ids=p, sc=p, ws=p, wsb=big):
        return h.mdx_join_resolve(ra, lda, rb, ldb, d, pairs, P, f32(tau), m_lo, m, off, ids, sc, ws, wsb, None)
    for kw in ({"ra": None}, {"rb": None}, {"pairs": None}, {"off": None}, {"ids": None}, {"sc": None}):
        assert resolve(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"P": 0}, {"m": 0}, {"d": 0}, {"P": -5}):
        assert resolve(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert resolve(P=1 << 31) == -1 and b"2^31" in h.mdx_last_error()
    assert resolve(lda=4) == -1 and b"lda" in h.mdx_last_error()
    assert resolve(m_lo=-1) == -1 and b"m_lo" in h.mdx_last_error()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert resolve(tau=bad) == -1 and b"finite" in h.mdx_last_error()
    assert resolve(ws=None) == -4 and resolve(wsb=16) == -4

    def select(sc=p, m=4, n=8, ld=8, tau=0.5, diag=-1, off=p, ids=p, out=p, cap=10, ws=p, wsb=big):
        return h.mdx_range_select(sc, m, n, ld, f32(tau), diag, off, ids, out, cap, ws, wsb, None)
    for kw in ({"sc": None}, {"off": None}, {"ids": None}, {"out": None}):
        assert select(**kw) == -1 and b"NULL" in h.mdx_last_error()
    for kw in ({"m": 0}, {"n": 0}, {"m": -1}):
        assert select(**kw) == -1 and b">= 1" in h.mdx_last_error()
    assert select(ld=4) == -1 and b"ld=4" in h.mdx_last_error()
    assert select(cap=-1) == -1 and b"capacity" in h.mdx_last_error()
    for bad in (float("nan"), float("inf")):
        assert select(tau=bad) == -1 and b"finite" in h.mdx_last_error()
    assert select(ws=None) == -4 and select(wsb=16) == -4


# ------------------------------------------------------------------ the Python checks

class _FakeIndex:
    storage = "f16"
    n, d = 4, 8


def test_python_checks_need_no_gpu():
    import torch
    from mdir_amd import ops, search
    cpu = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="fp32 device tensor"):
        search.range_search(None, cpu, cpu, 0.5)
    with pytest.raises(ValueError, match="fp32 device tensor"):
        search.self_join(None, cpu, 0.5)
    for bad in (float("nan"), float("inf"), "0.5", True, 1e39):
        with pytest.raises(ValueError, match="threshold"):
            ops._tau(bad)
    assert ops._tau(0.9) == float(np.float32(0.9)) and ops._tau(1) == 1.0
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.center_rows(cpu)
    with pytest.raises(ValueError, match="open DescriptorIndex"):
        ops.join_stats(_FakeIndex(), cpu)
    with pytest.raises(ValueError, match="open DescriptorIndex"):
        ops.join_candidates(_FakeIndex(), cpu, _FakeIndex(), cpu, 0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.range_select(cpu, 0.5)


def test_python_checks_of_the_index_and_sizes(monkeypatch):
    import torch
    from mdir_amd import ops, search
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rows = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="int8 DescriptorIndex"):
        search.self_join(object(), rows, 0.5)
    fake = ops.DescriptorIndex.__new__(ops.DescriptorIndex)
    fake.storage, fake.n, fake.d, fake._h = "f16", 4, 8, None
    with pytest.raises(ValueError, match="int8 index"):
        search.self_join(fake, rows, 0.5)
    fake.storage = "i8"
    fake.n = 5
    with pytest.raises(ValueError, match=r"index's \[5, 8\] rows"):
        search.range_search(fake, rows, rows, 0.5)
    fake.n = 4
    for kw in ({"chunk": 0}, {"chunk": 1.5}, {"max_pairs": 0}, {"max_pairs": True}):
        with pytest.raises(ValueError, match="chunk|max_pairs"):
            search.self_join(fake, rows, 0.5, **kw)
    with pytest.raises(ValueError, match="threshold"):
        search.self_join(fake, rows, float("nan"))
