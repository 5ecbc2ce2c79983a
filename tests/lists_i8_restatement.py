"""The int8 lists of the inverted file (include/mdx_lists_i8.h; mdir_amd/ivf.py, storage="i8") restated in numpy (a helper module,
imported by test_lists_i8_host.py, test_gpu_lists_i8.py and test_gpu_lists_i8_memcontract.py).

Nothing here is new arithmetic: the int8 scores are test_i8_host.quantize_np / scores_np, the candidates and the selection are
ivf_restatement's, the exact chain is oracle/chain.c and the certificate is test_rescore_host's float64 evaluation of U_q.  What this
module states is how the search puts them together."""
import numpy as np

import ivf_restatement as IR
from test_i8_host import quantize_np, scores_np
from test_rescore_host import bounds_np, depth_np, rank_order, upper_np

F32 = np.float32


def centred(queries, center=None):
    """x_q = q - center, one fp32 subtraction; ``queries`` fp32 [nq, d]."""
    queries = np.ascontiguousarray(queries, F32)
    return queries if center is None else (queries - np.asarray(center, F32)[None, :]).astype(F32)


def encode(rows, members):
    """(codes int8 [m, round_up(d, 64)], scales fp32 [m]) of mdx_lists_i8_encode: zero codes and a NaN scale for an id outside the rows."""
    rows = np.ascontiguousarray(rows, F32)
    n, d = rows.shape
    members = np.asarray(members, np.int64)
    ok = (members >= 0) & (members < n)
    c, s = quantize_np(rows)
    codes = np.zeros((len(members), (d + 63) // 64 * 64), np.int8)
    scales = np.full(len(members), np.nan, F32)
    codes[ok, :d] = c[members[ok]]
    scales[ok] = s[members[ok]]
    return codes, scales


def i8_scores(rows, queries, center=None):
    """fp32 [nq, n]: the MDX_I8 scores of the contract (include/mdx.h), the bits of an int8 index of the rows."""
    cx, sx = quantize_np(rows)
    cq, sq = quantize_np(centred(queries, center))
    return scores_np(cq, sq, cx, sx)


def search(labels, lists, probes, rows, queries, k, shortlist=None, center=None):
    """(ids int64 [nq, k], scores fp32 [nq, k], scanned int64 [nq], certified int64 [nq] or None) of IVFIndex.search on an int8 index
    without ``exact``; ``queries`` fp32 [nq, d]."""
    from oracle import chain
    rows = np.ascontiguousarray(rows, F32)
    n, d = rows.shape
    s8 = i8_scores(rows, queries, center)
    if shortlist is None:
        return IR.search_labels(labels, lists, probes, s8, k) + (None,)
    ids8, sc8, scanned = IR.search_labels(labels, lists, probes, s8, shortlist)
    xq = centred(queries, center)
    exact = chain.gemm_nt_chain(xq, rows)
    ids = np.full(ids8.shape, -1, np.int64)
    sc = np.full(ids8.shape, np.nan, F32)
    for q in range(len(ids8)):
        have = ids8[q][ids8[q] >= 0]
        ids[q, :len(have)], sc[q, :len(have)] = rank_order(exact[q, have], have)
    upper = upper_np(sc8[:, shortlist - 1], xq, bounds_np(rows), d)
    certified = np.where(scanned <= shortlist, shortlist, depth_np(sc, upper, max(n, shortlist)))
    return ids[:, :k], sc[:, :k], scanned, certified.astype(np.int64)


def planted(seed=39, n=323, d=64, nq=9, planted_queries=3, copies=5, lists=6):
    """Unit rows and queries for the certificate: the first ``planted_queries`` queries each have ``copies`` near-duplicates among the
    rows, made as q + 0.05 (p + 1) g / sqrt(d) with g normal, renormalised (p = 0 .. copies - 1: cosines of about 0.999 down to 0.97),
    at shuffled row ids; every other row and query is a random unit vector (cosines of about +- 0.125 at d = 64).  Returns (rows fp32
    [n, d], queries fp32 [nq, d], labels int64 [n] in [0, lists), centroids fp32 [lists, d])."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    queries = unit(rng.standard_normal((nq, d)))
    rows = unit(rng.standard_normal((n, d)))
    where = rng.permutation(n)[:planted_queries * copies].reshape(planted_queries, copies)
    for q in range(planted_queries):
        for p in range(copies):
            rows[where[q, p]] = unit(queries[q] + 0.05 * (p + 1) * rng.standard_normal(d) / np.sqrt(d))
    labels = rng.integers(0, lists, n).astype(np.int64)
    centroids = unit(rng.standard_normal((lists, d)))
    return rows.astype(F32), queries.astype(F32), labels, centroids.astype(F32)
