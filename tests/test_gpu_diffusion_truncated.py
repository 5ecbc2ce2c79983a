"""Truncated diffusion on an MI355X: mdx_knn_graph_weights against mdx_knn_graph and float64, mdx_diffusion_truncated against
a float64 restatement of its contract (include/mdx.h: the subgraph of the top-R rows, renormalised there, dense R x R CG),
its edge cases, bit-determinism and batch independence, the full solve it equals at R = N, a manifold, a full-size solve and
the `diffusion: {truncate}` key through ./eval.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import oracle as O
from test_gpu_diffusion import _CAPTURE, cg64, chains, dev, lists_of, small_problem, unit_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------ float64 restatement of the definition

def weights64(ids, sims, gamma):
    """(cols, w, counts) of the mutual kNN graph before normalisation, w in float64 (graph64 without its last step)."""
    ids = np.asarray(ids, dtype=np.int64)
    sims = np.asarray(sims, dtype=np.float64)
    n, k = ids.shape
    where = [dict() for _ in range(n)]
    for j in range(n):
        for t in range(k - 1, -1, -1):
            where[j][int(ids[j, t])] = t
    cols = np.full((n, k), -1, dtype=np.int64)
    w = np.zeros((n, k))
    counts = np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = 0
        for e in range(k):
            j = int(ids[i, e])
            if j < 0 or j >= n or j == i or where[i][j] != e or i not in where[j]:
                continue
            s = sims[i, e] if i < j else sims[j, where[j][i]]
            cols[i, c] = j
            w[i, c] = max(s, 0.0) ** gamma
            c += 1
        counts[i] = c
    return cols, w, counts


def subgraph64(t, rows_cols, rows_w, rows_counts, n):
    """Dense S^R [R, R] of one query in float64: t = its top-R ids, rows_* = the ELL rows of those ids (host copies of only
    these R rows).  A repeated id is a node at its first position only."""
    t = np.asarray(t, dtype=np.int64)
    r = len(t)
    first = {}
    for a in range(r - 1, -1, -1):
        first[int(t[a])] = a
    node = np.array([first[int(t[a])] == a for a in range(r)])
    W = np.zeros((r, r))
    for a in range(r):
        if not node[a]:
            continue
        for e in range(int(rows_counts[a])):
            b = first.get(int(rows_cols[a, e]), -1)
            if b >= 0:
                W[a, b] = rows_w[a, e]
    d = W.sum(axis=1)
    rinv = 1.0 / np.sqrt(d + 1e-12)
    return W * rinv[:, None] * rinv[None, :], node


def truncated64(s, top_ids, top_sims, cols, w, counts, kq, gamma, alpha, iters, tol):
    """Float64 truncated diffusion of every query: ([nq, n] outputs, residual [nq], steps [nq], f list, histories)."""
    s = np.asarray(s, dtype=np.float64)
    nq, n = s.shape
    out = s - 3
    res, steps, fs, hists = np.zeros(nq), np.zeros(nq, dtype=np.int64), [], []
    for q in range(nq):
        t = top_ids[q]
        S, node = subgraph64(t, cols[t], w[t], counts[t], n)
        r = len(t)
        sims = np.asarray(top_sims[q], dtype=np.float64)
        y = np.where((np.arange(r) < min(kq, r)) & node & (sims > 0), np.where(sims > 0, sims, 0) ** gamma, 0.0)
        hist = []
        f, rq, kq_steps = cg64(S, y[:, None], alpha, iters, tol, hist)
        f = f[:, 0]
        res[q], steps[q] = rq[0], kq_steps[0]
        pos = f > 0
        out[q, t[pos]] = f[pos]
        fs.append(f)
        hists.append(np.asarray(hist)[:, 0] if hist else np.zeros(0))
    return out, res, steps, fs, hists


def run(wgraph, s, r, kq, gamma, alpha, iters, tol, out=None):
    from mdir_amd import ops
    tid, tsim = ops.topk(s, r)
    o, res, steps = ops.diffusion_truncated(wgraph, s, tid, tsim, kq, gamma, alpha, iters, tol, out=out, return_residual=True)
    return tid, tsim, o, res, steps


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def same_bits(a, b):
    """fp32 arrays equal bit for bit, any NaN matching any NaN."""
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_against64(wgraph, s, r, kq, gamma, alpha, iters, tol):
    """The kernel against truncated64 on the kernel's own W and top-R lists: the bars of test_diffusion_solve_against_float64_cg."""
    tid, tsim, out, res, steps = run(wgraph, s, r, kq, gamma, alpha, iters, tol)
    cols, w, counts = host(*wgraph)
    s_h, tid, tsim, got, res, steps = host(s, tid, tsim, out, res, steps)
    want, res64, steps64, fs, hists = truncated64(s_h, tid, tsim, cols.astype(np.int64), w.astype(np.float64), counts, kq,
                                                  gamma, alpha, iters, tol)
    base = s_h - np.float32(3)
    collapsed = np.zeros(s_h.shape[0], dtype=bool)
    for q in range(s_h.shape[0]):
        f = fs[q]
        inside = np.zeros(s_h.shape[1], dtype=bool)
        inside[tid[q]] = True
        # outside T_q, and inside where float64 f is exactly 0 (unreached): s - 3 bit for bit
        assert same_bits(got[q, ~inside], base[q, ~inside]), q
        unreached = tid[q][f == 0]
        assert same_bits(got[q, unreached], base[q, unreached]), q
        scale = np.abs(f).max()
        if scale == 0:
            continue
        clear = tid[q][f > 1e-3 * scale]
        err = (np.abs(got[q, clear] - want[q, clear]) / scale).max()
        assert err <= 1e-4, (r, alpha, q, err)
        # step counts agree unless a float64 residual lies within a factor 2 of tol (a threshold coin-flip) or float64 stops
        # by collapsing far below tol (finite termination on a small subgraph, below what fp32 CG resolves)
        h = hists[q]
        collapsed[q] = h.size > 0 and h[-1] < 1e-2 * tol
        if h.size and not ((h > tol / 2) & (h < 2 * tol)).any() and not collapsed[q]:
            assert steps[q] == steps64[q], (r, alpha, q, steps[q], steps64[q])
    # residuals within 1 % (or 1e-6 absolute); where float64 collapsed, fp32 ends at its own floor
    np.testing.assert_allclose(res[~collapsed], res64[~collapsed], rtol=1e-2, atol=1e-6)
    assert (res[collapsed] <= 1e-5).all(), res[collapsed]
    return tid, got, want, fs


# ------------------------------------------------------------------------------------------------------ the weights

@pytest.mark.parametrize("n, k, gamma", [(500, 10, 3.0), (1500, 50, 3.0), (30, 50, 3.0), (700, 20, 1.0)])
def test_knn_graph_weights(n, k, gamma):
    """cols / counts are mdx_knn_graph's; w is float64's within 2e-6; w * (r_lo * r_hi) in fp32, the degree an fp32
    sequential sum in edge order, reproduces mdx_knn_graph's vals bit for bit."""
    from mdir_amd import ops
    rng = np.random.default_rng(n + k + 7)
    x = unit_rows(rng, n, 32)
    x[n // 2:n // 2 + 5] = x[3]
    ids, sims = lists_of(dev(x), k)
    cols, vals, counts = host(*ops.knn_graph(ids, sims, gamma))
    wc, w, wn = host(*ops.knn_graph_weights(ids, sims, gamma))
    assert np.array_equal(wc, cols) and np.array_equal(wn, counts)
    c64, w64, n64 = weights64(*host(ids, sims), gamma)
    assert np.array_equal(wc.astype(np.int64), c64) and np.array_equal(wn, n64)
    ok = c64 >= 0
    assert np.all(w[~ok] == 0)
    err = np.abs(w[ok] - w64[ok]) / np.maximum(np.abs(w64[ok]), 1e-30)
    assert err.size == 0 or err.max() <= 2e-6, err.max()
    rinv = np.empty(n, dtype=np.float32)
    for i in range(n):
        d = np.float32(0)
        for e in range(counts[i]):
            d = np.float32(d + w[i, e])
        rinv[i] = np.float32(1) / np.sqrt(np.float32(d + np.float32(1e-12)))
    again = np.zeros_like(vals)
    for i in range(n):
        c = counts[i]
        again[i, :c] = w[i, :c] * (rinv[i] * rinv[cols[i, :c]])
    assert np.array_equal(again.view(np.uint32), vals.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- solve

@pytest.fixture(scope="module")
def chain5k():
    from mdir_amd import ops
    db, q, x_t, q_t, gnd = small_problem(seed=31, n=5000)
    wgraph = ops.knn_graph_weights(*lists_of(x_t, 10), 3.0)
    s = ops.scores_rowmajor(x_t, q_t, "ND")
    return db, q, x_t, q_t, wgraph, s


@pytest.mark.parametrize("r", [1, 10, 100, 1000, 4096])
def test_truncated_solve_against_float64(chain5k, r):
    _, _, _, _, wgraph, s = chain5k
    for alpha, iters, tol in ((0.99, 20, 1e-6), (0.9, 8, 1e-6), (0.0, 3, 1e-6)):
        check_against64(wgraph, s, r, 10, 3.0, alpha, iters, tol)


@pytest.mark.parametrize("r", [100, 1000])
def test_truncated_solve_converges_to_the_dense_solution(chain5k, r):
    _, _, _, _, wgraph, s = chain5k
    s = s[:5].contiguous()
    tid, tsim, out, res, steps = run(wgraph, s, r, 10, 3.0, 0.9, 300, 1e-6)
    cols, w, counts = host(*wgraph)
    tid, tsim, got = host(tid, tsim, out)
    for q in range(s.shape[0]):
        S, node = subgraph64(tid[q], cols[tid[q]], w[tid[q]].astype(np.float64), counts[tid[q]], s.shape[1])
        sims = tsim[q].astype(np.float64)
        y = np.where((np.arange(r) < 10) & node & (sims > 0), np.where(sims > 0, sims, 0) ** 3.0, 0.0)
        fstar = np.linalg.solve(np.eye(r) - 0.9 * S, y)
        reached = fstar > 1e-6 * fstar.max()
        err = np.abs(got[q, tid[q][reached]] - fstar[reached]).max() / fstar.max()
        assert err <= 1e-4, (r, q, err)
    assert (res.cpu().numpy() <= 1e-6).all() and (steps.cpu().numpy() < 300).all()


def test_seed_prefix_of_topk_r_is_topk_kq():
    """The seeds of the truncated solve (the first kq of topk(s, R)) are the full solve's topk(s, kq): ids and scores, also
    with ties and NaN."""
    from mdir_amd import ops
    rng = np.random.default_rng(32)
    s = rng.random((9, 20000)).astype(np.float32)
    s[1, ::7] = 0.5                                                     # ties
    s[2] = np.round(s[2] * 20) / 20
    s[3, :50] = np.nan
    s[4, 100:200] = s[4].max()
    s_t = dev(s)
    for kq in (1, 10, 50):
        ki, ks = host(*ops.topk(s_t, kq))
        for r in (kq, 100, 1000, 4096):
            ri, rs = host(*ops.topk(s_t, r))
            assert np.array_equal(ri[:, :kq], ki), (kq, r)
            assert np.array_equal(rs[:, :kq].view(np.uint32), ks.view(np.uint32)), (kq, r)


def test_truncate_n_equals_the_full_solve():
    """truncate >= N: the same S bit for bit, so the same solve up to the order of the dot products' sums: within fp32
    tolerance of rerank.diffusion without truncate, and the same rankings where the scores are well separated."""
    from mdir_amd import ops, rerank
    rng = np.random.default_rng(33)
    db, q, gnd = chains(rng, 20, 30, 1500)
    x_t, q_t = dev(db), dev(q)
    n = db.shape[0]
    graph = rerank.DiffusionGraph(x_t, k=10, gamma=3.0, weights=True)
    full = rerank.diffusion(q_t, x_t, graph, kq=10, alpha=0.99, iters=20, tol=1e-6).cpu().numpy()
    trunc = rerank.diffusion(q_t, x_t, graph, kq=10, alpha=0.99, iters=20, tol=1e-6, truncate=4096).cpu().numpy()
    assert n < 4096
    rf, rt = full > -1.5, trunc > -1.5                                  # outputs below -1.5 are s - 3
    scale = np.where(rf, full, 0).max(axis=1)[:, None]
    both = rf & rt
    err = (np.abs(np.where(both, trunc - full, 0)) / scale).max()
    assert err <= 1e-4, err
    assert (np.where(rf & ~rt, full, 0) <= 1e-4 * scale).all() and (np.where(rt & ~rf, trunc, 0) <= 1e-4 * scale).all()
    assert same_bits(trunc[~rf & ~rt], full[~rf & ~rt])
    # the clearly reached rows rank first in both, in the same order wherever the scores are well separated
    order_f = np.argsort(-full, axis=1, kind="stable")
    order_t = np.argsort(-trunc, axis=1, kind="stable")
    compared = 0
    for q in range(full.shape[0]):
        m = int((full[q] > 1e-3 * scale[q, 0]).sum())
        sf = full[q, order_f[q, :m + 1]]
        gap = np.append(np.abs(np.diff(sf)) / scale[q, 0], np.inf)[:m]         # after the last row of all: none
        sep = np.ones(m, dtype=bool)
        sep[1:] &= gap[:m - 1] > 1e-3
        sep &= gap[:m] > 1e-3
        assert np.array_equal(order_f[q, :m][sep], order_t[q, :m][sep]), q
        compared += sep.sum()
    assert compared >= 100, compared


def test_empty_subgraph_gives_the_seeds():
    """No edge inside T_q: A = I, one step, f = y on the seeds and s - 3 elsewhere."""
    from mdir_amd import ops
    n, k, nq, kq, gamma = 3000, 4, 6, 5, 3.0
    ids = (torch.arange(n, device=DEV)[:, None] + torch.tensor([0, 1, 2, 3], device=DEV)[None, :]) % n
    sims = torch.full((n, k), 0.9, device=DEV)
    wgraph = ops.knn_graph_weights(ids, sims, gamma)                   # a one-way chain of lists: no mutual edge
    assert int(wgraph[2].sum()) == 0
    g = torch.Generator(device=DEV)
    g.manual_seed(34)
    s = torch.rand((nq, n), generator=g, device=DEV)
    tid, tsim, out, res, steps = run(wgraph, s, 100, kq, gamma, 0.99, 20, 1e-6)
    got, s_h, tid, tsim = host(out, s, tid, tsim)
    y = tsim[:, :kq].astype(np.float64) ** gamma
    np.testing.assert_allclose(np.take_along_axis(got, tid[:, :kq], axis=1), y, rtol=2e-6)
    mask = np.ones_like(got, dtype=bool)
    np.put_along_axis(mask, tid[:, :kq], False, axis=1)
    assert np.array_equal(got[mask], (s_h - np.float32(3))[mask])
    assert (steps.cpu().numpy() == 1).all() and (res.cpu().numpy() == 0).all()


def test_non_positive_seeds_and_nan_scores(chain5k):
    """All seeds <= 0: y = 0, no step, out = s - 3.  NaN scores: NaN rows rank last in T_q, weigh 0 as seeds, and the
    outputs still follow the float64 restatement (NaN - 3 = NaN where no positive f lands)."""
    _, _, _, _, wgraph, s = chain5k
    neg = -s.abs()[:4].contiguous() - 0.01
    tid, tsim, out, res, steps = run(wgraph, neg, 100, 10, 3.0, 0.99, 20, 1e-6)
    assert torch.equal(out, neg - 3)
    assert (steps == 0).all() and (res == 0).all()
    bad = s[:6].clone()
    bad[:, ::3] = float("nan")
    bad[1] = float("nan")                                              # a query with nothing but NaN
    bad[2, :] = bad[2].nan_to_num(0.0)
    tid, tsim, out, res, steps = run(wgraph, bad, 1000, 10, 3.0, 0.99, 20, 1e-6)
    got = out.cpu().numpy()
    assert np.isnan(got[1]).all() and steps[1].item() == 0
    check_against64(wgraph, bad, 1000, 10, 3.0, 0.99, 20, 1e-6)


def test_truncated_is_bit_deterministic_and_batch_independent():
    from mdir_amd import ops
    rng = np.random.default_rng(35)
    db, starts, _ = chains(rng, 30, 40, 2000)
    x_t = dev(db)
    q = np.concatenate([starts, db[rng.choice(db.shape[0], 270, replace=False)]])          # 300 queries
    wgraph = ops.knn_graph_weights(*lists_of(x_t, 10), 3.0)
    s = ops.scores_rowmajor(x_t, dev(q), "ND")
    tid, tsim = ops.topk(s, 1000)

    def go(lo, hi):
        return ops.diffusion_truncated(wgraph, s[lo:hi], tid[lo:hi].contiguous(), tsim[lo:hi].contiguous(), 10, 3.0, 0.99, 20,
                                       1e-6, return_residual=True)

    full = go(0, 300)
    again = go(0, 300)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    for size in (1, 7, 70):
        for lo in range(0, 300, size if size > 1 else 37):
            hi = min(300, lo + size)
            part = go(lo, hi)
            for x, y in zip(full, part):
                assert torch.equal(x[lo:hi], y), (size, lo)
    # in place: out is the scores
    c = s.clone()
    ops.diffusion_truncated(wgraph, c, tid, tsim, 10, 3.0, 0.99, 20, 1e-6, out=c)
    assert torch.equal(c, full[0])


def test_truncated_diffusion_follows_manifolds():
    """Chains among distractors, as test_diffusion_follows_manifolds, truncated to the top 2 500 of 3 450 rows: 85 % of the
    chains' rows lie inside their query's subgraph (float64), and the truncated solve follows them to the far ends that the
    dot product ranks among the distractors (float64: 0.45 against 0.13 mAP).  Margin asserted: +0.25 mAP; its mAP equals
    the float64 restatement's."""
    from mdir_amd import ops, rerank
    from mdir_amd.evaluate import compute_map
    rng = np.random.default_rng(24)
    db, q, gnd = chains(rng, 30, 15, 3000)
    x_t, q_t = dev(db), dev(q)
    k, kq, gamma, alpha, iters, tol, r = 5, 3, 3.0, 0.99, 20, 1e-6, 2500
    graph = rerank.DiffusionGraph(x_t, k=k, gamma=gamma, weights=True)
    scores = rerank.diffusion(q_t, x_t, graph, kq=kq, alpha=alpha, iters=iters, tol=tol, truncate=r)
    plain = ops.scores_rowmajor(x_t, q_t, "ND")
    tid = ops.topk(plain, r)[0].cpu().numpy()
    inside = np.mean([np.isin(g["ok"], tid[i]).mean() for i, g in enumerate(gnd)])
    assert inside >= 0.75, inside
    m_diff = compute_map(ops.rank_full(scores).t(), gnd, [1, 5, 10])[0]
    m_plain = compute_map(ops.rank_full(plain).t(), gnd, [1, 5, 10])[0]
    assert m_diff >= m_plain + 0.25, (m_diff, m_plain)
    tid, tsim = host(*ops.topk(plain, r))
    want, _, _, _, _ = truncated64(plain.cpu().numpy(), tid, tsim, graph.cols.cpu().numpy().astype(np.int64),
                                   graph.wvals.cpu().numpy().astype(np.float64), graph.counts.cpu().numpy(), kq, gamma, alpha,
                                   iters, tol)
    m64 = O.compute_map(np.argsort(-want, axis=1, kind="stable").T, gnd, [1, 5, 10])[0]
    assert abs(m_diff - m64) <= 1e-6, (m_diff, m64)


# ------------------------------------------------------------------------------------------------------- full size

@pytest.mark.parametrize("r", [1000, 4096])
def test_truncated_full_size_ring(r):
    """N = 1 004 993, k = 50 ring lattice (every edge mutual), 70 queries whose first-stage scores peak on a contiguous arc,
    so every subgraph row keeps about k edges.  Five queries against the float64 restatement, built from the host copy of
    only their R rows."""
    from mdir_amd import ops
    n, k, nq, kq, gamma, alpha, iters = 1004993, 50, 70, 10, 3.0, 0.99, 20
    off = torch.cat([torch.arange(1, 26), -torch.arange(1, 26)]).to(DEV)
    ids = (torch.arange(n, device=DEV)[:, None] + off[None, :]) % n
    sims = (1.0 - 0.01 * off.abs().float())[None, :].expand(n, k).contiguous()
    cols, w, counts = ops.knn_graph_weights(ids, sims, gamma)
    del ids, sims
    assert (counts == k).all()
    centre = torch.arange(nq, device=DEV)[:, None] * (n // nq) + 12345
    j = torch.arange(n, device=DEV)[None, :]
    dist = torch.minimum((j - centre) % n, (centre - j) % n).float()
    s = (0.9 - dist / n).contiguous()                                  # peaked on an arc around each centre
    tid, tsim, out, res, steps = run((cols, w, counts), s, r, kq, gamma, alpha, iters, 1e-6)
    assert (steps == iters).all() or (res <= 1e-6).all()
    pick = [0, 1, 33, 68, 69]
    t_h = tid[pick].cpu().numpy()
    sub_cols = [cols[tid[q]].cpu().numpy().astype(np.int64) for q in pick]
    sub_w = [w[tid[q]].cpu().numpy().astype(np.float64) for q in pick]
    sub_n = [counts[tid[q]].cpu().numpy() for q in pick]
    ts_h = tsim[pick].cpu().numpy()
    got = out[pick].cpu().numpy()
    res_h = res[pick].cpu().numpy()
    for i, q in enumerate(pick):
        S, node = subgraph64(t_h[i], sub_cols[i], sub_w[i], sub_n[i], n)
        assert node.all()
        assert (S > 0).sum(axis=1).mean() >= 0.9 * k
        sims_q = ts_h[i].astype(np.float64)
        y = np.where(np.arange(r) < kq, np.maximum(sims_q, 0) ** gamma, 0.0)
        f, res64, _ = cg64(S, y[:, None], alpha, iters, 1e-6)
        f = f[:, 0]
        scale = np.abs(f).max()
        clear = f > 1e-3 * scale
        err = (np.abs(got[i, t_h[i][clear]] - f[clear]) / scale).max()
        assert err <= 1e-4, (r, q, err)
        np.testing.assert_allclose(res_h[i], res64[0], rtol=1e-2, atol=1e-6)
    base = (s[pick] - 3).cpu().numpy()
    for i in range(len(pick)):
        outside = np.ones(n, dtype=bool)
        outside[t_h[i]] = False
        assert np.array_equal(got[i, outside].view(np.uint32), base[i, outside].view(np.uint32))


# ------------------------------------------------------------------------------------------------------- eval.py

def test_eval_py_with_truncated_diffusion(tmp_path):
    """./eval.py on the generated roxford5k (ranking: full) + 247tokyo1k (ranking: positions) set-up with the truncate key:
    the printed numbers equal the float64 restatement + compute_map on the descriptors the library extracted in that very
    run (the graph lists and the first-stage top-R are the library's own, on those descriptors)."""
    from mdir_amd import ops
    root = str(tmp_path / "synth")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_eval.py"), root], timeout=600)
    over = str(tmp_path / "diffusion.yml")
    p = {"k": 3, "kq": 2, "gamma": 3.0, "alpha": 0.9, "iters": 20, "tol": 1e-6, "truncate": 8}
    crit = ("diffusion: {k: %(k)d, kq: %(kq)d, gamma: %(gamma)s, alpha: %(alpha)s, iters: %(iters)d, tol: 1.0e-6, "
            "truncate: %(truncate)d}" % p)
    with open(over, "w") as f:
        f.write("validation:\n  roxford5k: {criterion: {%s, ranking: full}}\n  247tokyo1k: {criterion: {%s}}\n" % (crit, crit))
    dump = str(tmp_path / "desc")
    os.makedirs(dump)
    env = dict(os.environ, CIRTORCH_ROOT=root, MDIR_AMD_WORKERS="2")
    script = _CAPTURE % {"root": ROOT, "dump": dump, "args": ["eval.yml", os.path.join(root, "eval_synth.yml"), over]}
    proc = subprocess.run([sys.executable, "-c", script], env=env, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          timeout=900)
    out = proc.stdout
    assert proc.returncode == 0, out[-3000:]
    printed = {}
    for line in out.splitlines():
        for label in ("roxford.5k medium", "247tokyo.1k"):
            if line.strip().startswith(label):
                printed[label] = float(line.split()[-1])
    assert set(printed) == {"roxford.5k medium", "247tokyo.1k"}, out

    from mdir_amd.datasets import configdataset
    desc = [np.load(os.path.join(dump, "desc%d.npy" % i)) for i in (1, 2, 3)]
    want = {}
    for ds, label, key, vecs, qvecs in (("roxford5k", "roxford.5k medium", "ap_medium", desc[0], desc[1]),
                                        ("247tokyo1k", "247tokyo.1k", "ap", desc[2], desc[2])):
        cfg = configdataset(ds, os.path.join(root, "data", "test"))
        assert vecs.shape[0] == cfg["n"] and qvecs.shape[0] == cfg["nq"]
        x_t = dev(vecs)
        c64, w64, n64 = weights64(*host(*lists_of(x_t, p["k"])), p["gamma"])
        s = ops.scores_rowmajor(x_t, dev(qvecs), "ND")
        r = min(p["truncate"], vecs.shape[0])
        assert r < vecs.shape[0]                                       # the subgraph is a real truncation
        tid, tsim = host(*ops.topk(s, r))
        scores, _, _, _, _ = truncated64(s.cpu().numpy(), tid, tsim, c64, w64, n64, p["kq"], p["gamma"], p["alpha"],
                                         p["iters"], p["tol"])
        _, per = O.compute_map_and_print(ds, np.argsort(-scores, axis=1, kind="stable").T, cfg["gnd"])
        want[label] = round(100 * O.nanmean_metric(per[key]), 2)
    assert printed == want, (printed, want, out[-3000:])
