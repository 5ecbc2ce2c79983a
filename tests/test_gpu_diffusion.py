"""Diffusion on an MI355X: mdx_knn_graph and mdx_diffusion against a float64 restatement of their contract
(include/mdx.h), their bit-determinism and batch independence, diffusion on synthetic manifolds, a full-size solve, and the
`diffusion` key through ./eval.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------ float64 restatement of the definitions

def topk64(scores, k):
    """mdx_topk's order in float64: descending score, ascending id on ties."""
    part = np.argpartition(-scores, k - 1, axis=1)[:, :k]
    vals = np.take_along_axis(scores, part, axis=1)
    order = np.lexsort((part, -vals), axis=1)
    return np.take_along_axis(part, order, axis=1), np.take_along_axis(vals, order, axis=1)


def graph64(ids, sims, gamma):
    """(cols, vals, counts) of the normalised mutual kNN graph, vals in float64; cols padded with -1, vals with 0."""
    ids = np.asarray(ids, dtype=np.int64)
    sims = np.asarray(sims, dtype=np.float64)
    n, k = ids.shape
    where = [dict() for _ in range(n)]                  # where[j][i] = first position of i in L_j
    for j in range(n):
        for t in range(k - 1, -1, -1):
            where[j][int(ids[j, t])] = t
    cols = np.full((n, k), -1, dtype=np.int64)
    w = np.zeros((n, k))
    counts = np.zeros(n, dtype=np.int64)
    deg = np.zeros(n)
    for i in range(n):
        c = 0
        for e in range(k):
            j = int(ids[i, e])
            if j < 0 or j >= n or j == i or where[i][j] != e or i not in where[j]:
                continue                                # a repeated id is an edge at its first position only
            s = sims[i, e] if i < j else sims[j, where[j][i]]
            cols[i, c] = j
            w[i, c] = max(s, 0.0) ** gamma
            c += 1
        counts[i] = c
        deg[i] = w[i, :c].sum()
    r = 1.0 / np.sqrt(deg + 1e-12)
    vals = np.zeros((n, k))
    for i in range(n):
        c = counts[i]
        vals[i, :c] = w[i, :c] * r[i] * r[cols[i, :c]]
    return cols, vals, counts


def dense(cols, vals, counts, n):
    S = np.zeros((n, n))
    for i in range(n):
        c = counts[i]
        S[i, cols[i, :c]] = vals[i, :c]
    return S


def seeds64(seed_ids, seed_sims, n, gamma):
    y = np.zeros((n, seed_ids.shape[0]))
    for q in range(seed_ids.shape[0]):
        for j, s in zip(seed_ids[q], np.asarray(seed_sims[q], dtype=np.float64)):
            if 0 <= j < n:
                y[j, q] = max(s, 0.0) ** gamma
    return y


def cg64(S, y, alpha, iters, tol, history=None):
    """Column-wise CG on (I - alpha S) f = y with the contract's stopping rule; (f [n, nq], residual [nq], steps [nq]).
    ``history``: a list that receives every step's ||r|| / ||y|| [nq]."""
    n, nq = y.shape
    f = np.zeros_like(y)
    r = y.copy()
    p = y.copy()
    yy = (y * y).sum(0)
    rr = yy.copy()
    active = (yy > 0) & ~(rr <= tol * tol * yy)
    steps = np.zeros(nq, dtype=np.int64)
    for _ in range(iters):
        ap = p - alpha * (S @ p)
        pap = (p * ap).sum(0)
        go = active & (pap > 0)
        active &= go
        a = np.where(go, rr / np.where(go, pap, 1), 0)
        f += a * p
        r -= a * ap
        rrn = (r * r).sum(0)
        if history is not None:
            history.append(np.sqrt(rrn / np.where(yy > 0, yy, 1)))
        steps += active
        beta = np.where(active, rrn / np.where(active, rr, 1), 0)
        rr = np.where(active, rrn, rr)
        active &= ~(rrn <= tol * tol * yy)
        p = r + beta * p
    res = np.where(yy > 0, np.sqrt(rr / np.where(yy > 0, yy, 1)), 0)
    return f, res, steps


def final64(f, scores):
    """[nq, n]: f where positive, else the first-stage score - 3."""
    return np.where(f.T > 0, f.T, np.asarray(scores, dtype=np.float64) - 3)


def diffusion64(qvecs, vecs, k, kq, gamma, alpha, iters, tol, lists=None):
    """Float64 diffusion end to end: the graph from float64 top-k lists (or the given (ids, sims)), float64 CG."""
    x = vecs.astype(np.float64)
    n = x.shape[0]
    if lists is None:
        lists = topk64(x @ x.T, min(k, n))
    cols, vals, counts = graph64(*lists, gamma)
    s = qvecs.astype(np.float64) @ x.T
    sid, ssim = topk64(s, min(kq, n))
    f, res, steps = cg64(dense(cols, vals, counts, n), seeds64(sid, ssim, n, gamma), alpha, iters, tol)
    return final64(f, s), res, steps


def chains(rng, nchains, length, ndistract, d=64, step=0.15):
    """Chains of unit vectors x_{t+1} = normalise(x_t + step * u), u standard normal, among random distractors.
    Returns (database [N, d], queries [nchains, d] = the chain starts, gnd: the rest of each chain)."""
    rows, gnd, starts = [], [], []
    for c in range(nchains):
        x = unit_rows(rng, 1, d)[0].astype(np.float64)
        starts.append(x)
        ids = []
        for t in range(length):
            u = rng.standard_normal(d)
            x = x + step * u
            x /= np.linalg.norm(x)
            ids.append(len(rows))
            rows.append(x)
        gnd.append({"ok": ids, "junk": []})
    rows.extend(unit_rows(rng, ndistract, d).astype(np.float64))
    perm = rng.permutation(len(rows))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    db = np.asarray(rows)[perm].astype(np.float32)
    gnd = [{"ok": sorted(int(inv[i]) for i in g["ok"]), "junk": []} for g in gnd]
    return db, np.asarray(starts, dtype=np.float32), gnd


def lists_of(x_t, k):
    """The library's own top-k lists of the database against itself (what DiffusionGraph feeds mdx_knn_graph)."""
    from mdir_amd import ops
    return ops.topk(ops.scores_rowmajor(x_t, x_t, "ND"), min(k, x_t.shape[0]))


def check_graph(cols, vals, counts, ids, sims, gamma, rtol=2e-6):
    """The kernel's graph against graph64 of the SAME lists: mask and order exact, vals within rtol, S bit-symmetric."""
    c64, v64, n64 = graph64(ids, sims, gamma)
    cols, vals, counts = cols.cpu().numpy(), vals.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, n64)
    assert np.array_equal(cols.astype(np.int64), c64)              # valid entries in list order, then -1
    assert np.all(vals[c64 < 0] == 0)
    ok = c64 >= 0
    err = np.abs(vals[ok] - v64[ok]) / np.maximum(np.abs(v64[ok]), 1e-30)
    assert err.size == 0 or err.max() <= rtol, err.max()
    # exact symmetry: the entry (j, i) holds the same bits as (i, j)
    n = counts.shape[0]
    pos = {}
    for i in range(n):
        for e in range(counts[i]):
            pos[(i, int(cols[i, e]))] = vals[i, e]
    for (i, j), v in pos.items():
        assert pos[(j, i)].view(np.uint32) == v.view(np.uint32), (i, j)
    return c64, v64, n64


# ------------------------------------------------------------------------------------------------------ the graph

@pytest.mark.parametrize("n, k, gamma", [(500, 10, 3.0), (1500, 50, 3.0), (30, 50, 3.0), (400, 7, 0.0), (700, 20, 1.0)])
def test_knn_graph_against_float64(n, k, gamma):
    from mdir_amd import ops
    rng = np.random.default_rng(n + k)
    x = unit_rows(rng, n, 32)
    x[n // 2:n // 2 + 5] = x[3]                                    # duplicate rows: the tie order decides the lists
    x_t = dev(x)
    ids, sims = lists_of(x_t, k)                                   # k > n: lists of n entries
    cols, vals, counts = ops.knn_graph(ids, sims, gamma)
    check_graph(cols, vals, counts, ids.cpu().numpy(), sims.cpu().numpy(), gamma)
    assert counts.cpu().numpy().sum() > 0


def test_knn_graph_odd_lists():
    """Lists wider than n with repeated ids, ids outside [0, n), all-negative rows, and weights that vanish."""
    from mdir_amd import ops
    rng = np.random.default_rng(3)
    n, k = 40, 55
    ids = rng.integers(0, n, (n, k)).astype(np.int64)
    bad = rng.random((n, k)) < 0.1
    ids[bad] = rng.choice(np.array([-1, n, n + 3, -(1 << 40), 1 << 40], dtype=np.int64), bad.sum())
    sims = rng.uniform(-0.5, 1.0, (n, k)).astype(np.float32)
    sims[5] = -np.abs(sims[5]) - 0.01                              # a row with only negative similarities
    for gamma in (3.0, 0.5):
        cols, vals, counts = ops.knn_graph(dev(ids), dev(sims), gamma)
        c64, v64, n64 = check_graph(cols, vals, counts, ids, sims, gamma)
        assert n64.sum() > 0


# ---------------------------------------------------------------------------------------------------------- solve

def small_problem(seed=21, n=2000, nq=20, k=10):
    rng = np.random.default_rng(seed)
    db, starts, gnd = chains(rng, 20, 40, n - 800)
    x_t = dev(db)
    q = starts[:nq] if nq <= len(starts) else np.concatenate([starts, unit_rows(rng, nq - len(starts), db.shape[1])])
    return db, q, x_t, dev(q), gnd


def solve(graph, q_t, x_t, kq, gamma, alpha, iters, tol):
    from mdir_amd import ops
    s = ops.scores_rowmajor(x_t, q_t, "ND")
    sid, ssim = ops.topk(s, kq)
    out, res, steps = ops.diffusion(graph, s, sid, ssim, gamma, alpha, iters, tol, return_residual=True)
    return s, sid, ssim, out, res, steps


def test_diffusion_solve_against_float64_cg():
    from mdir_amd import ops
    db, q, x_t, q_t, _ = small_problem()
    n, k, kq, gamma = db.shape[0], 10, 10, 3.0
    ids, sims = lists_of(x_t, k)
    graph = ops.knn_graph(ids, sims, gamma)
    S = dense(*[t.cpu().numpy() for t in graph], n).astype(np.float64)       # the kernel's own S: the solve alone
    assert np.array_equal(S, S.T)
    for alpha, iters, tol in ((0.99, 20, 1e-6), (0.9, 8, 1e-6), (0.0, 3, 1e-6)):
        s, sid, ssim, out, res, steps = solve(graph, q_t, x_t, kq, gamma, alpha, iters, tol)
        y = seeds64(sid.cpu().numpy(), ssim.cpu().numpy(), n, gamma)
        hist = []
        f, res64, steps64 = cg64(S, y, alpha, iters, tol, hist)
        got = out.cpu().numpy()
        want = final64(f, s.cpu().numpy())
        scale = np.abs(f).max(axis=0)
        # f within 1e-4 of the column's largest value wherever float64's f is clearly positive (fp32 CG vs float64 CG)
        clear = f.T > 1e-3 * scale[:, None]
        assert clear.sum() > 0
        err = (np.abs(got - want) / scale[:, None])[clear].max()
        assert err <= 1e-4, (alpha, err)
        unreached = f.T == 0
        assert np.array_equal(got[unreached], (s.cpu().numpy() - np.float32(3))[unreached])
        # step counts agree wherever no float64 residual lies within a factor 2 of tol (no threshold coin-flip); residuals
        # within 1 % (or 1e-6 absolute, where fp32 reaches its floor)
        h = np.asarray(hist)
        sharp = ~((h > tol / 2) & (h < 2 * tol)).any(axis=0)
        assert sharp.sum() >= len(sharp) // 2
        assert np.array_equal(steps.cpu().numpy()[sharp], steps64[sharp]), (alpha, steps.cpu().numpy(), steps64)
        np.testing.assert_allclose(res.cpu().numpy(), res64, rtol=1e-2, atol=1e-6)

    # enough steps: within tol-scale of the dense solve (alpha = 0.9: cond(A) <= 19)
    s, sid, ssim, out, res, steps = solve(graph, q_t, x_t, kq, gamma, 0.9, 300, 1e-6)
    y = seeds64(sid.cpu().numpy(), ssim.cpu().numpy(), n, gamma)
    fstar = np.linalg.solve(np.eye(n) - 0.9 * S, y)
    got = out.cpu().numpy().T
    reached = fstar > 1e-6 * fstar.max(axis=0)
    err = np.abs(np.where(reached, got, 0) - np.where(reached, fstar, 0)).max(axis=0) / fstar.max(axis=0)
    assert err.max() <= 1e-4, err.max()
    assert (res.cpu().numpy() <= 1e-6).all() and (steps.cpu().numpy() < 300).all()


def test_diffusion_columns_stop_on_the_device():
    """A loose tol stops columns at different steps; a stopped column's outputs do not move with more iterations.  A
    column without a positive seed takes no step and keeps its first-stage scores - 3."""
    from mdir_amd import ops
    db, q, x_t, q_t, _ = small_problem(seed=22)
    n, gamma = db.shape[0], 3.0
    graph = ops.knn_graph(*lists_of(x_t, 10), gamma)
    s = ops.scores_rowmajor(x_t, q_t, "ND")
    sid, ssim = ops.topk(s, 10)
    ssim[3] = -ssim[3].abs() - 0.1                                 # column 3: every seed weight is 0
    a, ra, ka = ops.diffusion(graph, s, sid, ssim, gamma, 0.99, 20, 0.05, return_residual=True)
    b, rb, kb = ops.diffusion(graph, s, sid, ssim, gamma, 0.99, 60, 0.05, return_residual=True)
    ka, kb = ka.cpu().numpy(), kb.cpu().numpy()
    stopped = ka < 20
    assert stopped.sum() >= 3 and ka[3] == 0
    assert np.array_equal(ka[stopped], kb[stopped])
    assert torch.equal(a[torch.from_numpy(stopped).to(DEV)], b[torch.from_numpy(stopped).to(DEV)])
    assert torch.equal(ra[torch.from_numpy(stopped).to(DEV)], rb[torch.from_numpy(stopped).to(DEV)])
    assert (ra.cpu().numpy()[stopped] <= 0.05).all()
    assert torch.equal(a[3], s[3] - 3)
    # in place: out is the scores
    c = s.clone()
    ops.diffusion(graph, c, sid, ssim, gamma, 0.99, 20, 0.05, out=c)
    assert torch.equal(c, a)


def test_diffusion_is_bit_deterministic_and_batch_independent():
    from mdir_amd import ops
    rng = np.random.default_rng(23)
    db, starts, _ = chains(rng, 30, 40, 800)
    x_t = dev(db)
    q = np.concatenate([starts, db[rng.choice(db.shape[0], 270, replace=False)]])          # 300 queries
    q_t = dev(q)
    graph = ops.knn_graph(*lists_of(x_t, 10), 3.0)
    s = ops.scores_rowmajor(x_t, q_t, "ND")
    sid, ssim = ops.topk(s, 10)

    def run(lo, hi):
        return ops.diffusion(graph, s[lo:hi], sid[lo:hi].contiguous(), ssim[lo:hi].contiguous(), 3.0, 0.99, 20, 1e-6,
                             return_residual=True)

    full = run(0, 300)                                             # two groups: 256 + 44
    again = run(0, 300)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    batch70 = run(0, 70)
    for qi in (0, 1, 29, 69, 255, 256, 299):
        alone = run(qi, qi + 1)
        for x, y in zip(full, alone):
            assert torch.equal(x[qi], y[0]), qi
        if qi < 70:
            for x, y in zip(full, batch70):
                assert torch.equal(x[qi], y[qi]), qi


# ---------------------------------------------------------------------------------------- diffusion helps: manifolds

def test_diffusion_follows_manifolds():
    """Chains of unit vectors among random distractors: from a chain's start, diffusion finds the far end of the chain
    that the plain dot product ranks among the distractors (float64: 0.54 against 0.13 mAP).  Margin asserted: +0.15 mAP.
    Its mAP equals the float64 oracle's."""
    from mdir_amd import ops, rerank
    from mdir_amd.evaluate import compute_map
    rng = np.random.default_rng(24)
    db, q, gnd = chains(rng, 30, 15, 3000)
    x_t, q_t = dev(db), dev(q)
    k, kq, gamma, alpha, iters, tol = 5, 3, 3.0, 0.99, 20, 1e-6
    graph = rerank.DiffusionGraph(x_t, k=k, gamma=gamma)
    scores = rerank.diffusion(q_t, x_t, graph, kq=kq, alpha=alpha, iters=iters, tol=tol)
    plain = ops.scores_rowmajor(x_t, q_t, "ND")
    m_diff = compute_map(ops.rank_full(scores).t(), gnd, [1, 5, 10])[0]
    m_plain = compute_map(ops.rank_full(plain).t(), gnd, [1, 5, 10])[0]
    assert m_diff >= m_plain + 0.15, (m_diff, m_plain)
    ids, sims = lists_of(x_t, k)
    want, _, _ = diffusion64(q, db, k, kq, gamma, alpha, iters, tol, lists=(ids.cpu().numpy(), sims.cpu().numpy()))
    m64 = O.compute_map(np.argsort(-want, axis=1, kind="stable").T, gnd, [1, 5, 10])[0]
    assert abs(m_diff - m64) <= 1e-6, (m_diff, m64)


# ------------------------------------------------------------------------------------------------------- full size

def test_diffusion_full_size_ring():
    """N = 1 004 993, k = 50: a ring lattice (row i lists i +- 1 .. i +- 25, so every edge is mutual) through
    mdx_knn_graph, then a 70-query solve against float64 CG on the device, in well under a minute."""
    from mdir_amd import ops
    n, k, nq, kq, gamma, alpha, iters = 1004993, 50, 70, 10, 3.0, 0.99, 20
    off = torch.cat([torch.arange(1, 26), -torch.arange(1, 26)]).to(DEV)
    ids = (torch.arange(n, device=DEV)[:, None] + off[None, :]) % n
    sims = (1.0 - 0.01 * off.abs().float())[None, :].expand(n, k).contiguous()
    cols, vals, counts = ops.knn_graph(ids, sims, gamma)
    assert (counts == k).all()
    assert torch.equal(cols.long(), ids)
    g = torch.Generator(device=DEV)
    g.manual_seed(25)
    s = torch.rand((nq, n), generator=g, device=DEV) * 0.5
    sid, ssim = ops.topk(s, kq)
    ops.diffusion((cols, vals, counts), s[:1], sid[:1].contiguous(), ssim[:1].contiguous(), gamma, alpha, 2, 1e-6)   # warm
    torch.cuda.synchronize()
    t0 = time.time()
    out, res, steps = ops.diffusion((cols, vals, counts), s, sid, ssim, gamma, alpha, iters, 1e-6, return_residual=True)
    torch.cuda.synchronize()
    assert time.time() - t0 < 60

    # one SpMM step: after iters = 1, f = (y.y / y.Ay) y on the seeds
    idx = cols.long()
    v64 = vals.double()

    def apply_a(x):
        acc = torch.zeros_like(x)
        for e in range(k):
            acc += v64[:, e:e + 1] * x[idx[:, e]]
        return x - alpha * acc

    y = torch.zeros((n, nq), dtype=torch.float64, device=DEV)
    y.scatter_(0, sid.t(), ssim.t().double().clamp(min=0) ** gamma)
    one = ops.diffusion((cols, vals, counts), s, sid, ssim, gamma, alpha, 1, 1e-6)
    a0 = (y * y).sum(0) / (y * apply_a(y)).sum(0)
    want1 = (a0 * y).t().gather(1, sid)
    assert ((one.gather(1, sid).double() - want1).abs() / want1.abs()).max().item() <= 1e-5

    # float64 CG on the device, same rule
    f = torch.zeros_like(y)
    r, p = y.clone(), y.clone()
    yy = (y * y).sum(0)
    rr = yy.clone()
    for _ in range(iters):
        ap = apply_a(p)
        a = rr / (p * ap).sum(0)
        f += a * p
        r -= a * ap
        rrn = (r * r).sum(0)
        p = r + (rrn / rr) * p
        rr = rrn
    assert (steps == iters).all()
    res64 = (rr / yy).sqrt()
    assert ((res.double() - res64).abs() / res64).max().item() <= 1e-3
    scale = f.abs().max(0).values
    clear = f > 1e-3 * scale
    got = out.t().double()
    err = ((got - f).abs() / scale)[clear].max().item()
    assert err <= 1e-4, err
    # the true residual of the kernel's solution, recomputed in float64, is its reported residual's size
    fk = torch.where(got > -1.5, got, torch.zeros_like(got))          # outputs below -1.5 are s - 3: f <= 0 there
    true_res = ((y - apply_a(fk)).norm(dim=0) / yy.sqrt())
    assert (true_res <= 2 * res.double() + 1e-3).all(), (true_res.max().item(), res.max().item())


# ------------------------------------------------------------------------------------------------------- eval.py

_CAPTURE = r"""
import os, runpy, sys
import numpy as np
sys.path.insert(0, %(root)r)
import mdir_amd.score as S
orig, calls = S.extract_vectors_device, []
def capture(*args, **kwargs):
    v = orig(*args, **kwargs)
    calls.append(1)
    np.save(os.path.join(%(dump)r, "desc%%d.npy" %% len(calls)), v.cpu().numpy())
    return v
S.extract_vectors_device = capture
sys.argv = [os.path.join(%(root)r, "eval.py")] + %(args)r
runpy.run_path(sys.argv[0], run_name="__main__")
"""


def test_eval_py_with_diffusion(tmp_path):
    """./eval.py on the generated roxford5k (ranking: full) + 247tokyo1k (ranking: positions) set-up with the diffusion
    key: the printed numbers equal a float64 diffusion + compute_map on the descriptors the library extracted in that very
    run."""
    root = str(tmp_path / "synth")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_eval.py"), root], timeout=600)
    over = str(tmp_path / "diffusion.yml")
    # small k: the 15 Tokyo descriptors of the random-weight network lie close together (as in the DBA test)
    p = {"k": 3, "kq": 2, "gamma": 3.0, "alpha": 0.9, "iters": 20, "tol": 1e-6}
    crit = "diffusion: {k: %(k)d, kq: %(kq)d, gamma: %(gamma)s, alpha: %(alpha)s, iters: %(iters)d, tol: 1.0e-6}" % p
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
    want, gaps = {}, {}
    for ds, label, key, vecs, qvecs in (("roxford5k", "roxford.5k medium", "ap_medium", desc[0], desc[1]),
                                        ("247tokyo1k", "247tokyo.1k", "ap", desc[2], desc[2])):
        cfg = configdataset(ds, os.path.join(root, "data", "test"))
        assert vecs.shape[0] == cfg["n"] and qvecs.shape[0] == cfg["nq"]
        scores, _, _ = diffusion64(qvecs, vecs, p["k"], p["kq"], p["gamma"], p["alpha"], p["iters"], p["tol"])
        _, per = O.compute_map_and_print(ds, np.argsort(-scores, axis=1, kind="stable").T, cfg["gnd"])
        want[label] = round(100 * O.nanmean_metric(per[key]), 2)
        gaps[label] = float(np.diff(np.sort(scores, axis=1), axis=1).min())
    assert printed == want, (printed, want, "smallest float64 score gaps", gaps, out[-3000:])
