"""Re-ranking on an MI355X: mdx_knn_aggregate against a float64 restatement of its contract (include/mdx.h), its
bit-determinism, alpha-QE and DBA end to end, one full-size alpha-QE, and both keys through ./eval.py."""
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
EPS = 1e-6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------ float64 restatement of the definitions

def weights64(sims, alpha):
    s = np.asarray(sims, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        pos = s > 0                                          # False for NaN
    w = np.zeros_like(s)
    w[pos] = 1.0 if alpha == 0 else s[pos] ** alpha
    return w


def aggregate64(rows, ids, sims, alpha, self_rows=None, eps=EPS):
    """out_q = v / (||v|| + eps), v = self_q + sum_j w_j rows[ids[q, j]] over the ids inside [0, n)."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    nq, k = ids.shape
    w = weights64(sims, alpha)
    v = np.zeros((nq, rows.shape[1])) if self_rows is None else np.array(self_rows, dtype=np.float64)
    for j in range(k):
        ok = (ids[:, j] >= 0) & (ids[:, j] < n)
        v[ok] += w[ok, j, None] * rows[ids[ok, j]]
    return v / (np.linalg.norm(v, axis=1, keepdims=True) + eps)


def topk64(scores, k):
    """mdx_topk's order in float64: descending score, ascending id on ties."""
    part = np.argpartition(-scores, k - 1, axis=1)[:, :k]
    vals = np.take_along_axis(scores, part, axis=1)
    order = np.lexsort((part, -vals), axis=1)
    return np.take_along_axis(part, order, axis=1), np.take_along_axis(vals, order, axis=1)


def clear_gaps(scores64, k, gap=1e-5):
    """[nq] True where the first k + 1 float64 scores of a row are pairwise further apart than `gap` (no near-tie can
    reorder the top-k between fp32 and float64)."""
    m = min(k + 1, scores64.shape[1])
    top = -np.sort(np.partition(-scores64, m - 1, axis=1)[:, :m], axis=1)
    return (np.abs(np.diff(top, axis=1)) > gap).all(axis=1)


def qe64(qvecs, vecs, k, alpha):
    x = vecs.astype(np.float64)
    s = qvecs.astype(np.float64) @ x.T
    ids, sims = topk64(s, min(k, x.shape[0]))
    qx = aggregate64(x, ids, sims, alpha, self_rows=qvecs)
    return qx @ x.T, qx, ids, s


def dba64(vecs, k, alpha):
    x = vecs.astype(np.float64)
    ids, sims = topk64(x @ x.T, min(k, x.shape[0]))
    return aggregate64(x, ids, sims, alpha)


# ---------------------------------------------------------------------------------------------------- the kernel

def _strided(a, extra):
    """``a`` as a row slice of a wider device matrix (row stride d + extra)."""
    base = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device=DEV)
    base[:, :a.shape[1]] = dev(a)
    return base[:, :a.shape[1]]


def _problem(rng, n, d, nq, k):
    rows = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    ids = rng.integers(0, n, (nq, k)).astype(np.int64)
    bad = rng.random((nq, k)) < 0.05                                 # ids outside [0, n): never read
    ids[bad] = rng.choice(np.array([-1, n, n + 7, -(1 << 40), 1 << 40], dtype=np.int64), bad.sum())
    sims = rng.uniform(-0.3, 1.0, (nq, k)).astype(np.float32)       # negative: weight 0
    sims[rng.random((nq, k)) < 0.05] = np.nan                        # NaN: weight 0
    self_rows = (rng.standard_normal((nq, d)) / np.sqrt(d)).astype(np.float32)
    return rows, ids, sims, self_rows


@pytest.mark.parametrize("d", [128, 2047, 2048])
@pytest.mark.parametrize("k", [1, 2, 10, 100])
@pytest.mark.parametrize("nq", [1, 70, 513])
def test_knn_aggregate_against_float64(d, k, nq):
    from mdir_amd import ops
    rng = np.random.default_rng(1000 * d + 10 * k + nq)
    n = 3001
    rows, ids, sims, self_rows = _problem(rng, n, d, nq, k)
    r_t, i_t, s_t, self_t = dev(rows), dev(ids), dev(sims), dev(self_rows)
    r_pad, self_pad = _strided(rows, 4), _strided(self_rows, 3)      # ld % 4 == 0 (dwordx4 path) / ld % 4 != 0 (dwords)
    for alpha in (0.0, 0.5, 3.0):
        for with_self in (False, True):
            want = aggregate64(rows, ids, sims, alpha, self_rows if with_self else None)
            got = ops.knn_aggregate(r_t, i_t, s_t, alpha, self_rows=self_t if with_self else None).cpu().numpy()
            assert np.isfinite(got).all()
            err = np.abs(got - want).max()
            assert err <= 2e-6, (alpha, with_self, err)
            # non-trivial strides on every operand: the same bits (each element's chain and the norm's order do not move)
            out_pad = _strided(np.zeros((nq, d), np.float32), 5)
            got2 = ops.knn_aggregate(r_pad, i_t, s_t, alpha, self_rows=self_pad if with_self else None, out=out_pad)
            assert np.array_equal(got2.cpu().numpy(), got), (alpha, with_self)
            assert torch.isnan(out_pad.as_strided((nq, 5), (d + 5, 1), d)).all()   # nothing written past d


def test_knn_aggregate_zero_weight_rows_are_zero():
    from mdir_amd import ops
    rng = np.random.default_rng(5)
    rows = unit_rows(rng, 500, 2048)
    ids = rng.integers(0, 500, (9, 10)).astype(np.int64)
    sims = -rng.random((9, 10)).astype(np.float32)
    sims[::2, ::3] = np.nan
    sims[1, :] = 0.0
    ids[2, :] = -1                                                   # and a row with no valid neighbour at all
    for alpha in (0.0, 3.0):
        got = ops.knn_aggregate(dev(rows), dev(ids), dev(sims), alpha).cpu().numpy()
        assert np.array_equal(got, np.zeros_like(got))               # exact zeros, no NaN, no -0 question: 0 / eps


def test_knn_aggregate_is_bit_deterministic_and_batch_independent():
    from mdir_amd import ops
    rng = np.random.default_rng(6)
    for d in (2048, 2047, 4099):                                     # 4099: two column passes, store then rescale
        rows, ids, sims, self_rows = _problem(rng, 4000, d, 513, 10)
        r_t, i_t, s_t, q_t = dev(rows), dev(ids), dev(sims), dev(self_rows)
        a = ops.knn_aggregate(r_t, i_t, s_t, 3.0, self_rows=q_t)
        b = ops.knn_aggregate(r_t, i_t, s_t, 3.0, self_rows=q_t)
        assert torch.equal(a, b)
        for q in (0, 1, 255, 512):
            alone = ops.knn_aggregate(r_t, i_t[q:q + 1].contiguous(), s_t[q:q + 1].contiguous(), 3.0, self_rows=q_t[q:q + 1])
            assert torch.equal(alone[0], a[q]), (d, q)
        if d == 4099:
            assert np.abs(a.cpu().numpy() - aggregate64(rows, ids, sims, 3.0, self_rows)).max() <= 2e-6


def test_knn_aggregate_refuses_overlap_and_bad_shapes():
    from mdir_amd import ops
    rows = torch.zeros((10, 64), device=DEV)
    ids = torch.zeros((3, 2), dtype=torch.int64, device=DEV)
    sims = torch.ones((3, 2), device=DEV)
    with pytest.raises(ValueError, match="overlaps rows"):
        ops.knn_aggregate(rows, ids, sims, 3.0, out=rows[4:7])
    with pytest.raises(ValueError, match="alpha"):
        ops.knn_aggregate(rows, ids, sims, -1.0)
    with pytest.raises(ValueError):
        ops.knn_aggregate(rows, ids, sims[:, :1].contiguous(), 3.0)


# ------------------------------------------------------------------------------------------------ alpha-QE, DBA

def test_query_expansion_rparis_shape_against_float64():
    from mdir_amd import ops, rerank
    from mdir_amd.evaluate import compute_map
    rng = np.random.default_rng(7)
    n, nq, d, k, alpha = 6322, 70, 2048, 2, 3.0
    vecs = unit_rows(rng, n, d)
    src = rng.choice(n, nq, replace=False)
    q = vecs[src] + 0.9 * unit_rows(rng, nq, d)
    qvecs = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x_t, q_t = dev(vecs), dev(qvecs)
    scores, expanded = rerank.query_expansion(q_t, x_t, k, alpha)
    want_scores, want_exp, want_ids, s64 = qe64(qvecs, vecs, k, alpha)
    ids, _ = ops.topk(ops.scores_rowmajor(x_t, q_t, "ND"), k)
    clear = clear_gaps(s64, k)
    assert clear.sum() >= nq - 2
    assert np.array_equal(ids.cpu().numpy()[clear], want_ids[clear])
    assert np.abs(expanded.cpu().numpy()[clear] - want_exp[clear]).max() <= 2e-6
    assert np.abs(scores.cpu().numpy()[clear] - want_scores[clear]).max() <= 5e-6

    # mAP on generated ground truth: the source row and a few random rows are positives, a couple junk
    gnd = [{"ok": [int(src[i])] + rng.choice(n, 4, replace=False).tolist(), "junk": rng.choice(n, 2, replace=False).tolist()}
           for i in range(nq)]
    got = compute_map(ops.rank_full(scores).t(), gnd, [1, 5, 10])
    want = O.compute_map(np.argsort(-want_scores, axis=1, kind="stable").T, gnd, [1, 5, 10])
    assert abs(got[0] - want[0]) <= 1e-6
    np.testing.assert_allclose(np.asarray(got[1]), np.asarray(want[1]), atol=1e-6)


def test_query_expansion_modes_and_edge_cases():
    from mdir_amd import ops, rerank
    rng = np.random.default_rng(8)
    vecs, qvecs = unit_rows(rng, 3000, 256), unit_rows(rng, 33, 256)
    x_t, q_t = dev(vecs), dev(qvecs)
    plain, exp_plain = rerank.query_expansion(q_t, x_t, 5, 0.0)
    ix = ops.DescriptorIndex(x_t, "ND")
    via_index, exp_index = rerank.query_expansion(q_t, x_t, 5, 0.0, index=ix)
    assert torch.equal(via_index, plain) and torch.equal(exp_index, exp_plain)     # the chain on an index: the same bits
    split, _ = rerank.query_expansion(q_t, x_t, 5, 0.0, index=ix, compute="split3")
    assert (split - plain).abs().max().item() <= 1e-5
    ix.close()
    # k beyond N is clamped to N: every database row is a neighbour
    small = x_t[:7].contiguous()
    _, e = rerank.query_expansion(q_t, small, 50, 1.0)
    assert np.abs(e.cpu().numpy() - qe64(qvecs, vecs[:7], 50, 1.0)[1]).max() <= 2e-6
    with pytest.raises(ValueError):
        rerank.query_expansion(q_t, x_t, 5, 0.0, compute="split3")                  # split modes need an index


def test_database_augmentation_against_float64_and_chunk_independent():
    from mdir_amd import ops, rerank
    rng = np.random.default_rng(9)
    n, d, k, alpha = 20000, 512, 10, 3.0
    vecs = unit_rows(rng, n, d)
    x_t = dev(vecs)
    before = x_t.clone()
    a = rerank.database_augmentation(x_t, k, alpha, chunk=7)
    b = rerank.database_augmentation(x_t, k, alpha, chunk=4096)
    c = rerank.database_augmentation(x_t, k, alpha)
    assert torch.equal(x_t, before)                                   # the input is not touched
    assert a.data_ptr() != x_t.data_ptr()
    assert torch.equal(a, b) and torch.equal(a, c)                    # chunk size changes nothing
    # float64: the library's neighbours equal float64's wherever no near-tie can reorder them, and the augmented rows
    # are the float64 aggregate of those neighbours
    x64 = vecs.astype(np.float64)
    got = a.cpu().numpy()
    worst, checked = 0.0, 0
    for i0 in range(0, n, 2500):
        s64 = x64[i0:i0 + 2500] @ x64.T
        ids64, sims64 = topk64(s64, k)
        lib_ids, _ = ops.topk(ops.scores_rowmajor(x_t, x_t[i0:i0 + 2500], "ND"), k)
        clear = clear_gaps(s64, k)
        assert np.array_equal(lib_ids.cpu().numpy()[clear], ids64[clear])
        want = aggregate64(x64, ids64[clear], sims64[clear], alpha)
        worst = max(worst, float(np.abs(got[i0:i0 + 2500][clear] - want).max()))
        checked += int(clear.sum())
    assert checked >= 0.9 * n
    assert worst <= 2e-6
    # the reference's [D, N] layout through one transpose copy: the same bits
    assert torch.equal(rerank.database_augmentation(x_t.t().contiguous(), k, alpha, layout="DN"), a)


def test_database_augmentation_small_cases():
    from mdir_amd import rerank
    rng = np.random.default_rng(10)
    for n, d, k in ((5, 64, 10), (300, 130, 3)):                     # k clamped to N; d % 4 != 0 through an index
        vecs = unit_rows(rng, n, d)
        got = rerank.database_augmentation(dev(vecs), k, 3.0).cpu().numpy()
        assert np.abs(got - dba64(vecs, k, 3.0)).max() <= 2e-6


def test_query_expansion_full_size():
    """configs[2]: N = 1 004 993, Q = 70, D = 2048, in well under a minute; checked on sampled queries against float64
    on their gathered neighbours (no full CPU product)."""
    from mdir_amd import ops, rerank
    n, nq, d, k, alpha = 1004993, 70, 2048, 2, 3.0
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    x_t = torch.randn((n, d), generator=g, device=DEV)
    x_t /= x_t.norm(dim=1, keepdim=True)
    src = torch.arange(0, n, n // nq, device=DEV)[:nq]
    q_t = x_t[src] + 0.8 * torch.randn((nq, d), generator=g, device=DEV)
    q_t = (q_t / q_t.norm(dim=1, keepdim=True)).contiguous()
    rerank.query_expansion(q_t[:1].contiguous(), x_t, k, alpha)           # warm: code objects, sort probe
    torch.cuda.synchronize()
    t0 = time.time()
    scores, expanded = rerank.query_expansion(q_t, x_t, k, alpha)
    torch.cuda.synchronize()
    assert time.time() - t0 < 60
    first = ops.scores_rowmajor(x_t, q_t, "ND")
    ids, sims = ops.topk(first, k)
    tv, _ = torch.topk(first, k + 1, dim=1)
    assert torch.equal(first.gather(1, ids), tv[:, :k])                    # the k best scores
    ids, sims, exp = ids.cpu().numpy(), sims.cpu().numpy(), expanded.cpu().numpy()
    qv = q_t.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(12)
    for q in rng.choice(nq, 8, replace=False):
        nb = x_t[torch.from_numpy(ids[q]).to(DEV)].cpu().numpy().astype(np.float64)
        s64 = nb @ qv[q]
        assert np.abs(s64 - sims[q]).max() <= 5e-6
        want = aggregate64(nb, np.arange(k)[None], sims[q][None], alpha, self_rows=qv[q][None])[0]
        assert np.abs(exp[q] - want).max() <= 2e-6
        cols = rng.choice(n, 64, replace=False)
        want_sc = x_t[torch.from_numpy(cols).to(DEV)].cpu().numpy().astype(np.float64) @ exp[q].astype(np.float64)
        assert np.abs(scores[q, torch.from_numpy(cols).to(DEV)].cpu().numpy() - want_sc).max() <= 5e-6


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


def test_eval_py_with_query_expansion_and_dba(tmp_path):
    """./eval.py on the generated roxford5k + 247tokyo1k set-up with both re-ranking keys: the printed numbers equal a
    float64 DBA + alpha-QE + compute_map on the descriptors the library extracted in that very run."""
    root = str(tmp_path / "synth")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_eval.py"), root], timeout=600)
    over = str(tmp_path / "rerank.yml")
    # DBA's k is kept small: the 15 Tokyo descriptors of the random-weight network are close to one another, and an
    # average over 10 of them makes rows so alike that fp32 and float64 may order their scores differently
    crit = "{query_expansion: {k: 2, alpha: 3.0}, database_augmentation: {k: 3, alpha: 3.0}}"
    with open(over, "w") as f:
        f.write("validation:\n  roxford5k: {criterion: %s}\n  247tokyo1k: {criterion: %s}\n" % (crit, crit))
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
    # extraction order of the run: roxford5k database, roxford5k queries (cropped), 247tokyo1k database (queries = database)
    desc = [np.load(os.path.join(dump, "desc%d.npy" % i)) for i in (1, 2, 3)]
    want, gaps = {}, {}
    for ds, label, key, vecs, qvecs in (("roxford5k", "roxford.5k medium", "ap_medium", desc[0], desc[1]),
                                        ("247tokyo1k", "247tokyo.1k", "ap", desc[2], desc[2])):
        cfg = configdataset(ds, os.path.join(root, "data", "test"))
        assert vecs.shape[0] == cfg["n"] and qvecs.shape[0] == cfg["nq"]
        db = dba64(vecs, 3, 3.0)
        scores, _, _, _ = qe64(qvecs, db, 2, 3.0)
        _, per = O.compute_map_and_print(ds, np.argsort(-scores, axis=1, kind="stable").T, cfg["gnd"])
        want[label] = round(100 * O.nanmean_metric(per[key]), 2)
        gaps[label] = float(np.diff(np.sort(scores, axis=1), axis=1).min())
    assert printed == want, (printed, want, "smallest float64 score gaps", gaps, out[-3000:])
