"""Exact rescoring of shortlists and its certificate on the MI355X (include/mdx.h mdx_rescore / mdx_index_i8_bounds /
mdx_rescore_certify): rescored scores bit-equal to the fp32 index, the rank order, the certified depth sound against the exact
top-k (random, clustered, near-tied and 1 M-row data), the device bound against the float64 restatement of
tests/test_rescore_host.py, search(exact=True), determinism and eval.py."""
import numpy as np
import pytest
import torch

from test_i8_host import quantize_np, scores_np
from test_rescore_host import bounds_np, depth_np, rank_order, upper_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30).astype(np.float32)
    return x


def clustered_rows(rng, n, d, clusters=20, spread=0.05):
    c = unit_rows(rng, clusters, d)
    x = c[rng.integers(0, clusters, n)] + spread * rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return x.astype(np.float32)


def expected(full, ids, n):
    """Rescore's output restated from a full [nq, n] score matrix: scores at ids (NaN outside [0, n)), rank order."""
    nq, K = ids.shape
    out_ids = np.empty_like(ids)
    out_sc = np.empty((nq, K), np.float32)
    for q in range(nq):
        inside = (ids[q] >= 0) & (ids[q] < n)
        sc = np.full(K, np.nan, np.float32)
        sc[inside] = full[q, ids[q][inside]]
        out_ids[q], out_sc[q] = rank_order(sc, ids[q])
    return out_ids, out_sc


# ------------------------------------------------------------------ 1. bit-equality and order

@pytest.mark.parametrize("d", [1, 3, 100, 2048])
@pytest.mark.parametrize("K", [1, 7, 1000, 4096])
def test_rescore_equals_the_fp32_index(d, K):
    from mdir_amd import ops
    rng = np.random.default_rng(d * 7919 + K)
    n, nq = 4500, 5
    x = unit_rows(rng, n, d)
    x[10] = x[20]                                            # duplicate rows: equal scores, ascending id
    x[30] = 0                                                # a zero row: +0 scores
    x[31] = -0.0
    rows = dev(x)
    index = ops.DescriptorIndex(rows, "ND")
    for qlayout, with_center in (("ND", False), ("DN", True), ("ND", True), ("DN", False)):
        qn = unit_rows(rng, nq, d)
        qn[1] = x[10]
        q = qn if qlayout == "ND" else np.ascontiguousarray(qn.T)
        center = dev(rng.normal(0, 0.01, d).astype(np.float32)) if with_center else None
        full = index.scores(dev(q), qlayout, center=center).cpu().numpy()
        ids = np.stack([rng.permutation(n)[:K] for _ in range(nq)]).astype(np.int64)
        ids[0, :3 if K >= 3 else K] = [-1, n, n + 5][:min(K, 3)]     # out of range: NaN, sorted last
        if K >= 40:
            special = np.array([10, 20, 30, 31])
            rest = rng.permutation(np.setdiff1d(np.arange(n), special))
            ids[1] = np.concatenate([special, rest])[:K]
        got_ids, got_sc = ops.rescore(rows, dev(q), dev(ids), qlayout, center)
        want_ids, want_sc = expected(full, ids, n)
        np.testing.assert_array_equal(got_ids.cpu().numpy(), want_ids)
        np.testing.assert_array_equal(bits(got_sc.cpu().numpy()), bits(want_sc))
        if d % 4 == 0:
            rm = ops.scores_rowmajor(rows, dev(q), qlayout, center).cpu().numpy()
            np.testing.assert_array_equal(bits(rm), bits(full))
    index.close()


def test_rescore_reads_rows_at_a_stride_and_in_place_ids():
    from mdir_amd import ops
    rng = np.random.default_rng(3)
    n, d, ld, nq, K = 700, 100, 103, 3, 50
    big = dev(unit_rows(rng, n, ld))
    rows = big[:, :d]                                         # stride 103, not 16-byte aligned rows
    q = dev(unit_rows(rng, nq, d))
    full = ops.DescriptorIndex(rows.contiguous(), "ND").scores(q, "ND").cpu().numpy()
    ids = np.stack([rng.permutation(n)[:K] for _ in range(nq)]).astype(np.int64)
    got_ids, got_sc = ops.rescore(rows, q, dev(ids), "ND")
    want_ids, want_sc = expected(full, ids, n)
    np.testing.assert_array_equal(got_ids.cpu().numpy(), want_ids)
    np.testing.assert_array_equal(bits(got_sc.cpu().numpy()), bits(want_sc))


# ------------------------------------------------------------------ 2. soundness of the certificate

def _pipeline(rows, q, K, center=None, qlayout="ND"):
    from mdir_amd import ops
    index = ops.DescriptorIndex(rows, "ND", storage="i8")
    s8 = index.scores(q, qlayout, center=center)
    top_ids, top_sc = ops.topk(s8, K)
    ids, sc = ops.rescore(rows, q, top_ids, qlayout, center)
    depth, upper = ops.rescore_certify(sc, top_sc[:, K - 1], q, index.i8_bounds(), rows.shape[0], qlayout, center)
    out = dict(s8=s8, top_ids=top_ids, top_sc=top_sc, ids=ids, sc=sc, depth=depth, upper=upper, bounds=index.i8_bounds().clone())
    index.close()
    return out


def _assert_sound(rows, q, r, K, center=None, qlayout="ND"):
    from mdir_amd import ops
    ex_ids, ex_sc = ops.topk(ops.scores_rowmajor(rows, q, qlayout, center), K)
    ex_ids, ex_sc = ex_ids.cpu().numpy(), ex_sc.cpu().numpy()
    ids, sc, depth = r["ids"].cpu().numpy(), r["sc"].cpu().numpy(), r["depth"].cpu().numpy()
    for i in range(len(depth)):
        c = depth[i]
        np.testing.assert_array_equal(ids[i, :c], ex_ids[i, :c])
        np.testing.assert_array_equal(bits(sc[i, :c]), bits(ex_sc[i, :c]))
    return depth


@pytest.mark.parametrize("kind", ["random", "clustered"])
@pytest.mark.parametrize("d,K", [(64, 100), (256, 1000), (2048, 100)])
def test_certified_prefix_is_the_exact_top(kind, d, K):
    rng = np.random.default_rng(d + K)
    n, nq = 20000, 24
    x = unit_rows(rng, n, d) if kind == "random" else clustered_rows(rng, n, d)
    q = x[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, d), dtype=np.float32)
    rows, qd = dev(x), dev(q.astype(np.float32))
    depth = _assert_sound(rows, qd, _pipeline(rows, qd, K), K)
    print("%s d=%d K=%d: depth min %d median %g max %d" % (kind, d, K, depth.min(), np.median(depth), depth.max()))
    if kind == "clustered":
        assert depth.max() > 0


def test_certified_prefix_with_a_center_and_dim_major_queries():
    rng = np.random.default_rng(8)
    n, d, nq, K = 5000, 128, 9, 200
    x = clustered_rows(rng, n, d)
    q = np.ascontiguousarray((x[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, d))).astype(np.float32).T)
    center = dev(rng.normal(0, 0.01, d).astype(np.float32))
    rows, qd = dev(x), dev(q)
    _assert_sound(rows, qd, _pipeline(rows, qd, K, center=center, qlayout="DN"), K, center=center, qlayout="DN")


def test_headline_shape_one_million_rows():
    from mdir_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    n, d, nq, K = 1004993, 2048, 8, 1000
    rows = torch.randn((n, d), device=DEV, generator=g)
    rows /= rows.norm(dim=1, keepdim=True)
    q = rows[torch.arange(0, n, n // nq, device=DEV)[:nq]] + 0.05 * torch.randn((nq, d), device=DEV, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    r = _pipeline(rows, q, K)
    depth = _assert_sound(rows, q, r, K)
    print("1M x 2048, K=%d: depth %s" % (K, depth.tolist()))
    assert depth.min() >= 1                                   # a self-near query's top row is certified
    del rows
    torch.cuda.empty_cache()
    assert ops.RESCORE_MAX_K == 4096


# ------------------------------------------------------------------ 3. the feature does something

def test_rescoring_fixes_an_int8_top_k_and_certifies_it():
    rng = np.random.default_rng(21)
    n, d, k, K = 3000, 256, 10, 50
    x = unit_rows(rng, n, d)
    base = unit_rows(rng, 1, d)[0]
    for j in range(k):                                        # k near-duplicates: their int8 order is scrambled
        v = base + 3e-3 * rng.standard_normal(d).astype(np.float32)
        x[100 + 37 * j] = v / np.linalg.norm(v)
    q = base[None, :].copy()
    rows, qd = dev(x), dev(q)
    r = _pipeline(rows, qd, K)
    from mdir_amd import ops
    ex_ids, ex_sc = ops.topk(ops.scores_rowmajor(rows, qd, "ND"), k)
    i8_top = r["top_ids"].cpu().numpy()[0, :k]
    assert not np.array_equal(i8_top, ex_ids.cpu().numpy()[0]), "the int8 top-k happens to be exact; pick another seed"
    np.testing.assert_array_equal(r["ids"].cpu().numpy()[0, :k], ex_ids.cpu().numpy()[0])
    np.testing.assert_array_equal(bits(r["sc"].cpu().numpy()[0, :k]), bits(ex_sc.cpu().numpy()[0]))
    assert r["depth"].cpu().numpy()[0] >= k


def _near_tie_problem():
    """Rows a, b with chain(a) > chain(b) but int8(b) > int8(a), and a far row: found on the host with the restatement."""
    from oracle import chain
    rng = np.random.default_rng(99)
    d = 64
    for _ in range(20000):
        q = unit_rows(rng, 1, d)
        a = q[0] + 3e-3 * rng.standard_normal(d).astype(np.float32)
        b = q[0] + 3e-3 * rng.standard_normal(d).astype(np.float32)
        x = np.stack([b, a, -q[0]]).astype(np.float32)
        cx, sx = quantize_np(x)
        cq, sq = quantize_np(q)
        s8 = scores_np(cq, sq, cx, sx)[0]
        ex = chain.gemm_nt_chain(q, x)[0]
        if ex[1] > ex[0] and s8[0] > s8[1]:
            return x, q
    raise AssertionError("no near tie found")


def test_near_tie_outside_a_one_row_shortlist_gets_no_certificate():
    x, q = _near_tie_problem()
    rows, qd = dev(x), dev(q)
    r = _pipeline(rows, qd, 1)
    assert r["top_ids"].cpu().numpy()[0, 0] == 0              # the int8 shortlist holds b ...
    from mdir_amd import ops
    ex_ids, _ = ops.topk(ops.scores_rowmajor(rows, qd, "ND"), 1)
    assert ex_ids.cpu().numpy()[0, 0] == 1                    # ... the exact top-1 is a
    assert r["depth"].cpu().numpy()[0] == 0


# ------------------------------------------------------------------ 4. the device bound against the restatement

def _unpack(b):
    from mdir_amd import ops
    v = ops.unpack_i8_bounds(b)
    return v["s_max"], v["s_min"], v["l_max"], v["flag"]


@pytest.mark.parametrize("d", [3, 100, 512])
def test_upper_against_the_float64_restatement(d):
    rng = np.random.default_rng(d)
    n, nq, K = 4000, 12, 100
    x = clustered_rows(rng, n, d)
    q = (x[rng.integers(0, n, nq)] + 0.03 * rng.standard_normal((nq, d))).astype(np.float32)
    r = _pipeline(dev(x), dev(q), K)
    b = _unpack(r["bounds"])
    want = bounds_np(x)
    assert b == want
    t = r["top_sc"].cpu().numpy()[:, K - 1]
    u = upper_np(t, q, want, d)
    got = r["upper"].cpu().numpy().astype(np.float64)
    assert not np.isnan(u).any()
    assert (got >= u).all()
    assert (got - u <= 1e-5 * np.abs(u)).all(), np.max((got - u) / np.abs(u))
    np.testing.assert_array_equal(r["depth"].cpu().numpy(), depth_np(r["sc"].cpu().numpy(), got, n))


def test_void_rules_on_the_device():
    rng = np.random.default_rng(4)
    n, d, nq, K = 600, 64, 4, 20
    x = clustered_rows(rng, n, d, clusters=4)
    q = (x[:nq] + 0.01 * rng.standard_normal((nq, d))).astype(np.float32)
    base = _pipeline(dev(x), dev(q), K)["depth"].cpu().numpy()
    assert base.max() > 0
    # an infinite element: the shard's flag, no certificate anywhere
    xi = x.copy()
    xi[300, 5] = np.inf
    r = _pipeline(dev(xi), dev(q), K)
    assert _unpack(r["bounds"])[3] == 1 and (r["depth"].cpu().numpy() == 0).all()
    # a row with 0 < a < 2^-100
    xt = x.copy()
    xt[301] = 0
    xt[301, 7] = np.float32(2.0 ** -110)
    r = _pipeline(dev(xt), dev(q), K)
    assert _unpack(r["bounds"])[3] == 1 and (r["depth"].cpu().numpy() == 0).all()
    # a NaN row leaves no trace in the codes and needs none: its chain is NaN and ranks last; the prefix stays sound
    xn = x.copy()
    xn[302, 1:] = np.nan
    rows = dev(xn)
    r = _pipeline(rows, dev(q), K)
    assert _unpack(r["bounds"])[3] == 0
    _assert_sound(rows, dev(q), r, K)
    # a query with a NaN: that query alone has no certificate
    qn = q.copy()
    qn[2, 3] = np.nan
    r = _pipeline(dev(x), dev(qn), K)
    dq = r["depth"].cpu().numpy()
    assert dq[2] == 0 and (dq[[0, 1, 3]] == base[[0, 1, 3]]).all()
    # K == n: every entry
    r = _pipeline(dev(xi[:K]), dev(q), K)
    assert (r["depth"].cpu().numpy() == K).all()


# ------------------------------------------------------------------ 5. search(exact=True)

@pytest.mark.parametrize("storage", ["i8", "f16"])
def test_search_exact_equals_the_fp32_top_k(storage):
    from mdir_amd import ops
    from mdir_amd.search import search
    rng = np.random.default_rng(17)
    n, d, nq, k, K = 8000, 128, 20, 10, 64
    x = clustered_rows(rng, n, d)
    q = (x[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    q[3] = unit_rows(rng, 1, d)[0]                           # a query far from everything: likely uncertified
    rows, qd = dev(x), dev(q)
    index = ops.DescriptorIndex(rows, "ND", storage=storage)
    res = search(index, rows, qd, k, K, exact=True)
    ex_ids, ex_sc = ops.topk(ops.scores_rowmajor(rows, qd, "ND"), k)
    np.testing.assert_array_equal(res.ids.cpu().numpy(), ex_ids.cpu().numpy())
    np.testing.assert_array_equal(bits(res.scores.cpu().numpy()), bits(ex_sc.cpu().numpy()))
    fb = res.fallback.cpu().numpy()
    if storage == "f16":
        assert res.certified is None and fb.tolist() == list(range(nq))
    else:
        c = res.certified.cpu().numpy()
        assert fb.tolist() == np.nonzero(c < k)[0].tolist()
        plain = search(index, rows, qd, k, K)
        assert plain.fallback.numel() == 0
        ok = c >= k
        np.testing.assert_array_equal(plain.ids.cpu().numpy()[ok], ex_ids.cpu().numpy()[ok])
    with pytest.raises(ValueError, match="k=11"):
        search(index, rows, qd, 11, 10)
    index.close()
    x3 = dev(unit_rows(rng, 100, 3))
    i3 = ops.DescriptorIndex(x3, "ND", storage="i8")
    with pytest.raises(ValueError, match="d % 4 == 0"):
        search(i3, x3, dev(unit_rows(rng, 2, 3)), 1, 5, exact=True)
    i3.close()


# ------------------------------------------------------------------ 6. determinism and batch independence

def test_deterministic_and_independent_of_the_batch():
    from mdir_amd import ops
    rng = np.random.default_rng(12)
    n, d, nq, K = 5000, 200, 37, 333
    x = clustered_rows(rng, n, d)
    q = (x[rng.integers(0, n, nq)] + 0.03 * rng.standard_normal((nq, d))).astype(np.float32)
    rows, qd = dev(x), dev(q)
    a = _pipeline(rows, qd, K)
    b = _pipeline(rows, qd, K)
    for key in ("ids", "depth"):
        assert torch.equal(a[key], b[key])
    for key in ("sc", "upper"):
        np.testing.assert_array_equal(bits(a[key].cpu().numpy()), bits(b[key].cpu().numpy()))
    sub = [5, 0, 36, 17]
    ids_sub, sc_sub = ops.rescore(rows, qd[sub], a["top_ids"][sub], "ND")
    np.testing.assert_array_equal(ids_sub.cpu().numpy(), a["ids"].cpu().numpy()[sub])
    np.testing.assert_array_equal(bits(sc_sub.cpu().numpy()), bits(a["sc"].cpu().numpy()[sub]))
    index = ops.DescriptorIndex(rows, "ND", storage="i8")
    dep, up = ops.rescore_certify(sc_sub, a["top_sc"][sub, K - 1], qd[sub], index.i8_bounds(), n)
    np.testing.assert_array_equal(dep.cpu().numpy(), a["depth"].cpu().numpy()[sub])
    np.testing.assert_array_equal(bits(up.cpu().numpy()), bits(a["upper"].cpu().numpy()[sub]))
    # another batch around the same query: the same bits
    other = np.concatenate([unit_rows(rng, 3, d), q[9:10]]).astype(np.float32)
    ids_o, sc_o = ops.rescore(rows, dev(other), a["top_ids"][[0, 1, 2, 9]], "ND")
    np.testing.assert_array_equal(ids_o.cpu().numpy()[3], a["ids"].cpu().numpy()[9])
    np.testing.assert_array_equal(bits(sc_o.cpu().numpy()[3]), bits(a["sc"].cpu().numpy()[9]))
    index.close()


# ------------------------------------------------------------------ 7. eval.py

def test_eval_int8_rescore_overlay_end_to_end(tmp_path, monkeypatch):
    """eval.py's validation stage with scenarios/eval_int8_rescore.yml on the 247tokyo1k-shaped synthetic set (as
    test_gpu_i8.py's overlay test): the mAP equals compute_map on the restated composite ranking, for the overlay's
    shortlist (clamped to N) and for a shortlist below N, with ranking "positions" and "full" alike."""
    import os
    import pickle
    import subprocess
    import sys
    import yaml
    from conftest import ROOT
    from mdir_amd import ops, score, stages
    from mdir_amd.datasets import configdataset, initialize_transforms
    from mdir_amd.evaluate import compute_map
    from mdir_amd.network import load_network
    from mdir_amd.networks import extract_vectors_device
    from mdir_amd.scenario import dict_deep_overlay
    from mdir_amd.whiten import pcawhitenlearn
    from oracle import chain
    n_images = 90
    root = str(tmp_path / "synth")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_eval.py"), root, "vgg16", str(n_images)])
    monkeypatch.setenv("CIRTORCH_ROOT", root)
    monkeypatch.setenv("MDIR_AMD_WORKERS", "2")

    def scenario(*overlays):
        sc = {}
        for name in ("eval.yml",) + overlays:
            path = name if os.path.isabs(name) else os.path.join(ROOT, "scenarios", name)
            sc = dict_deep_overlay(sc, yaml.safe_load(open(path)))
        sc["validation"].pop("roxford5k")
        return sc

    raw = scenario(os.path.join(root, "eval_synth.yml"))
    raw["network"]["runtime"]["wrappers"]["eval"].pop("0_cirwhiten")
    cfg = configdataset("247tokyo1k", os.path.join(root, "data", "test"))
    images = [cfg["im_fname"](cfg, i) for i in range(cfg["n"])]
    net_raw = load_network(raw["network"], torch.device(DEV)).eval()
    tr = initialize_transforms("pil2np | totensor | normalize", net_raw.network_params.runtime["data"]["mean_std"])
    with torch.no_grad():
        X = extract_vectors_device(net_raw, images, 320, tr, device=torch.device(DEV)).cpu().numpy().astype(np.float64).T
    m, P = pcawhitenlearn(X, shrink=32, device=DEV)
    with open(os.path.join(root, "whiten.pkl"), "wb") as f:
        pickle.dump({"m": m, "P": np.real(P)}, f)

    indexed = []
    real = ops.DescriptorIndex

    def recording(vecs, *args, **kwargs):
        if kwargs.get("storage") == "i8":
            indexed.append(vecs.detach().cpu().numpy().copy())
        return real(vecs, *args, **kwargs)

    monkeypatch.setattr(score.ops, "DescriptorIndex", recording)
    key = "247tokyo1k/validation/score:ap_avg.4"
    results = {}
    for name, crit in (("overlay", None), ("k40", {"rescore": {"shortlist": 40}}),
                       ("k40_full", {"rescore": {"shortlist": 40}, "ranking": "full"})):
        overlays = [os.path.join(root, "eval_synth.yml"), "eval_int8_rescore.yml"]
        if crit:
            path = str(tmp_path / ("%s.yml" % name))
            with open(path, "w") as f:
                yaml.safe_dump({"validation": {"247tokyo1k": {"criterion": crit}}}, f)
            overlays.append(path)
        results[name] = stages.validate(scenario(*overlays), ())[0]["eval"][key]
    assert len(indexed) == 3
    vecs = indexed[0]
    assert vecs.shape == (n_images, 512)
    cx, sx = quantize_np(vecs)
    s8 = scores_np(cx, sx, cx, sx)                                       # query == database on this set
    exact = chain.gemm_nt_chain(vecs, vecs)
    r8 = chain.rank_full(s8)
    for name, K in (("overlay", min(100, n_images)), ("k40", 40)):
        ranks = r8.copy()
        for qi in range(n_images):
            ranks[qi, :K] = rank_order(exact[qi, r8[qi, :K]], r8[qi, :K])[0]
        want = np.nanmean(compute_map(ranks.T, cfg["gnd"])[1])
        print(">> 247tokyo1k (int8, rescore %d): mAP %.6f, restated %.6f" % (K, results[name], want))
        assert abs(results[name] - want) <= 1e-12
    assert results["k40"] == results["k40_full"]
