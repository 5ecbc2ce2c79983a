"""int8 shards (MDX_I8, include/mdx.h) on the MI355X: codes, scales and scores equal the numpy restatement of the contract
(tests/test_i8_host.py) bit for bit; the stated error bound, determinism, batch and shard independence; the ranking,
alpha-QE and eval.py on top of them."""
import numpy as np
import pytest
import torch

from test_i8_host import error_bound, quantize_np, scores_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rows(n, d, seed, special=True):
    """fp32 [n, d]: unit rows, and (special) an all-zero row, a single non-zero entry, a row whose x * inv fall exactly on
    k + 0.5 (a = 127 * 2^-8: inv = 2^8 exactly) and a row holding +-absmax twice."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30).astype(np.float32)
    if special and n >= 4:
        x[0] = 0
        x[1] = 0
        x[1, d // 2] = -0.375
        x[2] = (rng.integers(-126, 126, d) + 0.5).astype(np.float32) * np.float32(2.0 ** -8)
        x[2, 0] = np.float32(127 * 2.0 ** -8)
        x[3, 0], x[3, -1] = np.float32(0.75), np.float32(-0.75)
        x[3, 1:-1] = np.clip(x[3, 1:-1], -0.5, 0.5)
    return x


def restated(q, x, center=None):
    qc = q if center is None else (q - center[None, :]).astype(np.float32)
    cq, sq = quantize_np(qc)
    cx, sx = quantize_np(x)
    return scores_np(cq, sq, cx, sx)


# ------------------------------------------------------------------ codes and scales

@pytest.mark.parametrize("d", [1, 63, 64, 100, 2048, 4096])
@pytest.mark.parametrize("layout", ["ND", "DN"])
def test_quantize_i8_equals_the_restatement(d, layout):
    from mdir_amd import ops
    x = rows(300, d, seed=d)
    if d >= 4:
        x[4] = x[2] * np.float32(-1)                       # ties of the other sign
    src = dev(x if layout == "ND" else x.T)
    codes, scales = ops.quantize_i8(src, layout)
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (300, d) and tuple(scales.shape) == (300,)
    want_c, want_s = quantize_np(x)
    np.testing.assert_array_equal(codes.cpu().numpy(), want_c)
    np.testing.assert_array_equal(bits(scales.cpu().numpy()), bits(want_s))
    if d >= 4:
        assert not codes[0].any() and float(scales[0]) == 0.0
        assert int(codes[1, d // 2]) == -127 and int((codes[1] != 0).sum()) == 1
        assert int(codes[3, 0]) == 127 and int(codes[3, -1]) == -127


# ------------------------------------------------------------------ scores

SHAPES = [(1, 1, 1), (5, 3, 2), (17, 63, 5), (40, 65, 16), (333, 100, 17), (520, 300, 33), (4993, 2048, 70), (6322, 2048, 70),
          (75984, 512, 315), (1125, 512, 1125), (70000, 2048, 70), (5000, 256, 1), (5000, 256, 129), (40000, 192, 129),
          (33000, 64, 1)]


@pytest.mark.parametrize("n,d,nq", SHAPES)
def test_scores_equal_the_restatement(n, d, nq):
    from mdir_amd import ops
    x = rows(n, d, seed=n + d)
    rng = np.random.default_rng(nq)
    q = x[rng.integers(0, n, nq)] + np.float32(0.05) * rng.standard_normal((nq, d), dtype=np.float32)
    want = restated(q, x)
    ix = ops.DescriptorIndex(dev(x), "ND", row_offset=7, storage="i8")
    assert ix.row_offset == 7 and ix.device_bytes < n * d + 4096 * (d + 64)
    got = ix.scores(dev(q), "ND").cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(want))
    # both layouts of both matrices
    ixd = ops.DescriptorIndex(dev(x.T), "DN", storage="i8")
    np.testing.assert_array_equal(bits(ixd.scores(dev(q.T), "DN").cpu().numpy()), bits(want))


@pytest.mark.parametrize("n,d,nq", [(333, 100, 17), (6322, 2048, 70), (40000, 64, 129)])
@pytest.mark.parametrize("qlayout", ["ND", "DN"])
def test_scores_with_a_center(n, d, nq, qlayout):
    from mdir_amd import ops
    rng = np.random.default_rng(3)
    x = rows(n, d, seed=4)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    c = rng.normal(0, 0.1, d).astype(np.float32)
    ix = ops.DescriptorIndex(dev(x), "ND", storage="i8")
    got = ix.scores(dev(q if qlayout == "ND" else q.T), qlayout, center=dev(c)).cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(restated(q, x, c)))


def test_error_bound_against_the_unquantised_product():
    from mdir_amd import ops
    rng = np.random.default_rng(8)
    for n, d, nq in ((4000, 512, 40), (2000, 2048, 20), (500, 37, 9)):
        x = rows(n, d, seed=d, special=False)
        x[::5] *= np.float32(rng.uniform(0.01, 100.0))
        q = rng.standard_normal((nq, d), dtype=np.float32)
        s = ops.DescriptorIndex(dev(x), "ND", storage="i8").scores(dev(q), "ND").cpu().numpy()
        cx, sx = quantize_np(x)
        cq, sq = quantize_np(q)
        exact = q.astype(np.float64) @ x.astype(np.float64).T
        bound = error_bound(x, q, cx, sx, cq, sq, s)
        assert (np.abs(exact - s) <= bound).all()
        assert (np.abs(exact - s) / bound).max() > 1e-3                     # a worst-case bound, but not a vacuous one


def test_deterministic_batch_and_shard_independent():
    from mdir_amd import ops
    n, d, nq = 50000, 512, 150
    x = rows(n, d, seed=21)
    rng = np.random.default_rng(22)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    ix = ops.DescriptorIndex(dev(x), "ND", storage="i8")
    qd = dev(q)
    a = ix.scores(qd, "ND").cpu().numpy()
    np.testing.assert_array_equal(bits(ix.scores(qd, "ND").cpu().numpy()), bits(a))           # run to run
    for lo, hi in ((0, 1), (17, 18), (5, 70), (129, 150), (0, 129)):                             # other queries of the call
        np.testing.assert_array_equal(bits(ix.scores(dev(q[lo:hi]), "ND").cpu().numpy()), bits(a[lo:hi]))
    h = 23457                                                                                     # two shards, concatenated
    p1 = ops.DescriptorIndex(dev(x[:h]), "ND", storage="i8").scores(qd, "ND").cpu().numpy()
    p2 = ops.DescriptorIndex(dev(x[h:]), "ND", row_offset=h, storage="i8").scores(qd, "ND").cpu().numpy()
    np.testing.assert_array_equal(bits(np.concatenate([p1, p2], axis=1)), bits(a))


def test_refusals_on_the_device():
    from mdir_amd import ops
    x = dev(rows(100, 64, seed=1))
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    for compute in ("split3", "split2"):
        with pytest.raises(ValueError, match="stored as i8"):
            ix.scores(x, "ND", compute=compute)
    import ctypes
    from mdir_amd import _lib
    h = _lib.lib()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty((100, 100), dtype=torch.float32, device=DEV)
    rc = h.mdx_scores_ex(ix._h, ctypes.c_void_p(x.data_ptr()), 100, 1, None, ctypes.c_void_p(out.data_ptr()),
                         ctypes.c_void_p(ws.data_ptr()), 1 << 20, 1, None)
    assert rc == -1 and b"stored as int8" in h.mdx_last_error()


# ------------------------------------------------------------------ downstream

@pytest.mark.parametrize("n,d,nq", [(4993, 2048, 70), (1125, 512, 1125), (333, 100, 17)])
def test_ranking_of_int8_scores(n, d, nq):
    from mdir_amd import ops
    x = rows(n, d, seed=31)
    x[10:20] = x[30]                                                       # exact ties: ascending id
    rng = np.random.default_rng(32)
    q = x[rng.integers(0, n, nq)] + np.float32(0.02) * rng.standard_normal((nq, d), dtype=np.float32)
    want = restated(q, x)
    order = np.argsort(-want, axis=1, kind="stable")
    sc = ops.DescriptorIndex(dev(x), "ND", storage="i8").scores(dev(q), "ND")
    np.testing.assert_array_equal(ops.rank_full(sc).cpu().numpy(), order)
    ids, vals = ops.topk(sc, 50)
    np.testing.assert_array_equal(ids.cpu().numpy(), order[:, :50])
    np.testing.assert_array_equal(bits(vals.cpu().numpy()), bits(np.take_along_axis(want, order[:, :50], axis=1)))


def test_headline_shape_one_million_rows():
    """1 004 993 x 2048 x 70 (BASELINE.json configs[2] shape): sampled rows against numpy, every score against the exact
    restatement from the codes (float64 GEMM of integers on the device: exact), and all 70 ranking heads."""
    from mdir_amd import ops
    n, d, nq = 1004993, 2048, 70
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((n, d), device=DEV, generator=g)
    x /= x.norm(dim=1, keepdim=True)
    qi = torch.arange(0, n, n // nq, device=DEV)[:nq]
    q = (x[qi] + 0.05 * torch.randn((nq, d), device=DEV, generator=g)).contiguous()
    ix = ops.DescriptorIndex(x, "ND", storage="i8")
    assert ix.device_bytes == 62816 * (32 * 1024 + 64)
    sc = ix.scores(q, "ND")
    cx, sx = ops.quantize_i8(x, "ND")
    cq, sq = ops.quantize_i8(q, "ND")
    sample = np.sort(np.random.default_rng(6).choice(n, 3000, replace=False))
    xs = x[dev(sample)].cpu().numpy()
    wc, ws = quantize_np(xs)
    np.testing.assert_array_equal(cx[dev(sample)].cpu().numpy(), wc)
    np.testing.assert_array_equal(bits(sx[dev(sample)].cpu().numpy()), bits(ws))
    np.testing.assert_array_equal(bits(sc[:, dev(sample)].cpu().numpy()), bits(restated(q.cpu().numpy(), xs)))
    want = torch.empty((nq, n), dtype=torch.float32, device=DEV)
    cqd = cq.double()
    for lo in range(0, n, 131072):
        hi = min(n, lo + 131072)
        acc = cqd @ cx[lo:hi].double().T                                   # integers below 2^53: exact in any order
        want[:, lo:hi] = acc.float() * (sx[lo:hi][None, :] * sq[:, None])
    assert torch.equal(sc.view(torch.int32), want.view(torch.int32))
    ids, vals = ops.topk(sc, 100)
    wv, wi = torch.sort(want, dim=1, descending=True, stable=True)
    assert torch.equal(ids, wi[:, :100]) and torch.equal(vals.view(torch.int32), wv[:, :100].view(torch.int32))
    assert (ids[:, 0] == qi).float().mean() > 0.99


def test_query_expansion_on_an_int8_index():
    from mdir_amd import ops, rerank
    n, d, nq, k, alpha = 6000, 512, 40, 5, 3.0
    x = rows(n, d, seed=41, special=False)
    rng = np.random.default_rng(42)
    q = x[rng.integers(0, n, nq)] + np.float32(0.05) * rng.standard_normal((nq, d), dtype=np.float32)
    xd, qd = dev(x), dev(q)
    ix = ops.DescriptorIndex(xd, "ND", storage="i8")
    got, expanded = rerank.query_expansion(qd, xd, k, alpha, index=ix)
    s1 = restated(q, x)
    top = np.argsort(-s1, axis=1, kind="stable")[:, :k]
    sims = np.take_along_axis(s1, top, axis=1)
    want_exp = ops.knn_aggregate(xd, dev(top), dev(sims), alpha, self_rows=qd)
    assert torch.equal(expanded.view(torch.int32), want_exp.view(torch.int32))
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(restated(want_exp.cpu().numpy(), x)))


def test_eval_int8_overlay_end_to_end(tmp_path, monkeypatch):
    """eval.py's validation stage with scenarios/eval_int8.yml on a 247tokyo1k-shaped synthetic set (VGG16-GeM, 3 scales,
    learned whitening, as test_gpu_f16.py's configs[4] test): the mAP it reports is compute_map's on the numpy-restated
    int8 scores of the descriptors it indexed, ranked by stable descending order."""
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
    result = stages.validate(scenario(os.path.join(root, "eval_synth.yml"), "eval_int8.yml"), ())[0]["eval"]
    assert len(indexed) == 1
    vecs = indexed[0]
    assert vecs.shape == (n_images, 512)
    s = restated(vecs, vecs)                                                # query == database on this set
    ranks = np.argsort(-s, axis=1, kind="stable").T                         # [N, Q], as np.argsort(-scores, axis=0)
    want_map, aps = compute_map(ranks, cfg["gnd"])[:2]
    assert 0.05 < want_map < 0.999, want_map
    print(">> 247tokyo1k (int8): mAP %.6f, restated %.6f" % (result["247tokyo1k/validation/score:ap_avg.4"], np.nanmean(aps)))
    assert abs(result["247tokyo1k/validation/score:ap_avg.4"] - np.nanmean(aps)) <= 1e-12
