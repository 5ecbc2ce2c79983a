"""Truncated diffusion without a GPU: the three new C entry points are exported and declared, refuse every bad argument
before they launch anything and size their workspace right; the evaluation surface validates `diffusion: {truncate}`; the
Python layers check their arguments before any device work."""
import ctypes
import os

import pytest

from conftest import ROOT

P = ctypes.c_void_p
A, B, C, D, E, F, G, H = (P(0x100000 * i) for i in range(1, 9))
WS = P(0x10000000)
NEW = ("mdx_knn_graph_weights", "mdx_diffusion_truncated_workspace", "mdx_diffusion_truncated")


def _handle():
    from mdir_amd import _lib
    _lib.build()
    return _lib.lib()


def test_truncated_symbols_are_exported_and_declared():
    from mdir_amd import _lib, ops
    h = _handle()
    header = open(os.path.join(ROOT, "include", "mdx.h")).read()
    for name in NEW:
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in header, name
    assert "#define MDX_DIFFUSION_MAX_R 4096" in header
    assert ops.DIFFUSION_MAX_R == 4096
    assert h.mdx_abi_version() == 3


def _ru(x, m=256):
    return (x + m - 1) // m * m


@pytest.mark.parametrize("n, k, nq, r", [(1004993, 50, 70, 1000), (1004993, 50, 70, 4096), (4993, 50, 1, 1),
                                         (100, 7, 300, 100), (5000, 1, 3, 13), (10, 3, 2, 10)])
def test_truncated_workspace_formula(n, k, nq, r):
    h = _handle()
    assert h.mdx_diffusion_truncated_workspace(n, k, nq, r) == nq * (_ru(8 * k * r) + 2 * _ru(4 * r))


def test_truncated_workspace_refuses_bad_shapes():
    h = _handle()
    for args in ((0, 50, 70, 10), (100, 0, 70, 10), (100, 50, 0, 10), (100, 50, 7, 0), (5000, 50, 7, 4097),
                 (100, 50, 7, 101), (5000, 1 << 21, 7, 10), (5000, 50, 1 << 31, 10)):
        assert h.mdx_diffusion_truncated_workspace(*args) == 0, args


def _weights(h, ids=A, sims=B, n=100, k=5, gamma=3.0, cols=C, w=D, counts=E, ws=WS, ws_bytes=1 << 20):
    return h.mdx_knn_graph_weights(ids, sims, n, k, gamma, cols, w, counts, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, status, words", [
    ({"ids": None}, -1, b"NULL"), ({"sims": None}, -1, b"NULL"), ({"cols": None}, -1, b"NULL"),
    ({"w": None}, -1, b"NULL"), ({"counts": None}, -1, b"NULL"), ({"ws": None}, -1, b"NULL"),
    ({"n": 0}, -1, b"n=0"), ({"k": 0}, -1, b"k=0"), ({"n": -4}, -1, b"n=-4"), ({"n": 1 << 31}, -1, b"2^31"),
    ({"k": (1 << 20) + 1}, -1, b"too large"),
    ({"gamma": -1.0}, -1, b"gamma"), ({"gamma": float("nan")}, -1, b"gamma"), ({"gamma": float("inf")}, -1, b"gamma"),
    ({"ws_bytes": 399}, -4, b"workspace"),
])
def test_knn_graph_weights_argument_checks(bad, status, words):
    h = _handle()
    assert _weights(h, **bad) == status
    msg = h.mdx_last_error()
    assert msg.startswith(b"mdx_knn_graph_weights") and words in msg, msg


def _solve(h, cols=A, w=B, counts=C, n=100, k=5, scores=D, ld_scores=100, top_ids=E, top_sims=F, nq=7, r=20, kq=3,
           gamma=3.0, alpha=0.99, iters=20, tol=1e-6, out=G, ld_out=100, residual=None, steps=None, ws=WS, ws_bytes=1 << 30):
    return h.mdx_diffusion_truncated(cols, w, counts, n, k, scores, ld_scores, top_ids, top_sims, nq, r, kq, gamma, alpha,
                                     iters, tol, out, ld_out, residual, steps, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, status, words", [
    ({"cols": None}, -1, b"NULL"), ({"w": None}, -1, b"NULL"), ({"counts": None}, -1, b"NULL"),
    ({"scores": None}, -1, b"NULL"), ({"top_ids": None}, -1, b"NULL"), ({"top_sims": None}, -1, b"NULL"),
    ({"out": None}, -1, b"NULL"), ({"ws": None}, -1, b"NULL"),
    ({"n": 0, "ld_scores": 0, "ld_out": 0}, -1, b"n=0"), ({"k": 0}, -1, b"k=0"), ({"nq": 0}, -1, b"nq=0"),
    ({"r": 0}, -1, b"r=0"), ({"r": -1}, -1, b"r=-1"), ({"kq": 0}, -1, b"kq=0"), ({"kq": -2}, -1, b"kq=-2"),
    ({"n": 5000, "ld_scores": 5000, "ld_out": 5000, "r": 4097}, -1, b"r=4097"), ({"r": 101}, -1, b"r=101"),
    ({"n": 1 << 31, "ld_scores": 1 << 31, "ld_out": 1 << 31}, -1, b"2^31"), ({"k": (1 << 20) + 1}, -1, b"too large"),
    ({"nq": 1 << 31}, -1, b"too large"),
    ({"ld_scores": 99}, -1, b"ld_scores=99"), ({"ld_out": 50}, -1, b"ld_out=50"),
    ({"gamma": -0.5}, -1, b"gamma"), ({"gamma": float("nan")}, -1, b"gamma"), ({"gamma": float("inf")}, -1, b"gamma"),
    ({"alpha": -0.1}, -1, b"alpha"), ({"alpha": 1.0}, -1, b"alpha"), ({"alpha": 1.5}, -1, b"alpha"),
    ({"alpha": float("nan")}, -1, b"alpha"),
    ({"iters": 0}, -1, b"iters=0"), ({"iters": -3}, -1, b"iters=-3"),
    ({"tol": -1e-6}, -1, b"tol"), ({"tol": float("nan")}, -1, b"tol"), ({"tol": float("inf")}, -1, b"tol"),
    ({"out": P(0x400000 + 4 * 100 * 3)}, -1, b"overlaps scores"),          # out starts on scores' fourth row
    ({"out": D, "ld_out": 101}, -1, b"overlaps scores"),                    # in place, but with another stride
    ({"ws_bytes": 4096}, -4, b"workspace"),
    ({"ws": P(0x10000008)}, -1, b"aligned"),
])
def test_diffusion_truncated_argument_checks(bad, status, words):
    h = _handle()
    assert _solve(h, **bad) == status
    msg = h.mdx_last_error()
    assert msg.startswith(b"mdx_diffusion_truncated") and words in msg, msg


# ----------------------------------------------------------------------------------------------- evaluation surface

def _dataset(tmp_path):
    (tmp_path / "db.csv").write_text("identifier\na.jpg\nb.jpg\nc.jpg\n")
    (tmp_path / "q.tsv").write_text('query\tbbx\tok\tjunk\na.jpg\t\t["b.jpg"]\t[]\n')
    return {"name": "toy", "imgdir": "/img", "queries": str(tmp_path / "q.tsv"), "db": str(tmp_path / "db.csv")}


def _score(tmp_path, **criterion):
    from mdir_amd.score import initialize_score
    params = {"type": "cirdatasetap", "image_size": 64, "transforms": "pil2np | totensor | normalize",
              "mean_std": [[0.4] * 3, [0.2] * 3], "dataset": _dataset(tmp_path)}
    params.update(criterion)
    return initialize_score(params)


DEFAULTS = {"k": 50, "kq": 10, "gamma": 3.0, "alpha": 0.99, "iters": 20, "tol": 1e-6}
GIVEN = {"k": 7, "kq": 3, "gamma": 1, "alpha": 0.5, "iters": 5, "tol": 0}


@pytest.mark.parametrize("mask", range(64))
def test_truncate_with_every_subset_of_diffusion_keys(tmp_path, mask):
    keys = sorted(DEFAULTS)
    given = {key: GIVEN[key] for i, key in enumerate(keys) if mask >> i & 1}
    given["truncate"] = 1000
    s = _score(tmp_path, diffusion=given)
    assert s.diffusion == dict(DEFAULTS, **given)
    assert isinstance(s.diffusion["truncate"], int)


def test_truncate_absent_stays_absent(tmp_path):
    assert "truncate" not in _score(tmp_path, diffusion={"k": 5}).diffusion
    from mdir_amd import rerank
    assert "truncate" not in rerank.DIFFUSION_DEFAULTS


@pytest.mark.parametrize("truncate", [10, 11, 1000, 4096])
def test_truncate_bounds_accepted(tmp_path, truncate):
    assert _score(tmp_path, diffusion={"truncate": truncate}).diffusion["truncate"] == truncate


@pytest.mark.parametrize("value", [
    {"truncate": 0}, {"truncate": -1}, {"truncate": 2.5}, {"truncate": True}, {"truncate": False}, {"truncate": "1000"},
    {"truncate": 4097}, {"truncate": 9}, {"truncate": None}, {"truncate": 1000.0}, {"kq": 20, "truncate": 19},
])
def test_truncate_bad_values_rejected(tmp_path, value):
    with pytest.raises(ValueError, match="diffusion: truncate"):
        _score(tmp_path, diffusion=value)


def test_truncate_keeps_the_other_refusals(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="diffusion.*query_expansion"):
        _score(tmp_path, diffusion={"truncate": 100}, query_expansion={"k": 2, "alpha": 3.0})
    from mdir_amd import score as S

    def no_extraction(*args, **kwargs):
        raise AssertionError("extraction started")

    s = _score(tmp_path, diffusion={"truncate": 100})
    monkeypatch.setattr(S, "_world_size", lambda: 2)
    monkeypatch.setattr(S, "extract_vectors_device", no_extraction)
    import mdir_amd.sharded as SH
    monkeypatch.setattr(SH, "sharded_retrieval_map", no_extraction)
    with pytest.raises(ValueError, match="diffusion re-ranks in a single process"):
        s(None, "cpu", lambda *a: None)


def test_truncated_overlay_parses(tmp_path):
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_diffusion_truncated.yml")) as f:
        doc = yaml.safe_load(f)
    assert set(doc["validation"]) == {"roxford5k", "rparis6k", "247tokyo1k"}
    want = dict(DEFAULTS, truncate=1000)
    for ds in ("roxford5k", "rparis6k", "247tokyo1k"):
        crit = doc["validation"][ds]["criterion"]
        assert set(crit) == {"diffusion"}
        assert crit["diffusion"] == want
        assert _score(tmp_path, **crit).diffusion == want


# ------------------------------------------------------------------------------------------------------ Python API

class _Graph:
    """A graph object without the unnormalised weights (DiffusionGraph(weights=False))."""
    n = 10
    wvals = None


def test_rerank_truncate_checks_before_gpu_work():
    """Bad truncate values and a graph without weights are ValueErrors before any tensor is looked at."""
    from mdir_amd import rerank
    for kw in ({"truncate": 0}, {"truncate": -1}, {"truncate": 2.5}, {"truncate": True}, {"truncate": "1000"},
               {"truncate": 4097}, {"truncate": 9}, {"kq": 50, "truncate": 49}):
        with pytest.raises(ValueError, match="truncate"):
            rerank.diffusion(None, None, **kw)
    with pytest.raises(ValueError, match="weights=True"):
        rerank.diffusion(None, None, graph=_Graph(), truncate=100)


def test_ops_truncated_checks_before_gpu_work():
    from mdir_amd import ops
    g = (None, None, None)
    for gamma in (-1.0, float("nan"), "3"):
        with pytest.raises(ValueError, match="gamma"):
            ops.knn_graph_weights(None, None, gamma)
        with pytest.raises(ValueError, match="gamma"):
            ops.diffusion_truncated(g, None, None, None, 10, gamma, 0.5, 20, 1e-6)
    for alpha in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ops.diffusion_truncated(g, None, None, None, 10, 3.0, alpha, 20, 1e-6)
    for iters in (0, 2.0, True):
        with pytest.raises(ValueError, match="iters"):
            ops.diffusion_truncated(g, None, None, None, 10, 3.0, 0.5, iters, 1e-6)
    for kq in (0, 1.5, True):
        with pytest.raises(ValueError, match="kq"):
            ops.diffusion_truncated(g, None, None, None, kq, 3.0, 0.5, 20, 1e-6)
    with pytest.raises(ValueError, match="weights"):
        ops.diffusion_truncated(g, None, None, None, 10, 3.0, 0.5, 20, 1e-6)
    import torch
    with pytest.raises(RuntimeError, match="CUDA"):                 # host tensors: no CPU fallback
        ops.knn_graph_weights(torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2)), 3.0)
