"""Diffusion re-ranking without a GPU: the four C entry points are exported and declared, refuse every bad argument before
they launch anything and size their workspaces right; the evaluation surface validates the `diffusion` key and refuses a
sharded run; the Python layers check their arguments before any device work."""
import ctypes
import os

import pytest

from conftest import ROOT

P = ctypes.c_void_p
A, B, C, D, E, F, G, H = (P(0x100000 * i) for i in range(1, 9))
WS = P(0x10000000)
NEW = ("mdx_knn_graph_workspace", "mdx_knn_graph", "mdx_diffusion_workspace", "mdx_diffusion")


def _handle():
    from mdir_amd import _lib
    _lib.build()
    return _lib.lib()


def test_diffusion_symbols_are_exported_and_declared():
    from mdir_amd import _lib
    h = _handle()
    header = open(os.path.join(ROOT, "include", "mdx.h")).read()
    for name in NEW:
        assert hasattr(h, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in header, name
    assert h.mdx_abi_version() == 3


def test_workspace_sizes():
    h = _handle()
    assert h.mdx_knn_graph_workspace(1004993) == (1004993 * 4 + 255) // 256 * 256
    assert h.mdx_knn_graph_workspace(0) == 0
    for n, nq in ((1004993, 70), (4993, 1), (4993, 256), (1, 3)):
        nqp = (nq + 3) // 4 * 4
        block = (n * nqp * 4 + 255) // 256 * 256
        parts = ((256 * -(-n // 32) * 4) + 255) // 256 * 256
        assert h.mdx_diffusion_workspace(n, nq) == 4 * block + parts + 6 * 256 * 4, (n, nq)
    assert h.mdx_diffusion_workspace(1004993, 70) >= 4 * 1004993 * 72 * 4
    assert h.mdx_diffusion_workspace(100, 257) == 0 and h.mdx_diffusion_workspace(0, 5) == 0
    assert h.mdx_diffusion_workspace(100, 0) == 0


def _graph(h, ids=A, sims=B, n=100, k=5, gamma=3.0, cols=C, vals=D, counts=E, ws=WS, ws_bytes=1 << 20):
    return h.mdx_knn_graph(ids, sims, n, k, gamma, cols, vals, counts, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, status, words", [
    ({"ids": None}, -1, b"NULL"), ({"sims": None}, -1, b"NULL"), ({"cols": None}, -1, b"NULL"),
    ({"vals": None}, -1, b"NULL"), ({"counts": None}, -1, b"NULL"), ({"ws": None}, -1, b"NULL"),
    ({"n": 0}, -1, b"n=0"), ({"k": 0}, -1, b"k=0"), ({"n": -4}, -1, b"n=-4"),
    ({"n": 1 << 31}, -1, b"2^31"),
    ({"gamma": -1.0}, -1, b"gamma"), ({"gamma": float("nan")}, -1, b"gamma"), ({"gamma": float("inf")}, -1, b"gamma"),
    ({"ws_bytes": 399}, -4, b"workspace"),
])
def test_knn_graph_argument_checks(bad, status, words):
    h = _handle()
    assert _graph(h, **bad) == status
    msg = h.mdx_last_error()
    assert msg.startswith(b"mdx_knn_graph") and words in msg, msg


def _solve(h, cols=A, vals=B, counts=C, n=100, k=5, scores=D, ld_scores=100, seed_ids=E, seed_sims=F, nq=7, kq=3,
           gamma=3.0, alpha=0.99, iters=20, tol=1e-6, out=G, ld_out=100, residual=None, steps=None, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 30
    return h.mdx_diffusion(cols, vals, counts, n, k, scores, ld_scores, seed_ids, seed_sims, nq, kq, gamma, alpha, iters, tol,
                           out, ld_out, residual, steps, ws, ws_bytes, None)


@pytest.mark.parametrize("bad, status, words", [
    ({"cols": None}, -1, b"NULL"), ({"vals": None}, -1, b"NULL"), ({"counts": None}, -1, b"NULL"),
    ({"scores": None}, -1, b"NULL"), ({"seed_ids": None}, -1, b"NULL"), ({"seed_sims": None}, -1, b"NULL"),
    ({"out": None}, -1, b"NULL"), ({"ws": None}, -1, b"NULL"),
    ({"n": 0, "ld_scores": 0, "ld_out": 0}, -1, b"n=0"), ({"k": 0}, -1, b"k=0"), ({"nq": 0}, -1, b"nq=0"),
    ({"kq": 0}, -1, b"kq=0"), ({"nq": 257}, -1, b"nq=257"),
    ({"n": 1 << 31, "ld_scores": 1 << 31, "ld_out": 1 << 31}, -1, b"2^31"),
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
def test_diffusion_argument_checks(bad, status, words):
    h = _handle()
    assert _solve(h, **bad) == status
    msg = h.mdx_last_error()
    assert msg.startswith(b"mdx_diffusion") and words in msg, msg


def test_diffusion_status_maps_to_python_errors():
    from mdir_amd import _lib as L
    for status in (-1, -4):
        with pytest.raises(ValueError):
            L.check(status, "mdx_diffusion")


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


def test_cirdatasetap_without_the_key_has_no_diffusion(tmp_path):
    assert _score(tmp_path).diffusion is None


@pytest.mark.parametrize("mask", range(64))
def test_cirdatasetap_accepts_every_subset_of_diffusion_keys(tmp_path, mask):
    keys = sorted(DEFAULTS)
    given = {key: GIVEN[key] for i, key in enumerate(keys) if mask >> i & 1}
    s = _score(tmp_path, diffusion=given)
    want = dict(DEFAULTS, **given)
    assert s.diffusion == want
    for key in ("gamma", "alpha", "tol"):
        assert isinstance(s.diffusion[key], float)


def test_cirdatasetap_diffusion_with_dba(tmp_path):
    s = _score(tmp_path, diffusion={"k": 5}, database_augmentation={"k": 3, "alpha": 3.0})
    assert s.diffusion["k"] == 5 and s.database_augmentation == {"k": 3, "alpha": 3.0}


@pytest.mark.parametrize("value", [
    {"k": 0}, {"k": -1}, {"k": 2.5}, {"k": True}, {"k": "50"}, {"kq": 0}, {"kq": 1.0}, {"iters": 0}, {"iters": False},
    {"gamma": -1.0}, {"gamma": float("nan")}, {"gamma": float("inf")}, {"gamma": "3"},
    {"alpha": 1.0}, {"alpha": 1.2}, {"alpha": -0.1}, {"alpha": float("nan")}, {"alpha": True},
    {"tol": -1e-6}, {"tol": float("inf")}, {"tol": float("nan")},
    {"beta": 1}, {"k": 50, "steps": 20}, [50, 10], 3, "defaults",
])
def test_cirdatasetap_rejects_bad_diffusion_values(tmp_path, value):
    with pytest.raises(ValueError, match="diffusion"):
        _score(tmp_path, diffusion=value)


def test_cirdatasetap_refuses_diffusion_with_query_expansion(tmp_path):
    with pytest.raises(ValueError, match="diffusion.*query_expansion"):
        _score(tmp_path, diffusion={}, query_expansion={"k": 2, "alpha": 3.0})


def test_diffusion_refuses_a_sharded_run_before_extraction(tmp_path, monkeypatch):
    from mdir_amd import score as S

    def no_extraction(*args, **kwargs):
        raise AssertionError("extraction started")

    s = _score(tmp_path, diffusion={"k": 5})
    monkeypatch.setattr(S, "_world_size", lambda: 2)
    monkeypatch.setattr(S, "extract_vectors_device", no_extraction)
    import mdir_amd.sharded as SH
    monkeypatch.setattr(SH, "sharded_retrieval_map", no_extraction)
    with pytest.raises(ValueError, match="diffusion re-ranks in a single process"):
        s(None, "cpu", lambda *a: None)


def test_diffusion_overlay_parses(tmp_path):
    import yaml
    with open(os.path.join(ROOT, "scenarios", "eval_diffusion.yml")) as f:
        doc = yaml.safe_load(f)
    assert set(doc["validation"]) == {"roxford5k", "rparis6k", "247tokyo1k"}
    for ds in ("roxford5k", "rparis6k", "247tokyo1k"):
        crit = doc["validation"][ds]["criterion"]
        assert set(crit) == {"diffusion"}
        assert crit["diffusion"] == DEFAULTS
        assert _score(tmp_path, **crit).diffusion == DEFAULTS


# ------------------------------------------------------------------------------------------------------ Python API

def test_ops_checks_before_gpu_work():
    """Bad numbers are ValueErrors before any tensor is looked at (the arguments here are not even tensors)."""
    from mdir_amd import ops
    for gamma in (-1.0, float("nan"), float("inf"), "3"):
        with pytest.raises(ValueError, match="gamma"):
            ops.knn_graph(None, None, gamma)
        with pytest.raises(ValueError, match="gamma"):
            ops.diffusion((None, None, None), None, None, None, gamma, 0.5, 20, 1e-6)
    for alpha in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ops.diffusion((None, None, None), None, None, None, 3.0, alpha, 20, 1e-6)
    for iters in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="iters"):
            ops.diffusion((None, None, None), None, None, None, 3.0, 0.5, iters, 1e-6)
    for tol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            ops.diffusion((None, None, None), None, None, None, 3.0, 0.5, 20, tol)
    with pytest.raises(RuntimeError, match="CUDA"):                 # host tensors: no CPU fallback
        import torch
        ops.knn_graph(torch.zeros((3, 2), dtype=torch.int64), torch.zeros((3, 2)), 3.0)


def test_rerank_checks_before_gpu_work():
    from mdir_amd import rerank
    for kw in ({"k": 0}, {"k": 2.5}, {"gamma": -1.0}, {"gamma": float("nan")}, {"chunk": 0}, {"layout": "XY"}):
        with pytest.raises(ValueError):
            rerank.DiffusionGraph(None, **kw) if "layout" not in kw else rerank.DiffusionGraph(_Fake2d(), **kw)
    for kw in ({"kq": 0}, {"alpha": 1.0}, {"alpha": -0.5}, {"iters": 0}, {"tol": -1.0}, {"tol": float("nan")}):
        with pytest.raises(ValueError):
            rerank.diffusion(None, None, **kw)
    assert rerank.DIFFUSION_DEFAULTS == DEFAULTS


class _Fake2d:
    def dim(self):
        return 2
