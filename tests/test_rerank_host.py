"""Re-ranking (alpha-QE, DBA) without a GPU: the C entry point is exported and refuses every bad argument before it
launches anything; the evaluation surface validates its criterion keys and refuses a sharded run."""
import ctypes

import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)

P = ctypes.c_void_p
ROWS, IDS, SIMS, SELF, OUT = P(0x100000), P(0x200000), P(0x300000), P(0x400000), P(0x500000)


def _handle():
    from mdir_amd import _lib
    _lib.build()
    return _lib.lib()


def test_knn_aggregate_is_exported():
    from mdir_amd import _lib
    h = _handle()
    assert hasattr(h, "mdx_knn_aggregate")
    assert "mdx_knn_aggregate" in _lib.EXPORTS
    assert h.mdx_abi_version() == 3


def _call(h, rows=ROWS, n=100, d=64, ld=64, ids=IDS, sims=SIMS, nq=5, k=3, self_rows=None, ld_self=64, alpha=3.0,
          eps=1e-6, out=OUT, ld_out=64):
    return h.mdx_knn_aggregate(rows, n, d, ld, ids, sims, nq, k, self_rows, ld_self, alpha, eps, out, ld_out, None)


@pytest.mark.parametrize("bad, words", [
    ({"rows": None}, b"NULL"), ({"ids": None}, b"NULL"), ({"sims": None}, b"NULL"), ({"out": None}, b"NULL"),
    ({"n": 0}, b"n=0"), ({"d": 0}, b"d=0"), ({"nq": 0}, b"nq=0"), ({"k": 0}, b"k=0"), ({"k": -2}, b"k=-2"),
    ({"ld": 63}, b"ld=63"), ({"ld_out": 10}, b"ld_out=10"), ({"self_rows": SELF, "ld_self": 32}, b"ld_self=32"),
    ({"alpha": -1.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"), ({"alpha": float("inf")}, b"alpha"),
    ({"eps": -1e-6}, b"eps"), ({"eps": float("nan")}, b"eps"), ({"eps": float("inf")}, b"eps"),
    ({"out": P(0x100000 + 64 * 4 * 99)}, b"overlaps rows"),                         # out starts on rows' last row
    ({"out": P(0x100000 + 4 - 4 * (4 * 64 + 64))}, b"overlaps rows"),             # out's last element is rows[0, 0]
    ({"self_rows": SELF, "out": P(0x400000 + 4 * 64 * 2)}, b"overlaps self_rows"),
])
def test_knn_aggregate_argument_checks(bad, words):
    from mdir_amd import _lib as L
    h = _handle()
    assert _call(h, **bad) == -1
    msg = h.mdx_last_error()
    assert msg.startswith(b"mdx_knn_aggregate") and words in msg, msg
    with pytest.raises(ValueError):
        L.check(-1, "mdx_knn_aggregate")


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


def test_cirdatasetap_accepts_the_rerank_keys(tmp_path):
    plain = _score(tmp_path)
    assert plain.query_expansion is None and plain.database_augmentation is None
    s = _score(tmp_path, query_expansion={"k": 2, "alpha": 3}, database_augmentation={"k": 10, "alpha": 0.0})
    assert s.query_expansion == {"k": 2, "alpha": 3.0}
    assert s.database_augmentation == {"k": 10, "alpha": 0.0}


@pytest.mark.parametrize("key", ["query_expansion", "database_augmentation"])
@pytest.mark.parametrize("value", [
    {"k": 0, "alpha": 3.0}, {"k": -1, "alpha": 3.0}, {"k": 2.5, "alpha": 3.0}, {"k": True, "alpha": 3.0},
    {"k": "2", "alpha": 3.0}, {"k": 2, "alpha": -0.5}, {"k": 2, "alpha": float("nan")}, {"k": 2, "alpha": float("inf")},
    {"k": 2, "alpha": "3"}, {"k": 2}, {"alpha": 3.0}, {"k": 2, "alpha": 3.0, "beta": 1}, [2, 3.0], 2,
])
def test_cirdatasetap_rejects_bad_rerank_keys(tmp_path, key, value):
    with pytest.raises(ValueError, match=key):
        _score(tmp_path, **{key: value})


@pytest.mark.parametrize("criterion", [{"query_expansion": {"k": 2, "alpha": 3.0}},
                                       {"database_augmentation": {"k": 10, "alpha": 3.0}}])
def test_rerank_refuses_a_sharded_run_before_extraction(tmp_path, monkeypatch, criterion):
    from mdir_amd import score as S

    def no_extraction(*args, **kwargs):
        raise AssertionError("extraction started")

    s = _score(tmp_path, **criterion)
    monkeypatch.setattr(S, "_world_size", lambda: 2)
    monkeypatch.setattr(S, "extract_vectors_device", no_extraction)
    import mdir_amd.sharded as SH
    monkeypatch.setattr(SH, "sharded_retrieval_map", no_extraction)
    with pytest.raises(ValueError, match="single process"):
        s(None, "cpu", lambda *a: None)


def test_rerank_api_checks_before_gpu_work():
    """k < 1 and alpha < 0 are ValueErrors before any device is touched (the arguments here are not even tensors)."""
    from mdir_amd import rerank
    for k, alpha in ((0, 3.0), (-3, 3.0), (2, -1.0), (2, float("nan")), (1.5, 3.0)):
        with pytest.raises(ValueError):
            rerank.database_augmentation(None, k, alpha)
        with pytest.raises(ValueError):
            rerank.query_expansion(None, None, k, alpha)
    with pytest.raises(ValueError):
        rerank.database_augmentation(None, 2, 3.0, chunk=0)


def test_dba_chunk_respects_the_memory_cap():
    from mdir_amd import ops, rerank
    _handle()
    for n, k in ((1004993, 10), (100000, 10), (20000, 10), (7, 10)):
        c = rerank.dba_chunk(n, min(k, n))
        assert 1 <= c <= n
        need = c * n * 4 + ops.rank_workspace_bytes(n, c)
        assert need <= rerank.DBA_MEMORY_CAP or c == 1
        if c < n:     # and it is not needlessly small
            assert (c + 1) * n * 4 + ops.rank_workspace_bytes(n, c + 1) > rerank.DBA_MEMORY_CAP * 0.99


def test_overlays_parse(tmp_path):
    import os
    import yaml
    for name, keys in (("eval_aqe.yml", {"query_expansion"}), ("eval_dba_aqe.yml", {"query_expansion", "database_augmentation"})):
        with open(os.path.join(ROOT, "scenarios", name)) as f:
            doc = yaml.safe_load(f)
        for ds in ("roxford5k", "rparis6k", "247tokyo1k"):
            crit = doc["validation"][ds]["criterion"]
            assert set(crit) == keys
            assert crit["query_expansion"] == {"k": 2, "alpha": 3.0}
            if "database_augmentation" in crit:
                assert crit["database_augmentation"] == {"k": 10, "alpha": 3.0}
