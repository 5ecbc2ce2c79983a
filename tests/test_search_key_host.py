"""The ``search`` criterion key of mdir_amd/score.py, without a GPU: its validation -- every refusal, the defaults, the limits taken
from the index classes -- its interaction with the other keys, the single-process rule, and the overlays that use it."""
import os

import pytest

from conftest import ROOT


def _criterion(**keys):
    """CirDatasetAp on a dataset that is never read: the keys are validated before it is."""
    from mdir_amd.score import CirDatasetAp
    params = dict({"image_size": 64, "dataset": "no-such-dataset", "transforms": "pil2np | totensor | normalize",
                   "mean_std": [[0.5] * 3, [0.25] * 3]}, **keys)
    return CirDatasetAp(params)


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


IVF = {"index": "ivf", "depth": 100, "lists": 64, "nprobe": 8}
PQ = {"index": "ivfpq", "depth": 100, "lists": 64, "nprobe": 8}


def test_defaults_and_accepted_forms(tmp_path):
    from mdir_amd import ops
    s = _score(tmp_path)
    assert s.search is None and s.last_search is None and s.last_index is None       # without the key: as before
    assert _score(tmp_path, search={"index": "exact", "depth": 7}).search == {"index": "exact", "depth": 7, "recall": False}
    assert _score(tmp_path, search={"index": "i8", "depth": 7, "shortlist": 9}).search == \
        {"index": "i8", "depth": 7, "shortlist": 9, "exact": False, "recall": False}
    assert _score(tmp_path, search={"index": "f16", "depth": 7, "shortlist": 7, "exact": True, "recall": True}).search["exact"] is True
    assert _score(tmp_path, search=dict(IVF)).search == dict(IVF, storage="i8", shortlist=None, exact=False, recall=False)
    got = _score(tmp_path, search=dict(IVF, storage="f32", iters=5, seed=0)).search
    assert got["storage"] == "f32" and got["iters"] == 5 and got["seed"] == 0 and got["shortlist"] is None
    assert _score(tmp_path, search=dict(IVF, shortlist=200, exact=True)).search["exact"] is True
    assert _score(tmp_path, search=dict(PQ)).search == dict(PQ, m=64, refine=None, shortlist=None, rescore=None, recall=False)
    got = _score(tmp_path, search=dict(PQ, m=32, refine="i8", shortlist=400, rescore=100)).search
    assert (got["m"], got["refine"], got["shortlist"], got["rescore"]) == (32, "i8", 400, 100)
    assert _score(tmp_path, search={"index": "exact", "depth": ops.RESCORE_MAX_K}).search["depth"] == 4096
    # database_augmentation is allowed: it only changes the rows the index is built on
    s = _score(tmp_path, search=dict(IVF), database_augmentation={"k": 3, "alpha": 3.0}, neighbours="i8")
    assert s.search["lists"] == 64 and s.database_augmentation == {"k": 3, "alpha": 3.0}


def test_refused_together_with_other_keys():
    for keys, pair in (({"ranking": "full"}, "search together with ranking: full"),
                       ({"rescore": {"shortlist": 10}, "storage": "i8"}, "search together with rescore"),
                       ({"query_expansion": {"k": 3, "alpha": 3.0}}, "search together with query_expansion"),
                       ({"diffusion": {}}, "search together with diffusion"),
                       ({"k_reciprocal": {}}, "search together with k_reciprocal"),
                       ({"storage": "i8"}, "search together with storage: i8"),
                       ({"similarity": "split3"}, "search together with storage: f32 / similarity: split3")):
        with pytest.raises(ValueError, match=pair + ".*is not supported"):
            _criterion(search={"index": "exact", "depth": 5}, **keys)
    # allowed together: the keys pass, and only the dataset is then missing
    for keys in ({"search": dict(IVF)}, {"search": dict(PQ), "database_augmentation": {"k": 3, "alpha": 3.0}},
                 {"search": {"index": "exact", "depth": 5}, "ranking": "positions"}):
        with pytest.raises(Exception) as err:
            _criterion(**keys)
        assert "search" not in str(err.value), err.value


def test_refused_values():
    from mdir_amd import ops
    from mdir_amd.score import _search_params
    assert _search_params(None) is None
    for bad in (True, "ivf", [], {}, {"depth": 5}, {"index": "flat", "depth": 5}, {"index": None, "depth": 5}, {"index": ["ivf"], "depth": 5}):
        with pytest.raises(ValueError, match="search: a mapping"):
            _search_params(bad)
    # unknown sub-keys name the allowed ones of that index
    with pytest.raises(ValueError, match=r"search: index: exact: unknown keys \['shortlist'\] \(allowed: index, depth, recall\)"):
        _search_params({"index": "exact", "depth": 5, "shortlist": 9})
    with pytest.raises(ValueError, match=r"index: i8: unknown keys \['lists', 'nprobe'\]"):
        _search_params({"index": "i8", "depth": 5, "shortlist": 9, "lists": 4, "nprobe": 2})
    with pytest.raises(ValueError, match=r"index: ivf: unknown keys \['m'\].*allowed: index, depth, recall, lists, nprobe, storage, shortlist"):
        _search_params(dict(IVF, m=8))
    with pytest.raises(ValueError, match=r"index: ivfpq: unknown keys \['exact', 'storage'\]"):
        _search_params(dict(PQ, storage="i8", exact=True))
    # required
    for value, key in (({"index": "exact"}, "depth"), ({"index": "i8", "depth": 5}, "shortlist"), ({"index": "f16", "depth": 5}, "shortlist"),
                       ({"index": "ivf", "depth": 5, "nprobe": 2}, "lists"), ({"index": "ivf", "depth": 5, "lists": 2}, "nprobe"),
                       ({"index": "ivfpq", "depth": 5, "lists": 2}, "nprobe"), ({"index": "ivfpq", "lists": 2, "nprobe": 2}, "depth")):
        with pytest.raises(ValueError, match="search: index: %s: %s is required" % (value["index"], key)):
            _search_params(value)
    # depth: an integer in [1, the limit of every search]
    for bad in (0, -1, ops.RESCORE_MAX_K + 1, 5.0, "5", True, None):
        with pytest.raises(ValueError, match=r"search: depth must be an integer in \[1, %d\]" % ops.RESCORE_MAX_K):
            _search_params({"index": "exact", "depth": bad})
    for key in ("lists", "nprobe", "iters"):
        for bad in (0, 2.0, True, "4"):
            with pytest.raises(ValueError, match="search: %s must be an integer >= 1" % key):
                _search_params(dict(IVF, **{key: bad}))
    for bad in (-1, 0.5, False):
        with pytest.raises(ValueError, match="search: seed must be an integer >= 0"):
            _search_params(dict(PQ, seed=bad))
    with pytest.raises(ValueError, match="1 <= nprobe <= lists is required, got nprobe=65 lists=64"):
        _search_params(dict(IVF, nprobe=65))
    for bad in ("no", 1, None):
        with pytest.raises(ValueError, match="search: recall must be true or false"):
            _search_params({"index": "exact", "depth": 5, "recall": bad})
        with pytest.raises(ValueError, match="search: exact must be true or false"):
            _search_params({"index": "i8", "depth": 5, "shortlist": 9, "exact": bad})
    # shortlist: at least the depth, at most what one query rescoring holds
    for kind in ({"index": "i8"}, {"index": "f16"}, dict(IVF), dict(PQ)):
        for bad in (99, ops.RESCORE_MAX_K + 1, 200.0, True):
            with pytest.raises(ValueError, match=r"search: shortlist must be an integer in \[100, %d\]" % ops.RESCORE_MAX_K):
                _search_params(dict(kind, depth=100, shortlist=bad))
    with pytest.raises(ValueError, match="search: storage must be 'f32' or 'i8'"):
        _search_params(dict(IVF, storage="f16"))
    with pytest.raises(ValueError, match="shortlist and exact need storage: i8"):
        _search_params(dict(IVF, storage="f32", shortlist=200))
    with pytest.raises(ValueError, match="shortlist and exact need storage: i8"):
        _search_params(dict(IVF, storage="f32", exact=True))
    with pytest.raises(ValueError, match="exact: true needs a shortlist"):
        _search_params(dict(IVF, exact=True))
    for bad in (0, ops.PQ_MAX_M + 1, 8.0, True):
        with pytest.raises(ValueError, match=r"search: m must be an integer in \[1, %d\]" % ops.PQ_MAX_M):
            _search_params(dict(PQ, m=bad))
    for bad in ("f16", True, 8):
        with pytest.raises(ValueError, match="search: refine must be 'i8' or absent"):
            _search_params(dict(PQ, refine=bad))
    with pytest.raises(ValueError, match="rescore needs refine: i8 and a shortlist"):
        _search_params(dict(PQ, shortlist=400, rescore=100))
    with pytest.raises(ValueError, match="rescore needs refine: i8 and a shortlist"):
        _search_params(dict(PQ, refine="i8", rescore=100))
    for bad in (99, 401, True):
        with pytest.raises(ValueError, match=r"search: rescore must be an integer in \[100, 400\]"):
            _search_params(dict(PQ, refine="i8", shortlist=400, rescore=bad))


def test_search_is_single_process(monkeypatch):
    from mdir_amd import score
    obj = score.CirDatasetAp.__new__(score.CirDatasetAp)
    obj.dataset, obj.query_expansion, obj.database_augmentation, obj.diffusion, obj.rescore, obj.k_reciprocal = "x", None, None, None, None, None
    obj.search = score._search_params(dict(IVF))
    monkeypatch.setattr(score, "_rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="search builds and searches its index in a single process.*2 ranks"):
        obj(None, "cpu", None)


@pytest.mark.parametrize("name,index", (("eval_search_ivf.yml", "ivf"), ("eval_search_ivfpq.yml", "ivfpq"), ("eval_search_i8.yml", "i8")))
def test_overlays_parse(tmp_path, name, index):
    import yaml
    with open(os.path.join(ROOT, "scenarios", name)) as f:
        doc = yaml.safe_load(f)
    assert set(doc) == {"validation"} and doc["validation"]
    for ds, entry in doc["validation"].items():
        crit = entry["criterion"]
        assert set(crit) == {"search"} and crit["search"]["index"] == index
        s = _score(tmp_path, **crit)
        assert s.search["depth"] == crit["search"]["depth"] and s.search["recall"] in (True, False)


def test_call_logs_the_reference_rows_and_the_two_laps(tmp_path, monkeypatch):
    """``__call__`` with the key: extraction, then ``searched_map`` (replaced here: it needs the device) with the stop watch's lap, then
    the reference's logger rows -- ``dataset`` with the laps ``build_index`` and ``search`` in front of ``compute_score``, ``score_avg``,
    one ``score`` per query."""
    import numpy as np
    import torch
    from mdir_amd import score
    s = _score(tmp_path, search=dict(IVF))
    seen = {}

    def fake_extract(network, images, image_size, transforms, device=None, bbxs=None):
        return torch.zeros((len(images), 8))

    def fake_searched_map(self, vecs, qvecs, lap=None):
        seen["shapes"] = (tuple(vecs.shape), tuple(qvecs.shape))
        lap("build_index")
        lap("search")
        return {"map": 0.5}, {"ap": np.array([0.5])}

    monkeypatch.setattr(score, "extract_vectors_device", fake_extract)
    monkeypatch.setattr(score.CirDatasetAp, "searched_map", fake_searched_map)
    rows = []
    s(None, "cpu", lambda *row: rows.append(row))
    assert seen["shapes"] == ((3, 8), (1, 8))
    assert [r[2] for r in rows] == ["dataset", "score_avg", "score"]
    assert list(rows[0][3]) == ["extract_descriptors", "build_index", "search", "compute_score", "total_s"]
    assert rows[1][3] == {"map": 0.5} and rows[2][3] == {"ap": 0.5} and rows[2][0] == 0
    # without the key the laps are the two of the reference
    monkeypatch.setattr(score, "compute_map_and_print_from_scores", lambda dataset, scores, gnd: ({"map": 0.5}, {"ap": np.array([0.5])}))
    monkeypatch.setattr(score.ops, "scores_rowmajor", lambda vecs, qvecs, layout: None)
    rows = []
    _score(tmp_path)(None, "cpu", lambda *row: rows.append(row))
    assert list(rows[0][3]) == ["extract_descriptors", "compute_score", "total_s"]
