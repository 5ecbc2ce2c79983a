"""The ``search`` criterion key (mdir_amd/score.py, ``CirDatasetAp.searched_map``) on the device, driven without images or a network on
synthetic clustered descriptors: N = 1500 unit rows in 24 clusters, D = 64, 16 queries, an old-protocol and an rOxford-shaped gnd.

The equality chain: ``index: exact, depth: N`` is ``compute_map_and_print_from_scores``; ``index: exact, depth: 50`` is
``compute_map_topk`` of ``ops.topk(scores, 50)``; every route whose contract makes its list the exact top-50 -- the fp32 inverted file
and the int8 one with ``exact: true`` at ``nprobe == lists``, the int8 shard with ``exact: true``, IVF-PQ with every row in the
shortlist -- returns the same dicts bit for bit and a recall of exactly 1.  The approximate routes (two probes; ADC order) are
deterministic, give APs in [0, 1] and report the label recall and the overlap recall a numpy recomputation from their ids gives.  No
recall threshold: what an approximate route finds depends on the data.
"""
import numpy as np
import pytest
import torch

import overlap_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, Q, CLUSTERS, DEPTH = 1500, 64, 16, 24, 50
F32 = np.float32


class Data:
    pass


def _make(seed):
    rng = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    centres = unit(rng.standard_normal((CLUSTERS, D)))
    labels = rng.integers(0, CLUSTERS, N)
    rows = unit(centres[labels] + 0.12 * rng.standard_normal((N, D)))
    qlabels = rng.permutation(CLUSTERS)[:Q]
    queries = unit(centres[qlabels] + 0.12 * rng.standard_normal((Q, D)))
    old, rox = [], []
    for q in range(Q):
        own = rng.permutation(np.flatnonzero(labels == qlabels[q]))
        far = rng.permutation(np.flatnonzero(labels != qlabels[q]))
        assert len(own) >= 20
        old.append({"ok": np.concatenate([own[:8], far[:2]]), "junk": own[8:11]})
        rox.append({"easy": own[:5], "hard": np.concatenate([own[5:13], far[:2]]), "junk": own[13:18], "bbx": None})
    return rows, queries, old, rox


@pytest.fixture(scope="module")
def data():
    d = Data()
    rows, queries, d.old, d.rox = _make(seed=0)
    # on the CPU: every query has a positive among its exact top 50, and some query has one outside it (else: another seed)
    top = np.argsort(-(queries @ rows.T), axis=1, kind="stable")[:, :DEPTH]
    for gnd, keys in ((d.old, ("ok",)), (d.rox, ("easy", "hard"))):
        inside = [len(set(top[q].tolist()) & set(np.concatenate([g[k] for k in keys]).tolist())) for q, g in enumerate(gnd)]
        total = [len(np.concatenate([g[k] for k in keys])) for g in gnd]
        assert min(inside) >= 1 and any(i < t for i, t in zip(inside, total)), (inside, total)
    d.vecs, d.qvecs = torch.from_numpy(rows).to(DEV), torch.from_numpy(queries).to(DEV)
    from mdir_amd import ops
    d.scores = ops.scores_rowmajor(d.vecs, d.qvecs, "ND")
    d.exact_ids = ops.topk(d.scores, DEPTH)[0]
    d.runs = {}
    return d


PROTOCOLS = ("oxford5k", "roxford5k")


def _scorer(search, dataset, data):
    from mdir_amd import score
    obj = score.CirDatasetAp.__new__(score.CirDatasetAp)
    obj.dataset, obj.gnd = dataset, data.old if dataset == "oxford5k" else data.rox
    obj.database_augmentation, obj.neighbours = None, "exact"
    obj.search = score._search_params(dict(search))
    return obj


def _run(search, dataset, data):
    obj = _scorer(search, dataset, data)
    laps = []
    out = obj.searched_map(data.vecs, data.qvecs, lap=laps.append)
    assert laps == ["build_index", "search"]
    if obj.last_index is not None:                               # closed on the way out
        assert obj.last_index._h is None if hasattr(obj.last_index, "_h") else obj.last_index.coarse is None
    return out, obj


def _same(a, b, what=""):
    """Two ``(averages, per_query)`` results, bit for bit (NaN where a NaN is due)."""
    assert len(a) == len(b) == 2 and set(a[0]) == set(b[0]) and set(a[1]) == set(b[1]), what
    for part in (0, 1):
        for key in a[part]:
            np.testing.assert_array_equal(np.asarray(a[part][key]), np.asarray(b[part][key]), err_msg="%s %s" % (what, key))


def _exact50(dataset, data):
    if dataset not in data.runs:
        data.runs[dataset] = _run({"index": "exact", "depth": DEPTH}, dataset, data)[0]
    return data.runs[dataset]


@pytest.mark.parametrize("dataset", PROTOCOLS)
def test_exact_at_full_depth_is_the_scores_evaluation(dataset, data, capsys):
    from mdir_amd import evaluate as E
    out, obj = _run({"index": "exact", "depth": N}, dataset, data)
    mine = capsys.readouterr().out.splitlines()
    want = E.compute_map_and_print_from_scores(dataset, data.scores, obj.gnd)
    theirs = capsys.readouterr().out.splitlines()
    _same(out, want, dataset)
    assert mine[:len(theirs)] == theirs and len(mine) == len(theirs) + 1 and "top-%d label recall" % N in mine[-1]
    assert tuple(obj.last_search.ids.shape) == (Q, N) and obj.last_recall is None
    # a depth beyond N is clamped to N
    deeper, _ = _run({"index": "exact", "depth": 4096}, dataset, data)
    _same(deeper, want, dataset)


@pytest.mark.parametrize("dataset", PROTOCOLS)
def test_exact_at_depth_50_is_the_evaluation_of_topk(dataset, data):
    from mdir_amd import evaluate as E
    out = _exact50(dataset, data)
    gnd = data.old if dataset == "oxford5k" else data.rox
    want = E.compute_map_and_print_topk(dataset, data.exact_ids, gnd, N)
    _same(out, want, dataset)
    host = E.compute_map_and_print_topk(dataset, data.exact_ids.cpu().numpy(), gnd, N)         # np.isin row by row: the same positions
    _same(host, want, dataset)
    for key in ("found", "rows", "depth"):
        for a, b in ((want.stats, host.stats),) if dataset == "oxford5k" else [(want.stats[lv], host.stats[lv]) for lv in want.stats]:
            np.testing.assert_array_equal(a[key], b[key])
    full = E.compute_map_and_print_from_scores(dataset, data.scores, gnd)
    for key in out[1]:                                                                        # a prefix of the full AP, and a proper one somewhere
        live = ~np.isnan(full[1][key])
        assert (out[1][key][live] <= full[1][key][live]).all() and (out[1][key][live] >= 0).all()
    assert any((out[1][key][~np.isnan(full[1][key])] < full[1][key][~np.isnan(full[1][key])]).any() for key in out[1])


EXACT_ROUTES = {
    "ivf_f32": {"index": "ivf", "storage": "f32", "lists": CLUSTERS, "nprobe": CLUSTERS, "iters": 5},
    "ivf_i8": {"index": "ivf", "storage": "i8", "shortlist": 200, "exact": True, "lists": CLUSTERS, "nprobe": CLUSTERS, "iters": 5},
    "i8": {"index": "i8", "shortlist": 200, "exact": True},
    "ivfpq": {"index": "ivfpq", "lists": CLUSTERS, "nprobe": CLUSTERS, "shortlist": N, "iters": 5},
}


@pytest.mark.parametrize("dataset", PROTOCOLS)
@pytest.mark.parametrize("route", sorted(EXACT_ROUTES))
def test_routes_that_are_exact_by_contract(route, dataset, data, capsys):
    out, obj = _run(dict(EXACT_ROUTES[route], depth=DEPTH, recall=True), dataset, data)
    printed = capsys.readouterr().out
    _same(out, _exact50(dataset, data), "%s %s" % (route, dataset))
    assert torch.equal(obj.last_search.ids, data.exact_ids)
    assert obj.last_recall.shape == (Q,) and (obj.last_recall == 1.0).all()
    assert ">> %s: recall@%d against the exact top-%d: min 1.0000 / mean 1.0000" % (dataset, DEPTH, DEPTH) in printed
    if route == "ivfpq":
        assert int(obj.last_search.scanned.max()) <= N and obj.last_index.rows is not None
    if route in ("ivf_i8", "i8"):
        assert obj.last_search.certified is not None and obj.last_search.fallback.dtype == torch.int64


APPROXIMATE = {
    "ivf_2_probes": {"index": "ivf", "lists": CLUSTERS, "nprobe": 2, "iters": 5},
    "ivfpq_adc": {"index": "ivfpq", "lists": CLUSTERS, "nprobe": 4, "iters": 5},
}


@pytest.mark.parametrize("dataset", PROTOCOLS)
@pytest.mark.parametrize("route", sorted(APPROXIMATE))
def test_approximate_routes(route, dataset, data):
    search = dict(APPROXIMATE[route], depth=DEPTH, recall=True)
    out, obj = _run(search, dataset, data)
    again, obj2 = _run(search, dataset, data)
    _same(out, again, route)
    assert torch.equal(obj.last_search.ids, obj2.last_search.ids)
    for key, aps in out[1].items():
        aps = aps[~np.isnan(aps)]
        assert len(aps) and (aps >= 0).all() and (aps <= 1).all(), key
    if route == "ivfpq_adc":
        assert obj.last_index.rows is None                       # no shortlist: the rows are not kept
    ids = obj.last_search.ids.cpu().numpy()
    assert ids.shape == (Q, DEPTH)
    # the overlap recall, from the ids
    want = R.recall_at(ids, data.exact_ids.cpu().numpy(), [DEPTH])[:, 0]
    np.testing.assert_array_equal(obj.last_recall, want)
    print("%s %s: recall@%d min %.4f mean %.4f" % (route, dataset, DEPTH, want.min(), want.mean()))
    # the label recall, from the ids
    levels = {None: (("ok",), ("junk",))} if dataset == "oxford5k" else \
        {"easy": (("easy",), ("junk", "hard")), "medium": (("easy", "hard"), ("junk",)), "hard": (("hard",), ("junk", "easy"))}
    for level, (ok_keys, junk_keys) in levels.items():
        stats = obj.last_stats if level is None else obj.last_stats[level]
        for q, g in enumerate(obj.gnd):
            head = [int(x) for x in ids[q] if x >= 0]
            ok = set(np.concatenate([g[k] for k in ok_keys]).tolist())
            junk = set(np.concatenate([g[k] for k in junk_keys]).tolist())
            assert stats["found"][q] == len(ok & set(head)) and stats["rows"][q] == len(ok)
            assert stats["depth"][q] == len(head) - len(junk & set(head))
