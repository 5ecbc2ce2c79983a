"""The `graph` route of the ``search`` criterion key (mdir_amd/score.py, ``CirDatasetAp.searched_map``) on the device, driven as
test_gpu_search_key.py drives the other routes, on a toy database small enough for the beam to hold every row: N = 480 unit rows in 12
clusters, D = 64, 10 queries, an old-protocol and an rOxford-shaped gnd.  With ``beam >= N`` and the k-means medoids as entries every
row is reachable and the walk ends only when all of them are expanded, so the lists are the exact top-50: the dicts are those of
``index: exact`` at that depth bit for bit, and the recall is exactly 1."""
import numpy as np
import pytest
import torch

from test_gpu_search_key import _same, _scorer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, Q, CLUSTERS, DEPTH = 480, 64, 10, 12, 50
F32 = np.float32
PROTOCOLS = ("oxford5k", "roxford5k")
ROUTE = {"index": "graph", "depth": DEPTH, "degree": 16, "k0": 40, "beam": 512, "seeds": 12, "entries": "medoids", "lists": CLUSTERS,
         "iters": 5, "recall": True}


class Data:
    pass


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    centres = unit(rng.standard_normal((CLUSTERS, D)))
    labels = np.repeat(np.arange(CLUSTERS), N // CLUSTERS)
    rows = unit(centres[labels] + 0.12 * rng.standard_normal((N, D)))
    qlabels = rng.permutation(CLUSTERS)[:Q]
    queries = unit(centres[qlabels] + 0.12 * rng.standard_normal((Q, D)))
    d = Data()
    d.old, d.rox = [], []
    for q in range(Q):
        own = rng.permutation(np.flatnonzero(labels == qlabels[q]))
        far = rng.permutation(np.flatnonzero(labels != qlabels[q]))
        d.old.append({"ok": np.concatenate([own[:8], far[:2]]), "junk": own[8:11]})
        d.rox.append({"easy": own[:5], "hard": np.concatenate([own[5:13], far[:2]]), "junk": own[13:18], "bbx": None})
    d.vecs, d.qvecs = torch.from_numpy(rows).to(DEV), torch.from_numpy(queries).to(DEV)
    return d


def _run(search, dataset, data):
    obj = _scorer(search, dataset, data)
    laps = []
    out = obj.searched_map(data.vecs, data.qvecs, lap=laps.append)
    assert laps == ["build_index", "search"]
    return out, obj


@pytest.mark.parametrize("neighbours", ("exact", "i8"))
@pytest.mark.parametrize("dataset", PROTOCOLS)
def test_graph_route_with_a_beam_of_every_row_is_exact(dataset, neighbours, data, capsys):
    from mdir_amd import ops
    want, _ = _run({"index": "exact", "depth": DEPTH}, dataset, data)
    capsys.readouterr()
    out, obj = _run(dict(ROUTE, neighbours=neighbours), dataset, data)
    printed = capsys.readouterr().out
    _same(out, want, "graph %s" % dataset)
    exact_ids = ops.topk(ops.scores_rowmajor(data.vecs, data.qvecs, "ND"), DEPTH)[0]
    assert torch.equal(obj.last_search.ids, exact_ids)
    assert obj.last_recall.shape == (Q,) and (obj.last_recall == 1.0).all()
    assert ">> %s: recall@%d against the exact top-%d: min 1.0000 / mean 1.0000" % (dataset, DEPTH, DEPTH) in printed
    assert obj.last_index.entry_index is None                                                 # closed on the way out
    assert tuple(obj.last_index.graph.shape) == (N, 16) and 1 <= obj.last_index.entries.shape[0] <= CLUSTERS
    steps, scored = obj.last_search.steps.cpu().numpy(), obj.last_search.scored.cpu().numpy()
    assert (steps == N).all() and (scored == N).all()                                         # every row reached, scored once, expanded once
