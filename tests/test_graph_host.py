"""The graph index (include/mdx_graph.h; mdir_amd/graph.py; the `graph` route of the `search` criterion key), without a GPU:

  a. the numpy restatement (tests/graph_restatement.py) on cases worked out by hand, and its properties: the visited set changes
     `scored` only, a complete walk is the exact top-k, the optimised graph does not find less than the plain kNN graph;
  b. census: the prototypes of include/mdx_graph.h are exported, bound, apart from every other export tuple and covered by
     tests/test_gpu_graph_memcontract.py; the constants of the header, the restatement and ops agree;
  c. the library refuses every malformed call before any device work, and the Python wrappers and the key need no GPU for their checks.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import graph_restatement as R
from conftest import ROOT
from oracle import chain

NEW = ("mdx_graph_search", "mdx_graph_detours")
# (L, W) of the GPU table (tests/test_gpu_graph.py)
BEAMS = [(1, 1), (2, 1), (63, 2), (64, 1), (65, 8), (512, 1), (512, 8)]


# ------------------------------------------------------------------------------------------------------ a. the restatement

def test_walk_by_hand():
    """Six rows on a line, one query: the scores ARE the ids' preference 5 > 4 > 3 > 2 > 1 > 0 (row i scores i).
    graph: 0 -> 1, 2;  1 -> 0, 3;  2 -> 3, 3 (a repeat);  3 -> 4, 3 (a self loop);  4 -> 5, -1;  5 -> 9 (out of range), 4.
    L = 2, W = 1, seeds {0, 0, -1}:
      start  beam [0]                       scored 1
      step 1 expand 0: candidates 1, 2   -> beam [2, 1]     (0 evicted)                scored 3
      step 2 expand 2: candidates 3      -> beam [3, 2e]    (1 evicted, unexpanded)    scored 4
      step 3 expand 3: candidates 4      -> beam [4, 3e]                                 scored 5
      step 4 expand 4: candidates 5      -> beam [5, 4e]                                 scored 6
      step 5 expand 5: 9 invalid, 4 in the beam: no candidates -> beam [5e, 4e]
      no unexpanded entry: stop.  steps 5."""
    scores = np.arange(6, dtype=np.float32)[None, :]
    graph = np.array([[1, 2], [0, 3], [3, 3], [4, 3], [5, -1], [9, 4]], dtype=np.int32)
    seeds = np.array([[0, 0, -1]])
    ids, sc, steps, scored = R.graph_search(scores, graph, seeds, 2, 2)
    assert ids.tolist() == [[5, 4]] and sc.tolist() == [[5.0, 4.0]] and steps.tolist() == [5] and scored.tolist() == [6]
    # T = 2 cuts it after the second step; k = 2 of a beam of 2
    ids, sc, steps, scored = R.graph_search(scores, graph, seeds, 2, 2, T=2)
    assert ids.tolist() == [[3, 2]] and steps.tolist() == [2] and scored.tolist() == [4]
    # W = 2 from seeds {0, 1}: step 1 expands 1 and 0 (beam order), candidates {0.., 3, 2}: beam [3, 2]; step 2 expands 3, 2 -> [4, 3];
    # step 3 expands 4 -> [5, 4]; step 4 expands 5; stop
    ids, _, steps, scored = R.graph_search(scores, graph, np.array([[0, 1]]), 2, 2, W=2)
    assert ids.tolist() == [[5, 4]] and steps.tolist() == [4] and scored.tolist() == [6]
    # a beam longer than what can be reached pads: from seed 3 only 3, 4, 5 are reachable
    ids, sc, steps, _ = R.graph_search(scores, graph, np.array([[3]]), 5, 6)
    assert ids.tolist() == [[5, 4, 3, -1, -1]] and np.isnan(sc[0, 3:]).all() and steps.tolist() == [3]
    # no valid seed: nothing
    ids, sc, steps, scored = R.graph_search(scores, graph, np.array([[-1, 6]]), 1, 2)
    assert ids.tolist() == [[-1]] and np.isnan(sc).all() and steps.tolist() == [0] and scored.tolist() == [0]
    # equal scores go by id, NaN last
    tied = np.array([[1.0, np.nan, 1.0, 1.0, -0.0, 0.0]], dtype=np.float32)
    full = np.array([[1, 2, 3, 4, 5]] * 6, dtype=np.int32)
    ids, _, _, _ = R.graph_search(tied, full, np.array([[5]]), 6, 6)
    assert ids.tolist() == [[2, 3, 4, 5, 1, -1]]                                # row 0 is listed by nobody


def test_detours_by_hand():
    """Row 0 lists [1, 2, 3]; row 1 lists [2, 3, 0]; row 2 lists [3, 0, 1]; row 3 lists [-1, 0, 7] (7 is out of range, n = 4).
    Row 0: b = 1 at j = 0: nothing ranks before it: 0.  b = 2 at j = 1: t = 0 (a = 1): lists[1, :1] = [2] holds it: 1.
           b = 3 at j = 2: t = 0 (a = 1): lists[1, :2] = [2, 3] yes; t = 1 (a = 2): lists[2, :2] = [3, 0] yes: 2.
    Row 3: j = 0 invalid: K0 = 3; b = 0 at j = 1: t = 0 invalid: 0; j = 2 invalid: 3."""
    lists = np.array([[1, 2, 3], [2, 3, 0], [3, 0, 1], [-1, 0, 7]])
    det = R.detours(lists)
    assert det.dtype == np.int32 and det[0].tolist() == [0, 1, 2] and det[3].tolist() == [3, 0, 3]
    # row 1: b = 3 at j = 1: a = 2, lists[2, :1] = [3]: 1;  b = 0 at j = 2: a = 2: lists[2, :2] = [3, 0] yes; a = 3: lists[3, :2] = [-1, 0] yes: 2
    assert det[1].tolist() == [0, 1, 2]


def test_strip_and_interleave_by_hand():
    ids = np.array([[0, 2, 1, 3], [3, 1, 9, 0], [-1, 2, 0, 1], [3, 0, 1, 2]])
    assert R.strip_self(ids).tolist() == [[2, 1, 3], [3, 0, -1], [0, 1, -1], [0, 1, 2]]
    # lists without detours (det = rank order): forward = the first 2 of each list
    lists = np.array([[1, 2, 3], [0, 2, 3], [0, 3, 1], [2, 0, 1]])
    zero = np.zeros_like(lists)
    # forward: 0: [1, 2]; 1: [0, 2]; 2: [0, 3]; 3: [2, 0]
    # reverse of 0: sources holding 0, by (rank, source): (0, 1), (0, 2), (1, 3) -> [1, 2] (the first 2)
    #   row 0: interleave f [1, 2], r [1, 2] -> 1, 1, 2, 2 -> distinct: [1, 2]   (a repeat)
    # reverse of 2: (0, 3), (1, 0), (1, 1) -> [3, 0];  row 2: f [0, 3], r [3, 0] -> 0, 3, 3, 0 -> [0, 3]
    # reverse of 3: (1, 2) -> [2];  row 3: f [2, 0], r [2] -> 2, 2, 0 -> [2, 0]
    # reverse of 1: (0, 0) -> [0];  row 1: f [0, 2], r [0] -> 0, 0, 2 -> [0, 2]
    assert R.optimise(lists, 2, zero).tolist() == [[1, 2], [0, 2], [0, 3], [2, 0]]
    # a self id among the reverse sources cannot occur (lists hold no own id), but one in the forward list is dropped:
    loop = np.array([[0, 1], [0, -1]])
    # forward 0: [0, 1]; 1: [0]; reverse of 0: (0, 0), (0, 1) -> [0, 1]; row 0: 0, 0, 1, 1 -> drop own 0 -> [1, -1]
    # reverse of 1: (1, 0) -> [0]; row 1: f [0], r [0] -> [0, -1]
    assert R.optimise(loop, 2, np.zeros_like(loop)).tolist() == [[1, -1], [0, -1]]
    # the reverse list continues where the forward one ends
    star = np.array([[-1, -1], [0, -1], [0, -1], [0, -1]])
    assert R.optimise(star, 2, R.detours(star)).tolist() == [[1, 2], [0, -1], [0, -1], [0, -1]]


@pytest.mark.parametrize("L,W", BEAMS)
def test_visited_set_changes_scored_only(L, W):
    n, d, nq, Rr, S = 300, 8, 3, 7, 5
    rows, queries, graph, seeds = R.problem(n, d, nq, Rr, S, seed=L * 10 + W)
    scores = R.all_scores(rows, queries)
    k = min(L, 10)
    a = R.graph_search(scores, graph, seeds, k, L, W, T=40)
    b = R.graph_search(scores, graph, seeds, k, L, W, T=40, visited="none")
    np.testing.assert_array_equal(a[0], b[0])
    R.same_scores(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert (a[3] <= b[3]).all() and (b[3] <= S + b[2] * W * Rr).all()


@pytest.mark.parametrize("n,L,W", [(1, 1, 1), (2, 2, 1), (300, 300, 1), (300, 512, 8), (70, 70, 2)])
def test_complete_walk_is_the_exact_topk(n, L, W):
    rng = np.random.default_rng(n + L)
    rows = rng.standard_normal((n, 6)).astype(np.float32)
    queries = rng.standard_normal((4, 6)).astype(np.float32)
    if n > 4:
        rows[3] = rows[1]                                                  # a tie, by id
    scores = R.all_scores(rows, queries)
    graph = R.ring_graph(n, 3)
    k = min(n, 10)
    ids, sc, steps, _ = R.graph_search(scores, graph, np.zeros((4, 1), dtype=np.int64), k, L, W, T=n)
    want = chain.rank_full(scores)[:, :k]
    np.testing.assert_array_equal(ids, want)
    R.same_scores(sc, np.take_along_axis(scores, want, 1))
    assert (steps <= n).all()


def test_optimised_graph_finds_no_less_than_the_plain_one():
    """4096 unit rows by 64 in 64 clusters, 64 noisy queries (graph_restatement.clustered, seed 20); degree 16, k0 32, beam 64, width 1,
    8 seeds from 1024 sampled entries.  On this fixture the restatement gives recall@10 = 0.9891 for the optimised graph and 0.9719 for
    the kNN graph truncated to the same degree (the medoid entries of the issue's prototype are not part of this test).  Asserted: the
    relation, and the optimised graph's value as the restatement gives it."""
    rows, queries, _ = R.clustered()
    lists = R.strip_self(R.knn_lists(rows, 33))
    optimised, plain = R.optimise(lists, 16), R.truncate(lists, 16)
    scores = R.all_scores(rows, queries)
    exact = chain.rank_full(scores)[:, :10]
    entries = np.sort(np.random.default_rng(1).permutation(rows.shape[0])[:1024])
    seeds = entries[chain.rank_full(scores[:, entries])[:, :8]]
    found = {}
    for name, g in (("optimised", optimised), ("plain", plain)):
        found[name] = R.recall(R.graph_search(scores, g, seeds, 10, 64, 1, 256)[0], exact)
    print("recall@10: optimised %.4f, plain %.4f" % (found["optimised"], found["plain"]))
    assert found["optimised"] >= found["plain"]
    assert found["optimised"] - found["plain"] >= 0 and abs(found["optimised"] - 0.9890625) < 1e-12
    # every row of the optimised graph: distinct valid ids, no own id, full where the lists were
    own = np.arange(rows.shape[0])[:, None]
    assert ((optimised >= 0) & (optimised < rows.shape[0]) & (optimised != own)).all()
    assert all(len(set(r.tolist())) == 16 for r in optimised[:200])


def test_medoids_restatement():
    rows = np.array([[1, 0], [0.9, 0.1], [0, 1], [0, 1], [0.5, 0.5]], dtype=np.float32)
    cents = np.array([[1, 0], [0, 1], [-1, -1]], dtype=np.float32)
    # list 0: rows 0, 1, 4 -> 0; list 1: rows 2, 3 tie -> 2; list 2 empty
    assert R.medoids(rows, cents, np.array([0, 0, 1, 1, 0])).tolist() == [0, 2]


# ------------------------------------------------------------------------------------------------------------- b. census

def _declared():
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    assert re.search(r'^#include "mdx_graph.h"$', text, flags=re.M) and "graph index" in text
    assert text.index('#include "mdx_overlap.h"') < text.index('#include "mdx_graph.h"')
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx_graph.h")).read(), flags=re.S)


def test_every_graph_entry_point_is_covered():
    from mdir_amd import _lib, ops
    from test_gpu_graph_memcontract import CASES, COVERED
    declared = set(re.findall(r"\b(mdx_[a-z0-9_]+)\s*\(", _declared()))
    assert declared == set(_lib.GRAPH_EXPORTS) == set(NEW)
    others = [name for name in dir(_lib) if name.endswith("EXPORTS") and name != "GRAPH_EXPORTS"]
    assert {"EXPORTS", "KNN_JOIN_EXPORTS", "OVERLAP_EXPORTS", "KNN_REVERSE_EXPORTS", "IVF_EXPORTS"} <= set(others)
    for other in others:
        assert not declared & set(getattr(_lib, other)), other
    assert not {n for n in declared if "_workspace" in n}
    assert {"mdx_" + entry for entry in COVERED} == declared
    assert sum(len(c) for c in COVERED.values()) == len(CASES)
    for entry, cases in COVERED.items():
        assert len(cases) >= 2 and all(c.larger in cases and c.larger is not c for c in cases), entry
    mdx_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    assert not re.search(r"\bmdx_graph_[a-z]+\s*\(", mdx_h)
    header = open(os.path.join(ROOT, "include", "mdx_graph.h")).read()
    for name, value, mine in (("D", R.MAX_D, ops.GRAPH_MAX_D), ("DEGREE", R.MAX_DEGREE, ops.GRAPH_MAX_DEGREE),
                              ("SEEDS", R.MAX_SEEDS, ops.GRAPH_MAX_SEEDS), ("BEAM", R.MAX_BEAM, ops.GRAPH_MAX_BEAM),
                              ("WIDTH", R.MAX_WIDTH, ops.GRAPH_MAX_WIDTH), ("CANDIDATES", R.MAX_CANDIDATES, ops.GRAPH_MAX_CANDIDATES),
                              ("K0", R.MAX_K0, ops.GRAPH_MAX_K0)):
        assert "#define MDX_GRAPH_MAX_%s %d\n" % (name, value) in header and value == mine, name
    assert len(re.findall(r"#define MDX_GRAPH_MAX_", header)) == 7
    assert "#define MDX_ABI_VERSION 3\n" in open(os.path.join(ROOT, "include", "mdx.h")).read() and _lib.ABI_VERSION == 3
    makefile = open(os.path.join(ROOT, "mdir_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bmdx_graph\.hip\b", makefile, flags=re.M) and "include/mdx_graph.h" in makefile
    assert '"mdx_graph.h"' in open(os.path.join(ROOT, "mdir_amd", "_lib.py")).read()


# --------------------------------------------------------------------------------------------------- c. refusals, no device

def test_library_exports_binds_and_refuses_before_any_device_work():
    from mdir_amd import _lib
    _lib.build()
    h = _lib.lib()
    fn = h.mdx_graph_search
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 22
    assert h.mdx_abi_version() == _lib.ABI_VERSION == 3
    P = lambda i: ctypes.c_void_p(4096 + (i << 20))
    err = lambda: h.mdx_last_error()
    # rows n d ld graph R queries nq qlayout center seeds S k L W T table_bits ids scores steps scored stream
    good = dict(rows=P(0), n=100, d=64, ld=64, graph=P(1), R=8, queries=P(2), nq=3, qlayout=1, center=None, seeds=P(3), S=4, k=5, L=16, W=1,
                T=10, table_bits=0, ids=P(4), scores=P(5), steps=P(6), scored=P(7), stream=None)

    def refused(what, **change):
        args = dict(good, **change)
        assert fn(*args.values()) == -1, change
        assert b"mdx_graph_search" in err() and what in err(), (change, err())

    for name in ("rows", "graph", "queries", "seeds", "ids", "scores", "steps", "scored"):
        refused(b"NULL", **{name: None})
    for change in ({"n": 0}, {"n": 1 << 31}, {"nq": 0}, {"nq": 1 << 31}):
        refused(b"must be in [1, 2^31)", **change)
    for d in (0, R.MAX_D + 1):
        refused(b"d=%d must be in [1, 8192]" % d, d=d, ld=max(d, 1))
    refused(b"ld=63 < d=64", ld=63)
    for lay in (-1, 2):
        refused(b"qlayout %d" % lay, qlayout=lay)
    for deg in (0, R.MAX_DEGREE + 1):
        refused(b"R=%d must be in [1, 64]" % deg, R=deg)
    for s in (0, R.MAX_SEEDS + 1):
        refused(b"S=%d must be in [1, 512]" % s, S=s)
    for beam in (0, R.MAX_BEAM + 1):
        refused(b"L=%d must be in [1, 512]" % beam, L=beam, k=1)
    for k in (0, 17):
        refused(b"k=%d must be in [1, L=16]" % k, k=k)
    for w in (0, R.MAX_WIDTH + 1):
        refused(b"W=%d must be in [1, 8]" % w, W=w)
    refused(b"T=0 must be >= 1", T=0)
    for tb in (-1, 1, 7, 15):
        refused(b"table_bits=%d must be 0 or in [8, 14]" % tb, table_bits=tb)
    for name in ("seeds", "ids"):
        refused(b"8-byte aligned", **{name: ctypes.c_void_p(good[name].value + 4)})
    for name in ("rows", "graph", "queries", "scores", "steps", "scored"):
        refused(b"4-byte aligned", **{name: ctypes.c_void_p(good[name].value + 2)})
    refused(b"4-byte aligned", center=ctypes.c_void_p(8194))

    fd = h.mdx_graph_detours
    assert fd.restype is ctypes.c_int and len(fd.argtypes) == 5
    assert fd(None, 4, 4, P(1), None) == -1 and b"mdx_graph_detours: NULL" in err()
    assert fd(P(0), 4, 4, None, None) == -1 and b"mdx_graph_detours: NULL" in err()
    for n in (0, 1 << 31):
        assert fd(P(0), n, 4, P(1), None) == -1 and b"mdx_graph_detours: n=%d must be in [1, 2^31)" % n in err()
    for k0 in (0, R.MAX_K0 + 1):
        assert fd(P(0), 4, k0, P(1), None) == -1 and b"mdx_graph_detours: K0=%d must be in [1, 128]" % k0 in err()
    assert fd(ctypes.c_void_p(4100), 4, 4, P(1), None) == -1 and b"mdx_graph_detours: lists must be 8-byte aligned" in err()
    assert fd(P(0), 4, 4, ctypes.c_void_p(4098), None) == -1 and b"aligned" in err()


def test_wrapper_checks_need_no_gpu():
    from mdir_amd import graph, ops
    rows = torch.zeros((4, 8))
    g = torch.zeros((4, 2), dtype=torch.int32)
    seeds = torch.zeros((1, 1), dtype=torch.int64)
    with pytest.raises(ValueError, match="graph_search: rows must be a CUDA/ROCm tensor.*no CPU fallback"):
        ops.graph_search(rows, g, rows[:1], seeds, 1, 2)
    with pytest.raises(ValueError, match="graph_detours: lists must be a CUDA/ROCm tensor.*no CPU fallback"):
        ops.graph_detours(torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        graph.GraphIndex.from_lists(rows, torch.zeros((4, 3), dtype=torch.int64), 2)
    assert graph.GraphResult._fields == ("ids", "scores", "steps", "scored")


GRAPH = {"index": "graph", "depth": 10, "degree": 16, "beam": 64}


def test_graph_route_of_the_search_key():
    from mdir_amd import ops
    from mdir_amd.score import _search_params
    assert _search_params(dict(GRAPH)) == dict(GRAPH, recall=False, k0=32, width=1, seeds=8, entries="sample", n_entries=1024,
                                               neighbours="exact")
    got = _search_params(dict(GRAPH, entries="medoids", lists=24, iters=5, seed=3, neighbours="i8", k0=20, width=2, seeds=4, recall=True))
    assert (got["entries"], got["lists"], got["iters"], got["seed"], got["neighbours"], got["k0"], got["width"], got["seeds"]) == \
        ("medoids", 24, 5, 3, "i8", 20, 2, 4) and "n_entries" not in got
    got = _search_params(dict(GRAPH, neighbours={"ivf": {"lists": 64, "nprobe": 8}}))
    assert got["neighbours"] == {"ivf": {"lists": 64, "nprobe": 8, "storage": "i8", "reverse": True, "shortlist": 132}}
    for key in ("degree", "beam"):
        value = dict(GRAPH)
        del value[key]
        with pytest.raises(ValueError, match="search: index: graph: %s is required" % key):
            _search_params(value)
    with pytest.raises(ValueError, match="search: index: graph: depth is required"):
        _search_params({"index": "graph", "degree": 4, "beam": 8})
    with pytest.raises(ValueError, match=r"search: index: graph: unknown keys \['nprobe', 'shortlist'\] \(allowed: index, depth, recall, degree, k0, beam"):
        _search_params(dict(GRAPH, nprobe=2, shortlist=100))
    with pytest.raises(ValueError, match="search: index: graph: depth = 513 is above the beam limit 512"):
        _search_params(dict(GRAPH, depth=513, beam=512))
    for bad in (9, 513, 64.0, True):
        with pytest.raises(ValueError, match=r"search: beam must be an integer in \[10, 512\]"):
            _search_params(dict(GRAPH, beam=bad))
    for bad in (0, ops.GRAPH_MAX_DEGREE + 1, "16"):
        with pytest.raises(ValueError, match=r"search: degree must be an integer in \[1, 64\]"):
            _search_params(dict(GRAPH, degree=bad))
    for bad in (0, ops.GRAPH_MAX_K0 + 1):
        with pytest.raises(ValueError, match=r"search: k0 must be an integer in \[1, 128\]"):
            _search_params(dict(GRAPH, k0=bad))
    with pytest.raises(ValueError, match=r"search: width must be an integer in \[1, 8\]"):
        _search_params(dict(GRAPH, width=9))
    with pytest.raises(ValueError, match=r"search: width must be an integer in \[1, 8\]"):
        _search_params(dict(GRAPH, degree=64, width=9))
    for bad in (0, 513):
        with pytest.raises(ValueError, match=r"search: seeds must be an integer in \[1, 512\]"):
            _search_params(dict(GRAPH, seeds=bad))
    with pytest.raises(ValueError, match="search: entries must be 'sample' or 'medoids'"):
        _search_params(dict(GRAPH, entries="random"))
    with pytest.raises(ValueError, match="entries: medoids needs lists"):
        _search_params(dict(GRAPH, entries="medoids"))
    with pytest.raises(ValueError, match="n_entries goes with entries: sample"):
        _search_params(dict(GRAPH, entries="medoids", lists=4, n_entries=10))
    with pytest.raises(ValueError, match="lists and iters go with entries: medoids"):
        _search_params(dict(GRAPH, lists=4))
    with pytest.raises(ValueError, match="search: n_entries must be an integer >= 1"):
        _search_params(dict(GRAPH, n_entries=0))
    with pytest.raises(ValueError, match="search: neighbours: 'exact' or 'i8', or the mapping"):
        _search_params(dict(GRAPH, neighbours="f16"))
    with pytest.raises(ValueError, match=r"neighbours: i8 keeps at most 64 neighbours per row \(KNN_JOIN_MAX_K\); k0 \+ 1 = 65"):
        _search_params(dict(GRAPH, degree=32, neighbours="i8"))
    with pytest.raises(ValueError, match="neighbours: ivf: nprobe is required"):
        _search_params(dict(GRAPH, neighbours={"ivf": {"lists": 4}}))
    with pytest.raises(ValueError, match=r"neighbours: ivf keeps at most 128 neighbours per row"):
        _search_params(dict(GRAPH, k0=128, neighbours={"ivf": {"lists": 4, "nprobe": 2}}))


def test_messages_of_the_existing_routes_are_unchanged():
    from mdir_amd.score import _search_params
    with pytest.raises(ValueError, match=r"search: index: exact: unknown keys \['shortlist'\] \(allowed: index, depth, recall\)$"):
        _search_params({"index": "exact", "depth": 5, "shortlist": 9})
    with pytest.raises(ValueError, match=r"^search: index: ivf: unknown keys \['beam'\] \(allowed: index, depth, recall, lists, nprobe, storage, "
                                         r"shortlist, exact, iters, seed\)$"):
        _search_params({"index": "ivf", "depth": 5, "lists": 4, "nprobe": 2, "beam": 8})
    with pytest.raises(ValueError, match="^search: index: ivfpq: nprobe is required$"):
        _search_params({"index": "ivfpq", "depth": 5, "lists": 2})
    with pytest.raises(ValueError, match=r"^search: depth must be an integer in \[1, 4096\], got 600\.0$"):
        _search_params({"index": "exact", "depth": 600.0})
    assert _search_params({"index": "exact", "depth": 600}) == {"index": "exact", "depth": 600, "recall": False}
    assert _search_params({"index": "ivf", "depth": 100, "lists": 64, "nprobe": 8}) == \
        {"index": "ivf", "depth": 100, "lists": 64, "nprobe": 8, "storage": "i8", "shortlist": None, "exact": False, "recall": False}
    with pytest.raises(ValueError, match=r"search: a mapping \{index: exact \| i8 \| f16 \| ivf \| ivfpq \| graph, depth: K, \.\.\.\}"):
        _search_params({"index": "flat", "depth": 5})


def test_overlay_parses(tmp_path):
    import yaml
    from test_search_key_host import _score
    with open(os.path.join(ROOT, "scenarios", "eval_search_graph.yml")) as f:
        doc = yaml.safe_load(f)
    assert set(doc) == {"validation"} and doc["validation"]
    for ds, entry in doc["validation"].items():
        crit = entry["criterion"]
        assert set(crit) == {"search"} and crit["search"]["index"] == "graph"
        s = _score(tmp_path, **crit)
        assert s.search["depth"] == crit["search"]["depth"] and s.search["beam"] >= s.search["depth"] and s.search["recall"] is True
