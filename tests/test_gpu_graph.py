"""The graph index on the device (include/mdx_graph.h; ops.graph_search, ops.graph_detours; mdir_amd/graph.py): ids, score bits and
steps equal to the numpy restatement (tests/graph_restatement.py) at the boundaries of every size, on graphs and seeds with padding,
out-of-range ids, repeats and self loops, on special values, at every table size, under stream capture; the build against its
restatement for all three sources of neighbour lists."""
import numpy as np
import pytest
import torch

import graph_restatement as R
import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def strided(rows, ld, shift=0):
    """``rows`` on the device at row stride ``ld``; ``shift`` floats past a 16-byte boundary."""
    n, d = rows.shape
    base = torch.full((n * ld + 8,), float("nan"), dtype=torch.float32, device=DEV)
    view = base[shift:shift + n * ld].view(n, ld)[:, :d]
    view.copy_(dev(rows))
    return view


def check(got, want, scored_bound=None):
    np.testing.assert_array_equal(host(got[0]), want[0])
    R.same_scores(host(got[1]), want[1])
    np.testing.assert_array_equal(host(got[2]), want[2])
    scored = host(got[3])
    assert (scored >= (want[0] >= 0).sum(axis=1)).all()
    if scored_bound is not None:
        assert (scored <= scored_bound).all()


# n, d, ld, shift, nq, R, S, k, L, W, T
SHAPES = [
    (300, 1, 4, 0, 3, 7, 5, 1, 1, 1, 20),             # L = 1, k = 1, S above L
    (300, 63, 64, 0, 3, 7, 2, 2, 2, 1, 50),           # S at L, k = L
    (300, 64, 68, 0, 70, 32, 8, 10, 63, 2, 30),       # 70 queries, S below L
    (300, 65, 67, 0, 3, 7, 64, 64, 64, 1, 40),        # ld % 4 != 0: the scalar path of row_piece
    (300, 70, 72, 1, 1, 1, 3, 5, 65, 8, 1000),        # rows off the 16-byte boundary; R = 1, W = 8, one query
    (300, 256, 260, 0, 3, 64, 9, 100, 512, 8, 5),     # W * R = 512, L = 512, T cuts the walk short
    (300, 2048, 2052, 0, 3, 32, 4, 10, 64, 1, 1),     # T = 1
    (1, 64, 64, 0, 1, 1, 1, 1, 1, 1, 3),              # one row
    (2, 65, 68, 0, 3, 7, 3, 2, 2, 2, 5),              # two rows
    (300, 64, 64, 0, 3, 7, 512, 300, 512, 1, 400),    # S = 512; k above the reachable rows: padding
]


@pytest.mark.parametrize("shape", SHAPES, ids=["n%d-d%d-ld%d+%d-q%d-R%d-S%d-k%d-L%d-W%d-T%d" % s for s in SHAPES])
def test_shape_table(shape):
    from mdir_amd import ops
    n, d, ld, shift, nq, deg, S, k, L, W, T = shape
    rows, queries, graph, seeds = R.problem(n, d, nq, deg, S, seed=11)
    if shape == SHAPES[-1]:                                                                      # the first 100 rows are a world of their own
        graph[graph >= 100], seeds = -1, seeds % 100
    want = R.graph_search(R.all_scores(rows, queries), graph, seeds, k, L, W, T)
    got = ops.graph_search(strided(rows, ld, shift), dev(graph), dev(queries), dev(seeds), k, L, W, T)
    check(got, want, S + want[2] * W * deg)
    if shape == SHAPES[-1]:
        assert (want[0][:, 100:] == -1).all() and (want[0][:, 0] >= 0).all() and np.isnan(host(got[1])[:, 100:]).all()


def test_graphs_and_seeds_with_padding_components_and_no_valid_seed():
    from mdir_amd import ops
    n, d, nq = 300, 24, 4
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    # two components: a ring over rows 0 .. 149 and one over 150 .. 299, with -1, out-of-range ids, a repeat and a self loop per row
    half = n // 2
    ring = ((np.arange(half)[:, None] + 1 + np.arange(3)[None, :]) % half).astype(np.int32)
    graph = np.full((n, 8), -1, dtype=np.int32)
    graph[:half, :3], graph[half:, :3] = ring, ring + half
    graph[:, 4] = n + 7
    graph[:, 5] = graph[:, 0]
    graph[:, 6] = np.arange(n)
    graph[:, 7] = np.iinfo(np.int32).max
    seeds = np.array([[3, -1, 3, n], [-1, -5, n + 1, 2 ** 40], [200, 150, 150, 150], [10, 160, -1, -1]], dtype=np.int64)
    scores = R.all_scores(rows, queries)
    for L, W, T in ((400, 1, 1000), (16, 2, 1000), (150, 8, 1000)):
        want = R.graph_search(scores, graph, seeds, min(L, 200), L, W, T)
        got = ops.graph_search(dev(rows), dev(graph), dev(queries), dev(seeds), min(L, 200), L, W, T)
        check(got, want)
        assert want[2][1] == 0 and (want[0][1] == -1).all() and host(got[3])[1] == 0                  # no valid seed
    # the walk cannot leave a component: query 0 sees rows below 150 only, and with L >= 150 all of them, every one expanded
    want = R.graph_search(scores, graph, seeds, 200, 400, 1, 1000)
    assert (want[0][0, :half] < half).all() and (want[0][0, half:] == -1).all() and want[2][0] == half


def test_ties_nan_and_lattice():
    from mdir_amd import ops
    # duplicate rows: equal scores resolve by id
    n, d = 120, 16
    rng = np.random.default_rng(8)
    base = rng.standard_normal((n // 4, d)).astype(np.float32)
    rows = np.concatenate([base, base, base, base])[rng.permutation(n)]
    queries = rng.standard_normal((3, d)).astype(np.float32)
    queries[1, 5] = np.nan                                                                       # every score of query 1 is NaN
    graph = R.random_graph(rng, n, 7)
    seeds = rng.integers(0, n, size=(3, 6)).astype(np.int64)
    scores = R.all_scores(rows, queries)
    assert np.isnan(scores[1]).all()
    for L, W in ((20, 1), (64, 2)):
        want = R.graph_search(scores, graph, seeds, L, L, W, 100)
        check(ops.graph_search(dev(rows), dev(graph), dev(queries), dev(seeds), L, L, W, 100), want)
    assert (np.diff(want[0][1][want[0][1] >= 0]) > 0).all()                                     # all NaN: the order is the id's
    # exactly representable data: the scores are integers, whatever the order of the products
    for centred in (False, True):
        lat = lattice.common(300, 70, 5, seed=3, centred=centred)
        lattice.assert_exact_in_any_order(lat.qi.astype(np.float64), lat.xi.astype(np.float64))
        exact = lattice.expected(lat.qi, lat.xi, 1.0)
        graph = R.random_graph(np.random.default_rng(4), 300, 32)
        seeds = np.random.default_rng(6).integers(0, 300, size=(5, 8)).astype(np.int64)
        want = R.graph_search(exact, graph, seeds, 30, 64, 2, 100)
        center = None if lat.center is None else dev(lat.center)
        got = ops.graph_search(strided(lat.db, 72), dev(graph), dev(lat.queries), dev(seeds), 30, 64, 2, 100, center=center)
        check(got, want)
        np.testing.assert_array_equal(R.bits(host(got[1])), R.bits(want[1]))                     # integers, +0 for zero: plain bit equality


def test_table_bits_change_scored_only():
    from mdir_amd import ops
    n, d, nq, deg, S = 3000, 16, 4, 32, 8
    rows, queries, graph, seeds = R.problem(n, d, nq, deg, S, seed=21)
    want = R.graph_search(R.all_scores(rows, queries), graph, seeds, 50, 128, 2, 60)
    assert want[3].min() > 256                                                                   # more rows than the smallest table holds
    args = (dev(rows), dev(graph), dev(queries), dev(seeds), 50, 128, 2, 60)
    runs = {tb: ops.graph_search(*args, table_bits=tb) for tb in (8, 14, 0)}
    for tb, got in runs.items():
        check(got, want, S + want[2] * 2 * deg)
        for a, b in zip(got[:3], runs[0][:3]):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), tb
    np.testing.assert_array_equal(host(runs[14][3]), want[3])                                    # a table that holds every row: no chain twice
    assert (host(runs[8][3]) >= want[3]).all()
    for bad in (1, 7, 15, -8):
        with pytest.raises(ValueError, match="table_bits"):
            ops.graph_search(*args, table_bits=bad)


def test_a_query_depends_on_its_own_inputs_only():
    from mdir_amd import ops
    n, d, nq, deg, S = 300, 70, 7, 7, 5
    rows, queries, graph, seeds = R.problem(n, d, nq, deg, S, seed=31)
    center = np.random.default_rng(2).standard_normal(d).astype(np.float32)
    rows_t, graph_t = strided(rows, 72), dev(graph)
    for c in (None, center):
        want = R.graph_search(R.all_scores(rows, queries, c), graph, seeds, 10, 32, 2, 50)
        c_t = None if c is None else dev(c)
        got = ops.graph_search(rows_t, graph_t, dev(queries), dev(seeds), 10, 32, 2, 50, center=c_t)
        check(got, want)
        dn = ops.graph_search(rows_t, graph_t, dev(queries.T), dev(seeds), 10, 32, 2, 50, qlayout="DN", center=c_t)
        perm = np.random.default_rng(3).permutation(nq)
        moved = ops.graph_search(rows_t, graph_t, dev(queries[perm]), dev(seeds[perm]), 10, 32, 2, 50, center=c_t)
        alone = ops.graph_search(rows_t, graph_t, dev(queries[4:5]), dev(seeds[4:5]), 10, 32, 2, 50, center=c_t)
        for j in range(4):
            a = host(got[j].view(torch.int32) if j == 1 else got[j])
            np.testing.assert_array_equal(host(dn[j].view(torch.int32) if j == 1 else dn[j]), a)
            np.testing.assert_array_equal(host(moved[j].view(torch.int32) if j == 1 else moved[j]), a[perm])
            np.testing.assert_array_equal(host(alone[j].view(torch.int32) if j == 1 else alone[j]), a[4:5])


def test_complete_walk_is_topk_of_the_index():
    from mdir_amd import ops
    n, d, nq = 300, 65, 6
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[17] = rows[5]
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    rows_t, q_t = dev(rows), dev(queries)
    index = ops.DescriptorIndex(rows_t, "ND")
    try:
        want_ids, want_scores = ops.topk(index.scores(q_t, "ND"), 40)
    finally:
        index.close()
    seeds = torch.zeros((nq, 1), dtype=torch.int64, device=DEV)
    for L, W in ((300, 1), (512, 8)):
        ids, scores, steps, scored = ops.graph_search(rows_t, dev(R.ring_graph(n, 3)), q_t, seeds, 40, L, W, n)
        assert torch.equal(ids, want_ids) and torch.equal(scores.view(torch.int32), want_scores.view(torch.int32))
        assert int(scored.min()) == int(scored.max()) == n and int(steps.max()) <= n


@pytest.mark.parametrize("k0", (1, 2, 63, 64, 65, 128))
def test_detours(k0):
    from mdir_amd import ops
    n = max(k0 + 6, 9)
    rng = np.random.default_rng(k0)
    lists = np.stack([rng.permutation(n + 3)[:k0] for _ in range(n)]).astype(np.int64)          # distinct; n .. n + 2 are out of range
    lists[rng.random(lists.shape) < 0.1] = -1
    lists[0, 0] = 2 ** 33 + 1                                                                    # its low 32 bits would be row 1
    got = ops.graph_detours(dev(lists))
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(host(got), R.detours(lists))


@pytest.fixture(scope="module")
def small():
    rows, queries, _ = R.clustered(n=400, d=32, clusters=8, nq=5, seed=7)
    return rows, queries, dev(rows), dev(queries)


def test_build_from_every_source_of_lists(small):
    from mdir_amd import graph, ivf, ops, search
    rows, queries, rows_t, q_t = small
    degree, k0 = 8, 20
    lists = R.strip_self(R.knn_lists(rows, k0 + 1))
    want = R.optimise(lists, degree)
    np.testing.assert_array_equal(host(graph.strip_self(search.knn_join(None, rows_t, k0 + 1).ids)), lists)
    built = {}
    built["exact"] = graph.GraphIndex.build(rows_t, degree, k0, n_entries=50, seed=4)
    i8 = ops.DescriptorIndex(rows_t, "ND", storage="i8")
    coarse = ivf.IVFIndex.train(rows_t, 4, storage="f32", iters=3)
    try:
        built["i8"] = graph.GraphIndex.build(rows_t, degree, k0, neighbours=i8, n_entries=50, seed=4)
        built["ivf"] = graph.GraphIndex.build(rows_t, degree, k0, neighbours=ivf.IVFNeighbours(coarse, 4), n_entries=50, seed=4)
        built["lists"] = graph.GraphIndex.from_lists(rows_t, search.knn_join(None, rows_t, k0 + 1), degree, entries=built["exact"].entries)
    finally:
        i8.close()
        coarse.close()
    try:
        for name, index in built.items():                                                      # two builds agree, to the bit, with the restatement
            assert index.graph.dtype == torch.int32 and (index.n, index.d, index.degree) == (400, 32, degree)
            np.testing.assert_array_equal(host(index.graph), want, err_msg=name)
            assert torch.equal(index.entries, built["exact"].entries) and index.entries.shape == (50,)
        index = built["exact"]
        assert index.nbytes() >= 400 * degree * 4 + 50 * 8
        # the search: seeds from the entry rows, then the walk of the restatement
        scores = R.all_scores(rows, queries)
        entries = host(index.entries)
        seeds = entries[R.chain.rank_full(scores[:, entries])[:, :4]]
        np.testing.assert_array_equal(host(index.seeds_of(q_t, 4)), seeds)
        res = index.search(q_t, 10, beam=32, width=2, seeds=4)
        check(res, R.graph_search(scores, want, seeds, 10, 32, 2, 64))
        explicit = index.search(q_t, 10, beam=32, width=2, seeds=dev(seeds))
        assert torch.equal(res.ids, explicit.ids) and torch.equal(res.steps, explicit.steps)
        # state -> from_state
        again = graph.GraphIndex.from_state(index.state(), rows_t)
        try:
            back = again.search(q_t, 10, beam=32, width=2, seeds=4)
            assert torch.equal(back.ids, res.ids) and torch.equal(back.scores.view(torch.int32), res.scores.view(torch.int32))
            assert torch.equal(back.steps, res.steps) and set(index.state()) == {"graph", "entries", "n", "degree"}
        finally:
            again.close()
        index.close()
        with pytest.raises(ValueError, match="closed"):
            index.search(q_t, 10)
    finally:
        for index in built.values():
            index.close()


def test_entries_outside_the_rows_are_refused(small):
    from mdir_amd import graph
    _, _, rows_t, _ = small
    edges = dev(R.ring_graph(400, 4))
    for bad in ([0, 400], [-1, 3]):
        with pytest.raises(ValueError, match=r"entries must be ids in \[0, 400\)"):
            graph.GraphIndex(rows_t, edges, dev(np.array(bad, dtype=np.int64)))
    state = {"graph": edges.cpu(), "entries": torch.tensor([5, 400]), "n": 400, "degree": 4}
    with pytest.raises(ValueError, match="entries must be ids"):
        graph.GraphIndex.from_state(state, rows_t)


def test_medoids(small):
    from mdir_amd import cluster, graph
    rows, _, rows_t, _ = small
    km = cluster.kmeans(rows_t, 12, iters=4, seed=1)
    want = R.medoids(rows, host(km.centroids), host(km.labels))
    np.testing.assert_array_equal(host(graph.medoids(rows_t, km.centroids)), want)
    np.testing.assert_array_equal(host(graph.medoids(rows_t, km.centroids, km.labels)), want)
    assert len(want) == int((km.sizes > 0).sum())
    # duplicate rows: the tie goes to the smaller id
    twice = dev(np.concatenate([rows[:50], rows[:50]]))
    cents = twice[:3].contiguous()
    labels, _ = cluster.assign(cents, twice)
    got = host(graph.medoids(twice, cents))
    np.testing.assert_array_equal(got, R.medoids(host(twice), host(cents), host(labels)))
    assert (got < 50).all()


def test_capture_on_a_side_stream():
    from mdir_amd import ops
    n, d, nq, deg, S = 300, 70, 5, 7, 6
    data = [R.problem(n, d, nq, deg, S, seed=s, spoil=bool(s % 2)) for s in (51, 52)]
    rows_t, q_t, graph_t, seeds_t = (dev(x).clone() for x in data[0])

    def eager():
        return ops.graph_search(rows_t, graph_t, q_t, seeds_t, 10, 32, 2, 40)
    eager()                                                                                    # eager once, before anything is recorded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                                                 # one stream, one launch: no parallel branches
            outs_g = eager()
    torch.cuda.current_stream().wait_stream(side)
    for rows, queries, graph, seeds in (data[1], data[0]):                                     # new data, then the old again
        rows_t.copy_(dev(rows)), graph_t.copy_(dev(graph)), q_t.copy_(dev(queries)), seeds_t.copy_(dev(seeds))
        g.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in outs_g]
        want = R.graph_search(R.all_scores(rows, queries), graph, seeds, 10, 32, 2, 40)
        for a, b in zip(got, eager()):
            np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                          host(b).view(np.int32) if b.dtype == torch.float32 else host(b))
        np.testing.assert_array_equal(got[0], want[0])
        R.same_scores(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
