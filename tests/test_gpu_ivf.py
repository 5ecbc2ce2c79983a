"""The inverted file on the device (include/mdx_ivf.h; mdir_amd/ivf.py), bit for bit: the scan and the selection against the
restatement (tests/ivf_restatement.py) applied to the scores of an fp32 index of the same rows, ``nprobe == K`` against ``ops.topk``,
lists shared by 0, 1, a group and more than two groups of queries, special values, both routes of the selection, planted clusters,
``IVFIndex.train``, run-to-run equality and the three calls under graph capture."""
import numpy as np
import pytest
import torch

import ivf_restatement as IR
import kmeans_restatement as KR
import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
G = IR.QUERY_GROUP
SIZES = (0, 1, 63, 64, 65, 130)                     # the lists of the sweep: empty, one row, around a tile, two tiles and a bit


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def exact_scores(rows, queries, qlayout="ND", center=None):
    """fp32 [nq, n]: the scores of an fp32 index of the rows, the bits every route has to return."""
    from mdir_amd import ops
    index = ops.DescriptorIndex(dev(rows), "ND")
    try:
        return host(index.scores(dev(queries), qlayout, center=None if center is None else dev(center)))
    finally:
        index.close()


def placed(rows, ld, offset):
    """The rows on the device at row stride ``ld`` floats, ``offset`` floats behind a 16-byte boundary; the gaps hold NaN."""
    n, d = rows.shape
    flat = torch.full((n * ld + offset + 4,), float("nan"), device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + n * ld].view(n, ld)[:, :d]
    view.copy_(dev(rows))
    return view


def placements(d):
    up = (d + 3) // 4 * 4
    return (("contiguous", d, 0), ("stride on the 16-byte grid", up + 4, 0), ("stride off the grid", up + 5, 0), ("base off the grid", up + 4, 1))


def labels_of_sizes(rng, sizes):
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)


def check_result(res, labels, lists, scores, k):
    """The result of a search equals the restatement applied to the full score matrix, for the probes it reports."""
    ids, sc, scanned = IR.search_labels(labels, lists, host(res.probes), scores, k)
    IR.same_bits(host(res.scanned), scanned)
    IR.same_bits(host(res.ids), ids)
    IR.same_bits(host(res.scores), sc)
    return scanned


# ------------------------------------------------------------------------------------------------ scan + select against the restatement

@pytest.mark.parametrize("d", [1, 4, 63, 64, 65, 260])
def test_search_equals_the_restatement(d):
    from mdir_amd import ivf, ops
    rng = np.random.default_rng(d)
    lists, n = len(SIZES), sum(SIZES)
    rows = rng.standard_normal((n, d)).astype(F32)
    centroids = rng.standard_normal((lists, d)).astype(F32)
    center = rng.standard_normal(d).astype(F32)
    labels = labels_of_sizes(rng, SIZES)
    cents_t, labels_t = dev(centroids), dev(labels)
    indexes = [(name, ivf.IVFIndex(placed(rows, ld, off), cents_t, labels_t)) for name, ld, off in placements(d)]
    coarse = ops.DescriptorIndex(cents_t, "ND")
    for name, index in indexes:
        assert (index.rows.data_ptr() % 16 == 0) == ("base off" not in name) and index.host_sizes == list(SIZES)
        IR.same_bits(host(index.order), KR.csr(labels, lists)[0])
    turn = 0
    try:
        for nq in (1, 3, 9):
            queries = rng.standard_normal((nq, d)).astype(F32)
            for qlayout, with_center in (("ND", False), ("ND", True), ("DN", False), ("DN", True)):
                given = np.ascontiguousarray(queries.T) if qlayout == "DN" else queries
                c = center if with_center else None
                scores = exact_scores(rows, given, qlayout, c)
                q_t, c_t = dev(given), None if c is None else dev(c)
                for nprobe in (1, 2, lists):
                    want_probes = ops.topk(coarse.scores(q_t, qlayout, center=c_t), nprobe)[0]
                    name, index = indexes[turn % len(indexes)]                 # every placement meets every nq, layout and nprobe
                    turn += 1
                    first = index.search(q_t, 1, nprobe, qlayout, c_t)
                    assert torch.equal(first.probes, want_probes), (name, nq, qlayout, nprobe)
                    scanned = check_result(first, labels, lists, scores, 1)
                    assert first.ids.shape == (nq, 1) and first.scanned.dtype == torch.int64 and scanned.max() <= index.capacity(nprobe)
                    # k = 7, exactly the candidates of the query with the most (the others are padded), and three more than that
                    for k in sorted({7, max(1, int(scanned.max())), int(scanned.max()) + 3, max(1, int(scanned.min()))}):
                        res = index.search(q_t, k, nprobe, qlayout, c_t)
                        check_result(res, labels, lists, scores, k)
                        short = host(res.scanned) < k
                        assert (host(res.ids)[short, -1] == -1).all() and np.isnan(host(res.scores)[short, -1]).all(), (name, k)
    finally:
        coarse.close()
        for _, index in indexes:
            index.close()
    assert turn == 36


def test_query_chunks_change_no_bit(monkeypatch):
    from mdir_amd import ivf
    rng = np.random.default_rng(5)
    rows, cents, queries = (rng.standard_normal(s).astype(F32) for s in ((sum(SIZES), 20), (len(SIZES), 20), (9, 20)))
    labels = labels_of_sizes(rng, SIZES)
    index = ivf.IVFIndex(dev(rows), dev(cents), dev(labels))
    try:
        for qlayout, q in (("ND", queries), ("DN", np.ascontiguousarray(queries.T))):
            whole = index.search(dev(q), 12, 3, qlayout)
            monkeypatch.setattr(ivf, "CANDIDATE_MEMORY_CAP", 12 * index.capacity(3) * 4)       # four queries per step
            assert index.query_chunk(3) == 4
            parts = index.search(dev(q), 12, 3, qlayout)
            monkeypatch.undo()
            for a, b in zip(whole, parts):
                IR.same_bits(host(a), host(b))
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------ nprobe == K against ops.topk

def test_all_lists_probed_equals_topk_on_a_long_chain():
    from mdir_amd import ivf, ops
    rng = np.random.default_rng(8)
    n, d, lists, nq, k = 300, 2048, 5, 4, 50
    rows, cents, queries = (rng.standard_normal(s).astype(F32) for s in ((n, d), (lists, d), (nq, d)))
    rows_t, q_t = dev(rows), dev(queries)
    index = ivf.IVFIndex(rows_t, dev(cents), dev(rng.integers(0, lists, n)))
    full = ops.DescriptorIndex(rows_t, "ND")
    try:
        want_ids, want_sc = ops.topk(full.scores(q_t, "ND"), k)
        res = index.search(q_t, k, lists)
        assert torch.equal(res.ids, want_ids) and torch.equal(res.scores.view(torch.int32), want_sc.view(torch.int32))
        assert host(res.scanned).tolist() == [n] * nq
    finally:
        index.close()
        full.close()


def test_ties_across_lists_leave_in_ascending_id():
    """Lattice data: every score is a small integer, and duplicate rows (row i repeats row i // 2) give equal scores.  All centroids
    are zero, so every query probes the lists in the order 0, 1, 2; the upper half of the rows sits in list 0: of two duplicates the
    larger id is in the list probed first, and has to leave after the smaller one all the same."""
    from mdir_amd import ivf, ops
    n, d, nq, k, lists = 200, 24, 5, 60, 3
    lat = lattice.common(n, d, nq, seed=2, amp=1)
    lattice.assert_exact_in_any_order(lat.qi, lat.xi)
    want = lattice.expected(lat.qi, lat.xi, 1.0)
    labels = np.where(np.arange(n) >= n // 2, 0, 1 + np.arange(n) % 2).astype(np.int64)
    # the premise, on the reference scores: inside the top k there are neighbours with equal scores, from different lists, the
    # later one (the larger id) from the list probed earlier
    ref_ids = np.lexsort((np.broadcast_to(np.arange(n), want.shape), KR.order_key(want)), axis=1)[:, :k]
    crossing = 0
    for q in range(nq):
        s, i = want[q, ref_ids[q]], ref_ids[q]
        tie = np.flatnonzero(s[1:] == s[:-1])
        crossing += int((labels[i[tie + 1]] < labels[i[tie]]).sum())
        assert (i[tie] < i[tie + 1]).all()
    assert crossing >= nq
    rows_t, q_t = dev(lat.db), dev(lat.queries)
    index = ivf.IVFIndex(rows_t, torch.zeros((lists, d), device=DEV), dev(labels))
    full = ops.DescriptorIndex(rows_t, "ND")
    try:
        scores = full.scores(q_t, "ND")
        IR.same_bits(host(scores), want)
        want_ids, want_sc = ops.topk(scores, k)
        np.testing.assert_array_equal(host(want_ids), ref_ids)
        res = index.search(q_t, k, lists)
        assert host(res.probes).tolist() == [[0, 1, 2]] * nq
        IR.same_bits(host(res.ids), host(want_ids))
        IR.same_bits(host(res.scores), host(want_sc))
    finally:
        index.close()
        full.close()


# ------------------------------------------------------------------------------------------------ the three calls through ops

def run_ops(rows_t, members, offsets, probes, q_t, k, cap, items, qlayout="ND", center=None):
    """plan -> scan -> select through the ops wrappers; everything on the host, the plan as its views."""
    from mdir_amd import ops
    members_t, offsets_t, probes_t = dev(members), dev(offsets), dev(probes)
    nq, nprobe = probes.shape
    lists = len(offsets) - 1
    plan = ops.ivf_plan(probes_t, offsets_t, len(members), cap)
    cand_scores, cand_ids = ops.ivf_scan(rows_t, members_t, offsets_t, q_t, plan, nprobe, cap, items, qlayout, center)
    ids, sc = ops.ivf_select(cand_scores, cand_ids, plan, nprobe, lists, k)
    views = {name: host(v) for name, v in ops.ivf_plan_views(plan, nq, nprobe, lists).items()}
    return views, host(cand_scores), host(cand_ids), host(ids), host(sc)


def check_ops(out, members, offsets, probes, scores, k, cap):
    """The outputs of run_ops against the restatement: the plan, every candidate column (NaN / -1 beyond the count), the answer."""
    views, cand_scores, cand_ids, ids, sc = out
    nq, nprobe = probes.shape
    lists = len(offsets) - 1
    base, count, entries, items = IR.plan(probes, offsets, len(members), cap)
    IR.same_bits(views["base"], base), IR.same_bits(views["count"], count)
    firsts = np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.int64)
    IR.same_bits(views["first"], firsts)
    assert views["item"][lists] == items and (np.diff(views["item"]) >= 0).all() and views["item"][0] == 0
    for l in range(lists):                                                 # inside a list the entries are in no particular order
        assert sorted(views["entry"][firsts[l]:firsts[l + 1]].tolist()) == entries[l], l
    cands = IR.candidates(members, offsets, probes, cap)
    for q in range(nq):
        c = len(cands[q])
        assert c == count[q]
        IR.same_bits(cand_ids[q, :c], cands[q])
        IR.same_bits(cand_scores[q, :c], IR.candidate_scores(scores[q], cands[q]))
        assert (cand_ids[q, c:] == -1).all() and np.isnan(cand_scores[q, c:]).all()
    want_ids, want_sc, _ = IR.search(members, offsets, probes, scores, k, cap)
    IR.same_bits(ids, want_ids), IR.same_bits(sc, want_sc)
    return items


def test_lists_shared_by_no_one_a_group_and_more_than_two_groups():
    rng = np.random.default_rng(3)
    nq, d = 2 * G + 1, 36
    sizes = [70, 65, 130, 64] + [3] * G
    lists, n = len(sizes), sum(sizes)
    rows, queries = rng.standard_normal((n, d)).astype(F32), rng.standard_normal((nq, d)).astype(F32)
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    # list 3: every query (2 G + 1 of them: three groups, the last of one); list 2: the first G queries (one full group);
    # list 1: query G alone; lists 4 ..: one query each; list 0: nobody
    second = [2] * G + [1] + list(range(4, 4 + G))
    probes = np.array([[3, second[q]] if q % 2 else [second[q], 3] for q in range(nq)], np.int64)
    shared = np.bincount(probes.reshape(-1), minlength=lists)
    assert shared[0] == 0 and shared[1] == 1 and shared[2] == G and shared[3] == 2 * G + 1
    cap = 130 + 70
    scores = exact_scores(rows, queries)
    items = IR.plan(probes, offsets, n, cap)[3]
    assert items == 1 * 3 + 3 * 1 + 2 * 1 + G                              # list 3, list 2 (130 rows: 3 tiles), list 1 (2 tiles), the small lists
    for launched in (items, items + 5):                                    # the exact number of work items, and a bound above it
        out = run_ops(dev(rows), members, offsets, probes, dev(queries), 25, cap, launched)
        assert check_ops(out, members, offsets, probes, scores, 25, cap) == items


def test_special_values_and_ids_and_probes_out_of_range():
    rng = np.random.default_rng(4)
    n, d, nq, lists = 150, 8, 4, 4
    rows = rng.integers(-3, 4, (n, d)).astype(F32)
    rows[5] = NAN
    rows[6, 0], rows[7, 0] = INF, -INF
    rows[8] = 0
    rows[9] = F32(-0.0)
    queries = rng.integers(1, 4, (nq, d)).astype(F32)                      # positive: +inf and -inf rows score +inf and -inf
    queries[3] = 0                                                         # every finite row scores 0 for this query
    scores = exact_scores(rows, queries)
    assert np.isnan(scores[:, 5]).all() and (scores[:3, 6] == INF).all() and (scores[:3, 7] == -INF).all() and np.isnan(scores[3, 6])
    assert not np.signbit(scores[:, 8:10]).any()                           # the chain starts from +0: a zero score is +0
    members, offsets = KR.csr(rng.integers(0, lists, n), lists)
    members = members.copy()
    members[[2, 40, 149]] = (-1, n, 1 << 40)                               # never dereferenced: NaN, the id as given
    probes = np.array([[0, 1, 2], [3, -1, 0], [lists, 2, 1], [1, 2, 3]], np.int64)
    cap = n
    out = run_ops(dev(rows), members, offsets, probes, dev(queries), 40, cap, 64)
    check_ops(out, members, offsets, probes, scores, 40, cap)
    assert out[0]["base"][1, 1] == -1 and out[0]["base"][2, 0] == -1 and (out[0]["count"] < cap).all()
    # offsets that leave [0, m] are clamped, a cap below the candidates cuts the row
    wild = offsets.copy()
    wild[0], wild[-1] = -9, n + 100
    out = run_ops(dev(rows), members, wild, probes, dev(queries), 7, 50, 64)
    check_ops(out, members, wild, probes, scores, 7, 50)
    assert (out[0]["count"] == 50).any()


@pytest.mark.parametrize("count", [4095, 4096, 4097, 9000])
def test_selection_at_the_switch_between_its_routes(count):
    """Up to 4096 candidates are sorted in LDS as they are; above that the radix select picks the k that are.  Scores with few
    distinct values (the key of position k is shared by many candidates: the second select, over the ids), -0 beside +0, NaN and both
    infinities; the same list probed twice makes equal pairs."""
    from mdir_amd import ops
    rng = np.random.default_rng(count)
    nq, lists = 3, 2
    offsets = np.array([0, count, count + 10], np.int64)
    probes = np.array([[0], [0], [1]], np.int64)
    plan = ops.ivf_plan(dev(probes), dev(offsets), count + 10, count)
    ids = np.stack([rng.permutation(count).astype(np.int64) * 3 - 5 for _ in range(nq)])
    sc = rng.integers(-2, 3, (nq, count)).astype(F32)
    sc[0] = rng.standard_normal(count).astype(F32)                         # query 0: distinct scores; query 1: five values and the specials
    sc[1][rng.random(count) < 0.2] = F32(-0.0)
    sc[1][rng.random(count) < 0.05] = NAN
    sc[1, :4] = (INF, -INF, INF, NAN)
    for k in (1, 100, 4096):
        got_ids, got_sc = ops.ivf_select(dev(sc), dev(ids), plan, 1, lists, k)
        for q, c in enumerate((count, count, 10)):
            want_ids, want_sc = IR.select(sc[q, :c], ids[q, :c], k)
            IR.same_bits(host(got_ids)[q], want_ids), IR.same_bits(host(got_sc)[q], want_sc)
    # one list probed twice: every pair twice
    twice = np.array([[0, 0]], np.int64)
    half = count // 2 + 1
    plan = ops.ivf_plan(dev(twice), dev(np.array([0, half, half], np.int64)), half, 2 * half)
    pair_ids = np.concatenate([ids[1, :half], ids[1, :half]])[None]
    pair_sc = np.concatenate([sc[1, :half], sc[1, :half]])[None]
    got_ids, got_sc = ops.ivf_select(dev(pair_sc), dev(pair_ids), plan, 2, lists, 101)
    want_ids, want_sc = IR.select(pair_sc[0], pair_ids[0], 101)
    IR.same_bits(host(got_ids)[0], want_ids), IR.same_bits(host(got_sc)[0], want_sc)


# ------------------------------------------------------------------------------------------------ planted clusters, train

def test_one_probe_finds_the_exact_top_ten_on_planted_clusters():
    from mdir_amd import cluster, ivf, ops
    lists, k = 8, 10
    rows, truth, centres, queries, _ = IR.planted(seed=7, lists=lists, per=40, d=64, nq=16, noise=0.05)
    assert np.array_equal(KR.assign64(centres, rows)[0], truth)             # the reference's labels are the planted ones
    rows_t, q_t, cents_t = dev(rows), dev(queries), dev(centres)
    index = ivf.IVFIndex(rows_t, cents_t)
    full = ops.DescriptorIndex(rows_t, "ND")
    try:
        IR.same_bits(host(index.labels), truth)
        IR.same_bits(host(index.labels), host(cluster.assign(cents_t, rows_t)[0]))
        exact = full.scores(q_t, "ND")
        want_ids, want_sc = ops.topk(exact, k)
        # the premise, on the exact scores: a query's top ten lie in the list of its nearest centroid, 0.66 (0.6564 in float64, on
        # the CPU) above the best row of any other list
        scores, nearest = host(exact), host(ops.topk(index.coarse.scores(q_t, "ND"), 1)[0])[:, 0]
        for q in range(len(queries)):
            assert (truth[host(want_ids)[q]] == nearest[q]).all()
            assert host(want_sc)[q, -1] - scores[q, truth != nearest[q]].max() > 0.65
        res = index.search(q_t, k, 1)
        assert torch.equal(res.ids, want_ids) and torch.equal(res.scores.view(torch.int32), want_sc.view(torch.int32))
        assert host(res.probes)[:, 0].tolist() == nearest.tolist() and host(res.scanned).tolist() == [40] * len(queries)
    finally:
        index.close()
        full.close()


def test_train_builds_the_index_of_the_fit():
    from mdir_amd import cluster, ivf
    lists = 8
    rows, truth, _, queries, _ = IR.planted()
    rows_t = dev(rows)
    index = ivf.IVFIndex.train(rows_t, lists, iters=5, seed=3)
    try:
        n = len(rows)
        assert index.fit is not None and index.centroids is index.fit.centroids and index.labels is index.fit.labels
        assert torch.equal(index.labels, cluster.assign(index.centroids, rows_t)[0])
        order, offsets, sizes = host(index.order), host(index.offsets), host(index.sizes)
        assert sorted(order.tolist()) == list(range(n)) and offsets[0] == 0 and offsets[-1] == n
        assert np.array_equal(np.diff(offsets), sizes) and index.host_sizes == sizes.tolist()
        labels = host(index.labels)
        for l in range(lists):
            mine = order[offsets[l]:offsets[l + 1]]
            assert (np.diff(mine) > 0).all() and (labels[mine] == l).all()
        scores = exact_scores(rows, queries)
        check_result(index.search(dev(queries), 10, 3), labels, lists, scores, 10)
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------ repeatability and capture

def test_two_runs_give_equal_bits():
    from mdir_amd import ivf
    rng = np.random.default_rng(6)
    rows, cents, queries = (rng.standard_normal(s).astype(F32) for s in ((sum(SIZES), 100), (len(SIZES), 100), (2 * G + 3, 100)))
    index = ivf.IVFIndex(dev(rows), dev(cents), dev(labels_of_sizes(rng, SIZES)))
    try:
        a = index.search(dev(queries), 30, 3)
        b = index.search(dev(queries), 30, 3)
        for x, y in zip(a, b):
            IR.same_bits(host(x), host(y))
    finally:
        index.close()


def test_three_calls_in_one_captured_graph():
    from mdir_amd import ops
    rng = np.random.default_rng(9)
    sizes = (40, 0, 130, 65)
    lists, n, d, nq, nprobe, k = len(sizes), sum(sizes), 36, 5, 2, 20
    cap, items = 195, 3 * nq + 3
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    data = [(rng.standard_normal((n, d)).astype(F32), rng.standard_normal((nq, d)).astype(F32),
             np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64)) for _ in range(2)]
    rows_t, q_t, probes_t = dev(data[0][0]), dev(data[0][1]), dev(data[0][2])
    members_t, offsets_t = dev(members), dev(offsets)

    def eager():
        plan = ops.ivf_plan(probes_t, offsets_t, n, cap)
        cand_scores, cand_ids = ops.ivf_scan(rows_t, members_t, offsets_t, q_t, plan, nprobe, cap, items)
        return (cand_scores, cand_ids) + ops.ivf_select(cand_scores, cand_ids, plan, nprobe, lists, k)
    eager()                                                                                    # eager once, before anything is recorded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                                                 # one stream, one chain of launches: no parallel branches
            outs_g = eager()
    torch.cuda.current_stream().wait_stream(side)
    for rows, queries, probes in (data[1], data[0]):                                           # new data, then the old again
        rows_t.copy_(dev(rows)), q_t.copy_(dev(queries)), probes_t.copy_(dev(probes))
        g.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in outs_g]
        for a, b in zip(got, eager()):
            IR.same_bits(a, host(b))
        want_ids, want_sc, _ = IR.search(members, offsets, probes, exact_scores(rows, queries), k, cap)
        IR.same_bits(got[2], want_ids), IR.same_bits(got[3], want_sc)
