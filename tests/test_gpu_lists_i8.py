"""The int8 lists of the inverted file on the device (include/mdx_lists_i8.h; mdir_amd/ivf.py, storage="i8"), bit for bit: the encoder
against ``ops.quantize_i8``, the bounds against an int8 index of the rows, the scan and the selection against the restatement
(tests/ivf_restatement.py) applied to the scores of that index, ``nprobe == K`` against ``ops.topk``, lists shared by 0, 1, a group and
more than two groups of queries, ties, the rescored shortlist and its certificate against the fp32 index on planted data, padding,
query chunks, run-to-run equality and the calls under graph capture."""
import numpy as np
import pytest
import torch

import ivf_restatement as IR
import kmeans_restatement as KR
import lattice
import lists_i8_restatement as LR
from test_gpu_ivf import SIZES, dev, host, labels_of_sizes, placed, placements

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
G = IR.QUERY_GROUP
DIMS = [1, 4, 63, 64, 65, 260]                      # one, two and five k-blocks of 64, with the padding of the last one


def i8_scores(rows, queries, qlayout="ND", center=None):
    """fp32 [nq, n]: the scores of an int8 index of the rows, the bits the int8 scan has to return."""
    from mdir_amd import ops
    index = ops.DescriptorIndex(dev(rows), "ND", storage="i8")
    try:
        return host(index.scores(dev(queries), qlayout, center=None if center is None else dev(center)))
    finally:
        index.close()


def same_fields(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            IR.same_bits(host(x), host(y))


# ------------------------------------------------------------------------------------------------ encode and bounds

@pytest.mark.parametrize("d", DIMS)
def test_encode_equals_quantize_i8_in_list_order(d):
    from mdir_amd import ops
    rng = np.random.default_rng(d)
    n = sum(SIZES)
    rows = rng.standard_normal((n, d)).astype(F32)
    rows[7] = 0                                                            # an all-zero row: scale 0, codes 0
    order = KR.csr(labels_of_sizes(rng, SIZES), len(SIZES))[0]
    spoiled = order.copy()
    spoiled[[3, n - 1]] = (-1, n)                                          # never dereferenced: zero codes, a NaN scale
    want_codes, want_scales = (host(t) for t in ops.quantize_i8(dev(rows)))
    d_pad = (d + 63) // 64 * 64
    for name, ld, off in placements(d):
        rows_t = placed(rows, ld, off)
        codes, scales = ops.lists_i8_encode(rows_t, dev(order))
        assert codes.shape == (n, d_pad) and codes.dtype == torch.int8 and scales.shape == (n,) and codes.data_ptr() % 16 == 0
        IR.same_bits(host(codes)[:, :d], want_codes[order]), IR.same_bits(host(scales), want_scales[order])
        assert not host(codes)[:, d:].any(), name
        at = int(np.flatnonzero(order == 7)[0])
        assert host(scales)[at] == 0 and not host(codes)[at].any()
        codes, scales = ops.lists_i8_encode(rows_t, dev(spoiled))
        keep = np.ones(n, bool)
        keep[[3, n - 1]] = False
        IR.same_bits(host(codes)[keep, :d], want_codes[order[keep]]), IR.same_bits(host(scales)[keep], want_scales[order[keep]])
        assert np.isnan(host(scales)[~keep]).all() and not host(codes)[~keep].any(), name
    IR.same_bits(want_codes, LR.quantize_np(rows)[0]), IR.same_bits(want_scales, LR.quantize_np(rows)[1])


@pytest.mark.parametrize("d", DIMS + [1100])
def test_bounds_equal_those_of_an_int8_index(d):
    from mdir_amd import ops
    rng = np.random.default_rng(d)
    n = 323
    rows = (rng.standard_normal((n, d)) * np.exp(rng.standard_normal((n, 1)))).astype(F32)     # scales that differ
    rows[5] = 0
    rows_t = dev(rows)
    order = dev(rng.permutation(n).astype(np.int64))
    index = ops.DescriptorIndex(rows_t, "ND", storage="i8")
    try:
        codes, scales = ops.lists_i8_encode(rows_t, order)
        got = ops.lists_i8_bounds(codes, scales, d)
        assert got.dtype == torch.float64 and got.shape == (4,)
        IR.same_bits(host(got), host(index.i8_bounds()))
        assert ops.unpack_i8_bounds(got)["flag"] == 0 and ops.unpack_i8_bounds(got)["s_min"] > 0
        scales[11] = float("nan")                                          # a non-finite scale sets the flag
        assert ops.unpack_i8_bounds(ops.lists_i8_bounds(codes, scales, d))["flag"] == 1
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------ scan + select against the restatement

def check_result(res, labels, lists, scores, k):
    """The int8 ranking of a search equals the restatement applied to the int8 score matrix, for the probes it reports."""
    ids, sc, scanned = IR.search_labels(labels, lists, host(res.probes), scores, k)
    IR.same_bits(host(res.scanned), scanned)
    IR.same_bits(host(res.ids), ids)
    IR.same_bits(host(res.scores), sc)
    assert res.certified is None and res.fallback.numel() == 0 and res.fallback.dtype == torch.int64
    return scanned


@pytest.mark.parametrize("d", DIMS)
def test_search_equals_the_restatement(d):
    from mdir_amd import ivf, ops
    rng = np.random.default_rng(d)
    lists, n = len(SIZES), sum(SIZES)
    rows = rng.standard_normal((n, d)).astype(F32)
    centroids = rng.standard_normal((lists, d)).astype(F32)
    center = rng.standard_normal(d).astype(F32)
    labels = labels_of_sizes(rng, SIZES)
    cents_t, labels_t = dev(centroids), dev(labels)
    indexes = [(name, ivf.IVFIndex(placed(rows, ld, off), cents_t, labels_t, storage="i8")) for name, ld, off in placements(d)]
    coarse = ops.DescriptorIndex(cents_t, "ND")
    full = ops.DescriptorIndex(dev(rows), "ND", storage="i8")
    for name, index in indexes:
        assert index.storage == "i8" and index.codes.shape == (n, (d + 63) // 64 * 64) and index.host_sizes == list(SIZES)
        IR.same_bits(host(index.bounds), host(full.i8_bounds()))
        same_fields((index.codes, index.scales), (indexes[0][1].codes, indexes[0][1].scales))
    turn = 0
    try:
        for nq in (1, 3, 9):
            queries = rng.standard_normal((nq, d)).astype(F32)
            for qlayout, with_center in (("ND", False), ("ND", True), ("DN", False), ("DN", True)):
                given = np.ascontiguousarray(queries.T) if qlayout == "DN" else queries
                c = center if with_center else None
                q_t, c_t = dev(given), None if c is None else dev(c)
                scores_t = full.scores(q_t, qlayout, center=c_t)
                scores = host(scores_t)
                for nprobe in (1, 2, lists):
                    want_probes = ops.topk(coarse.scores(q_t, qlayout, center=c_t), nprobe)[0]
                    name, index = indexes[turn % len(indexes)]                 # every placement meets every nq, layout and nprobe
                    turn += 1
                    first = index.search(q_t, 1, nprobe, qlayout, c_t)
                    assert isinstance(first, ivf.IVFRescored) and torch.equal(first.probes, want_probes), (name, nq, qlayout, nprobe)
                    scanned = check_result(first, labels, lists, scores, 1)
                    assert first.ids.shape == (nq, 1) and scanned.max() <= index.capacity(nprobe)
                    for k in sorted({7, int(scanned.max()) + 3, max(1, int(scanned.min()))}):
                        res = index.search(q_t, k, nprobe, qlayout, c_t)
                        check_result(res, labels, lists, scores, k)
                        if nprobe == lists and k <= n:                         # every row is a candidate: topk of the int8 scores
                            want_ids, want_sc = ops.topk(scores_t, k)
                            IR.same_bits(host(res.ids), host(want_ids)), IR.same_bits(host(res.scores), host(want_sc))
    finally:
        coarse.close()
        full.close()
        for _, index in indexes:
            index.close()
    assert turn == 36
    IR.same_bits(scores, LR.i8_scores(rows, queries, c))                        # the int8 index itself is the numpy restatement


# ------------------------------------------------------------------------------------------------ the calls through ops: groups, ties

def run_ops(rows, members, offsets, probes, queries, k, cap, items):
    """encode -> plan -> scan -> select through the ops wrappers; the candidate block and the answer on the host."""
    from mdir_amd import ops
    members_t, offsets_t = dev(members), dev(offsets)
    nprobe, lists = probes.shape[1], len(offsets) - 1
    codes, scales = ops.lists_i8_encode(dev(rows), members_t)
    qcodes, qscales = ops.quantize_i8(ops.center_rows(dev(queries)))
    plan = ops.ivf_plan(dev(probes), offsets_t, len(members), cap)
    cand_scores, cand_ids = ops.lists_i8_scan(codes, scales, rows.shape[1], members_t, offsets_t, qcodes, qscales, plan, nprobe, cap, items)
    ids, sc = ops.ivf_select(cand_scores, cand_ids, plan, nprobe, lists, k)
    return host(cand_scores), host(cand_ids), host(ids), host(sc)


def check_ops(out, members, offsets, probes, scores, k, cap):
    cand_scores, cand_ids, ids, sc = out
    cands = IR.candidates(members, offsets, probes, cap)
    for q, c in enumerate(cands):
        IR.same_bits(cand_ids[q, :len(c)], c)
        IR.same_bits(cand_scores[q, :len(c)], IR.candidate_scores(scores[q], c))
        assert (cand_ids[q, len(c):] == -1).all() and np.isnan(cand_scores[q, len(c):]).all()
    want_ids, want_sc, _ = IR.search(members, offsets, probes, scores, k, cap)
    IR.same_bits(ids, want_ids), IR.same_bits(sc, want_sc)


def test_lists_shared_by_no_one_one_query_a_group_and_more_than_two_groups():
    rng = np.random.default_rng(3)
    nq, d = 2 * G + 1, 100
    sizes = [70, 65, 130, 64] + [3] * G
    lists, n = len(sizes), sum(sizes)
    rows, queries = rng.standard_normal((n, d)).astype(F32), rng.standard_normal((nq, d)).astype(F32)
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    # list 3: every query (2 G + 1 = 17 of them: three groups, the last of one); list 2: the first G queries (exactly one full
    # group); list 1: query G alone; lists 4 ..: one query each; list 0: nobody
    second = [2] * G + [1] + list(range(4, 4 + G))
    probes = np.array([[3, second[q]] if q % 2 else [second[q], 3] for q in range(nq)], np.int64)
    shared = np.bincount(probes.reshape(-1), minlength=lists)
    assert shared[0] == 0 and shared[1] == 1 and shared[2] == G == 8 and shared[3] == 17
    cap = 130 + 70
    scores = i8_scores(rows, queries)
    items = IR.plan(probes, offsets, n, cap)[3]
    for launched in (items, items + 5):                                    # the exact number of work items, and a bound above it
        check_ops(run_ops(rows, members, offsets, probes, queries, 25, cap, launched), members, offsets, probes, scores, 25, cap)
    # member ids and probes out of range, offsets that leave [0, m], a cap below the candidates
    spoiled, wild = members.copy(), offsets.copy()
    spoiled[[2, 40, n - 1]] = (-1, n, 1 << 40)
    wild[0], wild[-1] = -9, n + 100
    probes[0, 0], probes[5, 1] = -1, lists
    check_ops(run_ops(rows, spoiled, wild, probes, queries, 9, 150, items + 5), spoiled, wild, probes, scores, 9, 150)


def test_ties_across_lists_leave_in_ascending_id():
    """Lattice data with duplicate rows (row i repeats row i // 2): equal rows have equal codes and scales, so equal int8 scores.  All
    centroids are zero, so every query probes the lists in the order 0, 1, 2; the upper half of the rows sits in list 0: of two
    duplicates the larger id is in the list probed first, and has to leave after the smaller one all the same."""
    from mdir_amd import ivf, ops
    n, d, nq, k, lists = 200, 24, 5, 60, 3
    lat = lattice.common(n, d, nq, seed=2, amp=1)
    labels = np.where(np.arange(n) >= n // 2, 0, 1 + np.arange(n) % 2).astype(np.int64)
    rows_t, q_t = dev(lat.db), dev(lat.queries)
    index = ivf.IVFIndex(rows_t, torch.zeros((lists, d), device=DEV), dev(labels), storage="i8")
    full = ops.DescriptorIndex(rows_t, "ND", storage="i8")
    try:
        scores = full.scores(q_t, "ND")
        want_ids, want_sc = ops.topk(scores, k)
        crossing = 0                                                       # the premise: ties inside the top k that cross lists
        for q in range(nq):
            s, i = host(want_sc)[q], host(want_ids)[q]
            tie = np.flatnonzero(s[1:] == s[:-1])
            crossing += int((labels[i[tie + 1]] < labels[i[tie]]).sum())
            assert (i[tie] < i[tie + 1]).all()
        assert crossing >= nq
        res = index.search(q_t, k, lists)
        assert host(res.probes).tolist() == [[0, 1, 2]] * nq
        IR.same_bits(host(res.ids), host(want_ids)), IR.same_bits(host(res.scores), host(want_sc))
    finally:
        index.close()
        full.close()


# ------------------------------------------------------------------------------------------------ rescoring and the certificate

@pytest.fixture(scope="module")
def planted():
    """The planted data (tests/test_lists_i8_host.py evaluates its certificate in numpy: depths 12, 9 and 11 for the planted
    queries), an int8 and an fp32 index of them, and the fp32 index's answers, computed once."""
    from mdir_amd import ivf
    rows, queries, labels, centroids = LR.planted()
    rows_t, cents_t, labels_t, q_t = dev(rows), dev(centroids), dev(labels), dev(queries)
    i8 = ivf.IVFIndex(rows_t, cents_t, labels_t, storage="i8")
    f32 = ivf.IVFIndex(rows_t, cents_t, labels_t)
    lists = len(centroids)
    world = {"rows": rows, "queries": queries, "labels": labels, "lists": lists, "q": q_t, "i8": i8, "f32": f32,
             "want": {(k, nprobe): f32.search(q_t, k, nprobe) for k in (5, 16) for nprobe in (2, lists)}}
    yield world
    i8.close()
    f32.close()


def check_prefix(res, want, k):
    """The soundness property: the entries before certified[q] are the fp32 index's, bits and ids."""
    certified = host(res.certified)
    same_fields((res.probes, res.scanned), (want.probes, want.scanned))
    for q, c in enumerate(np.minimum(certified, k)):
        IR.same_bits(host(res.ids)[q, :c], host(want.ids)[q, :c]), IR.same_bits(host(res.scores)[q, :c], host(want.scores)[q, :c])
    return certified


def test_planted_queries_are_certified_and_every_prefix_is_sound(planted):
    w = planted
    lists, S = w["lists"], 16
    for nprobe in (lists, 2):
        res = w["i8"].search(w["q"], 5, nprobe, shortlist=S)
        assert res.certified.dtype == torch.int64 and res.fallback.numel() == 0 and res.ids.shape == (len(w["queries"]), 5)
        certified = check_prefix(res, w["want"][5, nprobe], 5)
        _, _, scanned, restated = LR.search(w["labels"], lists, host(res.probes), w["rows"], w["queries"], 5, S)
        IR.same_bits(host(res.scanned), scanned)
        assert (certified <= restated).all(), (certified, restated)         # the device rounds U_q up, the restatement does not
        print("nprobe %d: certified %s, restated in float64 %s" % (nprobe, certified.tolist(), restated.tolist()))
        if nprobe == lists:
            assert (host(res.scanned) == 323).all() and restated[:3].tolist() == [12, 9, 11]
            assert (certified[:3] >= 5).all(), certified
            same_fields((res.ids[:3], res.scores[:3]), (w["want"][5, nprobe].ids[:3], w["want"][5, nprobe].scores[:3]))


def test_a_shortlist_of_k_falls_back_for_every_query_and_exact_gives_the_fp32_result(planted):
    w = planted
    lists, S, nq = w["lists"], 16, len(w["queries"])
    for nprobe in (lists, 2):
        want = w["want"][16, nprobe]
        assert (host(want.scanned) > S).all()
        res = w["i8"].search(w["q"], S, nprobe, shortlist=S)
        certified = check_prefix(res, want, S)
        assert (certified < S).all(), certified             # the entry whose int8 score is t_q has a chain score <= U_q
        sure = w["i8"].search(w["q"], S, nprobe, shortlist=S, exact=True)
        assert host(sure.fallback).tolist() == list(range(nq)) and sure.fallback.dtype == torch.int64
        same_fields(sure[:4], want)
        IR.same_bits(host(sure.certified), certified)


def test_exact_leaves_the_certified_queries_out_of_the_fallback(planted):
    w = planted
    lists, S = w["lists"], 16
    for k, nprobe in ((5, lists), (5, 2), (10, lists)):
        res = w["i8"].search(w["q"], k, nprobe, shortlist=S)
        sure = w["i8"].search(w["q"], k, nprobe, shortlist=S, exact=True)
        certified = host(res.certified)
        assert host(sure.fallback).tolist() == np.flatnonzero(certified < k).tolist()
        if nprobe == lists:
            assert not set(host(sure.fallback).tolist()) & ({0, 1, 2} if k == 5 else {0, 2})
        if k == 10:                                                        # depths of 12, 9, 11, ... in float64: some run again, some do not
            assert 0 < sure.fallback.numel() < len(w["queries"]) and 1 in host(sure.fallback).tolist()
        same_fields(sure[:4], w["want"][k, nprobe] if k == 5 else w["f32"].search(w["q"], k, nprobe))
        IR.same_bits(host(sure.certified), certified)
        kept = certified >= k                                              # not run again: the rescored rows as they were
        same_fields((sure.ids[dev(kept)], sure.scores[dev(kept)]), (res.ids[dev(kept)], res.scores[dev(kept)]))


# ------------------------------------------------------------------------------------------------ padding, chunks, repeatability, capture

def small_world(seed, d=20, nq=9):
    from mdir_amd import ivf
    rng = np.random.default_rng(seed)
    rows, cents, queries = (rng.standard_normal(s).astype(F32) for s in ((sum(SIZES), d), (len(SIZES), d), (nq, d)))
    labels = labels_of_sizes(rng, SIZES)
    args = (dev(rows), dev(cents), dev(labels))
    return ivf.IVFIndex(*args, storage="i8"), ivf.IVFIndex(*args), queries


def test_fewer_candidates_than_the_shortlist_give_padding_and_the_whole_fp32_row():
    from mdir_amd import ivf
    rng = np.random.default_rng(12)
    lists, n, d = len(SIZES), sum(SIZES), 20
    rows = rng.standard_normal((n, d)).astype(F32)
    cents = rng.standard_normal((lists, d))
    cents = (cents / np.linalg.norm(cents, axis=1, keepdims=True)).astype(F32)
    # query q lies on centroid q % lists: with one probe it scans list q % lists, whatever rows that list holds
    queries = (4 * cents[np.arange(2 * lists) % lists] + 0.3 * rng.standard_normal((2 * lists, d))).astype(F32)
    args = (dev(rows), dev(cents), dev(labels_of_sizes(rng, SIZES)))
    i8, f32 = ivf.IVFIndex(*args, storage="i8"), ivf.IVFIndex(*args)
    try:
        k, S = 70, 100                                                     # lists of 0, 1, 63, 64 and 65 rows lie under both, 130 over S
        res = i8.search(dev(queries), k, 1, shortlist=S)
        want = f32.search(dev(queries), k, 1)
        scanned, certified = host(res.scanned), host(res.certified)
        assert host(res.probes)[:, 0].tolist() == (np.arange(2 * lists) % lists).tolist() and scanned.tolist() == list(SIZES) * 2
        assert (certified[scanned <= S] == S).all() and (certified[scanned > S] < S).all()
        short = scanned <= S
        same_fields((res.ids[dev(short)], res.scores[dev(short)]), (want.ids[dev(short)], want.scores[dev(short)]))
        assert (host(res.ids)[scanned < k, -1] == -1).all() and np.isnan(host(res.scores)[scanned < k, -1]).all()
        check_prefix(res, want, k)
        # a shortlist beyond the rows: everybody is padded
        res = i8.search(dev(queries), k, len(SIZES), shortlist=400)
        assert (host(res.certified) == 400).all()
        same_fields(res[:4], f32.search(dev(queries), k, len(SIZES)))
    finally:
        i8.close()
        f32.close()


def test_query_chunks_change_no_bit(monkeypatch):
    from mdir_amd import ivf
    i8, f32, queries = small_world(5)
    f32.close()
    try:
        for qlayout, q in (("ND", queries), ("DN", np.ascontiguousarray(queries.T))):
            # k = 40 = the shortlist: no query with more candidates than that is certified to depth k, so every one runs again
            for k, kw in ((12, {}), (12, {"shortlist": 40}), (40, {"shortlist": 40, "exact": True})):
                whole = i8.search(dev(q), k, 3, qlayout, **kw)
                per_query = 12 * i8.capacity(3) + 5 * i8.d + 4 + (28 * 40 + 8 if kw else 0)
                monkeypatch.setattr(ivf, "CANDIDATE_MEMORY_CAP", per_query * 4)                 # four queries per step
                assert i8.query_chunk(3, kw.get("shortlist")) == 4
                parts = i8.search(dev(q), k, 3, qlayout, **kw)
                monkeypatch.undo()
                same_fields(whole, parts)
                assert whole.fallback.numel() == (len(queries) if kw.get("exact") else 0)
    finally:
        i8.close()


def test_two_runs_give_equal_bits():
    i8, f32, queries = small_world(6, d=100, nq=2 * G + 3)
    f32.close()
    try:
        for k, kw in ((30, {}), (30, {"shortlist": 50}), (50, {"shortlist": 50, "exact": True})):
            same_fields(i8.search(dev(queries), k, 3, **kw), i8.search(dev(queries), k, 3, **kw))
    finally:
        i8.close()


def test_plan_scan_and_select_in_one_captured_graph():
    from mdir_amd import ops
    rng = np.random.default_rng(9)
    sizes = (40, 0, 130, 65)
    lists, n, d, nq, nprobe, k = len(sizes), sum(sizes), 100, 5, 2, 20
    cap, items = 195, 3 * nq + 3
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    data = [(rng.standard_normal((n, d)).astype(F32), rng.standard_normal((nq, d)).astype(F32),
             np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64)) for _ in range(2)]
    members_t, offsets_t = dev(members), dev(offsets)
    probes_t = dev(data[0][2])
    codes, scales = ops.lists_i8_encode(dev(data[0][0]), members_t)
    qcodes, qscales = ops.quantize_i8(dev(data[0][1]))

    def eager():
        plan = ops.ivf_plan(probes_t, offsets_t, n, cap)
        cand_scores, cand_ids = ops.lists_i8_scan(codes, scales, d, members_t, offsets_t, qcodes, qscales, plan, nprobe, cap, items)
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
        new_codes, new_scales = ops.lists_i8_encode(dev(rows), members_t)
        new_q = ops.quantize_i8(dev(queries))
        codes.copy_(new_codes), scales.copy_(new_scales), qcodes.copy_(new_q[0]), qscales.copy_(new_q[1]), probes_t.copy_(dev(probes))
        g.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in outs_g]
        for a, b in zip(got, eager()):
            IR.same_bits(a, host(b))
        want_ids, want_sc, _ = IR.search(members, offsets, probes, i8_scores(rows, queries), k, cap)
        IR.same_bits(got[2], want_ids), IR.same_bits(got[3], want_sc)
