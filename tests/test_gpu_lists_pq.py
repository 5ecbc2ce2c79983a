"""The product-quantised lists of the inverted file on the device (include/mdx_lists_pq.h; mdir_amd/pq.py, mdir_amd/ivfpq.py), bit for
bit: the table against the per-subspace fp32 indexes of the codewords, the codes and the search against the restatement
(tests/pq_restatement.py), lists shared by 0, 1 and more than 8 queries, a zero-error lattice on which the ADC ranking is the fp32
index's, the rescored shortlist against the fp32 index, the training loop against the restatement, query chunks, graph capture and
what the index holds."""
import gc
import weakref

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import kmeans_restatement as KR
import lattice
import pq_restatement as PR
from test_gpu_ivf import dev, exact_scores, host, labels_of_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SIZES = (0, 1, 63, 64, 65, 200)                     # empty, one row, around a wave of 64 lanes, three waves and a bit


def same_fields(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        IR.same_bits(host(x), host(y))


# ------------------------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("d,m_sub", [(8, 2), (12, 3), (60, 4), (64, 16), (256, 128), (2048, 64)])
def test_table_equals_the_scores_of_an_index_of_every_subspace(d, m_sub):
    from mdir_amd import ops
    rng = np.random.default_rng(d + m_sub)
    dsub = d // m_sub
    words = rng.standard_normal((m_sub, 256, dsub)).astype(F32)
    words[:, 5] = 0                                                        # chains that end on a zero, of either sign
    words_t = dev(words)
    center = rng.standard_normal(d).astype(F32)
    indexes = [ops.DescriptorIndex(words_t[m], "ND") for m in range(m_sub)]
    try:
        for nq in (1, 9, 70):
            queries = rng.standard_normal((nq, d)).astype(F32)
            queries[0, ::2] = -queries[0, ::2] * 0                         # -0 and +0 elements: products of -0
            for qlayout in ("ND", "DN"):
                given = dev(np.ascontiguousarray(queries.T) if qlayout == "DN" else queries)
                for c in (None, center):
                    got = ops.pq_lut(words_t, given, qlayout, None if c is None else dev(c))
                    assert got.shape == (nq, m_sub, 256) and got.dtype == torch.float32
                    for m in range(m_sub):
                        sub = dev(queries[:, m * dsub:(m + 1) * dsub])
                        want = indexes[m].scores(sub, "ND", center=None if c is None else dev(c[m * dsub:(m + 1) * dsub]))
                        IR.same_bits(host(got[:, m]), host(want))
            if d <= 256:
                IR.same_bits(host(got), PR.lut(words, queries, center))    # the restatement states the same table
    finally:
        for index in indexes:
            index.close()


# ------------------------------------------------------------------------------------------------ codes and search

def world(rng, d, m_sub, sizes=SIZES):
    lists, n = len(sizes), sum(sizes)
    rows = rng.standard_normal((n, d)).astype(F32)
    cents = rng.standard_normal((lists, d)).astype(F32)
    words = (F32(0.7) * rng.standard_normal((m_sub, 256, d // m_sub))).astype(F32)
    labels = labels_of_sizes(rng, sizes)
    return rows, cents, words, labels


def restated_search(words, codes, members, n, offsets, probes, coarse, queries, center, k):
    return PR.search(codes, members, n, offsets, PR.lut(words, queries, center), coarse, probes, k)


@pytest.mark.parametrize("d,m_sub", [(12, 3), (60, 4), (64, 16), (256, 128)])
def test_codes_and_search_equal_the_restatement(d, m_sub):
    from mdir_amd import ivfpq, ops
    rng = np.random.default_rng(d)
    rows, cents, words, labels = world(rng, d, m_sub)
    lists, n = len(SIZES), len(rows)
    center = rng.standard_normal(d).astype(F32)
    cents_t = dev(cents)
    index = ivfpq.IVFPQIndex(dev(rows), cents_t, dev(labels), m=m_sub, codebook=dev(words))
    coarse_index = ops.DescriptorIndex(cents_t, "ND")
    try:
        members, offsets = KR.csr(labels, lists)
        IR.same_bits(host(index.order), members), IR.same_bits(host(index.offsets), offsets)
        codes = PR.encode(words, rows[members] - cents[labels[members]])
        assert index.codes.dtype == torch.uint8 and index.codes.shape == (n, m_sub) and index.host_sizes == list(SIZES)
        IR.same_bits(host(index.codes), codes)
        IR.same_bits(host(index.codes), host(ivfpq._pq.encode(index.codebook, dev(rows[members] - cents[labels[members]]), chunk=37)))
        for nq in (1, 9):
            queries = rng.standard_normal((nq, d)).astype(F32)
            for qlayout, c in (("ND", None), ("DN", center)):
                q_t = dev(np.ascontiguousarray(queries.T) if qlayout == "DN" else queries)
                c_t = None if c is None else dev(c)
                for nprobe in (1, 3, lists):
                    want_probes, coarse = ops.topk(coarse_index.scores(q_t, qlayout, center=c_t), nprobe)
                    scanned_max = 0
                    for k in (7, 400):                                      # 400 is more than any query scans: padding
                        res = index.search(q_t, k, nprobe, qlayout, c_t)
                        assert isinstance(res, ivfpq.IVFPQResult) and torch.equal(res.probes, want_probes)
                        ids, sc, scanned = restated_search(words, codes, members, n, offsets, host(want_probes), host(coarse), queries, c, k)
                        IR.same_bits(host(res.scanned), scanned), IR.same_bits(host(res.ids), ids), IR.same_bits(host(res.scores), sc)
                        scanned_max = int(scanned.max())
                    assert scanned_max <= index.capacity(nprobe) < 400 and (host(res.ids)[:, -1] == -1).all()
    finally:
        index.close()
        coarse_index.close()


def test_lists_shared_by_no_one_one_query_and_more_than_eight():
    """Through the ops wrappers, with probes of the test's own: list 3 is probed by all 17 queries, list 2 by eight, list 1 by one, list
    0 by nobody; then member ids and probes out of range, offsets that leave [0, m] and a cap below the candidates."""
    from mdir_amd import ops
    rng = np.random.default_rng(3)
    nq, m_sub = 17, 8
    sizes = [70, 65, 200, 64] + [3] * 8
    lists, n = len(sizes), sum(sizes)
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    second = [2] * 8 + [1] + list(range(4, 12))
    probes = np.array([[3, second[q]] if q % 2 else [second[q], 3] for q in range(nq)], np.int64)
    shared = np.bincount(probes.reshape(-1), minlength=lists)
    assert shared[0] == 0 and shared[1] == 1 and shared[2] == 8 and shared[3] == 17
    codes = rng.integers(0, 256, (n, m_sub)).astype(np.uint8)
    table = rng.standard_normal((nq, m_sub, 256)).astype(F32)
    coarse = rng.standard_normal((nq, 2)).astype(F32)

    def run(members, offsets, probes, cap, k):
        members_t, offsets_t, probes_t = dev(members), dev(offsets), dev(probes)
        plan = ops.ivf_plan(probes_t, offsets_t, n, cap)
        cand_scores, cand_ids = ops.lists_pq_scan(dev(codes), members_t, n, offsets_t, dev(table), dev(coarse), probes_t, plan, cap)
        ids, sc = ops.ivf_select(cand_scores, cand_ids, plan, 2, lists, k)
        for q, (want_ids, want_sc) in enumerate(PR.scan(codes, members, n, offsets, table, coarse, probes, cap)):
            IR.same_bits(host(cand_ids)[q, :len(want_ids)], want_ids), IR.same_bits(host(cand_scores)[q, :len(want_ids)], want_sc)
            assert (host(cand_ids)[q, len(want_ids):] == -1).all() and np.isnan(host(cand_scores)[q, len(want_ids):]).all()
        want = PR.search(codes, members, n, offsets, table, coarse, probes, k, cap)
        IR.same_bits(host(ids), want[0]), IR.same_bits(host(sc), want[1])
    run(members, offsets, probes, 270, 25)
    spoiled, wild = members.copy(), offsets.copy()
    spoiled[[2, 40, n - 1]] = (-1, n, 1 << 40)
    wild[0], wild[-1] = -9, n + 100
    probes[0, 0], probes[5, 1] = -1, lists
    run(spoiled, wild, probes, 150, 9)
    # a strided view of the codes: the row stride reaches the kernel
    wide = torch.zeros((n, 12), dtype=torch.uint8, device=DEV)
    wide[:, :m_sub] = dev(codes)
    members_t, offsets_t, probes_t = dev(members), dev(offsets), dev(probes)
    plan = ops.ivf_plan(probes_t, offsets_t, n, 270)
    same_fields(ops.lists_pq_scan(wide[:, :m_sub], members_t, n, offsets_t, dev(table), dev(coarse), probes_t, plan, 270),
                ops.lists_pq_scan(dev(codes), members_t, n, offsets_t, dev(table), dev(coarse), probes_t, plan, 270))


# ------------------------------------------------------------------------------------------------ the zero-error lattice

def test_on_a_lattice_the_adc_ranking_is_the_fp32_index_s():
    """Integer centroids, codewords and queries in [-3, 3]; a row is its centroid plus one codeword per subspace.  Every product and
    every sum is a small integer, exact in fp32 in any order (lattice.assert_exact_in_any_order), the residual of a row is its
    codewords exactly, so its code decodes to it and the ADC score is the integer dot product: the ranking of IVFIndex on the same
    partition, bit for bit.  Codes from a handful of values make many equal rows in different lists: ties leave by ascending id."""
    from mdir_amd import ivf, ivfpq
    rng = np.random.default_rng(11)
    n, d, m_sub, lists, nq, k = 300, 16, 4, 5, 6, 80
    dsub = d // m_sub
    words = rng.integers(-3, 4, (m_sub, 256, dsub)).astype(F32)
    cents = rng.integers(-3, 4, (lists, d)).astype(F32)
    cents[1] = cents[0]                                                    # two lists around one centroid: equal rows across lists
    labels = rng.integers(0, lists, n).astype(np.int64)
    picks = rng.integers(0, 3, (n, m_sub))
    rows = cents[labels] + np.concatenate([words[m][picks[:, m]] for m in range(m_sub)], axis=1)
    queries = rng.integers(-3, 4, (nq, d)).astype(F32)
    lattice.assert_exact_in_any_order(queries, rows), lattice.assert_exact_in_any_order(queries, np.abs(cents) + 3)
    rows_t, cents_t, labels_t, q_t = dev(rows), dev(cents), dev(labels), dev(queries)
    pq_index = ivfpq.IVFPQIndex(rows_t, cents_t, labels_t, m=m_sub, codebook=dev(words))
    f32 = ivf.IVFIndex(rows_t, cents_t, labels_t)
    try:
        IR.same_bits(host(ivfpq._pq.decode(pq_index.codebook, pq_index.codes)), (rows - cents[labels])[host(pq_index.order)])
        ties = 0
        for nprobe in (2, lists):
            res, want = pq_index.search(q_t, k, nprobe), f32.search(q_t, k, nprobe)
            same_fields(res, want)
            exact = (queries.astype(np.int64) @ rows.astype(np.int64).T).astype(F32)
            ids, sc = host(res.ids), host(res.scores)
            for q in range(nq):
                IR.same_bits(sc[q][ids[q] >= 0], exact[q, ids[q][ids[q] >= 0]])
                tie = np.flatnonzero(sc[q][1:] == sc[q][:-1])
                assert (ids[q][tie] < ids[q][tie + 1]).all()
                ties += int((labels[ids[q][tie]] != labels[ids[q][tie + 1]]).sum())
        assert ties > nq                                                   # the premise: ties inside the top k that cross lists
    finally:
        pq_index.close()
        f32.close()


# ------------------------------------------------------------------------------------------------ the shortlist

def test_a_shortlist_returns_the_exact_chain_and_the_whole_fp32_row_where_it_covers_the_candidates():
    from mdir_amd import ivf, ivfpq
    rng = np.random.default_rng(12)
    d, m_sub = 20, 5
    rows, cents, words, labels = world(rng, d, m_sub)
    lists, n = len(SIZES), len(rows)
    cents = (cents / np.linalg.norm(cents, axis=1, keepdims=True)).astype(F32)
    # query q lies on centroid q % lists: with one probe it scans list q % lists, whatever rows that list holds
    queries = (4 * cents[np.arange(2 * lists) % lists] + 0.3 * rng.standard_normal((2 * lists, d))).astype(F32)
    args = (dev(rows), dev(cents), dev(labels))
    index, f32 = ivfpq.IVFPQIndex(*args, m=m_sub, codebook=dev(words)), ivf.IVFIndex(*args)
    try:
        exact = exact_scores(rows, queries)
        k, S = 70, 100                                                     # lists of 0, 1, 63, 64 and 65 rows lie under both, 200 over S
        for nprobe in (1, 2):
            res, want = index.search(dev(queries), k, nprobe, shortlist=S), f32.search(dev(queries), k, nprobe)
            adc = index.search(dev(queries), S, nprobe)
            same_fields((res.probes, res.scanned), (want.probes, want.scanned))
            ids, sc, scanned = host(res.ids), host(res.scores), host(res.scanned)
            if nprobe == 1:
                assert host(res.probes)[:, 0].tolist() == (np.arange(2 * lists) % lists).tolist() and scanned.tolist() == list(SIZES) * 2
            assert (scanned <= S).any() and (scanned > S).any()
            for q in range(len(queries)):
                have = ids[q] >= 0
                IR.same_bits(sc[q][have], exact[q, ids[q][have]])          # every returned score is the fp32 index's at that id
                assert have.sum() == min(k, scanned[q]) and np.isnan(sc[q][~have]).all()
                assert set(ids[q][have].tolist()) <= set(host(adc.ids)[q].tolist())               # taken from the ADC shortlist
                order = np.lexsort((ids[q][have], KR.order_key(sc[q][have])))
                assert (order == np.arange(have.sum())).all()              # sorted by (key, id)
                if scanned[q] <= S:
                    IR.same_bits(ids[q], host(want.ids)[q]), IR.same_bits(sc[q], host(want.scores)[q])
        # a shortlist beyond the rows: everybody is padded, the whole result is the fp32 index's
        same_fields(index.search(dev(queries), k, lists, shortlist=500), f32.search(dev(queries), k, lists))
    finally:
        index.close()
        f32.close()


# ------------------------------------------------------------------------------------------------ training

def training_data(d, seed=1, t=2048, m_sub=4, centres=40):
    """Clustered vectors (so that an iteration has something to learn), with a duplicate among the rows the seed draws as initial
    codewords: codeword 9 starts equal to codeword 2, wins nothing and has to keep its value."""
    rng = np.random.default_rng(d)
    vectors = (rng.standard_normal((centres, d))[rng.integers(0, centres, t)] + 0.3 * rng.standard_normal((t, d))).astype(F32)
    _, first = PR.draw(t, seed)
    vectors[first[9]] = vectors[first[2]]
    return vectors, first


@pytest.mark.parametrize("d", [16, 60])
def test_train_encode_and_decode_equal_the_restatement(d):
    """dsub = 4: every sub-vector starts on the 16-byte grid; dsub = 15: none but the first does (the dword path of mdx_kmeans_sums)."""
    from mdir_amd import pq
    m_sub, seed = 4, 1
    vectors, first = training_data(d, seed)
    vectors_t = dev(vectors)
    book = pq.train(vectors_t, m_sub, iters=3, seed=seed)
    words, history, updates = PR.train(vectors, m_sub, iters=3, seed=seed)
    assert book.iterations == updates == 3 and len(book.history) == len(history) == 4 * m_sub
    assert book.codewords.shape == (m_sub, 256, d // m_sub) and book.codewords.is_contiguous()
    IR.same_bits(host(book.codewords), words)
    np.testing.assert_allclose(book.history, history, rtol=1e-9, atol=1e-6)  # float64 sums of the same fp32 values, in another order
    again = pq.train(vectors_t, m_sub, iters=3, seed=seed, chunk=500)       # two runs, and another chunk: equal bits
    IR.same_bits(host(again.codewords), words)
    codes = pq.encode(book, vectors_t)
    IR.same_bits(host(codes), PR.encode(words, vectors))
    IR.same_bits(host(pq.encode(book, vectors_t, chunk=333)), host(codes))
    IR.same_bits(host(pq.decode(book, codes)), PR.decode(words, host(codes)))
    # after one update the emptied codeword has kept its value; its twin, which won the members of both, has moved
    initial = vectors[first].reshape(256, m_sub, d // m_sub).transpose(1, 0, 2)
    once = host(pq.train(vectors_t, m_sub, iters=1, seed=seed).codewords)
    IR.same_bits(once[:, 9], np.ascontiguousarray(initial[:, 9]))
    assert not np.array_equal(once[:, 2], initial[:, 2])
    # zero updates return the sampled codebook; training lowers the reconstruction error on the same data
    start = pq.train(vectors_t, m_sub, iters=0, seed=seed)
    assert start.iterations == 0 and len(start.history) == m_sub
    IR.same_bits(host(start.codewords), np.ascontiguousarray(initial))
    mse = lambda b: float(((vectors_t - pq.decode(b, pq.encode(b, vectors_t))).double() ** 2).sum(1).mean())
    assert mse(book) < mse(start), (mse(book), mse(start))
    # a training sample
    sampled = pq.train(vectors_t, m_sub, iters=2, seed=seed, train_rows=1024)
    IR.same_bits(host(sampled.codewords), PR.train(vectors, m_sub, iters=2, seed=seed, train_rows=1024)[0])


# ------------------------------------------------------------------------------------------------ chunks, capture, size

def small_index(seed, d=20, m_sub=5, nq=9, keep_rows=True):
    from mdir_amd import ivfpq
    rng = np.random.default_rng(seed)
    rows, cents, words, labels = world(rng, d, m_sub)
    queries = rng.standard_normal((nq, d)).astype(F32)
    return ivfpq.IVFPQIndex(dev(rows), dev(cents), dev(labels), m=m_sub, codebook=dev(words), keep_rows=keep_rows), queries


def test_query_chunks_change_no_bit(monkeypatch):
    from mdir_amd import ivf
    index, queries = small_index(5)
    try:
        for qlayout, q in (("ND", queries), ("DN", np.ascontiguousarray(queries.T))):
            for k, kw in ((12, {}), (12, {"shortlist": 40})):
                whole = index.search(dev(q), k, 3, qlayout, **kw)
                per_query = 12 * index.capacity(3) + 1024 * index.m + (28 * 40 if kw else 0)
                monkeypatch.setattr(ivf, "CANDIDATE_MEMORY_CAP", per_query * 4)                 # four queries per step
                assert index.query_chunk(3, kw.get("shortlist")) == 4
                parts = index.search(dev(q), k, 3, qlayout, **kw)
                monkeypatch.undo()
                same_fields(whole, parts)
                same_fields(whole, index.search(dev(q), k, 3, qlayout, **kw))                   # and two runs give equal bits
    finally:
        index.close()


def test_table_plan_scan_and_select_in_one_captured_graph():
    from mdir_amd import ops
    rng = np.random.default_rng(9)
    sizes = (40, 0, 200, 65)
    lists, n, d, m_sub, nq, nprobe, k, cap = len(sizes), sum(sizes), 24, 6, 5, 2, 20, 265
    members, offsets = KR.csr(labels_of_sizes(rng, sizes), lists)
    words = rng.standard_normal((m_sub, 256, d // m_sub)).astype(F32)
    data = [(rng.integers(0, 256, (n, m_sub)).astype(np.uint8), rng.standard_normal((nq, d)).astype(F32),
             np.stack([rng.permutation(lists)[:nprobe] for _ in range(nq)]).astype(np.int64),
             rng.standard_normal((nq, nprobe)).astype(F32)) for _ in range(2)]
    members_t, offsets_t, words_t = dev(members), dev(offsets), dev(words)
    codes_t, q_t, probes_t, coarse_t = (dev(a) for a in data[0])

    def eager():
        lut = ops.pq_lut(words_t, q_t)
        plan = ops.ivf_plan(probes_t, offsets_t, n, cap)
        cand_scores, cand_ids = ops.lists_pq_scan(codes_t, members_t, n, offsets_t, lut, coarse_t, probes_t, plan, cap)
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
    for codes, queries, probes, coarse in (data[1], data[0]):                                  # new data, then the old again
        codes_t.copy_(dev(codes)), q_t.copy_(dev(queries)), probes_t.copy_(dev(probes)), coarse_t.copy_(dev(coarse))
        g.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in outs_g]
        for a, b in zip(got, eager()):
            IR.same_bits(a, host(b))
        want_ids, want_sc, _ = PR.search(codes, members, n, offsets, PR.lut(words, queries), coarse, probes, k, cap)
        IR.same_bits(got[2], want_ids), IR.same_bits(got[3], want_sc)


def test_without_the_rows_the_index_holds_m_plus_eight_bytes_a_row():
    from mdir_amd import ivfpq
    rng = np.random.default_rng(21)
    d, m_sub = 64, 16
    rows, cents, words, labels = world(rng, d, m_sub)
    n, lists = len(rows), len(cents)
    rows_t, cents_t, labels_t, words_t = dev(rows), dev(cents), dev(labels), dev(words)
    kept = ivfpq.IVFPQIndex(rows_t, cents_t, labels_t, m=m_sub, codebook=words_t)
    bare = ivfpq.IVFPQIndex(rows_t, cents_t, labels_t, m=m_sub, codebook=words_t, keep_rows=False)
    try:
        # no padding of the codes (include/mdx_lists_pq.h: ldc = M): M bytes of code and 8 of id a row
        assert bare.nbytes() <= n * (m_sub + 8) + words_t.numel() * 4 + cents_t.numel() * 4 + bare.coarse.device_bytes
        assert bare.nbytes() >= n * (m_sub + 8) and kept.nbytes() == bare.nbytes() + rows_t.numel() * 4
        assert bare.rows is None and kept.rows is rows_t and bare.codes.shape == (n, m_sub)
        queries = dev(rng.standard_normal((7, d)).astype(F32))
        same_fields(bare.search(queries, 30, 3), kept.search(queries, 30, 3))
        with pytest.raises(ValueError, match="keep_rows=False"):
            bare.search(queries, 30, 3, shortlist=40)
        kept.close()
        ref = weakref.ref(rows_t)
        del rows_t, kept
        gc.collect()
        assert ref() is None                                               # nobody holds the rows any more
        assert bare.search(queries, 30, 3).ids.shape == (7, 30)
    finally:
        bare.close()
