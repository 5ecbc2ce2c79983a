"""Adding and removing rows of an IVF-PQ index after the build, and saving it (include/mdx_lists_edit.h; IVFPQIndex.add, .remove,
.attach_rows, .state and .from_state of mdir_amd/ivfpq.py), bit for bit: a streamed build against the one-shot constructor, removals
against the restatement (tests/lists_edit_restatement.py) and the searches on both against tests/pq_restatement.py, rows that leave and
come back, the exact second stage on attached rows, the state through torch.save, and an add that fails."""
import functools
import io

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import lists_edit_restatement as LR
import pq_restatement as PR
from test_gpu_ivf import host
from test_gpu_lists_pq import same_fields

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
LISTS, EMPTY, LATE = 7, 5, 6                        # list 5 stays empty; list 6 holds the last three rows only
N = 700
SHAPES = [(12, 3), (64, 16), (256, 128)]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def world(d, m_sub):
    """(rows [N, d], centroids [7, d], codewords, labels, queries) on the host, one fixed draw per shape, shared and never written.
    Centroid 5 repeats centroid 0 (the smaller id wins every tie: nobody is assigned to it) and centroid 6 is 100 e_0, which only the
    last three rows do not point away from -- with the explicit labels and with ``cluster.assign`` alike list 5 is empty and list 6 is
    populated by the end of the database only."""
    rng = np.random.default_rng(100 + d)
    rows = rng.standard_normal((N, d)).astype(F32)
    cents = rng.standard_normal((LISTS, d)).astype(F32)
    cents[EMPTY] = cents[0]
    cents[LATE] = 0
    cents[LATE, 0] = 100
    rows[:, 0] = -1
    rows[-3:, 0] = 3
    words = (F32(0.7) * rng.standard_normal((m_sub, 256, d // m_sub))).astype(F32)
    labels = rng.integers(0, EMPTY, N).astype(np.int64)
    labels[-3:] = LATE
    queries = rng.standard_normal((6, d)).astype(F32)
    for a in (rows, cents, words, labels, queries):
        a.setflags(write=False)
    return rows, cents, words, labels, queries


def one_shot(d, m_sub, explicit=True, keep_rows=False):
    """The parent's code: the constructor on all rows."""
    from mdir_amd import ivfpq
    rows, cents, words, labels, _ = world(d, m_sub)
    return ivfpq.IVFPQIndex(dev(rows), dev(cents), dev(labels) if explicit else None, m=m_sub, codebook=dev(words), keep_rows=keep_rows)


def streamed(d, m_sub, cuts, explicit=True):
    """The constructor on rows[:cuts[0]], then ``add`` of rows[cuts[i]:cuts[i + 1]]; only the current batch is on the device."""
    from mdir_amd import ivfpq
    rows, cents, words, labels, _ = world(d, m_sub)
    cuts = list(cuts) + [N]
    index = ivfpq.IVFPQIndex(dev(rows[:cuts[0]]), dev(cents), dev(labels[:cuts[0]]) if explicit else None, m=m_sub, codebook=dev(words),
                             keep_rows=False)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ids = index.add(dev(rows[lo:hi]), dev(labels[lo:hi]) if explicit else None)
        assert ids.dtype == torch.int64 and host(ids).tolist() == list(range(lo, hi))
    return index


def same_index(got, want):
    for name in ("codes", "order", "offsets"):
        IR.same_bits(host(getattr(got, name)), host(getattr(want, name)))
    assert got.host_sizes == want.host_sizes and (got.n, got.size, got.lists, got.m, got.d) == (want.n, want.size, want.lists, want.m, want.d)
    assert [got.capacity(p) for p in range(1, got.lists + 1)] == [want.capacity(p) for p in range(1, want.lists + 1)]
    assert got.nbytes() - want.nbytes() == 4 * got.n * got.d * ((got.rows is not None) - (want.rows is not None))


def restated(index, words, queries, k, nprobe):
    """PR.search on the structure the index holds, with the probes and coarse values of its own coarse index."""
    from mdir_amd import ops
    probes, coarse = ops.topk(index.coarse.scores(dev(queries), "ND"), nprobe)
    return PR.search(host(index.codes), host(index.order), index.n, host(index.offsets), PR.lut(words, queries), host(coarse), host(probes), k)


def check_restated(index, words, queries, k, nprobe):
    res = index.search(dev(queries), k, nprobe)
    ids, sc, scanned = restated(index, words, queries, k, nprobe)
    IR.same_bits(host(res.ids), ids), IR.same_bits(host(res.scores), sc), IR.same_bits(host(res.scanned), scanned)
    return res


# ------------------------------------------------------------------------------------------------ add

@pytest.mark.parametrize("explicit", [True, False], ids=["labels", "assigned"])
@pytest.mark.parametrize("first", [1, 256, N - 1])
@pytest.mark.parametrize("d,m_sub", SHAPES)
def test_a_streamed_build_equals_the_constructor(d, m_sub, first, explicit):
    """rows[:first] to the constructor and the rest in two batches (one, where the rest is a single row) against the constructor on all
    rows: every field of the contract, and every field of every search."""
    _, _, words, _, queries = world(d, m_sub)
    cuts = [first] if N - first < 2 else [first, first + (N - first) // 3]
    want, got = one_shot(d, m_sub, explicit), streamed(d, m_sub, cuts, explicit)
    try:
        # the premise: an empty list, and one only the added rows populate
        assert want.host_sizes[EMPTY] == 0 and host(want.order)[-3:].tolist() == [N - 3, N - 2, N - 1]
        assert want.host_sizes[LATE] == 3 and sum(want.host_sizes) == N
        same_index(got, want)
        assert got.rows is None and got.codes.is_contiguous()
        q_t = dev(queries)
        for k in (7, 400):
            for nprobe in (1, 3, LISTS):
                same_fields(got.search(q_t, k, nprobe), want.search(q_t, k, nprobe))
        same_fields(got.search(dev(np.ascontiguousarray(queries.T)), 9, 2, "DN", dev(queries[0])),
                    want.search(dev(np.ascontiguousarray(queries.T)), 9, 2, "DN", dev(queries[0])))
        res = check_restated(got, words, queries, 20, 3)
        assert (host(res.scanned) > 0).all()
    finally:
        want.close()
        got.close()


def test_chunks_of_an_add_change_no_bit():
    from mdir_amd import ivfpq
    d, m_sub = 64, 16
    rows, cents, words, labels, _ = world(d, m_sub)
    for explicit in (True, False):
        want = one_shot(d, m_sub, explicit)
        got = ivfpq.IVFPQIndex(dev(rows[:300]), dev(cents), dev(labels[:300]) if explicit else None, m=m_sub, codebook=dev(words),
                               keep_rows=False, chunk=64)
        try:
            got.add(dev(rows[300:]), dev(labels[300:]) if explicit else None, chunk=37)
            same_index(got, want)
        finally:
            want.close()
            got.close()


# ------------------------------------------------------------------------------------------------ remove

def test_remove_equals_the_restatement_and_the_searches_follow():
    d, m_sub = 64, 16
    rows, cents, words, labels, queries = world(d, m_sub)
    rng = np.random.default_rng(8)
    index = one_shot(d, m_sub)
    try:
        structure = (host(index.codes), host(index.order), host(index.offsets))
        tenth = rng.choice(N, N // 10, replace=False)
        whole = np.flatnonzero(labels == 2)                                 # a whole list
        gone = np.concatenate([tenth, whole, tenth[:9], [-1, N, N + 5, 1 << 40, -(1 << 40)]]).astype(np.int64)
        want, count = LR.remove(*structure, gone)
        assert count == len(set(tenth.tolist()) | set(whole.tolist())) < len(gone)
        before = index.search(dev(queries), 10, LISTS)
        assert host(before.scanned).tolist() == [N] * len(queries)
        assert index.remove(dev(rng.permutation(gone))) == count
        for got, w in zip((index.codes, index.order, index.offsets), want):
            IR.same_bits(host(got), w)
        sizes = np.diff(want[2]).tolist()
        assert index.host_sizes == sizes and sizes[2] == 0 and index.n == N and index.size == N - count == index.codes.shape[0]
        assert [index.capacity(p) for p in range(1, LISTS + 1)] == [max(1, c) for c in np.cumsum(sorted(sizes, reverse=True)).tolist()]
        # the searches are the restatement's on that structure; scanned falls; a removed id never comes back
        for k, nprobe in ((10, 1), (40, 3), (N, LISTS)):
            res = check_restated(index, words, queries, k, nprobe)
            assert not np.isin(host(res.ids), gone[(gone >= 0) & (gone < N)]).any()
        assert host(res.scanned).tolist() == [N - count] * len(queries)
        ids = host(res.ids)
        assert (np.sort(ids[:, :N - count], axis=1) == np.setdiff1d(np.arange(N), gone)).all() and (ids[:, N - count:] == -1).all()
        # ids that are not live any more are ignored; one that is counts once
        live = int(np.setdiff1d(np.arange(N), gone)[17])
        assert index.remove(dev(np.array([int(tenth[0]), live, int(whole[0]), live], np.int64))) == 1
        assert index.size == N - count - 1 and index.n == N and live not in host(index.order)
        assert index.remove(dev(gone)) == 0
        # removing everything raises and changes nothing
        held = (index.codes, index.order, index.offsets, list(index.host_sizes), index.size)
        with pytest.raises(ValueError, match="would leave no row"):
            index.remove(dev(np.arange(N, dtype=np.int64)))
        assert all(a is b for a, b in zip((index.codes, index.order, index.offsets), held))
        assert index.host_sizes == held[3] and index.size == held[4] and index.n == N
        check_restated(index, words, queries, 10, 3)
    finally:
        index.close()


@pytest.mark.parametrize("d,m_sub", SHAPES)
def test_removed_rows_come_back_under_new_ids_with_their_scores(d, m_sub):
    rows, _, _, labels, queries = world(d, m_sub)
    rng = np.random.default_rng(d)
    index = one_shot(d, m_sub)
    try:
        q_t = dev(queries)
        before = index.search(q_t, N, LISTS)
        back = np.sort(rng.choice(N, 60, replace=False))
        back = np.union1d(back, [N - 2])                                    # a row of the list of three
        assert index.remove(dev(back)) == len(back)
        ids = host(index.add(dev(rows[back]), dev(labels[back])))
        assert ids.tolist() == list(range(N, N + len(back))) and index.n == N + len(back) and index.size == N
        after = index.search(q_t, N, LISTS)
        assert host(after.scanned).tolist() == [N] * len(queries)
        old = np.arange(N + len(back))
        old[N:] = back                                                      # the row behind every id
        for q in range(len(queries)):
            was = np.empty(N, F32)
            was[host(before.ids)[q]] = host(before.scores)[q]
            now = np.empty(N, F32)
            got_ids = host(after.ids)[q]
            assert not np.isin(got_ids, back).any() and len(set(old[got_ids].tolist())) == N
            now[old[got_ids]] = host(after.scores)[q]
            IR.same_bits(now, was)
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------ rows, state, failures

def test_attached_rows_serve_the_shortlist_and_block_edits():
    d, m_sub = 64, 16
    rows, _, words, labels, queries = world(d, m_sub)
    want, got = one_shot(d, m_sub, keep_rows=True), streamed(d, m_sub, [256, 500])
    try:
        q_t, rows_t = dev(queries), dev(rows)
        with pytest.raises(ValueError, match="keep_rows=False"):
            got.search(q_t, 10, 3, shortlist=40)
        got.attach_rows(rows_t)
        assert got.rows is rows_t and got.nbytes() == want.nbytes()
        for k, nprobe, S in ((10, 1, 40), (30, 3, 100), (30, LISTS, 1000)):
            same_fields(got.search(q_t, k, nprobe, shortlist=S), want.search(q_t, k, nprobe, shortlist=S))
        for index in (got, want):
            with pytest.raises(ValueError, match="keeps the fp32 rows.*attach_rows\\(None\\)"):
                index.add(rows_t[:5], dev(labels[:5]))
            with pytest.raises(ValueError, match="keeps the fp32 rows.*attach_rows\\(None\\)"):
                index.remove(dev(np.arange(5, dtype=np.int64)))
        again = streamed(d, m_sub, [256, 500])                              # the refused edits changed nothing
        try:
            same_index(got, again)
        finally:
            again.close()
        with pytest.raises(ValueError, match="rows are \\(699, 64\\)"):
            got.attach_rows(rows_t[:N - 1])
        # after a removal the rows at removed ids are never read: they may hold anything
        got.attach_rows(None)
        gone = np.arange(0, N, 3, dtype=np.int64)
        assert got.rows is None and got.remove(dev(gone)) == len(gone)
        spoiled = rows.copy()
        spoiled[gone] = np.nan
        got.attach_rows(dev(spoiled))
        res, ref = got.search(q_t, 30, LISTS, shortlist=200), want.search(q_t, N, LISTS, shortlist=N)
        assert not np.isnan(host(res.scores)).any() and not np.isin(host(res.ids), gone).any()
        for q in range(len(queries)):
            exact = dict(zip(host(ref.ids)[q].tolist(), host(ref.scores)[q].view(np.uint32).tolist()))
            assert [exact[i] for i in host(res.ids)[q].tolist()] == host(res.scores)[q].view(np.uint32).tolist()
    finally:
        want.close()
        got.close()


def test_the_state_rebuilds_the_index_also_through_a_file():
    from mdir_amd import ivfpq
    d, m_sub = 64, 16
    rows, _, _, labels, queries = world(d, m_sub)
    index = streamed(d, m_sub, [256])
    copies = []
    try:
        index.remove(dev(np.arange(5, 400, 7, dtype=np.int64)))
        assert index.size < index.n == N
        state = index.state()
        assert sorted(state) == ["centroids", "codes", "codewords", "m", "n", "offsets", "order"]
        assert state["codes"] is index.codes and state["order"] is index.order and state["offsets"] is index.offsets
        assert state["centroids"] is index.centroids and state["codewords"] is index.codebook.codewords and (state["n"], state["m"]) == (N, m_sub)
        copies.append(ivfpq.IVFPQIndex.from_state(state))
        file = io.BytesIO()
        torch.save({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in state.items()}, file)
        file.seek(0)
        loaded = torch.load(file, weights_only=True)
        assert all(not v.is_cuda for v in loaded.values() if isinstance(v, torch.Tensor))
        copies.append(ivfpq.IVFPQIndex.from_state(loaded, device=DEV, rows=dev(rows)))
        q_t = dev(queries)
        for copy in copies:
            assert copy.codes.is_cuda and (copy.n, copy.size, copy.host_sizes) == (index.n, index.size, index.host_sizes)
            for k, nprobe in ((10, 1), (300, 3), (40, LISTS)):
                same_fields(copy.search(q_t, k, nprobe), index.search(q_t, k, nprobe))
        assert copies[0].nbytes() == index.nbytes() and copies[0].rows is None and copies[1].rows is not None
        assert copies[1].search(q_t, 10, 3, shortlist=50).ids.shape == (len(queries), 10)
        # a copy goes on where the original stood
        copies[0].add(dev(rows[:20]), dev(labels[:20]))
        index.add(dev(rows[:20]), dev(labels[:20]))
        same_index(copies[0], index)
    finally:
        index.close()
        for copy in copies:
            copy.close()


def test_a_failing_add_leaves_the_index_as_it_was(monkeypatch):
    from mdir_amd import ops
    d, m_sub = 12, 3
    rows, _, _, labels, queries = world(d, m_sub)
    index = streamed(d, m_sub, [600])
    try:
        held = (index.codes, index.order, index.offsets, index.n, index.size, list(index.host_sizes), list(index._capacity))
        bits = [host(t).copy() for t in held[:3]]
        bad = labels[:10].copy()
        bad[4] = LISTS

        def boom(*args, **kw):
            raise RuntimeError("no merge today")
        for call, error in ((lambda: index.add(dev(rows[:10]), dev(bad)), "labels must lie in \\[0, 7\\), got 0 .. 7"),
                            (lambda: index.add(dev(rows[:10]), dev(-bad)), "labels must lie in"),
                            (lambda: index.add(dev(rows[:10, :8]), dev(labels[:10])), "batch is \\[B, 8\\] and the index has D = 12"),
                            (lambda: index.add(torch.from_numpy(rows[:10].copy()), dev(labels[:10])), "batch must be a CUDA"),
                            (lambda: index.add(dev(rows[:10]), torch.from_numpy(labels[:10].copy())), "labels must be a CUDA"),
                            (lambda: index.add(dev(rows[:10]), dev(labels[:9])), "labels must be an int64 \\[10\\]")):
            with pytest.raises(ValueError, match=error):
                call()
        monkeypatch.setattr(ops, "lists_merge", boom)
        with pytest.raises(RuntimeError, match="no merge today"):
            index.add(dev(rows[:10]), dev(labels[:10]))
        monkeypatch.undo()
        now = (index.codes, index.order, index.offsets, index.n, index.size, index.host_sizes, index._capacity)
        assert all(a is b for a, b in zip(now[:3], held[:3])) and list(now[3:]) == list(held[3:])
        for t, b in zip(now[:3], bits):
            IR.same_bits(host(t), b)
        again = streamed(d, m_sub, [600])
        try:
            same_index(index, again)
        finally:
            again.close()
        assert host(index.add(dev(rows[:10]), dev(labels[:10]))).tolist() == list(range(N, N + 10))
    finally:
        index.close()


# ------------------------------------------------------------------------------------------------ the calls themselves

def test_merge_and_compact_in_one_captured_graph():
    """Both calls recorded once and replayed on new data: nothing is allocated by the library and nothing read back (the total of the
    compaction is given).  The merged structure is compacted in the same graph."""
    from mdir_amd import ops
    from test_gpu_lists_edit_memcontract import structure
    rng = np.random.default_rng(2)
    width, a_sizes, b_sizes = 16, (40, 0, 200, 65), (3, 9, 0, 130)
    m = sum(a_sizes) + sum(b_sizes)
    keep = np.zeros(m, bool)
    keep[::3] = True
    kept = LR.prefix(keep)
    total = int(kept[-1])
    data = [(structure(rng, a_sizes, width), structure(rng, b_sizes, width, first_id=sum(a_sizes))) for _ in range(2)]
    a_t, b_t = [dev(x) for x in data[0][0]], [dev(x) for x in data[0][1]]
    kept_t = dev(kept)

    def eager():
        merged = ops.lists_merge(*a_t, *b_t)
        return merged + ops.lists_compact(*merged, kept_t, total=total)
    eager()                                                                 # eager once, before anything is recorded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                             # one stream, one chain of launches: no parallel branches
            outs_g = eager()
    torch.cuda.current_stream().wait_stream(side)
    for a, b in (data[1], data[0]):                                        # new data, then the old again
        for t, x in zip(a_t + b_t, a + b):
            t.copy_(dev(x))
        g.replay()
        torch.cuda.synchronize()
        want = LR.merge(*a, *b)
        want = want + LR.compact(*want, kept)
        for got, w in zip(outs_g, want):
            IR.same_bits(host(got), w)
