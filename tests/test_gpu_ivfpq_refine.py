"""IVFPQIndex(..., refine="i8") on the device (mdir_amd/ivfpq.py; include/mdx_refine.h), bit for bit: what the module docstring
promises -- (a) the scores of an int8 index, (b) the int8 IVF search's rows and (c) the fp32 IVF search's rows where the shortlist
holds every candidate, (d) the restatement (tests/refine_restatement.py) whatever the query chunk --, the split build, removals, the
state through torch.save, and refine=None indexes beside all of it, unchanged."""
import functools
import io

import numpy as np
import pytest
import torch

import ivf_restatement as IR
import lists_i8_restatement as LI
import pq_restatement as PR
import refine_restatement as RR
from test_gpu_ivf import dev, exact_scores, host
from test_gpu_lists_i8 import i8_scores
from test_gpu_lists_pq import same_fields

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
N, LISTS, EMPTY, NQ = 400, 7, 4, 6                  # list 4 stays empty
SHAPES = [(64, 4), (64, 8), (100, 4)]               # (D, m): d_pad = 64 and 128


@functools.lru_cache(maxsize=None)
def world(d, m_sub):
    """(rows [N, d], centroids [7, d], codewords, labels, queries [6, d], center [d]) on the host, one fixed draw per shape, shared and
    never written."""
    rng = np.random.default_rng(1000 * d + m_sub)
    rows = rng.standard_normal((N, d)).astype(F32)
    rows[17] = 0                                                           # a zero row: scale 0
    cents = rng.standard_normal((LISTS, d)).astype(F32)
    words = (F32(0.7) * rng.standard_normal((m_sub, 256, d // m_sub))).astype(F32)
    labels = rng.integers(0, LISTS - 1, N).astype(np.int64)
    labels[labels >= EMPTY] += 1
    queries = rng.standard_normal((NQ, d)).astype(F32)
    center = (F32(0.1) * rng.standard_normal(d)).astype(F32)
    for a in (rows, cents, words, labels, queries, center):
        a.setflags(write=False)
    return rows, cents, words, labels, queries, center


def build(d, m_sub, lo=0, hi=N, refine="i8", keep_rows=False):
    from mdir_amd import ivfpq
    rows, cents, words, labels, _, _ = world(d, m_sub)
    return ivfpq.IVFPQIndex(dev(rows[lo:hi]), dev(cents), dev(labels[lo:hi]), m=m_sub, codebook=dev(words), keep_rows=keep_rows, refine=refine)


def restated(index, words, rows_by_id, queries, k, nprobe, shortlist, rescore=None, center=None):
    """RR.search on the structure the index holds -- its refinement payload encoded again on the host from the row of every id --
    with the probes and coarse values of its own coarse index."""
    from mdir_amd import ops
    probes, coarse = ops.topk(index.coarse.scores(dev(queries), "ND", center=None if center is None else dev(center)), nprobe)
    order = host(index.order)
    fine_codes, fine_scales = LI.encode(rows_by_id, order)
    return RR.search(host(index.codes), order, index.n, host(index.offsets), PR.lut(words, queries, center), host(coarse), host(probes),
                     fine_codes, fine_scales, queries, k, shortlist, rescore, center, rows_by_id)


def check_payload(index, rows_by_id):
    """refine_codes, refine_scales and where are what the contract says of the index's order."""
    order = host(index.order)
    codes, scales = LI.encode(rows_by_id, order)
    IR.same_bits(host(index.refine_codes), codes), IR.same_bits(host(index.refine_scales), scales)
    IR.same_bits(host(index.where), RR.where_of(order, index.n))
    assert index.refine == "i8" and index.refine_codes.dtype == torch.int8 and index.refine_codes.is_contiguous()


def check_restated(index, words, rows_by_id, queries, k, nprobe, shortlist, rescore=None):
    res = index.search(dev(queries), k, nprobe, shortlist=shortlist, rescore=rescore)
    ids, sc, scanned = restated(index, words, rows_by_id, queries, k, nprobe, shortlist, rescore)
    IR.same_bits(host(res.ids), ids), IR.same_bits(host(res.scores), sc), IR.same_bits(host(res.scanned), scanned)
    return res


# ------------------------------------------------------------------------------------------------ the search

@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("qlayout", ["ND", "DN"])
@pytest.mark.parametrize("d,m_sub", SHAPES)
def test_the_four_promises_of_the_search(d, m_sub, qlayout, centred, monkeypatch):
    from mdir_amd import ivf
    rows, cents, words, labels, queries, center = world(d, m_sub)
    center = center if centred else None
    index = build(d, m_sub, keep_rows=True)
    args = (dev(rows), dev(cents), dev(labels))
    i8, f32 = ivf.IVFIndex(*args, storage="i8"), ivf.IVFIndex(*args)
    try:
        check_payload(index, rows)
        q_t = dev(queries if qlayout == "ND" else np.ascontiguousarray(queries.T))
        c_t = None if center is None else dev(center)
        full8, full32 = i8_scores(rows, queries, center=center), exact_scores(rows, queries, center=center)
        seen = {"below": 0, "equal": 0, "above": 0}
        for nprobe, k in ((2, 10), (LISTS, 25)):
            scanned = host(index.search(q_t, k, nprobe, qlayout, c_t).scanned)
            assert scanned.min() > k
            # a shortlist below every query's candidates, equal to one query's, and above all of them
            for s in (k + 5, int(scanned[1]), int(scanned.max()) + 9):
                res = index.search(q_t, k, nprobe, qlayout, c_t, shortlist=s)
                want = restated(index, words, rows, queries, k, nprobe, s, None, center)
                for got, w in zip((res.ids, res.scores, res.scanned), want):            # (d)
                    IR.same_bits(host(got), w)
                ids, sc = host(res.ids), host(res.scores)
                assert (ids >= 0).all() and ids.shape == (NQ, k)
                for q in range(NQ):                                                      # (a)
                    IR.same_bits(sc[q], full8[q][ids[q]])
                ref8 = i8.search(q_t, k, nprobe, qlayout, c_t)
                IR.same_bits(host(res.probes), host(ref8.probes)), IR.same_bits(scanned, host(ref8.scanned))
                complete = scanned <= s                                                  # (b)
                IR.same_bits(ids[complete], host(ref8.ids)[complete]), IR.same_bits(sc[complete], host(ref8.scores)[complete])
                seen["below"] += int((scanned > s).sum())
                seen["equal"] += int((scanned == s).sum())
                seen["above"] += int((scanned < s).sum())
                ref32 = f32.search(q_t, k, nprobe, qlayout, c_t)
                for r in (k, (k + s) // 2, s):
                    sure = index.search(q_t, k, nprobe, qlayout, c_t, shortlist=s, rescore=r)
                    want = restated(index, words, rows, queries, k, nprobe, s, r, center)
                    for got, w in zip((sure.ids, sure.scores, sure.scanned), want):      # (d)
                        IR.same_bits(host(got), w)
                    for q in range(NQ):
                        IR.same_bits(host(sure.scores)[q], full32[q][host(sure.ids)[q]])
                    complete = scanned <= r                                              # (c)
                    IR.same_bits(host(sure.ids)[complete], host(ref32.ids)[complete])
                    IR.same_bits(host(sure.scores)[complete], host(ref32.scores)[complete])
                    if r == s:
                        seen["c"] = seen.get("c", 0) + int(complete.sum())
                    # the query chunk changes no bit
                    with monkeypatch.context() as patch:
                        patch.setattr(index, "query_chunk", lambda *a: 1)
                        same_fields(index.search(q_t, k, nprobe, qlayout, c_t, shortlist=s, rescore=r), sure)
                with monkeypatch.context() as patch:
                    patch.setattr(index, "query_chunk", lambda *a: 1)
                    same_fields(index.search(q_t, k, nprobe, qlayout, c_t, shortlist=s), res)
        assert min(seen.values()) > 0, seen
    finally:
        for x in (index, i8, f32):
            x.close()


def test_padding_comes_back_as_minus_one_behind_every_candidate():
    """k and S above a query's candidates: -1 / NaN behind them, with and without the exact stage, as in the IVF searches."""
    from mdir_amd import ivf
    d, m_sub = 64, 4
    rows, cents, words, labels, queries, _ = world(d, m_sub)
    index = build(d, m_sub, keep_rows=True)
    args = (dev(rows), dev(cents), dev(labels))
    i8, f32 = ivf.IVFIndex(*args, storage="i8"), ivf.IVFIndex(*args)
    try:
        q_t = dev(queries)
        k, s = 150, 200
        res = check_restated(index, words, rows, queries, k, 1, s)
        scanned = host(res.scanned)
        assert (scanned < k).any()
        ref = i8.search(q_t, k, 1)
        IR.same_bits(host(res.ids), host(ref.ids)), IR.same_bits(host(res.scores), host(ref.scores))
        for q in range(NQ):
            assert (host(res.ids)[q, scanned[q]:] == -1).all() and np.isnan(host(res.scores)[q, scanned[q]:]).all()
        sure = check_restated(index, words, rows, queries, k, 1, s, rescore=s)
        ref = f32.search(q_t, k, 1)
        IR.same_bits(host(sure.ids), host(ref.ids)), IR.same_bits(host(sure.scores), host(ref.scores))
    finally:
        for x in (index, i8, f32):
            x.close()


def test_refine_none_is_the_index_it_was():
    """A refine=None index beside a refine="i8" one: its ADC ranking and its fp32 route are the other's (rescore=S is the fp32 route's
    spelling there), its state has the keys it had, and the difference in nbytes is the three tensors."""
    d, m_sub = 64, 8
    rows, _, words, _, queries, _ = world(d, m_sub)
    plain, fine = build(d, m_sub, refine=None, keep_rows=True), build(d, m_sub, keep_rows=True)
    try:
        assert plain.refine is None and not hasattr(plain, "refine_codes") and not hasattr(plain, "where")
        assert sorted(plain.state()) == ["centroids", "codes", "codewords", "m", "n", "offsets", "order"]
        assert fine.nbytes() - plain.nbytes() == N * 64 + 4 * N + 8 * N
        assert fine.query_chunk(3) == plain.query_chunk(3) and fine.query_chunk(3, 1000) < plain.query_chunk(3, 1000)
        q_t = dev(queries)
        for k, nprobe, s in ((10, 2, 40), (30, LISTS, 300)):
            same_fields(plain.search(q_t, k, nprobe), fine.search(q_t, k, nprobe))
            same_fields(plain.search(q_t, k, nprobe, shortlist=s), fine.search(q_t, k, nprobe, shortlist=s, rescore=s))
            ids, sc, scanned = PR.search(host(plain.codes), host(plain.order), N, host(plain.offsets), PR.lut(words, queries),
                                         *(host(t) for t in _coarse(plain, queries, nprobe)), k)
            res = plain.search(q_t, k, nprobe)
            IR.same_bits(host(res.ids), ids), IR.same_bits(host(res.scores), sc), IR.same_bits(host(res.scanned), scanned)
        with pytest.raises(ValueError, match="needs an index built with refine"):
            plain.search(q_t, 10, 2, shortlist=40, rescore=20)
        fine.attach_rows(None)
        assert fine.search(q_t, 10, 2, shortlist=40).ids.shape == (NQ, 10)          # no fp32 rows are needed
        with pytest.raises(ValueError, match="is rescored on the fp32 rows"):
            fine.search(q_t, 10, 2, shortlist=40, rescore=20)
    finally:
        plain.close()
        fine.close()


def _coarse(index, queries, nprobe):
    from mdir_amd import ops
    probes, coarse = ops.topk(index.coarse.scores(dev(queries), "ND"), nprobe)
    return coarse, probes


# ------------------------------------------------------------------------------------------------ editing and saving

@pytest.mark.parametrize("d,m_sub", SHAPES)
def test_a_split_build_holds_the_payload_of_the_constructor(d, m_sub):
    rows, _, words, labels, queries, _ = world(d, m_sub)
    want, got = build(d, m_sub), build(d, m_sub, 0, 130)
    try:
        for lo, hi in ((130, 131), (131, N)):
            ids = got.add(dev(rows[lo:hi]), dev(labels[lo:hi]))
            assert host(ids).tolist() == list(range(lo, hi))
        for name in ("codes", "order", "offsets", "refine_codes", "refine_scales", "where"):
            IR.same_bits(host(getattr(got, name)), host(getattr(want, name)))
        assert got.nbytes() == want.nbytes() and (got.n, got.size, got.host_sizes) == (want.n, want.size, want.host_sizes)
        check_payload(got, rows)
        q_t = dev(queries)
        for k, nprobe, s in ((10, 2, 50), (40, LISTS, N)):
            same_fields(got.search(q_t, k, nprobe, shortlist=s), want.search(q_t, k, nprobe, shortlist=s))
        check_restated(got, words, rows, queries, 10, 3, 60)
    finally:
        want.close()
        got.close()


def test_removals_keep_the_payload_in_step():
    """A whole list, scattered ids and an id that was just added leave; the payload follows the order, and the searches are the
    restatement's on the rows that stay -- also with the exact stage on attached rows whose removed ids hold NaN."""
    d, m_sub = 100, 4
    rows, _, words, labels, queries, _ = world(d, m_sub)
    rng = np.random.default_rng(5)
    index = build(d, m_sub, 0, N - 20)
    try:
        added = host(index.add(dev(rows[N - 20:]), dev(labels[N - 20:])))
        whole = np.flatnonzero(labels == 2)
        scattered = rng.choice(N, 40, replace=False)
        gone = np.unique(np.concatenate([whole, scattered, added[-1:]]))
        assert index.remove(dev(rng.permutation(np.concatenate([gone, [-1, N, 1 << 40]])))) == len(gone)
        assert index.size == N - len(gone) and index.n == N and index.host_sizes[2] == 0
        check_payload(index, rows)
        assert (host(index.where)[gone] == -1).all() and (host(index.where) >= 0).sum() == index.size
        for k, nprobe, s in ((10, 1, 30), (20, 3, 200), (N, LISTS, N)):
            res = check_restated(index, words, rows, queries, k, nprobe, s)
            assert not np.isin(host(res.ids), gone).any()
        spoiled = rows.copy()
        spoiled[gone] = np.nan
        index.attach_rows(dev(spoiled))
        res = check_restated(index, words, spoiled, queries, 20, 3, 200, rescore=50)
        assert not np.isnan(host(res.scores)).any()
        with pytest.raises(ValueError, match="keeps the fp32 rows.*attach_rows\\(None\\)"):
            index.remove(dev(gone))
        index.attach_rows(None)
        # a removed row comes back under a new id, and scores as it did
        back = host(index.add(dev(rows[gone[:3]]), dev(labels[gone[:3]])))
        assert back.tolist() == [N, N + 1, N + 2] and index.n == N + 3
        by_id = np.concatenate([rows, rows[gone[:3]]])
        check_payload(index, by_id)
        check_restated(index, words, by_id, queries, 20, LISTS, 300)
    finally:
        index.close()


def test_the_state_rebuilds_a_refine_index_also_through_a_file():
    from mdir_amd import ivfpq
    d, m_sub = 64, 8
    rows, _, _, labels, queries, _ = world(d, m_sub)
    index, plain = build(d, m_sub, 0, 300), build(d, m_sub, refine=None)
    copies = []
    try:
        index.add(dev(rows[300:]), dev(labels[300:]))
        index.remove(dev(np.arange(5, 300, 7, dtype=np.int64)))
        state = index.state()
        assert sorted(state) == ["centroids", "codes", "codewords", "m", "n", "offsets", "order", "refine_codes", "refine_scales"]
        assert state["refine_codes"] is index.refine_codes and state["refine_scales"] is index.refine_scales
        copies.append(ivfpq.IVFPQIndex.from_state(state))
        file = io.BytesIO()
        torch.save({k: v.cpu() if isinstance(v, torch.Tensor) else v for k, v in state.items()}, file)
        file.seek(0)
        copies.append(ivfpq.IVFPQIndex.from_state(torch.load(file, weights_only=True), device=DEV, rows=dev(rows)))
        q_t = dev(queries)
        for copy in copies:
            assert copy.refine == "i8" and copy.refine_codes.is_cuda and copy.nbytes() - index.nbytes() == 4 * N * d * (copy.rows is not None)
            IR.same_bits(host(copy.where), host(index.where))
            for k, nprobe, s in ((10, 1, 30), (40, LISTS, 300)):
                same_fields(copy.search(q_t, k, nprobe), index.search(q_t, k, nprobe))
                same_fields(copy.search(q_t, k, nprobe, shortlist=s), index.search(q_t, k, nprobe, shortlist=s))
        assert copies[1].search(q_t, 10, 3, shortlist=50, rescore=20).ids.shape == (NQ, 10)
        copies[0].add(dev(rows[:9]), dev(labels[:9]))                       # a copy goes on where the original stood
        index.add(dev(rows[:9]), dev(labels[:9]))
        for name in ("codes", "order", "offsets", "refine_codes", "refine_scales", "where"):
            IR.same_bits(host(getattr(copies[0], name)), host(getattr(index, name)))
        # a state without the two keys still loads as a refine=None index
        old = ivfpq.IVFPQIndex.from_state(plain.state())
        copies.append(old)
        assert old.refine is None and not hasattr(old, "where") and old.nbytes() == plain.nbytes()
        same_fields(old.search(q_t, 10, 3), plain.search(q_t, 10, 3))
        with pytest.raises(ValueError, match="state\\['refine_scales'\\]"):
            ivfpq.IVFPQIndex.from_state({k: v for k, v in state.items() if k != "refine_scales"})
    finally:
        index.close()
        plain.close()
        for copy in copies:
            copy.close()
