"""Every similarity path, bit for bit, on exactly representable data (tests/lattice.py; the grids and the condition that makes
them order-independent are checked on the CPU in tests/test_lattice_host.py).

All comparisons are ``assert_array_equal`` on the uint32 bit patterns against ``lattice.expected``, an integer matrix product:
no tolerance, no oracle of a kernel's summation order.  A mismatch is a defect of a kernel or of its stated contract, never
rounding noise.  An exact-zero score is +0 on every path (tests/lattice.py says why; oracle/chain.c gives +0 as well), so the
rank order's "-0 == +0" never has to be used: ``expected`` holds +0 and the bits are compared.

  a. the common grid through every dispatch branch of mdir_amd/csrc/mdx_index.hip (lattice.TRIPLES names them): fp32, fp16 and
     int8 indexes, both layouts of both operands, with and without a centre, split3 / split2, the row-major route (also at a
     4-byte-aligned address), the rescore; MDX_SCORES_PIPE=0 on the 128-row shapes; MDX_F16_RING=1 in a child process
  b. the fp16 contract: all 11 significand bits, fp16 subnormals, +-65504, round to nearest even of fp32 inputs, and the
     non-finite rules (the fp16 twin of test_similarity_with_non_finite_and_denormal_values and
     test_rowmajor_product_with_infinities_in_a_padded_chunk)
  c. the split modes with two live pieces per operand and at other block exponents
  d. rankings, top-k lists, range results and kNN lists on top of massively tied scores: identical for every storage."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lattice
from conftest import ROOT
from lattice import bits
from oracle import chain as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(what))


class Operands:
    """The device copies of a Lattice: both layouts of both operands, the centre."""

    def __init__(self, L):
        self.x = {"ND": dev(L.db), "DN": dev(L.db.T)}
        self.q = {"ND": dev(L.queries), "DN": dev(L.queries.T)}
        self.c = None if L.center is None else dev(L.center)


def check_index(L, want, storage, computes=("chain",), what=()):
    """An index of ``storage`` built from either layout, asked in either layout, in every compute mode: the expected bits."""
    from mdir_amd import ops
    o = Operands(L)
    for xl in ("ND", "DN"):
        ix = ops.DescriptorIndex(o.x[xl], xl, storage=storage)
        try:
            for ql in ("ND", "DN"):
                for mode in computes:
                    same(ix.scores(o.q[ql], ql, center=o.c, compute=mode), want, what + (storage, mode, "db " + xl, "queries " + ql))
        finally:
            ix.close()


def check_rowmajor_and_rescore(L, want, what=()):
    from mdir_amd import ops
    o = Operands(L)
    n, d = L.db.shape
    nq = L.queries.shape[0]
    if d % 4 == 0:                                            # mdx_scores_rowmajor reads rows in pieces of four values
        flat = torch.empty(n * d + 1, dtype=torch.float32, device=DEV)
        shifted = flat[1:].view(n, d)                         # 4 bytes past an allocation boundary: 4-byte aligned, no more
        shifted.copy_(o.x["ND"])
        assert shifted.data_ptr() % 16 == 4
        for ql in ("ND", "DN"):
            same(ops.scores_rowmajor(o.x["ND"], o.q[ql], ql, center=o.c), want, what + ("rowmajor", ql))
            same(ops.scores_rowmajor(shifted, o.q[ql], ql, center=o.c), want, what + ("rowmajor + 4 bytes", ql))
    # rescore: all ids (a strided 4096 of them for a larger shard, the last row included) of a few queries, handed over shuffled
    qs = sorted({0, nq // 2, nq - 1})
    ids = np.arange(n) if n <= 4096 else np.unique(np.concatenate([np.arange(0, n, n // 4000)[:4090], [n - 1, n - 2, n - 17]]))
    rng = np.random.default_rng(n + d)
    given = np.stack([rng.permutation(ids) for _ in qs])
    got_ids, got_sc = ops.rescore(o.x["ND"], o.q["ND"][qs].contiguous(), dev(given), "ND", center=o.c)
    sub = np.ascontiguousarray(want[qs][:, ids])
    order = OC.rank_full(sub)                                 # descending score, ascending position = ascending id (ids is sorted)
    np.testing.assert_array_equal(got_ids.cpu().numpy(), ids[order], err_msg=str(what + ("rescore ids",)))
    same(got_sc, np.take_along_axis(sub, order, axis=1), what + ("rescore scores",))


def check_common(n, d, nq, storages=("f32", "f16", "i8"), extras=True):
    for centred in (False, True):
        L = lattice.common(n, d, nq, centred=centred)
        want = lattice.expected(L.qi, L.xi, 1.0)
        what = ((n, d, nq), "centred" if centred else "plain")
        for storage in storages:
            check_index(L, want, storage, ("chain", "split3", "split2") if storage == "f32" else ("chain",), what)
        if extras:
            check_rowmajor_and_rescore(L, want, what)


# ------------------------------------------------------------------------------------------------ a. every path, every branch

@pytest.mark.parametrize("n,d,nq", lattice.TRIPLES)
def test_every_path_on_the_common_grid(n, d, nq):
    check_common(n, d, nq)


@pytest.mark.parametrize("n,d,nq", lattice.R2_TRIPLES)
def test_unpipelined_consumer_on_the_common_grid(n, d, nq, monkeypatch):
    """MDX_SCORES_PIPE=0 (read per launch): the 128-row fp32 kernel without the pipelined consumer."""
    monkeypatch.setenv("MDX_SCORES_PIPE", "0")
    check_common(n, d, nq, storages=("f32",), extras=False)


@pytest.mark.parametrize("storage", ["f32", "f16", "i8"])
def test_partial_last_tile_behind_full_groups_stays_inside_the_scores(storage):
    """250 queries are two full groups of eight query tiles whose last tile holds 10 queries.  One launch takes both groups
    (grid.y = 2) and has to be told 250 queries, not the 256 its tiles have room for: the scores are the head of a larger
    buffer here, and the six rows behind them keep their fill."""
    from mdir_amd import ops
    n, d, nq = 200, 64, 250
    L = lattice.common(n, d, nq)
    whole = torch.full((nq + 6, n), 7.0, dtype=torch.float32, device=DEV)
    ix = ops.DescriptorIndex(dev(L.db), "ND", storage=storage)
    try:
        same(ix.scores(dev(L.queries), "ND", out=whole[:nq]), lattice.expected(L.qi, L.xi, 1.0), (storage, "250 queries"))
    finally:
        ix.close()
    assert bool((whole[nq:] == 7.0).all())


def _stream_shapes(triples):
    """The shapes whose fp16 shard takes the register-streaming kernel in-process (d_pad % 128 == 0): only there does
    MDX_F16_RING=1 change the kernel."""
    return [t for t in triples if (-(-t[1] // 64) * 64) % 128 == 0]


RING_GROUPS = {"small": [t for t in _stream_shapes(lattice.TRIPLES) if t[0] < 30000],
               "large-a": [t for t in _stream_shapes(lattice.TRIPLES) if t[0] >= 30000][0::2],
               "large-b": [t for t in _stream_shapes(lattice.TRIPLES) if t[0] >= 30000][1::2],
               "contract": _stream_shapes(lattice.F16_TRIPLES)}


def f16_table(group):
    """The fp16 part of the tables above for one group of shapes (the child process of test_f16_ring_kernel)."""
    if group == "contract":
        for n, d, nq in RING_GROUPS[group]:
            check_f16_wide(n, d, nq)
            check_f16_round(n, d, nq)
            check_f16_non_finite(n, d, nq)
    else:
        for n, d, nq in RING_GROUPS[group]:
            check_common(n, d, nq, storages=("f16",), extras=False)


@pytest.mark.parametrize("group", sorted(RING_GROUPS))
def test_f16_ring_kernel(group):
    """MDX_F16_RING=1 is read once per process: a child runs the fp16 part of the same tables on the ring kernel."""
    assert RING_GROUPS[group]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_lattice as T; T.f16_table(%r); print('LATTICE-F16-RING-OK')"
            % (ROOT, os.path.join(ROOT, "tests"), group))
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MDX_F16_RING="1"), text=True, capture_output=True, timeout=300)
    assert proc.returncode == 0 and "LATTICE-F16-RING-OK" in proc.stdout, (proc.stdout[-2000:], proc.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ b. the fp16 contract

def check_f16_wide(n, d, nq):
    for case in (dict(), dict(swap=True), dict(db_exp=-24), dict(db_exp=-24, q_exp=-24), dict(swap=True, q_exp=-24), dict(db_exp=-34),
                 dict(swap=True, q_exp=-34), dict(db_exp=5, top=True), dict(swap=True, q_exp=5, top=True)):
        L = lattice.f16_wide(n, d, nq, **case)
        check_index(L, lattice.expected(L.qi, L.xi, L.uq * L.ux), "f16", what=((n, d, nq), "f16_wide", sorted(case.items())))


def check_f16_round(n, d, nq):
    for band in lattice.F16_ROUND_BANDS:
        for swap in (False, True):
            L = lattice.f16_round(n, d, nq, band, swap=swap)
            check_index(L, lattice.expected(L.qi, L.xi, L.uq * L.ux), "f16", what=((n, d, nq), "f16_round", band, "swap" if swap else ""))


@pytest.mark.parametrize("n,d,nq", lattice.F16_TRIPLES + [(15, 4096, 8)])
def test_f16_uses_the_whole_significand_and_its_subnormals(n, d, nq):
    """|x| <= 2047 against |q| <= 3 and the reverse; the same on fp16's subnormal grid (one operand, both), below it, and with
    +-65504: the products are exact, the accumulation is fp32, no partial sum rounds -- the integer product, bit for bit."""
    check_f16_wide(n, d, nq)


@pytest.mark.parametrize("n,d,nq", lattice.F16_TRIPLES)
def test_f16_rounds_its_inputs_to_nearest_even(n, d, nq):
    """fp32 inputs that are not fp16 values (half-way cases of both parities and signs, their fp32 neighbours, the last value
    under the overflow threshold, values below 2^-25), as database and as queries: the product of ``astype(np.float16)``."""
    check_f16_round(n, d, nq)


def _classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def check_f16_non_finite(n, d, nq):
    from mdir_amd import ops
    assert n >= 15 and nq >= 8
    L = lattice.f16_wide(n, d, nq, seed=3)
    L.db[n - 2], L.xi[n - 2] = 0, 0                          # an all-zero row beside the poisoned last row
    L.db[3], L.xi[3] = 0, 0
    L.queries[nq - 2], L.qi[nq - 2] = 0, 0
    clean = lattice.expected(L.qi, L.xi, L.uq * L.ux)
    db, q = L.db.copy(), L.queries.copy()
    inf, edge = np.float32(np.inf), np.float32(65520.0)       # 65520 is half way to 65536: the smallest value that rounds to infinity
    db[n - 1, d - 1] = inf                                    # the last row of the partly padded tile, the last k before the padding
    db[1, 0] = -inf
    db[2, d // 2] = np.nan
    db[4, d - 1] = edge
    db[5, d // 3] = np.float32(-70000.0)
    db[6, 0], db[6, d - 1] = inf, -inf
    db[8, d - 1] = np.float32(1e30)
    q[0, d - 1] = inf
    q[1, 0] = np.nan
    q[2, d // 2] = -edge
    q[nq - 1, d - 1] = -inf                                   # the last query of the partly padded query tile
    bad_rows, bad_q = [n - 1, 1, 2, 4, 5, 6, 8], [0, 1, 2, nq - 1]
    with np.errstate(over="ignore", invalid="ignore"):
        x16 = db.astype(np.float16).astype(np.float64)
        q16 = q.astype(np.float16).astype(np.float64)
        assert np.isposinf(x16[4, d - 1]) and np.isneginf(x16[5, d // 3]) and np.isneginf(q16[2, d // 2])
        # the float64 product of the fp16-rounded operands, term by term (0 * inf = NaN, inf - inf = NaN, as IEEE has it)
        want_rows = np.stack([(q16 * x16[r][None, :]).sum(axis=1) for r in bad_rows], axis=1)      # [nq, bad rows]
        want_q = np.stack([(x16 * q16[t][None, :]).sum(axis=1) for t in bad_q])                    # [bad queries, n]
    assert (_classes(want_rows) != 0).any(axis=0).all() and (_classes(want_q) != 0).any(axis=1).all()
    assert {1, 2, 3} <= set(np.unique(_classes(want_rows))) | set(np.unique(_classes(want_q)))
    untouched = np.ones((nq, n), dtype=bool)
    untouched[:, bad_rows] = False
    untouched[bad_q, :] = False
    for xl in ("ND", "DN"):
        ix = ops.DescriptorIndex(dev(db if xl == "ND" else db.T), xl, storage="f16")
        try:
            for ql in ("ND", "DN"):
                got = ix.scores(dev(q if ql == "ND" else q.T), ql).cpu().numpy()
                what = str(((n, d, nq), "non-finite", xl, ql))
                # no other row or query changes a bit: nothing leaks through the zero padding
                np.testing.assert_array_equal(bits(got)[untouched], bits(clean)[untouched], err_msg=what)
                for block, want in ((got[:, bad_rows], want_rows), (got[bad_q, :], want_q)):
                    np.testing.assert_array_equal(_classes(block), _classes(want), err_msg=what)
                    fin = _classes(want) == 0
                    np.testing.assert_array_equal(block[fin], want[fin].astype(np.float32), err_msg=what)
        finally:
            ix.close()


@pytest.mark.parametrize("n,d,nq", lattice.F16_TRIPLES)
def test_f16_non_finite_values_stay_in_their_row_and_query(n, d, nq):
    """+-inf and NaN elements in database rows and in queries, fp32 values that round to infinity (65520, -70000, 1e30), in
    the last, partly padded tile and beside all-zero rows: a score is non-finite exactly where the float64 product of the
    fp16-rounded operands is, with the same class and sign, and no other row or query changes a bit."""
    check_f16_non_finite(n, d, nq)


# ------------------------------------------------------------------------------------------------ c. the split modes

@pytest.mark.parametrize("n,d,nq", lattice.SPLIT_TRIPLES)
def test_split_modes_with_two_live_pieces(n, d, nq):
    """x = a + b 2^-8 (split3) and x = a + b 2^-11 (split2) against one-piece operands, as database and as queries: every
    product the modes keep is exact and nothing they drop is nonzero, so they return the integer product."""
    for swap in (False, True):
        L = lattice.split3_two_piece(n, d, nq, swap=swap)
        check_index(L, lattice.expected(L.qi, L.xi, L.uq * L.ux), "f32", ("split3", "chain"), ((n, d, nq), "two-piece", "swap" if swap else ""))
        L = lattice.split2_two_piece(n, d, nq, swap=swap)
        check_index(L, lattice.expected(L.qi, L.xi, L.uq * L.ux), "f32", ("split2", "chain"), ((n, d, nq), "two-piece", "swap" if swap else ""))


@pytest.mark.parametrize("n,d,nq", [(65, 100, 17), (129, 2048, 17), (32769, 128, 57), (65521, 64, 17), (65537, 100, 129)])
def test_split_modes_at_other_block_exponents(n, d, nq):
    """The common grid with the database times 2^10 and the queries times 2^-13 (and unscaled, for the 256-row consumers the
    first table does not reach): the expected result times the exact power of two."""
    L = lattice.common(n, d, nq)
    for ex, eq in ((0, 0), (10, -13), (-40, 30)):
        M = L._replace(db=L.db * np.float32(2.0 ** ex), queries=L.queries * np.float32(2.0 ** eq))
        check_index(M, lattice.expected(L.qi, L.xi, 2.0 ** (ex + eq)), "f32", ("split3", "split2", "chain"), ((n, d, nq), "exponents", ex, eq))


# ------------------------------------------------------------------------------------------------ d. ranking on tied scores

N_TIED, NQ_TIED, KS = 5003, 37, (1, 10, 64, 1000)


class Tied:
    """Common-grid rows with |x| <= 1 besides their +-127: a few hundred distinct scores over 5003 rows, so every ranking is
    decided by the tie rule.  Computed once per dimension and shared, unchanged."""

    def __init__(self, d):
        self.L = L = lattice.common(N_TIED, d, NQ_TIED, seed=5, amp=1, period=29)
        self.want = lattice.expected(L.qi, L.xi, 1.0)
        self.rank = OC.rank_full(self.want)
        self.self_scores = lattice.expected(L.xi, L.xi, 1.0)             # [n, n], symmetric
        self.rows = dev(L.db)
        self.queries = dev(L.queries)

    def top_of_rows(self, k):
        """(ids, scores) [n, k]: the first k of every row of the self-similarity in rank_full's order (descending score,
        ascending id), from the integer scores: key = score * 8192 + (8191 - id)."""
        s = self.self_scores.astype(np.int64)
        key = s * 8192 + (8191 - np.arange(N_TIED, dtype=np.int64))[None, :]
        part = np.argpartition(-key, k, axis=1)[:, :k + 1]
        order = np.argsort(-np.take_along_axis(key, part, axis=1), axis=1)
        ids = np.take_along_axis(part, order, axis=1)
        return ids[:, :k], np.take_along_axis(self.self_scores, ids, axis=1)[:, :k], np.take_along_axis(s, ids, axis=1)


@pytest.fixture(scope="module", params=[64, 128])
def tied(request):
    return Tied(request.param)


def _csr(res):
    return res.offsets.cpu().numpy(), res.ids.cpu().numpy(), res.scores.cpu().numpy()


def _brute_csr(scores, tau, upper=False):
    """The CSR of every score >= tau per row in rank order (descending score, ascending id); ``upper``: columns j > row only."""
    offs, ids, vals = [0], [], []
    for r in range(scores.shape[0]):
        row = scores[r]
        hit = np.nonzero(row >= tau)[0]
        if upper:
            hit = hit[hit > r]
        hit = hit[np.lexsort((hit, -row[hit]))]
        ids.append(hit)
        vals.append(row[hit])
        offs.append(offs[-1] + hit.size)
    return np.array(offs, np.int64), np.concatenate(ids).astype(np.int64), np.concatenate(vals).astype(np.float32)


def _busy_value(scores):
    """A high score value that many pairs attain exactly: the threshold then cuts through a run of equal scores."""
    vals, counts = np.unique(scores[scores > 8000], return_counts=True)
    return float(vals[np.argmax(counts)])


def test_rankings_are_identical_for_every_storage(tied):
    from mdir_amd import ops, search
    ordered = np.take_along_axis(tied.want, tied.rank, axis=1)
    for k in KS:                                              # the k-th place lies inside a run of equal scores (a property of the data)
        assert (ordered[:, k - 1] == ordered[:, k]).mean() >= 0.1, k
    for storage in ("f32", "f16", "i8"):
        ix = ops.DescriptorIndex(tied.rows, "ND", storage=storage)
        try:
            sc = ix.scores(tied.queries, "ND")
            same(sc, tied.want, (storage, "scores"))
            np.testing.assert_array_equal(ops.rank_full(sc).cpu().numpy(), tied.rank, err_msg=storage)
            for k in KS:
                ids, vals = ops.topk(sc, k)
                np.testing.assert_array_equal(ids.cpu().numpy(), tied.rank[:, :k], err_msg="%s topk %d" % (storage, k))
                same(vals, np.take_along_axis(tied.want, tied.rank[:, :k], axis=1), (storage, "topk", k))
                if storage != "f32":                          # the first stage is exact here, so the shortlist is the exact one
                    res = search.search(ix, tied.rows, tied.queries, k, 1000, "ND", exact=False)
                    np.testing.assert_array_equal(res.ids.cpu().numpy(), tied.rank[:, :k], err_msg="%s search %d" % (storage, k))
                    same(res.scores, np.take_along_axis(tied.want, tied.rank[:, :k], axis=1), (storage, "search", k))
        finally:
            ix.close()


def test_range_search_and_self_join_at_a_tied_threshold(tied):
    from mdir_amd import ops, search
    n = N_TIED
    tau_q, tau_s = _busy_value(tied.want), _busy_value(tied.self_scores)
    assert (tied.want == tau_q).sum() >= 20 and (tied.self_scores == tau_s).sum() >= 200
    want_range = _brute_csr(tied.want, tau_q)
    want_join = _brute_csr(tied.self_scores, tau_s, upper=True)
    assert want_range[1].size > 100 and want_join[1].size > 1000
    ix = ops.DescriptorIndex(tied.rows, "ND", storage="i8")
    try:
        for index in (ix, None):
            route = "exact route" if index is None else "int8 route"
            for got, want in ((search.range_search(index, tied.rows, tied.queries, tau_q, "ND"), want_range),
                              (search.self_join(index, tied.rows, tau_s), want_join)):
                off, ids, vals = _csr(got)
                np.testing.assert_array_equal(off, want[0], err_msg=route)
                np.testing.assert_array_equal(ids, want[1], err_msg=route)
                same(vals, want[2], route)
        # the pruned route is what ran: far fewer candidates than pairs, and no hit missing among them
        stats = ops.join_stats(ix, tied.rows)
        _, count = ops.join_candidates(ix, stats, ix, stats, tau_s, 0, n, symmetric=True, capacity=1 << 22)
        assert want_join[1].size <= count < n * (n - 1) // 2 // 8, (count, want_join[1].size)
        qix = ops.DescriptorIndex(tied.queries, "ND", storage="i8")
        try:
            _, count = ops.join_candidates(qix, ops.join_stats(qix, tied.queries), ix, stats, tau_q, 0, NQ_TIED, capacity=1 << 20)
            assert want_range[1].size <= count < NQ_TIED * n // 8, (count, want_range[1].size)
        finally:
            qix.close()
    finally:
        ix.close()


def test_knn_join_with_the_kth_place_inside_a_run_of_equal_scores(tied):
    from mdir_amd import ops, search
    ix = ops.DescriptorIndex(tied.rows, "ND", storage="i8")
    pruned = {}
    try:
        for k in (1, 10, 64):
            want_ids, want_sc, ordered = tied.top_of_rows(k)
            assert (ordered[:, k - 1] == ordered[:, k]).mean() >= 0.1, k       # ties across the k-th place (a property of the data)
            for index in (ix, None):
                res = search.knn_join(index, tied.rows, k)
                np.testing.assert_array_equal(res.ids.cpu().numpy(), want_ids, err_msg="k=%d %s" % (k, "exact" if index is None else "int8"))
                same(res.scores, want_sc, ("knn_join", k))
                if index is not None:
                    pruned[k] = res.pruned_rows
    finally:
        ix.close()
    assert max(pruned.values()) == N_TIED, pruned             # the int8 route, not its fallback, produced at least one of them
