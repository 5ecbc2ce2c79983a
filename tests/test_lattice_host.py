"""The exactly representable grids of tests/lattice.py on a CPU-only box: on every grid the project's own host definitions
-- the fp32 chain oracle, the int8 restatement, the split3 / split2 restatements, the float64 product of the fp16-rounded
operands -- return ``lattice.expected`` bit for bit, so the grids mean what tests/test_gpu_lattice.py assumes; and the
condition ``sum_k |q_k||x_k| < 2^24`` holds for every shape and grid the GPU table runs: a shape that violates it fails
HERE, not silently on the GPU."""
import numpy as np
import pytest

import lattice
from lattice import bits
from oracle import chain as OC
from oracle import oracle as O
from test_i8_host import quantize_np, scores_np

SMALL = [t for t in lattice.TRIPLES if t[0] * t[1] * t[2] <= 1 << 23]      # the chain oracle is a scalar loop


def _same(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def _f16_product(L):
    with np.errstate(over="ignore"):
        q16 = L.queries.astype(np.float16).astype(np.float64)
        x16 = L.db.astype(np.float16).astype(np.float64)
    return (q16 @ x16.T).astype(np.float32)


def _effective(L):
    return L.queries if L.center is None else L.queries - L.center[None, :]


def _split3(L):
    return O.scores_split3(np.ascontiguousarray(L.db.T), np.ascontiguousarray(_effective(L).T)).T


def _split2(L):
    return O.scores_split2(np.ascontiguousarray(L.db.T), np.ascontiguousarray(_effective(L).T)).T


def _conditions(L, split=True):
    """The condition for the plain paths and, on the pieces, for the two split modes."""
    lattice.assert_exact_in_any_order(L.qi, L.xi)
    if split:
        q = _effective(L)
        lattice.assert_exact_in_any_order(lattice.split3_pieces(q), lattice.split3_pieces(L.db))
        lattice.assert_exact_in_any_order(lattice.split2_pieces(q), lattice.split2_pieces(L.db))


# ------------------------------------------------------------------------------------------------ the helper itself

def test_to_grid_and_expected():
    ints, u = lattice.to_grid(np.array([0.0, -0.0, 3 * 2.0 ** -24, -5 * 2.0 ** -20, 2.0 ** -23]))
    assert u == 2.0 ** -24 and ints.tolist() == [0, 0, 3, -80, 2]
    ints, u = lattice.to_grid(np.array([65504.0, -96.0]))
    assert u == 32.0 and ints.tolist() == [2047, -3]
    assert lattice.to_grid(np.zeros(3))[1] == 1.0
    rng = np.random.default_rng(0)
    q, x = rng.integers(-9, 10, (5, 33)), rng.integers(-2047, 2048, (7, 33))
    np.testing.assert_array_equal(lattice.expected(q, x, 0.25), ((q @ x.T) * 0.25).astype(np.float32))     # a true int64 matmul
    assert lattice.pair_magnitude(q, x) == int((np.abs(q) @ np.abs(x).T).max())
    assert lattice.pair_magnitude([q, 2 * q], [x]) == 3 * lattice.pair_magnitude(q, x)
    with pytest.raises(AssertionError):                       # 4096 products of 2047 * 3 reach 2^24
        lattice.assert_exact_in_any_order(np.full((1, 4096), 3), np.full((1, 4096), 2047))
    with pytest.raises(AssertionError):
        lattice.expected(np.full((1, 4096), 3), np.full((1, 4096), 2047), 1.0)
    assert bits(np.float32([-0.0]))[0] == 0x80000000 and bits(lattice.expected(np.zeros((1, 2), np.int64), np.ones((1, 2), np.int64), 1.0))[0, 0] == 0


def test_common_grid_holds_what_it_promises():
    L = lattice.common(700, 64, 90, centred=True)
    for ints in (L.xi, L.qi):
        top = np.abs(ints).max(axis=1)
        assert set(np.unique(top)) == {0, 127}                                # zero rows and rows whose int8 scale is 1
        assert (np.abs(ints) <= 15).sum() + (np.abs(ints) == 127).sum() == ints.size
        assert ((ints != 0).sum(axis=1) == 1).any() and (top == 0).any()      # one-hot rows, zero rows
        assert len(np.unique(ints[top > 0], axis=0)) < (top > 0).sum()           # duplicate rows beyond the zero rows
    assert np.signbit(L.db[L.db == 0]).any() and not np.signbit(L.db[L.db == 0]).all()      # both zeros
    np.testing.assert_array_equal(L.queries - L.center[None, :], L.qi.astype(np.float32))
    assert np.abs(L.center).max() <= 3 and (L.center != 0).any()
    c, s = quantize_np(L.db)
    np.testing.assert_array_equal(c, L.xi)
    assert set(np.unique(s)) == {np.float32(0), np.float32(1)}


# ------------------------------------------------------------------------------------------------ every grid, every host definition

@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("n,d,nq", SMALL)
def test_common_grid_on_every_host_definition(n, d, nq, centred):
    L = lattice.common(n, d, nq, centred=centred)
    _conditions(L)
    want = lattice.expected(L.qi, L.xi, L.uq * L.ux)
    q = _effective(L)
    np.testing.assert_array_equal(q, L.qi.astype(np.float32))
    _same(OC.gemm_nt_chain(q, L.db), want, "chain")
    _same(scores_np(*quantize_np(q), *quantize_np(L.db)), want, "int8")
    _same(_split3(L), want, "split3")
    _same(_split2(L), want, "split2")
    _same(_f16_product(L._replace(queries=q)), want, "fp16")


@pytest.mark.parametrize("n,d,nq", [t for t in lattice.TRIPLES if t not in SMALL])
def test_common_grid_condition_on_the_large_shapes(n, d, nq):
    for centred in (False, True):
        L = lattice.common(n, d, nq, centred=centred)
        _conditions(L)
        lattice.expected(L.qi, L.xi, 1.0)


def test_common_grid_of_the_ranking_tests():
    """The data of the GPU ranking tests: massively tied scores, and -- by the float64 restatement of the join's candidate
    test (test_join_host.candidates_np) -- data on which the int8 route prunes, so that it, not its fallback, is under test."""
    from test_join_host import candidates_np
    for d in (64, 128):
        L = lattice.common(5003, d, 37, seed=5, amp=1, period=29)
        _conditions(L, split=False)
        want = lattice.expected(L.qi, L.xi, 1.0)
        assert 50 <= len(np.unique(want)) <= 1000            # tied scores everywhere: 5003 rows share these values
        lattice.assert_exact_in_any_order(L.xi, L.xi)         # the self-join and the kNN join multiply the rows with themselves
        vals, counts = np.unique(want[want > 8000], return_counts=True)
        tau = float(vals[np.argmax(counts)])                  # a threshold that many pairs attain exactly
        cand = candidates_np(L.queries, L.db, tau)
        hit = want >= tau
        assert (want == tau).sum() >= 20 and not (hit & ~cand).any() and hit.sum() <= cand.sum() < cand.size // 8
        ordered = -np.sort(-want, axis=1)
        for k in (1, 10, 64, 1000):                           # the k-th place lies inside a run of equal scores
            assert (ordered[:, k - 1] == ordered[:, k]).mean() >= 0.1, (d, k)
        part = lattice.expected(L.xi[:640], L.xi, 1.0)        # the first row blocks of the self-join
        ordered = -np.sort(-part, axis=1)
        for k in (1, 10, 64):
            assert (ordered[:, k - 1] == ordered[:, k]).mean() >= 0.1, (d, k)
        cand = candidates_np(L.db[:640], L.db, 16129.0)
        assert not ((part >= 16129) & ~cand).any() and cand.sum() < cand.size // 8


F16_WIDE_CASES = [dict(), dict(swap=True), dict(db_exp=-24), dict(db_exp=-24, q_exp=-24), dict(swap=True, q_exp=-24),
                  dict(db_exp=-34), dict(swap=True, q_exp=-34), dict(db_exp=5, top=True), dict(swap=True, q_exp=5, top=True)]


@pytest.mark.parametrize("case", F16_WIDE_CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()) or "plain")
@pytest.mark.parametrize("n,d,nq", lattice.F16_TRIPLES + [(15, 4096, 8)])
def test_f16_wide_grid(n, d, nq, case):
    L = lattice.f16_wide(n, d, nq, **case)
    lattice.assert_exact_in_any_order(L.qi, L.xi)
    want = lattice.expected(L.qi, L.xi, L.uq * L.ux)
    _same(_f16_product(L), want, "fp16")
    wide = L.queries if case.get("swap") else L.db
    wexp = case.get("q_exp", 0) if case.get("swap") else case.get("db_exp", 0)
    with np.errstate(over="ignore"):
        w16 = wide.astype(np.float16)
    if wexp == -34:                                           # below the subnormal grid: the shard holds 0, 2^-24 or 2^-23
        assert set(np.unique(np.abs(w16.astype(np.float64)) * 2.0 ** 24)) <= {0.0, 1.0, 2.0} and (w16 != 0).any()
    else:                                                     # fp16 values already: all 11 significand bits in use
        np.testing.assert_array_equal(w16.astype(np.float32), wide)
        assert np.abs(np.ldexp(wide.astype(np.float64), -wexp)).max() == 2047
        if wexp == -24:
            tiny = np.abs(wide[wide != 0]) < 2.0 ** -14
            assert tiny.any() and not tiny.all()              # fp16 subnormals and normals side by side
        if case.get("top"):
            assert (wide == 65504).any() and (wide == -65504).any()
    if n * d * nq <= 1 << 23 and wexp == 0 and not case.get("top"):
        _same(OC.gemm_nt_chain(L.queries, L.db), want, "chain")       # fp16 values are fp32 values: the chain agrees
        _conditions(L)                                        # 11 significant bits: two bf16 pieces, one fp16 piece
        _same(_split3(L), want, "split3")
        _same(_split2(L), want, "split2")


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("band", lattice.F16_ROUND_BANDS)
@pytest.mark.parametrize("n,d,nq", lattice.F16_TRIPLES)
def test_f16_round_grid(n, d, nq, band, swap):
    L = lattice.f16_round(n, d, nq, band, swap=swap)
    lattice.assert_exact_in_any_order(L.qi, L.xi)             # the condition, AFTER rounding
    _same(_f16_product(L), lattice.expected(L.qi, L.xi, L.uq * L.ux), "fp16")
    wide = L.queries if swap else L.db
    w16 = wide.astype(np.float16).astype(np.float32)
    moved = wide != w16
    assert moved.sum() > 0.5 * (wide != 0).sum()              # these inputs are not fp16 values
    assert np.isfinite(w16).all()
    nz = wide[wide != 0]
    assert (nz > 0).any() and (nz < 0).any()
    if band == "halfway":                                     # ties went to even, up and down
        tie = np.abs(wide - np.floor(wide)) == 0.5
        assert tie.any() and (w16[tie] > wide[tie]).any() and (w16[tie] < wide[tie]).any()
        assert (w16[tie] % 2 == 0).all()
    elif band == "overflow":
        edge = np.nextafter(np.float32(65520), np.float32(0))
        assert (wide == edge).any() and (w16[wide == edge] == 65504).all()
    else:
        assert (w16[np.abs(wide) <= 2.0 ** -25] == 0).all() and (np.abs(wide) <= 2.0 ** -25).any()
        up = np.abs(wide) == np.nextafter(np.float32(2.0 ** -25), np.float32(1))
        assert up.any() and (np.abs(w16[up]) == 2.0 ** -24).all()


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("n,d,nq", [t for t in lattice.SPLIT_TRIPLES])
def test_split_two_piece_grids(n, d, nq, swap):
    small = n * d * nq <= 1 << 23
    # split3: x = a + b 2^-8
    L = lattice.split3_two_piece(n, d, nq, swap=swap)
    wide = L.queries if swap else L.db
    h, m, l = lattice.split3_pieces(wide)
    assert not l.any() and (h + m == wide).all()
    if wide.size >= 64:
        assert ((h != 0) & (m != 0)).mean() > 0.2              # two live pieces
    lattice.assert_exact_in_any_order(L.qi, L.xi)
    lattice.assert_exact_in_any_order(lattice.split3_pieces(L.queries), lattice.split3_pieces(L.db))
    if small:
        want = lattice.expected(L.qi, L.xi, L.uq * L.ux)
        _same(_split3(L), want, "split3")
        _same(OC.gemm_nt_chain(L.queries, L.db), want, "chain")
        lattice.assert_exact_in_any_order(lattice.split2_pieces(L.queries), lattice.split2_pieces(L.db))
        _same(_split2(L), want, "split2 on the split3 grid")  # 12 significant bits: two fp16 pieces hold them
    # split2: x = a + b 2^-11
    L = lattice.split2_two_piece(n, d, nq, swap=swap)
    wide, narrow = (L.queries, L.db) if swap else (L.db, L.queries)
    h, m = lattice.split2_pieces(wide)
    assert (h + m == wide).all()                              # nothing is left for a third piece
    if wide.size >= 64:
        assert ((h != 0) & (m != 0)).mean() > 0.2
    assert not lattice.split2_pieces(narrow)[1].any()         # one piece: the dropped mm product is zero
    lattice.assert_exact_in_any_order(L.qi, L.xi)
    lattice.assert_exact_in_any_order(lattice.split2_pieces(L.queries), lattice.split2_pieces(L.db))
    if small:
        want = lattice.expected(L.qi, L.xi, L.uq * L.ux)
        _same(_split2(L), want, "split2")                     # the header's formula hh + (hm + mh) / 2^11, summed in float64
        _same(OC.gemm_nt_chain(L.queries, L.db), want, "chain")
        lattice.assert_exact_in_any_order(lattice.split3_pieces(L.queries), lattice.split3_pieces(L.db))
        _same(_split3(L), want, "split3 on the split2 grid")  # 18 significant bits at most: three bf16 pieces hold them


def test_block_exponents_scale_the_result_exactly():
    """The common grid at other block exponents: database x 2^10, queries x 2^-13; the split restatements follow exactly."""
    L = lattice.common(65, 100, 17)
    want = lattice.expected(L.qi, L.xi, 2.0 ** -3)
    M = L._replace(db=L.db * np.float32(2.0 ** 10), queries=L.queries * np.float32(2.0 ** -13))
    _same(_split3(M), want, "split3")
    _same(_split2(M), want, "split2")
    _same(OC.gemm_nt_chain(M.queries, M.db), want, "chain")
