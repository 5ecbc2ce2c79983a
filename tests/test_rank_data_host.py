"""tests/rank_data.py on the CPU: its reference against the oracle (two independent statements of the ranking order) on every
row of every table, its generators against what they claim, its checkers against numpy rankers that are each wrong in one
way -- every flaw is rejected by a NAMED table row --, and the route queries of the C ABI (host arithmetic: no device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rank_data as R
from conftest import ROOT
from oracle import chain as OC

F32, U32 = np.float32, np.uint32

RANK_ROWS = {r.name: r for r in R.RANK_FULL}
SEG_ROWS = {r.name: r for r in R.SEGMENTS}
TOPK_ROWS = {r.name: r for r in R.TOPK}
POS_ROWS = {r.name: r for r in R.RANK_OF + [R.RANK_OF_ALL, R.RANK_OF_WIDE, R.RANK_COUNT_SHARDS[0]]}


def _scores(name):
    if name in RANK_ROWS:
        r = RANK_ROWS[name]
        return R.make(r.name, r.kind, r.nq, r.n)
    if name in TOPK_ROWS:
        r = TOPK_ROWS[name]
        return R.make(r.name, r.kind, r.nq, r.n)
    return R.segment_scores(SEG_ROWS[name])


# ------------------------------------------------------------------------------------------------ reference against oracle

def _same_as_oracle(sc, name):
    assert np.array_equal(R.reference_rank(sc), OC.rank_full(sc)), name


def test_reference_equals_the_oracle_on_every_ranking_row():
    assert len(RANK_ROWS) == len(R.RANK_FULL) and len(TOPK_ROWS) == len(R.TOPK)          # names are unique
    for name in list(RANK_ROWS) + list(SEG_ROWS):
        _same_as_oracle(_scores(name), name)


def test_reference_equals_the_oracle_on_every_topk_row():
    for r in R.TOPK:
        sc = _scores(r.name)[:1]                   # the rows of a case are drawn alike: one of them (the largest are 262144 wide)
        _same_as_oracle(sc, r.name)
        ids, vals = R.reference_topk(sc, r.k)
        assert np.array_equal(vals.view(U32), sc[0, ids[0]].view(U32)[None])
    for r in R.SAMPLED_EXACT:
        _same_as_oracle(R.sampled_candidates(1, r.n, r.k, r.ncand), r.name)


def test_reference_positions_equal_the_oracle_on_every_position_row():
    for r in R.RANK_OF + [R.RANK_OF_ALL, R.RANK_COUNT_SHARDS[0]]:
        sc, lists = R.position_case(r, R.RANK_COUNT_SHARDS[1] if r is R.RANK_COUNT_SHARDS[0] else None)
        assert [len(ids) for ids in lists] == list(r.lengths)
        want = R.reference_positions(sc, lists)
        for q, ids in enumerate(lists):
            assert np.array_equal(want[q], OC.rank_of(sc[q], ids)), (r.name, q)
    sc, lists = R.position_case(R.RANK_OF_WIDE)
    want = R.reference_positions(sc, lists)
    for q in range(0, R.RANK_OF_WIDE.nq, 64):       # (both sides count here; the oracle sorts: a sample of the 2049 queries)
        assert np.array_equal(want[q], OC.rank_of(sc[q], lists[q])), q
    full = R.reference_rank(sc[:8])
    assert all(full[q, want[q][0]] == lists[q][0] for q in range(8))


def test_key_round_trips_through_the_oracle():
    pool = R.ALL_BYTE_POOL
    key = R.desc_key(pool)
    assert [OC.desc_key(v) for v in pool[:256]] == key[:256].tolist()                     # finite, every byte value in every byte
    finite = ~np.isnan(pool)
    assert [OC.desc_key(v) for v in pool[finite]] == key[finite].tolist()
    assert (key[~finite] == R.NAN_KEY).all() and (~finite).sum() == 4 and OC.desc_key(float("nan")) == R.NAN_KEY
    back = R.key_to_float(key[finite])
    zero = pool[finite] == 0
    assert np.array_equal(back.view(U32)[~zero], pool[finite].view(U32)[~zero]) and (back.view(U32)[zero] == 0).all()     # -0 comes back as +0
    assert np.array_equal(R.desc_key(R.key_to_float(key)), key)
    for bad in (0, 0x007FFFFE, 0x80000000, 0xFF800001, 0xFFFFFFFE):
        with pytest.raises(ValueError, match="no float has key"):
            R.key_to_float(np.array([bad]))
    for good in (0x007FFFFF, 0x7FFFFFFF, 0x80000001, 0xFF800000, 0xFFFFFFFF):
        assert R.desc_key(R.key_to_float(np.array([good])))[0] == good


# ------------------------------------------------------------------------------------------------ the generators

def _gen(kind, nq=3, n=5000, seed=1):
    return R.KINDS[kind].gen(np.random.default_rng(seed), nq, n)


def test_generators_do_what_they_claim():
    for kind in R.KINDS:
        a, b = _gen(kind), _gen(kind)
        assert a.dtype == F32 and a.shape == (3, 5000) and np.array_equal(a.view(U32), b.view(U32)), kind      # deterministic
    for b in range(4):
        key = R.desc_key(_gen("byte%d" % b))
        x = np.bitwise_xor.reduce(key ^ key[:, :1], axis=1) | np.bitwise_or.reduce(key ^ key[:, :1], axis=1)
        assert (x & ~U32(0xFF << (8 * b)) == 0).all() and (x != 0).all(), b
        assert all(len(np.unique((row >> (8 * b)) & 0xFF)) == 256 for row in key), b
    key = R.desc_key(_gen("bytes_0_3"))
    diff = np.bitwise_or.reduce(key ^ key[:, :1], axis=1)
    assert (diff & U32(0x00FFFF00) == 0).all() and (diff & 0xFF != 0).all() and (diff >> 24 != 0).all()
    assert len(np.unique(R.desc_key(_gen("all_equal")))) == 1
    for kind, at in (("one_differs_0", 0), ("one_differs_4095", 4095), ("one_differs_4096", 4096), ("one_differs_last", 4999)):
        key = R.desc_key(_gen(kind))
        for q in range(3):
            assert np.flatnonzero(key[q] != key[q, (at + 1) % 5000]).tolist() == [at], (kind, q)
        assert key[0, at] < key[0, 1] < key[1, at] < key[2, at] == R.NAN_KEY                # better, worse, NaN
    sc = _gen("all_bytes")
    key = R.desc_key(sc)
    for b in range(4):
        assert all(len(np.unique((row >> (8 * b)) & 0xFF)) == 256 for row in key), b
    bits = sc.view(U32)
    for special in (0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0, 0x80000000) + R.NAN_BITS:
        assert (bits == special).any(axis=1).all(), hex(special)
    assert R.all_bytes(np.random.default_rng(0), 3, 65).shape == (3, 65)
    assert (np.diff(_gen("ascending"), axis=1) > 0).all() and (np.diff(_gen("descending"), axis=1) < 0).all()
    assert all(sorted(np.unique(row)) == [-0.5, 0.5] for row in _gen("two_values"))
    c = _gen("concentrated")
    assert abs(c.mean() - 0.3) < 1e-4 and 5e-5 < c.std() < 2e-4 and len(np.unique(R.desc_key(c) >> 16)) <= 2
    for kind, m in (("few_finite_7", 7), ("few_finite_30", 30), ("few_finite_1500", 1500)):
        sc = _gen(kind)
        assert (np.isfinite(sc).sum(axis=1) == m).all() and np.isnan(sc).sum() == 3 * (5000 - m)
        assert len(np.unique(sc.view(U32)[np.isnan(sc)])) == 4
    assert np.isfinite(R.KINDS["few_finite_7"].gen(np.random.default_rng(0), 2, 3)).all()
    g = _gen("gauss_ties")
    assert np.array_equal(g[:, 0:4995:5], g[:, 1:4996:5]) and len(np.unique(g[0])) > 3900


def test_segment_rows_carry_the_special_values_across_every_border():
    for r in R.SEGMENTS:
        sc = R.segment_scores(r)
        assert sc.shape == (r.nq, sum(r.widths)) and sum(b.shape[1] for b in R.split_blocks(sc, r.widths)) == sc.shape[1]
        if min(w for w in r.widths if w) >= 3:
            for border in np.cumsum(r.widths)[:-1]:
                if border == 0:
                    continue
                left, right = sc[0, border - 3:border], sc[0, border:border + 3]
                for side in (left, right):
                    assert np.isnan(side).sum() == 1 and (side == 0).sum() == 1 and (side == F32(0.125)).sum() == 1
                assert np.signbit(left[left == 0][0]) and not np.signbit(right[right == 0][0])


def test_every_kind_lies_in_every_band_of_the_rank_table():
    """gauss_ties and at least two more kinds per size; every kind on each side of every boundary (in every band between two
    neighbouring ones); each row on the route its size says."""
    sizes = sorted({r.n for r in R.RANK_FULL})
    assert tuple(sizes) == R.RANK_N_SMALL + R.RANK_N_TILED
    for n in sizes:
        kinds = [r.kind for r in R.RANK_FULL if r.n == n]
        assert kinds[0] == "gauss_ties" and len(set(kinds)) == len(kinds) >= 3, n
    edges = (0,) + R.RANK_BOUNDARIES + (sizes[-1],)
    for lo, hi in zip(edges[:-1], edges[1:]):
        have = {r.kind for r in R.RANK_FULL if lo < r.n <= hi}
        need = {k for k in R.ROTATED + ["gauss_ties"] if R.KINDS[k].min_n <= hi}
        assert need <= have, (lo, hi, sorted(need - have))
    assert all(r.route == ("SMALL" if r.n <= 8192 else "PACKED") and r.nq in (1, 3) for r in R.RANK_FULL)
    assert {r.route for r in R.RANK_FULL if r.id_offset > 1 << 32} == {"SMALL", "PACKED"}
    assert any(r.n % 2 and r.nq == 3 for r in R.RANK_FULL)


def test_sampled_candidate_rows_hold_the_count_they_are_built_for():
    """Restating the SAMPLED route's threshold on the host: exactly ``ncand`` columns are at or before the m-th best sample."""
    for r in R.SAMPLED_EXACT:
        sc = R.sampled_candidates(r.nq, r.n, r.k, r.ncand)
        m = R.sampled_threshold_rank(r.n, r.k)
        for q in range(r.nq):
            at = R.sampled_positions(r.n, q)
            assert len(np.unique(at)) == R.TKS_SAMPLES and at.max() < r.n
            comp = (R.desc_key(sc[q]).astype(np.uint64) << np.uint64(32)) | np.arange(r.n, dtype=np.uint64)
            thr = np.sort(comp[at])[m - 1]
            assert int((comp <= thr).sum()) == r.ncand, (r.name, q)
    assert [r.ncand for r in R.SAMPLED_EXACT] == [R.TKS_CAP, R.TKS_CAP + 1, 1023]
    # the restated threshold rank, pinned: max(6 k, 2048) candidates aimed at, m = ceil(that x 4096 / n), at least 9
    assert R.sampled_threshold_rank(262144, 1024) == 96 and R.sampled_threshold_rank(16384, 64) == 512
    assert R.sampled_threshold_rank(20479, 10) == 410 and R.sampled_threshold_rank(1 << 22, 1) == 9


# ------------------------------------------------------------------------------------------------ flawed rankers

def _rank_by(key, tie=None):
    ids = np.broadcast_to(np.arange(key.shape[1]), key.shape)
    return np.stack([np.lexsort(((ids[q] if tie is None else tie[q]), key[q])) for q in range(len(key))]).astype(np.int64)


def flaw_unstable(sc):
    key = R.desc_key(sc)
    return _rank_by(key, -np.broadcast_to(np.arange(key.shape[1]), key.shape))


def flaw_negative_zero_behind(sc):
    key = R.desc_key(sc).astype(np.int64) * 2
    return _rank_by(key + (np.ascontiguousarray(sc).view(U32) == 0x80000000))


def flaw_nan_first(sc):
    key = R.desc_key(sc).astype(np.int64)
    return _rank_by(np.where(key == R.NAN_KEY, -1, key))


def flaw_nan_by_bits(sc):
    key = R.desc_key(sc).astype(np.int64)
    return _rank_by(np.where(key == R.NAN_KEY, (1 << 32) + np.ascontiguousarray(sc).view(U32).astype(np.int64), key))


def flaw_ignores_byte(b):
    def ranker(sc):
        return _rank_by(R.desc_key(sc) & ~U32(0xFF << (8 * b)))
    return ranker


def flaw_topk_tie_order(sc, k):
    ids, _ = R.reference_topk(sc, k)
    key = np.take_along_axis(R.desc_key(sc), ids, axis=1)
    ids = np.stack([np.lexsort((-ids[q], key[q])) for q in range(len(ids))])
    ids = np.take_along_axis(R.reference_topk(sc, k)[0], ids, axis=1)
    return ids, np.take_along_axis(sc, ids, axis=1)


def flaw_topk_last_off_by_one(sc, k):
    rank = R.reference_rank(sc)
    ids = rank[:, :k].copy()
    ids[:, k - 1] = rank[:, k]
    return ids, np.take_along_axis(sc, ids, axis=1)


def flaw_topk_score_of_neighbour(sc, k):
    ids, vals = R.reference_topk(sc, k)
    vals = vals.copy()
    vals[:, k - 1] = np.take_along_axis(sc, R.reference_rank(sc)[:, k:k + 1], axis=1)[:, 0]
    return ids, vals


def flaw_positions_ignore_ids(sc, id_lists):
    key = R.desc_key(sc)
    return np.concatenate([[np.count_nonzero(key[q] < key[q, i]) for i in ids] for q, ids in enumerate(id_lists)] + [np.empty(0)]).astype(np.int64)


RANK_FLAWS = [
    ("unstable", flaw_unstable, "rank_full[2048,gauss_ties]"),
    ("unstable", flaw_unstable, "rank_full[8193,all_equal]"),
    ("-0 behind +0", flaw_negative_zero_behind, "rank_full[4095,all_bytes]"),
    ("-0 behind +0", flaw_negative_zero_behind, "segments[4096+4096]"),
    ("NaN first", flaw_nan_first, "rank_full[4097,few_finite_7]"),
    ("NaN first", flaw_nan_first, "segments[3000+5193]"),
    ("NaN by payload", flaw_nan_by_bits, "rank_full[8193,all_bytes]"),
    ("NaN by payload", flaw_nan_by_bits, "segments[8191+1]"),
    ("ignores byte 0", flaw_ignores_byte(0), "rank_full[6143,byte0]"),
    ("ignores byte 1", flaw_ignores_byte(1), "rank_full[6143,byte1]"),
    ("ignores byte 2", flaw_ignores_byte(2), "rank_full[2047,byte2]"),
    ("ignores byte 3", flaw_ignores_byte(3), "rank_full[8193,byte3]"),
    ("ignores byte 0", flaw_ignores_byte(0), "rank_full[6145,bytes_0_3]"),
    ("ignores byte 3", flaw_ignores_byte(3), "rank_full[6145,bytes_0_3]"),
    ("ignores byte 3", flaw_ignores_byte(3), "rank_full[8192,one_differs_4096]"),
]


@pytest.mark.parametrize("flaw,ranker,name", RANK_FLAWS, ids=["%s@%s" % (f, n) for f, _, n in RANK_FLAWS])
def test_each_wrong_ranker_is_rejected_by_a_named_row(flaw, ranker, name):
    sc = _scores(name)
    R.check_rank(R.reference_rank, sc, name)
    R.check_rank(lambda s: OC.rank_full(s) + 7, sc, name, id_offset=7)
    with pytest.raises(AssertionError, match=r"%s: wrong ranking, first at query \d+, position \d+" % name.replace("[", r"\[").replace("]", r"\]").replace("+", r"\+")):
        R.check_rank(ranker, sc, name)


TOPK_FLAWS = [
    ("tie order", flaw_topk_tie_order, "topk[16384,64,all_equal]", "ids"),
    ("tie order", flaw_topk_tie_order, "topk[40000,1500,two_values]", "ids"),
    ("last off by one", flaw_topk_last_off_by_one, "topk[12289,4096,gauss_ties]", "ids"),
    ("last off by one", flaw_topk_last_off_by_one, "topk[16648,66,gauss_ties]", "ids"),
    ("last off by one", flaw_topk_last_off_by_one, "topk[40000,2000,few_finite_1500]", "ids"),
    ("score of the neighbour", flaw_topk_score_of_neighbour, "topk[20383,1000,gauss_ties]", "score bits"),
]


@pytest.mark.parametrize("flaw,topk,name,what", TOPK_FLAWS, ids=["%s@%s" % (f, n) for f, _, n, _ in TOPK_FLAWS])
def test_each_wrong_topk_is_rejected_by_a_named_row(flaw, topk, name, what):
    r = TOPK_ROWS[name]
    sc = _scores(name)
    R.check_topk(R.reference_topk, sc, r.k, name)
    with pytest.raises(AssertionError, match=r"wrong top-%d %s, first at query" % (r.k, what)):
        R.check_topk(topk, sc, r.k, name)


@pytest.mark.parametrize("name", ["rank_of[4097]", "rank_of[300,arange]", "rank_count[8193,two shards]"])
def test_positions_off_inside_a_tie_run_are_rejected_by_a_named_row(name):
    r = POS_ROWS[name]
    sc, lists = R.position_case(r, R.RANK_COUNT_SHARDS[1] if r is R.RANK_COUNT_SHARDS[0] else None)
    R.check_positions(lambda s, l: np.concatenate(R.reference_positions(s, l)), sc, lists, name)
    with pytest.raises(AssertionError, match=r"wrong position, first at entry \d+ \(query \d+, id \d+\): got \d+, expected \d+"):
        R.check_positions(flaw_positions_ignore_ids, sc, lists, name)


def test_lookup_cases_hold_present_and_absent_ids():
    for r in R.RANK_POSITIONS:
        ranks, lists = R.lookup_case(r)
        assert ranks.shape == (r.nq, r.n + 3) and [len(ids) for ids in lists] == list(r.lengths)
        want = R.reference_lookup(ranks[:, :r.n], lists)
        assert want[0].tolist() == [0, r.n - 1, -1, -1, r.n // 2]
        assert (want[1][5:] >= -1).all() and (want[1] == -1).sum() >= 2 and len(np.unique(lists[1])) == len(lists[1]) == 600
    assert [r.n for r in R.RANK_POSITIONS] == [16383, 16384, 16385]


# ------------------------------------------------------------------------------------------------ the route queries

def _sampled_bytes(n, nq):
    up = lambda x: -(-x // 256) * 256
    nblk = -(-n // 4096)
    return up(nq * 8) + up(nq * 4) + up(nq * nblk * 4) + nq * nblk * 128 * 8 + nq * R.TKS_CAP * 8


def test_topk_route_table(monkeypatch):
    """mdx_topk_route answers every row of the top-k table as the row says, with the workspace mdx_topk is given; a workspace one
    byte below a route's own carve-up moves the call to the next route; MDX_NO_SAMPLED_TOPK is read per call."""
    from mdir_amd import _lib, ops
    monkeypatch.delenv("MDX_NO_SAMPLED_TOPK", raising=False)
    for r in R.TOPK + R.SAMPLED_EXACT:
        assert ops.topk_route(r.n, r.nq, r.k) == r.route, r.name
    rows = {(r.n, r.k): r.route for r in R.TOPK}
    assert rows[(16647, 66)] == "SORT" and rows[(16648, 66)] == "SELECT" and rows[(20383, 1000)] == "SORT" and rows[(20384, 1000)] == "SELECT"
    assert rows[(262143, 1024)] == "SELECT" and rows[(262144, 1024)] == "SAMPLED" and rows[(16383, 63)] == "SORT" and rows[(16384, 64)] == "SAMPLED"
    assert rows[(262400, 1025)] == "SELECT" and ops.topk_route(16384, 1, 65) == "SORT"                    # k <= 1024, 256 k <= n
    # (after: 16384 is too short for the select; at 262144 x 1024 the select's own carve-up is the larger one and does not fit either)
    for n, nq, k, after in ((16384, 3, 64, "SORT"), (262144, 3, 1024, "SORT"), (20479, 1, 10, "SELECT")):
        need = _sampled_bytes(n, nq)
        assert need <= ops.rank_workspace_bytes(n, nq)
        assert ops.topk_route(n, nq, k, need) == "SAMPLED" and ops.topk_route(n, nq, k, need - 1) == after, (n, k)
    monkeypatch.setenv("MDX_NO_SAMPLED_TOPK", "1")
    for r in R.TOPK + R.SAMPLED_EXACT:
        want = r.route if r.route != "SAMPLED" else ("SELECT" if 4 * (r.k + R.SEL_CAP) <= r.n else "SORT")
        assert ops.topk_route(r.n, r.nq, r.k) == want, r.name
    assert {ops.topk_route(r.n, r.nq, r.k) for r in R.TOPK if r.route == "SAMPLED"} == {"SELECT", "SORT"}
    # the select's carve-up: found by bisection between nothing and the ranking workspace, then missed by one byte
    for n, nq, k in ((32768, 3, 4096), (16648, 3, 66)):
        lo, hi = 0, ops.rank_workspace_bytes(n, nq)
        assert ops.topk_route(n, nq, k, hi) == "SELECT" and ops.topk_route(n, nq, k, lo) == "SORT"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if ops.topk_route(n, nq, k, mid) == "SELECT" else (mid, hi)
        assert ops.topk_route(n, nq, k, hi) == "SELECT" and ops.topk_route(n, nq, k, hi - 1) == "SORT"
        assert hi > nq * (k + R.SEL_CAP) * 8 + nq * k * 8 + ops.rank_workspace_bytes(k + R.SEL_CAP, nq)    # candidates, local ids, their sort
    monkeypatch.delenv("MDX_NO_SAMPLED_TOPK")
    assert ops.topk_route(16384, 3, 64) == "SAMPLED"
    h = _lib.lib()
    for bad in ((0, 1, 1, 0), (10, 0, 1, 0), (10, 1, 0, 0), (10, 1, 11, 0), (1 << 32, 1, 1, 0), (10, 65536, 1, 0)):
        assert h.mdx_topk_route(*bad) == -1, bad
    assert b"mdx_topk_route" in h.mdx_last_error()
    with pytest.raises(ValueError):
        ops.topk_route(10, 1, 11)


_ROUTE_CHILD = r"""
import sys
sys.path.insert(0, %r)
from mdir_amd import ops
print("ROUTES", " ".join(ops.rank_route(n) for n in (1, 2048, 8192, 8193, 1 << 24, (1 << 24) + 1)))
"""


@pytest.mark.parametrize("env,want", [
    ({}, "PACKED PACKED PACKED PACKED PACKED KV"),                              # no verdict: ballots, never SMALL
    ({"MDX_SORT_NO_PACK": "1"}, "KV KV KV KV KV KV"),
    ({"MDX_SORT_RANK": "atomic"}, "SMALL SMALL SMALL PACKED PACKED KV"),        # forced: no verdict is asked for
    ({"MDX_SORT_RANK": "atomic", "MDX_SORT_SMALL": "0"}, "PACKED PACKED PACKED PACKED PACKED KV"),
    ({"MDX_SORT_RANK": "ballot", "MDX_SORT_NO_PACK": "1", "MDX_SORT_SMALL": "0"}, "KV KV KV KV KV KV"),
])
def test_rank_route_without_a_probe_verdict(env, want):
    """The switches are read once per process, so each combination gets a process; none of them has ranked anything, so the
    probe has no verdict and mdx_rank_route must not run it: PACKED or KV, never SMALL, unless the atomic form is forced."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MDX_SORT_")}
    proc = subprocess.run([sys.executable, "-c", _ROUTE_CHILD % ROOT], env=dict(clean, **env), text=True, capture_output=True, timeout=300)
    assert proc.returncode == 0 and "ROUTES " + want in proc.stdout, (proc.stdout[-2000:], proc.stderr[-2000:])


def test_rank_route_refuses_what_the_ranking_refuses():
    from mdir_amd import _lib, ops
    h = _lib.lib()
    assert h.mdx_rank_route(0, None) == -1 and h.mdx_rank_route(-5, None) == -1 and h.mdx_rank_route(1 << 32, None) == -1
    assert b"mdx_rank_route" in h.mdx_last_error()
    with pytest.raises(ValueError):
        ops.rank_route(0)
    assert set(_lib.RANK_ROUTES.values()) == {"SMALL", "PACKED", "KV"} and set(_lib.TOPK_ROUTES.values()) == {"SAMPLED", "SELECT", "SORT"}
    text = open(os.path.join(ROOT, "include", "mdx.h")).read()
    for table, prefix in ((_lib.RANK_ROUTES, "MDX_RANK_ROUTE_"), (_lib.TOPK_ROUTES, "MDX_TOPK_ROUTE_")):
        for value, name in table.items():
            assert "#define %s%s %d\n" % (prefix, name, value) in text
