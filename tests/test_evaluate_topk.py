"""compute_map_topk / compute_map_and_print_topk (mdir_amd/evaluate.py): the evaluation of top-K lists, on the host.

  a. full rankings as heads (K = N) give the reference's outputs, bit for bit, on the 400 reference-generated problems of golden G19
     and on G8 (the fixtures, the generators and the expected values are those tests/test_evaluate.py reads);
  b. truncated heads against a restatement written as plain loops over the head (it shares nothing with ``_Positions``);
  c. the protocol dispatch is ``_evaluate``'s.
"""
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mdir_amd import evaluate as E

NAN = float("nan")


def same(got, want, what=""):
    """Bit for bit, NaN where a NaN is due."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=str(what))


# ------------------------------------------------------------------------------------------- a. full rankings: the reference

def _generators():
    sys.path.insert(0, GOLDEN)
    try:
        from make_golden import fuzz_map_case, fuzz_revisited_case
    finally:
        sys.path.remove(GOLDEN)
    return fuzz_map_case, fuzz_revisited_case


def _heads(ranks, extra=0):
    """[N, Q] ranking -> [Q, N + extra] heads, the tail padded with -1."""
    heads = np.ascontiguousarray(ranks.T).astype(np.int64)
    return np.concatenate([heads, np.full((heads.shape[0], extra), -1, dtype=np.int64)], axis=1)


def test_full_rankings_reproduce_the_reference_g19():
    fuzz_map_case, fuzz_revisited_case = _generators()
    g = np.load(os.path.join(GOLDEN, "g19_map_fuzz.npz"))
    errors = 0
    for seed in range(300):
        ranks, gnd, kappas = fuzz_map_case(seed)
        n = ranks.shape[0]
        if "error_%d" % seed in g:
            errors += 1
            with pytest.raises(BaseException) as caught:
                E.compute_map_topk(_heads(ranks), copy.deepcopy(gnd), n, list(kappas))
            assert type(caught.value).__name__ == str(g["error_%d" % seed][0]), seed
            continue
        for extra in (0, 3):                                   # K = N and K > N
            heads = _heads(ranks, extra)
            if seed % 2:
                heads = torch.from_numpy(heads)                # a host tensor is a host array
            mAP, aps, pr, prs = E.compute_map_topk(heads, copy.deepcopy(gnd), n, list(kappas))
            same(mAP, g["map_%d" % seed][0], seed)
            same(aps, g["aps_%d" % seed], seed)
            same(pr, g["pr_%d" % seed], seed)
            same(np.asarray(prs).reshape(g["prs_%d" % seed].shape), g["prs_%d" % seed], seed)
    assert 0 < errors < 100
    for seed in range(100):
        ranks, gnd = fuzz_revisited_case(1000 + seed)
        name = "roxford5k" if seed % 2 else "rparis6k"
        if "rev_error_%d" % seed in g:
            with pytest.raises(BaseException) as caught, contextlib.redirect_stdout(io.StringIO()):
                E.compute_map_and_print_topk(name, _heads(ranks), copy.deepcopy(gnd), ranks.shape[0])
            assert type(caught.value).__name__ == str(g["rev_error_%d" % seed][0]), seed
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            avg, per = E.compute_map_and_print_topk(name, _heads(ranks, seed % 3), copy.deepcopy(gnd), ranks.shape[0])
        assert set(avg) == {"map_easy", "map_medium", "map_hard"} and set(per) == {"ap_easy", "ap_medium", "ap_hard"}
        for k in avg:
            same(avg[k], g["rev_%s_%d" % (k, seed)][0], (k, seed))
        for k in per:
            same(per[k], g["rev_%s_%d" % (k, seed)], (k, seed))


def test_full_rankings_reproduce_the_reference_g8(golden, capsys):
    from oracle import oracle as O
    g = golden("g8_map.npz")
    rk, gnd = g["ranks"].astype(np.int64), json.loads(bytes(g["gnd_json"]).decode())
    n = rk.shape[0]
    avg, per = E.compute_map_and_print_topk("roxford5k", _heads(rk), gnd, n)
    assert set(avg) == {"map_easy", "map_medium", "map_hard"} and set(per) == {"ap_easy", "ap_medium", "ap_hard"}
    for lvl in ("easy", "medium", "hard"):
        assert avg["map_" + lvl] == float(g["rox_map_" + lvl])
        same(per["ap_" + lvl], g["rox_ap_" + lvl])
    # ... and prints the reference's two lines, then the label recall
    ref = io.StringIO()
    with contextlib.redirect_stdout(ref):
        want = E.compute_map_and_print("roxford5k", rk, gnd)
    lines = capsys.readouterr().out.splitlines()
    assert lines[:2] == ref.getvalue().splitlines() and len(lines) == 3
    assert lines[2] == ">> roxford5k: top-%d label recall E: 100.0, M: 100.0, H: 100.0" % n
    assert avg == want[0]
    medium = O.protocol_gnd(gnd, "medium")
    got, want = E.compute_map_topk(_heads(rk, 5), medium, n, [1, 5, 10]), E.compute_map(rk, medium, [1, 5, 10])
    for a, b in zip(got, want):
        same(a, b)
    assert E.compute_map_and_print_topk("oxford5k", _heads(rk), gnd, n) is None          # SURVEY.md quirk Q10, as the reference


# ----------------------------------------------------------------------------------------------- b. truncation: plain loops

def restated_terms(ranking, ok, junk, n):
    """The full ranking's AP as the reference adds it up: ``[(position, adjusted position, term)]`` of every positive in ranking
    order, and ``len(ok)``.  Sets, loops and the reference's expressions (evaluate.py:3-37, :85-100)."""
    okset = {int(i) for i in ok if 0 <= int(i) < n}
    junkset = {int(i) for i in junk if 0 <= int(i) < n}
    nok = len(ok)
    terms, njunk, j = [], 0, 0
    for p, row in enumerate(ranking):
        row = int(row)
        if row < 0:
            continue
        if row in okset:
            rank = p - njunk                                  # junk strictly before p
            p0 = 1.0 if rank == 0 else float(j) / rank
            p1 = float(j + 1) / (rank + 1)
            terms.append((p, rank, (p0 + p1) * (1.0 / nok) / 2.0))
            j += 1
        if row in junkset:
            njunk += 1
    return terms, nok


def restated_query(head, ranking, ok, junk, n, kappas):
    """(ap, [P@kappa], found, rows, depth) of one query's ``head`` -- a prefix of ``ranking`` plus padding -- by the issue's rule."""
    full, nok = restated_terms(ranking, ok, junk, n)
    mine, _ = restated_terms(head, ok, junk, n)
    ap = 0.0
    for _, _, term in mine:
        ap += term
    junkset = {int(i) for i in junk if 0 <= int(i) < n}
    valid = sum(1 for row in head if row >= 0)
    depth = valid - sum(1 for row in head if int(row) in junkset)
    rows = len({int(i) for i in ok if 0 <= int(i) < n})
    prs = []
    for kappa in kappas:
        if rows and len(mine) == rows or kappa <= depth:
            kq = min(max(rank for _, rank, _ in full) + 1, kappa) if full else kappa
            prs.append(sum(1 for _, rank, _ in full if rank + 1 <= kq) / kq)     # the FULL ranking's value
        else:
            prs.append(NAN)
    return ap, prs, len(mine), rows, depth


N, Q = 200, 12
DEPTHS = (1, 2, 7, 50, 199, 200, 250)
KAPPAS = [1, 5, 10, 60]


def _problem(seed):
    """Rankings [Q, N] and an old-protocol gnd with the cases of the issue built in: query 0 has a junk id at the very top and a
    positive right behind it, query 1 lists a positive twice and ids outside [0, N), query 2 has all its positives in its last ten
    places, query 3 has no positives, query 4 one id that is both ok and junk, query 5 no junk key."""
    rng = np.random.default_rng(seed)
    ranks = np.stack([rng.permutation(N) for _ in range(Q)]).astype(np.int64)
    gnd = []
    for q in range(Q):
        ok = ranks[q, rng.choice(N, int(rng.integers(1, 9)), replace=False)]
        junk = ranks[q, rng.choice(N, int(rng.integers(0, 6)), replace=False)]
        gnd.append({"ok": ok, "junk": junk})
    gnd[0] = {"ok": ranks[0, [1, 4, 30, 120]], "junk": ranks[0, [0, 3, 100]]}
    gnd[1] = {"ok": np.array([ranks[1, 2], ranks[1, 2], N, N + 7, -1, ranks[1, 60]]), "junk": np.array([ranks[1, 0], ranks[1, 0], -5, 10 * N])}
    gnd[2] = {"ok": ranks[2, -10:-4], "junk": ranks[2, [5]]}
    gnd[3] = {"ok": np.empty(0, dtype=np.int64), "junk": ranks[3, :3]}
    gnd[4] = {"ok": ranks[4, [2, 9]], "junk": ranks[4, [2, 5]]}
    gnd[5] = {"ok": ranks[5, [0, 40, 150]].tolist()}
    return ranks, gnd


def _head(ranks, k):
    return _heads(ranks.T, max(0, k - N))[:, :k].copy()


@pytest.mark.parametrize("seed", (0, 1))
def test_truncation_against_the_restatement(seed):
    ranks, gnd = _problem(seed)
    full = E.compute_map(ranks.T, gnd, KAPPAS)
    previous = np.zeros(Q)
    for k in DEPTHS:
        heads = _head(ranks, k)
        assert heads.shape == (Q, k) and ((heads[:, N:] == -1).all() if k > N else (heads >= 0).all())
        res = E.compute_map_topk(heads, gnd, N, KAPPAS)
        m, aps, pr, prs = res
        assert set(res.stats) == {"found", "rows", "depth"}
        for q in range(Q):
            junk = gnd[q].get("junk", [])
            if len(gnd[q]["ok"]) == 0:
                assert np.isnan(aps[q]) and np.isnan(prs[q]).all()
                continue
            ap, want_prs, found, rows, depth = restated_query(heads[q], ranks[q], gnd[q]["ok"], junk, N, KAPPAS)
            assert aps[q] == ap, (k, q)
            same(prs[q], want_prs, (k, q))
            assert (res.stats["found"][q], res.stats["rows"][q], res.stats["depth"][q]) == (found, rows, depth), (k, q)
            # the partial sum of the FULL ranking's terms over the positives at positions below K
            terms, _ = restated_terms(ranks[q], gnd[q]["ok"], junk, N)
            partial = 0.0
            for p, _, term in terms:
                if p < k:
                    partial += term
            assert aps[q] == partial, (k, q)
            # P@kappa: the full ranking's value wherever it is determined, NaN elsewhere
            for j, kappa in enumerate(KAPPAS):
                if kappa <= depth or (rows and found == rows):
                    assert prs[q, j] == full[3][q, j], (k, q, kappa)
                else:
                    assert np.isnan(prs[q, j]), (k, q, kappa)
        live = ~np.isnan(aps)
        assert (aps[live] >= previous[live]).all() and (aps[live] >= 0).all() and (aps[live] <= 1).all()
        previous = np.where(live, aps, previous)
        # the means: queries in order over the live ones; P@kappa skips what is undetermined, as nanmean does
        total = 0.0
        for q in np.flatnonzero(live):
            total += aps[q]
        assert m == total / live.sum()
        for j in range(len(KAPPAS)):
            col = prs[live, j]
            known, count = 0.0, 0
            for v in col:
                if not np.isnan(v):
                    known, count = known + v, count + 1
            assert (pr[j] == known / count) if count else np.isnan(pr[j])
        if k >= N:                                             # from K = N on: the full ranking's outputs, bit for bit
            for a, b in zip(res, full):
                same(a, b, k)
    # the cases the problem was built for
    at7 = E.compute_map_topk(_head(ranks, 7), gnd, N, KAPPAS)
    assert at7.stats["depth"][0] == 5 and at7.stats["found"][0] == 2              # junk at positions 0 and 3 of query 0's head
    assert at7[1][0] == E.compute_ap([0, 2], 4)                                    # its positives move up to 0 and 2
    assert at7.stats["rows"][1] == 2 and at7.stats["found"][1] == 1 and at7.stats["depth"][1] == 6
    assert at7[1][2] == 0.0 and at7.stats["found"][2] == 0                         # no positive in the head: AP 0.0, nothing raised
    assert np.isnan(at7[3][2, 2:]).all() and (at7[3][2, :2] == 0.0).all()          # junk at 5: kappa 10, 60 > depth 6; kappa 1, 5 determined
    assert at7.stats["found"][4] == 1 and at7.stats["depth"][4] == 5
    assert np.isnan(at7[1][3])


def test_padding_inside_short_heads():
    """A head with fewer valid entries than K (an inverted file that scanned fewer candidates): the padding holds no position."""
    ranks, gnd = _problem(2)
    short = _head(ranks, 7)
    short[:, 5:] = -1
    got = E.compute_map_topk(short, gnd, N, KAPPAS)
    want = E.compute_map_topk(_head(ranks, 5), gnd, N, KAPPAS)
    for a, b in zip(got, want):
        same(a, b)
    for key in ("found", "rows", "depth"):
        np.testing.assert_array_equal(got.stats[key], want.stats[key])
    assert got.stats["depth"][0] == 3                                              # five valid entries, two of them junk
    nothing = E.compute_map_topk(np.full((Q, 4), -1, dtype=np.int64), gnd, N, [1])
    assert (nothing.stats["depth"] == 0).all() and (nothing.stats["found"] == 0).all()
    assert (nothing[1][~np.isnan(nothing[1])] == 0.0).all() and np.isnan(nothing[3]).all() and np.isnan(nothing[2]).all()
    with pytest.raises(ValueError, match="heads"):
        E.compute_map_topk(short.astype(np.int32), gnd, N)
    with pytest.raises(ValueError, match="12 queries"):
        E.compute_map_topk(short[:3], gnd, N)


# ------------------------------------------------------------------------------------------------------------ c. protocols

def _revisited(seed):
    rng = np.random.default_rng(seed)
    ranks = np.stack([rng.permutation(N) for _ in range(Q)]).astype(np.int64)
    gnd = []
    for q in range(Q):
        ids = ranks[q, rng.choice(60, 20, replace=False)]                          # labelled rows near the top
        gnd.append({"easy": ids[:5], "hard": ids[5:15], "junk": ids[15:], "bbx": None})
    gnd[1]["easy"] = np.empty(0, dtype=np.int64)
    return ranks, gnd


@pytest.mark.parametrize("k", (10, 40, N))
def test_protocols_are_those_of_evaluate(k, capsys):
    ranks, gnd = _revisited(4)
    heads = _head(ranks, k)
    out = E.compute_map_and_print_topk("rparis6k", heads, gnd, N, kappas=[1, 5, 10])
    avg, per = out
    printed = capsys.readouterr().out.splitlines()
    assert set(avg) == {"map_easy", "map_medium", "map_hard"} and set(per) == {"ap_easy", "ap_medium", "ap_hard"}
    assert set(out.stats) == {"easy", "medium", "hard"}
    with contextlib.redirect_stdout(io.StringIO()) as ref:
        want = E._evaluate("rparis6k", gnd, [1, 5, 10], lambda g, kk: E.compute_map_topk(heads, g, N, kk))
    assert printed[:2] == ref.getvalue().splitlines() and printed[2].startswith(">> rparis6k: top-%d label recall E: " % k)
    for level, ok_keys, junk_keys in E._LEVELS:
        one = E.compute_map_topk(heads, E._protocol_gnd(gnd, ok_keys, junk_keys), N, [1, 5, 10])
        assert avg["map_" + level] == one[0] == want[0]["map_" + level]
        same(per["ap_" + level], one[1])
        same(per["ap_" + level], want[1]["ap_" + level])
        for key in ("found", "rows", "depth"):
            np.testing.assert_array_equal(out.stats[level][key], one.stats[key])
        assert E.label_recall(one.stats) == np.mean((one.stats["found"] / np.maximum(one.stats["rows"], 1))[one.stats["rows"] > 0])
    assert np.isnan(per["ap_easy"][1]) and not np.isnan(per["ap_medium"][1])
    if k == N:
        with contextlib.redirect_stdout(io.StringIO()):
            full = E.compute_map_and_print("rparis6k", ranks.T, gnd, kappas=[1, 5, 10])
        assert avg == full[0]
        for key in per:
            same(per[key], full[1][key])
    # the old protocol
    old = E._protocol_gnd(gnd, ("easy", "hard"), ("junk",))
    out = E.compute_map_and_print_topk("oxford5k", heads, old, N)
    one = E.compute_map_topk(heads, old, N)
    lines = capsys.readouterr().out.splitlines()
    assert set(out[0]) == {"map"} and set(out[1]) == {"ap"} and out[0]["map"] == one[0] and set(out.stats) == {"found", "rows", "depth"}
    same(out[1]["ap"], one[1])
    assert lines[0] == ">> oxford5k: mAP {:.2f}".format(np.around(one[0] * 100, decimals=2)) and len(lines) == 2
    assert lines[1] == ">> oxford5k: top-%d label recall %s" % (k, np.around(E.label_recall(one.stats) * 100, decimals=2))
    assert E.compute_map_and_print_topk("sfm120k", heads, gnd, N) is None
