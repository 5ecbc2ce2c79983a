"""Every ranking route of mdir_amd/csrc/mdx_rank.hip at its size boundaries and on keys built byte by byte, against the numpy
reference of tests/rank_data.py (held against the oracle on the CPU in tests/test_rank_data_host.py).

The caller of mdx_rank_full / mdx_topk cannot see which kernels ran.  Every row of rank_data's tables names the route it is
meant to pin -- SMALL (one workgroup, LDS), PACKED / KV (the tiled passes) under SORT, SELECT and SAMPLED for top-k -- and
each test here first ranks once (that settles the probe verdict the SMALL route depends on), then ASSERTS the row's route
through ``ops.rank_route`` / ``ops.topk_route`` and only then compares the result: a row whose route is not its label fails;
that is how a moved threshold is noticed.  Outputs and workspaces lie in ``memguard`` arenas pre-filled with 0xFF between
guard bands, so an entry left unwritten or a write past the end is seen as well.

The switch matrix runs the rank_full, segments and SORT-route top-k rows once more in a child process per setting
(MDX_SORT_SMALL=0, MDX_SORT_NO_PACK=1, both under MDX_SORT_RANK=ballot: the switches are read once per process), one child at
a time.  As a script: ``python tests/test_gpu_rank_boundaries.py child <setting>`` is that child; ``... routes`` prints
every table row with the route the device reports.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import memguard
import rank_data as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, U32 = np.float32, np.uint32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def guarded(fn, *args, **kw):
    """``ops.fn(*args)`` with its outputs and workspaces in guarded memory pre-filled with 0xFF; the guards are checked."""
    from mdir_amd import ops
    arena = memguard.Arena(DEV)
    with memguard.guarded(ops, arena, fill_out=0xFF, fill_ws=0xFF):
        out = getattr(ops, fn)(*args, **kw)
    torch.cuda.synchronize()
    arena.check()
    return out


@pytest.fixture(scope="module")
def ops():
    """mdir_amd.ops after one ranking call: the probe of the LDS order has its verdict, the route queries see it."""
    from mdir_amd import ops
    ops.rank_full(dev(np.zeros((1, 8), dtype=F32)))
    torch.cuda.synchronize()
    return ops


def rank_full(sc, id_offset=0):
    return host(guarded("rank_full", dev(sc), id_offset))


def topk(sc, k, id_offset=0):
    ids, vals = guarded("topk", dev(sc), k, id_offset)
    return host(ids), host(vals)


def expected_route(label, settings):
    """The ranking route of a row: its table label on the default switches; in a switch child what that child's setting turns
    the label into -- MDX_SORT_SMALL=0 (and ballots) take SMALL away, MDX_SORT_NO_PACK=1 turns PACKED into KV."""
    if label == "SMALL" and ("small0" in settings or "ballot" in settings):
        label = "PACKED"
    if label == "PACKED" and "nopack" in settings:
        label = "KV"
    return label


# ------------------------------------------------------------------------------------------------ the rows, one function each

def run_rank_row(ops, r, settings=()):
    want = expected_route(r.route, settings)
    assert ops.rank_route(r.n) == want, "%s is meant to pin %s, the library takes %s" % (r.name, want, ops.rank_route(r.n))
    sc = R.make(r.name, r.kind, r.nq, r.n)
    R.check_rank(lambda s: rank_full(s, r.id_offset), sc, r.name, r.id_offset)


def run_segment_row(ops, r, settings=()):
    n = sum(r.widths)
    want = expected_route(r.route, settings)
    assert ops.rank_route(n) == want, "%s is meant to pin %s, the library takes %s" % (r.name, want, ops.rank_route(n))
    sc = R.segment_scores(r)
    blocks = [dev(b) for b in R.split_blocks(sc, r.widths)]
    got = host(guarded("rank_full_segments", blocks))
    R.check_rank(lambda s: got, sc, r.name)
    assert np.array_equal(got, rank_full(sc)), "%s: not the ranking of the concatenation" % r.name


def run_topk_row(ops, r, settings=()):
    route = ops.topk_route(r.n, r.nq, r.k)
    assert route == r.route, "%s is meant to pin %s, the library takes %s" % (r.name, r.route, route)
    under = r.n if route == "SORT" else r.k + R.SEL_CAP if route == "SELECT" else None
    if under is not None:
        want = expected_route(r.inner, settings)
        assert ops.rank_route(under) == want, "%s: %s is meant to rank through %s, not %s" % (r.name, route, want, ops.rank_route(under))
    sc = R.make(r.name, r.kind, r.nq, r.n)
    got = topk(sc, r.k, r.id_offset)
    R.check_topk(lambda s, k: got, sc, r.k, r.name, r.id_offset)
    return sc, got


def without_sampling(ops, monkeypatch, r, sc, sampled):
    """The same call with MDX_NO_SAMPLED_TOPK=1 (read per call): another route, the same ids and the same score bits."""
    monkeypatch.setenv("MDX_NO_SAMPLED_TOPK", "1")
    other = ops.topk_route(r.n, r.nq, r.k)
    assert other in ("SELECT", "SORT"), "%s: still %s with MDX_NO_SAMPLED_TOPK=1" % (r.name, other)
    got = topk(sc, r.k, getattr(r, "id_offset", 0))
    monkeypatch.delenv("MDX_NO_SAMPLED_TOPK")
    assert ops.topk_route(r.n, r.nq, r.k) == "SAMPLED"
    assert np.array_equal(got[0], sampled[0]), "%s: ids differ between SAMPLED and %s" % (r.name, other)
    assert np.array_equal(got[1].view(U32), sampled[1].view(U32)), "%s: score bits differ between SAMPLED and %s" % (r.name, other)
    R.check_topk(lambda s, k: got, sc, r.k, r.name + " without sampling", getattr(r, "id_offset", 0))


# ------------------------------------------------------------------------------------------------ in process, default switches

@pytest.mark.parametrize("n", R.RANK_N_SMALL + R.RANK_N_TILED)
def test_rank_full_at_every_boundary(ops, n):
    rows = [r for r in R.RANK_FULL if r.n == n]
    assert len(rows) >= 3
    for r in rows:
        run_rank_row(ops, r)


@pytest.mark.parametrize("r", R.SEGMENTS, ids=[r.name for r in R.SEGMENTS])
def test_rank_full_segments_across_block_borders(ops, r):
    run_segment_row(ops, r)


@pytest.mark.parametrize("r", R.TOPK, ids=[r.name for r in R.TOPK])
def test_topk_on_every_route(ops, monkeypatch, r):
    monkeypatch.delenv("MDX_NO_SAMPLED_TOPK", raising=False)
    sc, got = run_topk_row(ops, r)
    if r.route == "SAMPLED":
        without_sampling(ops, monkeypatch, r, sc, got)


@pytest.mark.parametrize("r", R.SAMPLED_EXACT, ids=[r.name for r in R.SAMPLED_EXACT])
def test_sampled_topk_at_its_candidate_cap(ops, monkeypatch, r):
    """Rows built from the route's own sample columns (rank_data.sampled_candidates; the count is checked on the host): the
    candidate buffer filled to its last slot, one candidate more and fewer than k -- the last two are answered by the in-kernel
    exact select."""
    monkeypatch.delenv("MDX_NO_SAMPLED_TOPK", raising=False)
    assert ops.topk_route(r.n, r.nq, r.k) == r.route == "SAMPLED"
    sc = R.sampled_candidates(r.nq, r.n, r.k, r.ncand)
    got = topk(sc, r.k)
    R.check_topk(lambda s, k: got, sc, r.k, r.name)
    without_sampling(ops, monkeypatch, r, sc, got)


def rank_of(ops, sc, lists):
    pos, got_sc, offsets = guarded("rank_of", dev(sc), lists)
    assert offsets == np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).tolist()
    want_sc = np.concatenate([sc[q, ids] for q, ids in enumerate(lists)] + [np.empty(0, F32)]).astype(F32)
    assert np.array_equal(host(got_sc).view(U32), want_sc.view(U32)), "id_scores are not the listed ids' scores"
    return host(pos)


@pytest.mark.parametrize("r", R.RANK_OF + [R.RANK_OF_ALL, R.RANK_OF_WIDE], ids=lambda r: r.name)
def test_rank_of_at_the_sweep_and_tile_boundaries(ops, r):
    sc, lists = R.position_case(r)
    R.check_positions(lambda s, l: rank_of(ops, s, l), sc, lists, r.name)


def test_rank_count_over_two_shards(ops):
    """Counts over columns [0, a) at id_offset 0 plus counts over [a, n) at id_offset a are the positions in the whole row; a run
    of ties lies across the cut and its members are listed."""
    r, a = R.RANK_COUNT_SHARDS
    sc, lists = R.position_case(r, cut=a)
    flat = np.concatenate(lists)
    assert a - 1 in lists[0] and a in lists[0]
    ref_sc = dev(np.concatenate([sc[q, ids] for q, ids in enumerate(lists)]).astype(F32))
    ref_ids, off = dev(flat), dev(np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).astype(np.int64))

    def positions(s, l):
        cnt = torch.zeros(len(flat), dtype=torch.int64, device=DEV)
        ops.rank_count_(cnt, dev(s[:, :a]), 0, ref_sc, ref_ids, off)
        ops.rank_count_(cnt, dev(s[:, a:]), a, ref_sc, ref_ids, off)
        return host(cnt)
    R.check_positions(positions, sc, lists, r.name)


@pytest.mark.parametrize("r", R.RANK_POSITIONS, ids=lambda r: r.name)
def test_rank_positions_at_the_rows_per_block_boundary(ops, r):
    """The ranking is the first n columns of a wider matrix (ld = n + 3: rows 1 and 2 start at 8 bytes mod 16 or not, by n);
    ids that occur only beyond column n, or nowhere, give -1."""
    ranks, lists = R.lookup_case(r)
    wide = dev(ranks)
    pos, offsets = guarded("rank_positions", wide[:, :r.n], lists)
    want = np.concatenate(R.reference_lookup(ranks[:, :r.n], lists))
    assert offsets[-1] == len(want) and np.array_equal(host(pos), want), r.name
    assert (want == -1).sum() >= 4 and (want >= 0).sum() >= 500


# ------------------------------------------------------------------------------------------------ the switch matrix

SETTINGS = {
    "small0": {"MDX_SORT_SMALL": "0"},
    "nopack": {"MDX_SORT_NO_PACK": "1"},
    "small0+nopack+ballot": {"MDX_SORT_SMALL": "0", "MDX_SORT_NO_PACK": "1", "MDX_SORT_RANK": "ballot"},
}


def child(setting):
    from mdir_amd import ops as the_ops
    t0 = time.time()
    settings = tuple(setting.split("+"))
    the_ops.rank_full(dev(np.zeros((1, 8), dtype=F32)))
    torch.cuda.synchronize()
    for key, value in SETTINGS[setting].items():
        assert os.environ.get(key) == value, (key, os.environ.get(key))
    seen = set()
    for r in R.RANK_FULL:
        run_rank_row(the_ops, r, settings)
        seen.add(the_ops.rank_route(r.n))
    for r in R.SEGMENTS:
        run_segment_row(the_ops, r, settings)
    for r in R.TOPK:
        if r.route == "SORT":
            run_topk_row(the_ops, r, settings)
    want = {"small0": {"PACKED"}, "nopack": {"SMALL", "KV"}, "small0+nopack+ballot": {"KV"}}[setting]
    assert seen == want, (seen, want)
    print("RANK-BOUNDARIES-OK %s routes=%s seconds=%.1f" % (setting, "+".join(sorted(seen)), time.time() - t0))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_tables_under_the_sort_switches(setting):
    """MDX_SORT_SMALL=0: the tiled packed passes for every n <= 8192 too; MDX_SORT_NO_PACK=1: (key, id) words for every n above
    the one-workgroup sort; both with ballots: (key, id) words for every n.  One child at a time."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MDX_SORT_") and k != "MDX_NO_SAMPLED_TOPK"}
    env.update(SETTINGS[setting])
    t0 = time.time()
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "child", setting], env=env, text=True, capture_output=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the child for %s did not finish in %d s: %s" % (setting, e.timeout, (e.stderr or b"")[-3000:]))
    print("child %s: %.1f s" % (setting, time.time() - t0))
    assert proc.returncode >= 0, "the child for %s died on signal %d: %s" % (setting, -proc.returncode, proc.stderr[-3000:])
    assert proc.returncode == 0 and "RANK-BOUNDARIES-OK " + setting in proc.stdout, (proc.stdout[-2000:], proc.stderr[-3000:])
    print(proc.stdout.strip().splitlines()[-1])


def print_routes():
    """Every table row with the route the device reports for it (what profiles/r15_rank_boundaries.md records)."""
    from mdir_amd import ops as the_ops
    the_ops.rank_full(dev(np.zeros((1, 8), dtype=F32)))
    torch.cuda.synchronize()
    print("| row | nq | label | reported |\n|---|---|---|---|")
    for r in R.RANK_FULL:
        print("| %s | %d | %s | %s |" % (r.name, r.nq, r.route, the_ops.rank_route(r.n)))
    for r in R.SEGMENTS:
        print("| %s | %d | %s | %s |" % (r.name, r.nq, r.route, the_ops.rank_route(sum(r.widths))))
    for r in R.TOPK + R.SAMPLED_EXACT:
        route = the_ops.topk_route(r.n, r.nq, r.k)
        under = r.n if route == "SORT" else r.k + R.SEL_CAP if route == "SELECT" else None
        label = {"SORT": "SORT-trimmed/", "SELECT": "SELECT/", "SAMPLED": "SAMPLED"}[r.route] + ("-" + r.inner if r.inner == "fallback" else r.inner)
        print("| %s | %d | %s | %s |" % (r.name, r.nq, label, {"SORT": "SORT-trimmed/", "SELECT": "SELECT/", "SAMPLED": "SAMPLED"}[route]
                                         + (the_ops.rank_route(under) if under else "-fallback (by construction)" if r.inner == "fallback" else "")))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "child":
        child(sys.argv[2])
    elif sys.argv[1] == "routes":
        print_routes()
