"""Near-duplicate groups (include/mdx.h, "near-duplicate groups"; mdir_amd/search.py duplicate_groups) on the device.

The oracle is a plain sequential union-find, below, over ``oracle.chain.gemm_nt_chain(x, x) >= tau`` compared in fp32 on the upper
triangle.  The chain is pinned bit for bit elsewhere, so the labels must be EQUAL: there is no tolerance anywhere in this file.
Every case runs both routes (the int8 join kernel's candidates, and dense fp32 scores) and ``chunk`` in {128, 256, None} where the
number of rows allows."""
import functools

import numpy as np
import pytest
import torch

from oracle import chain as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


# ------------------------------------------------------------------ the oracle

def components(n, ei, ej):
    """int64 [n]: the smallest id of every row's component under the edges (ei[k], ej[k]): a sequential union-find."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(ei).tolist(), np.asarray(ej).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64)


def edges_of(chain, tau):
    """(i, j), i < j, of the pairs whose fp32 chain reaches the fp32 threshold (NaN never does)."""
    n = chain.shape[0]
    with np.errstate(invalid="ignore"):
        hit = (chain >= F32(tau)) & (np.arange(n)[None, :] > np.arange(n)[:, None])
    return np.nonzero(hit)


def oracle_labels(x, taus):
    chain = OC.gemm_nt_chain(x, x)
    return np.stack([components(x.shape[0], *edges_of(chain, t)) for t in taus])


def chunks_for(n):
    return [c for c in (128, 256) if n > c] + [None]


def run_routes(x, threshold, chunks=None, **kw):
    """duplicate_groups of x on both routes and every chunk: [(route, chunk, Groups)]."""
    from mdir_amd import ops, search
    rows = torch.from_numpy(np.array(x, dtype=F32)).to(DEV)
    index = ops.DescriptorIndex(rows, "ND", storage="i8")
    try:
        out = []
        for route, ix in (("pruned", index), ("exact", None)):
            for chunk in (chunks_for(x.shape[0]) if chunks is None else chunks):
                out.append((route, chunk, search.duplicate_groups(ix, rows, threshold, chunk=chunk, **kw)))
        torch.cuda.synchronize()
        return out
    finally:
        index.close()


def check_everywhere(x, taus, want=None):
    """Every route and chunk gives the oracle's labels for the sequence ``taus``; returns the oracle's labels [T, n]."""
    want = oracle_labels(x, taus) if want is None else want
    n = x.shape[0]
    hooks = sum(n - len(np.unique(w)) for w in want)
    for route, chunk, g in run_routes(x, list(taus)):
        got = g.labels.cpu().numpy()
        assert got.dtype == np.int64 and got.shape == want.shape, (route, chunk, got.shape)
        np.testing.assert_array_equal(got, want, err_msg="%s route, chunk=%s" % (route, chunk))
        assert g.stats["hooks"] == hooks, (route, chunk, g.stats, hooks)
        assert g.stats["chains"] <= g.stats["candidates"] and g.stats["edges"] >= (hooks > 0), (route, chunk, g.stats)
    return want


def lattice(rows):
    return np.ascontiguousarray(np.array(rows, F32))


# ------------------------------------------------------------------ smallest sizes

def test_one_row():
    want = check_everywhere(lattice([[1, 2, 0, 0, 0, 0, 0, 3]]), [1.0])
    assert want.tolist() == [[0]]
    (_, _, g), = run_routes(lattice([[1, 2, 0, 0, 0, 0, 0, 3]]), 14.0, chunks=[None])[:1]
    assert g.labels.tolist() == [0] and g.offsets.tolist() == [0, 1] and g.members.tolist() == [0]       # its own score is no edge


@pytest.mark.parametrize("tau, joined", [(3.0, True), (5.0, False), (4.0, True)], ids=["above", "below", "exactly-at"])
def test_two_rows(tau, joined):
    x = lattice([[1, 2, 0, 0, 0, 0, 0, 0], [2, 1, 0, 0, 0, 0, 0, 0]])              # integers: the chain is exactly 4, and == is a hit
    assert OC.gemm_nt_chain(x, x)[0, 1] == F32(4.0)
    want = check_everywhere(x, [tau])
    assert want.tolist() == [[0, 0] if joined else [0, 1]]


# ------------------------------------------------------------------ shapes of the forest

def path_rows(n, d):
    x = np.zeros((n, d), F32)
    x[np.arange(n), np.arange(n)] = 1
    x[np.arange(n), np.arange(n) + 1] = 1
    return x


@pytest.mark.parametrize("d", [304, 301], ids=["d304-vec", "d301-not-vec"])
@pytest.mark.parametrize("permuted", [False, True], ids=["in-order", "permuted"])
def test_path_graph_is_one_group(d, permuted):
    """x_i = e_i + e_{i+1}: consecutive rows score exactly 1, all others 0 -- one group that spans every chunk boundary, the deepest
    pointer chase.  Permuted, the hooks arrive in arbitrary id order and the label must still be the minimum id."""
    n = 300
    x = path_rows(n, d)
    if permuted:
        x = x[np.random.default_rng(300).permutation(n)]
    want = check_everywhere(x, [1.0])
    assert (want == 0).all()


def test_star_is_one_group():
    """The hub sum_k e_k has the LARGEST id and every leaf e_i scores 1 against it only: every hook contends on one tree."""
    n = 257
    x = np.zeros((n, n - 1), F32)
    x[np.arange(n - 1), np.arange(n - 1)] = 1
    x[n - 1] = 1
    want = check_everywhere(x, [1.0])
    assert (want == 0).all()


@functools.lru_cache(maxsize=None)
def clique_rows():
    rng = np.random.default_rng(500)
    x = rng.standard_normal((500, 128)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(F32)
    where = np.sort(rng.permutation(500)[:400])
    x[where] = x[where[0]]
    x.setflags(write=False)
    return x, where, oracle_labels(x, [0.9])


def test_clique():
    x, where, want = clique_rows()
    assert len(np.unique(want)) == 101 and (want[0, where] == where[0]).all()
    check_everywhere(x, [0.9], want)
    for route, chunk, g in run_routes(x, 0.9):
        assert g.labels.shape == (500,) and g.stats["hooks"] == 399, (route, chunk, g.stats)
        assert g.stats["chains"] <= g.stats["candidates"], (route, chunk, g.stats)
        if route == "pruned":
            assert g.stats["candidates"] >= 400 * 399 // 2, (chunk, g.stats)


def test_clique_through_the_splitting_path():
    """max_candidates = 1000 with 256-row chunks: every chunk of the clique overflows, is split to single 128-row blocks, and
    those run at their counted size -- the same labels."""
    x, where, want = clique_rows()
    (route, _, g), = run_routes(x, 0.9, chunks=[256], max_candidates=1000)[:1]
    assert route == "pruned"
    np.testing.assert_array_equal(g.labels.cpu().numpy(), want[0])
    assert g.stats["hooks"] == 399 and g.stats["candidates"] >= 400 * 399 // 2 and g.stats["chains"] <= g.stats["candidates"]


# ------------------------------------------------------------------ special rows

def test_special_rows():
    rng = np.random.default_rng(68)
    x = rng.standard_normal((68, 64)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(F32)
    x[5, 3] = np.nan
    x[17, 9] = np.inf
    x[30] = 0
    x[41] = 0
    x[41, 2] = F32(2.0 ** -145)
    want = check_everywhere(x, [0.0, 0.25])
    assert want[0, 5] == 5 and (want[0] == 5).sum() == 1 and (want[1] == 5).sum() == 1        # the NaN row: always alone
    chain = OC.gemm_nt_chain(x, x)
    with np.errstate(invalid="ignore"):
        zero_mates = np.nonzero(chain[30] >= 0)[0]
    assert len(zero_mates) > 60 and (want[0, zero_mates] == want[0, 30]).all()                # tau = 0: the zero row joins all of these


# ------------------------------------------------------------------ several thresholds

TAUS = [0.95, 0.9, 0.8, 0.8, 0.5]


def _planted():
    from test_knn_join_host import planted_groups
    return planted_groups(np.random.default_rng(700), 700, 64, 4, 0.3)


def _clustered():
    from test_join_host import _sets
    return _sets(np.random.default_rng(301), "clustered", 301, 100)


def _spread():
    from test_knn_join_host import planted_groups
    return planted_groups(np.random.default_rng(600), 600, 64, 4, 0.6)


@pytest.mark.parametrize("make", [_planted, _clustered, _spread], ids=["planted", "clustered", "spread"])
def test_thresholds_in_one_pass(make):
    from mdir_amd import ops, search
    x = make()
    n = x.shape[0]
    want = check_everywhere(x, TAUS)
    counts = [len(np.unique(w)) for w in want]
    # planted copies at noise 0.3 have a cosine near 1 / sqrt(1.09) = 0.96 and the clustered rows (3 centres of norm 10, noise 0.05
    # per element) one near 0.997: above every threshold, so those two sets have the same groups at each.  The spread set (noise 0.6)
    # has copies near 1 / sqrt(1.36) = 0.86 of their first row and near 1 / 1.36 = 0.74 of each other: its groups differ by level
    assert 1 < counts[4] <= counts[0] <= n and (make is not _spread or counts[4] < counts[2] < counts[0]), counts
    np.testing.assert_array_equal(want[2], want[3])
    order = np.argsort(TAUS, kind="stable")[::-1]                                             # thresholds falling: groups only merge
    for hi, lo in zip(order, order[1:]):
        finer, coarser = want[hi], want[lo]
        assert (coarser[finer] == coarser).all() and (coarser <= finer).all()                 # a finer group lies inside ONE coarser group
    rows = torch.from_numpy(x).to(DEV)
    index = ops.DescriptorIndex(rows, "ND", storage="i8")
    try:
        for t, tau in enumerate(TAUS):
            for ix in (index, None):
                one = search.duplicate_groups(ix, rows, tau)
                np.testing.assert_array_equal(one.labels.cpu().numpy(), want[t])
                assert one.stats["hooks"] == n - counts[t]
    finally:
        index.close()


def test_labels_are_the_components_of_self_join():
    """The product's own pairs, under the host union-find, give the labels."""
    from mdir_amd import ops, search
    x = _planted()
    n = x.shape[0]
    rows = torch.from_numpy(x).to(DEV)
    index = ops.DescriptorIndex(rows, "ND", storage="i8")
    try:
        for tau in (0.9, 0.5):
            off, ids, _ = search.self_join(index, rows, tau)
            i = np.repeat(np.arange(n), np.diff(off.cpu().numpy()))
            want = components(n, i, ids.cpu().numpy())
            assert len(i) > 0
            for ix in (index, None):
                np.testing.assert_array_equal(search.duplicate_groups(ix, rows, tau, chunk=256).labels.cpu().numpy(), want)
    finally:
        index.close()


def test_csr_and_determinism():
    x = _spread()                                             # every row alone at 0.95, groups of up to 4 below: both kinds of group
    n = x.shape[0]
    first = run_routes(x, TAUS, chunks=[256])
    again = run_routes(x, TAUS, chunks=[256])
    for (route, _, g), (_, _, h) in zip(first, again):
        assert torch.equal(g.labels, h.labels), route                                          # two runs: identical labels
        assert g.stats["hooks"] == h.stats["hooks"]
        assert len(g.offsets) == len(g.members) == len(TAUS)
        for t in range(len(TAUS)):
            lab, off, mem = g.labels[t].cpu().numpy(), g.offsets[t].cpu().numpy(), g.members[t].cpu().numpy()
            assert off.dtype == mem.dtype == np.int64 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 1).all()
            assert sorted(mem.tolist()) == list(range(n))
            reps = mem[off[:-1]]
            assert (lab[reps] == reps).all() and (np.diff(reps) > 0).all()                     # ascending label order
            assert set(reps.tolist()) == set(np.nonzero(lab == np.arange(n))[0].tolist())
            np.testing.assert_array_equal(np.diff(off), np.bincount(lab, minlength=n)[reps])      # singletons are present, as groups of one
            for k in range(len(reps)):
                seg = mem[off[k]:off[k + 1]]
                assert (lab[seg] == reps[k]).all() and (np.diff(seg) > 0).all() and seg[0] == reps[k]
        sizes = np.concatenate([np.diff(o.cpu().numpy()) for o in g.offsets])
        assert (sizes == 1).any() and (sizes > 1).any()
    one = run_routes(x, 0.9, chunks=[None])[0][2]
    assert one.labels.dim() == 1 and one.offsets.dim() == 1 and one.members.shape == (n,)
    assert torch.equal(one.labels, first[0][2].labels[1])
