"""Spherical k-means on the device (include/mdx_kmeans.h; mdir_amd/cluster.py): the argmax against ``ops.topk(block, 1)`` bit for
bit, the cluster sums against the fp32 segment chain of tests/kmeans_restatement.py bit for bit, the finish against its float64
restatement at the any-order bound, ``assign`` against ``topk`` of the whole score matrix at every chunk, the loop against the float64
loop on planted data, run-to-run equality of every output, and the three calls under graph capture."""
import numpy as np
import pytest
import torch

import kmeans_restatement as KR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
S = KR.SEGMENT
NAN, INF = F32(np.nan), F32(np.inf)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_bits(got, want, what=""):
    g, w = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in (got, want))
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    np.testing.assert_array_equal(bits(g), bits(w), err_msg=str(what))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ argmax

def _special_rows(k, rng):
    """Rows that meet the tie rule: every score equal; the maximum in the first and the last column; -0 against +0 both ways; -inf
    everywhere and with one finite score; a NaN among finite scores (in the first and in the last column); NaN alone."""
    rows = []
    rows.append(np.full(k, 2.5, F32))
    r = rng.integers(-5, 5, k).astype(F32); r[0] = r[-1] = 9; rows.append(r)
    r = np.full(k, -0.0, F32); r[k // 2] = 0.0; rows.append(r)                  # -0 == +0: the first column wins and keeps its sign
    r = np.full(k, 0.0, F32); r[-1] = -0.0; r[0] = -1.0 if k > 1 else 0.0; rows.append(r)
    rows.append(np.full(k, -INF, F32))
    r = np.full(k, -INF, F32); r[-1] = -3.0e38; rows.append(r)
    r = rng.integers(-5, 5, k).astype(F32); r[0] = NAN; rows.append(r)
    r = rng.integers(-5, 5, k).astype(F32); r[-1] = NAN; r[k // 3] = NAN; rows.append(r)
    rows.append(np.full(k, NAN, F32))
    r = np.full(k, NAN, F32); r[-1] = -INF; rows.append(r)                      # -inf beats NaN
    return np.stack(rows)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 257, 1025, 4099])
def test_argmax_is_the_first_entry_of_topk(k):
    from mdir_amd import ops
    rng = np.random.default_rng(k)
    blocks = [_special_rows(k, rng)]
    for m in (1, 3, 65):
        blocks.append(rng.integers(-3, 4, size=(m, k)).astype(F32))             # few distinct values: ties in every row
        blocks.append(rng.standard_normal((m, k)).astype(F32))
    for block in blocks:
        m = block.shape[0]
        ids, vals = ops.topk(dev(block), 1)
        want_l, want_b = ids.reshape(-1), vals.reshape(-1)
        host_l, host_b = KR.argmax_first(block)
        same_bits(want_l, host_l, ("restatement", k, m))                        # the restatement agrees with the ranking it restates
        same_bits(want_b, host_b, ("restatement", k, m))
        # contiguous; a leading dimension above K on and off the 16-byte grid; a base off the grid
        for ld, shift in ((k, 0), (k + 4 - k % 4, 0), (k + 3, 0), (k, 1)):
            flat = torch.full((m * ld + shift,), 77.0, device=DEV)
            view = flat[shift:].view(m, ld)[:, :k]
            view.copy_(dev(block))
            got_l, got_b = ops.kmeans_argmax(view)
            same_bits(got_l, want_l, (k, m, ld, shift))
            same_bits(got_b, want_b, (k, m, ld, shift))
        only_l, none = ops.kmeans_argmax(dev(block), out_best=False)
        assert none is None
        same_bits(only_l, want_l)
        out = torch.empty(m, device=DEV)
        none, only_b = ops.kmeans_argmax(dev(block), out_labels=False, out_best=out)
        assert none is None and only_b is out
        same_bits(only_b, want_b)


# ------------------------------------------------------------------------------------------------ sums

SIZES = (0, 1, S - 1, S, S + 1, 2 * S + 3)
N_SUMS = sum(SIZES) + 11                                   # eleven rows belong to no cluster


def _clusters(rng, n, sizes, spoil=True):
    """(members, offsets) of clusters of the given sizes over a random subset of the rows, each ascending; ``spoil``: an id of -1 and
    an id of n inside the largest cluster (they are skipped and shift the segment boundaries)."""
    chosen = rng.permutation(n)[:sum(sizes)]
    parts, at = [], 0
    for s in sizes:
        parts.append(np.sort(chosen[at:at + s]).astype(np.int64))
        at += s
    if spoil:
        big = int(np.argmax(sizes))
        parts[big] = np.concatenate([[-1], parts[big][:S], [n], parts[big][S:]])
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


@pytest.mark.parametrize("d", [1, 3, 4, 5, 36, 2052])
def test_sums_are_the_segment_chain(d):
    from mdir_amd import ops
    rng = np.random.default_rng(d)
    n, k = N_SUMS, len(SIZES)
    rows = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-6, 6, (n, 1)))).astype(F32)      # magnitudes apart: the order shows
    members, offsets = _clusters(rng, n, SIZES)
    assert len(members) <= n and (members == -1).sum() == 1 and (members == n).sum() == 1
    want = KR.sums32(rows, members, offsets, k)
    assert not want[0].any() and np.array_equal(want[1], rows[members[offsets[1]]] + F32(0))
    if d > 1:
        shuffled = KR.sums32(rows, members, offsets, k, segment=S // 2)
        assert not np.array_equal(shuffled, want)                                              # the data can tell one order from another
    m_t, o_t = dev(members), dev(offsets)
    same_bits(ops.kmeans_sums(dev(rows), m_t, o_t, k), want, ("contiguous", d))
    # a leading dimension above d (on the 16-byte grid and off it) and a base off the grid
    for ld, shift in ((d + 4 - d % 4, 0), (d + 1, 0), (d + 4 - d % 4, 1), (d, 3)):
        flat = torch.full((n * ld + shift,), 77.0, device=DEV)
        view = flat[shift:].view(n, ld)[:, :d]
        view.copy_(dev(rows))
        same_bits(ops.kmeans_sums(view, m_t, o_t, k), want, (d, ld, shift))
    # one cluster with every row in it
    every = np.arange(n, dtype=np.int64)
    one = ops.kmeans_sums(dev(rows), dev(every), dev(np.array([0, n], np.int64)), 1)
    same_bits(one, KR.sums32(rows, every, [0, n], 1), ("K = 1", d))
    # offsets beyond the members are clamped; a cluster that ends before it starts is empty
    wild = np.array([-5, 3, 2, n + 9], np.int64)
    same_bits(ops.kmeans_sums(dev(rows), dev(every), dev(wild), 3), KR.sums32(rows, every, wild, 3), ("clamped", d))


def test_sums_of_many_small_clusters():
    """More clusters than one thread of the offset scan owns a single one of (K > 1024), most of them empty or tiny."""
    from mdir_amd import ops
    rng = np.random.default_rng(8)
    n, d, k = 3000, 6, 2500
    rows = rng.standard_normal((n, d)).astype(F32)
    labels = rng.integers(0, k, n)
    labels[:700] = 1777                                                                        # one cluster of three segments among them
    members, offsets = KR.csr(labels, k)
    same_bits(ops.kmeans_sums(dev(rows), dev(members), dev(offsets), k), KR.sums32(rows, members, offsets, k))


# ------------------------------------------------------------------------------------------------ finish

@pytest.mark.parametrize("d", [1, 5, 256, 257, 2052])
def test_finish_within_the_any_order_bound(d):
    from mdir_amd import ops
    rng = np.random.default_rng(d)
    k = 7
    sums = (rng.standard_normal((k, d)) * np.exp(rng.uniform(-3, 8, (k, 1)))).astype(F32)
    sums[2] = 0
    sums[5] = F32(-0.0)
    prev = rng.standard_normal((k, d)).astype(F32)
    for previous in (prev, None):
        want = KR.finish64(sums, 1e-6, previous)
        got = ops.kmeans_finish(dev(sums), 1e-6, None if previous is None else dev(previous)).cpu().numpy()
        err = np.abs(got.astype(np.float64) - want)
        tol = KR.finish_tolerance(want, d)
        print("d=%d previous=%s: worst |got - want| / bound = %.3f" % (d, previous is not None, float((err[tol > 0] / tol[tol > 0]).max())))
        assert (err <= tol).all()
        for row in (2, 5):                                                                     # a zero row: the previous centroid's bits, or +0
            same_bits(got[row], prev[row] if previous is not None else np.zeros(d, F32))
    plain = ops.kmeans_finish(dev(sums), 0.0, dev(prev))                                       # eps = 0 is legal
    want = KR.finish64(sums, 0.0, prev)
    assert (np.abs(plain.cpu().numpy().astype(np.float64) - want) <= KR.finish_tolerance(want, d)).all()
    same_bits(ops.kmeans_finish(dev(sums), 0.0, dev(prev)), plain)                             # and a second run returns the same bits


# ------------------------------------------------------------------------------------------------ assign

def _unit(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def test_assign_is_topk_of_the_scores_at_every_chunk():
    from mdir_amd import cluster, ops
    rng = np.random.default_rng(1)
    n, k, d = 1000, 70, 36
    rows, cents = dev(_unit(rng, n, d)), _unit(rng, k, d)
    cents[11] = cents[3]                                                                       # two identical centroids: a tie in every row
    cents = dev(cents)
    index = ops.DescriptorIndex(cents, "ND")
    ids, vals = ops.topk(index.scores(rows, "ND"), 1)
    two = ops.topk(index.scores(rows, "ND"), 2)[1]
    index.close()
    assert not bool((ids == 11).any())
    for chunk in (1, 7, n, None):
        labels, best = cluster.assign(cents, rows, chunk=chunk)
        same_bits(labels, ids.reshape(-1), chunk)
        same_bits(best, vals.reshape(-1), chunk)
    # the labelled modes are handed through to scores.  Their scores lie within 2e-6 of the chain's (include/mdx.h, MDX_F32_SPLIT3 /
    # _SPLIT2), so the best score moves by at most that, and a label only where the chain's two best scores are within twice that
    gap = (two[:, 0] - two[:, 1]).cpu().numpy()
    for mode in ("split3", "split2"):
        labels, best = cluster.assign(cents, rows, chunk=300, compute=mode)
        assert float((best - vals.reshape(-1)).abs().max()) <= 2e-6
        moved = (labels != ids.reshape(-1)).cpu().numpy()
        assert (gap[moved] <= 4e-6).all()


# ------------------------------------------------------------------------------------------------ the loop

N, D, K = 600, 32, 6


@pytest.fixture(scope="module")
def planted():
    rows, truth = KR.planted(N, D, K, seed=5)
    init_a, init_b = KR.planted_inits(truth, K)
    return rows, truth, {"a": (init_a, KR.kmeans64(rows, K, init_a)), "b": (init_b, KR.kmeans64(rows, K, init_b))}


def _equal_fits(x, y):
    for a, b in zip(x[:3], y[:3]):
        same_bits(a, b)
    assert x.history == y.history and x.iterations == y.iterations and x.reseeded == y.reseeded


@pytest.mark.parametrize("case", ["a", "b"])
def test_kmeans_follows_the_float64_loop(planted, case):
    from mdir_amd import cluster
    rows, truth, fits = planted
    init, want = fits[case]
    rows_t = dev(rows)
    got = cluster.kmeans(rows_t, K, init=init)
    assert isinstance(got, cluster.KMeans) and got.centroids.shape == (K, D) and got.labels.dtype == torch.int64
    np.testing.assert_array_equal(got.labels.cpu().numpy(), want.labels)
    np.testing.assert_array_equal(got.sizes.cpu().numpy(), want.sizes)
    assert got.reseeded == want.reseeded == (0 if case == "a" else 1)
    assert got.iterations == want.iterations and len(got.history) == len(want.history)
    assert KR.pure(got.labels.cpu().numpy(), truth, K)
    np.testing.assert_allclose(got.history, want.history, rtol=1e-5)
    err = np.abs(got.centroids.cpu().numpy().astype(np.float64) - want.centroids)
    tol = KR.centroid_tolerance(want, D)
    print("case %s: %d assignments, worst |centroid - float64| / bound = %.3f" % (case, len(got.history), float((err / tol).max())))
    assert (err <= tol).all()
    # the centroids are exactly the library's own sums of the final partition, finished
    from mdir_amd import ops
    members, offsets = KR.csr(want.labels, K)
    again = KR.sums32(rows, members, offsets, K)
    same_bits(ops.kmeans_finish(dev(again), 1e-6), got.centroids)
    _equal_fits(got, cluster.kmeans(rows_t, K, init=init))                                     # a second run: the same bits everywhere
    _equal_fits(got, cluster.kmeans(rows_t, K, init=init, chunk=77))                           # whatever the chunk
    _equal_fits(got, cluster.kmeans(rows_t, K, init=rows_t[torch.tensor(init, device=DEV)]))   # the same centroids given as a tensor


def test_kmeans_sample_init_and_train_rows(planted):
    from mdir_amd import cluster
    rows, truth, _ = planted
    rows_t = dev(rows)
    one = cluster.kmeans(rows_t, K, seed=3)
    _equal_fits(one, cluster.kmeans(rows_t, K, seed=3))
    # iters=0 returns the initial centroids: the rows the seed drew, in the order drawn
    for seed in (3, 4):
        start = cluster.kmeans(rows_t, K, iters=0, seed=seed)
        ids = torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:K]
        same_bits(start.centroids, rows[ids.numpy()])
        assert start.iterations == 0 and len(start.history) == 1
    assert not torch.equal(torch.randperm(N, generator=torch.Generator().manual_seed(3))[:K],
                           torch.randperm(N, generator=torch.Generator().manual_seed(4))[:K])
    assert int(one.sizes.sum()) == N and one.labels.shape == (N,)
    half = cluster.kmeans(rows_t, K, train_rows=300, seed=1)
    assert half.labels.shape == (N,) and int(half.sizes.sum()) == N
    same_bits(half.sizes, torch.bincount(half.labels, minlength=K))
    _equal_fits(half, cluster.kmeans(rows_t, K, train_rows=300, seed=1))
    labels, _ = cluster.assign(half.centroids, rows_t)                                         # the labels are of ALL rows against the result
    same_bits(labels, half.labels)
    # the training sample is the sorted head of the seed's permutation: from the planted starts (ids of ALL rows) the loop follows
    # the float64 loop on that sample
    init_a, _ = KR.planted_inits(truth, K)
    sample = torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(1))[:300]).values.numpy()
    want = KR.kmeans64(rows, K, init_a, train_ids=sample)
    fit = cluster.kmeans(rows_t, K, init=init_a, train_rows=300, seed=1)
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), want.labels)
    assert fit.reseeded == want.reseeded == 0 and fit.iterations == want.iterations and KR.pure(want.labels, truth, K)


# ------------------------------------------------------------------------------------------------ capture

def test_three_calls_in_one_captured_graph():
    from mdir_amd import ops
    rng = np.random.default_rng(2)
    n, d, k = 700, 36, 5
    host = [(rng.standard_normal((n, k)).astype(F32), _unit(rng, n, d)) for _ in range(2)]
    scores, rows = dev(host[0][0]), dev(host[0][1])
    labels = torch.empty(n, dtype=torch.int64, device=DEV)
    best = torch.empty(n, device=DEV)
    members, offsets = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(k + 1, dtype=torch.int64, device=DEV)

    def csr_of(block):
        m, o = KR.csr(KR.argmax_first(block)[0], k)
        members.copy_(dev(m)), offsets.copy_(dev(o))

    def eager():
        ops.kmeans_argmax(scores, out_labels=labels, out_best=best)
        sums = ops.kmeans_sums(rows, members, offsets, k)
        return sums, ops.kmeans_finish(sums, 1e-6)
    csr_of(host[0][0])
    eager()                                                                                    # eager once, before anything is recorded
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                                                 # one stream, one chain of launches: no parallel branches
            sums_g, cents_g = eager()
    torch.cuda.current_stream().wait_stream(side)
    for block, unit in (host[1], host[0]):                                                     # new data, then the old again
        scores.copy_(dev(block)), rows.copy_(dev(unit))
        csr_of(block)
        labels.fill_(-1), best.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (labels, best, sums_g, cents_g)]
        labels.fill_(-1), best.fill_(-1)
        sums_e, cents_e = eager()
        for a, b in zip(got, (labels, best, sums_e, cents_e)):
            same_bits(a, b)
        same_bits(got[0], KR.argmax_first(block)[0])
        same_bits(got[2], KR.sums32(unit, members.cpu().numpy(), offsets.cpu().numpy(), k))
