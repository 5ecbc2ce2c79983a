"""The exact kNN join on the MI355X (include/mdx.h, "exact kNN join"; mdir_amd/search.py knn_join): the neighbour lists built on
the int8 shard -- bounds -> candidates -> resolve -- equal ``ops.topk`` of the fp32 chain scores of the same rows bit for bit (ids
and score bits), whatever the slices, the chunk and the candidate capacity; across ties at the k-th place; for NaN, infinite,
zero, tiny and huge rows; and the bound really prunes planted rows.  DBA and the diffusion graph built through an int8 index
are bit-equal to those built without."""
import ctypes

import numpy as np
import pytest
import torch

from test_knn_join_host import planted_groups, thresholds_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30).astype(np.float32)
    return x


def fp32_scores(rows, x):
    from mdir_amd import ops
    return ops.DescriptorIndex(dev(rows), "ND").scores(dev(x), "ND")


def expected(rows, k, block=8192):
    """ops.topk of the fp32 chain scores of the rows against themselves: (ids, scores) on the host."""
    from mdir_amd import ops
    fix = ops.DescriptorIndex(dev(rows), "ND")
    ids, sc = [], []
    for lo in range(0, rows.shape[0], block):
        i, s = ops.topk(fix.scores(dev(rows[lo:lo + block]), "ND"), k)
        ids.append(i.cpu().numpy())
        sc.append(s.cpu().numpy())
    fix.close()
    return np.concatenate(ids), np.concatenate(sc)


def assert_same(got_ids, got_scores, want):
    np.testing.assert_array_equal(got_ids.cpu().numpy(), want[0])
    np.testing.assert_array_equal(bits(got_scores.cpu().numpy()), bits(want[1]))


def stages(ix, r, k, slices=0, capacity=1 << 20, lo=0, hi=None):
    """bounds -> candidates -> resolve on rows [lo, hi), with no fallback: (ids, scores, counts, t, candidates)."""
    from mdir_amd import ops
    hi = r.shape[0] if hi is None else hi
    st = ops.join_stats(ix, r)
    t = ops.knn_bounds(ix, st, ix, st, lo, hi, k, slices)
    pairs, count = ops.join_candidates_rows(ix, st, ix, st, t, lo, hi, capacity)
    if count > capacity:
        assert pairs.numel() == capacity
        pairs, again = ops.join_candidates_rows(ix, st, ix, st, t, lo, hi, count)
        assert again == count == pairs.numel()
    ids, sc, counts = ops.knn_resolve(r, r, pairs, lo, hi - lo, k)
    return ids, sc, counts, t, count


# ------------------------------------------------------------------ shapes and k

@pytest.mark.parametrize("n", [1, 16, 127, 128, 129, 300, 1000])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 200])
def test_knn_join_equals_topk_of_the_chain(n, d):
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(n * 131 + d)
    rows = planted_groups(rng, n, d, 8, 0.5)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    top = min(n, ops.KNN_JOIN_MAX_K)
    want_all = expected(rows, top)
    for k in sorted({1, min(7, n), top}):                      # top == n where n <= MAX_K
        want = (want_all[0][:, :k], want_all[1][:, :k])
        ids, sc, counts, t, count = stages(ix, r, k)
        assert_same(ids, sc, want)
        assert (counts.cpu().numpy() >= k).all()
        kth = want[1][:, k - 1]
        assert (t.cpu().numpy() <= kth).all()                  # a lower bound of the exact k-th score
        res = knn_join(ix, r, k)
        assert_same(res.ids, res.scores, want)
        assert res.pruned_rows == (n if count <= n * n // 8 else 0)     # one chunk: the N / 8 rule decides its route
        none = knn_join(None, r, k)
        assert_same(none.ids, none.scores, want)
        assert none.pruned_rows == 0
    big = knn_join(None, r, n + 5)                             # k is clamped to N
    assert tuple(big.ids.shape) == (n, n)
    ix.close()


# ------------------------------------------------------------------ forced slices

def test_every_slicing_gives_the_same_thresholds():
    from mdir_amd import ops
    rng = np.random.default_rng(77)
    n, d, k = 1000, 64, 10
    rows = planted_groups(rng, n, d, 8, 0.5)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    st = ops.join_stats(ix, r)
    want = expected(rows, k)
    base = ops.knn_bounds(ix, st, ix, st, 0, n, k, 0).cpu().numpy()
    assert np.isfinite(base).all() and (base <= want[1][:, k - 1]).all()
    for slices in (1, 2, 3, 7, 64):
        t = ops.knn_bounds(ix, st, ix, st, 0, n, k, slices)
        np.testing.assert_array_equal(bits(t.cpu().numpy()), bits(base), err_msg="slices=%d" % slices)
        ids, sc, counts, _, _ = stages(ix, r, k, slices)
        assert (counts.cpu().numpy() >= k).all()
        assert_same(ids, sc, want)
    part = ops.knn_bounds(ix, st, ix, st, 384, 900, k, 2).cpu().numpy()        # a row range gives the rows' own values
    np.testing.assert_array_equal(bits(part), bits(base[384:900]))
    ix.close()


# ------------------------------------------------------------------ chunk and capacity invariance

def test_chunk_and_capacity_change_no_bit():
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(31)
    n, d, k = 1000, 100, 7
    rows = planted_groups(rng, n, d, 8, 0.5)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    want = expected(rows, k)
    for chunk in (128, 384, None):
        for capacity in (64, None):
            res = knn_join(ix, r, k, chunk=chunk, capacity=capacity)
            assert_same(res.ids, res.scores, want)
            assert res.pruned_rows == n
    ids, sc, _, _, count = stages(ix, r, k, capacity=64)
    assert count > 64
    assert_same(ids, sc, want)
    res = knn_join(None, r, k, chunk=77)
    assert_same(res.ids, res.scores, want)
    ix.close()


# ------------------------------------------------------------------ ties across the k-th place

@pytest.mark.parametrize("k", [10, 39])
def test_exact_copies_across_the_kth_place(k):
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(k)
    n, d = 500, 64
    rows = unit_rows(rng, n, d)
    copies = rng.choice(n, 40, replace=False)
    rows[copies] = rows[copies[0]]
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    want = expected(rows, k)
    assert len(set(want[1][copies[0]].view(np.uint32).tolist())) == 1            # the copies tie: the list is the k smallest ids
    np.testing.assert_array_equal(want[0][copies[0]], np.sort(copies)[:k])
    ids, sc, counts, _, _ = stages(ix, r, k)
    assert_same(ids, sc, want)
    assert (counts.cpu().numpy()[copies] >= 40).all()                            # every tie is a candidate
    res = knn_join(ix, r, k)
    assert_same(res.ids, res.scores, want)
    ix.close()


def test_all_equal_and_signed_zero_rows():
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(8)
    same = np.repeat(unit_rows(rng, 1, 100), 300, axis=0)
    zeros = unit_rows(rng, 300, 64)
    zeros[10:40] = 0.0
    zeros[40:70] = -0.0
    zeros[100] = 0.0
    only = np.zeros((200, 7), np.float32)
    only[::2] = -0.0
    for rows in (same, zeros, only):
        r = dev(rows)
        ix = ops.DescriptorIndex(r, "ND", storage="i8")
        for k in (1, 10, 64):
            want = expected(rows, k)
            ids, sc, counts, _, _ = stages(ix, r, k)
            assert_same(ids, sc, want)
            assert (counts.cpu().numpy() >= k).all()
            res = knn_join(ix, r, k)
            assert_same(res.ids, res.scores, want)
        ix.close()


# ------------------------------------------------------------------ awkward rows

def awkward_rows(rng, n, d):
    x = unit_rows(rng, n, d)
    x[100:110] = x[50]                                       # a group of duplicates
    x[200] = 0                                               # zero rows
    x[201] = 0
    x[300, 7] = np.nan                                       # a NaN row: every score NaN, ranked last
    x[400, 3] = np.inf                                       # an infinite element
    x[500] = x[60] * np.float32(2.0 ** -100)                 # tiny-scale rows (outside the int8 contract)
    x[501] = x[60] * np.float32(2.0 ** -70)
    x[600] = x[61] * np.float32(2.0 ** 30)                   # a large row
    for k in range(0, 2000, 10):                             # near duplicates a hair apart
        x[n - 1 - k] = x[k] + np.float32(1e-3) * rng.standard_normal(d, dtype=np.float32)
    return x


@pytest.mark.parametrize("d", [100, 256])
def test_awkward_rows_stay_exact(d):
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(9 + d)
    n, k = 3000, 10
    rows = awkward_rows(rng, n, d)
    rows[700] = 0
    rows[700, 0] = np.float32(2.0 ** -145)                   # a subnormal row whose int8 scale rounds to 0
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    want = expected(rows, k)
    assert np.isnan(want[1][300]).all()
    ids, sc, counts, t, _ = stages(ix, r, k)
    assert_same(ids, sc, want)
    t, counts = t.cpu().numpy(), counts.cpu().numpy()
    for row in (300, 400, 500, 700):                         # no pair of an uncovered row has a lower bound: t = -inf, every row a candidate
        assert t[row] == -np.inf and counts[row] == n, row
    assert np.isfinite(t[[0, 50, 200, 501, 600]]).all()
    assert (counts >= k).all() and counts[0] < n
    for chunk in (None, 1024):
        res = knn_join(ix, r, k, chunk=chunk)
        assert_same(res.ids, res.scores, want)
        assert res.pruned_rows == n
    ix.close()


# ------------------------------------------------------------------ pruning really happens

def test_the_bound_prunes_planted_rows():
    """Groups of 16 rows at noise 0.5, n = 4096, d = 256, k = 10: the float64 restatement of the bound keeps 16.0 candidates per
    row (the group), 1.6 k n in all; the device may keep a few more (its fp32 bound is rounded outwards), never above 4 k n."""
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(4096)
    n, d, k = 4096, 256, 10
    rows = planted_groups(rng, n, d, 16, 0.5)
    t64, _, cand = thresholds_np(rows, rows, k)
    print("float64 restatement: %.2f candidates per row" % (cand.sum() / n))
    assert cand.sum() <= 4 * k * n and abs(cand.sum() / n - 16.0) < 0.5
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    want = expected(rows, k)
    ids, sc, counts, t, count = stages(ix, r, k)
    print("device: %.2f candidates per row" % (count / n))
    assert_same(ids, sc, want)
    assert k * n <= count <= 4 * k * n
    assert int(counts.sum().item()) == count
    t = t.cpu().numpy()
    # the device rounds every l downwards in fp32 (a few 2^-24 of values below 1, and 2^-20 of b); 1e-12 covers the float64 restatement's own rounding
    assert np.isfinite(t).all() and (t <= t64 + 1e-12).all() and (t64 - t <= 1e-5).all()
    res = knn_join(ix, r, k)
    assert_same(res.ids, res.scores, want)
    assert res.pruned_rows == n
    ix.close()


# ------------------------------------------------------------------ the exact-route fallback

def test_structureless_rows_fall_back_and_stay_exact():
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(2048)
    n, d, k = 2048, 2048, 10
    rows = unit_rows(rng, n, d)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    st = ops.join_stats(ix, r)
    want = expected(rows, k)
    for chunk in (None, 512):
        step = n if chunk is None else chunk
        stay = 0
        for lo in range(0, n, step):                         # the rule of knn_join, chunk by chunk
            hi = min(n, lo + step)
            t = ops.knn_bounds(ix, st, ix, st, lo, hi, k)
            _, count = ops.join_candidates_rows(ix, st, ix, st, t, lo, hi, 0)
            assert count >= (hi - lo) * k
            stay += hi - lo if count <= (hi - lo) * n // 8 else 0
        res = knn_join(ix, r, k, chunk=chunk)
        print("chunk %s: %d of %d rows stayed on the int8 route" % (chunk, res.pruned_rows, n))
        assert_same(res.ids, res.scores, want)
        assert res.pruned_rows == stay
    ids, sc, _, _, _ = stages(ix, r, k)                      # the int8 route is exact here as well, it only prunes little
    assert_same(ids, sc, want)
    ix.close()


# ------------------------------------------------------------------ consumers

def test_dba_and_the_diffusion_graph_through_an_int8_index():
    from mdir_amd import ops, rerank
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(3000)
    n, d = 3000, 128
    rows = planted_groups(rng, n, d, 16, 0.5)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    # knn_join(None, ...) is the neighbour-list loop DBA ran: scores_rowmajor + topk on chunks of rows
    lists = knn_join(None, r, 10, chunk=700)
    want = expected(rows, 10)
    assert_same(lists.ids, lists.scores, want)
    i2, s2 = ops.topk(ops.scores_rowmajor(r, r[:64], "ND"), 10)
    assert_same(lists.ids[:64], lists.scores[:64], (i2.cpu().numpy(), s2.cpu().numpy()))
    plain = rerank.database_augmentation(r, 10, 3.0)
    np.testing.assert_array_equal(bits(plain.cpu().numpy()), bits(ops.knn_aggregate(r, dev(want[0]), dev(want[1]), 3.0).cpu().numpy()))
    via = rerank.database_augmentation(r, 10, 3.0, index=ix)
    np.testing.assert_array_equal(bits(via.cpu().numpy()), bits(plain.cpu().numpy()))
    for weights in (False, True):
        a = rerank.DiffusionGraph(r, k=10, weights=weights)
        b = rerank.DiffusionGraph(r, k=10, weights=weights, index=ix)
        assert a.edges() == b.edges() > 0
        np.testing.assert_array_equal(a.cols.cpu().numpy(), b.cols.cpu().numpy())
        np.testing.assert_array_equal(a.counts.cpu().numpy(), b.counts.cpu().numpy())
        np.testing.assert_array_equal(bits(a.vals.cpu().numpy()), bits(b.vals.cpu().numpy()))
        assert (a.wvals is None) == (b.wvals is None) == (not weights)
        if weights:
            np.testing.assert_array_equal(bits(a.wvals.cpu().numpy()), bits(b.wvals.cpu().numpy()))
    ix.close()


# ------------------------------------------------------------------ at scale

def test_knn_join_at_scale_equals_the_exact_route():
    from mdir_amd import ops
    from mdir_amd.search import knn_join
    rng = np.random.default_rng(100000)
    n, d, k = 100000, 256, 20
    r = dev(planted_groups(rng, n, d, 32, 0.5))
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    got = knn_join(ix, r, k)
    want = knn_join(None, r, k)
    assert got.pruned_rows == n and want.pruned_rows == 0
    np.testing.assert_array_equal(got.ids.cpu().numpy(), want.ids.cpu().numpy())
    np.testing.assert_array_equal(bits(got.scores.cpu().numpy()), bits(want.scores.cpu().numpy()))
    ix.close()


# ------------------------------------------------------------------ refusals

def test_entry_points_refuse_bad_operands():
    from mdir_amd import _lib, ops
    rng = np.random.default_rng(2)
    rows = dev(unit_rows(rng, 200, 64))
    i8 = ops.DescriptorIndex(rows, "ND", storage="i8")
    narrow = ops.DescriptorIndex(dev(unit_rows(rng, 200, 32)), "ND", storage="i8")
    st = ops.join_stats(i8, rows)
    h = _lib.lib()
    p = ctypes.c_void_p(st.data_ptr())
    t = torch.zeros(200, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    pairs = torch.empty(16, dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    tp, wp, pp, cp = (ctypes.c_void_p(x.data_ptr()) for x in (t, ws, pairs, count))

    def bounds(a=i8._h, b=i8._h, lo=0, hi=200, k=5, slices=0, wsb=1 << 20):
        return h.mdx_knn_bounds(a, p, b, p, lo, hi, k, slices, tp, wp, wsb, None)

    def cand(a=i8._h, b=i8._h, lo=0, hi=200, cap=16):
        return h.mdx_join_candidates_rows(a, p, b, p, lo, hi, tp, pp, cap, cp, None)
    for storage in ("f32", "f16"):
        other = ops.DescriptorIndex(rows, "ND", storage=storage)
        for kw in ({"a": other._h}, {"b": other._h}):
            assert bounds(**kw) == -1 and b"int8" in h.mdx_last_error()
            assert cand(**kw) == -1 and b"int8" in h.mdx_last_error()
        with pytest.raises(ValueError, match="int8"):
            ops.knn_bounds(other, st, i8, st, 0, 200, 5)
        with pytest.raises(ValueError, match="int8"):
            ops.join_candidates_rows(i8, st, other, st, t)
        other.close()
    assert bounds(b=narrow._h) == -1 and b"differ" in h.mdx_last_error()
    assert cand(b=narrow._h) == -1 and b"differ" in h.mdx_last_error()
    tiny = ops.DescriptorIndex(rows[:5], "ND", storage="i8")
    st5 = ops.join_stats(tiny, rows[:5])
    p5 = ctypes.c_void_p(st5.data_ptr())
    assert h.mdx_knn_bounds(tiny._h, p5, tiny._h, p5, 0, 5, 6, 0, tp, wp, 1 << 20, None) == -1 and b"rows of B" in h.mdx_last_error()
    assert h.mdx_knn_bounds(tiny._h, p5, tiny._h, p5, 0, 5, 5, 0, tp, wp, 1 << 20, None) == 0
    for kw in ({"lo": 64}, {"hi": 201}, {"lo": 128, "hi": 128}):
        assert bounds(**kw) == -1 and b"multiple of 128" in h.mdx_last_error()
        assert cand(**kw) == -1 and b"multiple of 128" in h.mdx_last_error()
    assert bounds(wsb=16) == -4 and b"workspace" in h.mdx_last_error()
    assert bounds() == 0 and cand() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="slices"):
        ops.knn_bounds(i8, st, i8, st, 0, 200, 5, slices=65)
    with pytest.raises(ValueError, match="KNN_JOIN_MAX_K"):
        ops.knn_bounds(i8, st, i8, st, 0, 200, 65)
    with pytest.raises(ValueError, match="k=6 > the 5 rows"):
        ops.knn_bounds(tiny, st5, tiny, st5, 0, 5, 6)
    with pytest.raises(ValueError, match="taus"):
        ops.join_candidates_rows(i8, st, i8, st, t[:100])
    for ix in (i8, narrow, tiny):
        ix.close()
