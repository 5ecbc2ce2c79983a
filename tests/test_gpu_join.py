"""Exact range search and self-join on the MI355X (include/mdx.h, "exact range search and self-join"; mdir_amd/search.py
range_search / self_join): both routes equal brute force bit for bit -- the fp32 index's mdx_scores, filtered at the threshold and
sorted by the rank key -- on small shapes, on a 20 000-row self-join with duplicate, zero, NaN, infinite and tiny rows, and on a
planted-duplicate set at scale; the bits do not depend on the candidate capacity, the chunk size or the run."""
import numpy as np
import pytest
import torch

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


def desc_key(s):
    """mdx_rank_full's key (oracle/chain.c desc_key), vectorised: smaller key = ranked earlier."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where((u & 0x7FFFFFFF) == 0, np.uint64(0), u)
    u = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(nan, np.uint64(0xFFFFFFFF), ~u & 0xFFFFFFFF)


def csr_from_hits(rows_i, ids, sc, m):
    """The CSR of include/mdx.h from hits (row, id, score) in any order."""
    order = np.lexsort((ids, desc_key(sc), rows_i))
    offsets = np.zeros(m + 1, np.int64)
    np.add.at(offsets, rows_i + 1, 1)
    return np.cumsum(offsets), ids[order].astype(np.int64), np.asarray(sc, np.float32)[order]


def brute(full, tau, upper_from=None):
    """Brute force from a dense [m, n] chain-score matrix: s >= tau (and j > upper_from + i for a self-join block)."""
    m, n = full.shape
    hit = full >= np.float32(tau)
    if upper_from is not None:
        hit &= np.arange(n)[None, :] > (upper_from + np.arange(m))[:, None]
    i, j = np.nonzero(hit)
    return csr_from_hits(i, j, full[i, j], m)


def assert_same(got, want):
    off, ids, sc = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1])
    np.testing.assert_array_equal(bits(sc), bits(want[2]))


def fp32_scores(rows, x):
    from mdir_amd import ops
    return ops.DescriptorIndex(dev(rows), "ND").scores(dev(x), "ND").cpu().numpy()


def taus(full, rng):
    """Thresholds at several quantiles and at scores that occur (ties at tau count)."""
    flat = full[np.isfinite(full)].ravel()
    out = [float(np.quantile(flat, q)) for q in (0.5, 0.9, 0.999)]
    out += [float(flat[rng.integers(0, flat.size)]), float(flat.max())]
    return out


# ------------------------------------------------------------------ range search, both routes, small shapes

@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 4993])
@pytest.mark.parametrize("d", [1, 63, 64, 100, 2048])
def test_range_search_equals_brute_force(n, d):
    from mdir_amd import ops
    from mdir_amd.search import range_search
    rng = np.random.default_rng(n * 131 + d)
    rows = unit_rows(rng, n, d)
    if n > 17:
        rows[5] = rows[9]                                    # duplicate rows: equal scores by ascending id
        rows[7] = 0                                          # a zero row
    ix = ops.DescriptorIndex(dev(rows), "ND", storage="i8")
    for nq in (1, 70, 300):
        q = unit_rows(rng, nq, d)
        if n > 17:
            q[0] = rows[3]                                   # a query equal to a row
        full = fp32_scores(rows, q)
        for tau in taus(full, rng):
            want = brute(full, tau)
            assert_same(range_search(ix, dev(rows), dev(q), tau), want)
            assert_same(range_search(None, dev(rows), dev(q), tau), want)


@pytest.mark.parametrize("d", [63, 2048])
def test_range_search_with_a_center_and_dim_major_queries(d):
    from mdir_amd import ops
    from mdir_amd.search import range_search
    rng = np.random.default_rng(d)
    n, nq = 3000, 70
    rows = unit_rows(rng, n, d)
    q = unit_rows(rng, nq, d)
    c = (0.01 * rng.standard_normal(d)).astype(np.float32)
    x = (q - c[None, :]).astype(np.float32)                  # one fp32 subtraction, as the library
    full = fp32_scores(rows, x)
    ix = ops.DescriptorIndex(dev(rows), "ND", storage="i8")
    for tau in taus(full, rng):
        want = brute(full, tau)
        assert_same(range_search(ix, dev(rows), dev(q.T), tau, qlayout="DN", center=dev(c)), want)
        assert_same(range_search(None, dev(rows), dev(q), tau, center=dev(c)), want)


# ------------------------------------------------------------------ self-join with awkward rows

def awkward_rows(rng, n, d):
    x = unit_rows(rng, n, d)
    x[100:110] = x[50]                                       # a group of duplicates
    x[200] = 0                                               # zero rows
    x[201] = 0
    x[300, 7] = np.nan                                       # a NaN row: every score NaN, never a hit
    x[400, 3] = np.inf                                       # an infinite element
    x[500] = x[60] * np.float32(2.0 ** -100)                 # tiny-scale rows (outside the int8 contract)
    x[501] = x[60] * np.float32(2.0 ** -70)
    x[600] = x[61] * np.float32(2.0 ** 30)                   # a large row
    for k in range(0, 2000, 10):                             # near duplicates a hair apart
        x[n - 1 - k] = x[k] + np.float32(1e-3) * rng.standard_normal(d, dtype=np.float32)
    return x


def brute_self(rows, tau, block=2500):
    n = rows.shape[0]
    parts_i, parts_j, parts_s = [], [], []
    from mdir_amd import ops
    fix = ops.DescriptorIndex(dev(rows), "ND")
    sym_checked = False
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        full = fix.scores(dev(rows[lo:hi]), "ND").cpu().numpy()
        if not sym_checked and hi < n:                       # chain(i, j) == chain(j, i) bitwise on sampled pairs
            rng = np.random.default_rng(lo)
            i = rng.integers(lo, hi, 2000)
            j = rng.integers(hi, n, 2000)
            other = fix.scores(dev(rows[j]), "ND").cpu().numpy()
            np.testing.assert_array_equal(bits(full[i - lo, j]), bits(other[np.arange(2000), i]))
            sym_checked = True
        hit = (full >= np.float32(tau)) & (np.arange(n)[None, :] > np.arange(lo, hi)[:, None])
        i, j = np.nonzero(hit)
        parts_i.append(i + lo)
        parts_j.append(j)
        parts_s.append(full[i, j])
    return csr_from_hits(np.concatenate(parts_i), np.concatenate(parts_j), np.concatenate(parts_s), n)


def test_self_join_equals_the_upper_triangle():
    from mdir_amd import ops
    from mdir_amd.search import self_join
    rng = np.random.default_rng(5)
    n, d = 20000, 2048
    rows = awkward_rows(rng, n, d)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    for tau in (0.99, 0.9, 0.1, 0.05):
        want = brute_self(rows, tau)
        got = self_join(ix, r, tau)
        assert_same(got, want)
        if tau in (0.9, 0.05):
            assert_same(self_join(None, r, tau), want)
    # chunking, capacity and repetition change no bit
    base = self_join(ix, r, 0.9)
    assert_same(self_join(ix, r, 0.9, chunk=128), [t.cpu().numpy() for t in base])
    assert_same(self_join(ix, r, 0.9, chunk=3000), [t.cpu().numpy() for t in base])
    assert_same(self_join(None, r, 0.9, chunk=777), [t.cpu().numpy() for t in base])
    assert_same(self_join(ix, r, 0.9), [t.cpu().numpy() for t in base])
    with pytest.raises(ValueError, match="max_pairs"):
        self_join(ix, r, 0.9, max_pairs=max(1, base.ids.numel() - 1))


def test_small_candidate_capacity_gives_the_same_bits():
    from mdir_amd import ops
    rng = np.random.default_rng(9)
    n, d = 3000, 100
    rows = awkward_rows(rng, n, d)
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    st = ops.join_stats(ix, r)
    big, count = ops.join_candidates(ix, st, ix, st, 0.8, 0, n, True, 1 << 22)
    small, count2 = ops.join_candidates(ix, st, ix, st, 0.8, 0, n, True, 3)
    assert count == count2 and count > 3 and small.numel() == 3
    assert set(big.cpu().numpy().tolist()) >= set(small.cpu().numpy().tolist())
    again, _ = ops.join_candidates(ix, st, ix, st, 0.8, 0, n, True, count)
    np.testing.assert_array_equal(np.sort(again.cpu().numpy()), np.sort(big.cpu().numpy()))
    a = ops.join_resolve(r, r, big, 0.8, 0, n)
    assert_same(ops.join_resolve(r, r, again, 0.8, 0, n), [t.cpu().numpy() for t in a])
    assert_same(a, brute_self(rows, 0.8, block=3000))


# ------------------------------------------------------------------ at scale: planted near-duplicate groups

def planted(rng, n, d, groups=2000):
    x = unit_rows(rng, n, d)
    members = rng.choice(n, size=(groups, 4), replace=False)
    sigma = rng.uniform(0.05, 1.3, groups).astype(np.float32)   # pair cosines ~ 1 / (1 + sigma^2): spread around 0.9 and 0.5
    for g in range(groups):
        base = x[members[g, 0]]
        for k in members[g, 1:]:
            v = base + sigma[g] * unit_rows(rng, 1, d)[0]
            x[k] = v / np.linalg.norm(v)
    return x


def test_self_join_at_scale_equals_the_exact_route():
    from mdir_amd import ops
    from mdir_amd.search import self_join
    rng = np.random.default_rng(12)
    n, d = 200000, 2048
    r = dev(planted(rng, n, d))
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    for tau in (0.9, 0.5):
        got = self_join(ix, r, tau)
        want = self_join(None, r, tau)
        assert got.ids.numel() > 1000
        assert_same(got, [t.cpu().numpy() for t in want])


# ------------------------------------------------------------------ rows whose int8 scale rounds to 0, refusals

@pytest.mark.parametrize("d", [1, 64, 100])
def test_subnormal_rows_reach_the_exact_stage(d):
    """A nonzero row whose max|x| is a subnormal so small that its int8 scale rounds to 0 has int8 scores 0; against a large row
    its exact scores are normal numbers.  Both routes must report those pairs at a tiny positive threshold."""
    from mdir_amd import ops
    from mdir_amd.search import range_search, self_join
    rng = np.random.default_rng(d + 1)
    n = 300
    rows = unit_rows(rng, n, d)
    rows[10] = 0
    rows[10, 0] = np.float32(2.0 ** -145)                    # scale = 2^-145 / 127 rounds to 0
    rows[11] = 0
    rows[11, :] = np.float32(2.0 ** -146)
    rows[20] = rows[20] * np.float32(2.0 ** 38)              # large rows: products with the subnormal ones are normal
    rows[21] = np.abs(rows[21]) * np.float32(2.0 ** 39)
    rows[30] = 0                                             # a zero row: scores exactly 0, pruned
    cx = quantize_scale(rows)
    assert cx[10] == 0 and cx[11] == 0
    r = dev(rows)
    ix = ops.DescriptorIndex(r, "ND", storage="i8")
    full = fp32_scores(rows, rows)
    tiny = full[(full > 0) & (full < 2.0 ** -80)]
    assert tiny.size > 0
    for tau in (float(tiny.min()), float(np.median(tiny)), 2.0 ** -120):
        want = brute(full, tau, upper_from=0)
        assert want[1].size > 0
        assert_same(self_join(ix, r, tau), want)
        assert_same(self_join(None, r, tau), want)
        q = rows[[10, 11, 20, 0]]
        wq = brute(fp32_scores(rows, q), tau)
        assert_same(range_search(ix, r, dev(q), tau), wq)
        assert_same(range_search(None, r, dev(q), tau), wq)


def quantize_scale(rows):
    from mdir_amd import ops
    return ops.quantize_i8(dev(rows), "ND")[1].cpu().numpy()


def test_entry_points_refuse_a_non_int8_index():
    import ctypes
    from mdir_amd import _lib, ops
    rng = np.random.default_rng(2)
    rows = dev(unit_rows(rng, 200, 64))
    i8 = ops.DescriptorIndex(rows, "ND", storage="i8")
    st = ops.join_stats(i8, rows)
    h = _lib.lib()
    p = ctypes.c_void_p(st.data_ptr())
    pairs = torch.empty(16, dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    pp, cp = ctypes.c_void_p(pairs.data_ptr()), ctypes.c_void_p(count.data_ptr())
    f32 = ctypes.c_float
    for storage in ("f32", "f16"):
        other = ops.DescriptorIndex(rows, "ND", storage=storage)
        assert h.mdx_join_stats(other._h, ctypes.c_void_p(rows.data_ptr()), 64, p, None) == -1
        assert b"int8" in h.mdx_last_error()
        for a, b in ((other._h, i8._h), (i8._h, other._h)):
            assert h.mdx_join_candidates(a, p, b, p, 0, 200, 0, f32(0.5), pp, 16, cp, None) == -1
            assert b"int8" in h.mdx_last_error()
        with pytest.raises(ValueError, match="int8"):
            ops.join_stats(other, rows)
        with pytest.raises(ValueError, match="int8"):
            ops.join_candidates(other, st, i8, st, 0.5)
        other.close()
    for bad in (float("nan"), float("inf")):
        assert h.mdx_join_candidates(i8._h, p, i8._h, p, 0, 200, 1, f32(bad), pp, 16, cp, None) == -1
    assert h.mdx_join_candidates(i8._h, p, i8._h, p, 0, 200, 1, f32(0.5), pp, -1, cp, None) == -1
    assert h.mdx_join_candidates(i8._h, p, i8._h, p, 64, 200, 1, f32(0.5), pp, 16, cp, None) == -1       # lo not a block start
    assert h.mdx_join_candidates(i8._h, p, i8._h, p, 0, 201, 1, f32(0.5), pp, 16, cp, None) == -1       # hi beyond n
    assert h.mdx_join_candidates(i8._h, p, i8._h, p, 0, 200, 1, f32(0.5), pp, 16, cp, None) == 0
    torch.cuda.synchronize()
